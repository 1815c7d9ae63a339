#pragma once
// crop_aug.h: crop training on the device (cvk_crop_select, cvk_crop_augment_u8).  A sample is rescaled to a VIRTUAL Hr x Wr image
// (cv2 INTER_LINEAR / INTER_NEAREST with the record's own double steps; it never reaches memory), an hc x wc window is cut out of
// it at a signed offset and whatever the window shows outside the resized image is pad.  cvk_crop_select chooses the window among
// the record's candidates by mmseg's cat_max_ratio rule from integer class counts and leaves the choice in a device table;
// cvk_crop_augment_u8 reads that table and writes the blurred, LUT-mapped, flipped and normalised crop.  The three small helpers
// of the resampling (aug_reflect101, aug_round_u8, aug_coord) live here, once, for k_augment_u8 as well.
#include "cvk_common.h"

namespace {

static_assert(sizeof(cvk_crop_record) == 416, "cvk_crop_record has implicit padding");

__device__ __forceinline__ int aug_reflect101(int x, int n) {
    if ((unsigned)x < (unsigned)n) return x;
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    x %= p;
    if (x < 0) x += p;
    return x < n ? x : p - x;
}

__device__ __forceinline__ float aug_round_u8(float v) { return fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f); }

// cv2 INTER_LINEAR source coordinate: f = (d + 0.5) * scale - 0.5, i = floor(f), weight f - i; clamped at both edges
__device__ __forceinline__ void aug_coord(int d, double scale, int n, int& i0, int& i1, float& a) {
    const double f = (d + 0.5) * scale - 0.5;
    int i = (int)floor(f);
    a = (float)(f - i);
    if (i < 0) { i = 0; a = 0.f; }
    if (i >= n - 1) { i = n - 1; a = 0.f; }
    i0 = i;
    i1 = i + 1 < n ? i + 1 : n - 1;
}

constexpr int CROP_MAX_CAND = 11, CROP_BINS = 256;
constexpr int CROP_CW = 64, CROP_CH = 32;             // window tile of one counting workgroup
constexpr int CROP_TW = 64, CROP_TH = 16, CROP_RMAX = 4;
constexpr int CROP_LW = CROP_TW + 2 * CROP_RMAX, CROP_LH = CROP_TH + 2 * CROP_RMAX;

// cv2 INTER_NEAREST source index of resized index d: min(floor(d * step), n - 1) in double (never below 0 either: the step is data)
__device__ __forceinline__ int crop_nearest(int d, double step, int n) { return max(min((int)floor(d * step), n - 1), 0); }

__device__ __forceinline__ int crop_ncand(const cvk_crop_record* rec) { return min(max(rec->ncand, 1), CROP_MAX_CAND); }

__global__ __launch_bounds__(256) void k_crop_clear(unsigned int* __restrict__ counts, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) counts[i] = 0u;
}

// ---- class counts of every candidate window (cvk_crop_select, first launch) ------------------------------------------------------
// Grid (tiles of the window, candidate, sample).  A workgroup cuts its CROP_CW x CROP_CH part of the candidate's window to the
// resized image; a lane owns a column (one source column index), a wave every fourth row (one source row index per row).  A wave
// first gathers the nearest-resampled labels of all its CROP_CH / 4 rows (the loads are independent: one latency, not eight), then
// counts them row by row into its own 256-bin LDS histogram.  Masks are made of runs of one class, and 64 LDS adds to one bin
// serialise, so for up to CROP_GROUP_ROUNDS labels per row the wave groups its lanes (ballot of the lanes that hold the first pending
// lane's label) and that lane adds the group's size; lanes still pending after that (noisy rows) add 1 each.  The workgroup then
// adds its non-zero bins to counts[n][candidate][256].  Integer atomics only: the table is exact whatever the order.
constexpr int CROP_GROUP_ROUNDS = 2;

__global__ __launch_bounds__(256) void k_crop_count(const void* __restrict__ masks, int mask_bytes, int Hs, int Ws, int hc, int wc,
                                                   int tiles_x, const cvk_crop_record* __restrict__ records, int ignore_index,
                                                   unsigned int* __restrict__ counts) {
    __shared__ unsigned int h[4 * CROP_BINS];
    const int n = blockIdx.z, cand = blockIdx.y;
    const cvk_crop_record* rec = records + n;
    if (cand >= crop_ncand(rec)) return;
    const int Hr = rec->Hr, Wr = rec->Wr, offy = rec->offy[cand], offx = rec->offx[cand];
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    // the tile in window coordinates, cut to (window ∩ resized image)
    const int y0 = max(ty * CROP_CH, -offy), y1 = min(min((ty + 1) * CROP_CH, hc), Hr - offy);
    const int x0 = max(tx * CROP_CW, -offx), x1 = min(min((tx + 1) * CROP_CW, wc), Wr - offx);
    if (y0 >= y1 || x0 >= x1) return;
    for (int i = threadIdx.x; i < 4 * CROP_BINS; i += 256) h[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned int* mine = h + wave * CROP_BINS;
    const double sy = rec->sy, sx = rec->sx;
    const int x = x0 + lane;                                        // x1 - x0 <= CROP_CW = 64: one column per lane
    const bool live = x < x1;
    const int mx = crop_nearest(x + offx, sx, Ws);                  // clamped into the row whatever x is
    const size_t base = (size_t)n * Hs * Ws;
    int lab[CROP_CH / 4];                                           // -1: nothing to count
#pragma unroll
    for (int k = 0; k < CROP_CH / 4; ++k) {
        const int y = y0 + wave + 4 * k;                            // uniform per wave
        lab[k] = -1;
        if (live && y < y1) {
            const size_t mi = base + (size_t)crop_nearest(y + offy, sy, Hs) * Ws + mx;
            const long v = mask_bytes == 1 ? (long)static_cast<const uint8_t*>(masks)[mi] : (long)static_cast<const int64_t*>(masks)[mi];
            if (v != (long)ignore_index && v >= 0 && v < CROP_BINS) lab[k] = (int)v;
        }
    }
#pragma unroll
    for (int k = 0; k < CROP_CH / 4; ++k) {
        const int l = lab[k];
        unsigned long long todo = __ballot(l >= 0);
        for (int round = 0; round < CROP_GROUP_ROUNDS && todo; ++round) {
            const int first = __ffsll((long long)todo) - 1;
            const int lv = __shfl(l, first);
            const unsigned long long same = __ballot(l == lv);
            if (lane == first) atomicAdd(&mine[lv], (unsigned int)__popcll(same));
            todo &= ~same;
        }
        if ((todo >> lane) & 1ull) atomicAdd(&mine[l], 1u);
    }
    __syncthreads();
    const int c = threadIdx.x;      // 256 threads, 256 bins
    const unsigned int v = h[c] + h[CROP_BINS + c] + h[2 * CROP_BINS + c] + h[3 * CROP_BINS + c];
    if (v) atomicAdd(&counts[((size_t)n * CROP_MAX_CAND + cand) * CROP_BINS + c], v);
}

// ---- the selection rule (cvk_crop_select, second launch) -------------------------------------------------------------------------
// One workgroup per sample, thread c owns bin c.  Candidates 0 .. ncand - 2 are tested in order: a candidate passes iff more than
// one label value occurs and (double)max / (double)sum < cat_max_ratio; the first that passes is taken, else candidate ncand - 1.
// selection[n] = {candidate, offy, offx, passed}.
__global__ __launch_bounds__(256) void k_crop_select(const unsigned int* __restrict__ counts, const cvk_crop_record* __restrict__ records,
                                                    double cat_max_ratio, int* __restrict__ selection) {
    __shared__ unsigned int s_distinct, s_max, s_sum;
    __shared__ int s_chosen;
    const int n = blockIdx.x;
    const cvk_crop_record* rec = records + n;
    const int ncand = crop_ncand(rec);
    if (threadIdx.x == 0) s_chosen = -1;
    for (int cand = 0; cand < ncand - 1; ++cand) {
        if (threadIdx.x == 0) { s_distinct = 0u; s_max = 0u; s_sum = 0u; }
        __syncthreads();
        if (s_chosen >= 0) break;       // uniform: written before the barrier above
        const unsigned int v = counts[((size_t)n * CROP_MAX_CAND + cand) * CROP_BINS + threadIdx.x];
        if (v) {
            atomicAdd(&s_distinct, 1u);
            atomicMax(&s_max, v);
            atomicAdd(&s_sum, v);
        }
        __syncthreads();
        if (threadIdx.x == 0 && s_distinct > 1u && (double)s_max / (double)s_sum < cat_max_ratio) s_chosen = cand;
        __syncthreads();
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int passed = s_chosen >= 0, cand = passed ? s_chosen : ncand - 1;
        int* row = selection + (size_t)n * 4;
        row[0] = cand; row[1] = rec->offy[cand]; row[2] = rec->offx[cand]; row[3] = passed;
    }
}

// ---- resize + crop + pad + blur + LUT + flip + normalise (cvk_crop_augment_u8) ---------------------------------------------------
// k_augment_u8's tile structure: a workgroup owns one CROP_TW x CROP_TH tile of one sample's hc x wc canvas (grid x, y, N).  Canvas
// pixel (y, x) shows resized pixel (y + offy, x + offx); the sample, its offsets (selection row) and Hr, Wr, sy, sx (record) are
// uniform per workgroup.  Stage A resamples the tile plus a blur halo of R pixels into LDS; the halo reflects (REFLECT_101) at the
// RESIZED IMAGE's borders, and positions further than R outside the image (pad, needed by no tap) are not sampled.  Stage B is the
// separable Gaussian, the LUT and the normalisation; pad pixels store constants; the flip mirrors the whole canvas at the store.
struct CropArgs {
    const uint8_t* frames;
    const void* masks;
    int mask_bytes, Hs, Ws, hc, wc;
    const cvk_crop_record* records;
    const int* selection;
    float m0, m1, m2, r0, r1, r2;
    int64_t pad_label;
    int pad_normalized;
    float* out;
    int64_t* out_masks;
    uint8_t* out_u8;
};

__device__ __forceinline__ void crop_store(const CropArgs& A, size_t o, float u0, float u1, float u2, bool normalise, int64_t label) {
    f32x4 f;
    f[0] = normalise ? (u0 * (1.f / 255.f) - A.m0) * A.r0 : 0.f;
    f[1] = normalise ? (u1 * (1.f / 255.f) - A.m1) * A.r1 : 0.f;
    f[2] = normalise ? (u2 * (1.f / 255.f) - A.m2) * A.r2 : 0.f;
    f[3] = 0.f;
    *reinterpret_cast<f32x4*>(A.out + o * 4) = f;
    if (A.out_u8) {
        A.out_u8[o * 3 + 0] = (uint8_t)u0;
        A.out_u8[o * 3 + 1] = (uint8_t)u1;
        A.out_u8[o * 3 + 2] = (uint8_t)u2;
    }
    A.out_masks[o] = label;
}

template <int R>
__device__ __forceinline__ void crop_tile(const CropArgs& A, const cvk_crop_record* rec, int offy, int offx, float* s_in, float* s_h,
                                          const uint8_t* s_lut, bool use_lut) {
    constexpr int LWr = CROP_TW + 2 * R, LHr = CROP_TH + 2 * R;
    const int n = blockIdx.z, x0 = blockIdx.x * CROP_TW, y0 = blockIdx.y * CROP_TH;
    const int Hr = rec->Hr, Wr = rec->Wr;
    const double sy = rec->sy, sx = rec->sx;
    const uint8_t* src = A.frames + (size_t)n * A.Hs * A.Ws * 3;

    // stage A: resized uint8 values of the tile and its halo -> s_in[c][ly][lx] (row stride CROP_LW)
    for (int idx = threadIdx.x; idx < LHr * LWr; idx += blockDim.x) {
        const int ly = idx / LWr, lx = idx - ly * LWr;
        const int py = y0 - R + ly + offy, px = x0 - R + lx + offx;        // resized coordinates before the reflection
        if (py < -R || py >= Hr + R || px < -R || px >= Wr + R) continue;  // no tap of an image pixel reaches it
        const int ry = aug_reflect101(py, Hr), rx = aug_reflect101(px, Wr);
        int iy0, iy1, ix0, ix1;
        float ay, ax;
        aug_coord(ry, sy, A.Hs, iy0, iy1, ay);
        aug_coord(rx, sx, A.Ws, ix0, ix1, ax);
        const uint8_t* p00 = src + ((size_t)iy0 * A.Ws + ix0) * 3;
        const uint8_t* p01 = src + ((size_t)iy0 * A.Ws + ix1) * 3;
        const uint8_t* p10 = src + ((size_t)iy1 * A.Ws + ix0) * 3;
        const uint8_t* p11 = src + ((size_t)iy1 * A.Ws + ix1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float top = (1.f - ax) * (float)p00[c] + ax * (float)p01[c];
            const float bot = (1.f - ax) * (float)p10[c] + ax * (float)p11[c];
            s_in[(c * CROP_LH + ly) * CROP_LW + lx] = aug_round_u8((1.f - ay) * top + ay * bot);
        }
    }
    float tp[2 * R + 1];
#pragma unroll
    for (int t = 0; t < 2 * R + 1; ++t) tp[t] = rec->taps[t];
    __syncthreads();

    if (R > 0) {  // horizontal pass over every staged row -> s_h[c][ly][tx] (row stride CROP_TW); pad columns and rows are not read later
        for (int idx = threadIdx.x; idx < LHr * CROP_TW; idx += blockDim.x) {
            const int ly = idx / CROP_TW, tx = idx - ly * CROP_TW;
            const int py = y0 - R + ly + offy, px = x0 + tx + offx;
            if (py < -R || py >= Hr + R || px < 0 || px >= Wr) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* row = s_in + (c * CROP_LH + ly) * CROP_LW + tx;
                float acc = 0.f;
#pragma unroll
                for (int t = 0; t < 2 * R + 1; ++t) acc = fmaf(tp[t], row[t], acc);
                s_h[(c * CROP_LH + ly) * CROP_TW + tx] = acc;
            }
        }
        __syncthreads();
    }

    const bool flip = rec->flip != 0;
    for (int idx = threadIdx.x; idx < CROP_TH * CROP_TW; idx += blockDim.x) {
        const int ty = idx / CROP_TW, tx = idx - ty * CROP_TW;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= A.hc || x >= A.wc) continue;
        const int xo = flip ? A.wc - 1 - x : x;
        const size_t o = ((size_t)n * A.hc + y) * A.wc + xo;
        const int ry = y + offy, rx = x + offx;
        if (ry < 0 || ry >= Hr || rx < 0 || rx >= Wr) {
            crop_store(A, o, 0.f, 0.f, 0.f, A.pad_normalized != 0, A.pad_label);
            continue;
        }
        float u[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v;
            if (R > 0) {
                float acc = 0.f;
#pragma unroll
                for (int t = 0; t < 2 * R + 1; ++t) acc = fmaf(tp[t], s_h[(c * CROP_LH + ty + t) * CROP_TW + tx], acc);
                v = aug_round_u8(acc);
            } else {
                v = s_in[(c * CROP_LH + ty) * CROP_LW + tx];
            }
            u[c] = use_lut ? (float)s_lut[(int)v] : v;
        }
        // mask: cv2 INTER_NEAREST of the resized pixel
        const size_t mi = ((size_t)n * A.Hs + crop_nearest(ry, sy, A.Hs)) * A.Ws + crop_nearest(rx, sx, A.Ws);
        const int64_t label = A.mask_bytes == 1 ? (int64_t)static_cast<const uint8_t*>(A.masks)[mi] : static_cast<const int64_t*>(A.masks)[mi];
        crop_store(A, o, u[0], u[1], u[2], true, label);
    }
}

__global__ void __launch_bounds__(256) k_crop_augment_u8(CropArgs A) {
    __shared__ float s_in[3 * CROP_LH * CROP_LW];
    __shared__ float s_h[3 * CROP_LH * CROP_TW];
    __shared__ uint8_t s_lut[256];
    const int n = blockIdx.z;
    const cvk_crop_record* rec = A.records + n;
    const int offy = A.selection[(size_t)n * 4 + 1], offx = A.selection[(size_t)n * 4 + 2];
    const int x0 = blockIdx.x * CROP_TW, y0 = blockIdx.y * CROP_TH;
    // a tile that shows nothing of the resized image writes constants only
    if (y0 + offy >= rec->Hr || y0 + CROP_TH + offy <= 0 || x0 + offx >= rec->Wr || x0 + CROP_TW + offx <= 0) {
        const bool flip = rec->flip != 0;
        for (int idx = threadIdx.x; idx < CROP_TH * CROP_TW; idx += blockDim.x) {
            const int ty = idx / CROP_TW, tx = idx - ty * CROP_TW;
            const int y = y0 + ty, x = x0 + tx;
            if (y >= A.hc || x >= A.wc) continue;
            const int xo = flip ? A.wc - 1 - x : x;
            crop_store(A, ((size_t)n * A.hc + y) * A.wc + xo, 0.f, 0.f, 0.f, A.pad_normalized != 0, A.pad_label);
        }
        return;
    }
    const bool use_lut = rec->use_lut != 0;
    if (use_lut)
        for (int i = threadIdx.x; i < 256; i += blockDim.x) s_lut[i] = rec->lut[i];   // visible after stage A's barrier
    const int k = rec->ksize;
    const int r = (k == 3 || k == 5 || k == 7 || k == 9) ? (k - 1) / 2 : 0;
    switch (r) {
        case 0: crop_tile<0>(A, rec, offy, offx, s_in, s_h, s_lut, use_lut); break;
        case 1: crop_tile<1>(A, rec, offy, offx, s_in, s_h, s_lut, use_lut); break;
        case 2: crop_tile<2>(A, rec, offy, offx, s_in, s_h, s_lut, use_lut); break;
        case 3: crop_tile<3>(A, rec, offy, offx, s_in, s_h, s_lut, use_lut); break;
        default: crop_tile<4>(A, rec, offy, offx, s_in, s_h, s_lut, use_lut); break;
    }
}

}  // namespace

extern "C" int cvk_crop_record_bytes(void) { return (int)sizeof(cvk_crop_record); }

extern "C" int cvk_crop_select(const void* masks, int mask_bytes, int N, int Hs, int Ws, int hc, int wc, const cvk_crop_record* records,
                               int ignore_index, double cat_max_ratio, uint32_t* counts, int32_t* selection, void* stream) {
    CVK_CHECK_ARG(masks && records && counts && selection, "cvk_crop_select: null pointer");
    CVK_CHECK_ARG(N > 0 && Hs > 0 && Ws > 0 && hc > 0 && wc > 0 && (mask_bytes == 1 || mask_bytes == 8), "cvk_crop_select: bad arguments");
    CVK_CHECK_ARG(cat_max_ratio > 0.0 && cat_max_ratio <= 1.0, "cvk_crop_select: cat_max_ratio outside (0, 1]");
    const long tiles_x = cvk_cdiv(wc, CROP_CW), tiles = tiles_x * cvk_cdiv(hc, CROP_CH);
    CVK_CHECK_ARG(N <= 65535 && tiles <= 0x7FFFFFFFL && (long)hc * wc <= 0x7FFFFFFFL && (long)N * CROP_MAX_CAND * CROP_BINS <= 0x7FFFFFFFL,
                  "cvk_crop_select: grid too large");
    const int words = N * CROP_MAX_CAND * CROP_BINS;
    hipLaunchKernelGGL(k_crop_clear, dim3(cvk_cdiv(words, 256)), dim3(256), 0, (hipStream_t)stream, (unsigned int*)counts, words);
    hipLaunchKernelGGL(k_crop_count, dim3((unsigned)tiles, CROP_MAX_CAND, N), dim3(256), 0, (hipStream_t)stream, masks, mask_bytes, Hs, Ws,
                       hc, wc, (int)tiles_x, records, ignore_index, (unsigned int*)counts);
    hipLaunchKernelGGL(k_crop_select, dim3(N), dim3(256), 0, (hipStream_t)stream, (const unsigned int*)counts, records, cat_max_ratio,
                       (int*)selection);
    CVK_LAUNCH_RETURN("cvk_crop_select");
}

extern "C" int cvk_crop_augment_u8(const uint8_t* frames, const void* masks, int mask_bytes, int N, int Hs, int Ws, int hc, int wc,
                                   const cvk_crop_record* records, const int32_t* selection, const float* mean3, const float* std3,
                                   int64_t pad_label, int pad_normalized, float* out, int64_t* out_masks, uint8_t* out_u8, void* stream) {
    CVK_CHECK_ARG(frames && masks && records && selection && mean3 && std3 && out && out_masks, "cvk_crop_augment_u8: null pointer");
    CVK_CHECK_ARG(N > 0 && Hs > 0 && Ws > 0 && hc > 0 && wc > 0 && (mask_bytes == 1 || mask_bytes == 8) && cvk_aligned16(out),
                  "cvk_crop_augment_u8: bad arguments");
    CVK_CHECK_ARG(N <= 65535 && cvk_cdiv(hc, CROP_TH) <= 65535, "cvk_crop_augment_u8: grid too large");
    CVK_CHECK_ARG(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "cvk_crop_augment_u8: zero std");
    CropArgs a;
    a.frames = frames; a.masks = masks; a.mask_bytes = mask_bytes;
    a.Hs = Hs; a.Ws = Ws; a.hc = hc; a.wc = wc;
    a.records = records; a.selection = selection;
    a.m0 = mean3[0]; a.m1 = mean3[1]; a.m2 = mean3[2];
    a.r0 = 1.f / std3[0]; a.r1 = 1.f / std3[1]; a.r2 = 1.f / std3[2];
    a.pad_label = pad_label; a.pad_normalized = pad_normalized;
    a.out = out; a.out_masks = out_masks; a.out_u8 = out_u8;
    hipLaunchKernelGGL(k_crop_augment_u8, dim3(cvk_cdiv(wc, CROP_TW), cvk_cdiv(hc, CROP_TH), N), dim3(256), 0, (hipStream_t)stream, a);
    CVK_LAUNCH_RETURN("cvk_crop_augment_u8");
}
