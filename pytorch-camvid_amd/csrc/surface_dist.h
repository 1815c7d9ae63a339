#pragma once
// ---- surface distances: Hausdorff, its percentile and ASSD (cvk_surface_distances; the definitions are in include/cvk.h) ---------------
// Borrows the row search and the column walk's constants of the distance transform (edt.h: edt_row_search, EDT_*) and the contour rule
// of the boundary F1 (boundary_f1.h: k_boundary_map, BF_*).  M = N H W, segment s = (n, direction, class) = (2 n + dir) C + c,
// direction 0 = prediction -> label, 1 = label -> prediction.  Seven kernels, all on the caller's stream:
//   k_sd_clear     zeroes the tail of the workspace: n and Q (uint64 [S] each), presence words [2 N], max [S], both histograms
//                  (first level [S][4096 + wide bins], second level [S][2][4096])
//   k_boundary_map (twice) the contour byte of both maps, uint8 [2][M]: the rule of the boundary F1, one device function
//   k_sd_cols      work-group = (map, image, 16 columns), the strip's contour bytes in LDS; thread = (column, class): the two uniform
//                  walks of k_edt_cols over contour bytes -> uint16 [2][M][C], the vertical distance to the nearest contour pixel of
//                  class c of that map in the column (0xFFFF: none); ORs the image's presence word of that map
//   k_sd_rows      work-group = one row (n, y): both maps' contour bytes of the row in LDS and, of a map whose partner row holds a
//                  contour pixel, the column distances transposed to [C][W].  Only a thread on a contour pixel of class c searches
//                  (edt_row_search<false>), only channel c of the other map, and only when that map has a contour of c in the image.
//                  Writes both planes of d2; n, max and Q are summed per class in LDS (integer atomics), one global integer atomic per
//                  (row, direction, class) that occurred.  First level of the select, per segment: one bin per value for d2 < 4096 (a
//                  rank that falls there is settled), one bin per 4096 values above (sd_bin1).  d2 < 64, the bulk, is counted per row
//                  in LDS and flushed with one add per non-empty bin; the rest goes straight to the segment's bins, equal keys of a
//                  wave first folded into one add
//   k_sd_pick      work-group = segment: k, r and the upper rank from n; the first-level bin of either rank and the rank inside it
//   k_sd_refine    thread = element of d2: for d2 >= 4096 in the bin of either rank, counts the low 12 bits (folded per wave as above)
//   k_sd_finish    work-group = segment: the low 12 bits of a rank whose bin is a wide one; writes the record's eight slots
// Every sum is an integer atomic, so neither the order of arrival nor the tiling changes a bit.  Every loop is bounded by W, H, the
// number of bins or the 64 lanes of a wave.
// LDS of k_sd_cols: 16 H B.  LDS of k_sd_rows: 2 W B of contour bytes + 512 C B of small-value counts (+ 4 W C B of column distances
// when all of it fits 64 KiB: 0.9 + 6 + 22.5 KiB at W = 480, C = 12; else the search reads the column distances from global memory)
// + 1 KiB of accumulators.
#include "cvk_common.h"
#include "edt.h"
#include "boundary_f1.h"

namespace {

constexpr int SD_SLOTS = 8, SD_LOW_BITS = 12, SD_LOW_BINS = 1 << SD_LOW_BITS, SD_MAX_SEG_GROUPS = 1 << 20;
constexpr int SD_SMALL = 64;                               // d2 below this is counted in LDS by k_sd_rows

// First-level bin of a d2: the value itself below 4096 (the select ends there), above it one bin per 4096 values
__host__ __device__ __forceinline__ int sd_bin1(int v) { return v < SD_LOW_BINS ? v : SD_LOW_BINS - 1 + (v >> SD_LOW_BITS); }

struct SdLayout {
    size_t col, bmap, sel, an, aq, present, amax, hist1, hist2, total;   // byte offsets; [an, total) is what k_sd_clear zeroes
    size_t M, S;
    int nb1;                                                              // first-level bins that a d2 of this image size can reach
};

__host__ __device__ __forceinline__ size_t sd_align16(size_t b) { return (b + 15) & ~(size_t)15; }

inline SdLayout sd_layout(int N, int H, int W, int C) {
    SdLayout L;
    L.M = (size_t)N * H * W;
    L.S = (size_t)N * 2 * C;
    L.nb1 = sd_bin1((int)((int64_t)(H - 1) * (H - 1) + (int64_t)(W - 1) * (W - 1))) + 1;
    L.col = 0;
    L.bmap = sd_align16(2 * L.M * C * sizeof(unsigned short));
    L.sel = L.bmap + sd_align16(2 * L.M);
    L.an = L.sel + sd_align16(L.S * 4 * sizeof(int));
    L.aq = L.an + sd_align16(L.S * 8);
    L.present = L.aq + sd_align16(L.S * 8);
    L.amax = L.present + sd_align16((size_t)2 * N * 4);
    L.hist1 = L.amax + sd_align16(L.S * 4);
    L.hist2 = L.hist1 + sd_align16(L.S * L.nb1 * 4);
    L.total = L.hist2 + sd_align16(L.S * 2 * SD_LOW_BINS * 4);
    return L;
}

__global__ __launch_bounds__(256) void k_sd_clear(uint4* __restrict__ p, size_t n16) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// grid (N strips, 2): (image, strip of EDT_COL_TX columns), map (0 = prediction, 1 = label).  LDS: the strip's contour bytes [H][EDT_COL_TX].
__global__ __launch_bounds__(256) void k_sd_cols(const unsigned char* __restrict__ bmap, unsigned short* __restrict__ col,
                                                unsigned* __restrict__ present, int strips, int N, int H, int W, int C) {
    extern __shared__ unsigned char sd_b[];
    const int which = blockIdx.y, n = blockIdx.x / strips, x0 = (blockIdx.x - n * strips) * EDT_COL_TX;
    const size_t img = ((size_t)which * N + n) * H * W;
    const unsigned char* B = bmap + img;
    for (int i = threadIdx.x; i < H * EDT_COL_TX; i += 256) {
        const int y = i / EDT_COL_TX, x = x0 + (i - y * EDT_COL_TX);
        sd_b[i] = x < W ? B[(size_t)y * W + x] : BF_NONE;
    }
    __syncthreads();
    const size_t os = (size_t)W * C;
    for (int item = threadIdx.x; item < EDT_COL_TX * C; item += 256) {
        const int xx = item / C, c = item - xx * C;
        if (x0 + xx >= W) continue;
        const unsigned char* s = sd_b + xx;
        unsigned short* o = col + (img + x0 + xx) * C + c;
        // the two walks of k_edt_cols: down, storing the distance to the nearest match above; up in batches, lowering what was stored
        int last = -1;
        for (int y = 0; y < H; ++y) {
            if (s[y * EDT_COL_TX] == c) last = y;
            o[y * os] = (unsigned short)(last < 0 ? EDT_NONE : (unsigned)(y - last));
        }
        int next = -1;
        for (int y1 = H; y1 > 0; y1 -= EDT_COL_BATCH) {
            unsigned v[EDT_COL_BATCH];
#pragma unroll
            for (int j = 0; j < EDT_COL_BATCH; ++j) v[j] = y1 - 1 - j >= 0 ? (unsigned)o[(y1 - 1 - j) * os] : 0u;
#pragma unroll
            for (int j = 0; j < EDT_COL_BATCH; ++j) {
                const int y = y1 - 1 - j;
                if (y < 0) break;
                if (s[y * EDT_COL_TX] == c) next = y;
                if (next >= 0 && (unsigned)(next - y) < v[j]) o[y * os] = (unsigned short)(next - y);
            }
        }
        if (last >= 0) atomicOr(&present[2 * n + which], 1u << c);
    }
}

// The largest q with q * q <= d2 * 2^32: the root in 2^-16 pixels.  d2 < 2^24, so d2 * 2^32 is exact in a double; the rounded double
// root is within one of the answer, and the two integer comparisons settle it.
__device__ __forceinline__ unsigned long long sd_isqrt_fx(int d2) {
    const unsigned long long v = (unsigned long long)(unsigned)d2 << 32;
    unsigned long long q = (unsigned long long)__builtin_sqrt((double)v);
    if (q * q > v) --q;
    else if ((q + 1) * (q + 1) <= v) ++q;
    return q;
}

// hist[key] += 1 for every active lane; lanes of the wave with one key send one add.  Call it from wave-uniform control flow.  At most
// 64 rounds: every round retires its leader.
__device__ __forceinline__ void sd_hist_add(unsigned* __restrict__ hist, bool active, size_t key) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned lo = __shfl((unsigned)key, leader), hi = __shfl((unsigned)(key >> 32), leader);
        const size_t k = ((size_t)hi << 32) | lo;
        const unsigned long long same = __ballot(active && key == k);
        if (lane == leader) atomicAdd(hist + k, (unsigned)__popcll(same));
        todo &= ~same;
    }
}

// grid N H.  LDS: contour bytes [2][Wp] (Wp = W rounded up to 4), the counts of small d2 [2][C][SD_SMALL], then STAGED the column
// distances [2][C][W].
template <bool STAGED>
__global__ __launch_bounds__(256) void k_sd_rows(const unsigned char* __restrict__ bmap, const unsigned short* __restrict__ col,
                                                const unsigned* __restrict__ present, int* __restrict__ d2,
                                                unsigned long long* __restrict__ an, unsigned long long* __restrict__ aq,
                                                unsigned* __restrict__ amax, unsigned* __restrict__ hist1, int nb1, size_t M, int H, int W,
                                                int C) {
    extern __shared__ unsigned char sd_lds[];
    __shared__ unsigned s_n[2][BF_MAX_K], s_mx[2][BF_MAX_K];
    __shared__ unsigned long long s_q[2][BF_MAX_K];
    const size_t row = blockIdx.x;
    const int n = (int)(row / H);
    const int Wp = (W + 3) & ~3;
    unsigned char* s_b = sd_lds;
    unsigned* s_small = reinterpret_cast<unsigned*>(sd_lds + 2 * Wp);
    unsigned short* s_col = reinterpret_cast<unsigned short*>(s_small + 2 * C * SD_SMALL);
    if (threadIdx.x < 2 * BF_MAX_K) {
        (&s_n[0][0])[threadIdx.x] = 0u;
        (&s_mx[0][0])[threadIdx.x] = 0u;
        (&s_q[0][0])[threadIdx.x] = 0ull;
    }
    for (int i = threadIdx.x; i < 2 * C * SD_SMALL; i += 256) s_small[i] = 0u;
    int mine = 0;                                          // bit dir: this thread saw a contour pixel of map dir
    for (int x = threadIdx.x; x < W; x += 256)
        for (int dir = 0; dir < 2; ++dir) {
            const unsigned char b = bmap[dir * M + row * W + x];
            s_b[dir * Wp + x] = b;
            if (b < C) mine |= 1 << dir;
        }
    // whether the row of either map holds a contour pixel (the OR is of truth values, one call per map); also the barrier for s_b
    // and the accumulators
    const int any = (__syncthreads_or(mine & 1) ? 1 : 0) | (__syncthreads_or(mine & 2) ? 2 : 0);
    const unsigned pres0 = present[2 * n], pres1 = present[2 * n + 1];
    if (STAGED) {
        // a search from map dir reads the distances of the other map
        for (int dir = 0; dir < 2; ++dir) {
            if (!((any >> dir) & 1)) continue;
            const int other = 1 - dir;
            const unsigned short* g = col + (other * M + row * W) * C;
            for (int i = threadIdx.x; i < W * C; i += 256) {
                const int x = i / C, c = i - x * C;
                s_col[(other * C + c) * W + x] = g[i];
            }
        }
        __syncthreads();
    }
    for (int x0 = 0; x0 < W; x0 += 256) {
        const int x = x0 + threadIdx.x;
        for (int dir = 0; dir < 2; ++dir) {
            const int other = 1 - dir;
            const unsigned pres_other = other ? pres1 : pres0;
            int out = -2, c = 0;
            if (x < W) {
                const unsigned char b = s_b[dir * Wp + x];
                if (b < C) {
                    c = b;
                    atomicAdd(&s_n[dir][c], 1u);
                    out = -1;
                    if ((pres_other >> c) & 1u) {
                        out = STAGED ? edt_row_search<false>(s_col + (other * C + c) * W, 1, nullptr, 0, x, W)
                                     : edt_row_search<false>(col + (other * M + row * W) * C + c, C, nullptr, 0, x, W);
                        atomicMax(&s_mx[dir][c], (unsigned)out);
                        atomicAdd(&s_q[dir][c], sd_isqrt_fx(out));
                    }
                }
                d2[dir * M + row * W + x] = out;
            }
            // the first level of the select: small values, the bulk of them, per row in LDS; the others straight to the segment's bins
            if (out >= 0 && out < SD_SMALL) atomicAdd(&s_small[(dir * C + c) * SD_SMALL + out], 1u);
            const size_t seg = ((size_t)2 * n + dir) * C + c;
            sd_hist_add(hist1, out >= SD_SMALL, seg * nb1 + sd_bin1(max(out, 0)));
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C * SD_SMALL; i += 256)
        if (s_small[i]) atomicAdd(&hist1[((size_t)2 * n * C + i / SD_SMALL) * nb1 + (i & (SD_SMALL - 1))], s_small[i]);
    if (threadIdx.x < 2 * C) {
        const int dir = threadIdx.x / C, c = threadIdx.x - dir * C;
        const size_t seg = ((size_t)2 * n + dir) * C + c;
        if (s_n[dir][c]) {
            atomicAdd(&an[seg], (unsigned long long)s_n[dir][c]);
            if (((dir ? pres0 : pres1) >> c) & 1u) {
                atomicMax(&amax[seg], s_mx[dir][c]);
                atomicAdd(&aq[seg], s_q[dir][c]);
            }
        }
    }
}

// The bin of `hist` [bins] that holds 0-based rank R (R below the histogram's total), and R's rank inside that bin.  All 256 threads
// call it; the answer is in res[0], res[1] after it returns.  s_part: 256 words of LDS.
__device__ __forceinline__ void sd_locate(const unsigned* __restrict__ hist, int bins, unsigned long long R, unsigned long long* s_part,
                                          long long* res) {
    const int per = (bins + 255) / 256, b0 = threadIdx.x * per, b1 = min(bins, b0 + per);
    unsigned long long sum = 0;
    for (int b = b0; b < b1; ++b) sum += hist[b];
    __syncthreads();                                       // s_part and res of an earlier call have been read
    s_part[threadIdx.x] = sum;
    __syncthreads();
    unsigned long long before = 0;
    for (int t = 0; t < (int)threadIdx.x; ++t) before += s_part[t];
    if (R >= before && R < before + sum) {
        unsigned long long cum = before;
        for (int b = b0; b < b1; ++b) {
            const unsigned h = hist[b];
            if (R < cum + h) {
                res[0] = b;
                res[1] = (long long)(R - cum);
                break;
            }
            cum += h;
        }
    }
    __syncthreads();
}

// n of segment seg and of its partner -> evaluated, k, r and the upper rank
__device__ __forceinline__ bool sd_ranks(const unsigned long long* __restrict__ an, size_t seg, int C, int qnum, int qden,
                                         unsigned long long& n, unsigned long long& m, unsigned long long& k, unsigned long long& r,
                                         unsigned long long& khi) {
    const size_t pair = seg / C, c = seg - pair * C;
    n = an[seg];
    m = an[(pair ^ 1) * C + c];
    if (n == 0 || m == 0) return false;
    const unsigned long long t = (n - 1) * (unsigned long long)qnum;
    k = t / (unsigned long long)qden;
    r = t - k * (unsigned long long)qden;
    khi = r > 0 ? min(k + 1, n - 1) : k;
    return true;
}

// sel[seg][4] = top-digit bin of rank k, k's rank inside it, the same two of the upper rank; -1 where the segment is not evaluated
__global__ __launch_bounds__(256) void k_sd_pick(const unsigned long long* __restrict__ an, const unsigned* __restrict__ hist1, int nb1,
                                                int* __restrict__ sel, size_t S, int C, int qnum, int qden) {
    __shared__ unsigned long long s_part[256];
    __shared__ long long s_res[4];
    for (size_t seg = blockIdx.x; seg < S; seg += gridDim.x) {
        unsigned long long n, m, k, r, khi;
        const bool ev = sd_ranks(an, seg, C, qnum, qden, n, m, k, r, khi);
        __syncthreads();                                   // s_res of the previous segment has been read
        if (threadIdx.x < 4) s_res[threadIdx.x] = -1;
        if (ev) {
            sd_locate(hist1 + seg * nb1, nb1, k, s_part, s_res);
            sd_locate(hist1 + seg * nb1, nb1, khi, s_part, s_res + 2);
        }
        __syncthreads();
        if (threadIdx.x < 4) sel[seg * 4 + threadIdx.x] = (int)s_res[threadIdx.x];
    }
}

// thread = element of d2 [2][M]: hist2[seg][j][low 12 bits] += 1 where d2 >= 4096 and its first-level bin is that of rank j of its
// segment (a rank that fell on a d2 below 4096 needs no second level)
__global__ __launch_bounds__(256) void k_sd_refine(const int* __restrict__ d2, const unsigned char* __restrict__ bmap,
                                                  const int* __restrict__ sel, unsigned* __restrict__ hist2, size_t M, int HW, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int v = -2;
    size_t seg = 0;
    if (i < 2 * M) {
        v = d2[i];
        if (v >= SD_LOW_BINS) {
            const int dir = i >= M;
            const size_t n = (i - dir * M) / HW;
            seg = (2 * n + dir) * C + bmap[i];
        }
    }
    const int top = sd_bin1(max(v, 0));
    const size_t low = (size_t)(v & (SD_LOW_BINS - 1));
    for (int j = 0; j < 2; ++j) {
        const bool hit = v >= SD_LOW_BINS && sel[seg * 4 + 2 * j] == top;
        sd_hist_add(hist2, hit, (seg * 2 + j) * SD_LOW_BINS + low);
    }
}

// record[seg][8]: n, m, max d2, Q, k, r, d2_lo, d2_hi (include/cvk.h)
__global__ __launch_bounds__(256) void k_sd_finish(const unsigned long long* __restrict__ an, const unsigned long long* __restrict__ aq,
                                                  const unsigned* __restrict__ amax, const int* __restrict__ sel,
                                                  const unsigned* __restrict__ hist2, long long* __restrict__ record, size_t S, int C,
                                                  int qnum, int qden) {
    __shared__ unsigned long long s_part[256];
    __shared__ long long s_res[4];
    for (size_t seg = blockIdx.x; seg < S; seg += gridDim.x) {
        unsigned long long n, m, k, r, khi;
        const bool ev = sd_ranks(an, seg, C, qnum, qden, n, m, k, r, khi);
        __syncthreads();
        if (threadIdx.x < 4) s_res[threadIdx.x] = -1;
        long long val[2] = {-1, -1};
        for (int j = 0; j < 2; ++j) {
            const int bin = ev ? sel[seg * 4 + 2 * j] : 0;         // below 4096: the value itself
            val[j] = bin;
            if (bin >= SD_LOW_BINS)
                sd_locate(hist2 + (seg * 2 + j) * SD_LOW_BINS, SD_LOW_BINS, (unsigned long long)sel[seg * 4 + 2 * j + 1], s_part, s_res + 2 * j);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            long long* o = record + seg * SD_SLOTS;
            o[0] = (long long)n;
            o[1] = (long long)m;
            o[2] = ev ? (long long)amax[seg] : -1;
            o[3] = ev ? (long long)aq[seg] : 0;
            o[4] = ev ? (long long)k : -1;
            o[5] = ev ? (long long)r : -1;
            for (int j = 0; j < 2; ++j)
                if (val[j] >= SD_LOW_BINS) val[j] = ((val[j] - (SD_LOW_BINS - 1)) << SD_LOW_BITS) | s_res[2 * j];
            o[6] = ev ? val[0] : -1;
            o[7] = ev ? val[1] : -1;
        }
    }
}

}  // namespace

extern "C" int64_t cvk_surface_workspace_bytes(int N, int H, int W, int num_classes) {
    if (cvk_edt_workspace_bytes(N, H, W, num_classes) == 0) return 0;
    const SdLayout L = sd_layout(N, H, W, num_classes);
    return (L.total - L.an) / 16 / 256 < 2147483648ULL ? (int64_t)L.total : 0;
}

extern "C" int cvk_surface_record_slots(void) { return SD_SLOTS; }

extern "C" int cvk_surface_distances(const int64_t* pred, const int64_t* label, int N, int H, int W, int num_classes, int ignore_index,
                                     int qnum, int qden, void* workspace, int32_t* d2, int64_t* record, void* stream) {
    CVK_CHECK_ARG(pred && label && workspace && d2 && record, "cvk_surface_distances: null pointer");
    const int rc = edt_check_sizes("cvk_surface_distances", N, H, W, num_classes);
    if (rc != CVK_OK) return rc;
    CVK_CHECK_ARG(cvk_surface_workspace_bytes(N, H, W, num_classes) > 0, "cvk_surface_distances: the workspace of N %d, %d classes is too large",
                  N, num_classes);
    CVK_CHECK_ARG(qden >= 1 && qden <= 10000 && qnum >= 0 && qnum <= qden,
                  "cvk_surface_distances: percentile fraction %d / %d, need 0 <= qnum <= qden <= 10000", qnum, qden);
    CVK_CHECK_ARG(((uintptr_t)workspace & 15u) == 0, "cvk_surface_distances: the workspace must be 16-byte aligned");
    CVK_CHECK_ARG(((uintptr_t)d2 & 3u) == 0 && ((uintptr_t)record & 7u) == 0, "cvk_surface_distances: d2 or record misaligned");
    hipStream_t s = (hipStream_t)stream;
    const int C = num_classes;
    const SdLayout L = sd_layout(N, H, W, C);
    char* ws = static_cast<char*>(workspace);
    unsigned short* col = reinterpret_cast<unsigned short*>(ws + L.col);
    unsigned char* bmap = reinterpret_cast<unsigned char*>(ws + L.bmap);
    int* sel = reinterpret_cast<int*>(ws + L.sel);
    unsigned long long* an = reinterpret_cast<unsigned long long*>(ws + L.an);
    unsigned long long* aq = reinterpret_cast<unsigned long long*>(ws + L.aq);
    unsigned* present = reinterpret_cast<unsigned*>(ws + L.present);
    unsigned* amax = reinterpret_cast<unsigned*>(ws + L.amax);
    unsigned* hist1 = reinterpret_cast<unsigned*>(ws + L.hist1);
    unsigned* hist2 = reinterpret_cast<unsigned*>(ws + L.hist2);
    const size_t n16 = (L.total - L.an) / 16;
    hipLaunchKernelGGL(k_sd_clear, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<uint4*>(ws + L.an), n16);
    const dim3 gpx(cvk_cdiv((long)L.M, 256));
    hipLaunchKernelGGL(k_boundary_map, gpx, dim3(256), 0, s, pred, label, bmap, N, H, W, C, ignore_index);
    hipLaunchKernelGGL(k_boundary_map, gpx, dim3(256), 0, s, label, label, bmap + L.M, N, H, W, C, ignore_index);
    const int strips = cvk_cdiv(W, EDT_COL_TX);
    hipLaunchKernelGGL(k_sd_cols, dim3((unsigned)N * strips, 2), dim3(256), (size_t)H * EDT_COL_TX, s, bmap, col, present, strips, N, H, W, C);
    const size_t bytes_b = (size_t)2 * ((W + 3) & ~3) + sizeof(unsigned) * 2 * C * SD_SMALL, staged = bytes_b + (size_t)4 * W * C;
    if (staged + 1024 <= EDT_LDS_LIMIT)
        hipLaunchKernelGGL(k_sd_rows<true>, dim3((unsigned)N * H), dim3(256), staged, s, bmap, col, present, d2, an, aq, amax, hist1, L.nb1,
                           L.M, H, W, C);
    else
        hipLaunchKernelGGL(k_sd_rows<false>, dim3((unsigned)N * H), dim3(256), bytes_b, s, bmap, col, present, d2, an, aq, amax, hist1,
                           L.nb1, L.M, H, W, C);
    const dim3 gseg((unsigned)(L.S < (size_t)SD_MAX_SEG_GROUPS ? L.S : (size_t)SD_MAX_SEG_GROUPS));
    hipLaunchKernelGGL(k_sd_pick, gseg, dim3(256), 0, s, an, hist1, L.nb1, sel, L.S, C, qnum, qden);
    hipLaunchKernelGGL(k_sd_refine, dim3((unsigned)((2 * L.M + 255) / 256)), dim3(256), 0, s, d2, bmap, sel, hist2, L.M, H * W, C);
    hipLaunchKernelGGL(k_sd_finish, gseg, dim3(256), 0, s, an, aq, amax, sel, hist2, reinterpret_cast<long long*>(record), L.S, C, qnum, qden);
    CVK_LAUNCH_RETURN("cvk_surface_distances");
}
