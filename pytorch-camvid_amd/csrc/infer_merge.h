#pragma once
// infer_merge.h: the two inference merges.  Multi-scale / flip test-time augmentation (cvk_tta_accumulate, cvk_tta_resize_input) folds one view's
// logits into a probability accumulator; sliding-window inference (cvk_window_merge) folds one window's logits into the full-size map
// under the same limits (TTA_MAX_C, TTA_MAX_DIM).  loss_rows.h is included for CE_CHUNK and the chunk staging (ce_chunk_load / _store).
#include "cvk_common.h"
#include "loss_rows.h"

namespace {

// ---- multi-scale / flip test-time augmentation (cvk_tta_accumulate, cvk_tta_resize_input) ---------------------------------------
// One launch per view folds that view's logits into the [M][C] probability accumulator: a workgroup owns CE_CHUNK consecutive
// accumulator rows (a contiguous span of 256 C floats), one thread per pixel.  The accumulator side is staged through LDS exactly
// as k_ce_fwd stages its logits (a thread's own row is C floats apart from its neighbour's: read and written directly, a wave
// would touch 64 lines for 64 * 4 useful bytes per instruction), with pitch C + 1 so the row walk is conflict free.  The gather
// side is not staged: a pixel reads the two or four source rows around its sample position straight from global memory, as
// 16-byte vectors where the layout allows; neighbouring pixels share source rows, and a view's logits are at most a few tens of
// MB that the pass walks in order, so these reads are L2 hits after the first touch.  The resampled logits, their softmax and the
// arg-max stay in registers (CP = C rounded up to a multiple of 4 is the compile-time register count).
// Sample positions come from integers (include/cvk.h); the divisions are per row and per column, never per channel: the rows a
// workgroup covers are tabulated in LDS by its first threads, a thread computes its own column once.
constexpr int TTA_MAX_C = 32;            // classes held in registers per pixel
constexpr int TTA_MAX_DIM = 16384;       // (2 d + 1) in - out stays inside int32

struct TtaTap {
    int i0, i1;                          // lower / upper source index (upper clamped to the last one)
    float w0, w1;                        // their weights (1 - f, f)
};

__device__ __forceinline__ TtaTap tta_tap(int dst, int in, int out) {
    const int den = 2 * out;
    int num = (2 * dst + 1) * in - out;
    num = num < 0 ? 0 : num;
    const int i0 = num / den, rem = num - i0 * den;
    TtaTap t;
    t.i0 = i0;
    t.i1 = i0 + 1 < in ? i0 + 1 : in - 1;
    t.w1 = (float)rem / (float)den;      // both exact in fp32 (< 2^24): one rounding
    t.w0 = 1.f - t.w1;
    return t;
}

template <int CP, bool IDENT>
__global__ __launch_bounds__(CE_CHUNK) void k_tta_accumulate(const float* __restrict__ logits, int ld, int h, int w,
                                                            float* __restrict__ acc, int64_t* __restrict__ pred, int H, int W, int M,
                                                            int C, int flip, int first, int last, float inv_k) {
    extern __shared__ float lds[];       // CE_CHUNK accumulator rows, pitch C + 1
    __shared__ TtaTap s_row[CE_CHUNK];   // the output rows this workgroup's pixels lie in (at most CE_CHUNK of them, at W = 1)
    __shared__ int s_img[CE_CHUNK];
    const int pitch = C + 1;
    const int m0 = blockIdx.x * CE_CHUNK;
    const int rows = min(CE_CHUNK, M - m0);
    const int gy0 = m0 / W;                                   // uniform: first row of the [N * H] rows this workgroup touches
    const int nrows = (m0 + rows - 1) / W - gy0 + 1;
    for (int r = threadIdx.x; r < nrows; r += CE_CHUNK) {
        const int gy = gy0 + r, n = gy / H;
        s_row[r] = tta_tap(gy - n * H, h, H);
        s_img[r] = n;
    }
    if (!first) ce_chunk_load(acc + (size_t)m0 * C, lds, rows * C, C);
    __syncthreads();
    int bi = 0;
    if ((int)threadIdx.x < rows) {
        // (row, column) of pixel m0 + threadIdx.x relative to row gy0: off < W + CE_CHUNK < 2^24, so the fp32 quotient is off by one at most
        const int off = m0 - gy0 * W + (int)threadIdx.x;
        int q = (int)((float)off * (1.f / (float)W));
        int x = off - q * W;
        if (x < 0) { x += W; --q; } else if (x >= W) { x -= W; ++q; }
        const TtaTap ty = s_row[q];
        const TtaTap tx = tta_tap(flip ? W - 1 - x : x, w, W);
        const float* img = logits + (size_t)s_img[q] * h * w * ld;
        const float* r00 = img + ((size_t)ty.i0 * w + tx.i0) * ld;
        float v[CP];
        const bool vec = (C & 3) == 0 && (ld & 3) == 0 && ((uintptr_t)logits & 15u) == 0;        // uniform
        if (IDENT) {                                          // view at the output size: weights (1, 0) both ways, one source row
            if (vec) {
#pragma unroll
                for (int j = 0; j < CP / 4; ++j) {
                    const f32x4 a = reinterpret_cast<const f32x4*>(r00)[j];
                    v[4 * j] = a[0]; v[4 * j + 1] = a[1]; v[4 * j + 2] = a[2]; v[4 * j + 3] = a[3];
                }
            } else {
#pragma unroll
                for (int c = 0; c < CP; ++c) v[c] = c < C ? r00[c] : 0.f;
            }
        } else {
            const float* r01 = img + ((size_t)ty.i0 * w + tx.i1) * ld;
            const float* r10 = img + ((size_t)ty.i1 * w + tx.i0) * ld;
            const float* r11 = img + ((size_t)ty.i1 * w + tx.i1) * ld;
            if (vec) {
#pragma unroll
                for (int j = 0; j < CP / 4; ++j) {
                    const f32x4 a = reinterpret_cast<const f32x4*>(r00)[j], b = reinterpret_cast<const f32x4*>(r01)[j];
                    const f32x4 c = reinterpret_cast<const f32x4*>(r10)[j], d = reinterpret_cast<const f32x4*>(r11)[j];
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[4 * j + k] = ty.w0 * (tx.w0 * a[k] + tx.w1 * b[k]) + ty.w1 * (tx.w0 * c[k] + tx.w1 * d[k]);
                }
            } else {
#pragma unroll
                for (int c = 0; c < CP; ++c)
                    v[c] = c < C ? ty.w0 * (tx.w0 * r00[c] + tx.w1 * r01[c]) + ty.w1 * (tx.w0 * r10[c] + tx.w1 * r11[c]) : 0.f;
            }
        }
        float mx = v[0];
#pragma unroll
        for (int c = 1; c < CP; ++c)
            if (c < C) mx = fmaxf(mx, v[c]);
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) { v[c] = expf(v[c] - mx); se += v[c]; }
        const float inv = 1.f / se;
        float* p = lds + threadIdx.x * pitch;
        float best = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            if (c < C) {
                float s = v[c] * inv;
                if (!first) s = p[c] + s;
                if (last) s *= inv_k;
                p[c] = s;
                if (c == 0 || s > best || (s != s && best == best)) { best = s; bi = c; }   // k_argmax's rule on the stored values
            }
        }
    }
    __syncthreads();
    ce_chunk_store(acc + (size_t)m0 * C, lds, rows * C, C);
    if (last && (int)threadIdx.x < rows) pred[m0 + threadIdx.x] = bi;
}

// A view's network input: [N][3][H][W] of any strides -> NHWC-4 [N][h][w][4]; grid (ceil(w / 256), h, N), so the row tap is uniform
// per workgroup and a thread divides once, for its column.
__global__ __launch_bounds__(256) void k_tta_resize_input(const float* __restrict__ src, int64_t sN, int64_t sC, int64_t sH, int64_t sW,
                                                         float* __restrict__ dst, int H, int W, int h, int w, int flip) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
    if (x >= w) return;
    const TtaTap ty = tta_tap(y, H, h);
    const TtaTap tx = tta_tap(flip ? w - 1 - x : x, W, w);
    const float* b = src + n * sN;
    const int64_t o00 = ty.i0 * sH + tx.i0 * sW, o01 = ty.i0 * sH + tx.i1 * sW, o10 = ty.i1 * sH + tx.i0 * sW, o11 = ty.i1 * sH + tx.i1 * sW;
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = b + c * sC;
        o[c] = ty.w0 * (tx.w0 * p[o00] + tx.w1 * p[o01]) + ty.w1 * (tx.w0 * p[o10] + tx.w1 * p[o11]);
    }
    o[3] = 0.f;
    *reinterpret_cast<f32x4*>(dst + (((size_t)n * h + y) * w + x) * 4) = o;
}

// ---- sliding-window inference: the merge of overlapping windows' logits (cvk_window_merge) ---------------------------------------
// One launch per window folds that window's logits into the full-size map: a workgroup owns CE_CHUNK consecutive pixels of the window
// (a contiguous span of 256 ld floats of the logits; in `out` one contiguous span of C floats per window row it touches).  The pass is
// element-wise, so it runs in the order of the floats, not one pixel per thread: consecutive lanes move consecutive 16-byte vectors of
// both sides (full lines, as ce_chunk_load / ce_chunk_store move theirs), and a pixel's terms — where it lies in `out`, how many windows
// cover it, whether this window is the first or the last of them — come from a table in LDS that the pixel's thread fills once.  Those
// terms are integer closed forms of the grid (include/cvk.h), divided out per window row (tabulated by the workgroup's first threads, as
// k_tta_accumulate tabulates its row taps) and per column, never per channel.  Only the values of the pixels this window finishes go
// through LDS (pitch C + 1), for the arg-max: one thread per finished pixel walks its row with a scalar running best.
struct WinGrid {
    int H, W, hw, ww, sy, sx, gy, gx, iy, ix, y1, x1;
};

struct WinCover {
    int lo, hi;                          // first / last grid index whose window holds the position
};

// windows of `win` positions at min(i * stride, size - win), i < g, stride <= win: the i whose window holds position p
__device__ __forceinline__ WinCover win_cover(int p, int size, int win, int stride, int g) {
    WinCover c;
    c.lo = p < win ? 0 : min((p - win) / stride + 1, g - 1);
    c.hi = p >= size - win ? g - 1 : p / stride;
    return c;
}

constexpr int WIN_FIRST = 1, WIN_LAST = 2;

__global__ __launch_bounds__(CE_CHUNK) void k_window_merge(const float* __restrict__ logits, int ld, float* __restrict__ out,
                                                          int64_t* __restrict__ pred, int M, int C, WinGrid g) {
    extern __shared__ float lds[];       // the finished pixels' values, pitch C + 1 (no bytes when pred is null)
    __shared__ int s_row_pix[CE_CHUNK], s_row_cnt[CE_CHUNK], s_row_fl[CE_CHUNK];   // the window rows this workgroup touches (at most CE_CHUNK, at ww = 1)
    __shared__ int s_pix[CE_CHUNK], s_cnt[CE_CHUNK], s_fl[CE_CHUNK];               // its pixels: index in out / pred, count, WIN_FIRST | WIN_LAST
    const int pitch = C + 1;
    const int m0 = blockIdx.x * CE_CHUNK;
    const int rows = min(CE_CHUNK, M - m0);
    const int r0 = m0 / g.ww;                                 // uniform: first of the [N * hw] window rows this workgroup touches
    const int nrows = (m0 + rows - 1) / g.ww - r0 + 1;
    for (int r = threadIdx.x; r < nrows; r += CE_CHUNK) {
        const int wr = r0 + r, n = wr / g.hw, y = g.y1 + (wr - n * g.hw);
        const WinCover cy = win_cover(y, g.H, g.hw, g.sy, g.gy);
        s_row_pix[r] = (n * g.H + y) * g.W + g.x1;
        s_row_cnt[r] = cy.hi - cy.lo + 1;
        s_row_fl[r] = (g.iy == cy.lo ? WIN_FIRST : 0) | (g.iy == cy.hi ? WIN_LAST : 0);
    }
    __syncthreads();
    if ((int)threadIdx.x < rows) {
        // (row, column) of pixel m0 + threadIdx.x relative to row r0: off < ww + CE_CHUNK < 2^24, so the fp32 quotient is off by one at most
        const int off = m0 - r0 * g.ww + (int)threadIdx.x;
        int q = (int)((float)off * (1.f / (float)g.ww));
        int x = off - q * g.ww;
        if (x < 0) { x += g.ww; --q; } else if (x >= g.ww) { x -= g.ww; ++q; }
        const WinCover cx = win_cover(g.x1 + x, g.W, g.ww, g.sx, g.gx);
        s_pix[threadIdx.x] = s_row_pix[q] + x;
        s_cnt[threadIdx.x] = s_row_cnt[q] * (cx.hi - cx.lo + 1);
        s_fl[threadIdx.x] = s_row_fl[q] & ((g.ix == cx.lo ? WIN_FIRST : 0) | (g.ix == cx.hi ? WIN_LAST : 0));
    }
    __syncthreads();
    const float* lg = logits + (size_t)m0 * ld;
    if ((C & 3) == 0 && (ld & 3) == 0 && (((uintptr_t)logits | (uintptr_t)out) & 15u) == 0) {       // uniform
        const int nv = C >> 2;
        for (int v = threadIdx.x; v < rows * nv; v += CE_CHUNK) {
            const int p = v / nv, c = (v - p * nv) * 4;
            const int fl = s_fl[p];
            f32x4 s = *reinterpret_cast<const f32x4*>(lg + (size_t)p * ld + c);
            float* o = out + (size_t)s_pix[p] * C + c;
            if (!(fl & WIN_FIRST)) s = *reinterpret_cast<const f32x4*>(o) + s;
            if (fl & WIN_LAST) {
                const float d = (float)s_cnt[p];
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] = __fdiv_rn(s[k], d);
                if (pred) {
                    float* q = lds + p * pitch + c;
                    q[0] = s[0]; q[1] = s[1]; q[2] = s[2]; q[3] = s[3];
                }
            }
            *reinterpret_cast<f32x4*>(o) = s;
        }
    } else {
        for (int f = threadIdx.x; f < rows * C; f += CE_CHUNK) {
            const int p = f / C, c = f - p * C;
            const int fl = s_fl[p];
            float s = lg[(size_t)p * ld + c];
            float* o = out + (size_t)s_pix[p] * C + c;
            if (!(fl & WIN_FIRST)) s = *o + s;
            if (fl & WIN_LAST) {
                s = __fdiv_rn(s, (float)s_cnt[p]);
                if (pred) lds[p * pitch + c] = s;
            }
            *o = s;
        }
    }
    if (!pred) return;                                        // uniform
    __syncthreads();
    if ((int)threadIdx.x < rows && (s_fl[threadIdx.x] & WIN_LAST)) {
        const float* p = lds + threadIdx.x * pitch;
        float best = p[0];
        int bi = 0;
        for (int c = 1; c < C; ++c) {
            const float v = p[c];
            if (v > best || (v != v && best == best)) { best = v; bi = c; }       // k_argmax's rule on the stored values
        }
        pred[s_pix[threadIdx.x]] = bi;
    }
}

}  // namespace

template <bool IDENT>
static bool tta_launch(int CP, int nb, size_t lds_bytes, hipStream_t s, const float* logits, int ld, int h, int w, float* acc, int64_t* pred,
                       int H, int W, int M, int C, int flip, int first, int last, float inv_k) {
#define TTA_CASE(cp)                                                                                                              \
    case cp:                                                                                                                      \
        hipLaunchKernelGGL((k_tta_accumulate<cp, IDENT>), dim3(nb), dim3(CE_CHUNK), lds_bytes, s, logits, ld, h, w, acc, pred, H, W, M, C, \
                           flip, first, last, inv_k);                                                                             \
        return true;
    switch (CP) {
        TTA_CASE(4) TTA_CASE(8) TTA_CASE(12) TTA_CASE(16) TTA_CASE(20) TTA_CASE(24) TTA_CASE(28) TTA_CASE(32)
    }
#undef TTA_CASE
    return false;
}

extern "C" int cvk_tta_accumulate(const float* logits, int ld, int h, int w, float* acc, int64_t* pred, int N, int H, int W, int C,
                                  int flip, int first, int last, float inv_k, void* stream) {
    CVK_CHECK_ARG(logits && acc && (pred || !last), "cvk_tta_accumulate: null pointer");
    CVK_CHECK_ARG(C <= TTA_MAX_C, "cvk_tta_accumulate: %d classes, the kernel holds at most %d per pixel in registers", C, TTA_MAX_C);
    CVK_CHECK_ARG(N > 0 && H > 0 && W > 0 && h > 0 && w > 0 && C > 0 && ld >= C && H <= TTA_MAX_DIM && W <= TTA_MAX_DIM &&
                      h <= TTA_MAX_DIM && w <= TTA_MAX_DIM && inv_k > 0.f && inv_k <= 3.0e38f,
                  "cvk_tta_accumulate: bad arguments");
    CVK_CHECK_ARG((int64_t)N * H * W * C < 2147483647LL - CE_CHUNK * TTA_MAX_C, "cvk_tta_accumulate: accumulator of 2^31 values or more");
    const int M = N * H * W, nb = cvk_cdiv(M, CE_CHUNK), CP = (C + 3) / 4 * 4;
    const size_t lds_bytes = (size_t)CE_CHUNK * (C + 1) * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    const bool ok = h == H && w == W
                        ? tta_launch<true>(CP, nb, lds_bytes, s, logits, ld, h, w, acc, pred, H, W, M, C, flip, first, last, inv_k)
                        : tta_launch<false>(CP, nb, lds_bytes, s, logits, ld, h, w, acc, pred, H, W, M, C, flip, first, last, inv_k);
    CVK_CHECK_ARG(ok, "cvk_tta_accumulate: no kernel for %d classes", C);
    CVK_LAUNCH_RETURN("cvk_tta_accumulate");
}

extern "C" int cvk_tta_resize_input(const float* src, int64_t sN, int64_t sC, int64_t sH, int64_t sW, float* dst, int N, int H, int W,
                                    int h, int w, int flip, void* stream) {
    CVK_CHECK_ARG(src && dst, "cvk_tta_resize_input: null pointer");
    CVK_CHECK_ARG(N > 0 && H > 0 && W > 0 && h > 0 && w > 0 && H <= TTA_MAX_DIM && W <= TTA_MAX_DIM && h <= TTA_MAX_DIM && w <= TTA_MAX_DIM &&
                      cvk_aligned16(dst),
                  "cvk_tta_resize_input: bad arguments");
    CVK_CHECK_ARG(N <= 65535, "cvk_tta_resize_input: grid too large");
    hipLaunchKernelGGL(k_tta_resize_input, dim3(cvk_cdiv(w, 256), h, N), dim3(256), 0, (hipStream_t)stream, src, sN, sC, sH, sW, dst, H, W,
                       h, w, flip);
    CVK_LAUNCH_RETURN("cvk_tta_resize_input");
}

extern "C" int cvk_window_merge(const float* logits, int ld, float* out, int64_t* pred, int N, int H, int W, int C, int hc, int wc,
                                int sy, int sx, int iy, int ix, void* stream) {
    CVK_CHECK_ARG(logits && out, "cvk_window_merge: null pointer");
    CVK_CHECK_ARG(C <= TTA_MAX_C, "cvk_window_merge: %d classes, the kernel serves at most %d", C, TTA_MAX_C);
    CVK_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && ld >= C && hc > 0 && wc > 0 && H <= TTA_MAX_DIM && W <= TTA_MAX_DIM &&
                      hc <= TTA_MAX_DIM && wc <= TTA_MAX_DIM,
                  "cvk_window_merge: bad arguments");
    CVK_CHECK_ARG(sy >= 1 && sy <= hc && sx >= 1 && sx <= wc, "cvk_window_merge: stride (%d, %d) outside 1..crop (%d, %d)", sy, sx, hc, wc);
    CVK_CHECK_ARG((int64_t)N * H * W * C < 2147483647LL, "cvk_window_merge: output of 2^31 values or more");
    WinGrid g;
    g.H = H; g.W = W; g.sy = sy; g.sx = sx; g.iy = iy; g.ix = ix;
    g.hw = hc < H ? hc : H;
    g.ww = wc < W ? wc : W;
    g.gy = (H - g.hw + sy - 1) / sy + 1;
    g.gx = (W - g.ww + sx - 1) / sx + 1;
    CVK_CHECK_ARG(iy >= 0 && iy < g.gy && ix >= 0 && ix < g.gx, "cvk_window_merge: window (%d, %d) outside the %d x %d grid", iy, ix, g.gy,
                  g.gx);
    g.y1 = iy * sy < H - g.hw ? iy * sy : H - g.hw;
    g.x1 = ix * sx < W - g.ww ? ix * sx : W - g.ww;
    const int M = N * g.hw * g.ww;
    const size_t lds_bytes = pred ? (size_t)CE_CHUNK * (C + 1) * sizeof(float) : 0;
    hipLaunchKernelGGL(k_window_merge, dim3(cvk_cdiv(M, CE_CHUNK)), dim3(CE_CHUNK), lds_bytes, (hipStream_t)stream, logits, ld, out, pred, M, C,
                       g);
    CVK_LAUNCH_RETURN("cvk_window_merge");
}
