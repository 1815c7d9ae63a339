#pragma once
// edt.h: exact Euclidean distance transform of a label batch.  The boundary loss takes phi from it; the surface-distance meter
// (surface_dist.h) shares its row search, its column walk's constants and its size checks.  loss_rows.h is included for
// k_lv_clear, which zeroes the presence words.
#include "cvk_common.h"
#include "loss_rows.h"

namespace {

// ---- exact Euclidean distance transform of a label batch (cvk_edt_squared / cvk_edt_signed; definitions in include/cvk.h) ------------
// A pixel's category is its class, or void (-1) when its label is ignore_index or outside [0, C).  Two passes, everything per image:
//   k_edt_cols  work-group = (image, 16 columns), their categories staged in LDS; thread = (column, channel), one walk down the column
//               and one up.  Channel c < C: the vertical distance to the nearest pixel of class c in the column; channel C: to the
//               nearest pixel of the column whose category differs from this pixel's (0xFFFF: none).  uint16 [N][H][W][C + 1].  ORs the
//               image's class-presence word (and its void flag) with an integer atomic.
//   k_edt_rows  work-group = one row (n, y): the row's column distances (transposed to [C + 1][W]) and categories sit in LDS; thread =
//               x, and per channel the outward search of edt_row_search: x - k and x + k for k = 0, 1, ... until k^2 >= best.  Every
//               x' with |x - x'| < k has been visited and every other one costs at least k^2, so the minimum is exact.  A class absent
//               from the image is skipped (-1).  For the distance to another category the column term of x' is channel C where x' has
//               this pixel's category and 0 elsewhere.  The integers of a 256-pixel tile are put in LDS in [x][c] order and stored as
//               contiguous words: int32 (SIGNED = false) or phi with sign and correctly rounded root applied (SIGNED = true).
// LDS of k_edt_cols: 16 H B (5.6 KiB at H = 360).  LDS of k_edt_rows: 2 W (C + 2) B of rows + 1 KiB x (C | 1) of output tile (12.6 + 13 KiB at W = 480, C = 12); a row that would not
// fit 64 KiB keeps only the categories (2 W B) in LDS and searches the column distances in global memory.
constexpr int EDT_MAX_C = 32;
constexpr int EDT_MAX_H = 65534;                   // a vertical distance is at most H - 1 < 0xFFFF
constexpr unsigned EDT_NONE = 0xFFFFu;
constexpr unsigned EDT_INF = 0xFFFFFFFFu;
constexpr int EDT_MAX_D2 = 1 << 24;                // (H - 1)^2 + (W - 1)^2 below this: every squared distance converts to fp32 exactly
constexpr size_t EDT_LDS_LIMIT = 64 * 1024;

__host__ __device__ __forceinline__ int edt_category(long t, int C, int ignore_index) {
    return t >= 0 && t < C && t != (long)ignore_index ? (int)t : -1;
}

// The correctly rounded fp32 root of an integer below 2^24 (exact in fp32).  sqrtf is IEEE-rounded in this build (no fast-math flag);
// __fsqrt_rn is not used: without OCML_BASIC_ROUNDED_OPERATIONS the toolchain defines it as the native approximation.
__device__ __forceinline__ float edt_root(int d2) { return __builtin_sqrtf((float)d2); }

// mask[2 n] = classes present in image n (bit c), mask[2 n + 1] = 1 when it has a void pixel; cleared before the launch.
// Work-group = (image, strip of EDT_COL_TX columns): the strip's categories, int8 [H][EDT_COL_TX] (H <= 4096: at most 64 KiB), are staged in
// LDS by all threads; then a thread owns one (column, channel) of the strip, channel fastest, and walks the column in LDS down and up;
// the map is stored on the way down and read back (its own stores) and lowered on the way up.
constexpr int EDT_COL_TX = 16, EDT_COL_BATCH = 8;

__global__ __launch_bounds__(256) void k_edt_cols(const int64_t* __restrict__ lab, unsigned short* __restrict__ col,
                                                 unsigned* __restrict__ mask, int strips, int H, int W, int C, int ignore_index) {
    extern __shared__ signed char edt_cat[];
    const int K = C + 1;
    const int n = blockIdx.x / strips, x0 = (blockIdx.x - n * strips) * EDT_COL_TX;
    const int64_t* L = lab + (size_t)n * H * W;
    for (int i = threadIdx.x; i < H * EDT_COL_TX; i += 256) {
        const int y = i / EDT_COL_TX, x = x0 + (i - y * EDT_COL_TX);
        edt_cat[i] = (signed char)(x < W ? edt_category((long)L[(size_t)y * W + x], C, ignore_index) : -1);
    }
    __syncthreads();
    const size_t os = (size_t)W * K;
    for (int item = threadIdx.x; item < EDT_COL_TX * K; item += 256) {
        const int xx = item / K, c = item - xx * K;
        if (x0 + xx >= W) continue;
        const signed char* s = edt_cat + xx;
        unsigned short* o = col + ((size_t)n * H * W + x0 + xx) * K + c;
        // Two walks with no data-dependent inner loop (lanes of a wave hold different classes): down, storing the distance to the nearest
        // match above; then up in batches of EDT_COL_BATCH rows, whose stored values are fetched together before they are lowered.
        if (c < C) {
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
            if (last >= 0) atomicOr(&mask[2 * n], 1u << c);
        } else {
            bool any_void = false;
            int prev = 0, start = 0;                       // the run of equal categories that holds y starts at `start`
            for (int y = 0; y < H; ++y) {
                const int k = s[y * EDT_COL_TX];
                any_void |= k < 0;
                if (y > 0 && k != prev) start = y;
                prev = k;
                o[y * os] = (unsigned short)(start > 0 ? (unsigned)(y - start + 1) : EDT_NONE);
            }
            int end = H - 1;                               // ... and ends at `end`
            for (int y1 = H; y1 > 0; y1 -= EDT_COL_BATCH) {
                unsigned v[EDT_COL_BATCH];
#pragma unroll
                for (int j = 0; j < EDT_COL_BATCH; ++j) v[j] = y1 - 1 - j >= 0 ? (unsigned)o[(y1 - 1 - j) * os] : 0u;
#pragma unroll
                for (int j = 0; j < EDT_COL_BATCH; ++j) {
                    const int y = y1 - 1 - j;
                    if (y < 0) break;
                    const int k = s[y * EDT_COL_TX];
                    if (y < H - 1 && k != prev) end = y;
                    prev = k;
                    if (end < H - 1 && (unsigned)(end + 1 - y) < v[j]) o[y * os] = (unsigned short)(end + 1 - y);
                }
            }
            if (any_void) atomicOr(&mask[2 * n + 1], 1u);
        }
    }
}

// min over x' of (x - x')^2 + g(x')^2, g(x') = col[x' * cstride] (0xFFFF: no such pixel in that column); OTHER: g(x') = 0 where
// cat[x'] != t.  -1 when no column has a finite term.  The one producer of the integers that both outputs are made of.
template <bool OTHER>
__device__ __forceinline__ int edt_row_search(const unsigned short* col, int cstride, const short* cat, int t, int x, int W) {
    unsigned best = EDT_INF;
    const int kmax = max(x, W - 1 - x);
    for (int k = 0; k <= kmax; ++k) {
        const unsigned k2 = (unsigned)k * (unsigned)k;
        if (k2 >= best) break;
        const int xl = x - k, xr = x + k;
        if (xl >= 0) {
            unsigned v = col[(size_t)xl * cstride];
            if (OTHER && cat[xl] != t) v = 0u;
            if (v != EDT_NONE) best = min(best, k2 + v * v);
        }
        if (k > 0 && xr < W) {
            unsigned v = col[(size_t)xr * cstride];
            if (OTHER && cat[xr] != t) v = 0u;
            if (v != EDT_NONE) best = min(best, k2 + v * v);
        }
    }
    return best == EDT_INF ? -1 : (int)best;
}

// grid N * H.  SIGNED: phi [M][C] floats; else to_class [M][C] and to_other [M] int32.
template <bool STAGED, bool SIGNED>
__global__ __launch_bounds__(256) void k_edt_rows(const int64_t* __restrict__ lab, const unsigned short* __restrict__ col,
                                                 const unsigned* __restrict__ mask, int* __restrict__ to_class,
                                                 int* __restrict__ to_other, float* __restrict__ phi, int H, int W, int C,
                                                 int ignore_index) {
    extern __shared__ unsigned char edt_lds[];
    const int K = C + 1, pitch = C | 1;
    const size_t row = blockIdx.x;
    const int n = (int)(row / H);
    short* s_cat = reinterpret_cast<short*>(edt_lds);
    unsigned short* s_col = reinterpret_cast<unsigned short*>(edt_lds) + W;                // [K][W], STAGED only
    const size_t rows_bytes = ((size_t)2 * W * (STAGED ? K + 1 : 1) + 3) & ~(size_t)3;
    int* s_out = reinterpret_cast<int*>(edt_lds + rows_bytes);                             // [256][pitch]
    const unsigned short* g = col + row * W * K;
    for (int x = threadIdx.x; x < W; x += 256) s_cat[x] = (short)edt_category((long)lab[row * W + x], C, ignore_index);
    if (STAGED)
        for (int i = threadIdx.x; i < W * K; i += 256) {
            const int x = i / K, c = i - x * K;
            s_col[c * W + x] = g[i];
        }
    const unsigned present = mask[2 * n];
    const bool several = __popc(present) + (int)(mask[2 * n + 1] & 1u) > 1;
    __syncthreads();
    for (int x0 = 0; x0 < W; x0 += 256) {
        const int x = x0 + threadIdx.x;
        int other = -1;
        if (x < W) {
            const int t = s_cat[x];
            if (several)
                other = STAGED ? edt_row_search<true>(s_col + C * W, 1, s_cat, t, x, W) : edt_row_search<true>(g + C, K, s_cat, t, x, W);
            for (int c = 0; c < C; ++c) {
                int d = -1;
                if (((present >> c) & 1u) && !(SIGNED && c == t))
                    d = STAGED ? edt_row_search<false>(s_col + c * W, 1, s_cat, t, x, W) : edt_row_search<false>(g + c, K, s_cat, t, x, W);
                if (SIGNED) {
                    float v;
                    if (c == t) v = other < 0 ? 0.f : -(edt_root(other) - 1.f);
                    else        v = d < 0 ? 0.f : edt_root(d);
                    s_out[threadIdx.x * pitch + c] = __builtin_bit_cast(int, v);
                } else {
                    s_out[threadIdx.x * pitch + c] = d;
                }
            }
            if (!SIGNED) to_other[row * W + x] = other;
        }
        __syncthreads();
        const int words = min(256, W - x0) * C;
        int* dst = (SIGNED ? reinterpret_cast<int*>(phi) : to_class) + (row * W + x0) * C;
        for (int j = threadIdx.x; j < words; j += 256) {
            const int px = j / C;
            dst[j] = s_out[px * pitch + (j - px * C)];
        }
        __syncthreads();
    }
}

}  // namespace

static size_t edt_cols_bytes(int N, int H, int W, int C) { return ((size_t)2 * N * H * W * (C + 1) + 15) & ~(size_t)15; }

static int edt_check_sizes(const char* who, int N, int H, int W, int C) {
    CVK_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: sizes must be positive, got N %d, H %d, W %d", who, N, H, W);
    CVK_CHECK_ARG(C >= 1 && C <= EDT_MAX_C, "%s: %d classes, the kernels serve 1 to %d", who, C, EDT_MAX_C);
    CVK_CHECK_ARG(H <= EDT_MAX_H, "%s: H %d, a column distance is 16 bits wide (H <= %d)", who, H, EDT_MAX_H);
    CVK_CHECK_ARG((int64_t)(H - 1) * (H - 1) + (int64_t)(W - 1) * (W - 1) < EDT_MAX_D2,
                  "%s: image too large, (H - 1)^2 + (W - 1)^2 must stay below 2^24 for exact fp32 roots, got H %d, W %d", who, H, W);
    CVK_CHECK_ARG((int64_t)N * H * W < 2147483648LL, "%s: 2^31 pixels or more", who);
    return CVK_OK;
}

extern "C" int64_t cvk_edt_workspace_bytes(int N, int H, int W, int C) {
    if (N <= 0 || H <= 0 || W <= 0 || C < 1 || C > EDT_MAX_C || H > EDT_MAX_H || (int64_t)N * H * W >= 2147483648LL ||
        (int64_t)(H - 1) * (H - 1) + (int64_t)(W - 1) * (W - 1) >= EDT_MAX_D2)
        return 0;
    return (int64_t)(edt_cols_bytes(N, H, W, C) + 16 * (((size_t)8 * N + 15) / 16));
}

template <bool SIGNED>
static void edt_launch(const int64_t* labels, int N, int H, int W, int C, int ignore_index, void* workspace, int* to_class, int* to_other,
                       float* phi, hipStream_t s) {
    unsigned short* col = static_cast<unsigned short*>(workspace);
    unsigned* mask = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + edt_cols_bytes(N, H, W, C));
    const int K = C + 1;
    hipLaunchKernelGGL(k_lv_clear, dim3(cvk_cdiv(2 * (long)N, 256)), dim3(256), 0, s, mask, 2 * N);
    const int strips = cvk_cdiv(W, EDT_COL_TX);
    hipLaunchKernelGGL(k_edt_cols, dim3((unsigned)N * strips), dim3(256), (size_t)H * EDT_COL_TX, s, labels, col, mask, strips, H, W, C,
                       ignore_index);
    const size_t tile = (size_t)4 * 256 * (C | 1);
    const size_t staged = (((size_t)2 * W * (K + 1) + 3) & ~(size_t)3) + tile, unstaged = (((size_t)2 * W + 3) & ~(size_t)3) + tile;
    if (staged <= EDT_LDS_LIMIT)
        hipLaunchKernelGGL((k_edt_rows<true, SIGNED>), dim3((unsigned)N * H), dim3(256), staged, s, labels, col, mask, to_class, to_other,
                           phi, H, W, C, ignore_index);
    else
        hipLaunchKernelGGL((k_edt_rows<false, SIGNED>), dim3((unsigned)N * H), dim3(256), unstaged, s, labels, col, mask, to_class,
                           to_other, phi, H, W, C, ignore_index);
}

extern "C" int cvk_edt_squared(const int64_t* labels, int N, int H, int W, int num_classes, int ignore_index, void* workspace,
                               int32_t* to_class, int32_t* to_other, void* stream) {
    CVK_CHECK_ARG(labels && workspace && to_class && to_other, "cvk_edt_squared: null pointer");
    const int rc = edt_check_sizes("cvk_edt_squared", N, H, W, num_classes);
    if (rc != CVK_OK) return rc;
    CVK_CHECK_ARG(((uintptr_t)workspace & 15u) == 0, "cvk_edt_squared: the workspace must be 16-byte aligned");
    edt_launch<false>(labels, N, H, W, num_classes, ignore_index, workspace, to_class, to_other, nullptr, (hipStream_t)stream);
    CVK_LAUNCH_RETURN("cvk_edt_squared");
}

extern "C" int cvk_edt_signed(const int64_t* labels, int N, int H, int W, int num_classes, int ignore_index, void* workspace, float* phi,
                              void* stream) {
    CVK_CHECK_ARG(labels && workspace && phi, "cvk_edt_signed: null pointer");
    const int rc = edt_check_sizes("cvk_edt_signed", N, H, W, num_classes);
    if (rc != CVK_OK) return rc;
    CVK_CHECK_ARG(((uintptr_t)workspace & 15u) == 0, "cvk_edt_signed: the workspace must be 16-byte aligned");
    edt_launch<true>(labels, N, H, W, num_classes, ignore_index, workspace, nullptr, nullptr, phi, (hipStream_t)stream);
    CVK_LAUNCH_RETURN("cvk_edt_signed");
}
