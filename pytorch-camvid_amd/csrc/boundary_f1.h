#pragma once
// boundary_f1.h: the boundary F1 (BF) score's contour map and its matched / unmatched contour counts.  The surface-distance
// meter (surface_dist.h) shares the contour rule (k_boundary_map, BF_*).
#include "cvk_common.h"

namespace {

// ---- boundary F1: per-image, per-class contour counts (cvk_boundary_counts, cvk_boundary_map; the rule is in include/cvk.h) ----------
// A pixel of a map becomes one byte: its class (< BF_MAX_K), BF_OTHER for a non-void value that is no class (outside [0, K), or
// ignore_index predicted where the label is not void: different from every class, no boundary of its own), BF_VOID for a void pixel or
// a position outside the image (never different, no boundary).  Values are compared as 64-bit integers before they become a byte, so
// 2^32 + c is no class, and nothing is ever indexed by a value that is not a class.
constexpr int BF_MAX_K = 32, BF_MAX_R2 = 256, BF_MAX_R = 16;
constexpr int BF_TH = 32, BF_TW = 64, BF_THREADS = 256;  // interior tile of a workgroup: 2048 pixels, 8 per thread
constexpr int BF_STAGE_BATCH = 8;
constexpr unsigned char BF_OTHER = 254, BF_VOID = 255, BF_NONE = 255;

__device__ __forceinline__ unsigned char bf_code(int64_t x, int64_t void_src, int K, int ignore) {
    if (void_src == (int64_t)ignore) return BF_VOID;
    return (x >= 0 && x < K && x != (int64_t)ignore) ? (unsigned char)x : BF_OTHER;
}

// the boundary byte of a pixel with code v from its 4-neighbours' codes: v when v is a class and a non-void neighbour differs
__device__ __forceinline__ unsigned char bf_boundary(unsigned char v, unsigned char up, unsigned char down, unsigned char left,
                                                     unsigned char right) {
    if (v >= BF_MAX_K) return BF_NONE;
    const bool diff = (up != BF_VOID && up != v) || (down != BF_VOID && down != v) || (left != BF_VOID && left != v) ||
                      (right != BF_VOID && right != v);
    return diff ? v : BF_NONE;
}

// code of position (y, x) of image n, BF_VOID outside the image
__device__ __forceinline__ unsigned char bf_code_at(const int64_t* __restrict__ map, const int64_t* __restrict__ void_from, int n, int y,
                                                    int x, int H, int W, int K, int ignore) {
    if (y < 0 || y >= H || x < 0 || x >= W) return BF_VOID;
    const size_t i = ((size_t)n * H + y) * W + x;
    return bf_code(map[i], void_from[i], K, ignore);
}

__global__ __launch_bounds__(256) void k_boundary_map(const int64_t* __restrict__ map, const int64_t* __restrict__ void_from,
                                                     unsigned char* __restrict__ out, int N, int H, int W, int K, int ignore) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;     // the grid covers N * H * W < 2^31 with less than 256 to spare
    if (m < N * H * W) {
        const int x = m % W, r = m / W, y = r % H, n = r / H;
        const unsigned char v = bf_code(map[m], void_from[m], K, ignore);
        unsigned char b = BF_NONE;
        if (v < BF_MAX_K)
            b = bf_boundary(v, bf_code_at(map, void_from, n, y - 1, x, H, W, K, ignore), bf_code_at(map, void_from, n, y + 1, x, H, W, K, ignore),
                            bf_code_at(map, void_from, n, y, x - 1, H, W, K, ignore), bf_code_at(map, void_from, n, y, x + 1, H, W, K, ignore));
        out[m] = b;
    }
}

// 0x80 in every byte of v that is zero, exactly (no carry runs from one byte into the next)
__device__ __forceinline__ unsigned int bf_zero_bytes(unsigned int v) {
    return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu);
}

// whether columns [x0, x1] of a boundary row (4-byte aligned, pitch a multiple of 4) hold byte c: aligned 32-bit LDS reads, four
// positions per compare, the bytes of the first and last word outside the span masked off
__device__ __forceinline__ bool bf_row_has(const unsigned char* row, int x0, int x1, unsigned char c) {
    const unsigned int* w = reinterpret_cast<const unsigned int*>(row);
    const unsigned int pat = 0x01010101u * c;
    const int d0 = x0 >> 2, d1 = x1 >> 2;
    for (int d = d0; d <= d1; ++d) {
        unsigned int z = bf_zero_bytes(w[d] ^ pat);
        if (d == d0) z &= 0xFFFFFFFFu << (8 * (x0 & 3));
        if (d == d1) z &= 0xFFFFFFFFu >> (8 * (3 - (x1 & 3)));
        if (z) return true;
    }
    return false;
}

// rows of the disc are searched nearest first, in up to BF_LEVELS bands of |dy|: 0..2, 3..5, 6..10, 11..16
constexpr int BF_LEVELS = 4;
__device__ __forceinline__ int bf_level_end(int lvl) { return lvl == 0 ? 2 : lvl == 1 ? 5 : lvl == 2 ? 10 : BF_MAX_R; }

// One workgroup per BF_TH x BF_TW tile of one image (grid: tiles of an image x N, flattened).  With R = isqrt(r2):
//   1. the codes of both maps for the tile plus a halo of R + 1 go to LDS (the only global reads);
//   2. both boundary byte maps for the tile plus a halo of R are derived from them (bf_boundary, as k_boundary_map);
//   3. the interior pixels that carry a boundary are counted (rows 0 / 2) and queued;
//   4. the queue is served by all threads in turn: an entry searches the disc in the other map's boundary bytes row by row, nearest rows
//      first, four positions per LDS read (bf_row_has), and leaves at the first hit (rows 1 / 3).  Positions outside the image are
//      BF_NONE there, so an offset never leaves the image.  The rows come in bands; the entries a band leaves unmatched are queued again
//      for the next one, so that the few entries that walk the whole disc fill whole waves instead of holding 63 finished lanes each.
// Counters are 32-bit LDS atomics (at most 2048 per workgroup), flushed by 64-bit global atomics where non-zero: integer sums, exact in
// any order.  LDS bytes: 2 (BF_TH + 2R + 2)(BF_TW + 2R + 2) codes + 2 (BF_TH + 2R) pitch boundary bytes, pitch = BF_TW + 2R rounded up
// to 4 (cvk_boundary_counts sizes them), + two 8 KiB queues + tables: 29 KiB at R = 4, 42 KiB at R = 16.
__global__ __launch_bounds__(BF_THREADS) void k_boundary_counts(const int64_t* __restrict__ pred, const int64_t* __restrict__ label,
                                                               unsigned long long* __restrict__ counts, int H, int W, int K, int ignore,
                                                               int r2, int R, int tiles_x, int tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bf_lds[];
    __shared__ unsigned int s_cnt[4 * BF_MAX_K];
    __shared__ unsigned short s_queue[2][2 * BF_TH * BF_TW];  // entry: interior pixel index | map << 11 (0: prediction, 1: label)
    __shared__ int s_half[BF_MAX_R + 1];                      // s_half[|dy|] = isqrt(r2 - dy * dy)
    __shared__ unsigned int s_nq[BF_LEVELS + 1];              // entries queued for each band
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int ty0 = (t / tiles_x) * BF_TH, tx0 = (t % tiles_x) * BF_TW;
    const int CH = BF_TH + 2 * R + 2, CW = BF_TW + 2 * R + 2, BH = BF_TH + 2 * R, BW = BF_TW + 2 * R, BP = (BW + 3) & ~3;
    const int csize = (CH * CW + 3) & ~3;
    unsigned char* cP = bf_lds;
    unsigned char* cG = cP + csize;
    unsigned char* bP = cG + csize;                           // 4-byte aligned, as every row of pitch BP is
    unsigned char* bG = bP + BH * BP;
    const int tid = threadIdx.x;
    for (int i = tid; i < 4 * BF_MAX_K; i += BF_THREADS) s_cnt[i] = 0;
    if (tid <= BF_LEVELS) s_nq[tid] = 0;
    if (tid <= R) {
        const int rem = r2 - tid * tid;
        int w = 0;
        while ((w + 1) * (w + 1) <= rem) ++w;
        s_half[tid] = w;
    }
    // BF_STAGE_BATCH independent loads of each map are in flight per thread before the first is used (the loop is latency bound
    // otherwise); a position outside the image reads nothing and takes the label ignore, which is BF_VOID in both maps
    for (int base = 0; base < CH * CW; base += BF_THREADS * BF_STAGE_BATCH) {
        int64_t l[BF_STAGE_BATCH], p[BF_STAGE_BATCH];
#pragma unroll
        for (int u = 0; u < BF_STAGE_BATCH; ++u) {
            const int i = base + u * BF_THREADS + tid, cy = i / CW, cx = i - cy * CW;
            const int y = ty0 - R - 1 + cy, x = tx0 - R - 1 + cx;
            const bool in = i < CH * CW && y >= 0 && y < H && x >= 0 && x < W;
            const size_t m = ((size_t)n * H + y) * W + x;
            l[u] = in ? label[m] : (int64_t)ignore;
            p[u] = in ? pred[m] : (int64_t)ignore;
        }
#pragma unroll
        for (int u = 0; u < BF_STAGE_BATCH; ++u) {
            const int i = base + u * BF_THREADS + tid;
            if (i < CH * CW) {
                cP[i] = bf_code(p[u], l[u], K, ignore);
                cG[i] = bf_code(l[u], l[u], K, ignore);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < BH * BP; i += BF_THREADS) {
        const int by = i / BP, bx = i - by * BP;
        unsigned char p = BF_NONE, g = BF_NONE;               // the pitch's padding columns hold no boundary
        if (bx < BW) {
            const int c = (by + 1) * CW + bx + 1;
            p = bf_boundary(cP[c], cP[c - CW], cP[c + CW], cP[c - 1], cP[c + 1]);
            g = bf_boundary(cG[c], cG[c - CW], cG[c + CW], cG[c - 1], cG[c + 1]);
        }
        bP[i] = p;
        bG[i] = g;
    }
    __syncthreads();
    for (int i = tid; i < BF_TH * BF_TW; i += BF_THREADS) {
        const int b = ((i / BF_TW) + R) * BP + (i % BF_TW) + R;
        const unsigned char p = bP[b], g = bG[b];
        if (p != BF_NONE) {
            atomicAdd(&s_cnt[p], 1u);
            s_queue[0][atomicAdd(&s_nq[0], 1u)] = (unsigned short)i;
        }
        if (g != BF_NONE) {
            atomicAdd(&s_cnt[2 * K + g], 1u);
            s_queue[0][atomicAdd(&s_nq[0], 1u)] = (unsigned short)(i | (1 << 11));
        }
    }
    __syncthreads();
    for (int lvl = 0, a_lo = 0; lvl < BF_LEVELS; ++lvl) {     // uniform: every thread walks the same bands
        const int a_hi = min(R, bf_level_end(lvl));
        const bool more = a_hi < R;
        const int nq = (int)s_nq[lvl];
        const unsigned short* qin = s_queue[lvl & 1];
        unsigned short* qout = s_queue[(lvl + 1) & 1];
        for (int q = tid; q < nq; q += BF_THREADS) {
            const int e = qin[q], which = e >> 11, i = e & (BF_TH * BF_TW - 1);
            const int by = (i / BF_TW) + R, bx = (i % BF_TW) + R;
            const unsigned char c = (which ? bG : bP)[by * BP + bx];
            const unsigned char* other = which ? bP : bG;
            bool hit = false;
            for (int k = a_lo ? 2 * a_lo - 1 : 0; k <= 2 * a_hi && !hit; ++k) {
                const int a = (k + 1) >> 1, dy = (k & 1) ? -a : a, w = s_half[a];
                hit = bf_row_has(other + (by + dy) * BP, bx - w, bx + w, c);
            }
            if (hit) atomicAdd(&s_cnt[(which ? 3 : 1) * K + c], 1u);
            else if (more) qout[atomicAdd(&s_nq[lvl + 1], 1u)] = (unsigned short)e;
        }
        __syncthreads();
        if (!more || s_nq[lvl + 1] == 0) break;               // uniform: read after the barrier, written before it
        a_lo = a_hi + 1;
    }
    for (int i = tid; i < 4 * K; i += BF_THREADS)
        if (s_cnt[i]) atomicAdd(&counts[(size_t)n * 4 * K + i], (unsigned long long)s_cnt[i]);
}

}  // namespace

extern "C" int cvk_boundary_counts(const int64_t* pred, const int64_t* label, int64_t* counts, int N, int H, int W, int num_classes,
                                   int ignore_index, int r2, void* stream) {
    CVK_CHECK_ARG(pred && label && counts, "cvk_boundary_counts: null pointer");
    CVK_CHECK_ARG(num_classes >= 1 && num_classes <= BF_MAX_K, "cvk_boundary_counts: %d classes, the kernel serves 1 to %d", num_classes,
                  BF_MAX_K);
    CVK_CHECK_ARG(r2 >= 0 && r2 <= BF_MAX_R2, "cvk_boundary_counts: squared tolerance %d outside 0..%d (16 pixels)", r2, BF_MAX_R2);
    CVK_CHECK_ARG(N > 0 && H > 0 && W > 0, "cvk_boundary_counts: sizes must be positive, got N %d, H %d, W %d", N, H, W);
    CVK_CHECK_ARG((int64_t)N * H * W < 2147483648LL, "cvk_boundary_counts: 2^31 pixels or more");
    int R = 0;
    while ((R + 1) * (R + 1) <= r2) ++R;
    const int tiles_x = cvk_cdiv(W, BF_TW), tiles = tiles_x * cvk_cdiv(H, BF_TH);
    const size_t codes = ((size_t)(BF_TH + 2 * R + 2) * (BF_TW + 2 * R + 2) + 3) & ~(size_t)3;
    const size_t lds_bytes = 2 * codes + 2 * (size_t)(BF_TH + 2 * R) * ((BF_TW + 2 * R + 3) & ~3);
    hipLaunchKernelGGL(k_boundary_counts, dim3((unsigned)tiles * (unsigned)N), dim3(BF_THREADS), lds_bytes, (hipStream_t)stream, pred, label,
                       reinterpret_cast<unsigned long long*>(counts), H, W, num_classes, ignore_index, r2, R, tiles_x, tiles);
    CVK_LAUNCH_RETURN("cvk_boundary_counts");
}

extern "C" int cvk_boundary_map(const int64_t* map, const int64_t* void_from, uint8_t* out_u8, int N, int H, int W, int num_classes,
                                int ignore_index, void* stream) {
    CVK_CHECK_ARG(map && out_u8, "cvk_boundary_map: null pointer");
    CVK_CHECK_ARG(num_classes >= 1 && num_classes <= BF_MAX_K, "cvk_boundary_map: %d classes, the kernel serves 1 to %d", num_classes,
                  BF_MAX_K);
    CVK_CHECK_ARG(N > 0 && H > 0 && W > 0, "cvk_boundary_map: sizes must be positive, got N %d, H %d, W %d", N, H, W);
    CVK_CHECK_ARG((int64_t)N * H * W < 2147483648LL, "cvk_boundary_map: 2^31 pixels or more");
    hipLaunchKernelGGL(k_boundary_map, dim3(cvk_cdiv((long)N * H * W, 256)), dim3(256), 0, (hipStream_t)stream, map,
                       void_from ? void_from : map, out_u8, N, H, W, num_classes, ignore_index);
    CVK_LAUNCH_RETURN("cvk_boundary_map");
}
