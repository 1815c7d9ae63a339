#pragma once
// grad_flat.h: passes over the flat gradient buffer's segment table.  Global-norm clipping (cvk_grad_norm, cvk_grad_scale,
// cvk_clip_coef) and accumulation over micro-batches (cvk_grad_accumulate).  The segment planner is optim_flat.h's plan_block0.
#include "cvk_common.h"
#include "optim_flat.h"

namespace {

// ---- global-norm gradient clipping (cvk_grad_norm, cvk_grad_scale) -----------------------------------------------------------------
// torch.nn.utils.clip_grad_norm_'s coefficient in fp32: clamp(max_norm / (total_norm + 1e-6), max=1).  `c > 1 ? 1 : c` keeps a NaN
// (fminf would return 1).  One expression for the host entry point and the finish kernel (IEEE division on both sides).
__host__ __device__ __forceinline__ float clip_coef_f32(float max_norm, float total_norm) {
    const float c = max_norm / (total_norm + 1e-6f);
    return c > 1.f ? 1.f : c;
}

constexpr int NORM_THREADS = 256;
constexpr int NORM_UNROLL = 4;                  // independent 16-byte loads per lane and trip
constexpr int NORM_MAX_BLOCKS = 2048;           // 8 workgroups per CU: a grid-stride streaming read

// The workgroup's segment (uniform binary search over block0, as k_adamw_ranges) and its place among the segment's workgroups.
// False when the table entry is unusable (cvk_grad_norm_plan refuses such a table on the host).
__device__ __forceinline__ bool norm_segment_of(const cvk_norm_segment* __restrict__ st, int ns, int64_t n, int64_t* off, int64_t* len,
                                                int* rank, int* nb) {
    const int b = blockIdx.x;
    int lo = 0, hi = ns - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (st[mid].block0 <= b) lo = mid;
        else hi = mid - 1;
    }
    *off = st[lo].offset;
    *len = st[lo].length;
    const int b0 = st[lo].block0;
    *nb = (lo + 1 < ns ? st[lo + 1].block0 : (int)gridDim.x) - b0;
    *rank = b - b0;
    return *off >= 0 && *len > 0 && *off + *len <= n && *nb > 0 && b >= b0;
}

// A segment as [head scalars][16-byte vectors][tail scalars]: head = the elements before the first 16-byte boundary of g + off.
__device__ __forceinline__ int64_t norm_head(const float* g, int64_t off, int64_t len) {
    const int64_t h = (4 - (int64_t)((reinterpret_cast<uintptr_t>(g + off) >> 2) & 3)) & 3;
    return h < len ? h : len;
}

// NaN-keeping maximum: once m is a NaN it stays one (torch.linalg.vector_norm(inf) of a buffer with a NaN is NaN).
__device__ __forceinline__ double norm_max(double m, double x) { return (x > m || x != x) ? x : m; }

template <bool INF>
__device__ __forceinline__ double norm_acc(double a, float x) {
    const double d = (double)x;
    return INF ? norm_max(a, fabs(d)) : fma(d, d, a);
}

template <bool INF>
__device__ __forceinline__ double norm_join(double a, double b) { return INF ? norm_max(a, b) : a + b; }

// A fixed tree: xor-shuffles inside each wave, then the 4 wave results in order.  Every thread of the workgroup calls it.
template <bool INF>
__device__ __forceinline__ double norm_block_reduce(double a, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = norm_join<INF>(a, __shfl_xor(a, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    return norm_join<INF>(norm_join<INF>(red[0], red[1]), norm_join<INF>(red[2], red[3]));
}

template <bool INF>
__global__ __launch_bounds__(NORM_THREADS) void k_grad_norm_partial(const float* __restrict__ g, int64_t n,
                                                                    const cvk_norm_segment* __restrict__ st, int ns,
                                                                    double* __restrict__ partials) {
    __shared__ double red[NORM_THREADS / 64];
    int64_t off, len;
    int rank, nb;
    const bool ok = norm_segment_of(st, ns, n, &off, &len, &rank, &nb);      // uniform
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (ok) {
        const int64_t head = norm_head(g, off, len);
        const int64_t nvec = (len - head) >> 2;
        const f32x4* __restrict__ gv = reinterpret_cast<const f32x4*>(g + off + head);
        const int64_t tid = (int64_t)rank * NORM_THREADS + threadIdx.x, stride = (int64_t)nb * NORM_THREADS;
        int64_t i = tid;
        for (; i + (NORM_UNROLL - 1) * stride < nvec; i += NORM_UNROLL * stride) {
            f32x4 x[NORM_UNROLL];
#pragma unroll
            for (int u = 0; u < NORM_UNROLL; ++u) x[u] = gv[i + u * stride];
#pragma unroll
            for (int u = 0; u < NORM_UNROLL; ++u) {
                a0 = norm_acc<INF>(a0, x[u][0]);
                a1 = norm_acc<INF>(a1, x[u][1]);
                a2 = norm_acc<INF>(a2, x[u][2]);
                a3 = norm_acc<INF>(a3, x[u][3]);
            }
        }
        for (; i < nvec; i += stride) {
            const f32x4 x = gv[i];
            a0 = norm_acc<INF>(a0, x[0]);
            a1 = norm_acc<INF>(a1, x[1]);
            a2 = norm_acc<INF>(a2, x[2]);
            a3 = norm_acc<INF>(a3, x[3]);
        }
        // the at most 3 + 3 elements around the vectors: the segment's first thread
        if (tid == 0) {
            for (int64_t j = 0; j < head; ++j) a0 = norm_acc<INF>(a0, g[off + j]);
            for (int64_t j = head + 4 * nvec; j < len; ++j) a0 = norm_acc<INF>(a0, g[off + j]);
        }
    }
    const double a = norm_join<INF>(norm_join<INF>(a0, a1), norm_join<INF>(a2, a3));
    const double r = norm_block_reduce<INF>(a, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = r;                 // every workgroup writes its slot: the finish reads all of them
}

// One workgroup: thread t joins partials t, t + 256, ... in order, then the fixed tree; thread 0 writes {total_norm, clip_coef}.
template <bool INF>
__global__ __launch_bounds__(NORM_THREADS) void k_grad_norm_finish(const double* __restrict__ partials, int nblocks, float max_norm,
                                                                   float* __restrict__ rec) {
    __shared__ double red[NORM_THREADS / 64];
    double a = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += NORM_THREADS) a = norm_join<INF>(a, partials[i]);
    const double r = norm_block_reduce<INF>(a, red);
    if (threadIdx.x == 0) {
        const float total = INF ? (float)r : (float)sqrt(r);
        rec[0] = total;
        rec[1] = clip_coef_f32(max_norm, total);
    }
}

// grad[i] *= clip_coef over the segment table (cvk_grad_scale).  A coefficient of exactly 1 leaves the buffer untouched.
__global__ __launch_bounds__(NORM_THREADS) void k_grad_scale(float* __restrict__ g, int64_t n, const cvk_norm_segment* __restrict__ st,
                                                             int ns, const float* __restrict__ rec) {
    const float coef = rec[1];
    if (coef == 1.f) return;
    int64_t off, len;
    int rank, nb;
    if (!norm_segment_of(st, ns, n, &off, &len, &rank, &nb)) return;
    const int64_t head = norm_head(g, off, len);
    const int64_t nvec = (len - head) >> 2;
    f32x4* __restrict__ gv = reinterpret_cast<f32x4*>(g + off + head);
    const int64_t tid = (int64_t)rank * NORM_THREADS + threadIdx.x, stride = (int64_t)nb * NORM_THREADS;
    for (int64_t i = tid; i < nvec; i += stride) {
        f32x4 x = gv[i];
        x[0] *= coef; x[1] *= coef; x[2] *= coef; x[3] *= coef;
        gv[i] = x;
    }
    if (tid == 0) {
        for (int64_t j = 0; j < head; ++j) g[off + j] *= coef;
        for (int64_t j = head + 4 * nvec; j < len; ++j) g[off + j] *= coef;
    }
}

// ---- gradient accumulation over micro-batches (cvk_grad_accumulate) ----------------------------------------------------------------
// One element of the fold.  MODE 0: dst = src; 1: dst = dst + src; 2: dst = (dst + src) * scale.  One correctly rounded fp32 add, then
// (mode 2) one separately rounded multiply: an add feeding a multiply has no fused form, and the file is built without fast-math, so
// the result is bitwise `(d + s) * scale` of IEEE fp32 whatever the vector width.
template <int MODE>
__device__ __forceinline__ float acc_one(float d, float s, float scale) {
    if (MODE == 0) return s;
    if (MODE == 1) return d + s;
    return (d + s) * scale;
}

// dst and src share the table (same offsets in both buffers) and both bases are 16-byte aligned (checked by the entry point), so the
// head / vector / tail split of a segment is the same on both sides.  Elements outside the table are neither read nor written.
template <int MODE>
__global__ __launch_bounds__(NORM_THREADS) void k_grad_accumulate(float* __restrict__ dst, const float* __restrict__ src, int64_t n,
                                                                  const cvk_norm_segment* __restrict__ st, int ns, float scale) {
    int64_t off, len;
    int rank, nb;
    if (!norm_segment_of(st, ns, n, &off, &len, &rank, &nb)) return;
    const int64_t head = norm_head(dst, off, len);
    const int64_t nvec = (len - head) >> 2;
    f32x4* __restrict__ dv = reinterpret_cast<f32x4*>(dst + off + head);
    const f32x4* __restrict__ sv = reinterpret_cast<const f32x4*>(src + off + head);
    const int64_t tid = (int64_t)rank * NORM_THREADS + threadIdx.x, stride = (int64_t)nb * NORM_THREADS;
    int64_t i = tid;
    for (; i + (NORM_UNROLL - 1) * stride < nvec; i += NORM_UNROLL * stride) {
        f32x4 s[NORM_UNROLL], d[NORM_UNROLL];
#pragma unroll
        for (int u = 0; u < NORM_UNROLL; ++u) {
            s[u] = sv[i + u * stride];
            if (MODE != 0) d[u] = dv[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < NORM_UNROLL; ++u) {
            f32x4 r;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = acc_one<MODE>(MODE != 0 ? d[u][k] : 0.f, s[u][k], scale);
            dv[i + u * stride] = r;
        }
    }
    for (; i < nvec; i += stride) {
        const f32x4 s = sv[i];
        f32x4 r;
        if (MODE != 0) r = dv[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = acc_one<MODE>(MODE != 0 ? r[k] : 0.f, s[k], scale);
        dv[i] = r;
    }
    if (tid == 0) {         // the at most 3 + 3 elements around the vectors: the segment's first thread
        for (int64_t j = 0; j < head; ++j) dst[off + j] = acc_one<MODE>(MODE != 0 ? dst[off + j] : 0.f, src[off + j], scale);
        for (int64_t j = head + 4 * nvec; j < len; ++j) dst[off + j] = acc_one<MODE>(MODE != 0 ? dst[off + j] : 0.f, src[off + j], scale);
    }
}

}  // namespace

extern "C" float cvk_clip_coef(float max_norm, float total_norm) { return clip_coef_f32(max_norm, total_norm); }

// Workgroups per segment: one per NORM_THREADS * NORM_UNROLL 16-byte vectors, at most NORM_MAX_BLOCKS in all.
extern "C" int cvk_grad_norm_plan(cvk_norm_segment* segments, int nsegments, int64_t n) {
    CVK_CHECK_ARG(segments, "cvk_grad_norm_plan: null pointer");
    CVK_CHECK_ARG(nsegments > 0 && n > 0, "cvk_grad_norm_plan: empty table or buffer (%d segments, %lld elements)", nsegments, (long long)n);
    int64_t total = 0;
    for (int r = 0; r < nsegments; ++r) {
        const cvk_norm_segment& e = segments[r];
        CVK_CHECK_ARG(e.offset >= 0 && e.length > 0 && e.length <= n && e.offset <= n - e.length, "cvk_grad_norm_plan: segment %d [%lld, "
                      "+%lld) outside the buffer of %lld elements", r, (long long)e.offset, (long long)e.length, (long long)n);
        total += e.length;
    }
    const int64_t blocks = plan_block0(segments, nsegments, total, (int64_t)NORM_THREADS * NORM_UNROLL * 4, NORM_MAX_BLOCKS);
    CVK_CHECK_ARG(blocks >= 0, "cvk_grad_norm_plan: too many workgroups");
    return (int)blocks;
}

extern "C" int cvk_grad_norm(const float* grad, int64_t n, const cvk_norm_segment* segments, int nsegments, int nblocks, float norm_type,
                             float max_norm, double* partials, float* record, void* stream) {
    CVK_CHECK_ARG(grad && segments && partials && record, "cvk_grad_norm: null pointer");
    CVK_CHECK_ARG(n > 0 && nsegments > 0 && nblocks >= nsegments, "cvk_grad_norm: empty table or buffer (%d segments, %d workgroups)",
                  nsegments, nblocks);
    const bool inf = norm_type == __builtin_inff();
    CVK_CHECK_ARG(inf || norm_type == 2.f, "cvk_grad_norm: norm_type %g (2 and infinity are implemented)", (double)norm_type);
    CVK_CHECK_ARG(max_norm >= 0.f, "cvk_grad_norm: max_norm %g is negative or not a number", (double)max_norm);
    CVK_CHECK_ARG((((uintptr_t)grad) & 3u) == 0 && (((uintptr_t)partials) & 7u) == 0, "cvk_grad_norm: misaligned buffer");
    if (inf) {
        hipLaunchKernelGGL(k_grad_norm_partial<true>, dim3(nblocks), dim3(NORM_THREADS), 0, (hipStream_t)stream, grad, n, segments, nsegments,
                           partials);
        hipLaunchKernelGGL(k_grad_norm_finish<true>, dim3(1), dim3(NORM_THREADS), 0, (hipStream_t)stream, (const double*)partials, nblocks,
                           max_norm, record);
    } else {
        hipLaunchKernelGGL(k_grad_norm_partial<false>, dim3(nblocks), dim3(NORM_THREADS), 0, (hipStream_t)stream, grad, n, segments, nsegments,
                           partials);
        hipLaunchKernelGGL(k_grad_norm_finish<false>, dim3(1), dim3(NORM_THREADS), 0, (hipStream_t)stream, (const double*)partials, nblocks,
                           max_norm, record);
    }
    CVK_LAUNCH_RETURN("cvk_grad_norm");
}

extern "C" int cvk_grad_scale(float* grad, int64_t n, const cvk_norm_segment* segments, int nsegments, int nblocks, const float* record,
                              void* stream) {
    CVK_CHECK_ARG(grad && segments && record, "cvk_grad_scale: null pointer");
    CVK_CHECK_ARG(n > 0 && nsegments > 0 && nblocks >= nsegments, "cvk_grad_scale: empty table or buffer (%d segments, %d workgroups)",
                  nsegments, nblocks);
    CVK_CHECK_ARG((((uintptr_t)grad) & 3u) == 0, "cvk_grad_scale: misaligned buffer");
    hipLaunchKernelGGL(k_grad_scale, dim3(nblocks), dim3(NORM_THREADS), 0, (hipStream_t)stream, grad, n, segments, nsegments, record);
    CVK_LAUNCH_RETURN("cvk_grad_scale");
}

extern "C" int cvk_grad_accumulate(float* dst, const float* src, int64_t n, const cvk_norm_segment* segments, int nsegments, int nblocks,
                                   int mode, float scale, void* stream) {
    CVK_CHECK_ARG(dst && src && segments, "cvk_grad_accumulate: null pointer");
    CVK_CHECK_ARG(dst != src, "cvk_grad_accumulate: dst and src are the same buffer");
    CVK_CHECK_ARG(n > 0 && nsegments > 0 && nblocks >= nsegments, "cvk_grad_accumulate: empty table or buffer (%d segments, %d workgroups)",
                  nsegments, nblocks);
    CVK_CHECK_ARG(mode >= 0 && mode <= 2, "cvk_grad_accumulate: mode %d (0: copy, 1: add, 2: add and scale)", mode);
    CVK_CHECK_ARG(scale - scale == 0.f, "cvk_grad_accumulate: scale %g is not finite", (double)scale);
    CVK_CHECK_ARG((((uintptr_t)dst) & 15u) == 0 && (((uintptr_t)src) & 15u) == 0,
                  "cvk_grad_accumulate: misaligned buffer (both bases must be 16-byte aligned)");
    const dim3 grid(nblocks), block(NORM_THREADS);
    if (mode == 0)
        hipLaunchKernelGGL(k_grad_accumulate<0>, grid, block, 0, (hipStream_t)stream, dst, src, n, segments, nsegments, scale);
    else if (mode == 1)
        hipLaunchKernelGGL(k_grad_accumulate<1>, grid, block, 0, (hipStream_t)stream, dst, src, n, segments, nsegments, scale);
    else
        hipLaunchKernelGGL(k_grad_accumulate<2>, grid, block, 0, (hipStream_t)stream, dst, src, n, segments, nsegments, scale);
    CVK_LAUNCH_RETURN("cvk_grad_accumulate");
}
