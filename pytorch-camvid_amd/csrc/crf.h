#pragma once
// ---- local-window mean-field CRF refinement (cvk_crf_step, cvk_crf_tile; the definition is in include/cvk.h) -----------------------
// One launch = one mean-field iteration: a register-blocked 2-D stencil over a multi-channel tile, neither MFMA nor atomics.
//   k_crf_step<CP, NT, STAGED>   work-group = NT threads = a tile of TH = NT PX / CRF_TW rows x CRF_TW columns of one image; CP = C
//                 rounded up to a multiple of 4 is the compile-time register count per pixel, PX = 2 the pixels per thread (the two
//                 accumulators per class and pixel are 2 PX CP registers), NT = 192: a tile of 8 x 48 pixels, 51 KiB of LDS at 12 classes
//                 and halo 3, so three work-groups share a CU and one stages while the others compute.  Four pixels per thread on a
//                 16 x 48 tile were measured first: 81 KiB of LDS then meant 3 waves per CU, nothing to hide a tile's staging or its
//                 LDS latency behind, and 179 us per iteration at 8 x 12 x 360 x 480.
//   STAGED        the tile of Q and of the guide I with its halo h = r d lies in LDS: one thread per staged pixel loads the pixel's C
//                 values (on the first call: its unary, soft-maxed on the way, so no Q_0 pass exists) and its guide colour, converted to
//                 grey levels once.  Q is pixel-major, CP / 4 16-byte slots per pixel plus one slot of skew after every fourth pixel, so
//                 that the 16 lanes of a ds_read_b128 group, whose pixels lie 2 columns apart at d = 1 (6.5 slots at 12 classes), fall on different slots.
//   !STAGED       the same loop reads the neighbour's Q row and guide colour from global memory (r d up to 20 fits no useful tile);
//                 on the first call k_crf_q0 writes Q_0 = softmax(U) into the scratch buffer beforehand.
// Register blocking.  A thread owns PX pixels of one row, d columns apart (adjacent at d = 1): x_k = x_0 + k d.  For a row offset i it
// walks the columns x_0 + m d, m = -r .. PX - 1 + r, reads that neighbour's C values and colour ONCE and feeds every pixel k with
// j = m - k in -r .. r: PX + 2 r reads serve PX (2 r + 1) taps.  Per pixel k the taps arrive with i ascending and, inside a row,
// j = m - k ascending: the row-major order of the definition, whatever the tile, the path or the batch.  The weights are recomputed
// from the colours every time; nothing per (pixel, offset) is stored.
// The colour term uses v_exp_f32 (__expf): its argument cb |dI|^2 <= 0 is rounded once in the scaling by log2(e), a relative error of
// |x| 2^-24 in a weight e^x, at most 0.37 x 2^-24 of the largest weight.  The softmax uses expf, as k_tta_accumulate does.
// Bounds.  Staged reads lie inside the staged tile by construction (row trow + h + i d < TH + 2 h, column xl0 + h + m d <= CRF_TW - 1
// + 2 h); global reads and every write are guarded by the image size; a neighbour outside the image is skipped, not weighted by zero.
#include "cvk_common.h"
#include <float.h>

namespace {

constexpr int CRF_MAX_C = 32, CRF_MAX_R = 5, CRF_MAX_D = 4, CRF_MAX_DIM = 16384;
constexpr int CRF_TAPS = (2 * CRF_MAX_R + 1) * (2 * CRF_MAX_R + 1);
constexpr int CRF_PX = 2, CRF_TW = 48;                        // 48 / CRF_PX = 24 thread columns: a multiple of every d in 1..4
constexpr size_t CRF_LDS_CAP = 158 * 1024;                    // dynamic LDS of the staged path (the tap tables take 1 KiB more)

struct CrfArgs {
    const float* unary;
    const float* qin;
    float* qout;
    int64_t* pred;
    const void* guide;
    const float* compat;
    int64_t gN, gC, gH, gW;
    int ld_u, is_prob, guide_u8, N, H, W, C, r, d, first, last, tiles_x, tiles_y;
    float a[3], b[3], cb, wa, ws;
    float ga[CRF_TAPS], gs[CRF_TAPS];
};

__device__ __forceinline__ f32x4 crf_guide(const CrfArgs& A, int n, int y, int x) {
    f32x4 v;
    if (A.guide_u8) {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(A.guide) + (((size_t)n * A.H + y) * A.W + x) * 3;
        v[0] = (float)p[0]; v[1] = (float)p[1]; v[2] = (float)p[2];
    } else {
        const float* p = reinterpret_cast<const float*>(A.guide) + n * A.gN + y * A.gH + x * A.gW;
        v[0] = __fmaf_rn(A.a[0], p[0], A.b[0]);
        v[1] = __fmaf_rn(A.a[1], p[A.gC], A.b[1]);
        v[2] = __fmaf_rn(A.a[2], p[2 * A.gC], A.b[2]);
    }
    v[3] = 0.f;
    return v;
}

// a dense or padded row of C floats -> CP registers (pad registers 0)
template <int CP>
__device__ __forceinline__ void crf_load_row(const float* __restrict__ p, int C, bool vec, float (&v)[CP]) {
    if (vec) {                                                // uniform: C == CP, 16-byte aligned rows
#pragma unroll
        for (int j = 0; j < CP / 4; ++j) {
            const f32x4 a = reinterpret_cast<const f32x4*>(p)[j];
            v[4 * j] = a[0]; v[4 * j + 1] = a[1]; v[4 * j + 2] = a[2]; v[4 * j + 3] = a[3];
        }
    } else {
#pragma unroll
        for (int c = 0; c < CP; ++c) v[c] = c < C ? p[c] : 0.f;
    }
}

template <int CP>
__device__ __forceinline__ void crf_unary(const CrfArgs& A, size_t pix, float (&u)[CP]) {
    const bool vec = (A.C & 3) == 0 && (A.ld_u & 3) == 0 && ((uintptr_t)A.unary & 15u) == 0;
    crf_load_row<CP>(A.unary + pix * A.ld_u, A.C, vec, u);
    if (A.is_prob) {
#pragma unroll
        for (int c = 0; c < CP; ++c) u[c] = logf(fmaxf(u[c], FLT_MIN));
    }
}

// max-subtracted softmax of v[0..C), in place; pad registers become 0
template <int CP>
__device__ __forceinline__ void crf_softmax(float (&v)[CP], int C) {
    float mx = v[0];
#pragma unroll
    for (int c = 1; c < CP; ++c)
        if (c < C) mx = fmaxf(mx, v[c]);
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        if (c < C) { v[c] = expf(v[c] - mx); se += v[c]; } else v[c] = 0.f;
    }
    const float inv = 1.f / se;
#pragma unroll
    for (int c = 0; c < CP; ++c) v[c] *= inv;
}

__device__ __forceinline__ int crf_slot(int pix, int nv) { return pix * nv + (pix >> 2); }

template <int CP>
__global__ __launch_bounds__(256) void k_crf_q0(const CrfArgs A, float* __restrict__ q0, int M) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= M) return;
    float v[CP];
    crf_unary<CP>(A, (size_t)p, v);
    crf_softmax<CP>(v, A.C);
    float* o = q0 + (size_t)p * A.C;
    if ((A.C & 3) == 0 && ((uintptr_t)q0 & 15u) == 0) {
#pragma unroll
        for (int j = 0; j < CP / 4; ++j) {
            f32x4 s; s[0] = v[4 * j]; s[1] = v[4 * j + 1]; s[2] = v[4 * j + 2]; s[3] = v[4 * j + 3];
            reinterpret_cast<f32x4*>(o)[j] = s;
        }
    } else {
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < A.C) o[c] = v[c];
    }
}

template <int CP, int NT, bool STAGED>
__global__ __launch_bounds__(NT) void k_crf_step(const CrfArgs A) {
    extern __shared__ f32x4 crf_lds[];                        // STAGED: Q slots, then one colour slot per staged pixel
    __shared__ float s_ga[CRF_TAPS], s_gs[CRF_TAPS];
    constexpr int PX = CRF_PX, NV = CP / 4, GROUPS = CRF_TW / PX, TH = NT / GROUPS;
    static_assert(TH * GROUPS == NT, "one thread per PX pixels of the tile");
    const int C = A.C, r = A.r, d = A.d, h = r * d, H = A.H, W = A.W, side = 2 * r + 1;
    const int tx = blockIdx.x % A.tiles_x, rest = blockIdx.x / A.tiles_x, ty = rest % A.tiles_y, n = rest / A.tiles_y;
    const int y0 = ty * TH, x0 = tx * CRF_TW;
    const int SW = CRF_TW + 2 * h, SH = TH + 2 * h, npix = SH * SW;
    f32x4* sq = crf_lds;
    f32x4* si = crf_lds + crf_slot(npix, NV) + 1;
    const bool qvec = (C & 3) == 0 && (((uintptr_t)A.qin | (uintptr_t)A.qout) & 15u) == 0;   // dense rows of C == CP floats
    for (int t = threadIdx.x; t < side * side; t += NT) {
        s_ga[t] = A.ga[t];
        s_gs[t] = A.gs[t];
    }
    if (STAGED) {
        for (int s = threadIdx.x; s < npix; s += NT) {
            const int ly = s / SW, lx = s - ly * SW, gy = y0 - h + ly, gx = x0 - h + lx;
            float q[CP];
            f32x4 im = {0.f, 0.f, 0.f, 0.f};
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const size_t pix = ((size_t)n * H + gy) * W + gx;
                if (A.first) {
                    crf_unary<CP>(A, pix, q);
                    crf_softmax<CP>(q, C);
                } else {
                    crf_load_row<CP>(A.qin + pix * C, C, qvec, q);
                }
                im = crf_guide(A, n, gy, gx);
            } else {
#pragma unroll
                for (int c = 0; c < CP; ++c) q[c] = 0.f;
            }
            f32x4* o = sq + crf_slot(s, NV);
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                f32x4 v; v[0] = q[4 * j]; v[1] = q[4 * j + 1]; v[2] = q[4 * j + 2]; v[3] = q[4 * j + 3];
                o[j] = v;
            }
            si[s] = im;
        }
    }
    __syncthreads();
    const int trow = threadIdx.x / GROUPS, g = threadIdx.x - trow * GROUPS;
    const int chunk = g / d, ph = g - chunk * d, xl0 = chunk * PX * d + ph;      // the thread's pixels: columns xl0 + k d of the tile
    const int gy = y0 + trow, gx0 = x0 + xl0;
    if (gy >= H || gx0 >= W) return;                          // no barrier below
    f32x4 ic[PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        const int xk = gx0 + k * d;
        if (xk < W) ic[k] = STAGED ? si[(trow + h) * SW + xl0 + h + k * d] : crf_guide(A, n, gy, xk);
        else ic[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float sa[PX][CP], ss[PX][CP], na[PX], ns[PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        na[k] = 0.f; ns[k] = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) { sa[k][c] = 0.f; ss[k][c] = 0.f; }
    }
    for (int i = -r; i <= r; ++i) {
        const int yy = gy + i * d;
        if (yy < 0 || yy >= H) continue;
        for (int m = -r; m <= PX - 1 + r; ++m) {
            const int xx = gx0 + m * d;
            if (xx < 0 || xx >= W) continue;
            float q[CP];
            f32x4 im;
            if (STAGED) {
                const int s = (trow + h + i * d) * SW + xl0 + h + m * d;
                const f32x4* p = sq + crf_slot(s, NV);
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const f32x4 v = p[j];
                    q[4 * j] = v[0]; q[4 * j + 1] = v[1]; q[4 * j + 2] = v[2]; q[4 * j + 3] = v[3];
                }
                im = si[s];
            } else {
                crf_load_row<CP>(A.qin + (((size_t)n * H + yy) * W + xx) * C, C, qvec, q);
                im = crf_guide(A, n, yy, xx);
            }
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                const int j = m - k;
                if (j >= -r && j <= r && (i | j) != 0) {
                    const int tap = (i + r) * side + j + r;
                    const float e0 = ic[k][0] - im[0], e1 = ic[k][1] - im[1], e2 = ic[k][2] - im[2];
                    const float d2 = e0 * e0 + e1 * e1 + e2 * e2;
                    const float ka = s_ga[tap] * __expf(A.cb * d2), ks = s_gs[tap];
                    na[k] += ka;
                    ns[k] += ks;
#pragma unroll
                    for (int c = 0; c < CP; ++c) {
                        sa[k][c] = fmaf(ka, q[c], sa[k][c]);
                        ss[k][c] = fmaf(ks, q[c], ss[k][c]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        const int xk = gx0 + k * d;
        if (xk >= W) continue;
        const size_t pix = ((size_t)n * H + gy) * W + xk;
        float u[CP], v[CP];
        crf_unary<CP>(A, pix, u);
        const float ra = na[k] > 0.f ? __fdiv_rn(A.wa, na[k]) : 0.f, rs = ns[k] > 0.f ? __fdiv_rn(A.ws, ns[k]) : 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) sa[k][c] = ra * sa[k][c] + rs * ss[k][c];             // the message m_c
        if (A.compat != nullptr) {                           // uniform
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                float acc = 0.f;
                if (c < C) {
#pragma unroll
                    for (int c2 = 0; c2 < CP; ++c2)
                        if (c2 < C) acc = fmaf(A.compat[c * C + c2], sa[k][c2], acc);
                }
                v[c] = u[c] - acc;
            }
        } else {
#pragma unroll
            for (int c = 0; c < CP; ++c) v[c] = u[c] + sa[k][c];                         // mu = -I: no C^2 product
        }
        crf_softmax<CP>(v, C);
        float* o = A.qout + pix * C;
        if (qvec) {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                f32x4 s; s[0] = v[4 * j]; s[1] = v[4 * j + 1]; s[2] = v[4 * j + 2]; s[3] = v[4 * j + 3];
                reinterpret_cast<f32x4*>(o)[j] = s;
            }
        } else {
#pragma unroll
            for (int c = 0; c < CP; ++c)
                if (c < C) o[c] = v[c];
        }
        if (A.last) {
            float best = 0.f;
            int bi = 0;
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                if (c < C) {
                    const float s = v[c];
                    if (c == 0 || s > best || (s != s && best == best)) { best = s; bi = c; }   // k_argmax's rule on the stored values
                }
            }
            A.pred[pix] = bi;
        }
    }
}

// dynamic LDS of the staged path for a (CP, PX, r d); what decides between the two paths
static size_t crf_lds_bytes(int CP, int TH, int h) {
    const int npix = (TH + 2 * h) * (CRF_TW + 2 * h);
    return sizeof(f32x4) * ((size_t)npix * (CP / 4) + (npix >> 2) + 1 + npix);
}
static inline int crf_threads(int) { return 192; }
static inline int crf_tile_rows(int CP) { return crf_threads(CP) * CRF_PX / CRF_TW; }

template <int CP, int NT>
static int crf_launch(const CrfArgs& A, bool staged, size_t lds_bytes, int nblocks, hipStream_t s) {
    if (staged) {
        static bool asked[64] = {};                           // more than 64 KiB of dynamic LDS has to be asked for, once per kernel and device
        int device = 0;
        if (lds_bytes > 64 * 1024 && (hipGetDevice(&device) != hipSuccess || device < 0 || device >= 64 || !asked[device])) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_crf_step<CP, NT, true>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)CRF_LDS_CAP);
            if (e != hipSuccess) {
                cvk_set_error("cvk_crf_step: %zu bytes of LDS refused: %s", lds_bytes, hipGetErrorString(e));
                return (int)e;
            }
            if (device >= 0 && device < 64) asked[device] = true;
        }
        hipLaunchKernelGGL((k_crf_step<CP, NT, true>), dim3(nblocks), dim3(NT), lds_bytes, s, A);
    } else {
        if (A.first) {
            const int M = A.N * A.H * A.W;
            hipLaunchKernelGGL((k_crf_q0<CP>), dim3(cvk_cdiv(M, 256)), dim3(256), 0, s, A, const_cast<float*>(A.qin), M);
        }
        hipLaunchKernelGGL((k_crf_step<CP, NT, false>), dim3(nblocks), dim3(NT), 0, s, A);
    }
    return CVK_OK;
}

static int crf_check_window(const char* who, int C, int radius, int dilation) {
    CVK_CHECK_ARG(C >= 1 && C <= CRF_MAX_C, "%s: %d classes, the kernel holds 1 to %d per pixel in registers", who, C, CRF_MAX_C);
    CVK_CHECK_ARG(radius >= 1 && radius <= CRF_MAX_R, "%s: radius %d outside 1..%d", who, radius, CRF_MAX_R);
    CVK_CHECK_ARG(dilation >= 1 && dilation <= CRF_MAX_D, "%s: dilation %d outside 1..%d", who, dilation, CRF_MAX_D);
    return CVK_OK;
}

}  // namespace

extern "C" int cvk_crf_tile(int C, int radius, int dilation, int* th, int* tw, int* staged) {
    if (int rc = crf_check_window("cvk_crf_tile", C, radius, dilation)) return rc;
    const int CP = (C + 3) / 4 * 4, TH = crf_tile_rows(CP);
    if (th) *th = TH;
    if (tw) *tw = CRF_TW;
    if (staged) *staged = crf_lds_bytes(CP, TH, radius * dilation) <= CRF_LDS_CAP ? 1 : 0;
    return CVK_OK;
}

extern "C" int cvk_crf_step(const float* unary, int ld_u, int unary_is_prob, const float* q_in, float* q_out, int64_t* pred,
                            const void* guide, int guide_u8, int64_t gN, int64_t gC, int64_t gH, int64_t gW, const float* guide_a,
                            const float* guide_b, const float* ga, const float* gs, float cb, float wa, float ws, const float* compat,
                            int N, int H, int W, int C, int radius, int dilation, int first, int last, void* stream) {
    CVK_CHECK_ARG(unary && q_in && q_out && guide && ga && gs, "cvk_crf_step: null pointer");
    CVK_CHECK_ARG(guide_u8 || (guide_a && guide_b), "cvk_crf_step: a float guide needs its scale and offset");
    if (int rc = crf_check_window("cvk_crf_step", C, radius, dilation)) return rc;
    CVK_CHECK_ARG(N > 0 && H > 0 && W > 0 && ld_u >= C && H <= CRF_MAX_DIM && W <= CRF_MAX_DIM, "cvk_crf_step: bad arguments");
    CVK_CHECK_ARG((int64_t)N * H * W * C < 2147483647LL, "cvk_crf_step: a buffer of 2^31 values or more");
    CVK_CHECK_ARG(q_in != q_out, "cvk_crf_step: q_in and q_out are one buffer; the iterations alternate between two");
    CVK_CHECK_ARG(pred || !last, "cvk_crf_step: the last iteration writes pred");
    CVK_CHECK_ARG(cb <= 0.f && cb >= -3.0e38f && wa >= 0.f && wa <= 3.0e38f && ws >= 0.f && ws <= 3.0e38f,
                  "cvk_crf_step: cb must be finite and <= 0, wa and ws finite and >= 0");
    CrfArgs A;
    A.unary = unary; A.qin = q_in; A.qout = q_out; A.pred = pred; A.guide = guide; A.compat = compat;
    A.gN = gN; A.gC = gC; A.gH = gH; A.gW = gW;
    A.ld_u = ld_u; A.is_prob = unary_is_prob != 0; A.guide_u8 = guide_u8 != 0; A.N = N; A.H = H; A.W = W; A.C = C; A.r = radius;
    A.d = dilation; A.first = first != 0; A.last = last != 0;
    for (int k = 0; k < 3; ++k) {
        A.a[k] = guide_u8 ? 1.f : guide_a[k];
        A.b[k] = guide_u8 ? 0.f : guide_b[k];
    }
    A.cb = cb; A.wa = wa; A.ws = ws;
    const int taps = (2 * radius + 1) * (2 * radius + 1);
    for (int t = 0; t < CRF_TAPS; ++t) {
        A.ga[t] = t < taps ? ga[t] : 0.f;
        A.gs[t] = t < taps ? gs[t] : 0.f;
    }
    const int CP = (C + 3) / 4 * 4, TH = crf_tile_rows(CP);
    A.tiles_x = cvk_cdiv(W, CRF_TW);
    A.tiles_y = cvk_cdiv(H, TH);
    const int64_t nblocks = (int64_t)A.tiles_x * A.tiles_y * N;
    CVK_CHECK_ARG(nblocks < 2147483647LL, "cvk_crf_step: grid too large");
    const size_t lds_bytes = crf_lds_bytes(CP, TH, radius * dilation);
    const bool staged = lds_bytes <= CRF_LDS_CAP;
    hipStream_t s = (hipStream_t)stream;
    int rc = CVK_EINVAL;
#define CRF_CASE(cp, nt) \
    case cp: rc = crf_launch<cp, nt>(A, staged, lds_bytes, (int)nblocks, s); break;
    switch (CP) {
        CRF_CASE(4, 192) CRF_CASE(8, 192) CRF_CASE(12, 192) CRF_CASE(16, 192) CRF_CASE(20, 192) CRF_CASE(24, 192) CRF_CASE(28, 192) CRF_CASE(32, 192)
    }
#undef CRF_CASE
    if (rc != CVK_OK) return rc;
    CVK_LAUNCH_RETURN("cvk_crf_step");
}
