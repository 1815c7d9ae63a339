#pragma once
// loss_boundary.h: boundary loss (Kervadec et al., MIDL 2019; cvk_boundary_loss_fwd / _bwd).
// loss = cb B + cc H, B = 1 / |V| sum_{q in V} sum_{c in S} phi_c(q) p_c(q), p = softmax(x), H = the weighted mean cross-entropy of
// k_ce_fwd_ex (label_smoothing 0), V = the pixels whose target is a class.  S is a bit mask.  phi is [M][C] dense.
//   k_bdl_fwd     the staging of k_ce_fwd_ex, thread = pixel: the pixel's row in LDS is overwritten with phi_c p_c (zeros outside V and
//                 S); then thread (c, r) = (tid % 32, tid / 32) sums column c over rows [32 r, 32 r + 32) of the tile in row order.
//                 part[k][nb]: valid pixels | out-of-range targets | cross-entropy sum | sum w[t] | class c's sum at 4 + c
//   k_bdl_finish  one work-group: every part row in fp64 (thread order, then one fixed tree); B = the sum of the class terms; reads the
//                 two coefficients from device memory and leaves them in the record for the backward
//   k_bdl_bwd     one pass, dlogits written once
// LDS: the (ld + 1) KiB tile + 1.2 KiB.  No float atomic: loss and gradient are bitwise reproducible.
// The staging and the weighted pixel terms come from loss_rows.h; edt.h is included for EDT_MAX_C, the widest phi that the distance
// transform writes.
#include "cvk_common.h"
#include "loss_rows.h"
#include "edt.h"

namespace {

constexpr int BDL_PART_HEAD = 4, BDL_REC_HEAD = 8, BDL_RECORD_FLOATS = BDL_REC_HEAD + EDT_MAX_C;

__global__ __launch_bounds__(256) void k_bdl_fwd(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                const float* __restrict__ phi, const float* __restrict__ weight, int want_ce,
                                                unsigned cmask, float* __restrict__ part, int nb, int M, int C, int ignore_index) {
    extern __shared__ float lds[];
    __shared__ float red[4];
    __shared__ float s_w[EDT_MAX_C];
    __shared__ float s_cs[8][EDT_MAX_C];
    ce_ex_stage_w(weight, s_w, C);                                   // visible after the first chunk's barriers
    const int pitch = ld + 1;
    const int cc = threadIdx.x & 31, cr = threadIdx.x >> 5;
    float acc = 0.f, div = 0.f, cnt = 0.f, bad = 0.f, csum = 0.f;
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK;
    for (int ch = 0; ch < CE_ROWS_PER_BLOCK / CE_CHUNK; ++ch) {
        const int m0 = base + ch * CE_CHUNK;
        if (m0 >= M) break;
        const int rows = min(CE_CHUNK, M - m0);
        __syncthreads();
        ce_chunk_load(logits + (size_t)m0 * ld, lds, rows * ld, ld);
        __syncthreads();
        if ((int)threadIdx.x < rows) {
            float* x = lds + threadIdx.x * pitch;
            const size_t m = (size_t)m0 + threadIdx.x;
            const long t = (long)target[m];
            if (t != (long)ignore_index && t >= 0 && t < C) {
                cnt += 1.f;
                if (want_ce) {
                    acc += ce_ex_pixel_loss(x, C, (int)t, s_w, 0.f);
                    div += s_w[t];
                }
                float mx = x[0];
                for (int c = 1; c < C; ++c) mx = fmaxf(mx, x[c]);
                float se = 0.f;
                for (int c = 0; c < C; ++c) se += expf(x[c] - mx);
                const float inv = 1.f / se;
                for (int c = 0; c < C; ++c) x[c] = ((cmask >> c) & 1u) ? phi[m * C + c] * (expf(x[c] - mx) * inv) : 0.f;
            } else {
                if (t != (long)ignore_index) bad += 1.f;
                for (int c = 0; c < C; ++c) x[c] = 0.f;
            }
        }
        __syncthreads();
        if (cc < C) {
            const int r1 = min(rows, cr * 32 + 32);
            float s = 0.f;
            for (int r = cr * 32; r < r1; ++r) s += lds[r * pitch + cc];
            csum += s;
        }
    }
    const float n = block_sum_256(cnt, red);
    const float b = block_sum_256(bad, red);
    const float s = block_sum_256(acc, red);
    const float d = block_sum_256(div, red);
    s_cs[cr][cc] = csum;
    __syncthreads();
    if ((int)threadIdx.x < C) {
        float v = 0.f;
        for (int r = 0; r < 8; ++r) v += s_cs[r][threadIdx.x];
        part[(size_t)(BDL_PART_HEAD + threadIdx.x) * nb + blockIdx.x] = v;
    }
    if (threadIdx.x == 0) {
        part[blockIdx.x] = n;
        part[nb + blockIdx.x] = b;
        part[2 * nb + blockIdx.x] = s;
        part[3 * nb + blockIdx.x] = d;
    }
}

// record: loss | |V| | out-of-range targets | B | H | cb | cc | sum w[t] | class c's share of B at 8 + c
__global__ __launch_bounds__(256) void k_bdl_finish(const float* __restrict__ part, int nb, const float* __restrict__ coef,
                                                   int want_b, int want_ce, int C, float* __restrict__ record) {
    __shared__ double s_tot[BDL_PART_HEAD + EDT_MAX_C];
    const int lane = threadIdx.x & 63;
    for (int k = threadIdx.x >> 6; k < BDL_PART_HEAD + C; k += 4) {            // a wave owns every fourth row: lane order, then one fixed tree
        double v = 0.0;
        for (int i = lane; i < nb; i += 64) v += (double)part[(size_t)k * nb + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) s_tot[k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double V = s_tot[0];
        double bsum = 0.0;
        for (int c = 0; c < C; ++c) {
            const double term = V > 0.0 ? s_tot[BDL_PART_HEAD + c] / V : 0.0;
            record[BDL_REC_HEAD + c] = (float)term;
            bsum += term;
        }
        for (int c = C; c < EDT_MAX_C; ++c) record[BDL_REC_HEAD + c] = 0.f;
        const double H = want_ce ? s_tot[2] / s_tot[3] : 0.0;                  // 0/0 = NaN when no pixel is valid, as cvk_softmax_ce_fwd_ex
        const float cb = want_b ? coef[0] : 0.f, cc = want_ce ? coef[1] : 0.f;
        double loss = 0.0;
        if (want_b) loss += (double)cb * bsum;
        if (want_ce) loss += (double)cc * H;
        record[0] = s_tot[1] > 0.0 ? __builtin_nanf("") : (float)loss;
        record[1] = (float)V;
        record[2] = (float)s_tot[1];
        record[3] = (float)bsum;
        record[4] = (float)H;
        record[5] = cb;
        record[6] = cc;
        record[7] = want_ce ? (float)s_tot[3] : 0.f;
    }
}

__global__ __launch_bounds__(256) void k_bdl_bwd(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                const float* __restrict__ phi, const float* __restrict__ weight, int want_ce,
                                                unsigned cmask, const float* __restrict__ record, const float* __restrict__ grad_out,
                                                float scale, float* __restrict__ dl, int ld_d, int M, int C, int ignore_index) {
    extern __shared__ float lds[];
    __shared__ float s_w[EDT_MAX_C];
    ce_ex_stage_w(weight, s_w, C);
    const float go = (grad_out != nullptr ? *grad_out : 1.f) * scale;
    const float kb = record[1] > 0.f ? record[5] * go / record[1] : 0.f;
    const float gce0 = want_ce ? record[6] * go / record[7] : 0.f;
    const int pitch = ld + 1;
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK;
    for (int ch = 0; ch < CE_ROWS_PER_BLOCK / CE_CHUNK; ++ch) {
        const int m0 = base + ch * CE_CHUNK;
        if (m0 >= M) break;
        const int rows = min(CE_CHUNK, M - m0);
        __syncthreads();
        ce_chunk_load(logits + (size_t)m0 * ld, lds, rows * ld, ld);
        __syncthreads();
        if ((int)threadIdx.x < rows) {
            float* x = lds + threadIdx.x * pitch;
            const size_t m = (size_t)m0 + threadIdx.x;
            const long t = (long)target[m];
            if (t == (long)ignore_index || t < 0 || t >= C) {
                for (int c = 0; c < ld; ++c) x[c] = 0.f;
            } else {
                float mx = x[0];
                for (int c = 1; c < C; ++c) mx = fmaxf(mx, x[c]);
                float se = 0.f;
                for (int c = 0; c < C; ++c) se += expf(x[c] - mx);
                const float inv = 1.f / se;
                float dot = 0.f;
                for (int c = 0; c < C; ++c)
                    if ((cmask >> c) & 1u) dot += phi[m * C + c] * (expf(x[c] - mx) * inv);
                const float gce = want_ce ? gce0 * s_w[t] : 0.f;
                for (int c = 0; c < C; ++c) {
                    const float p = expf(x[c] - mx) * inv;
                    const float f = ((cmask >> c) & 1u) ? phi[m * C + c] : 0.f;
                    x[c] = p * (kb * (f - dot)) + gce * (p - (c == (int)t ? 1.f : 0.f));
                }
                for (int c = C; c < ld; ++c) x[c] = 0.f;
            }
        }
        __syncthreads();
        if (ld_d == ld) {
            ce_chunk_store(dl + (size_t)m0 * ld_d, lds, rows * ld, ld);
        } else {
            for (int f = threadIdx.x; f < rows * ld_d; f += CE_CHUNK) {
                const int r = f / ld_d, c = f - r * ld_d;
                dl[(size_t)m0 * ld_d + f] = c < ld ? lds[r * pitch + c] : 0.f;
            }
        }
    }
}

}  // namespace

extern "C" int cvk_boundary_loss_part_floats(int M, int C) {
    return M > 0 && C >= 1 && C <= EDT_MAX_C ? (BDL_PART_HEAD + C) * cvk_ce_blocks(M) : 0;
}

extern "C" int cvk_boundary_loss_record_floats(void) { return BDL_RECORD_FLOATS; }

static int bdl_check(const char* who, const float* phi, const float* weight, int want_boundary, int want_ce, unsigned class_mask, int ld,
                     int M, int C) {
    CVK_CHECK_ARG(M > 0, "%s: sizes must be positive, got M %d", who, M);
    CVK_CHECK_ARG(C >= 1 && C <= EDT_MAX_C, "%s: %d classes, the kernels serve 1 to %d", who, C, EDT_MAX_C);
    CVK_CHECK_ARG(ld >= C && ld <= CE_MAX_LD, "%s: the pixel stride must be in [C, %d], got %d", who, CE_MAX_LD, ld);
    CVK_CHECK_ARG((want_boundary == 0 || want_boundary == 1) && (want_ce == 0 || want_ce == 1) && (want_boundary || want_ce),
                  "%s: want_boundary and want_ce must be 0 or 1 and not both 0", who);
    CVK_CHECK_ARG(!want_boundary || phi != nullptr, "%s: null pointer (the boundary term needs the distance maps)", who);
    CVK_CHECK_ARG(!want_boundary || (class_mask != 0u && (C == 32 || (class_mask >> C) == 0u)),
                  "%s: the class mask must name at least one class and none outside [0, C)", who);
    CVK_CHECK_ARG(weight == nullptr || want_ce, "%s: class weights enter the cross-entropy term only, and it is off", who);
    return CVK_OK;
}

extern "C" int cvk_boundary_loss_fwd(const float* logits, int ld, const int64_t* target, const float* phi, const float* weight,
                                     const float* coef, int want_boundary, int want_ce, unsigned class_mask, float* part, float* record,
                                     int M, int C, int ignore_index, void* stream) {
    CVK_CHECK_ARG(logits && target && coef && part && record, "cvk_boundary_loss_fwd: null pointer");
    const int rc = bdl_check("cvk_boundary_loss_fwd", phi, weight, want_boundary, want_ce, class_mask, ld, M, C);
    if (rc != CVK_OK) return rc;
    const int nb = cvk_ce_blocks(M);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_bdl_fwd, dim3(nb), dim3(256), CE_CHUNK * (ld + 1) * sizeof(float), s, logits, ld, target, phi, weight, want_ce,
                       want_boundary ? class_mask : 0u, part, nb, M, C, ignore_index);
    hipLaunchKernelGGL(k_bdl_finish, dim3(1), dim3(256), 0, s, part, nb, coef, want_boundary, want_ce, C, record);
    CVK_LAUNCH_RETURN("cvk_boundary_loss_fwd");
}

extern "C" int cvk_boundary_loss_bwd(const float* logits, int ld, const int64_t* target, const float* phi, const float* weight,
                                     int want_boundary, int want_ce, unsigned class_mask, const float* record, const float* grad_out,
                                     float scale, float* dlogits, int ld_d, int M, int C, int ignore_index, void* stream) {
    CVK_CHECK_ARG(logits && target && record && dlogits, "cvk_boundary_loss_bwd: null pointer");
    const int rc = bdl_check("cvk_boundary_loss_bwd", phi, weight, want_boundary, want_ce, class_mask, ld, M, C);
    if (rc != CVK_OK) return rc;
    CVK_CHECK_ARG(ld_d >= C, "cvk_boundary_loss_bwd: the gradient's pixel stride must be at least C, got %d", ld_d);
    hipLaunchKernelGGL(k_bdl_bwd, dim3(cvk_ce_blocks(M)), dim3(256), CE_CHUNK * (ld + 1) * sizeof(float), (hipStream_t)stream, logits, ld,
                       target, phi, weight, want_ce, want_boundary ? class_mask : 0u, record, grad_out, scale, dlogits, ld_d, M, C,
                       ignore_index);
    CVK_LAUNCH_RETURN("cvk_boundary_loss_bwd");
}
