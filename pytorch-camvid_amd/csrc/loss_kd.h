#pragma once
// loss_kd.h: knowledge-distillation loss, L = ce H + kd K (cvk_kd_loss_fwd / _bwd).
// H = the weighted mean cross-entropy of k_ce_fwd_ex, K = t2 / |D| sum over D of KL(softmax(tau z) || softmax(tau x)), x the student's
// and z the teacher's pixel row, each tensor with its own pixel stride.  One forward pass reads both: a chunk of 256 pixel rows of the
// student and the same rows of the teacher sit side by side in LDS (the staging of k_ce_fwd_ex, pitch ld + 1 each), thread = pixel.
// The two tiles fit 64 KiB of dynamic LDS while (ld_s + 1) + (ld_t + 1) <= KD_MAX_PITCH; beyond that STAGED = false and a thread
// walks its two rows in global memory.  A pixel's KL comes from the two log-sum-exps,
//   kl = sum_c e_c (b_c - a_c) / sum_c e_c + log sum_c exp(a_c) - log sum_c e_c,  a_c = tau (x_c - max x), b_c = tau (z_c - max z),
// e_c = exp(b_c): no logarithm of a softmax value is taken, and kl is exactly 0 when the two rows hold the same numbers.  Both maxima
// are in registers for the softmaxes, so the arg-max agreement (first index of the maximum, NaN wins: the rule of k_argmax) is free.
// Pixel sets: a labelled pixel (t in [0, C)) enters H; D = the labelled pixels, plus the ignored ones when distill_ignored; a null
// target labels nothing and puts every pixel into D; an out-of-range target is in neither set.  Every sum has one fixed order
// (thread, wave, workgroup, then k_kd_finish in fp64) and there is no float atomic.
// The chunk staging, ce_ex_stage_w and CE_EX_MAX_C come from loss_rows.h.
#include "cvk_common.h"
#include "loss_rows.h"

namespace {

constexpr int KD_MAX_PITCH = 64;           // (ld_s + 1) + (ld_t + 1) of the staged variant: 64 KiB of dynamic LDS
constexpr int KD_PART_ROWS = 7;            // CE numerator, sum w[t], valid pixels, out-of-range targets, KL sum, |D|, arg-max agreements
constexpr int KD_RECORD_FLOATS = 9;        // L, valid, out of range, sum w[t], H, K, |D|, agree, agree / |D|

__device__ __forceinline__ float kd_row_max(const float* x, int C, int* arg) {
    float best = x[0];
    int bi = 0;
    for (int c = 1; c < C; ++c) {
        const float v = x[c];
        if (v > best || (v != v && best == best)) { best = v; bi = c; }
    }
    *arg = bi;
    return best;
}

// lse = log sum exp(x) (when want_ce), kl and the arg-max agreement (when want_kd; z is not read otherwise)
__device__ __forceinline__ void kd_pixel_fwd(const float* x, const float* z, int C, float tau, bool want_ce, bool want_kd, float* lse,
                                             float* kl, bool* agree) {
    int ax, az;
    const float mx = kd_row_max(x, C, &ax);
    if (want_ce) {
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(x[c] - mx);
        *lse = mx + logf(se);
    }
    if (want_kd) {
        float ss = 0.f;
        for (int c = 0; c < C; ++c) ss += expf(tau * (x[c] - mx));
        const float mz = kd_row_max(z, C, &az);
        float sz = 0.f, dot = 0.f;
        for (int c = 0; c < C; ++c) {
            const float b = tau * (z[c] - mz), e = expf(b);
            sz += e;
            dot += e * (b - tau * (x[c] - mx));
        }
        *kl = dot / sz + (logf(ss) - logf(sz));
        *agree = ax == az;
    }
}

// o[k] = cw (p_k - [k = t]) + kw (ps_k - qs_k); o may alias x (column k is read before it is written); columns [C, ld_o) are zeroed
__device__ __forceinline__ void kd_pixel_grad(const float* x, const float* z, float* o, int ld_o, int C, int t, bool want_ce, float cw,
                                              bool want_kd, float kw, float tau) {
    int ax;
    const float mx = kd_row_max(x, C, &ax);
    float inv_e = 0.f, inv_s = 0.f, inv_z = 0.f, mz = 0.f;
    if (want_ce) {
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(x[c] - mx);
        inv_e = 1.f / se;
    }
    if (want_kd) {
        float ss = 0.f, sz = 0.f;
        for (int c = 0; c < C; ++c) ss += expf(tau * (x[c] - mx));
        mz = kd_row_max(z, C, &ax);
        for (int c = 0; c < C; ++c) sz += expf(tau * (z[c] - mz));
        inv_s = 1.f / ss;
        inv_z = 1.f / sz;
    }
    for (int c = 0; c < C; ++c) {
        const float d = x[c] - mx;
        float r = 0.f;
        if (want_ce) r = cw * (expf(d) * inv_e - (c == t ? 1.f : 0.f));
        if (want_kd) r += kw * (expf(tau * d) * inv_s - expf(tau * (z[c] - mz)) * inv_z);
        o[c] = r;
    }
    for (int c = C; c < ld_o; ++c) o[c] = 0.f;
}

// which sums pixel m enters: *t = its class when labelled (else -1); returns 1 if it is in D, and adds to *bad an out-of-range target
__device__ __forceinline__ bool kd_classify(const int64_t* __restrict__ target, int m, int C, int ignore_index, int distill_ignored,
                                            int* t, float* bad) {
    *t = -1;
    if (target == nullptr) return true;
    const long v = (long)target[m];
    if (v == (long)ignore_index) return distill_ignored != 0;
    if (v >= 0 && v < C) {
        *t = (int)v;
        return true;
    }
    if (bad != nullptr) *bad += 1.f;
    return false;
}

template <bool STAGED>
__global__ __launch_bounds__(256) void k_kd_fwd(const float* __restrict__ student, int ld_s, const float* __restrict__ teacher, int ld_t,
                                               const int64_t* __restrict__ target, const float* __restrict__ weight, float ce, float kd,
                                               float tau, int distill_ignored, float* __restrict__ part, int nb, int M, int C,
                                               int ignore_index) {
    extern __shared__ float lds[];
    __shared__ float red[4];
    __shared__ float s_w[CE_EX_MAX_C];
    ce_ex_stage_w(weight, s_w, C);
    __syncthreads();
    const int pitch_s = ld_s + 1, pitch_t = ld_t + 1;
    float* lds_t = lds + CE_CHUNK * pitch_s;
    float acc = 0.f, div = 0.f, cnt = 0.f, bad = 0.f, skl = 0.f, nd = 0.f, agr = 0.f;
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK;
    for (int ch = 0; ch < CE_ROWS_PER_BLOCK / CE_CHUNK; ++ch) {
        const int m0 = base + ch * CE_CHUNK;
        if (m0 >= M) break;
        const int rows = min(CE_CHUNK, M - m0);
        if (STAGED) {
            __syncthreads();
            ce_chunk_load(student + (size_t)m0 * ld_s, lds, rows * ld_s, ld_s);
            if (kd > 0.f) ce_chunk_load(teacher + (size_t)m0 * ld_t, lds_t, rows * ld_t, ld_t);
            __syncthreads();
        }
        if ((int)threadIdx.x < rows) {
            const int m = m0 + threadIdx.x;
            int t;
            const bool in_d = kd_classify(target, m, C, ignore_index, distill_ignored, &t, &bad);
            const bool want_ce = ce > 0.f && t >= 0, want_kd = kd > 0.f && in_d;
            if (want_ce || want_kd) {
                const float* x = STAGED ? lds + threadIdx.x * pitch_s : student + (size_t)m * ld_s;
                const float* z = !want_kd ? nullptr : STAGED ? lds_t + threadIdx.x * pitch_t : teacher + (size_t)m * ld_t;
                float lse = 0.f, kl = 0.f;
                bool same = false;
                kd_pixel_fwd(x, z, C, tau, want_ce, want_kd, &lse, &kl, &same);
                if (want_ce) acc += s_w[t] * (lse - x[t]);
                if (want_kd) {
                    skl += kl;
                    agr += same ? 1.f : 0.f;
                }
            }
            if (t >= 0) div += s_w[t];
            if (t >= 0 || target == nullptr) cnt += 1.f;
            if (in_d) nd += 1.f;
        }
    }
    const float v[KD_PART_ROWS] = {block_sum_256(acc, red), block_sum_256(div, red), block_sum_256(cnt, red), block_sum_256(bad, red),
                                   block_sum_256(skl, red), block_sum_256(nd, red),  block_sum_256(agr, red)};
    if (threadIdx.x == 0)
        for (int k = 0; k < KD_PART_ROWS; ++k) part[(size_t)k * nb + blockIdx.x] = v[k];
}

// One workgroup, fp64 in fixed order: rec[0] = L (NaN when a target was out of range), rec[1] = valid pixels, rec[2] = out-of-range
// targets, rec[3] = sum w[t], rec[4] = H (0 when ce = 0; 0/0 = NaN), rec[5] = K (0 when kd = 0; 0/0 = NaN), rec[6] = |D|, rec[7] = the
// pixels of D where student and teacher agree on the arg-max, rec[8] = rec[7] / rec[6] (both 0 when kd = 0, where no teacher is read;
// |D| is counted either way).
__global__ __launch_bounds__(256) void k_kd_finish(const float* __restrict__ part, int nb, float ce, float kd, float t2,
                                                  float* __restrict__ rec) {
    __shared__ double red[KD_PART_ROWS][256];
    double v[KD_PART_ROWS];
    for (int k = 0; k < KD_PART_ROWS; ++k) v[k] = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256)
        for (int k = 0; k < KD_PART_ROWS; ++k) v[k] += (double)part[(size_t)k * nb + i];
    for (int k = 0; k < KD_PART_ROWS; ++k) red[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o)
            for (int k = 0; k < KD_PART_ROWS; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double H = ce > 0.f ? red[0][0] / red[1][0] : 0.0;
        const double K = kd > 0.f ? (double)t2 * red[4][0] / red[5][0] : 0.0;
        const double L = (ce > 0.f ? (double)ce * H : 0.0) + (kd > 0.f ? (double)kd * K : 0.0);
        rec[0] = red[3][0] > 0.0 ? __builtin_nanf("") : (float)L;
        rec[1] = (float)red[2][0];
        rec[2] = (float)red[3][0];
        rec[3] = (float)red[1][0];
        rec[4] = (float)H;
        rec[5] = (float)K;
        rec[6] = (float)red[5][0];
        rec[7] = (float)red[6][0];
        rec[8] = kd > 0.f ? (float)(red[6][0] / red[5][0]) : 0.f;
    }
}

// The two coefficients of a pixel's gradient row, g = grad_out * scale folded in: labelled pixels take g ce w[t] / sum w[t], pixels of
// D take g kd t2 tau / |D|.
struct KdScale { float c, k; };

__device__ __forceinline__ KdScale kd_scale(const float* __restrict__ rec, const float* __restrict__ grad_out, float scale, float ce,
                                            float kd, float tau, float t2) {
    const float g = (grad_out != nullptr ? *grad_out : 1.f) * scale;
    KdScale s;
    s.c = ce > 0.f ? g * ce / rec[3] : 0.f;
    s.k = kd > 0.f ? g * kd * t2 * tau / rec[6] : 0.f;
    return s;
}

// Rows outside both sets and columns [C, ld_d) are written as zeros.
__global__ __launch_bounds__(256) void k_kd_bwd(const float* __restrict__ student, int ld_s, const float* __restrict__ teacher, int ld_t,
                                               const int64_t* __restrict__ target, const float* __restrict__ weight, float ce, float kd,
                                               float tau, float t2, int distill_ignored, const float* __restrict__ rec,
                                               const float* __restrict__ grad_out, float scale, float* __restrict__ dl, int ld_d, int M,
                                               int C, int ignore_index) {
    extern __shared__ float lds[];
    __shared__ float s_w[CE_EX_MAX_C];
    ce_ex_stage_w(weight, s_w, C);                   // visible after the first chunk's barriers
    const KdScale sc = kd_scale(rec, grad_out, scale, ce, kd, tau, t2);
    const int pitch_s = ld_s + 1, pitch_t = ld_t + 1;
    float* lds_t = lds + CE_CHUNK * pitch_s;
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK;
    for (int ch = 0; ch < CE_ROWS_PER_BLOCK / CE_CHUNK; ++ch) {
        const int m0 = base + ch * CE_CHUNK;
        if (m0 >= M) break;
        const int rows = min(CE_CHUNK, M - m0);
        __syncthreads();
        ce_chunk_load(student + (size_t)m0 * ld_s, lds, rows * ld_s, ld_s);
        if (kd > 0.f) ce_chunk_load(teacher + (size_t)m0 * ld_t, lds_t, rows * ld_t, ld_t);
        __syncthreads();
        if ((int)threadIdx.x < rows) {
            float* p = lds + threadIdx.x * pitch_s;
            int t;
            const bool in_d = kd_classify(target, m0 + threadIdx.x, C, ignore_index, distill_ignored, &t, nullptr);
            const bool want_ce = ce > 0.f && t >= 0, want_kd = kd > 0.f && in_d;
            if (want_ce || want_kd)
                kd_pixel_grad(p, lds_t + threadIdx.x * pitch_t, p, ld_s, C, t, want_ce, want_ce ? sc.c * s_w[t] : 0.f, want_kd, sc.k, tau);
            else
                for (int c = 0; c < ld_s; ++c) p[c] = 0.f;
        }
        __syncthreads();
        if (ld_d == ld_s) {
            ce_chunk_store(dl + (size_t)m0 * ld_d, lds, rows * ld_s, ld_s);
        } else {
            for (int f = threadIdx.x; f < rows * ld_d; f += CE_CHUNK) {
                const int r = f / ld_d, c = f - r * ld_d;
                dl[(size_t)m0 * ld_d + f] = c < ld_s ? lds[r * pitch_s + c] : 0.f;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_kd_bwd_rows(const float* __restrict__ student, int ld_s, const float* __restrict__ teacher,
                                                    int ld_t, const int64_t* __restrict__ target, const float* __restrict__ weight,
                                                    float ce, float kd, float tau, float t2, int distill_ignored,
                                                    const float* __restrict__ rec, const float* __restrict__ grad_out, float scale,
                                                    float* __restrict__ dl, int ld_d, int M, int C, int ignore_index) {
    __shared__ float s_w[CE_EX_MAX_C];
    ce_ex_stage_w(weight, s_w, C);
    __syncthreads();
    const KdScale sc = kd_scale(rec, grad_out, scale, ce, kd, tau, t2);
    for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (long)gridDim.x * blockDim.x) {
        float* o = dl + (size_t)m * ld_d;
        int t;
        const bool in_d = kd_classify(target, (int)m, C, ignore_index, distill_ignored, &t, nullptr);
        const bool want_ce = ce > 0.f && t >= 0, want_kd = kd > 0.f && in_d;
        if (want_ce || want_kd)
            kd_pixel_grad(student + (size_t)m * ld_s, want_kd ? teacher + (size_t)m * ld_t : nullptr, o, ld_d, C, t, want_ce,
                          want_ce ? sc.c * s_w[t] : 0.f, want_kd, sc.k, tau);
        else
            for (int c = 0; c < ld_d; ++c) o[c] = 0.f;
    }
}

}  // namespace

extern "C" int cvk_kd_loss_part_floats(int M) { return M > 0 ? KD_PART_ROWS * cvk_ce_blocks(M) : 0; }

extern "C" int cvk_kd_loss_record_floats(void) { return KD_RECORD_FLOATS; }

// the checks the two entry points share (x >= 0 and x > 0 are false for NaN); `who` names the entry point in the message
static int kd_loss_check(const char* who, const float* student, int ld_s, const float* teacher, int ld_t, const int64_t* target, float ce,
                         float kd, float tau, float t2, int M, int C) {
    CVK_CHECK_ARG(student, "%s: null pointer", who);
    CVK_CHECK_ARG(M > 0 && C > 0 && C <= CE_EX_MAX_C, "%s: bad arguments (M > 0 and 1 <= C <= 128)", who);
    CVK_CHECK_ARG(ld_s >= C && (teacher == nullptr || ld_t >= C), "%s: a pixel stride is smaller than C", who);
    CVK_CHECK_ARG(ce >= 0.f && kd >= 0.f && ce <= 3.0e38f && kd <= 3.0e38f, "%s: ce and kd must be finite and not negative", who);
    CVK_CHECK_ARG(ce > 0.f || kd > 0.f, "%s: ce and kd are both zero", who);
    CVK_CHECK_ARG(tau > 0.f && t2 > 0.f && tau <= 3.0e38f && t2 <= 3.0e38f, "%s: tau and t2 must be positive and finite", who);
    CVK_CHECK_ARG(target || !(ce > 0.f), "%s: a null target needs ce = 0", who);
    CVK_CHECK_ARG(teacher || !(kd > 0.f), "%s: a null teacher needs kd = 0", who);
    return CVK_OK;
}

// both tiles of the staged kernels fit the file's 64 KiB of dynamic LDS (no teacher tile when kd = 0)
static bool kd_staged(int ld_s, int ld_t, float kd) { return (ld_s + 1) + (kd > 0.f ? ld_t + 1 : 0) <= KD_MAX_PITCH; }

static size_t kd_lds_bytes(int ld_s, int ld_t, float kd) {
    return (size_t)CE_CHUNK * ((ld_s + 1) + (kd > 0.f ? ld_t + 1 : 0)) * sizeof(float);
}

extern "C" int cvk_kd_loss_fwd(const float* student, int ld_s, const float* teacher, int ld_t, const int64_t* target, const float* weight,
                               float ce, float kd, float tau, float t2, int distill_ignored, float* part, float* record, int M, int C,
                               int ignore_index, void* stream) {
    CVK_CHECK_ARG(part && record, "cvk_kd_loss_fwd: null pointer");
    if (int rc = kd_loss_check("cvk_kd_loss_fwd", student, ld_s, teacher, ld_t, target, ce, kd, tau, t2, M, C)) return rc;
    const int nb = cvk_ce_blocks(M);
    hipStream_t s = (hipStream_t)stream;
    if (kd_staged(ld_s, ld_t, kd))
        hipLaunchKernelGGL(k_kd_fwd<true>, dim3(nb), dim3(256), kd_lds_bytes(ld_s, ld_t, kd), s, student, ld_s, teacher, ld_t, target, weight,
                           ce, kd, tau, distill_ignored, part, nb, M, C, ignore_index);
    else
        hipLaunchKernelGGL(k_kd_fwd<false>, dim3(nb), dim3(256), 0, s, student, ld_s, teacher, ld_t, target, weight, ce, kd, tau,
                           distill_ignored, part, nb, M, C, ignore_index);
    hipLaunchKernelGGL(k_kd_finish, dim3(1), dim3(256), 0, s, part, nb, ce, kd, t2, record);
    CVK_LAUNCH_RETURN("cvk_kd_loss_fwd");
}

extern "C" int cvk_kd_loss_bwd(const float* student, int ld_s, const float* teacher, int ld_t, const int64_t* target, const float* weight,
                               float ce, float kd, float tau, float t2, int distill_ignored, const float* record, const float* grad_out,
                               float scale, float* dlogits, int ld_d, int M, int C, int ignore_index, void* stream) {
    CVK_CHECK_ARG(record && dlogits, "cvk_kd_loss_bwd: null pointer");
    if (int rc = kd_loss_check("cvk_kd_loss_bwd", student, ld_s, teacher, ld_t, target, ce, kd, tau, t2, M, C)) return rc;
    CVK_CHECK_ARG(ld_d >= C, "cvk_kd_loss_bwd: a pixel stride is smaller than C");
    hipStream_t s = (hipStream_t)stream;
    if (kd_staged(ld_s, ld_t, kd))
        hipLaunchKernelGGL(k_kd_bwd, dim3(cvk_ce_blocks(M)), dim3(256), kd_lds_bytes(ld_s, ld_t, kd), s, student, ld_s, teacher, ld_t, target,
                           weight, ce, kd, tau, t2, distill_ignored, record, grad_out, scale, dlogits, ld_d, M, C, ignore_index);
    else
        hipLaunchKernelGGL(k_kd_bwd_rows, dim3(cvk_cdiv(M, 256) < 8192 ? cvk_cdiv(M, 256) : 8192), dim3(256), 0, s, student, ld_s, teacher,
                           ld_t, target, weight, ce, kd, tau, t2, distill_ignored, record, grad_out, scale, dlogits, ld_d, M, C,
                           ignore_index);
    CVK_LAUNCH_RETURN("cvk_kd_loss_bwd");
}
