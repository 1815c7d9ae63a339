#pragma once
// calibration.h: the calibration meter and the temperature fit (cvk_calib_accumulate, cvk_calib_newton_accumulate,
// cvk_calib_newton_step; the definitions are in include/cvk.h).
// Meter.  One pass over the logits, thread = pixel, the staging of the losses (loss_rows.h: CE_CHUNK pixel rows in LDS at pitch
// ld + 1).  A pixel's top-label probability conf = 1 / sum_c exp(tau x_c - max) falls into one of B right-closed bins; the workgroup
// counts {pixels, correct pixels, sum floor(conf 2^30)} per (predicted class, bin) in an LDS table of 64-bit words with LDS integer
// atomics and adds the non-zero words to the global table with 64-bit global atomics: every word is an integer sum, exact and
// independent of the order.  The negative log-likelihood and the Brier score are summed per thread and per workgroup in fp64 and
// added to the record by a one-workgroup finish in a fixed order.  No float atomic.
// The table (24 C B bytes) and the staged rows (1 KiB (ld + 1)) share the 64 KiB of dynamic LDS this file's kernels keep to; rows
// wider than CE_MAX_LD, or rows that do not fit beside the table, are walked in global memory (STAGED = false).
// Fit.  NLL(tau) = mean(lse(tau x) - tau x_t) is convex in tau = 1 / T.  A pass leaves the sums of {nll, E_p[x] - x_t, Var_p[x]},
// p = softmax(tau x), in the state; a one-thread kernel takes a bracketed Newton step in fp64 and writes a log row.  tau lives in
// device memory: the caller chains passes and steps on one stream without a host sync.
#include "cvk_common.h"
#include "loss_rows.h"

namespace {

constexpr int CALIB_MAX_C = 128, CALIB_MAX_B = 64, CALIB_MAX_CELLS = 2048;   // 2048 cells of 3 words: 48 KiB of LDS table
constexpr int CALIB_LDS_BYTES = 65536;
constexpr int CALIB_PART_ROWS = 4;        // meter: sum nll, sum brier, valid, out of range; fit: sum nll, sum g, sum h, valid
constexpr int CALIB_STATE_TAU = 0, CALIB_STATE_LO = 1, CALIB_STATE_HI = 2, CALIB_STATE_G = 3, CALIB_STATE_H = 4, CALIB_STATE_L = 5,
              CALIB_STATE_N = 6, CALIB_STATE_K = 7, CALIB_STATE_TAU32 = 8;
constexpr int CALIB_LOG_COLUMNS = 8;

__device__ __forceinline__ double calib_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// z_c = tau x_c must be ONE rounded multiply: contracted into the subtraction of the maximum, fma(tau, x_c, -m) leaves the rounding
// residue of m in the maximum's own term, which then is not exp(0) = 1, and conf can exceed 1.  The compiler contracts across
// statements by default, and __fmul_rn is a plain product to it, so the two pixel kernels switch contraction off for their bodies
// (CALIB_NO_CONTRACT; the pragma is honoured per function and reaches the helpers inlined into them).
#define CALIB_NO_CONTRACT _Pragma("clang fp contract(off)")

// the first maximum of a row, a NaN wins: the rule of k_argmax
__device__ __forceinline__ float calib_row_max(const float* x, int C, int* arg) {
    float best = x[0];
    int bi = 0;
    for (int c = 1; c < C; ++c) {
        const float v = x[c];
        if (v > best || (v != v && best == best)) { best = v; bi = c; }
    }
    *arg = bi;
    return best;
}

// t = the pixel's class when it is valid, else -1; an out-of-range target adds to *bad
__device__ __forceinline__ int calib_target(const int64_t* __restrict__ target, int m, int C, int ignore_index, int* bad) {
    const int64_t v = target[m];
    if (v == (int64_t)ignore_index) return -1;
    if (v >= 0 && v < C) return (int)v;
    *bad += 1;
    return -1;
}

// table == nullptr (with target, part nullptr): only the maps are written.  Dynamic LDS: the table, then the staged rows.
template <bool STAGED>
__global__ __launch_bounds__(256) void k_calib_accumulate(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                         const float* __restrict__ tau_p, unsigned long long* __restrict__ hist,
                                                         double* __restrict__ part, int nb, float* __restrict__ conf_o,
                                                         int64_t* __restrict__ pred_o, int M, int C, int B, int ignore_index) {
    CALIB_NO_CONTRACT
    extern __shared__ unsigned long long calib_lds[];
    __shared__ double red[4];
    const int words = hist != nullptr ? C * B * 3 : 0;
    unsigned long long* table = calib_lds;
    float* rows_lds = reinterpret_cast<float*>(calib_lds + words);
    for (int i = threadIdx.x; i < words; i += 256) table[i] = 0ull;     // visible after the first chunk's barriers (or the one below)
    if (!STAGED) __syncthreads();
    const float tau = tau_p != nullptr ? *tau_p : 1.f;
    const int pitch = ld + 1;
    double s_nll = 0.0, s_brier = 0.0;
    int n_valid = 0, n_bad = 0;
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK;
    for (int ch = 0; ch < CE_ROWS_PER_BLOCK / CE_CHUNK; ++ch) {
        const int m0 = base + ch * CE_CHUNK;
        if (m0 >= M) break;
        const int rows = min(CE_CHUNK, M - m0);
        if (STAGED) {
            __syncthreads();
            ce_chunk_load(logits + (size_t)m0 * ld, rows_lds, rows * ld, ld);
            __syncthreads();
        }
        if ((int)threadIdx.x < rows) {
            const int m = m0 + threadIdx.x;
            const int t = target != nullptr ? calib_target(target, m, C, ignore_index, &n_bad) : -1;
            if (t >= 0 || conf_o != nullptr || pred_o != nullptr) {
                const float* x = STAGED ? rows_lds + threadIdx.x * pitch : logits + (size_t)m * ld;
                int pred;
                const float mx = tau * calib_row_max(x, C, &pred);      // tau > 0: max(tau x) = tau max(x), rounding is monotone
                float se = 0.f;
                for (int c = 0; c < C; ++c) se += expf(tau * x[c] - mx);
                const float conf = 1.f / se;
                if (conf_o != nullptr) conf_o[m] = conf;
                if (pred_o != nullptr) pred_o[m] = pred;
                if (t >= 0) {
                    ++n_valid;
                    s_nll += (double)((mx + logf(se)) - tau * x[t]);
                    float br = 0.f;
                    for (int c = 0; c < C; ++c) {
                        const float d = expf(tau * x[c] - mx) * conf - (c == t ? 1.f : 0.f);
                        br += d * d;
                    }
                    s_brier += (double)br;
                    int bin = (int)ceilf(conf * (float)B) - 1;
                    bin = bin < 0 ? 0 : bin > B - 1 ? B - 1 : bin;
                    const long long q = (long long)floorf(conf * 1073741824.f);
                    unsigned long long* cell = table + (pred * B + bin) * 3;
                    atomicAdd(cell, 1ull);
                    if (pred == t) atomicAdd(cell + 1, 1ull);
                    atomicAdd(cell + 2, (unsigned long long)q);
                }
            }
        }
    }
    if (hist == nullptr) return;
    const double v[CALIB_PART_ROWS] = {calib_block_sum(s_nll, red), calib_block_sum(s_brier, red), calib_block_sum((double)n_valid, red),
                                       calib_block_sum((double)n_bad, red)};       // its barriers order the table's atomics too
    if (threadIdx.x == 0)
        for (int k = 0; k < CALIB_PART_ROWS; ++k) part[(size_t)k * nb + blockIdx.x] = v[k];
    for (int i = threadIdx.x; i < words; i += 256)
        if (table[i] != 0ull) atomicAdd(&hist[i], table[i]);
}

// one workgroup, fp64 in fixed order: out[k] = sum_i part[k][i]
__device__ __forceinline__ void calib_reduce_parts(const double* __restrict__ part, int nb, double* out) {
    __shared__ double red[CALIB_PART_ROWS][256];
    double v[CALIB_PART_ROWS];
    for (int k = 0; k < CALIB_PART_ROWS; ++k) v[k] = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256)
        for (int k = 0; k < CALIB_PART_ROWS; ++k) v[k] += part[(size_t)k * nb + i];
    for (int k = 0; k < CALIB_PART_ROWS; ++k) red[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o)
            for (int k = 0; k < CALIB_PART_ROWS; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        __syncthreads();
    }
    for (int k = 0; k < CALIB_PART_ROWS; ++k) out[k] = red[k][0];
}

// record: {int64 valid, int64 out of range, double sum nll, double sum brier}; the call's sums are added to it
__global__ __launch_bounds__(256) void k_calib_finish(const double* __restrict__ part, int nb, long long* __restrict__ record) {
    double v[CALIB_PART_ROWS];
    calib_reduce_parts(part, nb, v);
    if (threadIdx.x == 0) {
        double* sums = reinterpret_cast<double*>(record);
        record[0] += (long long)v[2];
        record[1] += (long long)v[3];
        sums[2] += v[0];
        sums[3] += v[1];
    }
}

template <bool STAGED>
__global__ __launch_bounds__(256) void k_calib_newton(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                     const double* __restrict__ state, double* __restrict__ part, int nb, int M, int C,
                                                     int ignore_index) {
    CALIB_NO_CONTRACT
    extern __shared__ unsigned long long calib_lds[];
    __shared__ double red[4];
    float* rows_lds = reinterpret_cast<float*>(calib_lds);
    const float tau = (float)state[CALIB_STATE_TAU];
    const int pitch = ld + 1;
    double s_nll = 0.0, s_g = 0.0, s_h = 0.0;
    int n_valid = 0, skipped = 0;           // the fit skips an out-of-range target like an ignored one; the meter counts them
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK;
    for (int ch = 0; ch < CE_ROWS_PER_BLOCK / CE_CHUNK; ++ch) {
        const int m0 = base + ch * CE_CHUNK;
        if (m0 >= M) break;
        const int rows = min(CE_CHUNK, M - m0);
        if (STAGED) {
            __syncthreads();
            ce_chunk_load(logits + (size_t)m0 * ld, rows_lds, rows * ld, ld);
            __syncthreads();
        }
        if ((int)threadIdx.x < rows) {
            const int m = m0 + threadIdx.x;
            const int t = calib_target(target, m, C, ignore_index, &skipped);
            if (t >= 0) {
                const float* x = STAGED ? rows_lds + threadIdx.x * pitch : logits + (size_t)m * ld;
                int pred;
                const float mx = tau * calib_row_max(x, C, &pred);
                float se = 0.f, sx = 0.f;
                for (int c = 0; c < C; ++c) {
                    const float e = expf(tau * x[c] - mx);
                    se += e;
                    sx += e * x[c];
                }
                const float inv = 1.f / se, mean = sx * inv;
                float var = 0.f;
                for (int c = 0; c < C; ++c) {
                    const float d = x[c] - mean;
                    var += expf(tau * x[c] - mx) * d * d;
                }
                ++n_valid;
                s_nll += (double)((mx + logf(se)) - tau * x[t]);
                s_g += (double)(mean - x[t]);
                s_h += (double)(var * inv);
            }
        }
    }
    const double v[CALIB_PART_ROWS] = {calib_block_sum(s_nll, red), calib_block_sum(s_g, red), calib_block_sum(s_h, red),
                                       calib_block_sum((double)n_valid, red)};
    if (threadIdx.x == 0)
        for (int k = 0; k < CALIB_PART_ROWS; ++k) part[(size_t)k * nb + blockIdx.x] = v[k];
}

__global__ __launch_bounds__(256) void k_calib_newton_finish(const double* __restrict__ part, int nb, double* __restrict__ state) {
    double v[CALIB_PART_ROWS];
    calib_reduce_parts(part, nb, v);
    if (threadIdx.x == 0) {
        state[CALIB_STATE_L] += v[0];
        state[CALIB_STATE_G] += v[1];
        state[CALIB_STATE_H] += v[2];
        state[CALIB_STATE_N] += v[3];
    }
}

// One thread.  Row k of the log: [tau used, n, NLL, g, h, tau next, lo, hi] (lo, hi after the update).  final != 0: no update, tau
// next = tau.  The sums are zeroed either way.  A row past the log's end is not written.
__global__ void k_calib_newton_step(double* __restrict__ state, double* __restrict__ log, int log_rows, int final_pass) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double tau = state[CALIB_STATE_TAU], n = state[CALIB_STATE_N];
    double lo = state[CALIB_STATE_LO], hi = state[CALIB_STATE_HI];
    const double L = state[CALIB_STATE_L] / n, g = state[CALIB_STATE_G] / n, h = state[CALIB_STATE_H] / n;
    double next = tau;
    if (!final_pass && n > 0.0) {
        if (g < 0.0) lo = tau;
        else if (g > 0.0) hi = tau;
        const bool newton = h > 1e-12;
        double cand = newton ? tau - g / h : 0.0;
        if (!newton || !(cand > lo && cand < hi)) cand = sqrt(lo * hi);
        next = (double)(float)cand;
    }
    const int k = (int)state[CALIB_STATE_K];
    if (k >= 0 && k < log_rows) {
        double* row = log + (size_t)k * CALIB_LOG_COLUMNS;
        row[0] = tau; row[1] = n; row[2] = L; row[3] = g; row[4] = h; row[5] = next; row[6] = lo; row[7] = hi;
    }
    state[CALIB_STATE_TAU] = next;
    state[CALIB_STATE_LO] = lo;
    state[CALIB_STATE_HI] = hi;
    state[CALIB_STATE_G] = 0.0;
    state[CALIB_STATE_H] = 0.0;
    state[CALIB_STATE_L] = 0.0;
    state[CALIB_STATE_N] = 0.0;
    state[CALIB_STATE_K] = (double)(k + 1);
    *reinterpret_cast<float*>(state + CALIB_STATE_TAU32) = (float)next;
}

}  // namespace

// rows of ld floats staged beside `table_bytes` of LDS table
static bool calib_staged(int ld, size_t table_bytes) {
    return ld <= CE_MAX_LD && table_bytes + (size_t)CE_CHUNK * (ld + 1) * sizeof(float) <= (size_t)CALIB_LDS_BYTES;
}

extern "C" int cvk_calib_accumulate(const float* logits, int ld, const int64_t* target, const float* tau, int64_t* hist, double* part,
                                    void* record, float* conf, int64_t* pred, int M, int C, int bins, int ignore_index, void* stream) {
    CVK_CHECK_ARG(logits, "cvk_calib_accumulate: null pointer");
    const bool tables = hist != nullptr;
    CVK_CHECK_ARG(tables ? (target && part && record) : (!target && !part && !record),
                  "cvk_calib_accumulate: null pointer (hist, target, part and record go together)");
    CVK_CHECK_ARG(tables || conf || pred, "cvk_calib_accumulate: null pointer (no table and no map to write)");
    CVK_CHECK_ARG(M > 0 && C >= 1 && C <= CALIB_MAX_C, "cvk_calib_accumulate: bad arguments (M > 0 and 1 <= C <= 128)");
    CVK_CHECK_ARG(ld >= C, "cvk_calib_accumulate: the pixel stride is smaller than C");
    if (tables) {
        CVK_CHECK_ARG(bins >= 1 && bins <= CALIB_MAX_B, "cvk_calib_accumulate: bad arguments (1 <= bins <= 64)");
        CVK_CHECK_ARG(C * bins <= CALIB_MAX_CELLS, "cvk_calib_accumulate: C * bins exceeds 2048 (48 KiB of LDS table)");
    }
    const int nb = cvk_ce_blocks(M);
    const size_t table_bytes = tables ? (size_t)C * bins * 3 * sizeof(unsigned long long) : 0;
    hipStream_t s = (hipStream_t)stream;
    if (calib_staged(ld, table_bytes))
        hipLaunchKernelGGL(k_calib_accumulate<true>, dim3(nb), dim3(256), table_bytes + (size_t)CE_CHUNK * (ld + 1) * sizeof(float), s, logits,
                           ld, target, tau, (unsigned long long*)hist, part, nb, conf, pred, M, C, bins, ignore_index);
    else
        hipLaunchKernelGGL(k_calib_accumulate<false>, dim3(nb), dim3(256), table_bytes, s, logits, ld, target, tau,
                           (unsigned long long*)hist, part, nb, conf, pred, M, C, bins, ignore_index);
    if (tables) hipLaunchKernelGGL(k_calib_finish, dim3(1), dim3(256), 0, s, part, nb, (long long*)record);
    CVK_LAUNCH_RETURN("cvk_calib_accumulate");
}

extern "C" int cvk_calib_newton_accumulate(const float* logits, int ld, const int64_t* target, double* state, double* part, int M, int C,
                                           int ignore_index, void* stream) {
    CVK_CHECK_ARG(logits && target && state && part, "cvk_calib_newton_accumulate: null pointer");
    CVK_CHECK_ARG(M > 0 && C >= 1 && C <= CALIB_MAX_C, "cvk_calib_newton_accumulate: bad arguments (M > 0 and 1 <= C <= 128)");
    CVK_CHECK_ARG(ld >= C, "cvk_calib_newton_accumulate: the pixel stride is smaller than C");
    const int nb = cvk_ce_blocks(M);
    hipStream_t s = (hipStream_t)stream;
    if (calib_staged(ld, 0))
        hipLaunchKernelGGL(k_calib_newton<true>, dim3(nb), dim3(256), (size_t)CE_CHUNK * (ld + 1) * sizeof(float), s, logits, ld, target, state,
                           part, nb, M, C, ignore_index);
    else
        hipLaunchKernelGGL(k_calib_newton<false>, dim3(nb), dim3(256), 0, s, logits, ld, target, state, part, nb, M, C, ignore_index);
    hipLaunchKernelGGL(k_calib_newton_finish, dim3(1), dim3(256), 0, s, part, nb, state);
    CVK_LAUNCH_RETURN("cvk_calib_newton_accumulate");
}

extern "C" int cvk_calib_newton_step(double* state, double* log, int log_rows, int final_pass, void* stream) {
    CVK_CHECK_ARG(state && log, "cvk_calib_newton_step: null pointer");
    CVK_CHECK_ARG(log_rows >= 1, "cvk_calib_newton_step: bad arguments (log_rows >= 1)");
    hipLaunchKernelGGL(k_calib_newton_step, dim3(1), dim3(64), 0, (hipStream_t)stream, state, log, log_rows, final_pass);
    CVK_LAUNCH_RETURN("cvk_calib_newton_step");
}
