#pragma once
// optim_flat.h: the optimizers over the flat parameter buffer.  Fused AdamW (torch.optim.AdamW: reference train.py:100,133) and
// momentum SGD over one range table, each eager or captured, with the clip coefficient and the weight EMA folded in, and the
// per-iteration log row.  plan_block0, the planners' shared step, is also used by grad_flat.h.
#include "cvk_common.h"

namespace {

// ---- AdamW (cvk_adamw_step, cvk_adamw_step_ranges / _dev) -----------------------------------------------------------------------------
// One AdamW element update (torch.optim.AdamW, decoupled weight decay).  Shared by k_adamw (scalars as kernel arguments) and the
// range-table kernel: one expression list, so they cannot round differently.
// coef scales the gradient on its way in (global-norm clipping: the record of cvk_grad_norm); an unclipped step passes 1.f, and
// x * 1.f is x.
// Returns the parameter value it stored, for the EMA that goes on with it in the register.
__device__ __forceinline__ float adamw_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, int64_t i, float lr, float b1, float b2, float eps, float wd,
                                              float bc1, float bc2_sqrt, float coef) {
    const float gi = g[i] * coef;
    float pi = p[i] * (1.f - lr * wd);
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi -= (lr / bc1) * (mi / denom);
    p[i] = pi;
    return pi;
}

__global__ void k_adamw(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                        int64_t n, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        adamw_update(p, g, m, v, i, lr, b1, b2, eps, wd, bc1, bc2_sqrt, 1.f);
}

// AdamW over a range table (cvk_adamw_step_ranges, cvk_adamw_step_ranges_dev): workgroup b serves the range whose block0 is the last one
// <= b (a uniform binary search over the table) and strides over it with that range's workgroups.  Ranges outside [0, n) or with a record
// index outside [0, nhyper) are skipped (cvk_adamw_plan_ranges refuses them on the host).  One kernel template, two compile-time choices:
//   SRC: where the hyper records and the EMA's alpha come from.  AdamwArgSource: kernel arguments (eager).  AdamwDevSource: device memory
//        the host rewrites between graph replays (uniform loads, once per thread, before the loop).
//   EMA: the thread that has stored an element's new value moves the average towards it, ema += alpha * (p_new - ema), from the
//        register: param is not read again, and elements outside every range are not touched in ema either.  Without it `ema` and
//        alpha are never read and the loop is the plain update.
// `clip` is the {total_norm, clip_coef} record of cvk_grad_norm, read once per thread, or null: coefficient 1.f.
struct AdamwArgRecords {
    cvk_adamw_hyper r[CVK_ADAMW_ARG_RECORDS];
};

struct AdamwArgSource {
    AdamwArgRecords recs;
    float a;
    __device__ __forceinline__ const cvk_adamw_hyper* records() const { return recs.r; }
    __device__ __forceinline__ float alpha() const { return a; }
};

struct AdamwDevSource {
    const cvk_adamw_hyper* recs;
    const float* a;
    __device__ __forceinline__ const cvk_adamw_hyper* records() const { return recs; }
    __device__ __forceinline__ float alpha() const { return *a; }
};

template <class SRC, bool EMA>
__global__ void k_adamw_ranges(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                               float* __restrict__ ema, int64_t n, const cvk_adamw_range* __restrict__ rt, int nr, const SRC src,
                               int nhyper, const float* __restrict__ clip) {
    const int b = blockIdx.x;
    int lo = 0, hi = nr - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rt[mid].block0 <= b) lo = mid;
        else hi = mid - 1;
    }
    const int64_t off = rt[lo].offset, len = rt[lo].length;
    const int hx = rt[lo].hyper, b0 = rt[lo].block0;
    const int nb = (lo + 1 < nr ? rt[lo + 1].block0 : (int)gridDim.x) - b0;
    if (off < 0 || len <= 0 || off + len > n || hx < 0 || hx >= nhyper || nb <= 0 || b < b0) return;
    const cvk_adamw_hyper* __restrict__ hyper = src.records();
    const float lr = hyper[hx].lr, b1 = hyper[hx].beta1, b2 = hyper[hx].beta2, eps = hyper[hx].eps, wd = hyper[hx].weight_decay;
    const float bc1 = hyper[hx].bc1, bc2_sqrt = hyper[hx].bc2_sqrt;
    const float coef = clip != nullptr ? clip[1] : 1.f;
    float alpha = 0.f;
    if constexpr (EMA) alpha = src.alpha();
    for (int64_t i = off + (int64_t)(b - b0) * blockDim.x + threadIdx.x; i < off + len; i += (int64_t)nb * blockDim.x) {
        const float pi = adamw_update(p, g, m, v, i, lr, b1, b2, eps, wd, bc1, bc2_sqrt, coef);
        if constexpr (EMA) {
            const float e = ema[i];
            ema[i] = e + alpha * (pi - e);
        }
    }
}

// ---- momentum SGD over the same range table (cvk_sgd_step_ranges / _dev) ---------------------------------------------------------------
// One momentum-SGD element update (torch.optim.SGD: coupled L2 weight decay, dampening, Nesterov), in fp32.  Shared by the eager and the
// captured instantiation of k_sgd_ranges: one expression list, so they cannot round differently (the convention of adamw_update).
// coef scales the gradient on its way in, as in adamw_update.  `mom` (momentum != 0 under MOM): the buffer is in use; `first` is torch's
// `momentum_buffer is None`: the buffer becomes the (decayed) gradient itself, not (1 - dampening) * d.  Without `mom`, buf is neither
// read nor written.  Returns the parameter value it stored, for the EMA that goes on with it in the register.
__device__ __forceinline__ float sgd_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, int64_t i,
                                            float lr, float momentum, float dampening, float wd, bool nesterov, bool first, bool mom,
                                            float coef) {
    const float pi = p[i];
    float d = g[i] * coef;
    d = d + wd * pi;
    if (mom) {
        const float b = first ? d : momentum * buf[i] + (1.f - dampening) * d;
        buf[i] = b;
        d = nesterov ? d + momentum * b : b;
    }
    const float pn = pi - lr * d;
    p[i] = pn;
    return pn;
}

// Momentum SGD over a range table (cvk_sgd_step_ranges, cvk_sgd_step_ranges_dev): the table, the workgroup-to-range search, the record
// sources (a cvk_sgd_hyper has the size of a cvk_adamw_hyper and travels in the same slots), the clip record and the EMA tail are those of
// k_adamw_ranges.  MOM false: no record uses a momentum buffer; `buf` is never read or written (3 passes over the range instead of 5).
// Under MOM a record whose momentum is 0 still leaves its ranges of `buf` alone, as torch keeps no buffer for such a group.
static_assert(sizeof(cvk_sgd_hyper) == sizeof(cvk_adamw_hyper), "cvk_sgd_hyper travels in the record slots of cvk_adamw_hyper");

template <class SRC, bool EMA, bool MOM>
__global__ void k_sgd_ranges(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, float* __restrict__ ema,
                             int64_t n, const cvk_adamw_range* __restrict__ rt, int nr, const SRC src, int nhyper,
                             const float* __restrict__ clip) {
    const int b = blockIdx.x;
    int lo = 0, hi = nr - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rt[mid].block0 <= b) lo = mid;
        else hi = mid - 1;
    }
    const int64_t off = rt[lo].offset, len = rt[lo].length;
    const int hx = rt[lo].hyper, b0 = rt[lo].block0;
    const int nb = (lo + 1 < nr ? rt[lo + 1].block0 : (int)gridDim.x) - b0;
    if (off < 0 || len <= 0 || off + len > n || hx < 0 || hx >= nhyper || nb <= 0 || b < b0) return;
    const cvk_sgd_hyper* __restrict__ hyper = reinterpret_cast<const cvk_sgd_hyper*>(src.records());
    const float lr = hyper[hx].lr, momentum = hyper[hx].momentum, dampening = hyper[hx].dampening, wd = hyper[hx].weight_decay;
    const bool nesterov = hyper[hx].nesterov != 0.f, first = hyper[hx].first != 0.f;
    const bool mom = MOM && momentum != 0.f;
    const float coef = clip != nullptr ? clip[1] : 1.f;
    float alpha = 0.f;
    if constexpr (EMA) alpha = src.alpha();
    for (int64_t i = off + (int64_t)(b - b0) * blockDim.x + threadIdx.x; i < off + len; i += (int64_t)nb * blockDim.x) {
        const float pi = sgd_update(p, g, buf, i, lr, momentum, dampening, wd, nesterov, first, mom, coef);
        if constexpr (EMA) {
            const float e = ema[i];
            ema[i] = e + alpha * (pi - e);
        }
    }
}

// ---- the per-iteration log row (cvk_step_log) ------------------------------------------------------------------------------------------
// One row [loss, lr, beta1, ||gw||_2, ||gb||_2] of the per-iteration log, with `rec` (the {total_norm, clip_coef} record of cvk_grad_norm)
// followed by its two floats, into ring[(*counter % capacity) * cols ..] (cols = 5 or 7), then ++*counter.
// One workgroup of 256 threads: thread t sums the squares of elements t, t + 256, ... in fp64, then a fixed tree over LDS.
constexpr int STEP_LOG_THREADS = 256;

__device__ __forceinline__ double block_sum_sq_f64(const float* __restrict__ x, int n, double* red) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += STEP_LOG_THREADS) {
        const double xi = (double)x[i];
        s += xi * xi;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = STEP_LOG_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();                                               // red is reused by the next reduction
    return r;
}

__global__ __launch_bounds__(STEP_LOG_THREADS) void k_step_log(const float* __restrict__ loss, const cvk_adamw_hyper* __restrict__ hyper,
                                                               const float* __restrict__ gw, int nw, const float* __restrict__ gb, int nb,
                                                               const float* __restrict__ rec, float* __restrict__ ring, int capacity,
                                                               int64_t* __restrict__ counter) {
    __shared__ double red[STEP_LOG_THREADS];
    const double sw = block_sum_sq_f64(gw, nw, red);
    const double sb = block_sum_sq_f64(gb, nb, red);
    if (threadIdx.x == 0) {
        const int64_t c = *counter;
        float* row = ring + (c % capacity) * (rec != nullptr ? 7 : 5);
        row[0] = *loss;
        row[1] = hyper->lr;
        row[2] = hyper->beta1;
        row[3] = (float)sqrt(sw);
        row[4] = (float)sqrt(sb);
        if (rec != nullptr) {
            row[5] = rec[0];
            row[6] = rec[1];
        }
        *counter = c + 1;
    }
}

}  // namespace

// bc1 = 1 - beta1^step, bc2_sqrt = sqrt(1 - beta2^step), evaluated on the HOST (glibc powf) for both AdamW entry points: a
// device powf need not round like the host's, and the captured update must be bitwise the eager one.
static void adamw_bias_corrections(float beta1, float beta2, int step, float* bc1, float* bc2_sqrt) {
    *bc1 = 1.f - powf(beta1, (float)step);
    *bc2_sqrt = sqrtf(1.f - powf(beta2, (float)step));
}

static int adamw_blocks(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (int)(b < 8192 ? b : 8192);
}

extern "C" int cvk_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int step, void* stream) {
    CVK_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && n > 0 && step >= 1, "cvk_adamw_step: bad arguments");
    float bc1, bc2s;
    adamw_bias_corrections(beta1, beta2, step, &bc1, &bc2s);
    hipLaunchKernelGGL(k_adamw, dim3(adamw_blocks(n)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n,
                       lr, beta1, beta2, eps, weight_decay, bc1, bc2s);
    CVK_LAUNCH_RETURN("cvk_adamw_step");
}

extern "C" int cvk_adamw_hyper_fill(float lr, float beta1, float beta2, float eps, float weight_decay, int step, cvk_adamw_hyper* out) {
    CVK_CHECK_ARG(out && step >= 1, "cvk_adamw_hyper_fill: bad arguments");
    out->lr = lr;
    out->beta1 = beta1;
    out->beta2 = beta2;
    out->eps = eps;
    out->weight_decay = weight_decay;
    adamw_bias_corrections(beta1, beta2, step, &out->bc1, &out->bc2_sqrt);
    return CVK_OK;
}

// The planners' shared step: every entry's first workgroup (block0) and the total.  An entry of `length` elements gets one workgroup per
// `per` elements, at most its share of the budget (one per `per` elements of the `total`, at most `cap`, shared in proportion to the
// lengths), at least one.  Returns the workgroup count, or -1 as soon as it reaches 2^30.
template <class ENTRY>
static int64_t plan_block0(ENTRY* e, int count, int64_t total, int64_t per, int64_t cap) {
    int64_t budget = (total + per - 1) / per;
    if (budget > cap) budget = cap;
    int64_t blocks = 0;
    for (int r = 0; r < count; ++r) {
        int64_t nb = (e[r].length + per - 1) / per;
        const int64_t share = (int64_t)(((__int128)budget * e[r].length + total - 1) / total);
        if (nb > share) nb = share;
        if (nb < 1) nb = 1;
        e[r].block0 = (int32_t)blocks;
        blocks += nb;
        if (blocks >= (1LL << 30)) return -1;
    }
    return blocks;
}

// Workgroups per range: as many as k_adamw would give the range's elements alone (one per 256, at most 8192 in all).
extern "C" int cvk_adamw_plan_ranges(cvk_adamw_range* ranges, int nranges, int64_t n, int nhyper) {
    CVK_CHECK_ARG(ranges && nranges > 0 && n > 0 && nhyper > 0, "cvk_adamw_plan_ranges: bad arguments");
    int64_t total = 0;
    for (int r = 0; r < nranges; ++r) {
        const cvk_adamw_range& e = ranges[r];
        CVK_CHECK_ARG(e.offset >= 0 && e.length > 0 && e.offset + e.length <= n, "cvk_adamw_plan_ranges: range %d [%lld, +%lld) outside the "
                      "buffer of %lld elements", r, (long long)e.offset, (long long)e.length, (long long)n);
        CVK_CHECK_ARG(e.hyper >= 0 && e.hyper < nhyper, "cvk_adamw_plan_ranges: range %d names record %d of %d", r, e.hyper, nhyper);
        total += e.length;
    }
    const int64_t blocks = plan_block0(ranges, nranges, total, 256, 8192);
    CVK_CHECK_ARG(blocks >= 0, "cvk_adamw_plan_ranges: too many workgroups");
    return (int)blocks;
}

// One launch of the range kernel: SRC and EMA pick the instantiation, the argument list is the same for all four.
template <class SRC>
static void adamw_ranges_launch(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                const cvk_adamw_range* ranges, int nranges, int nblocks, const SRC& src, int nhyper, const float* record,
                                void* stream) {
    if (ema != nullptr)
        hipLaunchKernelGGL((k_adamw_ranges<SRC, true>), dim3(nblocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq,
                           ema, n, ranges, nranges, src, nhyper, record);
    else
        hipLaunchKernelGGL((k_adamw_ranges<SRC, false>), dim3(nblocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq,
                           ema, n, ranges, nranges, src, nhyper, record);
}

extern "C" int cvk_adamw_step_ranges(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                     const cvk_adamw_range* ranges, int nranges, int nblocks, const cvk_adamw_hyper* hyper, int nhyper,
                                     const float* record, float alpha, void* stream) {
    CVK_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && ranges && hyper, "cvk_adamw_step_ranges: null pointer");
    CVK_CHECK_ARG(!ema || (alpha > 0.f && alpha <= 1.f), "cvk_adamw_step_ranges: alpha %g outside (0, 1]", (double)alpha);
    CVK_CHECK_ARG(n > 0 && nranges > 0 && nblocks >= nranges && nhyper > 0 && nhyper <= CVK_ADAMW_ARG_RECORDS,
                  "cvk_adamw_step_ranges: bad arguments (records: %d, at most %d)", nhyper, CVK_ADAMW_ARG_RECORDS);
    AdamwArgSource src = {};
    for (int i = 0; i < nhyper; ++i) src.recs.r[i] = hyper[i];
    src.a = alpha;
    adamw_ranges_launch(param, grad, exp_avg, exp_avg_sq, ema, n, ranges, nranges, nblocks, src, nhyper, record, stream);
    CVK_LAUNCH_RETURN("cvk_adamw_step_ranges");
}

// alpha (DEVICE, one float) is what the kernel reads, rewritten by the host between graph replays; alpha_host is the value the host is
// about to upload there (at a capture: the first one), checked here because the device value cannot be.
extern "C" int cvk_adamw_step_ranges_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                         const cvk_adamw_range* ranges, int nranges, int nblocks, const cvk_adamw_hyper* hyper, int nhyper,
                                         const float* record, const float* alpha, float alpha_host, void* stream) {
    CVK_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && ranges && hyper && (!ema || alpha), "cvk_adamw_step_ranges_dev: null pointer");
    CVK_CHECK_ARG(!ema || (alpha_host > 0.f && alpha_host <= 1.f), "cvk_adamw_step_ranges_dev: alpha %g outside (0, 1]", (double)alpha_host);
    CVK_CHECK_ARG(n > 0 && nranges > 0 && nblocks >= nranges && nhyper > 0, "cvk_adamw_step_ranges_dev: bad arguments");
    const AdamwDevSource src = {hyper, alpha};
    adamw_ranges_launch(param, grad, exp_avg, exp_avg_sq, ema, n, ranges, nranges, nblocks, src, nhyper, record, stream);
    CVK_LAUNCH_RETURN("cvk_adamw_step_ranges_dev");
}

// ---- momentum SGD over the same range table (torch.optim.SGD) ----------------------------------------------------------------------
extern "C" int cvk_sgd_hyper_fill(float lr, float momentum, float dampening, float weight_decay, int nesterov, int first,
                                  cvk_sgd_hyper* out) {
    CVK_CHECK_ARG(out, "cvk_sgd_hyper_fill: null pointer");
    CVK_CHECK_ARG(lr >= 0.f, "cvk_sgd_hyper_fill: lr %g must be >= 0", (double)lr);
    CVK_CHECK_ARG(momentum >= 0.f, "cvk_sgd_hyper_fill: momentum %g must be >= 0", (double)momentum);
    CVK_CHECK_ARG(weight_decay >= 0.f, "cvk_sgd_hyper_fill: weight_decay %g must be >= 0", (double)weight_decay);
    CVK_CHECK_ARG(!nesterov || (momentum > 0.f && dampening == 0.f), "cvk_sgd_hyper_fill: nesterov needs a momentum > 0 and zero dampening "
                  "(momentum %g, dampening %g)", (double)momentum, (double)dampening);
    out->lr = lr;
    out->momentum = momentum;
    out->dampening = dampening;
    out->weight_decay = weight_decay;
    out->nesterov = nesterov ? 1.f : 0.f;
    out->first = first ? 1.f : 0.f;
    out->reserved = 0.f;
    return CVK_OK;
}

// One launch of the SGD range kernel: SRC, EMA and MOM pick the instantiation, the argument list is the same for all eight.
template <class SRC, bool MOM>
static void sgd_ranges_launch(float* param, const float* grad, float* buf, float* ema, int64_t n, const cvk_adamw_range* ranges, int nranges,
                              int nblocks, const SRC& src, int nhyper, const float* record, void* stream) {
    if (ema != nullptr)
        hipLaunchKernelGGL((k_sgd_ranges<SRC, true, MOM>), dim3(nblocks), dim3(256), 0, (hipStream_t)stream, param, grad, buf, ema, n, ranges,
                           nranges, src, nhyper, record);
    else
        hipLaunchKernelGGL((k_sgd_ranges<SRC, false, MOM>), dim3(nblocks), dim3(256), 0, (hipStream_t)stream, param, grad, buf, ema, n, ranges,
                           nranges, src, nhyper, record);
}

extern "C" int cvk_sgd_step_ranges(float* param, const float* grad, float* momentum_buf, float* ema, int64_t n,
                                   const cvk_adamw_range* ranges, int nranges, int nblocks, const cvk_sgd_hyper* hyper, int nhyper,
                                   const float* record, float alpha, void* stream) {
    CVK_CHECK_ARG(param && grad && ranges && hyper, "cvk_sgd_step_ranges: null pointer");
    CVK_CHECK_ARG(!ema || (alpha > 0.f && alpha <= 1.f), "cvk_sgd_step_ranges: alpha %g outside (0, 1]", (double)alpha);
    CVK_CHECK_ARG(n > 0 && nranges > 0 && nblocks >= nranges && nhyper > 0 && nhyper <= CVK_ADAMW_ARG_RECORDS,
                  "cvk_sgd_step_ranges: bad arguments (records: %d, at most %d)", nhyper, CVK_ADAMW_ARG_RECORDS);
    AdamwArgSource src = {};
    for (int i = 0; i < nhyper; ++i) {
        CVK_CHECK_ARG(momentum_buf || hyper[i].momentum == 0.f, "cvk_sgd_step_ranges: null momentum buffer, but record %d has momentum %g", i,
                      (double)hyper[i].momentum);
        src.recs.r[i] = {hyper[i].lr, hyper[i].momentum, hyper[i].dampening, hyper[i].weight_decay, hyper[i].nesterov, hyper[i].first,
                         hyper[i].reserved};                          // the 7 floats in their slots (static_assert above the kernel)
    }
    src.a = alpha;
    if (momentum_buf != nullptr)
        sgd_ranges_launch<AdamwArgSource, true>(param, grad, momentum_buf, ema, n, ranges, nranges, nblocks, src, nhyper, record, stream);
    else
        sgd_ranges_launch<AdamwArgSource, false>(param, grad, momentum_buf, ema, n, ranges, nranges, nblocks, src, nhyper, record, stream);
    CVK_LAUNCH_RETURN("cvk_sgd_step_ranges");
}

// hyper and alpha as in cvk_adamw_step_ranges_dev.  The device records cannot be checked here: a null momentum_buf selects the kernel that
// never touches a buffer, whatever momentum they carry (FlatSGD captures it only while every group's momentum is 0 and GraphedStep
// refuses to replay after that changes).
extern "C" int cvk_sgd_step_ranges_dev(float* param, const float* grad, float* momentum_buf, float* ema, int64_t n,
                                       const cvk_adamw_range* ranges, int nranges, int nblocks, const cvk_sgd_hyper* hyper, int nhyper,
                                       const float* record, const float* alpha, float alpha_host, void* stream) {
    CVK_CHECK_ARG(param && grad && ranges && hyper && (!ema || alpha), "cvk_sgd_step_ranges_dev: null pointer");
    CVK_CHECK_ARG(!ema || (alpha_host > 0.f && alpha_host <= 1.f), "cvk_sgd_step_ranges_dev: alpha %g outside (0, 1]", (double)alpha_host);
    CVK_CHECK_ARG(n > 0 && nranges > 0 && nblocks >= nranges && nhyper > 0, "cvk_sgd_step_ranges_dev: bad arguments");
    const AdamwDevSource src = {reinterpret_cast<const cvk_adamw_hyper*>(hyper), alpha};
    if (momentum_buf != nullptr)
        sgd_ranges_launch<AdamwDevSource, true>(param, grad, momentum_buf, ema, n, ranges, nranges, nblocks, src, nhyper, record, stream);
    else
        sgd_ranges_launch<AdamwDevSource, false>(param, grad, momentum_buf, ema, n, ranges, nranges, nblocks, src, nhyper, record, stream);
    CVK_LAUNCH_RETURN("cvk_sgd_step_ranges_dev");
}

// record (the {total_norm, clip_coef} record of cvk_grad_norm) may be null: rows of 5 floats; with it, rows of 7.
extern "C" int cvk_step_log(const float* loss, const cvk_adamw_hyper* hyper, const float* gw, int nw, const float* gb, int nb,
                            const float* record, float* ring, int capacity, int64_t* counter, void* stream) {
    CVK_CHECK_ARG(loss && hyper && gw && gb && ring && counter, "cvk_step_log: null pointer");
    CVK_CHECK_ARG(nw > 0 && nb > 0 && capacity > 0, "cvk_step_log: bad arguments");
    hipLaunchKernelGGL(k_step_log, dim3(1), dim3(STEP_LOG_THREADS), 0, (hipStream_t)stream, loss, hyper, gw, nw, gb, nb, record, ring,
                       capacity, counter);
    CVK_LAUNCH_RETURN("cvk_step_log");
}
