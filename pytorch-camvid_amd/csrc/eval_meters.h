#pragma once
// eval_meters.h: the evaluation reductions.  Class statistics of label masks (cvk_class_histogram), the per-pixel arg-max
// (cvk_argmax_channels: reference train.py:191) and the intersection / union histograms (cvk_confusion_accumulate: reference
// utils.py:162-190).  Every count is an integer atomic.
#include "cvk_common.h"

namespace {

// ---- class statistics of label masks (cvk_class_histogram) ---------------------------------------------------------------------------
// Class statistics of label masks: one workgroup per mask.  Every wave counts into its own LDS histogram (integer atomics:
// exact, so the totals do not depend on the order); the folded per-mask counts go to the device counters with 64-bit integer
// atomics: hist[c] += pixels of class c, hist[C + c] += the mask's counted pixels if c occurs in it, hist[2C] += labels outside
// [0, C) that are not ignore_index.
constexpr int HIST_THREADS = 1024, HIST_WAVES = HIST_THREADS / 64, HIST_MAX_C = 256;

__global__ __launch_bounds__(HIST_THREADS) void k_class_hist(const void* __restrict__ masks, int mask_bytes, int64_t hw, int C,
                                                             int ignore_index, unsigned long long* __restrict__ hist) {
    __shared__ unsigned int h[HIST_WAVES * HIST_MAX_C];
    __shared__ unsigned long long cnt[HIST_MAX_C];
    __shared__ unsigned long long s_tot;
    __shared__ unsigned int s_bad;
    for (int i = threadIdx.x; i < HIST_WAVES * C; i += HIST_THREADS) h[i] = 0u;
    if (threadIdx.x == 0) s_bad = 0u;
    __syncthreads();
    unsigned int* mine = h + (threadIdx.x >> 6) * C;
    const size_t base = (size_t)blockIdx.x * hw;
    unsigned int bad = 0u;
    for (int64_t i = threadIdx.x; i < hw; i += HIST_THREADS) {
        const long l = mask_bytes == 1 ? (long)static_cast<const uint8_t*>(masks)[base + i]
                                       : (long)static_cast<const int64_t*>(masks)[base + i];
        if (l == (long)ignore_index) continue;
        if (l >= 0 && l < C) atomicAdd(&mine[l], 1u);
        else ++bad;
    }
    if (bad) atomicAdd(&s_bad, bad);
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += HIST_THREADS) {
        unsigned long long n = 0;
        for (int k = 0; k < HIST_WAVES; ++k) n += h[k * C + c];
        cnt[c] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tot = 0;
        for (int c = 0; c < C; ++c) tot += cnt[c];
        s_tot = tot;
        if (s_bad) atomicAdd(&hist[2 * C], (unsigned long long)s_bad);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += HIST_THREADS) {
        if (cnt[c]) {
            atomicAdd(&hist[c], cnt[c]);
            atomicAdd(&hist[C + c], s_tot);
        }
    }
}

// ---- arg-max over the channels of a pixel row (cvk_argmax_channels) -----------------------------------------------------------------
__global__ void k_argmax(const float* __restrict__ logits, int ld, int64_t* __restrict__ out, int M, int C) {
    for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (long)gridDim.x * blockDim.x) {
        const float* p = logits + (size_t)m * ld;
        float best = p[0];
        int bi = 0;
        for (int c = 1; c < C; ++c) {
            const float v = p[c];
            if (v > best || (v != v && best == best)) { best = v; bi = c; }  // first max; NaN wins like ATen
        }
        out[m] = bi;
    }
}

// ---- per-class correct / predicted / labelled pixel counts (cvk_confusion_accumulate): hist[3][K], LDS histogram per workgroup --------
__global__ __launch_bounds__(256) void k_confusion(const int64_t* __restrict__ pred, const int64_t* __restrict__ label,
                                                  unsigned long long* __restrict__ hist, int M, int K, int ignore) {
    extern __shared__ unsigned int h[];  // [3][K]
    for (int i = threadIdx.x; i < 3 * K; i += blockDim.x) h[i] = 0;
    __syncthreads();
    for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (long)gridDim.x * blockDim.x) {
        const int64_t l = label[m], p = pred[m];  // compared as 64-bit values: 2^32 + c is no class and 2^32 + ignore not the ignore index
        if (l == (int64_t)ignore) continue;
        if (p >= 0 && p < K) {
            atomicAdd(&h[K + p], 1u);
            if (p == l) atomicAdd(&h[p], 1u);
        }
        if (l >= 0 && l < K) atomicAdd(&h[2 * K + l], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * K; i += blockDim.x)
        if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

}  // namespace

extern "C" int cvk_class_histogram(const void* masks, int mask_bytes, int N, int64_t HW, int num_classes, int ignore_index,
                                   int64_t* hist, void* stream) {
    CVK_CHECK_ARG(masks && hist, "cvk_class_histogram: null pointer");
    CVK_CHECK_ARG((mask_bytes == 1 || mask_bytes == 8) && N > 0 && HW > 0 && num_classes > 0 && num_classes <= HIST_MAX_C,
                  "cvk_class_histogram: bad arguments");
    hipLaunchKernelGGL(k_class_hist, dim3(N), dim3(HIST_THREADS), 0, (hipStream_t)stream, masks, mask_bytes, HW, num_classes,
                       ignore_index, (unsigned long long*)hist);
    CVK_LAUNCH_RETURN("cvk_class_histogram");
}

extern "C" int cvk_argmax_channels(const float* logits, int ld, int64_t* out, int M, int C, void* stream) {
    CVK_CHECK_ARG(logits && out && M > 0 && C > 0 && ld >= C, "cvk_argmax_channels: bad arguments");
    const int blocks = cvk_cdiv(M, 256) < 8192 ? cvk_cdiv(M, 256) : 8192;
    hipLaunchKernelGGL(k_argmax, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, ld, out, M, C);
    CVK_LAUNCH_RETURN("cvk_argmax_channels");
}

extern "C" int cvk_confusion_accumulate(const int64_t* pred, const int64_t* label, int64_t* hist, int M, int num_classes,
                                        int ignore_index, void* stream) {
    CVK_CHECK_ARG(pred && label && hist && M > 0 && num_classes > 0 && num_classes <= 4096, "cvk_confusion_accumulate: bad arguments");
    const int blocks = cvk_cdiv(M, 1024) < 1024 ? cvk_cdiv(M, 1024) : 1024;
    hipLaunchKernelGGL(k_confusion, dim3(blocks), dim3(256), 3 * num_classes * sizeof(unsigned int), (hipStream_t)stream, pred, label,
                       (unsigned long long*)hist, M, num_classes, ignore_index);
    CVK_LAUNCH_RETURN("cvk_confusion_accumulate");
}
