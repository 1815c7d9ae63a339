#pragma once
// loss_rows.h: what the loss kernels share.  NHWC logits rows are [M][ld] with C valid classes; one thread per pixel reads its C
// contiguous logits (a wave covers 64 * ld contiguous floats: fully used cache lines).  Here: the workgroup geometry (CE_*), the
// 256-thread sum, the global <-> LDS movement of a chunk of pixel rows, and the weighted, label-smoothed pixel terms of
// k_ce_fwd_ex / k_ce_bwd_ex that OHEM, Lovász, the boundary, focal + Dice and distillation losses reuse; the inference merges
// borrow CE_CHUNK.  One kernel, k_lv_clear, because two subjects launch it (Lovász and the distance transform, edt.h).  One entry
// point, cvk_ce_blocks: the number of workgroups of that geometry, which the launches of every loss take as their grid.
#include "cvk_common.h"

namespace {

constexpr int CE_ROWS_PER_BLOCK = 1024;  // 4 chunks of 256 pixels per workgroup
constexpr int CE_CHUNK = 256;            // one pixel per thread per chunk
constexpr int CE_MAX_LD = 63;            // widest pixel row staged through LDS ((ld + 1) * 1 KiB of dynamic LDS <= 64 KiB)

__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// Global <-> LDS movement of one chunk: the chunk's CE_CHUNK pixel rows are `n` contiguous floats in HBM (rows of ld
// floats); every wave instruction moves 64 consecutive float4 (1 KiB, fully used lines).  In LDS a pixel row has pitch
// ld + 1 floats, so the per-thread row walk below (thread = pixel, column c) is bank-conflict free.
__device__ __forceinline__ void ce_chunk_load(const float* __restrict__ g, float* lds, int n, int ld) {
    const int pitch = ld + 1;
    if ((ld & 3) == 0 && ((uintptr_t)g & 15u) == 0) {
        for (int f = threadIdx.x * 4; f < n; f += CE_CHUNK * 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(g + f);
            const int r = f / ld, c = f - r * ld;                  // ld % 4 == 0: the four floats share a row
            float* q = lds + r * pitch + c;
            q[0] = v[0]; q[1] = v[1]; q[2] = v[2]; q[3] = v[3];
        }
    } else {
        for (int f = threadIdx.x; f < n; f += CE_CHUNK) {
            const int r = f / ld;
            lds[r * pitch + (f - r * ld)] = g[f];
        }
    }
}

__device__ __forceinline__ void ce_chunk_store(float* __restrict__ g, const float* lds, int n, int ld) {
    const int pitch = ld + 1;
    if ((ld & 3) == 0 && ((uintptr_t)g & 15u) == 0) {
        for (int f = threadIdx.x * 4; f < n; f += CE_CHUNK * 4) {
            const int r = f / ld, c = f - r * ld;
            const float* q = lds + r * pitch + c;
            const f32x4 v = {q[0], q[1], q[2], q[3]};
            *reinterpret_cast<f32x4*>(g + f) = v;
        }
    } else {
        for (int f = threadIdx.x; f < n; f += CE_CHUNK) {
            const int r = f / ld;
            g[f] = lds[r * pitch + (f - r * ld)];
        }
    }
}

// ---- the pixel terms of the weighted, label-smoothed cross-entropy (kernels: k_ce_fwd_ex / k_ce_bwd_ex) --------------------------------
// For a pixel with target t, lse = log sum exp and W = sum_c w[c]:
//   loss = (1 - eps) w[t] (lse - x[t]) + (eps / C) sum_c w[c] (lse - x[c])
//   dx_k = g (softmax_k ((1 - eps) w[t] + (eps / C) W) - (1 - eps) w[t] [k = t] - (eps / C) w[k])
constexpr int CE_EX_MAX_C = 128;

__device__ __forceinline__ void ce_ex_stage_w(const float* __restrict__ w, float* s_w, int C) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) s_w[c] = w != nullptr ? w[c] : 1.f;
}

__device__ __forceinline__ float ce_ex_pixel_loss(const float* p, int C, int t, const float* s_w, float eps) {
    float mx = p[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, p[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(p[c] - mx);
    const float lse = mx + logf(se);
    float l = (1.f - eps) * s_w[t] * (lse - p[t]);
    if (eps != 0.f) {
        float sm = 0.f;
        for (int c = 0; c < C; ++c) sm += s_w[c] * (lse - p[c]);
        l += (eps / (float)C) * sm;
    }
    return l;
}

// o may alias p (every column is read before it is written); columns [C, ld_o) are zeroed
__device__ __forceinline__ void ce_ex_pixel_grad(const float* p, float* o, int ld_o, int C, int t, const float* s_w, float eps,
                                                 float wsum, float g) {
    float mx = p[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, p[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(p[c] - mx);
    const float inv = 1.f / se;
    const float es = eps / (float)C, wt = (1.f - eps) * s_w[t];
    const float a = wt + es * wsum;
    for (int c = 0; c < C; ++c) o[c] = (expf(p[c] - mx) * inv * a - (c == t ? wt : 0.f) - es * s_w[c]) * g;
    for (int c = C; c < ld_o; ++c) o[c] = 0.f;
}

// zeroes n words: the counters of the Lovász loss, the presence words of the distance transform
__global__ __launch_bounds__(256) void k_lv_clear(unsigned* __restrict__ ctr, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) ctr[i] = 0u;
}

}  // namespace

extern "C" int cvk_ce_blocks(int M) { return M > 0 ? cvk_cdiv(M, CE_ROWS_PER_BLOCK) : 0; }
