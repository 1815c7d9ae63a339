#pragma once
// loss_ce.h: softmax cross-entropy (nn.CrossEntropyLoss(), reference train.py:105,130-131; cvk_softmax_ce_fwd / _bwd), then the same with
// class weights, label smoothing and a reduction (cvk_softmax_ce_fwd_ex / _bwd_ex).  The workgroup geometry, the chunk staging and the
// weighted pixel terms come from loss_rows.h, where the other losses find them too.
#include "cvk_common.h"
#include "loss_rows.h"

namespace {

// part[b] = sum of -log softmax(logits)[target] over the block's valid pixels, part[nb + b] = number of valid pixels,
// part[2 nb + b] = number of pixels whose target is neither in [0, C) nor ignore_index.
__global__ __launch_bounds__(256) void k_ce_fwd(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                               float* __restrict__ part, int nb, int M, int C, int ignore_index) {
    extern __shared__ float lds[];
    __shared__ float red[4];
    const int pitch = ld + 1;
    float acc = 0.f, cnt = 0.f, bad = 0.f;
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK;
    for (int ch = 0; ch < CE_ROWS_PER_BLOCK / CE_CHUNK; ++ch) {
        const int m0 = base + ch * CE_CHUNK;
        if (m0 >= M) break;
        const int rows = min(CE_CHUNK, M - m0);
        __syncthreads();
        ce_chunk_load(logits + (size_t)m0 * ld, lds, rows * ld, ld);
        __syncthreads();
        if ((int)threadIdx.x < rows) {
            const float* p = lds + threadIdx.x * pitch;
            const long t = (long)target[m0 + threadIdx.x];
            if (t != (long)ignore_index) {
                float mx = p[0];
                for (int c = 1; c < C; ++c) mx = fmaxf(mx, p[c]);
                float se = 0.f;
                for (int c = 0; c < C; ++c) se += expf(p[c] - mx);
                if (t >= 0 && t < C) {
                    acc += (mx + logf(se)) - p[t];
                    cnt += 1.f;
                } else {
                    bad += 1.f;
                }
            }
        }
    }
    const float s = block_sum_256(acc, red);
    const float n = block_sum_256(cnt, red);
    const float b = block_sum_256(bad, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s;
        part[nb + blockIdx.x] = n;
        part[2 * nb + blockIdx.x] = b;
    }
}

// loss[0] = mean over the valid pixels (NaN when a target was out of range: nn.CrossEntropyLoss raises there),
// loss[1] = number of valid pixels (the backward's divisor), loss[2] = number of out-of-range targets.
__global__ __launch_bounds__(256) void k_ce_finish(const float* __restrict__ part, int nb, float* loss) {
    __shared__ double red[3][256];
    double a = 0.0, n = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) {
        a += (double)part[i];
        n += (double)part[nb + i];
        b += (double)part[2 * nb + i];
    }
    red[0][threadIdx.x] = a; red[1][threadIdx.x] = n; red[2][threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o)
            for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[0] = red[2][0] > 0.0 ? __builtin_nanf("") : (float)(red[0][0] / red[1][0]);   // 0/0 = NaN when every pixel is ignored (as torch)
        loss[1] = (float)red[1][0];
        loss[2] = (float)red[2][0];
    }
}

__global__ __launch_bounds__(256) void k_ce_bwd(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                               const float* __restrict__ loss3, const float* __restrict__ grad_out, float scale,
                                               float* __restrict__ dl, int ld_d, int M, int C, int ignore_index) {
    extern __shared__ float lds[];
    const int pitch = ld + 1;
    const float g = (grad_out != nullptr ? *grad_out : 1.f) * scale / loss3[1];
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK;
    for (int ch = 0; ch < CE_ROWS_PER_BLOCK / CE_CHUNK; ++ch) {
        const int m0 = base + ch * CE_CHUNK;
        if (m0 >= M) break;
        const int rows = min(CE_CHUNK, M - m0);
        __syncthreads();
        ce_chunk_load(logits + (size_t)m0 * ld, lds, rows * ld, ld);
        __syncthreads();
        if ((int)threadIdx.x < rows) {
            float* p = lds + threadIdx.x * pitch;
            const long t = (long)target[m0 + threadIdx.x];
            if (t == (long)ignore_index) {
                for (int c = 0; c < ld; ++c) p[c] = 0.f;
            } else {
                float mx = p[0];
                for (int c = 1; c < C; ++c) mx = fmaxf(mx, p[c]);
                float se = 0.f;
                for (int c = 0; c < C; ++c) se += expf(p[c] - mx);
                const float inv = 1.f / se;
                for (int c = 0; c < C; ++c) p[c] = (expf(p[c] - mx) * inv - ((long)c == t ? 1.f : 0.f)) * g;
                for (int c = C; c < ld; ++c) p[c] = 0.f;
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

// Wide pixel rows (ld > CE_MAX_LD floats, i.e. 64 classes or more): the LDS-staged kernels above would need more than 64 KiB of
// dynamic LDS, so one thread walks its pixel's row in global memory (reference train.py:105 puts no bound on class_num).
__global__ __launch_bounds__(256) void k_ce_fwd_rows(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                    float* __restrict__ part, int nb, int M, int C, int ignore_index) {
    __shared__ float red[4];
    float acc = 0.f, cnt = 0.f, bad = 0.f;
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK;
    for (int m = base + threadIdx.x; m < min(M, base + CE_ROWS_PER_BLOCK); m += CE_CHUNK) {
        const float* p = logits + (size_t)m * ld;
        const long t = (long)target[m];
        if (t == (long)ignore_index) continue;
        float mx = p[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, p[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(p[c] - mx);
        if (t >= 0 && t < C) {
            acc += (mx + logf(se)) - p[t];
            cnt += 1.f;
        } else {
            bad += 1.f;
        }
    }
    const float s = block_sum_256(acc, red);
    const float n = block_sum_256(cnt, red);
    const float b = block_sum_256(bad, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s;
        part[nb + blockIdx.x] = n;
        part[2 * nb + blockIdx.x] = b;
    }
}

__global__ __launch_bounds__(256) void k_ce_bwd_rows(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                    const float* __restrict__ loss3, const float* __restrict__ grad_out, float scale,
                                                    float* __restrict__ dl, int ld_d, int M, int C, int ignore_index) {
    const float g = (grad_out != nullptr ? *grad_out : 1.f) * scale / loss3[1];
    for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (long)gridDim.x * blockDim.x) {
        const float* p = logits + (size_t)m * ld;
        float* o = dl + (size_t)m * ld_d;
        const long t = (long)target[m];
        if (t == (long)ignore_index) {
            for (int c = 0; c < ld_d; ++c) o[c] = 0.f;
            continue;
        }
        float mx = p[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, p[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(p[c] - mx);
        const float inv = 1.f / se;
        for (int c = 0; c < C; ++c) o[c] = (expf(p[c] - mx) * inv - ((long)c == t ? 1.f : 0.f)) * g;
        for (int c = C; c < ld_d; ++c) o[c] = 0.f;
    }
}

// ---- cross-entropy with class weights, label smoothing and a reduction (cvk_softmax_ce_fwd_ex / _bwd_ex) ----------------------
// Same memory scheme as k_ce_fwd / k_ce_bwd (256 pixel rows staged per chunk, one thread per pixel; a thread walks its row in
// global memory when ld > CE_MAX_LD); the weight vector (all ones when absent) is staged in LDS once per workgroup.
// The pixel terms (CE_EX_MAX_C, ce_ex_stage_w, ce_ex_pixel_loss, ce_ex_pixel_grad) are in loss_rows.h: the other losses use them too.

// part[b], part[nb + b], part[2 nb + b], part[3 nb + b] = the block's loss sum, divisor sum (w[t] over the valid pixels), valid
// pixels, out-of-range targets.  loss_px (nullable): per-pixel loss, 0 at ignored pixels and NaN at out-of-range targets.
__global__ __launch_bounds__(256) void k_ce_fwd_ex(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                  const float* __restrict__ weight, float eps, float* __restrict__ part, int nb,
                                                  float* __restrict__ loss_px, int M, int C, int ignore_index) {
    extern __shared__ float lds[];
    __shared__ float red[4];
    __shared__ float s_w[CE_EX_MAX_C];
    ce_ex_stage_w(weight, s_w, C);                                   // visible after the first chunk's barriers
    const int pitch = ld + 1;
    float acc = 0.f, div = 0.f, cnt = 0.f, bad = 0.f;
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK;
    for (int ch = 0; ch < CE_ROWS_PER_BLOCK / CE_CHUNK; ++ch) {
        const int m0 = base + ch * CE_CHUNK;
        if (m0 >= M) break;
        const int rows = min(CE_CHUNK, M - m0);
        __syncthreads();
        ce_chunk_load(logits + (size_t)m0 * ld, lds, rows * ld, ld);
        __syncthreads();
        if ((int)threadIdx.x < rows) {
            const long t = (long)target[m0 + threadIdx.x];
            float l = 0.f;
            if (t != (long)ignore_index) {
                if (t >= 0 && t < C) {
                    l = ce_ex_pixel_loss(lds + threadIdx.x * pitch, C, (int)t, s_w, eps);
                    acc += l;
                    div += s_w[t];
                    cnt += 1.f;
                } else {
                    l = __builtin_nanf("");
                    bad += 1.f;
                }
            }
            if (loss_px != nullptr) loss_px[m0 + threadIdx.x] = l;
        }
    }
    const float s = block_sum_256(acc, red);
    const float d = block_sum_256(div, red);
    const float n = block_sum_256(cnt, red);
    const float b = block_sum_256(bad, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s;
        part[nb + blockIdx.x] = d;
        part[2 * nb + blockIdx.x] = n;
        part[3 * nb + blockIdx.x] = b;
    }
}

__global__ __launch_bounds__(256) void k_ce_fwd_ex_rows(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                       const float* __restrict__ weight, float eps, float* __restrict__ part, int nb,
                                                       float* __restrict__ loss_px, int M, int C, int ignore_index) {
    __shared__ float red[4];
    __shared__ float s_w[CE_EX_MAX_C];
    ce_ex_stage_w(weight, s_w, C);
    __syncthreads();
    float acc = 0.f, div = 0.f, cnt = 0.f, bad = 0.f;
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK;
    for (int m = base + threadIdx.x; m < min(M, base + CE_ROWS_PER_BLOCK); m += CE_CHUNK) {
        const long t = (long)target[m];
        float l = 0.f;
        if (t != (long)ignore_index) {
            if (t >= 0 && t < C) {
                l = ce_ex_pixel_loss(logits + (size_t)m * ld, C, (int)t, s_w, eps);
                acc += l;
                div += s_w[t];
                cnt += 1.f;
            } else {
                l = __builtin_nanf("");
                bad += 1.f;
            }
        }
        if (loss_px != nullptr) loss_px[m] = l;
    }
    const float s = block_sum_256(acc, red);
    const float d = block_sum_256(div, red);
    const float n = block_sum_256(cnt, red);
    const float b = block_sum_256(bad, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s;
        part[nb + blockIdx.x] = d;
        part[2 * nb + blockIdx.x] = n;
        part[3 * nb + blockIdx.x] = b;
    }
}

// Fixed-order fp64 reduction of the four partial rows: loss[0] = the reduced loss (mean: sum / divisor, 0/0 = NaN; sum and none:
// the sum; NaN when a target was out of range), loss[1] = valid pixels, loss[2] = out-of-range targets, loss[3] = the backward's
// divisor (mean: sum of w[t] over the valid pixels; sum and none: 1).
__global__ __launch_bounds__(256) void k_ce_finish_ex(const float* __restrict__ part, int nb, int reduction, float* loss) {
    __shared__ double red[4][256];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nb; i += 256)
        for (int k = 0; k < 4; ++k) v[k] += (double)part[k * nb + i];
    for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o)
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool mean = reduction == CVK_REDUCTION_MEAN;
        loss[0] = red[3][0] > 0.0 ? __builtin_nanf("") : (float)(mean ? red[0][0] / red[1][0] : red[0][0]);
        loss[1] = (float)red[2][0];
        loss[2] = (float)red[3][0];
        loss[3] = mean ? (float)red[1][0] : 1.f;
    }
}

// grad_out: one value per pixel for reduction 'none', else a scalar (nullptr = 1).  Ignored pixels and out-of-range targets get a
// zero gradient row.
__global__ __launch_bounds__(256) void k_ce_bwd_ex(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                  const float* __restrict__ weight, float eps, int reduction,
                                                  const float* __restrict__ loss4, const float* __restrict__ grad_out, float scale,
                                                  float* __restrict__ dl, int ld_d, int M, int C, int ignore_index) {
    extern __shared__ float lds[];
    __shared__ float s_w[CE_EX_MAX_C];
    ce_ex_stage_w(weight, s_w, C);
    __syncthreads();
    float wsum = 0.f;
    for (int c = 0; c < C; ++c) wsum += s_w[c];
    const bool per_px = reduction == CVK_REDUCTION_NONE;
    const float g0 = (per_px || grad_out == nullptr ? 1.f : *grad_out) * scale / loss4[3];
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
            float* p = lds + threadIdx.x * pitch;
            const long t = (long)target[m0 + threadIdx.x];
            if (t == (long)ignore_index || t < 0 || t >= C) {
                for (int c = 0; c < ld; ++c) p[c] = 0.f;
            } else {
                const float g = per_px ? g0 * grad_out[m0 + threadIdx.x] : g0;
                ce_ex_pixel_grad(p, p, ld, C, (int)t, s_w, eps, wsum, g);
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

__global__ __launch_bounds__(256) void k_ce_bwd_ex_rows(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                       const float* __restrict__ weight, float eps, int reduction,
                                                       const float* __restrict__ loss4, const float* __restrict__ grad_out, float scale,
                                                       float* __restrict__ dl, int ld_d, int M, int C, int ignore_index) {
    __shared__ float s_w[CE_EX_MAX_C];
    ce_ex_stage_w(weight, s_w, C);
    __syncthreads();
    float wsum = 0.f;
    for (int c = 0; c < C; ++c) wsum += s_w[c];
    const bool per_px = reduction == CVK_REDUCTION_NONE;
    const float g0 = (per_px || grad_out == nullptr ? 1.f : *grad_out) * scale / loss4[3];
    for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (long)gridDim.x * blockDim.x) {
        float* o = dl + (size_t)m * ld_d;
        const long t = (long)target[m];
        if (t == (long)ignore_index || t < 0 || t >= C) {
            for (int c = 0; c < ld_d; ++c) o[c] = 0.f;
            continue;
        }
        const float g = per_px ? g0 * grad_out[m] : g0;
        ce_ex_pixel_grad(logits + (size_t)m * ld, o, ld_d, C, (int)t, s_w, eps, wsum, g);
    }
}

}  // namespace

extern "C" int cvk_softmax_ce_fwd(const float* logits, int ld, const int64_t* target, float* part, float* loss, int M, int C,
                                  int ignore_index, void* stream) {
    CVK_CHECK_ARG(logits && target && part && loss && M > 0 && C > 0 && ld >= C, "cvk_softmax_ce_fwd: bad arguments");
    const int nb = cvk_ce_blocks(M);
    hipStream_t s = (hipStream_t)stream;
    if (ld <= CE_MAX_LD)
        hipLaunchKernelGGL(k_ce_fwd, dim3(nb), dim3(256), CE_CHUNK * (ld + 1) * sizeof(float), s, logits, ld, target, part, nb, M, C, ignore_index);
    else
        hipLaunchKernelGGL(k_ce_fwd_rows, dim3(nb), dim3(256), 0, s, logits, ld, target, part, nb, M, C, ignore_index);
    hipLaunchKernelGGL(k_ce_finish, dim3(1), dim3(256), 0, s, part, nb, loss);
    CVK_LAUNCH_RETURN("cvk_softmax_ce_fwd");
}

extern "C" int cvk_softmax_ce_bwd(const float* logits, int ld, const int64_t* target, const float* loss3, const float* grad_out,
                                  float scale, float* dlogits, int ld_d, int M, int C, int ignore_index, void* stream) {
    CVK_CHECK_ARG(logits && target && loss3 && dlogits && M > 0 && C > 0 && ld >= C && ld_d >= C, "cvk_softmax_ce_bwd: bad arguments");
    if (ld <= CE_MAX_LD)
        hipLaunchKernelGGL(k_ce_bwd, dim3(cvk_ce_blocks(M)), dim3(256), CE_CHUNK * (ld + 1) * sizeof(float), (hipStream_t)stream, logits, ld,
                           target, loss3, grad_out, scale, dlogits, ld_d, M, C, ignore_index);
    else
        hipLaunchKernelGGL(k_ce_bwd_rows, dim3(cvk_cdiv(M, 256) < 8192 ? cvk_cdiv(M, 256) : 8192), dim3(256), 0, (hipStream_t)stream, logits, ld,
                           target, loss3, grad_out, scale, dlogits, ld_d, M, C, ignore_index);
    CVK_LAUNCH_RETURN("cvk_softmax_ce_bwd");
}

extern "C" int cvk_ce_ex_part_floats(int M) { return M > 0 ? 4 * cvk_ce_blocks(M) : 0; }

static bool ce_ex_args_ok(int M, int C, int ld, float eps, int reduction) {
    return M > 0 && C > 0 && C <= CE_EX_MAX_C && ld >= C && eps >= 0.f && eps <= 1.f &&
           (reduction == CVK_REDUCTION_NONE || reduction == CVK_REDUCTION_MEAN || reduction == CVK_REDUCTION_SUM);
}

extern "C" int cvk_softmax_ce_fwd_ex(const float* logits, int ld, const int64_t* target, const float* weight, float label_smoothing,
                                     int reduction, float* part, float* loss, float* loss_px, int M, int C, int ignore_index,
                                     void* stream) {
    CVK_CHECK_ARG(logits && target && part && loss, "cvk_softmax_ce_fwd_ex: null pointer");
    CVK_CHECK_ARG(ce_ex_args_ok(M, C, ld, label_smoothing, reduction), "cvk_softmax_ce_fwd_ex: bad arguments");
    CVK_CHECK_ARG(reduction != CVK_REDUCTION_NONE || loss_px, "cvk_softmax_ce_fwd_ex: reduction none needs loss_px");
    const int nb = cvk_ce_blocks(M);
    hipStream_t s = (hipStream_t)stream;
    if (ld <= CE_MAX_LD)
        hipLaunchKernelGGL(k_ce_fwd_ex, dim3(nb), dim3(256), CE_CHUNK * (ld + 1) * sizeof(float), s, logits, ld, target, weight,
                           label_smoothing, part, nb, loss_px, M, C, ignore_index);
    else
        hipLaunchKernelGGL(k_ce_fwd_ex_rows, dim3(nb), dim3(256), 0, s, logits, ld, target, weight, label_smoothing, part, nb, loss_px, M,
                           C, ignore_index);
    hipLaunchKernelGGL(k_ce_finish_ex, dim3(1), dim3(256), 0, s, part, nb, reduction, loss);
    CVK_LAUNCH_RETURN("cvk_softmax_ce_fwd_ex");
}

extern "C" int cvk_softmax_ce_bwd_ex(const float* logits, int ld, const int64_t* target, const float* weight, float label_smoothing,
                                     int reduction, const float* loss4, const float* grad_out, float scale, float* dlogits, int ld_d,
                                     int M, int C, int ignore_index, void* stream) {
    CVK_CHECK_ARG(logits && target && loss4 && dlogits, "cvk_softmax_ce_bwd_ex: null pointer");
    CVK_CHECK_ARG(ce_ex_args_ok(M, C, ld, label_smoothing, reduction) && ld_d >= C, "cvk_softmax_ce_bwd_ex: bad arguments");
    CVK_CHECK_ARG(reduction != CVK_REDUCTION_NONE || grad_out, "cvk_softmax_ce_bwd_ex: reduction none needs a per-pixel grad_out");
    hipStream_t s = (hipStream_t)stream;
    if (ld <= CE_MAX_LD)
        hipLaunchKernelGGL(k_ce_bwd_ex, dim3(cvk_ce_blocks(M)), dim3(256), CE_CHUNK * (ld + 1) * sizeof(float), s, logits, ld, target,
                           weight, label_smoothing, reduction, loss4, grad_out, scale, dlogits, ld_d, M, C, ignore_index);
    else
        hipLaunchKernelGGL(k_ce_bwd_ex_rows, dim3(cvk_cdiv(M, 256) < 8192 ? cvk_cdiv(M, 256) : 8192), dim3(256), 0, s, logits, ld, target,
                           weight, label_smoothing, reduction, loss4, grad_out, scale, dlogits, ld_d, M, C, ignore_index);
    CVK_LAUNCH_RETURN("cvk_softmax_ce_bwd_ex");
}
