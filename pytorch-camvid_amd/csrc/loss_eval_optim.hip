// loss_eval_optim.hip: the six losses (softmax cross-entropy: nn.CrossEntropyLoss(), reference train.py:105,130-131; OHEM; Lovász;
// boundary; focal + Dice; distillation), the two inference merges and image ingest: kernels in the namespace below, their entry
// points after it, then the library-wide pieces.  What the losses share is in loss_rows.h.
// Every other subject is a self-contained header (own includes, own namespace; kernels, argument checks and entry points together)
// compiled as part of this translation unit:
//   loss_rows.h     workgroup geometry, chunk staging and weighted pixel terms of the losses; k_lv_clear
//   edt.h           exact Euclidean distance transform of label maps
//   boundary_f1.h   boundary F1 contour map and counts
//   surface_dist.h  Hausdorff, HD95 and ASSD (uses edt.h and boundary_f1.h)
//   eval_meters.h   class histogram, arg-max, confusion counts
//   optim_flat.h    AdamW, momentum SGD, the per-iteration log row
//   grad_flat.h     global-norm clipping and gradient accumulation
//   crop_aug.h      crop training: class-balanced window selection, resize + crop + pad + blur + LUT + flip
//   components.h    connected components of a class map (union-find over tiles) and the removal of small regions
//   crf.h           local-window mean-field CRF refinement of a prediction (a register-blocked stencil over an LDS tile)
// A new subject gets a header of that kind, not lines here.
#include "cvk_common.h"
#include "loss_rows.h"
#include "edt.h"
#include "boundary_f1.h"
#include "surface_dist.h"
#include "boundary_iou.h"
#include "eval_meters.h"
#include "optim_flat.h"
#include "grad_flat.h"
#include "crop_aug.h"
#include "components.h"
#include "crf.h"

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

// ---- OHEM cross-entropy (cvk_ohem_ce_fwd / _bwd) ----------------------------------------------------------------------------------
// A valid pixel's unweighted loss l = lse - x[t] is >= 0 (sum exp >= 1, max >= x[t]), so its bits read as an unsigned integer order
// like the value.  A pixel is kept iff l > lam or l >= L, L = the k-th largest l over the valid pixels, k = min(min_kept, V).  L is
// found exactly by a three-level radix select over the key's bits 30..0 (11 + 10 + 10), all on the device:
//   k_ohem_fwd       one pass over the logits (the staging of k_ce_fwd_ex): loss_px[m] = l (-1 where ignored, NaN where the target is
//                    out of range: both fall outside the key range and so out of every histogram) and the histogram of the top digit
//   k_ohem_refine<2> over loss_px: every workgroup finds the top-digit bin that holds rank k by scanning the histogram from above,
//   k_ohem_refine<3> then counts the next digit of the keys with the prefix found so far; workgroup 0 leaves (bin, rank inside it)
//   k_ohem_reduce    resolves the last digit, applies the predicate, writes workgroup partials of sum w[t] l, sum w[t], kept, bad
//   k_ohem_finish    one workgroup, fp64 in fixed order, writes the record
// Histograms are integer atomics (LDS per workgroup, then the non-zero bins to global memory): exact counts, whatever the order.
// Scratch words: hist1[2048] | hist2[1024] | hist3[1024] | state[8] | partials float[4 nb]; k_ohem_clear zeroes the first three and
// the state on the stream at the start of every forward.
constexpr int OHEM_B1 = 2048, OHEM_B23 = 1024;
constexpr int OHEM_HIST_WORDS = OHEM_B1 + 2 * OHEM_B23;
constexpr int OHEM_STATE_WORDS = 8;        // b1, rank in b1, V, k | b2, rank in b2 | bits of L | spare
constexpr int OHEM_HEAD_WORDS = OHEM_HIST_WORDS + OHEM_STATE_WORDS;
constexpr int OHEM_RECORD_FLOATS = 8;
constexpr unsigned OHEM_KEY_MAX = 0x7f800000u;   // +inf: keys above are negative (ignored) or NaN
constexpr int OHEM_MAX_LD = 54;            // staged forward: (ld + 1) KiB of tile + 8 KiB of histogram stay under 64 KiB
constexpr int OHEM_REFINE_MAX_BLOCKS = 2048;

__device__ __forceinline__ float ohem_pixel_loss(const float* p, int C, long t, int ignore_index) {
    if (t == (long)ignore_index) return -1.f;
    if (t < 0 || t >= C) return __builtin_nanf("");
    float mx = p[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, p[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(p[c] - mx);
    return (mx + logf(se)) - p[t];         // ce_ex_pixel_loss with eps = 0 and w = 1
}

__device__ __forceinline__ void ohem_hist_zero(unsigned* s_h, int bins) {
    for (int b = threadIdx.x; b < bins; b += 256) s_h[b] = 0u;
}

// after a barrier: the workgroup's non-zero bins go to the global histogram
__device__ __forceinline__ void ohem_hist_flush(const unsigned* s_h, unsigned* __restrict__ hist, int bins) {
    for (int b = threadIdx.x; b < bins; b += 256)
        if (s_h[b]) atomicAdd(&hist[b], s_h[b]);
}

// The bin of hist[256 * PER] that holds rank k counted from the top, by all 256 threads: s_out[0] = the bin, s_out[1] = the rank
// inside it (1 = its largest key), s_out[2] = the histogram's total.  k = 0 (no valid pixel) leaves bin 0, rank 0.  `k_of` maps the
// total to the rank (the first level takes k = min(min_kept, V) from it).  Ends with a barrier.
template <int PER, class KOF>
__device__ __forceinline__ void ohem_locate(const unsigned* __restrict__ hist, KOF k_of, unsigned* s_scan, unsigned* s_out) {
    const int i = threadIdx.x;
    unsigned h[PER], tot = 0u;
#pragma unroll
    for (int j = 0; j < PER; ++j) { h[j] = hist[i * PER + j]; tot += h[j]; }
    s_scan[i] = tot;
    if (i == 0) { s_out[0] = 0u; s_out[1] = 0u; }
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                  // inclusive suffix sums: s_scan[i] = the bins of threads i..255
        const unsigned v = i + o < 256 ? s_scan[i + o] : 0u;
        __syncthreads();
        s_scan[i] += v;
        __syncthreads();
    }
    const unsigned k = k_of(s_scan[0]);
    unsigned above = s_scan[i] - tot;
    if (above < k && k <= above + tot) {                 // one thread at most
#pragma unroll
        for (int j = PER - 1; j >= 0; --j) {
            if (k <= above + h[j]) { s_out[0] = (unsigned)(i * PER + j); s_out[1] = k - above; break; }
            above += h[j];
        }
    }
    if (i == 0) s_out[2] = s_scan[0];
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_ohem_clear(unsigned* __restrict__ scratch) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < OHEM_HEAD_WORDS) scratch[i] = 0u;
}

template <bool STAGED>
__global__ __launch_bounds__(256) void k_ohem_fwd(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                 float* __restrict__ loss_px, unsigned* __restrict__ hist1, int M, int C,
                                                 int ignore_index) {
    extern __shared__ float lds[];
    __shared__ unsigned s_h[OHEM_B1];
    ohem_hist_zero(s_h, OHEM_B1);                                    // visible after the first barrier below
    const int pitch = ld + 1;
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK;
    if (!STAGED) __syncthreads();
    for (int ch = 0; ch < CE_ROWS_PER_BLOCK / CE_CHUNK; ++ch) {
        const int m0 = base + ch * CE_CHUNK;
        if (m0 >= M) break;
        const int rows = min(CE_CHUNK, M - m0);
        if (STAGED) {
            __syncthreads();
            ce_chunk_load(logits + (size_t)m0 * ld, lds, rows * ld, ld);
            __syncthreads();
        }
        if ((int)threadIdx.x < rows) {
            const int m = m0 + threadIdx.x;
            const float* p = STAGED ? lds + threadIdx.x * pitch : logits + (size_t)m * ld;
            const float l = ohem_pixel_loss(p, C, (long)target[m], ignore_index);
            loss_px[m] = l;
            const unsigned key = __builtin_bit_cast(unsigned, l);
            if (key <= OHEM_KEY_MAX) atomicAdd(&s_h[key >> 20], 1u);
        }
    }
    __syncthreads();
    ohem_hist_flush(s_h, hist1, OHEM_B1);
}

// LEVEL 2: locate rank k in hist1, count digit 2 of the keys in that bin into hist2.  LEVEL 3: locate the rank left over in hist2, count
// digit 3 of the keys with both digits into hist3.  Workgroup 0 leaves what it located in the state words for the launches that follow.
template <int LEVEL>
__global__ __launch_bounds__(256) void k_ohem_refine(const float* __restrict__ loss_px, int M, unsigned* __restrict__ scratch,
                                                    int min_kept) {
    __shared__ unsigned s_h[OHEM_B23];
    __shared__ unsigned s_scan[256];
    __shared__ unsigned s_out[3];
    unsigned* state = scratch + OHEM_HIST_WORDS;
    ohem_hist_zero(s_h, OHEM_B23);
    unsigned prefix;
    if (LEVEL == 2) {
        ohem_locate<OHEM_B1 / 256>(scratch, [=](unsigned V) { return min((unsigned)min_kept, V); }, s_scan, s_out);
        prefix = s_out[0];
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            state[0] = s_out[0]; state[1] = s_out[1]; state[2] = s_out[2]; state[3] = min((unsigned)min_kept, s_out[2]);
        }
    } else {
        const unsigned b1 = state[0], k1 = state[1];
        ohem_locate<OHEM_B23 / 256>(scratch + OHEM_B1, [=](unsigned) { return k1; }, s_scan, s_out);
        prefix = (b1 << 10) | s_out[0];
        if (blockIdx.x == 0 && threadIdx.x == 0) { state[4] = s_out[0]; state[5] = s_out[1]; }
    }
    constexpr int SHIFT = LEVEL == 2 ? 20 : 10;
    for (long m = (long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long)gridDim.x * 256) {
        const unsigned key = __builtin_bit_cast(unsigned, loss_px[m]);
        if (key <= OHEM_KEY_MAX && (key >> SHIFT) == prefix) atomicAdd(&s_h[(key >> (SHIFT - 10)) & 1023u], 1u);
    }
    __syncthreads();
    ohem_hist_flush(s_h, scratch + (LEVEL == 2 ? OHEM_B1 : OHEM_B1 + OHEM_B23), OHEM_B23);
}

// kept: l > lam or l >= L (a NaN loss under a target in range, i.e. non-finite logits, stays in and makes the loss NaN)
__device__ __forceinline__ bool ohem_kept(float l, float lam, float L) { return l > lam || l >= L || l != l; }

// part[b], part[nb + b], part[2 nb + b], part[3 nb + b] = the block's sum of w[t] l, sum of w[t], kept pixels, out-of-range targets
__global__ __launch_bounds__(256) void k_ohem_reduce(const float* __restrict__ loss_px, const int64_t* __restrict__ target,
                                                    const float* __restrict__ weight, float lam, unsigned* __restrict__ scratch,
                                                    int nb, int M, int C, int ignore_index) {
    __shared__ float red[4];
    __shared__ float s_w[CE_EX_MAX_C];
    __shared__ unsigned s_scan[256];
    __shared__ unsigned s_out[3];
    unsigned* state = scratch + OHEM_HIST_WORDS;
    float* part = reinterpret_cast<float*>(scratch + OHEM_HEAD_WORDS);
    ce_ex_stage_w(weight, s_w, C);
    const unsigned b1 = state[0], b2 = state[4], k2 = state[5];
    ohem_locate<OHEM_B23 / 256>(scratch + OHEM_B1 + OHEM_B23, [=](unsigned) { return k2; }, s_scan, s_out);
    const unsigned lbits = (b1 << 20) | (b2 << 10) | s_out[0];
    const float L = __builtin_bit_cast(float, lbits);
    if (blockIdx.x == 0 && threadIdx.x == 0) state[6] = lbits;
    float acc = 0.f, div = 0.f, cnt = 0.f, bad = 0.f;
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK;
    for (int m = base + threadIdx.x; m < min(M, base + CE_ROWS_PER_BLOCK); m += CE_CHUNK) {
        const long t = (long)target[m];
        if (t == (long)ignore_index) continue;
        if (t < 0 || t >= C) { bad += 1.f; continue; }
        const float l = loss_px[m];
        if (ohem_kept(l, lam, L)) {
            acc += s_w[t] * l;
            div += s_w[t];
            cnt += 1.f;
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

// record: loss | V | out-of-range targets | sum of w[t] over the kept pixels | kept pixels | L | lam | k
__global__ __launch_bounds__(256) void k_ohem_finish(const unsigned* __restrict__ scratch, int nb, float lam, float* record) {
    __shared__ double red[4][256];
    const unsigned* state = scratch + OHEM_HIST_WORDS;
    const float* part = reinterpret_cast<const float*>(scratch + OHEM_HEAD_WORDS);
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
        record[0] = red[3][0] > 0.0 ? __builtin_nanf("") : (float)(red[0][0] / red[1][0]);   // 0/0 = NaN when no pixel is valid
        record[1] = (float)state[2];
        record[2] = (float)red[3][0];
        record[3] = (float)red[1][0];
        record[4] = (float)red[2][0];
        record[5] = __builtin_bit_cast(float, state[6]);
        record[6] = lam;
        record[7] = (float)state[3];
    }
}

// k_ce_bwd_ex with the kept predicate of the forward, read from the loss map it saved and the record's L and lam: rows that are not
// kept skip the softmax and are stored as zeros.
__global__ __launch_bounds__(256) void k_ohem_bwd(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                 const float* __restrict__ weight, const float* __restrict__ record,
                                                 const float* __restrict__ loss_px, const float* __restrict__ grad_out, float scale,
                                                 float* __restrict__ dl, int ld_d, int M, int C, int ignore_index) {
    extern __shared__ float lds[];
    __shared__ float s_w[CE_EX_MAX_C];
    ce_ex_stage_w(weight, s_w, C);
    const float g = (grad_out != nullptr ? *grad_out : 1.f) * scale / record[3];
    const float L = record[5], lam = record[6];
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
            if (t == (long)ignore_index || t < 0 || t >= C || !ohem_kept(loss_px[m0 + threadIdx.x], lam, L)) {
                for (int c = 0; c < ld; ++c) p[c] = 0.f;
            } else {
                ce_ex_pixel_grad(p, p, ld, C, (int)t, s_w, 0.f, 0.f, g);
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

__global__ __launch_bounds__(256) void k_ohem_bwd_rows(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                      const float* __restrict__ weight, const float* __restrict__ record,
                                                      const float* __restrict__ loss_px, const float* __restrict__ grad_out,
                                                      float scale, float* __restrict__ dl, int ld_d, int M, int C, int ignore_index) {
    __shared__ float s_w[CE_EX_MAX_C];
    ce_ex_stage_w(weight, s_w, C);
    __syncthreads();
    const float g = (grad_out != nullptr ? *grad_out : 1.f) * scale / record[3];
    const float L = record[5], lam = record[6];
    for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (long)gridDim.x * blockDim.x) {
        float* o = dl + (size_t)m * ld_d;
        const long t = (long)target[m];
        if (t == (long)ignore_index || t < 0 || t >= C || !ohem_kept(loss_px[m], lam, L)) {
            for (int c = 0; c < ld_d; ++c) o[c] = 0.f;
            continue;
        }
        ce_ex_pixel_grad(logits + (size_t)m * ld, o, ld_d, C, (int)t, s_w, 0.f, 0.f, g);
    }
}

// ---- Lovász-softmax (cvk_lovasz_softmax_fwd / _bwd) ---------------------------------------------------------------------------------
// Per (segment, class) the valid pixels are ordered by their error e descending, ties by pixel index ascending, and the loss is the dot
// product of the errors with the discrete derivative of the Jaccard index along that order (closed form in include/cvk.h).  The order
// comes from a stable LSD radix sort of 64-bit elements  key << 32 | pixel index << 1 | fg,  key = 0x3f800000 - bits(e) (e in [0, 1]
// is not negative, so its bits order like its value; ignored pixels carry 0xffffffff and end up behind every valid one), 8 bits a
// pass, 4 passes, S * C independent segments of P elements, work-groups of LV_TILE elements:
//   k_lv_err      one pass over the logits (the staging of k_ce_fwd_ex): writes every class's element of every pixel in pixel order,
//                 counts G per (segment, class), V per segment and the out-of-range targets (integer atomics), cross-entropy partials
//   k_lv_count    per pass: the work-group's histogram of the pass's digit -> counts[segment][digit][work-group]
//   k_lv_scan     per pass: exclusive scan of every (segment, digit) row over the work-groups, the row totals -> tot[segment][digit]
//   k_lv_scatter  per pass: a wave ranks its 512 consecutive elements 64 at a time by __ballot match masks (rank = the wave's running
//                 count of the digit + the matching lanes below), the four waves' counts are scanned per digit, the tile is put in
//                 sorted order in LDS (so equal digits leave as contiguous runs) and an element goes to
//                 lv_sort_dest(segment, digit base, work-group base, rank inside the tile's run): equal digits keep their order
//   k_lv_fgcount  foreground elements per work-group tile of the sorted buffer
//   k_lv_weight   F = foreground before the tile (integer sum of the tile counts) + a block scan; g in fp64 closed form, e g partials
//                 in fp64 in a fixed order, g scattered to the [M][ld_g] map in pixel order
//   k_lv_pairsum  L per pair: the tile partials in a fixed order
//   k_lv_finish   one work-group: segment and batch means, the record, 1 / (K counted) per segment for the backward
//   k_lv_bwd      one pass over the logits and the g map, dlogits written once
// LDS: k_lv_scatter the 16 KiB tile + 4 x 256 wave counters (then wave bases) + 3 x 256 digit bases = 23 KiB; k_lv_count 1 KiB; k_lv_err the
// (ld + 1) KiB tile + 1.1 KiB.  Every histogram is an integer count; there is no float atomic.
constexpr int LV_BINS = 1 << CVK_LOVASZ_DIGIT_BITS;
constexpr int LV_PASSES = 32 / CVK_LOVASZ_DIGIT_BITS;
constexpr int LV_TILE = CVK_LOVASZ_SORT_TILE;
constexpr int LV_WAVE_ELEMS = LV_TILE / 4, LV_ROUNDS = LV_WAVE_ELEMS / 64, LV_PER_THREAD = LV_TILE / 256;
constexpr unsigned LV_KEY_ONE = 0x3f800000u, LV_KEY_IGNORED = 0xffffffffu;
constexpr int LV_REC_HEAD = 8, LV_RECORD_FLOATS = LV_REC_HEAD + 2 * CE_EX_MAX_C;
constexpr int LV_MAX_LD = 60;              // staged passes: (ld + 1) KiB of tile + the static arrays stay under 64 KiB
static_assert(LV_BINS == 256 && LV_PASSES % 2 == 0, "one digit per thread; an even number of passes ends in the first buffer");

typedef unsigned long long lv_elem;

// Element index of rank `rank` among the keys of one digit inside one work-group: the segment's base, then the keys of smaller digits
// (digit_base), then the same digit in earlier work-groups (wg_base).  -1 (store nothing) when a piece is out of range.
__host__ __device__ __forceinline__ long long lv_sort_dest(long long seg_len, long long segment, long long digit_base, long long wg_base,
                                                           long long rank) {
    const long long pos = digit_base + wg_base + rank;
    if (seg_len <= 0 || segment < 0 || digit_base < 0 || wg_base < 0 || rank < 0 || pos >= seg_len) return -1;
    return segment * seg_len + pos;
}

// counts[segment][digit][work-group]
__host__ __device__ __forceinline__ long long lv_count_index(long long nwg, long long segment, long long digit, long long wg) {
    if (nwg <= 0 || segment < 0 || digit < 0 || digit >= LV_BINS || wg < 0 || wg >= nwg) return -1;
    return (segment * LV_BINS + digit) * nwg + wg;
}

struct LvPlan {                            // workspace layout, byte offsets (all multiples of 16)
    int S, C, P, nwg, nbe;                 // segments, classes, pixels per segment, sort work-groups per segment, k_lv_err work-groups
    size_t b, gmap, counts, tot, tilefg, partial, pairl, segl, ctr, invk, cepart, bytes;
};

static inline size_t lv_up16(size_t v) { return (v + 15) & ~(size_t)15; }

static bool lv_plan(int M, int C, int S, LvPlan* p) {
    if (M <= 0 || C <= 0 || C > CE_EX_MAX_C || S <= 0 || M % S != 0) return false;
    const long long P = M / S, nwg = (P + LV_TILE - 1) / LV_TILE;
    if (P >= (1ll << 30) || (long long)S * C > 65535 || nwg > (1ll << 22)) return false;
    const size_t E = (size_t)M * C, SC = (size_t)S * C;
    p->S = S; p->C = C; p->P = (int)P; p->nwg = (int)nwg; p->nbe = S * cvk_cdiv(P, CE_ROWS_PER_BLOCK);
    size_t o = 8 * E;
    p->b = o; o += 8 * E;
    p->gmap = o; o = lv_up16(o + 4 * E);
    p->counts = o; o = lv_up16(o + 4 * SC * LV_BINS * nwg);
    p->tot = o; o = lv_up16(o + 4 * SC * LV_BINS);
    p->tilefg = o; o = lv_up16(o + 4 * SC * nwg);
    p->partial = o; o = lv_up16(o + 8 * SC * nwg);
    p->pairl = o; o = lv_up16(o + 8 * SC);
    p->segl = o; o = lv_up16(o + 8 * (size_t)S);
    p->ctr = o; o = lv_up16(o + 4 * (SC + S + 1));           // G[S C] | V[S] | out-of-range targets
    p->invk = o; o = lv_up16(o + 4 * (size_t)S);
    p->cepart = o; o = lv_up16(o + 4 * 2 * (size_t)p->nbe);
    p->bytes = o;
    return true;
}

// exclusive scan of one value per thread over the 256 threads (all must call); *total = the sum
__device__ __forceinline__ unsigned lv_block_excl_scan(unsigned v, unsigned* s_wave, unsigned* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();                                       // s_wave may still be read by an earlier call
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    unsigned pre = 0u, tot = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < w) pre += s_wave[k];
        tot += s_wave[k];
    }
    *total = tot;
    return pre + inc - v;
}

__device__ __forceinline__ unsigned lv_block_sum(unsigned v, unsigned* s_wave) {
    unsigned tot;
    lv_block_excl_scan(v, s_wave, &tot);
    return tot;
}

// grid (ceil(P / 1024), S): a work-group stays inside one segment.  ctr: G[S C] | V[S] | out-of-range targets.
// cepart[b], cepart[nbe + b]: the work-group's cross-entropy sum and divisor sum (want_ce only).
template <bool STAGED>
__global__ __launch_bounds__(256) void k_lv_err(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                               const float* __restrict__ weight, int want_ce, lv_elem* __restrict__ buf,
                                               unsigned* __restrict__ ctr, float* __restrict__ cepart, int nbe, int P, int S, int C,
                                               int ignore_index) {
    extern __shared__ float lds[];
    __shared__ float red[4];
    __shared__ float s_w[CE_EX_MAX_C];
    __shared__ unsigned s_g[CE_EX_MAX_C + 2];                          // G per class | valid | out of range
    ce_ex_stage_w(weight, s_w, C);
    for (int c = threadIdx.x; c < C + 2; c += 256) s_g[c] = 0u;
    const int pitch = ld + 1;
    const int seg = blockIdx.y;
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK;
    float acc = 0.f, div = 0.f;
    if (!STAGED) __syncthreads();
    for (int ch = 0; ch < CE_ROWS_PER_BLOCK / CE_CHUNK; ++ch) {
        const int i0 = base + ch * CE_CHUNK;
        if (i0 >= P) break;
        const int rows = min(CE_CHUNK, P - i0);
        const size_t m0 = (size_t)seg * P + i0;
        if (STAGED) {
            __syncthreads();
            ce_chunk_load(logits + m0 * ld, lds, rows * ld, ld);
            __syncthreads();
        }
        if ((int)threadIdx.x < rows) {
            const unsigned i = (unsigned)(i0 + threadIdx.x);
            const size_t m = m0 + threadIdx.x;
            const float* x = STAGED ? lds + threadIdx.x * pitch : logits + m * ld;
            const long t = (long)target[m];
            const bool valid = t >= 0 && t < C && t != (long)ignore_index;
            float mx = 0.f, se = 1.f, rest = 0.f;
            if (valid) {
                atomicAdd(&s_g[t], 1u);
                atomicAdd(&s_g[C], 1u);
                mx = x[0];
                for (int c = 1; c < C; ++c) mx = fmaxf(mx, x[c]);
                se = 0.f;
                for (int c = 0; c < C; ++c) {
                    const float ex = expf(x[c] - mx);
                    se += ex;
                    if (c != (int)t) rest += ex;           // 1 - p[t] without the cancellation: the other classes' share
                }
                if (want_ce) {
                    acc += ce_ex_pixel_loss(x, C, (int)t, s_w, 0.f);
                    div += s_w[t];
                }
            } else if (t != (long)ignore_index) {
                atomicAdd(&s_g[C + 1], 1u);
            }
            for (int c = 0; c < C; ++c) {
                unsigned key = LV_KEY_IGNORED;
                const unsigned fg = valid && c == (int)t ? 1u : 0u;
                if (valid) {
                    const float e = fminf((fg ? rest : expf(x[c] - mx)) / se, 1.f);
                    key = e >= 0.f ? LV_KEY_ONE - __builtin_bit_cast(unsigned, e) : 0u;       // a NaN error sorts first
                }
                buf[((size_t)seg * C + c) * P + i] = ((lv_elem)key << 32) | (lv_elem)((i << 1) | fg);
            }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256)
        if (s_g[c]) atomicAdd(&ctr[seg * C + c], s_g[c]);
    if (threadIdx.x == 0) {
        if (s_g[C]) atomicAdd(&ctr[S * C + seg], s_g[C]);
        if (s_g[C + 1]) atomicAdd(&ctr[S * C + S], s_g[C + 1]);
    }
    if (want_ce) {
        const float s = block_sum_256(acc, red);
        const float d = block_sum_256(div, red);
        if (threadIdx.x == 0) {
            const int b = seg * gridDim.x + blockIdx.x;
            cepart[b] = s;
            cepart[nbe + b] = d;
        }
    }
}

// grid (nwg, S C)
__global__ __launch_bounds__(256) void k_lv_count(const lv_elem* __restrict__ buf, int P, int shift, unsigned* __restrict__ counts,
                                                 int nwg) {
    __shared__ unsigned s_h[LV_BINS];
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    const lv_elem* seg = buf + (size_t)blockIdx.y * P;
    const long long t0 = (long long)blockIdx.x * LV_TILE;
    for (int k = threadIdx.x; k < LV_TILE; k += 256)
        if (t0 + k < P) atomicAdd(&s_h[(unsigned)(seg[t0 + k] >> (32 + shift)) & (LV_BINS - 1)], 1u);
    __syncthreads();
    const long long at = lv_count_index(nwg, blockIdx.y, threadIdx.x, blockIdx.x);
    if (at >= 0) counts[at] = s_h[threadIdx.x];
}

// grid (256 digits, S C): the row counts[segment][digit][0 .. nwg) becomes its exclusive scan, its total goes to tot[segment][digit]
__global__ __launch_bounds__(256) void k_lv_scan(unsigned* __restrict__ counts, unsigned* __restrict__ tot, int nwg) {
    __shared__ unsigned s_wave[4];
    const long long row = lv_count_index(nwg, blockIdx.y, blockIdx.x, 0);
    if (row < 0) return;
    unsigned carry = 0u;
    for (int b = 0; b < nwg; b += 256) {
        const int k = b + threadIdx.x;
        const unsigned v = k < nwg ? counts[row + k] : 0u;
        unsigned total;
        const unsigned ex = lv_block_excl_scan(v, s_wave, &total);
        if (k < nwg) counts[row + k] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tot[blockIdx.y * LV_BINS + blockIdx.x] = carry;
}

// grid (nwg, S C).  Tile order = (wave, round, lane): wave w owns elements [w 512, (w + 1) 512) of the tile.
__global__ __launch_bounds__(256) void k_lv_scatter(const lv_elem* __restrict__ in, lv_elem* __restrict__ out, int P, int shift,
                                                   const unsigned* __restrict__ counts, const unsigned* __restrict__ tot, int nwg) {
    __shared__ unsigned s_cnt[4][LV_BINS];                 // the wave's running count of each digit, then its base inside the tile
    __shared__ unsigned s_dbase[LV_BINS], s_wbase[LV_BINS], s_tbase[LV_BINS], s_wave[4];
    __shared__ lv_elem s_el[LV_TILE];                      // the tile in sorted order: equal digits leave as contiguous runs
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int segc = blockIdx.y;
#pragma unroll
    for (int k = 0; k < 4; ++k) s_cnt[k][threadIdx.x] = 0u;
    __syncthreads();
    const lv_elem* seg = in + (size_t)segc * P;
    const long long t0 = (long long)blockIdx.x * LV_TILE + w * LV_WAVE_ELEMS + lane;
    const unsigned long long below = (1ull << lane) - 1ull;
    lv_elem el[LV_ROUNDS];
    unsigned rank[LV_ROUNDS];
#pragma unroll
    for (int r = 0; r < LV_ROUNDS; ++r) {
        const long long idx = t0 + r * 64;
        const bool valid = idx < P;
        el[r] = valid ? seg[idx] : 0ull;
        const unsigned d = (unsigned)(el[r] >> (32 + shift)) & (LV_BINS - 1);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < CVK_LOVASZ_DIGIT_BITS; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(valid && bit);
            peers &= bit ? m : ~m;
        }
        rank[r] = 0u;
        if (valid) {
            const unsigned before = s_cnt[w][d];
            rank[r] = before + (unsigned)__popcll(peers & below);
            if ((peers & below) == 0ull) s_cnt[w][d] = before + (unsigned)__popcll(peers);   // the lowest matching lane
        }
    }
    __syncthreads();
    {                                                      // thread = digit: the waves' bases inside the tile, the two global bases
        const int d = threadIdx.x;
        unsigned run = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned c = s_cnt[k][d];
            s_cnt[k][d] = run;
            run += c;
        }
        unsigned total;
        s_tbase[d] = lv_block_excl_scan(run, s_wave, &total);          // where the digit's run starts inside the sorted tile
        s_dbase[d] = lv_block_excl_scan(tot[segc * LV_BINS + d], s_wave, &total);
        const long long at = lv_count_index(nwg, segc, d, blockIdx.x);
        s_wbase[d] = at >= 0 ? counts[at] : 0xffffffffu;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < LV_ROUNDS; ++r) {
        if (t0 + r * 64 < P) {
            const unsigned d = (unsigned)(el[r] >> (32 + shift)) & (LV_BINS - 1);
            const unsigned at = s_tbase[d] + s_cnt[w][d] + rank[r];
            if (at < (unsigned)LV_TILE) s_el[at] = el[r];
        }
    }
    __syncthreads();
    const long long left = (long long)P - (long long)blockIdx.x * LV_TILE;
    const int n = left < LV_TILE ? (int)left : LV_TILE;
    for (int k = threadIdx.x; k < n; k += 256) {           // consecutive threads, consecutive destinations inside a run
        const lv_elem e = s_el[k];
        const unsigned d = (unsigned)(e >> (32 + shift)) & (LV_BINS - 1);
        const long long dst = lv_sort_dest(P, segc, s_dbase[d], s_wbase[d], (long long)k - (long long)s_tbase[d]);
        if (dst >= 0) out[dst] = e;
    }
}

// grid (nwg, S C): thread k of a tile owns its elements [8 k, 8 k + 8)
__global__ __launch_bounds__(256) void k_lv_fgcount(const lv_elem* __restrict__ buf, int P, unsigned* __restrict__ tilefg, int nwg) {
    __shared__ unsigned s_wave[4];
    const lv_elem* seg = buf + (size_t)blockIdx.y * P;
    const long long n0 = (long long)blockIdx.x * LV_TILE + threadIdx.x * LV_PER_THREAD;
    unsigned f = 0u;
#pragma unroll
    for (int j = 0; j < LV_PER_THREAD; ++j)
        if (n0 + j < P) f += (unsigned)(seg[n0 + j] & 1ull);
    const unsigned total = lv_block_sum(f, s_wave);
    if (threadIdx.x == 0) tilefg[(size_t)blockIdx.y * nwg + blockIdx.x] = total;
}

// grid (nwg, S C).  partial[segment class][work-group] = the tile's sum of e g (fp64, thread order then a fixed tree).
__global__ __launch_bounds__(256) void k_lv_weight(const lv_elem* __restrict__ buf, int P, int S, int C, int nwg,
                                                  const unsigned* __restrict__ tilefg, const unsigned* __restrict__ ctr, int mode_all,
                                                  float* __restrict__ gmap, int ld_g, double* __restrict__ partial) {
    __shared__ unsigned s_wave[4];
    __shared__ double s_red[256];
    const int segc = blockIdx.y, seg = segc / C, c = segc - seg * C;
    const long long G = ctr[segc], V = ctr[S * C + seg];
    const bool evaluated = V > 0 && (mode_all || G > 0);
    unsigned before = 0u;
    for (int k = threadIdx.x; k < (int)blockIdx.x; k += 256) before += tilefg[(size_t)segc * nwg + k];
    const unsigned F0 = lv_block_sum(before, s_wave);
    const lv_elem* sg = buf + (size_t)segc * P;
    const long long n0 = (long long)blockIdx.x * LV_TILE + threadIdx.x * LV_PER_THREAD;
    lv_elem el[LV_PER_THREAD];
    unsigned f = 0u;
#pragma unroll
    for (int j = 0; j < LV_PER_THREAD; ++j) {
        el[j] = n0 + j < P ? sg[n0 + j] : 0ull;
        f += (unsigned)(el[j] & 1ull);
    }
    unsigned total;
    long long F = (long long)F0 + lv_block_excl_scan(f, s_wave, &total);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < LV_PER_THREAD; ++j) {
        const long long n = n0 + j;
        if (n >= V) break;                                 // the valid pixels come first; V <= P
        const unsigned fg = (unsigned)(el[j] & 1ull);
        const unsigned i = (unsigned)(el[j] & 0xffffffffull) >> 1;
        const float e = __builtin_bit_cast(float, LV_KEY_ONE - (unsigned)(el[j] >> 32));
        double g = 0.0;
        if (evaluated) {
            if (G == 0) {
                g = n == 0 ? 1.0 : 0.0;
            } else {
                const long long U = G + n - F, I = G - F;
                g = fg ? 1.0 / (double)U : (double)I / ((double)U * (double)(U + 1));
            }
        }
        const float gf = (float)g;
        acc += (double)e * (double)gf;
        if (i < (unsigned)P) gmap[((size_t)seg * P + i) * ld_g + c] = gf;
        F += fg;
    }
    s_red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_red[threadIdx.x] += s_red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)segc * nwg + blockIdx.x] = s_red[0];
}

// grid (S C): pairl[pair] = L of the pair, its tile partials summed per thread in tile order, then one fixed tree
__global__ __launch_bounds__(256) void k_lv_pairsum(const double* __restrict__ partial, int nwg, double* __restrict__ pairl) {
    __shared__ double s_red[256];
    double l = 0.0;
    for (int k = threadIdx.x; k < nwg; k += 256) l += partial[(size_t)blockIdx.x * nwg + k];
    s_red[threadIdx.x] = l;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_red[threadIdx.x] += s_red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) pairl[blockIdx.x] = s_red[0];
}

// One work-group.  segl[S]: scratch; invk[seg] = 1 / (K_seg counted segments), 0 for a segment that is not counted.
__global__ __launch_bounds__(256) void k_lv_finish(const double* __restrict__ pairl, double* __restrict__ segl,
                                                  const unsigned* __restrict__ ctr, float* __restrict__ invk,
                                                  const float* __restrict__ cepart, int nbe, int S, int C, int mode_all,
                                                  float lovasz, float ce, float* __restrict__ record) {
    __shared__ double s_red[2][256];
    const int SC = S * C;
    double h = 0.0, dv = 0.0;
    if (ce > 0.f)
        for (int i = threadIdx.x; i < nbe; i += 256) { h += (double)cepart[i]; dv += (double)cepart[nbe + i]; }
    s_red[0][threadIdx.x] = h; s_red[1][threadIdx.x] = dv;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { s_red[0][threadIdx.x] += s_red[0][threadIdx.x + o]; s_red[1][threadIdx.x] += s_red[1][threadIdx.x + o]; }
        __syncthreads();
    }
    for (int s = threadIdx.x; s < S; s += 256) {           // segment means over the evaluated classes
        const bool any = ctr[SC + s] > 0u;
        double sum = 0.0;
        int K = 0;
        for (int c = 0; c < C; ++c)
            if (any && (mode_all || ctr[s * C + c] > 0u)) { sum += pairl[s * C + c]; ++K; }
        segl[s] = K > 0 ? sum / K : 0.0;
        invk[s] = (float)K;
    }
    for (int c = threadIdx.x; c < C; c += 256) {           // per class over the segments, for the record
        double sum = 0.0, g = 0.0;
        int n = 0;
        for (int s = 0; s < S; ++s) {
            const unsigned gc = ctr[s * C + c];
            g += (double)gc;
            if (ctr[SC + s] > 0u && (mode_all || gc > 0u)) { sum += pairl[s * C + c]; ++n; }
        }
        record[LV_REC_HEAD + c] = n > 0 ? (float)(sum / n) : __builtin_nanf("");
        record[LV_REC_HEAD + CE_EX_MAX_C + c] = (float)g;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0, valid = 0.0;
        int counted = 0, pairs = 0;
        for (int s = 0; s < S; ++s) {
            const int K = (int)invk[s];
            valid += (double)ctr[SC + s];
            if (K > 0) { total += segl[s]; ++counted; pairs += K; }
        }
        for (int s = 0; s < S; ++s) {
            const int K = (int)invk[s];
            invk[s] = K > 0 ? (float)(1.0 / ((double)K * counted)) : 0.f;
        }
        const double J = counted > 0 ? total / counted : 0.0;
        const double H = ce > 0.f ? s_red[0][0] / s_red[1][0] : 0.0;       // 0/0 = NaN when no pixel is valid, as cvk_softmax_ce_fwd_ex
        const unsigned bad = ctr[SC + S];
        record[0] = bad > 0u ? __builtin_nanf("") : (float)((double)lovasz * J + (ce > 0.f ? (double)ce * H : 0.0));
        record[1] = (float)valid;
        record[2] = (float)bad;
        record[3] = (float)J;
        record[4] = (float)H;
        record[5] = (float)pairs;
        record[6] = (float)counted;
        record[7] = ce > 0.f ? (float)s_red[1][0] : 0.f;
    }
}

// o may alias x (column c is read before it is written); columns [C, ld_o) are zeroed.  k = lovasz g / (K counted), gce = ce g w[t] / divisor.
__device__ __forceinline__ void lv_pixel_grad(const float* x, const float* __restrict__ gm, float* o, int ld_o, int C, int t, float k,
                                              float gce) {
    float mx = x[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, x[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(x[c] - mx);
    const float inv = 1.f / se;
    float dot = 0.f;
    for (int c = 0; c < C; ++c) dot += (c == t ? -k : k) * gm[c] * (expf(x[c] - mx) * inv);
    for (int c = 0; c < C; ++c) {
        const float p = expf(x[c] - mx) * inv;
        o[c] = p * ((c == t ? -k : k) * gm[c] - dot) + gce * (p - (c == t ? 1.f : 0.f));
    }
    for (int c = C; c < ld_o; ++c) o[c] = 0.f;
}

template <bool STAGED>
__global__ __launch_bounds__(256) void k_lv_bwd(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                               const float* __restrict__ weight, float lovasz, float ce,
                                               const float* __restrict__ record, const float* __restrict__ invk,
                                               const float* __restrict__ gmap, int ld_g, const float* __restrict__ grad_out, float scale,
                                               float* __restrict__ dl, int ld_d, int M, int P, int C, int ignore_index) {
    extern __shared__ float lds[];
    __shared__ float s_w[CE_EX_MAX_C];
    ce_ex_stage_w(weight, s_w, C);
    const float go = (grad_out != nullptr ? *grad_out : 1.f) * scale;
    const float lam = lovasz * go;
    const float gce0 = ce > 0.f ? ce * go / record[7] : 0.f;
    const int pitch = ld + 1;
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK;
    if (!STAGED) __syncthreads();
    for (int ch = 0; ch < CE_ROWS_PER_BLOCK / CE_CHUNK; ++ch) {
        const int m0 = base + ch * CE_CHUNK;
        if (m0 >= M) break;
        const int rows = min(CE_CHUNK, M - m0);
        if (STAGED) {
            __syncthreads();
            ce_chunk_load(logits + (size_t)m0 * ld, lds, rows * ld, ld);
            __syncthreads();
        }
        if ((int)threadIdx.x < rows) {
            const int m = m0 + threadIdx.x;
            const float* x = STAGED ? lds + threadIdx.x * pitch : logits + (size_t)m * ld;
            float* o = STAGED ? lds + threadIdx.x * pitch : dl + (size_t)m * ld_d;
            const int ld_o = STAGED ? ld : ld_d;
            const long t = (long)target[m];
            if (t == (long)ignore_index || t < 0 || t >= C) {
                for (int c = 0; c < ld_o; ++c) o[c] = 0.f;
            } else {
                lv_pixel_grad(x, gmap + (size_t)m * ld_g, o, ld_o, C, (int)t, lam * invk[m / P], ce > 0.f ? gce0 * s_w[t] : 0.f);
            }
        }
        if (STAGED) {
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
}

// ---- boundary loss (Kervadec et al., MIDL 2019; cvk_boundary_loss_fwd / _bwd) -----------------------------------------------------------
// loss = cb B + cc H, B = 1 / |V| sum_{q in V} sum_{c in S} phi_c(q) p_c(q), p = softmax(x), H = the weighted mean cross-entropy of
// k_ce_fwd_ex (label_smoothing 0), V = the pixels whose target is a class.  S is a bit mask.  phi is [M][C] dense.
//   k_bdl_fwd     the staging of k_ce_fwd_ex, thread = pixel: the pixel's row in LDS is overwritten with phi_c p_c (zeros outside V and
//                 S); then thread (c, r) = (tid % 32, tid / 32) sums column c over rows [32 r, 32 r + 32) of the tile in row order.
//                 part[k][nb]: valid pixels | out-of-range targets | cross-entropy sum | sum w[t] | class c's sum at 4 + c
//   k_bdl_finish  one work-group: every part row in fp64 (thread order, then one fixed tree); B = the sum of the class terms; reads the
//                 two coefficients from device memory and leaves them in the record for the backward
//   k_bdl_bwd     one pass, dlogits written once
// LDS: the (ld + 1) KiB tile + 1.2 KiB.  No float atomic: loss and gradient are bitwise reproducible.
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

// ---- fused focal + soft-Dice loss (cvk_seg_loss_fwd / _bwd) ---------------------------------------------------------------------
// L = ce F + dice D over the valid pixels of the batch, p = softmax(x), t = target, q = 1 - p[t]:
//   F = sum w[t] q^gamma (lse - x[t]) / sum w[t]
//   D = 1 - (1 / K) sum_{c in S} (2 I_c + s) / (P_c + T_c + s),  I_c = sum p[c] [t = c], P_c = sum p[c], T_c = sum [t = c]
// One forward pass serves both terms: a chunk of pixel rows is staged as in k_ce_fwd_ex, thread = pixel leaves exp(x - max) in the
// tile and (target, 1 / sum exp) beside it, then thread = (class, row segment) walks its column over its rows.  The segment sums are
// folded class by class in segment order, the workgroup partials by k_seg_finish in fp64: every sum has one fixed order and there is
// no float atomic.  ld > CE_MAX_LD: the same kernel with STAGED = false, a thread reads its pixel's row from global memory and the
// tile (pitch C + 1) holds the exponentials only.  A chunk is as many rows as fit SEG_TILE_FLOATS, 256 at most.
constexpr int SEG_TILE_FLOATS = 14848;     // 58 KiB of dynamic LDS: with the static arrays a workgroup stays under 64 KiB
constexpr int SEG_PART_HEAD = 4;           // partial rows: focal numerator, sum w[t], valid pixels, out-of-range targets, then I, P, T per class
constexpr int SEG_REC_HEAD = 7;            // record: L, valid, out of range, sum w[t], F, D, K, then dice_c[C], a_c[C], b_c[C]
constexpr int SEG_FINISH_THREADS = 1024;

struct SegPixel { float inv, pt, q, logpt; };     // 1 / sum exp, p[t], 1 - p[t], log p[t]

// exp(x[c] - max) of one pixel (into e when STORE; e may alias x).  q comes from the other classes' exponentials, so it keeps its
// relative precision when p[t] rounds to 1; log p[t] = -log1p(rest / e_t) there, x[t] - lse when the target is the unlikely class.
template <bool STORE>
__device__ __forceinline__ SegPixel seg_pixel_softmax(const float* x, float* e, int C, int t) {
    float mx = x[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, x[c]);
    const float xt = x[t] - mx;
    float rest = 0.f;
    for (int c = 0; c < C; ++c) {
        const float v = expf(x[c] - mx);
        if (c != t) rest += v;
        if (STORE) e[c] = v;
    }
    const float et = expf(xt), se = rest + et;
    SegPixel r;
    r.inv = 1.f / se;
    r.pt = et * r.inv;
    r.q = rest * r.inv;
    r.logpt = rest < et ? -log1pf(rest / et) : xt - logf(se);
    return r;
}

__device__ __forceinline__ float seg_pow(float q, float gamma) { return gamma == 0.f ? 1.f : powf(q, gamma); }

template <bool STAGED>
__global__ __launch_bounds__(256) void k_seg_fwd(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                const float* __restrict__ weight, float ce, float dice, float gamma,
                                                float* __restrict__ part, int nb, int M, int C, int ignore_index, int rows_r) {
    extern __shared__ float lds[];
    __shared__ float red[4];
    __shared__ float s_w[CE_EX_MAX_C];
    __shared__ int2 s_ti[CE_CHUNK];                  // per row of the chunk: target (-1: not counted) and the bits of 1 / sum exp
    __shared__ float s_cs[3][CE_CHUNK];
    ce_ex_stage_w(weight, s_w, C);                   // visible after the first chunk's barrier
    const int tid = threadIdx.x;
    const int pitch = (STAGED ? ld : C) + 1;
    const int nseg = CE_CHUNK / C;                   // C <= 128: at least two row segments per class
    const int seg_rows = ((rows_r + nseg - 1) / nseg) | 1;   // odd: with an odd pitch the segments start on distinct banks
    const int cs_c = tid / nseg, cs_s = tid - cs_c * nseg;
    const bool cs_on = cs_c < C;
    float acc = 0.f, div = 0.f, cnt = 0.f, bad = 0.f, sI = 0.f, sP = 0.f;
    int sT = 0;
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK, end = min(M, base + CE_ROWS_PER_BLOCK);
    for (int m0 = base; m0 < end; m0 += rows_r) {
        const int rows = min(rows_r, end - m0);
        __syncthreads();                             // the previous chunk's column walk is done with the tile
        if (STAGED) {
            ce_chunk_load(logits + (size_t)m0 * ld, lds, rows * ld, ld);
            __syncthreads();
        }
        if (tid < rows) {
            int tl = -1;
            float inv = 0.f;
            const long t = (long)target[m0 + tid];
            if (t != (long)ignore_index) {
                if (t >= 0 && t < C) {
                    const float* x = STAGED ? lds + tid * pitch : logits + (size_t)(m0 + tid) * ld;
                    if (dice > 0.f || ce > 0.f) {
                        const SegPixel px = dice > 0.f ? seg_pixel_softmax<true>(x, lds + tid * pitch, C, (int)t)
                                                       : seg_pixel_softmax<false>(x, nullptr, C, (int)t);
                        if (ce > 0.f) acc += s_w[t] * seg_pow(px.q, gamma) * -px.logpt;
                        inv = px.inv;
                    }
                    div += s_w[t];
                    cnt += 1.f;
                    tl = (int)t;
                } else {
                    bad += 1.f;
                }
            }
            s_ti[tid] = make_int2(tl, __float_as_int(inv));
        }
        if (dice > 0.f) {
            __syncthreads();
            if (cs_on) {
                const int r1 = min(rows, (cs_s + 1) * seg_rows);
                for (int r = cs_s * seg_rows; r < r1; ++r) {
                    const int2 ti = s_ti[r];
                    if (ti.x >= 0) {
                        const float p = lds[r * pitch + cs_c] * __int_as_float(ti.y);
                        sP += p;
                        if (ti.x == cs_c) { sI += p; ++sT; }
                    }
                }
            }
        }
    }
    const float s = block_sum_256(acc, red);
    const float d = block_sum_256(div, red);
    const float n = block_sum_256(cnt, red);
    const float b = block_sum_256(bad, red);
    if (tid == 0) {
        part[blockIdx.x] = s;
        part[nb + blockIdx.x] = d;
        part[2 * nb + blockIdx.x] = n;
        part[3 * nb + blockIdx.x] = b;
    }
    if (dice > 0.f) {
        s_cs[0][tid] = sI; s_cs[1][tid] = sP; s_cs[2][tid] = (float)sT;      // a workgroup counts at most 1024 pixels: exact
        __syncthreads();
        if (tid < C) {
            float I = 0.f, P = 0.f, T = 0.f;
            for (int k = 0; k < nseg; ++k) {
                I += s_cs[0][tid * nseg + k]; P += s_cs[1][tid * nseg + k]; T += s_cs[2][tid * nseg + k];
            }
            float* o = part + (size_t)(SEG_PART_HEAD + 3 * tid) * nb + blockIdx.x;
            o[0] = I; o[nb] = P; o[2 * (size_t)nb] = T;
        }
    }
}

// One workgroup: wave w reduces partial rows w, w + 16, ... in fp64 (lane-strided over the workgroups, then a fixed butterfly), then
// the record is written: rec[0] = L (NaN when a target was out of range), rec[1] = valid pixels, rec[2] = out-of-range targets,
// rec[3] = sum w[t], rec[4] = F (0 when ce = 0), rec[5] = D (0 when dice = 0), rec[6] = K, then per class dice_c (0 outside S),
// a_c = -2 / (K den_c), b_c = (2 I_c + s) / (K den_c^2) with den_c = P_c + T_c + s.  den_c = 0 (s = 0 and the class neither
// predicted nor present) counts as dice_c = 1 with a zero gradient.
__global__ __launch_bounds__(SEG_FINISH_THREADS) void k_seg_finish(const float* __restrict__ part, int nb, int C, float ce, float dice,
                                                                   float smooth, int average, float* __restrict__ rec) {
    __shared__ double sums[SEG_PART_HEAD + 3 * CE_EX_MAX_C];
    __shared__ double s_dc[CE_EX_MAX_C];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nrows = dice > 0.f ? SEG_PART_HEAD + 3 * C : SEG_PART_HEAD;
    for (int k = wave; k < nrows; k += SEG_FINISH_THREADS / 64) {
        const float* row = part + (size_t)k * nb;
        double v = 0.0;
        for (int i = lane; i < nb; i += 64) v += (double)row[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) sums[k] = v;
    }
    __syncthreads();
    const bool all = average == CVK_DICE_ALL;
    int K = 0;
    if (dice > 0.f)
        for (int c = 0; c < C; ++c) K += (all || sums[SEG_PART_HEAD + 3 * c + 2] > 0.0) ? 1 : 0;
    if (tid < C) {
        double dc = 0.0, a = 0.0, b = 0.0;
        if (dice > 0.f) {
            const double I = sums[SEG_PART_HEAD + 3 * tid], P = sums[SEG_PART_HEAD + 3 * tid + 1], T = sums[SEG_PART_HEAD + 3 * tid + 2];
            if (all || T > 0.0) {
                const double den = P + T + (double)smooth, num = 2.0 * I + (double)smooth;
                if (den > 0.0) {
                    dc = num / den;
                    a = -2.0 / (K * den);
                    b = num / (K * den * den);
                } else {
                    dc = 1.0;
                }
            }
        }
        s_dc[tid] = dc;
        rec[SEG_REC_HEAD + tid] = (float)dc;
        rec[SEG_REC_HEAD + C + tid] = (float)a;
        rec[SEG_REC_HEAD + 2 * C + tid] = (float)b;
    }
    __syncthreads();
    if (tid == 0) {
        double D = 0.0;
        if (K > 0) {
            double sd = 0.0;
            for (int c = 0; c < C; ++c) sd += s_dc[c];
            D = 1.0 - sd / K;
        }
        const double F = ce > 0.f ? sums[0] / sums[1] : 0.0;                 // 0/0 = NaN when every pixel is ignored, as k_ce_finish_ex
        const double L = (ce > 0.f ? (double)ce * F : 0.0) + (dice > 0.f ? (double)dice * D : 0.0);
        rec[0] = sums[3] > 0.0 ? __builtin_nanf("") : (float)L;
        rec[1] = (float)sums[2];
        rec[2] = (float)sums[3];
        rec[3] = (float)sums[1];
        rec[4] = (float)F;
        rec[5] = (float)D;
        rec[6] = (float)K;
    }
}

// One pixel's gradient row.  x: its C logits; o: the output row (INPLACE: o aliases x, the exponentials pass through it).  cw =
// ce w[t] / sum w[t] (0 when ce = 0), G = grad_out * scale:
//   o[k] = G (cw B ([k = t] - p[k]) + dice p[k] (b[k] + a[t] [k = t] - sum_c (b[c] + a[c] [c = t]) p[c])),
//   B = gamma p[t] q^(gamma - 1) log p[t] - q^gamma = q^gamma (gamma p[t] (log p[t] / q) - 1), log p[t] / q -> -1 as q -> 0.
template <bool INPLACE>
__device__ __forceinline__ void seg_pixel_grad(const float* x, float* o, int ld_o, int C, int t, float cw, float dice, float gamma,
                                               const float* s_a, const float* s_b, float G) {
    float mx = x[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, x[c]);
    const float xt = x[t] - mx;
    float rest = 0.f, dotb = 0.f;
    for (int c = 0; c < C; ++c) {
        const float v = expf(x[c] - mx);
        if (c != t) rest += v;
        dotb += s_b[c] * v;
        if (INPLACE) o[c] = v;
    }
    const float et = expf(xt), se = rest + et, inv = 1.f / se;
    const float pt = et * inv, q = rest * inv;
    float cf = 0.f;
    if (cw > 0.f) {
        const float logpt = rest < et ? -log1pf(rest / et) : xt - logf(se);
        const float ratio = q > 0.f ? logpt / q : -1.f;
        cf = cw * seg_pow(q, gamma) * (gamma * pt * ratio - 1.f);
    }
    const float at = s_a[t], dot = dotb * inv + at * pt;
    for (int c = 0; c < C; ++c) {
        const float p = (INPLACE ? o[c] : expf(x[c] - mx)) * inv;
        const bool hit = c == t;
        o[c] = G * (cf * ((hit ? 1.f : 0.f) - p) + dice * p * (s_b[c] + (hit ? at : 0.f) - dot));
    }
    for (int c = C; c < ld_o; ++c) o[c] = 0.f;
}

__device__ __forceinline__ void seg_stage_ab(const float* __restrict__ rec, float* s_a, float* s_b, int C) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        s_a[c] = rec[SEG_REC_HEAD + C + c];
        s_b[c] = rec[SEG_REC_HEAD + 2 * C + c];
    }
}

// Rows of ignored or out-of-range targets and columns [C, ld_d) are written as zeros.
__global__ __launch_bounds__(256) void k_seg_bwd(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                const float* __restrict__ weight, float ce, float dice, float gamma,
                                                const float* __restrict__ rec, const float* __restrict__ grad_out, float scale,
                                                float* __restrict__ dl, int ld_d, int M, int C, int ignore_index, int rows_r) {
    extern __shared__ float lds[];
    __shared__ float s_w[CE_EX_MAX_C], s_a[CE_EX_MAX_C], s_b[CE_EX_MAX_C];
    ce_ex_stage_w(weight, s_w, C);
    seg_stage_ab(rec, s_a, s_b, C);                  // visible after the first chunk's barriers
    const float G = (grad_out != nullptr ? *grad_out : 1.f) * scale;
    const float cscale = ce > 0.f ? ce / rec[3] : 0.f;
    const int pitch = ld + 1;
    const int base = blockIdx.x * CE_ROWS_PER_BLOCK, end = min(M, base + CE_ROWS_PER_BLOCK);
    for (int m0 = base; m0 < end; m0 += rows_r) {
        const int rows = min(rows_r, end - m0);
        __syncthreads();
        ce_chunk_load(logits + (size_t)m0 * ld, lds, rows * ld, ld);
        __syncthreads();
        if ((int)threadIdx.x < rows) {
            float* p = lds + threadIdx.x * pitch;
            const long t = (long)target[m0 + threadIdx.x];
            if (t == (long)ignore_index || t < 0 || t >= C) {
                for (int c = 0; c < ld; ++c) p[c] = 0.f;
            } else {
                seg_pixel_grad<true>(p, p, ld, C, (int)t, cscale * s_w[t], dice, gamma, s_a, s_b, G);
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

__global__ __launch_bounds__(256) void k_seg_bwd_rows(const float* __restrict__ logits, int ld, const int64_t* __restrict__ target,
                                                     const float* __restrict__ weight, float ce, float dice, float gamma,
                                                     const float* __restrict__ rec, const float* __restrict__ grad_out, float scale,
                                                     float* __restrict__ dl, int ld_d, int M, int C, int ignore_index) {
    __shared__ float s_w[CE_EX_MAX_C], s_a[CE_EX_MAX_C], s_b[CE_EX_MAX_C];
    ce_ex_stage_w(weight, s_w, C);
    seg_stage_ab(rec, s_a, s_b, C);
    __syncthreads();
    const float G = (grad_out != nullptr ? *grad_out : 1.f) * scale;
    const float cscale = ce > 0.f ? ce / rec[3] : 0.f;
    for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (long)gridDim.x * blockDim.x) {
        float* o = dl + (size_t)m * ld_d;
        const long t = (long)target[m];
        if (t == (long)ignore_index || t < 0 || t >= C) {
            for (int c = 0; c < ld_d; ++c) o[c] = 0.f;
            continue;
        }
        seg_pixel_grad<false>(logits + (size_t)m * ld, o, ld_d, C, (int)t, cscale * s_w[t], dice, gamma, s_a, s_b, G);
    }
}

// ---- knowledge-distillation loss, L = ce H + kd K (cvk_kd_loss_fwd / _bwd) ---------------------------------------------------------
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

// ---- multi-scale / flip test-time augmentation (cvk_tta_accumulate, cvk_tta_resize_input) ---------------------------------------
// One launch per view folds that view's logits into the [M][C] probability accumulator: a workgroup owns CE_CHUNK consecutive
// accumulator rows (a contiguous span of 256 C floats), one thread per pixel.  The accumulator side is staged through LDS exactly
// as k_ce_fwd stages its logits (a thread's own row is C floats apart from its neighbour's: read and written directly, a wave
// would touch 64 lines for 64 * 4 useful bytes per instruction), with pitch C + 1 so the row walk is conflict free.  The gather
// side is not staged: a pixel reads the two or four source rows around its sample position straight from global memory, as
// 16-byte vectors where the layout allows; neighbouring pixels share source rows, and a view's logits are at most a few tens of
// MB that the pass walks in order, so these reads are L2 hits after the first touch.  The resampled logits, their softmax and the
// arg-max stay in registers (CP = C rounded up to a multiple of 4 is the compile-time register count).
// Sample positions come from integers (include/cvk.h); the divisions are per row and per column, never per channel: the rows a
// workgroup covers are tabulated in LDS by its first threads, a thread computes its own column once.
constexpr int TTA_MAX_C = 32;            // classes held in registers per pixel
constexpr int TTA_MAX_DIM = 16384;       // (2 d + 1) in - out stays inside int32

struct TtaTap {
    int i0, i1;                          // lower / upper source index (upper clamped to the last one)
    float w0, w1;                        // their weights (1 - f, f)
};

__device__ __forceinline__ TtaTap tta_tap(int dst, int in, int out) {
    const int den = 2 * out;
    int num = (2 * dst + 1) * in - out;
    num = num < 0 ? 0 : num;
    const int i0 = num / den, rem = num - i0 * den;
    TtaTap t;
    t.i0 = i0;
    t.i1 = i0 + 1 < in ? i0 + 1 : in - 1;
    t.w1 = (float)rem / (float)den;      // both exact in fp32 (< 2^24): one rounding
    t.w0 = 1.f - t.w1;
    return t;
}

template <int CP, bool IDENT>
__global__ __launch_bounds__(CE_CHUNK) void k_tta_accumulate(const float* __restrict__ logits, int ld, int h, int w,
                                                            float* __restrict__ acc, int64_t* __restrict__ pred, int H, int W, int M,
                                                            int C, int flip, int first, int last, float inv_k) {
    extern __shared__ float lds[];       // CE_CHUNK accumulator rows, pitch C + 1
    __shared__ TtaTap s_row[CE_CHUNK];   // the output rows this workgroup's pixels lie in (at most CE_CHUNK of them, at W = 1)
    __shared__ int s_img[CE_CHUNK];
    const int pitch = C + 1;
    const int m0 = blockIdx.x * CE_CHUNK;
    const int rows = min(CE_CHUNK, M - m0);
    const int gy0 = m0 / W;                                   // uniform: first row of the [N * H] rows this workgroup touches
    const int nrows = (m0 + rows - 1) / W - gy0 + 1;
    for (int r = threadIdx.x; r < nrows; r += CE_CHUNK) {
        const int gy = gy0 + r, n = gy / H;
        s_row[r] = tta_tap(gy - n * H, h, H);
        s_img[r] = n;
    }
    if (!first) ce_chunk_load(acc + (size_t)m0 * C, lds, rows * C, C);
    __syncthreads();
    int bi = 0;
    if ((int)threadIdx.x < rows) {
        // (row, column) of pixel m0 + threadIdx.x relative to row gy0: off < W + CE_CHUNK < 2^24, so the fp32 quotient is off by one at most
        const int off = m0 - gy0 * W + (int)threadIdx.x;
        int q = (int)((float)off * (1.f / (float)W));
        int x = off - q * W;
        if (x < 0) { x += W; --q; } else if (x >= W) { x -= W; ++q; }
        const TtaTap ty = s_row[q];
        const TtaTap tx = tta_tap(flip ? W - 1 - x : x, w, W);
        const float* img = logits + (size_t)s_img[q] * h * w * ld;
        const float* r00 = img + ((size_t)ty.i0 * w + tx.i0) * ld;
        float v[CP];
        const bool vec = (C & 3) == 0 && (ld & 3) == 0 && ((uintptr_t)logits & 15u) == 0;        // uniform
        if (IDENT) {                                          // view at the output size: weights (1, 0) both ways, one source row
            if (vec) {
#pragma unroll
                for (int j = 0; j < CP / 4; ++j) {
                    const f32x4 a = reinterpret_cast<const f32x4*>(r00)[j];
                    v[4 * j] = a[0]; v[4 * j + 1] = a[1]; v[4 * j + 2] = a[2]; v[4 * j + 3] = a[3];
                }
            } else {
#pragma unroll
                for (int c = 0; c < CP; ++c) v[c] = c < C ? r00[c] : 0.f;
            }
        } else {
            const float* r01 = img + ((size_t)ty.i0 * w + tx.i1) * ld;
            const float* r10 = img + ((size_t)ty.i1 * w + tx.i0) * ld;
            const float* r11 = img + ((size_t)ty.i1 * w + tx.i1) * ld;
            if (vec) {
#pragma unroll
                for (int j = 0; j < CP / 4; ++j) {
                    const f32x4 a = reinterpret_cast<const f32x4*>(r00)[j], b = reinterpret_cast<const f32x4*>(r01)[j];
                    const f32x4 c = reinterpret_cast<const f32x4*>(r10)[j], d = reinterpret_cast<const f32x4*>(r11)[j];
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[4 * j + k] = ty.w0 * (tx.w0 * a[k] + tx.w1 * b[k]) + ty.w1 * (tx.w0 * c[k] + tx.w1 * d[k]);
                }
            } else {
#pragma unroll
                for (int c = 0; c < CP; ++c)
                    v[c] = c < C ? ty.w0 * (tx.w0 * r00[c] + tx.w1 * r01[c]) + ty.w1 * (tx.w0 * r10[c] + tx.w1 * r11[c]) : 0.f;
            }
        }
        float mx = v[0];
#pragma unroll
        for (int c = 1; c < CP; ++c)
            if (c < C) mx = fmaxf(mx, v[c]);
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) { v[c] = expf(v[c] - mx); se += v[c]; }
        const float inv = 1.f / se;
        float* p = lds + threadIdx.x * pitch;
        float best = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            if (c < C) {
                float s = v[c] * inv;
                if (!first) s = p[c] + s;
                if (last) s *= inv_k;
                p[c] = s;
                if (c == 0 || s > best || (s != s && best == best)) { best = s; bi = c; }   // k_argmax's rule on the stored values
            }
        }
    }
    __syncthreads();
    ce_chunk_store(acc + (size_t)m0 * C, lds, rows * C, C);
    if (last && (int)threadIdx.x < rows) pred[m0 + threadIdx.x] = bi;
}

// A view's network input: [N][3][H][W] of any strides -> NHWC-4 [N][h][w][4]; grid (ceil(w / 256), h, N), so the row tap is uniform
// per workgroup and a thread divides once, for its column.
__global__ __launch_bounds__(256) void k_tta_resize_input(const float* __restrict__ src, int64_t sN, int64_t sC, int64_t sH, int64_t sW,
                                                         float* __restrict__ dst, int H, int W, int h, int w, int flip) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
    if (x >= w) return;
    const TtaTap ty = tta_tap(y, H, h);
    const TtaTap tx = tta_tap(flip ? w - 1 - x : x, W, w);
    const float* b = src + n * sN;
    const int64_t o00 = ty.i0 * sH + tx.i0 * sW, o01 = ty.i0 * sH + tx.i1 * sW, o10 = ty.i1 * sH + tx.i0 * sW, o11 = ty.i1 * sH + tx.i1 * sW;
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = b + c * sC;
        o[c] = ty.w0 * (tx.w0 * p[o00] + tx.w1 * p[o01]) + ty.w1 * (tx.w0 * p[o10] + tx.w1 * p[o11]);
    }
    o[3] = 0.f;
    *reinterpret_cast<f32x4*>(dst + (((size_t)n * h + y) * w + x) * 4) = o;
}

// ---- sliding-window inference: the merge of overlapping windows' logits (cvk_window_merge) ---------------------------------------
// One launch per window folds that window's logits into the full-size map: a workgroup owns CE_CHUNK consecutive pixels of the window
// (a contiguous span of 256 ld floats of the logits; in `out` one contiguous span of C floats per window row it touches).  The pass is
// element-wise, so it runs in the order of the floats, not one pixel per thread: consecutive lanes move consecutive 16-byte vectors of
// both sides (full lines, as ce_chunk_load / ce_chunk_store move theirs), and a pixel's terms — where it lies in `out`, how many windows
// cover it, whether this window is the first or the last of them — come from a table in LDS that the pixel's thread fills once.  Those
// terms are integer closed forms of the grid (include/cvk.h), divided out per window row (tabulated by the workgroup's first threads, as
// k_tta_accumulate tabulates its row taps) and per column, never per channel.  Only the values of the pixels this window finishes go
// through LDS (pitch C + 1), for the arg-max: one thread per finished pixel walks its row with a scalar running best.
struct WinGrid {
    int H, W, hw, ww, sy, sx, gy, gx, iy, ix, y1, x1;
};

struct WinCover {
    int lo, hi;                          // first / last grid index whose window holds the position
};

// windows of `win` positions at min(i * stride, size - win), i < g, stride <= win: the i whose window holds position p
__device__ __forceinline__ WinCover win_cover(int p, int size, int win, int stride, int g) {
    WinCover c;
    c.lo = p < win ? 0 : min((p - win) / stride + 1, g - 1);
    c.hi = p >= size - win ? g - 1 : p / stride;
    return c;
}

constexpr int WIN_FIRST = 1, WIN_LAST = 2;

__global__ __launch_bounds__(CE_CHUNK) void k_window_merge(const float* __restrict__ logits, int ld, float* __restrict__ out,
                                                          int64_t* __restrict__ pred, int M, int C, WinGrid g) {
    extern __shared__ float lds[];       // the finished pixels' values, pitch C + 1 (no bytes when pred is null)
    __shared__ int s_row_pix[CE_CHUNK], s_row_cnt[CE_CHUNK], s_row_fl[CE_CHUNK];   // the window rows this workgroup touches (at most CE_CHUNK, at ww = 1)
    __shared__ int s_pix[CE_CHUNK], s_cnt[CE_CHUNK], s_fl[CE_CHUNK];               // its pixels: index in out / pred, count, WIN_FIRST | WIN_LAST
    const int pitch = C + 1;
    const int m0 = blockIdx.x * CE_CHUNK;
    const int rows = min(CE_CHUNK, M - m0);
    const int r0 = m0 / g.ww;                                 // uniform: first of the [N * hw] window rows this workgroup touches
    const int nrows = (m0 + rows - 1) / g.ww - r0 + 1;
    for (int r = threadIdx.x; r < nrows; r += CE_CHUNK) {
        const int wr = r0 + r, n = wr / g.hw, y = g.y1 + (wr - n * g.hw);
        const WinCover cy = win_cover(y, g.H, g.hw, g.sy, g.gy);
        s_row_pix[r] = (n * g.H + y) * g.W + g.x1;
        s_row_cnt[r] = cy.hi - cy.lo + 1;
        s_row_fl[r] = (g.iy == cy.lo ? WIN_FIRST : 0) | (g.iy == cy.hi ? WIN_LAST : 0);
    }
    __syncthreads();
    if ((int)threadIdx.x < rows) {
        // (row, column) of pixel m0 + threadIdx.x relative to row r0: off < ww + CE_CHUNK < 2^24, so the fp32 quotient is off by one at most
        const int off = m0 - r0 * g.ww + (int)threadIdx.x;
        int q = (int)((float)off * (1.f / (float)g.ww));
        int x = off - q * g.ww;
        if (x < 0) { x += g.ww; --q; } else if (x >= g.ww) { x -= g.ww; ++q; }
        const WinCover cx = win_cover(g.x1 + x, g.W, g.ww, g.sx, g.gx);
        s_pix[threadIdx.x] = s_row_pix[q] + x;
        s_cnt[threadIdx.x] = s_row_cnt[q] * (cx.hi - cx.lo + 1);
        s_fl[threadIdx.x] = s_row_fl[q] & ((g.ix == cx.lo ? WIN_FIRST : 0) | (g.ix == cx.hi ? WIN_LAST : 0));
    }
    __syncthreads();
    const float* lg = logits + (size_t)m0 * ld;
    if ((C & 3) == 0 && (ld & 3) == 0 && (((uintptr_t)logits | (uintptr_t)out) & 15u) == 0) {       // uniform
        const int nv = C >> 2;
        for (int v = threadIdx.x; v < rows * nv; v += CE_CHUNK) {
            const int p = v / nv, c = (v - p * nv) * 4;
            const int fl = s_fl[p];
            f32x4 s = *reinterpret_cast<const f32x4*>(lg + (size_t)p * ld + c);
            float* o = out + (size_t)s_pix[p] * C + c;
            if (!(fl & WIN_FIRST)) s = *reinterpret_cast<const f32x4*>(o) + s;
            if (fl & WIN_LAST) {
                const float d = (float)s_cnt[p];
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] = __fdiv_rn(s[k], d);
                if (pred) {
                    float* q = lds + p * pitch + c;
                    q[0] = s[0]; q[1] = s[1]; q[2] = s[2]; q[3] = s[3];
                }
            }
            *reinterpret_cast<f32x4*>(o) = s;
        }
    } else {
        for (int f = threadIdx.x; f < rows * C; f += CE_CHUNK) {
            const int p = f / C, c = f - p * C;
            const int fl = s_fl[p];
            float s = lg[(size_t)p * ld + c];
            float* o = out + (size_t)s_pix[p] * C + c;
            if (!(fl & WIN_FIRST)) s = *o + s;
            if (fl & WIN_LAST) {
                s = __fdiv_rn(s, (float)s_cnt[p]);
                if (pred) lds[p * pitch + c] = s;
            }
            *o = s;
        }
    }
    if (!pred) return;                                        // uniform
    __syncthreads();
    if ((int)threadIdx.x < rows && (s_fl[threadIdx.x] & WIN_LAST)) {
        const float* p = lds + threadIdx.x * pitch;
        float best = p[0];
        int bi = 0;
        for (int c = 1; c < C; ++c) {
            const float v = p[c];
            if (v > best || (v != v && best == best)) { best = v; bi = c; }       // k_argmax's rule on the stored values
        }
        pred[s_pix[threadIdx.x]] = bi;
    }
}

// uint8 HWC (cv2 BGR order kept) -> float32 NHWC, 4 channels per pixel (3 valid + zero pad): (v/255 - mean[c]) / std[c]
// = reference transforms.ToTensor + Normalize (transforms.py:485-538) with conf/settings.py:8-9 MEAN/STD passed in.
__global__ void k_preprocess_u8(const uint8_t* __restrict__ src, float* __restrict__ dst, long npix, float m0, float m1,
                                float m2, float r0, float r1, float r2) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long)gridDim.x * blockDim.x) {
        const uint8_t* p = src + i * 3;
        f32x4 v;
        v[0] = ((float)p[0] * (1.f / 255.f) - m0) * r0;
        v[1] = ((float)p[1] * (1.f / 255.f) - m1) * r1;
        v[2] = ((float)p[2] * (1.f / 255.f) - m2) * r2;
        v[3] = 0.f;
        *reinterpret_cast<f32x4*>(dst + i * 4) = v;
    }
}

// The reference's train / val transforms (transforms.py Resize -> RandomGaussianBlur -> RandomHorizontalFlip -> ColorJitter ->
// ToTensor -> Normalize, train.py:61-75) fused: a workgroup owns one AUG_TW x AUG_TH output tile of one image (grid x, y, N).
// Stage A resamples the tile plus a blur halo of R = (ksize-1)/2 pixels (REFLECT_101 in resized coordinates, cv2.GaussianBlur's
// default border) bilinearly from the source frame into LDS, rounded to uint8 values; stage B runs the separable Gaussian
// (horizontal into s_h, then vertical, fp32), rounds, applies the LUT and normalises with k_preprocess_u8's expression; the flip
// is applied at the store (the blur is symmetric and the LUT per pixel, so both commute with it).  R is uniform per image
// (blockIdx.z), hence a template argument chosen by one uniform switch.
constexpr int AUG_TW = 64, AUG_TH = 16, AUG_RMAX = 4;
constexpr int AUG_LW = AUG_TW + 2 * AUG_RMAX, AUG_LH = AUG_TH + 2 * AUG_RMAX;

struct AugArgs {
    const uint8_t* frames;
    const void* masks;
    int mask_bytes, Hs, Ws, H, W;
    double sy, sx;                      // Hs / H, Ws / W (cv2 computes both mappings in double)
    const cvk_augment_record* records;
    float m0, m1, m2, r0, r1, r2;
    float* out;
    int64_t* out_masks;
    uint8_t* out_u8;
};

// aug_reflect101, aug_round_u8 and aug_coord: crop_aug.h

template <int R>
__device__ __forceinline__ void aug_tile(const AugArgs& A, const cvk_augment_record* rec, float* s_in, float* s_h,
                                         const uint8_t* s_lut, bool use_lut) {
    constexpr int LWr = AUG_TW + 2 * R, LHr = AUG_TH + 2 * R;
    const int n = blockIdx.z, x0 = blockIdx.x * AUG_TW, y0 = blockIdx.y * AUG_TH;
    const uint8_t* src = A.frames + (size_t)n * A.Hs * A.Ws * 3;

    // stage A: resized uint8 values of the tile and its halo -> s_in[c][ly][lx] (row stride AUG_LW)
    for (int idx = threadIdx.x; idx < LHr * LWr; idx += blockDim.x) {
        const int ly = idx / LWr, lx = idx - ly * LWr;
        const int ry = aug_reflect101(y0 - R + ly, A.H), rx = aug_reflect101(x0 - R + lx, A.W);
        int iy0, iy1, ix0, ix1;
        float ay, ax;
        aug_coord(ry, A.sy, A.Hs, iy0, iy1, ay);
        aug_coord(rx, A.sx, A.Ws, ix0, ix1, ax);
        const uint8_t* p00 = src + ((size_t)iy0 * A.Ws + ix0) * 3;
        const uint8_t* p01 = src + ((size_t)iy0 * A.Ws + ix1) * 3;
        const uint8_t* p10 = src + ((size_t)iy1 * A.Ws + ix0) * 3;
        const uint8_t* p11 = src + ((size_t)iy1 * A.Ws + ix1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float top = (1.f - ax) * (float)p00[c] + ax * (float)p01[c];
            const float bot = (1.f - ax) * (float)p10[c] + ax * (float)p11[c];
            s_in[(c * AUG_LH + ly) * AUG_LW + lx] = aug_round_u8((1.f - ay) * top + ay * bot);
        }
    }
    float tp[2 * R + 1];
#pragma unroll
    for (int t = 0; t < 2 * R + 1; ++t) tp[t] = rec->taps[t];
    __syncthreads();

    if (R > 0) {  // horizontal pass over every staged row -> s_h[c][ly][tx] (row stride AUG_TW)
        for (int idx = threadIdx.x; idx < LHr * AUG_TW; idx += blockDim.x) {
            const int ly = idx / AUG_TW, tx = idx - ly * AUG_TW;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* row = s_in + (c * AUG_LH + ly) * AUG_LW + tx;
                float acc = 0.f;
#pragma unroll
                for (int t = 0; t < 2 * R + 1; ++t) acc = fmaf(tp[t], row[t], acc);
                s_h[(c * AUG_LH + ly) * AUG_TW + tx] = acc;
            }
        }
        __syncthreads();
    }

    const bool flip = rec->flip != 0;
    for (int idx = threadIdx.x; idx < AUG_TH * AUG_TW; idx += blockDim.x) {
        const int ty = idx / AUG_TW, tx = idx - ty * AUG_TW;
        const int y = y0 + ty, x = x0 + tx;
        if (y >= A.H || x >= A.W) continue;
        float u[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v;
            if (R > 0) {
                float acc = 0.f;
#pragma unroll
                for (int t = 0; t < 2 * R + 1; ++t) acc = fmaf(tp[t], s_h[(c * AUG_LH + ty + t) * AUG_TW + tx], acc);
                v = aug_round_u8(acc);
            } else {
                v = s_in[(c * AUG_LH + ty) * AUG_LW + tx];
            }
            u[c] = use_lut ? (float)s_lut[(int)v] : v;
        }
        const int xo = flip ? A.W - 1 - x : x;
        const size_t o = ((size_t)n * A.H + y) * A.W + xo;
        f32x4 f;
        f[0] = (u[0] * (1.f / 255.f) - A.m0) * A.r0;
        f[1] = (u[1] * (1.f / 255.f) - A.m1) * A.r1;
        f[2] = (u[2] * (1.f / 255.f) - A.m2) * A.r2;
        f[3] = 0.f;
        *reinterpret_cast<f32x4*>(A.out + o * 4) = f;
        if (A.out_u8) {
            A.out_u8[o * 3 + 0] = (uint8_t)u[0];
            A.out_u8[o * 3 + 1] = (uint8_t)u[1];
            A.out_u8[o * 3 + 2] = (uint8_t)u[2];
        }
        // mask: cv2 INTER_NEAREST, source floor(d * in / out) in double, clamped to the last row / column
        const int my = min((int)floor(y * A.sy), A.Hs - 1), mx = min((int)floor(x * A.sx), A.Ws - 1);
        const size_t mi = ((size_t)n * A.Hs + my) * A.Ws + mx;
        A.out_masks[o] = A.mask_bytes == 1 ? (int64_t)static_cast<const uint8_t*>(A.masks)[mi] : static_cast<const int64_t*>(A.masks)[mi];
    }
}

__global__ void __launch_bounds__(256) k_augment_u8(AugArgs A) {
    __shared__ float s_in[3 * AUG_LH * AUG_LW];
    __shared__ float s_h[3 * AUG_LH * AUG_TW];
    __shared__ uint8_t s_lut[256];
    const cvk_augment_record* rec = A.records + blockIdx.z;
    const bool use_lut = rec->use_lut != 0;
    if (use_lut)
        for (int i = threadIdx.x; i < 256; i += blockDim.x) s_lut[i] = rec->lut[i];   // visible after stage A's barrier
    const int k = rec->ksize;
    const int r = (k == 3 || k == 5 || k == 7 || k == 9) ? (k - 1) / 2 : 0;
    switch (r) {
        case 0: aug_tile<0>(A, rec, s_in, s_h, s_lut, use_lut); break;
        case 1: aug_tile<1>(A, rec, s_in, s_h, s_lut, use_lut); break;
        case 2: aug_tile<2>(A, rec, s_in, s_h, s_lut, use_lut); break;
        case 3: aug_tile<3>(A, rec, s_in, s_h, s_lut, use_lut); break;
        default: aug_tile<4>(A, rec, s_in, s_h, s_lut, use_lut); break;
    }
}

}  // namespace

extern "C" int cvk_augment_record_bytes(void) { return (int)sizeof(cvk_augment_record); }

extern "C" int cvk_augment_u8(const uint8_t* frames, const void* masks, int mask_bytes, int N, int Hs, int Ws, int H, int W,
                              const cvk_augment_record* records, const float* mean3, const float* std3, float* out,
                              int64_t* out_masks, uint8_t* out_u8, void* stream) {
    CVK_CHECK_ARG(frames && masks && records && mean3 && std3 && out && out_masks, "cvk_augment_u8: null pointer");
    CVK_CHECK_ARG(N > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0 && (mask_bytes == 1 || mask_bytes == 8) && cvk_aligned16(out),
                  "cvk_augment_u8: bad arguments");
    CVK_CHECK_ARG(N <= 65535 && cvk_cdiv(H, AUG_TH) <= 65535, "cvk_augment_u8: grid too large");
    CVK_CHECK_ARG(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "cvk_augment_u8: zero std");
    AugArgs a;
    a.frames = frames; a.masks = masks; a.mask_bytes = mask_bytes;
    a.Hs = Hs; a.Ws = Ws; a.H = H; a.W = W;
    a.sy = (double)Hs / H; a.sx = (double)Ws / W;
    a.records = records;
    a.m0 = mean3[0]; a.m1 = mean3[1]; a.m2 = mean3[2];
    a.r0 = 1.f / std3[0]; a.r1 = 1.f / std3[1]; a.r2 = 1.f / std3[2];
    a.out = out; a.out_masks = out_masks; a.out_u8 = out_u8;
    hipLaunchKernelGGL(k_augment_u8, dim3(cvk_cdiv(W, AUG_TW), cvk_cdiv(H, AUG_TH), N), dim3(256), 0, (hipStream_t)stream, a);
    CVK_LAUNCH_RETURN("cvk_augment_u8");
}

extern "C" int cvk_preprocess_u8(const uint8_t* src, float* dst, int N, int H, int W, const float* mean3, const float* std3,
                                 void* stream) {
    CVK_CHECK_ARG(src && dst && mean3 && std3 && N > 0 && H > 0 && W > 0 && cvk_aligned16(dst), "cvk_preprocess_u8: bad arguments");
    CVK_CHECK_ARG(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "cvk_preprocess_u8: zero std");
    const long npix = (long)N * H * W;
    const long b = (npix + 255) / 256;
    hipLaunchKernelGGL(k_preprocess_u8, dim3((int)(b < 8192 ? b : 8192)), dim3(256), 0, (hipStream_t)stream, src, dst, npix, mean3[0],
                       mean3[1], mean3[2], 1.f / std3[0], 1.f / std3[1], 1.f / std3[2]);
    CVK_LAUNCH_RETURN("cvk_preprocess_u8");
}

extern "C" int cvk_ce_blocks(int M) { return M > 0 ? cvk_cdiv(M, CE_ROWS_PER_BLOCK) : 0; }

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

extern "C" int cvk_ohem_scratch_bytes(int M) { return M > 0 ? (int)sizeof(unsigned) * (OHEM_HEAD_WORDS + 4 * cvk_ce_blocks(M)) : 0; }

extern "C" int cvk_ohem_record_floats(void) { return OHEM_RECORD_FLOATS; }

extern "C" int cvk_ohem_ce_fwd(const float* logits, int ld, const int64_t* target, const float* weight, float loss_thresh, int min_kept,
                               void* scratch, float* record, float* loss_px, int M, int C, int ignore_index, void* stream) {
    CVK_CHECK_ARG(logits && target && scratch && record && loss_px, "cvk_ohem_ce_fwd: null pointer");
    CVK_CHECK_ARG(M > 0 && C > 0 && C <= CE_EX_MAX_C && ld >= C, "cvk_ohem_ce_fwd: bad arguments");
    CVK_CHECK_ARG(min_kept >= 1, "cvk_ohem_ce_fwd: min_kept must be at least 1");
    CVK_CHECK_ARG(loss_thresh >= 0.f && loss_thresh <= 3.4028235e38f, "cvk_ohem_ce_fwd: loss_thresh must be finite and not negative");
    const int nb = cvk_ce_blocks(M);
    hipStream_t s = (hipStream_t)stream;
    unsigned* sc = static_cast<unsigned*>(scratch);
    hipLaunchKernelGGL(k_ohem_clear, dim3(cvk_cdiv(OHEM_HEAD_WORDS, 256)), dim3(256), 0, s, sc);
    if (ld <= OHEM_MAX_LD)
        hipLaunchKernelGGL(k_ohem_fwd<true>, dim3(nb), dim3(256), CE_CHUNK * (ld + 1) * sizeof(float), s, logits, ld, target, loss_px, sc, M,
                           C, ignore_index);
    else
        hipLaunchKernelGGL(k_ohem_fwd<false>, dim3(nb), dim3(256), 0, s, logits, ld, target, loss_px, sc, M, C, ignore_index);
    const int rb = cvk_cdiv(M, 2048) < OHEM_REFINE_MAX_BLOCKS ? cvk_cdiv(M, 2048) : OHEM_REFINE_MAX_BLOCKS;
    hipLaunchKernelGGL(k_ohem_refine<2>, dim3(rb), dim3(256), 0, s, loss_px, M, sc, min_kept);
    hipLaunchKernelGGL(k_ohem_refine<3>, dim3(rb), dim3(256), 0, s, loss_px, M, sc, min_kept);
    hipLaunchKernelGGL(k_ohem_reduce, dim3(nb), dim3(256), 0, s, loss_px, target, weight, loss_thresh, sc, nb, M, C, ignore_index);
    hipLaunchKernelGGL(k_ohem_finish, dim3(1), dim3(256), 0, s, sc, nb, loss_thresh, record);
    CVK_LAUNCH_RETURN("cvk_ohem_ce_fwd");
}

extern "C" int cvk_ohem_ce_bwd(const float* logits, int ld, const int64_t* target, const float* weight, const float* record,
                               const float* loss_px, const float* grad_out, float scale, float* dlogits, int ld_d, int M, int C,
                               int ignore_index, void* stream) {
    CVK_CHECK_ARG(logits && target && record && loss_px && dlogits, "cvk_ohem_ce_bwd: null pointer");
    CVK_CHECK_ARG(M > 0 && C > 0 && C <= CE_EX_MAX_C && ld >= C && ld_d >= C, "cvk_ohem_ce_bwd: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (ld <= CE_MAX_LD)
        hipLaunchKernelGGL(k_ohem_bwd, dim3(cvk_ce_blocks(M)), dim3(256), CE_CHUNK * (ld + 1) * sizeof(float), s, logits, ld, target,
                           weight, record, loss_px, grad_out, scale, dlogits, ld_d, M, C, ignore_index);
    else
        hipLaunchKernelGGL(k_ohem_bwd_rows, dim3(cvk_cdiv(M, 256) < 8192 ? cvk_cdiv(M, 256) : 8192), dim3(256), 0, s, logits, ld, target,
                           weight, record, loss_px, grad_out, scale, dlogits, ld_d, M, C, ignore_index);
    CVK_LAUNCH_RETURN("cvk_ohem_ce_bwd");
}

extern "C" int64_t cvk_lovasz_workspace_bytes(int M, int C, int segments) {
    LvPlan p;
    return lv_plan(M, C, segments, &p) ? (int64_t)p.bytes : 0;
}

extern "C" int cvk_lovasz_record_floats(void) { return LV_RECORD_FLOATS; }

extern "C" int64_t cvk_lovasz_sort_dest(int64_t seg_len, int64_t segment, int64_t digit_base, int64_t wg_base, int64_t rank) {
    return lv_sort_dest(seg_len, segment, digit_base, wg_base, rank);
}

extern "C" int64_t cvk_lovasz_sort_count_index(int64_t work_groups, int64_t segment, int64_t digit, int64_t work_group) {
    return lv_count_index(work_groups, segment, digit, work_group);
}

static int lovasz_check(const char* who, float lovasz, float ce, const float* weight, int per_image, int N, int pixels_per_image, int ld,
                        int ld_g, int C, LvPlan* plan) {
    CVK_CHECK_ARG(lovasz > 0.f && lovasz <= 3.4028235e38f, "%s: lovasz must be finite and greater than 0", who);
    CVK_CHECK_ARG(ce >= 0.f && ce <= 3.4028235e38f, "%s: ce must be finite and not negative", who);
    CVK_CHECK_ARG(weight == nullptr || ce > 0.f, "%s: class weights enter the cross-entropy term only, and ce is 0", who);
    CVK_CHECK_ARG(per_image == 0 || per_image == 1, "%s: per_image must be 0 or 1", who);
    CVK_CHECK_ARG(N > 0 && pixels_per_image > 0 && (long long)N * pixels_per_image < (1ll << 31), "%s: bad batch size", who);
    CVK_CHECK_ARG(C > 0 && C <= CE_EX_MAX_C && ld >= C && ld_g >= C, "%s: bad arguments", who);
    CVK_CHECK_ARG(lv_plan(N * pixels_per_image, C, per_image ? N : 1, plan), "%s: unsupported size (a segment of 2^30 pixels or more, "
                  "or more than 65535 segments)", who);
    return CVK_OK;
}

extern "C" int cvk_lovasz_softmax_fwd(const float* logits, int ld, const int64_t* target, const float* weight, float lovasz, float ce,
                                      int classes_mode, int per_image, int N, int pixels_per_image, void* workspace, float* record,
                                      float* gmap, int ld_g, int C, int ignore_index, void* stream) {
    CVK_CHECK_ARG(logits && target && workspace && record && gmap, "cvk_lovasz_softmax_fwd: null pointer");
    CVK_CHECK_ARG(classes_mode == CVK_LOVASZ_PRESENT || classes_mode == CVK_LOVASZ_ALL, "cvk_lovasz_softmax_fwd: bad classes_mode");
    CVK_CHECK_ARG(((uintptr_t)workspace & 15u) == 0, "cvk_lovasz_softmax_fwd: the workspace must be 16-byte aligned");
    LvPlan p;
    const int rc = lovasz_check("cvk_lovasz_softmax_fwd", lovasz, ce, weight, per_image, N, pixels_per_image, ld, ld_g, C, &p);
    if (rc != CVK_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    lv_elem* bufs[2] = {reinterpret_cast<lv_elem*>(ws), reinterpret_cast<lv_elem*>(ws + p.b)};
    unsigned* counts = reinterpret_cast<unsigned*>(ws + p.counts);
    unsigned* tot = reinterpret_cast<unsigned*>(ws + p.tot);
    unsigned* tilefg = reinterpret_cast<unsigned*>(ws + p.tilefg);
    double* partial = reinterpret_cast<double*>(ws + p.partial);
    double* pairl = reinterpret_cast<double*>(ws + p.pairl);
    double* segl = reinterpret_cast<double*>(ws + p.segl);
    unsigned* ctr = reinterpret_cast<unsigned*>(ws + p.ctr);
    float* invk = reinterpret_cast<float*>(ws + p.invk);
    float* cepart = reinterpret_cast<float*>(ws + p.cepart);
    const int SC = p.S * C, nctr = SC + p.S + 1, want_ce = ce > 0.f ? 1 : 0;
    hipLaunchKernelGGL(k_lv_clear, dim3(cvk_cdiv(nctr, 256)), dim3(256), 0, s, ctr, nctr);
    const dim3 ge(cvk_cdiv(p.P, CE_ROWS_PER_BLOCK), p.S);
    if (ld <= LV_MAX_LD)
        hipLaunchKernelGGL(k_lv_err<true>, ge, dim3(256), CE_CHUNK * (ld + 1) * sizeof(float), s, logits, ld, target, weight, want_ce,
                           bufs[0], ctr, cepart, p.nbe, p.P, p.S, C, ignore_index);
    else
        hipLaunchKernelGGL(k_lv_err<false>, ge, dim3(256), 0, s, logits, ld, target, weight, want_ce, bufs[0], ctr, cepart, p.nbe, p.P,
                           p.S, C, ignore_index);
    const dim3 gs(p.nwg, SC);
    for (int pass = 0; pass < LV_PASSES; ++pass) {
        const int shift = pass * CVK_LOVASZ_DIGIT_BITS;
        const lv_elem* in = bufs[pass & 1];
        hipLaunchKernelGGL(k_lv_count, gs, dim3(256), 0, s, in, p.P, shift, counts, p.nwg);
        hipLaunchKernelGGL(k_lv_scan, dim3(LV_BINS, SC), dim3(256), 0, s, counts, tot, p.nwg);
        hipLaunchKernelGGL(k_lv_scatter, gs, dim3(256), 0, s, in, bufs[(pass & 1) ^ 1], p.P, shift, counts, tot, p.nwg);
    }
    hipLaunchKernelGGL(k_lv_fgcount, gs, dim3(256), 0, s, bufs[0], p.P, tilefg, p.nwg);
    hipLaunchKernelGGL(k_lv_weight, gs, dim3(256), 0, s, bufs[0], p.P, p.S, C, p.nwg, tilefg, ctr, classes_mode == CVK_LOVASZ_ALL ? 1 : 0,
                       gmap, ld_g, partial);
    hipLaunchKernelGGL(k_lv_pairsum, dim3(SC), dim3(256), 0, s, partial, p.nwg, pairl);
    hipLaunchKernelGGL(k_lv_finish, dim3(1), dim3(256), 0, s, pairl, segl, ctr, invk, cepart, p.nbe, p.S, C,
                       classes_mode == CVK_LOVASZ_ALL ? 1 : 0, lovasz, ce, record);
    CVK_LAUNCH_RETURN("cvk_lovasz_softmax_fwd");
}

extern "C" int cvk_lovasz_softmax_bwd(const float* logits, int ld, const int64_t* target, const float* weight, float lovasz, float ce,
                                      int per_image, int N, int pixels_per_image, const void* workspace, const float* record,
                                      const float* gmap, int ld_g, const float* grad_out, float scale, float* dlogits, int ld_d, int C,
                                      int ignore_index, void* stream) {
    CVK_CHECK_ARG(logits && target && workspace && record && gmap && dlogits, "cvk_lovasz_softmax_bwd: null pointer");
    LvPlan p;
    const int rc = lovasz_check("cvk_lovasz_softmax_bwd", lovasz, ce, weight, per_image, N, pixels_per_image, ld, ld_g, C, &p);
    if (rc != CVK_OK) return rc;
    CVK_CHECK_ARG(ld_d >= C, "cvk_lovasz_softmax_bwd: bad arguments");
    const float* invk = reinterpret_cast<const float*>(static_cast<const char*>(workspace) + p.invk);
    const int M = N * pixels_per_image;
    hipStream_t s = (hipStream_t)stream;
    if (ld <= LV_MAX_LD)
        hipLaunchKernelGGL(k_lv_bwd<true>, dim3(cvk_ce_blocks(M)), dim3(256), CE_CHUNK * (ld + 1) * sizeof(float), s, logits, ld, target,
                           weight, lovasz, ce, record, invk, gmap, ld_g, grad_out, scale, dlogits, ld_d, M, p.P, C, ignore_index);
    else
        hipLaunchKernelGGL(k_lv_bwd<false>, dim3(cvk_ce_blocks(M)), dim3(256), 0, s, logits, ld, target, weight, lovasz, ce, record, invk,
                           gmap, ld_g, grad_out, scale, dlogits, ld_d, M, p.P, C, ignore_index);
    CVK_LAUNCH_RETURN("cvk_lovasz_softmax_bwd");
}

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

extern "C" int cvk_seg_loss_part_floats(int M, int C) {
    return M > 0 && C > 0 && C <= CE_EX_MAX_C ? (SEG_PART_HEAD + 3 * C) * cvk_ce_blocks(M) : 0;
}

extern "C" int cvk_seg_loss_record_floats(int C) { return C > 0 && C <= CE_EX_MAX_C ? SEG_REC_HEAD + 3 * C : 0; }

// x >= 0 is false for NaN
static bool seg_loss_args_ok(int M, int C, int ld, float ce, float dice, float gamma) {
    return M > 0 && C > 0 && C <= CE_EX_MAX_C && ld >= C && ce >= 0.f && dice >= 0.f && gamma >= 0.f && ce <= 3.0e38f && dice <= 3.0e38f &&
           gamma <= 3.0e38f;
}

static int seg_chunk_rows(int pitch) { return SEG_TILE_FLOATS / pitch < CE_CHUNK ? SEG_TILE_FLOATS / pitch : CE_CHUNK; }

extern "C" int cvk_seg_loss_fwd(const float* logits, int ld, const int64_t* target, const float* weight, float ce, float dice,
                                float focal_gamma, float dice_smooth, int dice_average, float* part, float* record, int M, int C,
                                int ignore_index, void* stream) {
    CVK_CHECK_ARG(logits && target && part && record, "cvk_seg_loss_fwd: null pointer");
    CVK_CHECK_ARG(seg_loss_args_ok(M, C, ld, ce, dice, focal_gamma) && dice_smooth >= 0.f && dice_smooth <= 3.0e38f,
                  "cvk_seg_loss_fwd: bad arguments");
    CVK_CHECK_ARG(ce > 0.f || dice > 0.f, "cvk_seg_loss_fwd: ce and dice are both zero");
    CVK_CHECK_ARG(dice_average == CVK_DICE_PRESENT || dice_average == CVK_DICE_ALL, "cvk_seg_loss_fwd: bad dice_average code");
    const int nb = cvk_ce_blocks(M);
    hipStream_t s = (hipStream_t)stream;
    if (ld <= CE_MAX_LD) {
        const int rows = seg_chunk_rows(ld + 1);
        hipLaunchKernelGGL(k_seg_fwd<true>, dim3(nb), dim3(256), (size_t)rows * (ld + 1) * sizeof(float), s, logits, ld, target, weight, ce,
                           dice, focal_gamma, part, nb, M, C, ignore_index, rows);
    } else {
        const int rows = seg_chunk_rows(C + 1);
        hipLaunchKernelGGL(k_seg_fwd<false>, dim3(nb), dim3(256), (size_t)rows * (C + 1) * sizeof(float), s, logits, ld, target, weight, ce,
                           dice, focal_gamma, part, nb, M, C, ignore_index, rows);
    }
    hipLaunchKernelGGL(k_seg_finish, dim3(1), dim3(SEG_FINISH_THREADS), 0, s, part, nb, C, ce, dice, dice_smooth, dice_average, record);
    CVK_LAUNCH_RETURN("cvk_seg_loss_fwd");
}

extern "C" int cvk_seg_loss_bwd(const float* logits, int ld, const int64_t* target, const float* weight, float ce, float dice,
                                float focal_gamma, const float* record, const float* grad_out, float scale, float* dlogits, int ld_d,
                                int M, int C, int ignore_index, void* stream) {
    CVK_CHECK_ARG(logits && target && record && dlogits, "cvk_seg_loss_bwd: null pointer");
    CVK_CHECK_ARG(seg_loss_args_ok(M, C, ld, ce, dice, focal_gamma) && ld_d >= C, "cvk_seg_loss_bwd: bad arguments");
    CVK_CHECK_ARG(ce > 0.f || dice > 0.f, "cvk_seg_loss_bwd: ce and dice are both zero");
    hipStream_t s = (hipStream_t)stream;
    if (ld <= CE_MAX_LD) {
        const int rows = seg_chunk_rows(ld + 1);
        hipLaunchKernelGGL(k_seg_bwd, dim3(cvk_ce_blocks(M)), dim3(256), (size_t)rows * (ld + 1) * sizeof(float), s, logits, ld, target, weight,
                           ce, dice, focal_gamma, record, grad_out, scale, dlogits, ld_d, M, C, ignore_index, rows);
    } else {
        hipLaunchKernelGGL(k_seg_bwd_rows, dim3(cvk_cdiv(M, 256) < 8192 ? cvk_cdiv(M, 256) : 8192), dim3(256), 0, s, logits, ld, target,
                           weight, ce, dice, focal_gamma, record, grad_out, scale, dlogits, ld_d, M, C, ignore_index);
    }
    CVK_LAUNCH_RETURN("cvk_seg_loss_bwd");
}

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

template <bool IDENT>
static bool tta_launch(int CP, int nb, size_t lds_bytes, hipStream_t s, const float* logits, int ld, int h, int w, float* acc, int64_t* pred,
                       int H, int W, int M, int C, int flip, int first, int last, float inv_k) {
#define TTA_CASE(cp)                                                                                                              \
    case cp:                                                                                                                      \
        hipLaunchKernelGGL((k_tta_accumulate<cp, IDENT>), dim3(nb), dim3(CE_CHUNK), lds_bytes, s, logits, ld, h, w, acc, pred, H, W, M, C, \
                           flip, first, last, inv_k);                                                                             \
        return true;
    switch (CP) {
        TTA_CASE(4) TTA_CASE(8) TTA_CASE(12) TTA_CASE(16) TTA_CASE(20) TTA_CASE(24) TTA_CASE(28) TTA_CASE(32)
    }
#undef TTA_CASE
    return false;
}

extern "C" int cvk_tta_accumulate(const float* logits, int ld, int h, int w, float* acc, int64_t* pred, int N, int H, int W, int C,
                                  int flip, int first, int last, float inv_k, void* stream) {
    CVK_CHECK_ARG(logits && acc && (pred || !last), "cvk_tta_accumulate: null pointer");
    CVK_CHECK_ARG(C <= TTA_MAX_C, "cvk_tta_accumulate: %d classes, the kernel holds at most %d per pixel in registers", C, TTA_MAX_C);
    CVK_CHECK_ARG(N > 0 && H > 0 && W > 0 && h > 0 && w > 0 && C > 0 && ld >= C && H <= TTA_MAX_DIM && W <= TTA_MAX_DIM &&
                      h <= TTA_MAX_DIM && w <= TTA_MAX_DIM && inv_k > 0.f && inv_k <= 3.0e38f,
                  "cvk_tta_accumulate: bad arguments");
    CVK_CHECK_ARG((int64_t)N * H * W * C < 2147483647LL - CE_CHUNK * TTA_MAX_C, "cvk_tta_accumulate: accumulator of 2^31 values or more");
    const int M = N * H * W, nb = cvk_cdiv(M, CE_CHUNK), CP = (C + 3) / 4 * 4;
    const size_t lds_bytes = (size_t)CE_CHUNK * (C + 1) * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    const bool ok = h == H && w == W
                        ? tta_launch<true>(CP, nb, lds_bytes, s, logits, ld, h, w, acc, pred, H, W, M, C, flip, first, last, inv_k)
                        : tta_launch<false>(CP, nb, lds_bytes, s, logits, ld, h, w, acc, pred, H, W, M, C, flip, first, last, inv_k);
    CVK_CHECK_ARG(ok, "cvk_tta_accumulate: no kernel for %d classes", C);
    CVK_LAUNCH_RETURN("cvk_tta_accumulate");
}

extern "C" int cvk_tta_resize_input(const float* src, int64_t sN, int64_t sC, int64_t sH, int64_t sW, float* dst, int N, int H, int W,
                                    int h, int w, int flip, void* stream) {
    CVK_CHECK_ARG(src && dst, "cvk_tta_resize_input: null pointer");
    CVK_CHECK_ARG(N > 0 && H > 0 && W > 0 && h > 0 && w > 0 && H <= TTA_MAX_DIM && W <= TTA_MAX_DIM && h <= TTA_MAX_DIM && w <= TTA_MAX_DIM &&
                      cvk_aligned16(dst),
                  "cvk_tta_resize_input: bad arguments");
    CVK_CHECK_ARG(N <= 65535, "cvk_tta_resize_input: grid too large");
    hipLaunchKernelGGL(k_tta_resize_input, dim3(cvk_cdiv(w, 256), h, N), dim3(256), 0, (hipStream_t)stream, src, sN, sC, sH, sW, dst, H, W,
                       h, w, flip);
    CVK_LAUNCH_RETURN("cvk_tta_resize_input");
}

extern "C" int cvk_window_merge(const float* logits, int ld, float* out, int64_t* pred, int N, int H, int W, int C, int hc, int wc,
                                int sy, int sx, int iy, int ix, void* stream) {
    CVK_CHECK_ARG(logits && out, "cvk_window_merge: null pointer");
    CVK_CHECK_ARG(C <= TTA_MAX_C, "cvk_window_merge: %d classes, the kernel serves at most %d", C, TTA_MAX_C);
    CVK_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0 && ld >= C && hc > 0 && wc > 0 && H <= TTA_MAX_DIM && W <= TTA_MAX_DIM &&
                      hc <= TTA_MAX_DIM && wc <= TTA_MAX_DIM,
                  "cvk_window_merge: bad arguments");
    CVK_CHECK_ARG(sy >= 1 && sy <= hc && sx >= 1 && sx <= wc, "cvk_window_merge: stride (%d, %d) outside 1..crop (%d, %d)", sy, sx, hc, wc);
    CVK_CHECK_ARG((int64_t)N * H * W * C < 2147483647LL, "cvk_window_merge: output of 2^31 values or more");
    WinGrid g;
    g.H = H; g.W = W; g.sy = sy; g.sx = sx; g.iy = iy; g.ix = ix;
    g.hw = hc < H ? hc : H;
    g.ww = wc < W ? wc : W;
    g.gy = (H - g.hw + sy - 1) / sy + 1;
    g.gx = (W - g.ww + sx - 1) / sx + 1;
    CVK_CHECK_ARG(iy >= 0 && iy < g.gy && ix >= 0 && ix < g.gx, "cvk_window_merge: window (%d, %d) outside the %d x %d grid", iy, ix, g.gy,
                  g.gx);
    g.y1 = iy * sy < H - g.hw ? iy * sy : H - g.hw;
    g.x1 = ix * sx < W - g.ww ? ix * sx : W - g.ww;
    const int M = N * g.hw * g.ww;
    const size_t lds_bytes = pred ? (size_t)CE_CHUNK * (C + 1) * sizeof(float) : 0;
    hipLaunchKernelGGL(k_window_merge, dim3(cvk_cdiv(M, CE_CHUNK)), dim3(CE_CHUNK), lds_bytes, (hipStream_t)stream, logits, ld, out, pred, M, C,
                       g);
    CVK_LAUNCH_RETURN("cvk_window_merge");
}

// ---- library-wide pieces ---------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void cvk_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" int cvk_version(void) { return CVK_VERSION; }
#ifndef CVK_ABI_HASH
#error "CVK_ABI_HASH is not defined: build through csrc/Makefile (it hashes include/cvk.h)"
#endif
extern "C" uint64_t cvk_abi_hash(void) { return CVK_ABI_HASH; }
extern "C" const char* cvk_last_error_string(void) { return g_err; }
