#pragma once
// loss_seg.h: fused focal + soft-Dice loss (cvk_seg_loss_fwd / _bwd).
// L = ce F + dice D over the valid pixels of the batch, p = softmax(x), t = target, q = 1 - p[t]:
//   F = sum w[t] q^gamma (lse - x[t]) / sum w[t]
//   D = 1 - (1 / K) sum_{c in S} (2 I_c + s) / (P_c + T_c + s),  I_c = sum p[c] [t = c], P_c = sum p[c], T_c = sum [t = c]
// One forward pass serves both terms: a chunk of pixel rows is staged as in k_ce_fwd_ex, thread = pixel leaves exp(x - max) in the
// tile and (target, 1 / sum exp) beside it, then thread = (class, row segment) walks its column over its rows.  The segment sums are
// folded class by class in segment order, the workgroup partials by k_seg_finish in fp64: every sum has one fixed order and there is
// no float atomic.  ld > CE_MAX_LD: the same kernel with STAGED = false, a thread reads its pixel's row from global memory and the
// tile (pitch C + 1) holds the exponentials only.  A chunk is as many rows as fit SEG_TILE_FLOATS, 256 at most.
// The chunk staging, ce_ex_stage_w and CE_EX_MAX_C come from loss_rows.h.
#include "cvk_common.h"
#include "loss_rows.h"

namespace {

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

}  // namespace

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
