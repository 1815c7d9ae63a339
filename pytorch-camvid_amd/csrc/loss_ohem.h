#pragma once
// loss_ohem.h: OHEM cross-entropy (cvk_ohem_ce_fwd / _bwd).
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
// The staging and the weighted pixel terms come from loss_rows.h.
#include "cvk_common.h"
#include "loss_rows.h"

namespace {

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

}  // namespace

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
