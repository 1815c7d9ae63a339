#pragma once
// loss_lovasz.h: Lovász-softmax (cvk_lovasz_softmax_fwd / _bwd).
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
// The staging, the weighted pixel terms, CE_EX_MAX_C and k_lv_clear (which zeroes the counters) come from loss_rows.h.
#include "cvk_common.h"
#include "loss_rows.h"

namespace {

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

}  // namespace

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
