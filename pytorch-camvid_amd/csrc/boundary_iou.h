#pragma once
// ---- chessboard depth, Boundary IoU (Cheng et al., CVPR 2021) and trimap counts (cvk_cheb_depth, cvk_boundary_iou_counts; the
// definitions are in include/cvk.h) ------------------------------------------------------------------------------------------------
// A pixel's code is bf_code of boundary_f1.h, unchanged; here void and BF_OTHER are codes like any other and bound the regions beside
// them.  depth0(z) = how many 3 x 3 erosions the pixel survives inside the region of its own code, plus one; with lim = max_depth + 1
// every stored distance is min(., lim), which changes no comparison against a band of at most max_depth.  Three kernels:
//   k_cheb_rows    work-group = CHEB_ROW_PIXELS / W whole rows (at least one), their codes in LDS; the bounded outward search along
//                  the row for the nearest other code -> code uint8 [M], h uint8 [M].  A work-group holds whole rows and walks them
//                  256 threads at a time against the staged row, so a run that crosses such a chunk's edge is searched like any
//                  other.  With W a multiple of 4 a thread takes 4 pixels: 16-byte loads, 32-bit stores.
//   k_cheb_cols    work-group = (image, strip of TX columns, CHEB_COL_TH rows) with a halo of min(max_depth, H - 1) rows, codes and h in
//                  LDS; depth0 = min over y' of max(|y - y'|, g), the walk up and the walk down each end at the first row of another
//                  code, at the image's edge and at |y - y'| >= best <= lim, so neither leaves the halo.  A thread takes 4 neighbouring
//                  pixels of a row (32-bit accesses when W is a multiple of 4).
//   k_biou_counts  work-group = CHEB_CNT_PIXELS pixels of one image: 4 B per pixel (two codes, two depths), the border term in closed
//                  form, six rows of K counters (+ nw K K trimap bins) in LDS.  A thread takes 16 neighbouring pixels (one 16-byte load
//                  per map when H W is a multiple of 16) and keeps its counts in registers while the pair of codes stays the same.
// Integers only: LDS counters are 32-bit (at most CHEB_CNT_PIXELS each), flushed by 64-bit global atomics where non-zero, so neither the
// order of arrival nor the tiling changes a bit.  Every loop is bounded by lim or by the tile.
// LDS: k_cheb_rows max(W, CHEB_ROW_PIXELS) B; k_cheb_cols 2 TX (CHEB_COL_TH + 2 halo) B: 14 KiB at max_depth 24 (TX 64), 36 KiB at 254
// (TX 32); k_biou_counts 768 B + 4 nw K K B (32 KiB at nw 8, K 32).
#include "cvk_common.h"
#include "boundary_f1.h"

namespace {

constexpr int CHEB_MAX_DEPTH = 254, CHEB_MAX_W = 32768, CHEB_MAX_WIDTHS = 8;
constexpr int CHEB_ROW_PIXELS = 2048;                      // k_cheb_rows: pixels of a work-group when rows are shorter than this
constexpr int CHEB_COL_TH = 64;                            // k_cheb_cols: interior rows of a work-group
constexpr int CHEB_CNT_PIXELS = 4096;                      // k_biou_counts: pixels of a work-group, 16 per thread
constexpr int BIOU_ROWS = 6;

struct ChebWidths {
    int w[CHEB_MAX_WIDTHS];
};

// distance from pixel i (column x) of a staged row to the nearest other code in that row, min(., lim); i - k and i + k stay in the row
__device__ __forceinline__ int cheb_row_h(const unsigned char* row, int i, int x, int W, int lim) {
    const unsigned char c = row[i];
    if (c >= BF_MAX_K) return 0;
    for (int k = 1; k < lim; ++k) {
        const bool l = x - k >= 0, r = x + k < W;
        if (!l && !r) break;
        if ((l && row[i - k] != c) || (r && row[i + k] != c)) return k;
    }
    return lim;
}

// VEC: W is a multiple of 4, the maps are 16-byte and the byte maps 4-byte aligned: a thread takes 4 pixels, two 16-byte loads per map
template <bool VEC>
__global__ __launch_bounds__(256) void k_cheb_rows(const int64_t* __restrict__ map, const int64_t* __restrict__ void_from,
                                                  unsigned char* __restrict__ code, unsigned char* __restrict__ hout, size_t rows_total,
                                                  int W, int R, int K, int ignore, int lim) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cheb_row[];
    const size_t r0 = (size_t)blockIdx.x * R;
    const int nr = (int)min((size_t)R, rows_total - r0), cnt = nr * W;
    const size_t base = r0 * W;
    const bool own = void_from == map;
    if (VEC) {
        for (int i = 4 * threadIdx.x; i < cnt; i += 1024) {
            const longlong2* pm = reinterpret_cast<const longlong2*>(map + base + i);
            const longlong2* pv = reinterpret_cast<const longlong2*>(void_from + base + i);
            const longlong2 m0 = pm[0], m1 = pm[1];
            const longlong2 v0 = own ? m0 : pv[0], v1 = own ? m1 : pv[1];
            const unsigned w = (unsigned)bf_code(m0.x, v0.x, K, ignore) | ((unsigned)bf_code(m0.y, v0.y, K, ignore) << 8) |
                               ((unsigned)bf_code(m1.x, v1.x, K, ignore) << 16) | ((unsigned)bf_code(m1.y, v1.y, K, ignore) << 24);
            *reinterpret_cast<unsigned*>(cheb_row + i) = w;
        }
    } else {
        for (int i = threadIdx.x; i < cnt; i += 256) {
            const int64_t m = map[base + i];
            cheb_row[i] = bf_code(m, own ? m : void_from[base + i], K, ignore);
        }
    }
    __syncthreads();
    if (VEC) {
        for (int i = 4 * threadIdx.x; i < cnt; i += 1024) {
            const int x = i % W;                           // the four pixels share a row: W % 4 == 0
            unsigned h = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) h |= (unsigned)cheb_row_h(cheb_row, i + k, x + k, W, lim) << (8 * k);
            *reinterpret_cast<unsigned*>(code + base + i) = *reinterpret_cast<const unsigned*>(cheb_row + i);
            *reinterpret_cast<unsigned*>(hout + base + i) = h;
        }
    } else {
        for (int i = threadIdx.x; i < cnt; i += 256) {
            code[base + i] = cheb_row[i];
            hout[base + i] = (unsigned char)cheb_row_h(cheb_row, i, i % W, W, lim);
        }
    }
}

__device__ __forceinline__ int cheb_border_term(int x, int y, int H, int W) { return 1 + min(min(x, W - 1 - x), min(y, H - 1 - y)); }

// depth0 of the class pixel at LDS position j (image row y) of a staged strip: the walk up and the walk down
__device__ __forceinline__ int cheb_col_depth(const unsigned char* sc, const unsigned char* sh, int j, int y, int H, int TX) {
    const unsigned char c = sc[j];
    int best = sh[j];                                      // 1 <= best <= lim = max_depth + 1, so |dy| <= max_depth below
    for (int dy = 1; dy < best && y - dy >= 0; ++dy) {
        const int q = j - dy * TX;
        if (sc[q] != c) {
            best = dy;
            break;
        }
        best = min(best, max(dy, (int)sh[q]));
    }
    for (int dy = 1; dy < best && y + dy < H; ++dy) {
        const int q = j + dy * TX;
        if (sc[q] != c) {
            best = dy;
            break;
        }
        best = min(best, max(dy, (int)sh[q]));
    }
    return best;
}

// grid N * chunks * strips.  LDS: codes [SR][TX], h [SR][TX], SR = CHEB_COL_TH + 2 halo; LDS row j is image row y0 - halo + j (rows
// outside the image are neither written nor read).  vec: W is a multiple of 4 and the three byte maps are 4-byte aligned; a thread
// then moves 4 pixels of a row per 32-bit access.  A thread computes 4 neighbouring pixels of a row either way.
__global__ __launch_bounds__(256) void k_cheb_cols(const unsigned char* __restrict__ code, const unsigned char* __restrict__ hin,
                                                  unsigned char* __restrict__ depth, int H, int W, int TX, int halo, int strips,
                                                  int chunks, int border, int vec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cheb_col[];
    const int per = strips * chunks, n = blockIdx.x / per, rem = blockIdx.x - n * per;
    const int y0 = (rem / strips) * CHEB_COL_TH, x0 = (rem % strips) * TX;
    const int SR = CHEB_COL_TH + 2 * halo, yb = y0 - halo, TXW = TX >> 2;
    const int ys = max(0, yb), ye = min(H, y0 + CHEB_COL_TH + halo);
    unsigned char* sc = cheb_col;
    unsigned char* sh = cheb_col + SR * TX;
    const size_t img = (size_t)n * H * W;
    if (vec) {
#pragma unroll 4
        for (int i = threadIdx.x; i < (ye - ys) * TXW; i += 256) {
            const int ry = i / TXW, wx = i - ry * TXW, x = x0 + 4 * wx, j = (ys - yb + ry) * TX + 4 * wx;
            const size_t g = img + (size_t)(ys + ry) * W + x;
            const bool in = x < W;                         // W % 4 == 0: the four pixels are inside together
            *reinterpret_cast<unsigned*>(sc + j) = in ? *reinterpret_cast<const unsigned*>(code + g) : 0xFFFFFFFFu;
            *reinterpret_cast<unsigned*>(sh + j) = in ? *reinterpret_cast<const unsigned*>(hin + g) : 0u;
        }
    } else {
        for (int i = threadIdx.x; i < (ye - ys) * TX; i += 256) {
            const int ry = i / TX, cx = i - ry * TX, x = x0 + cx, j = (ys - yb + ry) * TX + cx;
            const size_t g = img + (size_t)(ys + ry) * W + x;
            sc[j] = x < W ? code[g] : BF_VOID;
            sh[j] = x < W ? hin[g] : (unsigned char)0;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CHEB_COL_TH * TXW; i += 256) {
        const int ty = i / TXW, wx = i - ty * TXW, y = y0 + ty, xa = x0 + 4 * wx;
        if (y >= H || xa >= W) continue;
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = xa + k, j = (y - yb) * TX + 4 * wx + k;
            int out = 0;
            if (x < W && sc[j] < BF_MAX_K) {
                out = cheb_col_depth(sc, sh, j, y, H, TX);
                if (border) out = min(out, cheb_border_term(x, y, H, W));
            }
            if (vec) word |= (unsigned)out << (8 * k);
            else if (x < W) depth[img + (size_t)y * W + x] = (unsigned char)out;
        }
        if (vec) *reinterpret_cast<unsigned*>(depth + img + (size_t)y * W + xa) = word;
    }
}

// A thread's counts, kept in registers while the pair (label code, prediction code) stays what it is and added to the LDS counters when
// it changes: neighbouring pixels mostly share their classes, so most pixels cost no atomic.
struct BiouRun {
    int cl, cp;
    unsigned n, g, p, i;                                   // pixels of the run; of them in the label's band, the prediction's, both
    int tkey;                                              // trimap bin of the current run of one (width, label, prediction), -1: none
    unsigned tn;
};

__device__ __forceinline__ void biou_flush(unsigned* s_cnt, const BiouRun& r, int K) {
    if (r.n == 0) return;
    const bool gC = r.cl < K, pC = r.cp < K;
    if (gC) atomicAdd(&s_cnt[3 * K + r.cl], r.n);
    if (gC && r.g) atomicAdd(&s_cnt[r.cl], r.g);
    if (pC) atomicAdd(&s_cnt[4 * K + r.cp], r.n);
    if (pC && r.p) atomicAdd(&s_cnt[K + r.cp], r.p);
    if (gC && r.cl == r.cp) {
        atomicAdd(&s_cnt[5 * K + r.cl], r.n);
        if (r.i) atomicAdd(&s_cnt[2 * K + r.cl], r.i);
    }
}

__device__ __forceinline__ void biou_pixel(unsigned* s_cnt, unsigned* s_tri, BiouRun& r, int cp, int dp, int cl, int dl, int bt, int K,
                                           int dil, int nw, const ChebWidths& widths) {
    if (cl != r.cl || cp != r.cp) {
        biou_flush(s_cnt, r, K);
        r.cl = cl;
        r.cp = cp;
        r.n = r.g = r.p = r.i = 0u;
    }
    const bool gB = cl < K && min(dl, bt) <= dil, pB = cp < K && min(dp, bt) <= dil;
    r.n += 1u;
    r.g += gB;
    r.p += pB;
    r.i += gB && pB;
    if (nw > 0 && cl < K && cp < K) {
        int bin = nw;
        for (int i = nw - 1; i >= 0; --i)
            if (dl <= widths.w[i]) bin = i;
        if (bin < nw) {
            const int key = (bin * K + cl) * K + cp;
            if (key != r.tkey) {
                if (r.tn) atomicAdd(&s_tri[r.tkey], r.tn);
                r.tkey = key;
                r.tn = 0u;
            }
            r.tn += 1u;
        }
    }
}

// grid N * blocks_per_image.  VEC: H W is a multiple of 16 and the four maps are 16-byte aligned: a thread takes 16 neighbouring pixels,
// one 16-byte load per map; otherwise a thread takes every 256th pixel of the block's, byte by byte.
template <bool VEC>
__global__ __launch_bounds__(256) void k_biou_counts(const unsigned char* __restrict__ code_p, const unsigned char* __restrict__ depth_p,
                                                    const unsigned char* __restrict__ code_l, const unsigned char* __restrict__ depth_l,
                                                    unsigned long long* __restrict__ counts, unsigned long long* __restrict__ trimap,
                                                    ChebWidths widths, int nw, int H, int W, int K, int dil, int per_image) {
    extern __shared__ unsigned biou_tri[];                 // [nw][K][K]
    __shared__ unsigned s_cnt[BIOU_ROWS * BF_MAX_K];
    const int n = blockIdx.x / per_image, blk = blockIdx.x - n * per_image;
    const int HW = H * W, p0 = blk * CHEB_CNT_PIXELS;
    const size_t img = (size_t)n * HW;
    const int ntri = trimap ? nw * K * K : 0;
    if (!trimap) nw = 0;
    for (int i = threadIdx.x; i < BIOU_ROWS * K; i += 256) s_cnt[i] = 0u;
    for (int i = threadIdx.x; i < ntri; i += 256) biou_tri[i] = 0u;
    __syncthreads();
    BiouRun r = {-1, -1, 0u, 0u, 0u, 0u, -1, 0u};
    if (VEC) {
        const int p = p0 + threadIdx.x * 16;
        if (p < HW) {                                      // H W % 16 == 0: the sixteen pixels are inside together
            const uint4 vcp = *reinterpret_cast<const uint4*>(code_p + img + p), vdp = *reinterpret_cast<const uint4*>(depth_p + img + p);
            const uint4 vcl = *reinterpret_cast<const uint4*>(code_l + img + p), vdl = *reinterpret_cast<const uint4*>(depth_l + img + p);
            const unsigned wcp[4] = {vcp.x, vcp.y, vcp.z, vcp.w}, wdp[4] = {vdp.x, vdp.y, vdp.z, vdp.w};
            const unsigned wcl[4] = {vcl.x, vcl.y, vcl.z, vcl.w}, wdl[4] = {vdl.x, vdl.y, vdl.z, vdl.w};
            int y = p / W, x = p - y * W;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int s = 8 * (j & 3), q = j >> 2;
                biou_pixel(s_cnt, biou_tri, r, (wcp[q] >> s) & 255u, (wdp[q] >> s) & 255u, (wcl[q] >> s) & 255u, (wdl[q] >> s) & 255u,
                           cheb_border_term(x, y, H, W), K, dil, nw, widths);
                if (++x == W) {
                    x = 0;
                    ++y;
                }
            }
        }
    } else {
        for (int it = 0; it < CHEB_CNT_PIXELS / 256; ++it) {
            const int p = p0 + it * 256 + threadIdx.x;
            if (p >= HW) break;
            const int y = p / W, x = p - y * W;
            const size_t g = img + p;
            biou_pixel(s_cnt, biou_tri, r, code_p[g], depth_p[g], code_l[g], depth_l[g], cheb_border_term(x, y, H, W), K, dil, nw, widths);
        }
    }
    biou_flush(s_cnt, r, K);
    if (r.tn) atomicAdd(&biou_tri[r.tkey], r.tn);
    __syncthreads();
    for (int i = threadIdx.x; i < BIOU_ROWS * K; i += 256)
        if (s_cnt[i]) atomicAdd(&counts[(size_t)n * BIOU_ROWS * K + i], (unsigned long long)s_cnt[i]);
    for (int i = threadIdx.x; i < ntri; i += 256)
        if (biou_tri[i]) atomicAdd(&trimap[i], (unsigned long long)biou_tri[i]);
}

inline int cheb_check_sizes(const char* who, int N, int H, int W, int K) {
    CVK_CHECK_ARG(K >= 1 && K <= BF_MAX_K, "%s: %d classes, the kernels serve 1 to %d", who, K, BF_MAX_K);
    CVK_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: sizes must be positive, got N %d, H %d, W %d", who, N, H, W);
    CVK_CHECK_ARG((int64_t)N * H * W < 2147483648LL, "%s: 2^31 pixels or more", who);
    CVK_CHECK_ARG(W <= CHEB_MAX_W, "%s: rows of %d pixels, the row pass serves up to %d", who, W, CHEB_MAX_W);
    return CVK_OK;
}

}  // namespace

extern "C" int64_t cvk_cheb_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0 || W > CHEB_MAX_W || (int64_t)N * H * W >= 2147483648LL) return 0;
    return (((int64_t)N * H * W) + 15) & ~(int64_t)15;
}

extern "C" int cvk_cheb_depth(const int64_t* map, const int64_t* void_from, uint8_t* code_u8, uint8_t* depth_u8, void* workspace, int N,
                              int H, int W, int num_classes, int ignore_index, int max_depth, int border, void* stream) {
    CVK_CHECK_ARG(map && code_u8 && depth_u8 && workspace, "cvk_cheb_depth: null pointer");
    const int rc = cheb_check_sizes("cvk_cheb_depth", N, H, W, num_classes);
    if (rc != CVK_OK) return rc;
    CVK_CHECK_ARG(max_depth >= 1 && max_depth <= CHEB_MAX_DEPTH, "cvk_cheb_depth: max_depth %d outside 1..%d", max_depth, CHEB_MAX_DEPTH);
    CVK_CHECK_ARG(border == 0 || border == 1, "cvk_cheb_depth: border must be 0 or 1, got %d", border);
    hipStream_t s = (hipStream_t)stream;
    unsigned char* h = static_cast<unsigned char*>(workspace);
    const size_t rows = (size_t)N * H;
    const int R = W >= CHEB_ROW_PIXELS ? 1 : CHEB_ROW_PIXELS / W, lim = max_depth + 1;
    const int64_t* vf = void_from ? void_from : map;
    const bool vec4 = (W & 3) == 0 && (((uintptr_t)code_u8 | (uintptr_t)depth_u8 | (uintptr_t)h) & 3u) == 0;
    const dim3 grows((unsigned)((rows + R - 1) / R));
    if (vec4 && (((uintptr_t)map | (uintptr_t)vf) & 15u) == 0)
        hipLaunchKernelGGL(k_cheb_rows<true>, grows, dim3(256), (size_t)R * W, s, map, vf, code_u8, h, rows, W, R, num_classes, ignore_index,
                           lim);
    else
        hipLaunchKernelGGL(k_cheb_rows<false>, grows, dim3(256), (size_t)R * W, s, map, vf, code_u8, h, rows, W, R, num_classes, ignore_index,
                           lim);
    const int halo = min(max_depth, H - 1), TX = halo <= 64 ? 64 : 32;
    const int strips = cvk_cdiv(W, TX), chunks = cvk_cdiv(H, CHEB_COL_TH);
    CVK_CHECK_ARG((int64_t)N * strips * chunks < 2147483648LL, "cvk_cheb_depth: too many tiles");
    hipLaunchKernelGGL(k_cheb_cols, dim3((unsigned)N * strips * chunks), dim3(256), (size_t)2 * TX * (CHEB_COL_TH + 2 * halo), s, code_u8, h,
                       depth_u8, H, W, TX, halo, strips, chunks, border, vec4 ? 1 : 0);
    CVK_LAUNCH_RETURN("cvk_cheb_depth");
}

extern "C" int cvk_boundary_iou_counts(const uint8_t* code_p, const uint8_t* depth_p, const uint8_t* code_l, const uint8_t* depth_l,
                                       int64_t* counts, int64_t* trimap, const int* widths, int nw, int N, int H, int W, int num_classes,
                                       int dilation, void* stream) {
    CVK_CHECK_ARG(code_p && depth_p && code_l && depth_l && counts, "cvk_boundary_iou_counts: null pointer");
    const int rc = cheb_check_sizes("cvk_boundary_iou_counts", N, H, W, num_classes);
    if (rc != CVK_OK) return rc;
    CVK_CHECK_ARG(dilation >= 1 && dilation <= CHEB_MAX_DEPTH, "cvk_boundary_iou_counts: dilation %d outside 1..%d", dilation,
                  CHEB_MAX_DEPTH);
    CVK_CHECK_ARG(nw >= 0 && nw <= CHEB_MAX_WIDTHS, "cvk_boundary_iou_counts: %d trimap widths, the kernel serves up to %d", nw,
                  CHEB_MAX_WIDTHS);
    CVK_CHECK_ARG(!trimap || (widths && nw >= 1), "cvk_boundary_iou_counts: trimap bins without widths");
    ChebWidths wd = {};
    if (trimap)
        for (int i = 0; i < nw; ++i) {
            CVK_CHECK_ARG(widths[i] >= 1 && widths[i] <= CHEB_MAX_DEPTH, "cvk_boundary_iou_counts: width %d outside 1..%d", widths[i],
                          CHEB_MAX_DEPTH);
            CVK_CHECK_ARG(i == 0 || widths[i] > widths[i - 1], "cvk_boundary_iou_counts: the widths must be strictly increasing");
            wd.w[i] = widths[i];
        }
    const int per_image = cvk_cdiv((long)H * W, CHEB_CNT_PIXELS), K = num_classes;
    CVK_CHECK_ARG((int64_t)N * per_image < 2147483648LL, "cvk_boundary_iou_counts: too many tiles");
    const size_t lds = trimap ? sizeof(unsigned) * nw * K * K : 0;
    const bool vec = ((H * W) & 15) == 0 && (((uintptr_t)code_p | (uintptr_t)depth_p | (uintptr_t)code_l | (uintptr_t)depth_l) & 15u) == 0;
    unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
    unsigned long long* t = reinterpret_cast<unsigned long long*>(trimap);
    if (vec)
        hipLaunchKernelGGL(k_biou_counts<true>, dim3((unsigned)N * per_image), dim3(256), lds, (hipStream_t)stream, code_p, depth_p, code_l,
                           depth_l, c, t, wd, nw, H, W, K, dilation, per_image);
    else
        hipLaunchKernelGGL(k_biou_counts<false>, dim3((unsigned)N * per_image), dim3(256), lds, (hipStream_t)stream, code_p, depth_p, code_l,
                           depth_l, c, t, wd, nw, H, W, K, dilation, per_image);
    CVK_LAUNCH_RETURN("cvk_boundary_iou_counts");
}
