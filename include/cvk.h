/*
 * cvk.h — C ABI of libcvk.so: the MI355X (gfx950) kernels behind the CamVid UNet/SegNet training hot path.
 *
 * The upstream reference (weiaicunzai/pytorch-camvid) has NO native code and NO FFI on this path: its hot path
 * is torch.nn modules calling ATen.  The boundary a maintainer binds is therefore the set of torch operators the
 * reference invokes; each entry point below names the reference call site (file:line under the reference root)
 * whose ATen operator it replaces.  INTEGRATION.md shows the ctypes stub and the nn.Module that sits on top.
 *
 * Conventions
 *   - All pointers are DEVICE pointers owned by the caller (torch tensors); the library allocates nothing
 *     persistent and keeps no pointer past return.  Workspaces are caller-provided.
 *   - Every call only enqueues work on `stream` (a hipStream_t passed as void*) and never synchronises.
 *   - Re-entrant, no mutable globals except a thread-local last-error string.
 *   - Return value: 0 on success, CVK_E* (<0) on argument errors, or a positive hipError_t from the launch.
 *   - Activations are fp32 NHWC ("channels_last"): element (n,y,x,c) of a dense tensor lives at
 *     ((n*H + y)*W + x)*ld + c with pixel stride ld >= C.  A *view* (cvk_view) addresses a channel slice and/or a
 *     spatial window of a larger NHWC buffer: element (n,y,x,c) at  ptr + n*sN + y*sY + x*sX + c.
 *   - Conv weights are [Cout][3][3][Cin] (= torch OIHW with channels_last strides, i.e. KRSC).
 *   - Vectorised paths need 16-byte aligned base pointers and ld % 4 == 0; the conv kernels REQUIRE it
 *     (the host pads channel counts to a multiple of 4 with zero channels).
 */
#ifndef CVK_H
#define CVK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVK_VERSION 100          /* 0.1.0 */
#define CVK_OK 0
#define CVK_EINVAL (-1)          /* bad argument (shape, alignment, null pointer) */
#define CVK_EWORKSPACE (-2)      /* workspace too small */
#define CVK_STAT_ROWS 64         /* rows (pixels) summarised by one BN-statistics partial of the conv epilogue */

typedef struct cvk_view {        /* strided NHWC view, strides in floats */
    float*  ptr;                 /* address of element (0,0,0,0) of the view */
    int64_t sN, sY, sX;          /* image, row, pixel strides */
} cvk_view;

typedef struct cvk_viewh {       /* strided NHWC view of a bf16 (or, where stated, fp32) tensor; strides in ELEMENTS */
    void*   ptr;
    int64_t sN, sY, sX;
} cvk_viewh;

int         cvk_version(void);
/* first 64 bits of the SHA-256 of THIS header as the library was compiled against it (csrc/Makefile passes it as
 * -DCVK_ABI_HASH).  A host binding hashes the header it was written against and refuses a library built from another
 * one: entry points keep their names when argument lists change, and ctypes / cgo / JNI stubs do not check arity. */
uint64_t    cvk_abi_hash(void);
const char* cvk_last_error_string(void);

/* ---- layout at the module boundary: logical NCHW tensors of any strides <-> dense NHWC (ld >= C) --------------
 * replaces nothing in the reference (torch tensors are layout-polymorphic); it is the import/export step of
 * models/unet.py:94 `forward(x)` input and :156 return value. Pad channels [C,ld) of dst are written as 0. */
int cvk_import_nchw(const float* src, int64_t sN, int64_t sC, int64_t sH, int64_t sW,
                    float* dst, int ld, int N, int C, int H, int W, void* stream);
int cvk_export_nchw(const float* src, int ld, float* dst, int64_t dN, int64_t dC, int64_t dH, int64_t dW,
                    int N, int C, int H, int W, void* stream);
/* zero channels [0,C) of every pixel of an NHWC frame [N,H,W] that lies OUTSIDE the window
 * [y0,y0+h) x [x0,x0+w): the F.pad of models/unet.py:120-123 written in place into the concat buffer. */
int cvk_zero_frame(cvk_view buf, int N, int H, int W, int C, int y0, int x0, int h, int w, void* stream);

/* ---- conv 3x3, stride 1, zero pad 1 (nn.Conv2d(cin,cout,3,padding=1): models/unet.py:11, models/segnet.py:8) --
 * forward: y[m][co] = bias[co] + sum_{tap,ci} x[m+tap][ci] * w[co][tap][ci]      (implicit GEMM on fp32 MFMA)
 *   x: dense NHWC, ld = Cin (Cin % 4 == 0).  w: [Cout][9][Cin].  y: dense, pixel stride ldy >= Cout, columns
 *   [Cout,ldy) are written as 0.  bias may be NULL.
 *   stats (nullable): fused BatchNorm statistics partials, float[2][P][Cout], P = ceil(N*H*W / CVK_STAT_ROWS):
 *   stats[0][p][c] = sum of y over rows [64p,64p+64) ; stats[1][p][c] = sum of (y - partial mean)^2.
 * data-grad = the same kernel on dy with the packed weights of cvk_pack_weight_dgrad. */
int cvk_conv3x3_fwd(const float* x, const float* w, const float* bias, float* y, float* stats,
                    int N, int H, int W, int Cin, int Cout, int ldy, void* stream);
/* w_src: [Cout][9][Cin] -> dst [Cout][9][Cin_pad] (zero padded). */
int cvk_pack_weight_fwd(const float* w_src, float* dst, int Cout, int Cin, int Cin_pad, void* stream);
/* w_src: [Cout][9][Cin] -> dst [Cin_pad][9][Cout_pad], dst[ci][t][co] = w_src[co][8-t][ci] (flipped taps). */
int cvk_pack_weight_dgrad(const float* w_src, float* dst, int Cout, int Cin, int Cin_pad, int Cout_pad, void* stream);
/* weight-grad (ConvolutionBackward of train.py:131): dw[co][tap][ci] = sum_m dy[m][co] * x[m+tap][ci].
 *   x: dense, ld = Cin_pad; dy: dense, ld = ld_dy; dw: [Cout][9][Cin] (Cin <= Cin_pad real channels).
 *   Split over pixels into fp32 slabs in `workspace`, then a deterministic slab reduction. */
size_t cvk_conv3x3_wgrad_workspace_bytes(int N, int H, int W, int Cin_pad, int Cout);
int cvk_conv3x3_wgrad(const float* x, const float* dy, float* dw, int N, int H, int W, int Cin, int Cin_pad,
                      int Cout, int ld_dy, void* workspace, size_t workspace_bytes, void* stream);

/* Same operator through 1-D Winograd F(2,3) along the width (1.5x fewer MFMA FLOPs; csrc/wino.hip), for Cin % 64 == 0:
 *   U  = cvk_wino_weight_transform(w)                      [4][Cout][3][Cin] from w [Cout][3][3][Cin]
 *   Mo = cvk_conv3x3_wino_gemm(x, U)                       four transformed products, float[4][N*H*ceil(W/2)][ldm]
 *                                                          (cvk_conv3x3_wino_workspace_bytes(N,H,W,ldm) bytes)
 *   y, stats = cvk_wino_output(Mo, bias)                   output transform + bias + fused BN statistics partials;
 *                                                          y / stats / bias / ldy exactly as in cvk_conv3x3_fwd (ldy == ldm)
 * Data-grad: the same three calls on dy with the cvk_pack_weight_dgrad weights, bias = stats = NULL. */
int cvk_wino_weight_transform(const float* w, float* U, int Cout, int Cin, void* stream);
size_t cvk_conv3x3_wino_workspace_bytes(int N, int H, int W, int Cout_ld);
int cvk_conv3x3_wino_gemm(const float* x, const float* U, float* Mo, int N, int H, int W, int Cin, int Cout, int ldm,
                          void* stream);
int cvk_wino_output(const float* Mo, const float* bias, float* y, float* stats, int N, int H, int W, int Cout, int ldy,
                    void* stream);

/* The same three steps through 1-D Winograd F(4,3) (2x fewer MFMA FLOPs than the direct form; csrc/wino4.hip):
 *   U [6][Cout][3][Cin],  Mo float[ksplit][6][N*H*ceil(W/4)][ldm],  otherwise the contract of the F(2,3) calls above.
 * Layers with few tiles split the K = 3*Cin reduction over ksplit = cvk_conv3x3_wino4_ksplit(...) in {1,2,3} workgroups per
 * transform index (a fixed function of the shape); the partial planes are summed by cvk_wino4_output, which takes that
 * ksplit, and the workspace size query accounts for them. */
int cvk_wino4_weight_transform(const float* w, float* U, int Cout, int Cin, void* stream);
/* data-grad weights in one step: U[6][Cin][3][Cout] of the rotated, channel-transposed filter, straight from
 * w [Cout][3][3][Cin] (== cvk_pack_weight_dgrad without padding followed by cvk_wino4_weight_transform) */
int cvk_wino4_weight_transform_dgrad(const float* w, float* U, int Cout, int Cin, void* stream);
int cvk_conv3x3_wino4_ksplit(int N, int H, int W, int Cin, int Cout_ld);
size_t cvk_conv3x3_wino4_workspace_bytes(int N, int H, int W, int Cin, int Cout_ld);
int cvk_conv3x3_wino4_gemm(const float* x, const float* U, float* Mo, int N, int H, int W, int Cin, int Cout, int ldm,
                           void* stream);
int cvk_wino4_output(const float* Mo, const float* bias, float* y, float* stats, int N, int H, int W, int Cout, int ldy,
                     int ksplit, void* stream);

/* 2-D Winograd F(4x4,3x3) for channel-heavy layers (csrc/wino2d.hip): forward / data-grad of nn.Conv2d(k=3,pad=1)
 * (reference models/unet.py:11, bwd of train.py:131) as 36 batched GEMMs over T = cvk_w2d_tiles(N,H,W) 4x4 output tiles.
 *   U = cvk_w2d_weight_transform(w)        float[36][Cout][Cin] from w [Cout][3][3][Cin] (data-grad: from the
 *                                          cvk_pack_weight_dgrad pack, roles of Cin / Cout exchanged)
 *   cvk_conv3x3_w2d(x, U, ...)             input transform -> GEMMs -> output transform + bias; x dense [N,H,W,Cin],
 *                                          Cin % 32 == 0, Cout % 4 == 0, Cout >= 64; workspace of
 *                                          cvk_conv3x3_w2d_workspace_bytes(N,H,W,Cin,Cout) bytes.
 *   stats/counts (both or neither): BatchNorm statistics partials float[2][P][Cout] (sum, M2 about the partial mean) and
 *   float[P] pixel counts, P = cvk_w2d_stat_partials(N,H,W) -> cvk_bn_finalize_counts. */
int cvk_w2d_tiles(int N, int H, int W);
int cvk_w2d_tpad(int T);                      /* rows per transform plane: T rounded up to a multiple of 32 (zero rows) */
int cvk_w2d_stat_partials(int N, int H, int W);
size_t cvk_conv3x3_w2d_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int cvk_w2d_weight_transform(const float* w, float* U, int Cout, int Cin, void* stream);
/* the data-grad filter float[36][Cin][Cout] straight from the FORWARD weights w [Cout][3][3][Cin] (rotation by 180 degrees and
 * the channel exchange happen inside; equals cvk_w2d_weight_transform(cvk_pack_weight_dgrad(w)) bit for bit) */
int cvk_w2d_weight_transform_dgrad(const float* w, float* U, int Cout, int Cin, void* stream);
int cvk_conv3x3_w2d(const float* x, const float* U, const float* bias, float* y, float* stats, float* counts, int N, int H,
                    int W, int Cin, int Cout, int ldy, void* workspace, size_t workspace_bytes, void* stream);
/* the three passes of cvk_conv3x3_w2d, callable (and timed) one by one.  V float[36][Tpad][Cin] + 512 bytes of slack,
 * Tpad = cvk_w2d_tpad(T), rows beyond T zero; Mo float[f][36][T][Cout] with f = cvk_w2d_ksplit(T, Cin, Cout) K-range planes
 * (the tiles of the last partial round of workgroups are split in K; the output pass adds the planes in a fixed order and
 * therefore takes Cin as well).  cvk_w2d_output writes the columns [0, Cout) of every pixel of y and leaves the pad columns
 * [Cout, ldy) as they were. */
int cvk_w2d_ksplit(int T, int Cin, int Cout);
int cvk_w2d_input_transform(const float* x, float* V, int N, int H, int W, int Cin, void* stream);
int cvk_w2d_gemm(const float* V, const float* U, float* Mo, int T, int Cin, int Cout, void* stream);
int cvk_w2d_output(const float* Mo, const float* bias, float* y, float* stats, float* counts, int N, int H, int W, int Cin,
                   int Cout, int ldy, void* stream);
/* weight-grad through the transposed 2-D F(4x4,3x3) (contract of cvk_conv3x3_wgrad; channel counts multiples of 4):
 * dW = G^T [ sum_tiles (A dy A^T) (.) (B^T x B) ] G, 36 GEMMs whose depth is the tile index.  x == NULL: the first
 * 36*Tpad*Cin_pad floats of the workspace already hold V = cvk_w2d_input_transform(x) (kept from the forward pass).
 * Passes: E float[36][Tpad][Cout] (+ slack) = cvk_w2d_dy_transform(dy); P float[f][36][Cout][Cin_pad] = cvk_w2d_gemm_tn(E, V),
 * f = cvk_w2d_wgrad_ksplit(T, Cin_pad, Cout) depth ranges; dw = cvk_w2d_wgrad_output(P) adds them in a fixed order. */
size_t cvk_conv3x3_wgrad_w2d_workspace_bytes(int N, int H, int W, int Cin_pad, int Cout);
int cvk_conv3x3_wgrad_w2d(const float* x, const float* dy, float* dw, int N, int H, int W, int Cin, int Cin_pad, int Cout,
                          int ld_dy, void* workspace, size_t workspace_bytes, void* stream);
int cvk_w2d_wgrad_ksplit(int T, int Cin_pad, int Cout);
int cvk_w2d_dy_transform(const float* dy, int ld_dy, float* E, int N, int H, int W, int Cout, void* stream);
/* both transforms of dy in one launch: Vp = cvk_w2d_input_transform(dy) (the data-grad's operand, dy dense with row stride ld_dy =
 * Cout required by that GEMM) and E = cvk_w2d_dy_transform(dy) (the weight-grad's), bit for bit; dy crosses the fabric once */
int cvk_w2d_dy_transform_both(const float* dy, int ld_dy, float* Vp, float* E, int N, int H, int W, int Cout, void* stream);
int cvk_w2d_gemm_tn(const float* E, const float* V, float* P, int T, int Cin_pad, int Cout, void* stream);
int cvk_w2d_wgrad_output(const float* P, float* dw, int T, int Cin, int Cin_pad, int Cout, void* stream);

/* 2-D Winograd F(6x6,3x3) (csrc/wino2d.hip, the same kernels instantiated for 8x8 input tiles; points 0, +-1, +-2, +-1/2, inf):
 * 64 batched GEMMs over T = cvk_w6_tiles(N,H,W) 6x6 output tiles — 1.78 multiplies per output and input channel instead of
 * 2.25, and 1.78x instead of 2.25x the activation in transform-domain planes.  fp32 rounding about twice that of F(4x4,3x3)
 * (5e-6 relative L2 at 256 input channels).  Every cvk_w6_* entry point has the contract of its cvk_w2d_* namesake with 36 -> 64
 * planes: U float[64][Cout][Cin], V float[64][Tpad][Cin] (+ 512 bytes), Mo float[f][64][T][Cout], E float[64][Tpad][Cout],
 * P float[f][64][Cout][Cin_pad]; Tpad = cvk_w2d_tpad(T). */
int cvk_w6_tiles(int N, int H, int W);
int cvk_w6_stat_partials(int N, int H, int W);
size_t cvk_conv3x3_w6_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int cvk_w6_weight_transform(const float* w, float* U, int Cout, int Cin, void* stream);
int cvk_w6_weight_transform_dgrad(const float* w, float* U, int Cout, int Cin, void* stream);
int cvk_w6_ksplit(int T, int Cin, int Cout);
int cvk_w6_input_transform(const float* x, float* V, int N, int H, int W, int Cin, void* stream);
int cvk_w6_gemm(const float* V, const float* U, float* Mo, int T, int Cin, int Cout, void* stream);
int cvk_w6_output(const float* Mo, const float* bias, float* y, float* stats, float* counts, int N, int H, int W, int Cin,
                  int Cout, int ldy, void* stream);
int cvk_w6_wgrad_ksplit(int T, int Cin_pad, int Cout);
int cvk_w6_dy_transform(const float* dy, int ld_dy, float* E, int N, int H, int W, int Cout, void* stream);
int cvk_w6_dy_transform_both(const float* dy, int ld_dy, float* Vp, float* E, int N, int H, int W, int Cout, void* stream);
int cvk_w6_gemm_tn(const float* E, const float* V, float* P, int T, int Cin_pad, int Cout, void* stream);
/* cvk_w2d_gemm_tn / cvk_w6_gemm_tn on at most max_workgroups workgroups (rounded down to a multiple of 8; 0 = one per (tile, depth range) job): a
 * capped grid walks the jobs in a loop; a job owns its depth range and its plane of P, so P is bitwise independent of the cap */
int cvk_w2d_gemm_tn_wg(const float* E, const float* V, float* P, int T, int Cin_pad, int Cout, int max_workgroups, void* stream);
int cvk_w6_gemm_tn_wg(const float* E, const float* V, float* P, int T, int Cin_pad, int Cout, int max_workgroups, void* stream);
/* OPT-IN SPLIT-OPERAND PATH (round 5; the executor's default fp32 path is exact-fp32 MFMA — this one runs only under runner.w2d_split): the
 * GEMM stage above on the 16-bit matrix pipe with split fp32 operands, accumulated in fp32 (csrc/split3.hip, csrc/split_fmt.h, tools/study/).
 *   fmt 3: x = x1 + x2 + x3 in bf16, the six largest cross-products (v_mfma_f32_16x16x32_bf16): fp32-MFMA accuracy at 0.375 of its matrix time;
 *   fmt 2: 2^e * x = h1 + h2 in fp16, three cross-products (v_mfma_f32_16x16x32_f16): 0.19 of the matrix time.  The power-of-two scale per
 *          transform index comes from the EXACT largest magnitude of the tensor a transform reads and the absolute row sums of the transform
 *          matrix, so no element can leave fp16's range whatever the data; the GEMMs undo the scale exactly.  The magnitude lives in an "amax
 *          block" of device memory: cvk_amax_block_words() 32-bit words (8 slots one cache line apart, each an atomicMax of fp32 bit patterns —
 *          one hot word would serialise tens of thousands of waves in the L2; the value is the maximum over the slots, cvk_amax_block_value on a
 *          host copy).  Zero the block, then cvk_absmax_f32 (a pass over the tensor) or the *_amax variants of the passes that WRITE the tensor
 *          (below) fill it; every `amax*` argument of this section is such a block.  cvk_split_scale_exponent (host) returns e for (tile, kind, xi, word):
 *          kind 0 = B (input transforms V, V'), 1 = G (filters U), 2 = A (dy -> E).
 * Split planes: 16-bit [NX][C/32][fmt][Rpad][32] (Rpad = cvk_split3_rows_pad(R, 256) for V / V' / E, (R, 128) for U; C % 32 == 0).
 * cvk_split_planes / cvk_split3_planes: fp32 planes P[NX][R][C] -> split planes (a stand-alone pass: tests and studies).
 * cvk_w2d_gemm_split / _split3: Mo fp32 [NX][T][Cout] = V * U^T per transform index, both operands as split planes.  The *_split3 names are
 * the fmt-3 forms of the generic entry points (no amax words). */
int cvk_split3_rows_pad(int R, int mult);
int cvk_split3_planes(const float* P, void* S, int NX, int R, int Rpad, int C, void* stream);
int cvk_w2d_gemm_split3(const void* V3, const void* U3, float* Mo, int NX, int T, int Tpad, int Cin, int Cout, int Cpad, void* stream);
int cvk_amax_block_words(void);
unsigned cvk_amax_block_value(const unsigned* host_words, int n);
int cvk_absmax_f32(const float* x, long rows, int C, int ld, void* amax_block, void* stream);
int cvk_split_scale_exponent(int tile, int kind, int xi, unsigned amax_block);
int cvk_split_planes(int fmt, int tile, int kind, const float* P, void* S, const void* amax, int NX, int R, int Rpad, int C, void* stream);
int cvk_w2d_gemm_split(int fmt, int tile, const void* V, const void* U, float* Mo, const void* amax_v, const void* amax_u, int NX, int T, int Tpad,
                       int Cin, int Cout, int Cpad, void* stream);
/* ... the rest of the split-operand path (tile = 4 or 6 selects F(4x4,3x3) / F(6x6,3x3)): transforms that write split planes from their store loops
 * (V3 / Vp3 / E3 rows padded to cvk_split3_rows_pad(T, 256); E stays fp32 [NX][cvk_w2d_tpad(T)][C] with e_split = 0), the filter as split
 * planes (tmp: NX * Cout * Cin floats), the output pass for product planes without K-range partials, and the weight-grad GEMM
 * P[f][NX][Cout][Cin] = E^T V on split planes (f = cvk_w2d_gemm_tn_split3_ksplit; Cout % 256 == 0 && Cin % 128 == 0 or the reverse) with
 * its final pass for an explicit f. */
int cvk_w2d_input_transform_split3(int tile, const float* x, void* V3, int N, int H, int W, int Cin, void* stream);
int cvk_w2d_dy_transform_both_split3(int tile, const float* dy, int ld_dy, void* Vp3, void* E, int e_split, int N, int H, int W, int C,
                                     void* stream);
int cvk_w2d_weight_transform_split3(int tile, const float* w, void* U3, float* tmp, int Cout, int Cin, int dgrad, void* stream);
int cvk_w2d_input_transform_split(int fmt, int tile, const float* x, void* V, const void* amax_x, int N, int H, int W, int Cin, void* stream);
int cvk_w2d_dy_transform_both_split(int fmt, int tile, const float* dy, int ld_dy, void* Vp, void* E, int e_split, const void* amax_dy, int N, int H,
                                    int W, int C, void* stream);
int cvk_w2d_weight_transform_split(int fmt, int tile, const float* w, void* U, const void* amax_w, int Cout, int Cin, int dgrad, void* stream);
int cvk_w2d_output_plain(int tile, const float* Mo, const float* bias, float* y, float* stats, float* counts, int N, int H, int W,
                         int Cout, int ldy, void* stream);
int cvk_w2d_gemm_tn_split3_ksplit(int NX, int Tpad, int Cin, int Cout);
int cvk_w2d_gemm_tn_split3(const void* E3, const void* V3, float* P, int NX, int Tpad, int Cin, int Cout, void* stream);
int cvk_w2d_gemm_tn_split(int fmt, int tile, const void* E, const void* V, float* P, const void* amax_e, const void* amax_v, int NX, int Tpad, int Cin,
                          int Cout, void* stream);
int cvk_w2d_wgrad_output_f(int tile, const float* P, float* dw, int Cin, int Cin_pad, int Cout, int f, void* stream);
int cvk_w6_wgrad_output(const float* P, float* dw, int T, int Cin, int Cin_pad, int Cout, void* stream);
/* The fused F(4,3) convolution below in the opt-in fp16 split-operand form (csrc/split_fmt.h; runner.w2d_split = 2, never the default): same
 * contracts as cvk_wino4f_weight_transform / cvk_conv3x3_wino4f / cvk_conv3x3_wino4f_bnred plus the amax blocks of x and of the filter w; Uh has the
 * size of Uf (cvk_wino4f_weight_floats(Cn, Ck) * 4 bytes).  V = B^T d is split into two fp16 terms inside the staging pass, a K step is 18
 * v_mfma_f32_32x32x16_f16 instead of 48 v_mfma_f32_32x32x2f32. */
int cvk_wino4h_weight_transform(const float* w, void* Uh, const void* amax_w, int Cn, int Ck, int dgrad, void* stream);
int cvk_conv3x3_wino4h(const float* x, const void* Uh, const float* bias, float* y, float* stats, float* counts, const void* amax_x,
                       const void* amax_w, int N, int H, int W, int Cin, int Cout, int ldy, int max_workgroups, void* stream);
int cvk_conv3x3_wino4h_bnred(const float* x, const void* Uh, float* y, const void* amax_x, const void* amax_w, int N, int H, int W, int Cin,
                             int Cout, int ldy, const float* yP, const float* scale, const float* shift, const float* mean,
                             const float* rstd, float* part, int max_workgroups, void* stream);
/* FUSED 1-D Winograd F(4,3) (csrc/wino4f.hip; replaces nn.Conv2d(cin,cout,3,padding=1) fwd and its data-grad,
 * /root/reference/models/unet.py:11, models/segnet.py:8, for the 64/128-channel levels): one workgroup computes all six
 * transform indices of a 128 x 64 tile, the output transform, bias and BatchNorm statistics happen in registers — no
 * product planes, no output pass.  Uf = cvk_wino4f_weight_transform(w): cvk_wino4f_weight_floats(Cn, Ck) floats, the
 * K-sliced LDS image of (G g); dgrad != 0 builds the data-grad filter (180-degree rotation, channels exchanged) straight
 * from the forward weights w [Ck][3][3][Cn].  Cin % 32 == 0.  stats/counts (both or neither): P =
 * cvk_wino4f_stat_partials(N,H,W) partials [sum | M2 about the partial mean] [2][P][Cout] + the P pixel counts, to be
 * reduced by cvk_bn_finalize_counts.  The kernel is persistent (one workgroup per CU walks a list of tiles);
 * max_workgroups > 0 caps its grid (data-parallel runs leave CUs to RCCL's kernels), 0 = one per CU. */
size_t cvk_wino4f_weight_floats(int Cn, int Ck);
int cvk_wino4f_weight_transform(const float* w, float* Uf, int Cn, int Ck, int dgrad, void* stream);
/* n (<= CVK_WT_BATCH_MAX) filter transforms in ONE launch; `jobs` is a HOST array (copied into the kernel arguments).  A training step
 * rebuilds every Winograd-domain filter (the weights changed in optimizer.step(), train.py:134): 16 + 26 launches of 5-15 us each.
 *   cvk_wino4f_weight_transform_batch: job = cvk_wino4f_weight_transform(w, out, rows = Cn, cols = Ck, dgrad)      (tile ignored)
 *   cvk_w2d_weight_transform_batch:    job = cvk_w2d_ / cvk_w6_weight_transform[_dgrad](w, out, rows = Cout, cols = Cin), tile = 4 | 6 */
#define CVK_WT_BATCH_MAX 48
typedef struct cvk_wt_job { const float* w; float* out; int rows, cols, tile, dgrad; } cvk_wt_job;
int cvk_wino4f_weight_transform_batch(const cvk_wt_job* jobs, int n, void* stream);
int cvk_w2d_weight_transform_batch(const cvk_wt_job* jobs, int n, void* stream);
int cvk_wino4f_stat_partials(int N, int H, int W);
/* cvk_conv3x3_wino4f (forward form) that ALSO leaves the layer's weight-grad operand behind: the kernel's staging path computes exactly the
 * rows V_xi = B^T d that the plane GEMM of the weight-grad reads (cvk_wgradp_gemm_sm), so the centre-kernel-row slices are stored as six
 * SLICE-MAJOR planes Vsm[6][Cin / 16][cvk_wgradp_plane_rows(N,H,W)][16] (element (xi, row, c) at ((xi * Cin/16 + c/16) * rows + row) * 16 + c % 16;
 * a wave's store is 1 KiB contiguous).  The pad rows must have been zeroed by cvk_wgradp_zero_pads_sm.  y / stats / counts are bitwise those of
 * cvk_conv3x3_wino4f; stats and counts may both be NULL (frozen BatchNorm).  Replaces the x -> V pass of the weight-grad of
 * nn.Conv2d(cin,cout,3,padding=1) (/root/reference/models/unet.py:11, backward of train.py:131). */
int cvk_conv3x3_wino4f_vplanes(const float* x, const float* Uf, const float* bias, float* y, float* stats, float* counts, float* Vsm,
                               int N, int H, int W, int Cin, int Cout, int ldy, int max_workgroups, void* stream);
int cvk_conv3x3_wino4f(const float* x, const float* Uf, const float* bias, float* y, float* stats, float* counts, int N, int H,
                       int W, int Cin, int Cout, int ldy, int max_workgroups, void* stream);
/* The data-grad launch whose result y is the COMPLETE dL/d(activation) of the block that produced this conv's input
 * (nn.BatchNorm2d + ReLU backward of /root/reference/models/unet.py:12-13 starts with two column sums over exactly that
 * tensor): the epilogue also leaves  sum g  and  sum g * xhat,  g = y masked by the producer's ReLU (yP*scale+shift > 0),
 * xhat = (yP - mean) * rstd,  as part = float[2][cvk_wino4f_stat_partials(N,H,W)][Cout] for
 * cvk_colsum_finalize(part, partials, Cout, dbeta, dgamma) — cvk_bn_bwd_reduce is then not launched for that block.
 * yP: the producer's conv output [N*H*W][ldy] (same row stride as y); no bias, no forward statistics. */
int cvk_conv3x3_wino4f_bnred(const float* x, const float* Uf, float* y, int N, int H, int W, int Cin, int Cout, int ldy,
                             const float* yP, const float* scale, const float* shift, const float* mean, const float* rstd,
                             float* part, int max_workgroups, void* stream);

/* THIN layers (csrc/thin.hip): the stem nn.Conv2d(3, 64, 3, padding=1) (/root/reference/models/unet.py:103,
 * models/segnet.py first block) and the classifier head nn.Conv2d(64, class_num, 3, padding=1) (models/unet.py:127), forward,
 * data-grad and weight-grad.  The thin channel dimension is one 16-row side (or the k = 4) of v_mfma_f32_16x16x4_f32; a wave
 * walks down a 16-pixel (forward) / 4-pixel (weight-grad) column with the 3x3 window's rows in registers.
 *   cvk_conv3x3_thin_fwd: y = conv3x3(x, w) + bias; w [Cout][9][Cin_ld].  stats/counts (both or neither):
 *     P = cvk_thin_stat_partials(N,H,W,Cin_ld) partials [sum | M2 about the partial mean] [2][P][Cout] + P pixel counts for
 *     cvk_bn_finalize_counts.  Supported shapes: cvk_thin_fwd_supported(Cin_ld, Cout, ldy) != 0.
 *   cvk_conv3x3_thin_wgrad: dw [Cout][9][Cin] = sum_p dy[p][co] * x[p + tap][ci]; fixed-order reduction (bitwise
 *     reproducible).  Supported shapes: cvk_thin_wgrad_supported(Cin, Cin_ld, Cout, ld_dy) != 0. */
int cvk_thin_fwd_supported(int Cin_ld, int Cout, int ldy);
int cvk_thin_stat_partials(int N, int H, int W, int Cin_ld);
int cvk_conv3x3_thin_fwd(const float* x, const float* w, const float* bias, float* y, float* stats, float* counts, int N, int H,
                         int W, int Cin_ld, int Cout, int ldy, void* stream);
int cvk_thin_wgrad_supported(int Cin, int Cin_ld, int Cout, int ld_dy);
size_t cvk_conv3x3_thin_wgrad_workspace_bytes(int N, int H, int W, int Cin_ld, int Cout);
int cvk_conv3x3_thin_wgrad(const float* x, const float* dy, float* dw, int N, int H, int W, int Cin, int Cin_ld, int Cout,
                           int ld_dy, void* workspace, size_t workspace_bytes, void* stream);

/* Transposed F(4,3) weight-grad with both transforms outside the GEMM (csrc/wgradp.hip; the weight gradient of
 * nn.Conv2d(cin,cout,3,padding=1), /root/reference/models/unet.py:11, backward of train.py:131): x and dy are written once as
 * transform-domain planes (1.5x each, zero rows at every image border), the GEMM is one wave per workgroup with no vector
 * arithmetic and no barrier.  Contract of cvk_conv3x3_wgrad; Cin_pad % 64 == 0 and Cout % 64 == 0. */
size_t cvk_conv3x3_wgradp_workspace_bytes(int N, int H, int W, int Cin_pad, int Cout);
int cvk_conv3x3_wgradp(const float* x, const float* dy, const float* E6_pre, float* dw, int N, int H, int W, int Cin, int Cin_pad,
                       int Cout, int ld_dy, void* workspace, size_t workspace_bytes, void* stream);
/* E6_pre: NULL (the E planes are built from dy inside the call) or six planes float[6][cvk_wgradp_plane_rows(N,H,W)][Cout] that
 * the BatchNorm/ReLU-backward pass wrote on its way: cvk_wgradp_zero_pads (pad rows) then cvk_bn_bwd_dx_e6 (contract of
 * cvk_bn_bwd_dx_e with six planes E0..E5 in the padded plane layout; ld_dy == C). */
long cvk_wgradp_plane_rows(int N, int H, int W);
/* the steps of cvk_conv3x3_wgradp, separately callable: planes of x (is_dy == 0) or dy (is_dy != 0), then GEMM + reduction */
int cvk_wgradp_planes(const float* t, int ld, float* planes, int N, int H, int W, int C, int is_dy, void* stream);
size_t cvk_wgradp_gemm_workspace_bytes(int N, int H, int W, int Cin_pad, int Cout);
int cvk_wgradp_gemm(const float* E6, const float* V6, float* dw, int N, int H, int W, int Cin, int Cin_pad, int Cout, void* workspace,
                    size_t workspace_bytes, void* stream);
int cvk_wgradp_zero_pads(float* planes, int N, int H, int W, int C, void* stream);
/* the same three steps for SLICE-MAJOR V planes [6][C / 16][rows][16] (C % 16 == 0) — the layout cvk_conv3x3_wino4f_vplanes writes from the forward
 * pass, so that the weight-grad needs no pass over x at all: zero the pad rows before the forward launch; cvk_wgradp_planes_sm builds the
 * same planes from x in a pass of its own (forward ran another kernel; tests); cvk_wgradp_gemm_sm = cvk_wgradp_gemm reading them (E6 stays
 * row-major [6][rows][Cout]; same workspace size). */
int cvk_wgradp_zero_pads_sm(float* planes, int N, int H, int W, int C, void* stream);
int cvk_wgradp_planes_sm(const float* x, int ld, float* planes, int N, int H, int W, int C, void* stream);
int cvk_wgradp_gemm_sm(const float* E6, const float* V6sm, float* dw, int N, int H, int W, int Cin, int Cin_pad, int Cout, void* workspace,
                       size_t workspace_bytes, void* stream);
/* ... with only FOUR E planes: E0 and E5 of E = A dy are columns 4 xt and 4 xt + 3 of dy itself, so the BatchNorm-backward pass writes E1..E4 only
 * (cvk_wgradp_zero_pads4 for the pad rows, then cvk_bn_bwd_dx_e4p: contract of cvk_bn_bwd_dx_e6 with float E4p[4][cvk_wgradp_plane_rows][C]) and the GEMM
 * reads the two identity planes from dy: dense [N*H*W][Cout] followed by cvk_wgradp_dy_slack(W) * Cout ZERO floats (pad column groups of the last row
 * read past the tensor; their V rows are zero).  W % 4 == 0 (a ragged last group's E5 is 0, not a pixel of dy).  1.0x instead of 1.5x the tensor
 * written beside dy. */
int cvk_wgradp_zero_pads4(float* planes, int N, int H, int W, int C, void* stream);
int cvk_bn_bwd_dx_e4p(cvk_view dout, const float* y, int ldy, const float* scale, const float* shift, const float* mean,
                      const float* rstd, const float* dgamma, const float* dbeta, float* dy, int ld_dy, float* E4p, float* part,
                      int N, int H, int W, int C, int use_batch_stats, void* stream);
int cvk_wgradp_dy_slack(int W);
int cvk_wgradp_gemm_sm_dy(const float* E4p, const float* dy, const float* V6sm, float* dw, int N, int H, int W, int Cin, int Cin_pad, int Cout,
                          void* workspace, size_t workspace_bytes, void* stream);
/* The three plane GEMMs on a CAPPED grid: at most max_workgroups one-wave workgroups (rounded down to a multiple of 8; 0 = one per task, the launch
 * of the entry points above), which walk the tasks in a job loop.  A task owns its run of depth steps and its slab whichever workgroup runs it, so
 * dw is bitwise independent of the cap.  For callers that run bandwidth-bound work beside the GEMM (cvk_side_begin) or leave CUs to RCCL. */
int cvk_wgradp_gemm_wg(const float* E6, const float* V6, float* dw, int N, int H, int W, int Cin, int Cin_pad, int Cout, void* workspace,
                       size_t workspace_bytes, int max_workgroups, void* stream);
int cvk_wgradp_gemm_sm_wg(const float* E6, const float* V6sm, float* dw, int N, int H, int W, int Cin, int Cin_pad, int Cout, void* workspace,
                          size_t workspace_bytes, int max_workgroups, void* stream);
int cvk_wgradp_gemm_sm_dy_wg(const float* E4p, const float* dy, const float* V6sm, float* dw, int N, int H, int W, int Cin, int Cin_pad, int Cout,
                             void* workspace, size_t workspace_bytes, int max_workgroups, void* stream);
/* Fork / join of the library's side stream (csrc/side.cpp; one per device, created on first use, non-blocking, lowest priority).
 * cvk_side_begin(main) orders everything queued on `main` so far before whatever is launched from now on on the stream it returns (NULL: error);
 * cvk_side_join(main) orders everything launched on the side stream so far before whatever is queued on `main` from now on.  The caller keeps every
 * buffer the side stream's launches touch alive until the join.  cvk_side_launches(): how often the side stream was handed out in this process
 * (every group of launches that reaches it starts with one cvk_side_begin). */
void* cvk_side_begin(void* main_stream);
int cvk_side_join(void* main_stream);
long cvk_side_launches(void);
int cvk_bn_bwd_dx_e6(cvk_view dout, const float* y, int ldy, const float* scale, const float* shift, const float* mean,
                     const float* rstd, const float* dgamma, const float* dbeta, float* dy, int ld_dy, float* E6, float* part,
                     int N, int H, int W, int C, int use_batch_stats, void* stream);

/* weight-grad through the transposed F(4,3) (contract of cvk_conv3x3_wgrad; the workspace also holds the transformed
 * output-gradient planes E1..E4, float[4][N*H*ceil(W/4)][ld_dy], hence the extra ld_dy argument of the size query) */
size_t cvk_conv3x3_wgrad_wino4_workspace_bytes(int N, int H, int W, int Cin_pad, int Cout, int ld_dy);
int cvk_conv3x3_wgrad_wino4(const float* x, const float* dy, const float* E_pre, float* dw, int N, int H, int W, int Cin,
                            int Cin_pad, int Cout, int ld_dy, void* workspace, size_t workspace_bytes, void* stream);
/* E_pre: NULL (the call transforms dy itself) or the planes written by cvk_bn_bwd_dx_e — the BN/ReLU-backward pass that
 * produces dy can emit them on the way (same contract as cvk_bn_bwd_dx plus E; 4-channel vector layout only, CVK_EINVAL
 * otherwise; `part` gets cvk_bn_bwd_e_blocks(N,H,W) partial rows of C column sums). */
int cvk_bn_bwd_e_blocks(int N, int H, int W);
int cvk_bn_bwd_dx_e(cvk_view dout, const float* y, int ldy, const float* scale, const float* shift, const float* mean,
                    const float* rstd, const float* dgamma, const float* dbeta, float* dy, int ld_dy, float* E, float* part,
                    int N, int H, int W, int C, int use_batch_stats, void* stream);

/* weight-grad through the transposed F(2,3) (same contract as cvk_conv3x3_wgrad; any Cin_pad % 4 == 0) */
size_t cvk_conv3x3_wgrad_wino_workspace_bytes(int N, int H, int W, int Cin_pad, int Cout);
int cvk_conv3x3_wgrad_wino(const float* x, const float* dy, float* dw, int N, int H, int W, int Cin, int Cin_pad,
                           int Cout, int ld_dy, void* workspace, size_t workspace_bytes, void* stream);

/* ---- BatchNorm2d (+ReLU) (models/unet.py:12-13, models/segnet.py:9-10) -------------------------------------------
 * finalize (training): combines the conv-epilogue partials (Chan's parallel variance, fp64) into per-channel
 *   mean / rstd = 1/sqrt(biased var + eps), scale = gamma*rstd, shift = beta - mean*scale, and updates
 *   running_mean/var (unbiased var, momentum) and num_batches_tracked in place when those pointers are non-NULL. */
size_t cvk_bn_finalize_workspace_bytes(int P, int C);
int cvk_bn_finalize(const float* stats, int P, int M, int C, const float* gamma, const float* beta,
                    float* mean, float* rstd, float* scale, float* shift,
                    float* running_mean, float* running_var, int64_t* num_batches_tracked,
                    float momentum, float eps, void* workspace, size_t workspace_bytes, void* stream);
/* eval mode: scale/shift from running statistics (train.py:169 net.eval()); also fills mean/rstd. */
int cvk_bn_eval_params(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                       float* mean, float* rstd, float* scale, float* shift, int C, float eps, void* stream);
/* out = max(0, y*scale + shift), y dense (ldy), out a view. */
int cvk_bn_relu_apply(const float* y, int ldy, const float* scale, const float* shift, cvk_view out,
                      int N, int H, int W, int C, void* stream);
/* the same with nn.MaxPool2d(2,2) of the result fused in (/root/reference/models/unet.py:100-109, models/segnet.py:79): pool
 * float[N][H/2][W/2][C] dense, code (optional) uint8 arg-max codes as cvk_maxpool2x2_fwd; 4-channel vector layout only */
int cvk_bn_relu_apply_pool(const float* y, int ldy, const float* scale, const float* shift, cvk_view out, float* pool,
                           unsigned char* code, int N, int H, int W, int C, void* stream);
/* backward, pass 1: g = dout * [y*scale+shift > 0]; partial sums of g and g*xhat per row block:
 *   part float[2][PB][C], PB = cvk_bn_bwd_blocks(M). */
int cvk_bn_bwd_blocks(int M);
int cvk_bn_bwd_reduce(cvk_view dout, const float* y, int ldy, const float* scale, const float* shift,
                      const float* mean, const float* rstd, float* part, int N, int H, int W, int C, void* stream);
/* sums PB partial rows in fp64: out0[c] = sum part[0][:,c], out1[c] = sum part[1][:,c] (out1/part1 nullable) */
int cvk_colsum_finalize(const float* part, int PB, int C, float* out0, float* out1, void* stream);
/* n (<= CVK_COLSUM_BATCH_MAX) such finalisations, one output each, in ONE launch; `jobs` is a HOST array (copied into the
 * kernel arguments).  The executor collects the conv-bias gradients of a backward pass and finalises them at its end
 * (or when a data-parallel gradient bucket is handed to the all-reduce). */
#define CVK_COLSUM_BATCH_MAX 64
typedef struct cvk_colsum_job { const float* part; float* out; int PB, C; } cvk_colsum_job;
int cvk_colsum_finalize_batch(const cvk_colsum_job* jobs, int n, void* stream);
/* backward, pass 2: dy = scale*(g - dbeta/M - xhat*dgamma/M) (training) or dy = scale*g (eval: use_batch_stats=0);
 *   also emits column-sum partials of dy (conv bias gradient) into dbias_part float[PB][C] when non-NULL. */
/* Variants that also leave the EXACT largest magnitude they write in a device word (atomicMax of fp32 bit patterns; the caller zeroes the word
 * first) — what cvk_absmax_f32 of the written tensor would return, without the extra pass.  The opt-in fp16 split-operand path
 * (cvk_w2d_*_split with fmt 2) scales its planes by these words.  cvk_bn_relu_apply_pool_amax: either word may be NULL. */
int cvk_bn_relu_apply_amax(const float* y, int ldy, const float* scale, const float* shift, cvk_view out, int N, int H, int W, int C,
                           void* amax_block, void* stream);
int cvk_bn_relu_apply_pool_amax(const float* y, int ldy, const float* scale, const float* shift, cvk_view out, float* pool,
                                unsigned char* code, int N, int H, int W, int C, void* amax_out, void* amax_pool, void* stream);
int cvk_bn_bwd_dx_e_amax(int six, cvk_view dout, const float* y, int ldy, const float* scale, const float* shift, const float* mean,
                         const float* rstd, const float* dgamma, const float* dbeta, float* dy, int ld_dy, float* E, float* part, int N, int H,
                         int W, int C, int use_batch_stats, void* amax_block, void* stream);   /* six: 0 = cvk_bn_bwd_dx_e, 1 = cvk_bn_bwd_dx_e6 */
int cvk_bn_bwd_dx_amax(cvk_view dout, const float* y, int ldy, const float* scale, const float* shift, const float* mean,
                       const float* rstd, const float* dgamma, const float* dbeta, float* dy, int ld_dy, float* dbias_part, int N,
                       int H, int W, int C, int use_batch_stats, void* amax_block, void* stream);
int cvk_bn_bwd_dx(cvk_view dout, const float* y, int ldy, const float* scale, const float* shift,
                  const float* mean, const float* rstd, const float* dgamma, const float* dbeta,
                  float* dy, int ld_dy, float* dbias_part, int N, int H, int W, int C, int use_batch_stats, void* stream);

/* ---- MaxPool2d(2,2) (models/unet.py:92; with indices models/segnet.py:79) and MaxUnpool2d (segnet.py:80) ------
 * floor output size; first maximum wins ties.  code (nullable): uint8 window position 0..3 (= 2*dy+dx) of the
 * arg-max, the compact form of torch's int64 flat indices. */
int cvk_maxpool2x2_fwd(cvk_view x, float* out, uint8_t* code, int N, int H, int W, int C, void* stream);
/* dx(view) (+)= route(dout) ; arg-max recomputed from x when code == NULL.  accumulate=0 overwrites (and zeroes
 * the odd trailing row/column), accumulate=1 adds. */
int cvk_maxpool2x2_bwd(const float* dout, cvk_view x, const uint8_t* code, cvk_view dx, int accumulate,
                       int N, int H, int W, int C, void* stream);
/* ... that also leaves the first pass of the PRODUCING block's BatchNorm+ReLU backward (nn.BatchNorm2d + nn.ReLU of models/unet.py:12-13 in front of the
 * nn.MaxPool2d of :92; backward of train.py:131): the pool backward is the last writer of the block's output gradient dx and touches every element, so it
 * sums g = dx * [ReLU passed] and g * xhat on the way — part = float[2][cvk_maxpool2x2_bwd_bnred_blocks(N,H,W,C)][C] for cvk_colsum_finalize; yP [N*H*W][ldp]
 * is the block's conv output, scale / shift / mean / rstd as for cvk_bn_bwd_reduce, which is then not launched.  _blocks returns 0 for unsupported C. */
int cvk_maxpool2x2_bwd_bnred_blocks(int N, int H, int W, int C);
int cvk_maxpool2x2_bwd_bnred(const float* dout, cvk_view x, const uint8_t* code, cvk_view dx, int accumulate, int N, int H, int W, int C,
                             const float* yP, int ldp, const float* scale, const float* shift, const float* mean, const float* rstd,
                             float* part, void* stream);
int cvk_maxunpool2x2_fwd(const float* v, const uint8_t* code, float* out, int N, int H, int W, int C, void* stream);
int cvk_maxunpool2x2_bwd(const float* dout, const uint8_t* code, float* dv, int N, int H, int W, int C, void* stream);
/* uint8 codes -> torch-style int64 flat H*W indices in NCHW order (API parity with return_indices=True) */
int cvk_pool_code_to_index(const uint8_t* code, int64_t* idx, int N, int H, int W, int C, void* stream);

/* ---- bilinear x2, align_corners=True (nn.Upsample: models/unet.py:25) -----------------------------------------
 * x: dense [N,H,W,C] (ld=C) -> out dense [N,2H,2W,C];  bwd: dx = transpose(dout). */
int cvk_bilinear_up2_fwd(const float* x, float* out, int N, int H, int W, int C, void* stream);
int cvk_bilinear_up2_bwd(const float* dout, float* dx, int N, int H, int W, int C, void* stream);

/* ---- softmax cross-entropy, mean over pixels (nn.CrossEntropyLoss(): train.py:105,130-131) --------------------
 * logits: dense NHWC rows [M][ld] (ld <= 128), target int64 [M].  Pixels whose target equals ignore_index (torch's
 * default -100; the reference passes none, so every CamVid class incl. Void is trained) are left out of the mean and get
 * a zero gradient.  fwd writes loss[0] = mean over the valid pixels, loss[1] = their number, loss[2] = number of
 * targets outside [0,C) that are not ignore_index (then loss[0] = NaN: torch raises there); `part` is scratch of
 * 3 * cvk_ce_blocks(M) floats.  bwd: dlogits = (softmax - onehot) * (*grad_out) * scale / loss3[1]; loss3 is fwd's loss. */
int cvk_ce_blocks(int M);
int cvk_softmax_ce_fwd(const float* logits, int ld, const int64_t* target, float* part, float* loss,
                       int M, int C, int ignore_index, void* stream);
int cvk_softmax_ce_bwd(const float* logits, int ld, const int64_t* target, const float* loss3, const float* grad_out,
                       float scale, float* dlogits, int ld_d, int M, int C, int ignore_index, void* stream);

/* ---- softmax cross-entropy with class weights, label smoothing and a reduction (nn.CrossEntropyLoss(weight=w,
 * label_smoothing=eps, reduction=...)) ------------------------------------------------------------------------------
 * logits: dense NHWC rows [M][ld] (ld >= C, 0 < C <= 128), target int64 [M] (DEVICE).  weight: DEVICE float [C], nullable (all
 * ones); label_smoothing eps in [0, 1]; reduction CVK_REDUCTION_*.  With lse = log sum_c exp(x[c]) and t = target, a pixel's
 *   loss = (1 - eps) w[t] (lse - x[t]) + (eps / C) sum_c w[c] (lse - x[c]);
 * mean = sum of the losses / sum of w[t] (0/0 = NaN when every pixel is ignored), sum = their sum.  Pixels whose target equals
 * ignore_index count nowhere and get a zero gradient; any other target outside [0, C) makes the loss NaN and is counted, as in
 * cvk_softmax_ce_fwd.  fwd: `part` is DEVICE scratch of cvk_ce_ex_part_floats(M) floats; loss is DEVICE float[4]: loss[0] = the
 * reduced loss (reduction none: the sum), loss[1] = valid pixels, loss[2] = out-of-range targets, loss[3] = the backward's divisor
 * (mean: sum of w[t]; sum / none: 1).  loss_px: DEVICE float [M], per-pixel loss (0 where ignored, NaN where out of range);
 * required for reduction none, nullable otherwise.  No allocation, no float atomics (fixed-order fp64 finish), no host sync.
 * bwd: dlogits [M][ld_d] = g (softmax ((1 - eps) w[t] + (eps / C) sum_c w[c]) - (1 - eps) w[t] onehot(t) - (eps / C) w),
 * g = grad_out * scale / loss4[3]; loss4 is fwd's loss.  grad_out: DEVICE, float [M] for reduction none (required), else one
 * float (nullable: 1).  Rows of ignored or out-of-range targets and columns [C, ld_d) are written as zeros. */
#define CVK_REDUCTION_NONE 0
#define CVK_REDUCTION_MEAN 1
#define CVK_REDUCTION_SUM 2
int cvk_ce_ex_part_floats(int M);
int cvk_softmax_ce_fwd_ex(const float* logits, int ld, const int64_t* target, const float* weight, float label_smoothing,
                          int reduction, float* part, float* loss, float* loss_px, int M, int C, int ignore_index, void* stream);
int cvk_softmax_ce_bwd_ex(const float* logits, int ld, const int64_t* target, const float* weight, float label_smoothing,
                          int reduction, const float* loss4, const float* grad_out, float scale, float* dlogits, int ld_d,
                          int M, int C, int ignore_index, void* stream);

/* ---- fused focal + soft-Dice segmentation loss, L = ce F + dice D ------------------------------------------------------------
 * logits: dense NHWC rows [M][ld] (ld >= C, 0 < C <= 128), target int64 [M], weight float [C] nullable (all ones): all DEVICE.
 * ce, dice >= 0 and not both 0, focal_gamma >= 0, dice_smooth s >= 0 (all finite); dice_average CVK_DICE_*.  With p = softmax(x),
 * t = target and every sum over the valid pixels (t != ignore_index) of the call:
 *   F = sum w[t] (1 - p[t])^gamma (lse - x[t]) / sum w[t]          (gamma = 0: the weighted mean of cvk_softmax_ce_fwd_ex; 0/0 = NaN)
 *   I_c = sum p[c] [t = c], P_c = sum p[c], T_c = sum [t = c], dice_c = (2 I_c + s) / (P_c + T_c + s)
 *   D = 1 - (1 / K) sum_{c in S} dice_c, S = the classes with T_c > 0 (CVK_DICE_PRESENT) or every class (CVK_DICE_ALL), K = |S|;
 *   K = 0 gives D = 0; a class with P_c + T_c + s = 0 counts as dice_c = 1 with a zero gradient.  Class weights do not enter D.
 * A term whose coefficient is 0 is not computed and cannot make L NaN.  Any target outside [0, C) other than ignore_index makes L
 * NaN and is counted, as in cvk_softmax_ce_fwd.
 * fwd: `part` is DEVICE scratch of cvk_seg_loss_part_floats(M, C) floats; `record` is DEVICE float[cvk_seg_loss_record_floats(C)]:
 * record[0] = L, [1] = valid pixels, [2] = out-of-range targets, [3] = sum w[t], [4] = F (0 when ce = 0), [5] = D (0 when dice = 0),
 * [6] = K, then dice_c[C] (0 outside S), a_c[C] = -2 / (K den_c) and b_c[C] = (2 I_c + s) / (K den_c^2), den_c = P_c + T_c + s (0
 * outside S).  Two launches (one pass over the logits, a one-workgroup fp64 finish); no allocation, no float atomics (every sum in
 * one fixed order: bitwise reproducible), no host sync.
 * bwd: record is fwd's; one pass, dlogits [M][ld_d] =
 *   g (ce w[t] / record[3] B ([k = t] - p[k]) + dice p[k] (g_k - sum_c g_c p[c])),  g_c = b_c + a_c [t = c],
 *   B = gamma p[t] (1 - p[t])^(gamma - 1) log p[t] - (1 - p[t])^gamma (finite when p[t] rounds to 1),  g = grad_out * scale;
 * grad_out: one DEVICE float, nullable (1).  Rows of ignored or out-of-range targets and columns [C, ld_d) are written as zeros. */
#define CVK_DICE_PRESENT 0
#define CVK_DICE_ALL 1
int cvk_seg_loss_part_floats(int M, int C);
int cvk_seg_loss_record_floats(int C);
int cvk_seg_loss_fwd(const float* logits, int ld, const int64_t* target, const float* weight, float ce, float dice, float focal_gamma,
                     float dice_smooth, int dice_average, float* part, float* record, int M, int C, int ignore_index, void* stream);
int cvk_seg_loss_bwd(const float* logits, int ld, const int64_t* target, const float* weight, float ce, float dice, float focal_gamma,
                     const float* record, const float* grad_out, float scale, float* dlogits, int ld_d, int M, int C, int ignore_index,
                     void* stream);

/* ---- knowledge-distillation loss, L = ce H + kd K (cross-entropy on the labels + temperature-softened KL towards a teacher) -------
 * student: dense NHWC rows [M][ld_s], teacher: [M][ld_t] (each ld >= C, 0 < C <= 128; the two strides are independent), target int64
 * [M], weight float [C] nullable (all ones): all DEVICE.  ce, kd >= 0, finite and not both 0.  tau = float(1 / T) and t2 = float(T T)
 * for a temperature T > 0, each evaluated in double by the caller and rounded once; both positive and finite.  For a pixel with
 * student row x, teacher row z and target t:
 *   p = softmax(x), ps = softmax(tau x), qs = softmax(tau z),
 *   kl = sum_c qs_c (log qs_c - log ps_c), taken from the two log-sum-exps (no log of a softmax value; 0 when z holds x's numbers)
 *   H = sum_{valid} w[t] (lse(x) - x[t]) / sum_{valid} w[t]        (valid: t != ignore_index; the weighted mean of
 *                                                                   cvk_softmax_ce_fwd_ex; 0/0 = NaN)
 *   K = t2 sum_{m in D} kl_m / |D|                                 (0/0 = NaN)
 * D = the valid pixels, or every pixel when distill_ignored != 0 (an ignored pixel has no label but the teacher has an opinion).
 * Class weights enter H only.  A term whose coefficient is 0 is not computed and cannot make L NaN.  Any target outside [0, C) other
 * than ignore_index makes L NaN and is counted, as in cvk_softmax_ce_fwd; such a pixel is in neither set.  target may be null when
 * ce = 0: no pixel has a label, every pixel is in D and counts as valid.  teacher may be null when kd = 0: L = H.
 * fwd: `part` is DEVICE scratch of cvk_kd_loss_part_floats(M) floats; `record` is DEVICE float[cvk_kd_loss_record_floats()] = float[9]:
 * [0] = L, [1] = valid pixels, [2] = out-of-range targets, [3] = sum w[t], [4] = H (0 when ce = 0), [5] = K (0 when kd = 0), [6] = |D|,
 * [7] = pixels of D where student and teacher agree on the arg-max (first index of the maximum, as cvk_argmax_channels; 0 when
 * kd = 0), [8] = [7] / [6] (0 when kd = 0).  Counts stored as floats are exact up to 2^24 pixels.  Two launches (one pass over both
 * logit tensors, a one-workgroup fp64 finish); no allocation, no float atomics (every sum in one fixed order: bitwise reproducible), no
 * host sync.  The pass stages 256 pixel rows of each tensor in LDS while (ld_s + 1) + (ld_t + 1) <= 64 (the teacher's tile is left out
 * when kd = 0) and walks the rows in global memory beyond that.
 * bwd: record is fwd's; one pass that re-reads both tensors, dlogits [M][ld_d] (ld_d >= C), the student's gradient only:
 *   g (ce w[t] / record[3] (p_k - [k = t]) on valid pixels  +  kd t2 tau / record[6] (ps_k - qs_k) on pixels of D),
 * g = grad_out * scale; grad_out: one DEVICE float, nullable (1).  Rows outside both sets and columns [C, ld_d) are written as zeros. */
int cvk_kd_loss_part_floats(int M);
int cvk_kd_loss_record_floats(void);
int cvk_kd_loss_fwd(const float* student, int ld_s, const float* teacher, int ld_t, const int64_t* target, const float* weight, float ce,
                    float kd, float tau, float t2, int distill_ignored, float* part, float* record, int M, int C, int ignore_index,
                    void* stream);
int cvk_kd_loss_bwd(const float* student, int ld_s, const float* teacher, int ld_t, const int64_t* target, const float* weight, float ce,
                    float kd, float tau, float t2, int distill_ignored, const float* record, const float* grad_out, float scale,
                    float* dlogits, int ld_d, int M, int C, int ignore_index, void* stream);

/* ---- OHEM cross-entropy: online hard example mining with an on-device k-th-largest select ---------------------------------------
 * logits: dense NHWC rows [M][ld] (ld >= C, 0 < C <= 128), target int64 [M], weight float [C] nullable (all ones): all DEVICE.
 * A pixel's loss l = lse - x[t] is the unweighted fp32 cross-entropy (>= 0).  V = the valid pixels (t != ignore_index),
 * k = min(min_kept, V), L = the k-th largest l over the valid pixels.  A valid pixel is kept iff l > loss_thresh or l >= L (fp32
 * comparisons): every pixel harder than the threshold, never fewer than the min_kept hardest, ties at the boundary all kept.
 *   loss = sum_kept w[t] l / sum_kept w[t]                       (V = 0: 0/0 = NaN)
 * loss_thresh = -log(probability threshold) >= 0 and finite; min_kept >= 1.  Any target outside [0, C) other than ignore_index
 * makes the loss NaN and is counted, as in cvk_softmax_ce_fwd.
 * fwd: `scratch` is DEVICE memory of cvk_ohem_scratch_bytes(M) bytes (cleared by the call itself, on the stream); `record` is DEVICE
 * float[cvk_ohem_record_floats()] = float[8]: [0] = loss, [1] = V, [2] = out-of-range targets, [3] = sum_kept w[t], [4] = kept
 * pixels, [5] = L, [6] = loss_thresh, [7] = k (counts stored as floats are exact up to 2^24 pixels); loss_px: DEVICE float [M],
 * required: l per pixel, -1 where ignored, NaN where the target is out of range.  L is exact: a three-level radix select (11 + 10 +
 * 10 bits) over the bit patterns of l with integer histogram atomics; no float atomics, every float sum in one fixed order (bitwise
 * reproducible), no allocation, no host sync.  Ranks and counts are 32-bit.
 * bwd: record and loss_px are fwd's; dlogits [M][ld_d] = g w[t] / record[3] (softmax(x) - onehot(t)) on the kept rows,
 * g = grad_out * scale; grad_out: one DEVICE float, nullable (1).  The kept predicate is re-evaluated from loss_px, record[5] and
 * record[6], so it cannot differ from the forward's.  Rows that are not kept, ignored or out of range and columns [C, ld_d) are
 * written as zeros. */
int cvk_ohem_scratch_bytes(int M);
int cvk_ohem_record_floats(void);
int cvk_ohem_ce_fwd(const float* logits, int ld, const int64_t* target, const float* weight, float loss_thresh, int min_kept,
                    void* scratch, float* record, float* loss_px, int M, int C, int ignore_index, void* stream);
int cvk_ohem_ce_bwd(const float* logits, int ld, const int64_t* target, const float* weight, const float* record,
                    const float* loss_px, const float* grad_out, float scale, float* dlogits, int ld_d, int M, int C, int ignore_index,
                    void* stream);

/* ---- Lovász-softmax loss (Berman, Triki, Blaschko, CVPR 2018) with an on-device segmented radix sort; not in the reference --------
 * loss = lovasz * J + ce * H.  logits: dense NHWC rows [M][ld] (ld >= C, 0 < C <= 128), target int64 [M], weight float [C] nullable
 * (all ones, enters H only): all DEVICE.  M = N * pixels_per_image.  A segment is the whole batch (per_image = 0) or one image
 * (per_image = 1): S = 1 or N segments of P = M / S pixels.  Per segment and class c, over the valid pixels (t != ignore_index and t in
 * [0, C)) in memory order i, with p = softmax(x) in fp32:
 *   e_i = p_i[c] where t_i != c, and (sum_{j != c} exp_j) / sum_j exp_j where t_i = c;  G = the number of pixels with t_i = c
 *   order the valid pixels by e descending, ties by ascending i; at position n with F foreground pixels strictly before it,
 *   U = G + n - F, I = G - F:  g = 1 / U (foreground), g = I / (U (U + 1)) (background); G = 0: g = 1 at n = 0, else 0
 *   (evaluated in fp64, rounded once to fp32);  L_c = sum e_i g_i in fp64 in sorted order.
 * A (segment, class) pair is evaluated when the segment has a valid pixel and (classes_mode = CVK_LOVASZ_ALL or G > 0).  Segment loss =
 * mean of L_c over its K evaluated classes; a segment with K = 0 is not counted; J = mean over the counted segments (none: 0).
 * H = the weighted mean cross-entropy of cvk_softmax_ce_fwd_ex (label_smoothing 0), computed only when ce > 0 (0/0 = NaN when no pixel
 * is valid).  lovasz > 0, ce >= 0, both finite; weight needs ce > 0.  A target outside [0, C) other than ignore_index makes the loss NaN
 * and is counted; such a pixel and the ignored ones take part in no order and get a zero gradient row.
 * The order comes from a stable LSD radix sort, CVK_LOVASZ_DIGIT_BITS bits a pass over the 32-bit key 0x3f800000 - bits(e) (ignored:
 * 0xffffffff), S * C independent segments, work-groups of CVK_LOVASZ_SORT_TILE elements; histograms are integer counts, every float sum
 * has one fixed order: loss and gradient are bitwise reproducible.  Limits: P < 2^30, S * C <= 65535, ceil(P / tile) <= 2^22.
 * workspace: DEVICE, cvk_lovasz_workspace_bytes(M, C, segments) bytes (0: unsupported sizes), 16-byte aligned, contents need not be
 *   initialised.  Bytes [0, 8 M C) hold the sorted elements after fwd: segment (s, c) at element (s C + c) P, each uint64 =
 *   key << 32 | pixel index inside the segment << 1 | foreground bit.  Bytes [8 M C, 16 M C) are the second sort buffer.  Bytes
 *   [16 M C, 20 M C) are room for a dense g map ([M][C] floats) that `gmap` may point to; tables follow.
 * gmap: DEVICE float [M][ld_g] (ld_g >= C): g of every valid pixel and class in pixel order (0 for a pair that is not evaluated);
 *   rows of other pixels and columns [C, ld_g) are not written.
 * record: DEVICE float[cvk_lovasz_record_floats()] = float[264]: [0] = loss, [1] = valid pixels, [2] = out-of-range targets, [3] = J,
 *   [4] = H (0 when ce = 0), [5] = evaluated (segment, class) pairs, [6] = counted segments, [7] = sum of w[t] over the valid pixels
 *   (H's divisor, 0 when ce = 0); [8 + c] = L_c, the mean over the segments that evaluated class c (NaN: none did); [136 + c] = G_c
 *   over the batch; c < C, the other slots are not written.
 * bwd: dlogits [M][ld_d]: dx_j = p_j (s_j - sum_c s_c p_c) + ce g w[t] (p_j - [j = t]) / record[7], s_c = lovasz g sign_c gmap[c] /
 *   (K counted segments), sign_c = -1 for c = t and +1 otherwise, g = grad_out * scale; grad_out: one DEVICE float, nullable (1).
 *   Takes the workspace, record and gmap of the forward.  Rows of ignored or out-of-range pixels and columns [C, ld_d) are zeros.
 * cvk_lovasz_sort_dest / cvk_lovasz_sort_count_index: the two index functions of the sort, the same code the kernels run, for host
 *   tests: element index of (segment, digit base, work-group base, rank) in a buffer of segments of seg_len elements, and the index
 *   of (segment, digit, work-group) in the count table; -1 when a piece is out of range (the kernels then store nothing). */
#define CVK_LOVASZ_PRESENT 0
#define CVK_LOVASZ_ALL 1
#define CVK_LOVASZ_DIGIT_BITS 8
#define CVK_LOVASZ_SORT_TILE 2048
int64_t cvk_lovasz_workspace_bytes(int M, int C, int segments);
int     cvk_lovasz_record_floats(void);
int64_t cvk_lovasz_sort_dest(int64_t seg_len, int64_t segment, int64_t digit_base, int64_t wg_base, int64_t rank);
int64_t cvk_lovasz_sort_count_index(int64_t work_groups, int64_t segment, int64_t digit, int64_t work_group);
int cvk_lovasz_softmax_fwd(const float* logits, int ld, const int64_t* target, const float* weight, float lovasz, float ce,
                           int classes_mode, int per_image, int N, int pixels_per_image, void* workspace, float* record, float* gmap,
                           int ld_g, int C, int ignore_index, void* stream);
int cvk_lovasz_softmax_bwd(const float* logits, int ld, const int64_t* target, const float* weight, float lovasz, float ce,
                           int per_image, int N, int pixels_per_image, const void* workspace, const float* record, const float* gmap,
                           int ld_g, const float* grad_out, float scale, float* dlogits, int ld_d, int C, int ignore_index,
                           void* stream);

/* ---- exact Euclidean distance transform of a label batch, and the boundary loss on it (Kervadec et al., MIDL 2019); not in the
 * reference -----------------------------------------------------------------------------------------------------------------------------
 * labels: DEVICE int64 [N][H][W].  A pixel whose label is ignore_index or outside [0, num_classes) belongs to no class (void); it still
 * counts as "not class c" for every c.  Everything is per image.  With M = N H W:
 *   to_class [M][C] int32: the squared Euclidean distance to the nearest pixel of the image whose label is c, exact; -1 where the image
 *     has no pixel of class c.
 *   to_other [M] int32: the squared distance to the nearest pixel of the image whose category (class, or void) differs from this
 *     pixel's; -1 where there is none.
 *   phi [M][C] float (NHWC): +sqrt(to_class) where the pixel is not of class c, -(sqrt(to_other) - 1) where it is (Kervadec's
 *     one_hot2dist), 0 wherever the needed distance is -1.  The root is the correctly rounded fp32 root of the exactly converted integer.
 * Limits: 1 <= num_classes <= 32, H <= 65534, (H - 1)^2 + (W - 1)^2 < 2^24, N H W < 2^31.
 * workspace: DEVICE, cvk_edt_workspace_bytes(N, H, W, num_classes) bytes (0: unsupported sizes), 16-byte aligned, contents need not be
 *   initialised: the uint16 column distances [M][C + 1] (channel c: the vertical distance to the nearest pixel of class c in the column;
 *   channel C: to the nearest pixel of the column with another category; 0xFFFF: none), then per image the class-presence word and the
 *   void flag.  cvk_edt_squared and cvk_edt_signed run the same two passes and one device function makes the integers of both.
 * Boundary loss: loss = cb B + cc H.  logits: dense NHWC rows [M][ld] (C <= ld <= 63, 1 <= C <= 32), target int64 [M], phi float [M][C]
 * (cvk_edt_signed of the target with the same ignore_index), weight float [C] nullable (all ones, enters H only), coef float[2] =
 * {cb, cc}: all DEVICE; the coefficients are read by the kernels, so a captured graph follows a change of them.
 *   V = the pixels whose target is a class; S = the classes of class_mask (bit c); p = softmax(x) in fp32
 *   B = 1 / |V| sum_{q in V} sum_{c in S} phi_c(q) p_c(q), 0 when V is empty;  H = the weighted mean cross-entropy of
 *   cvk_softmax_ce_fwd_ex (label_smoothing 0; 0/0 = NaN when V is empty).  want_boundary / want_ce (0 or 1, not both 0) say which terms
 *   exist: a term that is off is not computed and its coefficient is not read (phi may be null without the boundary term; weight needs
 *   the cross-entropy term).  A target outside [0, C) other than ignore_index makes the loss NaN and is counted.
 * part: DEVICE scratch, cvk_boundary_loss_part_floats(M, C) floats.
 * record: DEVICE float[cvk_boundary_loss_record_floats()] = float[40]: [0] = loss, [1] = |V|, [2] = out-of-range targets, [3] = B,
 *   [4] = H, [5] = cb and [6] = cc as the forward read them (0 for a term that is off), [7] = sum of w[t] over V (0 without H),
 *   [8 + c] = class c's share of B (they sum to B; 0 for c >= C).
 * bwd: dlogits [M][ld_d] (ld_d >= C): dx_k = g cb p_k (phi_k [k in S] - sum_{c in S} phi_c p_c) / |V| + g cc w[t] (p_k - [k = t]) /
 *   record[7], g = grad_out * scale (grad_out: one DEVICE float, nullable = 1); cb, cc, |V| from the forward's record.  Rows of pixels
 *   outside V and columns [C, ld_d) are zeros.  Every sum has one fixed order and there is no float atomic. */
int64_t cvk_edt_workspace_bytes(int N, int H, int W, int num_classes);
int cvk_edt_squared(const int64_t* labels, int N, int H, int W, int num_classes, int ignore_index, void* workspace, int32_t* to_class,
                    int32_t* to_other, void* stream);
int cvk_edt_signed(const int64_t* labels, int N, int H, int W, int num_classes, int ignore_index, void* workspace, float* phi,
                   void* stream);
int cvk_boundary_loss_part_floats(int M, int C);
int cvk_boundary_loss_record_floats(void);
int cvk_boundary_loss_fwd(const float* logits, int ld, const int64_t* target, const float* phi, const float* weight, const float* coef,
                          int want_boundary, int want_ce, unsigned class_mask, float* part, float* record, int M, int C,
                          int ignore_index, void* stream);
int cvk_boundary_loss_bwd(const float* logits, int ld, const int64_t* target, const float* phi, const float* weight, int want_boundary,
                          int want_ce, unsigned class_mask, const float* record, const float* grad_out, float scale, float* dlogits,
                          int ld_d, int M, int C, int ignore_index, void* stream);

/* ---- class statistics of label masks (class weights for the loss above; SegNet's median-frequency balancing) ----------
 * masks: DEVICE [N][HW] of mask_bytes = 1 (uint8) or 8 (int64) per label (cvk_augment_u8's convention); 0 < num_classes <= 256.
 * Accumulates into DEVICE int64 hist[2 * num_classes + 1] (the caller zeroes it once): hist[c] += pixels of class c,
 * hist[num_classes + c] += the counted pixels (labels in [0, num_classes)) of every mask in which c occurs, hist[2 * num_classes]
 * += labels outside [0, num_classes) that are not ignore_index.  Labels equal to ignore_index are skipped.  One workgroup per
 * mask, integer atomics only (exact, so the result does not depend on the order); no host sync. */
int cvk_class_histogram(const void* masks, int mask_bytes, int N, int64_t HW, int num_classes, int ignore_index, int64_t* hist,
                        void* stream);

/* ---- evaluation (train.py:191 argmax; utils.py:162-190 histograms) -------------------------------------------- */
int cvk_argmax_channels(const float* logits, int ld, int64_t* out, int M, int C, void* stream);
/* hist int64[3][num_classes] += (intersection, prediction area, label area), pixels with label==ignore skipped */
int cvk_confusion_accumulate(const int64_t* pred, const int64_t* label, int64_t* hist, int M, int num_classes,
                             int ignore_index, void* stream);

/* ---- boundary F1 (BF score; Csurka et al., BMVC 2013): per-image, per-class contour counts (not in the reference) -------
 * pred, label: DEVICE int64 [N][H][W]; 1 <= num_classes <= 32; r2: squared tolerance in pixels, 0 <= r2 <= 256.
 * A pixel is void iff label == ignore_index, in both maps (the prediction is masked by the label).  A non-void pixel z of a map X
 * (the masked prediction or the label) is a boundary pixel of class c iff X(z) = c, 0 <= c < num_classes, c != ignore_index, and at
 * least one of its 4-neighbours inside the image is non-void and holds a value other than c.  A value outside [0, num_classes), or
 * ignore_index at a non-void pixel, has no boundary of its own, is different from every class for its neighbours and indexes
 * nothing.  A boundary pixel of class c in one map is matched iff the other map has a boundary pixel of class c at an integer
 * offset (dy, dx), dy * dy + dx * dx <= r2, inside the same image.
 * cvk_boundary_counts ADDS into DEVICE int64 counts[N][4][num_classes] (the caller zeroes it): row 0 = prediction boundary pixels,
 * row 1 = those matched in the label map, row 2 = label boundary pixels, row 3 = those matched in the prediction map.  One launch,
 * integer atomics only (exact: the result does not depend on the order or on the tiling), no allocation, no host sync.
 * cvk_boundary_map writes the boundary map of `map` alone: out_u8 [N][H][W] = the class whose boundary the pixel carries, or 255.
 * void_from (nullable) is the label map whose ignore_index pixels are void; NULL: map's own.  Both entry points evaluate one rule.
 * N * H * W < 2^31. */
int cvk_boundary_counts(const int64_t* pred, const int64_t* label, int64_t* counts, int N, int H, int W, int num_classes,
                        int ignore_index, int r2, void* stream);
int cvk_boundary_map(const int64_t* map, const int64_t* void_from, uint8_t* out_u8, int N, int H, int W, int num_classes,
                     int ignore_index, void* stream);

/* ---- surface distances: Hausdorff distance, its percentile (HD95) and the average symmetric surface distance (not in the reference) ---
 * pred, label: DEVICE int64 [N][H][W]; 1 <= num_classes <= 32.  Void pixels, the masked prediction and "contour pixel of class c" are
 * those of cvk_boundary_counts / cvk_boundary_map above, exactly: void iff label == ignore_index, in both maps; 4-connected; the image
 * border makes no contour; a value that is no class has no contour of its own but bounds its neighbours.  Everything is per image.
 * For a contour pixel z of class c of the prediction, d2_PG(z) is the squared Euclidean distance, an exact integer, to the nearest
 * contour pixel of class c of the label map of the same image, -1 when the label map has none; d2_GP is the same with the maps
 * exchanged.  Limits, those of the distance transform: H <= 65534, (H - 1)^2 + (W - 1)^2 < 2^24, N H W < 2^31.
 *   d2: DEVICE int32 [2][N][H][W]: plane 0 holds d2_PG at the prediction's contour pixels, plane 1 d2_GP at the label's; every other
 *     pixel holds -2.
 *   record: DEVICE int64 [N][2][num_classes][8], WRITTEN (not added into); direction 0 = P -> G, 1 = G -> P.  Of the segment (image,
 *     direction, class c), whose values are the d2 of the source map's contour pixels of class c:
 *       [0] n = contour pixels of class c in the source map,  [1] m = those in the other map;
 *           the segment is "evaluated" iff n > 0 and m > 0 (then every d2 of it is >= 0);
 *       [2] the largest d2 (-1 unless evaluated);
 *       [3] Q = the sum over the segment of isqrt(d2 << 32), the largest integer q with q * q <= d2 * 2^32: the distance in 2^-16 pixels,
 *           defined by integers alone (0 unless evaluated; q < 2^28 and fewer than 2^31 pixels, so Q fits);
 *       [4] k = floor((n - 1) qnum / qden),  [5] r = ((n - 1) qnum) mod qden;
 *       [6] d2_lo = the k-th smallest d2 of the segment (0-based),
 *       [7] d2_hi = the min(k + 1, n - 1)-th smallest when r > 0, else d2_lo;     [4]..[7] are -1 unless evaluated.
 *     qnum / qden is the percentile as a fraction, 0 <= qnum <= qden <= 10000 (95, 100 for HD95).  With a = sqrt(d2_lo), b = sqrt(d2_hi)
 *     the percentile of the distances under numpy's default "linear" rule is a + (b - a) r / qden; the Hausdorff distance of a class is
 *     the larger sqrt([2]) of the two directions; ASSD = (Q_PG + Q_GP) / 65536 / (n_P + n_G).
 * workspace: DEVICE, cvk_surface_workspace_bytes(N, H, W, num_classes) bytes (0: unsupported sizes), 16-byte aligned, contents need not
 *   be initialised: the entry point clears what it needs on the given stream.  It holds the uint16 column distances [2][M][C] to the
 *   contours of either map, the contour bytes [2][M], and per segment the integer sums and the two histograms of the select.
 * cvk_surface_record_slots() = 8.  Integer atomics only: the outputs do not depend on the order of arrival, two runs agree bit for bit.
 * No allocation, no host sync.  The rank values come from an exact histogram select per segment: one bin per value below 4096, above
 * it one bin per 4096 values and a second level over the low 12 bits. */
int64_t cvk_surface_workspace_bytes(int N, int H, int W, int num_classes);
int cvk_surface_record_slots(void);
int cvk_surface_distances(const int64_t* pred, const int64_t* label, int N, int H, int W, int num_classes, int ignore_index, int qnum,
                          int qden, void* workspace, int32_t* d2, int64_t* record, void* stream);

/* ---- chessboard depth, Boundary IoU (Cheng et al., CVPR 2021) and trimap counts (not in the reference) ---------------------------
 * Codes.  A pixel of an int64 map X [N][H][W] becomes one byte: its class when X is in [0, num_classes) and not ignore_index, 254 for
 * any other value, 255 (void) where void_from == ignore_index.  void_from (nullable: X's own) is the label map; a prediction takes the
 * label's void, as in cvk_boundary_counts.  1 <= num_classes <= 32.
 * Depth.  For a pixel z whose code is a class, depth0(z) is the smallest k >= 1 for which the (2k+1) x (2k+1) square around z, clipped
 * to the image, holds a pixel whose code differs from z's: void and 254 are codes like any other here and bound the regions beside
 * them (unlike the contour rule above, where void never differs).  A pixel whose code is no class has depth 0.  With the image border
 * counted as outside, depth1(z) = min(depth0(z), 1 + min(x, W-1-x, y, H-1-y)).  The class-c mask eroded d times by a 3 x 3 square is
 * {code = c and depth > d}, its band {code = c and depth <= d}: depth1 with a zero pad around the image (Cheng's), depth0 without.
 * cvk_cheb_depth writes code_u8 and depth_u8 (DEVICE uint8 [N][H][W]): depth_u8 = min(depth0, max_depth + 1) for border == 0 and
 * min(depth0, max_depth + 1, the border term) for border == 1; 1 <= max_depth <= 254 is the largest band any consumer compares
 * against, and no search runs farther.  workspace: DEVICE, cvk_cheb_workspace_bytes(N, H, W) bytes (0: unsupported sizes: W > 32768 or
 * N H W >= 2^31); it holds the row distances.  Two launches: rows, then columns (depth0 = min over y' of max(|y - y'|, g(x, y')), g the
 * row distance where the code is z's and 0 elsewhere).
 * cvk_boundary_iou_counts reads the codes and depth0 maps (border == 0, max_depth >= dilation and >= the last width) of the masked
 * prediction (p) and the label (l) and ADDS into DEVICE int64 counts[N][6][num_classes] (the caller zeroes it), per image and class c:
 *   row 0 bG = label pixels of class c with depth1 <= dilation,  row 1 bP = the same of the prediction,
 *   row 2 bI = pixels where both maps have class c and both are within their band,
 *   row 3 aG, row 4 aP = the areas of the two masks,  row 5 aI = the area of their intersection.
 * trimap (nullable): DEVICE int64 [nw][num_classes][num_classes], ADDED into: a pixel whose label and prediction are classes adds 1 at
 * [i][label][prediction] for the smallest i with depth0 of the label <= widths[i] (the image border is no boundary; deeper pixels add
 * nothing).  widths: HOST int [nw], strictly increasing, each in 1..254, 1 <= nw <= 8, copied into the launch arguments.
 * 1 <= dilation <= 254.  One launch, integer atomics only: two runs agree bit for bit.  No allocation, no host sync. */
int64_t cvk_cheb_workspace_bytes(int N, int H, int W);
int cvk_cheb_depth(const int64_t* map, const int64_t* void_from, uint8_t* code_u8, uint8_t* depth_u8, void* workspace, int N, int H,
                   int W, int num_classes, int ignore_index, int max_depth, int border, void* stream);
int cvk_boundary_iou_counts(const uint8_t* code_p, const uint8_t* depth_p, const uint8_t* code_l, const uint8_t* depth_l,
                            int64_t* counts, int64_t* trimap, const int* widths, int nw, int N, int H, int W, int num_classes,
                            int dilation, void* stream);

/* ---- connected components of a class map and the removal of small regions (not in the reference) --------------------------------
 * Codes.  A pixel of an int64 map X [N][H][W] has the code X when X is in [0, num_classes) and not ignore_index; every other value is
 * void, one code.  1 <= num_classes <= 32, N H W < 2^31, connectivity 4 or 8.
 * A component is a maximal set of pixels of one image with equal code, connected under `connectivity`; void pixels form components
 * too.  cvk_cc_label writes, DEVICE int32 [N][H][W] each: labels = y' W + x' of the first pixel of the pixel's component in row-major
 * order (so labels[p] <= index(p), with equality at exactly one pixel per component) and area = the size of the pixel's component, at
 * every pixel.  Four launches: a union-find per 32 x 64 tile in LDS, a lock-free merge over the tile seams (atomicMin; no work-group
 * waits for another), a flatten pass that counts areas by integer atomics, and the spread of the areas.  The result does not depend
 * on the order of arrival.
 * cvk_cc_filter reads map and the labels and area cvk_cc_label made of it under the same num_classes, ignore_index and connectivity
 * and writes out (DEVICE int64 [N][H][W], not overlapping map).  A class component is small iff area < min_area (min_area >= 1; 1
 * removes nothing); void components are never small.  mode 0 (fill): every pixel of a small component becomes fill_value.  mode 1
 * (neighbour): votes[k] of a small component S = the number of ordered pairs (p, q), p in S, q a neighbour of p inside the image under
 * `connectivity`, q of class k and q's component not small; S becomes the class with the most votes, the smallest such class on a
 * tie, and stays as it is without any vote.  One round: small components do not vote.  Every other pixel keeps its value bit for bit.
 * record (nullable): DEVICE int64 [N][num_classes][8], ADDED into (slot 2: raised to), the caller zeroes it; per image and class
 *   [0] components  [1] pixels  [2] largest area  [3] small components  [4] their pixels  [5] small components that changed value
 *   [6] pixels the class received from other classes  [7] small components without a vote (mode 1).
 * cvk_cc_record_slots() = 8.  workspace: DEVICE, cvk_cc_workspace_bytes(N, H, W, num_classes) bytes (0: unsupported sizes), the same
 * for both calls: parents int32 [M], code bytes [M], votes int32 [M][num_classes] indexed by a component's first pixel and touched
 * only there.  It need not be initialised and carries nothing from one call to the next.  No allocation, no host sync. */
int64_t cvk_cc_workspace_bytes(int N, int H, int W, int num_classes);
int cvk_cc_record_slots(void);
int cvk_cc_label(const int64_t* map, int32_t* labels, int32_t* area, int N, int H, int W, int num_classes, int ignore_index,
                 int connectivity, void* workspace, void* stream);
int cvk_cc_filter(const int64_t* map, const int32_t* labels, const int32_t* area, int64_t* out, int64_t* record, int N, int H, int W,
                  int num_classes, int ignore_index, int connectivity, int min_area, int mode, int64_t fill_value, void* workspace,
                  void* stream);

/* ---- multi-scale / flip test-time augmentation: the merge of the views' logits (not in the reference) ------------------
 * Bilinear resampling here is torch's F.interpolate(mode="bilinear", align_corners=False) with the sample position taken from
 * integers: for destination index d of `out` samples over `in` source samples, num = max((2 d + 1) in - out, 0), lower source
 * index i0 = num / (2 out), upper i1 = min(i0 + 1, in - 1), fraction f = float(num % (2 out)) / float(2 out) (rounded once),
 * weights (1 - f, f); the value is wy0 (wx0 a + wx1 b) + wy1 (wx0 c + wx1 d).  At in == out the weights are exactly (1, 0).
 *
 * cvk_tta_accumulate, one call per view, in view order: logits are the view's dense NHWC rows [N][h][w][ld] (ld >= C), acc is
 * dense float [N][H][W][C].  Per pixel (n, y, x): v = the logits resampled to H x W at (y, x) — at (y, W - 1 - x) when flip != 0,
 * the mirrored view turned back —, p = softmax(v) (max-subtracted) and
 *   first != 0: acc = p (acc is not read, the caller need not clear it), else acc += p;
 *   last  != 0: acc = (that sum) * inv_k, and pred (int64 [N][H][W], required) = the first-maximum channel of exactly the values
 *               stored (a NaN wins, as in cvk_argmax_channels).  first and last together: a softmax + arg-max pass.
 * Every sum runs in the order of the calls, no atomics: the result is bitwise reproducible.  1 <= C <= 32 (a pixel's classes are
 * held in registers), sizes up to 16384 per side, N * H * W * C < 2^31.  C % 4 == 0 with ld % 4 == 0 and 16-byte aligned pointers
 * moves rows as 16-byte vectors; anything else takes scalar paths.  One launch, no allocation, no host sync.
 *
 * cvk_tta_resize_input: a view's network input.  src: logical [N][3][H][W] float of any strides (in floats, as cvk_import_nchw)
 * -> dst dense NHWC [N][h][w][4] (cvk_preprocess_u8's layout, pad channel 0, 16-byte aligned), resampled as above; flip != 0
 * mirrors the result left-right (dst column x = resampled column w - 1 - x).  One launch. */
int cvk_tta_accumulate(const float* logits, int ld, int h, int w, float* acc, int64_t* pred, int N, int H, int W, int C, int flip,
                       int first, int last, float inv_k, void* stream);
int cvk_tta_resize_input(const float* src, int64_t sN, int64_t sC, int64_t sH, int64_t sW, float* dst, int N, int H, int W, int h, int w,
                         int flip, void* stream);

/* ---- sliding-window inference: the merge of overlapping windows' logits (not in the reference) --------------------------
 * The grid of an H x W image for a crop (hc, wc) and a stride (sy, sx), 1 <= sy <= hc, 1 <= sx <= wc (the rule of mmseg's
 * mode='slide'): window height hw = min(hc, H), gy = (max(H - hc, 0) + sy - 1) / sy + 1 window rows, row i starts at
 * y1(i) = min(i * sy, H - hw); columns likewise (ww, gx, x1).  All windows are hw x ww, the last row / column is pulled back inside
 * the image, no two windows coincide and every pixel is covered.  The windows that hold pixel (y, x) are grid rows lo_y..hi_y times
 * grid columns lo_x..hi_x with lo_y = y < hw ? 0 : min((y - hw) / sy + 1, gy - 1), hi_y = y >= H - hw ? gy - 1 : y / sy (x likewise),
 * cnt = (hi_y - lo_y + 1) * (hi_x - lo_x + 1) of them.
 *
 * cvk_window_merge, one call per window in row-major order of (iy, ix) on one stream: logits are window (iy, ix)'s dense NHWC rows
 * [N][hw][ww][ld] (ld >= C; the padding is never read into a result), out is dense float [N][H][W][C], pred int64 [N][H][W] or NULL.
 * Per pixel of the window, at image position (y, x) = (y1(iy) + wy, x1(ix) + wx), with l its logits:
 *   (iy, ix) == (lo_y, lo_x): out = l (out is not read: the caller never clears it), else out += l;
 *   (iy, ix) == (hi_y, hi_x): the pixel is finished: out = (that sum) / float(cnt), one correctly rounded fp32 division, and with
 *                             pred non-NULL pred = the first-maximum channel of exactly the values stored (a NaN wins, as in
 *                             cvk_argmax_channels).
 * Pixels outside the window are untouched.  Every sum runs in window order, no atomics, no memset: the result is bitwise
 * reproducible, and where cnt == 1 it is bitwise the window's logits.  1 <= C <= 32, sizes up to 16384 per side,
 * N * H * W * C < 2^31; a stride outside 1..crop or (iy, ix) outside the grid is CVK_EINVAL.  C % 4 == 0 with ld % 4 == 0 and
 * 16-byte aligned pointers moves 16-byte vectors; anything else takes scalar paths.  One launch, no allocation, no host sync. */
int cvk_window_merge(const float* logits, int ld, float* out, int64_t* pred, int N, int H, int W, int C, int hc, int wc, int sy, int sx,
                     int iy, int ix, void* stream);

/* ---- local-window mean-field CRF refinement of a prediction (Teichmann & Cipolla's ConvCRF form with a dilation; not in the
 * reference; the fully connected permutohedral CRF is NOT provided) -------------------------------------------------------------
 * Inputs.  U [N][H][W][C], the unary: logits, or probabilities (unary_is_prob != 0), which enter as U_c := log(max(U_c, FLT_MIN)).
 * A guide image I [N][3][H][W], I_k(p) = fma(a_k, x_k(p), b_k) in fp32, where x is the network's float input of any strides (in
 * elements, as cvk_import_nchw) and a_k = 255 std_k, b_k = 255 mean_k undo the normalisation on load (grey levels of 0..255); or,
 * with guide_u8 != 0, dense uint8 frames [N][H][W][3] taken as they are (the strides and a, b are ignored).  guide_a, guide_b: HOST
 * float [3] each (may be NULL with guide_u8), copied into the launch arguments.  Integers radius r in
 * 1..5, dilation d in 1..4, and T >= 1 iterations, one call each.
 * Offsets.  O = {(d i, d j) : -r <= i, j <= r} \ {(0, 0)}, walked in row-major order of (i, j); a neighbour p + o outside the image
 * contributes nothing, to no sum.
 * Kernels.  Appearance ka(p, o) = ga[o] * exp(cb * |I(p) - I(p + o)|^2), smoothness ks(p, o) = gs[o], with the tables
 * ga[o] = float32(exp(-|o|^2 / (2 theta_alpha^2))), gs[o] = float32(exp(-|o|^2 / (2 theta_gamma^2))) (|o|^2 = d^2 (i^2 + j^2), in
 * pixels) and cb = float32(-1 / (2 theta_beta^2)) made by the HOST in double precision and rounded once (cvk.crf_coefficients returns
 * exactly these); the tables are HOST float [(2r+1)^2] in row-major (i, j), the centre entry is never read, and they are copied into
 * the launch arguments.  The kernel's only exponentials are the colour term and the softmax.
 * Normalisation.  Each kernel by its own sum over the neighbours inside the image: na(p) = sum_o ka(p, o), ns(p) = sum_o ks(p, o);
 * a zero sum gives a zero message (a 1 x 1 image has no neighbour and returns softmax(U)).
 * Iteration.  Q_0 = softmax(U) (max-subtracted).  With Sa_c = sum_o ka(p, o) Q_t,c(p + o), Ss_c likewise,
 *   m_c(p) = (wa / na(p)) Sa_c + (ws / ns(p)) Ss_c      (each quotient evaluated once per pixel, 0 where the sum is 0)
 *   Q_{t+1}(p) = softmax_c(U_c(p) - sum_c' mu[c][c'] m_c'(p)),   mu = compat (DEVICE float [C][C]) or, when compat is NULL, -I
 *   (Potts): then Q_{t+1} = softmax(U + m) and no C^2 product is evaluated.
 * Every sum over o runs in the row-major order above in fp32, no atomics: two runs agree bit for bit, and a pixel's result does not
 * depend on where it lies in the launch grid or on the other images of the batch.
 * cvk_crf_step is ONE iteration, called T times on one stream: q_in and q_out are dense float [N][H][W][C], different buffers that
 * swap roles from call to call.
 *   first != 0: the call reads U in place of Q_t and takes the neighbours' softmax as it stages them (no Q_0 pass, no memset); q_in
 *               is scratch then (required all the same: the path that does not stage writes Q_0 there), else q_in = Q_t.
 *   last  != 0: q_out = probs = Q_T and pred (int64 [N][H][W], required then) = the first-maximum channel of exactly the values
 *               stored (a NaN wins, as in cvk_argmax_channels).  first and last together: T = 1.
 * Where the tile of Q and I with its halo r d fits the LDS it is staged there, each thread producing several pixels d apart so that
 * one read of a neighbour's C values feeds several outputs; where it does not, neighbours are read from global memory.  The two
 * paths evaluate the same expressions in the same order.  cvk_crf_tile reports the tile (th x tw pixels per work-group) and which
 * path (staged = 1 / 0) a (C, radius, dilation) takes; CVK_EINVAL outside the limits.
 * Limits: 1 <= C <= 32, ld_u >= C, sizes up to 16384 per side, N * H * W * C < 2^31, wa, ws >= 0 and cb <= 0 finite.  Weights are
 * recomputed from the staged image every iteration: nothing per (pixel, offset) is stored.  At most two launches (one on the staged
 * path), no allocation, no host sync; the calls can be captured. */
int cvk_crf_tile(int C, int radius, int dilation, int* th, int* tw, int* staged);
int cvk_crf_step(const float* unary, int ld_u, int unary_is_prob, const float* q_in, float* q_out, int64_t* pred, const void* guide,
                 int guide_u8, int64_t gN, int64_t gC, int64_t gH, int64_t gW, const float* guide_a, const float* guide_b,
                 const float* ga, const float* gs, float cb, float wa, float ws, const float* compat, int N, int H, int W, int C,
                 int radius, int dilation, int first, int last, void* stream);

/* ---- calibration meter and temperature fit (Guo et al., "On Calibration of Modern Neural Networks", ICML 2017; not in the
 * reference) ----
 * logits: DEVICE float rows [M][ld] with C classes (NHWC), target: DEVICE int64 [M], tau: DEVICE float, the inverse temperature 1 / T
 * (NULL: 1).  For a pixel with logits x and target t, in fp32:
 *   z_c = tau x_c, m = max_c z_c, se = sum_c expf(z_c - m) in class order, pred = the first maximum of x (a NaN wins: exactly
 *   cvk_argmax_channels), conf = 1 / se, the top-label probability (<= 1).
 *   valid iff t != ignore_index and 0 <= t < C; an out-of-range target is counted in the record and otherwise skipped.
 *   bin = clamp((int)ceilf(conf * (float)bins) - 1, 0, bins - 1): right-closed bins (b / bins, (b + 1) / bins].
 *   q = (int64)floor(conf * 2^30): with C <= 128 it carries every bit of conf; sum conf = sum q / 2^30, exact in 64-bit integers.
 *   nll = (m + logf(se)) - z_t;  brier = sum_c (p_c - [c == t])^2, p_c = expf(z_c - m) * conf.
 * cvk_calib_accumulate ADDS the valid pixels of the call to
 *   hist:   DEVICE int64 [C][bins][3], by predicted class and bin: {count, correct (pred == t), sum q}; 64-bit integer atomics;
 *   record: DEVICE 32 bytes {int64 valid, int64 out of range, double sum nll, double sum brier}: the fp64 sums go through `part`
 *           (DEVICE scratch of 4 * cvk_ce_blocks(M) doubles) and a one-workgroup finish in a fixed order; no float atomic: two
 *           calls on the same input give the same bits.
 * conf (DEVICE float [M]) and pred (DEVICE int64 [M]) are optional maps of EVERY pixel, written when non-NULL.  hist, target, part
 * and record go together: all NULL writes the maps only (one of them is required then; `bins` is not read).
 * Limits: 1 <= C <= 128, ld >= C, 1 <= bins <= 64, C * bins <= 2048 (the work-group's table: 48 KiB of LDS).  Two launches (one
 * without tables), no allocation, no host sync.
 *
 * Temperature fit: NLL(tau) = mean over the valid pixels of (lse(tau x) - tau x_t) is convex in tau, with gradient
 * g = mean(E_p[x] - x_t) and curvature h = mean(Var_p[x]), p = softmax(tau x), Var_p[x] = sum_c p_c (x_c - E_p[x])^2.
 * state: DEVICE double[9] = {tau, lo, hi, G, H, L, n, k, -}: the sums of g, h and nll terms, the valid pixels and the row counter;
 * the first 4 bytes of word 8 hold tau as a float, which is what cvk_calib_accumulate's `tau` can point at.  The caller initialises
 * it: {tau0 (a float's value), 1/64, 64, 0, 0, 0, 0, 0} and (float)tau0.
 * cvk_calib_newton_accumulate reads (float)state[0] and ADDS one batch's sums to G, H, L, n; a target that is ignore_index or out of
 * range is skipped (the meter's record counts the latter) (`part` as above; pixel terms in fp32,
 * sums in fp64, fixed order).  cvk_calib_newton_step (one thread, fp64) closes an iteration over any number of batches: with
 * g = G / n, h = H / n: g < 0 sets lo = tau, g > 0 sets hi = tau; the candidate is tau - g / h when h > 1e-12; when it is not
 * strictly inside (lo, hi), or h is too small, it is sqrt(lo * hi); the new tau is the candidate rounded to float once.  n == 0
 * leaves tau alone.  It writes row k of log (DEVICE double [log_rows][8]): {tau used, n, NLL = L / n, g, h, tau next, lo, hi}
 * (no row when k >= log_rows), zeroes the sums and increments k.  final_pass != 0: the row is written with tau next = tau and
 * nothing else changes (the NLL of the fitted tau).  A fit is a chain of these calls on one stream: no host sync, no allocation. */
int cvk_calib_accumulate(const float* logits, int ld, const int64_t* target, const float* tau, int64_t* hist, double* part, void* record,
                         float* conf, int64_t* pred, int M, int C, int bins, int ignore_index, void* stream);
int cvk_calib_newton_accumulate(const float* logits, int ld, const int64_t* target, double* state, double* part, int M, int C,
                                int ignore_index, void* stream);
int cvk_calib_newton_step(double* state, double* log, int log_rows, int final_pass, void* stream);

/* ---- input pipeline on device (transforms.ToTensor + Normalize: transforms.py:485-538, MEAN/STD conf/settings.py:8-9) ----
 * src uint8 [N,H,W,3] (channel order as decoded, i.e. cv2 BGR) -> dst float32 NHWC with ld = 4 (pad channel 0):
 * dst[c] = (src[c]/255 - mean3[c]) / std3[c].  mean3 / std3 are HOST pointers to 3 floats. */
int cvk_preprocess_u8(const uint8_t* src, float* dst, int N, int H, int W, const float* mean3, const float* std3, void* stream);

/* ---- training / validation transforms on device (transforms.py Resize -> RandomGaussianBlur -> RandomHorizontalFlip ->
 * ColorJitter -> ToTensor -> Normalize, composed in train.py:61-75), one launch per batch.
 * frames uint8 [N,Hs,Ws,3] (cv2 BGR), masks [N,Hs,Ws] of mask_bytes = 1 (uint8) or 8 (int64) per value -> out float32 NHWC
 * ld = 4 [N,H,W,4] (cvk_preprocess_u8's expression and layout), out_masks int64 [N,H,W], out_u8 (nullable) uint8 [N,H,W,3]: the
 * augmented frame before normalisation.  Per sample, in order: bilinear resize (cv2 INTER_LINEAR mapping (d + 0.5) * in / out
 * - 0.5, clamped at the edges, rounded half-up), separable Gaussian of ksize taps (fp32, REFLECT_101 in resized coordinates,
 * rounded half-up), the 256-entry LUT, the horizontal flip; masks: nearest resize (source floor(d * in / out)) and the flip.
 * records: DEVICE array of N cvk_augment_record; ksize outside {3,5,7,9} means no blur.  mean3 / std3 are HOST pointers to 3
 * floats.  No allocation and no synchronisation: the call can be captured in a graph. */
typedef struct cvk_augment_record {
    int32_t flip;                /* != 0: mirror left-right */
    int32_t ksize;               /* Gaussian taps: 3, 5, 7 or 9; anything else: no blur */
    int32_t use_lut;             /* != 0: apply lut (else it is the identity and is not read) */
    int32_t reserved;
    float   taps[12];            /* taps[0 .. ksize-1] */
    uint8_t lut[256];
} cvk_augment_record;
int cvk_augment_record_bytes(void);
int cvk_augment_u8(const uint8_t* frames, const void* masks, int mask_bytes, int N, int Hs, int Ws, int H, int W,
                   const cvk_augment_record* records, const float* mean3, const float* std3, float* out, int64_t* out_masks,
                   uint8_t* out_u8, void* stream);

/* ---- crop training on device: random rescale, class-balanced crop, pad, blur, LUT, flip (mmseg's RandomResize + RandomCrop +
 * Pad; the reference's own RandomScale, transforms.py:63-127, is the one-candidate case with negative offsets) --------------
 * Per sample n the frame is rescaled to a VIRTUAL Hr x Wr image that never reaches memory: cv2 INTER_LINEAR as in cvk_augment_u8
 * (f = (d + 0.5) * s - 0.5 in double, clamped at both edges, fp32 blend, rounded half-up) and INTER_NEAREST for the mask
 * (min(floor(d * s), n - 1) in double), with the steps s = sy, sx of the record (source pixels per resized pixel; Hs / Hr for a
 * cv2 dsize, 1 / fx for a cv2 factor).  Then the optional Gaussian of ksize taps (REFLECT_101 at the borders of the RESIZED image)
 * and the optional LUT, both as in cvk_augment_u8.  Pixel (y, x) of the hc x wc output shows resized pixel (y + offy, x + offx);
 * offsets are signed and whatever falls outside the resized image is pad: mask pad_label, uint8 0, float 0.0 in all four channels
 * (pad_normalized == 0) or black normalised, (0 - mean) / std (pad_normalized != 0).  flip mirrors the whole wc-wide canvas, pad
 * included.
 * A record carries ncand (1..11; clamped to that range) candidate offsets.  cvk_crop_select counts, per candidate, the resized
 * labels inside (window ∩ resized image) per value; labels equal to ignore_index or outside [0, 256) are not counted.  Candidates
 * 0 .. ncand - 2 are tested in order; one passes iff more than one value has a non-zero count and
 * (double)max_count / (double)sum_count < cat_max_ratio; the first that passes is chosen, else candidate ncand - 1 (mmseg's
 * RandomCrop loop).  counts: DEVICE uint32 [N][11][256], cleared by the call, then the counts of candidates 0 .. ncand - 1;
 * selection: DEVICE int32 [N][4] = {candidate, offy, offx, passed}.  Integer atomics only: both tables are exact.  Three launches.
 * cvk_crop_augment_u8 reads the selection rows on the device and writes out float32 [N,hc,wc,4] (cvk_preprocess_u8's expression,
 * fourth channel 0), out_masks int64 [N,hc,wc] and out_u8 (nullable) uint8 [N,hc,wc,3].  One launch.  mean3 / std3 are HOST
 * pointers.  Neither call allocates or synchronises.  hc * wc < 2^31.
 * sizeof(cvk_crop_record) == 416 (cvk_crop_record_bytes()): every field sits at a multiple of its own size, no implicit padding. */
typedef struct cvk_crop_record {
    double  sy, sx;              /*   0: source pixels per resized pixel */
    int32_t Hr, Wr;              /*  16: size of the resized image, each >= 1 */
    int32_t ncand;               /*  24: candidates in use, 1..11; the last one is the unconditional fallback */
    int32_t offy[11];            /*  28 */
    int32_t offx[11];            /*  72 */
    float   taps[9];             /* 116: taps[0 .. ksize-1] */
    uint8_t flip;                /* 152: != 0: mirror left-right */
    uint8_t use_lut;             /* 153: != 0: apply lut */
    uint8_t ksize;               /* 154: 3, 5, 7 or 9; anything else: no blur */
    uint8_t reserved[5];         /* 155 */
    uint8_t lut[256];            /* 160 */
} cvk_crop_record;
int cvk_crop_record_bytes(void);
int cvk_crop_select(const void* masks, int mask_bytes, int N, int Hs, int Ws, int hc, int wc, const cvk_crop_record* records,
                    int ignore_index, double cat_max_ratio, uint32_t* counts, int32_t* selection, void* stream);
int cvk_crop_augment_u8(const uint8_t* frames, const void* masks, int mask_bytes, int N, int Hs, int Ws, int hc, int wc,
                        const cvk_crop_record* records, const int32_t* selection, const float* mean3, const float* std3,
                        int64_t pad_label, int pad_normalized, float* out, int64_t* out_masks, uint8_t* out_u8, void* stream);

/* ---- fused AdamW over a flat fp32 buffer (torch.optim.AdamW: train.py:100,133) -------------------------------- */
int cvk_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* stream);

/* One hyper-parameter record: a group's lr / betas / eps / weight decay and the bias corrections of one step count.
 * cvk_adamw_hyper_fill (host function, no launch) fills one; bc1 = 1 - beta1^step and bc2_sqrt = sqrt(1 - beta2^step) come from the
 * same host expressions cvk_adamw_step evaluates. */
typedef struct cvk_adamw_hyper {
    float lr, beta1, beta2, eps, weight_decay;
    float bc1;                   /* 1 - beta1^step */
    float bc2_sqrt;              /* sqrt(1 - beta2^step) */
} cvk_adamw_hyper;
int cvk_adamw_hyper_fill(float lr, float beta1, float beta2, float eps, float weight_decay, int step, cvk_adamw_hyper* out);

/* AdamW over a RANGE TABLE of the flat buffers (fine-tuning: frozen parameters, parameter groups, a step count per parameter), with
 * optional global-norm clipping and an optional moving average of the weights, in one launch.
 *   ranges (DEVICE, nranges entries): the trainable ranges [offset, offset + length) of param / grad / exp_avg / exp_avg_sq (and ema),
 *     each with the index of the cvk_adamw_hyper record that updates it.  Elements outside every range (frozen parameters and their
 *     moments) are neither read nor written, in any buffer.  cvk_adamw_plan_ranges (host function, no launch) checks a HOST copy of the
 *     table against the buffer length n and the record count, fills every block0 (the range's first workgroup) and returns the workgroup
 *     count the launches take as nblocks, or a negative error.  The table uploaded to the device must be the planned one.
 *   The element update is cvk_adamw_step's, in the same operation order: one range over the whole buffer with one record, record and
 *     ema null, is bitwise cvk_adamw_step.
 *   record (DEVICE, may be null): the {total_norm, clip_coef} record of cvk_grad_norm.  Every gradient element is multiplied by record[1]
 *     on its way into the update (one more operand of the same expression list); the gradient buffer is not rewritten.  Null means
 *     coefficient 1.0f, and a step with a coefficient of 1.0f is bitwise the step with a null record.
 *   ema (DEVICE, may be null): one more fp32 buffer laid out like param.  The thread that has stored the new value p_new of an element
 *     goes on with it in the register: ema[i] += alpha * (p_new - ema[i]); param is not read again.  param, exp_avg and exp_avg_sq come
 *     out bitwise as with ema null.  0 < alpha <= 1 (alpha = 1 - decay).  With ema null no average is kept and alpha is ignored.
 * cvk_adamw_step_ranges (eager): hyper is a HOST array of nhyper <= CVK_ADAMW_ARG_RECORDS records; they and alpha travel as kernel
 *   arguments.
 * cvk_adamw_step_ranges_dev (captured graphs, GraphedStep(optimizer=...)): hyper (nhyper records) and alpha (one float) are in DEVICE
 *   memory, rewritten by the host between graph replays, so a replay picks up the scheduler's lr / beta1 and the update's alpha.
 *   alpha_host is the value the host uploads there next (at a capture: the first one) and is only checked, since the device value
 *   cannot be.  With ema null, alpha may be null and alpha_host is ignored. */
#define CVK_ADAMW_ARG_RECORDS 16
typedef struct cvk_adamw_range {
    int64_t offset;              /* first element of the range in the flat buffers */
    int64_t length;              /* elements, > 0 */
    int32_t hyper;               /* index of the cvk_adamw_hyper record */
    int32_t block0;              /* first workgroup of the range (cvk_adamw_plan_ranges) */
} cvk_adamw_range;
int cvk_adamw_plan_ranges(cvk_adamw_range* ranges, int nranges, int64_t n, int nhyper);
int cvk_adamw_step_ranges(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                          const cvk_adamw_range* ranges, int nranges, int nblocks, const cvk_adamw_hyper* hyper, int nhyper,
                          const float* record, float alpha, void* stream);
int cvk_adamw_step_ranges_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                              const cvk_adamw_range* ranges, int nranges, int nblocks, const cvk_adamw_hyper* hyper, int nhyper,
                              const float* record, const float* alpha, float alpha_host, void* stream);

/* ---- fused momentum SGD over the same range table (torch.optim.SGD) -------------------------------------------------------------
 * The second update rule of the flat optimizer.  Everything around the element update is cvk_adamw_step_ranges': the DEVICE range table
 * planned by cvk_adamw_plan_ranges (cvk_adamw_range; `hyper` indexes the cvk_sgd_hyper records here), the workgroup-to-range search,
 * the {total_norm, clip_coef} record (null: coefficient 1.0f), the ema buffer with ema[i] += alpha * (p_new - ema[i]) from the register,
 * the two record sources.  Elements outside every range are never touched, in any buffer.  The update, in fp32, one expression list for
 * both entry points (they cannot round differently):
 *     d = grad[i] * clip_coef;  d = d + weight_decay * param[i]                      (coupled L2, as torch; not decoupled)
 *     if momentum != 0:  b = first ? d : momentum * buf[i] + (1 - dampening) * d;  buf[i] = b;  d = nesterov ? d + momentum * b : b
 *     param[i] = param[i] - lr * d
 * `first` is torch's `momentum_buffer is None`: on a parameter's first step with a non-zero momentum the buffer becomes d itself.
 *
 * cvk_sgd_hyper: 7 floats, the size of cvk_adamw_hyper, so the records travel in the same slots (kernel arguments or the device ring of
 *   GraphedStep) and cvk_step_log, which reads floats 0 and 1 of its record, works unchanged: lr is float 0 and momentum float 1 (log
 *   column 2 carries the momentum where it carries beta1 for AdamW).  nesterov and first are 0.0f or 1.0f; reserved is 0.
 * cvk_sgd_hyper_fill (host function, no launch) fills one.  Refused: a negative or NaN lr, momentum or weight_decay; nesterov with
 *   momentum <= 0 or dampening != 0.
 * cvk_sgd_step_ranges (eager): hyper is a HOST array of nhyper <= CVK_ADAMW_ARG_RECORDS records; they and alpha travel as kernel
 *   arguments.  momentum_buf (DEVICE, laid out like param) may be null only if every record's momentum is 0 (checked on the host); with
 *   a null buffer the kernel neither reads nor writes one: 3 passes over the ranges instead of 5.  With a buffer, the ranges of a record
 *   whose momentum is 0 are still left alone in it.
 * cvk_sgd_step_ranges_dev (captured graphs): hyper and alpha in DEVICE memory, alpha_host only checked, as for
 *   cvk_adamw_step_ranges_dev.  The device records cannot be checked: a null momentum_buf runs the buffer-free kernel whatever they carry.
 * Both check their arguments like cvk_adamw_step_ranges[_dev] (null pointers, alpha outside (0, 1] with an ema, the record limit of the
 * argument form, an empty table) before any launch. */
typedef struct cvk_sgd_hyper {
    float lr, momentum, dampening, weight_decay;
    float nesterov;              /* 0 or 1 */
    float first;                 /* 0 or 1: the ranges of this record have no momentum buffer yet */
    float reserved;              /* 0 */
} cvk_sgd_hyper;
int cvk_sgd_hyper_fill(float lr, float momentum, float dampening, float weight_decay, int nesterov, int first, cvk_sgd_hyper* out);
int cvk_sgd_step_ranges(float* param, const float* grad, float* momentum_buf, float* ema, int64_t n,
                        const cvk_adamw_range* ranges, int nranges, int nblocks, const cvk_sgd_hyper* hyper, int nhyper,
                        const float* record, float alpha, void* stream);
int cvk_sgd_step_ranges_dev(float* param, const float* grad, float* momentum_buf, float* ema, int64_t n,
                            const cvk_adamw_range* ranges, int nranges, int nblocks, const cvk_sgd_hyper* hyper, int nhyper,
                            const float* record, const float* alpha, float alpha_host, void* stream);

/* ---- the per-iteration training log (train.py:133-143 print of loss / lr / Beta1; utils.visulaize_lastlayer utils.py:33-36) -------
 * One single-workgroup launch appends the row [loss, lr, beta1, ||gw||_2, ||gb||_2] (fp32) to a DEVICE ring of `capacity` rows at row
 * counter % capacity, then increments *counter (DEVICE int64).  loss: DEVICE scalar; hyper: DEVICE record (lr and beta1 of the step);
 * gw / gb: DEVICE gradients of nw / nb floats.  record (DEVICE, may be null): the {total_norm, clip_coef} record of cvk_grad_norm.
 * Null: rows of 5 floats.  Non-null: rows of 7 floats, the five columns, then record[0] and record[1].  The norms are sums of squares
 * in fp64 in a fixed order (no atomics: bitwise reproducible), rounded to fp32 after the square root.  No allocation and no
 * synchronisation: the call can be captured in a graph. */
int cvk_step_log(const float* loss, const cvk_adamw_hyper* hyper, const float* gw, int nw, const float* gb, int nb, const float* record,
                 float* ring, int capacity, int64_t* counter, void* stream);

/* ---- global-norm gradient clipping (torch.nn.utils.clip_grad_norm_) fused into the AdamW step ------------------------------------
 * The norm of the flat gradient buffer over a table of EXACT parameter segments, as a device record {total_norm, clip_coef} that the
 * AdamW launches (cvk_adamw_step_ranges, cvk_adamw_step_ranges_dev), the in-place scale and the log row (cvk_step_log) read.  The
 * flat gradient buffer is uninitialised between its segments (16-byte alignment padding, frozen parameters): the table lists
 * [offset, offset + length) per parameter that has a gradient, neighbours merged only where no padding float lies between them.  No
 * element outside the table is read.
 *
 * cvk_clip_coef (host function): torch's clip coefficient in fp32, max_norm / (total_norm + 1e-6f) clamped to at most 1 the way
 *   torch.clamp(max=1) clamps: a NaN norm gives NaN, an infinite norm gives 0.  The finish kernel evaluates the same expression.
 * cvk_grad_norm_plan (host function, no launch): checks a HOST copy of the table against the buffer length n (every segment inside
 *   [0, n), length > 0), fills every block0 and returns the workgroup count the launches take as nblocks, or a negative error.
 * cvk_grad_norm: two launches.  (1) nblocks workgroups reduce their share of the segments (16-byte loads where the address allows,
 *   every element converted to fp64) into one fp64 partial each: the sum of squares (norm_type 2) or the maximum of |g| (norm_type
 *   INFINITY; a NaN stays a NaN).  (2) one workgroup combines the partials in a fixed order and writes record[0] = total_norm (fp32:
 *   the square root of the fp64 sum, rounded once) and record[1] = cvk_clip_coef(max_norm, total_norm).  No atomics: the record is
 *   bitwise reproducible from run to run, eager or captured.  partials: DEVICE, nblocks doubles.  record: DEVICE, 2 floats.
 *   max_norm >= 0; norm_type 2 or INFINITY, anything else is refused.
 * cvk_grad_scale: grad[i] *= record[1] over the same table, in place (what torch's clip_grad_norm_ leaves in .grad); a coefficient
 *   of exactly 1 leaves the buffer untouched. */
typedef struct cvk_norm_segment {
    int64_t offset;              /* first element of the segment in the flat gradient buffer */
    int64_t length;              /* elements, > 0 */
    int32_t block0;              /* first workgroup of the segment (cvk_grad_norm_plan) */
    int32_t reserved;
} cvk_norm_segment;
float cvk_clip_coef(float max_norm, float total_norm);
int cvk_grad_norm_plan(cvk_norm_segment* segments, int nsegments, int64_t n);
int cvk_grad_norm(const float* grad, int64_t n, const cvk_norm_segment* segments, int nsegments, int nblocks, float norm_type,
                  float max_norm, double* partials, float* record, void* stream);
int cvk_grad_scale(float* grad, int64_t n, const cvk_norm_segment* segments, int nsegments, int nblocks, const float* record,
                   void* stream);

/* ---- gradient accumulation over micro-batches (GradAccumulator) -------------------------------------------------------------------
 * One streaming launch over a planned segment table (cvk_grad_norm_plan: the same table type and the same workgroup walk as the norm)
 * that folds one flat gradient buffer into another.  dst and src are two DEVICE buffers of n floats with the same layout; the table's
 * offsets apply to both.  Elements outside the table (alignment padding, frozen parameters) are neither read nor written.
 *   mode 0: dst = src                    (first micro-step of a window: initialises the accumulator, which never needs zeroing)
 *   mode 1: dst = dst + src              (middle micro-steps)
 *   mode 2: dst = (dst + src) * scale    (closing micro-step: dst is the fresh gradient buffer of the pass, src the accumulator)
 * Every element is one correctly rounded fp32 add and, in mode 2, one separately rounded fp32 multiply, in that order; no atomics:
 * the result is bitwise the same expression evaluated in IEEE fp32, run to run, eager or captured.  16-byte loads and stores in the
 * body of a segment, scalar heads and tails.  A table over a sub-range of the buffer (one data-parallel bucket) is planned like any
 * other table.  scale must be finite, both bases 16-byte aligned, dst != src; mode outside 0..2 is refused. */
int cvk_grad_accumulate(float* dst, const float* src, int64_t n, const cvk_norm_segment* segments, int nsegments, int nblocks,
                        int mode, float scale, void* stream);


/* ================================================================================================================
 * bf16-storage path (BASELINE.json configs[3] "bf16 + MFMA im2col path"; set_conv_precision(net, "bf16")).
 * Activations and activation gradients are bf16 NHWC in HBM, products bf16 x bf16 on the matrix cores with fp32
 * accumulation, BatchNorm statistics / parameter gradients / master weights fp32.  Same reference call sites as the
 * fp32 entry points above (models/unet.py:11-13,25,92; train.py:131).
 * ================================================================================================================ */

/* rows the packed weight tensors are padded to (multiple of the kernel's output-channel tile), and the number of
 * BatchNorm-statistics partials cvk_conv3x3_bf16s writes for a layer (one per 8 x 32 pixel tile, or one per strip of
 * tiles for the <= 64 x 64 channel layers); cvk_bf16s_stat_partials is the upper bound over all layers */
int cvk_bf16s_rows_pad(int cout);
int cvk_bf16s_stat_partials(int N, int H, int W);
int cvk_bf16s_stat_partials_c(int N, int H, int W, int Cin, int Cout);
/* fp32 master weights [Cout][3][3][Cin] -> bf16 [rows_pad(Cout)][9][Cin_pad] (forward), and the rotated/transposed
 * data-grad filter bf16 [rows_pad(Cin)][9][Cout_pad]; zero padded */
int cvk_pack_weight_fwd_bf16(const float* w, void* out, int Cout, int Cin, int Cin_pad, void* stream);
int cvk_pack_weight_dgrad_bf16(const float* w, void* out, int Cout, int Cin, int Cout_pad, void* stream);
/* n (<= CVK_PACK_BATCH_MAX) such packs in ONE launch: job i = cvk_pack_weight_fwd_bf16(w, out, Cout, Cin, Kpad) (dgrad = 0) or
 * cvk_pack_weight_dgrad_bf16(w, out, Cout, Cin, Kpad) (dgrad = 1); `jobs` is a HOST array (copied into the kernel arguments).
 * The executor packs every layer of a step up front when the weights have changed (models/unet.py:35-92: 23 conv layers). */
#define CVK_PACK_BATCH_MAX 48
typedef struct cvk_pack_job { const float* w; void* out; int Cout, Cin, Kpad, dgrad; } cvk_pack_job;
int cvk_pack_weights_bf16_batch(const cvk_pack_job* jobs, int n, void* stream);
/* y[N,H,W,ldy] (bf16) = conv3x3(x[N,H,W,Cin] bf16, w bf16 [rows_pad][9][Cin]) + bias; Cin % 32 == 0.  With stats != NULL:
 * stats[2][P][Cout] = per-tile (sum, M2 about the tile mean) of the fp32 results, counts[P] = pixels per tile,
 * P = cvk_bf16s_stat_partials_c(N,H,W,Cin,Cout) -> cvk_bn_finalize_counts.  Data-grad: the same call on dy and the dgrad pack. */
int cvk_conv3x3_bf16s(const void* x, const void* w, const float* bias, void* y, float* stats, float* counts,
                      int N, int H, int W, int Cin, int Cout, int ldy, void* stream);
/* the same with a cap on the workgroups of the persistent kernels (layers with >= 64 input and > 32 output channels run one
 * workgroup per CU that walks the tiles): under data-parallel training the executor leaves CVK_DP_RESERVE_CUS CUs to the RCCL
 * all-reduce kernels that run beside backward (legacy/train_tpu.py:115 hides the same exchange).  0 = every CU.  Results are
 * bitwise independent of the cap. */
int cvk_conv3x3_bf16s_wg(const void* x, const void* w, const float* bias, void* y, float* stats, float* counts,
                      int N, int H, int W, int Cin, int Cout, int ldy, int max_workgroups, void* stream);
/* The THIN layers of the bf16-storage mode on their own kernels (csrc/thin_bf16.hip: register-only, no LDS; round 5): the stem 3 -> 64
 * and the classifier head 64 -> class_num forward (models/unet.py:103,127) and the head's data-grad.  cvk_thin_bf16_mode(Cin, Cout of the
 * FORWARD layer, pitch of the kernel's input / output tensor, dgrad): 0 not thin, 1 head forward, 2 stem forward, 3 head data-grad.
 * cvk_pack_weight_thin_bf16: the forward layer's fp32 weights [Cout][3][3][Cin] -> the mode's filter pack (cvk_thin_bf16_pack_elems bf16).
 * cvk_conv3x3_thin_bf16: y bf16 [N,H,W,ld_out] = conv3x3(x bf16 [N,H,W,ld_in], pack) + bias; with stats != NULL statistics partials
 * stats[2][P][C] + counts[P], P = cvk_thin_bf16_stat_partials(N,H,W), C = Cout (mode 1) or 64 -> cvk_bn_finalize_counts. */
int cvk_thin_bf16_mode(int Cin, int Cout, int ld_in, int ld_out, int dgrad);
int cvk_thin_bf16_stat_partials(int N, int H, int W);
size_t cvk_thin_bf16_pack_elems(int mode);
int cvk_pack_weight_thin_bf16(const float* w, void* out, int Cout, int Cin, int mode, void* stream);
int cvk_conv3x3_thin_bf16(const void* x, const void* wpack, const float* bias, void* y, float* stats, float* counts, int N, int H, int W,
                          int ld_in, int Cout, int ld_out, int mode, void* stream);
/* which kernel the two calls above run for a layer geometry (a query of their dispatch, no launch; measurement tools label their
 * timings with the name a kernel trace shows): 0 k_conv_bf16s (tile kernel), 1 k_conv_bf16q, 2 k_conv_bf16h, 3 k_conv_bf16h on the
 * 128-row weight pack, 4 k_conv_bf16s_strip, 5 two k_conv_bf16s_strip passes (64 -> 128 channels without statistics); < 0: bad shape */
int cvk_conv3x3_bf16s_kernel(int N, int H, int W, int Cin, int Cout, int with_stats);
int cvk_bn_finalize_counts(const float* stats, const float* counts, int P, int M, int C, const float* gamma, const float* beta,
                           float* mean, float* rstd, float* scale, float* shift, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, float momentum, float eps, void* workspace, size_t workspace_bytes,
                           void* stream);
/* dw fp32 [Cout][9][Cin] = sum_pixels dy (x) x_shifted; x bf16 [N,H,W,ldx], dy bf16 [N,H,W,ld_dy] (ld % 8 == 0) */
size_t cvk_conv3x3_wgrad_bf16s_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int cvk_conv3x3_wgrad_bf16s(const void* x, const void* dy, float* dw, int N, int H, int W, int Cin, int ldx, int Cout,
                            int ld_dy, void* workspace, size_t workspace_bytes, void* stream);
/* The same in two steps, so that a backward pass can sum the partial results of ALL its layers in one launch at its end (the weight
 * gradients are read by nobody before the optimizer step / the all-reduce of their bucket: loss.backward() of train.py:131).
 * _slabs: the partial sums only — S = cvk_conv3x3_wgrad_bf16s_splits(...) slabs of Cout*9*Cin floats at `slabs`
 * (cvk_conv3x3_wgrad_bf16s_workspace_bytes of room); with S == 1 the one slab IS dw and may be written in place.
 * _reduce_batch: dw = slab 0 + slab 1 + ... (the order cvk_conv3x3_wgrad_bf16s uses: bitwise the same) for n <= CVK_WREDUCE_BATCH_MAX
 * layers; `jobs` is a HOST array (copied into the kernel arguments). */
int cvk_conv3x3_wgrad_bf16s_splits(int N, int H, int W, int Cin, int Cout);
int cvk_conv3x3_wgrad_bf16s_slabs(const void* x, const void* dy, float* slabs, int N, int H, int W, int Cin, int ldx, int Cout,
                                  int ld_dy, size_t slab_bytes, void* stream);
#define CVK_WREDUCE_BATCH_MAX 48
typedef struct cvk_wreduce_job { const float* slabs; float* dw; unsigned long long n; int splits, pad; } cvk_wreduce_job;
int cvk_wgrad_reduce_bf16s_batch(const cvk_wreduce_job* jobs, int n, void* stream);
/* logical NCHW fp32 (any strides) -> dense bf16 NHWC with ld % 8 == 0, pad channels zero */
int cvk_import_nchw_bf16(const float* src, int64_t sN, int64_t sC, int64_t sH, int64_t sW, void* dst, int ld,
                         int N, int C, int H, int W, void* stream);
/* out = relu(y*scale + shift): y bf16 [M][ldy]; out a view of bf16 (out_f32 = 0) or fp32 (out_f32 = 1, the logits);
 * pool != NULL: also writes MaxPool2d(2,2)(out) as dense bf16 [N,H/2,W/2,C] (models/unet.py:92 fused into this pass) */
int cvk_bn_relu_apply_bf16(const void* y, int ldy, const float* scale, const float* shift, cvk_viewh out, int out_f32,
                           void* pool, int N, int H, int W, int C, void* stream);
/* BatchNorm+ReLU backward on bf16 tensors; dout is a bf16 view, or fp32 (dout_f32 = 1: the loss gradient).
 * part: 2 * cvk_bn_bwd_blocks_bf16(M) * C floats (reduce) / cvk_bn_bwd_blocks_bf16(M) * C floats (dx: column sums of the
 * fp32 dy BEFORE its rounding to bf16, the conv bias gradient; NULL: dy only) -> cvk_colsum_finalize.  dy rows have pitch
 * ld_dy >= C, pad columns are written as 0. */
int cvk_bn_bwd_blocks_bf16(int M);
int cvk_bn_bwd_reduce_bf16(cvk_viewh dout, int dout_f32, const void* y, int ldy, const float* scale, const float* shift,
                           const float* mean, const float* rstd, float* part, int N, int H, int W, int C, void* stream);
int cvk_bn_bwd_dx_bf16(cvk_viewh dout, int dout_f32, const void* y, int ldy, const float* scale, const float* shift,
                       const float* mean, const float* rstd, const float* dgamma, const float* dbeta, void* dy, int ld_dy,
                       float* dbias_part, int N, int H, int W, int C, int use_batch_stats, void* stream);
/* MaxPool2d(2,2) backward: dout dense bf16 [N,H/2,W/2,C]; x = the pooled layer's stored input (view); dx (view) is
 * written, or added to when accumulate != 0 */
int cvk_maxpool2x2_bwd_bf16(const void* dout, cvk_viewh x, cvk_viewh dx, int accumulate, int N, int H, int W, int C, void* stream);
/* cvk_maxpool2x2_bwd_bf16 that also leaves the partial sums of the producing block's BatchNorm+ReLU backward (reference models/unet.py:12-13 under
 * nn.MaxPool2d(2,2), unet.py:92; the bf16 twin of cvk_maxpool2x2_bwd_bnred): when the pool directly follows a conv block this pass is the last writer of
 * the block's output gradient, and it sums g = dx * [ReLU passed] and g * xhat over the STORED (bf16) values on the way — part = float[2]
 * [cvk_maxpool2x2_bwd_bnred_blocks_bf16(N,H,W,C)][C] for cvk_colsum_finalize; yP [N*H*W][ldp] bf16 = the block's conv output, scale / shift / mean /
 * rstd its BatchNorm constants (contract of cvk_bn_bwd_reduce_bf16).  C % 8 == 0 and C/8 must divide 256 (blocks() returns 0 otherwise). */
int cvk_maxpool2x2_bwd_bnred_blocks_bf16(int N, int H, int W, int C);
int cvk_maxpool2x2_bwd_bnred_bf16(const void* dout, cvk_viewh x, cvk_viewh dx, int accumulate, int N, int H, int W, int C, const void* yP, int ldp,
                                  const float* scale, const float* shift, const float* mean, const float* rstd, float* part, void* stream);
/* MaxUnpool2d(2) of bf16 plans (reference models/segnet.py:80,104-116: self.unpool(x, idx, output_size)).  No index tensor is kept:
 * the arg-max of every 2x2 cell is recomputed from x, the stored input of the pooling layer ([N,H,W,C] view; first maximum in scan
 * order, NaN wins — ATen's rule, as cvk_maxpool2x2_bwd_bf16).  FORWARD is cvk_maxpool2x2_bwd_bf16(v, x, out, 0, ...): the pooled
 * values v [N,H/2,W/2,C] scattered to their arg-max pixels, every other pixel 0.  BACKWARD (this entry) gathers:
 * dv[n,yc,xc,c] = dout[n, arg-max pixel of cell (yc,xc), c]; dout dense [N,H,W,C], dv dense [N,H/2,W/2,C].  C % 8 == 0. */
int cvk_maxunpool2x2_bwd_bf16(const void* dout, cvk_viewh x, void* dv, int N, int H, int W, int C, void* stream);
int cvk_bilinear_up2_fwd_bf16(const void* x, void* out, int N, int H, int W, int C, void* stream);
int cvk_bilinear_up2_bwd_bf16(const void* dout, void* dx, int N, int H, int W, int C, void* stream);
int cvk_zero_frame_bf16(cvk_viewh buf, int N, int H, int W, int C, int y0, int x0, int h, int w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CVK_H */
