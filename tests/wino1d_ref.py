"""fp64 references, integer restatements of the host planners, fp32 restatements of the transform chains and the case tables for the
1-D Winograd conv kernels: csrc/wino.hip (F(2,3), `fam` 2) and csrc/wino4.hip (per-index F(4,3), `fam` 4).  They replace
nn.Conv2d(cin, cout, 3, padding=1) (forward with the BatchNorm batch statistics, data-grad and weight-grad).  No GPU and no library:
tests/test_wino1d_ref_cpu.py checks this file against torch.nn.functional, tests/test_gpu_wino1d.py checks the kernels against it.

Layouts are the C ABI's (include/cvk.h): activations NHWC, filters [Cout][3][3][Cin]."""
import math

import numpy as np
import torch
import torch.nn.functional as F

STAT_ROWS = 64      # CVK_STAT_ROWS
BK = 32             # csrc/conv_tile.h: K slice per LDS stage
GUARD = 4096        # floats behind every device buffer of the GPU tests


def cdiv(a, b):
    return -(-a // b)


def group(fam):
    """Output columns per transform group: F(2,3) pairs, F(4,3) groups of four."""
    return 2 if fam == 2 else 4


def nplanes(fam):
    return 4 if fam == 2 else 6


# ------------------------------------------------------------------------------------------------------------ fp64 references
def conv_fwd_ref(x, w, b=None):
    """y = conv2d(x, w, b, padding=1).  x [N][H][W][Cin], w [Cout][3][3][Cin], y [N][H][W][Cout], double."""
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), None if b is None else b.double(), padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


def conv_fwd_ref_rows(x, w, b, rows):
    """The rows `rows` (global image-row indices n*H + y) of conv_fwd_ref, each from its three-row input band: [len(rows)][W][Cout]."""
    N, H, W, Cin = x.shape
    wd = w.double().permute(0, 3, 1, 2)
    out = []
    for g in rows:
        n, y = divmod(g, H)
        band = torch.zeros(1, Cin, 3, W, dtype=torch.float64)
        for r in range(3):
            if 0 <= y + r - 1 < H:
                band[0, :, r] = x[n, y + r - 1].double().t()
        out.append(F.conv2d(band, wd, None if b is None else b.double(), padding=(0, 1))[0, :, 0].t())
    return torch.stack(out)


def conv_dgrad_ref(dy, w):
    """dx = conv_transpose2d(dy, w, padding=1).  dy [N][H][W][Cout], w [Cout][3][3][Cin], dx [N][H][W][Cin], double."""
    dx = F.conv_transpose2d(dy.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), padding=1)
    return dx.permute(0, 2, 3, 1).contiguous()


def conv_wgrad_ref(x, dy):
    """dW [Cout][3][3][Cin] of sum(conv2d(x, W, padding=1) * dy) by autograd in double."""
    Cin, Cout = x.shape[3], dy.shape[3]
    wz = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().permute(0, 3, 1, 2), wz, padding=1).backward(dy.double().permute(0, 3, 1, 2))
    return wz.grad.permute(0, 2, 3, 1).contiguous()


def stat_partials_ref(y):
    """cvk_conv3x3_fwd's statistics contract: float[2][P][C], P = ceil(N*H*W/64); per granule of 64 consecutive pixels the sum of y and
    the sum of squared deviations from that granule's own mean.  Also returns the pixel count of every granule."""
    C = y.shape[-1]
    flat = y.double().reshape(-1, C)
    M = flat.shape[0]
    P = cdiv(M, STAT_ROWS)
    out = torch.zeros(2, P, C, dtype=torch.float64)
    cnt = torch.zeros(P, dtype=torch.float64)
    for p in range(P):
        g = flat[p * STAT_ROWS:(p + 1) * STAT_ROWS]
        out[0, p] = g.sum(0)
        out[1, p] = ((g - g.mean(0)) ** 2).sum(0)
        cnt[p] = g.shape[0]
    return out, cnt


def chan_combine(sums, m2, cnt):
    """Mean and biased variance per channel from per-granule (sum, M2, count) by Chan's parallel formula, double."""
    sums, m2, cnt = sums.double(), m2.double(), cnt.double()
    M = cnt.sum()
    mean = sums.sum(0) / M
    var = (m2.sum(0) + (cnt[:, None] * (sums / cnt[:, None] - mean) ** 2).sum(0)) / M
    return mean, var


E_COEF = ((1., 1., 1., 1.), (1., -1., 1., -1.), (1., 2., 4., 8.), (1., -2., 4., -8.))   # rows 1..4 of A: E1..E4 of csrc/wino4.hip


def e_planes_ref(dy, ld):
    """The formula above k_wino4_dy_transform: E1..E4 = A dy over columns 4t..4t+3 (zero beyond the right edge), float[4][N*H*ceil(W/4)][ld]
    from dy [N][H][W][ld], double.  Also returns sum |coefficient * dy| per element (what the fp32 rounding of one plane scales with)."""
    N, H, W, C = dy.shape
    assert C == ld
    Wt = cdiv(W, 4)
    d = torch.zeros(N, H, 4 * Wt, ld, dtype=torch.float64)
    d[:, :, :W] = dy.double()
    d = d.reshape(N * H * Wt, 4, ld)
    A = torch.tensor(E_COEF, dtype=torch.float64)
    return torch.einsum("xi,tic->xtc", A, d), torch.einsum("xi,tic->xtc", A.abs(), d.abs())


def dgrad_filter(w):
    """The filter whose forward conv is the data-grad of w [Cout][3][3][Cin]: wd[ci][r][s][co] = w[co][2-r][2-s][ci]
    (cvk_pack_weight_dgrad without padding)."""
    return w.flip(1, 2).permute(3, 1, 2, 0).contiguous()


# --------------------------------------------------------------------------------------- integer restatements of the host planners
def plan_fwd(fam, N, H, W, Cin, ldm):
    """cvk_conv3x3_wino_gemm (full_tiles rule) / plan_wino4 of cvk_conv3x3_wino4_gemm.  bn: column tile of the instantiation; nfull: tiles
    whose block walks every transform index, the other tiles - nfull are cut into single-index blocks, each split `ksplit` ways in K."""
    Wt = cdiv(W, group(fam))
    Mt = N * H * Wt
    bn = 128 if ldm > 64 else (64 if ldm > 32 else 32)
    ksplit = 1
    if fam == 2:
        tilesN = cdiv(ldm, 128) if ldm > 64 else (cdiv(ldm, 64) if ldm > 32 else 1)
        tiles = cdiv(Mt, 128) * tilesN
        nfull = 0 if (tiles < 1024 and Cin >= 256) else tiles // 256 * 256
    else:
        tilesN = cdiv(ldm, 128) if ldm > 64 else 1
        tiles = cdiv(Mt, 128) * tilesN
        nfull = tiles // 256 * 256
        if (tiles < 1024 and Cin >= 256) or (ldm <= 64 and Cin >= 128):
            nfull = 0
        blocks = tiles * 6
        if nfull == 0 and blocks < 2048 and Cin >= 256:
            nK = 3 * Cin // BK
            best = blocks / (512.0 * cdiv(blocks, 512))
            for f in (2, 3):
                if nK % (2 * f):
                    continue
                fill = (blocks * f) / (512.0 * cdiv(blocks * f, 512))
                if fill > best + 0.08:
                    best, ksplit = fill, f
    return dict(Wt=Wt, Mt=Mt, bn=bn, tilesN=tilesN, tiles=tiles, nfull=nfull, ksplit=ksplit,
                grid=nfull + nplanes(fam) * ksplit * (tiles - nfull))


def output_chunk(fam, N, H, W, ldy):
    """Channels per block of the output pass: cvk_wino_output always 1024, cvk_wino4_output 1024 / 256 / 64 so that the grid covers the chip."""
    if fam == 2:
        return 1024
    P = cdiv(N * H * W, STAT_ROWS)
    chunk = 1024
    while chunk > 64 and P * cdiv(ldy, chunk) < 1024:
        chunk //= 4
    return chunk


def plan_wgrad(fam, N, H, W, Cin_pad, Cout):
    """plan_wgrad_wino / plan_wgrad_wino4 (the two differ in the tile width and in the 4 / 6 transform indices per tile)."""
    NH, Wt = N * H, cdiv(W, group(fam))
    bm = 128 if Cout > 64 else 64
    tilesM, tilesN = cdiv(Cout, bm), cdiv(3 * Cin_pad, 128)

    def useful(L):
        return Wt / (cdiv(Wt, L) * L) if Wt >= L else ((L // Wt) * Wt) / L
    L = 30 if useful(30) > useful(32) + 1e-9 else 32
    S = cdiv(Wt, L) if Wt >= L else 1
    R = 1 if Wt >= L else L // Wt
    nslices = NH * S if Wt >= L else cdiv(NH, R)
    units = tilesM * tilesN * nplanes(fam)
    max_splits = max(nslices // 16, 1)
    best, best_eff = 1, -1.0
    s = 1
    while s <= max_splits and s <= 2048:
        blocks = units * s
        if blocks > 4096 and s > 1:
            break
        if not (blocks < 512 and s < max_splits):
            eff = blocks / (256.0 * ((blocks + 255) // 256))
            if eff > best_eff + 0.02:
                best_eff, best = eff, s
        s += 1
    chunk = cdiv(nslices, best)
    return dict(Wt=Wt, bm=bm, tilesM=tilesM, tilesN=tilesN, L=L, S=S, R=R, nslices=nslices, splits=cdiv(nslices, chunk), chunk=chunk)


def wgrad_workspace_floats(fam, N, H, W, Cin_pad, Cout, ld_dy):
    p = plan_wgrad(fam, N, H, W, Cin_pad, Cout)
    slab = p["splits"] * nplanes(fam) * Cout * 3 * Cin_pad
    return slab if fam == 2 else 4 * N * H * p["Wt"] * ld_dy + slab


def arm_of(kind, fam, case):
    """Names the instantiation a case runs.
    kind "fwd",   case (N,H,W,Cin,Cout[,ldm]):                ("fwd", fam, BN, blocks, ksplit, output chunk); blocks is "multi" (every block
        walks all transform indices), "single" (nfull == 0) or "multi+single" (whole rounds of multi-index blocks and a single-index rest).
    kind "wgrad", case (N,H,W,Cin,Cin_pad,Cout,ld_dy):        ("wgrad", fam, BM, MULTIROW, L, "slab" | "split"); "split": more than one slab."""
    if kind == "fwd":
        N, H, W, Cin, Cout = case[:5]
        ldm = case[5] if len(case) > 5 else Cout
        p = plan_fwd(fam, N, H, W, Cin, ldm)
        blocks = "single" if p["nfull"] == 0 else ("multi" if p["nfull"] == p["tiles"] else "multi+single")
        return ("fwd", fam, p["bn"], blocks, p["ksplit"], output_chunk(fam, N, H, W, ldm))
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    p = plan_wgrad(fam, N, H, W, Cin_pad, Cout)
    return ("wgrad", fam, p["bm"], p["R"] > 1, p["L"], "split" if p["splits"] > 1 else "slab")


# -------------------------------------------------------------------------------------------------------------------- case tables
# (N, H, W, Cin, Cout[, ldm]); the comments name what the case is there for (family 4 unless said otherwise)
FWD_CASES = [
    (1, 9, 13, 64, 12, 12),        # BN 32
    (1, 9, 13, 64, 32),            # BN 32
    (1, 20, 33, 128, 64),          # BN 64; family 4: nfull = 0 because ldy <= 64 and Cin >= 128
    (3, 5, 7, 64, 64),             # ragged W mod 4 and mod 2
    (2, 7, 1, 64, 64),             # W = 1
    (1, 1, 9, 64, 128),            # H = 1
    (1, 6, 8, 256, 128),           # ksplit 1, one tile
    (1, 45, 60, 256, 64),          # ksplit 3, BN 64
    (1, 45, 60, 256, 256),         # ksplit 3, BN 128, tilesN 2
    (2, 45, 110, 256, 256),        # 40 tiles, ksplit 2
    (1, 17, 33, 64, 192),          # ragged last column tile
    (1, 17, 33, 64, 40, 44),       # ldm > Cout: columns [Cout, ldm) of y read 0
    (1, 128, 257, 64, 258, 260),   # output chunk 256 (514 granules x 2 channel blocks, the second 4 channels wide); three column tiles
]
# the nfull arm: 258 tiles = 256 multi-index + 2 single-index, output chunk 1024; fp64 on row bands, the rest against cvk_conv3x3_fwd
FWD_BIG_CASES = {4: [(2, 130, 508, 64, 128), (2, 130, 508, 64, 64)], 2: [(2, 130, 254, 64, 128), (2, 130, 254, 64, 64)]}

# (N, H, W, Cin, Cin_pad, Cout, ld_dy)
WGRAD_CASES = [
    (1, 32, 128, 64, 64, 64, 64),      # bm 64, L 32, one row per slice, 2 splits
    (2, 9, 40, 64, 64, 128, 128),      # bm 128, L 30, MULTIROW R = 3
    (1, 7, 28, 64, 64, 64, 64),        # bm 64, L 30, MULTIROW R = 4; the last slice is short
    (1, 3, 5, 64, 64, 64, 64),         # R = 16, one slice
    (3, 5, 33, 96, 96, 192, 192),      # tilesM 2, tilesN 3
    (1, 40, 120, 64, 64, 128, 128),    # L 30, 2 splits
    (2, 11, 130, 36, 36, 72, 72),      # S = 2, ragged second slice; Cin_pad no multiple of 32; Cout below one row tile
    (1, 50, 131, 32, 32, 40, 44),      # ld_dy > Cout, 6 splits with a short last one
    (2, 17, 60, 128, 128, 64, 64),     # tilesN 3, R = 2 with an odd number of rows
    (2, 24, 256, 64, 64, 64, 64),      # L 32, S = 2
    (1, 12, 20, 60, 64, 64, 64),       # Cin < Cin_pad; the pad channels of x are zero
    # what the cases above leave open: {bm 128, one row, L 32} and {bm 128, MULTIROW, L 32} of family 4, three instantiations of family 2
    (2, 6, 64, 64, 64, 128, 128),      # family 4: {bm 128, MULTIROW, L 32} (Wt = 16, R = 2); family 2: {bm 128, one row, L 32}
    (1, 16, 128, 32, 32, 72, 72),      # family 4: {bm 128, one row, L 32} (Wt = 32); family 2: the same with S = 2
    (1, 9, 20, 32, 32, 96, 96),        # family 2: {bm 128, MULTIROW, L 30} (Wt = 10, R = 3)
    (1, 8, 16, 32, 32, 96, 96),        # family 2: {bm 128, MULTIROW, L 32} (Wt = 8, R = 4)
    (2, 5, 8, 32, 32, 40, 40),         # family 2: {bm 64, MULTIROW, L 32} (Wt = 4, R = 8, the second slice holds two rows)
]
EPRE_CASES = [(1, 3, 5, 64, 64, 64, 64), (3, 5, 33, 96, 96, 192, 192), (1, 50, 131, 32, 32, 40, 44)]   # W = 5, 33, 131: ragged mod 4

FWD_ARMS = {
    2: {"bn": {32, 64, 128}, "blocks": {"single", "multi+single"}, "ksplit": {1}, "chunk": {1024}},
    4: {"bn": {32, 64, 128}, "blocks": {"single", "multi+single"}, "ksplit": {1, 2, 3}, "chunk": {64, 256, 1024}},
}
WGRAD_ARMS = {(bm, mr, L) for bm in (64, 128) for mr in (False, True) for L in (30, 32)}    # the 8 instantiations, per family


# ------------------------------------------------------------------------------- fp32 restatements of the two transform chains
# The constants are the kernels' (csrc/wino.hip, csrc/wino4.hip).  Products are accumulated in fp32 one K element after the other, the order
# of the MFMA chain of one workgroup (no K split, one slab: the longest chain any plan produces).
BT = {2: np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64),
      4: np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                   [0, 4, 0, -5, 0, 1]], dtype=np.float64)}
G = {2: np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64),
     4: np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                  [0, 0, 1]], dtype=np.float64)}
AT = {2: np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64),
      4: np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)}


def _windows(fam, xp, f):
    """d[tile][j][3 rows][Cin] of a zero-framed image xp [H+2][Wpad+2][Cin]: the g + 2 columns of every group of g output columns."""
    g = group(fam)
    H, Wt = xp.shape[0] - 2, (xp.shape[1] - 2) // g
    d = np.empty((H, Wt, g + 2, 3, xp.shape[2]), dtype=f)
    for y in range(H):
        for t in range(Wt):
            d[y, t] = xp[y:y + 3, g * t:g * t + g + 2].transpose(1, 0, 2)
    return d.reshape(H * Wt, g + 2, 3 * xp.shape[2])


def _frame(fam, x):
    g = group(fam)
    H, W, C = x.shape
    xp = np.zeros((H + 2, cdiv(W, g) * g + 2, C), dtype=x.dtype)
    xp[1:H + 1, 1:W + 1] = x
    return xp


def _fma(c, a, b):
    return (np.float64(c) * a.astype(np.float64) + b.astype(np.float64)).astype(np.float32)


# taps (columns d_j) and coefficients of the three fused multiply-adds of wino4.hip's staging path; xi 1..4 start from d4
W4_TAPS = ((0, 2, 4), (1, 2, 3), (1, 2, 3), (1, 2, 3), (1, 2, 3), (1, 3, 5))
W4_COEF = ((4, -5, 1), (-4, -4, 1), (4, -4, -1), (-2, -1, 2), (2, -1, -2), (4, -5, 1))


def _input_transform_f32(fam, xi, d):
    """V_xi = (B^T d)_xi of d [T][g+2][K] as the staging paths evaluate it: F(2,3) one fused multiply-add p + sg*q, F(4,3)
    fma(c0, d_j0, fma(c1, d_j1, fma(c2, d_j2, d4 | 0)))."""
    if fam == 2:
        return np.einsum("j,tjk->tk", BT[2][xi], d.astype(np.float64)).astype(np.float32)
    (j0, j1, j2), (c0, c1, c2) = W4_TAPS[xi], W4_COEF[xi]
    v = d[:, 4] if 1 <= xi <= 4 else np.zeros_like(d[:, 0])
    return _fma(c0, d[:, j0], _fma(c1, d[:, j1], _fma(c2, d[:, j2], v)))


def _seq_matmul(a, b):
    """sum_k a[.., k] * b[k, ..] accumulated in fp32 one k after the other (one fused multiply-add each, as the MFMA chain)."""
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    for k in range(a.shape[1]):
        acc = (acc.astype(np.float64) + a[:, k, None].astype(np.float64) * b[None, k].astype(np.float64)).astype(np.float32)
    return acc


def forward_chain_f32(fam, x, w):
    """y [H][W][Cout] of one image x [H][W][Cin], w [Cout][3][3][Cin] (no bias) through V = B^T d, U = G g, y = A^T m in fp32."""
    f = np.float32
    g = group(fam)
    H, W, Cin = x.shape
    Cout = w.shape[0]
    d = _windows(fam, _frame(fam, x.astype(f)), f)                                   # [T][g+2][3Cin]
    wr = w.astype(f).transpose(2, 1, 3, 0).reshape(3, 3 * Cin, Cout)                 # [s][r*Cin+ci][co]
    if fam == 4:                                                                     # k_wino4_weight: in double, rounded once
        U = np.einsum("xs,skc->xkc", G[4], wr.astype(np.float64)).astype(f)
    else:                                                                            # k_wino_weight: 0.5f * (g0 +- g1 + g2) in fp32
        U = np.stack([wr[0], f(0.5) * ((wr[0] + wr[1]) + wr[2]), f(0.5) * ((wr[0] - wr[1]) + wr[2]), wr[2]])
    m = [_seq_matmul(_input_transform_f32(fam, xi, d), U[xi]) for xi in range(nplanes(fam))]
    m = np.stack(m)                                                                  # [xi][T][Cout]
    y = np.zeros((H * (d.shape[0] // H), g, Cout), dtype=f)
    for i in range(g):                                                               # k_wino*_output, fp32 in its order of operations
        if fam == 2:
            y[:, i] = (m[0] + m[1]) + m[2] if i == 0 else (m[1] - m[2]) - m[3]
        elif i == 0:
            y[:, i] = (m[0] + (m[1] + m[2])) + (m[3] + m[4])
        elif i == 1:
            y[:, i] = (m[1] - m[2]) + f(2) * (m[3] - m[4])
        elif i == 2:
            y[:, i] = (m[1] + m[2]) + f(4) * (m[3] + m[4])
        else:
            y[:, i] = ((m[1] - m[2]) + f(8) * (m[3] - m[4])) + m[5]
    return y.reshape(H, -1, Cout)[:, :W]


def wgrad_chain_f32(fam, x, dy):
    """dW [Cout][3][3][Cin] of one image x [H][W][Cin], dy [H][W][Cout] through E = A dy, V = B^T d and the reduction G^T of
    k_wgrad_wino_reduce / k_wgrad_wino4_reduce in fp32; the tile sum runs in fp32 one tile after the other."""
    f = np.float32
    g = group(fam)
    H, W, Cin = x.shape
    Cout = dy.shape[2]
    d = _windows(fam, _frame(fam, x.astype(f)), f)
    Wt = d.shape[0] // H
    dyp = np.zeros((H, Wt * g, Cout), dtype=f)
    dyp[:, :W] = dy.astype(f)
    dyp = dyp.reshape(H * Wt, g, Cout)
    if fam == 2:
        A = np.array([[1, 0], [1, 1], [1, -1], [0, 1]], dtype=np.float64)           # (dy0, dy0+dy1, dy0-dy1, +dy1: the sign moves to the end)
    else:
        A = AT[4].T
    if fam == 2:                                                                     # E = a0 + sgA * a1, one fused multiply-add
        A = np.array([[1, 0], [1, 1], [1, -1], [0, 1]], dtype=np.float64)           # (dy0, dy0+dy1, dy0-dy1, +dy1: the sign moves to the end)
        E = [np.einsum("i,tic->tc", A[xi], dyp.astype(np.float64)).astype(f) for xi in range(4)]
    else:                                                                            # k_wino4_dy_transform; E0 / E5 are columns of dy
        d0, d1, d2, d3 = (dyp[:, i] for i in range(4))
        a, b, c, e = d0 + d2, d1 + d3, d0 + f(4) * d2, f(2) * d1 + f(8) * d3
        E = [d0, a + b, a - b, c + e, c - e, d3]
    P = [_seq_matmul(E[xi].T.copy(), _input_transform_f32(fam, xi, d)) for xi in range(nplanes(fam))]   # [Cout][3Cin]
    P = [p.reshape(Cout, 3, Cin) for p in P]
    dw = np.empty((Cout, 3, 3, Cin), dtype=f)
    if fam == 2:
        h = f(0.5) * (P[1] + P[2])
        dw[:, :, 0], dw[:, :, 1], dw[:, :, 2] = P[0] + h, f(0.5) * (P[1] - P[2]), h - P[3]
    else:
        s12, d12, s34, d34 = P[1] + P[2], P[2] - P[1], P[3] + P[4], P[3] - P[4]
        dw[:, :, 0] = (f(0.25) * P[0] - s12 * (f(1) / f(6))) + s34 * (f(1) / f(24))
        dw[:, :, 1] = d12 * (f(1) / f(6)) + d34 * (f(1) / f(12))
        dw[:, :, 2] = (s34 - s12) * (f(1) / f(6)) + P[5]
    return dw


def rel_l2(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def worst_row_rel_l2(got, ref):
    """Worst relative L2 over the slices along the first axis (image rows of y, output channels of dW)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    e = np.linalg.norm((got - ref).reshape(ref.shape[0], -1), axis=1)
    n = np.linalg.norm(ref.reshape(ref.shape[0], -1), axis=1)
    return float((e / n).max())


def measure_chain(kind, fam, Cin, seed=0):
    """(whole-tensor, worst-row) relative L2 rounding error of the fp32 restatement against fp64, on the data the GPU tests use
    (post-ReLU activations, He-scaled filters, standard-normal dy).  kind: "fwd", "dgrad" (the forward chain on a standard-normal input; Cin
    is the channel count it reduces over, the layer's Cout) or "wgrad".  Shapes: see MEASURE_SHAPE."""
    rng = np.random.default_rng(seed + 17 * fam + Cin)
    H, W, Cout = MEASURE_SHAPE[kind]
    x = rng.standard_normal((H, W, Cin))
    x = (x if kind == "dgrad" else np.maximum(x, 0)).astype(np.float32)     # the data-grad's input is dy, not an activation
    xt = torch.from_numpy(x)[None]
    if kind != "wgrad":
        w = (rng.standard_normal((Cout, 3, 3, Cin)) * math.sqrt(2.0 / (9 * Cin))).astype(np.float32)
        ref = conv_fwd_ref(xt, torch.from_numpy(w))[0].numpy()
        got = forward_chain_f32(fam, x, w)
    else:
        dy = rng.standard_normal((H, W, Cout)).astype(np.float32)
        ref = conv_wgrad_ref(xt, torch.from_numpy(dy)[None]).numpy()
        got = wgrad_chain_f32(fam, x, dy)
    return rel_l2(got, ref), worst_row_rel_l2(got, ref)


# (H, W, Cout) of the restatement.  forward / data-grad: 12 rows of 11 pixels (ragged for both families) x 32 channels - rows no longer
# than most rows of the GPU cases, so that averaging does not flatter the worst-row figure.  weight-grad: 22 x 120 pixels = 660 groups of
# four, the longest slab of any F(4,3) case (22 slices of 30 in (2, 11, 130)); for F(2,3) 1320 pairs, above its longest slab (540).
MEASURE_SHAPE = {"fwd": (12, 11, 32), "dgrad": (12, 11, 32), "wgrad": (22, 120, 16)}

# Measured by tests/test_wino1d_ref_cpu.py::test_chain_rounding (which asserts that a fresh measurement reproduces them within 10 %):
# (whole, worst row) at Cin = 64 and Cin = 512.  profiles/wino1d_margins.txt records them with the bounds.
MEASURED = {
    ("fwd", 2, 64): (2.451e-07, 2.756e-07), ("fwd", 2, 512): (7.130e-07, 7.843e-07),
    ("fwd", 4, 64): (5.979e-07, 6.862e-07), ("fwd", 4, 512): (1.600e-06, 1.861e-06),
    ("dgrad", 2, 64): (3.158e-07, 3.661e-07), ("dgrad", 2, 512): (9.004e-07, 1.020e-06),
    ("dgrad", 4, 64): (7.463e-07, 8.176e-07), ("dgrad", 4, 512): (2.115e-06, 2.280e-06),
    ("wgrad", 2, 64): (6.760e-07, 7.996e-07), ("wgrad", 2, 512): (7.019e-07, 7.724e-07),
    ("wgrad", 4, 64): (1.215e-06, 1.486e-06), ("wgrad", 4, 512): (1.215e-06, 1.503e-06),
}


def bound(kind, fam, Cin, which):
    """3 x (weight-grad: 6 x, the further factor 2 of tests/test_gpu_w6.py) the restatement's error at Cin, interpolated between the
    measurements at 64 and 512 as a power of Cin (it grows roughly as sqrt(Cin)); which: 0 whole tensor, 1 worst row."""
    e64, e512 = MEASURED[(kind, fam, 64)][which], MEASURED[(kind, fam, 512)][which]
    p = math.log(e512 / e64) / math.log(8.0)
    return (6.0 if kind == "wgrad" else 3.0) * e64 * (Cin / 64.0) ** p
