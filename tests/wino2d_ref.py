"""fp64 references, integer restatements of the host planners, fp32 restatements of the transform chains and the case tables for the
2-D Winograd conv kernels of csrc/wino2d.hip: F(4x4,3x3) (`cvk_w2d_*`, tile `mt` 4) and F(6x6,3x3) (`cvk_w6_*`, `mt` 6).  They replace
nn.Conv2d(cin, cout, 3, padding=1): forward with the BatchNorm batch statistics, data-grad and weight-grad.  No GPU and no library:
tests/test_wino2d_ref_cpu.py checks this file against torch.nn.functional, tests/test_gpu_wino2d.py checks the kernels against it.

Layouts are the C ABI's (include/cvk.h): activations NHWC, filters [Cout][3][3][Cin], transform planes [xi = i * NT + j][row][channel]."""
import math

import numpy as np
import torch

from tests.wino1d_ref import cdiv, chan_combine, conv_dgrad_ref, conv_fwd_ref, conv_wgrad_ref, dgrad_filter, rel_l2, worst_row_rel_l2  # noqa: F401

GUARD = 4096            # floats behind every device buffer of the GPU tests
SLACK = 128             # floats behind the V and E planes that partial column tiles of the weight-grad GEMM may read
W2_BN = 128             # csrc/wino2d.hip: output columns per GEMM workgroup
BM = 128                # ... and its rows
SLOTS = 512             # plan_w2d: resident GEMM workgroups
SIZE_CAP = 1 << 27      # floats in any one device buffer of a case (tests/test_wino2d_ref_cpu.py)
TILES = (4, 6)


def nt_of(mt):
    return mt + 2


def nx_of(mt):
    return (mt + 2) ** 2


def vw_of(mt):
    """Channels per thread of the transform kernels (W2T<MT>::VW)."""
    return 4 if mt == 4 else 2


# ------------------------------------------------------------------------------------------------------------ fp64 references
def _shifted(x, r, s):
    """x [N][H][W][C] moved so that element (y, x) holds x[y + r - 1][x + s - 1] (zero outside the frame)."""
    N, H, W, C = x.shape
    out = torch.zeros_like(x)
    ys, ye = max(0, 1 - r), min(H, H + 1 - r)
    xs, xe = max(0, 1 - s), min(W, W + 1 - s)
    out[:, ys:ye, xs:xe] = x[:, ys + r - 1:ye + r - 1, xs + s - 1:xe + s - 1]
    return out


def conv_fwd_mm(x, w, b=None):
    """conv_fwd_ref as nine matrix products in double, on whichever device x lives (the GPU tests run it there: the largest cases are 35 GFLOP).
    x [N][H][W][Cin], w [Cout][3][3][Cin] -> y [N][H][W][Cout]."""
    x, w = x.double(), w.double()
    N, H, W, Cin = x.shape
    y = torch.zeros(N * H * W, w.shape[0], dtype=torch.float64, device=x.device)
    for r in range(3):
        for s in range(3):
            y += _shifted(x, r, s).reshape(-1, Cin) @ w[:, r, s, :].t()
    if b is not None:
        y += b.double()
    return y.view(N, H, W, -1)


def conv_dgrad_mm(dy, w):
    """conv_dgrad_ref the same way: the forward conv of dy with the rotated, channel-transposed filter."""
    return conv_fwd_mm(dy, dgrad_filter(w))


def conv_wgrad_mm(x, dy):
    """conv_wgrad_ref the same way: dW[co][r][s][ci] = sum over pixels of dy[p][co] * x[p + (r - 1, s - 1)][ci]."""
    x, dy = x.double(), dy.double()
    Cin, Cout = x.shape[3], dy.shape[3]
    d = dy.reshape(-1, Cout).t().contiguous()
    dw = torch.empty(Cout, 3, 3, Cin, dtype=torch.float64, device=x.device)
    for r in range(3):
        for s in range(3):
            dw[:, r, s] = d @ _shifted(x, r, s).reshape(-1, Cin)
    return dw


# The matrices of the two tiles in double (points 0, +-1, +-2, inf; F(6x6) adds +-1/2): V = B^T d B, U = G g G^T, y = A^T m A, and the transposes
# the backward pass uses: E = A dy A^T (A = (A^T)^T) and dW = G^T P G.
BT = {4: np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                   [0, 4, 0, -5, 0, 1]], dtype=np.float64),
      6: np.array([[1, 0, -5.25, 0, 5.25, 0, -1, 0], [0, 1, 1, -4.25, -4.25, 1, 1, 0], [0, -1, 1, 4.25, -4.25, -1, 1, 0],
                   [0, .5, .25, -2.5, -1.25, 2, 1, 0], [0, -.5, .25, 2.5, -1.25, -2, 1, 0], [0, 2, 4, -2.5, -5, .5, 1, 0],
                   [0, -2, 4, 2.5, -5, -.5, 1, 0], [0, -1, 0, 5.25, 0, -5.25, 0, 1]], dtype=np.float64)}
G = {4: np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                  [0, 0, 1]], dtype=np.float64),
     6: np.array([[1, 0, 0], [-2 / 9, -2 / 9, -2 / 9], [-2 / 9, 2 / 9, -2 / 9], [1 / 90, 1 / 45, 2 / 45], [1 / 90, -1 / 45, 2 / 45],
                  [32 / 45, 16 / 45, 8 / 45], [32 / 45, -16 / 45, 8 / 45], [0, 0, 1]], dtype=np.float64)}
AT = {4: np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64),
      6: np.array([[1 if r == 0 else 0, 1, (-1) ** r, 2 ** r, (-2) ** r, 2.0 ** -r, (-2.0) ** -r, 1 if r == 5 else 0] for r in range(6)],
                  dtype=np.float64)}
A = {mt: AT[mt].T.copy() for mt in TILES}
GT = {mt: G[mt].T.copy() for mt in TILES}
# integer multiples of the fractional matrices, for the exact identity check: 24 G(4), 90 G(6), 4 B^T(6), 32 A^T(6)
INT_SCALE = {"G": {4: 24, 6: 90}, "BT": {4: 1, 6: 4}, "AT": {4: 1, 6: 32}}


def tile_windows(mt, x, halo=True):
    """x [N][H][W][C] (numpy or torch) -> the tiles in the kernels' order (image, tile row, tile column): with the one-pixel halo
    [T][NT][NT][C] (what B^T . B takes), without [T][MT][MT][C] (what A . A^T takes); zero outside the frame."""
    is_t = torch.is_tensor(x)
    N, H, W, C = x.shape
    th, tw = cdiv(H, mt), cdiv(W, mt)
    h = 1 if halo else 0
    n = mt + 2 * h
    shape = (N, th * mt + 2 * h, tw * mt + 2 * h, C)
    xp = torch.zeros(shape, dtype=x.dtype, device=x.device) if is_t else np.zeros(shape, dtype=x.dtype)
    xp[:, h:H + h, h:W + h] = x
    rows = []
    for i in range(n):
        cols = [xp[:, i:i + th * mt:mt, j:j + tw * mt:mt] for j in range(n)]            # [N][th][tw][C] each
        rows.append(torch.stack(cols, 3) if is_t else np.stack(cols, 3))               # [N][th][tw][n][C]
    d = torch.stack(rows, 3) if is_t else np.stack(rows, 3)                             # [N][th][tw][n][n][C]
    return d.reshape(N * th * tw, n, n, C)


def planes_ref(M, d):
    """M d M^T per tile and channel in double, with the sum of the absolute terms beside it (what an fp32 evaluation's rounding scales with):
    d [T][n][n][C] torch -> two tensors [rows(M)^2][T][C]."""
    Mt = torch.as_tensor(M, dtype=torch.float64, device=d.device)
    d = d.double()
    val = torch.einsum("ia,tabc,jb->ijtc", Mt, d, Mt)
    mag = torch.einsum("ia,tabc,jb->ijtc", Mt.abs(), d.abs(), Mt.abs())
    k = M.shape[0]
    return val.reshape(k * k, *val.shape[2:]), mag.reshape(k * k, *mag.shape[2:])


def filter_planes_ref(mt, w):
    """U [NX][Cout][Cin] = G g G^T of w [Cout][3][3][Cin] in double, and the sum of the absolute terms."""
    Gt = torch.as_tensor(G[mt], dtype=torch.float64, device=w.device)
    w = w.double()
    val = torch.einsum("ia,oabc,jb->ijoc", Gt, w, Gt)
    mag = torch.einsum("ia,oabc,jb->ijoc", Gt.abs(), w.abs(), Gt.abs())
    return val.reshape(nx_of(mt), *val.shape[2:]), mag.reshape(nx_of(mt), *mag.shape[2:])


def output_ref(mt, m, N, H, W):
    """y [N][H][W][C] = A^T m A of product planes m [NX][T][C] in double (tiles cropped at the frame), and the sum of the absolute terms."""
    n = nt_of(mt)
    th, tw = cdiv(H, mt), cdiv(W, mt)
    At = torch.as_tensor(AT[mt], dtype=torch.float64, device=m.device)
    m = m.double().reshape(n, n, N, th, tw, -1)
    out = []
    for a, mm in ((At, m), (At.abs(), m.abs())):
        o = torch.einsum("ia,abnyxc,jb->nyixjc", a, mm, a)
        out.append(o.reshape(N, th * mt, tw * mt, -1)[:, :H, :W].contiguous())
    return out


# Roundings on the longest path of one evaluation of each 1-D routine (a product with a power of two is exact); k of the element-wise bounds
# k u (|M| |d| |M^T|) of tests/test_gpu_wino2d.py is twice that (rows, then columns) — three more for the output pass (see OUT_DEPTH).
#   w2_bt: v0 = 4 d0 - 5 d2 + d4: the product by 5, two additions                                                          3
#   w6_bt: b3 = 2 d1 - 2.5 d3 + 0.5 d5: one product, two additions; v5 = a3 + b3                                           4
#   w2_a:  s02 + s13, each one addition                                                                                    2
#   w6_a:  ev = d0 + d2 + d4: two additions; ev + od                                                                       3
#   w2_g / w6_g: a rounded constant (1), t = g0 + g2, t + g1, the product; or two rounded products, their sum and one more  4
BT_DEPTH = {4: 3, 6: 4}
A_DEPTH = {4: 2, 6: 3}
G_DEPTH = {4: 4, 6: 4}
# k_w2d_output: A^T along the rows (w2_at: m0 + s12 + s34 with s12 rounded = 3; w6_at: four terms = 4), then the NT - 1 products of a column's
# contributions are added one after the other (at most NT - 2 additions of non-zero terms: 4 / 6), and the bias is added (1)
OUT_DEPTH = {4: 3 + 4 + 1, 6: 4 + 6 + 1}


# --------------------------------------------------------------------------------------- integer restatements of the host planners
def tiles(mt, N, H, W):
    return N * cdiv(H, mt) * cdiv(W, mt)


def tpad(T):
    return cdiv(T, 32) * 32


def tb(T):
    """w2_tb: tiles per block of the output pass = per statistics partial."""
    return 16 if T >= 8192 else 4


def plan_fwd(mt, T, Cin, Cout):
    """plan_w2d: NT GEMM tiles of 128 x 128 over nx planes; the tiles behind the last whole round of 512 workgroups (ids >= split_start) are cut
    into f K ranges.  grid = workgroups of the launch."""
    tilesM, tilesN = cdiv(T, BM), cdiv(Cout, W2_BN)
    NT = nx_of(mt) * tilesM * tilesN
    nK = Cin // 32
    full = NT // SLOTS * SLOTS
    R = NT - full
    f = 1
    if R > 0:
        f = max(1, min(SLOTS // R, 4, nK // 4))
    split_start = full if f > 1 else NT
    return dict(tilesM=tilesM, tilesN=tilesN, NT=NT, full=full, f=f, split_start=split_start, grid=split_start + (NT - split_start) * f)


def plan_out(mt, T, Cout):
    """w2i_output: vw channels per thread, cvn channel vectors per block, grid.y channel blocks, TB tiles per block, P blocks = partials."""
    vw = vw_of(mt)
    nv = Cout // vw
    cvn = 64 if nv >= 64 else (32 if nv >= 32 else 16)
    return dict(vw=vw, nv=nv, cvn=cvn, gy=cdiv(nv, cvn), TB=tb(T), P=cdiv(T, tb(T)))


def plan_wgrad(mt, T, Cin_pad, Cout):
    """plan_w2d_wgrad: 128 x 128 tiles of P_xi [Cout][Cin_pad]; the depth (Tpad / 32 slices) is cut into f ranges, range p = slices
    [p nK / f, (p + 1) nK / f)."""
    Tp = tpad(T)
    tilesM, tilesN = cdiv(Cout, 128), cdiv(Cin_pad, 128)
    nt, nK = nx_of(mt) * tilesM * tilesN, Tp // 32
    f = max(1, min(cdiv(1024, nt), nK // 4, 16))
    return dict(Tpad=Tp, tilesM=tilesM, tilesN=tilesN, nK=nK, f=f)


def fwd_workspace_floats(mt, N, H, W, Cin, Cout):
    T = tiles(mt, N, H, W)
    return nx_of(mt) * tpad(T) * Cin + SLACK + nx_of(mt) * T * plan_fwd(mt, T, Cin, Cout)["f"] * Cout


def wgrad_workspace_floats(mt, N, H, W, Cin_pad, Cout):
    p = plan_wgrad(mt, tiles(mt, N, H, W), Cin_pad, Cout)
    return nx_of(mt) * p["Tpad"] * (Cin_pad + Cout) + 2 * SLACK + p["f"] * nx_of(mt) * Cout * Cin_pad


def partial_counts(mt, N, H, W):
    """Live pixels of every statistics partial: TB consecutive tiles each, a ragged tile counted by the pixels inside the frame."""
    th, tw = cdiv(H, mt), cdiv(W, mt)
    T = N * th * tw
    TB = tb(T)
    cnt = [0] * cdiv(T, TB)
    for t in range(T):
        r = t % (th * tw)
        cnt[t // TB] += min(mt, H - mt * (r // tw)) * min(mt, W - mt * (r % tw))
    return cnt


def partial_of_pixel(mt, N, H, W):
    """int64 [N][H][W]: the statistics partial every pixel belongs to."""
    th, tw = cdiv(H, mt), cdiv(W, mt)
    n = torch.arange(N).view(N, 1, 1)
    ty = (torch.arange(H) // mt).view(1, H, 1)
    tx = (torch.arange(W) // mt).view(1, 1, W)
    return (n * th * tw + ty * tw + tx) // tb(N * th * tw)


def stat_depth(mt, T, Cout):
    """Roundings of one column sum in k_w2d_output: a thread adds the MT^2 pixels of its ceil(TB / pl) tiles one after the other, thread 0 of
    the column then adds the pl = 256 / cvn partial sums one after the other."""
    p = plan_out(mt, T, Cout)
    pl = 256 // p["cvn"]
    return cdiv(p["TB"], pl) * mt * mt + pl


def arm_of(kind, mt, case):
    """Names what a case runs.
    kind "fwd",   case (N,H,W,Cin,Cout[,ldy]):  ("fwd", mt, rounds, f, store, cvn, ragged, TB)
        rounds: "one" (no K split), "split-all" (every GEMM tile is cut in K) or "full+split" (whole rounds of workgroups, a split tail behind them:
        the only plan in which k_w2d_output's xi0 lies strictly inside (0, NX) and parts 1..f-1 exist for some tiles only);
        store: "raw" (every column tile 128 wide: buffer stores), "checked" (Cout < 128) or "raw+checked" (a ragged last column tile);
        cvn: channel vectors per block of the output pass, ragged: its last channel block is partly empty, TB: tiles per block.
    kind "dgrad", case (N,H,W,Cin,Cout) of the layer: the forward arm of the launch, whose depth is Cout and whose width is Cin.
    kind "out",   case (N,H,W,Cout): the output pass alone on f = 1 planes of depth 32.
    kind "wgrad", case (N,H,W,Cin,Cin_pad,Cout,ld_dy):  ("wgrad", mt, f, even, raggedM, raggedN); even: the nK depth slices divide by f."""
    if kind == "wgrad":
        N, H, W, Cin, Cin_pad, Cout, ld_dy = case
        p = plan_wgrad(mt, tiles(mt, N, H, W), Cin_pad, Cout)
        return ("wgrad", mt, p["f"], p["nK"] % p["f"] == 0, Cout % 128 != 0, Cin_pad % 128 != 0)
    N, H, W = case[:3]
    if kind == "out":
        Cin, Cout = 32, case[3]
    elif kind == "dgrad":
        Cin, Cout = case[4], case[3]
    else:
        Cin, Cout = case[3:5]
    T = tiles(mt, N, H, W)
    p, o = plan_fwd(mt, T, Cin, Cout), plan_out(mt, T, Cout)
    rounds = "one" if p["f"] == 1 else ("split-all" if p["split_start"] == 0 else "full+split")
    store = "raw" if Cout % W2_BN == 0 else ("checked" if Cout < W2_BN else "raw+checked")
    return (kind, mt, rounds, p["f"], store, o["cvn"], o["nv"] % o["cvn"] != 0, o["TB"])


# -------------------------------------------------------------------------------------------------------------------- case tables
# (N, H, W, Cin, Cout[, ldy]); the comments name the arm the case is there for
FWD_CASES = [
    (1, 96, 102, 256, 384),        # full+split for both tiles: F(4x4) T 624, NT 540, split_start 512, f 2; F(6x6) T 272, NT 576, split_start 512, f 2
    (1, 96, 102, 512, 384),        # the same with f 4
    (1, 48, 102, 512, 132),        # split-all, raw+checked, ragged channel block (cvn 32 / 64)
    (1, 44, 44, 384, 136),         # f 3
    (1, 13, 11, 288, 320),         # tilesN 3, f 2; F(4x4): ragged channel block at cvn 64
    (3, 5, 7, 32, 68),             # checked-only store, cvn 16 / 32 with a ragged block, Cout % 8 != 0
    (1, 1, 9, 96, 100),            # the same, H = 1
    (2, 7, 1, 64, 64),             # W = 1
    (1, 9, 13, 64, 132),           # raw+checked without a K split
    (2, 10, 14, 32, 64, 72),       # ldy > Cout
    # the seven cases of tests/test_gpu_w6.py
    (1, 5, 7, 32, 64),
    (2, 12, 18, 64, 64),
    (1, 22, 30, 256, 256),
    (2, 45, 60, 128, 192),
    (1, 3, 4, 512, 128),
    (8, 22, 30, 512, 256),
    (2, 90, 120, 64, 128),
]
# (N, H, W, Cin, Cout) of the layer: the launch reduces over Cout and writes Cin channels
DGRAD_CASES = [
    (1, 96, 102, 384, 256),        # full+split, f 2, for both tiles
    (1, 48, 102, 132, 512),        # split-all, raw+checked, ragged channel block
    (3, 5, 7, 68, 32),             # checked-only store, cvn 16 / 32 with a ragged block
    (1, 13, 11, 320, 288),         # tilesN 3, f 2
    (2, 12, 18, 64, 64),           # the three cases of tests/test_gpu_w6.py
    (1, 22, 30, 256, 128),
    (2, 45, 60, 128, 192),
]
# (N, H, W, Cout): the output pass alone.  TB = 16 needs T >= 8192: 91 x 91 tiles for either tile size, ragged on both edges
OUT_CASES = {
    4: [(1, 362, 363, 64), (2, 9, 14, 68), (1, 7, 5, 320)],
    6: [(1, 543, 541, 64), (2, 9, 14, 68), (1, 7, 5, 320)],
}
# (N, H, W, Cin, Cin_pad, Cout, ld_dy)
WGRAD_CASES = [
    (1, 180, 180, 32, 32, 64, 64),         # F(4x4): f 16, even.  F(6x6): f 7 over nK 29
    (1, 270, 270, 32, 32, 64, 64),         # F(6x6): f 16.  F(4x4): f 16 over nK 145, uneven
    (1, 50, 131, 32, 36, 68, 72),          # F(4x4): f 3 over nK 14; Cin_pad 36, ld_dy > Cout, Cout ragged
    (2, 40, 80, 60, 64, 72, 72),           # Cin < Cin_pad: the pad channels of x hold 1e30 and must not reach dW
    (3, 21, 27, 132, 132, 200, 200),       # 2 x 2 tiles, both ragged
    (2, 9, 14, 96, 96, 128, 128),          # whole M tile, ragged N tile
    # the four cases of tests/test_gpu_w6.py
    (2, 12, 18, 64, 64, 64, 64),
    (1, 22, 30, 256, 256, 128, 128),
    (2, 45, 60, 128, 128, 192, 192),
    (8, 22, 30, 512, 512, 256, 256),
]
# single passes: (N, H, W, C, ld) of the transform tests (ld: pitch of dy; the input transform takes dense tensors)
TRANSFORM_CASES = [(1, 5, 7, 32, 32), (2, 13, 11, 36, 44), (3, 12, 18, 64, 72), (1, 1, 9, 96, 96), (2, 7, 1, 8, 8), (1, 30, 41, 4, 12)]
FILTER_CASES = [(64, 32), (68, 36), (33, 65), (132, 200)]         # (Cout, Cin)

FWD_ARMS = {
    "rounds": {"one", "split-all", "full+split"},
    "f": {1, 2, 3, 4},
    "store": {"raw", "checked", "raw+checked"},
    # (cvn, ragged last channel block): F(4x4) takes 4 channels per thread (cvn 16 up to 124 channels), F(6x6) 2 (never below 32 vectors)
    "out": {4: {(16, False), (16, True), (32, False), (32, True), (64, False), (64, True)},
            6: {(32, False), (32, True), (64, False), (64, True)}},
    "TB": {4, 16},                  # 16 through OUT_CASES
}
WGRAD_ARMS = {
    "f": {4: {1, 3, 16}, 6: {1, 7, 16}},
    "even_split": {True, False},    # among the cases with f > 1: do the nK depth slices divide by f?
    "ragged": {(False, False), (True, True), (False, True), (True, False)},       # (M tile ragged, N tile ragged)
}


def case_buffers(kind, mt, case):
    """Floats of every device buffer a case allocates (without guard bands): the size cap of tests/test_wino2d_ref_cpu.py."""
    nx = nx_of(mt)
    if kind == "wgrad":
        N, H, W, Cin, Cin_pad, Cout, ld_dy = case
        T = tiles(mt, N, H, W)
        p = plan_wgrad(mt, T, Cin_pad, Cout)
        return dict(x=N * H * W * Cin_pad, dy=N * H * W * ld_dy, V=nx * p["Tpad"] * Cin_pad + SLACK, E=nx * p["Tpad"] * Cout + SLACK,
                    P=p["f"] * nx * Cout * Cin_pad, dw=Cout * 9 * Cin, ws=wgrad_workspace_floats(mt, N, H, W, Cin_pad, Cout))
    N, H, W = case[:3]
    if kind == "out":
        Cin, Cout, ldy = 32, case[3], case[3]
    elif kind == "dgrad":
        Cin, Cout, ldy = case[4], case[3], case[3]
    else:
        Cin, Cout = case[3:5]
        ldy = case[5] if len(case) > 5 else Cout
    T = tiles(mt, N, H, W)
    f = plan_fwd(mt, T, Cin, Cout)["f"]
    return dict(x=N * H * W * Cin, U=nx * Cout * Cin, V=nx * tpad(T) * Cin + SLACK, Mo=f * nx * T * Cout, y=N * H * W * ldy,
                ws=fwd_workspace_floats(mt, N, H, W, Cin, Cout))


# ------------------------------------------------------------------------------- fp32 restatements of the two transform chains
# Every operation below is one rounded fp32 operation in the order the kernels' source spells it (the compiler may contract a product and
# a sum into one fused operation, and the matrix cores keep more than fp32 inside a block: the device rounds less often, never more).
F32 = np.float32


def bt_f32(mt, d):
    """w2_bt / w6_bt on a list of NT float32 arrays."""
    c = F32
    if mt == 4:
        a, b, cc, e = d[4] - c(4) * d[2], d[3] - c(4) * d[1], d[4] - d[2], c(2) * (d[3] - d[1])
        return [c(4) * d[0] - c(5) * d[2] + d[4], a + b, a - b, cc + e, cc - e, c(4) * d[1] - c(5) * d[3] + d[5]]
    v0 = d[0] - d[6] + c(5.25) * (d[4] - d[2])
    v7 = d[7] - d[1] + c(5.25) * (d[3] - d[5])
    a1, b1 = d[2] + d[6] - c(4.25) * d[4], d[1] + d[5] - c(4.25) * d[3]
    a2, b2 = d[6] + c(0.25) * d[2] - c(1.25) * d[4], c(0.5) * d[1] - c(2.5) * d[3] + c(2) * d[5]
    a3, b3 = d[6] + c(4) * d[2] - c(5) * d[4], c(2) * d[1] - c(2.5) * d[3] + c(0.5) * d[5]
    return [v0, a1 + b1, a1 - b1, a2 + b2, a2 - b2, a3 + b3, a3 - b3, v7]


def at_f32(mt, m):
    """w2_at / w6_at."""
    c = F32
    s12, d12, s34, d34 = m[1] + m[2], m[1] - m[2], m[3] + m[4], m[3] - m[4]
    if mt == 4:
        return [m[0] + s12 + s34, d12 + c(2) * d34, s12 + c(4) * s34, d12 + c(8) * d34 + m[5]]
    s56, d56 = m[5] + m[6], m[5] - m[6]
    return [m[0] + s12 + s34 + s56, d12 + c(2) * d34 + c(0.5) * d56, s12 + c(4) * s34 + c(0.25) * s56, d12 + c(8) * d34 + c(0.125) * d56,
            s12 + c(16) * s34 + c(0.0625) * s56, d12 + c(32) * d34 + c(0.03125) * d56 + m[7]]


def g_f32(mt, g):
    """w2_g / w6_g; the constants are quotients of floats, as the compiler folds them."""
    c = F32
    t = g[0] + g[2]
    if mt == 4:
        m6 = c(-1) / c(6)
        q = (c(1) / c(24)) * g[0] + (c(1) / c(6)) * g[2]
        h = (c(1) / c(12)) * g[1]
        return [c(0.25) * g[0], m6 * (t + g[1]), m6 * (t - g[1]), q + h, q - h, g[2]]
    m29 = c(-2) / c(9)
    q = (c(1) / c(90)) * g[0] + (c(2) / c(45)) * g[2]
    r = (c(32) / c(45)) * g[0] + (c(8) / c(45)) * g[2]
    h, k = (c(1) / c(45)) * g[1], (c(16) / c(45)) * g[1]
    return [g[0], m29 * (t + g[1]), m29 * (t - g[1]), q + h, q - h, r + k, r - k, g[2]]


def a_f32(mt, d):
    """w2_a / w6_a."""
    c = F32
    if mt == 4:
        s02, s13, t02, t13 = d[0] + d[2], d[1] + d[3], d[0] + c(4) * d[2], c(2) * d[1] + c(8) * d[3]
        return [d[0], s02 + s13, s02 - s13, t02 + t13, t02 - t13, d[3]]
    ev, od = d[0] + d[2] + d[4], d[1] + d[3] + d[5]
    ev2, od2 = d[0] + c(4) * d[2] + c(16) * d[4], c(2) * d[1] + c(8) * d[3] + c(32) * d[5]
    ev3, od3 = d[0] + c(0.25) * d[2] + c(0.0625) * d[4], c(0.5) * d[1] + c(0.125) * d[3] + c(0.03125) * d[5]
    return [d[0], ev + od, ev - od, ev2 + od2, ev2 - od2, ev3 + od3, ev3 - od3, d[5]]


def gt_f32(mt, p):
    """w2_gt / w6_gt."""
    c = F32
    if mt == 4:
        s12, d12, s34, d34 = p[1] + p[2], p[2] - p[1], p[3] + p[4], p[3] - p[4]
        c6 = c(1) / c(6)
        return [c(0.25) * p[0] - c6 * s12 + (c(1) / c(24)) * s34, c6 * d12 + (c(1) / c(12)) * d34, -c6 * s12 + c6 * s34 + p[5]]
    s12, d12, s34, d34, s56, d56 = p[1] + p[2], p[1] - p[2], p[3] + p[4], p[3] - p[4], p[5] + p[6], p[5] - p[6]
    c29 = c(2) / c(9)
    return [p[0] - c29 * s12 + (c(1) / c(90)) * s34 + (c(32) / c(45)) * s56,
            -c29 * d12 + (c(1) / c(45)) * d34 + (c(16) / c(45)) * d56,
            -c29 * s12 + (c(2) / c(45)) * s34 + (c(8) / c(45)) * s56 + p[7]]


def _two_pass(fn, mt, d, n_in, n_out):
    """fn along the first tile axis for every column, then along the second for every row (k_w2d_input, k_w2d_dy): d [T][n_in][n_in][C]
    -> [n_out^2][T][C]."""
    w = [[None] * n_in for _ in range(n_out)]
    for j in range(n_in):
        v = fn(mt, [d[:, i, j] for i in range(n_in)])
        for i in range(n_out):
            w[i][j] = v[i]
    out = []
    for i in range(n_out):
        out.extend(fn(mt, w[i]))
    return np.stack(out)


def input_planes_f32(mt, x):
    """k_w2d_input: V [NX][T][C] of x [N][H][W][C] float32."""
    return _two_pass(bt_f32, mt, tile_windows(mt, x.astype(F32)), nt_of(mt), nt_of(mt))


def dy_planes_f32(mt, dy):
    """k_w2d_dy: E [NX][T][C]."""
    return _two_pass(a_f32, mt, tile_windows(mt, dy.astype(F32), halo=False), mt, nt_of(mt))


def filter_planes_f32(mt, w):
    """k_w2d_weight: U [NX][Cout][Cin] of w [Cout][3][3][Cin]: G along ky for every kx, then along kx."""
    n = nt_of(mt)
    w = w.astype(F32)
    a = [[None] * 3 for _ in range(n)]
    for kx in range(3):
        u = g_f32(mt, [w[:, 0, kx], w[:, 1, kx], w[:, 2, kx]])
        for p in range(n):
            a[p][kx] = u[p]
    out = []
    for p in range(n):
        out.extend(g_f32(mt, a[p]))
    return np.stack(out)


def _seq_matmul(a, b):
    """sum_k a[.., k] * b[k, ..] accumulated in fp32 one k after the other (one fused multiply-add each, as an MFMA chain without a K split:
    the longest chain any plan produces)."""
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=F32)
    for k in range(a.shape[1]):
        acc = (acc.astype(np.float64) + a[:, k, None].astype(np.float64) * b[None, k].astype(np.float64)).astype(F32)
    return acc


def output_f32(mt, m, N, H, W):
    """k_w2d_output without bias: for every column j of the product tile A^T along the rows, then its contribution A^T[.][j] to the MT output
    columns, added in the order of j.  m [NX][T][C] float32 -> y [N][H][W][C]."""
    n = nt_of(mt)
    o = [[None] * mt for _ in range(mt)]
    for j in range(n):
        z = at_f32(mt, [m[i * n + j] for i in range(n)])
        for i in range(mt):
            for jj in range(mt):
                cf = AT[mt][jj, j]
                if cf != 0:
                    t = F32(cf) * z[i]                    # powers of two: exact
                    o[i][jj] = t if o[i][jj] is None else o[i][jj] + t
    th, tw = cdiv(H, mt), cdiv(W, mt)
    y = np.stack([np.stack(r, 1) for r in o], 1)          # [T][mt][mt][C]
    y = y.reshape(N, th, tw, mt, mt, -1).transpose(0, 1, 3, 2, 4, 5).reshape(N, th * mt, tw * mt, -1)
    return y[:, :H, :W]


def forward_chain_f32(mt, x, w):
    """y [N][H][W][Cout] of x [N][H][W][Cin], w [Cout][3][3][Cin] (no bias) through V = B^T d B, U = G g G^T, a sequential K chain per
    transform index and y = A^T m A, all in fp32."""
    N, H, W, _ = x.shape
    V, U = input_planes_f32(mt, x), filter_planes_f32(mt, w)
    m = np.stack([_seq_matmul(V[xi], U[xi].T.copy()) for xi in range(nx_of(mt))])
    return output_f32(mt, m, N, H, W)


def wgrad_chain_f32(mt, x, dy):
    """dW [Cout][3][3][Cin] through E = A dy A^T, V = B^T d B, P_xi = E_xi^T V_xi summed over the tiles one after the other in fp32, and
    k_w2d_wgrad_out: G^T along the second index of xi, then along the first."""
    n = nt_of(mt)
    V, E = input_planes_f32(mt, x), dy_planes_f32(mt, dy)
    P = [_seq_matmul(E[xi].T.copy(), V[xi]) for xi in range(nx_of(mt))]                 # [Cout][Cin] each
    t = [gt_f32(mt, P[a * n:(a + 1) * n]) for a in range(n)]
    dw = np.empty((P[0].shape[0], 3, 3, P[0].shape[1]), dtype=F32)
    for kx in range(3):
        w3 = gt_f32(mt, [t[a][kx] for a in range(n)])
        for ky in range(3):
            dw[:, ky, kx] = w3[ky]
    return dw


# (N, H, W, C) of the restatement; K is the chain's depth: input channels (forward), dy channels (data-grad) or tiles (weight-grad).
# forward / data-grad: 13 x 11 pixels, ragged for both tiles in both directions, rows no longer than most rows of the GPU cases so that
# averaging does not flatter the worst-row figure; 32 output channels.  weight-grad: one row of K tiles, 16 x 16 channels.
def measure_chain(kind, mt, K, seed=0):
    """(whole-tensor, worst-row) relative L2 rounding error of the fp32 restatement against fp64, on the data the GPU tests use (post-ReLU
    activations, He-scaled filters, standard-normal dy)."""
    rng = np.random.default_rng(seed + 17 * mt + K)
    if kind == "wgrad":
        H, W, Cin, Cout = 2 * mt - 1, (K // 2) * mt - 1, 16, 16                          # 2 x K/2 tiles, the last row and column ragged
        x = np.maximum(rng.standard_normal((1, H, W, Cin)), 0).astype(F32)
        dy = rng.standard_normal((1, H, W, Cout)).astype(F32)
        ref = conv_wgrad_ref(torch.from_numpy(x), torch.from_numpy(dy)).numpy()
        got = wgrad_chain_f32(mt, x, dy)
        return rel_l2(got, ref), worst_row_rel_l2(got, ref)
    H, W, Cout = 13, 11, 32
    x = rng.standard_normal((1, H, W, K))
    x = (x if kind == "dgrad" else np.maximum(x, 0)).astype(F32)                         # the data-grad's input is dy, not an activation
    w = (rng.standard_normal((Cout, 3, 3, K)) * math.sqrt(2.0 / (9 * K))).astype(F32)
    ref = conv_fwd_ref(torch.from_numpy(x), torch.from_numpy(w))[0].numpy()
    got = forward_chain_f32(mt, x, w)[0]
    return rel_l2(got, ref), worst_row_rel_l2(got, ref)


DEPTHS = {"fwd": (32, 512), "dgrad": (32, 512), "wgrad": (32, 512)}        # the two depths of MEASURED: the range of the case tables

# Measured by tests/test_wino2d_ref_cpu.py::test_chain_rounding (which asserts that a fresh measurement reproduces them within 10 %):
# (whole, worst row) at the two depths.  profiles/wino2d_margins.txt records them with the bounds.
MEASURED = {
    ("fwd", 4, 32): (9.232e-07, 1.717e-06), ("fwd", 4, 512): (3.122e-06, 5.452e-06),
    ("fwd", 6, 32): (2.131e-06, 4.670e-06), ("fwd", 6, 512): (6.554e-06, 1.227e-05),
    ("dgrad", 4, 32): (1.148e-06, 2.149e-06), ("dgrad", 4, 512): (3.837e-06, 7.076e-06),
    ("dgrad", 6, 32): (2.257e-06, 4.246e-06), ("dgrad", 6, 512): (8.189e-06, 1.515e-05),
    ("wgrad", 4, 32): (1.051e-06, 1.347e-06), ("wgrad", 4, 512): (3.641e-06, 4.636e-06),
    ("wgrad", 6, 32): (2.136e-06, 2.740e-06), ("wgrad", 6, 512): (6.901e-06, 9.244e-06),
}
# the forward chain at the depths tests/test_gpu_w6.py quotes (1.4e-6 / 2.7e-6 and 2.7e-6 / 5.1e-6 there, on another shape and seed)
MEASURED_W6_DOC = {(4, 64): 1.282e-06, (4, 256): 2.450e-06, (6, 64): 2.913e-06, (6, 256): 4.612e-06}


def wgrad_depth(mt, case):
    """Depth of the weight-grad's longest accumulation chain in tiles: the slices of the longest of the f ranges, plus the f planes that
    k_w2d_wgrad_out adds one after the other."""
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    p = plan_wgrad(mt, tiles(mt, N, H, W), Cin_pad, Cout)
    return 32 * cdiv(p["nK"], p["f"]) + p["f"]


def bound(kind, mt, K, which):
    """3 x (weight-grad: 6 x, the further factor 2 of tests/test_gpu_w6.py) the restatement's error at depth K, interpolated between the two
    measurements as a power of K (clamped to the measured range); which: 0 whole tensor, 1 worst row."""
    k0, k1 = DEPTHS[kind]
    e0, e1 = MEASURED[(kind, mt, k0)][which], MEASURED[(kind, mt, k1)][which]
    p = math.log(e1 / e0) / math.log(k1 / k0)
    K = min(max(K, k0), k1)
    return (6.0 if kind == "wgrad" else 3.0) * e0 * (K / k0) ** p
