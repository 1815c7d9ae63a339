"""Host packs, integer restatements of the host dispatch, an fp32 restatement of the accumulation chains and the case tables for the direct
fp32 conv kernels of csrc/conv3x3.hip: k_conv3x3_igemm (cvk_conv3x3_fwd, forward and data-grad), k_conv3x3_wgrad / k_wgrad_smallco
(cvk_conv3x3_wgrad) and the two weight packs.  They replace nn.Conv2d(cin, cout, 3, padding=1).  No GPU and no library:
tests/test_direct_conv_ref_cpu.py checks this file against torch.nn.functional, tests/test_gpu_direct_conv.py checks the kernels against it.

The fp64 references are those of tests/wino1d_ref.py.  Layouts are the C ABI's (include/cvk.h): activations NHWC, filters [Cout][3][3][Cin]."""
import math

import numpy as np
import torch

from tests.wino1d_ref import (BK, GUARD, STAT_ROWS, cdiv, chan_combine, conv_dgrad_ref, conv_fwd_ref, conv_wgrad_ref,  # noqa: F401
                              rel_l2, stat_partials_ref, worst_row_rel_l2)


def pad4(c):
    return cdiv(c, 4) * 4


# ------------------------------------------------------------------------------------------------------------------ host packs
def pack_fwd_ref(w, Cin_pad):
    """cvk_pack_weight_fwd: w [Cout][3][3][Cin] -> [Cout][9][Cin_pad], channels [Cin, Cin_pad) zero."""
    Cout, Cin = w.shape[0], w.shape[-1]
    dst = torch.zeros(Cout, 9, Cin_pad, dtype=w.dtype)
    dst[:, :, :Cin] = w.reshape(Cout, 9, Cin)
    return dst


def pack_dgrad_ref(w, Cin_pad, Cout_pad):
    """cvk_pack_weight_dgrad: w [Cout][3][3][Cin] -> [Cin_pad][9][Cout_pad] with dst[ci][t][co] = w[co][8-t][ci], pads zero."""
    Cout, Cin = w.shape[0], w.shape[-1]
    src = w.reshape(Cout, 9, Cin)
    dst = torch.zeros(Cin_pad, 9, Cout_pad, dtype=w.dtype)
    for t in range(9):
        dst[:Cin, t, :Cout] = src[:, 8 - t, :].t()
    return dst


# --------------------------------------------------------------------------------------- integer restatements of the host dispatch
WGS_BLOCKS = 512        # csrc/conv3x3.hip: slabs of k_wgrad_smallco


def fwd_tile(ldy):
    """CVK_CONV_LAUNCH of cvk_conv3x3_fwd: the tile follows the output pitch, not Cout."""
    return (128, 128) if ldy > 64 else ((128, 64) if ldy > 32 else (256, 32))


def choose_splits(tiles, M):
    """csrc/conv_tile.h, line by line."""
    max_splits = max(M // (BK * 16), 1)
    best, best_eff = 1, -1.0
    s = 1
    while s <= max_splits and s <= 2048:
        blocks = tiles * s
        if blocks > 4096 and s > 1:
            break
        if not (blocks < 512 and s < max_splits):
            eff = blocks / (256.0 * ((blocks + 255) // 256))
            if eff > best_eff + 0.02:
                best_eff, best = eff, s
        s += 1
    return best


def plan_wgrad(M, Cin_pad, Cout):
    """csrc/conv_tile.h: tile by Cout (and the 64x64 tile for the stem's 36 columns), pixel ranges of `chunk` rows, a multiple of BK."""
    Ktot = 9 * Cin_pad
    if Cout > 64:
        bm, bn = 128, 128
    elif Cout > 32:
        bm, bn = 64, (64 if Ktot <= 64 else 128)
    else:
        bm, bn = 32, 256
    tilesM, tilesN = cdiv(Cout, bm), cdiv(Ktot, bn)
    splits = choose_splits(tilesM * tilesN, M)
    chunk = cdiv(cdiv(M, splits), BK) * BK
    splits = cdiv(M, chunk)
    return dict(bm=bm, bn=bn, tilesM=tilesM, tilesN=tilesN, splits=splits, chunk=chunk, last=M - (splits - 1) * chunk)


def wgrad_smallco(Cin, Cin_pad, Cout):
    return Cout <= 16 and Cin == 64 and Cin_pad == 64


def wgrad_workspace_bytes(N, H, W, Cin_pad, Cout):
    """cvk_conv3x3_wgrad_workspace_bytes: the slabs of the plan, or the 512 slabs of k_wgrad_smallco where that kernel can be chosen."""
    p = plan_wgrad(N * H * W, Cin_pad, Cout)
    need = p["splits"] * Cout * 9 * Cin_pad * 4
    small = WGS_BLOCKS * Cout * 9 * Cin_pad * 4 if wgrad_smallco(Cin_pad, Cin_pad, Cout) else 0
    return max(need, small)


def arm_of(kind, case, stats=False):
    """Names the instantiation a case runs.
    kind "fwd",   case (N,H,W,Cin,Cout[,ldy]):              (BM, BN, STATS, CIN32) of k_conv3x3_igemm
    kind "wgrad", case (N,H,W,Cin,Cin_pad,Cout,ld_dy):      ("smallco" | (BM, BN) of k_conv3x3_wgrad, (splits, chunk, rows of the last split));
        for "smallco" the plan is the one the workspace query is sized by, the kernel itself cuts the rows of the images into units."""
    if kind == "fwd":
        Cin, Cout = case[3], case[4]
        ldy = case[5] if len(case) > 5 else Cout
        return fwd_tile(ldy) + (bool(stats), Cin % 32 == 0)
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    p = plan_wgrad(N * H * W, Cin_pad, Cout)
    tile = "smallco" if wgrad_smallco(Cin, Cin_pad, Cout) else (p["bm"], p["bn"])
    return tile, (p["splits"], p["chunk"], p["last"])


def fwd_edges(case):
    """What the K loop and the tile walk of k_conv3x3_igemm meet at a case."""
    N, H, W, Cin, Cout = case[:5]
    ldy = case[5] if len(case) > 5 else Cout
    BM, BN = fwd_tile(ldy)
    M, Ktot = N * H * W, 9 * Cin
    nK = cdiv(Ktot, BK)
    generic = Cin % 32 != 0
    # a slice [32s, 32s+32) that holds elements of more than one filter tap (generic arm only: Cin % 32 == 0 aligns slices to taps)
    straddle = generic and any((BK * s) // Cin != min(BK * s + BK - 1, Ktot - 1) // Cin for s in range(nK))
    return dict(BM=BM, BN=BN, nK=nK, generic=generic, partial_k=Ktot % BK != 0, straddle=straddle,
                taps_per_slice=max(((min(BK * s + BK, Ktot) - 1) // Cin - (BK * s) // Cin + 1) for s in range(nK)),
                tilesM=cdiv(M, BM), tilesN=cdiv(ldy, BN),
                pb=cdiv(M, BM) > 1 and BM > W + 1,                 # max(m0 - W - 1, 0) > 0 for the second row tile
                ragged_m=M % BM != 0, ragged_n=Cout % BN != 0, ragged_second_column=cdiv(ldy, BN) > 1 and Cout % BN != 0,
                ld_pad=ldy > Cout, images_per_tile=cdiv(BM, H * W) + 1 if H * W < BM else 1)


def wgrad_edges(case):
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    tile, (splits, chunk, last) = arm_of("wgrad", case)
    p = plan_wgrad(N * H * W, Cin_pad, Cout)
    return dict(tile=tile, splits=splits, chunk=chunk, last=last, ragged_split=splits >= 2 and last != chunk, raster_wrap=H * W < BK,
                cin_pad=Cin < Cin_pad, ld_pad=ld_dy > Cout, ragged_m=Cout % p["bm"] != 0, ragged_n=(9 * Cin_pad) % p["bn"] != 0)


# -------------------------------------------------------------------------------------------------------------------- case tables
# forward (N, H, W, Cin, Cout[, ldy]) -> the tile and CIN32 the case is there for; each runs with and without stats, with and without bias
FWD_CASES = {
    (3, 19, 23, 32, 64): (128, 64, True),         # nK = 9 (odd tail step); 11 row tiles: pb > 0, ragged last tile, tiles cross rows and images
    (3, 19, 23, 64, 160): (128, 128, True),       # ragged second column tile
    (2, 17, 31, 96, 48): (128, 64, True),         # nK = 27; Cout ragged in a 64 tile
    (2, 17, 31, 32, 96): (128, 128, True),        # Cout < BN
    (3, 19, 23, 4, 64): (128, 64, False),         # generic arm, Ktot = 36: a slice spans 8 taps, nK = 2
    (5, 1, 37, 12, 64): (128, 64, False),         # generic arm, H = 1
    (4, 41, 1, 20, 36): (128, 64, False),         # generic arm, W = 1, Ktot = 180
    (3, 19, 23, 48, 24): (256, 32, False),        # generic arm, Ktot = 432: partial last slice
    (1, 1, 1, 64, 64): (128, 64, True),           # single pixel
    (2, 9, 13, 64, 64, 68): (128, 128, True),     # ldy crosses a dispatch boundary while Cout does not; columns [Cout, ldy) read 0
    (2, 9, 13, 32, 32, 36): (128, 64, True),      # the same at the lower boundary
    (40, 3, 5, 64, 20): (256, 32, True),          # a 256-row tile spans 17 images
    (2, 9, 13, 36, 12): (256, 32, False),         # generic arm where a slice straddles a tap
    (2, 9, 13, 20, 72): (128, 128, False),        # generic arm in the 128x128 tile (the table above leaves it open), Cout < BN
}
# data-grad: the layer Conv2d(Cin -> Cout) as (N, H, W, Cin, Cout); runs cvk_pack_weight_dgrad(w, Cin_pad = pad4(Cin), Cout_pad = pad4(Cout)) and
# cvk_conv3x3_fwd(dy, packed, NULL, dx, NULL, N, H, W, pad4(Cout), pad4(Cin), pad4(Cin)) as the engine does
DGRAD_CASES = [
    (2, 9, 13, 64, 12),        # the head: reduces over 12 channels (generic arm), 128x64 tile
    (3, 19, 23, 4, 64),        # source pitch 4: 256x32 tile
    (2, 17, 31, 96, 40),       # generic arm, 128x128 tile
    (2, 17, 31, 32, 160),      # CIN32, 256x32 tile, nK = 45
    (2, 9, 13, 3, 38),         # both pitches padded: column 3 of dx reads 0, columns 38, 39 of dy hold a finite value the zero filter rows cancel
]
# weight-grad (N, H, W, Cin, Cin_pad, Cout, ld_dy) -> the arm
WGRAD_CASES = {
    (2, 9, 13, 32, 32, 12, 12): (32, 256),         # one split
    (3, 19, 23, 48, 48, 24, 24): (32, 256),        # 2 splits, last split of 639 rows
    (40, 3, 5, 64, 64, 20, 20): (32, 256),         # HW < BK: the raster walk wraps by modulo
    (3, 19, 23, 3, 4, 64, 64): (64, 64),           # the stem: Cin < Cin_pad, the pad channel of x holds a large finite value
    (3, 19, 23, 3, 4, 40, 40): (64, 64),           # the same, ragged in Cout
    (3, 19, 23, 32, 32, 64, 64): (64, 128),
    (2, 17, 31, 96, 96, 48, 48): (64, 128),        # ragged in Cout, 7 column tiles (the last ragged)
    (2, 17, 31, 32, 32, 96, 96): (128, 128),       # ragged in Cout
    (3, 19, 23, 64, 64, 160, 160): (128, 128),     # two row tiles, the second ragged
    (1, 1, 1, 64, 64, 64, 64): (64, 128),          # single pixel
    (5, 1, 37, 12, 12, 64, 64): (64, 128),         # H = 1
    (4, 41, 1, 20, 20, 36, 36): (64, 128),         # W = 1
    (2, 24, 40, 64, 64, 64, 64): (64, 128),        # the 64 -> 64 layer the router sends here: 3 equal splits of 640
    (2, 9, 13, 32, 32, 38, 40): (64, 128),         # ld_dy > Cout: zero pad columns, the last 16-byte vector of a dy row straddles Cout
    (2, 9, 13, 64, 64, 12, 12): "smallco",         # the arm tests/test_gpu_blocks.py checks
}

FWD_ARMS = {(bm, bn, st, c32) for bm, bn in ((128, 128), (128, 64), (256, 32)) for st in (False, True) for c32 in (False, True)}   # 12
WGRAD_ARMS = {(128, 128), (64, 64), (64, 128), (32, 256), "smallco"}


# ------------------------------------------------------------------------------- fp32 restatement of the accumulation chains
# Forward / data-grad: every output is ONE chain over K = 9 Cin in the order k = tap * Cin + ci; each step rounds the product to fp32 and then
# the sum (no fused multiply-add: one rounding more per step than the matrix cores need, so the restatement errs on the large side).
# Weight-grad: the same chain over the pixels of one split (`chunk` rows), then the slabs added one after the other.
def _chain(a, b):
    """sum_k a[:, k, None] * b[None, k, :] in fp32, one k after the other, product and sum rounded separately."""
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    for k in range(a.shape[1]):
        acc = acc + a[:, k, None] * b[None, k]
    return acc


def im2col(x):
    """A [N*H*W][9*Cin] of x [N][H][W][Cin]: column tap * Cin + ci is the pixel shifted by tap (zero outside the frame)."""
    N, H, W, C = x.shape
    xp = np.zeros((N, H + 2, W + 2, C), dtype=x.dtype)
    xp[:, 1:H + 1, 1:W + 1] = x
    cols = [xp[:, r:r + H, s:s + W] for r in range(3) for s in range(3)]
    return np.stack(cols, axis=3).reshape(N * H * W, 9 * C)


def forward_chain_f32(x, w):
    """y [N][H][W][Cout] of x [N][H][W][Cin], w [Cout][3][3][Cin] (no bias)."""
    f = np.float32
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    return _chain(im2col(x.astype(f)), w.astype(f).reshape(Cout, 9 * Cin).T.copy()).reshape(N, H, W, Cout)


def wgrad_chain_f32(x, dy, chunk):
    """dW [Cout][3][3][Cin] of x [N][H][W][Cin], dy [N][H][W][Cout]: one slab per `chunk` pixels, slabs added in order."""
    f = np.float32
    Cin, Cout = x.shape[3], dy.shape[3]
    A = im2col(x.astype(f))
    d = dy.astype(f).reshape(-1, Cout)
    dw = None
    for m0 in range(0, A.shape[0], chunk):
        slab = _chain(d[m0:m0 + chunk].T.copy(), A[m0:m0 + chunk])
        dw = slab if dw is None else dw + slab
    return dw.reshape(Cout, 3, 3, Cin)


# forward / data-grad: 12 rows of 11 pixels x 32 channels (the scale of wino1d_ref.MEASURE_SHAPE).  weight-grad: 19 x 69 = 1311 pixels in two
# splits of 672 and 639 rows, the longest pixel chain and the most slabs after it of any case above but (2, 24, 40, ...) with its 3 x 640.
MEASURE_SHAPE = {"fwd": (12, 11, 32), "dgrad": (12, 11, 32), "wgrad": (19, 69, 16)}
MEASURE_CHUNK = 672


def measure_chain(kind, Cin, seed=0):
    """(whole-tensor, worst-row) relative L2 rounding error of the fp32 restatement against fp64 on the data the GPU tests use (post-ReLU
    activations, He-scaled filters, standard-normal dy).  kind "dgrad": the forward chain on a standard-normal input, Cin the channel
    count it reduces over (the layer's padded Cout)."""
    rng = np.random.default_rng(seed + 31 + Cin)
    H, W, Cout = MEASURE_SHAPE[kind]
    x = rng.standard_normal((1, H, W, Cin))
    x = (x if kind == "dgrad" else np.maximum(x, 0)).astype(np.float32)
    if kind != "wgrad":
        w = (rng.standard_normal((Cout, 3, 3, Cin)) * math.sqrt(2.0 / (9 * Cin))).astype(np.float32)
        ref = conv_fwd_ref(torch.from_numpy(x), torch.from_numpy(w))[0].numpy()
        got = forward_chain_f32(x, w)[0]
    else:
        dy = rng.standard_normal((1, H, W, Cout)).astype(np.float32)
        ref = conv_wgrad_ref(torch.from_numpy(x), torch.from_numpy(dy)).numpy()
        got = wgrad_chain_f32(x, dy, MEASURE_CHUNK)
    return rel_l2(got, ref), worst_row_rel_l2(got, ref)


# Measured by tests/test_direct_conv_ref_cpu.py::test_chain_rounding (which asserts that a fresh measurement reproduces them within 10 %):
# (whole, worst row) at Cin = 64 and Cin = 512.  profiles/direct_conv_margins.txt records them with the bounds.
MEASURED = {
    ("fwd", 64): (2.888e-07, 3.202e-07), ("fwd", 512): (8.487e-07, 9.396e-07),
    ("dgrad", 64): (4.138e-07, 4.552e-07), ("dgrad", 512): (1.211e-06, 1.351e-06),
    ("wgrad", 64): (3.035e-07, 3.925e-07), ("wgrad", 512): (2.943e-07, 3.836e-07),
}


def bound(kind, Cin, which):
    """3 x (weight-grad: 6 x) the restatement's error at Cin, interpolated between the measurements at 64 and 512 as a power of Cin (the
    forward chain grows roughly as sqrt(Cin), the weight-grad chain runs over pixels and does not depend on it); which: 0 whole tensor, 1
    worst row (image row of y, output channel of dW)."""
    e64, e512 = MEASURED[(kind, 64)][which], MEASURED[(kind, 512)][which]
    p = math.log(e512 / e64) / math.log(8.0)
    return (6.0 if kind == "wgrad" else 3.0) * e64 * (Cin / 64.0) ** p
