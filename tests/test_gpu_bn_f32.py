"""The fp32 BatchNorm passes of csrc/bn.hip called directly through the C ABI, each dispatch arm by a named case, against high-precision
restatements: tests/elem_bf16_ref.py (apply, pool2x2, bn_bwd_terms, bn_bwd_dy: they work for any storage type) and tests/bn_f32_ref.py
(statistics finalisation, eval parameters, E planes, padded plane layout), whose own correctness and the conditions assumed of the
inputs here tests/test_bn_f32_ref_cpu.py checks without a GPU.  Buffers, views and the case seeds are those of
tests/test_gpu_elem_bf16.py.

Conventions of every test:
  * inputs come from seeded generators (case_seed(name));
  * every output lives in a buffer with a guard of 64 elements before and after it, pre-filled with the fp32 NaN pattern 0x7FC00001 (0xEE
    for the arg-max bytes).  After the call every element the contract does not write (guards, channels [C, ld), the other channels of a
    wider buffer, the frame round a spatial window, the pad rows of the padded plane layout) must still hold exactly those bits, and
    every element it does write must be finite;
  * input pad columns (ldy > C) hold NaN: a read of them would surface in the finite check.

Tolerances are derived, none is measured.  u = 2^-24.
  statistics (reference: the same combination of the rounded fp32 partials in longdouble, so the difference is the kernel's fp64
  arithmetic and one rounding to fp32; P partials, S = sum s_p):
      mean      u |ref| + P 2^-52 sum|s_p| / M
      dvar      P 2^-52 (sum q_p + sum s_p^2/n_p + S^2/M) / M       the three sums of m2, each of at most P terms.  Counting every rounding
                (two per product s_p^2/n_p, the additions, S^2/M, the two differences) gives (P + 5) 2^-53, which P 2^-52 covers from
                P = 5 on; below that the count exceeds it by at most 2 2^-52 of a quantity that the fp32 rounding term beside it
                dwarfs by 2^28, so the bound is kept as stated
      rstd      u |ref| + ref^3 dvar / 2                            d/dv (v + eps)^-1/2
      scale     2u |ref| + |gamma| tol(rstd)                        the product's rounding and one to spare
      shift     3u (|beta| + |mean scale|) + |scale| tol(mean) + |mean| tol(scale) + tol(mean) tol(scale)
      running   3u (|(1 - m) old| + |m new|) + m tol(new)           fl(1 - m), product, sum; new = the fp32 mean, or the fp32 unbiased
                                                                    variance with tol = u |ref| + dvar M/(M - 1)
      num_batches_tracked   exactly old + 1
  second assertion of the cases drawn from a tensor, against the fp64 mean and biased variance of the tensor itself: the above plus
  the rounding of the partials to fp32, u sum|s_p| / M on the mean and u (sum q_p + 2 sum s_p^2/n_p) / M on the variance.  (To first
  order a rounding of s_p moves m2 by 2 ds_p (s_p/n_p - S/M); the stated bound dominates that when sum|s_p| (|mean_p - mean| - |mean_p|)
  <= 0, which the CPU file asserts of every case.)  The variance bound can exceed var + eps (the ill-conditioned case), where a
  first-order rstd bound means nothing: the assertion is the exact interval rstd(var + d) (1 - u) <= got <= rstd(max(var - d, 0)) (1 + u).
  eval parameters: rstd 2u |ref|: the sum rv + eps contributes u/2, and the significands of sqrt(x) and 1/sqrt(x) multiply to 2 (or
  both are 1), so their two half-ulps are at most 1.5u of the values together.
  apply      3u (|y scale| + |shift|) + u |ref|
  dy         6u |scale| (|g| + |dbeta|/M + |xhat dgamma|/M) + u |ref|
  column sums (partials finalised by cvk_colsum_finalize)   (ceil(rows/ppp) + ppp + 8) u sum|term| per channel with rows = ceil(M/PB),
             PB = cvk_bn_bwd_blocks(M), ppp = 256 // (cw/V), cw the width of the channel's column chunk (1024 four-wide, 256 scalar)
  E passes   part: (4 ceil(tiles/ppp) + ppp + 8) u sum|dy|, tiles = ceil(Mt/PB) column groups per block, cvk_bn_bwd_e_blocks rows;
             planes: sum|coef_i| tol(dy_i) + 4u sum|coef_i dy_i|
  cvk_colsum_finalize_batch   u |ref| + 2^-52 PB sum|term|; bitwise equal to cvk_colsum_finalize
  pool and arg-max code of the fused apply: bitwise functions of the kernel's OWN `out`.

Excluded elements: an element whose fp64 z lies in the band of elem_bf16_ref.bn_bwd_terms may have its mask decided either way; it is
left out of the dy (and E) comparison and its column out of the sums.  At most min(8, int(1e-5 numel)) per case, else the test fails;
the CPU file asserts that no case here has any.  Exact zeros (channel 0: shift = 0, every third y = 0) are NOT excluded.
test_one_relu_decision_forward_and_backward places inputs INSIDE the band and needs neither reference nor exclusion.

Dispatch arms against cases (instantiations read off the dispatch code of bn.hip):
  k_bn_stats_l1 + k_bn_stats_l2          STAT every case through cvk_bn_finalize: G = 1 (P < 32 and P = 33), G = 3 (p100), G = 64 (p2100_synthetic);
                                         two-chain loop entered from P = 5 on, its tail by every P but 8
  k_bn_stats_l1_counts + k_bn_stats_l2   the same cases through cvk_bn_finalize_counts (granule counts: bitwise; ragged counts: to tolerance)
  k_bn_eval_params                       test_bn_eval_params C in {1, 255, 256, 257}
  k_bn_relu_apply<4>                     APPLY v4_dense, v4_ldy32_c24, v4_slice128, v4_window
  k_bn_relu_apply<1>                     APPLY v1_c5_ldy8, v1_c64_ldy66, v1_c64_stride66, v1_c12_scale_off4
  k_bn_relu_apply_pool                   POOL pool_odd_slice, pool_c20, pool_one_cell
  k_bn_bwd<4,0> / k_bn_bwd<4,1>          BN v4_* through cvk_bn_bwd_reduce / cvk_bn_bwd_dx
  k_bn_bwd<1,0> / k_bn_bwd<1,1>          BN v1_*
  k_bn_bwd_dx_e   six_H == 0             E e_w13_c64, e_w7_c12_ld16, e_w52_c64, e_w4_c1028 (cvk_bn_bwd_dx_e)
                  six_rows > 0 / < 0     E6 e6_w12_c64, e6_w13_c64 through cvk_bn_bwd_dx_e6 / cvk_bn_bwd_dx_e4p
  k_colsum_finalize                      every column-sum check; k_colsum_finalize_batch: test_colsum_finalize_batch"""
import ctypes

import numpy as np
import pytest
import torch

from tests import bn_f32_ref as S
from tests import elem_bf16_ref as R
from tests import test_gpu_elem_bf16 as G
from tests.test_gpu_elem_bf16 import Box, Lay, case_seed, dev, excluded_cap, libs, rows_padded, stream, worst_fraction

pytestmark = pytest.mark.gpu
U = R.U32
LD = S.LD
SENT32 = G.SENT32
SENT8 = 0xEE
GUARD = G.GUARD
EPS = 1e-5
MOMENTUM = 0.1
EINVAL, EWORKSPACE = -1, -2


# ------------------------------------------------------------------------------------------------ shared: generators and cases
def bn_inputs(shape, seed):
    """bn_inputs of tests/test_gpu_elem_bf16.py with y and dout left in fp32: [M, C] row-major over (N,H,W) and per-channel fp32 constants.
    Channel 0 carries the exact-zero edge: shift = 0 and every third y = 0."""
    N, H, W, C = shape
    M = N * H * W
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(M, C, generator=g) * 1.3 + 0.2
    y[::3, 0] = 0.0
    gamma = torch.rand(C, generator=g) + 0.5
    beta = 0.3 * torch.randn(C, generator=g)
    y64 = y.double()
    mean = y64.mean(0).float()
    rstd = (y64.var(0, unbiased=False) + EPS).rsqrt().float()
    scale = gamma * rstd
    shift = beta - mean * scale
    shift[0] = 0.0
    dout = torch.randn(M, C, generator=g)
    return {"y": y, "dout": dout, "scale": scale, "shift": shift, "mean": mean, "rstd": rstd}


DOUT_LAYOUTS = dict(G.DOUT_LAYOUTS, stride66={"ld": 66})

# name: (N,H,W,C), ldy, view of dout, V (the vector width the layout selects)
BN_CASES = {
    "v4_c64_m71": ((1, 1, 71, 64), 64, "dense", 4),                  # ragged last row block (rows 15, last block 11)
    "v4_c12_m70": ((2, 5, 7, 12), 12, "dense", 4),                   # cvn 3, ppp 85, thread 255 idle
    "v1_c5_ldy8": ((2, 5, 7, 5), 8, "dense", 1),
    "v1_c64_ldy66": ((2, 5, 7, 64), 66, "dense", 1),                 # demoted by the pitch of y
    "v1_c64_stride66": ((2, 5, 7, 64), 64, "stride66", 1),           # demoted by the gradient view's sX
    "v1_c301": ((1, 3, 5, 301), 301, "dense", 1),                    # two scalar column chunks: 256 (ppp 1) and 45 (ppp 5, 31 threads idle)
    "v4_c1024": ((1, 3, 5, 1024), 1024, "dense", 4),                 # ppp 1
    "v4_c1028": ((1, 3, 5, 1028), 1028, "dense", 4),                 # second chunk of one vector: ppp 256
    "v4_c8_m19500": ((1, 150, 130, 8), 8, "dense", 4),               # PB 500, rows 39, ppp 128
    "v4_c24_ldy32_slice": ((2, 5, 7, 24), 32, "slice", 4),           # ldy > C, gradient = channel slice of a wider buffer
    "v4_c32_window": ((2, 4, 6, 32), 32, "window", 4),               # gradient = spatial sub-window: the non-linear pixel map
    "v1_c6_window": ((2, 4, 6, 6), 6, "window", 1),
}

# name: (N,H,W,C), ldy, layout of the output view, V, offset of the scale pointer in bytes
APPLY_CASES = {
    "v4_dense": ((2, 5, 7, 64), 64, {}, 4, 0),
    "v4_ldy32_c24": ((2, 5, 7, 24), 32, {}, 4, 0),
    "v4_slice128": ((2, 5, 7, 64), 64, {"ld": 128, "c0": 64}, 4, 0),
    "v4_window": ((2, 4, 6, 32), 32, {"ph": 3, "pw": 4, "y0": 1, "x0": 2}, 4, 0),
    "v1_c5_ldy8": ((2, 5, 7, 5), 8, {}, 1, 0),
    "v1_c64_ldy66": ((2, 5, 7, 64), 66, {}, 1, 0),
    "v1_c64_stride66": ((2, 5, 7, 64), 64, {"ld": 66}, 1, 0),
    "v1_c12_scale_off4": ((2, 5, 7, 12), 12, {}, 1, 4),
}

# name: (N,H,W,C), ldy, layout of the output view
POOL_CASES = {
    "pool_odd_slice": ((1, 9, 7, 64), 64, {"ld": 128, "c0": 64}),    # odd H and W: the trailing row and column go through `out`, feed no cell
    "pool_c20": ((2, 4, 6, 20), 20, {}),
    "pool_one_cell": ((1, 2, 2, 4), 4, {}),
}

# name: (N,H,W,C), ld_dy
E_CASES = {
    "e_w13_c64": ((2, 3, 13, 64), 64),                               # ragged last group (one column)
    "e_w7_c12_ld16": ((1, 5, 7, 12), 16),                            # pad columns of dy and E stay sentinel
    "e_w52_c64": ((1, 3, 52, 64), 64),
    "e_w4_c1028": ((1, 2, 4, 1028), 1028),                           # two column chunks
}
E6_CASES = {"e6_w12_c64": (2, 9, 12, 64), "e6_w13_c64": (2, 9, 13, 64)}

STAT_M = {"m1": 1, "m64": 64, "m71": 71, "p5": 263, "p8": 512, "p9": 513, "p31": 1953, "p33": 2100, "p100": 6353}
STAT_CASES = list(STAT_M) + ["p2100_synthetic"]
STAT_C = (1, 63, 64, 65, 130)
STAT_SPECIAL = ("illcond_m4544", "constant_m71")


def stat_problem(name, C, ragged=False):
    """One statistics case: fp32 partials [2][P][C] with their counts, the tensor they came from (fp64 [M, C]; None for the synthetic
    case), and fp32 gamma, beta, running statistics.  ragged: arbitrary counts summing to M instead of granules of 64."""
    rng = np.random.default_rng(case_seed(f"{name}_c{C}") + (50021 if ragged else 0))
    mu, sd = rng.normal(0.0, 2.0, C), rng.uniform(0.5, 1.5, C)
    y = None
    if name == "p2100_synthetic":
        P = 2100
        counts = [int(v) for v in rng.integers(1, 129, P)] if ragged else [64] * (P - 1) + [40]
        n = np.asarray(counts, dtype=np.float64)[:, None]
        stats = np.stack([n * mu + np.sqrt(n) * sd * rng.normal(size=(P, C)), n * sd * sd * rng.uniform(0.5, 1.5, (P, C))]).astype(np.float32)
        M = int(sum(counts))
    else:
        if name == "illcond_m4544":
            M = 71 * 64
            y = 100.0 + 0.01 * rng.normal(size=(M, C))
        elif name == "constant_m71":
            M = 71
            const = rng.uniform(-3.0, 3.0, C)
            const[0] = 0.0
            y = np.broadcast_to(const, (M, C))
        else:
            M = STAT_M[name]
            y = rng.normal(size=(M, C)) * sd + mu
        y = y.astype(np.float32).astype(np.float64)
        counts = S.granule_counts(M)
        if ragged:
            cuts = np.sort(rng.choice(np.arange(1, M), size=len(counts) - 1, replace=False)) if M > 1 else np.zeros(0, dtype=np.int64)
            counts = [int(v) for v in np.diff(np.concatenate([[0], cuts, [M]]))]
        stats = S.partials(y, counts)
    assert bool((stats[1] >= 0).all()) and min(counts) >= 1
    f = np.float32
    return {"stats": stats, "counts": counts, "M": M, "y": y, "gamma": rng.uniform(0.5, 1.5, C).astype(f), "beta": (0.3 * rng.normal(size=C)).astype(f),
            "running_mean": (0.2 * rng.normal(size=C)).astype(f), "running_var": rng.uniform(0.5, 1.5, C).astype(f)}


# ------------------------------------------------------------------------------------------------ shared: buffers and views
class IBox:
    """Box for integer outputs: n elements of `dtype` between two guards, everything pre-filled with `sent`."""

    def __init__(self, n, dtype, sent):
        self.n, self.sent = n, sent
        self.raw = torch.full((GUARD + n + GUARD,), sent, dtype=dtype, device=dev())
        self.ptr = self.raw.data_ptr() + GUARD * self.raw.element_size()

    def settle(self, written=True):
        torch.cuda.synchronize()
        h = self.raw.cpu()
        assert bool((h[:GUARD] == self.sent).all()) and bool((h[GUARD + self.n:] == self.sent).all()), "a guard was overwritten"
        body = h[GUARD:GUARD + self.n]
        if written is not True:
            assert bool((body[~written.reshape(-1)] == self.sent).all()), "an element outside the contract was written"
        return body


def fbox(n):
    return Box(n, f32=True)


def untouched(box):
    """nothing at all was written"""
    mask = torch.zeros(box.n, dtype=torch.bool)
    if isinstance(box, IBox):
        box.settle(mask)
    else:
        box.settle(mask, finite=False)


def fview(lay, ptr):
    _lib, _ = libs()
    return _lib.View(ptr + lay.offset * 4, *lay.strides)


def cols_mask(rows, ld, C):
    m = torch.zeros(rows, ld, dtype=torch.bool)
    m[:, :C] = True
    return m


def report(entry, case, frac):
    print(f"[bn_f32] {entry} {case}: largest error = {frac:.3f} of its bound")


def d64(inp):
    return {k: v.double() for k, v in inp.items()}


def np_fraction(err, tol):
    """max err/tol of longdouble arrays; a zero bound admits a zero error only"""
    err, tol = np.asarray(err, dtype=LD), np.asarray(tol, dtype=LD)
    assert bool(((tol > 0) | (err == 0)).all()), "a nonzero error where the bound is zero"
    return float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1), 0))) if err.size else 0.0


# ------------------------------------------------------------------------------------------------ 1. statistics
def run_finalize(prob, counts=None, running=True, nbt_old=41):
    """cvk_bn_finalize (counts None) or cvk_bn_finalize_counts on a problem; every output in a guarded buffer.  Returns fp32 numpy arrays."""
    _lib, lib = libs()
    P, C = prob["stats"].shape[1:]
    stats = torch.from_numpy(prob["stats"]).to(dev())
    gamma, beta = torch.from_numpy(prob["gamma"]).to(dev()), torch.from_numpy(prob["beta"]).to(dev())
    out = {k: fbox(C) for k in ("mean", "rstd", "scale", "shift")}
    rm, rv, nbt = fbox(C), fbox(C), IBox(1, torch.int64, -7)
    if running:
        rm.body().copy_(torch.from_numpy(prob["running_mean"]))
        rv.body().copy_(torch.from_numpy(prob["running_var"]))
        nbt.raw[GUARD] = nbt_old
    wsb = lib.cvk_bn_finalize_workspace_bytes(P, C)
    ws = torch.empty(wsb // 8, dtype=torch.float64, device=dev())
    tail = (prob["M"], C, gamma.data_ptr(), beta.data_ptr(), *[out[k].ptr for k in ("mean", "rstd", "scale", "shift")], rm.ptr if running else None,
            rv.ptr if running else None, nbt.ptr if running else None, MOMENTUM, EPS, ws.data_ptr(), wsb, stream())
    if counts is None:
        _lib.check(lib.cvk_bn_finalize(stats.data_ptr(), P, *tail))
    else:
        cnt = torch.tensor(counts, dtype=torch.float32, device=dev())
        _lib.check(lib.cvk_bn_finalize_counts(stats.data_ptr(), cnt.data_ptr(), P, *tail))
    got = {k: b.settle(True)[1].numpy() for k, b in out.items()}
    if running:
        got["running_mean"], got["running_var"] = rm.settle(True)[1].numpy(), rv.settle(True)[1].numpy()
        assert int(nbt.settle()[0]) == nbt_old + 1
    else:
        untouched(rm), untouched(rv), untouched(nbt)
    return got


def stat_bounds(ref, prob):
    """the bounds of the module docstring, longdouble [C] each; also dvar"""
    P, M = len(prob["counts"]), prob["M"]
    u, e52, m = LD(U), LD(2) ** -52, LD(np.float32(MOMENTUM))
    gamma, beta = prob["gamma"].astype(LD), prob["beta"].astype(LD)
    t = {"mean": u * np.abs(ref["mean"]) + P * e52 * ref["abs_s"] / M}
    dvar = P * e52 * ref["var_mag"] / M
    t["rstd"] = u * np.abs(ref["rstd"]) + ref["rstd"] ** 3 * dvar / 2
    t["scale"] = 2 * u * np.abs(ref["scale"]) + np.abs(gamma) * t["rstd"]
    t["shift"] = 3 * u * (np.abs(beta) + np.abs(ref["mean"] * ref["scale"])) + np.abs(ref["scale"]) * t["mean"] + np.abs(ref["mean"]) * t["scale"] + \
        t["mean"] * t["scale"]
    tnew = u * np.abs(ref["unbiased"]) + dvar * (LD(M) / LD(M - 1) if M > 1 else LD(1))
    for k, new, tn in (("running_mean", ref["mean"], t["mean"]), ("running_var", ref["unbiased"], tnew)):
        t[k] = 3 * u * (np.abs((1 - m) * prob[k].astype(LD)) + np.abs(m * new)) + m * tn
    return t, dvar


def check_finalize(entry, case, got, prob, counts):
    ref = S.finalize(prob["stats"], counts, prob["M"], prob["gamma"], prob["beta"], EPS, MOMENTUM, prob["running_mean"], prob["running_var"])
    tol, dvar = stat_bounds(ref, prob)
    for k in ("mean", "rstd", "scale", "shift", "running_mean", "running_var"):
        frac = np_fraction(np.abs(got[k].astype(LD) - ref[k]), tol[k])
        report(entry + " " + k, case, frac)
        assert frac <= 1.0, k
    if prob["y"] is None:
        return ref
    # what the layout MEANS: mean and biased variance of the tensor, up to the rounding of the partials to fp32
    u, M = LD(U), prob["M"]
    y = prob["y"].astype(LD)
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    frac = np_fraction(np.abs(got["mean"].astype(LD) - mean), tol["mean"] + u * ref["abs_s"] / M)
    report(entry + " mean against the tensor", case, frac)
    assert frac <= 1.0
    d = dvar + u * ref["round_mag"] / M
    eps = LD(np.float32(EPS))
    lo, hi = 1 / np.sqrt(var + d + eps) * (1 - u), 1 / np.sqrt(np.maximum(var - d, 0) + eps) * (1 + u)
    r = got["rstd"].astype(LD)
    assert bool(((lo <= r) & (r <= hi)).all()), "rstd outside the interval the tensor's variance allows"
    return ref


@pytest.mark.parametrize("C", STAT_C)
@pytest.mark.parametrize("name", STAT_CASES)
def test_bn_finalize(name, C):
    """cvk_bn_finalize on partials over granules of 64 rows with a ragged last one: every output against the longdouble combination of
    the same fp32 partials and, for cases drawn from a tensor, against the tensor's own fp64 mean and variance (module docstring).
    Without running statistics the four outputs are bitwise the same and nothing else is written; cvk_bn_finalize_counts with the
    granule counts gives bitwise the same as cvk_bn_finalize (1/n_p is exact or the same division either way)."""
    prob = stat_problem(name, C)
    got = run_finalize(prob)
    check_finalize("cvk_bn_finalize", f"{name} C={C}", got, prob, prob["counts"])
    bare = run_finalize(prob, running=False)
    for k in ("mean", "rstd", "scale", "shift"):
        assert np.array_equal(got[k].view(np.int32), bare[k].view(np.int32)), k
    by_counts = run_finalize(prob, counts=prob["counts"])
    for k in got:
        assert np.array_equal(got[k].view(np.int32), by_counts[k].view(np.int32)), k


@pytest.mark.parametrize("C", STAT_C)
@pytest.mark.parametrize("name", STAT_CASES)
def test_bn_finalize_counts_with_ragged_counts(name, C):
    """cvk_bn_finalize_counts with arbitrary counts that sum to M (for the synthetic case: 1..128 rows per partial), same bounds."""
    prob = stat_problem(name, C, ragged=True)
    assert sum(prob["counts"]) == prob["M"] and (prob["M"] <= 64 or prob["counts"] != S.granule_counts(prob["M"]))
    got = run_finalize(prob, counts=prob["counts"])
    check_finalize("cvk_bn_finalize_counts", f"{name} C={C}", got, prob, prob["counts"])


def test_bn_finalize_ill_conditioned():
    """mean 100, standard deviation 0.01, M = 71 * 64: sum s_p^2/n_p and S^2/M agree to 8 digits; the fp64 combination keeps the variance
    to the stated dvar (a relative 5e-6 here), which an fp32 combination, or the naive sum of squares, would miss by orders."""
    prob = stat_problem("illcond_m4544", 5)
    ref = check_finalize("cvk_bn_finalize", "illcond_m4544", run_finalize(prob), prob, prob["counts"])
    assert bool((ref["var"] < 2e-4).all()) and bool((ref["mean"] > 99).all())


def test_bn_finalize_constant_channels():
    """True variance 0 (channel 0: the constant 0): q_p = 0 and m2 is a difference of equal sums whose fp64 roundings may leave it
    negative; clamped, rstd = 1/sqrt(eps) within u (dvar is ~1e-15 here), and never NaN."""
    prob = stat_problem("constant_m71", 5)
    assert bool((prob["stats"][1] == 0).all())
    got = run_finalize(prob)
    ref = check_finalize("cvk_bn_finalize", "constant_m71", got, prob, prob["counts"])
    want = 1 / np.sqrt(LD(np.float32(EPS)))
    assert bool((np.abs(got["rstd"].astype(LD) - want) <= LD(U) * want).all()) and bool((ref["var"] < 1e-12).all())
    assert got["mean"][0] == 0 and got["shift"][0] == prob["beta"][0]


@pytest.mark.parametrize("fault", ["running_mean_only", "running_var_only", "wrong_P", "workspace_short"])
def test_bn_finalize_error_contract(fault):
    """Exactly one running pointer NULL and P != ceil(M/64) are CVK_EINVAL, a workspace one byte short of
    cvk_bn_finalize_workspace_bytes is CVK_EWORKSPACE; no output is written."""
    _lib, lib = libs()
    prob = stat_problem("m71", 65)
    P, C = prob["stats"].shape[1:]
    stats = torch.from_numpy(prob["stats"]).to(dev())
    gb = torch.ones(2, C, device=dev())
    boxes = [fbox(C) for _ in range(6)]
    nbt = IBox(1, torch.int64, -7)
    wsb = lib.cvk_bn_finalize_workspace_bytes(P, C)
    assert wsb == 1 * C * 3 * 8
    ws = torch.empty(wsb // 8, dtype=torch.float64, device=dev())
    rm = None if fault == "running_var_only" else boxes[4].ptr
    rv = None if fault == "running_mean_only" else boxes[5].ptr
    rc = lib.cvk_bn_finalize(stats.data_ptr(), P + 1 if fault == "wrong_P" else P, prob["M"], C, gb[0].data_ptr(), gb[1].data_ptr(), *[b.ptr for b in boxes[:4]],
                             rm, rv, nbt.ptr, MOMENTUM, EPS, ws.data_ptr(), wsb - 1 if fault == "workspace_short" else wsb, stream())
    assert rc == (EWORKSPACE if fault == "workspace_short" else EINVAL)
    assert "cvk_bn_finalize" in lib.cvk_last_error_string().decode()
    for b in boxes + [nbt]:
        untouched(b)
    if fault.startswith("running"):
        cnt = torch.tensor(prob["counts"], dtype=torch.float32, device=dev())
        rc = lib.cvk_bn_finalize_counts(stats.data_ptr(), cnt.data_ptr(), P, prob["M"], C, gb[0].data_ptr(), gb[1].data_ptr(), *[b.ptr for b in boxes[:4]],
                                        rm, rv, nbt.ptr, MOMENTUM, EPS, ws.data_ptr(), wsb, stream())
        assert rc == EINVAL
        for b in boxes + [nbt]:
            untouched(b)


@pytest.mark.parametrize("C", [1, 255, 256, 257])
def test_bn_eval_params(C):
    """cvk_bn_eval_params around its block size of 256: rstd to 2u relative (module docstring), mean bitwise running_mean, scale and
    shift to the bounds of the statistics with tol(mean) = 0."""
    _lib, lib = libs()
    rng = np.random.default_rng(case_seed(f"eval_c{C}"))
    f = np.float32
    p = {"gamma": rng.uniform(0.5, 1.5, C).astype(f), "beta": (0.3 * rng.normal(size=C)).astype(f), "running_mean": rng.normal(size=C).astype(f),
         "running_var": rng.uniform(0.01, 4.0, C).astype(f)}
    d = {k: torch.from_numpy(v).to(dev()) for k, v in p.items()}
    out = {k: fbox(C) for k in ("mean", "rstd", "scale", "shift")}
    _lib.check(lib.cvk_bn_eval_params(*[d[k].data_ptr() for k in ("gamma", "beta", "running_mean", "running_var")],
                                      *[out[k].ptr for k in ("mean", "rstd", "scale", "shift")], C, EPS, stream()))
    got = {k: b.settle(True)[1].numpy() for k, b in out.items()}
    ref = S.eval_params(p["gamma"], p["beta"], p["running_mean"], p["running_var"], EPS)
    assert np.array_equal(got["mean"].view(np.int32), p["running_mean"].view(np.int32))
    u = LD(U)
    trstd = 2 * u * ref["rstd"]
    tscale = 2 * u * np.abs(ref["scale"]) + np.abs(p["gamma"].astype(LD)) * trstd
    tshift = 3 * u * (np.abs(p["beta"].astype(LD)) + np.abs(ref["mean"] * ref["scale"])) + np.abs(ref["mean"]) * tscale
    for k, t in (("rstd", trstd), ("scale", tscale), ("shift", tshift)):
        frac = np_fraction(np.abs(got[k].astype(LD) - ref[k]), t)
        report("cvk_bn_eval_params " + k, f"C={C}", frac)
        assert frac <= 1.0, k


# ------------------------------------------------------------------------------------------------ 2. apply
def expect_v4(C, lds, lay, ptr_offsets=()):
    return 4 if C % 4 == 0 and all(v % 4 == 0 for v in lds) and all(s % 4 == 0 for s in lay.strides) and lay.offset % 4 == 0 and \
        all(o % 16 == 0 for o in ptr_offsets) else 1


def check_apply(entry, name, inp, shape, lay, vals):
    N, H, W, C = shape
    got = lay.window(vals).double()
    q = d64(inp)
    y64 = q["y"].view(N, H, W, C)
    ref = R.apply(y64, q["scale"], q["shift"])
    bound = 3 * U * ((y64 * q["scale"]).abs() + q["shift"].abs()) + U * ref.abs()
    frac = worst_fraction((got - ref).abs(), bound)
    report(entry, name, frac)
    assert frac <= 1.0
    zero_edge = (y64[..., 0] == 0)
    assert bool(zero_edge.any()) and bool((got[..., 0][zero_edge] == 0).all())
    assert bool((ref > 0).any()) and bool((ref == 0).any())


@pytest.mark.parametrize("name", list(APPLY_CASES))
def test_bn_relu_apply(name):
    """cvk_bn_relu_apply, both instantiations and every condition that demotes to the scalar one (C, the pitch of y, a stride of the
    view, a pointer that is only 4-byte aligned).  Bound: 3u (|y scale| + |shift|) + u |ref|."""
    _lib, lib = libs()
    shape, ldy, lay_kw, V, sc_off = APPLY_CASES[name]
    N, H, W, C = shape
    lay = Lay(shape, **lay_kw)
    assert V == expect_v4(C, [ldy], lay, [sc_off])
    inp = bn_inputs(shape, case_seed(name))
    y = rows_padded(inp["y"], ldy)
    sc = torch.full((C + 4,), float("nan"))
    sc[sc_off // 4:sc_off // 4 + C] = inp["scale"]
    sc, sh = sc.to(dev()), inp["shift"].to(dev())
    out = fbox(lay.numel)
    _lib.check(lib.cvk_bn_relu_apply(y.data_ptr(), ldy, sc.data_ptr() + sc_off, sh.data_ptr(), fview(lay, out.ptr), N, H, W, C, stream()))
    _, vals = out.settle(lay.mask())
    check_apply("cvk_bn_relu_apply", name, inp, shape, lay, vals)


def pool_and_code(a):
    """[N,H,W,C] fp32 -> (pooled values, code 0..3 of the first maximum in scan order (0,0),(0,1),(1,0),(1,1)) of every full 2x2 cell"""
    N, H, W, C = a.shape
    Ho, Wo = H // 2, W // 2
    cells = a[:, :2 * Ho, :2 * Wo].reshape(N, Ho, 2, Wo, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, Ho, Wo, 4, C)
    best = cells[:, :, :, 0].clone()
    code = torch.zeros(N, Ho, Wo, C, dtype=torch.uint8)
    for k in (1, 2, 3):
        upd = cells[:, :, :, k] > best
        best = torch.where(upd, cells[:, :, :, k], best)
        code = torch.where(upd, torch.full_like(code, k), code)
    return best, code


@pytest.mark.parametrize("name", list(POOL_CASES))
def test_bn_relu_apply_pool(name):
    """cvk_bn_relu_apply_pool: `out` to the bound of the plain pass (odd trailing rows and columns included); pool and code bitwise
    from the kernel's OWN out (no fp64 arg-max, so a near-tie cannot fail); with code = NULL the same out and pool."""
    _lib, lib = libs()
    shape, ldy, lay_kw = POOL_CASES[name]
    N, H, W, C = shape
    Ho, Wo = H // 2, W // 2
    lay = Lay(shape, **lay_kw)
    inp = bn_inputs(shape, case_seed(name))
    y = rows_padded(inp["y"], ldy)
    sc, sh = inp["scale"].to(dev()), inp["shift"].to(dev())

    def run(with_code):
        out, pl, code = fbox(lay.numel), fbox(N * Ho * Wo * C), IBox(N * Ho * Wo * C, torch.uint8, SENT8)
        _lib.check(lib.cvk_bn_relu_apply_pool(y.data_ptr(), ldy, sc.data_ptr(), sh.data_ptr(), fview(lay, out.ptr), pl.ptr, code.ptr if with_code else None,
                                              N, H, W, C, stream()))
        return out.settle(lay.mask()), pl.settle(True), code
    (obits, vals), (pbits, _), code = run(True)
    check_apply("cvk_bn_relu_apply_pool", name, inp, shape, lay, vals)
    want_pool, want_code = pool_and_code(lay.window(vals).contiguous())
    assert torch.equal(want_pool, R.pool2x2(lay.window(vals)))
    assert torch.equal(pbits, want_pool.contiguous().view(torch.int32).reshape(-1))
    assert torch.equal(code.settle(), want_code.reshape(-1))
    assert len(set(want_code.reshape(-1).tolist())) == 4 or name == "pool_one_cell"         # every code occurs
    (obits2, _), (pbits2, _), code2 = run(False)
    assert torch.equal(obits, obits2) and torch.equal(pbits, pbits2)
    untouched(code2)


def test_bn_relu_apply_pool_refuses_a_non_vector_layout():
    """C = 6: CVK_EINVAL (the caller then runs the plain pass and the pool), nothing written."""
    _lib, lib = libs()
    N, H, W, C = 1, 4, 4, 6
    y = torch.zeros(N * H * W, C, device=dev())
    c = torch.ones(2, 8, device=dev())
    out, pl, code = fbox(N * H * W * C), fbox(N * 2 * 2 * C), IBox(N * 2 * 2 * C, torch.uint8, SENT8)
    rc = lib.cvk_bn_relu_apply_pool(y.data_ptr(), C, c[0].data_ptr(), c[1].data_ptr(), fview(Lay((N, H, W, C)), out.ptr), pl.ptr, code.ptr, N, H, W, C, stream())
    assert rc == EINVAL and "cvk_bn_relu_apply_pool" in lib.cvk_last_error_string().decode()
    untouched(out), untouched(pl), untouched(code)


# ------------------------------------------------------------------------------------------------ 3. backward
def bn_device_operands(shape, ldy, kind, seed):
    inp = bn_inputs(shape, seed)
    lay = Lay(shape, **DOUT_LAYOUTS[kind])
    dout = lay.embed(inp["dout"]).to(dev())
    ops = {"y": rows_padded(inp["y"], ldy), "dout": dout, "view": fview(lay, dout.data_ptr()), "lay": lay}
    for k in ("scale", "shift", "mean", "rstd"):
        ops[k] = inp[k].to(dev())
    ops["consts"] = [ops[k].data_ptr() for k in ("scale", "shift", "mean", "rstd")]
    return inp, ops


def chunk_factors(C, V, per_thread):
    """per channel (per_thread(ppp) + ppp + 8) u with ppp = 256 // (cw/V) of the channel's column chunk"""
    cchunk = 1024 if V == 4 else 256
    f = torch.empty(C, dtype=torch.float64)
    for c0 in range(0, C, cchunk):
        cw = min(cchunk, C - c0)
        ppp = 256 // (cw // V)
        f[c0:c0 + cw] = (per_thread(ppp) + ppp + 8) * U
    return f


def sum_factor(lib, M, C, V):
    PB = lib.cvk_bn_bwd_blocks(M)
    rows = -(-M // PB)
    assert PB == -(-M // rows)
    return PB, chunk_factors(C, V, lambda ppp: -(-rows // ppp))


def reference_terms(name, inp):
    q = d64(inp)
    mask, g, gx, band = R.bn_bwd_terms(q["dout"], q["y"], q["scale"], q["shift"], q["mean"], q["rstd"])
    assert int(band.sum()) <= excluded_cap(band.numel()), (name, int(band.sum()))
    edge = (q["y"][:, 0] == 0)
    assert bool(edge.any()) and not bool(mask[:, 0][edge].any()) and not bool(band[:, 0][edge].any())
    return q, g, gx, band


def check_sums(entry, name, got, ref_terms, factor, cols):
    err = (got.double() - ref_terms.sum(0)).abs()
    frac = worst_fraction(err, factor * ref_terms.abs().sum(0), keep=cols)
    report(entry, name, frac)
    assert frac <= 1.0


def dy_reference(q, g, gx, M, use_batch_stats):
    """(fp32 dgamma, dbeta as the kernel gets them, reference dy, its bound without the u |ref| of the store)"""
    C = g.shape[1]
    if use_batch_stats:
        dgamma, dbeta = gx.sum(0).float(), g.sum(0).float()
    else:
        dgamma = dbeta = torch.full((C,), float("nan"))
    ref = R.bn_bwd_dy(q["dout"], q["y"], q["scale"], q["shift"], q["mean"], q["rstd"], dgamma.double(), dbeta.double(), M, use_batch_stats)
    xhat = (q["y"] - q["mean"]) * q["rstd"]
    A = 6 * U * q["scale"].abs() * (g.abs() + ((dbeta.double().abs() + (xhat * dgamma.double()).abs()) / M if use_batch_stats else 0.0))
    return dgamma, dbeta, ref, A + U * ref.abs()


@pytest.mark.parametrize("name", list(BN_CASES))
def test_bn_bwd_reduce(name):
    """cvk_bn_bwd_reduce + cvk_colsum_finalize: dbeta = sum g and dgamma = sum g*xhat per channel within (ceil(rows/ppp) + ppp + 8) u
    sum|term|, for both vector widths, every lane layout (idle threads, one pass, 256 passes), ragged and full last row block, two column
    chunks, and every gradient view.  Every partial row [0, PB) of both planes is written.  The zero edge of channel 0 tests the strict
    mask.  With out1 = NULL the first sums are bitwise the same."""
    _lib, lib = libs()
    shape, ldy, kind, V = BN_CASES[name]
    N, H, W, C = shape
    M = N * H * W
    inp, ops = bn_device_operands(shape, ldy, kind, case_seed(name))
    assert V == expect_v4(C, [ldy], ops["lay"])
    PB, factor = sum_factor(lib, M, C, V)
    part = fbox(2 * PB * C)
    _lib.check(lib.cvk_bn_bwd_reduce(ops["view"], ops["y"].data_ptr(), ldy, *ops["consts"], part.ptr, N, H, W, C, stream()))
    db, dg, db1 = fbox(C), fbox(C), fbox(C)
    _lib.check(lib.cvk_colsum_finalize(part.ptr, PB, C, db.ptr, dg.ptr, stream()))
    _lib.check(lib.cvk_colsum_finalize(part.ptr, PB, C, db1.ptr, None, stream()))
    part.settle(True)
    q, g, gx, band = reference_terms(name, inp)
    cols = ~band.any(0)
    check_sums("cvk_bn_bwd_reduce dbeta", name, db.settle(True)[1], g, factor, cols)
    check_sums("cvk_bn_bwd_reduce dgamma", name, dg.settle(True)[1], gx, factor, cols)
    assert torch.equal(db1.settle(True)[0], db.settle(True)[0])


@pytest.mark.parametrize("use_batch_stats", [1, 0])
@pytest.mark.parametrize("name", list(BN_CASES))
def test_bn_bwd_dx(name, use_batch_stats):
    """cvk_bn_bwd_dx into rows of C + 4 floats (the pad columns keep the sentinel): dy within 6u |scale| (|g| + |dbeta|/M + |xhat dgamma|/M)
    + u |ref|, the column sums of dy (every partial row [0, PB) written) within the bound of the sums; with ld_dy = C and no partial
    buffer the same dy bits.  dgamma and dbeta are the fp64 reference's sums rounded to fp32; with running statistics
    (use_batch_stats = 0) they are NULL.  A wrong 1/M moves the batch-statistics form by a relative 1/M: 1.4 % at M = 70."""
    _lib, lib = libs()
    shape, ldy, kind, V = BN_CASES[name]
    N, H, W, C = shape
    M = N * H * W
    inp, ops = bn_device_operands(shape, ldy, kind, case_seed(name))
    PB, factor = sum_factor(lib, M, C, V)
    q, g, gx, band = reference_terms(name, inp)
    dgamma, dbeta, ref, bound = dy_reference(q, g, gx, M, use_batch_stats)
    dgd, dbd = dgamma.to(dev()), dbeta.to(dev())

    def run(ld_dy, with_part):
        assert V == expect_v4(C, [ldy, ld_dy], ops["lay"])
        dy = fbox(M * ld_dy)
        part = fbox(PB * C) if with_part else None
        _lib.check(lib.cvk_bn_bwd_dx(ops["view"], ops["y"].data_ptr(), ldy, *ops["consts"], dgd.data_ptr() if use_batch_stats else None,
                                     dbd.data_ptr() if use_batch_stats else None, dy.ptr, ld_dy, part.ptr if with_part else None, N, H, W, C,
                                     use_batch_stats, stream()))
        bits, vals = dy.settle(cols_mask(M, ld_dy, C))
        return bits.view(M, ld_dy)[:, :C], vals.view(M, ld_dy)[:, :C].double(), part
    bits, got, part = run(C + 4, True)
    frac = worst_fraction((got - ref).abs(), bound, keep=~band)
    report("cvk_bn_bwd_dx dy", f"{name} stats={use_batch_stats}", frac)
    assert frac <= 1.0
    if not use_batch_stats:                                  # masked elements are exact zeros, the zero edge among them
        assert bool((got[:, 0][q["y"][:, 0] == 0] == 0).all())
    part.settle(True)
    dbias = fbox(C)
    _lib.check(lib.cvk_colsum_finalize(part.ptr, PB, C, dbias.ptr, None, stream()))
    check_sums("cvk_bn_bwd_dx column sums", f"{name} stats={use_batch_stats}", dbias.settle(True)[1], ref, factor, ~band.any(0))
    bits2, _, _ = run(C, False)
    assert torch.equal(bits, bits2)


# ------------------------------------------------------------------------------------------------ 4. one ReLU decision
def test_one_relu_decision_forward_and_backward():
    """The forward keeps max(0, y*scale + shift); the backward passes re-evaluate y*scale + shift > 0.  If one occurrence were contracted
    to a fused multiply-add and another not, an activation that was zeroed would still receive gradient.  512 elements of a (2,5,7,64)
    case, eight per channel, are set to fl(-shift/scale) displaced by -2..+2 ulps, where the two evaluations differ; dout is nowhere
    zero and the statistics are the running ones, so dy = scale*dout where the mask passes.  Elementwise and exactly (dy != 0) == (out > 0)
    for cvk_bn_relu_apply and cvk_bn_relu_apply_pool against cvk_bn_bwd_dx and cvk_bn_bwd_dx_e."""
    _lib, lib = libs()
    shape = (2, 5, 7, 64)
    N, H, W, C = shape
    M = N * H * W
    inp = bn_inputs(shape, case_seed("relu_decision"))
    inp["shift"][0] = 0.25                                      # channel 0 too gets a nonzero root
    g = torch.Generator().manual_seed(case_seed("relu_decision_places"))
    root = (-inp["shift"].double() / inp["scale"].double()).float()
    placed = torch.zeros(M, C, dtype=torch.bool)
    for c in range(C):
        rows = torch.randperm(M, generator=g)[:8]
        for i, m in enumerate(rows.tolist()):
            v = root[c].clone()
            k = i % 5 - 2
            for _ in range(abs(k)):
                v = torch.nextafter(v, torch.tensor(float("inf") if k > 0 else float("-inf")))
            inp["y"][m, c] = v
            placed[m, c] = True
    assert int(placed.sum()) == 512
    inp["dout"] = torch.where(inp["dout"] == 0, torch.ones_like(inp["dout"]), inp["dout"])
    z32 = inp["y"] * inp["scale"] + inp["shift"]                 # either evaluation: the placed elements sit within a few ulps of the root
    assert bool((z32[placed].abs() <= 8 * U * (inp["y"] * inp["scale"]).abs()[placed]).all())
    d = {k: v.to(dev()) for k, v in inp.items()}
    consts = [d[k].data_ptr() for k in ("scale", "shift", "mean", "rstd")]
    lay = Lay(shape)
    zeros = torch.zeros(C, device=dev())

    out1, out2, pl = fbox(M * C), fbox(M * C), fbox(N * (H // 2) * (W // 2) * C)
    _lib.check(lib.cvk_bn_relu_apply(d["y"].data_ptr(), C, consts[0], consts[1], fview(lay, out1.ptr), N, H, W, C, stream()))
    _lib.check(lib.cvk_bn_relu_apply_pool(d["y"].data_ptr(), C, consts[0], consts[1], fview(lay, out2.ptr), pl.ptr, None, N, H, W, C, stream()))
    dy1, dy2, E, part = fbox(M * C), fbox(M * C), fbox(4 * N * H * 2 * C), fbox(lib.cvk_bn_bwd_e_blocks(N, H, W) * C)
    _lib.check(lib.cvk_bn_bwd_dx(fview(lay, d["dout"].data_ptr()), d["y"].data_ptr(), C, *consts, None, None, dy1.ptr, C, None, N, H, W, C, 0, stream()))
    _lib.check(lib.cvk_bn_bwd_dx_e(fview(lay, d["dout"].data_ptr()), d["y"].data_ptr(), C, *consts, zeros.data_ptr(), zeros.data_ptr(), dy2.ptr, C, E.ptr,
                                   part.ptr, N, H, W, C, 0, stream()))
    alive = [b.settle(True)[1] > 0 for b in (out1, out2)]
    grads = [b.settle(True)[1] != 0 for b in (dy1, dy2)]
    assert torch.equal(alive[0], alive[1])
    on = alive[0].view(M, C)
    assert 0 < int(on[placed].sum()) < 512                       # the placed elements fall on both sides
    for gr, who in zip(grads, ("cvk_bn_bwd_dx", "cvk_bn_bwd_dx_e")):
        wrong = gr.view(M, C) != on
        assert not bool(wrong.any()), f"{who}: {int(wrong.sum())} elements ({int((wrong & placed).sum())} of the placed ones) get gradient against the forward's decision"


# ------------------------------------------------------------------------------------------------ 5. E-plane passes
def e_reference(name, shape, use_batch_stats):
    N, H, W, C = shape
    M = N * H * W
    inp, ops = bn_device_operands(shape, C, "dense", case_seed(name))
    q, g, gx, band = reference_terms(name, inp)
    dgamma, dbeta, ref, bound = dy_reference(q, g, gx, M, use_batch_stats)
    sh4 = (N, H, W, C)
    planes = S.e_planes(ref.view(sh4))
    tol = S.e_planes(bound.view(sh4), S.E_COEF.abs()) + 4 * U * S.e_planes(ref.abs().view(sh4), S.E_COEF.abs())
    keep = S.e_planes(band.double().view(sh4), torch.ones(1, 4, dtype=torch.float64))[0] == 0
    return ops, dgamma.to(dev()), dbeta.to(dev()), ref, bound, band, planes, tol, keep


def e_sum_factor(lib, shape):
    N, H, W, C = shape
    Mt = N * H * (-(-W // 4))
    pb = lib.cvk_bn_bwd_blocks(N * H * W)
    tiles = -(-Mt // pb)
    nb = lib.cvk_bn_bwd_e_blocks(N, H, W)
    assert nb == -(-Mt // tiles)
    return nb, chunk_factors(C, 4, lambda ppp: 4 * (-(-tiles // ppp)))


def check_dy_and_part(entry, name, lib, shape, dy_vals, part, nb, factor, ref, bound, band):
    _lib, _ = libs()
    C = shape[3]
    frac = worst_fraction((dy_vals.double() - ref).abs(), bound, keep=~band)
    report(entry + " dy", name, frac)
    assert frac <= 1.0
    part.settle(True)
    dbias = fbox(C)
    _lib.check(lib.cvk_colsum_finalize(part.ptr, nb, C, dbias.ptr, None, stream()))
    check_sums(entry + " column sums", name, dbias.settle(True)[1], ref, factor, ~band.any(0))


def check_planes(entry, name, got, planes, tol, keep):
    frac = worst_fraction((got.double() - planes).abs(), tol, keep=keep.unsqueeze(0).expand_as(planes))
    report(entry + " planes", name, frac)
    assert frac <= 1.0


@pytest.mark.parametrize("use_batch_stats", [1, 0])
@pytest.mark.parametrize("name", list(E_CASES))
def test_bn_bwd_dx_e(name, use_batch_stats):
    """cvk_bn_bwd_dx_e: dy and the cvk_bn_bwd_e_blocks partial rows as the plain pass; E1..E4 [4][N*H*ceil(W/4)][ld_dy] from the
    reference dy within sum|coef_i| tol(dy_i) + 4u sum|coef_i dy_i|, missing columns of a ragged last group counting as zero; the pad
    columns [C, ld_dy) of dy and of E keep the sentinel."""
    _lib, lib = libs()
    shape, ld_dy = E_CASES[name]
    N, H, W, C = shape
    M, Wt = N * H * W, -(-W // 4)
    Mt = N * H * Wt
    ops, dgd, dbd, ref, bound, band, planes, tol, keep = e_reference(name, shape, use_batch_stats)
    nb, factor = e_sum_factor(lib, shape)
    dy, E, part = fbox(M * ld_dy), fbox(4 * Mt * ld_dy), fbox(nb * C)
    _lib.check(lib.cvk_bn_bwd_dx_e(ops["view"], ops["y"].data_ptr(), C, *ops["consts"], dgd.data_ptr(), dbd.data_ptr(), dy.ptr, ld_dy, E.ptr, part.ptr,
                                   N, H, W, C, use_batch_stats, stream()))
    case = f"{name} stats={use_batch_stats}"
    _, vals = dy.settle(cols_mask(M, ld_dy, C))
    check_dy_and_part("cvk_bn_bwd_dx_e", case, lib, shape, vals.view(M, ld_dy)[:, :C], part, nb, factor, ref, bound, band)
    _, ev = E.settle(cols_mask(4 * Mt, ld_dy, C))
    check_planes("cvk_bn_bwd_dx_e", case, ev.view(4, N, H, Wt, ld_dy)[..., :C], planes[1:5], tol[1:5], keep)


@pytest.mark.parametrize("use_batch_stats", [1, 0])
@pytest.mark.parametrize("form", ["e6", "e4p"])
@pytest.mark.parametrize("name", list(E6_CASES))
def test_bn_bwd_dx_e_padded_planes(name, form, use_batch_stats):
    """cvk_bn_bwd_dx_e6 (E0..E5) and cvk_bn_bwd_dx_e4p (E1..E4) in the padded plane layout: row Wtp + (n (H + 2) + y + 1) Wtp + xt of
    cvk_wgradp_plane_rows rows per plane; the pad rows (first and last, one above and below every image, the columns [ceil(W/4), Wtp))
    keep the sentinel: zeroing them is another call's business.  W = 12 has three full groups, W = 13 a ragged fourth."""
    _lib, lib = libs()
    shape = E6_CASES[name]
    N, H, W, C = shape
    M, Wt = N * H * W, -(-W // 4)
    Wtp, rows, prow = S.padded_layout(N, H, W)
    assert rows == lib.cvk_wgradp_plane_rows(N, H, W) and Wtp == 8
    ops, dgd, dbd, ref, bound, band, planes, tol, keep = e_reference(name, shape, use_batch_stats)
    nb, factor = e_sum_factor(lib, shape)
    sel = slice(0, 6) if form == "e6" else slice(1, 5)
    npl = 6 if form == "e6" else 4
    dy, E, part = fbox(M * C), fbox(npl * rows * C), fbox(nb * C)
    fn = lib.cvk_bn_bwd_dx_e6 if form == "e6" else lib.cvk_bn_bwd_dx_e4p
    _lib.check(fn(ops["view"], ops["y"].data_ptr(), C, *ops["consts"], dgd.data_ptr(), dbd.data_ptr(), dy.ptr, C, E.ptr, part.ptr, N, H, W, C,
                  use_batch_stats, stream()))
    case = f"{name} {form} stats={use_batch_stats}"
    _, vals = dy.settle(True)
    check_dy_and_part("cvk_bn_bwd_dx_" + form, case, lib, shape, vals.view(M, C), part, nb, factor, ref, bound, band)
    written = torch.zeros(npl, rows, C, dtype=torch.bool)
    written[:, prow.reshape(-1)] = True
    assert int(written[0, :, 0].sum()) == N * H * Wt < rows
    _, ev = E.settle(written)
    check_planes("cvk_bn_bwd_dx_" + form, case, ev.view(npl, rows, C)[:, prow.reshape(-1)].view(npl, N, H, Wt, C), planes[sel], tol[sel], keep)
    if form == "e6":                                          # E0 and E5 are columns 4 xt and 4 xt + 3 of the dy just written, bit for bit
        d = torch.zeros(N, H, 4 * Wt, C)
        d[:, :, :W] = vals.view(N, H, W, C)
        got = ev.view(6, rows, C)[:, prow.reshape(-1)].view(6, N, H, Wt, C)
        assert torch.equal(got[0], d[:, :, 0::4]) and torch.equal(got[5], d[:, :, 3::4])


@pytest.mark.parametrize("form,fault", [(f, x) for f in ("e", "e6", "e4p") for x in ("c6", "ldy66")] + [("e6", "ld_dy_wider"), ("e4p", "ld_dy_wider")])
def test_bn_bwd_dx_e_refusals(form, fault):
    """A non-vector layout (C = 6; a pitch of y of 66) is CVK_EINVAL for all three forms, ld_dy != C for the padded two; nothing is
    written.  (cvk_bn_bwd_dx_e itself takes ld_dy > C: e_w7_c12_ld16.)"""
    _lib, lib = libs()
    N, H, W = 1, 2, 8
    C = 6 if fault == "c6" else 8
    ldy = 66 if fault == "ldy66" else C
    ld_dy = C + 4 if fault == "ld_dy_wider" else C
    M = N * H * W
    y = torch.zeros(M, ldy, device=dev())
    dout = torch.ones(M, C, device=dev())
    c = torch.ones(6, 8, device=dev())
    rows = lib.cvk_wgradp_plane_rows(N, H, W)
    dy, E, part = fbox(M * ld_dy), fbox(6 * rows * ld_dy), fbox(lib.cvk_bn_bwd_e_blocks(N, H, W) * C)
    fn = {"e": lib.cvk_bn_bwd_dx_e, "e6": lib.cvk_bn_bwd_dx_e6, "e4p": lib.cvk_bn_bwd_dx_e4p}[form]
    rc = fn(fview(Lay((N, H, W, C)), dout.data_ptr()), y.data_ptr(), ldy, *[c[i].data_ptr() for i in range(6)], dy.ptr, ld_dy, E.ptr, part.ptr, N, H, W, C, 1,
            stream())
    assert rc == EINVAL and "cvk_bn_bwd_dx_e" in lib.cvk_last_error_string().decode()
    untouched(dy), untouched(E), untouched(part)


# ------------------------------------------------------------------------------------------------ 6. batched column sums
def run_colsum_batch(jobs_spec, seed):
    """one launch over jobs of (PB, C): each against the longdouble column sums, bitwise against cvk_colsum_finalize, guards intact"""
    _lib, lib = libs()
    g = torch.Generator().manual_seed(seed)
    parts = [(torch.randn(PB, C, generator=g) * (1 + i)).to(dev()) for i, (PB, C) in enumerate(jobs_spec)]
    outs = [fbox(C) for _, C in jobs_spec]
    arr = (_lib.ColsumJob * len(jobs_spec))(*[_lib.ColsumJob(p.data_ptr(), o.ptr, PB, C) for p, o, (PB, C) in zip(parts, outs, jobs_spec)])
    _lib.check(lib.cvk_colsum_finalize_batch(ctypes.addressof(arr), len(jobs_spec), stream()))
    worst = 0.0
    for p, o, (PB, C) in zip(parts, outs, jobs_spec):
        bits, vals = o.settle(True)
        h = p.cpu().numpy().astype(LD)
        ref, mag = h.sum(0), np.abs(h).sum(0)
        worst = max(worst, np_fraction(np.abs(vals.numpy().astype(LD) - ref), LD(U) * np.abs(ref) + LD(2) ** -52 * PB * mag))
        single = fbox(C)
        _lib.check(lib.cvk_colsum_finalize(p.data_ptr(), PB, C, single.ptr, None, stream()))
        assert torch.equal(single.settle(True)[0], bits), (PB, C)
    return worst


def test_colsum_finalize_batch():
    """cvk_colsum_finalize_batch: five jobs of very different sizes in one launch (the grid is sized by the widest, so a narrower job's
    surplus blocks must write nothing: guards), then CVK_COLSUM_BATCH_MAX small ones; n = 0 and n = 65 are CVK_EINVAL."""
    _lib, lib = libs()
    assert _lib.COLSUM_BATCH_MAX == 64
    frac = run_colsum_batch([(1, 1), (5, 63), (500, 64), (17, 130), (512, 12)], 61)
    report("cvk_colsum_finalize_batch", "five jobs", frac)
    assert frac <= 1.0
    frac = run_colsum_batch([(1 + i % 7, 1 + (i * 5) % 70) for i in range(64)], 62)
    report("cvk_colsum_finalize_batch", "64 jobs", frac)
    assert frac <= 1.0
    p, o = torch.ones(2, 4, device=dev()), fbox(4)
    arr = (_lib.ColsumJob * 65)(*[_lib.ColsumJob(p.data_ptr(), o.ptr, 2, 4) for _ in range(65)])
    for n in (0, 65):
        assert lib.cvk_colsum_finalize_batch(ctypes.addressof(arr), n, stream()) == EINVAL
    untouched(o)
