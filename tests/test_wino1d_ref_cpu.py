"""tests/wino1d_ref.py checked without a GPU: its fp64 references against torch.nn.functional, the rounding error that the tolerances of
tests/test_gpu_wino1d.py are derived from (a numpy fp32 restatement of the transform chains of csrc/wino.hip and csrc/wino4.hip against
fp64), and the coverage of every kernel arm by the case tables.  Run with -s for the figures that profiles/wino1d_margins.txt records."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import wino1d_ref as R

RAGGED = [(2, 5, 7, 12, 20), (1, 1, 9, 8, 4), (3, 6, 1, 4, 8)]   # N, H, W, Cin, Cout


@pytest.mark.parametrize("N,H,W,Cin,Cout", RAGGED)
def test_references_agree_with_torch(N, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(N, H, W, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, 3, 3, Cin, generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    dy = torch.randn(N, H, W, Cout, generator=g, dtype=torch.float64)
    xn, wn = x.permute(0, 3, 1, 2).clone().requires_grad_(True), w.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(xn, wn, b, padding=1)
    y.backward(dy.permute(0, 3, 1, 2))
    yr = R.conv_fwd_ref(x, w, b)
    assert torch.allclose(yr, y.detach().permute(0, 2, 3, 1), rtol=0, atol=1e-12)
    assert torch.allclose(R.conv_dgrad_ref(dy, w), xn.grad.permute(0, 2, 3, 1), rtol=0, atol=1e-12)
    assert torch.allclose(R.conv_wgrad_ref(x, dy), wn.grad.permute(0, 2, 3, 1), rtol=0, atol=1e-11)
    # the data-grad is the forward conv of dy with the rotated, channel-transposed filter
    assert torch.allclose(R.conv_fwd_ref(dy, R.dgrad_filter(w)), R.conv_dgrad_ref(dy, w), rtol=0, atol=1e-12)
    # single rows from their three-row bands
    rows = sorted({0, H - 1, N * H - 1, (N * H) // 2})
    assert torch.allclose(R.conv_fwd_ref_rows(x, w, b, rows), yr.reshape(N * H, W, Cout)[rows], rtol=0, atol=1e-12)
    # statistics partials: Chan's combination of the granules is the batch mean and biased variance
    st, cnt = R.stat_partials_ref(yr)
    assert st.shape == (2, R.cdiv(N * H * W, 64), Cout) and cnt.sum().item() == N * H * W
    mean, var = R.chan_combine(st[0], st[1], cnt)
    flat = yr.reshape(-1, Cout)
    assert torch.allclose(mean, flat.mean(0), rtol=0, atol=1e-12) and torch.allclose(var, flat.var(0, unbiased=False), rtol=1e-12, atol=1e-12)
    # E planes: column by column, zero beyond the right edge
    E, Eabs = R.e_planes_ref(dy, Cout)
    Wt = R.cdiv(W, 4)
    assert E.shape == (4, N * H * Wt, Cout)
    for t in (0, N * H * Wt - 1):
        row, xt = divmod(t, Wt)
        n, yy = divmod(row, H)
        col = [dy[n, yy, 4 * xt + i] if 4 * xt + i < W else torch.zeros(Cout, dtype=torch.float64) for i in range(4)]
        for k, cf in enumerate(R.E_COEF):
            assert torch.allclose(E[k, t], sum(c * d for c, d in zip(cf, col)), rtol=0, atol=1e-12)
    assert (Eabs >= E.abs() - 1e-12).all()


@pytest.mark.parametrize("fam", [2, 4])
def test_restated_chains_are_the_operator(fam):
    """The fp32 restatements compute the convolution and its weight-grad (errors at rounding level, far from a wrong constant), and the
    F(4,3) tap tables of the staging path spell B^T."""
    rng = np.random.default_rng(fam)
    x = np.maximum(rng.standard_normal((5, 7, 8)), 0).astype(np.float32)
    w = rng.standard_normal((4, 3, 3, 8)).astype(np.float32)
    dy = rng.standard_normal((5, 7, 4)).astype(np.float32)
    xt = torch.from_numpy(x)[None]
    assert R.rel_l2(R.forward_chain_f32(fam, x, w), R.conv_fwd_ref(xt, torch.from_numpy(w))[0].numpy()) < 2e-6
    assert R.rel_l2(R.wgrad_chain_f32(fam, x, dy), R.conv_wgrad_ref(xt, torch.from_numpy(dy)[None]).numpy()) < 2e-6
    for xi in range(6):
        row = np.zeros(6)
        for j, c in zip(R.W4_TAPS[xi], R.W4_COEF[xi]):
            row[j] += c
        row[4] += 1 <= xi <= 4
        assert (row == R.BT[4][xi]).all()
    # Cook-Toom identity of the three matrices: A^T [(G g) (.) (B^T d)] is the correlation of d with g
    d, g = rng.standard_normal(R.group(fam) + 2), rng.standard_normal(3)
    want = np.array([d[i:i + 3] @ g for i in range(R.group(fam))])
    assert np.allclose(R.AT[fam] @ ((R.G[fam] @ g) * (R.BT[fam] @ d)), want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("kind", ["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("fam", [2, 4])
def test_chain_rounding(kind, fam):
    """Where the tolerances come from: the relative L2 rounding error of the fp32 restatement against fp64 at 64 and 512 input channels
    (whole tensor, and the worst image row of y / output channel of dW).  wino1d_ref.MEASURED holds these figures; bound() is 3 x
    (weight-grad: 6 x) their interpolation in Cin.  F(4,3) rounds about 2.5 x coarser than F(2,3) (transform constants 4, 5, 8), the
    forward chain grows about as sqrt(Cin), the weight-grad chain does not depend on Cin (it reduces over pixels)."""
    for Cin in (64, 512):
        whole, row = R.measure_chain(kind, fam, Cin)
        print(f"[wino1d restatement] {kind} F({fam},3) Cin={Cin}: whole {whole:.3e}, worst row {row:.3e}; "
              f"bounds {R.bound(kind, fam, Cin, 0):.3e} / {R.bound(kind, fam, Cin, 1):.3e}")
        for got, rec in zip((whole, row), R.MEASURED[(kind, fam, Cin)]):
            assert abs(got - rec) <= 0.1 * rec, (kind, fam, Cin, got, rec)
        assert whole <= row < 1.5 * whole
    e64, e512 = R.MEASURED[(kind, fam, 64)][0], R.MEASURED[(kind, fam, 512)][0]
    if kind == "wgrad":
        assert 0.8 < e512 / e64 < 1.25
    else:
        assert 2.0 < e512 / e64 < math.sqrt(8) * 1.2
    assert 1.5 < R.MEASURED[(kind, 4, 64)][0] / R.MEASURED[(kind, 2, 64)][0] < 3.5
    # bound(): the measured points themselves, monotone in between
    f = 6.0 if kind == "wgrad" else 3.0
    for which in (0, 1):
        assert math.isclose(R.bound(kind, fam, 64, which), f * R.MEASURED[(kind, fam, 64)][which], rel_tol=1e-12)
        assert math.isclose(R.bound(kind, fam, 512, which), f * R.MEASURED[(kind, fam, 512)][which], rel_tol=1e-12)
        lo, hi = sorted((R.bound(kind, fam, 64, which), R.bound(kind, fam, 512, which)))
        assert lo <= R.bound(kind, fam, 256, which) <= hi


@pytest.mark.parametrize("fam", [2, 4])
def test_case_tables_cover_every_arm(fam):
    """Fails when a case is dropped: over the tables, arm_of reaches the three column tiles, single-index-only and mixed grids, every K split
    and output chunk (family 4) of the forward kernels, and all eight <BM, MULTIROW, L> weight-grad instantiations with and without a
    slab split and with more than one slice per image row."""
    arms = [R.arm_of("fwd", fam, c) for c in R.FWD_CASES + R.FWD_BIG_CASES[fam]]
    assert all(a[:2] == ("fwd", fam) for a in arms)
    want = R.FWD_ARMS[fam]
    assert {a[2] for a in arms} == want["bn"]
    assert {a[3] for a in arms} >= want["blocks"]
    assert {a[4] for a in arms} == want["ksplit"]
    assert {a[5] for a in arms} == want["chunk"]
    # each column tile with a K split where there is one, and the mixed grid with both wide tiles
    if fam == 4:
        assert {(a[2], a[4]) for a in arms} >= {(64, 3), (128, 3), (128, 2), (128, 1), (64, 1), (32, 1)}
    assert {a[2] for a in arms if a[3] == "multi+single"} >= {64, 128}
    for c in R.FWD_BIG_CASES[fam]:
        p = R.plan_fwd(fam, *c[:4], c[4])
        assert (p["tiles"], p["nfull"]) == (258, 256) and R.output_chunk(fam, c[0], c[1], c[2], c[4]) == 1024
    w = [R.arm_of("wgrad", fam, c) for c in R.WGRAD_CASES]
    assert {a[2:5] for a in w} == R.WGRAD_ARMS
    assert {a[5] for a in w} == {"slab", "split"}
    plans = [R.plan_wgrad(fam, c[0], c[1], c[2], c[4], c[5]) for c in R.WGRAD_CASES]
    assert any(p["S"] > 1 for p in plans) and any(p["tilesM"] > 1 and p["tilesN"] > 2 for p in plans)
    assert any(p["splits"] > 1 and p["nslices"] % p["chunk"] for p in plans)        # a short last slab
    assert any(p["R"] > 1 and (c[0] * c[1]) % p["R"] for p, c in zip(plans, R.WGRAD_CASES))   # a short last slice
    assert all(c in R.WGRAD_CASES for c in R.EPRE_CASES) and all(c[2] % 4 for c in R.EPRE_CASES)


def test_arms_of_the_stated_cases():
    """The arms the case tables are there for, as the planners' restatement derives them (family 4)."""
    fw = {c: R.plan_fwd(4, *c[:4], c[5] if len(c) > 5 else c[4]) for c in R.FWD_CASES}
    assert fw[(1, 20, 33, 128, 64)]["nfull"] == 0 and fw[(1, 20, 33, 128, 64)]["bn"] == 64
    assert (fw[(1, 6, 8, 256, 128)]["ksplit"], fw[(1, 6, 8, 256, 128)]["tiles"]) == (1, 1)
    assert (fw[(1, 45, 60, 256, 64)]["ksplit"], fw[(1, 45, 60, 256, 64)]["bn"]) == (3, 64)
    assert (fw[(1, 45, 60, 256, 256)]["ksplit"], fw[(1, 45, 60, 256, 256)]["tilesN"]) == (3, 2)
    assert (fw[(2, 45, 110, 256, 256)]["ksplit"], fw[(2, 45, 110, 256, 256)]["tiles"]) == (2, 40)
    assert R.output_chunk(4, 1, 128, 257, 260) == 256 and R.output_chunk(4, 1, 9, 13, 12) == 64

    def wg(c):
        p = R.plan_wgrad(4, c[0], c[1], c[2], c[4], c[5])
        return (p["bm"], p["L"], p["S"], p["R"], p["splits"], p["tilesM"], p["tilesN"])
    assert wg((1, 32, 128, 64, 64, 64, 64)) == (64, 32, 1, 1, 2, 1, 2)
    assert wg((2, 9, 40, 64, 64, 128, 128)) == (128, 30, 1, 3, 1, 1, 2)
    assert wg((1, 7, 28, 64, 64, 64, 64)) == (64, 30, 1, 4, 1, 1, 2)
    assert wg((1, 3, 5, 64, 64, 64, 64))[2:5] == (1, 16, 1)
    assert wg((3, 5, 33, 96, 96, 192, 192))[5:] == (2, 3)
    assert wg((1, 40, 120, 64, 64, 128, 128))[:5] == (128, 30, 1, 1, 2)
    assert wg((2, 11, 130, 36, 36, 72, 72))[1:5] == (30, 2, 1, 2)
    assert wg((1, 50, 131, 32, 32, 40, 44))[4] == 6
    assert wg((2, 17, 60, 128, 128, 64, 64))[2:] == (1, 2, 1, 1, 3)
    assert wg((2, 24, 256, 64, 64, 64, 64))[:3] == (64, 32, 2)
    assert wg((2, 6, 64, 64, 64, 128, 128))[:4] == (128, 32, 1, 2)
    assert wg((1, 16, 128, 32, 32, 72, 72))[:4] == (128, 32, 1, 1)
