"""tests/direct_conv_ref.py checked without a GPU: its host packs and the shared fp64 references against torch.nn.functional and autograd, the
rounding error that the tolerances of tests/test_gpu_direct_conv.py are derived from (a numpy fp32 restatement of the accumulation chains
of csrc/conv3x3.hip against fp64), and the coverage of every kernel instantiation and named edge by the case tables.  Run with -s for the
figures that profiles/direct_conv_margins.txt records."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import direct_conv_ref as R

RAGGED = [(2, 5, 7, 3, 5), (1, 1, 9, 12, 4), (3, 6, 1, 4, 10)]   # N, H, W, Cin, Cout


@pytest.mark.parametrize("N,H,W,Cin,Cout", RAGGED)
def test_packs_and_references_agree_with_torch(N, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(N, H, W, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, 3, 3, Cin, generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    dy = torch.randn(N, H, W, Cout, generator=g, dtype=torch.float64)
    xn, wn = x.permute(0, 3, 1, 2).clone().requires_grad_(True), w.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(xn, wn, b, padding=1)
    y.backward(dy.permute(0, 3, 1, 2))
    want_y, want_dx, want_dw = y.detach().permute(0, 2, 3, 1), xn.grad.permute(0, 2, 3, 1), wn.grad.permute(0, 2, 3, 1)
    assert torch.allclose(R.conv_fwd_ref(x, w, b), want_y, rtol=0, atol=1e-12)
    assert torch.allclose(R.conv_dgrad_ref(dy, w), want_dx, rtol=0, atol=1e-12)
    assert torch.allclose(R.conv_wgrad_ref(x, dy), want_dw, rtol=0, atol=1e-11)
    # forward pack: the conv of the zero-padded input with the padded filter is the conv
    Cp, Op = R.pad4(Cin) + 4, R.pad4(Cout) + 8
    pf = R.pack_fwd_ref(w, Cp)
    assert pf.shape == (Cout, 9, Cp) and bool((pf[:, :, Cin:] == 0).all()) and torch.equal(pf[:, :, :Cin], w.reshape(Cout, 9, Cin))
    xpad = torch.zeros(N, H, W, Cp, dtype=torch.float64)
    xpad[..., :Cin] = x
    assert torch.allclose(R.conv_fwd_ref(xpad, pf.view(Cout, 3, 3, Cp), b), want_y, rtol=0, atol=1e-12)
    # data-grad pack: element by element, pads zero, and the forward conv of the padded dy with it is the data-grad
    pd = R.pack_dgrad_ref(w, Cp, Op)
    assert pd.shape == (Cp, 9, Op) and bool((pd[Cin:] == 0).all()) and bool((pd[:, :, Cout:] == 0).all())
    for ci, t, co in ((0, 0, 0), (Cin - 1, 8, Cout - 1), (Cin // 2, 3, Cout // 2), (0, 5, Cout - 1)):
        assert pd[ci, t, co] == w.reshape(Cout, 9, Cin)[co, 8 - t, ci]
    dypad = torch.full((N, H, W, Op), 7.0, dtype=torch.float64)        # the zero filter rows cancel whatever the pad columns hold
    dypad[..., :Cout] = dy
    dx = R.conv_fwd_ref(dypad, pd.view(Cp, 3, 3, Op))
    assert torch.allclose(dx[..., :Cin], want_dx, rtol=0, atol=1e-12) and bool((dx[..., Cin:] == 0).all())
    # statistics partials: Chan's combination of the granules is the batch mean and biased variance
    st, cnt = R.stat_partials_ref(want_y)
    mean, var = R.chan_combine(st[0], st[1], cnt)
    flat = want_y.reshape(-1, Cout)
    assert cnt[-1].item() == N * H * W - 64 * (st.shape[1] - 1)
    assert torch.allclose(mean, flat.mean(0), rtol=0, atol=1e-12) and torch.allclose(var, flat.var(0, unbiased=False), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("Cin", [4, 12, 36, 64])
def test_restated_chains_are_the_operator(Cin):
    """The fp32 restatements compute the convolution and its weight-grad: they agree with fp64 to within the bound derived from them, also
    at the channel counts below 64 to which bound() extrapolates; im2col places every tap."""
    rng = np.random.default_rng(Cin)
    x = np.maximum(rng.standard_normal((2, 5, 7, Cin)), 0).astype(np.float32)
    w = (rng.standard_normal((6, 3, 3, Cin)) * math.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    dy = rng.standard_normal((2, 5, 7, 6)).astype(np.float32)
    xt, wt, dyt = torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(dy)
    A = R.im2col(x)
    assert A.shape == (70, 9 * Cin)
    for n, yy, xx, tap in ((0, 0, 0, 0), (1, 4, 6, 8), (1, 2, 3, 5), (0, 4, 0, 6)):
        sy, sx = yy + tap // 3 - 1, xx + tap % 3 - 1
        want = x[n, sy, sx] if 0 <= sy < 5 and 0 <= sx < 7 else np.zeros(Cin, dtype=np.float32)
        assert (A[(n * 5 + yy) * 7 + xx, tap * Cin:(tap + 1) * Cin] == want).all()
    y, ref = R.forward_chain_f32(x, w), R.conv_fwd_ref(xt, wt).numpy()
    assert R.rel_l2(y, ref) < R.bound("fwd", Cin, 0)
    assert R.worst_row_rel_l2(y.reshape(10, 7, 6), ref.reshape(10, 7, 6)) < R.bound("fwd", Cin, 1)
    dxin = rng.standard_normal((2, 5, 7, Cin)).astype(np.float32)
    dx, ref = R.forward_chain_f32(dxin, w), R.conv_fwd_ref(torch.from_numpy(dxin), wt).numpy()
    assert R.rel_l2(dx, ref) < R.bound("dgrad", Cin, 0)
    ref = R.conv_wgrad_ref(xt, dyt).numpy()
    for chunk in (32, 64, 70):
        dw = R.wgrad_chain_f32(x, dy, chunk)
        assert R.rel_l2(dw, ref) < R.bound("wgrad", Cin, 0) and R.worst_row_rel_l2(dw, ref) < R.bound("wgrad", Cin, 1)


@pytest.mark.parametrize("kind", ["fwd", "dgrad", "wgrad"])
def test_chain_rounding(kind):
    """Where the tolerances come from: the relative L2 rounding error of the fp32 restatement against fp64 at 64 and 512 input channels
    (whole tensor, and the worst image row of y / output channel of dW).  direct_conv_ref.MEASURED holds these figures; bound() is 3 x
    (weight-grad: 6 x) their interpolation in Cin.  The forward chain grows about as sqrt(Cin); the weight-grad chain reduces over pixels
    and does not depend on Cin."""
    for Cin in (64, 512):
        whole, row = R.measure_chain(kind, Cin)
        print(f"[direct restatement] {kind} Cin={Cin}: whole {whole:.3e}, worst row {row:.3e}; "
              f"bounds {R.bound(kind, Cin, 0):.3e} / {R.bound(kind, Cin, 1):.3e}")
        for got, rec in zip((whole, row), R.MEASURED[(kind, Cin)]):
            assert abs(got - rec) <= 0.1 * rec, (kind, Cin, got, rec)
        assert whole <= row < 1.5 * whole
    e64, e512 = R.MEASURED[(kind, 64)][0], R.MEASURED[(kind, 512)][0]
    if kind == "wgrad":
        assert 0.8 < e512 / e64 < 1.25
    else:
        assert 2.0 < e512 / e64 < math.sqrt(8) * 1.2
    f = 6.0 if kind == "wgrad" else 3.0
    for which in (0, 1):
        assert math.isclose(R.bound(kind, 64, which), f * R.MEASURED[(kind, 64)][which], rel_tol=1e-12)
        assert math.isclose(R.bound(kind, 512, which), f * R.MEASURED[(kind, 512)][which], rel_tol=1e-12)
        lo, hi = sorted((R.bound(kind, 64, which), R.bound(kind, 512, which)))
        assert lo <= R.bound(kind, 256, which) <= hi
    cins = sorted({c[3] for c in R.FWD_CASES} if kind == "fwd" else {R.pad4(c[4]) for c in R.DGRAD_CASES} if kind == "dgrad"
                  else {c[3] for c in R.WGRAD_CASES})
    print(f"[direct restatement] {kind} bounds (whole / worst row): "
          + ", ".join(f"Cin={c}: {R.bound(kind, c, 0):.3e} / {R.bound(kind, c, 1):.3e}" for c in cins))


def test_planner_restatement():
    """choose_splits / plan_wgrad on shapes worked out by hand from csrc/conv_tile.h (the GPU test holds the restatement against the
    library's workspace query at every case)."""
    assert R.choose_splits(2, 1311) == 2 and R.choose_splits(5, 1920) == 3 and R.choose_splits(1, 234) == 1
    # 64 tiles over 64 Ki pixels: s = 8 is the first to fill two whole rounds of 256 (eff 1.0), and nothing later beats it by 0.02
    assert R.choose_splits(64, 65536) == 8
    p = R.plan_wgrad(1311, 48, 24)
    assert (p["bm"], p["bn"], p["tilesM"], p["tilesN"], p["splits"], p["chunk"], p["last"]) == (32, 256, 1, 2, 2, 672, 639)
    p = R.plan_wgrad(1920, 64, 64)
    assert (p["bm"], p["bn"], p["tilesN"], p["splits"], p["chunk"], p["last"]) == (64, 128, 5, 3, 640, 640)
    assert R.plan_wgrad(1311, 4, 64)["bn"] == 64 and R.plan_wgrad(1311, 8, 64)["bn"] == 128
    assert R.wgrad_smallco(64, 64, 16) and not R.wgrad_smallco(64, 64, 17) and not R.wgrad_smallco(60, 64, 12) and not R.wgrad_smallco(32, 32, 12)
    assert R.wgrad_workspace_bytes(2, 9, 13, 64, 12) == 512 * 12 * 576 * 4
    assert R.wgrad_workspace_bytes(2, 9, 13, 32, 12) == 12 * 288 * 4
    assert R.fwd_tile(32) == (256, 32) and R.fwd_tile(33) == (128, 64) and R.fwd_tile(64) == (128, 64) and R.fwd_tile(65) == (128, 128)


def test_case_tables_cover_every_arm_and_edge():
    """Fails when a case is dropped: over the tables, arm_of reaches all 12 instantiations of k_conv3x3_igemm (3 tiles x STATS x CIN32), all 4
    of k_conv3x3_wgrad and k_wgrad_smallco, and every edge the kernels treat on a path of its own."""
    assert len(R.FWD_ARMS) == 12
    assert {R.arm_of("fwd", c, st) for c in R.FWD_CASES for st in (False, True)} == R.FWD_ARMS
    e = {c: R.fwd_edges(c) for c in R.FWD_CASES}
    for generic in (False, True):
        nks = {v["nK"] for v in e.values() if v["generic"] == generic}
        assert any(n % 2 for n in nks) and any(n % 2 == 0 for n in nks)           # the peeled odd tail step, both arms
    assert any(v["nK"] == 2 for v in e.values())                                   # the prologue's three loads reach past the end of K
    assert any(v["nK"] == 9 for v in e.values()) and any(v["nK"] == 27 for v in e.values())
    assert any(v["partial_k"] for v in e.values())
    assert all(v["partial_k"] or v["straddle"] for v in e.values() if v["generic"]) and not any(v["straddle"] for v in e.values() if not v["generic"])
    assert any(v["straddle"] and v["taps_per_slice"] == 2 for v in e.values()) and any(v["taps_per_slice"] == 8 for v in e.values())
    for tile in ((128, 128), (128, 64), (256, 32)):
        mine = [v for v in e.values() if (v["BM"], v["BN"]) == tile]
        assert any(v["pb"] for v in mine) and any(v["ragged_m"] for v in mine) and any(v["ragged_n"] for v in mine), tile
    assert any(v["ragged_second_column"] for v in e.values())
    assert {R.fwd_tile(c[5]) for c in R.FWD_CASES if len(c) > 5} == {(128, 128), (128, 64)}
    for c in R.FWD_CASES:
        if len(c) > 5:                                                             # ldy crosses a dispatch boundary, Cout does not
            assert e[c]["ld_pad"] and R.fwd_tile(c[5]) != R.fwd_tile(c[4])
    assert any(v["images_per_tile"] >= 17 for v in e.values())
    assert any(c[1] == 1 and c[2] > 1 for c in R.FWD_CASES) and any(c[2] == 1 and c[1] > 1 for c in R.FWD_CASES)
    assert (1, 1, 1, 64, 64) in R.FWD_CASES
    # data-grad: both K walks, all three tiles, a padded source pitch
    d = [R.arm_of("fwd", (c[0], c[1], c[2], R.pad4(c[4]), R.pad4(c[3]))) for c in R.DGRAD_CASES]
    assert {a[:2] for a in d} == {(128, 128), (128, 64), (256, 32)} and {a[3] for a in d} == {False, True}
    assert any(c[3] % 4 for c in R.DGRAD_CASES) and any(c[4] % 4 for c in R.DGRAD_CASES)
    # weight-grad
    assert {R.arm_of("wgrad", c)[0] for c in R.WGRAD_CASES} == R.WGRAD_ARMS and len(R.WGRAD_ARMS) == 5
    g = {c: R.wgrad_edges(c) for c in R.WGRAD_CASES}
    assert any(v["ragged_split"] for v in g.values()) and any(v["splits"] >= 3 for v in g.values()) and any(v["splits"] == 1 for v in g.values())
    assert any(v["raster_wrap"] and c[1] * c[2] > 1 for c, v in g.items())
    assert any(v["cin_pad"] and v["tile"] == (64, 64) for v in g.values())
    assert any(v["ld_pad"] and c[5] % 4 for c, v in g.items())                     # the last 16-byte vector of a dy row straddles Cout
    for tile in R.WGRAD_ARMS - {"smallco", (64, 64)}:
        assert any(v["ragged_m"] for v in g.values() if v["tile"] == tile), tile
    assert any(c[1] == 1 and c[2] > 1 for c in R.WGRAD_CASES) and any(c[2] == 1 and c[1] > 1 for c in R.WGRAD_CASES)
    assert (1, 1, 1, 64, 64, 64, 64) in R.WGRAD_CASES
    # nothing above about 2000 pixels x 160 channels
    for c in list(R.FWD_CASES) + R.DGRAD_CASES + list(R.WGRAD_CASES):
        assert c[0] * c[1] * c[2] <= 2000 and max(c[3:]) <= 160


def test_arms_of_the_stated_cases():
    """The arm written beside every case is the arm arm_of computes, and the splits the comments name are the plan's."""
    for c, (bm, bn, c32) in R.FWD_CASES.items():
        for st in (False, True):
            assert R.arm_of("fwd", c, st) == (bm, bn, st, c32), c
    for c, tile in R.WGRAD_CASES.items():
        assert R.arm_of("wgrad", c)[0] == tile, c
    assert R.arm_of("wgrad", (2, 9, 13, 32, 32, 12, 12))[1] == (1, 256, 234)
    assert R.arm_of("wgrad", (3, 19, 23, 48, 48, 24, 24))[1] == (2, 672, 639)
    assert R.arm_of("wgrad", (2, 24, 40, 64, 64, 64, 64))[1] == (3, 640, 640)
    assert R.arm_of("wgrad", (40, 3, 5, 64, 64, 20, 20))[1] == (1, 608, 600)
    e = R.fwd_edges((3, 19, 23, 32, 64))
    assert (e["nK"], e["tilesM"], e["pb"], e["ragged_m"]) == (9, 11, True, True)
    e = R.fwd_edges((3, 19, 23, 4, 64))
    assert (e["nK"], e["taps_per_slice"]) == (2, 8)
    assert R.fwd_edges((2, 17, 31, 96, 48))["nK"] == 27 and R.fwd_edges((4, 41, 1, 20, 36))["nK"] == 6
    e = R.fwd_edges((3, 19, 23, 48, 24))
    assert e["partial_k"] and e["nK"] == 14
    assert R.fwd_edges((40, 3, 5, 64, 20))["images_per_tile"] >= 17
    assert R.fwd_edges((2, 9, 13, 36, 12))["straddle"]
