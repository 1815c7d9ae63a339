"""tests/wino2d_ref.py checked without a GPU: its fp64 references against torch.nn.functional, the transform matrices against the Winograd
identity in exact integer arithmetic, the rounding error that the tolerances of tests/test_gpu_wino2d.py are derived from (a numpy fp32
restatement of the transform chains of csrc/wino2d.hip against fp64), the coverage of every arm by the case tables, and the size cap of the
cases.  Run with -s for the figures that profiles/wino2d_margins.txt records."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import wino2d_ref as R

RAGGED = [(2, 5, 7, 12, 20), (1, 1, 9, 8, 4), (3, 6, 1, 4, 8), (1, 13, 11, 6, 5)]   # N, H, W, Cin, Cout


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
    for fwd, dgrad, wgrad in ((R.conv_fwd_ref, R.conv_dgrad_ref, R.conv_wgrad_ref), (R.conv_fwd_mm, R.conv_dgrad_mm, R.conv_wgrad_mm)):
        assert torch.allclose(fwd(x, w, b), y.detach().permute(0, 2, 3, 1), rtol=0, atol=1e-12)
        assert torch.allclose(fwd(x, w), (y.detach() - b.view(1, -1, 1, 1)).permute(0, 2, 3, 1), rtol=0, atol=1e-12)
        assert torch.allclose(dgrad(dy, w), xn.grad.permute(0, 2, 3, 1), rtol=0, atol=1e-12)
        assert torch.allclose(wgrad(x, dy), wn.grad.permute(0, 2, 3, 1), rtol=0, atol=1e-11)
    # the chain of reference passes is the operator, for both tiles: y = A^T [sum_ci (G g G^T) (.) (B^T d B)] A, dW = G^T [sum_t E (.) V] G
    yr = R.conv_fwd_ref(x, w)
    for mt in R.TILES:
        V, Vmag = R.planes_ref(R.BT[mt], R.tile_windows(mt, x))
        U, Umag = R.filter_planes_ref(mt, w)
        assert V.shape == (R.nx_of(mt), R.tiles(mt, N, H, W), Cin) and U.shape == (R.nx_of(mt), Cout, Cin)
        assert (Vmag >= V.abs() - 1e-12).all() and (Umag >= U.abs() - 1e-12).all()
        m = torch.einsum("xtk,xck->xtc", V, U)
        yy, ymag = R.output_ref(mt, m, N, H, W)
        assert torch.allclose(yy, yr, rtol=0, atol=1e-10) and (ymag >= yy.abs() - 1e-10).all()
        E, _ = R.planes_ref(R.A[mt], R.tile_windows(mt, dy, halo=False))
        P = torch.einsum("xtc,xtk->xck", E, V).reshape(R.nt_of(mt), R.nt_of(mt), Cout, Cin)
        Gt = torch.as_tensor(R.GT[mt])
        dw = torch.einsum("ra,abok,sb->orsk", Gt, P, Gt)
        assert torch.allclose(dw, R.conv_wgrad_ref(x, dy), rtol=0, atol=1e-9)
        # tile order and cropping: tile t of image n covers rows mt * ty .. and columns mt * tx ..
        th, tw = R.cdiv(H, mt), R.cdiv(W, mt)
        d = R.tile_windows(mt, x, halo=False)
        t = (N - 1) * th * tw + (th - 1) * tw + (tw - 1)
        hh, ww = H - mt * (th - 1), W - mt * (tw - 1)
        assert torch.equal(d[t, :hh, :ww], x[N - 1, mt * (th - 1):, mt * (tw - 1):]) and d[t].abs().sum() == d[t, :hh, :ww].abs().sum()
        # statistics partials: the counts add up, and every pixel's partial holds it
        cnt, pid = R.partial_counts(mt, N, H, W), R.partial_of_pixel(mt, N, H, W)
        assert sum(cnt) == N * H * W and torch.equal(torch.bincount(pid.flatten(), minlength=len(cnt)), torch.tensor(cnt))


@pytest.mark.parametrize("mt", R.TILES)
def test_winograd_identity_is_exact_on_integers(mt):
    """A^T [(G g G^T) (.) (B^T d B)] A is the correlation of d with g, checked in int64 on integer data with the integer multiples of the
    matrices (24 G, 90 G, 4 B^T, 32 A^T are integer matrices): no rounding anywhere.  The same for the transposes of the backward pass:
    G^T [(A dy A^T) (.) (B^T d B)] G is the weight gradient of one tile."""
    n = R.nt_of(mt)
    sg, sb, sa = R.INT_SCALE["G"][mt], R.INT_SCALE["BT"][mt], R.INT_SCALE["AT"][mt]

    def integer(M, s):
        Mi = np.rint(M * s).astype(np.int64)
        assert np.abs(Mi - M * s).max() < 1e-12, "not an integer multiple"
        return Mi
    Gi, Bi, Ai = integer(R.G[mt], sg), integer(R.BT[mt], sb), integer(R.AT[mt], sa)
    assert Gi.shape == (n, 3) and Bi.shape == (n, n) and Ai.shape == (mt, n)
    assert (integer(R.A[mt], sa) == Ai.T).all() and (integer(R.GT[mt], sg) == Gi.T).all()
    rng = np.random.default_rng(mt)
    for _ in range(8):
        d = rng.integers(-9, 10, (n, n)).astype(np.int64)
        g = rng.integers(-9, 10, (3, 3)).astype(np.int64)
        dy = rng.integers(-9, 10, (mt, mt)).astype(np.int64)
        V = Bi @ d @ Bi.T
        y = Ai @ ((Gi @ g @ Gi.T) * V) @ Ai.T
        want = np.array([[(d[i:i + 3, j:j + 3] * g).sum() for j in range(mt)] for i in range(mt)], dtype=np.int64)
        assert (y == (sg * sb * sa) ** 2 * want).all()
        dw = Gi.T @ ((Ai.T @ dy @ Ai) * V) @ Gi
        want = np.array([[(d[r:r + mt, s:s + mt] * dy).sum() for s in range(3)] for r in range(3)], dtype=np.int64)
        assert (dw == (sg * sb * sa) ** 2 * want).all()


@pytest.mark.parametrize("mt", R.TILES)
def test_restated_chains_are_the_operator(mt):
    """The fp32 restatements compute the convolution and its weight-grad (errors at rounding level, far from a wrong constant), and each
    restated 1-D routine is its matrix."""
    rng = np.random.default_rng(mt)
    x = np.maximum(rng.standard_normal((2, 7, 9, 8)), 0).astype(np.float32)
    w = rng.standard_normal((4, 3, 3, 8)).astype(np.float32)
    dy = rng.standard_normal((2, 7, 9, 4)).astype(np.float32)
    xt, wt, dyt = torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(dy)
    assert R.rel_l2(R.forward_chain_f32(mt, x, w), R.conv_fwd_ref(xt, wt).numpy()) < 5e-6
    assert R.rel_l2(R.wgrad_chain_f32(mt, x, dy), R.conv_wgrad_ref(xt, dyt).numpy()) < 5e-6
    n = R.nt_of(mt)
    for fn, M, k in ((R.bt_f32, R.BT[mt], n), (R.at_f32, R.AT[mt], n), (R.g_f32, R.G[mt], 3), (R.a_f32, R.A[mt], mt), (R.gt_f32, R.GT[mt], n)):
        v = rng.standard_normal((k, 5)).astype(np.float32)
        got = np.stack(fn(mt, [v[i] for i in range(k)])).astype(np.float64)
        assert np.abs(got - M @ v.astype(np.float64)).max() <= 1e-5 * (np.abs(M) @ np.abs(v)).max()
    # the single passes against their fp64 matrices, with the element-wise bounds the GPU test uses
    u = 2.0 ** -24
    V, Vmag = R.planes_ref(R.BT[mt], R.tile_windows(mt, xt))
    assert (np.abs(R.input_planes_f32(mt, x) - V.numpy()) <= 2 * R.BT_DEPTH[mt] * u * 1.001 * Vmag.numpy()).all()
    E, Emag = R.planes_ref(R.A[mt], R.tile_windows(mt, dyt, halo=False))
    assert (np.abs(R.dy_planes_f32(mt, dy) - E.numpy()) <= 2 * R.A_DEPTH[mt] * u * 1.001 * Emag.numpy()).all()
    U, Umag = R.filter_planes_ref(mt, wt)
    assert (np.abs(R.filter_planes_f32(mt, w) - U.numpy()) <= 2 * R.G_DEPTH[mt] * u * 1.001 * Umag.numpy()).all()
    m = rng.standard_normal((R.nx_of(mt), R.tiles(mt, 2, 7, 9), 4)).astype(np.float32)
    yy, ymag = R.output_ref(mt, torch.from_numpy(m), 2, 7, 9)
    assert (np.abs(R.output_f32(mt, m, 2, 7, 9) - yy.numpy()) <= (R.OUT_DEPTH[mt] - 1) * u * 1.001 * ymag.numpy()).all()


@pytest.mark.parametrize("kind", ["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("mt", R.TILES)
def test_chain_rounding(kind, mt):
    """Where the tolerances come from: the relative L2 rounding error of the fp32 restatement against fp64 at depths 32 and 512 (input
    channels; weight-grad: tiles), for the whole tensor and for the worst image row of y / output channel of dW.  wino2d_ref.MEASURED holds
    these figures; bound() is 3 x (weight-grad: 6 x) their interpolation in the depth.  Every chain grows about as the square root of its
    depth; F(6x6) rounds about twice as coarsely as F(4x4) (transform constants up to 32 and 5.25)."""
    k0, k1 = R.DEPTHS[kind]
    for K in (k0, k1):
        whole, row = R.measure_chain(kind, mt, K)
        print(f"[wino2d restatement] {kind} F({mt}x{mt}) depth {K}: whole {whole:.3e}, worst row {row:.3e}; "
              f"bounds {R.bound(kind, mt, K, 0):.3e} / {R.bound(kind, mt, K, 1):.3e}")
        for got, rec in zip((whole, row), R.MEASURED[(kind, mt, K)]):
            assert abs(got - rec) <= 0.1 * rec, (kind, mt, K, got, rec)
        assert whole <= row < 2.5 * whole
    e0, e1 = R.MEASURED[(kind, mt, k0)][0], R.MEASURED[(kind, mt, k1)][0]
    assert 2.5 < e1 / e0 < 4.0 * 1.2                       # sqrt(512 / 32) = 4
    assert 1.5 < R.MEASURED[(kind, 6, k0)][0] / R.MEASURED[(kind, 4, k0)][0] < 3.0
    f = 6.0 if kind == "wgrad" else 3.0
    for which in (0, 1):
        assert math.isclose(R.bound(kind, mt, k0, which), f * R.MEASURED[(kind, mt, k0)][which], rel_tol=1e-12)
        assert math.isclose(R.bound(kind, mt, k1, which), f * R.MEASURED[(kind, mt, k1)][which], rel_tol=1e-12)
        assert R.bound(kind, mt, k0, which) <= R.bound(kind, mt, 256, which) <= R.bound(kind, mt, k1, which)
        assert R.bound(kind, mt, 4 * k1, which) == R.bound(kind, mt, k1, which)          # clamped: no extrapolation


@pytest.mark.parametrize("mt", R.TILES)
def test_figures_of_test_gpu_w6_are_reproduced(mt):
    """tests/test_gpu_w6.py quotes 1.4e-6 / 2.7e-6 for F(4x4) and 2.7e-6 / 5.1e-6 for F(6x6) at 64 / 256 input channels for the forward chain:
    this restatement gives the same within 20 % (another shape and seed), and bound() at those depths stays within 20 % of 3 x the quoted
    figure, so the two files' tolerances are the same rule."""
    quoted = {(4, 64): 1.4e-6, (4, 256): 2.7e-6, (6, 64): 2.7e-6, (6, 256): 5.1e-6}
    for Cin in (64, 256):
        whole, _ = R.measure_chain("fwd", mt, Cin)
        print(f"[wino2d restatement] fwd F({mt}x{mt}) Cin={Cin}: whole {whole:.3e} (tests/test_gpu_w6.py: {quoted[(mt, Cin)]:.1e})")
        assert abs(whole - R.MEASURED_W6_DOC[(mt, Cin)]) <= 0.1 * R.MEASURED_W6_DOC[(mt, Cin)]
        assert abs(whole - quoted[(mt, Cin)]) <= 0.2 * quoted[(mt, Cin)]
        assert abs(R.bound("fwd", mt, Cin, 0) - 3 * quoted[(mt, Cin)]) <= 0.2 * 3 * quoted[(mt, Cin)]


@pytest.mark.parametrize("mt", R.TILES)
def test_case_tables_cover_every_arm(mt):
    """Fails when a case is dropped: over the tables, arm_of reaches every kind of GEMM round, K split and store path, every (cvn, ragged)
    block shape of the output pass, both block heights, and for the weight-grad every depth split (at its cap, uneven, none) and every
    combination of ragged tiles."""
    fw = [R.arm_of("fwd", mt, c) for c in R.FWD_CASES]
    dg = [R.arm_of("dgrad", mt, c) for c in R.DGRAD_CASES]
    out = [R.arm_of("out", mt, c) for c in R.OUT_CASES[mt]]
    for arms in (fw, fw + dg + out):
        if arms is fw:
            assert {a[2] for a in arms} == R.FWD_ARMS["rounds"]
            assert {a[3] for a in arms} == R.FWD_ARMS["f"]
            assert {a[4] for a in arms} == R.FWD_ARMS["store"]
            assert {(a[5], a[6]) for a in arms} == R.FWD_ARMS["out"][mt]
        else:
            assert {a[7] for a in arms} == R.FWD_ARMS["TB"]
    assert {a[7] for a in out} == {4, 16} and all(a[2:4] == ("one", 1) for a in out)
    # the arms of the issue, by name
    assert any(a[2] == "full+split" and a[3] == 2 for a in fw) and any(a[2] == "full+split" and a[3] == 4 for a in fw)
    assert any(a[2] == "full+split" for a in dg) and any(a[6] for a in dg)
    assert any(a[2] == "split-all" and a[4] == "raw+checked" and a[6] for a in fw)
    assert any(a[4] == "checked" and a[6] for a in fw)                      # a ragged column tile that is the only one, wider than 64
    assert any(c[4] % 8 for c in R.FWD_CASES) and any(len(c) > 5 and c[5] > c[4] for c in R.FWD_CASES)
    assert any(c[1] == 1 for c in R.FWD_CASES) and any(c[2] == 1 for c in R.FWD_CASES)
    wg = [R.arm_of("wgrad", mt, c) for c in R.WGRAD_CASES]
    assert {a[2] for a in wg} == R.WGRAD_ARMS["f"][mt]
    assert {a[3] for a in wg if a[2] > 1} == R.WGRAD_ARMS["even_split"]
    assert {a[4:6] for a in wg} == R.WGRAD_ARMS["ragged"]
    assert any(c[3] < c[4] for c in R.WGRAD_CASES) and any(c[4] % 32 for c in R.WGRAD_CASES) and any(c[6] > c[5] for c in R.WGRAD_CASES)
    plans = [R.plan_wgrad(mt, R.tiles(mt, *c[:3]), c[4], c[5]) for c in R.WGRAD_CASES]
    assert any(p["tilesM"] == 2 and p["tilesN"] == 2 for p in plans)


def test_arms_of_the_stated_cases():
    """The arms the case tables are there for, as the planners' restatement derives them."""
    def fw(mt, c):
        T = R.tiles(mt, *c[:3])
        p = R.plan_fwd(mt, T, c[3], c[4])
        return (T, p["NT"], p["split_start"], p["f"])
    assert fw(4, (1, 96, 102, 256, 384)) == (624, 540, 512, 2) and fw(6, (1, 96, 102, 256, 384)) == (272, 576, 512, 2)
    assert fw(4, (1, 96, 102, 512, 384)) == (624, 540, 512, 4) and fw(6, (1, 96, 102, 512, 384)) == (272, 576, 512, 4)
    assert fw(6, (8, 45, 60, 512, 256))[1:] == (640, 512, 4)                # the batch-8 step's 512 -> 256 layer at 45 x 60 under F(6x6)
    for mt in R.TILES:
        assert R.arm_of("fwd", mt, (1, 48, 102, 512, 132))[2:5] == ("split-all", 2, "raw+checked")
        assert R.arm_of("fwd", mt, (1, 44, 44, 384, 136))[3] == 3
        assert R.arm_of("fwd", mt, (1, 13, 11, 288, 320))[3] == 2 and R.plan_fwd(mt, R.tiles(mt, 1, 13, 11), 288, 320)["tilesN"] == 3
        assert R.arm_of("fwd", mt, (1, 9, 13, 64, 132))[2:5] == ("one", 1, "raw+checked")
        assert R.arm_of("out", mt, R.OUT_CASES[mt][0])[7] == 16 and R.tiles(mt, *R.OUT_CASES[mt][0][:3]) == 8281
    assert R.arm_of("fwd", 4, (3, 5, 7, 32, 68))[4:7] == ("checked", 16, True) and R.arm_of("fwd", 6, (1, 1, 9, 96, 100))[4:7] == ("checked", 32, True)
    assert R.tb(8191) == 4 and R.tb(8192) == 16

    def wg(mt, c):
        p = R.plan_wgrad(mt, R.tiles(mt, *c[:3]), c[4], c[5])
        return (p["f"], p["nK"])
    assert wg(4, (1, 180, 180, 32, 32, 64, 64)) == (16, 64) and wg(6, (1, 180, 180, 32, 32, 64, 64)) == (7, 29)
    assert wg(6, (1, 270, 270, 32, 32, 64, 64)) == (16, 64) and wg(4, (1, 270, 270, 32, 32, 64, 64)) == (16, 145)
    assert wg(4, (1, 50, 131, 32, 36, 68, 72)) == (3, 14)
    assert R.stat_depth(4, 100, 64) == 16 + 16 and R.stat_depth(6, 100, 256) == 36 + 4 and R.stat_depth(4, 8281, 64) == 16 + 16
    assert R.stat_depth(6, 8281, 64) == 2 * 36 + 8 and R.stat_depth(4, 8281, 256) == 4 * 16 + 4


@pytest.mark.parametrize("mt", R.TILES)
def test_no_case_is_workload_sized(mt):
    """Nobody covers an arm with a workload-sized case: no device buffer of any case holds more than 2^27 floats."""
    for kind, table in (("fwd", R.FWD_CASES), ("dgrad", R.DGRAD_CASES), ("out", R.OUT_CASES[mt]), ("wgrad", R.WGRAD_CASES)):
        for c in table:
            sizes = R.case_buffers(kind, mt, c)
            assert max(sizes.values()) <= R.SIZE_CAP, (kind, mt, c, sizes)
