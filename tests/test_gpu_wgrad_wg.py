"""The capped-grid entry points of the two big fp32 weight-grad GEMMs (cvk_wgradp_gemm*_wg, cvk_w2d_gemm_tn_wg / cvk_w6_gemm_tn_wg): a workgroup of
a capped grid walks the jobs in a loop, a job owns its depth range and its slab / plane whichever workgroup runs it — so every cap, down to one
workgroup, gives bitwise the result of the full launch.  Every output buffer carries a NaN guard band behind it that must come back untouched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096        # floats of NaN behind every output


def _lib():
    from pytorch_camvid_amd import _lib as L
    return L.load(), L.check


def _s():
    return torch.cuda.current_stream().cuda_stream


def _guarded(n):
    """n output floats (NaN: every one must be written) + the guard band."""
    return torch.full((n + GUARD,), float("nan"), device="cuda")


def _check_guard(t, n, what):
    assert torch.isfinite(t[:n]).all(), what + ": output not fully written"
    assert torch.isnan(t[n:]).all(), what + ": wrote behind its output"


def _caps(njobs):
    """full (one workgroup per job), 3/4, 1/2 of it, one workgroup"""
    return [0, njobs * 3 // 4, njobs // 2, 1]


@pytest.mark.parametrize("Cin,Cout", [(64, 64), (128, 64)])
def test_plane_gemm_is_bitwise_independent_of_the_grid_cap(Cin, Cout):
    """The smallest geometry the plane-GEMM route accepts: N = 2, 64 x 128 (4096 tile rows; W % 4 == 0 for the four-plane form).  All three forms:
    row-major V, slice-major V, slice-major V with E0 / E5 read from dy."""
    lib, check = _lib()
    N, H, W = 2, 64, 128
    g = torch.Generator().manual_seed(7 + Cin + Cout)
    M = N * H * W
    x = torch.relu(torch.randn(N, H, W, Cin, generator=g)).cuda()
    slack = lib.cvk_wgradp_dy_slack(W) * Cout
    dyb = torch.zeros(M * Cout + slack, device="cuda")
    dyb[:M * Cout] = torch.randn(M * Cout, generator=g).cuda()
    rows = lib.cvk_wgradp_plane_rows(N, H, W)
    V, Vsm, E6 = (torch.full((6 * rows * c,), float("nan"), device="cuda") for c in (Cin, Cin, Cout))
    check(lib.cvk_wgradp_planes(x.data_ptr(), Cin, V.data_ptr(), N, H, W, Cin, 0, _s()), "planes(x)")
    check(lib.cvk_wgradp_planes_sm(x.data_ptr(), Cin, Vsm.data_ptr(), N, H, W, Cin, _s()), "planes_sm(x)")
    check(lib.cvk_wgradp_planes(dyb.data_ptr(), Cout, E6.data_ptr(), N, H, W, Cout, 1, _s()), "planes(dy)")
    E4p = E6[rows * Cout:5 * rows * Cout]
    wsb = lib.cvk_wgradp_gemm_workspace_bytes(N, H, W, Cin, Cout)
    runs = wsb // (4 * 6 * Cout * 3 * Cin)
    njobs = 6 * (Cin // 64) * (Cout // 64) * runs
    assert njobs >= 64, njobs
    nd = Cout * 9 * Cin
    forms = {"gemm": (lib.cvk_wgradp_gemm, lib.cvk_wgradp_gemm_wg, (E6.data_ptr(), V.data_ptr())),
             "gemm_sm": (lib.cvk_wgradp_gemm_sm, lib.cvk_wgradp_gemm_sm_wg, (E6.data_ptr(), Vsm.data_ptr())),
             "gemm_sm_dy": (lib.cvk_wgradp_gemm_sm_dy, lib.cvk_wgradp_gemm_sm_dy_wg, (E4p.data_ptr(), dyb.data_ptr(), Vsm.data_ptr()))}
    ref6 = None
    for name, (plain, capped, ops) in forms.items():
        ws = _guarded(wsb // 4)
        dw0 = _guarded(nd)
        check(plain(*ops, dw0.data_ptr(), N, H, W, Cin, Cin, Cout, ws.data_ptr(), wsb, _s()), name)
        torch.cuda.synchronize()
        _check_guard(dw0, nd, name)
        _check_guard(ws, wsb // 4, name + " slabs")
        slabs0 = ws[:wsb // 4].clone()
        for cap in _caps(njobs):
            ws = _guarded(wsb // 4)
            dw = _guarded(nd)
            check(capped(*ops, dw.data_ptr(), N, H, W, Cin, Cin, Cout, ws.data_ptr(), wsb, cap, _s()), name + "_wg")
            torch.cuda.synchronize()
            _check_guard(dw, nd, "%s_wg cap %d" % (name, cap))
            _check_guard(ws, wsb // 4, "%s_wg cap %d slabs" % (name, cap))
            assert torch.equal(ws[:wsb // 4], slabs0), (name, cap)
            assert torch.equal(dw[:nd], dw0[:nd]), (name, cap)
        if ref6 is None:
            ref6 = dw0[:nd].clone()
        else:       # the three forms read the same planes: one weight gradient
            assert torch.equal(dw0[:nd], ref6), name
    rc = lib.cvk_wgradp_gemm_wg(E6.data_ptr(), V.data_ptr(), dw0.data_ptr(), N, H, W, Cin, Cin, Cout, ws.data_ptr(), wsb, -1, _s())
    assert rc == -1 and b"max_workgroups" in lib.cvk_last_error_string()


@pytest.mark.parametrize("mt", [6, 4])
def test_transposed_2d_gemm_is_bitwise_independent_of_the_grid_cap(mt):
    """256 -> 256 at N = 2, 48 x 48 through F(6x6,3x3) and F(4x4,3x3): the partial planes P, and dw behind the fixed-order output pass."""
    lib, check = _lib()
    N, H, W, Cin, Cout = 2, 48, 48, 256, 256
    f = lambda name: getattr(lib, ("cvk_w6_" if mt == 6 else "cvk_w2d_") + name)
    g = torch.Generator().manual_seed(31 + mt)
    x = torch.relu(torch.randn(N, H, W, Cin, generator=g)).cuda()
    dy = torch.randn(N, H, W, Cout, generator=g).cuda()
    nx = (mt + 2) ** 2
    T = f("tiles")(N, H, W)
    Tp = lib.cvk_w2d_tpad(T)
    fs = f("wgrad_ksplit")(T, Cin, Cout)
    njobs = nx * ((Cout + 127) // 128) * ((Cin + 127) // 128) * fs
    V = torch.zeros(nx * Tp * Cin + 128, device="cuda")
    E = torch.zeros(nx * Tp * Cout + 128, device="cuda")
    check(f("input_transform")(x.data_ptr(), V.data_ptr(), N, H, W, Cin, _s()), "input")
    check(f("dy_transform")(dy.data_ptr(), Cout, E.data_ptr(), N, H, W, Cout, _s()), "dy")
    np_, nd = fs * nx * Cout * Cin, Cout * 9 * Cin

    def run(cap):
        P, dw = _guarded(np_), _guarded(nd)
        if cap is None:
            check(f("gemm_tn")(E.data_ptr(), V.data_ptr(), P.data_ptr(), T, Cin, Cout, _s()), "gemm_tn")
        else:
            check(f("gemm_tn_wg")(E.data_ptr(), V.data_ptr(), P.data_ptr(), T, Cin, Cout, cap, _s()), "gemm_tn_wg")
        check(f("wgrad_output")(P.data_ptr(), dw.data_ptr(), T, Cin, Cin, Cout, _s()), "wgrad_out")
        torch.cuda.synchronize()
        _check_guard(P, np_, "P cap %s" % cap)
        _check_guard(dw, nd, "dw cap %s" % cap)
        return P[:np_], dw[:nd]
    P0, dw0 = run(None)
    for cap in _caps(njobs):
        P, dw = run(cap)
        assert torch.equal(P, P0), (mt, cap)
        assert torch.equal(dw, dw0), (mt, cap)
    rc = f("gemm_tn_wg")(E.data_ptr(), V.data_ptr(), P0.data_ptr(), T, Cin, Cout, -1, _s())
    assert rc == -1 and b"max_workgroups" in lib.cvk_last_error_string()
