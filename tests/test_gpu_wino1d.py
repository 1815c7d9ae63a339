"""Raw C-ABI parity of the 1-D Winograd conv kernels, arm by arm: csrc/wino.hip (F(2,3): cvk_wino_* / cvk_conv3x3_wino_*, `fam` 2) and
csrc/wino4.hip (per-index F(4,3): cvk_wino4_* / cvk_conv3x3_wino4_*, `fam` 4) against the fp64 operator they replace,
nn.Conv2d(cin, cout, 3, padding=1): forward with the BatchNorm statistics partials, data-grad, weight-grad, the E planes of the
F(4,3) weight-grad, and the host-side argument contract.

tests/wino1d_ref.py holds the references, the case tables with the arm each case is there for (tests/test_wino1d_ref_cpu.py asserts that
they cover every instantiation) and the tolerances: bound(kind, fam, Cin, which) is 3 x (weight-grad 6 x) the rounding error of a numpy fp32
restatement of the kernels' transform chains against fp64, for the whole tensor (which = 0) and for the worst image row of y / output
channel of dW (which = 1).  Every output and workspace buffer is NaN-filled and followed by a guard band that must stay untouched.
Run with -s for the used fraction of every bound (profiles/wino1d_margins.txt)."""
import functools
import math

import pytest
import torch

from tests import wino1d_ref as R

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
SENTINEL = -7.0
EINVAL, EWORKSPACE = -1, -2


def _lib():
    from pytorch_camvid_amd import _lib
    return _lib.load(), _lib.check


def _s():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """n NaN floats on the device followed by a guard band of R.GUARD sentinels."""

    def __init__(self, n, fill=float("nan")):
        self.n = int(n)
        self.raw = torch.full((self.n + R.GUARD,), fill, device="cuda")
        self.raw[self.n:] = SENTINEL
        self.t = self.raw[:self.n]

    def ptr(self):
        return self.raw.data_ptr()

    def check_guard(self, what):
        assert bool((self.raw[self.n:] == SENTINEL).all()), f"{what}: guard band written"


def _used(tag, value, bound):
    print(f"[wino1d] {tag}: {value:.3e} = {value / bound:.3f} of its bound {bound:.3e}")
    return value


def _rel(got, ref):
    return ((got - ref).norm() / ref.norm()).item()


def _worst_row(got, ref, rows):
    e = (got - ref).reshape(rows, -1).norm(dim=1)
    return (e / ref.reshape(rows, -1).norm(dim=1)).max().item()


def _weights(fam, w, Cn, Ck, dgrad=False):
    """U [planes][Cn][3][Ck] on the device.  forward: from w [Cn][3][3][Ck].  dgrad: from the layer's w [Ck][3][3][Cn] — family 4 in one step
    (cvk_wino4_weight_transform_dgrad), family 2 through cvk_pack_weight_dgrad."""
    lib, check = _lib()
    U = Buf(R.nplanes(fam) * Cn * 3 * Ck)
    wd = w.cuda()
    if not dgrad:
        fn = lib.cvk_wino_weight_transform if fam == 2 else lib.cvk_wino4_weight_transform
        check(fn(wd.data_ptr(), U.ptr(), Cn, Ck, _s()), "weight transform")
    elif fam == 4:
        check(lib.cvk_wino4_weight_transform_dgrad(wd.data_ptr(), U.ptr(), Ck, Cn, _s()), "weight transform (dgrad)")
    else:
        packed = Buf(Cn * 9 * Ck)
        check(lib.cvk_pack_weight_dgrad(wd.data_ptr(), packed.ptr(), Ck, Cn, Cn, Ck, _s()), "pack (dgrad)")
        check(lib.cvk_wino_weight_transform(packed.ptr(), U.ptr(), Cn, Ck, _s()), "weight transform")
        torch.cuda.synchronize()
        packed.check_guard("packed weights")
    torch.cuda.synchronize()
    U.check_guard("U")
    assert bool(torch.isfinite(U.t).all())
    return U


def _pipeline(fam, xd, U, Cn, ldm, bias, stats):
    """gemm + output on x [N][H][W][Ck] (device).  Returns y [N][H][W][ldm] and the statistics partials [2][P][Cn] (or None), both on the device;
    asserts the planner restatement against the library's queries, and the guard bands."""
    lib, check = _lib()
    N, H, W, Ck = xd.shape
    p = R.plan_fwd(fam, N, H, W, Ck, ldm)
    if fam == 4:
        assert lib.cvk_conv3x3_wino4_ksplit(N, H, W, Ck, ldm) == p["ksplit"]
        assert lib.cvk_conv3x3_wino4_workspace_bytes(N, H, W, Ck, ldm) == 4 * 6 * p["ksplit"] * p["Mt"] * ldm
    else:
        assert lib.cvk_conv3x3_wino_workspace_bytes(N, H, W, ldm) == 4 * 4 * p["Mt"] * ldm
    Mo = Buf(R.nplanes(fam) * p["ksplit"] * p["Mt"] * ldm)
    y = Buf(N * H * W * ldm)
    P = R.cdiv(N * H * W, R.STAT_ROWS)
    st = Buf(2 * P * Cn) if stats else None
    bp = bias.data_ptr() if bias is not None else None
    sp = st.ptr() if stats else None
    if fam == 4:
        check(lib.cvk_conv3x3_wino4_gemm(xd.data_ptr(), U.ptr(), Mo.ptr(), N, H, W, Ck, Cn, ldm, _s()), "gemm")
        check(lib.cvk_wino4_output(Mo.ptr(), bp, y.ptr(), sp, N, H, W, Cn, ldm, p["ksplit"], _s()), "output")
    else:
        check(lib.cvk_conv3x3_wino_gemm(xd.data_ptr(), U.ptr(), Mo.ptr(), N, H, W, Ck, Cn, ldm, _s()), "gemm")
        check(lib.cvk_wino_output(Mo.ptr(), bp, y.ptr(), sp, N, H, W, Cn, ldm, _s()), "output")
    torch.cuda.synchronize()
    for b, what in ((Mo, "Mo"), (y, "y"), (st, "stats")):
        if b is not None:
            b.check_guard(what)
    assert bool(torch.isfinite(Mo.t).all()), "a product plane element was never written"
    yv = y.t.view(N, H, W, ldm)
    assert bool(torch.isfinite(yv).all())
    if ldm > Cn:
        assert bool((yv[..., Cn:] == 0).all()), "columns [Cout, ldm) of y must read 0"
    return yv, (st.t.view(2, P, Cn) if stats else None)


def _check_y(tag, kind, fam, Ck, got, ref, factor=1.0):
    """got / ref [rows][...] double on one device: whole-tensor and worst-row relative L2 against the derived bounds."""
    rows = ref.shape[0]
    b0, b1 = factor * R.bound(kind, fam, Ck, 0), factor * R.bound(kind, fam, Ck, 1)
    whole = _used(f"{tag} whole", _rel(got, ref), b0)
    row = _used(f"{tag} worst row", _worst_row(got, ref, rows), b1)
    assert whole < b0, (tag, whole, b0)
    assert row < b1, (tag, row, b1)


def _granules(t, P):
    """[M][C] -> [P][64][C], the last granule zero-padded."""
    pad = P * R.STAT_ROWS - t.shape[0]
    return torch.cat([t, torch.zeros(pad, t.shape[1], dtype=t.dtype, device=t.device)]).view(P, R.STAT_ROWS, t.shape[1])


def _check_stats(tag, fam, Ck, st, ref, bias, own):
    """st [2][P][C] from the kernel; ref [M][C] the fp64 y; own [M][C] the y the kernel wrote, in double (all on one device).
    1. Chan's combination against the mean and variance of ref, with the bounds of tests/test_gpu_w6.py.
    2. The per-granule sums against the fp64 granule sums of ref:  sum_{p,c} (dsum)^2 <= 64 sum (dy)^2 by Cauchy-Schwarz over the 64 pixels
       of a granule, so |dsum|_2 <= 8 bound_y |y|_2, plus the accumulation term of 3.
    3. The per-granule sums against the fp64 granule sums of the kernel's own y, element by element: what is left is the kernel's fp32
       accumulation alone.  It forms d = y - b (one rounding), adds the up to 64 d of a granule (63 roundings, each at most u sum|d|) and
       restores the bias with cnt * b + sum (two roundings of at most u (sum|d| + cnt |b|)): |dsum| <= 66 u (sum|y - b| + cnt |b|)."""
    M, C = ref.shape
    P = st.shape[1]
    cnt = torch.full((P,), float(R.STAT_ROWS), dtype=torch.float64, device=ref.device)
    cnt[-1] = M - (P - 1) * R.STAT_ROWS
    b = torch.zeros(C, dtype=torch.float64, device=ref.device) if bias is None else bias.double()
    sums, m2 = st[0].double(), st[1].double()
    assert bool((m2 >= 0).all())
    absum = _granules((own - b).abs(), P).sum(1) + cnt[:, None] * b.abs()
    cap = 66 * U24 * (1 + 2.0 ** -16) * absum
    err = (sums - _granules(own, P).sum(1)).abs()
    assert bool((err <= cap).all()), (tag, (err - cap).max().item())
    print(f"[wino1d] {tag} granule sums of the kernel's own y: largest error = {(err / cap.clamp_min(1e-300)).max().item():.3f} of its bound")
    bound = 8 * R.bound("fwd", fam, Ck, 0) * ref.norm().item() + 66 * U24 * absum.norm().item()
    err = _used(f"{tag} granule sums", (sums - _granules(ref, P).sum(1)).norm().item(), bound)
    assert err < bound, (tag, err, bound)
    mean, var = R.chan_combine(sums, m2, cnt)
    rmean, rvar = ref.mean(0), ref.var(0, unbiased=False)
    assert (mean - rmean).abs().max().item() < 1e-5 * max(1.0, rmean.abs().max().item()), tag
    assert bool(((var - rvar).abs() <= 1e-4 * rvar + 1e-6 * (ref ** 2).mean(0)).all()), tag


@functools.lru_cache(maxsize=None)
def _fwd_data(case):
    """Seeded on the CPU, shared by both families: post-ReLU activations, He-scaled filter, bias, and the fp64 reference."""
    N, H, W, Cin, Cout = case[:5]
    g = torch.Generator().manual_seed(1000 * N + 10 * H + W + Cin + 3 * Cout)
    x = torch.relu(torch.randn(N, H, W, Cin, generator=g))
    w = torch.randn(Cout, 3, 3, Cin, generator=g) * math.sqrt(2.0 / (9 * Cin))
    b = torch.randn(Cout, generator=g)
    return x, w, b, R.conv_fwd_ref(x, w, b)


@pytest.mark.parametrize("fam", [2, 4])
@pytest.mark.parametrize("case", R.FWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_forward_and_statistics_vs_fp64(fam, case):
    N, H, W, Cin, Cout = case[:5]
    ldm = case[5] if len(case) > 5 else Cout
    x, w, b, ref = _fwd_data(case)
    tag = f"fwd F({fam},3) {case}"
    print(f"[wino1d] {tag}: arm {R.arm_of('fwd', fam, case)}")
    xd, bd = x.cuda(), b.cuda()
    U = _weights(fam, w, Cout, Cin)
    refd = ref.cuda().reshape(N * H, W, Cout)
    y, st = _pipeline(fam, xd, U, Cout, ldm, bd, True)
    _check_y(tag, "fwd", fam, Cin, y[..., :Cout].double().reshape(N * H, W, Cout), refd)
    _check_stats(tag, fam, Cin, st, refd.reshape(-1, Cout), bd, y[..., :Cout].double().reshape(-1, Cout))
    # stats = NULL
    y1, _ = _pipeline(fam, xd, U, Cout, ldm, bd, False)
    _check_y(tag + " stats=NULL", "fwd", fam, Cin, y1[..., :Cout].double().reshape(N * H, W, Cout), refd)
    # bias = NULL
    nob = refd - bd.double()
    y2, st2 = _pipeline(fam, xd, U, Cout, ldm, None, True)
    _check_y(tag + " bias=NULL", "fwd", fam, Cin, y2[..., :Cout].double().reshape(N * H, W, Cout), nob)
    _check_stats(tag + " bias=NULL", fam, Cin, st2, nob.reshape(-1, Cout), None, y2[..., :Cout].double().reshape(-1, Cout))


@pytest.mark.parametrize("fam,case", [(f, c) for f in (2, 4) for c in R.FWD_BIG_CASES[f]], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_forward_multi_index_blocks_and_wide_chunk(fam, case):
    """The nfull arm: 256 blocks that walk every transform index and 2 tiles cut into single-index blocks, output chunk 1024.  fp64 on the
    first and last row of each image and on the image rows around the Mo row where the single-index tiles begin (128 * nfull / tilesN);
    the whole tensor against cvk_conv3x3_fwd at twice the tolerance (both sides carry fp32 rounding)."""
    lib, check = _lib()
    N, H, W, Cin, Cout = case
    p = R.plan_fwd(fam, N, H, W, Cin, Cout)
    assert (p["tiles"], p["nfull"]) == (258, 256) and R.output_chunk(fam, N, H, W, Cout) == 1024
    tag = f"fwd F({fam},3) {case}"
    print(f"[wino1d] {tag}: arm {R.arm_of('fwd', fam, case)}")
    g = torch.Generator().manual_seed(W + Cout)
    x = torch.relu(torch.randn(N, H, W, Cin, generator=g))
    w = torch.randn(Cout, 3, 3, Cin, generator=g) * math.sqrt(2.0 / (9 * Cin))
    b = torch.randn(Cout, generator=g)
    edge = (128 * p["nfull"] // p["tilesN"]) // p["Wt"]
    rows = sorted({n * H + y for n in range(N) for y in (0, H - 1)} | {edge - 1, edge, edge + 1})
    ref = R.conv_fwd_ref_rows(x, w, b, rows).cuda()
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    U = _weights(fam, w, Cout, Cin)
    y, st = _pipeline(fam, xd, U, Cout, Cout, bd, True)
    yd = y.double().reshape(N * H, W, Cout)
    _check_y(tag + " fp64 rows", "fwd", fam, Cin, yd[rows], ref)
    direct = Buf(N * H * W * Cout)
    check(lib.cvk_conv3x3_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), direct.ptr(), None, N, H, W, Cin, Cout, Cout, _s()), "direct")
    torch.cuda.synchronize()
    direct.check_guard("direct y")
    _check_y(tag + " against cvk_conv3x3_fwd", "fwd", fam, Cin, yd, direct.t.double().view(N * H, W, Cout), factor=2.0)
    # the statistics of the tensor the kernel wrote (itself checked above)
    _check_stats(tag, fam, Cin, st, yd.reshape(-1, Cout), bd, yd.reshape(-1, Cout))


@functools.lru_cache(maxsize=None)
def _dgrad_data(case):
    """The forward table read as data-grads: dy has the case's Cin channels (what the gemm reduces over), dx its Cout channels — the
    layer is Conv2d(case Cout -> case Cin) with filter w [case Cin][3][3][case Cout]."""
    N, H, W, Ck, Cn = case[:5]
    g = torch.Generator().manual_seed(7 + 1000 * N + 10 * H + W + Ck + 3 * Cn)
    w = torch.randn(Ck, 3, 3, Cn, generator=g) * math.sqrt(2.0 / (9 * Cn))
    dy = torch.randn(N, H, W, Ck, generator=g)
    return w, dy, R.conv_dgrad_ref(dy, w)


@pytest.mark.parametrize("fam", [2, 4])
@pytest.mark.parametrize("case", R.FWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_data_grad_vs_fp64(fam, case):
    N, H, W, Ck, Cn = case[:5]
    ldm = case[5] if len(case) > 5 else Cn
    w, dy, ref = _dgrad_data(case)
    tag = f"dgrad F({fam},3) {case}"
    U = _weights(fam, w, Cn, Ck, dgrad=True)
    dx, _ = _pipeline(fam, dy.cuda(), U, Cn, ldm, None, False)
    _check_y(tag, "dgrad", fam, Ck, dx[..., :Cn].double().reshape(N * H, W, Cn), ref.cuda().reshape(N * H, W, Cn))


@pytest.mark.parametrize("Cout,Cin", [(64, 64), (40, 96), (128, 36), (7, 5)])
def test_wino4_dgrad_weights_equal_pack_then_transform(Cout, Cin):
    """include/cvk.h: cvk_wino4_weight_transform_dgrad == cvk_pack_weight_dgrad without padding followed by cvk_wino4_weight_transform,
    bit for bit (both evaluate G g in double from the same three floats and round once); and both are the fp64 G g of the rotated,
    channel-transposed filter rounded to fp32."""
    lib, check = _lib()
    g = torch.Generator().manual_seed(Cout * 1000 + Cin)
    w = torch.randn(Cout, 3, 3, Cin, generator=g)
    one = _weights(4, w, Cin, Cout, dgrad=True)
    packed = Buf(Cin * 9 * Cout)
    two = Buf(6 * Cin * 3 * Cout)
    check(lib.cvk_pack_weight_dgrad(w.cuda().data_ptr(), packed.ptr(), Cout, Cin, Cin, Cout, _s()), "pack")
    check(lib.cvk_wino4_weight_transform(packed.ptr(), two.ptr(), Cin, Cout, _s()), "transform")
    torch.cuda.synchronize()
    packed.check_guard("packed")
    two.check_guard("U")
    assert torch.equal(packed.t.view(Cin, 3, 3, Cout).cpu(), R.dgrad_filter(w))
    assert torch.equal(one.t, two.t)
    Gm = torch.from_numpy(R.G[4])
    want = torch.einsum("xs,crsk->xcrk", Gm, R.dgrad_filter(w).double()).float()      # [6][Cin][3][Cout]
    # double arithmetic rounded once: at most one fp32 ulp from the exactly rounded value (the sums of thirds are not exact in double either)
    got = one.t.view(6, Cin, 3, Cout).cpu()
    assert bool(((got - want).abs() <= want.abs() * 2.0 ** -23).all())


@functools.lru_cache(maxsize=None)
def _wgrad_data(case):
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    g = torch.Generator().manual_seed(11 + 1000 * N + 10 * H + W + Cin + 3 * Cout)
    x = torch.zeros(N, H, W, Cin_pad)
    x[..., :Cin] = torch.relu(torch.randn(N, H, W, Cin, generator=g))
    dy = torch.full((N, H, W, ld_dy), 7.0)                      # columns [Cout, ld_dy) belong to nobody: they must not reach dW
    dy[..., :Cout] = torch.randn(N, H, W, Cout, generator=g)
    return x, dy, R.conv_wgrad_ref(x[..., :Cin], dy[..., :Cout])


def _wgrad_call(fam, xd, dyd, case, ws, E_pre=None):
    lib, check = _lib()
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    dw = Buf(Cout * 9 * Cin)
    if fam == 4:
        check(lib.cvk_conv3x3_wgrad_wino4(xd.data_ptr(), dyd.data_ptr(), E_pre, dw.ptr(), N, H, W, Cin, Cin_pad, Cout, ld_dy, ws.ptr(), 4 * ws.n,
                                          _s()), "wgrad")
    else:
        check(lib.cvk_conv3x3_wgrad_wino(xd.data_ptr(), dyd.data_ptr(), dw.ptr(), N, H, W, Cin, Cin_pad, Cout, ld_dy, ws.ptr(), 4 * ws.n, _s()),
              "wgrad")
    torch.cuda.synchronize()
    dw.check_guard("dW")
    ws.check_guard("workspace")
    assert bool(torch.isfinite(dw.t).all())
    return dw.t.view(Cout, 3, 3, Cin)


def _wgrad_ws_floats(fam, case):
    """Workspace size from the library's query; asserts that the slab count it implies is the restatement's."""
    lib, _ = _lib()
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    p = R.plan_wgrad(fam, N, H, W, Cin_pad, Cout)
    if fam == 4:
        nbytes = lib.cvk_conv3x3_wgrad_wino4_workspace_bytes(N, H, W, Cin_pad, Cout, ld_dy)
        slab = nbytes // 4 - 4 * N * H * p["Wt"] * ld_dy
    else:
        nbytes = lib.cvk_conv3x3_wgrad_wino_workspace_bytes(N, H, W, Cin_pad, Cout)
        slab = nbytes // 4
    per = R.nplanes(fam) * Cout * 3 * Cin_pad
    assert nbytes % 4 == 0 and slab % per == 0 and slab // per == p["splits"], (nbytes, p)
    assert nbytes == 4 * R.wgrad_workspace_floats(fam, N, H, W, Cin_pad, Cout, ld_dy)
    return nbytes // 4


@pytest.mark.parametrize("fam", [2, 4])
@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_weight_grad_vs_fp64(fam, case):
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    x, dy, ref = _wgrad_data(case)
    tag = f"wgrad F({fam},3) {case}"
    print(f"[wino1d] {tag}: arm {R.arm_of('wgrad', fam, case)}")
    xd, dyd = x.cuda(), dy.cuda()
    n = _wgrad_ws_floats(fam, case)
    outs = [_wgrad_call(fam, xd, dyd, case, Buf(n)) for _ in range(2)]
    assert torch.equal(outs[0], outs[1])
    _check_y(tag, "wgrad", fam, Cin, outs[0].double(), ref.cuda())          # rows of dW: output channels


@pytest.mark.parametrize("case", R.EPRE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_wgrad_wino4_e_planes_and_e_pre(case):
    """E_pre = NULL leaves E1..E4 = A dy at the head of the workspace: against fp64, where every element passes through two fp32 roundings
    of at most u times sum |coefficient * dy| each (k_wino4_dy_transform adds pairs, then the pairs).  The same planes handed back as E_pre
    give bitwise the same dW and the head of the workspace stays unwritten."""
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    x, dy, ref = _wgrad_data(case)
    xd, dyd = x.cuda(), dy.cuda()
    n = _wgrad_ws_floats(4, case)
    ne = 4 * N * H * R.cdiv(W, 4) * ld_dy
    ws = Buf(n)
    first = _wgrad_call(4, xd, dyd, case, ws).clone()
    E = ws.t[:ne].clone()
    Eref, Eabs = R.e_planes_ref(dy, ld_dy)
    err = (E.double().cpu().view_as(Eref) - Eref).abs()
    cap = 2.0 * U24 * (1 + 2.0 ** -20) * Eabs
    assert bool((err <= cap).all()), (err - cap).max().item()
    print(f"[wino1d] E planes {case}: largest error = {(err / cap.clamp_min(1e-300)).max().item():.3f} of its bound")
    ws2 = Buf(n)
    second = _wgrad_call(4, xd, dyd, case, ws2, E_pre=E.data_ptr())
    assert torch.equal(first, second)
    assert bool(torch.isnan(ws2.t[:ne]).all()), "with E_pre the E region of the workspace must stay unwritten"
    _check_y(f"wgrad F(4,3) E_pre {case}", "wgrad", 4, Cin, second.double(), ref.cuda())


def _err():
    lib, _ = _lib()
    return lib.cvk_last_error_string().decode()


@pytest.mark.parametrize("fam", [2, 4])
def test_host_side_contract(fam):
    """Every rejection returns before any launch: the NaN-filled outputs stay NaN, and cvk_last_error_string names the entry point."""
    lib, _ = _lib()
    N, H, W, Cin, Cout = 1, 4, 8, 64, 64
    x, dy = torch.zeros(N, H, W, Cin, device="cuda"), torch.zeros(N, H, W, Cout, device="cuda")
    U, Mo, y, dw = Buf(6 * Cout * 3 * Cin), Buf(6 * 3 * N * H * W * Cout), Buf(N * H * W * Cout), Buf(Cout * 9 * Cin)
    case = (N, H, W, Cin, Cin, Cout, Cout)
    n = _wgrad_ws_floats(fam, case)
    ws = Buf(n)
    if fam == 4:
        gemm, gname, wname = lib.cvk_conv3x3_wino4_gemm, "cvk_conv3x3_wino4_gemm", "cvk_conv3x3_wgrad_wino4"

        def wgrad(ld_dy, nbytes):
            return lib.cvk_conv3x3_wgrad_wino4(x.data_ptr(), dy.data_ptr(), None, dw.ptr(), N, H, W, Cin, Cin, Cout, ld_dy, ws.ptr(), nbytes, _s())
    else:
        gemm, gname, wname = lib.cvk_conv3x3_wino_gemm, "cvk_conv3x3_wino_gemm", "cvk_conv3x3_wgrad_wino"

        def wgrad(ld_dy, nbytes):
            return lib.cvk_conv3x3_wgrad_wino(x.data_ptr(), dy.data_ptr(), dw.ptr(), N, H, W, Cin, Cin, Cout, ld_dy, ws.ptr(), nbytes, _s())
    assert wgrad(Cout, 4 * n - 1) == EWORKSPACE and wname + ":" in _err()
    assert wgrad(Cout - 4, 4 * n) == EINVAL and wname + ":" in _err()
    for bad in (32, 96, 60):
        assert gemm(x.data_ptr(), U.ptr(), Mo.ptr(), N, H, W, bad, Cout, Cout, _s()) == EINVAL and gname + ":" in _err()
    if fam == 4:
        for ks in (0, 4, -1):
            assert lib.cvk_wino4_output(Mo.ptr(), None, y.ptr(), None, N, H, W, Cout, Cout, ks, _s()) == EINVAL and "cvk_wino4_output:" in _err()
    torch.cuda.synchronize()
    for b in (Mo, y, dw, ws):
        assert bool(torch.isnan(b.raw[:b.n]).all())
        b.check_guard("rejected call")
