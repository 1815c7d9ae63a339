"""Raw C-ABI parity of the direct fp32 conv kernels of csrc/conv3x3.hip, arm by arm, against the fp64 operator they replace,
nn.Conv2d(cin, cout, 3, padding=1): cvk_conv3x3_fwd (k_conv3x3_igemm: forward with the BatchNorm statistics partials, and the data-grad through
cvk_pack_weight_dgrad), cvk_conv3x3_wgrad (k_conv3x3_wgrad + k_wgrad_reduce, k_wgrad_smallco), the two weight packs against host
permutations, and the host-side argument contract.

tests/direct_conv_ref.py holds the packs, the case tables with the arm each case is there for (tests/test_direct_conv_ref_cpu.py asserts that
they cover every instantiation and edge) and the tolerances: bound(kind, Cin, which) is 3 x (weight-grad 6 x) the rounding error of a numpy
fp32 restatement of the kernels' accumulation chains against fp64, for the whole tensor (which = 0) and for the worst image row of y / output
channel of dW (which = 1).  Every output and workspace buffer is NaN-filled and followed by a guard band that must stay untouched.
Run with -s for the used fraction of every bound (profiles/direct_conv_margins.txt)."""
import functools
import math

import pytest
import torch

from tests import direct_conv_ref as R

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
SENTINEL = -7.0
EINVAL, EWORKSPACE = -1, -2
X_PAD_VALUE = 1.0e30        # what the pad channels of x hold in the weight-grad cases with Cin < Cin_pad: finite in every slab, absent from dW


def _lib():
    from pytorch_camvid_amd import _lib
    return _lib.load(), _lib.check


def _s():
    return torch.cuda.current_stream().cuda_stream


def _id(c):
    return "-".join(map(str, c))


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
    print(f"[direct] {tag}: {value:.3e} = {value / bound:.3f} of its bound {bound:.3e}")
    return value


def _rel(got, ref):
    return ((got - ref).norm() / ref.norm()).item()


def _worst_row(got, ref, rows):
    e = (got - ref).reshape(rows, -1).norm(dim=1)
    return (e / ref.reshape(rows, -1).norm(dim=1)).max().item()


def _check_y(tag, kind, Ck, got, ref):
    """got / ref [rows][...] double on one device: whole-tensor and worst-row relative L2 against the derived bounds."""
    rows = ref.shape[0]
    b0, b1 = R.bound(kind, Ck, 0), R.bound(kind, Ck, 1)
    whole = _used(f"{tag} whole", _rel(got, ref), b0)
    row = _used(f"{tag} worst row", _worst_row(got, ref, rows), b1)
    assert whole < b0, (tag, whole, b0)
    assert row < b1, (tag, row, b1)


def _fwd(xd, wd, bias, N, H, W, Cin, Cout, ldy, stats):
    """cvk_conv3x3_fwd on device tensors.  Returns y [N][H][W][ldy] and the statistics partials [2][P][Cout] (or None); asserts the guard
    bands, that every element of both was written, and that the pad columns of y read 0."""
    lib, check = _lib()
    y = Buf(N * H * W * ldy)
    P = R.cdiv(N * H * W, R.STAT_ROWS)
    st = Buf(2 * P * Cout) if stats else None
    check(lib.cvk_conv3x3_fwd(xd.data_ptr(), wd.data_ptr(), None if bias is None else bias.data_ptr(), y.ptr(), st.ptr() if stats else None,
                              N, H, W, Cin, Cout, ldy, _s()), "cvk_conv3x3_fwd")
    torch.cuda.synchronize()
    y.check_guard("y")
    yv = y.t.view(N, H, W, ldy)
    assert bool(torch.isfinite(yv).all()), "an element of y was never written"
    if ldy > Cout:
        assert bool((yv[..., Cout:] == 0).all()), "columns [Cout, ldy) of y must read 0"
    if stats:
        st.check_guard("stats")
        assert bool(torch.isfinite(st.t).all()), "a statistics partial was never written"
    return yv, (st.t.view(2, P, Cout) if stats else None)


def _granules(t, P):
    """[M][C] -> [P][64][C], the last granule zero-padded."""
    pad = P * R.STAT_ROWS - t.shape[0]
    return torch.cat([t, torch.zeros(pad, t.shape[1], dtype=t.dtype, device=t.device)]).view(P, R.STAT_ROWS, t.shape[1])


def _check_stats(tag, Ck, st, ref, own):
    """st [2][P][C] from the kernel; ref [M][C] the fp64 y; own [M][C] the y the kernel wrote, in double (all on one device).  The last
    granule holds cnt = M - 64 (P - 1) rows; every check below uses that count, so a kernel that took 64 there fails 2.
    1. Chan's combination against the mean and variance of ref, with the bounds of tests/test_gpu_w6.py.
    2. Against the kernel's own y, element by element: what is left is the epilogue's fp32 arithmetic alone.  A wave owns the 64 rows of a
       granule; a lane adds its 32 values of one column one after the other (31 roundings, the first addition is exact) and one cross-half
       shuffle-add follows: 32 roundings of at most u sum|y| each, |dsum| <= 33 u sum|y| with one u of slack.
       M2: mean' = sum' / cnt (one more rounding, u |sum|), so delta = mean' - mean has |delta| <= 34 u sum|y| / cnt =: dmax, and the exact sum
       of (y - mean')^2 is M2 + cnt delta^2.  Each term is formed with a rounded difference and a rounded square ((1 + u)^3), the terms are
       added like the sum (32 roundings): together below 40 u.  So |m2 - M2| <= 40 u (M2 + cnt dmax^2) + cnt dmax^2.
    3. The per-granule sums against the fp64 granule sums of ref: sum_{p,c} (dsum)^2 <= 64 sum (dy)^2 by Cauchy-Schwarz over the 64 pixels
       of a granule, so |dsum|_2 <= 8 bound_y |y|_2, plus the accumulation term of 2."""
    M, C = ref.shape
    P = st.shape[1]
    assert P == R.cdiv(M, R.STAT_ROWS)
    cnt = torch.full((P,), float(R.STAT_ROWS), dtype=torch.float64, device=ref.device)
    cnt[-1] = M - (P - 1) * R.STAT_ROWS
    sums, m2 = st[0].double(), st[1].double()
    assert bool((m2 >= 0).all())
    g = _granules(own, P)
    absum, exact = g.abs().sum(1), g.sum(1)
    cap = 33 * U24 * (1 + 2.0 ** -16) * absum
    err = (sums - exact).abs()
    assert bool((err <= cap).all()), (tag, (err - cap).max().item())
    print(f"[direct] {tag} granule sums of the kernel's own y: largest error = {(err / cap.clamp_min(1e-300)).max().item():.3f} of its bound")
    mean = exact / cnt[:, None]
    live = (torch.arange(R.STAT_ROWS, device=ref.device)[None, :] < cnt[:, None])[:, :, None]           # rows of the granule inside the tensor
    M2 = (((g - mean[:, None, :]) ** 2) * live).sum(1)
    drift = cnt[:, None] * (34 * U24 * absum / cnt[:, None]) ** 2
    cap = 40 * U24 * (M2 + drift) + drift
    err = (m2 - M2).abs()
    assert bool((err <= cap).all()), (tag, (err - cap).max().item())
    print(f"[direct] {tag} granule M2 of the kernel's own y: largest error = {(err / cap.clamp_min(1e-300)).max().item():.3f} of its bound")
    bound = 8 * R.bound("fwd", Ck, 0) * ref.norm().item() + 33 * U24 * absum.norm().item()
    e = _used(f"{tag} granule sums", (sums - _granules(ref, P).sum(1)).norm().item(), bound)
    assert e < bound, (tag, e, bound)
    cmean, cvar = R.chan_combine(sums, m2, cnt)
    rmean, rvar = ref.mean(0), ref.var(0, unbiased=False)
    assert (cmean - rmean).abs().max().item() < 1e-5 * max(1.0, rmean.abs().max().item()), tag
    assert bool(((cvar - rvar).abs() <= 1e-4 * rvar + 1e-6 * (ref ** 2).mean(0)).all()), tag


# ---------------------------------------------------------------------------------------------------------------------------- packs
@pytest.mark.parametrize("Cout,Cin,Cin_pad", [(64, 3, 4), (12, 12, 12), (40, 160, 160), (160, 40, 44), (7, 5, 36)], ids=lambda v: str(v))
def test_pack_weight_fwd_is_the_host_permutation(Cout, Cin, Cin_pad):
    lib, check = _lib()
    g = torch.Generator().manual_seed(Cout * 1000 + Cin)
    w = torch.randn(Cout, 3, 3, Cin, generator=g)
    dst = Buf(Cout * 9 * Cin_pad)
    check(lib.cvk_pack_weight_fwd(w.cuda().data_ptr(), dst.ptr(), Cout, Cin, Cin_pad, _s()), "cvk_pack_weight_fwd")
    torch.cuda.synchronize()
    dst.check_guard("packed weights")
    assert torch.equal(dst.t.cpu().view(Cout, 9, Cin_pad), R.pack_fwd_ref(w, Cin_pad))


@pytest.mark.parametrize("Cout,Cin,Cin_pad,Cout_pad", [(64, 3, 4, 64), (12, 64, 64, 12), (40, 96, 96, 40), (160, 12, 12, 160), (38, 3, 8, 44),
                                                        (5, 7, 40, 36)], ids=lambda v: str(v))
def test_pack_weight_dgrad_is_the_host_permutation(Cout, Cin, Cin_pad, Cout_pad):
    lib, check = _lib()
    g = torch.Generator().manual_seed(Cout * 1000 + Cin + 1)
    w = torch.randn(Cout, 3, 3, Cin, generator=g)
    dst = Buf(Cin_pad * 9 * Cout_pad)
    check(lib.cvk_pack_weight_dgrad(w.cuda().data_ptr(), dst.ptr(), Cout, Cin, Cin_pad, Cout_pad, _s()), "cvk_pack_weight_dgrad")
    torch.cuda.synchronize()
    dst.check_guard("packed weights")
    assert torch.equal(dst.t.cpu().view(Cin_pad, 9, Cout_pad), R.pack_dgrad_ref(w, Cin_pad, Cout_pad))


# -------------------------------------------------------------------------------------------------------------------------- forward
@functools.lru_cache(maxsize=None)
def _fwd_data(case):
    """Seeded on the CPU: post-ReLU activations, He-scaled filter, bias, and the fp64 reference (with the bias)."""
    N, H, W, Cin, Cout = case[:5]
    g = torch.Generator().manual_seed(1000 * N + 10 * H + W + Cin + 3 * Cout)
    x = torch.relu(torch.randn(N, H, W, Cin, generator=g))
    w = torch.randn(Cout, 3, 3, Cin, generator=g) * math.sqrt(2.0 / (9 * Cin))
    b = torch.randn(Cout, generator=g)
    return x, w, b, R.conv_fwd_ref(x, w, b)


@pytest.mark.parametrize("case", list(R.FWD_CASES), ids=_id)
def test_forward_and_statistics_vs_fp64(case):
    N, H, W, Cin, Cout = case[:5]
    ldy = case[5] if len(case) > 5 else Cout
    x, w, b, ref = _fwd_data(case)
    tag = f"fwd {case}"
    print(f"[direct] {tag}: arms {R.arm_of('fwd', case, False)} and {R.arm_of('fwd', case, True)}")
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    refd = ref.cuda().reshape(N * H, W, Cout)

    def run(bias, stats, xs=xd):
        return _fwd(xs, wd, bias, xs.shape[0], H, W, Cin, Cout, ldy, stats)
    # stats and bias, against fp64
    y, st = run(bd, True)
    own = y[..., :Cout].double()
    _check_y(tag, "fwd", Cin, own.reshape(N * H, W, Cout), refd)
    _check_stats(tag, Cin, st, refd.reshape(-1, Cout), own.reshape(-1, Cout))
    # a second launch, and stats = NULL: the same bits
    y2, st2 = run(bd, True)
    assert torch.equal(y, y2) and torch.equal(st, st2), "two launches differ"
    y3, _ = run(bd, False)
    assert torch.equal(y, y3), "y depends on whether the statistics are taken"
    # bias = NULL is a zero bias, with and without statistics
    yn, stn = run(None, True)
    yz, stz = run(torch.zeros_like(bd), True)
    assert torch.equal(yn, yz) and torch.equal(stn, stz), "bias = NULL differs from a zero bias"
    yn2, _ = run(None, False)
    assert torch.equal(yn, yn2)
    nob = refd - bd.double()
    ownn = yn[..., :Cout].double()
    _check_y(tag + " bias=NULL", "fwd", Cin, ownn.reshape(N * H, W, Cout), nob)
    _check_stats(tag + " bias=NULL", Cin, stn, nob.reshape(-1, Cout), ownn.reshape(-1, Cout))
    # a sub-batch: every output is its own K-ordered chain, so rows a:b of the whole-batch y come back bit for bit whatever tile they fall in
    if N > 1:
        a, e = 1, (N if N == 2 else N - 1)
        for stats in (False, True):
            ys, _ = run(bd, stats, xd[a:e])
            assert torch.equal(ys, y[a:e]), f"sub-batch [{a}:{e}) differs from the whole batch (stats {stats})"


# ------------------------------------------------------------------------------------------------------------------------ data-grad
@functools.lru_cache(maxsize=None)
def _dgrad_data(case):
    N, H, W, Cin, Cout = case
    g = torch.Generator().manual_seed(7 + 1000 * N + 10 * H + W + Cin + 3 * Cout)
    w = torch.randn(Cout, 3, 3, Cin, generator=g) * math.sqrt(2.0 / (9 * Cin))
    dy = torch.full((N, H, W, R.pad4(Cout)), 7.0)          # pad columns: finite, cancelled by the zero rows of the packed filter
    dy[..., :Cout] = torch.randn(N, H, W, Cout, generator=g)
    return w, dy, R.conv_dgrad_ref(dy[..., :Cout], w)


@pytest.mark.parametrize("case", R.DGRAD_CASES, ids=_id)
def test_data_grad_vs_fp64(case):
    """The layer's data-grad as the engine runs it: cvk_pack_weight_dgrad to the two pitches, then cvk_conv3x3_fwd on dy without bias and
    statistics, writing dx at the source pitch."""
    lib, check = _lib()
    N, H, W, Cin, Cout = case
    ldx, ldd = R.pad4(Cin), R.pad4(Cout)
    w, dy, ref = _dgrad_data(case)
    tag = f"dgrad {case}"
    print(f"[direct] {tag}: arm {R.arm_of('fwd', (N, H, W, ldd, ldx))}")
    packed = Buf(ldx * 9 * ldd)
    check(lib.cvk_pack_weight_dgrad(w.cuda().data_ptr(), packed.ptr(), Cout, Cin, ldx, ldd, _s()), "cvk_pack_weight_dgrad")
    torch.cuda.synchronize()
    packed.check_guard("packed weights")
    assert torch.equal(packed.t.cpu().view(ldx, 9, ldd), R.pack_dgrad_ref(w, ldx, ldd))
    dx, _ = _fwd(dy.cuda(), packed.t, None, N, H, W, ldd, ldx, ldx, False)
    if ldx > Cin:
        assert bool((dx[..., Cin:] == 0).all()), "pad columns of dx must read 0"
    _check_y(tag, "dgrad", ldd, dx[..., :Cin].double().reshape(N * H, W, Cin), ref.cuda().reshape(N * H, W, Cin))


# ---------------------------------------------------------------------------------------------------------------------- weight-grad
@functools.lru_cache(maxsize=None)
def _wgrad_data(case):
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    g = torch.Generator().manual_seed(11 + 1000 * N + 10 * H + W + Cin + 3 * Cout)
    x = torch.zeros(N, H, W, Cin_pad)
    x[..., :Cin] = torch.relu(torch.randn(N, H, W, Cin, generator=g))
    dy = torch.zeros(N, H, W, ld_dy)                            # columns [Cout, ld_dy) are zero by the ABI's contract
    dy[..., :Cout] = torch.randn(N, H, W, Cout, generator=g)
    return x, dy, R.conv_wgrad_ref(x[..., :Cin], dy[..., :Cout])


def _wgrad_call(xd, dyd, case):
    """One cvk_conv3x3_wgrad into fresh buffers; the workspace is as large as the library's query says, and the query is the restated plan's."""
    lib, check = _lib()
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    nbytes = lib.cvk_conv3x3_wgrad_workspace_bytes(N, H, W, Cin_pad, Cout)
    assert nbytes == R.wgrad_workspace_bytes(N, H, W, Cin_pad, Cout), (nbytes, R.arm_of("wgrad", case))
    ws, dw = Buf(nbytes // 4), Buf(Cout * 9 * Cin)
    check(lib.cvk_conv3x3_wgrad(xd.data_ptr(), dyd.data_ptr(), dw.ptr(), N, H, W, Cin, Cin_pad, Cout, ld_dy, ws.ptr(), nbytes, _s()),
          "cvk_conv3x3_wgrad")
    torch.cuda.synchronize()
    dw.check_guard("dW")
    ws.check_guard("workspace")
    assert bool(torch.isfinite(dw.t).all()), "an element of dW was never written"          # exactly Cout * 9 * Cin: the guard follows
    tile, (splits, _, _) = R.arm_of("wgrad", case)
    if tile != "smallco":
        assert bool(torch.isfinite(ws.t[:splits * Cout * 9 * Cin_pad]).all()), "an element of a slab was never written"
    return dw.t.view(Cout, 3, 3, Cin)


@pytest.mark.parametrize("case", list(R.WGRAD_CASES), ids=_id)
def test_weight_grad_vs_fp64(case):
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    x, dy, ref = _wgrad_data(case)
    tag = f"wgrad {case}"
    print(f"[direct] {tag}: arm {R.arm_of('wgrad', case)}")
    xd, dyd = x.cuda(), dy.cuda()
    if Cin < Cin_pad:
        xd[..., Cin:] = X_PAD_VALUE
    outs = [_wgrad_call(xd, dyd, case) for _ in range(2)]
    assert torch.equal(outs[0], outs[1]), "two launches differ"
    if Cin < Cin_pad:
        assert torch.equal(outs[0], _wgrad_call(x.cuda(), dyd, case)), "the pad channels of x reached dW"
    _check_y(tag, "wgrad", Cin, outs[0].double(), ref.cuda())          # rows of dW: output channels


# ---------------------------------------------------------------------------------------------------------------- argument contract
def _err():
    lib, _ = _lib()
    return lib.cvk_last_error_string().decode()


def test_host_side_contract():
    """Every rejection returns the documented code before any launch: the NaN-filled outputs stay NaN, and cvk_last_error_string names the
    entry point."""
    lib, _ = _lib()
    N, H, W, Cin, Cout = 1, 4, 8, 64, 64
    x, dy = torch.zeros(N * H * W * Cin + 4, device="cuda"), torch.zeros(N * H * W * Cout + 4, device="cuda")
    w = torch.zeros(Cout * 9 * Cin + 4, device="cuda")
    y, dw, pk = Buf(N * H * W * Cout), Buf(Cout * 9 * Cin), Buf(Cout * 9 * Cin)
    nbytes = lib.cvk_conv3x3_wgrad_workspace_bytes(N, H, W, Cin, Cout)
    ws = Buf(nbytes // 4)
    xp, dyp, wp = x.data_ptr(), dy.data_ptr(), w.data_ptr()
    assert xp % 16 == 0 and dyp % 16 == 0 and wp % 16 == 0 and ws.ptr() % 16 == 0

    def fwd(xq=xp, wq=wp, yq=y.ptr(), cin=Cin, cout=Cout, ldy=Cout):
        return lib.cvk_conv3x3_fwd(xq, wq, None, yq, None, N, H, W, cin, cout, ldy, _s())

    def wgrad(xq=xp, dyq=dyp, dwq=dw.ptr(), cin=Cin, cin_pad=Cin, ld_dy=Cout, wsq=ws.ptr(), nb=nbytes):
        return lib.cvk_conv3x3_wgrad(xq, dyq, dwq, N, H, W, cin, cin_pad, Cout, ld_dy, wsq, nb, _s())
    for kw in (dict(cin=6), dict(cin=62), dict(ldy=Cout - 4), dict(xq=xp + 4), dict(wq=wp + 8), dict(xq=None), dict(wq=None), dict(yq=None),
               dict(cin=0), dict(cout=0, ldy=0)):
        assert fwd(**kw) == EINVAL and "cvk_conv3x3_fwd:" in _err(), kw
    for kw in (dict(cin_pad=Cin - 4), dict(cin_pad=Cin + 2), dict(ld_dy=Cout + 2), dict(ld_dy=Cout - 4), dict(xq=xp + 4), dict(dyq=dyp + 8),
               dict(wsq=ws.ptr() + 4), dict(xq=None), dict(dyq=None), dict(dwq=None), dict(wsq=None), dict(cin=0)):
        assert wgrad(**kw) == EINVAL and "cvk_conv3x3_wgrad:" in _err(), kw
    assert wgrad(nb=nbytes - 1) == EWORKSPACE and "cvk_conv3x3_wgrad:" in _err()
    # the head's arm has a workspace floor of its own (512 slabs)
    nsmall = lib.cvk_conv3x3_wgrad_workspace_bytes(N, H, W, 64, 12)
    assert nsmall == R.wgrad_workspace_bytes(N, H, W, 64, 12) == 512 * 12 * 576 * 4
    wsmall = Buf(nsmall // 4)
    assert lib.cvk_conv3x3_wgrad(xp, dyp, dw.ptr(), N, H, W, 64, 64, 12, 12, wsmall.ptr(), nsmall - 1, _s()) == EWORKSPACE
    assert "cvk_conv3x3_wgrad:" in _err()
    assert lib.cvk_conv3x3_wgrad_workspace_bytes(0, H, W, Cin, Cout) == 0
    for args in ((None, pk.ptr(), Cout, Cin, Cin), (wp, None, Cout, Cin, Cin), (wp, pk.ptr(), Cout, Cin, Cin - 1), (wp, pk.ptr(), 0, Cin, Cin)):
        assert lib.cvk_pack_weight_fwd(*args, _s()) == EINVAL and "cvk_pack_weight_fwd:" in _err(), args
    for args in ((None, pk.ptr(), Cout, Cin, Cin, Cout), (wp, None, Cout, Cin, Cin, Cout), (wp, pk.ptr(), Cout, Cin, Cin - 1, Cout),
                 (wp, pk.ptr(), Cout, Cin, Cin, Cout - 1)):
        assert lib.cvk_pack_weight_dgrad(*args, _s()) == EINVAL and "cvk_pack_weight_dgrad:" in _err(), args
    torch.cuda.synchronize()
    for b in (y, dw, pk, ws, wsmall):
        assert bool(torch.isnan(b.raw[:b.n]).all())
        b.check_guard("rejected call")
