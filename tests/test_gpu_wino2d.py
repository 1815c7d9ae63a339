"""Raw C-ABI parity of the 2-D Winograd fp32 kernels of csrc/wino2d.hip, arm by arm and for both tiles (F(4x4,3x3) `cvk_w2d_*`, F(6x6,3x3)
`cvk_w6_*`), against the fp64 operator they replace, nn.Conv2d(cin, cout, 3, padding=1): the planners against their integer restatement, every
single pass against its fp64 matrix, the forward pipeline with the BatchNorm statistics partials, the data-grad, the weight-grad, the
bitwise identities between the fused calls and their passes, and the host-side argument contract.

tests/wino2d_ref.py holds the references, the case tables with the arm each case is there for (tests/test_wino2d_ref_cpu.py asserts that
they cover every arm) and the tolerances: bound(kind, mt, K, which) is 3 x (weight-grad 6 x) the rounding error of a numpy fp32 restatement of
the kernels' chains against fp64, for the whole tensor (which = 0) and for the worst image row of y / output channel of dW (which = 1).
The fp64 references of the pipelines are nine matrix products in double on the device (conv_fwd_mm, checked against torch.nn.functional on
the CPU).  Every output and workspace buffer is NaN-filled and followed by a guard band that must stay untouched.  Run with -s for the used
fraction of every bound (profiles/wino2d_margins.txt).

The library has the fused calls cvk_conv3x3_w2d / cvk_conv3x3_wgrad_w2d for F(4x4) only; F(6x6) runs pass by pass everywhere."""
import functools
import math

import pytest
import torch

from tests import wino2d_ref as R

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
SLOP = 1.001                # second-order terms of the (1 + u)^k products
SENTINEL = -7.0
PAD_VALUE = 5.0             # what the pad columns of y and dy hold
X_PAD_VALUE = 1.0e30        # what the pad channels of x hold in the weight-grad cases with Cin < Cin_pad
EINVAL = -1


def _lib():
    from pytorch_camvid_amd import _lib
    return _lib.load(), _lib.check


def _s():
    return torch.cuda.current_stream().cuda_stream


def _id(c):
    return "-".join(map(str, c))


def fam(mt):
    lib, _ = _lib()
    pre = "cvk_w2d_" if mt == 4 else "cvk_w6_"
    return lambda name: getattr(lib, pre + name)


def _name(mt, name):
    return ("cvk_w2d_" if mt == 4 else "cvk_w6_") + name


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
    print(f"[wino2d] {tag}: {value:.3e} = {value / bound:.3f} of its bound {bound:.3e}")
    return value


def _used_elem(tag, err, cap):
    """Element-wise |err| <= cap; prints the largest used fraction."""
    frac = (err / cap.clamp_min(1e-300)).max().item()
    print(f"[wino2d] {tag}: largest element error = {frac:.3f} of its bound")
    assert bool((err <= cap).all()), (tag, frac)


def _rel(got, ref):
    return ((got - ref).norm() / ref.norm()).item()


def _worst_row(got, ref, rows):
    e = (got - ref).reshape(rows, -1).norm(dim=1)
    return (e / ref.reshape(rows, -1).norm(dim=1)).max().item()


def _check_y(tag, kind, mt, K, got, ref):
    """got / ref [rows][...] double on the device: whole-tensor and worst-row relative L2 against the derived bounds."""
    rows = ref.shape[0]
    b0, b1 = R.bound(kind, mt, K, 0), R.bound(kind, mt, K, 1)
    whole = _used(f"{tag} whole", _rel(got, ref), b0)
    row = _used(f"{tag} worst row", _worst_row(got, ref, rows), b1)
    assert whole < b0, (tag, whole, b0)
    assert row < b1, (tag, row, b1)


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_tensors():
    yield
    for fn in (_fwd_data, _dgrad_data, _wgrad_data):
        fn.cache_clear()


# ---------------------------------------------------------------------------------------------------------------------- the passes
def _filter(mt, wd, Cout, Cin, dgrad=False):
    """cvk_w*_weight_transform[_dgrad] of w [Cout][3][3][Cin] on the device: U [NX][Cout][Cin] (dgrad: [NX][Cin][Cout])."""
    _, check = _lib()
    U = Buf(R.nx_of(mt) * Cout * Cin)
    name = "weight_transform_dgrad" if dgrad else "weight_transform"
    check(fam(mt)(name)(wd.data_ptr(), U.ptr(), Cout, Cin, _s()), _name(mt, name))
    torch.cuda.synchronize()
    U.check_guard("U")
    assert bool(torch.isfinite(U.t).all()), "an element of U was never written"
    return U


def _input(mt, xd, N, H, W, C):
    """cvk_w*_input_transform: V [NX][Tpad][C] + 128 floats of slack.  Rows [T, Tpad) read 0, the slack stays NaN."""
    _, check = _lib()
    nx, T = R.nx_of(mt), R.tiles(mt, N, H, W)
    Tp = R.tpad(T)
    V = Buf(nx * Tp * C + R.SLACK)
    check(fam(mt)("input_transform")(xd.data_ptr(), V.ptr(), N, H, W, C, _s()), _name(mt, "input_transform"))
    torch.cuda.synchronize()
    _check_planes(V, nx, T, Tp, C, "V")
    return V


def _check_planes(B, nx, T, Tp, C, what):
    B.check_guard(what)
    planes = B.t[:nx * Tp * C].view(nx, Tp, C)
    assert bool(torch.isfinite(planes[:, :T]).all()), f"an element of {what} was never written"
    assert bool((planes[:, T:] == 0).all()), f"rows [T, Tpad) of {what} must read 0"
    assert bool(torch.isnan(B.t[nx * Tp * C:]).all()), f"the slack behind {what} was written"


def _dy(mt, dyd, ld, N, H, W, C):
    """cvk_w*_dy_transform: E [NX][Tpad][C] + slack."""
    _, check = _lib()
    nx, T = R.nx_of(mt), R.tiles(mt, N, H, W)
    Tp = R.tpad(T)
    E = Buf(nx * Tp * C + R.SLACK)
    check(fam(mt)("dy_transform")(dyd.data_ptr(), ld, E.ptr(), N, H, W, C, _s()), _name(mt, "dy_transform"))
    torch.cuda.synchronize()
    _check_planes(E, nx, T, Tp, C, "E")
    return E


def _gemm(mt, V, U, T, Cin, Cout):
    """cvk_w*_gemm into NaN-filled planes Mo [f][NX][T][Cout]: part 0 is written everywhere, parts 1..f-1 exactly on the GEMM tiles behind
    split_start (tile id = xi * tilesM * tilesN + row tile * tilesN + column tile), nowhere else."""
    _, check = _lib()
    nx = R.nx_of(mt)
    p = R.plan_fwd(mt, T, Cin, Cout)
    Mo = Buf(p["f"] * nx * T * Cout)
    check(fam(mt)("gemm")(V.ptr(), U.ptr(), Mo.ptr(), T, Cin, Cout, _s()), _name(mt, "gemm"))
    torch.cuda.synchronize()
    Mo.check_guard("Mo")
    parts = Mo.t.view(p["f"], nx, T, Cout)
    assert bool(torch.isfinite(parts[0]).all()), "an element of the product planes was never written"
    if p["f"] > 1:
        dev = parts.device
        ids = (torch.arange(nx, device=dev).view(nx, 1, 1) * (p["tilesM"] * p["tilesN"])
               + (torch.arange(T, device=dev) // R.BM).view(1, T, 1) * p["tilesN"] + (torch.arange(Cout, device=dev) // R.W2_BN).view(1, 1, Cout))
        split = ids >= p["split_start"]
        for k in range(1, p["f"]):
            assert torch.equal(torch.isfinite(parts[k]), split), f"K-range plane {k} is not written exactly on the split tiles"
    return Mo


def _output(mt, Mo, bias, N, H, W, Cin, Cout, ldy, stats, plain=False):
    """cvk_w*_output (plain: cvk_w2d_output_plain) into a NaN-filled y whose pad columns hold PAD_VALUE.  Returns y [N][H][W][ldy],
    the statistics [2][P][Cout] and the counts [P] (or None, None)."""
    lib, check = _lib()
    y = Buf(N * H * W * ldy)
    yv = y.t.view(N, H, W, ldy)
    yv[..., Cout:] = PAD_VALUE
    P = R.plan_out(mt, R.tiles(mt, N, H, W), Cout)["P"]
    st, cnt = (Buf(2 * P * Cout), Buf(P)) if stats else (None, None)
    args = (Mo.ptr(), None if bias is None else bias.data_ptr(), y.ptr(), st.ptr() if stats else None, cnt.ptr() if stats else None, N, H, W)
    if plain:
        check(lib.cvk_w2d_output_plain(mt, *args, Cout, ldy, _s()), "cvk_w2d_output_plain")
    else:
        check(fam(mt)("output")(*args, Cin, Cout, ldy, _s()), _name(mt, "output"))
    torch.cuda.synchronize()
    _check_out(y, st, cnt, Cout, ldy)
    return yv, (st.t.view(2, P, Cout) if stats else None), (cnt.t if stats else None)


def _check_out(y, st, cnt, Cout, ldy):
    y.check_guard("y")
    yv = y.t.view(-1, ldy)
    assert bool(torch.isfinite(yv[:, :Cout]).all()), "an element of y[..., :Cout] was never written"
    assert bool((yv[:, Cout:] == PAD_VALUE).all()), "the columns [Cout, ldy) of y must be left as they were"
    if st is not None:
        st.check_guard("stats")
        cnt.check_guard("counts")
        assert bool(torch.isfinite(st.t).all()) and bool(torch.isfinite(cnt.t).all()), "a statistics partial was never written"


def _check_stats(tag, mt, N, H, W, Cout, st, cnt, own):
    """st [2][P][Cout], cnt [P] from a run WITHOUT bias (y = o bit for bit); own [N][H][W][Cout]: that run's y in double.
    1. Counts are exact per partial: a partial owns TB consecutive tiles, a ragged tile counts its pixels inside the frame.
    2. Sums against the fp64 sums of the kernel's own y.  In k_w2d_output a thread adds the MT^2 pixels of its ceil(TB / pl) tiles one after the
       other and thread 0 of the column adds the pl = 256 / cvn partial sums one after the other: D = ceil(TB / pl) MT^2 + pl roundings
       (wino2d_ref.stat_depth), each at most u times a partial sum of |o|:  |a - sum o| <= D u sum |o|.
    3. M2 is formed as b - a^2 / cnt with b = sum fl(o^2) added the same way: |b - sum o^2| <= (D + 1) u sum o^2.  a^2 / cnt: the error of a
       enters as 2 |sum o| D u sum|o| / cnt <= 2 D u sum o^2 (Cauchy-Schwarz: (sum |o|)^2 <= cnt sum o^2), the square and the quotient round
       once each (2 u a^2 / cnt <= 2 u sum o^2), the difference once more (u M2 <= u sum o^2):
       |m2 - M2| <= (3 D + 4) u sum o^2 - the bound scales with the partial's sum of squares, not with M2 (the form cancels)."""
    T = R.tiles(mt, N, H, W)
    cref = torch.tensor(R.partial_counts(mt, N, H, W), dtype=torch.float64, device=own.device)
    P = cref.numel()
    assert st.shape == (2, P, Cout) and cnt.shape == (P,)
    assert torch.equal(cnt.double(), cref), f"{tag}: pixel counts of the partials"
    pid = R.partial_of_pixel(mt, N, H, W).to(own.device).flatten()
    flat = own.reshape(-1, Cout)
    z = torch.zeros(P, Cout, dtype=torch.float64, device=own.device)
    S, Sabs, Q = z.index_add(0, pid, flat), z.index_add(0, pid, flat.abs()), z.index_add(0, pid, flat * flat)
    D = R.stat_depth(mt, T, Cout)
    _used_elem(f"{tag} partial sums of the kernel's own y (depth {D})", (st[0].double() - S).abs(), D * U24 * SLOP * Sabs)
    M2 = (Q - S * S / cref[:, None]).clamp_min(0)
    assert bool((st[1] >= 0).all())
    _used_elem(f"{tag} partial M2 of the kernel's own y", (st[1].double() - M2).abs(), (3 * D + 4) * U24 * SLOP * Q)


def _check_chan(tag, st, cnt, ref):
    """Chan's combination of the partials against the mean and biased variance of the fp64 y, with the bounds of tests/test_gpu_w6.py."""
    flat = ref.reshape(-1, ref.shape[-1])
    cmean, cvar = R.chan_combine(st[0], st[1], cnt)
    rmean, rvar = flat.mean(0), flat.var(0, unbiased=False)
    assert (cmean - rmean).abs().max().item() < 1e-5 * max(1.0, rmean.abs().max().item()), tag
    assert bool(((cvar - rvar).abs() <= 1e-4 * rvar + 1e-6 * (flat ** 2).mean(0)).all()), tag


# ------------------------------------------------------------------------------------------------------------------------- planners
@pytest.mark.parametrize("mt", R.TILES)
def test_planners_agree_with_the_restatement(mt):
    lib, _ = _lib()
    f = fam(mt)
    ws_fwd = lib.cvk_conv3x3_w2d_workspace_bytes if mt == 4 else lib.cvk_conv3x3_w6_workspace_bytes
    shapes = {(c[:3], c[3], c[4]) for c in R.FWD_CASES} | {(c[:3], c[4], c[3]) for c in R.DGRAD_CASES} | {(c[:3], 32, c[3]) for c in R.OUT_CASES[mt]}
    for (N, H, W), Cin, Cout in sorted(shapes):
        T = R.tiles(mt, N, H, W)
        assert f("tiles")(N, H, W) == T and lib.cvk_w2d_tpad(T) == R.tpad(T)
        assert f("ksplit")(T, Cin, Cout) == R.plan_fwd(mt, T, Cin, Cout)["f"], (N, H, W, Cin, Cout)
        assert f("stat_partials")(N, H, W) == R.plan_out(mt, T, Cout)["P"] == len(R.partial_counts(mt, N, H, W))
        assert ws_fwd(N, H, W, Cin, Cout) == 4 * R.fwd_workspace_floats(mt, N, H, W, Cin, Cout)
    for N, H, W, Cin, Cin_pad, Cout, ld_dy in R.WGRAD_CASES:
        T = R.tiles(mt, N, H, W)
        assert f("tiles")(N, H, W) == T
        assert f("wgrad_ksplit")(T, Cin_pad, Cout) == R.plan_wgrad(mt, T, Cin_pad, Cout)["f"], (N, H, W, Cin_pad, Cout)
        if mt == 4:                 # the weight-grad's workspace query exists for F(4x4) only
            assert lib.cvk_conv3x3_wgrad_w2d_workspace_bytes(N, H, W, Cin_pad, Cout) == 4 * R.wgrad_workspace_floats(4, N, H, W, Cin_pad, Cout)
    for T in (1, 31, 32, 33, 8191, 8192):
        assert lib.cvk_w2d_tpad(T) == R.tpad(T)
    # zero or negative sizes: every query answers 0
    for bad in (0, -1):
        assert f("tiles")(bad, 4, 4) == 0 and f("tiles")(1, bad, 4) == 0 and f("tiles")(1, 4, bad) == 0
        assert f("stat_partials")(bad, 4, 4) == 0 and f("stat_partials")(1, 4, bad) == 0
        assert lib.cvk_w2d_tpad(bad) == 0
        assert f("ksplit")(bad, 64, 64) == 0 and f("ksplit")(8, bad, 64) == 0 and f("ksplit")(8, 64, bad) == 0
        assert f("wgrad_ksplit")(bad, 64, 64) == 0 and f("wgrad_ksplit")(8, bad, 64) == 0 and f("wgrad_ksplit")(8, 64, bad) == 0
        assert ws_fwd(bad, 4, 4, 64, 64) == 0 and ws_fwd(1, 4, 4, bad, 64) == 0 and ws_fwd(1, 4, 4, 64, bad) == 0
        assert lib.cvk_conv3x3_wgrad_w2d_workspace_bytes(bad, 4, 4, 64, 64) == 0 and lib.cvk_conv3x3_wgrad_w2d_workspace_bytes(1, 4, 4, 64, bad) == 0


# -------------------------------------------------------------------------------------------------------------------- single passes
@pytest.mark.parametrize("mt", R.TILES)
@pytest.mark.parametrize("case", R.TRANSFORM_CASES, ids=_id)
def test_input_transform_vs_fp64(mt, case):
    """V = B^T d B element by element: |V - V64| <= k u (|B^T| |d| |B|) with k = 2 BT_DEPTH (6 for w2_bt, 8 for w6_bt: the roundings on the
    longest path of one 1-D pass, rows then columns; the input is fp32 data, so nothing else enters)."""
    N, H, W, C, _ = case
    g = torch.Generator().manual_seed(31 * H + W + C)
    x = torch.randn(N, H, W, C, generator=g).cuda()
    V = _input(mt, x, N, H, W, C)
    nx, T = R.nx_of(mt), R.tiles(mt, N, H, W)
    ref, mag = R.planes_ref(R.BT[mt], R.tile_windows(mt, x))
    got = V.t[:nx * R.tpad(T) * C].view(nx, -1, C)[:, :T].double()
    _used_elem(f"input F({mt}x{mt}) {case}", (got - ref).abs(), 2 * R.BT_DEPTH[mt] * U24 * SLOP * mag)


@pytest.mark.parametrize("mt", R.TILES)
@pytest.mark.parametrize("case", R.TRANSFORM_CASES, ids=_id)
def test_dy_transform_vs_fp64(mt, case):
    """E = A dy A^T element by element with k = 2 A_DEPTH (4 for w2_a, 6 for w6_a), at ld_dy == C and at the case's pitch; the pad columns
    of dy hold a finite value that must not reach E (the two runs agree bit for bit)."""
    N, H, W, C, ld = case
    g = torch.Generator().manual_seed(37 * H + W + C)
    dy = torch.randn(N, H, W, C, generator=g).cuda()
    nx, T = R.nx_of(mt), R.tiles(mt, N, H, W)
    ref, mag = R.planes_ref(R.A[mt], R.tile_windows(mt, dy, halo=False))
    E = _dy(mt, dy, C, N, H, W, C)
    _used_elem(f"dy F({mt}x{mt}) {case}", (E.t[:nx * R.tpad(T) * C].view(nx, -1, C)[:, :T].double() - ref).abs(), 2 * R.A_DEPTH[mt] * U24 * SLOP * mag)
    if ld > C:
        wide = torch.full((N, H, W, ld), PAD_VALUE, device="cuda")
        wide[..., :C] = dy
        E2 = _dy(mt, wide, ld, N, H, W, C)
        assert torch.equal(E2.t[:nx * R.tpad(T) * C], E.t[:nx * R.tpad(T) * C]), "E depends on the pitch of dy"


@pytest.mark.parametrize("mt", R.TILES)
@pytest.mark.parametrize("Cout,Cin", R.FILTER_CASES)
def test_weight_transforms_vs_fp64(mt, Cout, Cin):
    """U = G g G^T, forward and data-grad (the filter rotated by 180 degrees, channels exchanged), with k = 2 G_DEPTH = 8: per 1-D pass a
    rounded constant, two additions and the product."""
    g = torch.Generator().manual_seed(Cout * 1000 + Cin)
    w = torch.randn(Cout, 3, 3, Cin, generator=g).cuda()
    k = 2 * R.G_DEPTH[mt] * U24 * SLOP
    ref, mag = R.filter_planes_ref(mt, w)
    U = _filter(mt, w, Cout, Cin)
    _used_elem(f"filter F({mt}x{mt}) {Cout}x{Cin}", (U.t.view(-1, Cout, Cin).double() - ref).abs(), k * mag)
    ref, mag = R.filter_planes_ref(mt, R.dgrad_filter(w))
    U = _filter(mt, w, Cout, Cin, dgrad=True)
    _used_elem(f"dgrad filter F({mt}x{mt}) {Cout}x{Cin}", (U.t.view(-1, Cin, Cout).double() - ref).abs(), k * mag)


@pytest.mark.parametrize("mt,case", [(mt, c) for mt in R.TILES for c in R.OUT_CASES[mt]], ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_output_pass_vs_fp64(mt, case):
    """The output pass alone on random product planes (f = 1: depth 32), through cvk_w*_output and cvk_w2d_output_plain (the same bits):
    |y - (A^T m A + bias)| <= k u (|A^T| |m| |A| + |bias|) with k = OUT_DEPTH (8 / 11: A^T along the rows, the running sum over the columns,
    the bias).  The first case of each tile has T = 8281 >= 8192: 16 tiles per block, a thread of the statistics walks several tiles."""
    N, H, W, Cout = case
    nx, T = R.nx_of(mt), R.tiles(mt, N, H, W)
    tag = f"out F({mt}x{mt}) {case}"
    print(f"[wino2d] {tag}: arm {R.arm_of('out', mt, case)}")
    g = torch.Generator(device="cuda").manual_seed(T + Cout)
    Mo = Buf(nx * T * Cout)
    Mo.t.copy_(torch.randn(nx * T * Cout, generator=g, device="cuda"))
    bias = torch.randn(Cout, generator=g, device="cuda")
    ref, mag = R.output_ref(mt, Mo.t.view(nx, T, Cout), N, H, W)
    y, _, _ = _output(mt, Mo, bias, N, H, W, 32, Cout, Cout, False)
    _used_elem(tag, (y.double() - (ref + bias.double())).abs(), R.OUT_DEPTH[mt] * U24 * SLOP * (mag + bias.double().abs()))
    yp, stp, cp = _output(mt, Mo, bias, N, H, W, 32, Cout, Cout, True, plain=True)
    ys, sts, cs = _output(mt, Mo, bias, N, H, W, 32, Cout, Cout, True)
    assert torch.equal(y, yp) and torch.equal(y, ys), "y depends on the entry point or on whether the statistics are taken"
    assert torch.equal(stp, sts) and torch.equal(cp, cs), "cvk_w2d_output_plain differs from the tile's output pass on f = 1 planes"
    yn, stn, cn = _output(mt, Mo, None, N, H, W, 32, Cout, Cout, True)
    _check_stats(tag, mt, N, H, W, Cout, stn, cn, yn.double())
    Mo.check_guard("Mo")


# -------------------------------------------------------------------------------------------------------------------------- forward
@functools.lru_cache(maxsize=None)
def _fwd_data(case):
    """Seeded on the CPU: post-ReLU activations, He-scaled filter, bias; on the device with the fp64 reference (with the bias)."""
    N, H, W, Cin, Cout = case[:5]
    g = torch.Generator().manual_seed(1000 * N + 10 * H + W + Cin + 3 * Cout)
    x = torch.relu(torch.randn(N, H, W, Cin, generator=g)).cuda()
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) * math.sqrt(2.0 / (9 * Cin))).cuda()
    b = torch.randn(Cout, generator=g).cuda()
    return x, w, b, R.conv_fwd_mm(x, w, b)


def _pipeline(mt, x, U, bias, N, H, W, Cin, Cout, ldy, stats):
    V = _input(mt, x, N, H, W, Cin)
    Mo = _gemm(mt, V, U, R.tiles(mt, N, H, W), Cin, Cout)
    out = _output(mt, Mo, bias, N, H, W, Cin, Cout, ldy, stats)
    V.check_guard("V")
    Mo.check_guard("Mo")
    return out, Mo


@pytest.mark.parametrize("mt", R.TILES)
@pytest.mark.parametrize("case", R.FWD_CASES, ids=_id)
def test_forward_and_statistics_vs_fp64(mt, case):
    N, H, W, Cin, Cout = case[:5]
    ldy = case[5] if len(case) > 5 else Cout
    x, w, b, ref = _fwd_data(case)
    tag = f"fwd F({mt}x{mt}) {case}"
    print(f"[wino2d] {tag}: arm {R.arm_of('fwd', mt, case)}")
    U = _filter(mt, w, Cout, Cin)
    (y, st, cnt), Mo = _pipeline(mt, x, U, b, N, H, W, Cin, Cout, ldy, True)
    own = y[..., :Cout].double()
    _check_y(tag, "fwd", mt, Cin, own.reshape(N * H, W, Cout), ref.reshape(N * H, W, Cout))
    _check_chan(tag, st, cnt, ref)
    # a second launch of the whole pipeline, and stats = NULL: the same bits
    (y2, st2, cnt2), _ = _pipeline(mt, x, U, b, N, H, W, Cin, Cout, ldy, True)
    assert torch.equal(y, y2) and torch.equal(st, st2) and torch.equal(cnt, cnt2), "two launches differ"
    y3, _, _ = _output(mt, Mo, b, N, H, W, Cin, Cout, ldy, False)
    assert torch.equal(y, y3), "y depends on whether the statistics are taken"
    # bias = NULL is a zero bias, with and without statistics
    yn, stn, cn = _output(mt, Mo, None, N, H, W, Cin, Cout, ldy, True)
    yz, stz, cz = _output(mt, Mo, torch.zeros_like(b), N, H, W, Cin, Cout, ldy, True)
    assert torch.equal(yn, yz) and torch.equal(stn, stz) and torch.equal(cn, cz), "bias = NULL differs from a zero bias"
    yn2, _, _ = _output(mt, Mo, None, N, H, W, Cin, Cout, ldy, False)
    assert torch.equal(yn, yn2)
    ownn = yn[..., :Cout].double()
    _check_y(tag + " bias=NULL", "fwd", mt, Cin, ownn.reshape(N * H, W, Cout), (ref - b.double()).reshape(N * H, W, Cout))
    # statistics: against the kernel's own y where y = o bit for bit (no bias); with the bias the sums move by cnt * bias (one rounded product,
    # one rounded sum: 2 u (|sum| + cnt |bias|)) and M2, taken about the partial mean of o, keeps its bits
    _check_stats(tag, mt, N, H, W, Cout, stn, cn, ownn)
    shift = cn.double()[:, None] * b.double()[None, :]
    _used_elem(f"{tag} partial sums with bias", (st[0].double() - (stn[0].double() + shift)).abs(), 2 * U24 * SLOP * (stn[0].double().abs() + shift.abs()))
    assert torch.equal(st[1], stn[1]) and torch.equal(cnt, cn), "M2 or the counts depend on the bias"


# ------------------------------------------------------------------------------------------------------------------------ data-grad
@functools.lru_cache(maxsize=None)
def _dgrad_data(case):
    N, H, W, Cin, Cout = case
    g = torch.Generator().manual_seed(7 + 1000 * N + 10 * H + W + Cin + 3 * Cout)
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) * math.sqrt(2.0 / (9 * Cin))).cuda()
    dy = torch.randn(N, H, W, Cout, generator=g).cuda()
    return w, dy, R.conv_dgrad_mm(dy, w)


@pytest.mark.parametrize("mt", R.TILES)
@pytest.mark.parametrize("case", R.DGRAD_CASES, ids=_id)
def test_data_grad_vs_fp64(mt, case):
    """The layer's data-grad as the engine runs it: cvk_w*_weight_transform_dgrad from the forward weights, then the forward passes on dy without
    bias and statistics; the launch reduces over Cout and writes Cin channels."""
    N, H, W, Cin, Cout = case
    w, dy, ref = _dgrad_data(case)
    tag = f"dgrad F({mt}x{mt}) {case}"
    print(f"[wino2d] {tag}: arm {R.arm_of('dgrad', mt, case)}")
    U = _filter(mt, w, Cout, Cin, dgrad=True)
    (dx, _, _), _ = _pipeline(mt, dy, U, None, N, H, W, Cout, Cin, Cin, False)
    _check_y(tag, "dgrad", mt, Cout, dx.double().reshape(N * H, W, Cin), ref.reshape(N * H, W, Cin))
    (dx2, _, _), _ = _pipeline(mt, dy, U, None, N, H, W, Cout, Cin, Cin, False)
    assert torch.equal(dx, dx2), "two launches differ"


# ---------------------------------------------------------------------------------------------------------------------- weight-grad
@functools.lru_cache(maxsize=None)
def _wgrad_data(case):
    """x [N][H][W][Cin_pad] with zero pad channels, dy [N][H][W][ld_dy] whose pad columns hold PAD_VALUE, and the fp64 dW."""
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    g = torch.Generator().manual_seed(11 + 1000 * N + 10 * H + W + Cin + 3 * Cout)
    x = torch.zeros(N, H, W, Cin_pad)
    x[..., :Cin] = torch.relu(torch.randn(N, H, W, Cin, generator=g))
    dy = torch.full((N, H, W, ld_dy), PAD_VALUE)
    dy[..., :Cout] = torch.randn(N, H, W, Cout, generator=g)
    x, dy = x.cuda(), dy.cuda()
    return x, dy, R.conv_wgrad_mm(x[..., :Cin], dy[..., :Cout])


def _wgrad_passes(mt, xd, dyd, case, V=None):
    """The four passes into fresh buffers.  Returns dW [Cout][3][3][Cin], the product planes [f][NX][Cout][Cin_pad] and V."""
    _, check = _lib()
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    nx, T = R.nx_of(mt), R.tiles(mt, N, H, W)
    f = R.plan_wgrad(mt, T, Cin_pad, Cout)["f"]
    if V is None:
        V = _input(mt, xd, N, H, W, Cin_pad)
    E = _dy(mt, dyd, ld_dy, N, H, W, Cout)
    P, dw = Buf(f * nx * Cout * Cin_pad), Buf(Cout * 9 * Cin)
    check(fam(mt)("gemm_tn")(E.ptr(), V.ptr(), P.ptr(), T, Cin_pad, Cout, _s()), _name(mt, "gemm_tn"))
    check(fam(mt)("wgrad_output")(P.ptr(), dw.ptr(), T, Cin, Cin_pad, Cout, _s()), _name(mt, "wgrad_output"))
    torch.cuda.synchronize()
    for b, what in ((V, "V"), (E, "E"), (P, "P"), (dw, "dW")):
        b.check_guard(what)
    assert bool(torch.isfinite(dw.t).all()), "an element of dW was never written"
    return dw.t.view(Cout, 3, 3, Cin), P.t.view(f, nx, Cout, Cin_pad), V


@pytest.mark.parametrize("mt", R.TILES)
@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=_id)
def test_weight_grad_vs_fp64(mt, case):
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    x, dy, ref = _wgrad_data(case)
    tag = f"wgrad F({mt}x{mt}) {case}"
    print(f"[wino2d] {tag}: arm {R.arm_of('wgrad', mt, case)}, chain depth {R.wgrad_depth(mt, case)}")
    dw, P, _ = _wgrad_passes(mt, x, dy, case)
    assert not bool(torch.isnan(P).any()), "an element of the f product planes was never written"
    dw2, P2, _ = _wgrad_passes(mt, x, dy, case)
    assert torch.equal(dw, dw2) and torch.equal(P, P2), "two launches differ"
    if Cin < Cin_pad:
        xp = x.clone()
        xp[..., Cin:] = X_PAD_VALUE
        dw3, P3, _ = _wgrad_passes(mt, xp, dy, case)
        assert torch.equal(dw, dw3), "the pad channels of x reached dW"
        assert torch.equal(P[..., :Cin], P3[..., :Cin])
    _check_y(tag, "wgrad", mt, R.wgrad_depth(mt, case), dw.double(), ref)           # rows of dW: output channels


# --------------------------------------------------------------------------------------------------------------- bitwise identities
FUSED_FWD = [(3, 5, 7, 32, 68), (2, 10, 14, 32, 64, 72), (1, 13, 11, 288, 320), (1, 96, 102, 256, 384)]


@pytest.mark.parametrize("case", FUSED_FWD, ids=_id)
def test_fused_forward_is_the_three_passes(case):
    """cvk_conv3x3_w2d == input transform, GEMM, output pass, bit for bit (y, statistics, counts), in a workspace of exactly the queried size."""
    lib, check = _lib()
    N, H, W, Cin, Cout = case[:5]
    ldy = case[5] if len(case) > 5 else Cout
    x, w, b, _ = _fwd_data(case)
    U = _filter(4, w, Cout, Cin)
    (y, st, cnt), _ = _pipeline(4, x, U, b, N, H, W, Cin, Cout, ldy, True)
    nbytes = lib.cvk_conv3x3_w2d_workspace_bytes(N, H, W, Cin, Cout)
    P = cnt.numel()
    for stats in (True, False):
        ws, yf = Buf(nbytes // 4), Buf(N * H * W * ldy)
        yf.t.view(N, H, W, ldy)[..., Cout:] = PAD_VALUE
        stf, cf = (Buf(2 * P * Cout), Buf(P)) if stats else (None, None)
        check(lib.cvk_conv3x3_w2d(x.data_ptr(), U.ptr(), b.data_ptr(), yf.ptr(), stf.ptr() if stats else None, cf.ptr() if stats else None,
                                  N, H, W, Cin, Cout, ldy, ws.ptr(), nbytes, _s()), "cvk_conv3x3_w2d")
        torch.cuda.synchronize()
        ws.check_guard("workspace")
        _check_out(yf, stf, cf, Cout, ldy)
        assert torch.equal(yf.t.view(N, H, W, ldy), y), "cvk_conv3x3_w2d differs from its three passes"
        if stats:
            assert torch.equal(stf.t.view(2, P, Cout), st) and torch.equal(cf.t, cnt)


FUSED_WGRAD = [(2, 12, 18, 64, 64, 64, 64), (1, 50, 131, 32, 36, 68, 72), (2, 40, 80, 60, 64, 72, 72), (3, 21, 27, 132, 132, 200, 200),
               (1, 180, 180, 32, 32, 64, 64)]


@pytest.mark.parametrize("case", FUSED_WGRAD, ids=_id)
def test_fused_weight_grad_is_the_four_passes(case):
    """cvk_conv3x3_wgrad_w2d with x == the same call with x = NULL and V = cvk_w2d_input_transform(x) at the start of the workspace == the
    four passes, bit for bit, in a workspace of exactly the queried size."""
    lib, check = _lib()
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    x, dy, _ = _wgrad_data(case)
    dw, _, V = _wgrad_passes(4, x, dy, case)
    nbytes = lib.cvk_conv3x3_wgrad_w2d_workspace_bytes(N, H, W, Cin_pad, Cout)
    nv = 36 * R.tpad(R.tiles(4, N, H, W)) * Cin_pad
    for preload in (False, True):
        ws, dwf = Buf(nbytes // 4), Buf(Cout * 9 * Cin)
        if preload:
            ws.t[:nv] = V.t[:nv]
        check(lib.cvk_conv3x3_wgrad_w2d(None if preload else x.data_ptr(), dy.data_ptr(), dwf.ptr(), N, H, W, Cin, Cin_pad, Cout, ld_dy,
                                        ws.ptr(), nbytes, _s()), "cvk_conv3x3_wgrad_w2d")
        torch.cuda.synchronize()
        ws.check_guard("workspace")
        dwf.check_guard("dW")
        assert torch.equal(dwf.t.view(Cout, 3, 3, Cin), dw), f"cvk_conv3x3_wgrad_w2d (x = {'NULL' if preload else 'x'}) differs from its four passes"


@pytest.mark.parametrize("mt", R.TILES)
@pytest.mark.parametrize("case", [(1, 180, 180, 32, 32, 64, 64), (1, 50, 131, 32, 36, 68, 72), (2, 40, 80, 60, 64, 72, 72), (2, 12, 18, 64, 64, 64, 64)],
                         ids=_id)
def test_wgrad_output_f_is_the_planned_output(mt, case):
    """cvk_w2d_wgrad_output_f(tile, ..., f) with the plan's f == cvk_w*_wgrad_output, on random product planes."""
    lib, check = _lib()
    N, H, W, Cin, Cin_pad, Cout, ld_dy = case
    nx, T = R.nx_of(mt), R.tiles(mt, N, H, W)
    f = R.plan_wgrad(mt, T, Cin_pad, Cout)["f"]
    g = torch.Generator(device="cuda").manual_seed(T + Cout + f)
    P = torch.randn(f * nx * Cout * Cin_pad, generator=g, device="cuda")
    a, b = Buf(Cout * 9 * Cin), Buf(Cout * 9 * Cin)
    check(fam(mt)("wgrad_output")(P.data_ptr(), a.ptr(), T, Cin, Cin_pad, Cout, _s()), _name(mt, "wgrad_output"))
    check(lib.cvk_w2d_wgrad_output_f(mt, P.data_ptr(), b.ptr(), Cin, Cin_pad, Cout, f, _s()), "cvk_w2d_wgrad_output_f")
    torch.cuda.synchronize()
    a.check_guard("dW")
    b.check_guard("dW")
    assert bool(torch.isfinite(a.t).all()) and torch.equal(a.t, b.t)
    # and it is G^T (sum of the f planes) G: against fp64 with k = f - 1 additions and two passes of w*_gt (at most 6 roundings each)
    Gt = torch.as_tensor(R.GT[mt], device="cuda")
    planes = P.view(f, R.nt_of(mt), R.nt_of(mt), Cout, Cin_pad)[..., :Cin].double()
    ref = torch.einsum("ra,fabok,sb->orsk", Gt, planes, Gt)
    mag = torch.einsum("ra,fabok,sb->orsk", Gt.abs(), planes.abs(), Gt.abs())
    _used_elem(f"wgrad output F({mt}x{mt}) {case} f={f}", (a.t.view(Cout, 3, 3, Cin).double() - ref).abs(), (f - 1 + 12) * U24 * SLOP * mag)


# ---------------------------------------------------------------------------------------------------------------- argument contract
def _err():
    lib, _ = _lib()
    return lib.cvk_last_error_string().decode()


@pytest.mark.parametrize("mt", R.TILES)
def test_host_side_contract(mt):
    """Every documented rejection returns CVK_EINVAL (a workspace too small for the fused calls included: that is the code they return) before
    any launch: the NaN-filled outputs and workspaces stay NaN, and cvk_last_error_string names the entry point."""
    lib, _ = _lib()
    f = fam(mt)
    N, H, W, Cin, Cout = 1, 4, 8, 32, 64
    nx, T = R.nx_of(mt), R.tiles(mt, N, H, W)
    Tp = R.tpad(T)
    src = torch.zeros(nx * Tp * Cout + 1024, device="cuda")        # stands for every input operand: large enough for each of them
    sp = src.data_ptr()
    assert sp % 16 == 0
    out, out2, out3 = Buf(nx * Tp * Cout + R.SLACK), Buf(nx * Tp * Cout + R.SLACK), Buf(2 * Cout + 16)
    op, op2, op3 = out.ptr(), out2.ptr(), out3.ptr()
    assert op % 16 == 0 and op2 % 16 == 0
    s = _s()

    def rejected(name, fn, *args):
        assert fn(*args) == EINVAL, (name, args)
        assert name + ":" in _err(), (name, args, _err())

    n = _name(mt, "weight_transform")
    for args in ((None, op, Cout, Cin), (sp, None, Cout, Cin), (sp, op, 0, Cin), (sp, op, Cout, 0), (sp, op, -1, Cin)):
        rejected(n, f("weight_transform"), *args, s)
        rejected(n + "_dgrad", f("weight_transform_dgrad"), *args, s)
    n = _name(mt, "input_transform")
    for args in ((None, op, N, H, W, Cin), (sp, None, N, H, W, Cin), (sp, op, 0, H, W, Cin), (sp, op, N, 0, W, Cin), (sp, op, N, H, 0, Cin),
                 (sp, op, N, H, W, 0), (sp, op, N, H, W, 6), (sp + 4, op, N, H, W, Cin), (sp, op + 8, N, H, W, Cin)):
        rejected(n, f("input_transform"), *args, s)
    n = _name(mt, "gemm")
    for args in ((None, sp, op, T, Cin, Cout), (sp, None, op, T, Cin, Cout), (sp, sp, None, T, Cin, Cout), (sp, sp, op, 0, Cin, Cout),
                 (sp, sp, op, T, 16, Cout), (sp, sp, op, T, 48, Cout), (sp, sp, op, T, 0, Cout), (sp, sp, op, T, Cin, 0),
                 (sp + 4, sp, op, T, Cin, Cout), (sp, sp + 8, op, T, Cin, Cout), (sp, sp, op + 4, T, Cin, Cout)):
        rejected(n, f("gemm"), *args, s)
    # the output pass, through the tile's entry point and through cvk_w2d_output_plain (which takes no Cin)
    outs = (  # Mo, bias, y, stats, counts, N, H, W, Cin, Cout, ldy
        (None, None, op, None, None, N, H, W, Cin, Cout, Cout), (sp, None, None, None, None, N, H, W, Cin, Cout, Cout),
        (sp, None, op, None, None, 0, H, W, Cin, Cout, Cout), (sp, None, op, None, None, N, 0, W, Cin, Cout, Cout),
        (sp, None, op, None, None, N, H, 0, Cin, Cout, Cout),
        (sp, None, op, None, None, N, H, W, Cin, 60, 60), (sp, None, op, None, None, N, H, W, Cin, 32, 64), (sp, None, op, None, None, N, H, W, Cin, 66, 68),
        (sp, None, op, None, None, N, H, W, Cin, Cout, Cout - 4), (sp, None, op, None, None, N, H, W, Cin, Cout, Cout + 2),
        (sp, None, op, op2, None, N, H, W, Cin, Cout, Cout), (sp, None, op, None, op3, N, H, W, Cin, Cout, Cout),
        (sp + 4, None, op, None, None, N, H, W, Cin, Cout, Cout), (sp, None, op + 8, None, None, N, H, W, Cin, Cout, Cout))
    for args in outs:
        rejected(_name(mt, "output"), f("output"), *args, s)
        rejected("cvk_w2d_output_plain", lib.cvk_w2d_output_plain, mt, *args[:8], *args[9:], s)
    for cin in (0, 16, 48):
        rejected(_name(mt, "output"), f("output"), sp, None, op, None, None, N, H, W, cin, Cout, Cout, s)
    rejected("cvk_w2d_output_plain", lib.cvk_w2d_output_plain, 5, sp, None, op, None, None, N, H, W, Cout, Cout, s)
    for name in ("dy_transform", "dy_transform_both"):
        both = name.endswith("both")
        for dyq, ld, e1, e2, n_, c in ((None, Cout, op, op2, N, Cout), (sp, Cout, None, op2, N, Cout), (sp, Cout, op, op2, 0, Cout), (sp, Cout, op, op2, N, 0),
                                      (sp, Cout, op, op2, N, 6), (sp, Cout - 4, op, op2, N, Cout), (sp, Cout + 2, op, op2, N, Cout),
                                      (sp + 4, Cout, op, op2, N, Cout), (sp, Cout, op + 8, op2, N, Cout)):
            ptrs = (e2, e1) if both else (e1,)                       # the second operand of _both is E; V' stands first
            rejected(_name(mt, name), f(name), dyq, ld, *ptrs, n_, H, W, c, s)
    rejected(_name(mt, "dy_transform_both"), f("dy_transform_both"), sp, Cout, None, op, N, H, W, Cout, s)
    rejected(_name(mt, "dy_transform_both"), f("dy_transform_both"), sp, Cout, op2 + 4, op, N, H, W, Cout, s)
    tn = ((None, sp, op, T, Cin, Cout), (sp, None, op, T, Cin, Cout), (sp, sp, None, T, Cin, Cout), (sp, sp, op, 0, Cin, Cout), (sp, sp, op, T, 0, Cout),
          (sp, sp, op, T, 6, Cout), (sp, sp, op, T, Cin, 0), (sp, sp, op, T, Cin, 6), (sp + 4, sp, op, T, Cin, Cout), (sp, sp + 8, op, T, Cin, Cout),
          (sp, sp, op + 4, T, Cin, Cout))
    for args in tn:
        rejected(_name(mt, "gemm_tn"), f("gemm_tn"), *args, s)
        rejected(_name(mt, "gemm_tn_wg"), f("gemm_tn_wg"), *args, 0, s)
    rejected(_name(mt, "gemm_tn_wg"), f("gemm_tn_wg"), sp, sp, op, T, Cin, Cout, -1, s)
    for args in ((None, op, T, Cin, Cin, Cout), (sp, None, T, Cin, Cin, Cout), (sp, op, 0, Cin, Cin, Cout), (sp, op, T, 0, Cin, Cout),
                 (sp, op, T, Cin + 4, Cin, Cout), (sp, op, T, Cin, Cin, 0)):
        rejected(_name(mt, "wgrad_output"), f("wgrad_output"), *args, s)
    for args in ((5, sp, op, Cin, Cin, Cout, 1), (mt, None, op, Cin, Cin, Cout, 1), (mt, sp, None, Cin, Cin, Cout, 1), (mt, sp, op, 0, Cin, Cout, 1),
                 (mt, sp, op, Cin + 4, Cin, Cout, 1), (mt, sp, op, Cin, Cin, 0, 1), (mt, sp, op, Cin, Cin, Cout, 0), (mt, sp, op, Cin, Cin, Cout, 65)):
        rejected("cvk_w2d_wgrad_output_f", lib.cvk_w2d_wgrad_output_f, *args, s)
    torch.cuda.synchronize()
    for b in (out, out2, out3):
        assert bool(torch.isnan(b.t).all()), "a rejected call wrote"
        b.check_guard("rejected call")


def test_host_side_contract_of_the_fused_calls():
    """cvk_conv3x3_w2d and cvk_conv3x3_wgrad_w2d reject before their first pass: y, dW and the workspace stay NaN.  Cin = 16 is below what the
    workspace query knows (it answers 0): the call must not take that for a workspace that is large enough."""
    lib, _ = _lib()
    N, H, W, Cin, Cout = 1, 4, 8, 32, 64
    src = torch.zeros(36 * 32 * Cout + 1024, device="cuda")
    sp, s = src.data_ptr(), _s()
    nb = lib.cvk_conv3x3_w2d_workspace_bytes(N, H, W, 64, Cout)             # sized for the widest Cin tried below
    ws, y, st, cnt = Buf(nb // 4), Buf(N * H * W * (Cout + 8)), Buf(2 * 2 * Cout), Buf(2)
    assert ws.ptr() % 16 == 0 and y.ptr() % 16 == 0

    def fwd(xq=sp, uq=sp, yq=y.ptr(), stq=None, cq=None, n=N, cin=Cin, cout=Cout, ldy=Cout, wsq=ws.ptr(), nbytes=nb):
        return lib.cvk_conv3x3_w2d(xq, uq, None, yq, stq, cq, n, H, W, cin, cout, ldy, wsq, nbytes, s)
    need = lib.cvk_conv3x3_w2d_workspace_bytes(N, H, W, Cin, Cout)
    for kw in (dict(xq=None), dict(uq=None), dict(yq=None), dict(wsq=None), dict(n=0), dict(cin=16), dict(cin=48), dict(cin=0), dict(cout=60, ldy=60),
               dict(cout=66, ldy=68), dict(ldy=Cout - 4), dict(ldy=Cout + 2), dict(stq=st.ptr()), dict(cq=cnt.ptr()), dict(xq=sp + 4), dict(uq=sp + 8),
               dict(yq=y.ptr() + 4), dict(wsq=ws.ptr() + 4), dict(nbytes=need - 1), dict(nbytes=0), dict(cin=16, nbytes=0)):
        assert fwd(**kw) == EINVAL, kw
        assert "cvk_conv3x3_w2d:" in _err(), (kw, _err())
    nbw = lib.cvk_conv3x3_wgrad_w2d_workspace_bytes(N, H, W, Cin, Cout)
    wsw, dw = Buf(nbw // 4), Buf(Cout * 9 * Cin)

    def wgrad(xq=sp, dyq=sp, dwq=dw.ptr(), n=N, cin=Cin, cin_pad=Cin, cout=Cout, ld=Cout, wsq=wsw.ptr(), nbytes=nbw):
        return lib.cvk_conv3x3_wgrad_w2d(xq, dyq, dwq, n, H, W, cin, cin_pad, cout, ld, wsq, nbytes, s)
    for kw in (dict(dyq=None), dict(dwq=None), dict(wsq=None), dict(n=0), dict(cin=0), dict(cin=Cin + 4), dict(cin_pad=Cin + 2), dict(cout=0), dict(cout=66),
               dict(ld=Cout - 4), dict(ld=Cout + 2), dict(xq=sp + 4), dict(dyq=sp + 8), dict(wsq=wsw.ptr() + 4), dict(nbytes=nbw - 1), dict(nbytes=0)):
        assert wgrad(**kw) == EINVAL, kw
        assert "cvk_conv3x3_wgrad_w2d:" in _err(), (kw, _err())
    torch.cuda.synchronize()
    for b in (ws, y, st, cnt, wsw, dw):
        assert bool(torch.isnan(b.t).all()), "a rejected call wrote"
        b.check_guard("rejected call")
