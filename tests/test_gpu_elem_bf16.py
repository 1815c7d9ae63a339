"""The ten elementwise entry points of the bf16-storage mode (csrc/elem_bf16.hip) called directly through the C ABI, each dispatch arm
by a named case, against the fp64 restatements of tests/elem_bf16_ref.py (whose own correctness tests/test_elem_bf16_ref_cpu.py
checks against torch).

Conventions of every test:
  * inputs come from seeded torch.Generators; bf16 operands are rounded on the host, so kernel and reference see identical values;
  * every output lives in a buffer with a guard of 64 elements before and after it, pre-filled with a NaN bit pattern (bf16 0x7FC1,
    fp32 0x7FC00001).  After the call every element the contract does not write (guards, the other channels of a wider buffer, the
    frame around a spatial sub-window) must still hold exactly those bits, and every element it does write must be finite;
  * input pad columns (ldy > C) hold NaN: a read of them would surface in the finite check.

Tolerances are derived, none is measured.  u = 2^-24 is the unit roundoff of the fp32 arithmetic inside the kernels.
  * stored as bf16:  |got - ref| <= bf16_half_ulp(ref) + A.  The first term is one round-to-nearest of the exact value (truncation errs by
    up to twice that; a tie may still fall either way), A the first-order fp32 error of the kernel's expression:
      apply      A = 3u (|y*scale| + |shift|)         product, sum, and one to spare for the fused form
      dy         A = 6u |scale| (|g| + |dbeta|/M + |xhat*dgamma|/M)      1/M, two products, xhat (two roundings), two differences, scale
      bilinear   A = 8 max(H,W) u max|input|          the tap position scale*dst is an fp32 product of up to max(H,W): 2u max(H,W) per
                                                      axis on a weight, times a difference of two inputs (2 max|input|), two axes
      its adjoint A = 40u sum|w*g|                    the general form of the sums below with at most 36 terms
  * stored as fp32:  A + u |ref|.
  * column sums (partials finalised by cvk_colsum_finalize): (ceil(rows/ppp) + ppp + 8) u sum|term| per channel: a thread adds
    ceil(rows/ppp) terms in sequence, one thread adds the ppp threads' results, 8 covers the term's own arithmetic (<= 6u above) and the
    fp64 finalisation's rounding to fp32; rows = ceil(M/PB), PB = cvk_bn_bwd_blocks_bf16(M), ppp = 256 // (C/V) with V the vector
    width the case's alignment selects.  The terms are g, g*xhat and the UNROUNDED dy: the dx pass sums its fp32 dy before the bf16
    store (k_bnbwd_bf16: `s0[j] += r`), so the reference sums the fp64 dy, not the stored one.
  * passes without arithmetic are compared bitwise: import, pool scatter (with accumulation: one rounding of an exact fp32 sum), zero
    frame, the pooled tensor of the apply pass.

Excluded elements: the device evaluates the ReLU mask in fp32; an element whose fp64 z lies in the band of elem_bf16_ref.bn_bwd_terms
may fall either way and is left out of the backward comparisons, its column out of the sum comparisons.  At most 1e-5 of a case's
elements and never more than 8 may be excluded, else the test fails.  With the generators here no small case has any (asserted on
the CPU by tests/test_elem_bf16_ref_cpu.py).  Exact zeros are NOT excluded: channel 0 has shift = 0 and some y = 0, so z = 0 exactly;
there the output is 0 and the gradient is masked (z > 0, not >= 0).

Dispatch arms against cases (kernel instantiations as a kernel trace names them):
  k_apply_bf16<8,false,false,true>   APPLY v8_dense, v8_window, v8_ldy32        k_apply_bf16<8,false,true,true>   APPLY v8_pool_odd_slice
  k_apply_bf16<8,true,false,false>   APPLY v8_f32                               k_apply_bf16<4,true,false,false>  APPLY v4_f32_logits
  k_apply_bf16<4,false,false,false>  APPLY v4_bf16, v4_by_pitch                 k_apply_bf16<4,false,true,false>  APPLY v4_pool
  (the 8-wide bf16 arms without streaming loads exist only behind the experiments build's switch: the product library never takes them)
  k_bnbwd_bf16<8,0,false,false>  BN v8_c64_m71, v8_c24_ldy32_slice, v8_c8_m19500, v8_c1024, v8_c2048, v8_c32_window
  k_bnbwd_bf16<8,0,true,false>   BN v8_c64_m70_f32            k_bnbwd_bf16<4,0,true,false>  BN v4_c12_f32, v4_c12_window_f32
  k_bnbwd_bf16<4,0,false,false>  BN v4_c12_m71, v4_c1024_ldy1028                 k_bnbwd_bf16<V,1,...>: the same cases through the dx pass
  k_bnbwd_bf16<8,0,false,true>, k_bnbwd_bf16<8,1,false,true>   test_streaming_variants_at_the_128_mib_threshold
  k_bilinear_fwd_bf16<8>  C in {8, 64}       k_bilinear_fwd_bf16_tiled  C in {128, 256}"""
import pytest
import torch

from tests import elem_bf16_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U = R.U32
GUARD = 64
SENT16 = 0x7FC1          # a quiet bf16 NaN no kernel produces
SENT32 = 0x7FC00001      # the same for fp32
EPS = 1e-5


# ------------------------------------------------------------------------------------------------ shared: generators and cases
def bn_inputs(shape, seed, dout_f32, device="cpu"):
    """The operands of one BatchNorm case, [M, C] row-major over (N,H,W): y bf16, dout bf16 or fp32, per-channel fp32 constants.
    Channel 0 carries the exact-zero edge: shift = 0 and every third y = 0."""
    N, H, W, C = shape
    M = N * H * W
    g = torch.Generator(device=device).manual_seed(seed)
    y = (torch.randn(M, C, generator=g, device=device) * 1.3 + 0.2).to(BF)
    y[::3, 0] = 0.0
    gamma = torch.rand(C, generator=g, device=device) + 0.5
    beta = 0.3 * torch.randn(C, generator=g, device=device)
    y64 = y.double()
    mean = y64.mean(0).float()
    rstd = (y64.var(0, unbiased=False) + EPS).rsqrt().float()
    del y64
    scale = gamma * rstd
    shift = beta - mean * scale
    shift[0] = 0.0
    dout = torch.randn(M, C, generator=g, device=device)
    if not dout_f32:
        dout = dout.to(BF)
    return {"y": y, "dout": dout, "scale": scale, "shift": shift, "mean": mean, "rstd": rstd}


def excluded_cap(numel):
    return min(8, int(1e-5 * numel))


# name: (N,H,W,C), ldy, dout_f32, view of dout, V (the vector width the alignment selects)
BN_CASES = {
    "v8_c64_m71": ((1, 1, 71, 64), 64, 0, "dense", 8),                # ragged last row block (rows 15, last block 11)
    "v8_c64_m70_f32": ((2, 5, 7, 64), 64, 1, "dense", 8),             # full last block, fp32 gradient
    "v4_c12_f32": ((2, 5, 7, 12), 12, 1, "dense", 4),                 # the logits' layer: cvn 3, ppp 85, thread 255 idle
    "v4_c12_m71": ((1, 1, 71, 12), 12, 0, "dense", 4),
    "v8_c24_ldy32_slice": ((2, 5, 7, 24), 32, 0, "slice", 8),         # cvn 3 eight-wide, ldy > C, gradient = channel slice of a wider buffer
    "v8_c8_m19500": ((1, 150, 130, 8), 8, 0, "dense", 8),             # ppp 256, rows 20, PB 975
    "v8_c1024": ((1, 3, 5, 1024), 1024, 0, "dense", 8),
    "v8_c2048": ((1, 3, 5, 2048), 2048, 0, "dense", 8),               # ppp 1
    "v4_c1024_ldy1028": ((1, 3, 5, 1024), 1028, 0, "dense", 4),       # demoted to four-wide by the pitch: cvn 256
    "v8_c32_window": ((2, 4, 6, 32), 32, 0, "window", 8),             # gradient = spatial sub-window: the non-linear pixel map
    "v4_c12_window_f32": ((2, 4, 6, 12), 12, 1, "window", 4),
}

# name: (N,H,W,C), ldy, out_f32, pool, layout of the output view, V
APPLY_CASES = {
    "v8_dense": ((2, 5, 7, 64), 64, 0, 0, {}, 8),
    "v8_pool_odd_slice": ((1, 9, 7, 64), 64, 0, 1, {"ld": 128, "c0": 64}, 8),
    "v8_window": ((2, 4, 6, 32), 32, 0, 0, {"ph": 3, "pw": 4, "y0": 1, "x0": 2}, 8),
    "v8_f32": ((2, 6, 10, 16), 16, 1, 0, {}, 8),
    "v4_f32_logits": ((2, 5, 7, 12), 12, 1, 0, {}, 4),
    "v4_bf16": ((2, 5, 7, 12), 12, 0, 0, {}, 4),
    "v4_pool": ((2, 4, 6, 20), 20, 0, 1, {}, 4),
    "v4_by_pitch": ((2, 5, 7, 64), 68, 0, 0, {}, 4),
    "v8_ldy32": ((2, 5, 7, 24), 32, 0, 0, {}, 8),
}


def case_seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003


# ------------------------------------------------------------------------------------------------ shared: buffers and views
def dev():
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def libs():
    from pytorch_camvid_amd import _lib
    return _lib, _lib.load()


class Box:
    """n elements of device memory between two guards, everything pre-filled with the sentinel bits."""

    def __init__(self, n, f32=False):
        self.n, self.f32 = n, f32
        self.sent = SENT32 if f32 else SENT16
        self.raw = torch.full((GUARD + n + GUARD,), self.sent, dtype=torch.int32 if f32 else torch.int16, device=dev())
        self.esize = self.raw.element_size()
        self.ptr = self.raw.data_ptr() + GUARD * self.esize
        assert self.ptr % 16 == 0

    def body(self):
        """typed device view of the n elements"""
        return self.raw[GUARD:GUARD + self.n].view(torch.float32 if self.f32 else BF)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == self.sent).all()) and bool((self.raw[GUARD + self.n:] == self.sent).all())

    def settle(self, written, finite=True):
        """host copy (bits, values) of the n elements, after checking the guards, that everything outside `written` (a flat bool
        mask; True = all) still holds the sentinel, and that everything inside it is finite"""
        torch.cuda.synchronize()
        h = self.raw.cpu()
        assert bool((h[:GUARD] == self.sent).all()) and bool((h[GUARD + self.n:] == self.sent).all()), "a guard was overwritten"
        bits = h[GUARD:GUARD + self.n]
        vals = bits.view(torch.float32 if self.f32 else BF)
        if written is True:
            written = torch.ones(self.n, dtype=torch.bool)
        written = written.reshape(-1)
        assert bool((bits[~written] == self.sent).all()), "an element outside the contract was written"
        if finite:
            assert bool(torch.isfinite(vals[written].float()).all()), "a written element is not finite (or was left unwritten)"
        return bits, vals


class Lay:
    """An [N,H,W,C] view inside a buffer [N][H+ph][W+pw][ld], starting at (y0, x0, c0)."""

    def __init__(self, shape, ld=None, ph=0, pw=0, y0=0, x0=0, c0=0):
        self.N, self.H, self.W, self.C = shape
        self.ld = ld or self.C
        self.Hb, self.Wb, self.y0, self.x0, self.c0 = self.H + ph, self.W + pw, y0, x0, c0
        self.shape = (self.N, self.Hb, self.Wb, self.ld)
        self.numel = self.N * self.Hb * self.Wb * self.ld
        self.offset = (y0 * self.Wb + x0) * self.ld + c0
        self.strides = (self.Hb * self.Wb * self.ld, self.Wb * self.ld, self.ld)

    def view(self, ptr, esize):
        _lib, _ = libs()
        return _lib.ViewH(ptr + self.offset * esize, *self.strides)

    def window(self, t):
        """the view's elements of a flat or buffer-shaped host tensor, as [N,H,W,C]"""
        return t.reshape(self.shape)[:, self.y0:self.y0 + self.H, self.x0:self.x0 + self.W, self.c0:self.c0 + self.C]

    def mask(self):
        m = torch.zeros(self.shape, dtype=torch.bool)
        self.window(m)[...] = True
        return m.reshape(-1)

    def embed(self, values, fill=float("nan")):
        """host buffer with `values` [N,H,W,C] in the view and `fill` elsewhere"""
        b = torch.full(self.shape, fill, dtype=values.dtype)
        self.window(b)[...] = values.reshape(self.N, self.H, self.W, self.C)
        return b


DOUT_LAYOUTS = {"dense": {}, "slice": {"ld": 48, "c0": 8}, "window": {"ph": 3, "pw": 4, "y0": 1, "x0": 2}}


def rows_padded(t, ld):
    """[M, C] -> device [M, ld] with NaN pad columns"""
    b = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype)
    b[:, :t.shape[1]] = t
    return b.to(dev())


def report(entry, case, frac):
    print(f"[elem_bf16] {entry} {case}: largest error = {frac:.3f} of its bound")


def worst_fraction(err, bound, keep=None):
    """max err/bound over the kept elements; a zero bound admits a zero error only"""
    ok0 = (bound > 0) | (err == 0)
    f = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)), torch.zeros_like(err))
    if keep is not None:
        ok0, f = ok0 | ~keep, torch.where(keep, f, torch.zeros_like(f))
    assert bool(ok0.all()), "a nonzero error where the bound is zero"
    return float(f.max()) if f.numel() else 0.0


def d64(inp):
    return {k: v.double() for k, v in inp.items()}


# ------------------------------------------------------------------------------------------------ 1. import
IMPORT_CASES = {  # name: (N, C, H, W, ld), how the source is laid out
    "contiguous": ((2, 3, 5, 7, 32), "contiguous"),
    "channels_last": ((1, 3, 4, 6, 8), "channels_last"),
    "spatial_slice": ((2, 12, 3, 5, 16), "slice"),
    "no_pad": ((1, 8, 2, 3, 8), "contiguous"),
}
SPECIALS = [1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 0.0, -0.0,
            float("inf"), float("-inf"), 3.4e38, -3.4e38, 3.3895313892515355e38, 2.0 ** -126, 2.0 ** -133 * 1.5]


@pytest.mark.parametrize("name", list(IMPORT_CASES))
def test_import_nchw_bf16_is_bitwise_round_to_nearest_even(name):
    """cvk_import_nchw_bf16: no arithmetic, so channels < C are bitwise rne_bf16(src) for any source strides, and the pad channels
    are +0 bits.  The values include exact ties (1 + 2^-8 and its fp32 neighbours, 1 + 3*2^-8), both zeros, both infinities, finite
    values that round to infinity (3.4e38) and the largest one that does not, the smallest normal and a subnormal — so here, and only
    here, written elements may be infinite."""
    _lib, lib = libs()
    (N, C, H, W, ld), kind = IMPORT_CASES[name]
    g = torch.Generator().manual_seed(case_seed(name))
    vals = torch.randn(N, C, H, W, generator=g)
    vals.view(-1)[:len(SPECIALS)] = torch.tensor(SPECIALS)
    vals = vals.view(-1)[torch.randperm(vals.numel(), generator=g)].view(N, C, H, W)
    if kind == "contiguous":
        src = vals.to(dev())
    elif kind == "channels_last":
        src = vals.to(dev()).contiguous(memory_format=torch.channels_last)
        assert src.stride(1) == 1
    else:
        big = torch.full((N, C, H + 2, W + 3), float("nan"))
        big[:, :, 1:-1, 2:-1] = vals
        src = big.to(dev())[:, :, 1:-1, 2:-1]
        assert not src.is_contiguous()
    out = Box(N * H * W * ld)
    _lib.check(lib.cvk_import_nchw_bf16(src.data_ptr(), *src.stride(), out.ptr, ld, N, C, H, W, stream()))
    bits, _ = out.settle(True, finite=False)
    bits = bits.view(N, H, W, ld)
    want = R.rne_bf16(vals).permute(0, 2, 3, 1).contiguous().view(torch.int16)
    assert torch.equal(bits[..., :C], want)
    assert bool((bits[..., C:] == 0).all())
    assert bool(torch.isinf(want.view(BF).float()).any()) and bool((want == -32768).any())        # the edge values are really in there


# ------------------------------------------------------------------------------------------------ 2. apply
@pytest.mark.parametrize("name", list(APPLY_CASES))
def test_bn_relu_apply_bf16(name):
    """cvk_bn_relu_apply_bf16, one case per dispatch arm.  Bound: bf16_half_ulp(ref) + 3u (|y*scale| + |shift|) for bf16 outputs,
    3u (|y*scale| + |shift|) + u |ref| for fp32 ones (module docstring).  With the fused pool, the pooled tensor is bitwise the maximum
    of the kernel's OWN stored outputs over every full 2x2 cell (odd trailing rows and columns feed no cell).
    NaN inputs are kept out on purpose: fmaxf(NaN, 0) returns 0 on the device where torch's ReLU propagates the NaN; the network never
    feeds one, and the behaviour is left as it is."""
    _lib, lib = libs()
    shape, ldy, f32, pool, lay_kw, V = APPLY_CASES[name]
    N, H, W, C = shape
    assert V == (8 if C % 8 == 0 and ldy % 8 == 0 and all(lay_kw.get(k, 0) % 8 == 0 for k in ("ld", "c0")) else 4)
    inp = bn_inputs(shape, case_seed(name), 0)
    lay = Lay(shape, **lay_kw)
    y = rows_padded(inp["y"], ldy)
    sc, sh = inp["scale"].to(dev()), inp["shift"].to(dev())
    out = Box(lay.numel, f32=bool(f32))
    pl = Box(N * (H // 2) * (W // 2) * C) if pool else None
    _lib.check(lib.cvk_bn_relu_apply_bf16(y.data_ptr(), ldy, sc.data_ptr(), sh.data_ptr(), lay.view(out.ptr, out.esize), f32,
                                          pl.ptr if pool else None, N, H, W, C, stream()))
    _, vals = out.settle(lay.mask())
    got = lay.window(vals).double()
    q = d64(inp)
    y64 = q["y"].view(N, H, W, C)
    ref = R.apply(y64, q["scale"], q["shift"])
    A = 3 * U * ((y64 * q["scale"]).abs() + q["shift"].abs())
    bound = A + U * ref.abs() if f32 else R.bf16_half_ulp(ref) + A
    frac = worst_fraction((got - ref).abs(), bound)
    report("cvk_bn_relu_apply_bf16", name, frac)
    assert frac <= 1.0
    zero_edge = (y64[..., 0] == 0)
    assert bool(zero_edge.any()) and bool((got[..., 0][zero_edge] == 0).all())
    if pool:
        pbits, _ = pl.settle(True)
        want = R.pool2x2(lay.window(vals).float()).to(BF).contiguous().view(torch.int16).reshape(-1)
        assert torch.equal(pbits, want)


# ------------------------------------------------------------------------------------------------ 3. / 4. BatchNorm + ReLU backward
def bn_device_operands(name):
    shape, ldy, f32, kind, V = BN_CASES[name]
    N, H, W, C = shape
    inp = bn_inputs(shape, case_seed(name), f32)
    lay = Lay(shape, **DOUT_LAYOUTS[kind])
    strides_ok = all(s % (4 if f32 else 8) == 0 for s in lay.strides) and (lay.offset * (4 if f32 else 2)) % 16 == 0
    assert V == (8 if C % 8 == 0 and ldy % 8 == 0 and strides_ok else 4)
    dout = lay.embed(inp["dout"]).to(dev())
    ops = {"y": rows_padded(inp["y"], ldy), "dout": dout, "view": lay.view(dout.data_ptr(), dout.element_size())}
    for k in ("scale", "shift", "mean", "rstd"):
        ops[k] = inp[k].to(dev())
    return inp, ops


def sum_factor(lib, M, C, V):
    PB = lib.cvk_bn_bwd_blocks_bf16(M)
    rows = -(-M // PB)
    ppp = 256 // (C // V)
    return PB, (-(-rows // ppp) + ppp + 8) * U


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


@pytest.mark.parametrize("name", list(BN_CASES))
def test_bn_bwd_reduce_bf16(name):
    """cvk_bn_bwd_reduce_bf16 + cvk_colsum_finalize: dbeta = sum g and dgamma = sum g*xhat per channel within
    (ceil(rows/ppp) + ppp + 8) u sum|term| (module docstring), for every vector width, lane layout, row blocking (M = 71 leaves a ragged
    last block, M = 70 none), gradient type and gradient view.  The zero edge of channel 0 tests the strict mask: with `>=` the
    gradients at z == 0 would enter the sums.  Columns holding an excluded element are left out (cap: module docstring)."""
    _lib, lib = libs()
    shape, ldy, f32, kind, V = BN_CASES[name]
    N, H, W, C = shape
    M = N * H * W
    inp, ops = bn_device_operands(name)
    PB, factor = sum_factor(lib, M, C, V)
    part = Box(2 * PB * C, f32=True)
    _lib.check(lib.cvk_bn_bwd_reduce_bf16(ops["view"], f32, ops["y"].data_ptr(), ldy, ops["scale"].data_ptr(), ops["shift"].data_ptr(),
                                          ops["mean"].data_ptr(), ops["rstd"].data_ptr(), part.ptr, N, H, W, C, stream()))
    db, dg = Box(C, f32=True), Box(C, f32=True)
    _lib.check(lib.cvk_colsum_finalize(part.ptr, PB, C, db.ptr, dg.ptr, stream()))
    part.settle(True)
    q, g, gx, band = reference_terms(name, inp)
    cols = ~band.any(0)
    check_sums("cvk_bn_bwd_reduce_bf16 dbeta", name, db.settle(True)[1], g, factor, cols)
    check_sums("cvk_bn_bwd_reduce_bf16 dgamma", name, dg.settle(True)[1], gx, factor, cols)


def test_bn_bwd_bf16_rejects_more_than_256_channel_vectors():
    """C = 1028 is no multiple of 8, so access is four-wide: 257 channel vectors for 256 threads.  The call must fail with an error
    code and a message, without a launch (the partial buffer keeps its sentinel)."""
    _lib, lib = libs()
    C = 1028
    y = torch.zeros(2, C, dtype=BF, device=dev())
    d = torch.zeros(2, C, dtype=BF, device=dev())
    c = torch.zeros(4, C, device=dev())
    part = Box(2 * C, f32=True)
    rc = lib.cvk_bn_bwd_reduce_bf16(_lib.ViewH(d.data_ptr(), 2 * C, 2 * C, C), 0, y.data_ptr(), C, c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(),
                                    c[3].data_ptr(), part.ptr, 1, 1, 2, C, stream())
    assert rc != 0
    msg = lib.cvk_last_error_string().decode()
    assert "cvk_bn_bwd_reduce_bf16" in msg and "1028" in msg, msg
    with pytest.raises(_lib.CvkError):
        _lib.check(rc)
    part.settle(torch.zeros(2 * C, dtype=torch.bool))


@pytest.mark.parametrize("use_batch_stats", [1, 0])
@pytest.mark.parametrize("name", list(BN_CASES))
def test_bn_bwd_dx_bf16(name, use_batch_stats):
    """cvk_bn_bwd_dx_bf16 with ld_dy = max(32, C) as the engine passes it: dy within bf16_half_ulp(ref) + 6u |scale| (|g| + |dbeta|/M +
    |xhat*dgamma|/M); the pad columns C..ld_dy-1 (C = 12, 24) are +0 bits in every row, the last block's included; the column sums
    of the unrounded dy within the bound of the sums; without a partial buffer the same dy bits and nothing else.  dgamma and dbeta
    are the fp64 reference's sums rounded to fp32; with running statistics (use_batch_stats = 0) the kernel must not look at them:
    they are NaN then.  A wrong 1/M (M + 1 for M, say) moves the masked elements of the batch-statistics form by a relative 1/(M + 1):
    1.4 % at M = 70, several bf16 spacings; the zero edge of channel 0 tests the strict mask."""
    _lib, lib = libs()
    shape, ldy, f32, kind, V = BN_CASES[name]
    N, H, W, C = shape
    M = N * H * W
    ld_dy = max(32, C)
    inp, ops = bn_device_operands(name)
    PB, factor = sum_factor(lib, M, C, V)
    q, g, gx, band = reference_terms(name, inp)
    if use_batch_stats:
        dgamma, dbeta = gx.sum(0).float(), g.sum(0).float()
    else:
        dgamma = dbeta = torch.full((C,), float("nan"))
    dgd, dbd = dgamma.to(dev()), dbeta.to(dev())

    def run(with_part):
        dy = Box(M * ld_dy)
        part = Box(PB * C, f32=True) if with_part else None
        _lib.check(lib.cvk_bn_bwd_dx_bf16(ops["view"], f32, ops["y"].data_ptr(), ldy, ops["scale"].data_ptr(), ops["shift"].data_ptr(),
                                          ops["mean"].data_ptr(), ops["rstd"].data_ptr(), dgd.data_ptr(), dbd.data_ptr(), dy.ptr, ld_dy,
                                          part.ptr if with_part else None, N, H, W, C, use_batch_stats, stream()))
        return dy, part
    dy, part = run(True)
    bits, vals = dy.settle(True)
    assert bool((bits.view(M, ld_dy)[:, C:] == 0).all()), "pad columns of dy are not +0"
    got = vals.view(M, ld_dy)[:, :C].double()
    ref = R.bn_bwd_dy(q["dout"], q["y"], q["scale"], q["shift"], q["mean"], q["rstd"], dgamma.double(), dbeta.double(), M, use_batch_stats)
    xhat = (q["y"] - q["mean"]) * q["rstd"]
    A = 6 * U * q["scale"].abs() * (g.abs() + ((dbeta.double().abs() + (xhat * dgamma.double()).abs()) / M if use_batch_stats else 0.0))
    frac = worst_fraction((got - ref).abs(), R.bf16_half_ulp(ref) + A, keep=~band)
    report("cvk_bn_bwd_dx_bf16 dy", f"{name} stats={use_batch_stats}", frac)
    assert frac <= 1.0
    if not use_batch_stats:                                  # masked elements are exact zeros, the zero edge among them
        assert bool((got[:, 0][q["y"][:, 0] == 0] == 0).all())
    part.settle(True)
    dbias = Box(C, f32=True)
    _lib.check(lib.cvk_colsum_finalize(part.ptr, PB, C, dbias.ptr, None, stream()))
    check_sums("cvk_bn_bwd_dx_bf16 column sums", f"{name} stats={use_batch_stats}", dbias.settle(True)[1], ref, factor, ~band.any(0))
    dy2, _ = run(False)
    bits2, _ = dy2.settle(True)
    assert torch.equal(bits, bits2)


def test_streaming_variants_at_the_128_mib_threshold():
    """The two streaming-load instantiations of k_bnbwd_bf16 (reduce and dx with a bf16 gradient) are taken from 128 MiB per tensor
    on: [4,512,512,64] bf16 is exactly that.  Same bounds as the small cases; rows = 1024, ppp = 32.  The fp64 reference is computed
    with plain torch operations on the device, eight channels at a time (a host reference of 67 M elements would take minutes).
    Excluded elements: at most 8 (1e-5 of 67 M would be 671)."""
    _lib, lib = libs()
    shape = (4, 512, 512, 64)
    N, H, W, C = shape
    M = N * H * W
    assert M * C * 2 == 128 << 20
    inp = bn_inputs(shape, 9, 0, device=dev())
    PB, factor = sum_factor(lib, M, C, 8)
    assert PB == 1024
    view = _lib.ViewH(inp["dout"].data_ptr(), H * W * C, W * C, C)
    ptrs = [inp[k].data_ptr() for k in ("scale", "shift", "mean", "rstd")]
    part = Box(2 * PB * C, f32=True)
    _lib.check(lib.cvk_bn_bwd_reduce_bf16(view, 0, inp["y"].data_ptr(), C, *ptrs, part.ptr, N, H, W, C, stream()))
    db, dg = Box(C, f32=True), Box(C, f32=True)
    _lib.check(lib.cvk_colsum_finalize(part.ptr, PB, C, db.ptr, dg.ptr, stream()))
    c64 = {k: inp[k].double() for k in ("scale", "shift", "mean", "rstd")}

    def block(c0):
        s = slice(c0, c0 + 8)
        return s, [inp["dout"][:, s].double(), inp["y"][:, s].double()] + [c64[k][s] for k in ("scale", "shift", "mean", "rstd")]
    sums = torch.zeros(4, C, dtype=torch.float64, device=dev())
    colbad = torch.zeros(C, dtype=torch.bool, device=dev())
    nband = 0
    for c0 in range(0, C, 8):
        s, a = block(c0)
        mask, g, gx, band = R.bn_bwd_terms(*a)
        nband += int(band.sum())
        colbad[s] = band.any(0)
        sums[0, s], sums[1, s], sums[2, s], sums[3, s] = g.sum(0), g.abs().sum(0), gx.sum(0), gx.abs().sum(0)
        if c0 == 0:
            edge = a[1][:, 0] == 0
            assert bool(edge.any()) and not bool(mask[:, 0][edge].any()) and not bool(band[:, 0][edge].any())
    print(f"[elem_bf16] streaming case: {nband} excluded elements")
    assert nband <= excluded_cap(M * C)
    part.settle(True)
    sums, cols = sums.cpu(), ~colbad.cpu()
    for entry, box, i in (("dbeta", db, 0), ("dgamma", dg, 2)):
        frac = worst_fraction((box.settle(True)[1].double() - sums[i]).abs(), factor * sums[i + 1], keep=cols)
        report("cvk_bn_bwd_reduce_bf16 (streaming) " + entry, "4x512x512x64", frac)
        assert frac <= 1.0
    dbeta, dgamma = sums[0].float().to(dev()), sums[2].float().to(dev())
    dy = Box(M * C)
    bpart = Box(PB * C, f32=True)
    _lib.check(lib.cvk_bn_bwd_dx_bf16(view, 0, inp["y"].data_ptr(), C, *ptrs, dgamma.data_ptr(), dbeta.data_ptr(), dy.ptr, C, bpart.ptr,
                                      N, H, W, C, 1, stream()))
    dbias = Box(C, f32=True)
    _lib.check(lib.cvk_colsum_finalize(bpart.ptr, PB, C, dbias.ptr, None, stream()))
    torch.cuda.synchronize()
    assert dy.guards_intact()
    got_all = dy.body().view(M, C)
    dsum = torch.zeros(2, C, dtype=torch.float64, device=dev())
    frac = 0.0
    for c0 in range(0, C, 8):
        s, a = block(c0)
        _, g, _, band = R.bn_bwd_terms(*a)
        ref = R.bn_bwd_dy(*a, dgamma[s].double(), dbeta[s].double(), M, 1)
        xhat = (a[1] - a[4]) * a[5]
        A = 6 * U * a[2].abs() * (g.abs() + (dbeta[s].double().abs() + (xhat * dgamma[s].double()).abs()) / M)
        got = got_all[:, s].double()
        assert bool(torch.isfinite(got).all())
        r = torch.where(band, torch.zeros_like(ref), (got - ref).abs() / (R.bf16_half_ulp(ref) + A))
        frac = max(frac, float(r.max()))
        dsum[0, s], dsum[1, s] = ref.sum(0), ref.abs().sum(0)
    report("cvk_bn_bwd_dx_bf16 (streaming) dy", "4x512x512x64", frac)
    assert frac <= 1.0
    bpart.settle(True)
    dsum = dsum.cpu()
    frac = worst_fraction((dbias.settle(True)[1].double() - dsum[0]).abs(), factor * dsum[1], keep=cols)
    report("cvk_bn_bwd_dx_bf16 (streaming) column sums", "4x512x512x64", frac)
    assert frac <= 1.0


# ------------------------------------------------------------------------------------------------ 5. / 6. bilinear x2
BILINEAR_FWD = [(C, hw) for C in (8, 64) for hw in ((1, 1), (1, 5), (2, 2), (3, 7), (5, 4))] + \
               [(C, hw) for C in (128, 256) for hw in ((2, 2), (3, 17), (5, 33), (9, 16))]


@pytest.mark.parametrize("C,hw", BILINEAR_FWD)
def test_bilinear_up2_fwd_bf16(C, hw):
    """cvk_bilinear_up2_fwd_bf16: the flat kernel (C = 8, 64; one row, one column, one pixel) and the LDS-tiled one (C = 128, 256,
    H, W >= 2: ragged 4 x 32 tiles in both directions, a second tile column at W = 17 and 33, the clamp of the staged input at the
    border, two channel chunks).  Bound: bf16_half_ulp(ref) + 8 max(H,W) u max|input|."""
    _lib, lib = libs()
    N, (H, W) = 2, hw
    g = torch.Generator().manual_seed(1000 * C + 37 * H + W)
    x = torch.randn(N, H, W, C, generator=g).to(BF)
    xd = x.to(dev())
    out = Box(N * 4 * H * W * C)
    _lib.check(lib.cvk_bilinear_up2_fwd_bf16(xd.data_ptr(), out.ptr, N, H, W, C, stream()))
    _, vals = out.settle(True)
    ref = R.bilinear_up2(x.double())
    bound = R.bf16_half_ulp(ref) + 8 * max(H, W) * U * float(x.double().abs().max())
    frac = worst_fraction((vals.view(ref.shape).double() - ref).abs(), bound)
    report("cvk_bilinear_up2_fwd_bf16", f"C={C} {H}x{W}", frac)
    assert frac <= 1.0


@pytest.mark.parametrize("shape", [(2, 1, 1, 8), (1, 2, 2, 8), (2, 3, 7, 64), (3, 5, 40, 64), (1, 9, 16, 128)])
def test_bilinear_up2_bwd_bf16(shape):
    """cvk_bilinear_up2_bwd_bf16, the 6 x 6 gather: one pixel, the smallest interpolating size, odd sizes, [3,5,40,64] = 320 work items
    per row (two workgroups per row, the second ragged; 30 workgroups: no multiple of 8 for the XCD remap), 128 channels.  Bound:
    bf16_half_ulp(ref) + 40u sum|w*g| (the general form of the sums: at most 36 terms)."""
    _lib, lib = libs()
    N, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    go = torch.randn(N, 2 * H, 2 * W, C, generator=g).to(BF)
    gd = go.to(dev())
    dx = Box(N * H * W * C)
    _lib.check(lib.cvk_bilinear_up2_bwd_bf16(gd.data_ptr(), dx.ptr, N, H, W, C, stream()))
    _, vals = dx.settle(True)
    ref = R.bilinear_up2_adjoint(go.double())
    bound = R.bf16_half_ulp(ref) + 40 * U * R.bilinear_up2_adjoint(go.double().abs())
    frac = worst_fraction((vals.view(ref.shape).double() - ref).abs(), bound)
    report("cvk_bilinear_up2_bwd_bf16", "x".join(map(str, shape)), frac)
    assert frac <= 1.0


# ------------------------------------------------------------------------------------------------ 7. zero frame
@pytest.mark.parametrize("name,shape,lay_kw,frame", [
    ("four_sides", (2, 6, 9, 8), {}, (1, 2, 3, 4)),
    ("whole_tensor_inside", (2, 5, 7, 8), {}, (0, 0, 5, 7)),
    ("empty_inside", (1, 4, 6, 16), {}, (0, 0, 0, 6)),
    ("channel_slice", (2, 5, 6, 4), {"ld": 16, "c0": 4}, (2, 1, 2, 3)),
])
def test_zero_frame_bf16(name, shape, lay_kw, frame):
    """cvk_zero_frame_bf16: +0 bits outside the window [y0, y0+h) x [x0, x0+w) of the view, the window itself and every other channel
    of the buffer untouched (they keep the sentinel the buffer was filled with)."""
    _lib, lib = libs()
    N, H, W, C = shape
    y0, x0, h, w = frame
    lay = Lay(shape, **lay_kw)
    buf = Box(lay.numel)
    _lib.check(lib.cvk_zero_frame_bf16(lay.view(buf.ptr, buf.esize), N, H, W, C, y0, x0, h, w, stream()))
    written = torch.zeros(lay.shape, dtype=torch.bool)
    lay.window(written)[...] = True
    lay.window(written)[:, y0:y0 + h, x0:x0 + w] = False
    bits, _ = buf.settle(written)
    assert bool((bits[written.reshape(-1)] == 0).all())
    assert int(written.sum()) == N * (H * W - h * w) * C


# ------------------------------------------------------------------------------------------------ 8. pool scatter with accumulation
def test_maxpool2x2_bwd_bf16_accumulates_with_one_rounding():
    """cvk_maxpool2x2_bwd_bf16 with accumulate = 1 into a channel slice of a wider buffer, odd sizes: bitwise
    rne_bf16(base.float() + scatter.float()) — the fp32 sum of two bf16 values is exact, so one rounding.  The activations are
    coarse post-ReLU values (ties inside a cell, dead cells): the first-maximum rule decides."""
    _lib, lib = libs()
    shape = (2, 5, 7, 16)
    N, H, W, C = shape
    g = torch.Generator().manual_seed(8)
    x = (torch.randint(-2, 4, shape, generator=g).float() * 0.5).clamp_min(0.0).to(BF)
    v = torch.randn(N, H // 2, W // 2, C, generator=g).to(BF)
    base = torch.randn(shape, generator=g).to(BF)
    lay = Lay(shape, ld=32, c0=16)
    xd = lay.embed(x).to(dev())
    vd = v.to(dev())
    dx = Box(lay.numel)
    dx.body().view(lay.shape)[..., 16:32] = base.to(dev())
    _lib.check(lib.cvk_maxpool2x2_bwd_bf16(vd.data_ptr(), lay.view(xd.data_ptr(), 2), lay.view(dx.ptr, 2), 1, N, H, W, C, stream()))
    bits, _ = dx.settle(lay.mask())
    scatter = R.pool2x2_scatter(v.float(), x.float())
    assert bool((scatter[:, H - 1] == 0).all()) and bool((scatter[:, :, W - 1] == 0).all())      # odd trailing row / column: no cell
    want = R.rne_bf16(base.float() + scatter)
    assert torch.equal(lay.window(bits).contiguous(), want.view(torch.int16))
