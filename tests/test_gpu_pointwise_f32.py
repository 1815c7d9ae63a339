"""The fp32 pool, unpool, bilinear x2, import / export and zero-frame passes of csrc/pointwise.hip called directly through the C ABI,
each dispatch arm by a named case, against the references of tests/pointwise_f32_ref.py (whose own correctness, and that the bounds
below are not too tight, tests/test_pointwise_f32_ref_cpu.py checks without a GPU).  Buffers, views and case seeds are those of
tests/test_gpu_elem_bf16.py.

Conventions of every test:
  * inputs come from seeded generators (case_seed(name)); pool inputs are coarse post-ReLU values (multiples of 0.5, clamped at 0), so
    cells hold ties and dead cells and the first-maximum rule decides;
  * every output lives in a buffer with a guard of 64 elements before and after it, pre-filled with the fp32 NaN pattern 0x7FC00001
    (0xEE for the arg-max bytes, -7 for indices).  After the call every element the contract does not write (guards, the other
    channels of a wider buffer, the frame round a spatial window, the float in front of a misaligned tensor) must still hold exactly
    those bits, and every element it does write must be finite (the one NaN case of the pool forward excepted);
  * a strided input holds NaN everywhere outside its view: a read of it would surface in the output;
  * the scalar arms are reached by C % 4 != 0, by a stride that is no multiple of 4, or by a tensor that starts one float past a
    16-byte boundary INSIDE its own allocation (Buf(off=1)); no call gets a pointer its contract forbids.

Tolerances.  Pool, unpool, code-to-index, import, export and zero frame do no arithmetic: compared bitwise (with accumulate = 1: one
fp32 addition, done in float32 on the host).  Bilinear, u = 2^-24, derived in pointwise_f32_ref.bilinear_fwd_bound / _bwd_bound:
      forward    8 max(H,W) u max|x| + u |ref|
      backward   40u sum|w g| + 4 max(H,W) u sum|g| over the pixel's 6x6 candidate window
against exact fp64 taps.  No two arms are compared with each other: the compiler may contract a*b + c differently per instantiation
and the walk sums in another order than the gather; every arm answers to the fp64 bound alone.

Dispatch arms against cases (instantiations read off the dispatch code at the end of pointwise.hip):
  k_maxpool_fwd<4>          POOL v4_dense, v4_odd, v4_one_cell, v4_c64_tall, v4_slice, v4_window, v4_nan, v4_signed_zero (x aligned,
                            strides % 4 == 0, C % 4 == 0), each with and without `code`
  k_maxpool_fwd<1>          POOL v1_c6 (C % 4), v1_by_alignment (x one float off), v1_by_stride (ld = 10)
  k_pool_scatter<4,0>       the v4_* cases through cvk_maxpool2x2_bwd without `code`, accumulate 0 and 1
  k_pool_scatter<4,1>       the same with `code` (x is a null view then: never read); UNPOOL v4_* through cvk_maxunpool2x2_fwd
  k_pool_scatter<1,0>/<1,1> POOL v1_* (dx laid out like x: C % 4, one float off, ld = 10); UNPOOL v1_c6, v1_by_alignment
  k_unpool_bwd<1>, k_code_to_index   every UNPOOL case (one instantiation each)
  k_import_small            IMPORT small_* (C <= 4, ld == 4, dst aligned)      k_import_generic   IMPORT the same one float off, c5_ld8
  k_export_generic, k_zero_frame     one instantiation each: test_export_nchw_*, test_zero_frame_*
  k_bilinear_fwd_tiled      FWD C in {64, 128} at (2,2), (3,17), (5,33), (9,16): C % 64 == 0, H, W >= 2
  k_bilinear_fwd<4>         FWD C = 8 at (1,1), (1,5), (5,1), (3,7); C = 64 at (1,5) (H == 1 keeps it off the tiled arm)
  k_bilinear_fwd<1>         FWD C = 6, and C = 8 with x and out one float off, at (3,7), (1,1)
  k_bilinear_bwd<4>         BWD (2,1,1,8), (1,1,9,64): vector layout, H == 1
  k_bilinear_bwd<1>         BWD (2,3,7,6), (1,1,1,3)
  k_bilinear_bwd_walk<4>    BWD (1,2,2,8): one strip of RS = H = 2.  (2,5,7,64): RS 4, strips of 4 and 1 rows.  (3,9,40,64): 640 work items
                            per row = 3 column blocks (gx), strips 4 + 4 + 1, 27 workgroups (no multiple of 8: the XCD remap's ragged
                            tail).  (1,13,16,128): gx 2, strips 4 + 4 + 4 + 1.  (2,22,128,2048): N W C/4 = 131072 columns, so
                            ceil(400000 / 131072) = 4 strips wanted, RS = 22 / 4 = 5, strips 5 + 5 + 5 + 5 + 2
  (cvk_maxpool2x2_bwd_bnred has its own test in tests/test_gpu_blocks.py.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pointwise_f32_ref as P
from tests import test_gpu_elem_bf16 as G
from tests.test_gpu_bn_f32 import IBox, SENT8
from tests.test_gpu_elem_bf16 import Box, Lay, case_seed, dev, libs, stream, worst_fraction

pytestmark = pytest.mark.gpu
U = P.U32
GUARD = G.GUARD
SENT32 = G.SENT32
SENT64 = -7
NAN = float("nan")
WINDOW = {"ph": 3, "pw": 4, "y0": 1, "x0": 2}


def report(entry, case, frac):
    print(f"[pointwise_f32] {entry} {case}: largest error = {frac:.3f} of its bound")


# ------------------------------------------------------------------------------------------------ shared: buffers
class Buf:
    """An fp32 buffer of a Lay's shape that starts `off` floats past a 16-byte boundary inside a Box: sentinel bits everywhere, or
    the bits of `fill` (a host float tensor of the buffer's shape).  The `off` floats in front belong to nobody."""

    def __init__(self, lay, off=0, fill=None):
        self.lay, self.off = lay, off
        self.box = Box(off + lay.numel, f32=True)
        self.ptr = self.box.ptr + 4 * off
        if fill is not None:
            self.box.raw[GUARD + off:GUARD + off + lay.numel] = fill.reshape(-1).view(torch.int32).to(dev())

    def view(self):
        _lib, _ = libs()
        return _lib.View(self.ptr + 4 * self.lay.offset, *self.lay.strides)

    def put(self, values):
        """write host values [N,H,W,C] into the view"""
        b = self.box.body()[self.off:self.off + self.lay.numel]
        self.lay.window(b)[...] = values.to(dev())

    def settle(self, written=None, finite=True):
        """(bits, values) of the view as host [N,H,W,C] tensors after Box.settle: only `written` (a bool mask of the buffer's shape;
        default: the whole view) may have changed"""
        m = self.lay.mask() if written is None else written.reshape(-1)
        bits, vals = self.box.settle(torch.cat([torch.zeros(self.off, dtype=torch.bool), m]), finite=finite)
        return self.lay.window(bits[self.off:]).contiguous(), self.lay.window(vals[self.off:]).contiguous()

    def snapshot(self):
        torch.cuda.synchronize()
        return self.box.raw.cpu()


def null_view():
    _lib, _ = libs()
    return _lib.View(None, 0, 0, 0)


def bits_of(t):
    return t.contiguous().view(torch.int32)


def vector_width(C, lay, off):
    return 4 if C % 4 == 0 and off == 0 and lay.offset % 4 == 0 and all(s % 4 == 0 for s in lay.strides) else 1


# ------------------------------------------------------------------------------------------------ 1. max pool
# name: (N,H,W,C), layout of x (and of dx), floats past a 16-byte boundary, planted values, V
POOL_CASES = {
    "v4_dense": ((2, 4, 6, 8), {}, 0, None, 4),
    "v4_odd": ((1, 5, 7, 16), {}, 0, None, 4),                       # odd in both directions
    "v4_one_cell": ((2, 2, 2, 4), {}, 0, None, 4),
    "v4_c64_tall": ((1, 9, 3, 64), {}, 0, None, 4),
    "v1_c6": ((2, 5, 7, 6), {}, 0, None, 1),                         # C % 4 != 0
    "v1_by_alignment": ((1, 4, 6, 8), {}, 1, None, 1),
    "v4_slice": ((2, 5, 7, 16), {"ld": 32, "c0": 16}, 0, None, 4),   # channel slice of a wider buffer
    "v4_window": ((2, 5, 7, 16), WINDOW, 0, None, 4),                # spatial window: sY != W * sX
    "v1_by_stride": ((2, 5, 7, 8), {"ld": 10}, 0, None, 1),
    "v4_nan": ((2, 4, 6, 8), {}, 0, "nan", 4),
    "v4_signed_zero": ((2, 4, 6, 8), {}, 0, "signed_zero", 4),
}


def pool_case(name):
    """(x [N,H,W,C] host fp32, Lay, off).  Planted in cell (0,0) of image 0 — "nan": a NaN at position 0, 1, 3 in channels 0, 1, 3 and
    at positions 0 AND 2 in channel 2 (the later one is taken); "signed_zero": an all-zero cell that starts with +0.0 and goes on
    with -0.0 in channel 0 and the reverse in channel 1 (equal values: position 0 wins and its sign bit is what comes out)."""
    shape, lay_kw, off, plant, V = POOL_CASES[name]
    g = torch.Generator().manual_seed(case_seed(name))
    x = (torch.randint(-2, 4, shape, generator=g).float() * 0.5).clamp_min(0.0)
    if plant == "nan":
        x[0, 0, 0, 0] = NAN
        x[0, 0, 1, 1] = NAN
        x[0, 0, 0, 2] = NAN
        x[0, 1, 0, 2] = NAN
        x[0, 1, 1, 3] = NAN
    if plant == "signed_zero":
        x[0, :2, :2, 0] = -0.0
        x[0, 0, 0, 0] = 0.0
        x[0, :2, :2, 1] = 0.0
        x[0, 0, 0, 1] = -0.0
    lay = Lay(shape, **lay_kw)
    assert V == vector_width(shape[3], lay, off)
    return x, lay, off


@pytest.mark.parametrize("with_code", [1, 0])
@pytest.mark.parametrize("name", list(POOL_CASES))
def test_maxpool2x2_fwd(name, with_code):
    """cvk_maxpool2x2_fwd: the pooled tensor is bitwise the coded element of its cell (so the sign of a zero and a NaN come through),
    the code is the first maximum in scan order with ATen's NaN rule; with code == NULL the same pooled tensor.  x is a strided view
    with NaN all round it and is not modified."""
    _lib, lib = libs()
    x, lay, off = pool_case(name)
    N, H, W, C = x.shape
    n = N * (H // 2) * (W // 2) * C
    xb = Buf(lay, off, fill=lay.embed(x))
    before = xb.snapshot()
    out = Box(n, f32=True)
    code = IBox(n, torch.uint8, SENT8) if with_code else None
    _lib.check(lib.cvk_maxpool2x2_fwd(xb.view(), out.ptr, code.ptr if with_code else None, N, H, W, C, stream()))
    want, wcode = P.pool_code(x)
    bits, _ = out.settle(True, finite=POOL_CASES[name][3] != "nan")
    assert torch.equal(bits, bits_of(want).reshape(-1))
    if with_code:
        assert torch.equal(code.settle(), wcode.reshape(-1))
    assert torch.equal(xb.snapshot(), before)
    assert len(torch.unique(wcode)) == 4 or n < 64                               # ties and all four positions are really in there
    if POOL_CASES[name][3] == "nan":
        assert wcode[0, 0, 0, :4].tolist() == [0, 1, 2, 3] and bool(torch.isnan(want[0, 0, 0, :4]).all())
    if POOL_CASES[name][3] == "signed_zero":
        assert wcode[0, 0, 0, :2].tolist() == [0, 0] and bits_of(want)[0, 0, 0, :2].tolist() == [0, -2 ** 31]


@pytest.mark.parametrize("name", list(POOL_CASES))
def test_maxpool2x2_bwd(name):
    """cvk_maxpool2x2_bwd into a dx laid out like x, with the code (x a null view then) and without (arg-max recomputed from x), with
    accumulate 0 and 1.  Without accumulate the whole view is written: dout at the coded pixel, +0 bits elsewhere, an odd trailing row
    / column included.  With it: bitwise base + scatter in float32, and the odd trailing row / column keeps its bits."""
    _lib, lib = libs()
    x, lay, off = pool_case(name)
    N, H, W, C = x.shape
    g = torch.Generator().manual_seed(case_seed(name) + 1)
    dout = torch.randn(N, H // 2, W // 2, C, generator=g)
    base = torch.randn(N, H, W, C, generator=g)
    _, wcode = P.pool_code(x)
    scatter = P.unpool_fwd(dout, wcode, H, W)
    xb = Buf(lay, off, fill=lay.embed(x))
    dd, cd = dout.to(dev()), wcode.to(dev())
    for use_code in (1, 0):
        for acc in (0, 1):
            dxb = Buf(lay, off)
            if acc:
                dxb.put(base)
            _lib.check(lib.cvk_maxpool2x2_bwd(dd.data_ptr(), null_view() if use_code else xb.view(), cd.data_ptr() if use_code else None,
                                              dxb.view(), acc, N, H, W, C, stream()))
            bits, _ = dxb.settle()
            want = base + scatter if acc else scatter
            assert torch.equal(bits, bits_of(want)), (name, use_code, acc, int((bits != bits_of(want)).sum()))
            if acc:
                assert torch.equal(bits[:, 2 * (H // 2):], bits_of(base[:, 2 * (H // 2):]))
                assert torch.equal(bits[:, :, 2 * (W // 2):], bits_of(base[:, :, 2 * (W // 2):]))
            else:
                assert bool((bits[:, 2 * (H // 2):] == 0).all()) and bool((bits[:, :, 2 * (W // 2):] == 0).all())


def test_pool_entry_points_refuse_what_they_cannot_do():
    """H < 2 for the pool forward, a backward with neither code nor x, an unpool without code: a non-zero return, no launch (every
    buffer keeps its sentinel)."""
    _lib, lib = libs()
    lay = Lay((1, 1, 4, 4))
    xb = Buf(lay, fill=torch.ones(lay.shape))
    out, dxb = Box(16, f32=True), Buf(Lay((1, 2, 4, 4)))
    assert lib.cvk_maxpool2x2_fwd(xb.view(), out.ptr, None, 1, 1, 4, 4, stream()) != 0
    assert "cvk_maxpool2x2_fwd" in lib.cvk_last_error_string().decode()
    assert lib.cvk_maxpool2x2_bwd(xb.ptr, null_view(), None, dxb.view(), 0, 1, 2, 4, 4, stream()) != 0
    assert "cvk_maxpool2x2_bwd" in lib.cvk_last_error_string().decode()
    assert lib.cvk_maxunpool2x2_fwd(xb.ptr, None, out.ptr, 1, 2, 4, 4, stream()) != 0
    out.settle(torch.zeros(16, dtype=torch.bool), finite=False)
    dxb.settle(torch.zeros(dxb.lay.numel, dtype=torch.bool), finite=False)


# ------------------------------------------------------------------------------------------------ 2. unpool, code to index
# name: (N,H,W,C), floats `out` lies past a 16-byte boundary, V
UNPOOL_CASES = {
    "v4_dense": ((2, 4, 6, 8), 0, 4),
    "v4_odd": ((1, 5, 7, 16), 0, 4),
    "v4_one_cell": ((2, 2, 2, 4), 0, 4),
    "v4_c64_tall": ((1, 9, 3, 64), 0, 4),
    "v1_c6": ((2, 5, 7, 6), 0, 1),
    "v1_by_alignment": ((1, 4, 6, 8), 1, 1),
}


@pytest.mark.parametrize("name", list(UNPOOL_CASES))
def test_unpool_and_indices(name):
    """cvk_maxunpool2x2_fwd writes all of out: v at the coded pixel, +0 bits elsewhere (odd trailing row / column too);
    cvk_maxunpool2x2_bwd of that out returns v bitwise, and of a random gradient the coded pixels; cvk_pool_code_to_index equals
    torch's max_pool2d indices exactly.  The code is the reference's, from a coarse x with ties."""
    _lib, lib = libs()
    shape, off, V = UNPOOL_CASES[name]
    N, H, W, C = shape
    assert V == vector_width(C, Lay(shape), off)
    Ho, Wo = H // 2, W // 2
    g = torch.Generator().manual_seed(case_seed(name) + 2)
    x = (torch.randint(-2, 4, shape, generator=g).float() * 0.5).clamp_min(0.0)
    v = torch.randn(N, Ho, Wo, C, generator=g)
    r = torch.randn(N, H, W, C, generator=g)
    _, wcode = P.pool_code(x)
    vd, cd, rd = v.to(dev()), wcode.to(dev()), r.to(dev())
    out = Buf(Lay(shape), off)
    _lib.check(lib.cvk_maxunpool2x2_fwd(vd.data_ptr(), cd.data_ptr(), out.ptr, N, H, W, C, stream()))
    bits, _ = out.settle()
    assert torch.equal(bits, bits_of(P.unpool_fwd(v, wcode, H, W)))
    for grad, want in ((out.ptr, v), (rd.data_ptr(), P.unpool_bwd(r, wcode))):
        dv = Box(N * Ho * Wo * C, f32=True)
        _lib.check(lib.cvk_maxunpool2x2_bwd(grad, cd.data_ptr(), dv.ptr, N, H, W, C, stream()))
        assert torch.equal(dv.settle(True)[0], bits_of(want).reshape(-1))
    idx = IBox(N * C * Ho * Wo, torch.int64, SENT64)
    _lib.check(lib.cvk_pool_code_to_index(cd.data_ptr(), idx.ptr, N, H, W, C, stream()))
    got = idx.settle().view(N, C, Ho, Wo)
    assert torch.equal(got, F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2, return_indices=True)[1])
    assert torch.equal(got, P.pool_index(wcode, W))


# ------------------------------------------------------------------------------------------------ 3. import, export, zero frame
# name: (N,C,H,W), ld, floats dst lies past a 16-byte boundary
IMPORT_CASES = {
    "small_c3": ((2, 3, 5, 7), 4, 0),                                # k_import_small
    "small_c3_off1": ((2, 3, 5, 7), 4, 1),                           # the same through k_import_generic
    "small_c4": ((1, 4, 3, 2), 4, 0),
    "c5_ld8": ((2, 5, 3, 5), 8, 0),
}


@pytest.mark.parametrize("name", list(IMPORT_CASES))
def test_import_nchw_from_a_crop(name):
    """cvk_import_nchw from a non-contiguous source (the interior of a larger NCHW tensor, NaN round it) to [N,H,W,ld]: bitwise the
    source in channels < C, +0 bits in the pad channels; k_import_small and k_import_generic answer to the same reference."""
    _lib, lib = libs()
    (N, C, H, W), ld, off = IMPORT_CASES[name]
    g = torch.Generator().manual_seed(case_seed(name))
    vals = torch.randn(N, C, H, W, generator=g)
    big = torch.full((N, C, H + 2, W + 3), NAN)
    big[:, :, 1:-1, 2:-1] = vals
    src = big.to(dev())[:, :, 1:-1, 2:-1]
    assert not src.is_contiguous()
    out = Buf(Lay((N, H, W, ld)), off)
    _lib.check(lib.cvk_import_nchw(src.data_ptr(), *src.stride(), out.ptr, ld, N, C, H, W, stream()))
    bits, _ = out.settle()
    assert np.array_equal(bits.numpy(), P.import_nchw_ref(bits_of(vals).numpy(), ld))


@pytest.mark.parametrize("C,ld", [(3, 4), (5, 8), (12, 12)])
def test_export_nchw_into_a_slice(C, ld):
    """cvk_export_nchw from [N,H,W,ld] (NaN pads) into the interior of a larger NCHW tensor whose surroundings keep the sentinel."""
    _lib, lib = libs()
    N, H, W = 2, 5, 7
    g = torch.Generator().manual_seed(10 * C + ld)
    src = torch.full((N, H, W, ld), NAN)
    src[..., :C] = torch.randn(N, H, W, C, generator=g)
    sd = src.to(dev())
    shape = (N, C + 2, H + 2, W + 3)
    box = Box(int(np.prod(shape)), f32=True)
    dst = box.body().view(shape)[:, 1:C + 1, 1:-1, 2:-1]
    _lib.check(lib.cvk_export_nchw(sd.data_ptr(), ld, dst.data_ptr(), *dst.stride(), N, C, H, W, stream()))
    written = torch.zeros(shape, dtype=torch.bool)
    written[:, 1:C + 1, 1:-1, 2:-1] = True
    bits, _ = box.settle(written)
    got = bits.view(shape)[:, 1:C + 1, 1:-1, 2:-1]
    assert np.array_equal(got.numpy(), P.export_nchw_ref(bits_of(src).numpy(), C))


@pytest.mark.parametrize("lay_kw", [{}, dict(WINDOW, ld=16, c0=4)], ids=["dense", "window_slice"])
def test_zero_frame_of_a_view(lay_kw):
    """cvk_zero_frame on a dense view and on a spatial window of a channel slice: +0 bits outside [y0, y0+h) x [x0, x0+w) of the
    view; the window, the other channels and the surrounding pixels keep the sentinel."""
    _lib, lib = libs()
    shape, (y0, x0, h, w) = (2, 5, 7, 8), (1, 2, 3, 4)
    N, H, W, C = shape
    lay = Lay(shape, **lay_kw)
    buf = Buf(lay)
    _lib.check(lib.cvk_zero_frame(buf.view(), N, H, W, C, y0, x0, h, w, stream()))
    written = torch.zeros(lay.shape, dtype=torch.bool)
    lay.window(written)[...] = True
    lay.window(written)[:, y0:y0 + h, x0:x0 + w] = False
    bits, _ = buf.settle(written)
    want = P.zero_frame_ref(np.full(shape, SENT32, dtype=np.int32), C, y0, x0, h, w)
    assert np.array_equal(bits.numpy(), want)


# ------------------------------------------------------------------------------------------------ 4. bilinear x2
# (C, (H, W), floats x and out lie past a 16-byte boundary); N = 2
BILINEAR_FWD = [(C, hw, 0) for C in (64, 128) for hw in ((2, 2), (3, 17), (5, 33), (9, 16))] + \
               [(8, hw, 0) for hw in ((1, 1), (1, 5), (5, 1), (3, 7))] + [(64, (1, 5), 0)] + \
               [(C, hw, off) for C, off in ((6, 0), (8, 1)) for hw in ((3, 7), (1, 1))]
# (N, H, W, C)
BILINEAR_BWD = [(2, 1, 1, 8), (1, 1, 9, 64), (2, 3, 7, 6), (1, 1, 1, 3), (1, 2, 2, 8), (2, 5, 7, 64), (3, 9, 40, 64), (1, 13, 16, 128)]
BILINEAR_BWD_LARGE = (2, 22, 128, 2048)


def bilinear_fwd_input(C, hw):
    g = torch.Generator().manual_seed(1000 * C + 37 * hw[0] + hw[1])
    return torch.randn(2, hw[0], hw[1], C, generator=g)


def bilinear_bwd_input(shape):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    return torch.randn(N, 2 * H, 2 * W, C, generator=g)


@pytest.mark.parametrize("C,hw,off", BILINEAR_FWD, ids=[f"C{C}_{hw[0]}x{hw[1]}" + "_off1" * off for C, hw, off in BILINEAR_FWD])
def test_bilinear_up2_fwd(C, hw, off):
    """cvk_bilinear_up2_fwd: the tiled arm (ragged 4 x 32 tiles both ways, a second tile column at W = 17 and 33, the staging clamp at
    the border, two channel chunks at C = 128), the flat four-wide one (one row, one column, one pixel) and the scalar one.
    Bound: 8 max(H,W) u max|x| + u |ref|."""
    _lib, lib = libs()
    x = bilinear_fwd_input(C, hw)
    N, H, W, _ = x.shape
    xb = Buf(Lay(tuple(x.shape)), off, fill=x)
    out = Buf(Lay((N, 2 * H, 2 * W, C)), off)
    _lib.check(lib.cvk_bilinear_up2_fwd(xb.ptr, out.ptr, N, H, W, C, stream()))
    _, vals = out.settle()
    ref = P.bilinear_up2(x.double())
    frac = worst_fraction((vals.double() - ref).abs(), P.bilinear_fwd_bound(x.double(), ref))
    report("cvk_bilinear_up2_fwd", f"C={C} {H}x{W} off={off}", frac)
    assert frac <= 1.0


@pytest.mark.parametrize("shape", BILINEAR_BWD, ids=["x".join(map(str, s)) for s in BILINEAR_BWD])
def test_bilinear_up2_bwd(shape):
    """cvk_bilinear_up2_bwd: the 6 x 6 gather four-wide (H == 1) and scalar, and the separable walk with one strip, with a ragged
    last strip, with three column blocks per row and a workgroup count that is no multiple of 8 (module docstring).
    Bound: 40u sum|w g| + 4 max(H,W) u sum_window|g|."""
    _lib, lib = libs()
    N, H, W, C = shape
    go = bilinear_bwd_input(shape)
    gd = go.to(dev())
    dx = Box(N * H * W * C, f32=True)
    _lib.check(lib.cvk_bilinear_up2_bwd(gd.data_ptr(), dx.ptr, N, H, W, C, stream()))
    _, vals = dx.settle(True)
    ref = P.bilinear_up2_adjoint(go.double())
    frac = worst_fraction((vals.view(ref.shape).double() - ref).abs(), P.bilinear_bwd_bound(go.double(), H, W))
    report("cvk_bilinear_up2_bwd", "x".join(map(str, shape)), frac)
    assert frac <= 1.0


def test_bilinear_up2_bwd_scalar_by_alignment():
    """k_bilinear_bwd<1> by a dx one float off a 16-byte boundary, at a shape the walk would take otherwise."""
    _lib, lib = libs()
    shape = (2, 3, 7, 8)
    N, H, W, C = shape
    go = bilinear_bwd_input(shape)
    gd = go.to(dev())
    dx = Buf(Lay(shape), 1)
    _lib.check(lib.cvk_bilinear_up2_bwd(gd.data_ptr(), dx.ptr, N, H, W, C, stream()))
    _, vals = dx.settle()
    ref = P.bilinear_up2_adjoint(go.double())
    frac = worst_fraction((vals.double() - ref).abs(), P.bilinear_bwd_bound(go.double(), H, W))
    report("cvk_bilinear_up2_bwd", "x".join(map(str, shape)) + " off=1", frac)
    assert frac <= 1.0


def test_bilinear_up2_bwd_walk_with_strips_of_five_rows():
    """[2,22,128,2048]: the one size class at which the walk's strips are higher than four rows (131072 columns -> 4 strips wanted ->
    RS = 5, five strips, the last of two rows).  46 M gradient floats: generated on the device, and the fp64 reference and bound
    computed there with the same plain expressions, 128 channels at a time."""
    _lib, lib = libs()
    N, H, W, C = BILINEAR_BWD_LARGE
    g = torch.Generator(device=dev()).manual_seed(sum(BILINEAR_BWD_LARGE))
    go = torch.randn(N, 2 * H, 2 * W, C, generator=g, device=dev())
    dx = Box(N * H * W * C, f32=True)
    _lib.check(lib.cvk_bilinear_up2_bwd(go.data_ptr(), dx.ptr, N, H, W, C, stream()))
    torch.cuda.synchronize()
    assert dx.guards_intact()
    got_all = dx.body().view(N, H, W, C)
    frac = 0.0
    for c0 in range(0, C, 128):
        g64 = go[..., c0:c0 + 128].double()
        got = got_all[..., c0:c0 + 128].double()
        assert bool(torch.isfinite(got).all())
        frac = max(frac, float(((got - P.bilinear_up2_adjoint(g64)).abs() / P.bilinear_bwd_bound(g64, H, W)).max()))
    report("cvk_bilinear_up2_bwd", "x".join(map(str, BILINEAR_BWD_LARGE)), frac)
    assert frac <= 1.0
