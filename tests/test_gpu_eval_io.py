"""The kernels that bring an image in and turn logits into mIoU, called through the C ABI and compared with the numpy restatements
of tests/eval_io_ref.py (which tests/test_eval_io_ref_cpu.py checks without a GPU): cvk_import_nchw, cvk_export_nchw, cvk_zero_frame
(csrc/pointwise.hip), cvk_preprocess_u8 (csrc/ingest.h), cvk_argmax_channels, cvk_confusion_accumulate (csrc/eval_meters.h; both headers are
compiled as part of loss_eval_optim.hip) and their Python wrappers preprocess_uint8, argmax_channels and ConfusionMeter.

These operations move data or count integers, so every comparison is exact (bit patterns for the float passes); the one exception
is cvk_preprocess_u8 against fp64, under the bound derived in eval_io_ref.preprocess_bound.

Conventions of every test:
  * every output lives between two guards of 64 elements holding a sentinel (fp32: the NaN bit pattern 0x7FC00001, int64: -7), and
    the elements the kernel must write start as the sentinel too.  After the call the guards, and everything else the contract does
    not write, must still hold it; an element left unwritten differs from the reference;
  * float data are random 32-bit patterns with -0.0, signalling and quiet NaNs with payloads, denormals and both infinities planted:
    a pass that moves data must return them bit for bit, and a pad must be the bit pattern 0, not -0.0 and not 0 * x;
  * input pad columns (ld > C) hold NaN or +inf, so a read of them surfaces in the output."""
import ctypes

import numpy as np
import pytest
import torch

from tests import eval_io_ref as R

pytestmark = pytest.mark.gpu
GUARD = 64
SENT32 = 0x7FC00001                   # a quiet NaN no kernel here produces
PADNAN = 0x7FC00002                   # another one, for input pads: it must never reach an output
SENT64 = -7
SPECIAL_BITS = np.array([0x80000000, 0x7F800001, 0xFFC12345, 0x7FC00000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x00000000],
                        dtype=np.uint32).view(np.int32)        # -0.0, sNaN, -qNaN+payload, qNaN, +-denormal, +-inf, +0.0
GRID_CAP = 16384 * 256                # elements one sweep of pointwise.hip's capped grid covers
SECOND_MEAN_STD = ((0.5, -0.25, 0.9), (0.05, 0.05, 2.0))


def dev():
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def libs():
    from pytorch_camvid_amd import _lib
    return _lib, _lib.load()


def pkg():
    import pytorch_camvid_amd as A
    return A


class Box:
    """n elements of device memory (fp32 bit patterns as int32, or int64) between two guards, everything pre-filled with the sentinel."""

    def __init__(self, n, i64=False):
        self.n = n
        self.sent = SENT64 if i64 else SENT32
        self.raw = torch.full((GUARD + n + GUARD,), self.sent, dtype=torch.int64 if i64 else torch.int32, device=dev())
        self.ptr = self.raw.data_ptr() + GUARD * self.raw.element_size()
        assert self.ptr % 16 == 0

    def body(self):
        return self.raw[GUARD:GUARD + self.n]

    def host(self):
        """numpy copy of the n elements, after checking the guards"""
        torch.cuda.synchronize()
        h = self.raw.cpu().numpy()
        assert (h[:GUARD] == self.sent).all() and (h[GUARD + self.n:] == self.sent).all(), "a guard was overwritten"
        return h[GUARD:GUARD + self.n].copy()


def random_bits(shape, seed):
    """int32 host tensor of random bit patterns; about three elements in ten hold one of SPECIAL_BITS, in turn."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-2 ** 31, 2 ** 31, tuple(shape), generator=g, dtype=torch.int64).to(torch.int32)
    flat = t.reshape(-1)
    at = torch.nonzero(torch.rand(flat.numel(), generator=g) < 0.3).reshape(-1)
    flat[at] = torch.from_numpy(SPECIAL_BITS.copy())[torch.arange(at.numel()) % len(SPECIAL_BITS)]
    return t


# name: (N,C,H,W) -> (shape of the buffer, the logical [N,C,H,W] view of it)
SRC_LAYOUTS = {
    "contiguous": lambda N, C, H, W: ((N, C, H, W), lambda b: b),
    "channels_last": lambda N, C, H, W: ((N, H, W, C), lambda b: b.permute(0, 3, 1, 2)),
    "crop": lambda N, C, H, W: ((N, C, H + 2, W + 5), lambda b: b[:, :, 1:-1, 2:-3]),
    "channel_step2": lambda N, C, H, W: ((N, 2 * C, H, W), lambda b: b[:, ::2]),
    "expand_n": lambda N, C, H, W: ((1, C, H, W), lambda b: b.expand(N, -1, -1, -1)),
    "expand_c": lambda N, C, H, W: ((N, 1, H, W), lambda b: b.expand(-1, C, -1, -1)),
}
DST_LAYOUTS = {
    "contiguous": lambda N, C, H, W: ((N, C, H, W), lambda b: b),
    "channels_last": lambda N, C, H, W: ((N, H, W, C), lambda b: b.permute(0, 3, 1, 2)),
    "slice": lambda N, C, H, W: ((N, C + 3, H + 2, W + 4), lambda b: b[:, 1:C + 1, 1:-1, 3:-1]),
}
SIZES = ((1, 1, 1), (2, 5, 7), (3, 9, 11))


# ------------------------------------------------------------------------------------------------ cvk_import_nchw
def run_import(N, C, H, W, ld, layout, seed, dst_offset=0):
    """One call: source bits in `layout` -> dst (dst_offset floats past a 16-byte boundary), compared with import_nchw_ref."""
    _lib, lib = libs()
    shape, view = SRC_LAYOUTS[layout](N, C, H, W)
    base = random_bits(shape, seed)
    base_d = base.to(dev()).view(torch.float32)
    src = view(base_d)
    assert tuple(src.shape) == (N, C, H, W)
    n = N * H * W * ld
    out = Box(dst_offset + n)
    _lib.check(lib.cvk_import_nchw(src.data_ptr(), *src.stride(), out.ptr + 4 * dst_offset, ld, N, C, H, W, stream()))
    got = out.host()
    assert (got[:dst_offset] == SENT32).all(), "an element before dst was written"
    want = R.import_nchw_ref(view(base).numpy(), ld)
    got = got[dst_offset:].reshape(N, H, W, ld)
    assert (got[..., C:] == 0).all(), "a pad channel is not +0.0"
    assert np.array_equal(got, want), (layout, (N, C, H, W), ld, int((got != want).sum()))


@pytest.mark.parametrize("C,ld,offset", [(3, 4, 0), (3, 4, 1), (1, 4, 0), (4, 4, 0), (5, 8, 0), (12, 12, 0), (64, 64, 0)])
def test_import_nchw_bitwise_for_every_source_layout(C, ld, offset):
    """cvk_import_nchw == import_nchw_ref bit for bit, pads exactly +0.0, for every source layout and size.  C <= 4 with ld = 4 takes
    k_import_small; the same case with dst 4 bytes past a 16-byte boundary, and every other case, k_import_generic.
    Written against: a stride swapped or dropped in the source address (sH for sW, the channel stride taken as H*W: the crop,
    step-2 and expanded sources), `c < ld` instead of `c < C` in the pad test or a pad written as v[C-1], walking C where ld is
    meant in the destination index, 16-byte stores at a misaligned dst."""
    for li, layout in enumerate(SRC_LAYOUTS):
        for si, (N, H, W) in enumerate(SIZES):
            run_import(N, C, H, W, ld, layout, seed=100 * C + 10 * li + si, dst_offset=offset)


@pytest.mark.parametrize("N,C,H,W,offset", [(2, 3, 1100, 1000, 0), (2, 3, 1100, 1000, 1), (1, 1, 2049, 2049, 0)])
def test_import_nchw_past_the_grid_cap(N, C, H, W, offset):
    """The grid-stride loops: 2x3x1100x1000 with ld = 4 is 8.8M elements, more than twice what k_import_generic's capped grid covers
    in one sweep (the dst offset selects that kernel; aligned, k_import_small makes one sweep of 2.2M pixels); 1x1x2049x2049 is one
    row and a bit more than a sweep of k_import_small.  Written against: a stride of the loop that is not the grid's size, a 32-bit
    element index."""
    assert N * H * W * 4 > GRID_CAP and (offset == 0 or N * H * W * 4 > 2 * GRID_CAP) and (C != 1 or N * H * W > GRID_CAP)
    run_import(N, C, H, W, 4, "contiguous", seed=7 + offset, dst_offset=offset)


# ------------------------------------------------------------------------------------------------ cvk_export_nchw
def run_export(N, C, H, W, ld, layout, seed, src_bits=None):
    """One call: dense NHWC bits (pads NaN) -> the `layout` view of a sentinel-filled buffer; returns that buffer's host copy after
    comparing all of it (the view with export_nchw_ref, the rest with the sentinel)."""
    _lib, lib = libs()
    if src_bits is None:
        src_bits = random_bits((N, H, W, ld), seed)
        src_bits[..., C:] = PADNAN
    src_d = src_bits.to(dev())
    shape, view = DST_LAYOUTS[layout](N, C, H, W)
    out = Box(int(np.prod(shape)))
    dst = view(out.body().view(torch.float32).view(shape))
    assert tuple(dst.shape) == (N, C, H, W)
    _lib.check(lib.cvk_export_nchw(src_d.data_ptr(), ld, dst.data_ptr(), *dst.stride(), N, C, H, W, stream()))
    got = out.host().reshape(shape)
    want = np.full(shape, SENT32, dtype=np.int32)
    view(torch.from_numpy(want))[...] = torch.from_numpy(R.export_nchw_ref(src_bits.numpy(), C))
    assert np.array_equal(got, want), (layout, (N, C, H, W), ld, int((got != want).sum()))
    return view(torch.from_numpy(got)).numpy()


@pytest.mark.parametrize("C,ld", [(3, 3), (3, 4), (1, 4), (5, 8), (12, 12), (12, 15), (64, 64)])
def test_export_nchw_bitwise_for_every_destination_layout(C, ld):
    """cvk_export_nchw == export_nchw_ref bit for bit into contiguous NCHW, channels_last and a slice of a larger tensor whose
    surroundings (and the guards) keep the sentinel; with ld > C the NaN pads must not arrive anywhere.
    Written against: walking C where ld is meant in the source index (or the reverse), a destination stride swapped or assumed
    dense, one element too many per pixel."""
    for li, layout in enumerate(DST_LAYOUTS):
        for si, (N, H, W) in enumerate(SIZES):
            run_export(N, C, H, W, ld, layout, seed=200 * C + 10 * li + si + ld)


def test_export_nchw_past_the_grid_cap():
    """2x3x1100x1000: 6.6M elements, more than one sweep of the capped grid."""
    assert 2 * 3 * 1100 * 1000 > GRID_CAP
    run_export(2, 3, 1100, 1000, 4, "contiguous", seed=11)


@pytest.mark.parametrize("C,ld", [(3, 4), (5, 8), (12, 12)])
def test_import_then_export_is_the_identity_on_bit_patterns(C, ld):
    """Import (from a cropped source) then export (to channels_last and to a slice) returns every bit pattern: -0.0, NaN payloads,
    signalling NaNs, denormals and both infinities are planted by random_bits.  Written against: any arithmetic on the way
    (x * 1, x + 0, a flushed denormal, a quieted NaN)."""
    _lib, lib = libs()
    N, H, W = 2, 5, 7
    shape, view = SRC_LAYOUTS["crop"](N, C, H, W)
    base = random_bits(shape, 300 + C)
    logical = view(base).numpy()
    for pattern in SPECIAL_BITS:
        assert (logical == pattern).any()
    src = view(base.to(dev()).view(torch.float32))
    mid = Box(N * H * W * ld)
    _lib.check(lib.cvk_import_nchw(src.data_ptr(), *src.stride(), mid.ptr, ld, N, C, H, W, stream()))
    nhwc = torch.from_numpy(mid.host().reshape(N, H, W, ld))
    for layout in ("channels_last", "slice", "contiguous"):
        back = run_export(N, C, H, W, ld, layout, seed=0, src_bits=nhwc)
        assert np.array_equal(back, logical)


# ------------------------------------------------------------------------------------------------ cvk_zero_frame
def frame_bits(shape, seed):
    """random finite values with NaN, +inf and -inf sprinkled in: 0 * x would leave NaN behind"""
    t = random_bits(shape, seed).reshape(-1)
    t[1::5] = int(SPECIAL_BITS[3])
    t[2::7] = int(SPECIAL_BITS[6])
    t[3::11] = int(SPECIAL_BITS[7])
    return t.reshape(shape)


def run_zero_frame(N, H, W, C, win, sliced, seed):
    _lib, lib = libs()
    y0, x0, h, w = win
    ldb, c0 = (2 * C, C) if sliced else (C, 0)
    start = frame_bits((N, H, W, ldb), seed)
    buf = Box(N * H * W * ldb)
    buf.body().copy_(start.reshape(-1))
    v = _lib.View(buf.ptr + 4 * c0, H * W * ldb, W * ldb, ldb)
    _lib.check(lib.cvk_zero_frame(v, N, H, W, C, y0, x0, h, w, stream()))
    got = buf.host().reshape(N, H, W, ldb)
    want = start.numpy().copy()
    want[..., c0:] = R.zero_frame_ref(want[..., c0:], C, y0, x0, h, w)
    assert np.array_equal(got[..., :c0], start.numpy()[..., :c0]), "the other half of the buffer changed"
    assert np.array_equal(got, want), ((N, H, W, C), win, sliced, int((got != want).sum()))


#                y0 x0 h  w     of a 5 x 7 frame
ZERO_WINDOWS = {"interior": (1, 2, 3, 3), "top_left": (0, 0, 2, 3), "bottom_right": (3, 4, 2, 3), "left_edge": (1, 0, 2, 2),
                "right_edge": (1, 5, 3, 2), "top_edge": (0, 2, 2, 3), "bottom_edge": (4, 1, 1, 4), "full": (0, 0, 5, 7),
                "empty_h": (2, 3, 0, 4), "empty_w": (1, 1, 3, 0), "one_row": (2, 0, 1, 7), "one_column": (0, 3, 5, 1),
                "one_pixel": (4, 6, 1, 1)}


@pytest.mark.parametrize("C", [1, 3, 4, 6, 64])
def test_zero_frame_bitwise_for_every_window(C):
    """cvk_zero_frame == zero_frame_ref bit for bit on a 3x5x7 buffer of random values, NaN and inf: +0.0 outside the window, the
    window untouched, for dense views and for the upper channel half of a buffer twice as wide (whose lower half must not change).
    Written against: `y <= y0 + h` or `x <= x0 + w` (one row / column too few zeroed: every window that ends inside the frame),
    `y > y0` (the window's first row zeroed), multiplying by zero instead of storing it, sX taken as C (the sliced view), an
    empty window treated as 'nothing to do'."""
    for wi, (name, win) in enumerate(ZERO_WINDOWS.items()):
        for sliced in (False, True):
            run_zero_frame(3, 5, 7, C, win, sliced, seed=400 + 10 * wi + C)


def test_zero_frame_past_the_grid_cap():
    """3x151x151x64 = 4.4M elements: more than one sweep of the capped grid."""
    assert 3 * 151 * 151 * 64 > GRID_CAP
    run_zero_frame(3, 151, 151, 64, (10, 20, 100, 90), False, seed=13)


# ------------------------------------------------------------------------------------------------ cvk_preprocess_u8
def f3(v):
    return (ctypes.c_float * 3)(*v)


def run_preprocess(u8, mean, std):
    """raw call on uint8 [N,H,W,3] (numpy); checks pad and bound; returns the int32 bits [N,H,W,4]"""
    _lib, lib = libs()
    N, H, W, _ = u8.shape
    src = torch.from_numpy(u8).to(dev())
    out = Box(N * H * W * 4)
    _lib.check(lib.cvk_preprocess_u8(src.data_ptr(), out.ptr, N, H, W, f3(mean), f3(std), stream()))
    bits = out.host().reshape(N, H, W, 4)
    assert (bits[..., 3] == 0).all(), "pad channel 3 is not +0.0"
    got = bits.view(np.float32)[..., :3].astype(np.float64)
    err = np.abs(got - R.preprocess_ref(u8, mean, std))
    bound = R.preprocess_bound(u8, mean, std)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"preprocess {u8.shape} mean {mean[0]:.3f}: worst error / bound = {ratio:.3f}")
    assert not np.isnan(got).any() and (err <= bound).all(), ratio
    return bits


def mean_std_pairs():
    F = pkg().functional
    return ((F.CAMVID_MEAN, F.CAMVID_STD), SECOND_MEAN_STD)


def test_preprocess_all_byte_values_layout_accuracy_and_order():
    """All 256 values in each channel, in a different order per channel: |got - fp64| <= 6 u (v/255 + |mean|)/std elementwise
    (eval_io_ref.preprocess_bound has the derivation), pad channel exactly +0.0, and the output non-decreasing in v per channel.
    Written against: channels swapped or one constant used for all three, pad channel 3 written as v[2], v/256 or a truncated 1/255,
    std multiplied instead of divided, the subtraction after the scaling."""
    img, perms = R.preprocess_all_values()
    for mean, std in mean_std_pairs():
        bits = run_preprocess(img, mean, std)
        vals = bits.view(np.float32).reshape(256, 4)
        for c in range(3):
            by_v = vals[np.argsort(perms[c]), c]
            assert (np.diff(by_v.astype(np.float64)) >= 0).all(), f"channel {c} is not monotonic in v"
            assert by_v[0] < by_v[255]


@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (2, 7, 9), (1, 1449, 1449)])
def test_preprocess_sizes_and_the_python_wrapper(N, H, W):
    """Random images at one pixel, an odd size with a partial block, and 1449 x 1449 = 2,099,601 pixels: one more sweep than the
    8192 x 256 grid covers.  A.preprocess_uint8 returns the bits of the raw call as a logical [N,3,H,W] view with pixel stride 4.
    Written against: a loop stride that is not the grid's size, 3 taken for the destination's pixel stride or 4 for the source's,
    a wrapper that drops or reorders the constants."""
    A = pkg()
    assert (N * H * W > 8192 * 256) == (H == 1449)
    u8 = np.random.default_rng(N * H * W).integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    u8.reshape(-1)[:3] = (0, 255, 128)
    for i, (mean, std) in enumerate(mean_std_pairs()):
        bits = run_preprocess(u8, mean, std)
        for x in [A.preprocess_uint8(torch.from_numpy(u8).to(dev()), mean, std)] + ([A.preprocess_uint8(torch.from_numpy(u8).to(dev()))] if i == 0 else []):
            assert tuple(x.shape) == (N, 3, H, W) and x.dtype == torch.float32
            p = x.permute(0, 2, 3, 1)
            assert p.stride() == (H * W * 4, W * 4, 4, 1) and x.data_ptr() % 16 == 0
            assert np.array_equal(p.contiguous().view(torch.int32).cpu().numpy(), bits[..., :3])


# ------------------------------------------------------------------------------------------------ cvk_argmax_channels
def run_argmax(rows, C):
    """raw call on float32 [M, ld] rows (numpy) -> int64 [M], guards checked"""
    _lib, lib = libs()
    M, ld = rows.shape
    src = torch.from_numpy(rows).to(dev())
    out = Box(M, i64=True)
    _lib.check(lib.cvk_argmax_channels(src.data_ptr(), ld, out.ptr, M, C, stream()))
    return out.host()


def check_argmax(rows, C, planted, got):
    want = R.argmax_ref(rows[:, :C])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (rows.shape, C, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist(), {int(p): planted.get(int(p)) for p in bad[:5]})
    assert np.array_equal(got, torch.argmax(torch.from_numpy(np.ascontiguousarray(rows[:, :C])), dim=-1).numpy())
    for p, (name, win) in planted.items():
        assert got[p] == win, (p, name)


@pytest.mark.parametrize("C", [1, 2, 3, 11, 12, 13, 32, 64, 130])
def test_argmax_channels_exact_with_ties_nan_inf_and_pads(C):
    """cvk_argmax_channels == argmax_ref == torch.argmax on the CPU, for M in {1, 255, 256, 257, 4099} and ld in {C, C + 3} with the
    pads holding +inf and NaN.  Rows are random multiples of 1/4 (ties occur by themselves) with the cases of
    eval_io_ref.ARGMAX_CASES planted at rows 0, 255, 256, M - 1 and throughout; with one row, every case gets its own call.
    Written against: `v >= best` (last maximum: all_equal, dup2, dup3, inf_twice, both zero orders), a NaN test that lets a later
    NaN or a later +inf replace the first NaN (nan_twice, nan_first), NaN ignored (nan_after_inf, nan_last), walking C where ld is
    meant in the row address or the reverse (ld = C + 3: the pads would win), a loop that starts at the wrong channel, `m <= M`."""
    for M in (1, 255, 256, 257, 4099):
        for ld in (C, C + 3):
            for shift in (range(len(R.ARGMAX_CASES)) if M == 1 else (C,)):
                rows, planted = R.argmax_rows(M, C, ld, seed=1000 * C + M, shift=shift)
                check_argmax(rows, C, planted, run_argmax(rows, C))


@pytest.mark.parametrize("ld", [3, 6])
def test_argmax_channels_past_the_grid_cap(ld):
    """M = 8192 * 256 + 257 rows of C = 3: the rows from 8192 * 256 on are reached only by the grid-stride loop; row 8192 * 256 and
    the last row are planted.  Written against: a missing or mis-strided loop, a 32-bit `m * ld`."""
    M = R.ARGMAX_GRID_CAP + 257
    rows, planted = R.argmax_rows(M, 3, ld, seed=ld)
    assert R.ARGMAX_GRID_CAP in planted and M - 1 in planted
    check_argmax(rows, 3, planted, run_argmax(rows, 3))


@pytest.mark.parametrize("N,H,W", [(2, 5, 7), (2, 1, 9), (2, 9, 1), (3, 1, 1)])
def test_argmax_channels_wrapper_layouts(N, H, W):
    """A.argmax_channels on NCHW-contiguous logits (one copy), channels_last logits (zero copy) and the 12-channel slice of a
    16-channel channels_last tensor (the zero-copy ld > C route of _as_nhwc; its 4 spare channels hold +inf and NaN), also with
    H = 1 and W = 1, where a size-1 dimension's stride is arbitrary.  Written against: a wrapper that passes C for ld or reads
    the permuted tensor's memory in NCHW order."""
    A = pkg()
    C, M = 12, N * H * W
    rows, planted = R.argmax_rows(M, C, 16, seed=M)
    want = R.argmax_ref(rows[:, :C]).reshape(N, H, W)
    wide = torch.from_numpy(rows).to(dev()).reshape(N, H, W, 16).permute(0, 3, 1, 2)       # channels_last, 16 channels
    dense = torch.from_numpy(np.ascontiguousarray(rows[:, :C])).to(dev()).reshape(N, H, W, C).permute(0, 3, 1, 2)
    for name, logits in (("channels_last", dense), ("nchw", dense.contiguous()), ("slice", wide[:, :C])):
        assert tuple(logits.shape) == (N, C, H, W)
        got = A.argmax_channels(logits)
        assert got.dtype == torch.int64 and tuple(got.shape) == (N, H, W)
        assert np.array_equal(got.cpu().numpy(), want), name
        assert torch.equal(got.cpu(), torch.argmax(logits.cpu(), dim=1)), name


# ------------------------------------------------------------------------------------------------ cvk_confusion_accumulate
KI = [(1, -100), (2, 1), (12, 11), (12, -100), (12, 255), (13, 0), (256, 255), (4096, 7)]


def run_confusion(hist, pred, label, K, ignore):
    _lib, lib = libs()
    p, l = torch.from_numpy(pred).to(dev()), torch.from_numpy(label).to(dev())
    assert p.dtype == torch.int64 and l.dtype == torch.int64
    _lib.check(lib.cvk_confusion_accumulate(p.data_ptr(), l.data_ptr(), hist.ptr, p.numel(), K, ignore, stream()))
    torch.cuda.synchronize()


def new_hist(K, start=None):
    hist = Box(3 * K, i64=True)
    if start is None:
        hist.body().zero_()
    else:
        hist.body().copy_(torch.from_numpy(start.reshape(-1)))
    return hist


def check_counts(got, want, pred, label, K, ignore, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, K, ignore, [(tuple(b), int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:6]])
    assert (got[0] <= np.minimum(got[1], got[2])).all()
    assert got[2].sum() == int(((label >= 0) & (label < K) & (label != ignore)).sum())


@pytest.mark.parametrize("K,ignore", KI)
def test_confusion_counts_exact(K, ignore):
    """hist == confusion_ref for M in {1, 1023, 1025, 70001}: random classes, one class everywhere, every label ignored (hist, which
    starts non-zero, must not change) and the planted values -1, K, 255, -100 in pred and in label.  With M = 1 every planted pair
    of eval_io_ref.confusion_planted_pairs that holds no 64-bit value gets its own call.
    Written against: the `p < K` or `p >= 0` guard dropped (an LDS write out of the histogram: -1, K, 255), the prediction area
    counted before the ignore test, `l == ignore` tested on pred, the label area counted only where pred is in range, a histogram
    row stride other than K, a partial last block dropped (M = 1023, 1025), hist overwritten instead of added to."""
    pairs = [(p, l) for p, l in R.confusion_planted_pairs(K, ignore) if abs(p) < 2 ** 31 and abs(l) < 2 ** 31]
    for p, l in pairs + [(K - 1, K - 1), (0, K - 1)]:
        pred, label = np.array([p], dtype=np.int64), np.array([l], dtype=np.int64)
        hist = new_hist(K)
        run_confusion(hist, pred, label, K, ignore)
        check_counts(hist.host().reshape(3, K), R.confusion_ref(pred, label, K, ignore), pred, label, K, ignore, ("pixel", p, l))
    for M in (1023, 1025, 70_001):
        for kind in ("random", "planted32", "constant", "ignored"):
            pred, label = R.confusion_inputs(M, K, ignore, seed=M + K, kind="random" if kind == "planted32" else kind)
            if kind == "planted32":
                at = np.linspace(0, M - 1, num=len(pairs)).astype(np.int64)
                pred[at], label[at] = np.array(pairs, dtype=np.int64).T
            start = np.arange(3 * K, dtype=np.int64).reshape(3, K) * 3 + 1 if kind == "ignored" else np.zeros((3, K), dtype=np.int64)
            hist = new_hist(K, start)
            run_confusion(hist, pred, label, K, ignore)
            want = start + R.confusion_ref(pred, label, K, ignore)
            if kind == "ignored":
                assert np.array_equal(want, start)
            check_counts(hist.host().reshape(3, K) - start, want - start, pred, label, K, ignore, (kind, M))


@pytest.mark.parametrize("K,ignore", KI)
def test_confusion_compares_64_bit_values(K, ignore):
    """pred and label are int64 and compared as such: 2**32 + c is no class (it is neither an intersection with pred == c nor a
    label or prediction of class c), 2**32 + ignore is not the ignore index (the pixel's prediction still counts) and
    -(2**32) + c is negative.  Every planted pair alone (M = 1), and all of them spread over M in {1023, 1025, 70001}.
    Written against: `(int)label[m]`, `(int)pred[m]` -- the low word taken for the value."""
    for p, l in R.confusion_planted_pairs(K, ignore):
        pred, label = np.array([p], dtype=np.int64), np.array([l], dtype=np.int64)
        hist = new_hist(K)
        run_confusion(hist, pred, label, K, ignore)
        check_counts(hist.host().reshape(3, K), R.confusion_ref(pred, label, K, ignore), pred, label, K, ignore, ("pixel", p, l))
    for M in (1023, 1025, 70_001):
        pred, label = R.confusion_inputs(M, K, ignore, seed=M + K, kind="planted")
        assert (np.abs(pred) >= 2 ** 32).any() and (np.abs(label) >= 2 ** 32).any()
        hist = new_hist(K)
        run_confusion(hist, pred, label, K, ignore)
        check_counts(hist.host().reshape(3, K), R.confusion_ref(pred, label, K, ignore), pred, label, K, ignore, ("planted", M))


def test_confusion_accumulates_past_the_block_cap_and_into_a_non_zero_hist():
    """Three updates (the last M = 1024 * 1024 + 777, past the point where the block count stops growing) into one hist that starts
    at 2**33 per counter: the sum of the three references on top of the start, so the kernel adds in 64 bits and overwrites nothing.
    Written against: a loop stride that is not the grid's size, hist stored instead of added to, a 32-bit global counter."""
    K, ignore = 12, 11
    start = np.full((3, K), 2 ** 33, dtype=np.int64) + np.arange(3 * K, dtype=np.int64).reshape(3, K)
    hist = new_hist(K, start)
    want = start.copy()
    for M, kind in ((70_001, "random"), (1025, "planted"), (1024 * 1024 + 777, "planted")):
        pred, label = R.confusion_inputs(M, K, ignore, seed=M, kind=kind)
        run_confusion(hist, pred, label, K, ignore)
        want += R.confusion_ref(pred, label, K, ignore)
        got = hist.host().reshape(3, K)
        assert np.array_equal(got, want), (M, [(tuple(b), int((got - want)[tuple(b)])) for b in np.argwhere(got != want)[:8]])


def same(a, b):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12


@pytest.mark.parametrize("K,ignore,kinds", [(12, 11, ("absent", "absent")), (12, 11, ("random", "planted")), (12, -100, ("random", "planted")),
                                            (12, 255, ("absent",)), (13, 0, ("random", "constant")), (2, 1, ("random",)),
                                            (12, 11, ("ignored",)), (12, -100, ("ignored", "ignored"))])
def test_confusion_meter_metrics_against_the_formulas(K, ignore, kinds):
    """ConfusionMeter over several updates: hist == the sum of confusion_ref, compute() == miou_ref and precision_recall() ==
    precision_recall_ref to 1e-12.  Covers a class absent from pred and label (its NaN IoU is left out of the mean), ignore outside
    [0, K) (every class counts), 64-bit values through the wrapper, and a meter that saw only ignored pixels (mIoU NaN, accuracy 0,
    no division error).  Written against: the mean taken over all K classes or with NaN counted as 0, union without `- inter`,
    accuracy over the prediction area, precision and recall swapped, the ignored class kept in the means."""
    A = pkg()
    meter = A.ConfusionMeter(K, ignore, dev())
    want = np.zeros((3, K), dtype=np.int64)
    for i, kind in enumerate(kinds):
        pred, label = R.confusion_inputs(4097 + i, K, ignore, seed=31 * K + i, kind=kind)
        shape = (1, 17, 241 + i) if i == 0 else (4097 + i,)
        meter.update(torch.from_numpy(pred).to(dev()).reshape(shape), torch.from_numpy(label).to(dev()).reshape(shape))
        want += R.confusion_ref(pred, label, K, ignore)
    assert np.array_equal(meter.hist.cpu().numpy(), want)
    acc, iou, miou = meter.compute()
    acc_r, iou_r, miou_r = R.miou_ref(want, ignore)
    assert same(acc, acc_r) and same(miou, miou_r), ((acc, acc_r), (miou, miou_r))
    assert np.allclose(iou.numpy(), iou_r, rtol=0, atol=1e-12, equal_nan=True)
    prec, rec = meter.precision_recall()
    prec_r, rec_r = R.precision_recall_ref(want, ignore)
    assert same(prec, prec_r) and same(rec, rec_r), ((prec, prec_r), (rec, rec_r))
    if set(kinds) == {"absent"}:
        assert np.isnan(iou_r[K // 2]) and not np.isnan(miou)
    if set(kinds) == {"ignored"}:
        assert not want.any() and np.isnan(miou) and acc == 0.0 and prec == 0.0 and rec == 0.0
    meter.reset()
    assert not meter.hist.any()


def test_confusion_meter_refuses_other_dtypes_and_shapes():
    A = pkg()
    meter = A.ConfusionMeter(12, 11, dev())
    ok = torch.zeros(4, 5, dtype=torch.int64, device=dev())
    with pytest.raises(ValueError):
        meter.update(ok.to(torch.int32), ok)
    with pytest.raises(ValueError):
        meter.update(ok, ok.to(torch.int32))
    with pytest.raises(ValueError):
        meter.update(ok, ok[:, :4])
    with pytest.raises(ValueError):
        meter.update(ok.reshape(-1), ok)
    assert not meter.hist.any()
