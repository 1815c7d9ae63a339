"""CPU-side checks of sliding-window inference: cvk.SlidingWindow's grid and counts against the restatement of tests/window_ref.py and
against brute force, the closed forms of include/cvk.h that the kernel evaluates, the constructor / argument validation, the checks of
cvk_window_merge before any launch, and the `window=None` defaults of the workflow."""
import inspect

import pytest
import torch

from tests import window_ref as R


@pytest.mark.parametrize("H,W,crop,stride", R.GRID_TABLE)
def test_grid_and_counts_match_the_restatement_and_brute_force(H, W, crop, stride):
    import pytorch_camvid_amd as A
    sw = A.SlidingWindow(crop=crop, stride=stride)
    wins = sw.windows(H, W)
    assert wins == R.windows(H, W, crop, stride)
    hw, ww = min(crop[0], H), min(crop[1], W)
    assert all((h, w) == (hw, ww) for _, _, h, w in wins)                           # equal sizes
    assert len(set(wins)) == len(wins)                                               # no two coincide
    assert all(0 <= y1 and y1 + h <= H and 0 <= x1 and x1 + w <= W for y1, x1, h, w in wins)
    assert wins == sorted(wins)                                                      # row-major visiting order
    gy = (max(H - crop[0], 0) + stride[0] - 1) // stride[0] + 1
    gx = (max(W - crop[1], 0) + stride[1] - 1) // stride[1] + 1
    assert len(wins) == gy * gx
    assert [y1 for y1, x1, _, _ in wins if x1 == 0] == [min(i * stride[0], H - hw) for i in range(gy)]
    cnt = sw.counts(H, W)
    assert cnt.dtype == torch.int64 and tuple(cnt.shape) == (H, W)
    assert torch.equal(cnt, R.counts(H, W, crop, stride))
    brute = torch.zeros((H, W), dtype=torch.int64)
    for y1, x1, h, w in wins:
        brute[y1:y1 + h, x1:x1 + w] += 1
    assert torch.equal(cnt, brute) and int(cnt.min()) >= 1


def _cover(p, size, win, stride, g):
    """include/cvk.h's closed forms: (first, last) grid index whose window holds position p."""
    lo = 0 if p < win else min((p - win) // stride + 1, g - 1)
    hi = g - 1 if p >= size - win else p // stride
    return lo, hi


@pytest.mark.parametrize("H,W,crop,stride", R.GRID_TABLE)
def test_closed_forms_give_the_covering_windows(H, W, crop, stride):
    """The windows holding a pixel are a contiguous range of grid rows times one of grid columns, and the closed forms name them."""
    for size, c, s in ((H, crop[0], stride[0]), (W, crop[1], stride[1])):
        win = min(c, size)
        g = (max(size - c, 0) + s - 1) // s + 1
        starts = [min(i * s, size - win) for i in range(g)]
        for p in range(size):
            holding = [i for i, a in enumerate(starts) if a <= p < a + win]
            assert holding == list(range(holding[0], holding[-1] + 1))
            assert _cover(p, size, win, s, g) == (holding[0], holding[-1]), (p, size, c, s)


def test_merge_fp32_restatement():
    """One window covering the image is the identity; two half-overlapping windows average the overlap in fp32."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn((1, 3, 4, 6), generator=g)
    out, pred = R.merge_fp32([x], 4, 6, (8, 8), (8, 8))
    assert torch.equal(out, x) and torch.equal(pred, x.argmax(dim=1))
    a, b = torch.randn((1, 3, 4, 4), generator=g), torch.randn((1, 3, 4, 4), generator=g)
    out, _ = R.merge_fp32([a, b], 4, 6, (4, 4), (2, 2))
    assert torch.equal(out[..., :2], a[..., :2]) and torch.equal(out[..., 4:], b[..., 2:])
    assert torch.equal(out[..., 2:4], (a[..., 2:] + b[..., :2]) / 2)
    tie = torch.tensor([[[[0.25]], [[0.5]], [[0.5]], [[0.1]]]])
    assert R.argmax_first(tie).item() == 1
    assert R.argmax_first(torch.tensor([[[[3.0]], [[float("nan")]], [[5.0]]]])).item() == 1      # a NaN wins


def test_constructor_and_input_validation():
    import pytorch_camvid_amd as A
    sw = A.SlidingWindow()
    assert sw.crop == (360, 480) and sw.stride == (240, 320)
    assert len(sw.windows(720, 960)) == 9 and sw.windows(360, 480) == [(0, 0, 360, 480)]
    assert A.SlidingWindow(crop=[8, 12], stride=[3, 7]).crop == (8, 12)
    for bad in ((0, 4), (4, -1), (4,), (4, 4, 4), 4, None, (4.0, 4), ("4", 4), (True, 4)):
        with pytest.raises(ValueError, match="crop"):
            A.SlidingWindow(crop=bad, stride=(1, 1))
        with pytest.raises(ValueError, match="stride"):
            A.SlidingWindow(crop=(8, 8), stride=bad)
    for stride in ((9, 8), (8, 9)):
        with pytest.raises(ValueError, match="stride must not exceed crop"):
            A.SlidingWindow(crop=(8, 8), stride=stride)
    with pytest.raises(ValueError, match="no pixel"):
        sw.windows(0, 5)
    with pytest.raises(ValueError, match=r"\[N, 3, H, W\]"):
        sw(torch.nn.Identity(), torch.zeros(3, 17, 23))
    with pytest.raises(ValueError, match=r"\[N, 3, H, W\]"):
        sw.logits(torch.nn.Identity(), torch.zeros(1, 3, 17, 23, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sw(torch.nn.Identity(), torch.zeros(1, 3, 17, 23))
    with pytest.raises(ValueError, match="SlidingWindow or None"):
        A.TestTimeAugmentation(window=(360, 480))
    tta = A.TestTimeAugmentation(window=sw)
    assert tta.window is sw and A.TestTimeAugmentation().window is None


class _Untouchable(torch.nn.Module):
    training = False

    def forward(self, x):
        raise AssertionError("the network was called")

    def eval(self):
        raise AssertionError("the network was touched")

    def train(self, mode=True):
        raise AssertionError("the network was touched")

    def parameters(self, recurse=True):
        raise AssertionError("the network was touched")


def test_tta_and_window_together_raise_before_the_network_is_touched():
    import pytorch_camvid_amd as A
    sw, tta = A.SlidingWindow(), A.TestTimeAugmentation()
    net = _Untouchable()

    def batches():
        raise AssertionError("the batches were read")
        yield

    frame = torch.zeros((8, 8, 3), dtype=torch.uint8)
    for call in (lambda: A.evaluate(net, batches(), tta=tta, window=sw), lambda: A.evaluate_report(net, batches(), tta=tta, window=sw),
                 lambda: A.predict(net, frame, tta=tta, window=sw)):
        with pytest.raises(ValueError, match=r"TestTimeAugmentation\(\.\.\., window=window\)"):
            call()
    with pytest.raises(ValueError, match="SlidingWindow or None"):
        A.evaluate(net, batches(), window=tta)                                       # a TTA object in the window slot


def test_window_defaults_to_none_everywhere():
    import pytorch_camvid_amd as A
    for fn in (A.evaluate, A.evaluate_report, A.predict):
        assert inspect.signature(fn).parameters["window"].default is None, fn
    assert inspect.signature(A.TestTimeAugmentation.__init__).parameters["window"].default is None
    assert "SlidingWindow" in A.__all__


def test_entry_point_validates_before_any_launch():
    from pytorch_camvid_amd import _lib
    lib = _lib.load()
    p = 256                                                # a non-null, 16-byte aligned "pointer": never dereferenced on these paths
    wm = lib.cvk_window_merge
    #       logits ld out pred N  H   W   C  hc wc sy sx iy ix stream
    assert wm(None, 12, p, p, 1, 17, 23, 12, 8, 12, 3, 7, 0, 0, None) == -1 and b"null pointer" in lib.cvk_last_error_string()
    assert wm(p, 12, None, p, 1, 17, 23, 12, 8, 12, 3, 7, 0, 0, None) == -1 and b"null pointer" in lib.cvk_last_error_string()
    assert wm(p, 40, p, p, 1, 17, 23, 33, 8, 12, 3, 7, 0, 0, None) == -1
    assert b"33 classes" in lib.cvk_last_error_string() and b"at most 32" in lib.cvk_last_error_string()
    for args in ((p, 8, p, p, 1, 17, 23, 12, 8, 12, 3, 7, 0, 0, None),              # ld < C
                 (p, 12, p, p, 0, 17, 23, 12, 8, 12, 3, 7, 0, 0, None),             # no images
                 (p, 12, p, p, 1, 17, 23, 0, 8, 12, 3, 7, 0, 0, None),              # no classes
                 (p, 12, p, p, 1, 17, 20000, 12, 8, 12, 3, 7, 0, 0, None),          # side above 16384
                 (p, 12, p, p, 1, 17, 23, 12, 0, 12, 3, 7, 0, 0, None),             # empty crop
                 (p, 12, p, p, 1, 17, 23, 12, 8, 20000, 3, 7, 0, 0, None)):
        assert wm(*args) == -1 and b"bad arguments" in lib.cvk_last_error_string(), args
    for sy, sx in ((9, 7), (3, 13), (0, 7), (3, -1)):                                # stride outside 1..crop
        assert wm(p, 12, p, p, 1, 17, 23, 12, 8, 12, sy, sx, 0, 0, None) == -1 and b"stride" in lib.cvk_last_error_string(), (sy, sx)
    for iy, ix in ((4, 0), (0, 3), (-1, 0), (0, -1)):                                # 17 x 23, crop 8 x 12, stride 3 x 7: a 4 x 3 grid
        assert wm(p, 12, p, p, 1, 17, 23, 12, 8, 12, 3, 7, iy, ix, None) == -1
        assert b"outside the 4 x 3 grid" in lib.cvk_last_error_string(), (iy, ix)
    assert wm(p, 12, p, p, 1, 5, 7, 12, 8, 12, 3, 7, 0, 1, None) == -1 and b"outside the 1 x 1 grid" in lib.cvk_last_error_string()
    assert wm(p, 32, p, p, 8, 16384, 16384, 32, 8, 12, 3, 7, 0, 0, None) == -1 and b"2^31" in lib.cvk_last_error_string()
