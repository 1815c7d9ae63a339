"""CPU-side checks of the test-time-augmentation feature: the fp64 restatement the GPU tests compare against (tests/tta_ref.py)
agrees with torch's own operators, the integer bilinear weights are the coordinate formula's, cvk.TestTimeAugmentation's size rule
and validation, the argument checks of cvk_tta_accumulate / cvk_tta_resize_input before any launch, and the `tta=None` defaults."""
import inspect
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import tta_ref as R


@pytest.mark.parametrize("src,dst", [((12, 16), (17, 23)), ((23, 31), (17, 23)), ((17, 23), (17, 23)), ((8, 8), (16, 16)),
                                     ((33, 29), (16, 16)), ((56, 75), (45, 60)), ((1, 5), (4, 3))])
def test_restatement_agrees_with_torch_fp64(src, dst):
    """Up-scaling, down-scaling and identity sizes: resize + softmax + flip of the restatement against F.interpolate(bilinear,
    align_corners=False) + softmax + flip in torch fp64, to 1e-12."""
    g = torch.Generator().manual_seed(src[0] * 100 + dst[1])
    x = 3.0 * torch.randn((2, 5, *src), generator=g, dtype=torch.float64)
    want = F.interpolate(x, dst, mode="bilinear", align_corners=False)
    got = R.resize(x, *dst)
    assert got.dtype == torch.float64 and (got - want).abs().max() <= 1e-12
    for flipped in (False, True):
        p = torch.softmax(want, dim=1)
        p = p.flip(-1) if flipped else p
        assert (R.view_probs(x, flipped, *dst) - p).abs().max() <= 1e-12
        assert (R.input_view(x, *dst, flipped) - (want.flip(-1) if flipped else want)).abs().max() <= 1e-12
    if src == dst:
        assert torch.equal(got, x)


def test_merge_is_the_ordered_mean_and_first_max():
    lg, fl = R.draw_views(0, 2, 12, ((12, 16), (17, 23), (23, 31)))
    probs, pred = R.merge(lg, fl, 17, 23)
    acc = None
    for x, f in zip(lg, fl):
        p = torch.softmax(F.interpolate(x.double(), (17, 23), mode="bilinear", align_corners=False), dim=1)
        p = p.flip(-1) if f else p
        acc = p if acc is None else acc + p
    assert (probs - acc / 6).abs().max() <= 1e-12
    assert (probs.sum(dim=1) - 1).abs().max() <= 1e-12
    assert torch.equal(pred, probs.argmax(dim=1))
    tie = torch.tensor([[[[0.25]], [[0.5]], [[0.5]], [[0.1]]]], dtype=torch.float64)
    assert R.argmax_first(tie).item() == 1


@pytest.mark.parametrize("out,inn", [(17, 12), (17, 23), (23, 31), (16, 8), (16, 33), (480, 360), (960, 1200), (7, 7), (720, 720)])
def test_integer_weights_equal_the_fp64_coordinate_formula(out, inn):
    i0, i1, w0, w1 = R.taps(out, inn)
    src = np.maximum((np.arange(out, dtype=np.float64) + 0.5) * (inn / out) - 0.5, 0.0)
    assert np.array_equal(i0, np.floor(src + 1e-9).astype(np.int64))           # 1e-9: the fp64 coordinate may sit an ulp under an integer
    assert np.abs(w1 - (src - i0)).max() <= 1e-9 and np.abs(w0 + w1 - 1.0).max() == 0.0
    assert np.array_equal(i1, np.minimum(i0 + 1, inn - 1)) and i0.min() >= 0 and i1.max() <= inn - 1
    if out == inn:
        assert np.array_equal(i0, np.arange(out)) and (w0 == 1.0).all() and (w1 == 0.0).all()


def test_view_sizes_follow_the_size_rule():
    import pytorch_camvid_amd as A
    tta = A.TestTimeAugmentation()
    assert tta.scales == (0.75, 1.0, 1.25) and tta.flip is True and tta.size_divisor == 1
    assert tta.view_sizes(360, 480) == [(270, 360, False), (270, 360, True), (360, 480, False), (360, 480, True), (450, 600, False),
                                        (450, 600, True)]
    assert tta.view_sizes(17, 23) == [(13, 17, False), (13, 17, True), (17, 23, False), (17, 23, True), (21, 29, False), (21, 29, True)]
    assert A.TestTimeAugmentation((0.5, 1.0), flip=False).view_sizes(45, 60) == [(23, 30, False), (45, 60, False)]   # floor(22.5 + 0.5)
    t32 = A.TestTimeAugmentation((0.75, 1.0, 1.25), size_divisor=32)
    assert t32.view_sizes(360, 480) == [(288, 384, False), (288, 384, True), (384, 480, False), (384, 480, True), (480, 608, False),
                                        (480, 608, True)]
    for t in (tta, t32, A.TestTimeAugmentation((1.5, 0.3), flip=False, size_divisor=7)):
        for H, W in ((360, 480), (17, 23), (64, 96)):
            assert t.view_sizes(H, W) == R.view_sizes(H, W, t.scales, t.flip, t.size_divisor)
            for (h, w, _), s in zip(t.view_sizes(H, W)[::2 if t.flip else 1], t.scales):
                d = t.size_divisor
                assert h % d == 0 and w % d == 0 and h == d * math.ceil(math.floor(H * s + 0.5) / d)
    # the view evaluate_report takes its loss from: scale 1.0, not mirrored, at the label size
    assert tta.loss_view(360, 480) == 2 and A.TestTimeAugmentation((0.5, 1.5)).loss_view(360, 480) is None
    assert t32.loss_view(360, 480) is None and t32.loss_view(64, 96) == 2


def test_constructor_validation():
    import pytorch_camvid_amd as A
    for bad in ((), (0.0, 1.0), (-1.0,), (float("nan"),), (float("inf"),), None, ("a",)):
        with pytest.raises(ValueError, match="scales"):
            A.TestTimeAugmentation(scales=bad)
    for bad in (0, -1, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="size_divisor"):
            A.TestTimeAugmentation(size_divisor=bad)
    with pytest.raises(ValueError, match="leaves no pixel"):
        A.TestTimeAugmentation((0.01,)).view_sizes(17, 23)
    tta = A.TestTimeAugmentation((1.0,), flip=False)
    with pytest.raises(ValueError, match=r"\[N, 3, H, W\]"):
        next(tta.views(torch.zeros(3, 17, 23)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tta(torch.nn.Identity(), torch.zeros(1, 3, 17, 23))


def test_entry_points_validate_before_any_launch():
    from pytorch_camvid_amd import _lib
    lib = _lib.load()
    p = 256                                                # a non-null, 16-byte aligned "pointer": never dereferenced on these paths
    acc = lib.cvk_tta_accumulate
    assert acc(None, 12, 4, 4, p, p, 1, 4, 4, 12, 0, 1, 1, 1.0, None) == -1 and b"null pointer" in lib.cvk_last_error_string()
    assert acc(p, 12, 4, 4, None, p, 1, 4, 4, 12, 0, 1, 1, 1.0, None) == -1 and b"null pointer" in lib.cvk_last_error_string()
    assert acc(p, 12, 4, 4, p, None, 1, 4, 4, 12, 0, 1, 1, 1.0, None) == -1 and b"null pointer" in lib.cvk_last_error_string()   # last needs pred
    assert acc(p, 40, 4, 4, p, p, 1, 4, 4, 33, 0, 1, 1, 1.0, None) == -1
    assert b"33 classes" in lib.cvk_last_error_string() and b"at most 32" in lib.cvk_last_error_string()
    for args in ((p, 8, 4, 4, p, p, 1, 4, 4, 12, 0, 1, 1, 1.0, None),           # ld < C
                 (p, 12, 0, 4, p, p, 1, 4, 4, 12, 0, 1, 1, 1.0, None),          # empty source
                 (p, 12, 4, 4, p, p, 1, 4, 20000, 12, 0, 1, 1, 1.0, None),      # side above 16384
                 (p, 12, 4, 4, p, p, 1, 4, 4, 0, 0, 1, 1, 1.0, None),           # no classes
                 (p, 12, 4, 4, p, p, 1, 4, 4, 12, 0, 1, 1, 0.0, None),          # inv_k
                 (p, 12, 4, 4, p, p, 1, 4, 4, 12, 0, 1, 1, float("nan"), None)):
        assert acc(*args) == -1 and b"bad arguments" in lib.cvk_last_error_string(), args
    assert acc(p, 32, 4, 4, p, p, 8, 16384, 16384, 32, 0, 1, 1, 1.0, None) == -1 and b"2^31" in lib.cvk_last_error_string()
    rs = lib.cvk_tta_resize_input
    assert rs(None, 1, 1, 1, 1, p, 1, 4, 4, 4, 4, 0, None) == -1 and b"null pointer" in lib.cvk_last_error_string()
    assert rs(p, 1, 1, 1, 1, None, 1, 4, 4, 4, 4, 0, None) == -1 and b"null pointer" in lib.cvk_last_error_string()
    assert rs(p, 1, 1, 1, 1, p + 4, 1, 4, 4, 4, 4, 0, None) == -1 and b"bad arguments" in lib.cvk_last_error_string()     # dst alignment
    assert rs(p, 1, 1, 1, 1, p, 1, 4, 4, 0, 4, 0, None) == -1 and b"bad arguments" in lib.cvk_last_error_string()
    assert rs(p, 1, 1, 1, 1, p, 70000, 4, 4, 4, 4, 0, None) == -1 and b"grid too large" in lib.cvk_last_error_string()


def test_tta_defaults_to_none_everywhere():
    import pytorch_camvid_amd as A
    for fn in (A.evaluate, A.evaluate_report, A.predict):
        par = inspect.signature(fn).parameters
        assert par["tta"].default is None and list(par)[-1] == "tta", fn
    assert "TestTimeAugmentation" in A.__all__


def test_chosen_seeds_keep_near_ties_under_the_cap():
    """The GPU tests allow a prediction to differ from the restatement's only where its two largest mean probabilities are within twice
    the probability tolerance, on at most 0.2 % of a case's pixels: the restatement alone must stay inside that cap for the seeds used."""
    for name, (seed, N, C, (H, W), sources, _) in R.CASES.items():
        lg, fl = R.draw_views(seed, N, C, sources)
        probs, _ = R.merge(lg, fl, H, W)
        assert int(R.near_ties(probs, 2e-5).sum()) <= 0.002 * N * H * W, name      # 2e-5: twice the largest tolerance any case gets
