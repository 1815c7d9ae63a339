"""CPU-side checks of the cross-entropy options (class weights, label smoothing, reductions) and the class-statistics meter:
argument validation of the new entry points before any launch, the loss module's constructor and state_dict, and the two
class-weight formulas against a numpy restatement.  No compute calls (no GPU here)."""
import numpy as np
import pytest
import torch

import pytorch_camvid_amd as A
from pytorch_camvid_amd import _lib, functional as F

P = 4096                              # a fake, 16-byte aligned device address: every call below is refused before a launch
NONE, MEAN, SUM = 0, 1, 2             # include/cvk.h CVK_REDUCTION_*


def _err():
    return _lib.load().cvk_last_error_string()


def test_ce_fwd_ex_argument_validation_without_gpu():
    lib = _lib.load()
    fwd = lib.cvk_softmax_ce_fwd_ex
    #          logits ld  target weight eps  red   part loss px   M     C   ignore stream
    assert fwd(None, 12, P, None, 0.1, MEAN, P, P, None, 1024, 12, -100, None) == -1
    assert b"null" in _err()
    assert fwd(P, 12, None, None, 0.1, MEAN, P, P, None, 1024, 12, -100, None) == -1
    assert fwd(P, 12, P, None, 0.1, MEAN, None, P, None, 1024, 12, -100, None) == -1
    assert fwd(P, 12, P, None, 0.1, MEAN, P, None, None, 1024, 12, -100, None) == -1
    assert b"null" in _err()
    assert fwd(P, 12, P, None, 0.1, MEAN, P, P, None, 1024, 0, -100, None) == -1              # C <= 0
    assert b"bad arguments" in _err()
    assert fwd(P, 12, P, None, 0.1, MEAN, P, P, None, 1024, -3, -100, None) == -1
    assert fwd(P, 12, P, None, 0.1, MEAN, P, P, None, 1024, 13, -100, None) == -1             # ld < C
    assert fwd(P, 200, P, None, 0.1, MEAN, P, P, None, 1024, 129, -100, None) == -1           # C > 128
    assert fwd(P, 12, P, None, 0.1, MEAN, P, P, None, 0, 12, -100, None) == -1                # M
    assert fwd(P, 12, P, None, 0.1, 3, P, P, None, 1024, 12, -100, None) == -1                # reduction code
    assert fwd(P, 12, P, None, 0.1, -1, P, P, None, 1024, 12, -100, None) == -1
    assert fwd(P, 12, P, None, -0.1, MEAN, P, P, None, 1024, 12, -100, None) == -1            # eps outside [0, 1]
    assert fwd(P, 12, P, None, 1.5, MEAN, P, P, None, 1024, 12, -100, None) == -1
    assert fwd(P, 12, P, None, float("nan"), MEAN, P, P, None, 1024, 12, -100, None) == -1
    assert b"bad arguments" in _err()
    assert fwd(P, 12, P, None, 0.1, NONE, P, P, None, 1024, 12, -100, None) == -1             # 'none' without a loss map
    assert b"loss_px" in _err()
    assert lib.cvk_ce_ex_part_floats(1025) == 8 and lib.cvk_ce_ex_part_floats(0) == 0


def test_ce_bwd_ex_argument_validation_without_gpu():
    lib = _lib.load()
    bwd = lib.cvk_softmax_ce_bwd_ex
    #          logits ld  target weight eps  red   loss4 gout scale dl  ld_d M     C   ignore stream
    assert bwd(None, 12, P, None, 0.1, MEAN, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1
    assert b"null" in _err()
    assert bwd(P, 12, P, None, 0.1, MEAN, None, None, 1.0, P, 12, 1024, 12, -100, None) == -1
    assert bwd(P, 12, P, None, 0.1, MEAN, P, None, 1.0, None, 12, 1024, 12, -100, None) == -1
    assert b"null" in _err()
    assert bwd(P, 12, P, None, 0.1, MEAN, P, None, 1.0, P, 12, 1024, 0, -100, None) == -1     # C <= 0
    assert b"bad arguments" in _err()
    assert bwd(P, 11, P, None, 0.1, MEAN, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1    # ld < C
    assert bwd(P, 12, P, None, 0.1, MEAN, P, None, 1.0, P, 11, 1024, 12, -100, None) == -1    # ld_d < C
    assert bwd(P, 12, P, None, 0.1, 7, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1       # reduction code
    assert bwd(P, 12, P, None, 2.0, MEAN, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1    # eps
    assert b"bad arguments" in _err()
    assert bwd(P, 12, P, None, 0.1, NONE, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1    # 'none' needs a per-pixel grad_out
    assert b"grad_out" in _err()


def test_class_histogram_argument_validation_without_gpu():
    lib = _lib.load()
    h = lib.cvk_class_histogram
    #        masks bytes N  HW     C    ignore hist stream
    assert h(None, 1, 2, 172800, 12, -100, P, None) == -1
    assert b"null" in _err()
    assert h(P, 1, 2, 172800, 12, -100, None, None) == -1
    assert b"null" in _err()
    assert h(P, 4, 2, 172800, 12, -100, P, None) == -1        # mask_bytes
    assert b"bad arguments" in _err()
    assert h(P, 2, 2, 172800, 12, -100, P, None) == -1
    assert h(P, 1, 0, 172800, 12, -100, P, None) == -1        # N
    assert h(P, 8, 2, 0, 12, -100, P, None) == -1             # HW
    assert h(P, 8, 2, 172800, 0, -100, P, None) == -1         # C <= 0
    assert h(P, 8, 2, 172800, 257, -100, P, None) == -1       # C > 256
    assert b"bad arguments" in _err()


def test_loss_constructor_validation_and_state_dict():
    w = torch.rand(12) + 0.5
    lf = A.CrossEntropyLoss(weight=w, label_smoothing=0.1, reduction="sum")
    ref = torch.nn.CrossEntropyLoss(weight=w, label_smoothing=0.1, reduction="sum")
    assert list(lf.state_dict()) == list(ref.state_dict()) == ["weight"]
    assert torch.equal(lf.state_dict()["weight"], ref.state_dict()["weight"])
    assert dict(lf.named_buffers())["weight"] is w
    assert list(A.CrossEntropyLoss().state_dict()) == list(torch.nn.CrossEntropyLoss().state_dict()) == []
    # the weight round-trips through state_dict as torch's does
    other = A.CrossEntropyLoss(weight=torch.zeros(12))
    other.load_state_dict(ref.state_dict())
    assert torch.equal(other.weight, w)
    # a module move converts the buffer (.double() as a device-free stand-in for .cuda())
    assert lf.double().weight.dtype == torch.float64
    # positional parameters keep their meaning; the new ones are keyword-only
    lf = A.CrossEntropyLoss(0.5, 11)
    assert (lf.grad_scale, lf.ignore_index, lf.weight, lf.reduction, lf.label_smoothing) == (0.5, 11, None, "mean", 0.0)
    with pytest.raises(TypeError):
        A.CrossEntropyLoss(1.0, -100, w)
    for bad in ("avg", "elementwise_mean", None):
        with pytest.raises(ValueError, match="reduction"):
            A.CrossEntropyLoss(reduction=bad)
    for eps in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="label_smoothing"):
            A.CrossEntropyLoss(label_smoothing=eps)
    A.CrossEntropyLoss(label_smoothing=1.0)
    A.CrossEntropyLoss(label_smoothing=0.0)
    with pytest.raises(ValueError, match="1-D"):
        A.CrossEntropyLoss(weight=torch.ones(3, 4))
    with pytest.raises(ValueError, match="1-D"):
        A.CrossEntropyLoss(weight=[1.0, 2.0])
    with pytest.raises(ValueError, match="reduction"):
        A.cross_entropy(torch.zeros(1, 3, 2, 2), torch.zeros(1, 2, 2, dtype=torch.int64), reduction="avg")


def test_options_refuse_cpu_tensors_loudly():
    x = torch.zeros(1, 3, 2, 2)
    t = torch.zeros(1, 2, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.CrossEntropyLoss(weight=torch.ones(3))(x, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.cross_entropy(x, t, label_smoothing=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.cross_entropy(x, t, reduction="none")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.cross_entropy(x, t, 1)                   # third positional int = ignore_index, as before weight existed


def _median_frequency_np(pix, img):
    w = np.zeros(len(pix))
    present = [c for c in range(len(pix)) if pix[c] > 0]
    freq = {c: pix[c] / img[c] for c in present}
    med = float(np.median([freq[c] for c in present]))
    for c in present:
        w[c] = med / freq[c]
    return w


def _enet_np(pix):
    total = float(sum(pix))
    return np.array([1.0 / np.log(1.02 + p / total) if p > 0 else 0.0 for p in pix])


def _counts_of(masks, C, ignore_index):
    """numpy restatement of cvk_class_histogram's two counters over a list of masks."""
    pix = np.zeros(C, dtype=np.int64)
    img = np.zeros(C, dtype=np.int64)
    for m in masks:
        v = m[(m != ignore_index) & (m >= 0) & (m < C)]
        b = np.bincount(v, minlength=C)
        pix += b
        img += np.where(b > 0, b.sum(), 0)
    return pix, img


def test_class_weight_formulas_match_numpy():
    rng = np.random.default_rng(0)
    C = 12
    # class 4 never occurs, class 11 is the ignored class; some images lack some classes
    masks = []
    for i in range(6):
        m = rng.choice([0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11], size=(24, 32), p=[.3, .2, .15, .1, .05, .05, .04, .03, .02, .01, .05])
        if i % 2:
            m[m == 9] = 0
        if i == 3:
            m[:4] = 200                          # out of range: counted nowhere
        masks.append(m)
    pix, img = _counts_of(masks, C, 11)
    assert pix[4] == 0 and pix[11] == 0 and img[9] < img[0]
    for method, ref in (("median_frequency", _median_frequency_np(pix, img)), ("enet", _enet_np(pix))):
        w = F.weights_from_counts(pix, img, method)
        np.testing.assert_allclose(w, ref, rtol=1e-12)
        assert w[4] == 0 and w[11] == 0 and (w[[0, 1, 2, 3, 5, 6, 7, 8, 9, 10]] > 0).all()
    # the class at the median frequency gets weight 1 (odd number of present classes: 11 without the ignored one -> drop one)
    pix2, img2 = pix.copy(), img.copy()
    pix2[10] = img2[10] = 0
    w = F.weights_from_counts(pix2, img2, "median_frequency")
    assert np.isclose(np.sort(w[w > 0])[4], 1.0)
    # ENet weights are bounded by 1/ln(1.02) and fall with frequency
    w = F.weights_from_counts(pix, img, "enet")
    assert w.max() < 1 / np.log(1.02) and w[0] == w[w > 0].min()
    assert not F.weights_from_counts(np.zeros(C), np.zeros(C)).any()
    with pytest.raises(ValueError, match="method"):
        F.weights_from_counts(pix, img, "inverse")
    with pytest.raises(ValueError, match="method"):
        A.class_weights([], 12, method="inverse")
    with pytest.raises(ValueError, match="no batches"):
        A.class_weights([], 12)
