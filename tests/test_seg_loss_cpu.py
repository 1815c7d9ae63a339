"""CPU-side checks of the fused focal + soft-Dice loss: argument validation of cvk_seg_loss_fwd / _bwd before any launch, the size
queries, the module's constructor and state_dict, the refusal of CPU tensors, and the fp64 restatement (tests/seg_loss_ref.py) that
the GPU tests compare the kernels with: against torch's cross-entropy, against the closed-form gradient the kernel implements, and
in the corner cases.  No compute calls (no GPU here)."""
import pytest
import torch

import pytorch_camvid_amd as A
from pytorch_camvid_amd import _lib
from tests import seg_loss_ref as R

P = 4096                              # a fake, 16-byte aligned device address: every call below is refused before a launch
PRESENT, ALL = 0, 1                   # include/cvk.h CVK_DICE_*
NAN, INF = float("nan"), float("inf")


def _err():
    return _lib.load().cvk_last_error_string()


def test_seg_loss_fwd_argument_validation_without_gpu():
    fwd = _lib.load().cvk_seg_loss_fwd
    #          logits ld  target weight ce  dice gamma s    avg      part rec M     C   ignore stream
    assert fwd(None, 12, P, None, 1.0, 0.5, 2.0, 1.0, PRESENT, P, P, 1024, 12, -100, None) == -1
    assert b"null" in _err()
    assert fwd(P, 12, None, None, 1.0, 0.5, 2.0, 1.0, PRESENT, P, P, 1024, 12, -100, None) == -1
    assert fwd(P, 12, P, None, 1.0, 0.5, 2.0, 1.0, PRESENT, None, P, 1024, 12, -100, None) == -1
    assert fwd(P, 12, P, None, 1.0, 0.5, 2.0, 1.0, PRESENT, P, None, 1024, 12, -100, None) == -1
    assert b"null" in _err()
    assert fwd(P, 12, P, None, 1.0, 0.5, 2.0, 1.0, PRESENT, P, P, 1024, 0, -100, None) == -1          # C <= 0
    assert b"bad arguments" in _err()
    assert fwd(P, 12, P, None, 1.0, 0.5, 2.0, 1.0, PRESENT, P, P, 1024, -3, -100, None) == -1
    assert fwd(P, 200, P, None, 1.0, 0.5, 2.0, 1.0, PRESENT, P, P, 1024, 129, -100, None) == -1       # C > 128
    assert fwd(P, 12, P, None, 1.0, 0.5, 2.0, 1.0, PRESENT, P, P, 1024, 13, -100, None) == -1         # ld < C
    assert fwd(P, 12, P, None, 1.0, 0.5, 2.0, 1.0, PRESENT, P, P, 0, 12, -100, None) == -1            # M <= 0
    assert fwd(P, 12, P, None, 1.0, 0.5, 2.0, 1.0, PRESENT, P, P, -5, 12, -100, None) == -1
    for bad in (-0.5, NAN, INF):
        assert fwd(P, 12, P, None, bad, 0.5, 2.0, 1.0, PRESENT, P, P, 1024, 12, -100, None) == -1, bad    # ce
        assert fwd(P, 12, P, None, 1.0, bad, 2.0, 1.0, PRESENT, P, P, 1024, 12, -100, None) == -1, bad    # dice
        assert fwd(P, 12, P, None, 1.0, 0.5, bad, 1.0, PRESENT, P, P, 1024, 12, -100, None) == -1, bad    # gamma
        assert fwd(P, 12, P, None, 1.0, 0.5, 2.0, bad, PRESENT, P, P, 1024, 12, -100, None) == -1, bad    # smooth
        assert b"bad arguments" in _err()
    assert fwd(P, 12, P, None, 0.0, 0.0, 2.0, 1.0, PRESENT, P, P, 1024, 12, -100, None) == -1         # both coefficients zero
    assert b"both zero" in _err()
    assert fwd(P, 12, P, None, 1.0, 0.5, 2.0, 1.0, 2, P, P, 1024, 12, -100, None) == -1               # average code
    assert b"dice_average" in _err()
    assert fwd(P, 12, P, None, 1.0, 0.5, 2.0, 1.0, -1, P, P, 1024, 12, -100, None) == -1


def test_seg_loss_bwd_argument_validation_without_gpu():
    bwd = _lib.load().cvk_seg_loss_bwd
    #          logits ld  target weight ce  dice gamma rec gout scale dl ld_d M     C   ignore stream
    assert bwd(None, 12, P, None, 1.0, 0.5, 2.0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1
    assert b"null" in _err()
    assert bwd(P, 12, None, None, 1.0, 0.5, 2.0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1
    assert bwd(P, 12, P, None, 1.0, 0.5, 2.0, None, None, 1.0, P, 12, 1024, 12, -100, None) == -1
    assert bwd(P, 12, P, None, 1.0, 0.5, 2.0, P, None, 1.0, None, 12, 1024, 12, -100, None) == -1
    assert b"null" in _err()
    assert bwd(P, 12, P, None, 1.0, 0.5, 2.0, P, None, 1.0, P, 12, 1024, 0, -100, None) == -1         # C <= 0
    assert b"bad arguments" in _err()
    assert bwd(P, 200, P, None, 1.0, 0.5, 2.0, P, None, 1.0, P, 200, 1024, 129, -100, None) == -1     # C > 128
    assert bwd(P, 11, P, None, 1.0, 0.5, 2.0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1        # ld < C
    assert bwd(P, 12, P, None, 1.0, 0.5, 2.0, P, None, 1.0, P, 11, 1024, 12, -100, None) == -1        # ld_d < C
    assert bwd(P, 12, P, None, 1.0, 0.5, 2.0, P, None, 1.0, P, 12, 0, 12, -100, None) == -1           # M <= 0
    for bad in (-1.0, NAN, INF):
        assert bwd(P, 12, P, None, bad, 0.5, 2.0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1, bad
        assert bwd(P, 12, P, None, 1.0, bad, 2.0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1, bad
        assert bwd(P, 12, P, None, 1.0, 0.5, bad, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1, bad
        assert b"bad arguments" in _err()
    assert bwd(P, 12, P, None, 0.0, 0.0, 2.0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1
    assert b"both zero" in _err()


def test_seg_loss_size_queries():
    lib = _lib.load()
    # per workgroup of 1024 pixels: focal numerator, sum of weights, valid, out of range, then I, P, T per class
    assert lib.cvk_seg_loss_part_floats(1025, 12) == (4 + 3 * 12) * 2 == (4 + 3 * 12) * lib.cvk_ce_blocks(1025)
    assert lib.cvk_seg_loss_part_floats(8 * 360 * 480, 12) == 40 * 1350
    assert lib.cvk_seg_loss_part_floats(0, 12) == 0 and lib.cvk_seg_loss_part_floats(1024, 0) == 0
    assert lib.cvk_seg_loss_part_floats(1024, 129) == 0
    # L, valid, out of range, sum w, F, D, K, then dice_c, a_c, b_c
    assert lib.cvk_seg_loss_record_floats(12) == 7 + 36 and lib.cvk_seg_loss_record_floats(128) == 7 + 384
    assert lib.cvk_seg_loss_record_floats(0) == 0 and lib.cvk_seg_loss_record_floats(129) == 0


def test_constructor_validation_and_state_dict():
    w = torch.rand(12) + 0.5
    lf = A.SegmentationLoss(1.0, 0.5, focal_gamma=2.0, weight=w)
    assert isinstance(lf, torch.nn.Module)
    assert list(lf.state_dict()) == ["weight"] and torch.equal(lf.state_dict()["weight"], w)
    assert dict(lf.named_buffers())["weight"] is w
    assert list(A.SegmentationLoss().state_dict()) == []
    other = A.SegmentationLoss(weight=torch.zeros(12))
    other.load_state_dict(lf.state_dict())
    assert torch.equal(other.weight, w)
    assert lf.double().weight.dtype == torch.float64          # a module move converts the buffer
    lf = A.SegmentationLoss()
    assert (lf.ce, lf.dice, lf.focal_gamma, lf.weight, lf.ignore_index, lf.dice_smooth, lf.dice_average, lf.grad_scale) == \
        (1.0, 0.0, 0.0, None, -100, 1.0, "present", 1.0)
    with pytest.raises(TypeError):
        A.SegmentationLoss(1.0, 0.5, 2.0)                     # everything after the two coefficients is keyword-only
    for name in ("ce", "dice", "focal_gamma", "dice_smooth"):
        for bad in (-0.1, NAN, INF):
            kw = {"ce": 1.0, "dice": 0.5, name: bad}
            with pytest.raises(ValueError, match=name):
                A.SegmentationLoss(**kw)
    with pytest.raises(ValueError, match="both"):
        A.SegmentationLoss(0.0, 0.0)
    with pytest.raises(ValueError, match="dice_average"):
        A.SegmentationLoss(dice_average="macro")
    with pytest.raises(ValueError, match="1-D"):
        A.SegmentationLoss(weight=torch.ones(3, 4))
    with pytest.raises(ValueError, match="1-D"):
        A.SegmentationLoss(weight=[1.0, 2.0])
    with pytest.raises(RuntimeError, match="no forward"):
        A.SegmentationLoss().last_terms
    f = A.FocalLoss()
    assert (f.ce, f.dice, f.focal_gamma, f.ignore_index) == (1.0, 0.0, 2.0, -100) and list(f.state_dict()) == []
    f = A.FocalLoss(0.5, w, 11)
    assert f.focal_gamma == 0.5 and f.weight is w and f.ignore_index == 11
    d = A.DiceLoss()
    assert (d.ce, d.dice, d.dice_smooth, d.dice_average, d.ignore_index) == (0.0, 1.0, 1.0, "present", -100)
    d = A.DiceLoss(0.0, "all", 11)
    assert (d.dice_smooth, d.dice_average, d.ignore_index) == (0.0, "all", 11)


def test_cpu_tensors_are_refused_loudly():
    x = torch.zeros(1, 3, 2, 2)
    t = torch.zeros(1, 2, 2, dtype=torch.int64)
    for lf in (A.SegmentationLoss(1.0, 0.5), A.SegmentationLoss(weight=torch.ones(3)), A.FocalLoss(), A.DiceLoss()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lf(x, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.segmentation_loss(x, t, 1.0, 0.5, focal_gamma=2.0)
    with pytest.raises(ValueError, match="both"):
        A.segmentation_loss(x, t, 0.0, 0.0)


def _case(C, seed, ignore_index=-100, N=2, H=9, W=11):
    g = torch.Generator().manual_seed(seed)
    x = 3 * torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    t = torch.randint(0, C, (N, H, W), generator=g)
    t[t == 1] = 0                                             # class 1 never occurs: "present" and "all" differ
    t[torch.rand(N, H, W, generator=g) < 0.15] = ignore_index
    w = torch.rand(C, generator=g, dtype=torch.float64) * 2 + 0.1
    return x, t, w


@pytest.mark.parametrize("ignore_index", [-100, 3])
def test_restatement_with_gamma_0_is_torch_cross_entropy(ignore_index):
    x, t, w = _case(7, 1, ignore_index)
    for weight in (None, w):
        xr = x.clone().requires_grad_(True)
        L, F, D, _ = R.seg_loss(xr, t, 1.0, 0.0, weight=weight, ignore_index=ignore_index)
        L.backward()
        xt = x.clone().requires_grad_(True)
        ref = torch.nn.functional.cross_entropy(xt, t, weight=weight, ignore_index=ignore_index)
        ref.backward()
        assert abs(L.item() - ref.item()) <= 1e-14 * abs(ref.item()) and L.item() == F.item()
        assert (xr.grad - xt.grad).abs().max() <= 1e-15


@pytest.mark.parametrize("average", ["present", "all"])
@pytest.mark.parametrize("ce,dice", [(1.0, 0.0), (0.0, 1.0), (1.0, 0.5)])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0])
def test_autograd_of_the_restatement_is_the_closed_form_gradient(gamma, ce, dice, average):
    """Validates the formula the kernels implement (a_c, b_c, the focal bracket) before a GPU sees it."""
    for C, smooth, weighted in ((5, 1.0, True), (12, 0.0, False), (33, 1.0, True)):
        x, t, w = _case(C, 10 + C, ignore_index=2)
        kw = dict(focal_gamma=gamma, weight=w if weighted else None, ignore_index=2, dice_smooth=smooth, dice_average=average)
        xr = x.clone().requires_grad_(True)
        L, F, D, dc = R.seg_loss(xr, t, ce, dice, **kw)
        L.backward()
        g = R.seg_loss_grad_closed_form(x, t, ce, dice, **kw)
        assert (xr.grad - g).abs().max() <= 1e-13 * max(g.abs().max().item(), 1e-3), (C, (xr.grad - g).abs().max().item())
        assert (xr.grad[(t == 2).unsqueeze(1).expand_as(x)] == 0).all()
        if average == "present":                              # class 2 is ignored everywhere, class 1 never occurs
            assert dc[1] == 0 and dc[2] == 0
        elif smooth > 0:
            assert dc[1] > 0 and dc[2] > 0
        assert torch.isclose(L, ce * F + dice * D, rtol=1e-14)


def test_restatement_corner_cases():
    x, t, w = _case(6, 3)
    t_ign = torch.full_like(t, -100)
    # no valid pixel: K = 0 gives D = 0 with a zero gradient, the focal term is 0/0
    xr = x.clone().requires_grad_(True)
    L, F, D, dc = R.seg_loss(xr, t_ign, 0.0, 1.0)
    L.backward()
    assert L.item() == 0.0 and D.item() == 0.0 and torch.isnan(F).item() and (dc == 0).all() and (xr.grad == 0).all()
    assert (R.seg_loss_grad_closed_form(x, t_ign, 0.0, 1.0) == 0).all()
    L, F, D, _ = R.seg_loss(x, t_ign, 1.0, 0.5)
    assert torch.isnan(L).item() and D.item() == 0.0
    # "all" with no valid pixel: every class is the empty-against-empty case, dice_c = s / s = 1, D = 0
    L, _, D, dc = R.seg_loss(x, t_ign, 0.0, 1.0, dice_average="all")
    assert L.item() == 0.0 and D.item() == 0.0 and (dc == 1).all()
    # a perfect, saturated prediction drives both terms to 0
    xs = torch.full((1, 4, 3, 3), -40.0, dtype=torch.float64)
    ts = torch.randint(0, 4, (1, 3, 3), generator=torch.Generator().manual_seed(0))
    xs.scatter_(1, ts.unsqueeze(1), 40.0)
    L, F, D, _ = R.seg_loss(xs, ts, 1.0, 1.0, focal_gamma=2.0, dice_smooth=0.0)
    assert abs(F.item()) < 1e-30 and abs(D.item()) < 1e-12
