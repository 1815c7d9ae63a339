"""The input rules the loss nodes share, over the seven entry routes (the two cross-entropy nodes, SegmentationLoss, OhemCrossEntropyLoss,
LovaszSoftmaxLoss, BoundaryLoss, DistillationLoss with a matching teacher): one fault at a time on [1, 3, 2, 2] logits and a [1, 2, 2]
target, each refused with its exception type and message before any kernel is launched; then one clean forward and backward per route
(a 0-dim finite loss, a gradient of the logits' shape).  What the losses compute is held to fp64 by each loss's own suite."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROUTES = {
    "ce": ("CrossEntropyLoss", lambda A, w: A.CrossEntropyLoss(weight=w)),
    "ce_ex": ("CrossEntropyLoss", lambda A, w: A.CrossEntropyLoss(weight=w, label_smoothing=0.1)),
    "seg": ("SegmentationLoss", lambda A, w: A.SegmentationLoss(1, .5, weight=w)),
    "ohem": ("OhemCrossEntropyLoss", lambda A, w: A.OhemCrossEntropyLoss(0.7, 4, weight=w)),
    "lovasz": ("LovaszSoftmaxLoss", lambda A, w: A.LovaszSoftmaxLoss(1, .5, weight=w)),
    "boundary": ("BoundaryLoss", lambda A, w: A.BoundaryLoss(1, .5, weight=w)),
    "distill": ("DistillationLoss", lambda A, w: A.DistillationLoss(1, 1, weight=w)),
}


def dev():
    return torch.device("cuda:0")


def _inputs():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 3, 2, 2, generator=g).to(dev())
    t = torch.tensor([[[0, 1], [2, 1]]]).to(dev())
    return x, t


def _call(route, x, t, weight=None):
    import pytorch_camvid_amd as A
    lf = ROUTES[route][1](A, weight)
    if route == "distill":
        return lf(x, t, (0.5 * x.detach()).flip(1))      # a teacher of the logits' shape, dtype and device
    return lf(x, t)


# fault -> (logits, target, weight) of the good inputs (x, t), exception type, a piece of its message ({who}: the module's name)
FAULTS = {
    "logits_on_cpu": (lambda x, t: (x.cpu(), t, None), RuntimeError, "pytorch_camvid_amd.{who} needs HIP tensors (no CPU fallback)"),
    "float64_logits": (lambda x, t: (x.double(), t, None), RuntimeError, "float32 logits"),
    "int32_target": (lambda x, t: (x, t.int(), None), RuntimeError, "float32 logits and int64 target"),
    "target_shape": (lambda x, t: (x, torch.zeros((1, 2, 3), dtype=torch.int64, device=x.device), None), ValueError,
                     "Expected target size [1, 2, 2], got [1, 2, 3]"),
    "weight_length": (lambda x, t: (x, t, torch.ones(2, device=x.device)), RuntimeError, "for all 3 classes"),
    "weight_on_cpu": (lambda x, t: (x, t, torch.ones(3)), RuntimeError, "no implicit copy"),
    "float64_weight": (lambda x, t: (x, t, torch.ones(3, dtype=torch.float64, device=x.device)), RuntimeError,
                       "expected a float32 weight"),
    "logits_3d": (lambda x, t: (x[0], t, None), ValueError, None),         # the type only: four routes say so at the tuple unpack
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_one_fault_is_refused_with_its_message(route, fault):
    import re
    make, exc, piece = FAULTS[fault]
    x, t, w = make(*_inputs())
    match = None if piece is None else re.escape(piece.format(who=ROUTES[route][0]))
    with pytest.raises(exc, match=match):
        _call(route, x, t, w)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_clean_forward_and_backward(route):
    x, t = _inputs()
    x.requires_grad_(True)
    loss = _call(route, x, t)
    loss.backward()
    assert loss.dim() == 0 and torch.isfinite(loss).item()
    assert x.grad is not None and x.grad.shape == x.shape
