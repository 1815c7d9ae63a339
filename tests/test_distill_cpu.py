"""CPU-side checks of the knowledge-distillation loss: the fp64 restatement (tests/distill_ref.py) the GPU tests compare the kernels
with, against torch's cross-entropy and kl_div, against the closed-form gradient the backward kernel implements, and in the corner
cases; argument validation of cvk_kd_loss_fwd / _bwd before any launch; the size queries, the module's constructor and state_dict, and
the refusal of CPU tensors.  No compute calls (no GPU here)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pytorch_camvid_amd as A
from pytorch_camvid_amd import _lib
from tests import distill_ref as R

P = 4096                              # a fake, 16-byte aligned device address: every call below is refused before a launch
NAN, INF = float("nan"), float("inf")


def _err():
    return _lib.load().cvk_last_error_string()


def _case(C, seed, ignore_index=-100, N=2, H=7, W=9):
    g = torch.Generator().manual_seed(seed)
    x = 3 * torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    z = 3 * torch.randn(N, C, H, W, generator=g, dtype=torch.float64)
    t = torch.randint(0, C, (N, H, W), generator=g)
    t[torch.rand(N, H, W, generator=g) < 0.2] = ignore_index
    w = torch.rand(C, generator=g, dtype=torch.float64) * 2 + 0.1
    return x, z, t, w


@pytest.mark.parametrize("ignore_index", [-100, 3])
@pytest.mark.parametrize("distill_ignored", [False, True])
def test_restatement_at_T_1_is_torch_cross_entropy_and_kl_div(ignore_index, distill_ignored):
    x, z, t, w = _case(7, 1, ignore_index)
    for weight in (None, w):
        L, H, K, nD, agree = R.distill_loss(x, z, t, 1.0, 0.5, 1.0, 1.0, weight, ignore_index, distill_ignored)
        want_h = F.cross_entropy(x, t, weight=weight, ignore_index=ignore_index)
        keep = torch.ones_like(t, dtype=torch.bool) if distill_ignored else t != ignore_index
        xs, zs = x.permute(0, 2, 3, 1)[keep], z.permute(0, 2, 3, 1)[keep]
        want_k = F.kl_div(torch.log_softmax(xs, 1), torch.softmax(zs, 1), reduction="sum") / int(keep.sum())
        assert nD == int(keep.sum()) and agree == int((xs.argmax(1) == zs.argmax(1)).sum())
        assert abs(H.item() - want_h.item()) <= 1e-12 * abs(want_h.item())
        assert abs(K.item() - want_k.item()) <= 1e-12 * abs(want_k.item())
        assert abs(L.item() - (want_h + 0.5 * want_k).item()) <= 1e-12 * abs(L.item())


@pytest.mark.parametrize("T", [1.0, 2.0, 4.0, 8.0])
@pytest.mark.parametrize("ce,kd", [(1.0, 0.0), (0.0, 1.0), (1.0, 0.5)])
@pytest.mark.parametrize("distill_ignored", [False, True])
def test_autograd_of_the_restatement_is_the_closed_form_gradient(T, ce, kd, distill_ignored):
    """Validates the formula the kernels implement (the t2 tau / |D| factor in particular) before a GPU sees it."""
    tau, t2 = A.distillation_scales(T)
    for C, weighted in ((5, True), (12, False), (33, True)):
        x, z, t, w = _case(C, 10 + C, ignore_index=2)
        weight = w if weighted else None
        xr = x.clone().requires_grad_(True)
        L = R.distill_loss(xr, z, t, ce, kd, tau, t2, weight, 2, distill_ignored)[0]
        L.backward(torch.tensor(0.7, dtype=torch.float64))
        want = R.distill_grad(x, z, t, ce, kd, tau, t2, weight, 2, distill_ignored, g=0.7)
        assert (xr.grad - want).abs().max() <= 1e-12 * want.abs().max()


def test_distillation_scales_are_rounded_once():
    for T in (1.0, 2.0, 3.0, 4.0, 8.0, 0.7):
        tau, t2 = A.distillation_scales(T)
        assert tau == float(np.float32(1.0 / T)) and t2 == float(np.float32(T * T))
    for bad in (0.0, -1.0, NAN, INF, 1e30, 1e-30):
        with pytest.raises(ValueError):
            A.distillation_scales(bad)


def test_restatement_corner_cases():
    x, z, t, w = _case(6, 3)
    tau, t2 = A.distillation_scales(2.0)
    t_ign = torch.full_like(t, -100)
    # no valid pixel: H is 0/0; K too unless the ignored pixels are distilled
    L, H, K, nD, _ = R.distill_loss(x, z, t_ign, 1.0, 1.0, tau, t2, w)
    assert torch.isnan(H) and torch.isnan(K) and torch.isnan(L) and nD == 0
    L, H, K, nD, _ = R.distill_loss(x, z, t_ign, 0.0, 1.0, tau, t2, None, distill_ignored=True)
    assert H.item() == 0.0 and torch.isfinite(L) and L.item() == K.item() and nD == t.numel()
    # ce = 0 needs no target: every pixel is in D, the same numbers as an all-valid target
    a = R.distill_loss(x, z, None, 0.0, 1.0, tau, t2)
    b = R.distill_loss(x, z, torch.zeros_like(t), 0.0, 1.0, tau, t2)
    assert a[0].item() == b[0].item() and a[3] == b[3] == t.numel() and a[4] == b[4]
    # kd = 0 needs no teacher and is the weighted cross-entropy
    L, H, K, nD, agree = R.distill_loss(x, None, t, 1.0, 0.0, tau, t2, w)
    assert K.item() == 0.0 and agree == 0 and abs(L.item() - F.cross_entropy(x, t, weight=w).item()) <= 1e-12 * abs(L.item())
    # an out-of-range target: NaN, and the pixel is in neither set
    t_bad = t.clone()
    t_bad[0, 0, 0] = 6
    L, _, K, nD, _ = R.distill_loss(x, z, t_bad, 1.0, 1.0, tau, t2, distill_ignored=True)
    assert torch.isnan(L) and torch.isfinite(K) and nD == t.numel() - 1
    # the teacher's own values: K = 0 exactly
    assert R.distill_loss(x, x.clone(), t, 0.0, 1.0, tau, t2)[2].item() == 0.0


def test_kd_loss_fwd_argument_validation_without_gpu():
    fwd = _lib.load().cvk_kd_loss_fwd
    #          student ld_s teacher ld_t target weight ce kd  tau  t2  ign'd part rec M   C   ignore stream
    assert fwd(None, 12, P, 12, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, P, 1024, 12, -100, None) == -1
    assert b"null" in _err()
    assert fwd(P, 12, P, 12, P, None, 1.0, 1.0, 0.25, 16.0, 0, None, P, 1024, 12, -100, None) == -1
    assert fwd(P, 12, P, 12, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, None, 1024, 12, -100, None) == -1
    assert b"null" in _err()
    assert fwd(P, 12, P, 12, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, P, 1024, 0, -100, None) == -1           # C <= 0
    assert b"bad arguments" in _err()
    assert fwd(P, 200, P, 200, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, P, 1024, 129, -100, None) == -1       # C > 128
    assert b"bad arguments" in _err()
    assert fwd(P, 12, P, 12, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, P, 0, 12, -100, None) == -1             # M <= 0
    assert fwd(P, 11, P, 12, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, P, 1024, 12, -100, None) == -1          # ld_s < C
    assert b"stride" in _err()
    assert fwd(P, 12, P, 11, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, P, 1024, 12, -100, None) == -1          # ld_t < C
    assert b"stride" in _err()
    for bad in (-0.5, NAN, INF):
        assert fwd(P, 12, P, 12, P, None, bad, 1.0, 0.25, 16.0, 0, P, P, 1024, 12, -100, None) == -1, bad     # ce
        assert fwd(P, 12, P, 12, P, None, 1.0, bad, 0.25, 16.0, 0, P, P, 1024, 12, -100, None) == -1, bad     # kd
        assert b"finite and not negative" in _err()
    assert fwd(P, 12, P, 12, P, None, 0.0, 0.0, 0.25, 16.0, 0, P, P, 1024, 12, -100, None) == -1          # both coefficients zero
    assert b"both zero" in _err()
    for bad in (0.0, -0.25, NAN, INF):
        assert fwd(P, 12, P, 12, P, None, 1.0, 1.0, bad, 16.0, 0, P, P, 1024, 12, -100, None) == -1, bad      # tau
        assert fwd(P, 12, P, 12, P, None, 1.0, 1.0, 0.25, bad, 0, P, P, 1024, 12, -100, None) == -1, bad      # t2
        assert b"positive and finite" in _err()
    assert fwd(P, 12, P, 12, None, None, 1.0, 1.0, 0.25, 16.0, 0, P, P, 1024, 12, -100, None) == -1       # no target, ce > 0
    assert b"null target" in _err()
    assert fwd(P, 12, None, 0, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, P, 1024, 12, -100, None) == -1        # no teacher, kd > 0
    assert b"null teacher" in _err()


def test_kd_loss_bwd_argument_validation_without_gpu():
    bwd = _lib.load().cvk_kd_loss_bwd
    #          student ld_s teacher ld_t target weight ce kd  tau  t2  ign'd rec gout scale dl ld_d M   C   ignore stream
    assert bwd(None, 12, P, 12, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1
    assert b"null" in _err()
    assert bwd(P, 12, P, 12, P, None, 1.0, 1.0, 0.25, 16.0, 0, None, None, 1.0, P, 12, 1024, 12, -100, None) == -1
    assert bwd(P, 12, P, 12, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, None, 1.0, None, 12, 1024, 12, -100, None) == -1
    assert b"null" in _err()
    assert bwd(P, 12, P, 12, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, None, 1.0, P, 12, 1024, 0, -100, None) == -1        # C <= 0
    assert b"bad arguments" in _err()
    assert bwd(P, 200, P, 200, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, None, 1.0, P, 200, 1024, 129, -100, None) == -1   # C > 128
    assert bwd(P, 12, P, 12, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, None, 1.0, P, 12, 0, 12, -100, None) == -1          # M <= 0
    assert b"bad arguments" in _err()
    assert bwd(P, 11, P, 12, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1       # ld_s < C
    assert bwd(P, 12, P, 11, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1       # ld_t < C
    assert bwd(P, 12, P, 12, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, None, 1.0, P, 11, 1024, 12, -100, None) == -1       # ld_d < C
    assert b"stride" in _err()
    for bad in (-1.0, NAN, INF):
        assert bwd(P, 12, P, 12, P, None, bad, 1.0, 0.25, 16.0, 0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1, bad
        assert bwd(P, 12, P, 12, P, None, 1.0, bad, 0.25, 16.0, 0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1, bad
        assert b"finite and not negative" in _err()
    assert bwd(P, 12, P, 12, P, None, 0.0, 0.0, 0.25, 16.0, 0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1
    assert b"both zero" in _err()
    for bad in (0.0, -4.0, NAN, INF):
        assert bwd(P, 12, P, 12, P, None, 1.0, 1.0, bad, 16.0, 0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1, bad
        assert bwd(P, 12, P, 12, P, None, 1.0, 1.0, 0.25, bad, 0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1, bad
        assert b"positive and finite" in _err()
    assert bwd(P, 12, P, 12, None, None, 1.0, 1.0, 0.25, 16.0, 0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1
    assert b"null target" in _err()
    assert bwd(P, 12, None, 0, P, None, 1.0, 1.0, 0.25, 16.0, 0, P, None, 1.0, P, 12, 1024, 12, -100, None) == -1
    assert b"null teacher" in _err()


def test_kd_loss_size_queries():
    lib = _lib.load()
    # per workgroup of 1024 pixels: CE numerator, sum of weights, valid, out of range, KL sum, |D|, agreements
    assert lib.cvk_kd_loss_part_floats(1025) == 7 * 2 == 7 * lib.cvk_ce_blocks(1025)
    assert lib.cvk_kd_loss_part_floats(8 * 360 * 480) == 7 * 1350
    assert lib.cvk_kd_loss_part_floats(0) == 0 and lib.cvk_kd_loss_part_floats(-4) == 0
    assert lib.cvk_kd_loss_record_floats() == 9


def test_constructor_validation_and_state_dict():
    w = torch.rand(12) + 0.5
    lf = A.DistillationLoss(1.0, 0.5, 2.0, weight=w, ignore_index=11, distill_ignored=True)
    assert isinstance(lf, torch.nn.Module)
    assert (lf.ce, lf.kd, lf.temperature, lf.distill_ignored, lf.ignore_index, lf.grad_scale) == (1.0, 0.5, 2.0, True, 11, 1.0)
    assert list(lf.state_dict()) == ["weight"] and torch.equal(lf.state_dict()["weight"], w)
    other = A.DistillationLoss(weight=torch.zeros(12))
    other.load_state_dict(lf.state_dict())
    assert torch.equal(other.weight, w)
    d = A.DistillationLoss()
    assert (d.ce, d.kd, d.temperature, d.distill_ignored, d.ignore_index) == (1.0, 1.0, 4.0, False, -100) and d.weight is None
    for bad in (-1.0, NAN, INF):
        with pytest.raises(ValueError, match="ce must be"):
            A.DistillationLoss(ce=bad)
        with pytest.raises(ValueError, match="kd must be"):
            A.DistillationLoss(kd=bad)
    with pytest.raises(ValueError, match="both be 0"):
        A.DistillationLoss(0.0, 0.0)
    for bad in (0.0, -2.0, NAN, INF):
        with pytest.raises(ValueError, match="temperature"):
            A.DistillationLoss(temperature=bad)
        with pytest.raises(ValueError, match="temperature"):
            A.distillation_loss(torch.zeros(1, 3, 2, 2), None, torch.zeros(1, 3, 2, 2), 0.0, 1.0, bad)
    with pytest.raises(ValueError, match="1-D"):
        A.DistillationLoss(weight=torch.ones(3, 4))
    with pytest.raises(RuntimeError, match="no forward"):
        d.last_terms
    with pytest.raises(RuntimeError, match="no forward"):
        d.last_agreement
    with pytest.raises(RuntimeError, match="no forward"):
        d.last_record
    # the attributes are read at every call: a bad assignment is caught at the next call, before anything runs
    d.temperature = 0.0
    with pytest.raises(ValueError, match="temperature"):
        d(torch.zeros(1, 3, 2, 2), None, None)
    # bind: the two-argument form keeps the module and the buffer
    buf = torch.zeros(1, 3, 2, 2)
    bound = lf.bind(buf)
    assert bound.loss is lf and bound.teacher_logits is buf and callable(bound)
    with pytest.raises(ValueError, match="bind"):
        lf.bind(None)
    for name in ("DistillationLoss", "distillation_loss", "distillation_scales"):
        assert name in A.__all__


def test_cpu_tensors_are_refused_loudly():
    x = torch.zeros(1, 3, 2, 2)
    t = torch.zeros(1, 2, 2, dtype=torch.int64)
    for lf in (A.DistillationLoss(), A.DistillationLoss(weight=torch.ones(3)), A.DistillationLoss(0.0, 1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lf(x, t, x.clone())
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lf.bind(x.clone())(x, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.distillation_loss(x, t, x.clone())
