"""CPU-side checks of the distance transform and the boundary loss: the scipy form of tests/edt_ref.py against its brute-force form,
the argument checks of the seven entry points before any launch (called with dummy pointers), the size functions, the Python surface
(names, defaults, refusals, the coefficient properties) and the fp64 loss's analytic gradient against torch autograd."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import edt_ref as R
from tests.boundary_ref import blocky_maps

K, IGN = 12, 11
P = 4096                                   # a dummy non-null, 16-byte aligned pointer: every call below fails before any launch


def _tiny_maps():
    maps = []
    for H, W in ((1, 1), (1, 9), (7, 1), (5, 7), (9, 11)):
        _, lab = blocky_maps(10 * H + W, 2, H, W, cell=(3, 4), void=0.1)
        maps += [(f"blocky {H}x{W} #{n}", m) for n, m in enumerate(lab)]
        maps += [(f"{name} {H}x{W}", m) for name, m in R.special_maps(H, W, K, IGN).items()]
    return maps


def test_scipy_form_equals_brute_force_on_tiny_maps():
    pytest.importorskip("scipy.ndimage")
    seen_minus = seen_far = False
    for name, m in _tiny_maps():
        a, b = R.squared_maps(m, K, IGN)
        c, d = R.squared_maps_brute(m, K, IGN)
        assert np.array_equal(a, c), name
        assert np.array_equal(b, d), name
        seen_minus |= bool((b < 0).any())
        seen_far |= bool(a.max() >= 64)
    assert seen_minus and seen_far


def test_hand_worked_maps():
    m = np.array([[0, 0, 1],
                  [0, IGN, 1]], dtype=np.int64)
    tc, to = R.squared_maps_brute(m, K, IGN)
    assert tc[:, :, 0].tolist() == [[0, 0, 1], [0, 1, 2]]
    assert tc[:, :, 1].tolist() == [[4, 1, 0], [4, 1, 0]]
    assert (tc[:, :, 2:] == -1).all()                      # absent classes, the ignored class among them
    assert to.tolist() == [[2, 1, 1], [1, 1, 1]]           # the void pixel differs from both classes, and they from it
    phi = R.signed_from_squared(m, tc, to, K, IGN)
    r2 = np.sqrt(np.float32(2))
    assert phi[0].tolist() == [[-(r2 - 1), 0.0, 1.0], [0.0, 1.0, r2]]
    assert phi[1].tolist() == [[2.0, 1.0, 0.0], [2.0, 1.0, 0.0]]
    assert not phi[2:].any()
    one = np.full((3, 4), 5, dtype=np.int64)
    tc, to = R.squared_maps(one, K, IGN)
    assert (tc[:, :, 5] == 0).all() and (np.delete(tc, 5, axis=2) == -1).all() and (to == -1).all()
    assert not R.signed_from_squared(one, tc, to, K, IGN).any()


def _lib():
    from pytorch_camvid_amd import _lib
    return _lib.load()


def _refused(rc, lib, *words):
    msg = lib.cvk_last_error_string().decode()
    assert rc == -1 and all(w in msg for w in words), (rc, msg)


def test_edt_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib()
    for name, call in (("cvk_edt_squared", lambda lab, N, H, W, C, ws: lib.cvk_edt_squared(lab, N, H, W, C, IGN, ws, P, P, None)),
                       ("cvk_edt_signed", lambda lab, N, H, W, C, ws: lib.cvk_edt_signed(lab, N, H, W, C, IGN, ws, P, None))):
        _refused(call(None, 1, 8, 8, K, P), lib, name, "null pointer")
        _refused(call(P, 1, 8, 8, K, None), lib, name, "null pointer")
        _refused(call(P, 0, 8, 8, K, P), lib, name, "sizes must be positive")
        _refused(call(P, 1, -8, 8, K, P), lib, name, "sizes must be positive")
        _refused(call(P, 1, 8, 0, K, P), lib, name, "sizes must be positive")
        _refused(call(P, 1, 8, 8, 0, P), lib, name, "0 classes", "1 to 32")
        _refused(call(P, 1, 8, 8, 33, P), lib, name, "33 classes", "1 to 32")
        _refused(call(P, 1, 65535, 1, K, P), lib, name, "H 65535", "16 bits")
        _refused(call(P, 1, 2898, 2898, K, P), lib, name, "below 2^24")            # 2 * 2897^2 = 16785218 >= 2^24
        _refused(call(P, 1, 1, 4097, K, P), lib, name, "below 2^24")               # 4096^2 = 2^24
        _refused(call(P, 2048, 1024, 1024, K, P), lib, name, "2^31 pixels")
        _refused(call(P, 1, 8, 8, K, P + 8), lib, name, "16-byte aligned")
    _refused(lib.cvk_edt_squared(P, 1, 8, 8, K, IGN, P, None, P, None), lib, "null pointer")
    _refused(lib.cvk_edt_squared(P, 1, 8, 8, K, IGN, P, P, None, None), lib, "null pointer")
    _refused(lib.cvk_edt_signed(P, 1, 8, 8, K, IGN, P, None, None), lib, "null pointer")


def test_boundary_loss_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib()
    full = (1 << K) - 1

    def fwd(logits=P, ld=K, target=P, phi=P, weight=None, coef=P, wb=1, wc=0, mask=full, part=P, rec=P, M=100, C=K):
        return lib.cvk_boundary_loss_fwd(logits, ld, target, phi, weight, coef, wb, wc, mask, part, rec, M, C, -100, None)

    def bwd(logits=P, ld=K, target=P, phi=P, weight=None, wb=1, wc=0, mask=full, rec=P, d=P, ld_d=K, M=100, C=K):
        return lib.cvk_boundary_loss_bwd(logits, ld, target, phi, weight, wb, wc, mask, rec, None, 1.0, d, ld_d, M, C, -100, None)

    for who, f in (("cvk_boundary_loss_fwd", fwd), ("cvk_boundary_loss_bwd", bwd)):
        for arg in ("logits", "target", "rec"):
            _refused(f(**{arg: None}), lib, who, "null pointer")
        _refused(f(phi=None), lib, who, "null pointer", "distance maps")
        _refused(f(M=0), lib, who, "sizes must be positive")
        _refused(f(C=0, ld=4), lib, who, "0 classes")
        _refused(f(C=33, ld=36), lib, who, "33 classes")
        _refused(f(ld=K - 1), lib, who, "pixel stride")
        _refused(f(ld=64), lib, who, "pixel stride")
        _refused(f(wb=0, wc=0), lib, who, "not both 0")
        _refused(f(wb=2), lib, who, "must be 0 or 1")
        _refused(f(mask=0), lib, who, "class mask")
        _refused(f(mask=1 << K), lib, who, "class mask")
        _refused(f(weight=P), lib, who, "class weights enter the cross-entropy term only")
    _refused(fwd(coef=None), lib, "null pointer")
    _refused(fwd(part=None), lib, "null pointer")
    _refused(bwd(d=None), lib, "null pointer")
    _refused(bwd(ld_d=K - 1), lib, "gradient's pixel stride")


def test_workspace_and_record_sizes():
    lib = _lib()
    M = 8 * 360 * 480
    assert lib.cvk_edt_workspace_bytes(8, 360, 480, K) >= 2 * M * (K + 1) + 8 * 8
    assert lib.cvk_edt_workspace_bytes(8, 360, 480, K) < 2 * M * (K + 1) + 4096
    sizes = [lib.cvk_edt_workspace_bytes(n, h, w, c) for n, h, w, c in ((1, 1, 1, 1), (1, 5, 7, 1), (1, 5, 7, 2), (2, 5, 7, 2), (2, 6, 7, 2),
                                                                       (2, 6, 8, 32))]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    for bad in ((0, 8, 8, K), (1, 8, 8, 0), (1, 8, 8, 33), (1, 65535, 1, K), (1, 1, 4097, K), (2048, 1024, 1024, K)):
        assert lib.cvk_edt_workspace_bytes(*bad) == 0, bad
    assert lib.cvk_edt_workspace_bytes(1, 4096, 1, K) > 0 and lib.cvk_edt_workspace_bytes(1, 1, 4096, K) > 0
    assert lib.cvk_boundary_loss_record_floats() == 8 + 32
    parts = [lib.cvk_boundary_loss_part_floats(m, c) for m, c in ((1, 1), (1024, 1), (1025, 1), (1025, 12), (M, 12), (M, 32))]
    assert all(p > 0 for p in parts) and parts == sorted(parts)
    assert lib.cvk_boundary_loss_part_floats(1025, 12) == (4 + 12) * lib.cvk_ce_blocks(1025)
    assert lib.cvk_boundary_loss_part_floats(0, 12) == 0 and lib.cvk_boundary_loss_part_floats(10, 33) == 0


def test_python_surface():
    import pytorch_camvid_amd as A
    for name in ("BoundaryLoss", "boundary_loss", "squared_distance_maps", "signed_distance_maps"):
        assert name in A.__all__ and hasattr(A, name), name
    sig = inspect.signature(A.BoundaryLoss.__init__).parameters
    assert [(k, v.default) for k, v in sig.items() if k != "self"] == [("boundary", 1.0), ("ce", 0.0), ("classes", None), ("weight", None),
                                                                       ("ignore_index", -100), ("grad_scale", 1.0)]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("classes", "weight", "ignore_index", "grad_scale"))
    for f in (A.squared_distance_maps, A.signed_distance_maps):
        s = inspect.signature(f).parameters
        assert [(k, v.default) for k, v in s.items()][1:] == [("num_classes", 12), ("ignore_index", 11)]
    lf = A.BoundaryLoss()
    assert lf.boundary == 1.0 and lf.ce == 0.0 and lf.classes is None and lf.ignore_index == -100 and lf.grad_scale == 1.0
    assert lf.coef.tolist() == [1.0, 0.0] and "coef" in dict(lf.named_buffers()) and lf.weight is None
    with pytest.raises(RuntimeError, match="no forward has run yet"):
        lf.last_terms


@pytest.mark.parametrize("kwargs,match", [
    (dict(boundary=-1.0), "boundary must be a finite number"),
    (dict(boundary=float("inf")), "boundary must be a finite number"),
    (dict(ce=float("nan")), "ce must be a finite number"),
    (dict(boundary=0.0, ce=0.0), "no term"),
    (dict(classes=[]), "non-empty sequence"),
    (dict(classes=[1, 1]), "distinct"),
    (dict(classes=[0, 32]), "class indices"),
    (dict(classes=[-1]), "class indices"),
    (dict(classes=[1.5]), "class indices"),
    (dict(boundary=0.0, ce=1.0, classes=[1]), "boundary is 0"),
    (dict(weight=torch.ones(12)), "needs ce > 0"),
    (dict(ce=1.0, weight=torch.ones(3, 4)), "1-D tensor"),
    (dict(ce=1.0, weight=[1.0] * 12), "1-D tensor"),
])
def test_constructor_and_functional_refusals(kwargs, match):
    import pytorch_camvid_amd as A
    with pytest.raises(ValueError, match=match):
        A.BoundaryLoss(**kwargs)
    with pytest.raises(ValueError, match=match):
        A.boundary_loss(torch.zeros(1, 12, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), **kwargs)


def test_coefficient_properties_fill_the_buffer_and_fixed_terms_stay_fixed():
    import pytorch_camvid_amd as A
    lf = A.BoundaryLoss(0.01, 1.0)
    lf.boundary = 0.25
    lf.ce = 0.5
    assert lf.coef.tolist() == [0.25, 0.5] and (lf.boundary, lf.ce) == (0.25, 0.5)
    lf.boundary = 0.0                                      # lowering to 0 is allowed: the term is still computed, times 0
    lf.boundary = 1.0
    assert lf.coef.tolist() == [1.0, 0.5]
    with pytest.raises(ValueError, match="finite number"):
        lf.ce = -1.0
    only_b = A.BoundaryLoss(1.0, 0.0)
    with pytest.raises(ValueError, match="ce was 0 at construction"):
        only_b.ce = 0.1
    only_b.ce = 0.0
    only_h = A.BoundaryLoss(0.0, 1.0)
    with pytest.raises(ValueError, match="boundary was 0 at construction"):
        only_h.boundary = 0.01
    assert only_b.coef.tolist() == [1.0, 0.0] and only_h.coef.tolist() == [0.0, 1.0]
    sd = A.BoundaryLoss(0.3, 0.7, weight=torch.ones(12)).state_dict()
    assert sorted(sd) == ["coef", "weight"] and sd["coef"].tolist() == pytest.approx([0.3, 0.7])


def test_cpu_tensors_and_bad_label_maps_are_refused():
    import pytorch_camvid_amd as A
    lab = torch.zeros(2, 5, 7, dtype=torch.int64)
    for f in (A.squared_distance_maps, A.signed_distance_maps):
        with pytest.raises(ValueError, match="on the GPU"):
            f(lab)
        for bad in (lab.int(), lab[0], lab[:, :0], lab.numpy(), None):
            with pytest.raises(ValueError, match=r"int64 tensor of shape \[N, H, W\]"):
                f(bad)
        for k in (0, 33, 12.0, True):
            with pytest.raises(ValueError, match="1 to 32 classes"):
                f(lab, num_classes=k)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.BoundaryLoss()(torch.zeros(2, 12, 5, 7), lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.boundary_loss(torch.zeros(2, 12, 5, 7), lab)


@pytest.mark.parametrize("classes,ce,weighted", [(None, 0.0, False), ([0, 2, 3], 0.0, False), (None, 0.6, True), ([1, 4], 0.3, False)])
def test_fp64_gradient_is_torch_autograd_of_the_same_formula(classes, ce, weighted):
    pytest.importorskip("scipy.ndimage")
    N, C, H, W, ign = 2, 5, 9, 11, -100
    rng = np.random.default_rng(5)
    _, lab = blocky_maps(3, N, H, W, K=C, ignore=ign, cell=(3, 4), void=0.15)
    phi = R.batch_maps(lab, C, ign)[2]
    x = 2 * rng.standard_normal((N, C, H, W))
    w = rng.random(C) * 2 + 0.1 if weighted else None
    got = R.loss_and_grad(x, lab, phi, boundary=0.7, ce=ce, classes=classes, weight=w, ignore=ign)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    p = torch.softmax(xt, dim=1)
    valid = torch.tensor(lab != ign)
    S = torch.zeros(C, dtype=torch.float64)
    S[list(range(C)) if classes is None else classes] = 1.0
    f = torch.tensor(phi, dtype=torch.float64) * S[None, :, None, None]
    B = (f * p * valid[:, None]).sum() / valid.sum()
    loss = 0.7 * B
    if ce > 0:
        loss = loss + ce * torch.nn.functional.cross_entropy(xt, torch.tensor(lab), weight=None if w is None else torch.tensor(w),
                                                             ignore_index=ign)
    loss.backward()
    assert got["valid"] == int(valid.sum()) and 0 < got["valid"] < N * H * W
    assert got["loss"] == pytest.approx(loss.item(), rel=1e-12)
    assert got["B"] == pytest.approx(B.item(), rel=1e-12) and got["class_terms"].sum() == pytest.approx(got["B"], rel=1e-12)
    assert np.abs(got["grad"] - xt.grad.numpy()).max() <= 1e-12 * np.abs(xt.grad.numpy()).max()
    assert not got["grad"][np.broadcast_to(~valid.numpy()[:, None], x.shape)].any()
    none = R.loss_and_grad(x, np.full_like(lab, ign), phi, boundary=0.7, ignore=ign)
    assert none["loss"] == 0.0 and not none["grad"].any()
