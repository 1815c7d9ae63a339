"""FlatSGD, the parts that need no GPU: the numpy restatement of the update (tests/sgd_ref.py) against torch.optim.SGD in float64, the host
function cvk_sgd_hyper_fill, the argument checks of the two step entry points (refused on the host, before any launch), the constructor's
option checks and GraphedStep's type check."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from . import sgd_ref


# ---- 1. the restatement is torch's SGD ----------------------------------------------------------------------------------------------------
def _combinations():
    for mom, damp, nest, wd in itertools.product((0.0, 0.9), (0.0, 0.3), (False, True), (0.0, 1e-2)):
        if nest and (mom <= 0 or damp != 0):
            continue                                     # torch refuses them
        yield mom, damp, nest, wd


@pytest.mark.parametrize("mom,damp,nest,wd", list(_combinations()))
def test_restatement_is_torch_sgd_in_float64(mom, damp, nest, wd):
    """Four steps with hand-assigned gradients; the third tensor gets its first gradient at step 3 (its buffer is initialised while the
    others' are updated: two records).  Before every step the restatement starts from torch's own state, so both sides evaluate the same
    short expression in fp64 from identical inputs: at most 7 roundings each on any path here (Nesterov excludes dampening, so one of
    the 9 multiplications is by an exact 1), and 16 * 2^-53 of the magnitude sum covers both."""
    rng = np.random.default_rng(5)
    shapes, lr = [(7,), (3, 5), (11,)], 0.05
    params = [torch.tensor(rng.standard_normal(s), dtype=torch.float64, requires_grad=True) for s in shapes]
    opt = torch.optim.SGD(params, lr=lr, momentum=mom, dampening=damp, weight_decay=wd, nesterov=nest)
    sizes = [int(np.prod(s)) for s in shapes]
    offs = [2, 13, 31]                                   # gaps between the tensors and in front of the first
    n = 45
    has_buf = [False] * 3
    tol = 16 * 2.0 ** -53
    for step in range(1, 5):
        live = [0, 1] if step < 3 else [0, 1, 2]
        g = np.zeros(n)
        for i, p in enumerate(params):
            if i in live:
                gi = rng.standard_normal(shapes[i]) * 10.0 ** rng.integers(-3, 2)
                p.grad = torch.tensor(gi, dtype=torch.float64)
                g[offs[i]:offs[i] + sizes[i]] = gi.ravel()
            else:
                p.grad = None
        flat = np.full(n, np.nan)
        buf = np.full(n, np.nan)
        for i, p in enumerate(params):
            flat[offs[i]:offs[i] + sizes[i]] = p.detach().numpy().ravel()
            b = opt.state[p].get("momentum_buffer") if p in opt.state else None
            assert (b is not None) == has_buf[i]
            if b is not None:
                buf[offs[i]:offs[i] + sizes[i]] = b.numpy().ravel()
        # exact inputs: the hyper-parameters as python floats, not rounded to float32 (torch takes them as doubles)
        keys, records, ranges = {}, [], []
        for i in live:
            first = mom != 0 and not has_buf[i]
            if first not in keys:
                keys[first] = len(records)
                records.append(sgd_ref.Record(lr, mom, damp, wd, nest, first))
            ranges.append((offs[i], sizes[i], keys[first]))
        if mom != 0:
            assert len(records) == (2 if step == 3 else 1)
        want = sgd_ref.sgd_step(flat, g, buf if mom != 0 else None, None, ranges, records)
        opt.step()
        for i, p in enumerate(params):
            s = slice(offs[i], offs[i] + sizes[i])
            if i not in live:
                assert not want.covered[s].any() and np.array_equal(p.detach().numpy().ravel(), flat[s])
                continue
            if mom != 0:
                has_buf[i] = True
            err = np.abs(p.detach().numpy().ravel() - want.p[s])
            assert np.all(err <= tol * want.S_p[s]), (step, i, float((err / want.S_p[s]).max()) / 2.0 ** -53)
            if mom != 0:
                b = opt.state[p]["momentum_buffer"].numpy().ravel()
                errb = np.abs(b - want.buf[s])
                assert np.all(errb <= tol * want.S_b[s]), (step, i)
            else:
                assert "momentum_buffer" not in opt.state[p] or opt.state[p]["momentum_buffer"] is None
        u = ~want.covered                                # the gaps and the dormant tensor come back as they went in
        assert np.array_equal(want.p[u], flat[u], equal_nan=True) and np.isnan(want.p[:2]).all()


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("ema", [False, True])
@pytest.mark.parametrize("mom", [False, True])
def test_float32_restatement_stays_inside_the_derived_bounds(clip, ema, mom):
    """The assertions of the GPU value check (sgd_ref.check_case), on the reference's own float32 evaluation of the same inputs (one
    rounding per operation, nothing contracted): the inputs leave no element outside the bounds."""
    p, g, buf, e = sgd_ref.case_inputs()
    coef = float(np.float32(sgd_ref.CASE_CLIP[1])) if clip else 1.0
    alpha = float(np.float32(sgd_ref.CASE_ALPHA)) if ema else None
    got = sgd_ref.sgd_step(p, g, buf if mom else None, e if ema else None, sgd_ref.CASE_RANGES, sgd_ref.case_records(mom), coef, alpha,
                           np.float32)
    assert got.p.dtype == np.float32
    sgd_ref.check_case(got.p, got.buf if mom else buf, got.ema if ema else e, clip, ema, mom, f"float32 numpy clip={clip} ema={ema} mom={mom}")
    if mom:
        want = sgd_ref.sgd_step(p, g, buf, None, sgd_ref.CASE_RANGES, sgd_ref.case_records(True), coef, None)
        assert float(np.abs(got.p[want.covered] - want.p[want.covered]).max()) > 0       # float32 really rounded somewhere


# ---- 2. cvk_sgd_hyper_fill ------------------------------------------------------------------------------------------------------------------
def _refused(lib, rc, name, word):
    msg = lib.cvk_last_error_string().decode()
    assert rc == -1 and msg.startswith(name + ":") and word in msg, (name, rc, msg)


def test_sgd_hyper_fill_fields_and_refusals():
    from pytorch_camvid_amd import _lib as L
    lib = L.load()
    assert ctypes.sizeof(L.SgdHyper) == ctypes.sizeof(L.AdamwHyper) == 28
    assert L.SgdHyper.lr.offset == 0 and L.SgdHyper.momentum.offset == 4       # what cvk_step_log reads as lr and beta1
    f32 = lambda x: float(np.float32(x))
    h = L.SgdHyper()
    for i in range(7):
        (ctypes.c_float * 7).from_buffer(h)[i] = -7.0                           # every field must be written
    assert lib.cvk_sgd_hyper_fill(0.05, 0.9, 0.3, 1e-2, 0, 1, ctypes.addressof(h)) == 0
    assert (h.lr, h.momentum, h.dampening, h.weight_decay) == (f32(0.05), f32(0.9), f32(0.3), f32(1e-2))
    assert (h.nesterov, h.first, h.reserved) == (0.0, 1.0, 0.0)
    assert lib.cvk_sgd_hyper_fill(0.0, 0.99, 0.0, 0.0, 1, 0, ctypes.addressof(h)) == 0
    assert (h.lr, h.momentum, h.dampening, h.weight_decay, h.nesterov, h.first, h.reserved) == (0.0, f32(0.99), 0.0, 0.0, 1.0, 0.0, 0.0)
    assert lib.cvk_sgd_hyper_fill(1e-3, 0.0, 0.3, 0.0, 0, 0, ctypes.addressof(h)) == 0     # dampening without momentum: torch allows it
    assert (h.momentum, h.dampening, h.nesterov, h.first) == (0.0, f32(0.3), 0.0, 0.0)
    name = "cvk_sgd_hyper_fill"
    a = ctypes.addressof(h)
    _refused(lib, lib.cvk_sgd_hyper_fill(0.1, 0.9, 0.0, 0.0, 0, 0, None), name, "null")
    for bad in (-1e-3, float("nan")):
        _refused(lib, lib.cvk_sgd_hyper_fill(bad, 0.9, 0.0, 0.0, 0, 0, a), name, "lr")
        _refused(lib, lib.cvk_sgd_hyper_fill(0.1, bad, 0.0, 0.0, 0, 0, a), name, "momentum")
        _refused(lib, lib.cvk_sgd_hyper_fill(0.1, 0.9, 0.0, bad, 0, 0, a), name, "weight_decay")
    _refused(lib, lib.cvk_sgd_hyper_fill(0.1, 0.0, 0.0, 0.0, 1, 0, a), name, "nesterov")
    _refused(lib, lib.cvk_sgd_hyper_fill(0.1, 0.9, 0.3, 0.0, 1, 0, a), name, "nesterov")
    _refused(lib, lib.cvk_sgd_hyper_fill(0.1, 0.9, float("nan"), 0.0, 1, 0, a), name, "nesterov")


# ---- 3. the step entry points refuse bad arguments before any launch ----------------------------------------------------------------------
def test_sgd_entry_points_refuse_bad_arguments_before_any_launch():
    from pytorch_camvid_amd import _lib as L
    lib = L.load()
    p = 4096                                                  # never dereferenced: every call is refused on the host
    eager, captured = "cvk_sgd_step_ranges", "cvk_sgd_step_ranges_dev"
    # null pointers.  A null ema is the step without an average, a null momentum buffer the buffer-free step and a null clip record the
    # unclipped step: none of them is refused as such; every other buffer is, and so is an average whose device alpha is null
    _refused(lib, lib.cvk_sgd_step_ranges(None, p, p, None, 8, p, 1, 1, p, 1, None, 0.1, None), eager, "null")
    _refused(lib, lib.cvk_sgd_step_ranges(p, None, p, p, 8, p, 1, 1, p, 1, p, 0.1, None), eager, "null")
    _refused(lib, lib.cvk_sgd_step_ranges(p, p, p, p, 8, None, 1, 1, p, 1, p, 0.1, None), eager, "null")
    _refused(lib, lib.cvk_sgd_step_ranges(p, p, None, p, 8, p, 1, 1, None, 1, p, 0.1, None), eager, "null")
    _refused(lib, lib.cvk_sgd_step_ranges_dev(None, p, p, None, 8, p, 1, 1, p, 1, None, p, 0.1, None), captured, "null")
    _refused(lib, lib.cvk_sgd_step_ranges_dev(p, None, None, None, 8, p, 1, 1, p, 1, None, p, 0.1, None), captured, "null")
    _refused(lib, lib.cvk_sgd_step_ranges_dev(p, p, p, None, 8, p, 1, 1, None, 1, None, p, 0.1, None), captured, "null")
    _refused(lib, lib.cvk_sgd_step_ranges_dev(p, p, p, p, 8, p, 1, 1, p, 1, p, None, 0.1, None), captured, "null")
    # alpha outside (0, 1], with and without a clip record, with and without a momentum buffer
    for alpha in (0.0, 1.5, -0.25, float("nan")):
        for rec in (None, p):
            for buf in (None, p):
                _refused(lib, lib.cvk_sgd_step_ranges(p, p, buf, p, 8, p, 1, 1, p, 1, rec, alpha, None), eager, "alpha")
                _refused(lib, lib.cvk_sgd_step_ranges_dev(p, p, buf, p, 8, p, 1, 1, p, 1, rec, p, alpha, None), captured, "alpha")
    # the record limit of the kernel-argument form; an empty table in both
    _refused(lib, lib.cvk_sgd_step_ranges(p, p, p, p, 8, p, 1, 1, p, L.ADAMW_ARG_RECORDS + 1, None, 0.1, None), eager, "records")
    _refused(lib, lib.cvk_sgd_step_ranges(p, p, p, p, 8, p, 0, 0, p, 1, None, 0.1, None), eager, "bad arguments")
    _refused(lib, lib.cvk_sgd_step_ranges_dev(p, p, p, p, 8, p, 0, 0, p, 1, None, p, 0.1, None), captured, "bad arguments")
    # a null momentum buffer with a record that has a momentum (the host array is real here: it is read), also behind a record without
    recs = (L.SgdHyper * 2)()
    assert lib.cvk_sgd_hyper_fill(0.1, 0.0, 0.0, 0.0, 0, 0, ctypes.addressof(recs)) == 0
    assert lib.cvk_sgd_hyper_fill(0.1, 0.9, 0.0, 0.0, 0, 0, ctypes.addressof(recs) + ctypes.sizeof(L.SgdHyper)) == 0
    _refused(lib, lib.cvk_sgd_step_ranges(p, p, None, None, 8, p, 1, 1, ctypes.addressof(recs), 2, None, 0.0, None), eager, "momentum")
    _refused(lib, lib.cvk_sgd_step_ranges(p, p, None, p, 8, p, 1, 1, ctypes.addressof(recs) + ctypes.sizeof(L.SgdHyper), 1, p, 0.5, None),
             eager, "momentum")


# ---- 4. the constructor ---------------------------------------------------------------------------------------------------------------------
def test_sgd_options_are_checked_before_the_device():
    import pytorch_camvid_amd as A
    net = A.UNet(3, 12)
    for kw in (dict(lr=-1e-3), dict(momentum=-0.1), dict(weight_decay=-1e-4), dict(lr=float("nan")),
               dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1), dict(nesterov=True, momentum=0.0)):
        with pytest.raises(ValueError):
            A.FlatSGD(net, **kw)
    with pytest.raises(ValueError, match="ema_decay"):
        A.FlatSGD(net, momentum=0.9, ema_decay=1.0)
    with pytest.raises(ValueError, match="norm_type"):
        A.FlatSGD(net, momentum=0.9, max_grad_norm=1.0, norm_type=3)
    assert all(not p.is_cuda for p in net.parameters())
    for kw in (dict(), dict(lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4), dict(momentum=0.99, dampening=0.3, ema_decay=0.999),
               dict(momentum=0.9, max_grad_norm=1.0, ema_decay=0.0, ema_warmup=True)):
        with pytest.raises(RuntimeError, match="GPU"):                   # valid options: the next check is the device
            A.FlatSGD(A.UNet(3, 12), **kw)
    assert issubclass(A.FlatSGD, torch.optim.Optimizer) and issubclass(A.FlatAdamW, torch.optim.Optimizer)


# ---- 5. GraphedStep's type check ------------------------------------------------------------------------------------------------------------
def test_graphedstep_still_refuses_torch_optimizers():
    import pytorch_camvid_amd as A
    net = A.UNet(3, 12)
    x, t = torch.zeros(1, 3, 16, 16), torch.zeros(1, 16, 16, dtype=torch.long)
    for opt in (torch.optim.AdamW(net.parameters(), lr=1e-3), torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9)):
        with pytest.raises(TypeError, match="only FlatAdamW"):
            A.GraphedStep(net, A.CrossEntropyLoss(), x, t, optimizer=opt)
