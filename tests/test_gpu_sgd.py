"""FlatSGD on the GPU.  Kernel level: cvk_sgd_step_ranges / cvk_sgd_step_ranges_dev on raw buffers against tests/sgd_ref.py (the case, its
derived bounds and its assertions live there, and tests/test_sgd_cpu.py runs the same assertions on the reference's own float32
evaluation).  Network level, UNet(3, 12) at 2 x 3 x 48 x 64: against torch.optim.SGD on identical gradients, after real backward passes,
the captured iteration against the eager loop bit for bit, a late start, accumulation windows and the state-dict round trip.

Bound against torch.optim.SGD (both sides fp32 evaluations of the same expression from the same inputs): per step twice the per-step
bound 10 u S_p of sgd_ref.bounds, summed over the steps so far; the errors already in p and in the buffer are carried on by the factors
|1 - lr wd|, momentum and lr * momentum, all at most 1 at the settings used here."""
import ctypes

import numpy as np
import pytest
import torch

from . import sgd_ref

pytestmark = pytest.mark.gpu

SHAPE = (2, 48, 64)
ENCODER = ("down1", "down2", "down3", "down4", "down5")


def dev():
    return torch.device("cuda:0")


def _f32(x):
    return float(np.float32(x))


# ---- kernel level ----------------------------------------------------------------------------------------------------------------------------
def _records(L, lib, recs):
    arr = (L.SgdHyper * len(recs))()
    for k, r in enumerate(recs):
        L.check(lib.cvk_sgd_hyper_fill(r.lr, r.momentum, r.dampening, r.weight_decay, int(r.nesterov), int(r.first),
                                       ctypes.addressof(arr) + k * ctypes.sizeof(L.SgdHyper)), "cvk_sgd_hyper_fill")
    return arr


def _case_table(L, lib, nrec):
    """The case's range table on the device.  cvk_adamw_plan_ranges checks it against the buffer (every range inside [0, n), every record
    index valid); the workgroups are then the case's own: at this size the planner never gives a range fewer workgroups than it has
    256-element pieces, and the stride loop's second trip would go untested."""
    R = sgd_ref
    arr = (L.AdamwRange * len(R.CASE_RANGES))(*[L.AdamwRange(o, m, r, 0) for o, m, r in R.CASE_RANGES])
    assert lib.cvk_adamw_plan_ranges(ctypes.addressof(arr), len(R.CASE_RANGES), R.CASE_N, nrec) > 0
    for e, b0 in zip(arr, R.CASE_BLOCK0):
        e.block0 = b0
    assert all(0 <= e.offset and e.offset + e.length <= R.CASE_N for e in arr) and R.CASE_BLOCKS > R.CASE_BLOCK0[-1]
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev())


def _run_case(clip, ema, mom, dev_form, recs=None, with_buf=None):
    """One step of the case through the argument form or the device-record form; returns (p, buf, ema) as float32 numpy arrays (buf and ema
    are the buffers as they are afterwards, handed to the kernel or not)."""
    from pytorch_camvid_amd import _lib as L
    lib = L.load()
    R = sgd_ref
    recs = R.case_records(mom) if recs is None else recs
    with_buf = mom if with_buf is None else with_buf
    p, g, buf, e = [torch.from_numpy(a).to(dev()) for a in R.case_inputs()]
    table = _case_table(L, lib, len(recs))
    hyper = _records(L, lib, recs)
    rec = torch.tensor(R.CASE_CLIP, dtype=torch.float32, device=dev()) if clip else None
    stream = torch.cuda.current_stream().cuda_stream
    head = (p.data_ptr(), g.data_ptr(), buf.data_ptr() if with_buf else None, e.data_ptr() if ema else None, R.CASE_N, table.data_ptr(),
            len(R.CASE_RANGES), R.CASE_BLOCKS)
    if dev_form:
        hdev = torch.from_numpy(np.frombuffer(bytes(hyper), np.float32).copy()).to(dev())
        adev = torch.tensor([R.CASE_ALPHA], dtype=torch.float32, device=dev())
        L.check(lib.cvk_sgd_step_ranges_dev(*head, hdev.data_ptr(), len(recs), rec.data_ptr() if clip else None, adev.data_ptr() if ema else None,
                                            R.CASE_ALPHA, stream), "cvk_sgd_step_ranges_dev")
    else:
        L.check(lib.cvk_sgd_step_ranges(*head, ctypes.addressof(hyper), len(recs), rec.data_ptr() if clip else None, R.CASE_ALPHA, stream),
                "cvk_sgd_step_ranges")
    torch.cuda.synchronize()
    return p.cpu().numpy(), buf.cpu().numpy(), e.cpu().numpy()


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("ema", [False, True])
@pytest.mark.parametrize("mom", [False, True])
def test_range_step_against_the_reference_and_both_forms_bitwise(clip, ema, mom):
    a = _run_case(clip, ema, mom, False)
    b = _run_case(clip, ema, mom, True)
    for x, y, name in zip(a, b, ("param", "buf", "ema")):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{name}: argument form and device-record form differ"
    sgd_ref.check_case(*a, clip, ema, mom, f"gfx950 clip={clip} ema={ema} mom={mom}")


def test_a_record_without_momentum_leaves_its_ranges_of_the_buffer_alone():
    """A buffer is handed over (another group needs it) but record 1 has momentum 0: torch keeps no buffer for that group, and its ranges
    of `buf` come back bit for bit; the update of those ranges is the buffer-free one."""
    R = sgd_ref
    recs = R.case_records(True)
    recs[1] = R.record(0.03, 0.0, 0.3, 1e-2, False, False)
    p0, g0, buf0, e0 = R.case_inputs()
    for dev_form in (False, True):
        p, buf, e = _run_case(True, True, True, dev_form, recs=recs)
        coef, alpha = _f32(R.CASE_CLIP[1]), _f32(R.CASE_ALPHA)
        want = R.sgd_step(p0, g0, buf0, e0, R.CASE_RANGES, recs, coef, alpha)
        bp, bb, be = R.bounds(want, e0, alpha)
        c, ub = want.covered, want.used_buf
        assert ub.any() and (c & ~ub).any()
        assert np.array_equal(buf.view(np.uint32)[~ub], buf0.view(np.uint32)[~ub])
        assert np.all(np.abs(p[c] - want.p[c]) <= bp[c]) and np.all(np.abs(buf[ub] - want.buf[ub]) <= bb[ub])
        assert np.all(np.abs(e[c] - want.ema[c]) <= be[c])
        assert np.array_equal(p.view(np.uint32)[~c], p0.view(np.uint32)[~c]) and np.array_equal(e.view(np.uint32)[~c], e0.view(np.uint32)[~c])


# ---- network level -----------------------------------------------------------------------------------------------------------------------------
def _batch(seed, shape=SHAPE):
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, h, w, generator=g).to(dev()), torch.randint(0, 12, (n, h, w), generator=g).to(dev())


def _backward(A, net, seed):
    for p in net.parameters():
        p.grad = None
    x, t = _batch(seed)
    A.CrossEntropyLoss()(net(x), t).backward()


def _twin_nets(A, n=2, seed=0, classes=12):
    torch.manual_seed(seed)
    nets = [A.UNet(3, classes).to(dev()).train()]
    for _ in range(n - 1):
        other = A.UNet(3, classes).to(dev()).train()
        other.load_state_dict(nets[0].state_dict())
        nets.append(other)
    return nets


def _random_grads(nets, seed, scale=1e-2):
    """The same random gradient into .grad of every twin's trainable parameters (fresh tensors: the optimizer gathers them into its own
    flat buffer); the others get None."""
    g = torch.Generator(device=dev()).manual_seed(seed)
    for ps in zip(*[net.parameters() for net in nets]):
        gr = torch.randn(ps[0].shape, generator=g, device=dev()) * scale
        for p in ps:
            p.grad = gr.clone() if p.requires_grad else None


def _flatten(opt, params):
    """`params` (in the order of opt._plist) gathered into the optimizer's flat layout."""
    out = torch.zeros_like(opt._flat)
    for p, o in zip(params, opt._offs):
        q = p.detach().permute(0, 2, 3, 1) if p.dim() == 4 else p.detach()
        out[o:o + p.numel()] = q.reshape(-1)
    return out


def _bound_p(opt, idx, g, coef=1.0):
    """10 u S_p of the step `opt` is about to take over the parameters `idx` with the flat gradient g, as a flat float64 device tensor (0
    outside the step's ranges): sgd_ref's magnitude sums, evaluated on the device (34.5 M elements)."""
    recs, ranges = opt._ranges(idx)
    out = torch.zeros(opt._flat.numel(), dtype=torch.float64, device=dev())
    for o, m, r in ranges:
        gi, i = recs[r]
        grp = opt.param_groups[gi]
        lr, mom, damp, wd = (_f32(grp[k]) for k in ("lr", "momentum", "dampening", "weight_decay"))
        s = slice(o, o + m)
        pa = opt._flat[s].double().abs()
        a_d = g[s].double().abs() * abs(coef) + wd * pa
        if mom != 0.0:
            a_b = mom * opt._buf[s].double().abs() + abs(1.0 - damp) * a_d if opt._has_buf[i] else a_d
            a_d = a_d + mom * a_b if grp["nesterov"] else a_b
        out[s] = 10 * sgd_ref.U32 * (pa + lr * a_d)
    return out


def _against_torch(A, nesterov, freeze_steps=0, steps=3):
    from pytorch_camvid_amd import optim
    a, b = _twin_nets(A)
    kw = dict(lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=nesterov)
    for net in (a, b):
        if freeze_steps:
            for name in ENCODER:
                getattr(net, name).requires_grad_(False)
    oa = A.FlatSGD(a, ema_decay=0.9 if freeze_steps else None, **kw)
    ob = torch.optim.SGD(b.parameters(), **kw)
    sa, sb = [torch.optim.lr_scheduler.OneCycleLR(o, max_lr=0.05, total_steps=steps + 4) for o in (oa, ob)]
    assert oa._buf is not None and not any(oa._has_buf)
    frozen = torch.zeros(oa._flat.numel(), dtype=torch.bool, device=dev())
    for p, o in zip(oa._plist, oa._offs):
        if not p.requires_grad:
            frozen[o:o + p.numel()] = True
    assert bool(frozen.any()) == bool(freeze_steps)
    if freeze_steps:                                    # whatever a frozen parameter has in the buffer and the average is never read either
        oa._buf.view(torch.int32)[frozen] = sgd_ref.NAN_BITS
        oa._ema.view(torch.int32)[frozen] = sgd_ref.NAN_BITS
    start = [t.clone() for t in (oa._flat, oa._buf, oa._ema if freeze_steps else oa._buf)]
    bparams = optim._block_params(b)
    tol = torch.zeros(oa._flat.numel(), dtype=torch.float64, device=dev())
    momenta = []
    for it in range(steps):
        if freeze_steps and it == freeze_steps:
            for x, y, z in zip((oa._flat, oa._buf, oa._ema), start, ("param", "buf", "ema")):
                assert torch.equal(x.view(torch.int32)[frozen], y.view(torch.int32)[frozen]), z
            oa._ema[frozen] = oa._flat[frozen]
            for net in (a, b):
                for name in ENCODER:
                    getattr(net, name).requires_grad_(True)
        _random_grads([a, b], 500 + it)
        idx = oa._trainable()
        recs, _ = oa._ranges(idx)
        late = bool(freeze_steps) and it == freeze_steps
        assert len(recs) == (2 if late else 1), (it, recs)           # the late parameters' buffers start while the others' go on
        assert len(idx) == len(oa._plist) or it < freeze_steps
        tol += 2 * _bound_p(oa, idx, oa._flat_grad(idx))
        ga, gb = oa.param_groups[0], ob.param_groups[0]
        assert ga["lr"] == gb["lr"] and ga["momentum"] == gb["momentum"]
        momenta.append(ga["momentum"])
        oa.step(); ob.step(); sa.step(); sb.step()
        diff = (oa._flat.double() - _flatten(oa, bparams).double()).abs()
        ratio = float((diff / tol.clamp_min(1e-300)).max())
        print(f"nesterov={nesterov} freeze={freeze_steps} step {it + 1}: worst |p - p_torch| / bound = {ratio:.3e}")
        assert bool((diff <= tol).all()), (it, ratio)
        if it < freeze_steps:
            assert torch.equal(oa._flat.view(torch.int32)[frozen], start[0].view(torch.int32)[frozen])
    assert len(set(momenta)) >= 3                        # OneCycleLR cycled the momentum, and both optimizers followed it
    assert all(oa._has_buf) and not torch.equal(oa._flat, start[0])
    return oa


@pytest.mark.parametrize("nesterov", [False, True])
def test_three_steps_agree_with_torch_sgd_on_identical_gradients(nesterov):
    import pytorch_camvid_amd as A
    _against_torch(A, nesterov)


def test_late_start_initialises_the_late_buffers_while_the_others_update():
    import pytorch_camvid_amd as A
    oa = _against_torch(A, False, freeze_steps=2, steps=4)
    assert oa.ema_updates == 4 and bool(torch.isfinite(oa._ema).all()) and bool(torch.isfinite(oa._buf).all())


def test_step_after_real_backward_passes():
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd.optim import ema_alpha
    net, = _twin_nets(A, 1)
    opt = A.FlatSGD(net, lr=0.05, momentum=0.9, dampening=0.1, weight_decay=1e-4, max_grad_norm=1.0, ema_decay=0.9)
    x, _ = _batch(7)
    net.eval()
    with torch.no_grad():
        y0 = net(x).clone()
    net.train()
    _backward(A, net, 600)
    opt.step()                                           # the first step: the buffers become the gradient
    _backward(A, net, 601)
    gl = opt._flat_grad()
    p0, o0 = opt._plist[0], opt._offs[0]
    assert opt._gbuf is None and gl.data_ptr() == p0.grad.data_ptr() - 4 * o0                 # the executor's buffer, not a copy
    assert gl.untyped_storage().data_ptr() == p0.grad.untyped_storage().data_ptr()
    before = [t.cpu().numpy() for t in (opt._flat, gl, opt._buf, opt._ema)]
    idx = opt._trainable()
    n = opt._flat.numel()
    bound_dev = _bound_p(opt, idx, gl, 1.0)              # with coefficient 1: rescaled below once the step has written its record
    opt.step()
    coef, alpha = float(opt.clip_coef.item()), float(ema_alpha(0.9, False, 2))
    assert 0.0 < coef <= 1.0 and opt.ema_updates == 2
    g = opt.param_groups[0]
    rec = sgd_ref.record(g["lr"], g["momentum"], g["dampening"], g["weight_decay"], False, False)
    want = sgd_ref.sgd_step(*before, [(0, n, 0)], [rec], coef, alpha)
    bp, bb, be = sgd_ref.bounds(want, before[3], alpha)
    got = [t.cpu().numpy() for t in (opt._flat, opt._buf, opt._ema)]
    for name, a, b, bd in zip(("param", "buf", "ema"), got, (want.p, want.buf, want.ema), (bp, bb, be)):
        err = np.abs(a.astype(np.float64) - b)
        print(f"{name}: worst error / bound = {float((err / np.maximum(bd, 1e-300)).max()):.3f}")
        assert np.all(err <= bd), name
    # the device evaluation of the bound the torch comparisons use is sgd_ref's (there with coefficient 1: an upper bound of this one)
    assert np.all(bound_dev.cpu().numpy() >= bp * (1 - 1e-12))
    if coef == 1.0:
        assert np.allclose(bound_dev.cpu().numpy(), bp, rtol=1e-12, atol=0)
    net.eval()
    with torch.no_grad():
        y1 = net(x).clone()
    assert not torch.equal(y0, y1)
    torch.manual_seed(77)
    fresh = A.UNet(3, 12).to(dev())
    fresh.load_state_dict(net.state_dict())
    fresh.eval()
    with torch.no_grad():
        y2 = fresh(x)
    assert torch.equal(y1, y2)                           # the stepped network forgot its derived (Winograd) weights


def _make(A, iters, momentum):
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    opt = A.FlatSGD(net, lr=0.01, momentum=momentum, weight_decay=1e-4, max_grad_norm=1.0, ema_decay=0.99)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=0.02, total_steps=iters + 4, cycle_momentum=momentum != 0)
    return net, opt, sched


@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_captured_iteration_is_bitwise_the_eager_loop(momentum):
    import pytorch_camvid_amd as A
    iters = 4
    net, opt, sched = _make(A, iters, momentum)
    st0 = {k: v.clone() for k, v in net.state_dict().items()}
    lossf = A.CrossEntropyLoss()
    gs = A.GraphedStep(net, lossf, *_batch(1), optimizer=opt, scheduler=sched, log_capacity=8)
    assert opt.ema_updates == 0 and not any(opt._has_buf) and (opt._buf is not None) == (momentum != 0)      # the capture runs nothing
    net.load_state_dict(st0)
    opt._ema.copy_(opt._flat)
    ref, opt_r, sched_r = _make(A, iters, momentum)
    ref.load_state_dict(net.state_dict())
    opt_r._ema.copy_(opt_r._flat)
    set_by_scheduler = []
    for it in range(iters):
        x, t = _batch(100 + it)
        g = opt.param_groups[0]
        set_by_scheduler.append((np.float32(g["lr"]), np.float32(g["momentum"])))
        assert g["lr"] == opt_r.param_groups[0]["lr"] and g["momentum"] == opt_r.param_groups[0]["momentum"]
        la = gs.replay(x, t)
        opt_r.zero_grad()
        lb = lossf(ref(x), t)
        lb.backward()
        opt_r.step()
        sched_r.step()
        assert torch.equal(la, lb), (it, la.item(), lb.item())
        assert torch.equal(opt._flat, opt_r._flat) and torch.equal(opt._ema, opt_r._ema), it
        assert torch.equal(opt._clip_rec, opt_r._clip_rec), it
        assert torch.equal(opt.grad_norm, opt_r.grad_norm) and torch.equal(opt.clip_coef, opt_r.clip_coef)
        if momentum:
            assert torch.equal(opt._buf, opt_r._buf), it
            assert all(opt._has_buf) and all(opt_r._has_buf)
        else:
            assert opt._buf is None and opt_r._buf is None and not any(opt._has_buf)
        assert opt.ema_updates == opt_r.ema_updates == it + 1 and opt._step == opt_r._step == it + 1
    rows, dropped = gs.log()
    assert dropped == 0 and rows.shape == (iters, 7)
    for it, (lr, mom) in enumerate(set_by_scheduler):
        assert rows[it, 1] == lr and rows[it, 2] == mom, (it, rows[it], lr, mom)
    assert len({float(r[1]) for r in rows}) == iters                     # the scheduler moved the lr at every step ...
    assert len({float(r[2]) for r in rows}) == (3 if momentum else 1)    # ... and the momentum down and up again: 0.95, a, b, a
    assert not torch.equal(opt._ema, opt._flat)
    # the variant is fixed at the capture: a momentum switched between zero and non-zero is refused, and accepted again when switched back
    step0 = opt._step
    old = opt.param_groups[0]["momentum"]
    opt.param_groups[0]["momentum"] = 0.0 if momentum else 0.9
    with pytest.raises(RuntimeError, match="changed since the capture"):
        gs.replay()
    assert opt._step == step0
    opt.param_groups[0]["momentum"] = old
    gs.replay()
    assert opt._step == step0 + 1
    torch.cuda.synchronize()


def test_accumulation_window_and_state_dict_round_trip():
    import pytorch_camvid_amd as A
    a, b = _twin_nets(A, seed=3)
    kw = dict(lr=0.02, momentum=0.9, dampening=0.1, weight_decay=1e-4, max_grad_norm=1.0, ema_decay=0.9, ema_warmup=True)
    oa = A.FlatSGD(a, **kw)
    lossf = A.CrossEntropyLoss()
    acc = A.GradAccumulator(a, steps=2)
    for w in range(2):
        for m in range(2):
            x, t = _batch(300 + 10 * w + m)
            lossf(a(x), t).backward()
            snap = [t_.clone() for t_ in (oa._flat, oa._buf, oa._ema)]
            oa.step()                                    # inside an open window: nothing has a gradient, nothing changes, no EMA update
            assert oa.ema_updates == (w + 1 if acc.ready else w)
            if acc.ready:
                assert not torch.equal(oa._flat, snap[0])
                oa.zero_grad(set_to_none=True)
            else:
                assert all(torch.equal(u, v) for u, v in zip(snap, (oa._flat, oa._buf, oa._ema))) and oa._step == w
    assert oa._step == 2 and all(oa._has_buf)
    # state_dict -> a new FlatSGD on a twin -> one more step on both
    sd, nsd = oa.state_dict(), {k: v.clone() for k, v in a.state_dict().items()}
    own = sd["flat_sgd"]
    assert set(own) == {"step", "has_buffer", "momentum_buffer", "offsets", "max_grad_norm", "norm_type", "ema", "ema_decay", "ema_warmup",
                        "ema_updates"}
    assert own["step"] == 2 and own["ema_updates"] == 2 and all(own["has_buffer"]) and torch.equal(own["momentum_buffer"], oa._buf)
    assert own["momentum_buffer"].data_ptr() != oa._buf.data_ptr()
    b.load_state_dict(nsd)
    ob = A.FlatSGD(b, lr=0.5, ema_decay=0.5)             # other options, no momentum, no buffer: the saved ones win
    assert ob._buf is None
    ob.load_state_dict(sd)
    assert ob.param_groups[0]["momentum"] == 0.9 and ob.ema_decay == 0.9 and ob.ema_updates == 2 and ob._has_buf == oa._has_buf
    assert torch.equal(ob._buf, oa._buf) and torch.equal(ob._ema, oa._ema) and torch.equal(ob._flat, oa._flat)
    for p in a.parameters():
        p.grad = None
    _random_grads([a, b], 410)
    for p in a.parameters():
        assert p.grad is not None
    # (the accumulator only folds what backward writes; hand-assigned gradients reach step() as they are)
    oa.step(); ob.step()
    assert torch.equal(ob._flat, oa._flat) and torch.equal(ob._buf, oa._buf) and torch.equal(ob._ema, oa._ema)
    assert torch.equal(ob._clip_rec, oa._clip_rec) and ob._step == oa._step == 3
    # a state without a buffer (momentum 0 throughout) keeps none; a state of another layout is refused
    plain = A.FlatSGD(_twin_nets(A, 1)[0], lr=0.01).state_dict()
    assert plain["flat_sgd"]["momentum_buffer"] is None and not any(plain["flat_sgd"]["has_buffer"])
    assert "ema" not in plain["flat_sgd"]
    bad = dict(sd)
    bad["flat_sgd"] = dict(own, offsets=[o + 4 for o in own["offsets"]])
    with pytest.raises(ValueError, match="different network layout"):
        ob.load_state_dict(bad)
    bad["flat_sgd"] = dict(own, momentum_buffer=own["momentum_buffer"][:-4])
    with pytest.raises(ValueError, match="different network layout"):
        ob.load_state_dict(bad)
    with pytest.raises(ValueError, match="different network layout"):
        ob.load_state_dict(dict(sd, flat_sgd=dict(own, has_buffer=own["has_buffer"][:-1])))
    assert torch.equal(ob._flat, oa._flat) and torch.equal(ob._buf, oa._buf)
