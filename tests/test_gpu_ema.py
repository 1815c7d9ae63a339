"""The weight EMA inside the fused AdamW step (FlatAdamW(ema_decay=...)) on the GPU: the step's own results bitwise untouched, the average
against an fp64 recursion, nothing written outside the trainable ranges, more than one launch, swap_ema(), the captured iteration against
the eager loop bit for bit, accumulation windows and the state-dict round trip.  Every case runs a UNet at batch (2, 48, 64).

Bound of every comparison with the fp64 recursion (EMA_ULPS): one update e + alpha * (p - e) makes at most three fp32 roundings (the
difference, the product, the sum; two when the compiler contracts the last two into one FMA) of quantities of magnitude at most 2 max|p|,
and the error already in e is multiplied by 1 - alpha <= 1.  After k updates |ema - ema64| <= k * 6 * 2^-24 * 2 max|p| < k * 2^-21 max|p|."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPE = (2, 48, 64)
ENCODER = ("down1", "down2", "down3", "down4", "down5")
EMA_ULPS = 2.0 ** -21


def dev():
    return torch.device("cuda:0")


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
    """The same random gradient into .grad of every twin (fresh tensors: the optimizer gathers them into its own flat buffer)."""
    g = torch.Generator(device=dev()).manual_seed(seed)
    for ps in zip(*[net.parameters() for net in nets]):
        gr = torch.randn(ps[0].shape, generator=g, device=dev()) * scale
        for p in ps:
            p.grad = gr.clone()


def _follow(ema64, opt, alpha):
    """One step of the fp64 recursion on the fp32 parameters as they are now, with the fp32 value of alpha; returns max|p|."""
    p = opt._flat.double()
    ema64 += float(alpha) * (p - ema64)
    return float(opt._flat.abs().max())


def _check_against(ema64, opt, k, pmax, what, where=None):
    err = (opt._ema.double() - ema64).abs()
    if where is not None:
        err = err[where]
    worst, bound = float(err.max()), k * EMA_ULPS * pmax
    print(f"{what}: after {k} update(s) max |ema - ema64| = {worst:.3e}, bound {bound:.3e} (max|p| = {pmax:.4f})")
    assert worst <= bound, (what, k, worst, bound)


# ---- 1. the step itself is untouched ---------------------------------------------------------------------------------------------------
def test_parameters_and_moments_are_bitwise_those_of_the_step_without_ema():
    import pytorch_camvid_amd as A
    nets = _twin_nets(A, 4)
    plain, plain_ema = A.FlatAdamW(nets[0], lr=2e-3), A.FlatAdamW(nets[1], lr=2e-3, ema_decay=0.9)
    clip = A.FlatAdamW(nets[2], lr=2e-3, max_grad_norm=0.5)
    clip_ema = A.FlatAdamW(nets[3], lr=2e-3, max_grad_norm=0.5, ema_decay=0.9)
    assert plain._ema is None and clip._ema is None and torch.equal(plain_ema._ema, plain_ema._flat)
    start = plain_ema._ema.clone()
    for it in range(3):
        _random_grads(nets, 40 + it)
        for o in (plain, plain_ema, clip, clip_ema):
            o.step()
        for a, b in ((plain, plain_ema), (clip, clip_ema)):
            assert torch.equal(a._flat, b._flat) and torch.equal(a._m, b._m) and torch.equal(a._v, b._v), it
            assert a._step == b._step and a._steps == b._steps
        assert torch.equal(clip._clip_rec, clip_ema._clip_rec) and clip_ema.clip_coef.item() < 1.0
        assert not torch.equal(plain._flat, clip._flat)                    # the clipped pair really took another step
    assert plain_ema.ema_updates == clip_ema.ema_updates == 3 and plain.ema_updates == 0
    assert not torch.equal(plain_ema._ema, start) and not torch.equal(plain_ema._ema, plain_ema._flat)
    assert not torch.equal(plain_ema._ema, clip_ema._ema)


# ---- 2. the average is right -------------------------------------------------------------------------------------------------------------
def test_average_against_the_fp64_recursion():
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd.optim import ema_alpha
    net, = _twin_nets(A, 1)
    opt = A.FlatAdamW(net, lr=2e-3, ema_decay=0.9, ema_warmup=True)
    ema64 = opt._flat.double()
    pmax = float(opt._flat.abs().max())
    for k in range(1, 6):
        _random_grads([net], 50 + k)
        opt.step()
        alpha = ema_alpha(0.9, True, k)
        assert alpha.dtype == np.float32 and (k > 1 or alpha == np.float32(1 - 2 / 11))
        pmax = max(pmax, _follow(ema64, opt, alpha))
        _check_against(ema64, opt, k, pmax, "warm-up, decay 0.9")
    assert opt.ema_updates == 5
    # a step in which nothing has a gradient is the no-op it was and counts no update
    before = opt._ema.clone()
    for p in net.parameters():
        p.grad = None
    opt.step()
    assert opt.ema_updates == 5 and opt._step == 5 and torch.equal(opt._ema, before)


# ---- 3. nothing outside the ranges is touched ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [12, 21])
def test_ema_outside_the_trainable_ranges_is_neither_read_nor_written(classes):
    """12 classes: no alignment padding; a 21-class head has padding floats behind its three 21-float vectors.  The padding behind a trainable
    parameter lies inside its (rounded-up) AdamW range: a NaN there stays a NaN; the frozen segments keep their very bits."""
    import pytorch_camvid_amd as A
    net, = _twin_nets(A, 1, classes=classes)
    for name in ENCODER:
        getattr(net, name).requires_grad_(False)
    opt = A.FlatAdamW(net, lr=2e-3, ema_decay=0.9, max_grad_norm=0.5 if classes == 21 else None)
    trainable = torch.zeros(opt._flat.numel(), dtype=torch.bool, device=dev())
    frozen = torch.zeros_like(trainable)
    for p, o in zip(opt._plist, opt._offs):
        (trainable if p.requires_grad else frozen)[o:o + p.numel()] = True
    assert bool(trainable.any()) and bool(frozen.any()) and not bool((trainable & frozen).any())
    assert bool((~(trainable | frozen)).any()) == (classes == 21)
    poison = torch.full_like(opt._ema, float("nan")).view(torch.int32) + 0x0ABC       # a NaN with a payload
    opt._ema.view(torch.int32)[~trainable] = poison[~trainable]
    before = opt._ema.clone()
    assert torch.equal(torch.isnan(before), ~trainable)
    for it in range(2):
        x, t = _batch(60 + it)
        for p in net.parameters():
            p.grad = None
        A.CrossEntropyLoss()(net(x), t).backward()                          # targets below 12: valid for both heads
        assert all((p.grad is None) == (not p.requires_grad) for p in net.parameters())
        opt.step()
    assert opt.ema_updates == 2
    assert torch.equal(torch.isnan(opt._ema), ~trainable)
    assert torch.equal(opt._ema.view(torch.int32)[frozen], before.view(torch.int32)[frozen])
    assert bool(torch.isfinite(opt._ema[trainable]).all()) and not torch.equal(opt._ema[trainable], before[trainable])
    assert bool(torch.isfinite(opt._flat[trainable | frozen]).all())


# ---- 4. more than 16 records -------------------------------------------------------------------------------------------------------------------
def test_twenty_groups_take_two_launches_and_every_element_moves():
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd import _lib, optim
    from pytorch_camvid_amd.optim import ema_alpha
    net, = _twin_nets(A, 1)
    params = optim._block_params(net)
    cut = [i * len(params) // 20 for i in range(21)]
    groups = [{"params": params[cut[i]:cut[i + 1]], "lr": 1e-3 * (1 + i / 20)} for i in range(20)]
    assert all(g["params"] for g in groups)
    opt = A.FlatAdamW(net, groups=groups, ema_decay=0.9)
    recs, _ = opt._ranges(list(range(len(params))))
    assert len(recs) == 20 > _lib.ADAMW_ARG_RECORDS                         # two launches: 16 records, then 4
    start = opt._ema.clone()
    ema64 = start.double()
    pmax = float(opt._flat.abs().max())
    _random_grads([net], 70)
    opt.step()
    real = torch.zeros(opt._flat.numel(), dtype=torch.bool, device=dev())
    for p, o in zip(opt._plist, opt._offs):
        real[o:o + p.numel()] = True
    assert bool(real.all())                                                 # 12 classes: every float of the buffer is a parameter
    moved = opt._ema != start
    assert bool(moved.all()), f"{int((~moved).sum())} elements of the average did not move"
    pmax = max(pmax, _follow(ema64, opt, ema_alpha(0.9, False, 1)))
    _check_against(ema64, opt, 1, pmax, "20 groups")


# ---- 5. swap -----------------------------------------------------------------------------------------------------------------------------------
def test_swap_ema_exchanges_the_weights_and_invalidates_derived_weights():
    import pytorch_camvid_amd as A
    a, b = _twin_nets(A)
    oa, ob = A.FlatAdamW(a, lr=2e-3, ema_decay=0.9), A.FlatAdamW(b, lr=2e-3, ema_decay=0.9)
    for it in range(3):
        _backward(A, a, 80 + it); _backward(A, b, 80 + it)
        oa.step(); ob.step()
    x, _ = _batch(90)
    a.eval()
    with torch.no_grad():
        live = a(x).clone()                                                 # derived weights of the LIVE parameters are cached now
    params, avg = oa._flat.clone(), oa._ema.clone()
    names = {k for k, _ in a.named_parameters()}
    with oa.swap_ema() as inside:
        assert inside is oa
        assert torch.equal(oa._flat, avg) and torch.equal(oa._ema, params)
        esd, nsd = oa.ema_state_dict(), a.state_dict()
        assert list(esd.keys()) == list(nsd.keys())
        for k in nsd:
            assert torch.equal(esd[k], nsd[k]) and esd[k].shape == nsd[k].shape and esd[k].stride() == nsd[k].stride(), k
            if k in names:
                assert esd[k].data_ptr() != nsd[k].data_ptr(), k            # clones, not views of the buffers
        with torch.no_grad():
            got = a(x).clone()
        torch.manual_seed(5)
        fresh = A.UNet(3, 12).to(dev())
        fresh.load_state_dict(esd)
        fresh.eval()
        with torch.no_grad():
            want = fresh(x)
        assert torch.equal(got, want) and not torch.equal(got, live)
        with pytest.raises(RuntimeError, match="swap_ema"):
            oa.step()
        with pytest.raises(RuntimeError, match="swap_ema"):
            with oa.swap_ema():
                pass
        assert torch.equal(oa._flat, avg) and torch.equal(oa._ema, params)  # the refused calls changed nothing
    assert torch.equal(oa._flat, params) and torch.equal(oa._ema, avg)
    with torch.no_grad():
        assert torch.equal(a(x), live)                                      # and the live weights are what runs again
    # outside the context ema_state_dict() is the same dict, without a swap
    for k, v in oa.ema_state_dict().items():
        assert torch.equal(v, esd[k]), k
    a.train()
    _backward(A, a, 95); _backward(A, b, 95)
    oa.step(); ob.step()
    assert torch.equal(oa._flat, ob._flat) and torch.equal(oa._m, ob._m) and torch.equal(oa._v, ob._v) and torch.equal(oa._ema, ob._ema)
    assert oa.ema_updates == ob.ema_updates == 4
    # an exception inside the block still swaps back
    with pytest.raises(KeyError):
        with oa.swap_ema():
            raise KeyError("boom")
    assert torch.equal(oa._flat, ob._flat) and torch.equal(oa._ema, ob._ema)
    with pytest.raises(RuntimeError, match="no EMA"):
        with A.FlatAdamW(_twin_nets(A, 1)[0]).swap_ema():
            pass


# ---- 6. captured == eager ------------------------------------------------------------------------------------------------------------------------
def _make(A, iters):
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    opt = A.FlatAdamW(net, lr=1e-3, ema_decay=0.99, ema_warmup=True, max_grad_norm=0.5)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=2e-3, total_steps=iters + 4, cycle_momentum=True)
    return net, opt, sched


def test_captured_iteration_with_ema_is_bitwise_the_eager_loop():
    """The eager loop writes its own log rows with the kernel the graph ends in (cvk_step_log with the record of the step it has just
    taken), so the rows compare bit for bit, all seven columns."""
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd import _lib
    from pytorch_camvid_amd.graph import last_layer_params
    lib = _lib.load()
    iters = 4
    net, opt, sched = _make(A, iters)
    st0 = {k: v.clone() for k, v in net.state_dict().items()}
    lossf = A.CrossEntropyLoss()
    gs = A.GraphedStep(net, lossf, *_batch(1), optimizer=opt, scheduler=sched, log_capacity=iters)
    assert opt.ema_updates == 0                                             # the capture runs nothing
    net.load_state_dict(st0)
    opt._ema.copy_(opt._flat)
    ref, opt_r, sched_r = _make(A, iters)
    ref.load_state_dict(net.state_dict())
    opt_r._ema.copy_(opt_r._flat)
    (_, rw), (_, rb) = last_layer_params(ref)
    ring = torch.zeros(2 + iters * 7, device=dev(), dtype=torch.float32)
    hyper = torch.zeros(7, device=dev(), dtype=torch.float32)
    stream = torch.cuda.current_stream().cuda_stream
    for it in range(iters):
        x, t = _batch(100 + it)
        la = gs.replay(x, t)
        opt_r.zero_grad()
        lb = lossf(ref(x), t)
        lb.backward()
        g = opt_r.param_groups[0]
        opt_r.step()
        rec = _lib.AdamwHyper()
        _lib.check(lib.cvk_adamw_hyper_fill(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                            float(g["weight_decay"]), opt_r._step, ctypes.addressof(rec)), "cvk_adamw_hyper_fill")
        hyper.copy_(torch.tensor(list(np.frombuffer(bytes(rec), np.float32)), dtype=torch.float32))
        _lib.check(lib.cvk_step_log(lb.data_ptr(), hyper.data_ptr(), rw.grad.data_ptr(), rw.grad.numel(), rb.grad.data_ptr(),
                                    rb.grad.numel(), opt_r._clip_rec.data_ptr(), ring.data_ptr() + 8, iters, ring.data_ptr(), stream),
                   "cvk_step_log")
        sched_r.step()
        assert torch.equal(la, lb), (it, la.item(), lb.item())
        assert torch.equal(opt._flat, opt_r._flat) and torch.equal(opt._m, opt_r._m) and torch.equal(opt._v, opt_r._v), it
        assert torch.equal(opt._ema, opt_r._ema), it
        assert torch.equal(opt._clip_rec, opt_r._clip_rec), it
        assert opt.ema_updates == opt_r.ema_updates == it + 1 and opt._step == opt_r._step
        assert torch.equal(gs._logbuf, ring), it
    assert not torch.equal(opt._ema, opt._flat)
    rows, dropped = gs.log()
    assert dropped == 0 and rows.shape == (iters, 7) and bool((rows[:, 6] < 1.0).any())
    # a new decay is uploaded with the next replay; switching the EMA off is refused
    opt.ema_decay = opt_r.ema_decay = 0.5
    x, t = _batch(200)
    gs.replay(x, t)
    opt_r.zero_grad()
    lossf(ref(x), t).backward()
    opt_r.step(); sched_r.step()
    assert torch.equal(opt._ema, opt_r._ema) and torch.equal(opt._flat, opt_r._flat)
    step0, updates0 = opt._step, opt.ema_updates
    with opt.swap_ema():
        with pytest.raises(RuntimeError, match="swap_ema"):
            gs.replay()
    opt.ema_decay = None
    with pytest.raises(RuntimeError, match="changed since the capture"):
        gs.replay()
    with pytest.raises(RuntimeError, match="after construction"):
        opt.step()
    opt.ema_decay = 0.5
    assert opt._step == step0 and opt.ema_updates == updates0
    gs.replay()
    torch.cuda.synchronize()


# ---- 7. accumulation -----------------------------------------------------------------------------------------------------------------------------
def test_one_update_per_accumulation_window():
    import pytorch_camvid_amd as A
    a, b = _twin_nets(A, seed=3)
    oa = A.FlatAdamW(a, lr=1e-3, ema_decay=0.9, ema_warmup=True)
    ob = A.FlatAdamW(b, lr=1e-3, ema_decay=0.9, ema_warmup=True)
    lossf = A.CrossEntropyLoss()
    acc = A.GradAccumulator(b, steps=2)
    k = torch.tensor(np.float32(0.5), device=dev())
    for w in range(2):
        batches = [_batch(300 + 10 * w + m) for m in range(2)]
        total = None
        for x, t in batches:                                                # the twin: the window's mean, ((g1 + g2) * float32(1 / 2))
            for p in a.parameters():
                p.grad = None
            lossf(a(x), t).backward()
            gs = [p.grad.detach().clone() for p in a.parameters()]
            total = gs if total is None else [u + v for u, v in zip(total, gs)]
        for p, g in zip(a.parameters(), total):
            p.grad = g * k
        oa.step()
        for x, t in batches:
            lossf(b(x), t).backward()
            ob.step()                                                       # before the window closes: a no-op that counts no update
            assert ob.ema_updates == (w + 1 if acc.ready else w)
            if acc.ready:
                ob.zero_grad(set_to_none=True)
        assert torch.equal(oa._flat, ob._flat) and torch.equal(oa._ema, ob._ema), w
    assert oa.ema_updates == ob.ema_updates == 2 and not torch.equal(ob._ema, ob._flat)


# ---- 8. state-dict round trip --------------------------------------------------------------------------------------------------------------------
TODAYS_KEYS = {"step", "steps", "exp_avg", "exp_avg_sq", "offsets", "max_grad_norm", "norm_type"}


def test_state_dict_round_trip_and_the_formats_without_an_ema():
    import pytorch_camvid_amd as A
    a, b, c = _twin_nets(A, 3)
    oa = A.FlatAdamW(a, lr=2e-3, ema_decay=0.9, ema_warmup=True)
    ob = A.FlatAdamW(b, lr=2e-3, ema_decay=0.9, ema_warmup=True)
    plain = A.FlatAdamW(c, lr=2e-3)
    for it in range(2):
        _random_grads([a, b, c], 400 + it)
        oa.step(); ob.step(); plain.step()
    sd, nsd = ob.state_dict(), {k: v.clone() for k, v in b.state_dict().items()}
    assert set(sd["flat_adamw"]) == TODAYS_KEYS | {"ema", "ema_decay", "ema_warmup", "ema_updates"}
    assert sd["flat_adamw"]["ema_updates"] == 2 and sd["flat_adamw"]["ema_decay"] == 0.9 and sd["flat_adamw"]["ema_warmup"] is True
    assert set(plain.state_dict()["flat_adamw"]) == TODAYS_KEYS             # a non-EMA optimizer saves exactly what it saved before
    del ob, b
    torch.manual_seed(9)
    d = A.UNet(3, 12).to(dev()).train()
    d.load_state_dict(nsd)
    od = A.FlatAdamW(d, lr=1e-4, ema_decay=0.5)                            # other options: the saved ones win
    od.load_state_dict(sd)
    assert od.ema_decay == 0.9 and od.ema_warmup is True and od.ema_updates == 2
    assert torch.equal(od._ema, oa._ema) and torch.equal(od._flat, oa._flat)
    for it in range(2):
        _random_grads([a, d], 410 + it)
        oa.step(); od.step()
    assert torch.equal(od._flat, oa._flat) and torch.equal(od._m, oa._m) and torch.equal(od._v, oa._v) and torch.equal(od._ema, oa._ema)
    assert od.ema_updates == oa.ema_updates == 4
    # a state saved without an EMA: the average restarts from the parameters as loaded, the count from 0
    od.load_state_dict(plain.state_dict())
    assert od.ema_updates == 0 and torch.equal(od._ema, od._flat) and od.ema_decay == 0.9 and od._step == 2
    # a state saved with an EMA into an optimizer without one: ignored
    plain.load_state_dict(sd)
    assert plain._ema is None and plain.ema_decay is None and plain._step == 2
    assert set(plain.state_dict()["flat_adamw"]) == TODAYS_KEYS
    _random_grads([c], 420)
    plain.step()
