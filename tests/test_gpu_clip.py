"""Global-norm gradient clipping on the GPU: the norm kernels against an fp64 reference (real backward gradients, a buffer with NaN in every
padding float and frozen segment), clip_grad_norm_ against torch's, the clipped FlatAdamW step (bitwise against the unclipped step on
pre-scaled gradients, and against torch's clip + AdamW), the captured iteration against the eager loop bit for bit, bf16 mode, and the
data-parallel form in child processes.

Tolerance of every norm comparison (NORM_RTOL): the kernel accumulates in fp64 — 3.5e7 terms carry a relative error below 1e-8 — and rounds
once to fp32, so its result is within 1 ulp of the correctly rounded exact value; 2 ulp = 2 * 2^-23 = 2.4e-7 relative are allowed.  The
infinity norm is exact."""
import ctypes
import json
import math
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "clip_worker.py")
NORM_RTOL = 2.4e-7
INF = float("inf")
ENCODER = ("down1", "down2", "down3", "down4", "down5")


def dev():
    return torch.device("cuda:0")


def _batch(shape, seed, classes=12):
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, h, w, generator=g).to(dev()), torch.randint(0, classes, (n, h, w), generator=g).to(dev())


def _backward(A, net, shape, seed, classes=12):
    for p in net.parameters():
        p.grad = None
    x, t = _batch(shape, seed, classes)
    A.CrossEntropyLoss()(net(x), t).backward()


def _ref_norms(grads):
    """(2-norm, infinity norm) of the gathered gradients in fp64 on the device."""
    flat = torch.cat([g.detach().double().reshape(-1) for g in grads])
    return torch.linalg.vector_norm(flat).item(), torch.linalg.vector_norm(flat, INF).item()


def _close(got, want, what):
    print(f"{what}: got {got!r} want {want!r} rel {abs(got - want) / want:.3e}")
    assert abs(got - want) <= NORM_RTOL * want, (what, got, want)


def _no_torch_fallback(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("clip_grad_norm_ fell back to torch for the executor's flat gradient buffer")
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", boom)


def _ulp_distance(a, b):
    """Largest distance in units of the last place between two fp32 tensors of equal signs."""
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    assert bool(((ia < 0) == (ib < 0)).logical_or((a == 0) & (b == 0)).all())
    return int((ia - ib).abs().max())


# ---- 5. the norm value ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 48, 64), (8, 360, 480)])
def test_total_norm_against_fp64(shape, monkeypatch):
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    _backward(A, net, shape, 11)
    grads = [p.grad for p in net.parameters()]
    before = [g.clone() for g in grads]
    want2, wantinf = _ref_norms(grads)
    _no_torch_fallback(monkeypatch)
    got2 = A.clip_grad_norm_(net, 1e30)
    assert got2.dim() == 0 and got2.dtype == torch.float32 and got2.is_cuda
    _close(got2.item(), want2, f"2-norm {shape}")
    gotinf = A.clip_grad_norm_(net.parameters(), 1e30, norm_type=INF)
    print(f"inf-norm {shape}: got {gotinf.item()!r} want {wantinf!r}")
    assert gotinf.item() == wantinf
    assert all(torch.equal(a, b) for a, b in zip(grads, before))          # coefficient 1: nothing rewritten
    # the optimizer's record is the same reduction over the same buffer: the same bits
    opt = A.FlatAdamW(net, max_grad_norm=1e30)
    _backward(A, net, shape, 11)
    opt.step()
    assert opt.grad_norm.item() == got2.item() and opt.clip_coef.item() == 1.0


# ---- 6. padding and frozen segments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [5, 21])
@pytest.mark.parametrize("frozen", [(), ENCODER])
def test_norm_never_reads_padding_or_frozen_segments(classes, frozen):
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd import engine, optim
    torch.manual_seed(1)
    net = A.UNet(3, classes).to(dev())
    names = {id(p): k for k, p in net.named_parameters()}
    params = optim._block_params(net)
    offs, total = engine.layout_grads(params)
    assert total > sum(p.numel() for p in params)                         # this head has padding floats
    flat = torch.full((total,), float("nan"), device=dev())
    g = torch.Generator(device=dev()).manual_seed(2)
    real, pairs = [], []
    for p, o in zip(params, offs):
        if names[id(p)].split(".")[0] in frozen:
            continue
        seg = torch.randn(p.numel(), generator=g, device=dev()) * 1e-2
        flat[o:o + p.numel()] = seg
        real.append(seg)
        pairs.append((o, p.numel()))
    want2, wantinf = _ref_norms(real)
    plan = optim._NormPlan(optim.norm_segments(pairs), total, dev())
    rec = torch.zeros(2, device=dev())
    s = torch.cuda.current_stream().cuda_stream
    plan.norm(flat.data_ptr(), 2.0, 1.0, rec, s)
    got = rec.cpu()
    assert math.isfinite(got[0].item())
    _close(got[0].item(), want2, f"2-norm, {classes} classes, frozen={bool(frozen)}")
    assert got[1].item() == float(np.float32(1.0) / (np.float32(got[0].item()) + np.float32(1e-6)))
    plan.norm(flat.data_ptr(), INF, 1.0, rec, s)
    assert rec[0].item() == wantinf
    # the in-place scale touches the same segments only: the NaNs stay where they were, every real element is scaled once
    keep = flat.clone()
    plan.norm(flat.data_ptr(), 2.0, 0.5 * want2, rec, s)
    plan.scale(flat.data_ptr(), rec, s)
    coef = rec[1]
    assert 0.49 < coef.item() < 0.51
    nan = torch.isnan(keep)
    assert torch.equal(torch.isnan(flat), nan)
    assert torch.equal(flat[~nan], keep[~nan] * coef)


# ---- 7. clip_grad_norm_ against torch ---------------------------------------------------------------------------------------------------
def test_clip_grad_norm_matches_torch(monkeypatch):
    import pytorch_camvid_amd as A
    torch_clip = torch.nn.utils.clip_grad_norm_
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    net.down1.requires_grad_(False)                                        # parameters without a gradient are skipped, as in torch
    _backward(A, net, (2, 48, 64), 12)
    withgrad = [p for p in net.parameters() if p.grad is not None]
    assert len(withgrad) < len(list(net.parameters()))
    saved = [p.grad.clone() for p in withgrad]
    norm0, _ = _ref_norms(saved)
    for factor in (0.5, 10.0):
        twins = [torch.nn.Parameter(torch.zeros_like(g)) for g in saved]
        for q, g in zip(twins, saved):
            q.grad = g.clone()
        for p, g in zip(withgrad, saved):
            p.grad.copy_(g)
        want = torch_clip(twins, factor * norm0)
        with monkeypatch.context() as m:
            _no_torch_fallback(m)
            got = A.clip_grad_norm_(net, factor * norm0)
        _close(got.item(), norm0, f"returned norm, max_norm = {factor} x norm")
        print(f"torch's own fp32 norm: {want.item()!r}")
        assert abs(want.item() - got.item()) <= NORM_RTOL * want.item()
        if factor > 1:
            for p, g in zip(withgrad, saved):
                assert torch.equal(p.grad, g)                              # coefficient 1: bitwise unchanged
        else:
            worst = max(_ulp_distance(p.grad, q.grad) for p, q in zip(withgrad, twins))
            print(f"scaled gradients: largest distance from torch's {worst} ulp")
            assert worst <= 2
        assert all(p.grad is None for p in net.down1.parameters())
    with pytest.raises(RuntimeError, match="non-finite"):
        next(p for p in withgrad if p.dim() == 1).grad[0] = float("nan")
        A.clip_grad_norm_(net, 1.0, error_if_nonfinite=True)
    n = A.clip_grad_norm_(net, 1.0)                                        # torch: NaN norm, NaN coefficient, every gradient NaN
    assert math.isnan(n.item()) and bool(torch.isnan(withgrad[0].grad).all())


# ---- 8. the optimizer step -----------------------------------------------------------------------------------------------------------------
def _twin_nets(A, n=2, seed=0):
    torch.manual_seed(seed)
    nets = [A.UNet(3, 12).to(dev()).train()]
    for _ in range(n - 1):
        other = A.UNet(3, 12).to(dev()).train()
        other.load_state_dict(nets[0].state_dict())
        nets.append(other)
    return nets


def _opt_equal(a, b, net_a, net_b):
    assert torch.equal(a._flat, b._flat) and torch.equal(a._m, b._m) and torch.equal(a._v, b._v)
    assert a._step == b._step and a._steps == b._steps
    for (k, x), y in zip(net_a.state_dict().items(), net_b.state_dict().values()):
        assert torch.equal(x, y), k


def test_step_with_a_huge_max_norm_is_bitwise_the_unclipped_step():
    import pytorch_camvid_amd as A
    a, b = _twin_nets(A)
    oa, ob = A.FlatAdamW(a, lr=2e-3, max_grad_norm=1e30), A.FlatAdamW(b, lr=2e-3)
    for it in range(5):
        _backward(A, a, (2, 48, 64), 20 + it)
        _backward(A, b, (2, 48, 64), 20 + it)
        oa.step(); ob.step()
        assert oa.clip_coef.item() == 1.0 and oa.grad_norm.item() > 0
        _opt_equal(oa, ob, a, b)
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["flat_adamw"]["max_grad_norm"] == 1e30 and sb["flat_adamw"]["max_grad_norm"] is None and sa["flat_adamw"]["norm_type"] == 2.0
    oc = A.FlatAdamW(b, lr=2e-3)
    oc.load_state_dict(sa)
    assert oc.max_grad_norm == 1e30 and oc._steps == oa._steps
    old = dict(sa)
    old["flat_adamw"] = {k: v for k, v in sa["flat_adamw"].items() if k not in ("max_grad_norm", "norm_type")}    # saved before clipping existed
    od = A.FlatAdamW(b, lr=2e-3, max_grad_norm=3.0, norm_type=INF)
    od.load_state_dict(old)
    assert od.max_grad_norm == 3.0 and od.norm_type == INF and od._step == 5


@pytest.mark.parametrize("norm_type", [2.0, INF])
def test_clipped_step_is_the_unclipped_step_on_prescaled_gradients(norm_type):
    """Pins the fused multiply without depending on a reduction order: scale the twin's gradients on the device by the recorded coefficient
    (one fp32 multiply per element, what the kernel does on the way in) and take the unclipped step.  `.grad` of the clipped network stays
    unscaled."""
    import pytorch_camvid_amd as A
    a, b, probe = _twin_nets(A, 3)
    _backward(A, probe, (2, 48, 64), 30)                                    # a third twin measures the first step's norm
    first = A.clip_grad_norm_(probe, 1e30, norm_type=norm_type).item()
    del probe
    oa, ob = A.FlatAdamW(a, lr=2e-3, max_grad_norm=0.5 * first, norm_type=norm_type), A.FlatAdamW(b, lr=2e-3)
    clipped = 0
    for it in range(5):
        _backward(A, a, (2, 48, 64), 30 + it)
        _backward(A, b, (2, 48, 64), 30 + it)
        ga = [p.grad.clone() for p in a.parameters()]
        oa.step()
        coef = oa.clip_coef
        clipped += coef.item() < 1.0
        for p, g0 in zip(a.parameters(), ga):
            assert torch.equal(p.grad, g0)                                  # the fused step does not rewrite the gradients
        for p in b.parameters():
            p.grad.mul_(coef)
        ob.step()
        _opt_equal(oa, ob, a, b)
        if it == 0:                                                         # the gradients `first` was measured on
            assert coef.item() == float(np.float32(0.5 * first) / (np.float32(first) + np.float32(1e-6)))
    assert clipped >= 1


def _groups(named):
    nd = [p for k, p in named if p.dim() == 1]
    wd = [p for k, p in named if p.dim() != 1]
    return [{"params": nd, "weight_decay": 0.0, "lr": 2e-3}, {"params": wd, "weight_decay": 5e-2, "lr": 1e-3}]


def test_clipped_flat_adamw_matches_torch_clip_plus_adamw():
    """The construction and the tolerance of tests/test_gpu_finetune.py::test_flat_adamw_groups_frozen_and_late_unfreezing_match_torch
    (rtol 1e-5, atol 1e-7): identical random gradients into FlatAdamW(max_grad_norm=) and into torch's clip_grad_norm_ + AdamW on twin
    parameters, two groups, 6 steps, the encoder frozen for the first three.  Gradient norm ~ 1e-2 * sqrt(34.5e6) = 59 against max_norm 10:
    every step is clipped, the norm is global over both groups."""
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    twin = {k: torch.nn.Parameter(p.detach().clone()) for k, p in net.named_parameters()}
    opt = A.FlatAdamW(net, groups=_groups(list(net.named_parameters())), betas=(0.9, 0.99), max_grad_norm=10.0)
    opt_t = torch.optim.AdamW(_groups(list(twin.items())), betas=(0.9, 0.99), foreach=False)
    g = torch.Generator(device=dev()).manual_seed(3)
    for it in range(6):
        frozen = ENCODER if it < 3 else ()
        for k, p in net.named_parameters():
            if k.split(".")[0] in frozen:
                p.grad = twin[k].grad = None
            else:
                gr = torch.randn(p.shape, generator=g, device=dev()) * 1e-2
                p.grad, twin[k].grad = gr.clone(), gr.clone()
        want = torch.nn.utils.clip_grad_norm_(list(twin.values()), 10.0)
        opt.step()
        opt_t.step()
        print(f"step {it}: norm {opt.grad_norm.item()!r} (torch {want.item()!r}), coef {opt.clip_coef.item()!r}")
        assert opt.clip_coef.item() < 1.0
        assert abs(opt.grad_norm.item() - want.item()) <= 1e-5 * want.item()
    worst = 0.0
    for k, p in net.named_parameters():
        d = (p.detach() - twin[k].detach()).abs()
        worst = max(worst, float((d - 1e-5 * twin[k].detach().abs()).max()))
        assert torch.allclose(p.detach(), twin[k].detach(), rtol=1e-5, atol=1e-7), (k, float(d.max()))
    print(f"largest |difference| - rtol * |torch| over all parameters: {worst:.3e} (allowed 1e-7)")


# ---- 9. captured == eager ---------------------------------------------------------------------------------------------------------------------
def _make(A, iters, seed=0, max_grad_norm=0.5):
    torch.manual_seed(seed)
    net = A.UNet(3, 12).to(dev()).train()
    opt = A.FlatAdamW(net, groups=_groups(list(net.named_parameters())), max_grad_norm=max_grad_norm)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=[2e-3, 1e-3], total_steps=iters + 4, cycle_momentum=True)
    return net, opt, sched


def _state_equal(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_state_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_state_equal(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("shape", [(2, 48, 64), (2, 360, 480)])
def test_captured_clipped_iteration_is_bitwise_the_eager_loop(shape):
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd.graph import last_layer_params
    iters = 6
    net, opt, sched = _make(A, iters)
    st0 = {k: v.clone() for k, v in net.state_dict().items()}
    lossf = A.CrossEntropyLoss()
    gs = A.GraphedStep(net, lossf, *_batch(shape, 1), optimizer=opt, scheduler=sched, log_capacity=iters)
    net.load_state_dict(st0)
    ref, opt_r, sched_r = _make(A, iters)
    ref.load_state_dict(net.state_dict())
    (_, rw), (_, rb) = last_layer_params(ref)
    losses, lrs, beta1s, last, recs = [], [], [], [], []
    for it in range(iters):
        x, t = _batch(shape, 100 + it)
        la = gs.replay(x, t)
        lrs.append(opt_r.param_groups[0]["lr"]); beta1s.append(opt_r.param_groups[0]["betas"][0])
        opt_r.zero_grad()
        lb = lossf(ref(x), t)
        lb.backward()
        last.append((torch.linalg.vector_norm(rw.grad.double()).item(), torch.linalg.vector_norm(rb.grad.double()).item()))
        want, _ = _ref_norms([p.grad for p in ref.parameters()])
        opt_r.step()
        sched_r.step()
        recs.append((opt_r.grad_norm.item(), opt_r.clip_coef.item()))
        _close(recs[-1][0], want, f"eager norm, step {it}")
        assert torch.equal(la, lb), (it, la.item(), lb.item())
        losses.append(la.item())
        assert torch.equal(opt._clip_rec, opt_r._clip_rec), it
        for (k, p), q in zip(net.named_parameters(), ref.parameters()):
            assert torch.equal(p, q), (it, k)
        assert torch.equal(opt._m, opt_r._m) and torch.equal(opt._v, opt_r._v), it
        for (k, b), c in zip(net.named_buffers(), ref.buffers()):
            assert torch.equal(b, c), (it, k)
    print("norm, coefficient per step:", recs)
    assert any(c < 1.0 for _, c in recs)
    assert opt._step == opt_r._step == iters
    assert _state_equal(opt.state_dict(), opt_r.state_dict())
    assert _state_equal(sched.state_dict(), sched_r.state_dict())
    rows, dropped = gs.log()
    assert dropped == 0 and rows.shape == (iters, 7) and rows.dtype == np.float32
    assert np.array_equal(rows[:, 0], np.array(losses, np.float32))
    assert np.array_equal(rows[:, 1], np.array(lrs, np.float32))
    assert np.array_equal(rows[:, 2], np.array(beta1s, np.float32))
    want = np.array(last)
    assert np.all(np.abs(rows[:, 3:5].astype(np.float64) - want) <= 1e-6 * want), (rows[:, 3:5], want)
    assert np.array_equal(rows[:, 5], np.array([n for n, _ in recs], np.float32))
    assert np.array_equal(rows[:, 6], np.array([c for _, c in recs], np.float32))
    # max_grad_norm and norm_type are baked into the graph
    step0 = opt._step
    opt.max_grad_norm = 1.0
    with pytest.raises(RuntimeError, match="changed since the capture"):
        gs.replay()
    opt.max_grad_norm = 0.5
    opt.norm_type = INF
    with pytest.raises(RuntimeError, match="changed since the capture"):
        gs.replay()
    opt.norm_type = 2.0
    assert opt._step == step0
    gs.replay()
    torch.cuda.synchronize()


def test_unclipped_capture_keeps_five_log_columns():
    import pytorch_camvid_amd as A
    net, opt, sched = _make(A, 3, max_grad_norm=None)
    gs = A.GraphedStep(net, A.CrossEntropyLoss(), *_batch((2, 48, 64), 1), optimizer=opt, scheduler=sched, log_capacity=3)
    gs.replay()
    rows, _ = gs.log()
    assert rows.shape == (1, 5)
    opt.max_grad_norm = 1.0                                                # clipping switched on after the capture: refused
    with pytest.raises(RuntimeError, match="changed since the capture"):
        gs.replay()


def _child(args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.Popen([sys.executable, WORKER] + [str(a) for a in args], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _join(procs, timeout=420):
    """Wait for the children under one time limit each; the first failure stops the test (the rest are ended), nothing is started again."""
    try:
        for p in procs:
            out, _ = p.communicate(timeout=timeout)
            assert p.returncode == 0, f"child exited with {p.returncode}:\n{out[-3000:]}"
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()


def test_captured_clipped_iteration_is_reproducible_across_processes():
    with tempfile.TemporaryDirectory() as d:
        outs = [os.path.join(d, f"run{i}.json") for i in range(2)]
        for o in outs:                                                     # one after the other: two fresh processes
            _join([_child(["repro", o])])
        a, b = (json.load(open(o)) for o in outs)
    assert a["log_shape"] == [4, 7] and a["dropped"] == 0
    assert any(it["coef"] < 1.0 for it in a["iters"]), a["iters"]
    assert a == b


# ---- 10. bf16 mode -------------------------------------------------------------------------------------------------------------------------
def test_bf16_mode_gradients_are_fp32_and_clip_the_same_way(monkeypatch):
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    A.set_conv_precision(net, "bf16")
    opt = A.FlatAdamW(net, lr=2e-3, max_grad_norm=0.25)
    _backward(A, net, (2, 96, 128), 13)
    grads = [p.grad for p in net.parameters()]
    assert all(g.dtype == torch.float32 for g in grads)
    want, _ = _ref_norms(grads)
    opt.step()
    _close(opt.grad_norm.item(), want, "bf16 mode 2-norm")
    assert opt.clip_coef.item() == float(min(np.float32(1.0), np.float32(0.25) / (np.float32(opt.grad_norm.item()) + np.float32(1e-6))))
    _no_torch_fallback(monkeypatch)
    assert A.clip_grad_norm_(net, 1e30).item() == opt.grad_norm.item()


# ---- 11. data parallel -------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def test_data_parallel_clipped_loops_equal_the_single_process():
    """World size 1 over RCCL (every bucket really issued): the eager and the captured clipped loops under ddp.DataParallel equal the plain
    single-process loops bit for bit — the norm is taken from the all-reduced buffer, after GradSync.finish / the captured waits.  With two
    GPUs visible, world size 2 on two shards: both ranks record the same norm and coefficient bits at every step."""
    with tempfile.TemporaryDirectory() as d:
        single, w1 = os.path.join(d, "single.json"), os.path.join(d, "w1.json")
        _join([_child(["single", single])])
        _join([_child(["ddp", w1, 0, 1, _free_port()])])
        s, r = json.load(open(single)), json.load(open(w1))
        assert r["buckets"] >= 4
        assert any(it["coef"] < 1.0 for it in s["eager"]), s["eager"]
        assert s["eager"] == s["captured"]                                 # single process: captured == eager
        assert r["eager"] == s["eager"] and r["captured"] == s["captured"]
        assert r["log"] == s["log"] and r["log_shape"] == s["log_shape"] == [4, 7]
        if torch.cuda.device_count() >= 2:
            port = _free_port()
            outs = [os.path.join(d, f"w2r{k}.json") for k in range(2)]
            _join([_child(["ddp", outs[k], k, 2, port]) for k in range(2)])
            r0, r1 = (json.load(open(o)) for o in outs)
            for loop in ("eager", "captured"):
                assert [it["rec"] for it in r0[loop]] == [it["rec"] for it in r1[loop]], loop
