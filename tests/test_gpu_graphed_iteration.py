"""The whole training iteration (reference train.py:124-150) as ONE captured graph: GraphedStep(optimizer=FlatAdamW, scheduler=OneCycleLR,
log_capacity=...) against the eager loop `zero_grad; net(x); CE; backward; opt.step(); sched.step()` on a twin network, bit for bit —
loss, parameters, AdamW moments, BatchNorm statistics and the optimizer's state_dict; the per-iteration log against the twin's
values; the refusals after the optimizer is rebuilt or the network changes mode; the data-parallel form over a world-size-1 RCCL group."""
import json
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

LR = 2e-3


def dev():
    return torch.device("cuda:0")


def _batch(shape, seed):
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, h, w, generator=g).to(dev()), torch.randint(0, 12, (n, h, w), generator=g).to(dev())


def _make(A, model, iters, seed=0):
    torch.manual_seed(seed)
    net = A.get_model(model, 3, 12).to(dev()).train()
    opt = A.FlatAdamW(net, lr=LR, weight_decay=1e-2)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=LR, total_steps=iters + 4, cycle_momentum=True)
    return net, opt, sched


def _graphed(A, model, shape, iters, log_capacity, seed=0):
    net, opt, sched = _make(A, model, iters, seed)
    st0 = {k: v.clone() for k, v in net.state_dict().items()}
    lossf = A.CrossEntropyLoss()
    gs = A.GraphedStep(net, lossf, *_batch(shape, 1), optimizer=opt, scheduler=sched, log_capacity=log_capacity)
    net.load_state_dict(st0)                      # the capture's warm-up passes advanced the BatchNorm statistics
    return net, opt, sched, gs


def _state_equal(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_state_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_state_equal(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("model,shape", [("unet", (2, 48, 64)), ("unet", (2, 360, 480)), ("segnet", (2, 48, 64))])
def test_captured_iteration_is_bitwise_the_eager_loop(model, shape):
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd.graph import last_layer_params
    iters = 8
    net, opt, sched, gs = _graphed(A, model, shape, iters, log_capacity=iters)
    ref, opt_r, sched_r = _make(A, model, iters)
    ref.load_state_dict(net.state_dict())
    lossf = A.CrossEntropyLoss()
    (_, rw), (_, rb) = last_layer_params(ref)
    losses, lrs, beta1s, norms = [], [], [], []
    for it in range(iters):
        x, t = _batch(shape, 100 + it)
        la = gs.replay(x, t)
        lrs.append(opt_r.param_groups[0]["lr"]); beta1s.append(opt_r.param_groups[0]["betas"][0])
        opt_r.zero_grad()
        lb = lossf(ref(x), t)
        lb.backward()
        norms.append((torch.linalg.vector_norm(rw.grad.double()).item(), torch.linalg.vector_norm(rb.grad.double()).item()))
        opt_r.step()
        sched_r.step()
        assert torch.equal(la, lb), (it, la.item(), lb.item())
        losses.append(la.item())
        for (k, p), q in zip(net.named_parameters(), ref.parameters()):
            assert torch.equal(p, q), (it, k)
        assert torch.equal(opt._m, opt_r._m) and torch.equal(opt._v, opt_r._v), it
        for (k, b), c in zip(net.named_buffers(), ref.buffers()):
            assert torch.equal(b, c), (it, k)
        assert opt.param_groups[0]["lr"] == opt_r.param_groups[0]["lr"]
        assert opt.param_groups[0]["betas"] == opt_r.param_groups[0]["betas"]
    assert opt._step == opt_r._step == iters
    assert _state_equal(opt.state_dict(), opt_r.state_dict())
    assert _state_equal(sched.state_dict(), sched_r.state_dict())

    rows, dropped = gs.log()
    assert dropped == 0 and rows.shape == (iters, 5) and rows.dtype == np.float32
    assert np.array_equal(rows[:, 0], np.array(losses, np.float32))                   # the replayed loss, bit for bit
    assert np.array_equal(rows[:, 1], np.array(lrs, np.float32))                      # the lr / beta1 the step used
    assert np.array_equal(rows[:, 2], np.array(beta1s, np.float32))
    want = np.array(norms)
    assert np.all(np.abs(rows[:, 3:].astype(np.float64) - want) <= 1e-6 * want), (rows[:, 3:], want)
    r2, d2 = gs.log()
    assert r2.shape == (0, 5) and d2 == 0                                              # nothing new since the last read

    # the captured steps continue as eager ones: the same optimizer, the step count kept on the host
    for _ in range(2):
        opt.step()
        opt_r.step()
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        assert torch.equal(p, q), k
    assert torch.equal(opt._m, opt_r._m) and opt._step == opt_r._step == iters + 2


def test_log_ring_wraps_around_and_is_reproducible():
    import pytorch_camvid_amd as A
    shape = (2, 48, 64)
    logs = []
    for run in range(2):
        net, opt, sched, gs = _graphed(A, "unet", shape, 5, log_capacity=3, seed=7)
        losses = []
        for it in range(5):
            losses.append(gs.replay(*_batch(shape, 200 + it)).item())
        rows, dropped = gs.log()
        assert dropped == 2 and rows.shape == (3, 5)
        assert np.array_equal(rows[:, 0], np.array(losses[2:], np.float32))        # the newest three, oldest first
        gs.replay(*_batch(shape, 300))
        r1, d1 = gs.log()
        assert d1 == 0 and r1.shape == (1, 5)
        logs.append(np.concatenate([rows, r1]))
        del gs
    assert logs[0].tobytes() == logs[1].tobytes()


def test_replay_refuses_a_rebuilt_optimizer_or_eval_mode():
    import pytorch_camvid_amd as A
    shape = (2, 48, 64)
    net, opt, sched, gs = _graphed(A, "unet", shape, 4, log_capacity=0)
    gs.replay(*_batch(shape, 2))
    A.FlatAdamW(net, lr=LR)                       # re-homes every parameter into a new flat buffer
    with pytest.raises(RuntimeError, match="changed since the capture"):
        gs.replay(*_batch(shape, 3))
    net, opt, sched, gs = _graphed(A, "unet", shape, 4, log_capacity=2)
    step0 = opt._step
    net.eval()
    with pytest.raises(RuntimeError, match="changed since the capture"):
        gs.replay(*_batch(shape, 3))
    assert opt._step == step0                     # a refused replay does not count a step
    net.train()
    gs.replay(*_batch(shape, 3))
    torch.cuda.synchronize()


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def test_world1_rccl_captured_iteration_equals_eager_data_parallel_loop():
    """GraphedStep(allow_grad_sync=True, optimizer=FlatAdamW, scheduler=OneCycleLR) under ddp.DataParallel: the AdamW step is captured
    after the all-reduces and the four iterations equal the eager data-parallel loop bit for bit (tests/graphed_ddp_worker.py, in a
    child process so that the group dies with it)."""
    from tests.graphed_ddp_worker import run
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "w1.json")
        mp.spawn(run, args=(_free_port(), out), nprocs=1, join=True)
        res = json.load(open(out))
    assert res["buckets"] >= 4 and res["step"] == [4, 4]
    for it, r in enumerate(res["iters"]):
        assert r["loss"] and r["params"] and r["moments"] and r["bn"], (it, r)
