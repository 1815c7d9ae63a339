"""Gradient accumulation over micro-batches on the device: cvk_grad_accumulate against numpy float32 (bitwise), a window through
GradAccumulator against its restatement in torch fp32 (bitwise) and against the fp64 oracle, optimizers stepped on the window's
gradient, the window captured by GraphedStep, and the eager data-parallel path (two ranks over gloo, a world-1 RCCL group)."""
import copy
import json
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

SHAPE = (2, 48, 64)
ENCODER = ("down1", "down2", "down3", "down4", "down5")


def dev():
    return torch.device("cuda:0")


def _batch(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n, h, w = shape
    return torch.randn(n, 3, h, w, generator=g), torch.randint(0, 12, (n, h, w), generator=g)


def _dbatch(shape, seed):
    return tuple(v.to(dev()) for v in _batch(shape, seed))


def _zero(net):
    for p in net.parameters():
        p.grad = None


# ---- 4. the kernel ---------------------------------------------------------------------------------------------------------------------------
NAN_BITS = 0x7FC00ABC
LENGTHS = (1, 3, 4, 5, 1023, 2_500_003)


def _tables():
    """Two segment tables over one buffer: every segment starts on a multiple of 4 floats / on 1, 2 or 3 floats past one."""
    out = []
    for shifts in ((0,) * len(LENGTHS), (1, 2, 3, 1, 2, 3)):
        segs, o = [], 8
        for n, s in zip(LENGTHS, shifts):
            o = (o + 3) // 4 * 4 + s
            segs.append((o, n))
            o += n + 5                                  # a gap of uncovered floats behind every segment
        out.append((segs, o + 9))
    return out


@pytest.mark.parametrize("table", [0, 1])
@pytest.mark.parametrize("mode,scale", [(0, 1.0), (1, 1.0), (2, 1.0 / 3), (2, 0.25), (2, 1.0)])
def test_kernel_against_numpy_float32_bitwise(table, mode, scale):
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd import accumulate
    segs, n = _tables()[table]
    assert all((o % 4 == 0) == (table == 0) for o, _ in segs)
    rng = np.random.default_rng(7 + table)
    d = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(np.float32)
    s = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(np.float32)
    inside = np.zeros(n, bool)
    for o, m in segs:
        inside[o:o + m] = True
    d.view(np.uint32)[~inside] = NAN_BITS               # whatever lies outside the table must come back bit-identical ...
    s.view(np.uint32)[~inside] = NAN_BITS               # ... and must not be read into anything
    sc = np.float32(scale)
    want = d.copy()
    with np.errstate(all="ignore"):
        if mode == 0:
            want[inside] = s[inside]
        elif mode == 1:
            want[inside] = d[inside] + s[inside]
        else:
            want[inside] = (d[inside] + s[inside]).astype(np.float32) * sc
    assert want.dtype == np.float32
    dt, st = torch.from_numpy(d.copy()).to(dev()), torch.from_numpy(s.copy()).to(dev())
    tab = accumulate._Table(segs, n, dev())
    rc = A.load_library().cvk_grad_accumulate(dt.data_ptr(), st.data_ptr(), n, tab.table.data_ptr(), tab.nseg, tab.blocks, mode, float(sc),
                                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    got = dt.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert np.array_equal(st.cpu().numpy().view(np.uint32), s.view(np.uint32))      # the source is read only
    assert int((got.view(np.uint32) == NAN_BITS).sum()) == int((~inside).sum())


# ---- 5. a window against its restatement -----------------------------------------------------------------------------------------------------
def _twins(kind="unet", seed=3, setup=None):
    import pytorch_camvid_amd as A
    torch.manual_seed(seed)
    mk = A.UNet if kind == "unet" else A.SegNet
    a, b = mk(3, 12).to(dev()).train(), mk(3, 12).to(dev()).train()
    b.load_state_dict(a.state_dict())
    for net in (a, b):
        if setup is not None:
            setup(A, net)
    return a, b


def _restated(net, lossf, batches, mean):
    """(per-parameter expected gradient or None, per-micro-batch losses): the K micro-batches one at a time with zero_grad in between,
    ((g1 + g2) + ... + gK) * float32(1 / K) in torch fp32."""
    total, losses = None, []
    for x, t in batches:
        _zero(net)
        loss = lossf(net(x), t)
        loss.backward()
        losses.append(loss.detach().clone())
        gs = [None if p.grad is None else p.grad.detach().clone() for p in net.parameters()]
        total = gs if total is None else [None if u is None else u + v for u, v in zip(total, gs)]
    _zero(net)
    if mean:
        k = torch.tensor(np.float32(1.0 / len(batches)), device=dev())
        total = [None if u is None else u * k for u in total]
    return total, losses


def _window(net, acc, lossf, batches, check_untouched=True):
    """The same micro-batches through the accumulator; returns the micro-batch losses."""
    before = [p.detach().clone() for p in net.parameters()] if check_untouched else None
    losses = []
    for k, (x, t) in enumerate(batches):
        assert acc.micro_step == k
        loss = lossf(net(x), t)
        loss.backward()
        losses.append(loss.detach().clone())
        if k < len(batches) - 1:
            assert not acc.ready
            assert all(p.grad is None for p in net.parameters()), k
            if check_untouched:
                assert all(torch.equal(p, q) for p, q in zip(net.parameters(), before)), k
    assert acc.ready and acc.micro_step == 0
    return losses


def _check_window(kind, K, mean, setup=None, frozen=()):
    import pytorch_camvid_amd as A
    a, b = _twins(kind, setup=setup)
    lossf = A.CrossEntropyLoss()
    batches = [_dbatch(SHAPE, 40 + k) for k in range(K)]
    want, la = _restated(a, lossf, batches, mean)
    acc = A.GradAccumulator(b, steps=K, mean=mean)
    n0 = acc.launches
    lb = _window(b, acc, lossf, batches)
    assert acc.launches - n0 == K                       # one launch per micro-batch
    assert all(torch.equal(u, v) for u, v in zip(la, lb))
    for (k, p), w in zip(b.named_parameters(), want):
        if k.split(".")[0] in frozen:
            assert p.grad is None and w is None, k
            continue
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.equal(p.grad, w), (k, K, mean)
    for (k, u), v in zip(a.named_buffers(), b.buffers()):      # running statistics: updated per micro-batch, as one at a time
        assert torch.equal(u, v), k
    return a, b, acc


@pytest.mark.parametrize("mean", [True, False])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_window_is_bitwise_its_restatement(K, mean):
    _check_window("unet", K, mean)


def test_window_segnet():
    _check_window("segnet", 3, True)


def test_window_bf16_mode():
    """bf16 storage: parameter gradients are fp32 in the same flat layout, the same fold serves them."""
    _check_window("unet", 3, True, setup=lambda A, net: A.set_conv_precision(net, "bf16"))


def test_window_frozen_encoder():
    def freeze(A, net):
        for s in ENCODER:
            getattr(net, s).requires_grad_(False)
            getattr(net, s).eval()
    _check_window("unet", 3, True, setup=freeze, frozen=ENCODER)


def test_detach_and_steps_one_restore_the_plain_backward():
    import pytorch_camvid_amd as A
    a, b = _twins()
    lossf = A.CrossEntropyLoss()
    x, t = _dbatch(SHAPE, 5)
    lossf(a(x), t).backward()
    acc = A.GradAccumulator(b, steps=1)
    lossf(b(x), t).backward()
    assert acc.ready and acc.launches == 0 and acc._buf is None
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(a.parameters(), b.parameters()))
    acc.steps = 2
    _zero(b)
    lossf(b(x), t).backward()
    assert all(p.grad is None for p in b.parameters())
    acc.detach()
    lossf(b(x), t).backward()
    assert all(p.grad is not None for p in b.parameters())


def _step_launches(net, x, t):
    """[(kernel name, (op index, direction))] of one forward + backward, from the executor's own launch record (engine.PROF / PROF_OPS)."""
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd import engine
    _zero(net)
    torch.cuda.synchronize()
    engine.PROF, engine.PROF_OPS = [], []
    try:
        A.CrossEntropyLoss()(net(x), t).backward()
        torch.cuda.synchronize()
        return [(r[0], op) for r, op in zip(engine.PROF, engine.PROF_OPS)]
    finally:
        engine.PROF, engine.PROF_OPS = None, None


def test_launch_sequence_without_a_window_is_the_plain_one():
    """A network that never had an accumulator, one with steps=1 attached and one after detach() record the same launches in the same order
    (the executor's launch record: every timed kernel of forward and backward with the op that issued it)."""
    import pytorch_camvid_amd as A
    a, b = _twins()
    x, t = _dbatch(SHAPE, 5)
    for net in (a, b):                                  # the first pass of a network records its weight-transform jobs: warm both alike
        _step_launches(net, x, t)
    want = _step_launches(a, x, t)
    assert len(want) > 100
    acc = A.GradAccumulator(b, steps=1)
    assert _step_launches(b, x, t) == want and acc.launches == 0
    acc.steps = 2
    first = _step_launches(b, x, t)                     # an open window: the same kernels (the fold is not a timed executor launch)
    assert first == want and acc.launches == 1
    acc.detach()
    assert _step_launches(b, x, t) == want and acc.launches == 1
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(a.parameters(), b.parameters()))


def test_replay_is_refused_in_the_middle_of_an_eager_window():
    import pytorch_camvid_amd as A
    a, b = _twins()
    lossf = A.CrossEntropyLoss()
    acc = A.GradAccumulator(b, steps=2)
    xs, ts = zip(*[_dbatch(SHAPE, 7 + k) for k in range(2)])
    gs = A.GraphedStep(b, lossf, torch.stack(xs), torch.stack(ts), accumulator=acc)
    lossf(b(xs[0]), ts[0]).backward()                   # an eager micro-step opens a window
    assert acc.micro_step == 1
    with pytest.raises(RuntimeError, match="middle of an eager window"):
        gs.replay()
    acc.reset()
    gs.replay()
    torch.cuda.synchronize()
    assert acc.micro_step == 0 and all(p.grad is not None for p in b.parameters())


def test_input_gradient_is_returned_on_every_micro_step():
    import pytorch_camvid_amd as A
    a, b = _twins()
    lossf = A.CrossEntropyLoss()
    acc = A.GradAccumulator(b, steps=2)
    for k in range(2):
        x, t = _dbatch(SHAPE, 60 + k)
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        _zero(a)
        lossf(a(xa), t).backward()
        lossf(b(xb), t).backward()
        assert xb.grad is not None and torch.equal(xa.grad, xb.grad), k
    assert acc.ready


# ---- 6. against the fp64 oracle --------------------------------------------------------------------------------------------------------------
def test_window_mean_against_the_fp64_oracle():
    """The window's mean gradient against oracle/torch_ref.py run in fp64 on the same K micro-batches and averaged in fp64.  The tolerance is
    the per-parameter gradient tolerance of a single batch at this geometry, tests/test_gpu_finetune.py:46-58 (_grad_tolerances):
    ||g - g64|| <= max(4 x the reference graph's own fp32-vs-fp64 distance, 1e-3) x ||g64||.  K gradients each within their own bound have
    a mean within the mean of the bounds (triangle inequality), which is what is asserted.  That source was preferred over
    tests/test_gpu_train_parity.py (no gradient tolerance: it compares loss trajectories) and tests/test_gpu_nets.py:156-165 (gradient NORMS
    against goldens, relative 0.25): it is the one existing per-parameter, element-wise single-batch gradient bound at this 2 x 48 x 64
    geometry, and it is the stricter of the candidates.  Conv biases in front of a training-mode
    BatchNorm have a zero true gradient; they are held to the absolute bound of tests/test_gpu_nets.py:160 (|g| < 1e-4)."""
    import pytorch_camvid_amd as A
    from oracle import torch_ref as R
    K = 3
    torch.manual_seed(4)
    ref = R.build("unet", 3, 12).train()
    net = A.UNet(3, 12).to(dev()).train()
    net.load_state_dict(ref.state_dict())
    r64 = copy.deepcopy(ref).double()
    names = [k for k, _ in ref.named_parameters()]
    mean64 = [torch.zeros_like(p) for p in r64.parameters()]
    bound = [0.0] * len(names)
    batches = [_batch(SHAPE, 70 + k) for k in range(K)]
    for x, t in batches:
        for m in (ref, r64):
            for p in m.parameters():
                p.grad = None
        torch.nn.functional.cross_entropy(ref(x), t).backward()
        torch.nn.functional.cross_entropy(r64(x.double()), t).backward()
        for i, (q, q64) in enumerate(zip(ref.parameters(), r64.parameters())):
            n64 = float(q64.grad.norm())
            drift = float((q.grad.double() - q64.grad).norm()) / n64 if n64 > 0 else 0.0
            bound[i] += max(4.0 * drift, 1e-3) * n64 / K
            mean64[i] += q64.grad / K
    acc = A.GradAccumulator(net, steps=K)
    lossf = A.CrossEntropyLoss()
    _window(net, acc, lossf, [(x.to(dev()), t.to(dev())) for x, t in batches], check_untouched=False)
    worst = 0.0
    for i, (k, p) in enumerate(net.named_parameters()):
        if k.endswith("conv.0.bias"):
            assert p.grad.abs().max().item() < 1e-4, k
            continue
        err = float((p.grad.detach().cpu().double() - mean64[i]).norm())
        worst = max(worst, err / bound[i])
        print(f"{k}: |window mean - fp64 mean| {err:.3e}, bound {bound[i]:.3e}")
        assert err <= bound[i], (k, err, bound[i])
    print(f"largest error / bound over all parameters: {worst:.3f}")


# ---- 7. optimizers ---------------------------------------------------------------------------------------------------------------------------
def _opt(A, net, which, windows):
    if which == "flat":
        opt = A.FlatAdamW(net, lr=1e-3, max_grad_norm=0.5)
    else:
        opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    return opt, torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=2e-3, total_steps=windows + 4)


def _set_grads(net, grads):
    for p, g in zip(net.parameters(), grads):
        p.grad = None if g is None else g.clone()


@pytest.mark.parametrize("which", ["flat", "torch"])
def test_two_windows_equal_the_optimizer_stepped_on_the_restated_mean(which):
    import pytorch_camvid_amd as A
    K, windows = 3, 2
    a, b = _twins()
    oa, sa = _opt(A, a, which, windows)
    ob, sb = _opt(A, b, which, windows)
    lossf = A.CrossEntropyLoss()
    acc = A.GradAccumulator(b, steps=K)
    for w in range(windows):
        batches = [_dbatch(SHAPE, 200 + 10 * w + k) for k in range(K)]
        want, _ = _restated(a, lossf, batches, True)
        _set_grads(a, want)
        oa.step(); sa.step(); oa.zero_grad(set_to_none=True)
        for k, (x, t) in enumerate(batches):
            lossf(b(x), t).backward()
            before = [p.detach().clone() for p in b.parameters()] if k < K - 1 else None
            if not acc.ready:                           # the loop of the README: a step before the window closes is a no-op
                ob.step()
                assert all(torch.equal(p, q) for p, q in zip(b.parameters(), before))
            else:
                ob.step(); sb.step(); ob.zero_grad(set_to_none=True)
        for (k, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p, q), (w, k)
        if which == "flat":
            assert torch.equal(oa._m, ob._m) and torch.equal(oa._v, ob._v), w
            assert oa._step == ob._step == w + 1 and oa._steps == ob._steps
            assert torch.equal(oa._clip_rec, ob._clip_rec), w       # grad_norm and clip_coef of the window's gradient
            assert float(ob.clip_coef) < 1.0
        else:
            for p, q in zip(a.parameters(), b.parameters()):
                sp, sq = oa.state[p], ob.state[q]
                assert torch.equal(sp["exp_avg"], sq["exp_avg"]) and torch.equal(sp["exp_avg_sq"], sq["exp_avg_sq"])
                assert float(sp["step"]) == float(sq["step"]) == w + 1
        for (k, u), v in zip(a.named_buffers(), b.buffers()):
            assert torch.equal(u, v), k


# ---- 8. the captured window ------------------------------------------------------------------------------------------------------------------
def test_captured_window_is_bitwise_the_eager_window_loop():
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd.graph import last_layer_params
    K, replays = 3, 3
    a, b = _twins()
    oa, sa = _opt(A, a, "flat", replays)
    ob, sb = _opt(A, b, "flat", replays)
    lossf = A.CrossEntropyLoss()
    acc_a = A.GradAccumulator(a, steps=K)
    acc_b = A.GradAccumulator(b, steps=K)
    with pytest.raises(NotImplementedError, match="allow_grad_sync"):
        A.GraphedStep(b, lossf, torch.zeros(K, *SHAPE[:1], 3, *SHAPE[1:], device=dev()), torch.zeros(K, *SHAPE, dtype=torch.long, device=dev()),
                      allow_grad_sync=True, optimizer=ob, accumulator=acc_b)
    st0 = {k: v.clone() for k, v in b.state_dict().items()}

    def window(seed):
        xs, ts = zip(*[_dbatch(SHAPE, seed + k) for k in range(K)])
        return torch.stack(xs), torch.stack(ts)
    gs = A.GraphedStep(b, lossf, *window(1), optimizer=ob, scheduler=sb, log_capacity=replays, accumulator=acc_b)
    b.load_state_dict(st0)
    assert acc_b.micro_step == 0
    (_, rw), (_, rb) = last_layer_params(a)
    want_rows = []
    for it in range(replays):
        x, t = window(300 + 10 * it)
        lg = gs.replay(x, t)
        lr, beta1 = oa.param_groups[0]["lr"], oa.param_groups[0]["betas"][0]
        micro = []
        for k in range(K):
            loss = lossf(a(x[k]), t[k])
            loss.backward()
            micro.append(loss.detach())
        assert acc_a.ready
        le = torch.stack(micro).mean()                  # the fp32 mean of the eager micro-losses
        last = (torch.linalg.vector_norm(rw.grad.double()).item(), torch.linalg.vector_norm(rb.grad.double()).item())
        oa.step(); sa.step()
        want_rows.append((le.item(), lr, beta1, last, oa.grad_norm.item(), oa.clip_coef.item()))
        oa.zero_grad(set_to_none=True)
        assert torch.equal(lg, le), (it, lg.item(), le.item())
        for (k, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p, q), (it, k)
        assert torch.equal(oa._m, ob._m) and torch.equal(oa._v, ob._v) and torch.equal(oa._clip_rec, ob._clip_rec), it
        for (k, u), v in zip(a.named_buffers(), b.buffers()):
            assert torch.equal(u, v), (it, k)
    assert oa._step == ob._step == replays and oa._steps == ob._steps
    rows, dropped = gs.log()
    assert dropped == 0 and rows.shape == (replays, 7)  # one row per update
    for row, (le, lr, beta1, last, gn, cc) in zip(rows, want_rows):
        assert row[0] == np.float32(le) and row[1] == np.float32(lr) and row[2] == np.float32(beta1)
        assert abs(float(row[3]) - last[0]) <= 1e-6 * last[0] and abs(float(row[4]) - last[1]) <= 1e-6 * last[1]
        assert row[5] == np.float32(gn) and row[6] == np.float32(cc)
    # the accumulator's identity, steps and mean are baked into the graph
    step0 = ob._step
    acc_b.steps = K + 1
    with pytest.raises(RuntimeError, match="changed since the capture"):
        gs.replay()
    acc_b.steps = K
    acc_b.mean = False
    with pytest.raises(RuntimeError, match="changed since the capture"):
        gs.replay()
    acc_b.mean = True
    assert ob._step == step0
    gs.replay()
    torch.cuda.synchronize()


# ---- 9. data parallel, eager -----------------------------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def test_two_ranks_accumulate_then_exchange_once():
    """Two ranks on this GPU over gloo (tests/accumulate_gpu_worker.py): no collective on the non-closing micro-steps, every bucket once
    on the closing one, bitwise equal gradients on both ranks, equal to the mean over ranks of the per-rank restated means within the
    tolerance of the existing two-rank test for a single backward (tests/test_gpu_ddp.py:66: rtol 1e-6, atol 1e-12)."""
    from tests.accumulate_gpu_worker import run
    K = 3
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(run, args=(2, free_port(), d, SHAPE, K), nprocs=2, join=True)
        r0, r1 = torch.load(os.path.join(d, "rank0.pt")), torch.load(os.path.join(d, "rank1.pt"))
    for r in (r0, r1):
        assert r["launched"][:K - 1] == [[]] * (K - 1)
        last = r["launched"][K - 1]
        assert len(last) >= 4 and last[0][0] == 0 and len(set(last)) == len(last)
        assert r["folded"] == last and r["none_before_close"]
    assert r0["launched"] == r1["launched"]
    for a, b in zip(r0["grads"], r1["grads"]):
        assert torch.equal(a, b)
    assert any(not torch.equal(a, b) for a, b in zip(r0["restated"], r1["restated"]))     # the shards differ
    for i, (a, b) in enumerate(zip(r0["restated"], r1["restated"])):
        assert torch.allclose(r0["grads"][i], (a + b) / 2, rtol=1e-6, atol=1e-12), i


def _world1_worker(rank, port, out_path):
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd import ddp
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(dev())
    ddp.init_process_group("nccl", rank=0, world_size=1, device_id=dev())
    K = 3
    a, b = _twins()
    lossf = A.CrossEntropyLoss()
    wrapped = ddp.DataParallel(b, always_issue=True, bucket_mb=8.0)
    issued = []
    real = wrapped.sync._issue
    wrapped.sync._issue = lambda call, t: issued.append(int(t.numel())) or real(call, t)
    lossf(wrapped(*_dbatch(SHAPE, 1)[:1]), _dbatch(SHAPE, 1)[1]).backward()
    one = len(issued)
    _zero(b)
    acc = A.GradAccumulator(wrapped, steps=K)
    batches = [_dbatch(SHAPE, 40 + k) for k in range(K)]
    want, _ = _restated(a, lossf, batches, True)
    del issued[:]
    per_step = []
    for x, t in batches:
        lossf(wrapped(x), t).backward()
        per_step.append(len(issued))
    torch.cuda.synchronize()
    res = {"buckets_one_backward": one, "per_step": per_step, "launches": acc.launches,
           "equal": all(torch.equal(p.grad, w) for p, w in zip(b.parameters(), want))}
    with open(out_path, "w") as f:
        json.dump(res, f)
    torch.distributed.destroy_process_group()


def test_world1_rccl_collectives_per_window():
    """A world-1 RCCL group with always_issue: the collectives of a whole window are the buckets of ONE backward, the fold runs once per
    bucket on the closing micro-step, and the result is bitwise the restated mean (AVG over one rank)."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "w1.json")
        mp.spawn(_world1_worker, args=(free_port(), out), nprocs=1, join=True)
        res = json.load(open(out))
    b = res["buckets_one_backward"]
    assert b >= 4 and res["per_step"] == [0, 0, b], res
    assert res["launches"] == 2 + b and res["equal"], res
