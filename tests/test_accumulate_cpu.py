"""Gradient accumulation on the host side (no GPU): the window state machine of GradAccumulator, the argument check of
cvk_grad_accumulate, the per-bucket fold tables of the data-parallel path, and the synchroniser switch (no_sync, non-closing
micro-steps) under gloo with CPU tensors."""
import os
import socket
import tempfile

import pytest
import torch
import torch.multiprocessing as mp

import pytorch_camvid_amd as A
from pytorch_camvid_amd import accumulate, ddp, engine
from pytorch_camvid_amd.modules import runner_of
from pytorch_camvid_amd.optim import norm_segments

ENCODER = ("down1", "down2", "down3", "down4", "down5")


def _plan(net, N=1, H=32, W=32):
    plan = engine.Plan(N, 3, H, W)
    plan.output = net._emit(plan, plan.input)
    plan.seal()
    names = {id(m): n for n, m in net.named_modules()}
    for op in plan.convs:
        op.name = names[id(op.holder)]
    return plan


class _St:
    """What engine.Runner.backward has in its RunState when it opens a pass (host side only)."""

    def __init__(self, plan, fill=None):
        self.params = [t for h in plan.holders for t in h.block_params()]
        self.goffs, self.total = engine.layout_grads(self.params)
        self.gflat = torch.zeros(self.total) if fill is None else fill
        self.device = self.gflat.device
        self.fold = None


def _pass(acc, net, plan=None):
    """One backward pass as the executor drives the accumulator, without the launches."""
    plan = plan or _plan(net)
    st = _St(plan)
    fold = acc.open_pass(st, plan, st.total)
    if fold is not None:
        fold.done()
    return fold


def test_window_state_machine_two_windows_reset_and_detach():
    net = A.UNet(3, 12).train()
    acc = A.GradAccumulator(net, steps=3)
    assert runner_of(net).accumulator is acc and acc.attached
    assert (acc.ready, acc.micro_step, acc.scale) == (False, 0, 1.0 / 3)
    plan = _plan(net)
    seen = []
    for _ in range(2):                                  # two windows
        for k in range(3):
            f = _pass(acc, net, plan)
            seen.append((f.mode, f.closing, acc.ready, acc.micro_step))
    assert seen == [(0, False, False, 1), (1, False, False, 2), (2, True, True, 0)] * 2
    _pass(acc, net, plan)
    assert acc.micro_step == 1 and not acc.ready
    acc.reset()                                         # drop the partial window
    assert acc.micro_step == 0 and not acc.ready
    assert _pass(acc, net, plan).mode == 0              # a new window starts with the initialising fold
    acc.reset()
    acc.detach()
    assert runner_of(net).accumulator is None and not acc.attached
    again = A.GradAccumulator(net, steps=2, mean=False) # a detached network takes a new one
    assert again.scale == 1.0


def test_steps_one_is_no_accumulator():
    net = A.UNet(3, 12).train()
    acc = A.GradAccumulator(net, steps=1)
    assert _pass(acc, net) is None and acc.ready and acc.micro_step == 0


def test_refusals():
    net = A.UNet(3, 12).train()
    for bad in (0, -1, 1.5, True, "2"):
        with pytest.raises((ValueError, TypeError)):
            A.GradAccumulator(net, steps=bad)
    assert runner_of(net).accumulator is None           # a refused construction attaches nothing
    acc = A.GradAccumulator(net, steps=2)
    with pytest.raises(RuntimeError, match="already has an accumulator"):
        A.GradAccumulator(net, steps=4)
    with pytest.raises(ValueError):
        acc.steps = 0
    _pass(acc, net)
    with pytest.raises(RuntimeError, match="middle of a window"):
        acc.steps = 3


def test_mid_window_change_of_the_trainable_set_is_refused_by_name():
    net = A.UNet(3, 12).train()
    acc = A.GradAccumulator(net, steps=2)
    _pass(acc, net)
    net.down2.requires_grad_(False)
    with pytest.raises(RuntimeError, match=r"middle of a window.*requires_grad of the conv weight of down2\.0"):
        _pass(acc, net)
    assert acc.micro_step == 1                          # the refused pass did not advance the window
    net.down2.requires_grad_(True)
    net.down3.eval()
    with pytest.raises(RuntimeError, match=r"BatchNorm mode \(train / eval\) of down3\.0"):
        _pass(acc, net)
    net.train()
    assert _pass(acc, net).closing and acc.ready
    net.down2.requires_grad_(False)                     # between windows it is fine
    assert _pass(acc, net).mode == 0
    # another input geometry inside the window: same parameters, same layout
    assert _pass(acc, net, _plan(net, 2, 48, 64)).closing


def test_grad_accumulate_argument_errors_return_einval_without_a_launch():
    lib = A.load_library()
    ok = dict(dst=4096, src=8192, n=64, seg=16384, nseg=1, nb=1, mode=1, scale=1.0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cvk_grad_accumulate(a["dst"], a["src"], a["n"], a["seg"], a["nseg"], a["nb"], a["mode"], a["scale"], None)
    for kw, word in ((dict(dst=None), b"null"), (dict(src=None), b"null"), (dict(seg=None), b"null"), (dict(mode=3), b"mode 3"),
                     (dict(mode=-1), b"mode -1"), (dict(scale=float("inf")), b"not finite"), (dict(scale=float("nan")), b"not finite"),
                     (dict(dst=4100), b"misaligned"), (dict(src=8200), b"misaligned"), (dict(n=0), b"empty"), (dict(nb=0), b"empty"),
                     (dict(src=4096), b"same buffer")):
        assert call(**kw) == -1 and word in lib.cvk_last_error_string(), (kw, lib.cvk_last_error_string())


def _bucket_tables(net, bucket_mb):
    plan = _plan(net, 8, 360, 480)
    st = _St(plan, fill=torch.empty(0))

    class Owner:
        bucket_floats = int(bucket_mb * (1 << 20) / 4)
    call = ddp._SyncCall(Owner(), st, plan)
    segs = accumulate.fold_segments(plan, st.params, st.goffs)
    return plan, st, call.buckets, segs


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("bucket_mb", [0.25, 32.0])
def test_bucket_fold_tables_tile_the_trainable_norm_table(frozen, bucket_mb):
    net = A.UNet(3, 12).train()
    if frozen:                                          # the frozen-encoder pattern of tests/test_finetune_plan_cpu.py
        for s in ENCODER:
            getattr(net, s).requires_grad_(False)
            getattr(net, s).eval()
    plan, st, buckets, segs = _bucket_tables(net, bucket_mb)
    want = norm_segments((o, p.numel()) for o, p in zip(st.goffs, st.params) if p.requires_grad)
    assert segs == want and len(buckets) >= (2 if frozen or bucket_mb < 1 else 4)
    pieces = []
    for lo, hi, _ in buckets:
        part = accumulate.clip_segments(segs, lo, hi)
        assert part and all(lo <= o and o + n <= hi for o, n in part)
        accumulate.plan_table(part, st.total)           # the library accepts every bucket's table
        pieces.extend(part)
    # norm_segments refuses overlaps and merges exact neighbours: the union of the bucket tables is the table itself
    assert norm_segments(pieces) == want
    assert sum(n for _, n in pieces) == sum(p.numel() for p in st.params if p.requires_grad)
    covered = torch.zeros(st.total, dtype=torch.int8)
    for o, n in pieces:
        covered[o:o + n] += 1
    assert int(covered.max()) == 1
    for o, p in zip(st.goffs, st.params):
        assert int(covered[o:o + p.numel()].sum()) == (p.numel() if p.requires_grad else 0)
        pad = (p.numel() + 3) // 4 * 4
        assert int(covered[o + p.numel():o + pad].sum()) == 0       # no alignment padding either


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _sync_switch_rank(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    torch.manual_seed(5)
    net = A.UNet(3, 12).train()
    wrapped = ddp.DataParallel(net, bucket_mb=0.25, broadcast=False)
    acc = A.GradAccumulator(wrapped, steps=3)
    R = runner_of(net)
    assert R.accumulator is acc                         # attached to the wrapped module's runner
    plan = _plan(net)
    made = []
    real_begin = wrapped.sync.begin
    wrapped.sync.begin = lambda st, plan=None: made.append(1) or real_begin(st, plan)
    log = []

    def one_pass():
        g = torch.Generator().manual_seed(100 * rank + len(log))
        st = _St(plan)
        st.gflat = torch.randn(st.total, generator=g)
        before = st.gflat.clone()
        fold = R.accumulator.open_pass(st, plan, st.total) if R.accumulator is not None else None
        if fold is not None:
            fold.bucket = lambda st_, lo, hi: fold.folded.append((lo, hi))      # host side only: record, no launch
        st.fold = fold
        n0 = len(made)
        call = R.begin_sync(st, plan, fold)
        if call is not None:
            for slot in range(len(plan.convs) - 1, -1, -1):
                call.layer_done(st, slot)
            call.finish(st)
        if fold is not None:
            fold.done()
        log.append({"created": len(made) - n0, "launched": list(wrapped.sync.launched), "changed": not torch.equal(before, st.gflat),
                    "folded": list(fold.folded) if fold is not None else None})
    for _ in range(3):                                  # one window: two silent micro-steps, then the exchange
        one_pass()
    acc.detach()
    with wrapped.no_sync():                             # torch's contract: no collective inside the context
        one_pass()
        assert not wrapped.sync.enabled
    assert wrapped.sync.enabled
    one_pass()                                          # and the plain backward still exchanges
    torch.save(log, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_no_sync_and_non_closing_micro_steps_create_no_sync_call():
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_sync_switch_rank, args=(2, _free_port(), d), nprocs=2, join=True)
        logs = [torch.load(os.path.join(d, f"rank{r}.pt")) for r in range(2)]
    for log in logs:
        for i in (0, 1, 3):                             # non-closing micro-steps, no_sync
            assert log[i]["created"] == 0 and log[i]["launched"] == [] and not log[i]["changed"], i
        for i in (2, 4):                                # the closing micro-step, the plain backward
            assert log[i]["created"] == 1 and len(log[i]["launched"]) >= 3 and log[i]["changed"], i
        assert log[2]["folded"] == log[2]["launched"]   # every bucket is folded once, before it leaves, in order
        assert log[4]["folded"] is None
    assert logs[0][2]["launched"] == logs[1][2]["launched"] == logs[0][4]["launched"]
