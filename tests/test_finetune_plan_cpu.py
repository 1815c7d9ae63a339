"""Fine-tuning on the host side (no GPU): the per-block flags a plan records (BatchNorm mode, which parameters need a gradient, whether
anything upstream needs the input's gradient), the backward work they prune from the routes, the plan-cache key, and gradient buckets
that leave frozen ranges out (gloo, world 2)."""
import os
import socket
import tempfile

import torch
import torch.multiprocessing as mp

import pytorch_camvid_amd as A
from pytorch_camvid_amd import engine
from pytorch_camvid_amd.modules import plan_key_blocks, runner_of

ENCODER = ("down1", "down2", "down3", "down4", "down5")


def _plan(net, N=8, H=360, W=480):
    plan = engine.Plan(N, 3, H, W)
    plan.output = net._emit(plan, plan.input)
    plan.seal()
    names = {id(m): n for n, m in net.named_modules()}
    for op in plan.convs:
        op.name = names[id(op.holder)]
    return plan


def _freeze(net, stages, bn_eval=True):
    for s in stages:
        m = getattr(net, s)
        m.requires_grad_(False)
        if bn_eval:
            m.eval()


def _work(R, plan):
    """{block name: (weight-grad, data-grad, BatchNorm backward)} of a training pass with a backward."""
    routes = R.routes(plan, True, True)
    out = {}
    for op in plan.convs:
        rt = routes[op.idx]
        out[op.name] = (rt.wgrad is not None, rt.dgrad is not None, op.active)
    return out


def test_unet_frozen_encoder_prunes_the_encoder_backward():
    net = A.UNet(3, 12).train()
    _freeze(net, ENCODER)
    plan = _plan(net)
    work = _work(runner_of(net), plan)
    for op in plan.convs:
        enc = op.name.split(".")[0] in ENCODER
        assert op.bn_train == (not enc) and op.trainable == (not enc), op.name
        if enc:     # no weight-grad, no data-grad, no BatchNorm backward, no V planes kept by the forward pass
            assert work[op.name] == (False, False, False) and not runner_of(net).routes(plan, True, True)[op.idx].keeps_v, op.name
    # upsample1.conv reads the upsampled bottleneck (frozen): it trains but needs no data-grad
    assert work["upsample1.conv"] == (True, False, True)
    # up_k.0 read the concat buffers: the trainable upsample half needs their data-grad (the skip half is computed and discarded)
    for k in range(1, 5):
        assert work[f"up{k}.0"] == (True, True, True) and work[f"up{k}.1"] == (True, True, True)
        assert work[f"upsample{k}.conv"][0]
    assert work["output"] == (True, True, True)
    # the concat skip sides are pruned: the max pools behind the skip tensors and the bottleneck's upsampling run no backward
    pools = [o for o in plan.ops if isinstance(o, engine.MaxPool)]
    ups = [o for o in plan.ops if isinstance(o, engine.Upsample)]
    assert len(pools) == 4 and not any(p.wants for p in pools)
    assert [u.wants for u in ups] == [False, True, True, True]


def test_unet_head_only():
    net = A.UNet(3, 12).train()
    for n, m in net.named_children():
        if n != "output":
            m.requires_grad_(False)
    plan = _plan(net)
    work = _work(runner_of(net), plan)
    assert work.pop("output") == (True, False, True)          # the head's own gradients only: nothing upstream needs its input's gradient
    assert all(v == (False, False, False) for v in work.values()), work
    assert not any(getattr(o, "wants", False) for o in plan.ops if not isinstance(o, engine.ConvBnRelu))


def test_unet_batchnorm_eval_only():
    """Every parameter trains, the encoder's BatchNorm layers use (and keep) their running statistics: the whole backward runs."""
    net = A.UNet(3, 12).train()
    for s in ENCODER:
        getattr(net, s).eval()
    plan = _plan(net)
    work = _work(runner_of(net), plan)
    assert all(v == (True, op.name != "down1.0", True) for op, v in zip(plan.convs, work.values()))
    assert [op.bn_train for op in plan.convs] == [op.name.split(".")[0] not in ENCODER for op in plan.convs]
    assert all(o.wants for o in plan.ops if isinstance(o, (engine.MaxPool, engine.Upsample)))


def test_segnet_frozen_encoder():
    net = A.SegNet(3, 12).train()
    _freeze(net, [f"encoder{k}" for k in range(1, 6)])
    plan = _plan(net, 2, 64, 96)
    work = _work(runner_of(net), plan)
    for op in plan.convs:
        if op.name.startswith("encoder"):
            assert work[op.name] == (False, False, False), op.name
    assert work["decoder5.0"] == (True, False, True)          # reads the unpooled bottleneck: no data-grad
    assert all(work[op.name] == (True, True, True) for op in plan.convs if op.name.startswith("decoder") and op.name != "decoder5.0")
    assert not any(o.wants for o in plan.ops if isinstance(o, engine.MaxPool))
    unpools = [o for o in plan.ops if isinstance(o, engine.Unpool)]
    assert [u.wants for u in unpools] == [False, True, True, True, True]


def test_frozen_stem_and_input_gradient():
    """A frozen stem still runs its data-grad when the network input requires a gradient (saliency maps), and none when it does not."""
    net = A.UNet(3, 12).train()
    net.down1[0].requires_grad_(False)
    plan = _plan(net, 1, 32, 32)
    assert not plan.convs[0].active
    plan = engine.Plan(1, 3, 32, 32)
    plan.input_needs_grad = True
    plan.output = net._emit(plan, plan.input)
    plan.seal()
    assert plan.convs[0].active and plan.convs[0].src_needs_grad and not plan.convs[0].trainable
    assert runner_of(net).routes(plan, True, True)[plan.convs[0].idx].wgrad is None


def test_routes_match_the_default_when_everything_trains():
    """Flags that prune nothing leave every route as it was."""
    a, b = A.UNet(3, 12).train(), A.UNet(3, 12).train()
    b.down1.requires_grad_(False)
    b.down1.requires_grad_(True)
    ra = runner_of(a).routes(_plan(a), True, True)
    rb = runner_of(b).routes(_plan(b), True, True)
    assert list(ra.values()) == list(rb.values())


def test_plan_key_changes_with_requires_grad_eval_and_head_swap():
    net = A.UNet(3, 12).train()
    k0 = plan_key_blocks(net)
    net.down2.requires_grad_(False)
    k1 = plan_key_blocks(net)
    assert k1 != k0
    net.down2[1].conv[1].bias.requires_grad_(True)            # one BatchNorm bias: still a new key
    assert plan_key_blocks(net) not in (k0, k1)
    net.down2.requires_grad_(True)
    assert plan_key_blocks(net) == k0
    net.down3.eval()
    assert plan_key_blocks(net) != k0
    net.train()
    assert plan_key_blocks(net) == k0
    net.output = A.BasicConv2d(64, 21)
    assert plan_key_blocks(net) != k0


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _gradsync_rank(rank, world, port, out_dir):
    import torch.distributed as dist
    from pytorch_camvid_amd import ddp
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    net = A.UNet(3, 12).train()
    _freeze(net, ("down2", "down4"))
    net.up2[0].conv[1].requires_grad_(False)                  # a frozen BatchNorm inside a trainable block
    plan = _plan(net, 1, 32, 32)
    params = [t for h in plan.holders for t in h.block_params()]

    class St:
        pass
    st = St()
    st.params = params
    st.goffs, total = engine.layout_grads(params)
    g = torch.Generator().manual_seed(100 + rank)
    st.gflat = torch.randn(total, generator=g)
    before = st.gflat.clone()
    sync = ddp.GradSync(bucket_mb=0.25)
    call = sync.begin(st, plan)
    for slot in range(len(plan.convs) - 1, -1, -1):             # every slot reported (the executor reports trainable ones only): frozen ones are ignored
        call.layer_done(st, slot)
    call.finish(st)
    torch.save({"before": before, "after": st.gflat, "launched": sync.launched, "offs": st.goffs,
                "req": [p.requires_grad for p in params], "sizes": [p.numel() for p in params]}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_gradsync_buckets_leave_out_frozen_ranges():
    world = 2
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_gradsync_rank, args=(world, _free_port(), d), nprocs=world, join=True)
        rs = [torch.load(os.path.join(d, f"rank{r}.pt")) for r in range(world)]
    r0 = rs[0]
    frozen = [(o, o + n) for o, n, q in zip(r0["offs"], r0["sizes"], r0["req"]) if not q]
    assert len(frozen) == 4 * 4 + 2
    for lo, hi in r0["launched"]:
        assert all(hi <= a or b <= lo for a, b in frozen), (lo, hi)
    mean = (rs[0]["before"] + rs[1]["before"]) / 2
    for r in rs:
        for o, n, q in zip(r["offs"], r["sizes"], r["req"]):
            if q:       # every trainable segment is exchanged ...
                assert torch.allclose(r["after"][o:o + n], mean[o:o + n], rtol=1e-6, atol=1e-7)
            else:       # ... and no frozen one is touched
                assert torch.equal(r["after"][o:o + n], r["before"][o:o + n])
    assert r0["launched"] == rs[1]["launched"] and len(r0["launched"]) >= 3
