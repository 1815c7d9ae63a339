"""fp32 weight-grads on the library's side stream (CVK_WGRAD_SIDE=1; Runner.wgrad_side): parameter gradients and BatchNorm buffers are bitwise those
of the single-stream order; stream capture and an attached gradient synchroniser keep the single-stream order.

What can and cannot show a missing lifetime reference: a block that backward frees in the MIDDLE of the pass while the side stream still reads it is
re-used by the pass's own later allocations, and the bitwise comparison is what catches that.  The `poison` cases re-allocate and fill with NaN
everything the pass has released once backward has returned; those fills are queued behind the pass's last join, so they check only that nothing
queued after backward can reach the side stream's operands — not more."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _forks():
    from pytorch_camvid_amd import _lib
    return _lib.load().cvk_side_launches()


def _chain():
    """conv-BN-ReLU x 3 planned and executed as ONE module (one Runner, one backward pass over three blocks): the weight-grad of block c runs beside
    the passes of block b and is joined by b's data-grad, b's beside a's; at 2 x 64 x 128 the middle block (64 -> 64) takes the plane-GEMM route"""
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd.modules import _Stage
    return _Stage(A.BasicConv2d(3, 64), A.BasicConv2d(64, 64), A.BasicConv2d(64, 12))


def _make(kind):
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    return (_chain() if kind == "chain" else A.UNet(3, 12)).to(dev()).train()


def _runners(net):
    from pytorch_camvid_amd.modules import runner_of
    return [runner_of(net)]


def _batch(seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 3, 64, 128, generator=g).to(dev()), torch.randint(0, 12, (2, 64, 128), generator=g).to(dev())


def _step(kind, side, poison=False):
    """One forward + backward; returns ({name: grad}, {name: buffer}, forks of the pass)."""
    import pytorch_camvid_amd as A
    net = _make(kind)
    for r in _runners(net):
        r.wgrad_side = side
    x, t = _batch()
    loss = A.CrossEntropyLoss()(net(x), t)
    torch.cuda.synchronize()
    f0 = _forks()
    loss.backward()
    if poison:
        # everything backward released sits in the caching allocator: take it all again on the main stream and fill it with NaN before the
        # device has caught up (these fills are ordered behind the pass's final join: see the module docstring)
        junk, reserved = [], torch.cuda.memory_reserved()
        for mb in (256, 64, 16, 4, 1):
            while torch.cuda.memory_reserved() - torch.cuda.memory_allocated() >= mb << 20:
                junk.append(torch.full((mb << 18,), float("nan"), device=dev()))
                if torch.cuda.memory_reserved() > reserved:     # a new segment, not a cached block: the cache has none of this size left
                    junk.pop()
                    reserved = torch.cuda.memory_reserved()
                    break
        assert junk
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in net.named_parameters()}
    bufs = {k: b.clone() for k, b in net.named_buffers()}
    return grads, bufs, _forks() - f0


@pytest.fixture(scope="module")
def single_stream():
    return {kind: _step(kind, False) for kind in ("chain", "unet")}


@pytest.mark.parametrize("kind", ["chain", "unet"])
@pytest.mark.parametrize("poison", [False, True])
def test_side_stream_gradients_are_bitwise_the_single_stream_ones(single_stream, kind, poison):
    g0, b0, forks0 = single_stream[kind]
    assert forks0 == 0
    g1, b1, forks1 = _step(kind, True, poison)
    assert 0 < forks1 <= sum(g.dim() == 4 for g in g1.values()), forks1      # at most one fork per conv block (the families that fork)
    for k in g0:
        assert torch.isfinite(g1[k]).all(), k
        assert torch.equal(g0[k], g1[k]), k
    for k in b0:
        assert torch.equal(b0[k], b1[k]), k


def test_the_middle_block_of_the_chain_takes_the_plane_gemm():
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd import engine
    net = _make("chain")
    x, t = _batch()
    engine.PROF = []
    try:
        A.CrossEntropyLoss()(net(x), t).backward()
        torch.cuda.synchronize()
        names = [p[0] for p in engine.PROF]
    finally:
        engine.PROF = None
    assert "k_wgradp_gemm" in names, names


def test_graphed_step_keeps_the_single_stream_order():
    import pytorch_camvid_amd as A
    g0, _, _ = _step("unet", False)
    net = _make("unet")
    for r in _runners(net):
        r.wgrad_side = True
    x, t = _batch()
    lossf = A.CrossEntropyLoss()
    per_pass = _step("unet", True)[2]
    f0 = _forks()
    gs = A.GraphedStep(net, lossf, x, t, warmup=2)
    assert _forks() - f0 == 2 * per_pass   # the two eager warm-up passes forked as an eager pass does; the captured pass did not
    net.load_state_dict(_make("unet").state_dict())
    f1 = _forks()
    gs.replay(x, t)
    torch.cuda.synchronize()
    assert _forks() == f1
    for k, p in net.named_parameters():
        assert torch.equal(p.grad, g0[k]), k


def test_attached_grad_sync_keeps_the_single_stream_order(tmp_path):
    import torch.distributed as dist
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd import ddp
    g0, _, _ = _step("unet", False)
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "store"), rank=0, world_size=1)
    try:
        net = _make("unet")
        for r in _runners(net):
            r.wgrad_side = True
        wrapped = ddp.DataParallel(net)
        x, t = _batch()
        f0 = _forks()
        A.CrossEntropyLoss()(wrapped(x), t).backward()
        torch.cuda.synchronize()
        assert _forks() == f0
        for k, p in net.named_parameters():
            assert torch.equal(p.grad, g0[k]), k
    finally:
        dist.destroy_process_group()
