"""One process with a world-size-1 RCCL group (tests/test_gpu_graphed_iteration.py): the whole data-parallel training iteration captured
as one graph — forward, CE, backward with its bucketed all-reduces, FlatAdamW, OneCycleLR — against the eager ddp.DataParallel loop."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (2, 48, 64)
ITERS = 4


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    n, h, w = SHAPE
    return torch.randn(n, 3, h, w, generator=g), torch.randint(0, 12, (n, h, w), generator=g)


def run(rank, port, out_path):
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd import ddp
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ddp.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    torch.manual_seed(5)
    net = A.UNet(3, 12).to(dev).train()
    ref = A.UNet(3, 12).to(dev).train()
    ref.load_state_dict(net.state_dict())
    st0 = {k: v.clone() for k, v in net.state_dict().items()}
    lossf = A.CrossEntropyLoss()

    def parts(lr):
        return dict(lr=lr, weight_decay=1e-2)

    # the eager data-parallel loop first (train.py:124-134), its states kept on the host
    ref_dp = ddp.DataParallel(ref, always_issue=True, bucket_mb=8.0)
    opt_r = A.FlatAdamW(ref, **parts(2e-3))
    sched_r = torch.optim.lr_scheduler.OneCycleLR(opt_r, max_lr=2e-3, total_steps=ITERS + 2, cycle_momentum=True)
    eager = []
    for it in range(ITERS):
        x, t = (v.to(dev) for v in _batch(40 + it))
        opt_r.zero_grad()
        loss = lossf(ref_dp(x), t)
        loss.backward()
        opt_r.step()
        sched_r.step()
        torch.cuda.synchronize()
        eager.append({"loss": loss.detach().cpu().clone(), "params": [p.detach().cpu().clone() for p in ref.parameters()],
                      "m": opt_r._m.cpu(), "v": opt_r._v.cpu(), "bn": [b.detach().cpu().clone() for b in ref.buffers()]})

    # the same iterations as ONE captured graph each, all-reduces included
    wrapped = ddp.DataParallel(net, always_issue=True, bucket_mb=8.0)
    opt = A.FlatAdamW(net, **parts(2e-3))
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=2e-3, total_steps=ITERS + 2, cycle_momentum=True)
    x0, t0 = (v.to(dev) for v in _batch(39))
    gs = A.GraphedStep(net, lossf, x0, t0, allow_grad_sync=True, optimizer=opt, scheduler=sched)
    net.load_state_dict(st0)                              # the capture's warm-up passes advanced the BatchNorm statistics
    res = {"buckets": len(wrapped.sync.launched), "iters": []}
    for it in range(ITERS):
        x, t = (v.to(dev) for v in _batch(40 + it))
        la = gs.replay(x, t)
        torch.cuda.synchronize()
        e = eager[it]
        res["iters"].append({
            "loss": bool(torch.equal(la.detach().cpu(), e["loss"])),
            "params": all(torch.equal(p.detach().cpu(), q) for p, q in zip(net.parameters(), e["params"])),
            "moments": bool(torch.equal(opt._m.cpu(), e["m"]) and torch.equal(opt._v.cpu(), e["v"])),
            "bn": all(torch.equal(b.detach().cpu(), c) for b, c in zip(net.buffers(), e["bn"]))})
    res["step"] = [opt._step, opt_r._step]
    with open(out_path, "w") as f:
        json.dump(res, f)
    torch.distributed.destroy_process_group()
