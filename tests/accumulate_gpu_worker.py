"""One rank of the two-rank rehearsal of data-parallel gradient accumulation on one GPU: the real executor under ddp.DataParallel with a
GradAccumulator, gradients exchanged over gloo once per window (tests/test_gpu_accumulate.py)."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(rank, world, port, out_dir, shape, K):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd import ddp
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    torch.manual_seed(100 + rank)                            # different init per rank: the broadcast makes them equal
    net = A.UNet(3, 12).to(dev).train()
    dp = ddp.DataParallel(net, bucket_mb=8.0)
    twin = A.UNet(3, 12).to(dev).train()                     # the same weights without the wrapper: the restated mean of this rank
    twin.load_state_dict(net.state_dict())
    lossf = A.CrossEntropyLoss()
    n, h, w = shape
    batches = []
    for k in range(K):
        g = torch.Generator().manual_seed(1234 + 17 * k + rank)
        batches.append((torch.randn(n, 3, h, w, generator=g).to(dev), torch.randint(0, 12, (n, h, w), generator=g).to(dev)))
    total = None
    for x, t in batches:
        for p in twin.parameters():
            p.grad = None
        lossf(twin(x), t).backward()
        gs = [p.grad.detach().clone() for p in twin.parameters()]
        total = gs if total is None else [u + v for u, v in zip(total, gs)]
    scale = torch.tensor(1.0 / K, dtype=torch.float32, device=dev)
    restated = [(u * scale).cpu() for u in total]
    acc = A.GradAccumulator(dp, steps=K)
    folds = []
    real_open = acc.open_pass
    acc.open_pass = lambda st, plan, total_: folds.append(real_open(st, plan, total_)) or folds[-1]
    launched, none_before_close = [], True
    for k, (x, t) in enumerate(batches):
        lossf(dp(x), t).backward()
        launched.append(list(dp.sync.launched))
        if k < K - 1:
            none_before_close = none_before_close and all(p.grad is None for p in net.parameters()) and not acc.ready
    torch.cuda.synchronize()
    out = {"grads": [p.grad.detach().cpu().clone() for p in net.parameters()], "restated": restated, "launched": launched,
           "folded": list(folds[-1].folded), "none_before_close": bool(none_before_close and acc.ready)}
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()
