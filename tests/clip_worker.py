"""Child processes of tests/test_gpu_clip.py (each started once, with its own time limit, never retried):

    python tests/clip_worker.py repro OUT            the captured clipped iteration in a fresh process: bytes of parameters, moments and log
    python tests/clip_worker.py single OUT           the reference of the data-parallel run: eager + captured clipped loops, no process group
    python tests/clip_worker.py ddp OUT RANK WORLD PORT   the same loops under ddp.DataParallel on an RCCL group of WORLD ranks
"""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (2, 48, 64)
ITERS = 4
LR = 2e-3
MAX_NORM = 0.5


def batch(seed, dev):
    g = torch.Generator().manual_seed(seed)
    n, h, w = SHAPE
    return torch.randn(n, 3, h, w, generator=g).to(dev), torch.randint(0, 12, (n, h, w), generator=g).to(dev)


def groups(net):
    named = list(net.named_parameters())
    return [{"params": [p for _, p in named if p.dim() == 1], "weight_decay": 0.0, "lr": LR},
            {"params": [p for _, p in named if p.dim() != 1], "weight_decay": 5e-2, "lr": LR / 2}]


def make(A, dev, seed=5):
    torch.manual_seed(seed)
    return A.UNet(3, 12).to(dev).train()


def optimizer(A, net):
    opt = A.FlatAdamW(net, groups=groups(net), max_grad_norm=MAX_NORM)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=[LR, LR / 2], total_steps=ITERS + 4, cycle_momentum=True)
    return opt, sched


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def eager_loop(A, net, fwd, dev, seed0):
    """ITERS iterations of zero_grad; forward; CE; backward; clipped step; scheduler.  Returns per-iteration digests and norm records."""
    opt, sched = optimizer(A, net)
    lossf = A.CrossEntropyLoss()
    out = []
    for it in range(ITERS):
        x, t = batch(seed0 + it, dev)
        opt.zero_grad()
        loss = lossf(fwd(x), t)
        loss.backward()
        opt.step()
        sched.step()
        torch.cuda.synchronize()
        out.append({"loss": digest(loss), "state": digest(opt._flat, opt._m, opt._v, *net.buffers()), "rec": digest(opt._clip_rec),
                    "norm": float(opt.grad_norm), "coef": float(opt.clip_coef)})
    return out


def captured_loop(A, net, dev, seed0, allow_grad_sync):
    opt, sched = optimizer(A, net)
    st0 = {k: v.clone() for k, v in net.state_dict().items()}
    lossf = A.CrossEntropyLoss()
    gs = A.GraphedStep(net, lossf, *batch(seed0 - 1, dev), allow_grad_sync=allow_grad_sync, optimizer=opt, scheduler=sched, log_capacity=ITERS)
    net.load_state_dict(st0)                              # the capture's warm-up passes advanced the BatchNorm statistics
    out = []
    for it in range(ITERS):
        loss = gs.replay(*batch(seed0 + it, dev))
        torch.cuda.synchronize()
        out.append({"loss": digest(loss), "state": digest(opt._flat, opt._m, opt._v, *net.buffers()), "rec": digest(opt._clip_rec),
                    "norm": float(opt.grad_norm), "coef": float(opt.clip_coef)})
    rows, dropped = gs.log()
    return out, hashlib.sha256(rows.tobytes()).hexdigest(), list(rows.shape), dropped


def main():
    mode, out_path = sys.argv[1], sys.argv[2]
    import pytorch_camvid_amd as A
    dev = torch.device("cuda:0")
    res = {}
    if mode == "repro":
        its, log, shape, dropped = captured_loop(A, make(A, dev), dev, 300, False)
        res = {"iters": its, "log": log, "log_shape": shape, "dropped": dropped}
    elif mode == "single":
        net = make(A, dev)
        res["eager"] = eager_loop(A, net, net, dev, 40)
        its, log, shape, _ = captured_loop(A, make(A, dev), dev, 40, False)
        res["captured"], res["log"], res["log_shape"] = its, log, shape
    elif mode == "ddp":
        from pytorch_camvid_amd import ddp
        rank, world, port = int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", port
        dev = torch.device("cuda", rank if torch.cuda.device_count() >= world else 0)
        torch.cuda.set_device(dev)
        ddp.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        seed0 = 40 + 1000 * rank                          # every rank its own shard; rank 0's is the single-process batch
        net = make(A, dev)
        wrapped = ddp.DataParallel(net, always_issue=True, bucket_mb=8.0)
        res["eager"] = eager_loop(A, net, wrapped, dev, seed0)
        res["buckets"] = len(wrapped.sync.launched)
        net2 = make(A, dev)
        ddp.DataParallel(net2, always_issue=True, bucket_mb=8.0)
        its, log, shape, _ = captured_loop(A, net2, dev, seed0, True)
        res["captured"], res["log"], res["log_shape"] = its, log, shape
        torch.cuda.synchronize()
        torch.distributed.destroy_process_group()
    else:
        raise SystemExit(f"unknown mode {mode}")
    with open(out_path, "w") as f:
        json.dump(res, f)
    sys.stdout.flush()
    os._exit(0)           # as tests/conftest.py: skip the teardown of HIP / RCCL globals, which can crash after the work is done


if __name__ == "__main__":
    main()
