#!/usr/bin/env python3
"""Host enqueue time and wall time per training iteration at the headline shape (UNet, batch 8 x 3 x 360 x 480, FlatAdamW, OneCycleLR
with cycle_momentum, the reference's per-iteration log on), eager against captured:
  eager:   zero_grad -> net(x) -> CE -> backward -> opt.step() -> sched.step(), then the log of train.py:135-143 + utils.visulaize_lastlayer
           (loss.item(), lr, beta1, the two last-layer gradient norms: a host sync every iteration)
  graphed: GraphedStep(optimizer=, scheduler=, log_capacity=).replay() per iteration, gs.log() once per epoch of --iters iterations
host = time spent in the loop body before any wait for the GPU; wall = elapsed time of an epoch / iterations (log read included).
Legs alternate --reps times; medians are reported, and one JSON line at the end.
                                            usage (GPU box): python tools/bench_graphed_iteration.py [--iters 20] [--reps 3]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_camvid_amd as A  # noqa: E402
from pytorch_camvid_amd.graph import last_layer_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="iterations per epoch (one log read per epoch in the graphed loop)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, H, W = a.batch, 360, 480
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, 3, H, W, generator=g).to(dev)
    t = torch.randint(0, 12, (N, H, W), generator=g).to(dev)
    total = a.iters * (2 * a.reps + 2) + 8

    def setup():
        torch.manual_seed(0)
        net = A.UNet(3, 12).to(dev).train()
        opt = A.FlatAdamW(net, lr=5e-4, weight_decay=1e-2)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=5e-4, total_steps=total, cycle_momentum=True)
        return net, opt, sched

    lossf = A.CrossEntropyLoss()
    net_e, opt_e, sched_e = setup()
    (_, lw), (_, lb) = last_layer_params(net_e)
    net_g, opt_g, sched_g = setup()
    gs = A.GraphedStep(net_g, lossf, x, t, optimizer=opt_g, scheduler=sched_g, log_capacity=a.iters)

    def eager_epoch():
        host = 0.0
        t0 = time.perf_counter()
        for _ in range(a.iters):
            h0 = time.perf_counter()
            opt_e.zero_grad()
            loss = lossf(net_e(x), t)
            loss.backward()
            opt_e.step()
            sched_e.step()
            host += time.perf_counter() - h0
            _line = (loss.item(), opt_e.param_groups[0]["lr"], opt_e.param_groups[0]["betas"][0], lw.grad.norm().item(), lb.grad.norm().item())
        return host / a.iters, (time.perf_counter() - t0) / a.iters

    def graphed_epoch():
        host = 0.0
        t0 = time.perf_counter()
        for _ in range(a.iters):
            h0 = time.perf_counter()
            gs.replay()
            host += time.perf_counter() - h0
        rows, dropped = gs.log()
        assert dropped == 0 and rows.shape[0] == a.iters
        return host / a.iters, (time.perf_counter() - t0) / a.iters

    eager_epoch(); graphed_epoch()              # warm-up: plans, allocator, derived-weight caches
    torch.cuda.synchronize()
    res = {"eager": [], "graphed": []}
    for _ in range(a.reps):
        res["eager"].append(eager_epoch())
        torch.cuda.synchronize()
        res["graphed"].append(graphed_epoch())
        torch.cuda.synchronize()
    out = {"shape": [N, 3, H, W], "iters_per_epoch": a.iters, "reps": a.reps}
    print(f"UNet {N}x3x{H}x{W}, FlatAdamW + OneCycleLR + per-iteration log; median of {a.reps} epochs of {a.iters} iterations")
    for k, v in res.items():
        host = sorted(h for h, _ in v)[len(v) // 2] * 1e3
        wall = sorted(w for _, w in v)[len(v) // 2] * 1e3
        out[f"{k}_host_ms_per_iter"] = round(host, 3)
        out[f"{k}_wall_ms_per_iter"] = round(wall, 3)
        print(f"{k:8s} host enqueue {host:8.3f} ms/iter   wall {wall:8.3f} ms/iter")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
