#!/usr/bin/env python3
"""HIP-event timing of the fused momentum-SGD step at the headline shape (UNet, 8 x 3 x 360 x 480, fp32; 34.5 M parameter floats = 138.1 MB
per flat buffer, gradients of one real backward pass):
  (a) the eager FlatAdamW.step() (seven passes over the buffer: read p, g, m, v; write p, m, v): the yardstick of this run;
  (b) the eager FlatSGD.step() with momentum 0.9 (five passes: read p, g, buf; write p, buf), plain and with Nesterov;
  (c) the eager FlatSGD.step() with momentum 0 (three passes: read p, g; write p; no buffer exists);
  (d) torch.optim.SGD with the options of (b) and (c) on the same network (multi-tensor launches over 92 tensors);
  (e) the captured iteration (GraphedStep(optimizer=, scheduler=, log_capacity=)) with FlatAdamW and with FlatSGD, wall time per replay.
By traffic (b) should take at most 5/7 and (c) at most 3/7 of (a), plus the run's own min - max spread; the JSON carries both ratios.
Every step leg also reports the host time per call spent enqueueing: a leg whose device time equals it is limited by Python, not the kernel.
Legs alternate --reps times in one process; medians and min / max; one JSON line at the end, also written to --out.
                                            usage (GPU box): python tools/bench_sgd.py [--iters 50] [--reps 5] [--graph-iters 20]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytorch_camvid_amd as A  # noqa: E402


def timed(fn, iters):
    """(device us per call between two events, host us per call spent enqueueing).  Where the two are equal the host is the limit: the
    device waited for Python, and the figure says nothing about the kernel."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3, host / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5, help="interleaved repetitions; the median is reported")
    ap.add_argument("--graph-iters", type=int, default=20, help="replays per timed epoch of the captured iteration")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgd_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, H, W = a.batch, 360, 480
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, 3, H, W, generator=g).to(dev)
    t = torch.randint(0, 12, (N, H, W), generator=g).to(dev)
    lossf = A.CrossEntropyLoss()
    lr, wd = 1e-3, 1e-4                     # small enough that hundreds of steps on one gradient stay finite

    def net_with_grads():
        torch.manual_seed(0)
        net = A.UNet(3, 12).to(dev).train()
        return net

    # one real backward per optimizer: every step leg runs on these gradients
    legs, keep = {}, []

    def flat_leg(name, make):
        net = net_with_grads()
        opt = make(net)
        lossf(net(x), t).backward()
        keep.append((net, opt))
        legs[name] = opt.step
        return opt

    def torch_leg(name, **kw):
        net = net_with_grads()
        lossf(net(x), t).backward()
        opt = torch.optim.SGD(net.parameters(), lr=lr, weight_decay=wd, **kw)
        keep.append((net, opt))
        legs[name] = opt.step

    opt_a = flat_leg("adamw_step_us", lambda net: A.FlatAdamW(net, lr=5e-4, weight_decay=1e-2))
    flat_leg("sgd_momentum_us", lambda net: A.FlatSGD(net, lr=lr, momentum=0.9, weight_decay=wd))
    flat_leg("sgd_nesterov_us", lambda net: A.FlatSGD(net, lr=lr, momentum=0.9, weight_decay=wd, nesterov=True))
    opt_0 = flat_leg("sgd_plain_us", lambda net: A.FlatSGD(net, lr=lr, momentum=0.0, weight_decay=wd))
    torch_leg("torch_sgd_momentum_us", momentum=0.9)
    torch_leg("torch_sgd_nesterov_us", momentum=0.9, nesterov=True)
    torch_leg("torch_sgd_plain_us")
    nbytes = 4 * opt_a._flat.numel()
    for fn in legs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    assert opt_0._buf is None               # the momentum-free legs never allocated a buffer
    res, host = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():
            d, h = timed(fn, a.iters)
            res[k].append(d)
            host[k].append(h)
    out = {"shape": [N, 3, H, W], "buffer_bytes": nbytes, "iters": a.iters, "reps": a.reps}
    for k, v in res.items():
        out[k] = round(sorted(v)[len(v) // 2], 2)
        out[k + "_min_max"] = [round(min(v), 2), round(max(v), 2)]
        out[k.replace("_us", "_host_us")] = round(sorted(host[k])[len(v) // 2], 2)
    out["sgd_momentum_over_adamw"] = round(out["sgd_momentum_us"] / out["adamw_step_us"], 3)        # expectation: <= 5/7 = 0.714
    out["sgd_plain_over_adamw"] = round(out["sgd_plain_us"] / out["adamw_step_us"], 3)              # expectation: <= 3/7 = 0.429
    out["adamw_TBps"] = round(7 * nbytes / (out["adamw_step_us"] * 1e-6) / 1e12, 3)
    out["sgd_momentum_TBps"] = round(5 * nbytes / (out["sgd_momentum_us"] * 1e-6) / 1e12, 3)
    out["sgd_plain_TBps"] = round(3 * nbytes / (out["sgd_plain_us"] * 1e-6) / 1e12, 3)
    del legs, opt_a, opt_0
    keep.clear()

    # (e) the captured iteration with each optimizer: wall time per replay, epochs alternate
    total = a.graph_iters * (a.reps + 2) + 8
    steps = {}
    for name, make in (("graphed_adamw_ms", lambda net: A.FlatAdamW(net, lr=5e-4, weight_decay=1e-2)),
                       ("graphed_sgd_ms", lambda net: A.FlatSGD(net, lr=lr, momentum=0.9, weight_decay=wd))):
        net = net_with_grads()
        opt = make(net)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=opt.param_groups[0]["lr"], total_steps=total, cycle_momentum=True)
        steps[name] = A.GraphedStep(net, lossf, x, t, optimizer=opt, scheduler=sched, log_capacity=a.graph_iters)

    def epoch(gs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.graph_iters):
            gs.replay()
        rows, _ = gs.log()
        assert rows.shape[0] == a.graph_iters
        return (time.perf_counter() - t0) / a.graph_iters * 1e3

    for gs in steps.values():
        epoch(gs)
    wall = {k: [] for k in steps}
    for _ in range(a.reps):
        for k, gs in steps.items():
            wall[k].append(epoch(gs))
    for k, v in wall.items():
        out[k] = round(sorted(v)[len(v) // 2], 3)
        out[k + "_min_max"] = [round(min(v), 3), round(max(v), 3)]
    print(f"UNet {N}x3x{H}x{W}: {nbytes / 1e6:.1f} MB per flat buffer; medians of {a.reps} x {a.iters} calls")
    print(f"(a) FlatAdamW.step()                     {out['adamw_step_us']:9.1f} us   {out['adamw_TBps']:.2f} TB/s over 7 passes")
    print(f"(b) FlatSGD.step(), momentum 0.9         {out['sgd_momentum_us']:9.1f} us   {out['sgd_momentum_TBps']:.2f} TB/s over 5 passes; "
          f"(b) / (a) = {out['sgd_momentum_over_adamw']:.3f} (5/7 = 0.714); Nesterov {out['sgd_nesterov_us']:.1f} us")
    print(f"(c) FlatSGD.step(), momentum 0           {out['sgd_plain_us']:9.1f} us   {out['sgd_plain_TBps']:.2f} TB/s over 3 passes; "
          f"(c) / (a) = {out['sgd_plain_over_adamw']:.3f} (3/7 = 0.429)")
    print("    host enqueue per call: " + ", ".join(f"{k[:-3]} {out[k.replace('_us', '_host_us')]:.0f} us" for k in res))
    print(f"(d) torch.optim.SGD                      {out['torch_sgd_momentum_us']:9.1f} us   Nesterov {out['torch_sgd_nesterov_us']:.1f} us   "
          f"momentum 0 {out['torch_sgd_plain_us']:.1f} us")
    print(f"(e) captured iteration                   FlatAdamW {out['graphed_adamw_ms']:.3f} ms   FlatSGD {out['graphed_sgd_ms']:.3f} ms")
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
