#!/usr/bin/env python3
"""HIP-event timing of the weight EMA inside the fused AdamW step at the headline shape (UNet, 8 x 3 x 360 x 480, fp32; 34.5 M parameter
floats = 138.1 MB per flat buffer, gradients of one real backward pass):
  (a) the eager FlatAdamW.step() without an EMA (seven passes over the buffer: read p, g, m, v; write p, m, v);
  (b) the same step with ema_decay (nine passes: read and write ema as well, no further launch);
  (c) step (a) followed by one torch lerp_ over the two flat buffers (ten passes and one more launch): the best a user can do by hand;
  (d) the captured iteration (GraphedStep(optimizer=, scheduler=, log_capacity=)) without and with the EMA, wall time per replay.
Legs alternate --reps times in one process; medians and min / max; one JSON line at the end, also written to --out.
                                            usage (GPU box): python tools/bench_ema.py [--iters 50] [--reps 5] [--graph-iters 20]"""
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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5, help="interleaved repetitions; the median is reported")
    ap.add_argument("--graph-iters", type=int, default=20, help="replays per timed epoch of the captured iteration")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, H, W = a.batch, 360, 480
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, 3, H, W, generator=g).to(dev)
    t = torch.randint(0, 12, (N, H, W), generator=g).to(dev)
    lossf = A.CrossEntropyLoss()

    def setup(ema_decay=None, total_steps=None):
        torch.manual_seed(0)
        net = A.UNet(3, 12).to(dev).train()
        opt = A.FlatAdamW(net, lr=5e-4, weight_decay=1e-2, ema_decay=ema_decay, ema_warmup=ema_decay is not None)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=5e-4, total_steps=total_steps, cycle_momentum=True) if total_steps else None
        return net, opt, sched

    # one real backward per optimizer: the step legs all run on these gradients
    net_p, opt_p, _ = setup()
    lossf(net_p(x), t).backward()
    net_e, opt_e, _ = setup(a.decay)
    lossf(net_e(x), t).backward()
    net_h, opt_h, _ = setup()
    lossf(net_h(x), t).backward()
    by_hand = opt_h._flat.clone()
    nbytes = 4 * opt_p._flat.numel()

    def step_then_lerp():
        opt_h.step()
        by_hand.lerp_(opt_h._flat, 1.0 - a.decay)

    legs = {"step_us": opt_p.step, "step_ema_us": opt_e.step, "step_then_lerp_us": step_then_lerp}
    for fn in legs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():
            res[k].append(timed(fn, a.iters))
    out = {"shape": [N, 3, H, W], "buffer_bytes": nbytes, "iters": a.iters, "reps": a.reps, "ema_decay": a.decay}
    for k, v in res.items():
        out[k] = round(sorted(v)[len(v) // 2], 2)
        out[k + "_min_max"] = [round(min(v), 2), round(max(v), 2)]
    out["ema_cost_us"] = round(out["step_ema_us"] - out["step_us"], 2)
    out["ema_cost_bound_us"] = round(out["step_us"] * 2 / 7, 2)          # two more passes on top of seven
    out["step_TBps"] = round(7 * nbytes / (out["step_us"] * 1e-6) / 1e12, 3)
    out["step_ema_TBps"] = round(9 * nbytes / (out["step_ema_us"] * 1e-6) / 1e12, 3)
    del net_p, opt_p, net_e, opt_e, net_h, opt_h, by_hand

    # (d) the captured iteration, without and with the EMA: wall time per replay, epochs alternate
    total = a.graph_iters * (a.reps + 2) + 8
    steps = {}
    for name, decay in (("graphed_ms", None), ("graphed_ema_ms", a.decay)):
        net, opt, sched = setup(decay, total)
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
    print(f"UNet {N}x3x{H}x{W}: {nbytes / 1e6:.1f} MB per flat buffer, decay {a.decay}; medians of {a.reps} x {a.iters} calls")
    print(f"(a) FlatAdamW.step()                {out['step_us']:9.1f} us   {out['step_TBps']:.2f} TB/s over 7 passes")
    print(f"(b) FlatAdamW.step() with EMA       {out['step_ema_us']:9.1f} us   {out['step_ema_TBps']:.2f} TB/s over 9 passes; "
          f"(b) - (a) = {out['ema_cost_us']:.1f} us, 2/7 of (a) = {out['ema_cost_bound_us']:.1f} us")
    print(f"(c) step() + lerp_ by hand          {out['step_then_lerp_us']:9.1f} us")
    print(f"(d) captured iteration              {out['graphed_ms']:9.3f} ms   with EMA {out['graphed_ema_ms']:9.3f} ms")
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
