#!/usr/bin/env python3
"""HIP-event timing of global-norm gradient clipping at the headline shape (UNet, 8 x 3 x 360 x 480, fp32; 34.5 M gradient floats = 138.1 MB
in the executor's flat buffer, gradients of one real backward pass):
  (a) the norm reduction + finish alone (cvk_grad_norm: two launches) and the bytes per second it reads;
  (b) the eager FlatAdamW.step() without and with max_grad_norm;
  (c) torch.nn.utils.clip_grad_norm_ on the same gradients followed by the unclipped step — what (b, clipped) replaces;
  (d) the captured iteration (GraphedStep(optimizer=, scheduler=, log_capacity=)) without and with clipping, wall time per replay.
max_norm is half the measured norm, so the fused legs really scale.  torch's leg runs on its own copies of the gradients with max_norm
1e30: the same launches (its in-place multiply by the clamped coefficient is unconditional) on values that survive repetition.
Legs alternate --reps times; medians; one JSON line at the end.
                                            usage (GPU box): python tools/bench_clip.py [--iters 50] [--reps 5] [--graph-iters 20]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, H, W = a.batch, 360, 480
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, 3, H, W, generator=g).to(dev)
    t = torch.randint(0, 12, (N, H, W), generator=g).to(dev)
    lossf = A.CrossEntropyLoss()

    def setup(max_grad_norm=None, total_steps=None):
        torch.manual_seed(0)
        net = A.UNet(3, 12).to(dev).train()
        opt = A.FlatAdamW(net, lr=5e-4, weight_decay=1e-2, max_grad_norm=max_grad_norm)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=5e-4, total_steps=total_steps, cycle_momentum=True) if total_steps else None
        return net, opt, sched

    # one real backward per optimizer: the step legs all run on these gradients
    net_p, opt_p, _ = setup()
    lossf(net_p(x), t).backward()
    norm = A.clip_grad_norm_(net_p, 1e30).item()
    max_norm = 0.5 * norm
    net_c, opt_c, _ = setup(max_norm)
    lossf(net_c(x), t).backward()
    grad = opt_c._flat_grad()
    nbytes = 4 * sum(p.numel() for p in net_c.parameters())
    plan = opt_c._norm_plan(opt_c._trainable())
    stream = torch.cuda.current_stream().cuda_stream
    # torch's clip rewrites the gradients in place: it gets its own copies
    twins = [torch.nn.Parameter(torch.empty_like(p)) for p in net_p.parameters()]
    for q, p in zip(twins, net_p.parameters()):
        q.grad = p.grad.clone(memory_format=torch.preserve_format)

    def torch_clip_then_step():
        torch.nn.utils.clip_grad_norm_(twins, 1e30)     # max_norm 1e30: the same launches (norms, coefficient, the in-place multiply of every
        opt_p.step()                                    # gradient by the clamped coefficient) on gradients that stay as they are

    legs = {
        "norm_us": lambda: plan.norm(grad.data_ptr(), 2.0, max_norm, opt_c._clip_rec, stream),
        "step_us": opt_p.step,
        "step_clipped_us": opt_c.step,
        "torch_clip_then_step_us": torch_clip_then_step,
    }
    for fn in legs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():
            res[k].append(timed(fn, a.iters))
    out = {"shape": [N, 3, H, W], "grad_bytes": nbytes, "iters": a.iters, "reps": a.reps, "total_norm": norm, "max_norm": max_norm}
    for k, v in res.items():
        out[k] = round(sorted(v)[len(v) // 2], 2)
        out[k + "_min_max"] = [round(min(v), 2), round(max(v), 2)]
    out["norm_read_TBps"] = round(nbytes / (out["norm_us"] * 1e-6) / 1e12, 3)
    del net_p, opt_p, net_c, opt_c, twins, grad, plan

    # (d) the captured iteration, without and with clipping: wall time per replay, epochs alternate
    total = a.graph_iters * (a.reps + 2) + 8
    steps = {}
    for name, mx in (("graphed_ms", None), ("graphed_clipped_ms", max_norm)):
        net, opt, sched = setup(mx, total)
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
    print(f"UNet {N}x3x{H}x{W}: {nbytes / 1e6:.1f} MB of gradients, norm {norm:.4f}; medians of {a.reps} x {a.iters} calls")
    print(f"(a) norm reduction + finish         {out['norm_us']:9.1f} us   {out['norm_read_TBps']:.2f} TB/s read")
    print(f"(b) FlatAdamW.step()                {out['step_us']:9.1f} us   with max_grad_norm {out['step_clipped_us']:9.1f} us")
    print(f"(c) torch clip_grad_norm_ + step()  {out['torch_clip_then_step_us']:9.1f} us")
    print(f"(d) captured iteration              {out['graphed_ms']:9.3f} ms   with max_grad_norm {out['graphed_clipped_ms']:9.3f} ms")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
