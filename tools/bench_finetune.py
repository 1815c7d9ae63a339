#!/usr/bin/env python3
"""Training-step time of three fine-tuning patterns at the headline shape (UNet, 8 x 3 x 360 x 480, FlatAdamW), eager and captured
(GraphedStep with the optimizer), in fp32 and in bf16 mode:
  all   every parameter trains (the bench.py workload plus the optimizer step)
  enc   down1 ... down5 frozen and their BatchNorm layers in eval mode (the decoder and the head train)
  head  only the classifier head (`output`) trains
eager = zero_grad -> net(x) -> CE -> backward -> opt.step(), one synchronisation per leg; graphed = GraphedStep.replay() per step.
The legs of one precision alternate --reps times (all, enc, head, all, ...); medians are reported, and one JSON line at the end.
                                            usage (GPU box): python tools/bench_finetune.py [--steps 10] [--reps 3] [--precision fp32 bf16]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_camvid_amd as A  # noqa: E402

ENCODER = ("down1", "down2", "down3", "down4", "down5")


def make(pattern, precision, dev):
    torch.manual_seed(0)
    net = A.set_conv_precision(A.UNet(3, 12).to(dev).train(), precision)
    if pattern == "enc":
        for s in ENCODER:
            getattr(net, s).requires_grad_(False)
            getattr(net, s).eval()
    elif pattern == "head":
        for n, m in net.named_children():
            if n != "output":
                m.requires_grad_(False)
    return net, A.FlatAdamW(net, lr=1e-4, weight_decay=1e-2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="timed steps per leg")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", nargs="+", default=["fp32", "bf16"], choices=["fp32", "bf16"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, H, W = a.batch, 360, 480
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, 3, H, W, generator=g).to(dev)
    t = torch.randint(0, 12, (N, H, W), generator=g).to(dev)
    lossf = A.CrossEntropyLoss()
    out = {"shape": [N, 3, H, W], "steps": a.steps, "reps": a.reps}
    for prec in a.precision:
        legs = {}
        for pat in ("all", "enc", "head"):
            net_e, opt_e = make(pat, prec, dev)
            net_g, opt_g = make(pat, prec, dev)
            gs = A.GraphedStep(net_g, lossf, x, t, optimizer=opt_g)

            def eager(net=net_e, opt=opt_e):
                opt.zero_grad()
                lossf(net(x), t).backward()
                opt.step()
            for _ in range(3):
                eager()
                gs.replay()
            legs[pat] = {"eager": eager, "graphed": gs.replay, "ms": {"eager": [], "graphed": []}, "keep": (net_e, net_g, gs)}
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for pat, leg in legs.items():
                for kind in ("eager", "graphed"):
                    fn = leg[kind]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        fn()
                    torch.cuda.synchronize()
                    leg["ms"][kind].append((time.perf_counter() - t0) / a.steps * 1e3)
        res = {}
        for pat, leg in legs.items():
            res[pat] = {k: round(statistics.median(v), 3) for k, v in leg["ms"].items()}
            res[pat]["samples"] = {k: [round(s, 3) for s in v] for k, v in leg["ms"].items()}
            print(f"{prec:5s} {pat:5s} eager {res[pat]['eager']:8.3f} ms  graphed {res[pat]['graphed']:8.3f} ms", flush=True)
        for pat in ("enc", "head"):
            res[pat]["graphed_vs_all"] = round(res[pat]["graphed"] / res["all"]["graphed"], 3)
            res[pat]["eager_vs_all"] = round(res[pat]["eager"] / res["all"]["eager"], 3)
        out[prec] = res
        legs.clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
