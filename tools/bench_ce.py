#!/usr/bin/env python3
"""HIP-event timing of the loss at the headline shape (8 x 12 x 360 x 480, logits from a real UNet so the pixel stride ld is the
network's): the default CrossEntropyLoss (k_ce_fwd -> k_ce_finish -> k_ce_bwd) against the weighted + label-smoothed one
(k_ce_fwd_ex -> k_ce_finish_ex -> k_ce_bwd_ex), forward and backward through the raw entry points, interleaved; plus one
cvk_class_histogram launch over the batch's masks (uint8 and int64).  Prints us per call and the weighted / default ratio.
                                            usage (GPU box): python tools/bench_ce.py [--iters 200] [--reps 5]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_camvid_amd as A  # noqa: E402
from pytorch_camvid_amd import _lib  # noqa: E402
from pytorch_camvid_amd.functional import _as_nhwc  # noqa: E402


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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5, help="interleaved repetitions; the median is reported")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, C, H, W = 8, 12, 360, 480
    torch.manual_seed(0)
    net = A.UNet(3, C).to(dev).train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, 3, H, W, generator=g).to(dev)
    t = torch.randint(0, C, (N, H, W), generator=g).to(dev)
    with torch.no_grad():
        logits = net(x).detach()
    ld = _as_nhwc(logits)[1]
    del net
    w = A.class_weights([t], C)
    # the raw entry points, so the host's autograd bookkeeping stays out of the numbers (a call enqueues in a few us)
    lib, check = _lib.load(), _lib.check
    s = torch.cuda.current_stream().cuda_stream
    lg, tg = _as_nhwc(logits)[0], t
    M = N * H * W
    part = torch.empty(lib.cvk_ce_ex_part_floats(M), device=dev)
    loss = torch.empty(4, device=dev)
    d = torch.empty(M * C, device=dev)
    args = (lg.data_ptr(), ld, tg.data_ptr())
    calls = {
        "default": (lambda: check(lib.cvk_softmax_ce_fwd(*args, part.data_ptr(), loss.data_ptr(), M, C, -100, s), "fwd"),
                    lambda: check(lib.cvk_softmax_ce_bwd(*args, loss.data_ptr(), None, 1.0, d.data_ptr(), C, M, C, -100, s), "bwd")),
        "weighted + smoothed": (
            lambda: check(lib.cvk_softmax_ce_fwd_ex(*args, w.data_ptr(), 0.1, 1, part.data_ptr(), loss.data_ptr(), None, M, C, -100, s), "fwd"),
            lambda: check(lib.cvk_softmax_ce_bwd_ex(*args, w.data_ptr(), 0.1, 1, loss.data_ptr(), None, 1.0, d.data_ptr(), C, M, C, -100, s),
                          "bwd")),
    }
    for f, b in calls.values():
        for _ in range(10):
            f(); b()
    torch.cuda.synchronize()
    res = {}
    for _ in range(a.reps):
        for k, (f, b) in calls.items():
            res.setdefault(("fwd", k), []).append(timed(f, a.iters))
            res.setdefault(("bwd", k), []).append(timed(b, a.iters))
    med = {key: sorted(v)[len(v) // 2] for key, v in res.items()}
    print(f"logits {N}x{C}x{H}x{W}, ld {ld}; median of {a.reps} x {a.iters} calls")
    tot = {}
    for k in calls:
        tot[k] = med[("fwd", k)] + med[("bwd", k)]
        print(f"{k:20s} fwd (+ finish) {med[('fwd', k)]:7.1f} us   bwd {med[('bwd', k)]:7.1f} us   total {tot[k]:7.1f} us")
    print(f"ratio weighted + smoothed / default: {tot['weighted + smoothed'] / tot['default']:.3f}")
    meter = A.ClassFrequencyMeter(C, device=dev)
    for name, m in (("uint8", t.to(torch.uint8)), ("int64", t)):
        meter.update(m)
        us = timed(lambda: meter.update(m), a.iters)
        print(f"class histogram ({name} masks, {N}x{H}x{W}): {us:.1f} us per batch")


if __name__ == "__main__":
    main()
