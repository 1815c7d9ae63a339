#!/usr/bin/env python3
"""HIP-event timing of the segmentation losses at the headline shape (8 x 12 x 360 x 480, logits from a real UNet so the pixel stride
ld is the network's), forward + backward, in one process and in interleaved rounds:
  (a) cvk.CrossEntropyLoss()
  (b) cvk.SegmentationLoss(1.0, 0.5) and cvk.SegmentationLoss(1.0, 0.5, focal_gamma=2.0)          (one fused pass each way)
  (c) cvk.CrossEntropyLoss()(y, t) + 0.5 * dice composed from torch ops on softmax(y)
Two views: the raw entry points of (a) and (b), forward and backward apart, with the bytes each launch must move (forward: the
logits and the targets read once; backward: the same read plus dlogits written) and the resulting TB/s next to the 6.29 TB/s copy
peak measured on this hardware; and the whole forward + backward through autograd for all of them, where (c) can be compared.
Prints us per call (median, min, max over the rounds), the ratios (b)/(a), and whether (b) is faster than (c) by more than (c)'s own
run-to-run spread in this process.
                    usage (GPU box): python tools/bench_seg_loss.py [--iters 100] [--reps 7] [--json profiles/x.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_camvid_amd as A  # noqa: E402
from pytorch_camvid_amd import _lib  # noqa: E402
from pytorch_camvid_amd.functional import _as_nhwc  # noqa: E402

COPY_PEAK_TBS = 6.29


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def torch_dice(y, t, smooth=1.0):
    """The soft Dice term of cvk.SegmentationLoss (dice_average='present', no ignored pixel) from torch ops."""
    C = y.shape[1]
    p = torch.softmax(y, 1)
    oh = torch.nn.functional.one_hot(t, C).permute(0, 3, 1, 2).to(p.dtype)
    I = (p * oh).sum((0, 2, 3)); P = p.sum((0, 2, 3)); T = oh.sum((0, 2, 3))
    present = (T > 0).to(p.dtype)
    return 1 - ((2 * I + smooth) / (P + T + smooth) * present).sum() / present.sum()


def stats(v):
    v = sorted(v)
    return {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds; median, min and max are reported")
    ap.add_argument("--json", default=None, help="also write the summary there")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_seg_loss.py needs the GPU: no timing is taken without one")
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
    M = N * H * W
    fwd_bytes = 4.0 * M * ld + 8.0 * M
    bwd_bytes = fwd_bytes + 4.0 * M * C

    # ---- the raw entry points: forward (+ finish) and backward apart
    lib, check = _lib.load(), _lib.check
    s = torch.cuda.current_stream().cuda_stream
    lg = _as_nhwc(logits)[0]
    part = torch.empty(lib.cvk_seg_loss_part_floats(M, C), device=dev)
    rec = torch.empty(lib.cvk_seg_loss_record_floats(C), device=dev)
    d = torch.empty(M * C, device=dev)
    args = (lg.data_ptr(), ld, t.data_ptr())

    def seg(gamma):
        return (lambda: check(lib.cvk_seg_loss_fwd(*args, None, 1.0, 0.5, gamma, 1.0, 0, part.data_ptr(), rec.data_ptr(), M, C, -100, s), "fwd"),
                lambda: check(lib.cvk_seg_loss_bwd(*args, None, 1.0, 0.5, gamma, rec.data_ptr(), None, 1.0, d.data_ptr(), C, M, C, -100, s), "bwd"))

    raw = {
        "a: cross-entropy": (lambda: check(lib.cvk_softmax_ce_fwd(*args, part.data_ptr(), rec.data_ptr(), M, C, -100, s), "fwd"),
                             lambda: check(lib.cvk_softmax_ce_bwd(*args, rec.data_ptr(), None, 1.0, d.data_ptr(), C, M, C, -100, s), "bwd")),
        "b: ce + 0.5 dice": seg(0.0),
        "b: focal(2) + 0.5 dice": seg(2.0),
    }
    # ---- forward + backward through autograd
    xg = logits.clone().requires_grad_(True)
    assert _as_nhwc(xg)[1] == ld
    ce = A.CrossEntropyLoss()

    def step(lossf):
        def run():
            xg.grad = None
            lossf(xg, t).backward()
        return run

    full = {
        "a: cross-entropy": step(ce),
        "b: ce + 0.5 dice": step(A.SegmentationLoss(1.0, 0.5)),
        "b: focal(2) + 0.5 dice": step(A.SegmentationLoss(1.0, 0.5, focal_gamma=2.0)),
        "c: ce + 0.5 torch dice": step(lambda y, tt: ce(y, tt) + 0.5 * torch_dice(y, tt)),
    }
    # what is timed computes the same thing: (b) against (c)
    lb = A.SegmentationLoss(1.0, 0.5)(xg, t).item()
    lc = (ce(xg, t) + 0.5 * torch_dice(xg, t)).item()
    assert abs(lb - lc) <= 1e-5 * abs(lc), (lb, lc)

    for f, b in raw.values():
        for _ in range(10):
            f(); b()
    for f in full.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    res = {}
    for _ in range(a.reps):
        for k, (f, b) in raw.items():
            res.setdefault(("raw fwd", k), []).append(timed(f, a.iters))
            res.setdefault(("raw bwd", k), []).append(timed(b, a.iters))
        for k, f in full.items():
            res.setdefault(("fwd+bwd", k), []).append(timed(f, a.iters))
    st = {key: stats(v) for key, v in res.items()}

    print(f"logits {N}x{C}x{H}x{W}, ld {ld}; {a.reps} interleaved rounds x {a.iters} calls; copy peak {COPY_PEAK_TBS} TB/s")
    out = {"shape": [N, C, H, W], "ld": ld, "iters": a.iters, "reps": a.reps, "copy_peak_tbs": COPY_PEAK_TBS,
           "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes, "raw": {}, "fwd_bwd": {}}
    for k in raw:
        row = {}
        for which, nbytes in (("raw fwd", fwd_bytes), ("raw bwd", bwd_bytes)):
            m = st[(which, k)]
            row[which.split()[1]] = dict(m, bytes=nbytes, tbs=nbytes / (m["median_us"] * 1e-6) / 1e12)
        out["raw"][k] = row
        print(f"{k:24s} fwd (+ finish) {row['fwd']['median_us']:7.1f} us  {row['fwd']['bytes'] / 1e6:6.1f} MB  {row['fwd']['tbs']:5.2f} TB/s"
              f"   bwd {row['bwd']['median_us']:7.1f} us  {row['bwd']['bytes'] / 1e6:6.1f} MB  {row['bwd']['tbs']:5.2f} TB/s")
    for k in full:
        m = st[("fwd+bwd", k)]
        out["fwd_bwd"][k] = m
        print(f"{k:24s} fwd + bwd through autograd {m['median_us']:8.1f} us  (min {m['min_us']:.1f}, max {m['max_us']:.1f})")
    fa = out["fwd_bwd"]["a: cross-entropy"]["median_us"]
    fc = out["fwd_bwd"]["c: ce + 0.5 torch dice"]
    ra = sum(out["raw"]["a: cross-entropy"][w]["median_us"] for w in ("fwd", "bwd"))
    out["ratios"] = {}
    for k in ("b: ce + 0.5 dice", "b: focal(2) + 0.5 dice"):
        fb = out["fwd_bwd"][k]
        rb = sum(out["raw"][k][w]["median_us"] for w in ("fwd", "bwd"))
        spread = fc["max_us"] - fc["min_us"]
        ok = fc["median_us"] - fb["median_us"] > spread
        out["ratios"][k] = {"b_over_a_fwd_bwd": fb["median_us"] / fa, "b_over_a_raw": rb / ra, "c_over_b_fwd_bwd": fc["median_us"] / fb["median_us"],
                            "c_spread_us": spread, "b_faster_than_c_by_more_than_c_spread": bool(ok)}
        print(f"{k}: (b)/(a) {fb['median_us'] / fa:.3f} through autograd, {rb / ra:.3f} raw kernels; (c)/(b) {fc['median_us'] / fb['median_us']:.2f}; "
              f"(c) - (b) = {fc['median_us'] - fb['median_us']:.1f} us against (c)'s spread of {spread:.1f} us: {'faster' if ok else 'NOT faster'}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
