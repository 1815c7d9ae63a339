#!/usr/bin/env python3
"""HIP-event timing of the boundary F1 counts at 8 x 360 x 480 (r2 20) and 8 x 720 x 960 (r2 81), the default tolerance of 0.75 % of
the diagonal at either size, in one process and in interleaved rounds, on blocky maps (a coarse random class grid enlarged by 7 x 9
cells; the prediction is the label shifted by (2, -2) with 3 % of its pixels redrawn; 5 % of the label pixels are void):
  (a) `BoundaryMeter.update` (a zeroed [N,4,K] tensor + one launch of cvk_boundary_counts) and the launch alone;
  (b) `ConfusionMeter.update` on the same tensors: the yardstick.  Both passes read the same 16 B per pixel, the boundary pass re-reads
      the halo of its 32 x 64 tile: (32 + 2R + 2)(64 + 2R + 2) / 2048 of the pixels with R = isqrt(r2);
  (c) the same counts composed from torch ops (one-hot maps, a 3 x 3 erosion for the contours, a (2R + 1)-square `max_pool2d` for the
      tolerance).  A square window only approximates the disc and the 4-neighbourhood, so its TIME is compared, never its values.
Prints us per call (median, min, max over the rounds).
                    usage (GPU box): python tools/bench_boundary.py [--iters 50] [--reps 7] [--json profiles/boundary_bench.json]"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_camvid_amd as A  # noqa: E402
from pytorch_camvid_amd import _lib  # noqa: E402

TILE = (32, 64)                     # BF_TH x BF_TW of csrc/boundary_f1.h
K, IGNORE = 12, 11


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def stats(v):
    v = sorted(v)
    return {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1]}


def blocky_maps(seed, N, H, W, dev):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, K - 1, (N, -(-H // 7) + 1, -(-W // 9) + 1), generator=g)
    label = coarse.repeat_interleave(7, dim=1).repeat_interleave(9, dim=2)[:, :H, :W].contiguous()
    pred = torch.roll(label, (2, -2), dims=(1, 2)).clone()
    redraw = torch.rand((N, H, W), generator=g) < 0.03
    pred[redraw] = torch.randint(0, K - 1, (int(redraw.sum()),), generator=g)
    label[torch.rand((N, H, W), generator=g) < 0.05] = IGNORE
    return pred.to(dev), label.to(dev)


def torch_counts(pred, label, R):
    """An approximation of the counts from torch ops (see the module text): [N,4,K] float."""
    valid = (label != IGNORE).unsqueeze(1)
    out = []
    oh = [F.one_hot(m.clamp(0, K - 1), K).permute(0, 3, 1, 2).float() * valid for m in (pred, label)]
    contour = [o - (-F.max_pool2d(-o, 3, 1, 1)) for o in oh]
    near = [F.max_pool2d(c, 2 * R + 1, 1, R) for c in contour]
    for a, b in ((0, 1), (1, 0)):
        out += [contour[a].sum(dim=(2, 3)), (contour[a] * near[b]).sum(dim=(2, 3))]
    return torch.stack(out, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds; median, min and max are reported")
    ap.add_argument("--json", default=None, help="also write the summary there")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_boundary.py needs the GPU: no timing is taken without one")
    dev = torch.device("cuda:0")
    lib, check = _lib.load(), _lib.check
    s = torch.cuda.current_stream().cuda_stream
    cases, fns = [], {}
    for N, H, W in ((8, 360, 480), (8, 720, 960)):
        r2 = A.boundary_tolerance(H, W)
        R = math.isqrt(r2)
        pred, label = blocky_maps(H, N, H, W, dev)
        bm, cm = A.BoundaryMeter(K, IGNORE), A.ConfusionMeter(K, IGNORE, dev)
        buf = torch.zeros((N, 4, K), device=dev, dtype=torch.int64)

        def update(bm=bm, pred=pred, label=label):
            bm.reset()
            bm.update(pred, label)

        def launch(pred=pred, label=label, buf=buf, N=N, H=H, W=W, r2=r2):
            check(lib.cvk_boundary_counts(pred.data_ptr(), label.data_ptr(), buf.data_ptr(), N, H, W, K, IGNORE, r2, s), "cvk_boundary_counts")

        def confusion(cm=cm, pred=pred, label=label):
            cm.update(pred, label)

        def composed(pred=pred, label=label, R=R):
            return torch_counts(pred, label, R)

        update()
        c = bm.counts().sum(dim=0)
        tag = f"{N}x{H}x{W}"
        halo = (TILE[0] + 2 * R + 2) * (TILE[1] + 2 * R + 2) / (TILE[0] * TILE[1])
        cases.append({"shape": [N, H, W], "r2": r2, "R": R, "halo_reread_factor": halo, "bytes_per_pixel": 16,
                      "boundary_pixels": [int(c[0].sum()), int(c[2].sum())], "matched": [int(c[1].sum()), int(c[3].sum())]})
        fns[tag] = {"BoundaryMeter.update": update, "cvk_boundary_counts": launch, "ConfusionMeter.update": confusion, "torch ops": composed}
    for group in fns.values():
        for f in group.values():
            for _ in range(3):
                f()
    torch.cuda.synchronize()
    res = {}
    for _ in range(a.reps):
        for tag, group in fns.items():
            for name, f in group.items():
                res.setdefault((tag, name), []).append(timed(f, a.iters if name != "torch ops" else max(1, a.iters // 10)))
    for case, tag in zip(cases, fns):
        N, H, W = case["shape"]
        st = {name: stats(res[(tag, name)]) for name in fns[tag]}
        ratios = [b / c for b, c in zip(res[(tag, "cvk_boundary_counts")], res[(tag, "ConfusionMeter.update")])]
        case.update(times=st, launch_over_confusion={"median": sorted(ratios)[len(ratios) // 2], "min": min(ratios), "max": max(ratios)},
                    torch_ops_over_update=st["torch ops"]["median_us"] / st["BoundaryMeter.update"]["median_us"],
                    launch_gbs_at_16_bytes_per_pixel=16.0 * N * H * W / st["cvk_boundary_counts"]["median_us"] / 1e3)
        print(f"{tag}, r2 {case['r2']} (R {case['R']}): {case['boundary_pixels']} boundary pixels, {case['matched']} matched; halo re-read "
              f"factor of the {TILE[0]}x{TILE[1]} tile {case['halo_reread_factor']:.2f}")
        for name, m in st.items():
            print(f"  {name:24s} {m['median_us']:9.1f} us (min {m['min_us']:.1f}, max {m['max_us']:.1f})")
        r = case["launch_over_confusion"]
        print(f"  launch / confusion pass {r['median']:.2f} (min {r['min']:.2f}, max {r['max']:.2f}, round by round); torch ops / update "
              f"{case['torch_ops_over_update']:.1f}; {case['launch_gbs_at_16_bytes_per_pixel']:.0f} GB/s at 16 B/pixel")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"tile": list(TILE), "classes": K, "ignore_index": IGNORE, "iters": a.iters, "reps": a.reps, "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
