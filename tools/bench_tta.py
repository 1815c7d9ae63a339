#!/usr/bin/env python3
"""HIP-event timing of the test-time-augmentation merge at the headline shape (8 x 12 x 360 x 480, scales 0.75 / 1.0 / 1.25 with flip:
six views whose logits come from a real UNet, so their pixel stride is the network's), in one process and in interleaved rounds:
  (a) cvk_tta_accumulate, each of the six launches timed apart and reported by kind (first: stores, middle: read-modify-write,
      last: read-modify-write + mean + arg-max), with the bytes each launch must move (the view's logits gathered once + the
      accumulator read, except on the first view, + the accumulator written + the predictions on the last view) and the resulting
      TB/s next to the 6.29 TB/s copy peak measured on this hardware;
  (b) the whole merge: the six launches of (a) against the same merge composed from torch ops on the same tensors
      (interpolate, softmax, flip, add_ per view, then mul_ and argmax);
  (c) a whole `tta(net, images)` against K = 6 plain eval forwards at 360 x 480 and against the six views' forwards alone.
Prints us per call (median, min, max over the rounds).
                    usage (GPU box): python tools/bench_tta.py [--iters 50] [--reps 7] [--json profiles/tta_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

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


def stats(v):
    v = sorted(v)
    return {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--net-iters", type=int, default=3, help="calls per round of the timings that run the network")
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds; median, min and max are reported")
    ap.add_argument("--json", default=None, help="also write the summary there")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_tta.py needs the GPU: no timing is taken without one")
    dev = torch.device("cuda:0")
    N, C, H, W = 8, 12, 360, 480
    torch.manual_seed(0)
    net = A.UNet(3, C).to(dev).eval()
    x = torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    tta = A.TestTimeAugmentation(scales=(0.75, 1.0, 1.25), flip=True)
    sizes = tta.view_sizes(H, W)
    K = len(sizes)
    with torch.no_grad():
        views = list(tta.views(x))
        logits = [net(v).detach().clone() for v in views]
    M = N * H * W

    # ---- (a) the launches, one by one
    lib, check = _lib.load(), _lib.check
    s = torch.cuda.current_stream().cuda_stream
    acc = torch.empty((N, H, W, C), device=dev)
    pred = torch.empty((N, H, W), device=dev, dtype=torch.int64)
    inv_k = float(np.float32(1.0) / np.float32(K))
    nhwc = [_as_nhwc(lg) for lg in logits]

    def launch(i):
        (lg, ld), (h, w, fl) = nhwc[i], sizes[i]
        lh, lw = lg.shape[1], lg.shape[2]
        return lambda: check(lib.cvk_tta_accumulate(lg.data_ptr(), ld, lh, lw, acc.data_ptr(), pred.data_ptr(), N, H, W, C, int(fl),
                                                    int(i == 0), int(i == K - 1), inv_k, s), "cvk_tta_accumulate")

    def nbytes(i):
        lg = nhwc[i][0]
        return 4.0 * N * lg.shape[1] * lg.shape[2] * C + 4.0 * M * C * (1 if i == 0 else 2) + (8.0 * M if i == K - 1 else 0.0)

    launches = [launch(i) for i in range(K)]

    def fused_merge():
        for f in launches:
            f()

    # ---- (b) the same merge from torch ops
    tacc = torch.empty((N, C, H, W), device=dev).contiguous(memory_format=torch.channels_last)

    def torch_merge():
        for i, (lg, (_, _, fl)) in enumerate(zip(logits, sizes)):
            p = torch.softmax(F.interpolate(lg, (H, W), mode="bilinear", align_corners=False), dim=1)
            if fl:
                p = p.flip(-1)
            if i == 0:
                tacc.copy_(p)
            else:
                tacc.add_(p)
        tacc.mul_(inv_k)
        return tacc.argmax(dim=1)

    fused_merge()
    tp = torch_merge()
    err = float((acc.permute(0, 3, 1, 2) - tacc).abs().max())
    differ = int((tp != pred).sum())
    assert err <= 1e-5, err                                     # what is timed computes the same thing
    print(f"fused merge against the torch composition: max |probs difference| {err:.2e}, {differ} of {M} predictions differ")

    # ---- (c) with the network
    def whole_tta():
        tta(net, x)

    def plain_forwards():
        with torch.no_grad():
            for _ in range(K):
                net(x)

    def view_forwards():
        with torch.no_grad():
            for v in tta.views(x):
                net(v)

    for f in launches:
        for _ in range(5):
            f()
    for f in (fused_merge, torch_merge, whole_tta, plain_forwards, view_forwards):
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    res = {}
    for _ in range(a.reps):
        for i, f in enumerate(launches):
            res.setdefault(("launch", i), []).append(timed(f, a.iters))
        res.setdefault(("merge", "fused"), []).append(timed(fused_merge, max(1, a.iters // 5)))
        res.setdefault(("merge", "torch"), []).append(timed(torch_merge, max(1, a.iters // 5)))
        res.setdefault(("net", "tta(net, images)"), []).append(timed(whole_tta, a.net_iters))
        res.setdefault(("net", f"{K} plain forwards at {H}x{W}"), []).append(timed(plain_forwards, a.net_iters))
        res.setdefault(("net", "the six views' forwards"), []).append(timed(view_forwards, a.net_iters))
    st = {k: stats(v) for k, v in res.items()}

    print(f"accumulator {N}x{C}x{H}x{W}, views {sizes}; {a.reps} interleaved rounds x {a.iters} calls; copy peak {COPY_PEAK_TBS} TB/s")
    out = {"shape": [N, C, H, W], "scales": list(tta.scales), "flip": tta.flip, "views": [list(v) for v in sizes], "iters": a.iters,
           "reps": a.reps, "copy_peak_tbs": COPY_PEAK_TBS, "max_abs_diff_to_torch_composition": err, "predictions_differing": differ,
           "launches": [], "by_kind": {}, "merge": {}, "with_network": {}}
    kinds = {}
    for i in range(K):
        m = st[("launch", i)]
        kind = "first" if i == 0 else "last" if i == K - 1 else "middle"
        lg, ld = nhwc[i]
        row = dict(m, view=i, kind=kind, logits_hw=[lg.shape[1], lg.shape[2]], ld=ld, flipped=sizes[i][2], bytes=nbytes(i),
                   tbs=nbytes(i) / (m["median_us"] * 1e-6) / 1e12)
        out["launches"].append(row)
        kinds.setdefault(kind, []).append(row)
        print(f"view {i} {kind:6s} logits {lg.shape[1]}x{lg.shape[2]} ld {ld}{' mirrored' if sizes[i][2] else '         '}: {m['median_us']:7.1f} us "
              f"(min {m['min_us']:.1f}, max {m['max_us']:.1f})  {nbytes(i) / 1e6:6.1f} MB  {row['tbs']:5.2f} TB/s "
              f"({100 * row['tbs'] / COPY_PEAK_TBS:.0f} % of the copy peak)")
    for kind, rows in kinds.items():
        us = sorted(r["median_us"] for r in rows)[len(rows) // 2]
        b = sum(r["bytes"] for r in rows) / len(rows)
        tbs = sum(r["bytes"] for r in rows) / sum(r["median_us"] for r in rows) / 1e6
        out["by_kind"][kind] = {"median_us": us, "mean_bytes": b, "tbs": tbs}
        print(f"{kind:6s}: {us:7.1f} us per launch, {b / 1e6:6.1f} MB modelled, {tbs:5.2f} TB/s")
    fm, tm = st[("merge", "fused")], st[("merge", "torch")]
    out["merge"] = {"fused": fm, "torch": tm, "torch_over_fused": tm["median_us"] / fm["median_us"]}
    print(f"whole merge, six views: fused {fm['median_us']:.1f} us (min {fm['min_us']:.1f}, max {fm['max_us']:.1f}); torch ops "
          f"{tm['median_us']:.1f} us (min {tm['min_us']:.1f}, max {tm['max_us']:.1f}); torch / fused {tm['median_us'] / fm['median_us']:.2f}")
    for (grp, k), m in st.items():
        if grp == "net":
            out["with_network"][k] = m
            print(f"{k:32s} {m['median_us'] / 1e3:8.2f} ms (min {m['min_us'] / 1e3:.2f}, max {m['max_us'] / 1e3:.2f})")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
