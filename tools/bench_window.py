#!/usr/bin/env python3
"""HIP-event timing of the sliding-window merge at 8 x 12 x 720 x 960, crop 360 x 480, stride 240 x 320 (nine windows whose logits
come from a real UNet, so their pixel stride is the network's), in one process and in interleaved rounds:
  (a) cvk_window_merge, each of the nine launches timed apart, with the bytes each launch must move (the window's logits + `out` read
      where the window is not the first to cover a pixel + `out` written + 8 B of `pred` per pixel the window finishes) and the
      resulting TB/s next to the 6.29 TB/s copy peak measured on this hardware;
  (b) the whole merge: the nine launches of (a) against the same merge composed from torch ops on the same tensors (zero_, a slice add_
      per window, a division by the count matrix, argmax; the count matrix itself is built outside the timed region);
  (c) a whole `sw(net, images)` against nine plain eval forwards at the crop size.
Prints us per call (median, min, max over the rounds).
                    usage (GPU box): python tools/bench_window.py [--iters 50] [--reps 7] [--json profiles/window_bench.json]"""
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


def stats(v):
    v = sorted(v)
    return {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1]}


def launch_bytes(sw, N, C, H, W):
    """Modelled bytes of each launch, from the grid alone: per window (logits, out read, out written, pred)."""
    wins = sw.windows(H, W)
    first = torch.full((H, W), -1, dtype=torch.int64)
    last = torch.full((H, W), -1, dtype=torch.int64)
    for k, (y1, x1, h, w) in enumerate(wins):
        tile = first[y1:y1 + h, x1:x1 + w]
        tile[tile < 0] = k
        last[y1:y1 + h, x1:x1 + w] = k
    rows = []
    for k, (y1, x1, h, w) in enumerate(wins):
        nfirst = int((first[y1:y1 + h, x1:x1 + w] == k).sum())
        nlast = int((last[y1:y1 + h, x1:x1 + w] == k).sum())
        rows.append({"logits": 4.0 * N * h * w * C, "out_read": 4.0 * N * (h * w - nfirst) * C, "out_written": 4.0 * N * h * w * C,
                     "pred": 8.0 * N * nlast})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--net-iters", type=int, default=2, help="calls per round of the timings that run the network")
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds; median, min and max are reported")
    ap.add_argument("--json", default=None, help="also write the summary there")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_window.py needs the GPU: no timing is taken without one")
    dev = torch.device("cuda:0")
    N, C, H, W = 8, 12, 720, 960
    sw = A.SlidingWindow(crop=(360, 480), stride=(240, 320))
    wins = sw.windows(H, W)
    K = len(wins)
    gx = len({x1 for _, x1, _, _ in wins})
    torch.manual_seed(0)
    net = A.UNet(3, C).to(dev).eval()
    x = torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        logits = [net(x[:, :, y1:y1 + h, x1:x1 + w]).detach().clone() for y1, x1, h, w in wins]
    M = N * H * W

    # ---- (a) the launches, one by one
    lib, check = _lib.load(), _lib.check
    s = torch.cuda.current_stream().cuda_stream
    out = torch.empty((N, H, W, C), device=dev)
    pred = torch.empty((N, H, W), device=dev, dtype=torch.int64)
    nhwc = [_as_nhwc(lg) for lg in logits]
    (hc, wc), (sy, sx) = sw.crop, sw.stride

    def launch(k):
        lg, ld = nhwc[k]
        return lambda: check(lib.cvk_window_merge(lg.data_ptr(), ld, out.data_ptr(), pred.data_ptr(), N, H, W, C, hc, wc, sy, sx, k // gx, k % gx, s),
                             "cvk_window_merge")

    launches = [launch(k) for k in range(K)]
    model = launch_bytes(sw, N, C, H, W)

    def fused_merge():
        for f in launches:
            f()

    # ---- (b) the same merge from torch ops
    tout = torch.empty((N, C, H, W), device=dev).contiguous(memory_format=torch.channels_last)
    cnt = sw.counts(H, W).to(dev).to(torch.float32)

    def torch_merge():
        tout.zero_()
        for (y1, x1, h, w), lg in zip(wins, logits):
            tout[:, :, y1:y1 + h, x1:x1 + w].add_(lg)
        tout.div_(cnt)
        return tout.argmax(dim=1)

    fused_merge()
    tp = torch_merge()
    differ_bits = int((out.permute(0, 3, 1, 2).contiguous().view(torch.int32) != tout.contiguous().view(torch.int32)).sum())
    differ = int((tp != pred).sum())
    err = float((out.permute(0, 3, 1, 2) - tout).abs().max())
    print(f"fused merge against the torch composition: {differ_bits} of {M * C} values differ in bits (max |difference| {err:.2e}), "
          f"{differ} of {M} predictions differ")
    assert err <= 1e-5, err                                     # what is timed computes the same thing

    # ---- (c) with the network
    crop_x = x[:, :, :hc, :wc].contiguous()

    def whole_sw():
        sw(net, x)

    def plain_forwards():
        with torch.no_grad():
            for _ in range(K):
                net(crop_x)

    for f in launches:
        for _ in range(5):
            f()
    for f in (fused_merge, torch_merge, whole_sw, plain_forwards):
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    res = {}
    for _ in range(a.reps):
        for k, f in enumerate(launches):
            res.setdefault(("launch", k), []).append(timed(f, a.iters))
        res.setdefault(("merge", "fused"), []).append(timed(fused_merge, max(1, a.iters // 5)))
        res.setdefault(("merge", "torch"), []).append(timed(torch_merge, max(1, a.iters // 5)))
        res.setdefault(("net", "sw(net, images)"), []).append(timed(whole_sw, a.net_iters))
        res.setdefault(("net", f"{K} plain forwards at {hc}x{wc}"), []).append(timed(plain_forwards, a.net_iters))
    st = {k: stats(v) for k, v in res.items()}

    print(f"output {N}x{C}x{H}x{W}, crop {sw.crop}, stride {sw.stride}, {K} windows; {a.reps} interleaved rounds x {a.iters} calls; "
          f"copy peak {COPY_PEAK_TBS} TB/s")
    summary = {"shape": [N, C, H, W], "crop": list(sw.crop), "stride": list(sw.stride), "windows": [list(w) for w in wins], "iters": a.iters,
               "reps": a.reps, "copy_peak_tbs": COPY_PEAK_TBS, "values_differing_in_bits_from_torch_composition": differ_bits, "max_abs_diff_to_torch_composition": err,
               "predictions_differing": differ, "launches": [], "merge": {}, "with_network": {}}
    for k in range(K):
        m, b = st[("launch", k)], model[k]
        total = sum(b.values())
        row = dict(m, window=k, at=list(wins[k][:2]), ld=nhwc[k][1], bytes=total, bytes_by_part=b, tbs=total / (m["median_us"] * 1e-6) / 1e12)
        summary["launches"].append(row)
        print(f"window {k} at {wins[k][:2]} ld {nhwc[k][1]}: {m['median_us']:7.1f} us (min {m['min_us']:.1f}, max {m['max_us']:.1f})  "
              f"{total / 1e6:6.1f} MB  {row['tbs']:5.2f} TB/s ({100 * row['tbs'] / COPY_PEAK_TBS:.0f} % of the copy peak)")
    all_b, all_us = sum(r["bytes"] for r in summary["launches"]), sum(r["median_us"] for r in summary["launches"])
    summary["all_launches"] = {"sum_of_medians_us": all_us, "bytes": all_b, "tbs": all_b / all_us / 1e6}
    print(f"nine launches: {all_us:.1f} us in all, {all_b / 1e6:.1f} MB modelled, {all_b / all_us / 1e6:.2f} TB/s")
    fm, tm = st[("merge", "fused")], st[("merge", "torch")]
    summary["merge"] = {"fused": fm, "torch": tm, "torch_over_fused": tm["median_us"] / fm["median_us"]}
    print(f"whole merge, {K} windows: fused {fm['median_us']:.1f} us (min {fm['min_us']:.1f}, max {fm['max_us']:.1f}); torch ops "
          f"{tm['median_us']:.1f} us (min {tm['min_us']:.1f}, max {tm['max_us']:.1f}); torch / fused {tm['median_us'] / fm['median_us']:.2f}")
    for (grp, k), m in st.items():
        if grp == "net":
            summary["with_network"][k] = m
            print(f"{k:32s} {m['median_us'] / 1e3:8.2f} ms (min {m['min_us'] / 1e3:.2f}, max {m['max_us'] / 1e3:.2f})")
    sw_ms = st[("net", "sw(net, images)")]["median_us"]
    summary["merge_share_of_sw"] = fm["median_us"] / sw_ms
    print(f"the merge is {100 * fm['median_us'] / sw_ms:.1f} % of sw(net, images)")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
