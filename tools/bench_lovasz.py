#!/usr/bin/env python3
"""HIP-event timing of the Lovász-softmax loss at the headline shape (8 x 12 x 360 x 480, logits from a real UNet so the pixel stride ld
is the network's), in one process and in interleaved rounds:
  (a) cvk.CrossEntropyLoss(weight=w): cvk_softmax_ce_fwd_ex / _bwd_ex, the in-run yardstick
  (b) cvk.LovaszSoftmaxLoss(): cvk_lovasz_softmax_fwd (error pass, four radix passes of three launches, weight pass, finish) / _bwd
  (c) the same loss composed from torch ops: softmax, and per class |fg - p|, torch.sort, a gather, two cumsums, the Jaccard
      differences and a dot product, autograd back through all of it
Three views: the raw entry points of (a) and (b), forward and backward apart, with the bytes DESIGN.md's traffic model says they must
move and the TB/s against the 6.29 TB/s copy peak measured on this hardware; forward + backward through autograd of (b) against
cvk.CrossEntropyLoss() and (a); and (b) against (c) on the same tensors, the two results compared first.  A second raw row times (b)
with per_image=True (96 segments of 172800 elements instead of 12 of 1382400).
                    usage (GPU box): python tools/bench_lovasz.py [--iters 100] [--reps 7] [--json profiles/lovasz_bench.json]"""
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


def torch_lovasz(y, t):
    """Lovász-softmax over the whole batch from torch ops (every class occurs and no pixel is ignored in this benchmark)."""
    C = y.shape[1]
    p = torch.softmax(y, dim=1).permute(0, 2, 3, 1).reshape(-1, C)
    tf = t.reshape(-1)
    losses = []
    for c in range(C):
        fg = (tf == c).to(p.dtype)
        es, perm = torch.sort((fg - p[:, c]).abs(), descending=True)
        fgs = fg[perm]
        G = fgs.sum()
        jac = 1.0 - (G - fgs.cumsum(0)) / (G + (1.0 - fgs).cumsum(0))
        losses.append(torch.dot(es, torch.cat([jac[:1], jac[1:] - jac[:-1]])))
    return torch.stack(losses).mean()


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
        sys.exit("tools/bench_lovasz.py needs the GPU: no timing is taken without one")
    dev = torch.device("cuda:0")
    N, C, H, W = 8, 12, 360, 480
    torch.manual_seed(0)
    net = A.UNet(3, C).to(dev).train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, 3, H, W, generator=g).to(dev)
    t = torch.randint(0, C, (N, H, W), generator=g).to(dev)
    w = (torch.rand(C, generator=g) + 0.5).to(dev)
    with torch.no_grad():
        logits = net(x).detach()
    ld = _as_nhwc(logits)[1]
    del net
    M = N * H * W
    E = 8.0 * M * C                                                   # one sweep of the 64-bit elements
    ce_fwd_bytes = 4.0 * M * ld + 8.0 * M
    ce_bwd_bytes = ce_fwd_bytes + 4.0 * M * C
    lv_fwd_bytes = (ce_fwd_bytes + E) + 4 * 3 * E + (2 * E + 4.0 * M * C)    # error pass, four passes (count, scatter in and out), weights
    lv_bwd_bytes = ce_bwd_bytes + 4.0 * M * C                         # the g map read beside the logits

    # ---- the raw entry points: forward and backward apart
    lib, check = _lib.load(), _lib.check
    s = torch.cuda.current_stream().cuda_stream
    lg = _as_nhwc(logits)[0]
    part = torch.empty(lib.cvk_ce_ex_part_floats(M), device=dev)
    loss4 = torch.empty(4, device=dev)
    rec = torch.empty(lib.cvk_lovasz_record_floats(), device=dev)
    d = torch.empty(M * C, device=dev)
    args = (lg.data_ptr(), ld, t.data_ptr(), w.data_ptr())
    spaces = {}

    def lv(per_image):
        S = N if per_image else 1
        ws = spaces.setdefault(S, torch.empty(lib.cvk_lovasz_workspace_bytes(M, C, S), dtype=torch.uint8, device=dev))
        gmap = ws[16 * M * C:20 * M * C]
        fwd = lambda: check(lib.cvk_lovasz_softmax_fwd(lg.data_ptr(), ld, t.data_ptr(), None, 1.0, 0.0, 0, int(per_image), N, H * W,
                                                       ws.data_ptr(), rec.data_ptr(), gmap.data_ptr(), C, C, -100, s), "fwd")
        bwd = lambda: check(lib.cvk_lovasz_softmax_bwd(lg.data_ptr(), ld, t.data_ptr(), None, 1.0, 0.0, int(per_image), N, H * W,
                                                       ws.data_ptr(), rec.data_ptr(), gmap.data_ptr(), C, None, 1.0, d.data_ptr(), C, C,
                                                       -100, s), "bwd")
        return fwd, bwd, lv_fwd_bytes, lv_bwd_bytes

    raw = {
        "a: weighted cross-entropy": (lambda: check(lib.cvk_softmax_ce_fwd_ex(*args, 0.0, 1, part.data_ptr(), loss4.data_ptr(), None, M, C, -100, s), "fwd"),
                                      lambda: check(lib.cvk_softmax_ce_bwd_ex(*args, 0.0, 1, loss4.data_ptr(), None, 1.0, d.data_ptr(), C, M, C, -100, s), "bwd"),
                                      ce_fwd_bytes, ce_bwd_bytes),
        "b: lovasz": lv(False),
        "b: lovasz, per image": lv(True),
    }

    # ---- forward + backward through autograd
    xg = logits.clone().requires_grad_(True)
    assert _as_nhwc(xg)[1] == ld

    def step(lossf):
        def run():
            xg.grad = None
            lossf(xg, t).backward()
        return run

    lovasz = A.LovaszSoftmaxLoss()
    full = {
        "cross-entropy": step(A.CrossEntropyLoss()),
        "a: weighted cross-entropy": step(A.CrossEntropyLoss(weight=w)),
        "b: lovasz": step(lovasz),
        "c: lovasz from torch ops": step(torch_lovasz),
    }
    # what is timed computes the same thing: (b) against (c), loss and gradient
    full["b: lovasz"]()
    lb, gb = lovasz.last_record[0].item(), xg.grad.clone()
    full["c: lovasz from torch ops"]()
    lc, gc = torch_lovasz(xg, t).item(), xg.grad.clone()
    agree = {"loss_b": lb, "loss_c": lc, "loss_rel": abs(lb - lc) / abs(lc), "grad_rel_to_max": ((gb - gc).abs().max() / gc.abs().max()).item()}
    assert agree["loss_rel"] <= 1e-3, agree          # (c) sorts its own fp32 errors and differences fp32 Jaccard values: reported, loosely held

    for f, b, _, _ in raw.values():
        for _ in range(5):
            f(); b()
    for f in full.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    res = {}
    for _ in range(a.reps):
        for k, (f, b, _, _) in raw.items():
            res.setdefault(("raw fwd", k), []).append(timed(f, a.iters))
            res.setdefault(("raw bwd", k), []).append(timed(b, a.iters))
        for k, f in full.items():
            res.setdefault(("fwd+bwd", k), []).append(timed(f, a.iters))
    st = {key: stats(v) for key, v in res.items()}

    print(f"logits {N}x{C}x{H}x{W}, ld {ld}; {a.reps} interleaved rounds x {a.iters} calls; copy peak {COPY_PEAK_TBS} TB/s; "
          f"workspace {lib.cvk_lovasz_workspace_bytes(M, C, 1) / 1e6:.1f} MB")
    out = {"shape": [N, C, H, W], "ld": ld, "iters": a.iters, "reps": a.reps, "copy_peak_tbs": COPY_PEAK_TBS,
           "workspace_bytes": lib.cvk_lovasz_workspace_bytes(M, C, 1), "b_against_c": agree, "raw": {}, "fwd_bwd": {}}
    for k, (_, _, fb, bb) in raw.items():
        row = {}
        for which, nbytes in (("raw fwd", fb), ("raw bwd", bb)):
            m = st[(which, k)]
            row[which.split()[1]] = dict(m, bytes=nbytes, tbs=nbytes / (m["median_us"] * 1e-6) / 1e12,
                                         model_us=nbytes / (COPY_PEAK_TBS * 1e12) * 1e6)
        out["raw"][k] = row
        print(f"{k:28s} fwd {row['fwd']['median_us']:8.1f} us  {row['fwd']['bytes'] / 1e6:7.1f} MB  {row['fwd']['tbs']:5.2f} TB/s  (model "
              f"{row['fwd']['model_us']:.0f} us)   bwd {row['bwd']['median_us']:7.1f} us  {row['bwd']['bytes'] / 1e6:6.1f} MB  "
              f"{row['bwd']['tbs']:5.2f} TB/s  (model {row['bwd']['model_us']:.0f} us)")
    for k in full:
        m = st[("fwd+bwd", k)]
        out["fwd_bwd"][k] = m
        print(f"{k:28s} fwd + bwd through autograd {m['median_us']:9.1f} us  (min {m['min_us']:.1f}, max {m['max_us']:.1f})")
    fb, fc = out["fwd_bwd"]["b: lovasz"], out["fwd_bwd"]["c: lovasz from torch ops"]
    spread = fc["max_us"] - fc["min_us"]
    ok = fc["median_us"] - fb["median_us"] > spread
    out["ratios"] = {"b_over_ce_fwd_bwd": fb["median_us"] / out["fwd_bwd"]["cross-entropy"]["median_us"],
                     "c_over_b_fwd_bwd": fc["median_us"] / fb["median_us"], "c_spread_us": spread,
                     "b_faster_than_c_by_more_than_c_spread": bool(ok)}
    print(f"(b)/cross-entropy through autograd {out['ratios']['b_over_ce_fwd_bwd']:.2f}; (c)/(b) {out['ratios']['c_over_b_fwd_bwd']:.2f}; "
          f"(c) - (b) = {fc['median_us'] - fb['median_us']:.1f} us against (c)'s spread of {spread:.1f} us: {'faster' if ok else 'NOT faster'}")
    print(f"(b) against (c) on the same tensors: {agree}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
