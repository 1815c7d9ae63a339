#!/usr/bin/env python3
"""HIP-event timing of the OHEM cross-entropy at the headline shape (8 x 12 x 360 x 480, logits from a real UNet so the pixel stride ld
is the network's), in one process and in interleaved rounds:
  (a) cvk.CrossEntropyLoss(weight=w): cvk_softmax_ce_fwd_ex / _bwd_ex, the kernels the OHEM passes are built from
  (b) cvk.OhemCrossEntropyLoss(0.7, 100000, weight=w): cvk_ohem_ce_fwd (six launches) / cvk_ohem_ce_bwd
  (c) the same rule composed from torch ops: cross_entropy(reduction='none'), a full sort for the k-th largest loss, the two
      comparisons, a masked weighted mean, autograd back through all of it
Three views: the raw entry points of (a) and (b), forward and backward apart, with the bytes they must move and the TB/s against the
6.29 TB/s copy peak measured on this hardware; forward + backward through autograd of (b) against cvk.CrossEntropyLoss() and (a); and
(b) against (c) on the same tensors, the two results compared first.  The logits of an untrained network sit near log C, the case
where the per-pixel losses cluster in a few top-level histogram bins; a second raw row times the forward on 3 * randn logits, whose
losses spread over many bins.
                    usage (GPU box): python tools/bench_ohem.py [--iters 100] [--reps 7] [--json profiles/ohem_bench.json]"""
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
THRESH, MIN_KEPT = 0.7, 100000


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def torch_ohem(y, t, w, lam, min_kept):
    """The rule of cvk.OhemCrossEntropyLoss from torch ops (no ignored pixel in this benchmark)."""
    lmap = torch.nn.functional.cross_entropy(y, t, reduction="none")
    flat = lmap.detach().flatten()
    L = torch.sort(flat, descending=True).values[min(min_kept, flat.numel()) - 1]
    kept = ((lmap.detach() > lam) | (lmap.detach() >= L)).to(lmap.dtype)
    wk = w[t] * kept
    return (wk * lmap).sum() / wk.sum()


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
        sys.exit("tools/bench_ohem.py needs the GPU: no timing is taken without one")
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
    lam = A.ohem_loss_threshold(THRESH)
    ce_fwd_bytes = 4.0 * M * ld + 8.0 * M
    ce_bwd_bytes = ce_fwd_bytes + 4.0 * M * C
    ohem_fwd_bytes = ce_fwd_bytes + 4.0 * M + 3 * 4.0 * M + 8.0 * M      # the map written once and read three times, the targets read again
    ohem_bwd_bytes = ce_bwd_bytes + 4.0 * M

    # ---- the raw entry points: forward and backward apart
    lib, check = _lib.load(), _lib.check
    s = torch.cuda.current_stream().cuda_stream
    lg = _as_nhwc(logits)[0]
    spread_logits = (3 * torch.randn(N, H, W, ld, generator=g)).to(dev)
    part = torch.empty(lib.cvk_ce_ex_part_floats(M), device=dev)
    loss4 = torch.empty(4, device=dev)
    scratch = torch.empty(lib.cvk_ohem_scratch_bytes(M), dtype=torch.uint8, device=dev)
    rec = torch.empty(lib.cvk_ohem_record_floats(), device=dev)
    px = torch.empty(M, device=dev)
    d = torch.empty(M * C, device=dev)
    args = (lg.data_ptr(), ld, t.data_ptr(), w.data_ptr())

    def ohem_fwd(ptr):
        return lambda: check(lib.cvk_ohem_ce_fwd(ptr, ld, t.data_ptr(), w.data_ptr(), lam, MIN_KEPT, scratch.data_ptr(), rec.data_ptr(),
                                                 px.data_ptr(), M, C, -100, s), "fwd")

    def ohem_bwd(ptr):
        return lambda: check(lib.cvk_ohem_ce_bwd(ptr, ld, t.data_ptr(), w.data_ptr(), rec.data_ptr(), px.data_ptr(), None, 1.0,
                                                 d.data_ptr(), C, M, C, -100, s), "bwd")

    raw = {
        "a: weighted cross-entropy": (lambda: check(lib.cvk_softmax_ce_fwd_ex(*args, 0.0, 1, part.data_ptr(), loss4.data_ptr(), None, M, C, -100, s), "fwd"),
                                      lambda: check(lib.cvk_softmax_ce_bwd_ex(*args, 0.0, 1, loss4.data_ptr(), None, 1.0, d.data_ptr(), C, M, C, -100, s), "bwd"),
                                      ce_fwd_bytes, ce_bwd_bytes),
        "b: ohem": (ohem_fwd(lg.data_ptr()), ohem_bwd(lg.data_ptr()), ohem_fwd_bytes, ohem_bwd_bytes),
        "b: ohem, spread losses": (ohem_fwd(spread_logits.data_ptr()), ohem_bwd(spread_logits.data_ptr()), ohem_fwd_bytes, ohem_bwd_bytes),
    }
    kept = {}
    for k in ("b: ohem", "b: ohem, spread losses"):
        raw[k][0]()
        r = rec.cpu().tolist()
        kept[k] = {"valid": r[1], "kept": r[4], "L": r[5], "lambda": r[6], "k": r[7],
                   "top_level_bins_in_use": int(torch.unique(px[px >= 0].view(torch.int32) >> 20).numel())}

    # ---- forward + backward through autograd
    xg = logits.clone().requires_grad_(True)
    assert _as_nhwc(xg)[1] == ld

    def step(lossf):
        def run():
            xg.grad = None
            lossf(xg, t).backward()
        return run

    ohem = A.OhemCrossEntropyLoss(THRESH, MIN_KEPT, weight=w)
    full = {
        "cross-entropy": step(A.CrossEntropyLoss()),
        "a: weighted cross-entropy": step(A.CrossEntropyLoss(weight=w)),
        "b: ohem": step(ohem),
        "c: ohem from torch ops": step(lambda y, tt: torch_ohem(y, tt, w, lam, MIN_KEPT)),
    }
    # what is timed computes the same thing: (b) against (c), loss and gradient
    full["b: ohem"]()
    lb, gb = ohem.last_record[0].item(), xg.grad.clone()
    full["c: ohem from torch ops"]()
    lc, gc = torch_ohem(xg, t, w, lam, MIN_KEPT).item(), xg.grad.clone()
    agree = {"loss_b": lb, "loss_c": lc, "loss_rel": abs(lb - lc) / abs(lc), "grad_rel_to_max": ((gb - gc).abs().max() / gc.abs().max()).item()}
    assert agree["loss_rel"] <= 1e-4, agree          # (c) selects on its own fp32 map: a pixel at the boundary may differ, so the gradient is reported only

    for f, b, _, _ in raw.values():
        for _ in range(10):
            f(); b()
    for f in full.values():
        for _ in range(5):
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

    print(f"logits {N}x{C}x{H}x{W}, ld {ld}; thresh {THRESH}, min_kept {MIN_KEPT}; {a.reps} interleaved rounds x {a.iters} calls; "
          f"copy peak {COPY_PEAK_TBS} TB/s")
    out = {"shape": [N, C, H, W], "ld": ld, "thresh": THRESH, "min_kept": MIN_KEPT, "iters": a.iters, "reps": a.reps,
           "copy_peak_tbs": COPY_PEAK_TBS, "selection": kept, "b_against_c": agree, "raw": {}, "fwd_bwd": {}}
    for k, (_, _, fb, bb) in raw.items():
        row = {}
        for which, nbytes in (("raw fwd", fb), ("raw bwd", bb)):
            m = st[(which, k)]
            row[which.split()[1]] = dict(m, bytes=nbytes, tbs=nbytes / (m["median_us"] * 1e-6) / 1e12)
        out["raw"][k] = row
        print(f"{k:28s} fwd {row['fwd']['median_us']:7.1f} us  {row['fwd']['bytes'] / 1e6:6.1f} MB  {row['fwd']['tbs']:5.2f} TB/s"
              f"   bwd {row['bwd']['median_us']:7.1f} us  {row['bwd']['bytes'] / 1e6:6.1f} MB  {row['bwd']['tbs']:5.2f} TB/s")
    for k, v in kept.items():
        print(f"{k:28s} {v}")
    for k in full:
        m = st[("fwd+bwd", k)]
        out["fwd_bwd"][k] = m
        print(f"{k:28s} fwd + bwd through autograd {m['median_us']:8.1f} us  (min {m['min_us']:.1f}, max {m['max_us']:.1f})")
    ra = out["raw"]["a: weighted cross-entropy"]
    rb = out["raw"]["b: ohem"]
    fb, fc = out["fwd_bwd"]["b: ohem"], out["fwd_bwd"]["c: ohem from torch ops"]
    spread = fc["max_us"] - fc["min_us"]
    ok = fc["median_us"] - fb["median_us"] > spread
    out["ratios"] = {"b_over_a_raw_fwd": rb["fwd"]["median_us"] / ra["fwd"]["median_us"],
                     "b_over_a_raw_bwd": rb["bwd"]["median_us"] / ra["bwd"]["median_us"],
                     "b_over_ce_fwd_bwd": fb["median_us"] / out["fwd_bwd"]["cross-entropy"]["median_us"],
                     "c_over_b_fwd_bwd": fc["median_us"] / fb["median_us"], "c_spread_us": spread,
                     "b_faster_than_c_by_more_than_c_spread": bool(ok)}
    print(f"(b)/(a) raw forward {out['ratios']['b_over_a_raw_fwd']:.2f}, raw backward {out['ratios']['b_over_a_raw_bwd']:.2f}; (b)/cross-entropy "
          f"through autograd {out['ratios']['b_over_ce_fwd_bwd']:.2f}; (c)/(b) {out['ratios']['c_over_b_fwd_bwd']:.2f}; (c) - (b) = "
          f"{fc['median_us'] - fb['median_us']:.1f} us against (c)'s spread of {spread:.1f} us: {'faster' if ok else 'NOT faster'}")
    print(f"(b) against (c) on the same tensors: {agree}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
