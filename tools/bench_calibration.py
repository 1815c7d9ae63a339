#!/usr/bin/env python3
"""HIP-event timing of the calibration meter and the temperature fit at the headline shape (8 x 12 x 360 x 480, ld 12), in one process
and in interleaved rounds:
  ce      cvk_softmax_ce_fwd: the yardstick.  It reads the same 4 ld M + 8 M bytes (77.4 MB) as every pass below
  meter   cvk.CalibrationMeter.update: cvk_calib_accumulate with tables (the cross-entropy's traffic + the LDS histogram)
  map     cvk.confidence_map: the same kernel without tables (reads 4 ld M, writes 12 M)
  newton  one cvk_calib_newton_accumulate pass
  fit     cvk.TemperatureScaler(iterations=20).fit over four stored batches: 84 passes, 21 steps, no host sync
against the torch-op compositions on the same tensors: for the meter softmax, max, bucketize and three bincounts; for the fit
torch.optim.LBFGS on log T (20 iterations).  Two kinds of logits: an untrained UNet's (confidences near 1 / C: few bins in use) and
3 * randn sharpened towards the labels (confidences clustered in the top bins, where the 64-bit LDS atomics of a wave collide most).
The meter's tables and the fitted temperature are compared with the compositions before anything is timed.
                    usage (GPU box): python tools/bench_calibration.py [--iters 100] [--reps 7] [--json profiles/calibration_bench.json]"""
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
BINS = 15
CE_FWD_LAST_RECORDED_US = 26.7


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


def torch_meter(logits, t, C, bins, edges):
    """The meter's top-label table from torch ops: (count, correct, sum conf) per bin over every pixel (no ignored pixel here)."""
    conf, pred = torch.softmax(logits, dim=1).max(dim=1)
    b = torch.bucketize(conf.flatten(), edges, right=False).clamp_(0, bins - 1)
    right = (pred == t).flatten()
    return (torch.bincount(b, minlength=bins), torch.bincount(b, weights=right.double(), minlength=bins),
            torch.bincount(b, weights=conf.flatten().double(), minlength=bins))


def torch_fit(logits_list, labels_list, iterations):
    """Guo's recipe: LBFGS on log T over the stored logits; every closure evaluation re-reads them all."""
    log_t = torch.zeros((), device=logits_list[0].device, requires_grad=True)
    opt = torch.optim.LBFGS([log_t], lr=1.0, max_iter=iterations, line_search_fn="strong_wolfe")
    n = sum(l.numel() for l in labels_list)

    def closure():
        opt.zero_grad()
        loss = sum(torch.nn.functional.cross_entropy(x * torch.exp(-log_t), t, reduction="sum") for x, t in zip(logits_list, labels_list)) / n
        loss.backward()
        return loss

    opt.step(closure)
    return float(torch.exp(log_t.detach()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds; median, min and max are reported")
    ap.add_argument("--json", default=None, help="also write the summary there")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_calibration.py needs the GPU: no timing is taken without one")
    dev = torch.device("cuda:0")
    N, C, H, W = 8, 12, 360, 480
    M = N * H * W
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    net = A.UNet(3, C).to(dev).eval()
    t = torch.randint(0, C, (N, H, W), generator=g).to(dev)
    with torch.no_grad():
        flat = net(torch.randn(N, 3, H, W, generator=g).to(dev)).detach()
    del net
    sharp = (3 * torch.randn(N, H, W, C, generator=g)).to(dev)
    sharp.scatter_add_(3, t.unsqueeze(3), torch.full((N, H, W, 1), 6.0, device=dev))     # the label's logit raised: most pixels right and sure
    sharp = sharp.permute(0, 3, 1, 2)
    kinds = {"unet": flat, "sharp": sharp}
    for v in kinds.values():
        assert _as_nhwc(v)[1] == C
    ld = C
    nbytes = 4.0 * ld * M + 8.0 * M
    map_bytes = 4.0 * ld * M + 12.0 * M

    lib, check = _lib.load(), _lib.check
    s = torch.cuda.current_stream().cuda_stream
    part3 = torch.empty(3 * lib.cvk_ce_blocks(M), device=dev)
    loss3 = torch.empty(4, device=dev)
    part4 = torch.empty(4 * lib.cvk_ce_blocks(M), device=dev, dtype=torch.float64)
    state = torch.zeros(9, device=dev, dtype=torch.float64)
    state[0], state[1], state[2] = 1.0, 1.0 / 64.0, 64.0
    edges = (torch.arange(1, BINS, device=dev, dtype=torch.float32) / BINS)
    runs, facts = {}, {}
    for kind, logits in kinds.items():
        lg = _as_nhwc(logits)[0]
        meter = A.CalibrationMeter(C, -100, BINS, device=dev)
        four = [logits] * 4, [t] * 4
        scaler = A.TemperatureScaler(iterations=20, ignore_index=-100, device=dev)
        runs[kind] = {
            "ce": lambda lg=lg: check(lib.cvk_softmax_ce_fwd(lg.data_ptr(), ld, t.data_ptr(), part3.data_ptr(), loss3.data_ptr(), M, C, -100, s), "ce"),
            "meter": lambda meter=meter, logits=logits: meter.update(logits, t),
            "map": lambda logits=logits: A.confidence_map(logits),
            "newton": lambda lg=lg: check(lib.cvk_calib_newton_accumulate(lg.data_ptr(), ld, t.data_ptr(), state.data_ptr(), part4.data_ptr(),
                                                                           M, C, -100, s), "newton"),
            "fit": lambda scaler=scaler, four=four: scaler.fit(*four),
            "torch meter": lambda logits=logits: torch_meter(logits, t, C, BINS, edges),
            "torch fit": lambda four=four: torch_fit(four[0], four[1], 20),
        }
        # what is timed computes the same thing
        meter.update(logits, t)
        top = meter.hist.sum(dim=0)
        cnt, right, conf = torch_meter(logits, t, C, BINS, edges)
        moved = int((top[:, 0] - cnt).abs().sum()) // 2                    # pixels a last-bit difference in conf puts into the neighbouring bin
        scores = meter.compute()
        scaler.fit(*four)
        T_torch = torch_fit(four[0], four[1], 20)
        facts[kind] = {"ece": scores["ece"], "nll": scores["nll"], "accuracy": scores["accuracy"],
                       "bins_in_use": int((top[:, 0] > 0).sum()), "share_in_top_bin": float(top[-1, 0]) / M,
                       "pixels_binned_otherwise_than_torch": moved,
                       "correct_total": [int(top[:, 1].sum()), int(right.sum())],
                       "T_fit": scaler.temperature, "T_lbfgs": T_torch, "converged": scaler.converged, "at_bound": scaler.at_bound}
        # torch takes the arg-max of the rounded probabilities, the meter of the logits: logits a last bit apart may tie there
        assert moved <= 1e-4 * M and abs(int(top[:, 1].sum()) - int(right.sum())) <= 1e-5 * M, facts[kind]
        meter.reset()

    calls = {"fit": max(1, a.iters // 20), "torch fit": 1}              # per round; the LBFGS line search re-reads the logits up to 25 times an iteration
    for fns in runs.values():
        for k, f in fns.items():
            for _ in range(1 if k in calls else 10):
                f()
    torch.cuda.synchronize()
    res = {}
    for _ in range(a.reps):
        for kind, fns in runs.items():
            for k, f in fns.items():
                res.setdefault((kind, k), []).append(timed(f, calls.get(k, a.iters)))
    print(f"logits {N}x{C}x{H}x{W}, ld {ld}, {BINS} bins; {a.reps} interleaved rounds x {a.iters} calls ({calls['fit']} for the fit, 1 for the LBFGS fit); "
          f"copy peak {COPY_PEAK_TBS} TB/s; cross-entropy forward last recorded at {CE_FWD_LAST_RECORDED_US} us")
    out = {"shape": [N, C, H, W], "ld": ld, "bins": BINS, "iters": a.iters, "reps": a.reps, "copy_peak_tbs": COPY_PEAK_TBS,
           "bytes": {"ce, meter, newton": nbytes, "map": map_bytes}, "ce_fwd_last_recorded_us": CE_FWD_LAST_RECORDED_US, "kinds": {}}
    for kind, fns in runs.items():
        st = {k: stats(res[(kind, k)]) for k in fns}
        ce = st["ce"]["median_us"]
        for k in ("ce", "meter", "newton"):
            st[k]["tbs"] = nbytes / (st[k]["median_us"] * 1e-6) / 1e12
        st["map"]["tbs"] = map_bytes / (st["map"]["median_us"] * 1e-6) / 1e12
        ratios = {"meter_over_ce": st["meter"]["median_us"] / ce, "map_over_ce": st["map"]["median_us"] / ce,
                  "newton_over_ce": st["newton"]["median_us"] / ce, "fit_over_84_ce": st["fit"]["median_us"] / (84 * ce),
                  "torch_meter_over_meter": st["torch meter"]["median_us"] / st["meter"]["median_us"],
                  "torch_fit_over_fit": st["torch fit"]["median_us"] / st["fit"]["median_us"]}
        out["kinds"][kind] = {"timings": st, "ratios": ratios, "facts": facts[kind]}
        print(f"-- {kind}: {facts[kind]}")
        for k, m in st.items():
            print(f"{k:12s} {m['median_us']:10.1f} us  (min {m['min_us']:.1f}, max {m['max_us']:.1f})" + (f"  {m['tbs']:5.2f} TB/s" if "tbs" in m else ""))
        print("   " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
