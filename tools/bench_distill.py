#!/usr/bin/env python3
"""HIP-event timing of the knowledge-distillation loss at the headline shape (8 x 12 x 360 x 480; student logits from a real UNet and
teacher logits from a real SegNet, so each pixel stride is its network's), in one process and in interleaved rounds:
  (a) the weighted cross-entropy, cvk_softmax_ce_fwd_ex / _bwd_ex                     (one logit tensor read)
  (b) cvk.DistillationLoss(1.0, 1.0, temperature=4.0), cvk_kd_loss_fwd / _bwd         (both logit tensors read, one fused pass each way)
  (c) F.cross_entropy(x, t) + t2 * F.kl_div(log_softmax(x / T), softmax(z / T), 'sum') / M composed from torch ops
Two views: the raw entry points of (a) and (b), forward (+ finish) and backward apart, with the bytes each must move (forward:
4 M (ld_s + ld_t) + 8 M read, for (a) without ld_t; backward: the same plus 4 M C written) and the resulting TB/s next to the 6.29 TB/s
copy peak measured on this hardware, and the forward's ratio (b)/(a) next to the traffic model's (4 (ld_s + ld_t) + 8) / (4 ld_s + 8);
and the whole forward + backward through autograd, where (c) can be compared, with the agreement of (b) and (c) on the loss.
                    usage (GPU box): python tools/bench_distill.py [--iters 100] [--reps 7] [--json profiles/distill_bench.json]"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds; median, min and max are reported")
    ap.add_argument("--temperature", type=float, default=4.0)
    ap.add_argument("--json", default=None, help="also write the summary there")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_distill.py needs the GPU: no timing is taken without one")
    dev = torch.device("cuda:0")
    N, C, H, W = 8, 12, 360, 480
    T = a.temperature
    tau, t2 = A.distillation_scales(T)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, 3, H, W, generator=g).to(dev)
    t = torch.randint(0, C, (N, H, W), generator=g).to(dev)
    w = (torch.rand(C, generator=g) + 0.5).to(dev)
    logits = []
    for k, name in enumerate(("unet", "segnet")):
        torch.manual_seed(k)
        net = A.get_model(name, 3, C).to(dev).train()
        with torch.no_grad():
            logits.append(net(x).detach())
        del net
    student, teacher = logits
    (lg, ld_s), (zg, ld_t) = _as_nhwc(student), _as_nhwc(teacher)
    M = N * H * W
    ce_fwd_bytes = 4.0 * M * ld_s + 8.0 * M
    kd_fwd_bytes = 4.0 * M * (ld_s + ld_t) + 8.0 * M
    model_ratio = kd_fwd_bytes / ce_fwd_bytes

    # ---- the raw entry points: forward (+ finish) and backward apart
    lib, check = _lib.load(), _lib.check
    s = torch.cuda.current_stream().cuda_stream
    part = torch.empty(max(lib.cvk_kd_loss_part_floats(M), lib.cvk_ce_ex_part_floats(M)), device=dev)
    rec = torch.empty(lib.cvk_kd_loss_record_floats(), device=dev)
    d = torch.empty(M * C, device=dev)
    kd_head = (lg.data_ptr(), ld_s, zg.data_ptr(), ld_t, t.data_ptr(), w.data_ptr(), 1.0, 1.0, tau, t2, 0)
    raw = {
        "a: weighted cross-entropy": (
            lambda: check(lib.cvk_softmax_ce_fwd_ex(lg.data_ptr(), ld_s, t.data_ptr(), w.data_ptr(), 0.0, 1, part.data_ptr(), rec.data_ptr(),
                                                    None, M, C, -100, s), "fwd"),
            lambda: check(lib.cvk_softmax_ce_bwd_ex(lg.data_ptr(), ld_s, t.data_ptr(), w.data_ptr(), 0.0, 1, rec.data_ptr(), None, 1.0,
                                                    d.data_ptr(), C, M, C, -100, s), "bwd"),
            ce_fwd_bytes),
        "b: distillation": (
            lambda: check(lib.cvk_kd_loss_fwd(*kd_head, part.data_ptr(), rec.data_ptr(), M, C, -100, s), "fwd"),
            lambda: check(lib.cvk_kd_loss_bwd(*kd_head, rec.data_ptr(), None, 1.0, d.data_ptr(), C, M, C, -100, s), "bwd"),
            kd_fwd_bytes),
    }
    # ---- forward + backward through autograd
    xg = student.clone().requires_grad_(True)
    assert _as_nhwc(xg)[1] == ld_s
    kd = A.DistillationLoss(1.0, 1.0, T, weight=w)

    def torch_kd(y, tt):
        ls = torch.log_softmax(y / T, 1)
        q = torch.softmax(teacher / T, 1)
        return F.cross_entropy(y, tt, weight=w) + (T * T) * F.kl_div(ls, q, reduction="sum") / M

    def step(lossf):
        def run():
            xg.grad = None
            lossf(xg, t).backward()
        return run

    full = {
        "a: weighted cross-entropy": step(A.CrossEntropyLoss(weight=w)),
        "b: distillation": step(kd.bind(teacher)),
        "c: torch ce + kl_div": step(torch_kd),
    }
    # what is timed computes the same thing: (b) against (c), loss and gradient
    full["b: distillation"]()
    lb, gb = kd.last_record[0].item(), xg.grad.clone()
    xg.grad = None
    lc_t = torch_kd(xg, t)
    lc_t.backward()
    lc = lc_t.item()
    agree_loss = abs(lb - lc) / abs(lc)
    agree_grad = ((gb - xg.grad).abs().max() / xg.grad.abs().max()).item()
    assert agree_loss <= 1e-5 and agree_grad <= 1e-4, (lb, lc, agree_grad)
    terms, share = kd.last_terms.tolist(), kd.last_agreement.item()

    for f, b, _ in raw.values():
        for _ in range(10):
            f(); b()
    for f in full.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    res = {}
    for _ in range(a.reps):
        for k, (f, b, _) in raw.items():
            res.setdefault(("raw fwd", k), []).append(timed(f, a.iters))
            res.setdefault(("raw bwd", k), []).append(timed(b, a.iters))
        for k, f in full.items():
            res.setdefault(("fwd+bwd", k), []).append(timed(f, a.iters))
    st = {key: stats(v) for key, v in res.items()}

    print(f"logits {N}x{C}x{H}x{W}, ld_s {ld_s}, ld_t {ld_t}, T {T}; {a.reps} interleaved rounds x {a.iters} calls; copy peak {COPY_PEAK_TBS} TB/s")
    print(f"H {terms[0]:.6f}, K {terms[1]:.6f}, arg-max agreement {share:.4f}; (b) against (c): loss rel {agree_loss:.2e}, grad rel-to-max "
          f"{agree_grad:.2e}")
    out = {"shape": [N, C, H, W], "ld_s": ld_s, "ld_t": ld_t, "temperature": T, "iters": a.iters, "reps": a.reps,
           "copy_peak_tbs": COPY_PEAK_TBS, "terms": terms, "argmax_agreement": share, "b_vs_c_loss_rel": agree_loss,
           "b_vs_c_grad_rel_to_max": agree_grad, "raw": {}, "fwd_bwd": {}}
    for k, (_, _, fwd_bytes) in raw.items():
        row = {}
        for which, nbytes in (("raw fwd", fwd_bytes), ("raw bwd", fwd_bytes + 4.0 * M * C)):
            m = st[(which, k)]
            row[which.split()[1]] = dict(m, bytes=nbytes, tbs=nbytes / (m["median_us"] * 1e-6) / 1e12)
        out["raw"][k] = row
        print(f"{k:26s} fwd (+ finish) {row['fwd']['median_us']:7.1f} us  {row['fwd']['bytes'] / 1e6:6.1f} MB  {row['fwd']['tbs']:5.2f} TB/s"
              f"   bwd {row['bwd']['median_us']:7.1f} us  {row['bwd']['bytes'] / 1e6:6.1f} MB  {row['bwd']['tbs']:5.2f} TB/s")
    for k in full:
        m = st[("fwd+bwd", k)]
        out["fwd_bwd"][k] = m
        print(f"{k:26s} fwd + bwd through autograd {m['median_us']:8.1f} us  (min {m['min_us']:.1f}, max {m['max_us']:.1f})")
    ra, rb = out["raw"]["a: weighted cross-entropy"], out["raw"]["b: distillation"]
    fb, fc = out["fwd_bwd"]["b: distillation"], out["fwd_bwd"]["c: torch ce + kl_div"]
    spread = fc["max_us"] - fc["min_us"]
    ok = fc["median_us"] - fb["median_us"] > spread
    out["ratios"] = {"fwd_b_over_a": rb["fwd"]["median_us"] / ra["fwd"]["median_us"], "fwd_traffic_model": model_ratio,
                     "bwd_b_over_a": rb["bwd"]["median_us"] / ra["bwd"]["median_us"],
                     "bwd_traffic_model": (kd_fwd_bytes + 4.0 * M * C) / (ce_fwd_bytes + 4.0 * M * C),
                     "c_over_b_fwd_bwd": fc["median_us"] / fb["median_us"], "c_spread_us": spread,
                     "b_faster_than_c_by_more_than_c_spread": bool(ok)}
    r = out["ratios"]
    print(f"forward (b)/(a) {r['fwd_b_over_a']:.3f} (traffic model {r['fwd_traffic_model']:.3f}); backward (b)/(a) {r['bwd_b_over_a']:.3f} "
          f"(traffic model {r['bwd_traffic_model']:.3f}); (c)/(b) {r['c_over_b_fwd_bwd']:.2f}; (c) - (b) = "
          f"{fc['median_us'] - fb['median_us']:.1f} us against (c)'s spread of {spread:.1f} us: {'faster' if ok else 'NOT faster'}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
