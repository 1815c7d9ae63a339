#!/usr/bin/env python3
"""HIP-event timing of the distance transform and the boundary loss at the headline shape (8 x 12 x 360 x 480; labels =
tests/boundary_ref.py::blocky_maps(0, 8, 360, 480), 11 classes + void; logits from a real UNet so the pixel stride ld is the network's),
in one process and in interleaved rounds:
  raw entry points   cvk_edt_squared and cvk_edt_signed (clear + column pass + row pass each), cvk_boundary_loss_fwd / _bwd, against the
                     weighted cross-entropy's cvk_softmax_ce_fwd_ex / _bwd_ex on the same tensors, with the bytes DESIGN.md's traffic
                     model says they must move and the TB/s against the 6.29 TB/s copy peak measured on this hardware
  by kernel          the column pass, the row pass and the loss kernels apart, from a kernel trace of the same calls (torch.profiler;
                     "unavailable" where the trace cannot be taken)
  through autograd   cvk.BoundaryLoss() (maps + loss + backward) against (a) F.softmax and (phi * p) composed from torch ops on
                     PRECOMPUTED maps and (b) the host path: scipy's distance_transform_edt of the same batch on this machine's CPU,
                     one core, timed once
  adversarial        the distance transform of a batch in which every class is a single pixel in one corner, so that every search
                     runs the full width: the data dependence of the row pass, on record
                    usage (GPU box): python tools/bench_boundary_loss.py [--iters 100] [--reps 7] [--json profiles/boundary_loss_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_camvid_amd as A  # noqa: E402
from pytorch_camvid_amd import _lib  # noqa: E402
from pytorch_camvid_amd.functional import _as_nhwc  # noqa: E402
from tests.boundary_ref import blocky_maps  # noqa: E402

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


def torch_boundary(phi):
    def f(y, t):
        valid = (t != 11)[:, None]
        return (phi * torch.softmax(y, dim=1) * valid).sum() / valid.sum()
    return f


def scipy_maps(labels, C, ign):
    """Kervadec's one_hot2dist per image and class on the host, as the public implementations do it in the data loader."""
    from scipy.ndimage import distance_transform_edt as edt
    out = np.zeros((labels.shape[0], C) + labels.shape[1:], dtype=np.float32)
    for n, lab in enumerate(labels):
        for c in range(C):
            pos = (lab == c) & (lab != ign)
            if pos.any():
                out[n, c] = edt(~pos) * ~pos - (edt(pos) - 1) * pos
    return out


def kernel_trace(calls, iters):
    """{kernel name prefix: mean us} of the k_edt_* / k_bdl_* kernels over `iters` rounds of `calls`, or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                for f in calls:
                    f()
            torch.cuda.synchronize()
        rows = {}
        for ev in prof.key_averages():
            for name in ("k_edt_cols", "k_edt_rows", "k_bdl_fwd", "k_bdl_finish", "k_bdl_bwd", "k_lv_clear"):
                if name in ev.key:
                    total = getattr(ev, "device_time_total", None)
                    if total is None:
                        total = ev.cuda_time_total
                    rows[ev.key[:120]] = {"mean_us": total / max(ev.count, 1), "calls": ev.count}
        return rows or None
    except Exception as e:                                 # no tracer on this box: the event timings above stand alone
        return {"unavailable": repr(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds; median, min and max are reported")
    ap.add_argument("--json", default=None, help="also write the summary there")
    ap.add_argument("--no-host", action="store_true", help="skip the scipy host path")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_boundary_loss.py needs the GPU: no timing is taken without one")
    dev = torch.device("cuda:0")
    N, C, H, W, IGN = 8, 12, 360, 480, 11
    torch.manual_seed(0)
    net = A.UNet(3, C).to(dev).train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, 3, H, W, generator=g).to(dev)
    labels_np = blocky_maps(0, N, H, W)[1]
    t = torch.from_numpy(labels_np).to(dev)
    w = (torch.rand(C, generator=g) + 0.5).to(dev)
    with torch.no_grad():
        logits = net(x).detach()
    ld = _as_nhwc(logits)[1]
    del net
    M = N * H * W
    adv_np = np.zeros((N, H, W), dtype=np.int64)           # class 0 everywhere, every other class one pixel in the top-left corner
    for c in range(1, C - 1):
        adv_np[:, 0, c - 1] = c
    adv = torch.from_numpy(adv_np).to(dev)

    ce_fwd_bytes = 4.0 * M * ld + 8.0 * M
    ce_bwd_bytes = ce_fwd_bytes + 4.0 * M * C
    col_bytes = (8.0 + 2.0 * (C + 1)) * M
    sq_bytes = col_bytes + (2.0 * (C + 1) + 8.0 + 4.0 * C + 4.0) * M   # + to_other
    sg_bytes = col_bytes + (2.0 * (C + 1) + 8.0 + 4.0 * C) * M
    bl_fwd_bytes = ce_fwd_bytes + 4.0 * M * C
    bl_bwd_bytes = bl_fwd_bytes + 4.0 * M * C

    lib, check = _lib.load(), _lib.check
    s = torch.cuda.current_stream().cuda_stream
    lg = _as_nhwc(logits)[0]
    ws = torch.empty(lib.cvk_edt_workspace_bytes(N, H, W, C), dtype=torch.uint8, device=dev)
    to_class = torch.empty((N, H, W, C), dtype=torch.int32, device=dev)
    to_other = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    phi = torch.empty((N, H, W, C), device=dev)
    part_ce = torch.empty(lib.cvk_ce_ex_part_floats(M), device=dev)
    loss4 = torch.empty(4, device=dev)
    part = torch.empty(lib.cvk_boundary_loss_part_floats(M, C), device=dev)
    rec = torch.empty(lib.cvk_boundary_loss_record_floats(), device=dev)
    coef = torch.tensor([1.0, 0.0], device=dev)
    d = torch.empty(M * C, device=dev)
    mask = (1 << C) - 1
    ce_args = (lg.data_ptr(), ld, t.data_ptr(), w.data_ptr())

    def squared(lab):
        return lambda: check(lib.cvk_edt_squared(lab.data_ptr(), N, H, W, C, IGN, ws.data_ptr(), to_class.data_ptr(), to_other.data_ptr(), s), "edt")

    def signed(lab):
        return lambda: check(lib.cvk_edt_signed(lab.data_ptr(), N, H, W, C, IGN, ws.data_ptr(), phi.data_ptr(), s), "edt")

    bl_fwd = lambda: check(lib.cvk_boundary_loss_fwd(lg.data_ptr(), ld, t.data_ptr(), phi.data_ptr(), None, coef.data_ptr(), 1, 0, mask,
                                                     part.data_ptr(), rec.data_ptr(), M, C, IGN, s), "fwd")
    bl_bwd = lambda: check(lib.cvk_boundary_loss_bwd(lg.data_ptr(), ld, t.data_ptr(), phi.data_ptr(), None, 1, 0, mask, rec.data_ptr(), None,
                                                     1.0, d.data_ptr(), C, M, C, IGN, s), "bwd")
    raw = {
        "edt squared, adversarial": (squared(adv), sq_bytes),
        "edt signed, adversarial": (signed(adv), sg_bytes),
        "edt squared": (squared(t), sq_bytes),
        "edt signed": (signed(t), sg_bytes),                # last of the four: phi of the blocky labels is what the loss rows read
        "weighted cross-entropy fwd": (lambda: check(lib.cvk_softmax_ce_fwd_ex(*ce_args, 0.0, 1, part_ce.data_ptr(), loss4.data_ptr(), None, M, C,
                                                                               IGN, s), "fwd"), ce_fwd_bytes),
        "weighted cross-entropy bwd": (lambda: check(lib.cvk_softmax_ce_bwd_ex(*ce_args, 0.0, 1, loss4.data_ptr(), None, 1.0, d.data_ptr(), C, M, C,
                                                                               IGN, s), "bwd"), ce_bwd_bytes),
        "boundary loss fwd": (bl_fwd, bl_fwd_bytes),
        "boundary loss bwd": (bl_bwd, bl_bwd_bytes),
    }

    # ---- forward + backward through autograd
    xg = logits.clone().requires_grad_(True)
    assert _as_nhwc(xg)[1] == ld
    bl = A.BoundaryLoss(ignore_index=IGN)

    def step(lossf):
        def run():
            xg.grad = None
            lossf(xg, t).backward()
        return run

    phi_pre = A.signed_distance_maps(t, C, IGN)
    full = {
        "cross-entropy": step(A.CrossEntropyLoss(ignore_index=IGN)),
        "boundary loss (maps + loss)": step(bl),
        "a: softmax and (phi * p) from torch ops, maps precomputed": step(torch_boundary(phi_pre)),
    }
    full["boundary loss (maps + loss)"]()
    lb, gb = bl.last_record[0].item(), xg.grad.clone()
    full["a: softmax and (phi * p) from torch ops, maps precomputed"]()
    la, ga = torch_boundary(phi_pre)(xg, t).item(), xg.grad.clone()
    agree = {"loss_kernel": lb, "loss_torch": la, "loss_rel": abs(lb - la) / abs(la), "grad_rel_to_max": ((gb - ga).abs().max() / ga.abs().max()).item()}
    assert agree["loss_rel"] <= 1e-4, agree

    host = None
    if not a.no_host:
        torch.set_num_threads(1)
        t0 = time.perf_counter()
        host_phi = scipy_maps(labels_np, C, IGN)
        host = {"seconds": time.perf_counter() - t0, "threads": 1}
        import scipy
        host["scipy"] = scipy.__version__
        # scipy's maps are fp64 roots rounded once; the kernel's are the fp32 roots of the integers: equal to an ulp
        host["max_abs_diff_to_kernel"] = float(np.abs(host_phi - phi_pre.cpu().numpy()).max())

    for f, _ in raw.values():
        for _ in range(3):
            f()
    for f in full.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    res = {}
    for _ in range(a.reps):
        for k, (f, _) in raw.items():
            res.setdefault(("raw", k), []).append(timed(f, 10 if "adversarial" in k else a.iters))
        for k, f in full.items():
            res.setdefault(("fwd+bwd", k), []).append(timed(f, a.iters))
    st = {key: stats(v) for key, v in res.items()}
    trace = {"blocky": kernel_trace([raw["edt squared"][0], raw["edt signed"][0], bl_fwd, bl_bwd], 20),
             "adversarial": kernel_trace([raw["edt signed, adversarial"][0]], 3)}

    print(f"logits {N}x{C}x{H}x{W}, ld {ld}; {a.reps} interleaved rounds x {a.iters} calls (adversarial: 10); copy peak {COPY_PEAK_TBS} TB/s; "
          f"workspace {ws.numel() / 1e6:.1f} MB + phi {phi.numel() * 4 / 1e6:.1f} MB")
    out = {"shape": [N, C, H, W], "ld": ld, "iters": a.iters, "reps": a.reps, "copy_peak_tbs": COPY_PEAK_TBS, "workspace_bytes": ws.numel(),
           "phi_bytes": phi.numel() * 4, "kernel_against_torch": agree, "host": host, "raw": {}, "fwd_bwd": {}, "kernel_trace": trace}
    for k, (_, nbytes) in raw.items():
        m = st[("raw", k)]
        out["raw"][k] = dict(m, bytes=nbytes, tbs=nbytes / (m["median_us"] * 1e-6) / 1e12, model_us=nbytes / (COPY_PEAK_TBS * 1e12) * 1e6)
        r = out["raw"][k]
        print(f"{k:30s} {r['median_us']:10.1f} us (min {r['min_us']:.1f}, max {r['max_us']:.1f})  {nbytes / 1e6:7.1f} MB  {r['tbs']:5.2f} TB/s  "
              f"(model {r['model_us']:.1f} us)")
    for which, rows in trace.items():
        for name, row in (rows or {}).items():
            print(f"trace, {which}: {name[:90]:90s} {row}")
    for k in full:
        m = st[("fwd+bwd", k)]
        out["fwd_bwd"][k] = m
        print(f"{k:60s} fwd + bwd through autograd {m['median_us']:9.1f} us  (min {m['min_us']:.1f}, max {m['max_us']:.1f})")
    fb = out["fwd_bwd"]["boundary loss (maps + loss)"]["median_us"]
    fa = out["fwd_bwd"]["a: softmax and (phi * p) from torch ops, maps precomputed"]["median_us"]
    out["ratios"] = {"boundary_over_ce_fwd_bwd": fb / out["fwd_bwd"]["cross-entropy"]["median_us"], "torch_over_boundary_fwd_bwd": fa / fb,
                     "host_maps_over_boundary_step": host["seconds"] * 1e6 / fb if host else None,
                     "adversarial_over_blocky_signed": out["raw"]["edt signed, adversarial"]["median_us"] / out["raw"]["edt signed"]["median_us"]}
    print(f"ratios: {out['ratios']}")
    print(f"kernel against torch ops on the same tensors: {agree}")
    print(f"host path: {host}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
