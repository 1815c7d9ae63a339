#!/usr/bin/env python3
"""HIP-event timing of the surface-distance meter (cvk_surface_distances: Hausdorff, HD95, ASSD) at 8 x 360 x 480 and 8 x 720 x 960, in
one process and in interleaved rounds, on blocky maps (a coarse random class grid enlarged by 7 x 9 cells; the prediction is the label
shifted by (2, -2) with 3 % of its pixels redrawn; 5 % of the label pixels are void):
  (a) `SurfaceDistanceMeter.update` (a new record tensor + one call) and the entry point alone (its eight launches);
  (b) yardsticks on the same tensors: `BoundaryMeter.update`, `ConfusionMeter.update`, and `cvk_edt_squared` of the label map (the dense
      distance transform the sparse search is meant to undercut);
  (c) the adversarial pair: one small blob of a class in opposite corners, one per map, so that every search runs the full width;
  (d) the host path of the public libraries, timed once on one core: per image and class scipy's distance_transform_edt of the
      complement of either contour mask, then maximum, percentile and mean of the distances read at the other contour.
Prints us per call (median, min, max over the rounds) and the traffic model's floor next to the measured time.
                    usage (GPU box): python tools/bench_surface.py [--iters 50] [--reps 7] [--json profiles/surface_bench.json]"""
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
from tools.bench_boundary import blocky_maps, stats, timed  # noqa: E402

K, IGNORE = 12, 11
COPY_PEAK_TBS = 6.29


def model_bytes(N, H, W, lib):
    """The traffic model of DESIGN.md: bytes per call if every byte moved once at the copy peak."""
    M = N * H * W
    per_pixel = (24 + 2) + (2 + 4 * K) + (2 + 4 * K + 8) + 8          # contour bytes | column walk | row search | refine
    S = 2 * N * K
    far = (H - 1) ** 2 + (W - 1) ** 2
    nb1 = (far if far < 4096 else 4095 + (far >> 12)) + 1             # first-level bins: one per value below 4096, one per 4096 above
    cleared = S * (16 + 4 + 4 * nb1 + 2 * 4096 * 4) + 8 * N
    return per_pixel * M + cleared, 4 * K * M                         # second: the up-walk's re-read of its own stores when it misses L2


def corner_blobs(N, H, W, dev):
    label = torch.zeros((N, H, W), dtype=torch.int64)
    pred = label.clone()
    label[:, 2:5, 2:5] = 1
    pred[:, H - 5:H - 2, W - 5:W - 2] = 1
    return pred.to(dev), label.to(dev)


def host_path(pred, label, q=95.0):
    """MONAI / medpy's recipe with scipy, per image and class, on the meter's contours.  Returns seconds."""
    from scipy import ndimage
    bP = A.label_boundaries(pred, K, IGNORE, void_from=label).cpu().numpy()
    bG = A.label_boundaries(label, K, IGNORE).cpu().numpy()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for n in range(bP.shape[0]):
        for c in range(K):
            p, g = bP[n] == c, bG[n] == c
            if not (p.any() and g.any()):
                continue
            dPG, dGP = ndimage.distance_transform_edt(~g)[p], ndimage.distance_transform_edt(~p)[g]
            max(dPG.max(), dGP.max()), max(np.percentile(dPG, q), np.percentile(dGP, q)), (dPG.sum() + dGP.sum()) / (len(dPG) + len(dGP))
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds; median, min and max are reported")
    ap.add_argument("--json", default=None, help="also write the summary there")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_surface.py needs the GPU: no timing is taken without one")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    lib, check = _lib.load(), _lib.check
    s = torch.cuda.current_stream().cuda_stream
    cases, fns = [], {}
    for N, H, W, kind in ((8, 360, 480, "blocky"), (8, 720, 960, "blocky"), (8, 360, 480, "corner blobs")):
        pred, label = blocky_maps(H, N, H, W, dev) if kind == "blocky" else corner_blobs(N, H, W, dev)
        sm, bm, cm = A.SurfaceDistanceMeter(K, IGNORE), A.BoundaryMeter(K, IGNORE), A.ConfusionMeter(K, IGNORE, dev)
        ws = torch.empty(lib.cvk_surface_workspace_bytes(N, H, W, K), device=dev, dtype=torch.uint8)
        d2 = torch.empty((2, N, H, W), device=dev, dtype=torch.int32)
        rec = torch.empty((N, 2, K, 8), device=dev, dtype=torch.int64)
        ews = torch.empty(lib.cvk_edt_workspace_bytes(N, H, W, K), device=dev, dtype=torch.uint8)
        to_class = torch.empty((N, H, W, K), device=dev, dtype=torch.int32)
        to_other = torch.empty((N, H, W), device=dev, dtype=torch.int32)

        def update(sm=sm, pred=pred, label=label):
            sm.reset()
            sm.update(pred, label)

        def entry(pred=pred, label=label, ws=ws, d2=d2, rec=rec, N=N, H=H, W=W):
            check(lib.cvk_surface_distances(pred.data_ptr(), label.data_ptr(), N, H, W, K, IGNORE, 19, 20, ws.data_ptr(), d2.data_ptr(),
                                            rec.data_ptr(), s), "cvk_surface_distances")

        def boundary(bm=bm, pred=pred, label=label):
            bm.reset()
            bm.update(pred, label)

        def confusion(cm=cm, pred=pred, label=label):
            cm.update(pred, label)

        def edt(label=label, ews=ews, to_class=to_class, to_other=to_other, N=N, H=H, W=W):
            check(lib.cvk_edt_squared(label.data_ptr(), N, H, W, K, IGNORE, ews.data_ptr(), to_class.data_ptr(), to_other.data_ptr(), s),
                  "cvk_edt_squared")

        update()
        out = sm.compute()
        r = sm.records()
        floor, reread = model_bytes(N, H, W, lib)
        case = {"shape": [N, H, W], "maps": kind, "contour_pixels": [int(r[:, 0, :, 0].sum()), int(r[:, 1, :, 0].sum())],
                "largest_d2": int(r[..., 2].max()), "hd95": out["hd95"], "hd": out["hd"], "assd": out["assd"],
                "workspace_bytes": ws.numel(), "model_bytes": floor, "model_reread_bytes": reread,
                "model_floor_us": floor / COPY_PEAK_TBS / 1e6}
        if kind == "blocky":
            case["scipy_host_seconds_once"] = host_path(pred, label)
        cases.append(case)
        fns[f"{N}x{H}x{W} {kind}"] = {"SurfaceDistanceMeter.update": update, "cvk_surface_distances": entry, "BoundaryMeter.update": boundary,
                                     "ConfusionMeter.update": confusion, "cvk_edt_squared(label)": edt}
    for group in fns.values():
        for f in group.values():
            for _ in range(3):
                f()
    torch.cuda.synchronize()
    res = {}
    for _ in range(a.reps):
        for tag, group in fns.items():
            for name, f in group.items():
                res.setdefault((tag, name), []).append(timed(f, a.iters))
    for case, tag in zip(cases, fns):
        st = {name: stats(res[(tag, name)]) for name in fns[tag]}
        ratios = sorted(x / y for x, y in zip(res[(tag, "cvk_surface_distances")], res[(tag, "cvk_edt_squared(label)")]))
        case.update(times=st, entry_over_edt={"median": ratios[len(ratios) // 2], "min": ratios[0], "max": ratios[-1]},
                    entry_over_model_floor=st["cvk_surface_distances"]["median_us"] / case["model_floor_us"])
        print(f"{tag}: contour pixels {case['contour_pixels']}, largest d2 {case['largest_d2']}, hd95 {case['hd95']:.3f}, hd {case['hd']:.3f}, "
              f"assd {case['assd']:.3f}")
        for name, m in st.items():
            print(f"  {name:28s} {m['median_us']:9.1f} us (min {m['min_us']:.1f}, max {m['max_us']:.1f})")
        e = case["entry_over_edt"]
        print(f"  entry point / cvk_edt_squared {e['median']:.2f} (min {e['min']:.2f}, max {e['max']:.2f}, round by round); model floor "
              f"{case['model_floor_us']:.1f} us at {COPY_PEAK_TBS} TB/s, measured / floor {case['entry_over_model_floor']:.1f}"
              + (f"; scipy on the host, once: {case['scipy_host_seconds_once']:.2f} s" if "scipy_host_seconds_once" in case else ""))
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"classes": K, "ignore_index": IGNORE, "percentile": 95, "iters": a.iters, "reps": a.reps,
                       "copy_peak_tbs": COPY_PEAK_TBS, "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
