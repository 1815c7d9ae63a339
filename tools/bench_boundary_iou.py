#!/usr/bin/env python3
"""HIP-event timing of the Boundary IoU / trimap meter (cvk_cheb_depth twice + cvk_boundary_iou_counts) at 8 x 360 x 480 (dilation 12)
and 8 x 720 x 960 (dilation 24), in one process and in interleaved rounds, on the blocky maps of tests/boundary_ref.py (a coarse random
class grid enlarged by 7 x 9 cells; the prediction is the label shifted by (2, -2) with 3 % of its pixels redrawn; 5 % of the label
pixels are void):
  (a) `BoundaryIoUMeter.update` without and with five trimap widths (1, 2, 4, 8, 16), and its parts: one cvk_cheb_depth, the count
      launch alone;
  (b) yardsticks on the same tensors: `ConfusionMeter.update`, `BoundaryMeter.update`, `SurfaceDistanceMeter.update`, and
      `cvk_edt_squared` of the label map;
  (c) the host path of the public code, timed once on one core: per image and class scipy's binary_erosion of both masks with a zero
      pad, `dilation` iterations, then the band intersection and union.
Prints us per call (median, min, max over the rounds) and the traffic model's floor next to the measured time.
                    usage (GPU box): python tools/bench_boundary_iou.py [--iters 50] [--reps 7] [--json profiles/boundary_iou_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytorch_camvid_amd as A  # noqa: E402
from pytorch_camvid_amd import _lib  # noqa: E402
from tests.boundary_ref import blocky_maps  # noqa: E402
from tools.bench_boundary import stats, timed  # noqa: E402

K, IGNORE = 12, 11
COPY_PEAK_TBS = 6.29
TRIMAP = (1, 2, 4, 8, 16)
COL_TH = 64                       # csrc/boundary_iou.h: CHEB_COL_TH


def model_bytes(N, H, W, max_depth):
    """The traffic model of DESIGN.md: bytes per call if every byte moved once at the copy peak.  Per pixel: the row pass reads 8 B of
    the label and 16 B for the prediction (its own value and the label's void) and writes code + h for each; the column pass reads
    code + h with its halo rows and writes the depth, per map; the count pass reads the four byte maps."""
    halo = min(max_depth, H - 1)
    cols = 2 * (COL_TH + 2 * halo) / COL_TH + 1
    return int(N * H * W * ((8 + 2) + (16 + 2) + 2 * cols + 4))


def host_path(pred, label, d):
    """Cheng's recipe with scipy instead of cv2.erode, per image and class.  Returns seconds."""
    from scipy import ndimage
    p, g = pred.cpu().numpy(), label.cpu().numpy()
    k = np.ones((3, 3), dtype=bool)
    t0 = time.perf_counter()
    for n in range(p.shape[0]):
        void = g[n] == IGNORE
        for c in range(K):
            if c == IGNORE:
                continue
            mp, mg = (p[n] == c) & ~void, g[n] == c
            bp = mp & ~ndimage.binary_erosion(mp, k, iterations=d, border_value=0)
            bg = mg & ~ndimage.binary_erosion(mg, k, iterations=d, border_value=0)
            (bp & bg).sum(), (bp | bg).sum()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds; median, min and max are reported")
    ap.add_argument("--json", default=None, help="also write the summary there")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_boundary_iou.py needs the GPU: no timing is taken without one")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    lib, check = _lib.load(), _lib.check
    s = torch.cuda.current_stream().cuda_stream
    cases, fns = [], {}
    for N, H, W in ((8, 360, 480), (8, 720, 960)):
        pred, label = (torch.from_numpy(m).to(dev) for m in blocky_maps(H, N, H, W, K, IGNORE))
        d = A.boundary_dilation(H, W)
        plain, tri = A.BoundaryIoUMeter(K, IGNORE), A.BoundaryIoUMeter(K, IGNORE, trimap_widths=TRIMAP)
        cm, bm, sm = A.ConfusionMeter(K, IGNORE, dev), A.BoundaryMeter(K, IGNORE), A.SurfaceDistanceMeter(K, IGNORE)
        ws = torch.empty(lib.cvk_cheb_workspace_bytes(N, H, W), device=dev, dtype=torch.uint8)
        maps = torch.empty((4, N, H, W), device=dev, dtype=torch.uint8)
        cnt = torch.zeros((N, 6, K), device=dev, dtype=torch.int64)
        ews = torch.empty(lib.cvk_edt_workspace_bytes(N, H, W, K), device=dev, dtype=torch.uint8)
        to_class = torch.empty((N, H, W, K), device=dev, dtype=torch.int32)
        to_other = torch.empty((N, H, W), device=dev, dtype=torch.int32)

        def update(m=plain, pred=pred, label=label):
            m.reset()
            m.update(pred, label)

        def update_tri(m=tri, pred=pred, label=label):
            m.reset()
            m.update(pred, label)

        def depth(label=label, ws=ws, maps=maps, N=N, H=H, W=W, d=d):
            check(lib.cvk_cheb_depth(label.data_ptr(), None, maps[2].data_ptr(), maps[3].data_ptr(), ws.data_ptr(), N, H, W, K, IGNORE, d, 0,
                                     s), "cvk_cheb_depth")

        def count(maps=maps, cnt=cnt, N=N, H=H, W=W, d=d):
            check(lib.cvk_boundary_iou_counts(maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(), maps[3].data_ptr(), cnt.data_ptr(),
                                              None, None, 0, N, H, W, K, d, s), "cvk_boundary_iou_counts")

        def confusion(cm=cm, pred=pred, label=label):
            cm.update(pred, label)

        def boundary(bm=bm, pred=pred, label=label):
            bm.reset()
            bm.update(pred, label)

        def surface(sm=sm, pred=pred, label=label):
            sm.reset()
            sm.update(pred, label)

        def edt(label=label, ews=ews, to_class=to_class, to_other=to_other, N=N, H=H, W=W):
            check(lib.cvk_edt_squared(label.data_ptr(), N, H, W, K, IGNORE, ews.data_ptr(), to_class.data_ptr(), to_other.data_ptr(), s),
                  "cvk_edt_squared")

        check(lib.cvk_cheb_depth(pred.data_ptr(), label.data_ptr(), maps[0].data_ptr(), maps[1].data_ptr(), ws.data_ptr(), N, H, W, K, IGNORE,
                                 d, 0, s), "cvk_cheb_depth")
        depth()
        update_tri()
        out = tri.compute()
        c = tri.counts()
        case = {"shape": [N, H, W], "dilation": d, "trimap_widths": list(TRIMAP), "biou": out["biou"], "biou_image": out["biou_image"],
                "trimap_miou": [float(v) for v in out["trimap_miou"]], "band_pixels": [int(c[:, 0].sum()), int(c[:, 1].sum())],
                "mask_pixels": [int(c[:, 3].sum()), int(c[:, 4].sum())], "model_bytes": model_bytes(N, H, W, d),
                "model_bytes_trimap": model_bytes(N, H, W, max(d, TRIMAP[-1])),
                "scipy_host_seconds_once": host_path(pred, label, d)}
        case["model_floor_us"] = case["model_bytes"] / COPY_PEAK_TBS / 1e6
        case["model_floor_trimap_us"] = case["model_bytes_trimap"] / COPY_PEAK_TBS / 1e6
        cases.append(case)
        fns[f"{N}x{H}x{W}"] = {"BoundaryIoUMeter.update": update, "BoundaryIoUMeter.update, 5 trimap widths": update_tri,
                               "cvk_cheb_depth(label)": depth, "cvk_boundary_iou_counts": count, "ConfusionMeter.update": confusion,
                               "BoundaryMeter.update": boundary, "SurfaceDistanceMeter.update": surface, "cvk_edt_squared(label)": edt}
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
        case.update(times=st, update_over_model_floor=st["BoundaryIoUMeter.update"]["median_us"] / case["model_floor_us"],
                    update_trimap_over_model_floor=st["BoundaryIoUMeter.update, 5 trimap widths"]["median_us"] / case["model_floor_trimap_us"],
                    update_over_confusion=st["BoundaryIoUMeter.update"]["median_us"] / st["ConfusionMeter.update"]["median_us"])
        print(f"{tag}: dilation {case['dilation']}, band pixels {case['band_pixels']} of {case['mask_pixels']}, biou {case['biou']:.4f}, "
              f"trimap mIoU {['%.4f' % v for v in case['trimap_miou']]}")
        for name, m in st.items():
            print(f"  {name:42s} {m['median_us']:9.1f} us (min {m['min_us']:.1f}, max {m['max_us']:.1f})")
        print(f"  model floor {case['model_floor_us']:.1f} us ({case['model_floor_trimap_us']:.1f} us with the trimap widths) at {COPY_PEAK_TBS} "
              f"TB/s, measured / floor {case['update_over_model_floor']:.1f} ({case['update_trimap_over_model_floor']:.1f}); update / "
              f"ConfusionMeter.update {case['update_over_confusion']:.2f}; scipy on the host, once: {case['scipy_host_seconds_once']:.2f} s")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"classes": K, "ignore_index": IGNORE, "iters": a.iters, "reps": a.reps, "copy_peak_tbs": COPY_PEAK_TBS, "cases": cases},
                      f, indent=1)


if __name__ == "__main__":
    main()
