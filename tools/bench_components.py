#!/usr/bin/env python3
"""HIP-event timing of connected components and small-region removal (cvk_cc_label, cvk_cc_filter) at 8 x 360 x 480 and 8 x 720 x 960, in
one process and in interleaved rounds, on three kinds of map:
  blocky    a coarse random 12-class grid enlarged by 7 x 9 cells, 3 % of the pixels redrawn (tests/boundary_ref.py);
  speckled  24 x 32 cells with 2 % single-pixel and two-pixel specks of other classes: what an arg-max map looks like;
  random    two classes at p = 0.5: percolation-like components, the adversarial case for the unions.
Timed: `connected_components`, `remove_small_regions` in both modes (min_area 64), `RegionMeter.update`; yardsticks on the same tensors:
`ConfusionMeter.update` (one read of 16 B per pixel), `cvk_cheb_depth` of the map, and scipy's `label` per image and code on one host
core, timed once.  Prints us per call (median, min, max over the rounds) next to the traffic model of DESIGN.md.
                    usage (GPU box): python tools/bench_components.py [--iters 50] [--reps 7] [--json profiles/components_bench.json]"""
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
from tests import components_ref as R  # noqa: E402
from tests.boundary_ref import blocky_maps  # noqa: E402
from tools.bench_boundary import stats, timed  # noqa: E402

K, IGNORE = 12, 11
COPY_PEAK_TBS = 6.29
MIN_AREA = 64
# DESIGN.md's traffic model, bytes per pixel
MODEL_BYTES = {"connected_components": 41.5, "remove_small_regions, neighbor": 83.5, "remove_small_regions, fill": 78.5,
               "RegionMeter.update": 178.0}


def host_label(m, k, ignore):
    """scipy's label per image and code with the 4-structure, as public code does it.  Returns seconds."""
    from scipy import ndimage
    c = R.codes(m, k, ignore)
    t0 = time.perf_counter()
    for n in range(c.shape[0]):
        for code in np.unique(c[n]):
            ndimage.label(c[n] == code)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds; median, min and max are reported")
    ap.add_argument("--json", default=None, help="also write the summary there")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_components.py needs the GPU: no timing is taken without one")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    lib, check = _lib.load(), _lib.check
    s = torch.cuda.current_stream().cuda_stream
    cases, fns = [], {}
    for N, H, W in ((8, 360, 480), (8, 720, 960)):
        pred_b, label_b = blocky_maps(H, N, H, W, K, IGNORE)
        kinds = {"blocky": (pred_b, label_b, K, IGNORE),
                 "speckled": (R.speckled(H, N, H, W, K, IGNORE), R.speckled(H, N, H, W, K, IGNORE, speck=0.0), K, IGNORE),
                 "random": (R.random_two_class(H, N, H, W, 0.5), R.random_two_class(H + 1, N, H, W, 0.5), 2, -100)}
        for kind, (p_np, l_np, k, ig) in kinds.items():
            pred, label = torch.from_numpy(p_np).to(dev), torch.from_numpy(l_np).to(dev)
            meter, cm = A.RegionMeter(k, ig, min_area=MIN_AREA), A.ConfusionMeter(k, ig, dev)
            ws = torch.empty(lib.cvk_cheb_workspace_bytes(N, H, W), device=dev, dtype=torch.uint8)
            maps = torch.empty((2, N, H, W), device=dev, dtype=torch.uint8)
            rf_n, rf_f = A.RegionFilter(MIN_AREA, k, ig), A.RegionFilter(MIN_AREA, k, ig, mode="fill")

            def label_fn(pred=pred, k=k, ig=ig):
                A.connected_components(pred, k, ig)

            def neighbor(rf=rf_n, pred=pred):
                rf(pred)

            def fill(rf=rf_f, pred=pred):
                rf(pred)

            def update(m=meter, pred=pred, label=label):
                m.reset()
                m.update(pred, label)

            def confusion(cm=cm, pred=pred, label=label):
                cm.update(pred, label)

            def depth(pred=pred, ws=ws, maps=maps, N=N, H=H, W=W, k=k, ig=ig):
                check(lib.cvk_cheb_depth(pred.data_ptr(), None, maps[0].data_ptr(), maps[1].data_ptr(), ws.data_ptr(), N, H, W, k, ig, 12, 0, s),
                      "cvk_cheb_depth")

            update()
            sc = meter.compute()
            neighbor()
            rec = rf_n.last_record.sum(0).cpu().numpy()
            tag = f"{N}x{H}x{W} {kind}"
            cases.append({"shape": [N, H, W], "map": kind, "classes": k, "min_area": MIN_AREA, "components": int(rec[:, 0].sum()),
                          "small_components": int(rec[:, 3].sum()), "small_pixels": int(rec[:, 4].sum()), "largest": int(rec[:, 2].max()),
                          "isolated": int(rec[:, 7].sum()), "fragmentation": sc["fragmentation"], "miou_filtered": sc["miou_filtered"],
                          "workspace_bytes": int(lib.cvk_cc_workspace_bytes(N, H, W, k)),
                          "model_floor_us": {n: b * N * H * W / COPY_PEAK_TBS / 1e6 for n, b in MODEL_BYTES.items()},
                          "scipy_label_host_seconds_once": host_label(p_np, k, ig)})
            fns[tag] = {"connected_components": label_fn, "remove_small_regions, neighbor": neighbor, "remove_small_regions, fill": fill,
                        "RegionMeter.update": update, "ConfusionMeter.update": confusion, "cvk_cheb_depth": depth}
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
        case.update(times=st, over_model_floor={n: st[n]["median_us"] / case["model_floor_us"][n] for n in MODEL_BYTES},
                    over_confusion={n: st[n]["median_us"] / st["ConfusionMeter.update"]["median_us"] for n in MODEL_BYTES})
        print(f"{tag}: {case['components']} class components, {case['small_components']} below {MIN_AREA} px ({case['small_pixels']} px, "
              f"{case['isolated']} isolated), largest {case['largest']}; fragmentation {case['fragmentation']:.2f}, "
              f"filtered mIoU {case['miou_filtered']:.4f}; scipy label on the host, once: {case['scipy_label_host_seconds_once']:.2f} s")
        for name, m in st.items():
            extra = ""
            if name in MODEL_BYTES:
                extra = f"  model {case['model_floor_us'][name]:.1f} us, x{case['over_model_floor'][name]:.1f}; x{case['over_confusion'][name]:.2f} of ConfusionMeter.update"
            print(f"  {name:34s} {m['median_us']:9.1f} us (min {m['min_us']:.1f}, max {m['max_us']:.1f}){extra}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"iters": a.iters, "reps": a.reps, "copy_peak_tbs": COPY_PEAK_TBS, "min_area": MIN_AREA, "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
