#!/usr/bin/env python3
"""HIP-event timing of crop training on the device (cvk_crop_select + cvk_crop_augment_u8) at batch 8, 720 x 960 frames, crop
360 x 480, every stage on (9-tap blur, flip, LUT, eleven candidates), at ratios 0.5, 1.0, 2.0 and with the ratio drawn per sample;
interleaved legs in one process:
  (a) `cvk_augment_u8` at the same output size (960x720 -> 480x360, every stage on): the yardstick;
  (b) `cvk_crop_select` alone, on uniformly random labels and on blocky maps (long runs of one class, as real masks have);
  (c) `cvk_crop_augment_u8` alone (the selection table of an earlier call);
  (d) the pair;
  (e) the same geometry composed from torch operators per sample (F.interpolate, slicing, F.pad, flip) with the offsets given.
Prints us per call (median, min, max over the rounds) next to DESIGN.md's traffic model.
                usage (GPU box): python tools/bench_crop_augment.py [--iters 100] [--reps 7] [--json profiles/crop_augment_bench.json]"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorch_camvid_amd import transforms as T  # noqa: E402
from tools.bench_boundary import stats, timed  # noqa: E402

N, HS, WS, HC, WC = 8, 720, 960, 360, 480
AUGMENT_TBS = 2.0                 # cvk_augment_u8's rate with every stage on: what the model divides bytes by


def model_augment_bytes(recs):
    """the float NHWC-4 + int64 mask stores, plus the window's source footprint at 3 + 1 bytes per pixel"""
    b = N * HC * WC * (16 + 8)
    for r in recs:
        b += int(min(HC, int(r["Hr"])) * float(r["sy"]) * min(WC, int(r["Wr"])) * float(r["sx"])) * 4
    return b


def records(ratio):
    """eleven drawn candidates per sample at a forced (or, ratio=None, drawn) ratio; blur, flip and LUT forced on"""
    params = []
    for _ in range(N):
        r = random.uniform(0.5, 2.0) if ratio is None else ratio
        Hr, Wr = T.resized_hw(HS, WS, r)
        cands = [(random.randint(0, max(Hr - HC, 0)), random.randint(0, max(Wr - WC, 0))) for _ in range(11)]
        params.append({"r": r, "Hr": Hr, "Wr": Wr, "sy": HS / Hr, "sx": WS / Wr, "cands": cands, "flip": True, "blur": (9, 2.9),
                       "jitter": [("brightness", 1.3)]})
    return T.CropCompose.pack(params)


def torch_geometry(frames, masks, rec, sel):
    """resize, cut, pad, flip per sample with torch operators (no blur, LUT or normalisation: the geometry alone)"""
    xs, ms = [], []
    for n in range(N):
        Hr, Wr, oy, ox = int(rec[n]["Hr"]), int(rec[n]["Wr"]), int(sel[n][1]), int(sel[n][2])
        x = F.interpolate(frames[n].permute(2, 0, 1)[None].float(), size=(Hr, Wr), mode="bilinear", align_corners=False)
        m = F.interpolate(masks[n][None, None].float(), size=(Hr, Wr), mode="nearest")
        x, m = x[..., oy:oy + HC, ox:ox + WC], m[..., oy:oy + HC, ox:ox + WC]
        ph, pw = HC - x.shape[-2], WC - x.shape[-1]
        x, m = F.pad(x, (0, pw, 0, ph)), F.pad(m, (0, pw, 0, ph), value=11.0)
        xs.append(x.flip(-1)); ms.append(m.flip(-1).long())
    return torch.cat(xs), torch.cat(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds; median, min and max are reported")
    ap.add_argument("--json", default=None, help="also write the summary there")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_crop_augment.py needs the GPU: no timing is taken without one")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (N, HS, WS, 3), generator=g, dtype=torch.uint8).to(dev)
    masks = torch.randint(0, 12, (N, HS, WS), generator=g, dtype=torch.uint8).to(dev)
    coarse = torch.randint(0, 11, (N, HS // 40 + 1, WS // 60 + 1), generator=g, dtype=torch.uint8)
    blocky = coarse.repeat_interleave(40, dim=1).repeat_interleave(60, dim=2)[:, :HS, :WS].contiguous().to(dev)
    fixed = torch.from_numpy(T.Compose.pack([{"flip": True, "blur": (9, 2.9), "jitter": [("brightness", 1.3)]}] * N).view(np.uint8)).to(dev)
    random.seed(0)
    fns = {"cvk_augment_u8 960x720 -> 480x360 (yardstick)": lambda: T.augment_u8(frames, masks, fixed, (HC, WC))}
    cases = {}
    for ratio in (0.5, 1.0, 2.0, None):
        tag = "ratio drawn" if ratio is None else f"ratio {ratio}"
        rec = records(ratio)
        grec = torch.from_numpy(rec.view(np.uint8)).to(dev)
        counts = torch.empty((N, 11, 256), device=dev, dtype=torch.int32)
        sel = torch.empty((N, 4), device=dev, dtype=torch.int32)

        def select(m=masks, grec=grec, counts=counts, sel=sel):
            T.crop_select(m, grec, (HS, WS), (HC, WC), 11, 0.75, counts, sel)

        def select_blocky(grec=grec, counts=counts, sel=sel):
            T.crop_select(blocky, grec, (HS, WS), (HC, WC), 11, 0.75, counts, sel)

        def augment(grec=grec, sel=sel):
            T.crop_augment_u8(frames, masks, grec, sel, (HC, WC))

        def pair(grec=grec, counts=counts, sel=sel):
            T.crop_select(masks, grec, (HS, WS), (HC, WC), 11, 0.75, counts, sel)
            T.crop_augment_u8(frames, masks, grec, sel, (HC, WC))

        select_blocky()
        sel_blocky = sel.cpu().numpy().copy()
        select()
        sel_host = sel.cpu().numpy().copy()             # outside the timed region: the torch leg is given the offsets

        def composed(rec=rec, sel_host=sel_host):
            torch_geometry(frames, masks, rec, sel_host)

        fns.update({f"{tag}: cvk_crop_select": select, f"{tag}: cvk_crop_select, blocky masks": select_blocky,
                    f"{tag}: cvk_crop_augment_u8": augment, f"{tag}: the pair": pair, f"{tag}: torch operators, geometry only": composed})
        cases[tag] = {"resized": [[int(r["Hr"]), int(r["Wr"])] for r in rec], "chosen_candidate": sel_host[:, 0].tolist(),
                      "chosen_candidate_blocky": sel_blocky[:, 0].tolist(), "model_augment_bytes": model_augment_bytes(rec),
                      "model_augment_us": model_augment_bytes(rec) / AUGMENT_TBS / 1e6, "gathers": 11 * N * HC * WC}
    for f in fns.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    res = {}
    for _ in range(a.reps):
        for name, f in fns.items():
            res.setdefault(name, []).append(timed(f, a.iters if "torch operators" not in name else max(a.iters // 10, 1)))
    st = {name: stats(v) for name, v in res.items()}
    for name, m in st.items():
        print(f"  {name:52s} {m['median_us']:9.1f} us (min {m['min_us']:.1f}, max {m['max_us']:.1f})")
    for tag, c in cases.items():
        print(f"  {tag}: model of the augment launch {c['model_augment_bytes'] / 1e6:.1f} MB, {c['model_augment_us']:.1f} us at {AUGMENT_TBS} TB/s; "
              f"chosen candidates {c['chosen_candidate']} (blocky masks {c['chosen_candidate_blocky']})")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"batch": N, "source": [HS, WS], "crop": [HC, WC], "iters": a.iters, "reps": a.reps, "model_rate_tbs": AUGMENT_TBS,
                       "cases": cases, "times": st}, f, indent=1)


if __name__ == "__main__":
    main()
