#!/usr/bin/env python3
"""HIP-event timing of the fused device transforms (cvk_augment_u8) at batch 8, 960x720 -> 480x360, every stage forced on
(9-tap blur, flip, LUT), plus the validation form (resize only).  Prints us per batch and the bytes the launch must move over
that time.                                  usage (GPU box): python tools/bench_augment.py [--iters 200] [--batch 8]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_camvid_amd import transforms as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, Hs, Ws, H, W = a.batch, 720, 960, 360, 480
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (N, Hs, Ws, 3), generator=g, dtype=torch.uint8).to(dev)
    masks = torch.randint(0, 12, (N, Hs, Ws), generator=g, dtype=torch.uint8).to(dev)
    forced = [{"flip": True, "blur": (9, 2.9), "jitter": [("brightness", 1.3)]}] * N
    plain = [{"flip": False, "blur": None, "jitter": None}] * N
    # bytes one launch must move: source frames + masks read once, float NHWC-4 + int64 masks written
    nbytes = N * (Hs * Ws * 3 + Hs * Ws + H * W * 16 + H * W * 8)
    for name, params in (("train, all stages on (k=9, flip, LUT)", forced), ("valid (resize only)", plain)):
        rec = torch.from_numpy(T.Compose.pack(params).view(np.uint8)).to(dev)
        for _ in range(10):
            T.augment_u8(frames, masks, rec, (H, W))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            T.augment_u8(frames, masks, rec, (H, W))
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / a.iters * 1e3
        print(f"{name}: {us:.1f} us per batch of {N} ({nbytes / 1e6:.1f} MB moved, {nbytes / us / 1e6:.2f} TB/s)")


if __name__ == "__main__":
    main()
