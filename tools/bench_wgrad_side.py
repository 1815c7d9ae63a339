#!/usr/bin/env python3
"""Probe for the side stream (csrc/side.cpp): one weight-grad of block L beside the bandwidth-bound passes of block L-1, at two pairs of the
headline step, per weight-grad family:
  plane GEMM   up4.1 (64 -> 64) at 8 x 360 x 480: cvk_wgradp_gemm_sm_dy_wg (+ its reduce)  |  up4.0's passes at 64 channels: cvk_bn_bwd_reduce,
               cvk_colsum_finalize, cvk_wgradp_zero_pads4, cvk_bn_bwd_dx_e4p
  2-D GEMM     down3.1 (256 -> 256) at 8 x 90 x 120: cvk_w6_gemm_tn_wg + cvk_w6_wgrad_output |  down3.0's passes at 256 channels: cvk_bn_bwd_reduce,
               cvk_colsum_finalize, cvk_bn_bwd_dx, cvk_w6_dy_transform_both
Timed three ways (device events on the main stream, L2 / Infinity Cache flushed before every repetition, median of --reps): serial on one stream;
the GEMM forked onto the side stream with its grid capped to leave 0 / 32 / 64 / 96 CUs, joined behind the passes; each half alone (the GEMM at
that cap; the passes cannot be capped, so they have one figure).  Writes the table to --out."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_camvid_amd import _lib
from pytorch_camvid_amd._lib import View, check

FREE = (0, 32, 64, 96)
_flush = None


def timed(fn, reps):
    global _flush
    if _flush is None:
        _flush = torch.empty(1 << 28, device="cuda")
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        _flush.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def rnd(*shape):
    return torch.randn(*shape, device="cuda")


class Passes:
    """The BatchNorm-backward passes of a block with C output channels at N x H x W (training-mode statistics), as ConvBnRelu.bwd issues them."""

    def __init__(self, lib, N, H, W, C, plane):
        self.lib, self.dims, self.plane = lib, (N, H, W, C), plane
        M = N * H * W
        self.dout, self.y = rnd(N, H, W, C), rnd(M, C)
        self.view = View(self.dout.data_ptr(), H * W * C, W * C, C)
        self.vec = [rnd(C) for _ in range(6)]       # scale, shift, mean, rstd, dgamma, dbeta
        self.PB = lib.cvk_bn_bwd_blocks(M)
        self.part = torch.zeros(2 * max(self.PB, lib.cvk_bn_bwd_e_blocks(N, H, W)) * C, device="cuda")
        self.dy = torch.zeros(M * C + lib.cvk_wgradp_dy_slack(W) * C, device="cuda")
        if plane:
            self.E = torch.zeros(4 * lib.cvk_wgradp_plane_rows(N, H, W) * C, device="cuda")
        else:
            T = lib.cvk_w6_tiles(N, H, W)
            n = 64 * lib.cvk_w2d_tpad(T) * C + 128
            self.E, self.Vp = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")

    def __call__(self, s):
        lib, (N, H, W, C) = self.lib, self.dims
        sc, sh, mean, rstd, dg, db = (v.data_ptr() for v in self.vec)
        head = (self.view, self.y.data_ptr(), C, sc, sh, mean, rstd)
        check(lib.cvk_bn_bwd_reduce(*head, self.part.data_ptr(), N, H, W, C, s), "reduce")
        check(lib.cvk_colsum_finalize(self.part.data_ptr(), self.PB, C, db, dg, s), "colsum")
        if self.plane:
            check(lib.cvk_wgradp_zero_pads4(self.E.data_ptr(), N, H, W, C, s), "zero_pads4")
            check(lib.cvk_bn_bwd_dx_e4p(*head, dg, db, self.dy.data_ptr(), C, self.E.data_ptr(), self.part.data_ptr(), N, H, W, C, 1, s), "dx+E4p")
        else:
            check(lib.cvk_bn_bwd_dx(*head, dg, db, self.dy.data_ptr(), C, self.part.data_ptr(), N, H, W, C, 1, s), "dx")
            check(lib.cvk_w6_dy_transform_both(self.dy.data_ptr(), C, self.Vp.data_ptr(), self.E.data_ptr(), N, H, W, C, s), "dy_both")


class PlaneWgrad:
    def __init__(self, lib, N, H, W, ci, co):
        self.lib, self.a = lib, (N, H, W, ci, ci, co)
        rows = lib.cvk_wgradp_plane_rows(N, H, W)
        M = N * H * W
        self.dy = torch.zeros(M * co + lib.cvk_wgradp_dy_slack(W) * co, device="cuda")
        self.dy[:M * co] = rnd(M * co)
        self.E4, self.V = rnd(4 * rows * co), rnd(6 * rows * ci)
        self.wsb = lib.cvk_wgradp_gemm_workspace_bytes(N, H, W, ci, co)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device="cuda")
        self.dw = torch.empty(co * 9 * ci, device="cuda")
        self.per_cu = 8         # one-wave workgroups, two per SIMD

    def __call__(self, s, cap):
        check(self.lib.cvk_wgradp_gemm_sm_dy_wg(self.E4.data_ptr(), self.dy.data_ptr(), self.V.data_ptr(), self.dw.data_ptr(), *self.a,
                                                self.ws.data_ptr(), self.wsb, cap, s), "gemm_sm_dy_wg")


class W6Wgrad:
    def __init__(self, lib, N, H, W, ci, co):
        self.lib = lib
        self.T = T = lib.cvk_w6_tiles(N, H, W)
        Tp = lib.cvk_w2d_tpad(T)
        self.a = (T, ci, co)
        self.E, self.V = rnd(64 * Tp * co + 128), rnd(64 * Tp * ci + 128)
        self.P = torch.empty(lib.cvk_w6_wgrad_ksplit(T, ci, co) * 64 * co * ci, device="cuda")
        self.dw = torch.empty(co * 9 * ci, device="cuda")
        self.ci = ci
        self.per_cu = 2         # 256 threads, 64 KiB of LDS

    def __call__(self, s, cap):
        T, ci, co = self.a
        check(self.lib.cvk_w6_gemm_tn_wg(self.E.data_ptr(), self.V.data_ptr(), self.P.data_ptr(), T, ci, co, cap, s), "gemm_tn_wg")
        check(self.lib.cvk_w6_wgrad_output(self.P.data_ptr(), self.dw.data_ptr(), T, ci, ci, co, s), "wgrad_output")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r07_wgrad_side_probe.txt"))
    a = ap.parse_args()
    lib = _lib.load()
    main_s = torch.cuda.current_stream().cuda_stream
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = ["pair {weight-grad of block L | passes of block L-1}, us, median of %d cold repetitions; %d CUs" % (a.reps, cus),
             "%-34s %8s %8s | %-5s %9s %11s %9s" % ("pair", "serial", "passes", "free", "gemm", "overlapped", "vs serial")]
    pairs = [("plane GEMM up4.1 | up4.0 8x360x480", PlaneWgrad(lib, 8, 360, 480, 64, 64), Passes(lib, 8, 360, 480, 64, True)),
             ("2-D GEMM down3.1 | down3.0 8x90x120", W6Wgrad(lib, 8, 90, 120, 256, 256), Passes(lib, 8, 90, 120, 256, False))]
    for name, wg, ps in pairs:
        serial = timed(lambda: (wg(main_s, 0), ps(main_s)), a.reps)
        alone = timed(lambda: ps(main_s), a.reps)
        for free in FREE:
            cap = (cus - free) * wg.per_cu if free else 0

            def overlapped():
                s = lib.cvk_side_begin(main_s)
                assert s
                wg(s, cap)
                ps(main_s)
                check(lib.cvk_side_join(main_s), "join")
            g = timed(lambda: wg(main_s, cap), a.reps)
            o = timed(overlapped, a.reps)
            lines.append("%-34s %8.1f %8.1f | %-5d %9.1f %11.1f %+9.1f" % (name, serial, alone, free, g, o, o - serial))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
