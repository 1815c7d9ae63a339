#!/usr/bin/env python3
"""HIP-event timing of the local-window CRF refinement (cvk.LocalCRF, cvk_crf_step) at 8 x 12 x 360 x 480 and 8 x 12 x 720 x 960, in one
process and in interleaved rounds, for the default window (r, d) = (3, 1) (staged in LDS) and for (5, 2) (halo 10: read from global
memory).  Timed per shape and window:
  one iteration (a T = 1 call: softmax of the neighbours on load, arg-max on store), T = 5, and (T = 5 - T = 1) / 4, a middle iteration;
  the same refinement composed from torch operators on the same tensors (shifted slices; T = 5), with min / max;
  cvk_window_merge of one full-size window on the same shape: the one-pass yardstick (reads the logits, writes the map and the arg-max).
Logits are 3 x randn, the guide a blocky image (7 x 9 cells of random colour, +-6 levels of noise), as in tests/test_gpu_crf.py.
Prints us per call (median, min, max over the rounds) next to the traffic model of DESIGN.md.
                    usage (GPU box): python tools/bench_crf.py [--iters 20] [--reps 7] [--json profiles/crf_bench.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytorch_camvid_amd as A  # noqa: E402
from pytorch_camvid_amd import _lib  # noqa: E402
from pytorch_camvid_amd.functional import CAMVID_MEAN, CAMVID_STD  # noqa: E402
from tests import crf_ref as R  # noqa: E402
from tools.bench_boundary import stats, timed  # noqa: E402

C = 12
COPY_PEAK_TBS = 6.29


def model_bytes_per_pixel(r, d):
    """DESIGN.md's HBM model of one iteration: unary 4C + Q out 4C + (Q in 4C + guide 12) x the halo overhead of the tile"""
    th, tw, staged = A.crf_tile(C, r, d)
    h = r * d
    halo = (th + 2 * h) * (tw + 2 * h) / (th * tw) if staged else 1.0
    return 8 * C + (4 * C + 12) * halo, staged


def torch_crf(U, I, crf, T):
    """the refinement from torch operators: U [N,H,W,C], I [N,H,W,3] grey levels"""
    ga, gs = crf.ga.ravel().tolist(), crf.gs.ravel().tolist()
    N, H, W, _ = U.shape
    Q = torch.softmax(U, -1)
    for _ in range(T):
        Sa, Ss = torch.zeros_like(Q), torch.zeros_like(Q)
        na, ns = torch.zeros((N, H, W), device=U.device), torch.zeros((N, H, W), device=U.device)
        for tap, dy, dx in R.offsets(crf.radius, crf.dilation):
            v = R._views(H, W, dy, dx)
            if v is None:
                continue
            (py, px), (qy, qx) = v
            diff = I[:, py, px] - I[:, qy, qx]
            ka = ga[tap] * torch.exp(crf.cb * (diff * diff).sum(-1))
            qn = Q[:, qy, qx]
            Sa[:, py, px] += ka[..., None] * qn
            Ss[:, py, px] += gs[tap] * qn
            na[:, py, px] += ka
            ns[:, py, px] += gs[tap]
        m = crf.wa * Sa / na.clamp_min(1e-30)[..., None] + crf.ws * Ss / ns.clamp_min(1e-30)[..., None]
        Q = torch.softmax(U + m, -1)
    return Q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=1, help="calls of the torch composition per round (it takes 10^2 to 10^3 as long)")
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds; median, min and max are reported")
    ap.add_argument("--json", default=None, help="also write the summary there")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_crf.py needs the GPU: no timing is taken without one")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    lib, check = _lib.load(), _lib.check
    s = torch.cuda.current_stream().cuda_stream
    cases, fns, iters = [], {}, {}
    for N, H, W in ((8, 360, 480), (8, 720, 960)):
        frames = R.blocky_frames(N, H, W, H)
        x = torch.from_numpy(R.normalise(frames, CAMVID_MEAN, CAMVID_STD)).to(dev)
        logits = (3.0 * torch.randn((N, H, W, C), generator=torch.Generator().manual_seed(H))).to(dev).permute(0, 3, 1, 2)
        out, pred = torch.empty((N, H, W, C), device=dev), torch.empty((N, H, W), device=dev, dtype=torch.int64)
        for r, d in ((3, 1), (5, 2)):
            one, five = A.LocalCRF(1, r, d), A.LocalCRF(5, r, d)
            I = (x.permute(0, 2, 3, 1) * torch.from_numpy(five.guide_scale).to(dev) + torch.from_numpy(five.guide_offset).to(dev)).contiguous()
            U = logits.permute(0, 2, 3, 1)

            def t1(one=one, logits=logits, x=x):
                one.refine(logits, x)

            def t5(five=five, logits=logits, x=x):
                five.refine(logits, x)

            def composed(five=five, U=U, I=I):
                torch_crf(U, I, five, 5)

            def merge(logits=logits, out=out, pred=pred, N=N, H=H, W=W):
                check(lib.cvk_window_merge(logits.data_ptr(), C, out.data_ptr(), pred.data_ptr(), N, H, W, C, H, W, H, W, 0, 0, s),
                      "cvk_window_merge")

            fused = five.refine(logits, x)[0].permute(0, 2, 3, 1)
            ref = torch_crf(U, I, five, 5)
            bpp, staged = model_bytes_per_pixel(r, d)
            tag = f"{N}x{C}x{H}x{W} (r,d)=({r},{d})"
            cases.append({"shape": [N, C, H, W], "radius": r, "dilation": d, "staged": staged, "tile": list(A.crf_tile(C, r, d)[:2]),
                          "model_bytes_per_pixel_iteration": bpp, "model_floor_us_iteration": bpp * N * H * W / COPY_PEAK_TBS / 1e6,
                          "max_abs_diff_fused_vs_torch": float((fused - ref).abs().max()),
                          "argmax_changed_by_refinement": float((fused.argmax(-1) != U.argmax(-1)).float().mean())})
            fns[tag] = {"T = 1": t1, "T = 5": t5, "torch composition, T = 5": composed, "cvk_window_merge": merge}
            iters[tag] = {"T = 1": a.iters, "T = 5": a.iters, "torch composition, T = 5": a.torch_iters, "cvk_window_merge": a.iters}
            del ref
    for tag, group in fns.items():
        for name, f in group.items():
            for _ in range(1 if name.startswith("torch") else 3):
                f()
    torch.cuda.synchronize()
    res = {}
    for _ in range(a.reps):
        for tag, group in fns.items():
            for name, f in group.items():
                res.setdefault((tag, name), []).append(timed(f, iters[tag][name]))
    for case, tag in zip(cases, fns):
        st = {name: stats(res[(tag, name)]) for name in fns[tag]}
        mid = sorted((b - o) / 4.0 for o, b in zip(res[(tag, "T = 1")], res[(tag, "T = 5")]))
        st["middle iteration, (T5 - T1) / 4"] = stats(mid)
        floor = case["model_floor_us_iteration"]
        case.update(times=st, iteration_over_model_floor=st["middle iteration, (T5 - T1) / 4"]["median_us"] / floor,
                    t5_over_model_floor=st["T = 5"]["median_us"] / (5 * floor),
                    torch_min_over_fused_max=st["torch composition, T = 5"]["min_us"] / st["T = 5"]["max_us"],
                    torch_median_over_fused_median=st["torch composition, T = 5"]["median_us"] / st["T = 5"]["median_us"],
                    iteration_over_window_merge=st["middle iteration, (T5 - T1) / 4"]["median_us"] / st["cvk_window_merge"]["median_us"])
        print(f"{tag}: {'staged in LDS' if case['staged'] else 'read from global memory'}, model {case['model_bytes_per_pixel_iteration']:.1f} B per "
              f"pixel and iteration = {floor:.1f} us; fused vs torch max |diff| {case['max_abs_diff_fused_vs_torch']:.1e}; the refinement "
              f"changes {100 * case['argmax_changed_by_refinement']:.1f} % of the arg-maxes")
        for name, m in st.items():
            print(f"  {name:34s} {m['median_us']:11.1f} us (min {m['min_us']:.1f}, max {m['max_us']:.1f})")
        print(f"  an iteration takes x{case['iteration_over_model_floor']:.2f} its model and x{case['iteration_over_window_merge']:.2f} a "
              f"cvk_window_merge; torch's fastest run / the fused slowest run = x{case['torch_min_over_fused_max']:.0f}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"iters": a.iters, "torch_iters": a.torch_iters, "reps": a.reps, "copy_peak_tbs": COPY_PEAK_TBS, "cases": cases}, f,
                      indent=1)


if __name__ == "__main__":
    main()
