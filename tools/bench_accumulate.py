#!/usr/bin/env python3
"""HIP-event timing of gradient accumulation (GradAccumulator, cvk_grad_accumulate) at the headline shape (UNet, 8 x 3 x 360 x 480, fp32;
34.5 M gradient floats = 138.1 MB per flat buffer):
  (a) the three kernel modes over the UNet's whole segment table: microseconds and bytes per second (mode 0 moves 8 B per element, modes 1
      and 2 move 12 B).  The timing loop alternates between two buffer pairs (552 MB), so nothing is served from the 256 MiB Infinity Cache;
  (b) a window of K = 4 micro-batches: four plain forward + backward passes with zero_grad in between (no accumulator: what a step costs
      today), the same four through the accumulator, and the autograd idiom ((loss / K).backward() four times without zero_grad);
  (c) with --dp: (b) under ddp.DataParallel on a world-1 RCCL group (always_issue) in a child process, with the collectives per window.
Legs alternate --reps times; medians and min / max; one JSON line at the end (--out also writes it to a file).
                                            usage (GPU box): python tools/bench_accumulate.py [--iters 50] [--reps 5] [--windows 5] [--dp]"""
import argparse
import json
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_camvid_amd as A  # noqa: E402
from pytorch_camvid_amd import accumulate, engine, optim  # noqa: E402

K = 4


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def median_of(legs, reps, iters, warm=2):
    for fn in legs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            res[k].append(timed(fn, iters))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in res.items()}


def kernel_legs(dev):
    net = A.UNet(3, 12)
    params = optim._block_params(net)
    offs, total = engine.layout_grads(params)
    segs = accumulate.norm_segments((o, p.numel()) for o, p in zip(offs, params))
    tab = accumulate._Table(segs, total, dev)
    pairs = [(torch.randn(total, device=dev), torch.randn(total, device=dev)) for _ in range(2)]
    lib, stream, turn = A.load_library(), torch.cuda.current_stream().cuda_stream, [0]

    def leg(mode):
        def fn():
            d, s = pairs[turn[0] & 1]
            turn[0] += 1
            accumulate.check(lib.cvk_grad_accumulate(d.data_ptr(), s.data_ptr(), total, tab.table.data_ptr(), tab.nseg, tab.blocks, mode, 0.25,
                                                     stream), "cvk_grad_accumulate")
        return fn
    return {f"mode{m}_us": leg(m) for m in range(3)}, sum(n for _, n in segs), len(segs), tab.blocks


def window_legs(dev, batch, wrap=None):
    """{leg: one window of K micro-batches}; every leg has its own network (same seed)."""
    lossf = A.CrossEntropyLoss()
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(batch, 3, 360, 480, generator=g).to(dev) for _ in range(K)]
    ts = [torch.randint(0, 12, (batch, 360, 480), generator=g).to(dev) for _ in range(K)]

    def make():
        torch.manual_seed(0)
        net = A.UNet(3, 12).to(dev).train()
        return net, (wrap(net) if wrap is not None else net)
    (n_plain, f_plain), (n_acc, f_acc), (n_auto, f_auto) = make(), make(), make()
    acc = A.GradAccumulator(f_acc, steps=K)

    def zero(net):
        for p in net.parameters():
            p.grad = None

    def plain():
        for x, t in zip(xs, ts):
            zero(n_plain)
            lossf(f_plain(x), t).backward()

    def accumulated():
        for x, t in zip(xs, ts):
            lossf(f_acc(x), t).backward()
        assert acc.ready
        zero(n_acc)

    def autograd():
        for x, t in zip(xs, ts):
            (lossf(f_auto(x), t) / K).backward()
        zero(n_auto)
    return {"plain_4_passes_ms": plain, "accumulator_window_ms": accumulated, "autograd_idiom_ms": autograd}, (f_plain, f_acc, f_auto)


def _dp_child(rank, port, batch, reps, windows, out_path):
    from pytorch_camvid_amd import ddp
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ddp.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    legs, wrapped = window_legs(dev, batch, wrap=lambda net: ddp.DataParallel(net, always_issue=True))
    counts = {}
    for (name, fn), w in zip(legs.items(), wrapped):
        issued = []
        real = w.sync._issue
        w.sync._issue = lambda call, t, issued=issued, real=real: issued.append(1) or real(call, t)
        fn()
        counts[name.replace("_ms", "_collectives")] = len(issued)
    res = median_of(legs, reps, windows, warm=1)
    out = dict(counts)
    for k, (med, lo, hi) in res.items():
        out[k] = round(med / 1e3, 3)
        out[k + "_min_max"] = [round(lo / 1e3, 3), round(hi / 1e3, 3)]
    with open(out_path, "w") as f:
        json.dump(out, f)
    torch.distributed.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="kernel launches per timed repetition")
    ap.add_argument("--reps", type=int, default=5, help="interleaved repetitions; the median is reported")
    ap.add_argument("--windows", type=int, default=5, help="windows per timed repetition")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--dp", action="store_true", help="also the window legs under ddp.DataParallel on a world-1 RCCL group (child process)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    legs, floats, nseg, blocks = kernel_legs(dev)
    out = {"shape": [a.batch, 3, 360, 480], "K": K, "grad_floats": floats, "segments": nseg, "workgroups": blocks, "iters": a.iters,
           "reps": a.reps, "windows": a.windows, "kernel_working_set_bytes": 16 * floats}
    for k, (med, lo, hi) in median_of(legs, a.reps, a.iters, warm=5).items():
        bpe = 8 if k.startswith("mode0") else 12
        out[k] = round(med, 2)
        out[k + "_min_max"] = [round(lo, 2), round(hi, 2)]
        out[k.replace("_us", "_TBps")] = round(bpe * floats / (med * 1e-6) / 1e12, 3)
    del legs
    torch.cuda.empty_cache()
    wl, _ = window_legs(dev, a.batch)
    for k, (med, lo, hi) in median_of(wl, a.reps, a.windows, warm=2).items():
        out[k] = round(med / 1e3, 3)
        out[k + "_min_max"] = [round(lo / 1e3, 3), round(hi / 1e3, 3)]
    out["accumulator_minus_plain_ms"] = round(out["accumulator_window_ms"] - out["plain_4_passes_ms"], 3)
    out["autograd_minus_accumulator_ms"] = round(out["autograd_idiom_ms"] - out["accumulator_window_ms"], 3)
    del wl
    torch.cuda.empty_cache()
    if a.dp:
        import tempfile
        import torch.multiprocessing as mp
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "dp.json")
            mp.spawn(_dp_child, args=(port, a.batch, a.reps, a.windows, path), nprocs=1, join=True)
            out["dp_world1"] = json.load(open(path))
    for m in range(3):
        print(f"(a) mode {m}: {out[f'mode{m}_us']:8.1f} us   {out[f'mode{m}_TBps']:.2f} TB/s")
    print(f"(b) window of {K}: plain passes {out['plain_4_passes_ms']:.3f} ms, accumulator {out['accumulator_window_ms']:.3f} ms, "
          f"autograd idiom {out['autograd_idiom_ms']:.3f} ms")
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
