"""bench.py host logic (no GPU): a plain run is the default (--full off), and what --dump-outputs writes — the arrays a caller of the
timed step holds, float32, whole or a fixed seeded sample, under 64 MB for either network at its BASELINE.json size."""
import numpy as np
import pytest
import torch

import bench
import pytorch_camvid_amd as A


def test_plain_run_is_the_default():
    a = bench.parse(["--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_sample_is_whole_or_fixed():
    t = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    assert np.array_equal(bench.sample_output(t, 1000, "x"), t.numpy())                  # small enough: the array itself, its shape kept
    s1, s2 = bench.sample_output(t, 64, "x"), bench.sample_output(t.clone(), 64, "x")
    assert s1.shape == (64,) and s1.dtype == np.float32 and np.array_equal(s1, s2)      # the same positions every time
    assert len(np.unique(s1)) == 64 and np.all(np.diff(s1) > 0)                         # distinct, in flattened order
    assert not np.array_equal(s1, bench.sample_output(t, 64, "y"))                      # each array has its own positions
    # the logical (flattened) order, not the storage order: a channels-last tensor samples the same values
    cl = t.reshape(10, 100, 1, 1).contiguous(memory_format=torch.channels_last)
    assert np.array_equal(bench.sample_output(cl, 64, "x"), s1)


@pytest.mark.parametrize("model,batch,h,w", [("unet", 8, 360, 480), ("segnet", 8, 360, 480), ("unet", 4, 720, 960)])
def test_dump_fits_and_round_trips(tmp_path, model, batch, h, w):
    torch.manual_seed(0)
    net = A.get_model(model, 3, 12)
    for p in net.parameters():
        p.grad = torch.randn_like(p)
    logits = torch.randn(batch, 12, h, w)
    out = bench.capture_outputs(net, torch.tensor(2.5), logits)
    assert set(out) == ({"loss", "logits"} | {"grad." + n for n, _ in net.named_parameters()}
                        | {"bn." + n for n, b in net.named_buffers() if b.is_floating_point()})
    assert all(a.dtype == np.float32 for a in out.values()) and out["loss"].tolist() == [2.5]
    assert sum(a.nbytes for a in out.values()) <= bench.DUMP_MAX_BYTES
    for n, p in net.named_parameters():
        if p.numel() <= bench.DUMP_CAP_PARAM:
            assert np.array_equal(out["grad." + n], p.grad.numpy())
    bench.write_outputs(str(tmp_path), out)
    for name, a in out.items():
        b = np.load(tmp_path / (name + ".npy"))
        assert b.dtype == np.float32 and np.array_equal(a, b)
