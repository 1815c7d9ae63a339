"""`python bench.py` without --full on the headline workload: it times the steps and prints the headline fields, nothing else runs
(no instrumented profile, no CPU baseline, no dp_overhead child, no extra legs); --dump-outputs writes the last timed step's outputs,
bitwise the same in two runs with the same arguments (no floating-point atomic anywhere)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_plain_run_and_dumped_outputs(tmp_path):
    dirs = [tmp_path / "a", tmp_path / "b"]
    recs = [_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(d)) for d in dirs]
    for d in recs:
        assert d["metric"] == "images/sec fwd+bwd UNet 3x360x480 bs=8" and d["unit"] == "images/s" and d["higher_is_better"] is True
        assert d["dtype"] == "f32" and d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
        assert abs(d["value"] - 8 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
        assert d["roofline"] is None and d["cpu_baseline"] is None and d["config"]["w2d_tile"]["logits_vs_reference"] is None
        for k in ("conv_kernels", "hbm_kernels", "extra_configs", "dp_overhead"):
            assert k not in d, k
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1])) and "loss.npy" in names and "logits.npy" in names
    assert sum(n.startswith("grad.") for n in names) == 92 and sum(n.startswith("bn.") for n in names) == 46
    total = 0
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 * 10 ** 6
    assert np.load(dirs[0] / "logits.npy").shape == (1 << 21,)              # 8 x 12 x 360 x 480 logits: the seeded sample
    assert abs(float(np.load(dirs[0] / "loss.npy")[0]) - recs[0]["config"]["loss"]) < 1e-6
