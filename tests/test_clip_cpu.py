"""Global-norm gradient clipping, the parts that need no GPU: the host clip-coefficient function against numpy fp32, argument validation of
the new entry points before any launch, the segment planner (no padding float and no frozen parameter inside a segment) and the option checks
of FlatAdamW / clip_grad_norm_."""
import ctypes
import math

import numpy as np
import pytest
import torch


def _lib():
    from pytorch_camvid_amd import _lib
    return _lib, _lib.load()


def test_host_clip_coef_is_torchs_expression_in_fp32():
    _, lib = _lib()
    rng = np.random.default_rng(0)
    norms = np.concatenate([np.float32([0.0, 1e-30, 1e-6, 0.5, 1.0, 3.0, 1e10, 3e38]), rng.lognormal(0, 6, 400).astype(np.float32)])
    maxes = np.concatenate([np.float32([0.0, 1e-3, 0.1, 1.0, 5.0, 1e30]), rng.lognormal(0, 4, 40).astype(np.float32)])
    for mx in maxes:
        for n in norms:
            with np.errstate(over="ignore"):
                want = np.float32(mx) / (np.float32(n) + np.float32(1e-6))
            want = np.float32(1.0) if want > 1 else np.float32(want)
            got = np.float32(lib.cvk_clip_coef(float(mx), float(n)))
            assert got.tobytes() == want.tobytes(), (mx, n, got, want)
    assert math.isnan(lib.cvk_clip_coef(3.0, float("nan")))          # torch.clamp(3 / (nan + 1e-6), max=1) is nan; fminf would give 1
    assert lib.cvk_clip_coef(3.0, float("inf")) == 0.0
    t = torch.clamp(torch.tensor(3.0) / (torch.tensor(float("nan")) + 1e-6), max=1.0)
    assert math.isnan(t.item()) and t.dtype == torch.float32


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    L, lib = _lib()
    inf = float("inf")

    def refused(rc, name):
        msg = lib.cvk_last_error_string().decode()
        assert rc == -1 and msg.startswith(name + ":"), (name, rc, msg)

    p = 4096                                                  # never dereferenced: every call is refused on the host
    refused(lib.cvk_grad_norm(None, 8, p, 1, 1, 2.0, 1.0, p, p, None), "cvk_grad_norm")
    refused(lib.cvk_grad_norm(p, 8, None, 1, 1, 2.0, 1.0, p, p, None), "cvk_grad_norm")
    refused(lib.cvk_grad_norm(p, 8, p, 1, 1, 2.0, 1.0, None, p, None), "cvk_grad_norm")
    refused(lib.cvk_grad_norm(p, 8, p, 1, 1, 2.0, 1.0, p, None, None), "cvk_grad_norm")
    refused(lib.cvk_grad_norm(p, 8, p, 0, 0, 2.0, 1.0, p, p, None), "cvk_grad_norm")            # empty table
    for nt in (1.0, 0.0, 3.0, -inf, float("nan")):
        refused(lib.cvk_grad_norm(p, 8, p, 1, 1, nt, 1.0, p, p, None), "cvk_grad_norm")
    for mx in (-1.0, -0.0 - 1e-30, float("nan")):
        refused(lib.cvk_grad_norm(p, 8, p, 1, 1, inf, mx, p, p, None), "cvk_grad_norm")
    refused(lib.cvk_grad_scale(None, 8, p, 1, 1, p, None), "cvk_grad_scale")
    refused(lib.cvk_grad_scale(p, 8, p, 1, 1, None, None), "cvk_grad_scale")
    refused(lib.cvk_grad_scale(p, 8, p, 0, 0, p, None), "cvk_grad_scale")
    # the clipped AdamW step and the 7-column log row: the folded entry points with a record.  A null record is no longer an error there
    # (it means coefficient 1 / 5-column rows); in its place, an average without a usable alpha is refused
    eager, captured = "cvk_adamw_step_ranges", "cvk_adamw_step_ranges_dev"
    refused(lib.cvk_adamw_step_ranges(p, p, p, p, p, 8, p, 1, 1, p, 1, p, 1.5, None), eager)                 # ema with alpha outside (0, 1]
    assert "alpha" in lib.cvk_last_error_string().decode()
    refused(lib.cvk_adamw_step_ranges(p, p, p, p, None, 8, p, 0, 0, p, 1, p, 0.0, None), eager)
    refused(lib.cvk_adamw_step_ranges(p, p, p, p, None, 8, p, 1, 1, p, L.ADAMW_ARG_RECORDS + 1, p, 0.0, None), eager)
    refused(lib.cvk_adamw_step_ranges_dev(p, p, p, p, p, 8, p, 1, 1, p, 1, p, None, 0.5, None), captured)    # ema with a null device alpha
    assert "null" in lib.cvk_last_error_string().decode()
    refused(lib.cvk_adamw_step_ranges_dev(p, None, p, p, None, 8, p, 1, 1, p, 1, p, None, 0.0, None), captured)
    refused(lib.cvk_adamw_step_ranges_dev(p, p, p, p, None, 8, p, 0, 0, p, 1, p, None, 0.0, None), captured)
    # without an average alpha is ignored, not checked: the alpha test comes before the table test in both entry points, and an
    # out-of-range alpha with an empty table is refused for the table
    refused(lib.cvk_adamw_step_ranges(p, p, p, p, None, 8, p, 0, 0, p, 1, p, 1.5, None), eager)
    assert "bad arguments" in lib.cvk_last_error_string().decode() and "alpha" not in lib.cvk_last_error_string().decode()
    refused(lib.cvk_adamw_step_ranges_dev(p, p, p, p, None, 8, p, 0, 0, p, 1, p, None, float("nan"), None), captured)
    assert "bad arguments" in lib.cvk_last_error_string().decode() and "alpha" not in lib.cvk_last_error_string().decode()
    refused(lib.cvk_adamw_step_ranges(p, p, p, p, p, 8, p, 0, 0, p, 1, p, 1.5, None), eager)               # ... and with one, for alpha
    assert "alpha" in lib.cvk_last_error_string().decode()
    refused(lib.cvk_step_log(p, p, p, 4, p, 4, p, p, 0, p, None), "cvk_step_log")
    refused(lib.cvk_step_log(p, p, p, 4, p, 4, p, None, 4, p, None), "cvk_step_log")
    # the planner: null, empty, segments outside [0, n)
    refused(lib.cvk_grad_norm_plan(None, 1, 8), "cvk_grad_norm_plan")
    one = (L.NormSegment * 1)(L.NormSegment(0, 8, 0, 0))
    refused(lib.cvk_grad_norm_plan(ctypes.addressof(one), 0, 8), "cvk_grad_norm_plan")
    for o, m in ((-1, 4), (0, 0), (4, 8), (8, 1), (0, 9), (2 ** 62, 2 ** 62)):
        bad = (L.NormSegment * 2)(L.NormSegment(0, 4, 0, 0), L.NormSegment(o, m, 0, 0))
        refused(lib.cvk_grad_norm_plan(ctypes.addressof(bad), 2, 8), "cvk_grad_norm_plan")
    assert lib.cvk_grad_norm_plan(ctypes.addressof(one), 1, 8) == 1 and one[0].block0 == 0


def _padding_floats(params, offs, total):
    real = np.zeros(total, bool)
    for p, o in zip(params, offs):
        real[o:o + p.numel()] = True
    return ~real


def test_segment_planner_skips_padding_and_frozen_parameters():
    """A 21-class head: numels 64*9*21 (weight), 21, 21, 21.  layout_grads pads each to a multiple of 4 floats; the AdamW range table merges
    across that padding, the norm table must not."""
    from pytorch_camvid_amd import engine, optim
    L, lib = _lib()
    blocks = [(3, 64), (64, 64), (64, 21)]                     # [w, b, gamma, beta] per conv block, execution order; the head is last
    params = []
    for ci, co in blocks:
        params += [torch.empty(co, ci, 3, 3), torch.empty(co), torch.empty(co), torch.empty(co)]
    offs, total = engine.layout_grads(params)
    pad = _padding_floats(params, offs, total)
    assert pad.sum() == 3 * 3 + 0 + 0                         # three 21-float vectors padded to 24; 64*9*21 is a multiple of 4

    def covered(segs):
        c = np.zeros(total, bool)
        for o, n in segs:
            assert not c[o:o + n].any()
            c[o:o + n] = True
        return c

    every = list(range(len(params)))
    segs = optim.norm_segments((offs[i], params[i].numel()) for i in every)
    c = covered(segs)
    assert not (c & pad).any() and (c | pad).all()
    # the head comes first in the buffer: weight and bias touch (12096 is a multiple of 4) and merge, 21 | pad | 21 | pad | 21 | pad do not;
    # the 64-channel blocks behind have no padding and merge into the last head vector's neighbour only after its padding
    head = [i for i in every if i >= 8]
    hs = optim.norm_segments((offs[i], params[i].numel()) for i in head)
    assert hs == [(0, 64 * 9 * 21 + 21), (offs[10], 21), (offs[11], 21)], hs
    assert len(segs) == 4 and segs[3] == (offs[4], sum(params[i].numel() for i in range(8)))
    # frozen first block (indices 0..3) and a frozen BatchNorm weight of the head: absent
    idx = [i for i in every if i >= 4 and i != 10]
    fs = optim.norm_segments((offs[i], params[i].numel()) for i in idx)
    c = covered(fs)
    for i in every:
        assert c[offs[i]:offs[i] + params[i].numel()].all() == (i in idx) and c[offs[i]:offs[i] + params[i].numel()].any() == (i in idx), i
    assert not (c & pad).any()
    # the C planner accepts the table and hands every segment at least one workgroup, in order
    arr = (L.NormSegment * len(segs))(*[L.NormSegment(o, n, 0, 0) for o, n in segs])
    nb = lib.cvk_grad_norm_plan(ctypes.addressof(arr), len(segs), total)
    b0 = [s.block0 for s in arr]
    assert nb >= len(segs) and b0[0] == 0 and all(b > a for a, b in zip(b0, b0[1:])) and b0[-1] < nb
    with pytest.raises(ValueError, match="overlapping"):
        optim.norm_segments([(0, 8), (4, 8)])
    # the full UNet: 138.1 MB in one segment with 12 classes, at most 2048 workgroups
    full = (L.NormSegment * 1)(L.NormSegment(0, 34533924, 0, 0))
    assert lib.cvk_grad_norm_plan(ctypes.addressof(full), 1, 34533924) == 2048


def test_option_checks_run_without_a_gpu():
    import pytorch_camvid_amd as A
    net = A.UNet(3, 12)
    with pytest.raises(ValueError, match="max_norm"):
        A.FlatAdamW(net, max_grad_norm=-1)
    with pytest.raises(ValueError, match="max_norm"):
        A.FlatAdamW(net, max_grad_norm=float("nan"))
    for nt in (1, 3.0, "fro", 0):
        with pytest.raises(ValueError, match="norm_type"):
            A.FlatAdamW(net, max_grad_norm=1.0, norm_type=nt)
    with pytest.raises(ValueError, match="norm_type"):
        A.FlatAdamW(net, norm_type=1.0)                       # checked even while clipping is off
    with pytest.raises(RuntimeError, match="GPU"):           # valid options: the next check is the device
        A.FlatAdamW(A.UNet(3, 12), max_grad_norm=1.0, norm_type=float("inf"))
    with pytest.raises(ValueError, match="max_norm"):
        A.clip_grad_norm_(net, -1.0)
    with pytest.raises(ValueError, match="norm_type"):
        A.clip_grad_norm_(net, 1.0, norm_type=1.0)
    # CPU gradients are not the executor's flat buffer: torch's own function serves them, with torch's return value
    ps = [torch.nn.Parameter(torch.ones(5)), torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2))]
    ps[0].grad, ps[1].grad = torch.full((5,), 2.0), torch.full((3,), -2.0)
    n = A.clip_grad_norm_(ps, 1.0)
    assert n.dim() == 0 and abs(n.item() - math.sqrt(32.0)) < 1e-6 and ps[2].grad is None
    assert torch.allclose(ps[0].grad, torch.full((5,), 2.0 / math.sqrt(32.0)), rtol=1e-5)


def test_abi_tables_agree():
    from tests import test_abi
    test_abi.test_library_builds_loads_and_exports_every_declared_symbol()
    test_abi.test_integration_doc_matches_the_header()
