"""OHEM cross-entropy without a GPU: the fp64 restatement (tests/ohem_ref.py) against an independent composition
(F.cross_entropy(reduction='none') + torch.topk + masked mean) on hand-built cases, the constructor's refusals, the loss threshold,
and the raw entry points' sizes and argument errors."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ohem_ref as R


def _compose(x, t, thresh, min_kept, w=None, ignore_index=-100):
    """(loss, kept) from torch ops only, fp64."""
    x = x.double()
    lmap = F.cross_entropy(x, t, reduction="none", ignore_index=ignore_index)
    valid = t != ignore_index
    V = int(valid.sum())
    if V == 0:
        return torch.tensor(float("nan"), dtype=torch.float64), torch.zeros_like(valid)
    lam = float(np.float32(-np.log(np.float64(thresh))))
    L = torch.topk(lmap[valid], min(min_kept, V)).values[-1]
    kept = valid & ((lmap > lam) | (lmap >= L))
    wt = torch.ones(x.shape[1], dtype=torch.float64) if w is None else w.double()
    wk = wt[t.clamp(0)] * kept
    return (wk * lmap).sum() / wk.sum(), kept


def _pixels(margins, C=4):
    """[1, C, 1, n] logits whose target (class 0) leads the other classes by margins[i], so the losses are ordered by the margins."""
    n = len(margins)
    x = torch.zeros(1, C, 1, n, dtype=torch.float64)
    x[0, 0, 0] = torch.tensor(margins, dtype=torch.float64)
    return x, torch.zeros(1, 1, n, dtype=torch.int64)


def _agree(x, t, thresh, min_kept, w=None, ignore_index=-100):
    loss, kept, L, V, l = R.ohem(x, t, thresh, min_kept, w, ignore_index)
    want, kept_c = _compose(x, t, thresh, min_kept, w, ignore_index)
    assert torch.equal(kept, kept_c)
    assert torch.allclose(loss, want, rtol=1e-12, atol=0, equal_nan=True), (loss, want)
    return loss, kept, L, V, l


def test_threshold_branch_keeps_every_pixel_harder_than_thresh():
    x, t = _pixels([-3.0, -2.0, -1.0, 0.0, 4.0, 5.0, 6.0, 7.0])
    # p_t < 0.7 for the first four (margin 0: p = 1/4), > 0.9 for the rest; min_kept = 2 asks for fewer than the threshold gives
    loss, kept, L, V, l = _agree(x, t, 0.7, 2)
    assert kept[0, 0].tolist() == [True] * 4 + [False] * 4 and V == 8
    assert L == l[0, 0, 1].item()                        # the second largest loss


def test_min_kept_branch_keeps_the_hardest():
    x, t = _pixels([4.0, 5.0, 6.0, 7.0, 8.0, 9.0])      # every p_t > 0.9: the threshold keeps nothing
    loss, kept, L, V, l = _agree(x, t, 0.7, 3)
    assert kept[0, 0].tolist() == [True, True, True, False, False, False]
    assert L == l[0, 0, 2].item()
    assert abs(loss.item() - l[0, 0, :3].mean().item()) < 1e-15


def test_boundary_ties_are_all_kept():
    x, t = _pixels([4.0, 5.0, 5.0, 5.0, 6.0, 7.0])
    loss, kept, L, V, l = _agree(x, t, 0.7, 2)           # rank 2 falls on the three-way tie
    assert kept[0, 0].tolist() == [True, True, True, True, False, False]
    assert int(kept.sum()) == 4 >= 2


def test_min_kept_at_least_v_is_the_weighted_mean_cross_entropy():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 5, 7, 9, generator=g, dtype=torch.float64) * 3
    t = torch.randint(0, 5, (2, 7, 9), generator=g)
    t[0, :2] = -100
    w = torch.rand(5, generator=g, dtype=torch.float64) + 0.2
    V = int((t != -100).sum())
    for mk in (V, V + 1, 10 ** 6):
        loss, kept, _, v, _ = _agree(x, t, 0.05, mk, w)
        assert v == V and torch.equal(kept, t != -100)
        assert torch.allclose(loss, F.cross_entropy(x, t, weight=w), rtol=1e-12)


def test_no_valid_pixel_gives_nan():
    x, t = _pixels([0.0, 1.0])
    t[:] = -100
    loss, kept, L, V, l = _agree(x, t, 0.7, 1)
    assert torch.isnan(loss).item() and V == 0 and not kept.any() and (l == -1).all()


def test_all_equal_losses_keep_everything():
    x = torch.zeros(2, 12, 6, 5, dtype=torch.float64)    # zero-initialised logits: every loss is log 12
    t = torch.randint(0, 12, (2, 6, 5), generator=torch.Generator().manual_seed(1))
    loss, kept, L, V, l = _agree(x, t, 0.01, 7)          # lambda = 4.6 > log 12: only the rank decides
    assert kept.all() and V == 60
    assert abs(loss.item() - np.log(12.0)) < 1e-14


def test_select_applies_the_rule_in_fp32():
    m = np.array([0.5, -1.0, 2.0, np.nan, 2.0, 0.25, 3.0], np.float32)
    kept, L, V, k = R.select(m, np.float32(2.5), 2)
    assert kept.tolist() == [False, False, True, False, True, False, True] and L == np.float32(2.0) and (V, k) == (5, 2)
    kept, L, V, k = R.select(m, np.float32(0.3), 1)
    assert kept.tolist() == [True, False, True, False, True, False, True] and L == np.float32(3.0) and (V, k) == (5, 1)
    kept, L, V, k = R.select(m, np.float32(9.0), 99)
    assert kept.tolist() == [True, False, True, False, True, True, True] and L == np.float32(0.25) and (V, k) == (5, 5)
    kept, L, V, k = R.select(np.array([-1.0, np.nan], np.float32), 0.1, 3)
    assert not kept.any() and (V, k) == (0, 0)


def test_constructor_refusals_and_threshold():
    import pytorch_camvid_amd as A
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="thresh"):
            A.OhemCrossEntropyLoss(thresh=bad)
        with pytest.raises(ValueError, match="thresh"):
            A.ohem_loss_threshold(bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="min_kept"):
            A.OhemCrossEntropyLoss(min_kept=bad)
    with pytest.raises(ValueError, match="1-D tensor"):
        A.OhemCrossEntropyLoss(weight=torch.ones(2, 3))
    lf = A.OhemCrossEntropyLoss(0.7, 1000, weight=torch.ones(12), ignore_index=11)
    assert "weight" in lf.state_dict() and lf.min_kept == 1000 and lf.ignore_index == 11
    with pytest.raises(RuntimeError, match="no forward has run yet"):
        lf.last_record
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lf(torch.zeros(1, 12, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="min_kept"):
        A.ohem_cross_entropy(torch.zeros(1, 12, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), 0.7, 0)
    for th in (0.7, 0.9, 0.05, 1.0, 1e-30):
        lam = A.ohem_loss_threshold(th)
        assert np.float32(lam) == np.float32(-np.log(np.float64(th))) and lam == float(np.float32(lam))
        assert lam == float(R.loss_threshold(th))
    assert A.OhemCrossEntropyLoss(0.9).loss_threshold == A.ohem_loss_threshold(0.9)


def test_entry_point_sizes_and_argument_errors_without_gpu():
    from pytorch_camvid_amd import _lib
    lib = _lib.load()
    assert lib.cvk_ohem_record_floats() == 8
    assert lib.cvk_ohem_scratch_bytes(1) > 0 and lib.cvk_ohem_scratch_bytes(8 * 360 * 480) > lib.cvk_ohem_scratch_bytes(1)
    assert lib.cvk_ohem_scratch_bytes(0) == 0
    p = 4096                                             # any non-null address: argument errors return before a launch
    ok = dict(logits=p, ld=12, target=p, weight=None, lam=0.35, min_kept=10, scratch=p, record=p, loss_px=p, M=100, C=12, ign=-100)

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.cvk_ohem_ce_fwd(a["logits"], a["ld"], a["target"], a["weight"], a["lam"], a["min_kept"], a["scratch"], a["record"],
                                   a["loss_px"], a["M"], a["C"], a["ign"], None)

    for kw, msg in ((dict(logits=None), b"null"), (dict(target=None), b"null"), (dict(scratch=None), b"null"),
                    (dict(record=None), b"null"), (dict(loss_px=None), b"null"), (dict(C=0), b"bad arguments"),
                    (dict(C=129, ld=132), b"bad arguments"), (dict(ld=11), b"bad arguments"), (dict(M=0), b"bad arguments"),
                    (dict(min_kept=0), b"min_kept"), (dict(lam=-0.5), b"loss_thresh"), (dict(lam=float("inf")), b"loss_thresh"),
                    (dict(lam=float("nan")), b"loss_thresh")):
        assert fwd(**kw) == -1, kw
        err = lib.cvk_last_error_string()
        assert err.startswith(b"cvk_ohem_ce_fwd") and msg in err, (kw, err)

    def bwd(**kw):
        a = dict(dict(ok, ld_d=12, dl=p), **kw)
        return lib.cvk_ohem_ce_bwd(a["logits"], a["ld"], a["target"], a["weight"], a["record"], a["loss_px"], None, 1.0, a["dl"],
                                   a["ld_d"], a["M"], a["C"], a["ign"], None)

    for kw, msg in ((dict(record=None), b"null"), (dict(loss_px=None), b"null"), (dict(dl=None), b"null"),
                    (dict(ld_d=11), b"bad arguments"), (dict(C=200, ld=200, ld_d=200), b"bad arguments")):
        assert bwd(**kw) == -1, kw
        err = lib.cvk_last_error_string()
        assert err.startswith(b"cvk_ohem_ce_bwd") and msg in err, (kw, err)
