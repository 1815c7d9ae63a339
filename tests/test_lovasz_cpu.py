"""CPU-side checks of the Lovász-softmax loss: the fp64 restatement against itself (closed-form weights against the cumulative Jaccard
formulation), the sort's two index functions exhausted on small sizes, the raw entry points' sizes and argument errors, the
constructor's refusals and the exported names."""
import os
import re

import numpy as np
import pytest
import torch

from tests import lovasz_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(kind, N=2, C=5, H=7, W=9, seed=0):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, C, (N, H, W))
    if kind == "random":
        x = 3 * rng.standard_normal((N, C, H, W))
    elif kind == "zeros":
        x = np.zeros((N, C, H, W))
    elif kind == "saturated":
        x = 60.0 * (2 * rng.integers(0, 2, (N, C, H, W)) - 1)
    elif kind == "absent":
        x = 3 * rng.standard_normal((N, C, H, W))
        t[t == 2] = 3                                       # class 2 never occurs
    else:
        raise ValueError(kind)
    t[rng.random((N, H, W)) < 0.15] = -100
    return x, t


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("classes", ["present", "all"])
@pytest.mark.parametrize("kind", ["random", "zeros", "saturated", "absent"])
def test_the_two_formulations_agree(kind, classes, per_image):
    x, t = _case(kind)
    a = R.lovasz_softmax(x, t, classes=classes, per_image=per_image, weights=R.weights_closed_form)
    b = R.lovasz_softmax(x, t, classes=classes, per_image=per_image, weights=R.weights_cumulative_jaccard)
    assert abs(a["loss"] - b["loss"]) <= 1e-12 and a["pairs"] == b["pairs"] and a["counted"] == b["counted"]
    assert np.allclose(a["class_loss"], b["class_loss"], rtol=0, atol=1e-12, equal_nan=True)
    assert np.abs(a["dlogits"] - b["dlogits"]).max() <= 1e-12
    assert 0.0 <= a["loss"] <= 1.0 + 1e-12
    if kind == "absent":
        assert np.isnan(a["class_loss"][2]) == (classes == "present")
    if kind == "zeros":                                     # every error ties: the stable order is the memory order
        assert (R.stable_order(np.full(9, 0.2)) == np.arange(9)).all()


def test_weights_sum_to_the_jaccard_loss_and_match_torch_autograd():
    rng = np.random.default_rng(3)
    for G in (0, 1, 5, 40):
        fg = np.zeros(40, bool)
        fg[rng.permutation(40)[:G]] = True
        g = R.weights_closed_form(fg)
        assert np.abs(g - R.weights_cumulative_jaccard(fg)).max() <= 1e-15
        assert (g >= 0).all() and abs(g.sum() - 1.0) <= 1e-12          # J runs from 0 to 1 - 0 / V = 1
    # the restatement's gradient is the derivative of its loss (the order is locally constant)
    x, t = _case("random", N=1, C=4, H=5, W=6, seed=5)
    out = R.lovasz_softmax(x, t, classes="all")
    eps, worst = 1e-6, 0.0
    for idx in [(0, 1, 2, 3), (0, 0, 0, 0), (0, 3, 4, 5)]:
        xp, xm = x.copy(), x.copy()
        xp[idx] += eps
        xm[idx] -= eps
        num = (R.lovasz_softmax(xp, t, classes="all")["loss"] - R.lovasz_softmax(xm, t, classes="all")["loss"]) / (2 * eps)
        worst = max(worst, abs(num - out["dlogits"][idx]))
    assert worst <= 1e-8, worst


def test_empty_and_all_ignored():
    x, t = _case("random")
    out = R.lovasz_softmax(x, np.full_like(t, -100))
    assert out["loss"] == 0.0 and out["counted"] == 0 and (out["dlogits"] == 0).all()
    t[1] = -100                                              # one image without a valid pixel: not counted
    one = R.lovasz_softmax(x, t, per_image=True)
    assert one["counted"] == 1 and abs(one["loss"] - R.lovasz_softmax(x[:1], t[:1])["loss"]) <= 1e-15


def test_sort_index_functions_exhausted():
    """Every destination of every pass, for every small size around the tile, goes through the library's own index functions: all in
    range, none written twice, and the result is the stable order."""
    from pytorch_camvid_amd import _lib
    lib = _lib.load()
    dest, cidx = lib.cvk_lovasz_sort_dest, lib.cvk_lovasz_sort_count_index
    rng = np.random.default_rng(11)
    for tile in (4, 7):
        for P in list(range(1, 3 * tile + 2)) + [5 * tile - 1]:
            for S in (1, 3):
                keys = rng.integers(0, 2 ** 32, (S, P), dtype=np.uint64)
                keys[:, ::3] = keys[:, :1]                  # ties
                keys[rng.random((S, P)) < 0.2] = 0xFFFFFFFF
                perm = R.radix_sort_emulation(keys, tile, 8, dest, cidx, segments=S)
                for s in range(S):
                    assert (perm[s] == np.argsort(keys[s], kind="stable")).all(), (tile, P, S, s)
    # out-of-range pieces are refused, not wrapped
    assert dest(10, 2, 3, 4, 2) == 29 and dest(10, 2, 3, 4, 3) == -1 and dest(10, 0, 0, 0, 10) == -1
    for bad in ((0, 0, 0, 0, 0), (10, -1, 0, 0, 0), (10, 0, -1, 0, 0), (10, 0, 0, -1, 0), (10, 0, 0, 0, -1), (10, 0, 2 ** 32 - 1, 0, 0)):
        assert dest(*bad) == -1, bad
    assert cidx(3, 1, 255, 2) == (1 * 256 + 255) * 3 + 2 and cidx(3, 0, 0, 0) == 0
    for bad in ((0, 0, 0, 0), (3, -1, 0, 0), (3, 0, 256, 0), (3, 0, -1, 0), (3, 0, 0, 3), (3, 0, 0, -1)):
        assert cidx(*bad) == -1, bad
    # the largest supported sizes stay inside 63 bits
    assert dest(2 ** 30 - 1, 65534, 0, 0, 2 ** 30 - 2) == 65534 * (2 ** 30 - 1) + 2 ** 30 - 2


def test_workspace_size_reaches_the_stated_model():
    from pytorch_camvid_amd import _lib
    from pytorch_camvid_amd import functional as F
    lib = _lib.load()
    assert lib.cvk_lovasz_record_floats() == F.LOVASZ_RECORD_HEAD + 2 * F.LOVASZ_CLASS_SLOTS == 264
    hdr = open(os.path.join(ROOT, "include", "cvk.h")).read()
    assert int(re.search(r"#define CVK_LOVASZ_SORT_TILE (\d+)", hdr).group(1)) == F.LOVASZ_SORT_TILE
    assert int(re.search(r"#define CVK_LOVASZ_DIGIT_BITS (\d+)", hdr).group(1)) == 8
    ws = lib.cvk_lovasz_workspace_bytes
    M, C = 8 * 360 * 480, 12
    for S in (1, 8):
        n = ws(M, C, S)
        model = 2 * 8 * M * C + 4 * M * C                  # two ping-pong buffers and the g map
        assert model <= n <= 1.03 * model, (S, n, model)
    assert abs(2 * 8 * M * C / 1e6 - 265.4) < 0.1 and abs(4 * M * C / 1e6 - 66.4) < 0.1          # the figures DESIGN.md states
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "265.4 MB" in design and "66.4 MB" in design
    # monotone in M, in C and in the number of segments
    for S in (1, 2):
        sizes = [ws(m, 12, S) for m in (2, 100, 2048, 2050, 4096, 100000, 1382400)]
        assert all(a > 0 for a in sizes) and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    sizes = [ws(7200, c, 2) for c in (1, 2, 5, 12, 13, 128)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    sizes = [ws(7200, 12, s) for s in (1, 2, 4, 8)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    # unsupported: no pixel, no class, too many classes, segments that do not divide the batch, too many (segment, class) pairs
    for bad in ((0, 12, 1), (100, 0, 1), (100, 129, 1), (100, 12, 0), (100, 12, 3), (65536 * 2, 2, 65536)):
        assert ws(*bad) == 0, bad


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from pytorch_camvid_amd import _lib
    lib = _lib.load()
    p = 4096                                             # any non-null aligned address: argument errors return before a launch
    ok = dict(logits=p, ld=12, target=p, weight=None, lovasz=1.0, ce=0.0, mode=0, per_image=0, N=2, hw=50, ws=p, record=p, gmap=p,
              ld_g=12, C=12, ign=-100)

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.cvk_lovasz_softmax_fwd(a["logits"], a["ld"], a["target"], a["weight"], a["lovasz"], a["ce"], a["mode"], a["per_image"],
                                          a["N"], a["hw"], a["ws"], a["record"], a["gmap"], a["ld_g"], a["C"], a["ign"], None)

    for kw, msg in ((dict(logits=None), b"null"), (dict(target=None), b"null"), (dict(ws=None), b"null"), (dict(record=None), b"null"),
                    (dict(gmap=None), b"null"), (dict(ws=4100), b"aligned"), (dict(mode=2), b"classes_mode"),
                    (dict(per_image=2), b"per_image"), (dict(C=0), b"bad arguments"), (dict(C=129, ld=132, ld_g=132), b"bad arguments"),
                    (dict(ld=11), b"bad arguments"), (dict(ld_g=11), b"bad arguments"), (dict(N=0), b"batch size"),
                    (dict(hw=0), b"batch size"), (dict(N=2 ** 16, hw=2 ** 15), b"batch size"), (dict(lovasz=0.0), b"lovasz"),
                    (dict(lovasz=float("nan")), b"lovasz"), (dict(lovasz=float("inf")), b"lovasz"), (dict(ce=-1.0), b"ce must"),
                    (dict(ce=float("nan")), b"ce must"), (dict(weight=p), b"class weights"),
                    (dict(N=40000, hw=4, per_image=1), b"unsupported size")):
        assert fwd(**kw) == -1, kw
        err = lib.cvk_last_error_string()
        assert err.startswith(b"cvk_lovasz_softmax_fwd") and msg in err, (kw, err)

    def bwd(**kw):
        a = dict(dict(ok, ld_d=12, dl=p), **kw)
        return lib.cvk_lovasz_softmax_bwd(a["logits"], a["ld"], a["target"], a["weight"], a["lovasz"], a["ce"], a["per_image"], a["N"],
                                          a["hw"], a["ws"], a["record"], a["gmap"], a["ld_g"], None, 1.0, a["dl"], a["ld_d"], a["C"],
                                          a["ign"], None)

    for kw, msg in ((dict(record=None), b"null"), (dict(gmap=None), b"null"), (dict(dl=None), b"null"), (dict(ws=None), b"null"),
                    (dict(ld_d=11), b"bad arguments"), (dict(C=200, ld=200, ld_d=200, ld_g=200), b"bad arguments"),
                    (dict(lovasz=-1.0), b"lovasz"), (dict(weight=p), b"class weights"), (dict(per_image=-1), b"per_image")):
        assert bwd(**kw) == -1, kw
        err = lib.cvk_last_error_string()
        assert err.startswith(b"cvk_lovasz_softmax_bwd") and msg in err, (kw, err)


def test_constructor_refusals_and_exports():
    import pytorch_camvid_amd as A
    for name in ("LovaszSoftmaxLoss", "lovasz_softmax"):
        assert name in A.__all__ and hasattr(A, name), name
    for kw in (dict(lovasz=0.0), dict(lovasz=-1.0), dict(lovasz=float("nan")), dict(lovasz=float("inf")), dict(ce=-0.5),
               dict(ce=float("inf")), dict(classes="some"), dict(per_image=1), dict(weight=torch.ones(12)),
               dict(ce=1.0, weight=torch.ones(3, 4)), dict(ce=1.0, weight=[1.0] * 12)):
        with pytest.raises(ValueError):
            A.LovaszSoftmaxLoss(**kw)
    with pytest.raises(ValueError):
        A.lovasz_softmax(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), classes="nope")
    lf = A.LovaszSoftmaxLoss(0.5, 1.0, classes="all", per_image=True, weight=torch.ones(12), ignore_index=11)
    assert (lf.lovasz, lf.ce, lf.classes, lf.per_image, lf.ignore_index) == (0.5, 1.0, "all", True, 11)
    assert "weight" in lf.state_dict()
    with pytest.raises(RuntimeError, match="no forward"):
        lf.last_record
    with pytest.raises(RuntimeError, match="no forward"):
        lf.sorted_view()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lf(torch.zeros(1, 12, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
