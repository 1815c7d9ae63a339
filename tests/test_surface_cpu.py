"""CPU-side checks of the surface-distance meter: the two forms of the numpy reference agree, cvk.surface_distance_scores on hand-made
records, argument validation and workspace sizing of the C entry points, and evaluate_report's signature and its `boundary` argument.  No GPU."""
import inspect
import math

import numpy as np
import pytest
import torch

from tests import boundary_ref as B
from tests import surface_ref as S

K, IGN = 12, 11


@pytest.mark.parametrize("H,W,seed", [(1, 1, 0), (5, 7, 1), (9, 17, 2), (12, 10, 3)])
def test_scipy_form_equals_brute_force(H, W, seed):
    pred, label = B.blocky_maps(seed, 2, H, W, cell=(2, 3))
    for qnum, qden in ((19, 20), (1, 2)):
        d2a, ra = S.surface(pred, label, K, IGN, qnum, qden)
        d2b, rb = S.surface(pred, label, K, IGN, qnum, qden, nearest=S.nearest_d2_brute)
        assert np.array_equal(d2a, d2b) and np.array_equal(ra, rb)
    assert ((d2a >= -2).all()) and (d2a[0] != -2).sum() == ra[:, 0, :, 0].sum() and (d2a[1] != -2).sum() == ra[:, 1, :, 0].sum()


def _records(segments, qnum, qden, Kc=3):
    """records [images, 2, Kc, 8] from {(image, direction, class): int array of d2}; the partner count m is the other direction's n."""
    images = 1 + max(i for i, _, _ in segments)
    rec = np.zeros((images, 2, Kc, S.SLOTS), dtype=np.int64)
    for i in range(images):
        for d in range(2):
            for c in range(Kc):
                v = np.asarray(segments.get((i, d, c), []), dtype=np.int64)
                m = len(segments.get((i, 1 - d, c), []))
                rec[i, d, c] = S.segment_record(v if m else np.full(len(v), -1), m, qnum, qden)
    return rec


@pytest.mark.parametrize("percentile", [0, 50, 95, 100, "97.5", 12.5])
def test_scores_of_hand_made_records(percentile):
    import pytorch_camvid_amd as A
    qnum, qden = A.surface_percentile(percentile)
    rng = np.random.default_rng(5)
    seg = {(0, 0, 0): rng.integers(0, 4096 ** 2, 37), (0, 1, 0): rng.integers(0, 4096 ** 2, 41),
           (0, 0, 1): [9], (0, 1, 1): [16, 25],
           (1, 0, 0): rng.integers(0, 50, 200), (1, 1, 0): rng.integers(0, 50, 2),
           (1, 0, 2): [4, 4, 4]}                                              # class 2 of image 1: a contour in the prediction only
    rec = _records(seg, qnum, qden)
    out = A.surface_distance_scores(rec, ignore_index=None, percentile=percentile)
    q = float(percentile)
    assert out["percentile"] == q and out["images"] == 2
    assert out["unmatched"].tolist() == [0, 0, 1] and out["unmatched"].dtype == np.int64

    def seg_scores(i, c):
        dP, dG = (np.sqrt(np.asarray(seg[(i, d, c)], dtype=np.float64)) for d in range(2))
        return (max(np.percentile(dP, q), np.percentile(dG, q)), max(dP.max(), dG.max()),
                (dP.sum() + dG.sum()) / (len(dP) + len(dG)))

    table = {(i, c): seg_scores(i, c) for i, c in ((0, 0), (0, 1), (1, 0))}
    # the bounds: values are at most 4096 px and a handful of fp64 operations, so 1e-9 absolute for the percentile and the maximum; the
    # fixed-point sum floors every distance to 2^-16 px, so the mean is at most 2^-16 low
    for j, name in enumerate(("hd95", "hd", "assd")):
        tol = 2.0 ** -16 if name == "assd" else 1e-9
        image = [np.mean([table[(0, 0)][j], table[(0, 1)][j]]), table[(1, 0)][j]]
        per_class = [np.mean([table[(0, 0)][j], table[(1, 0)][j]]), table[(0, 1)][j]]
        print(name, out[name], np.mean(image), out[name + "_per_class"], per_class)
        assert abs(out[name] - np.mean(image)) <= tol
        assert np.abs(out[name + "_per_class"][:2] - per_class).max() <= tol
        assert math.isnan(out[name + "_per_class"][2])                       # unmatched: excluded from every mean
        if name == "assd":
            assert out[name] <= np.mean(image) + 1e-12 and (out[name + "_per_class"][:2] <= np.asarray(per_class) + 1e-12).all()
    other = 37 if percentile != 37 else 38                                   # records made with another percentile are refused
    with pytest.raises(ValueError, match="not made with percentile"):
        A.surface_distance_scores(rec, percentile=other)
    masked = A.surface_distance_scores(rec, ignore_index=1, percentile=percentile)
    assert math.isnan(masked["hd_per_class"][1]) and masked["hd"] == out["hd"]


def test_scores_with_nothing_evaluated_are_nan():
    import pytorch_camvid_amd as A
    rec = _records({(0, 0, 1): [1, 2], (1, 1, 2): [3]}, 19, 20)
    out = A.surface_distance_scores(rec)
    assert out["images"] == 0 and out["unmatched"].tolist() == [0, 1, 1]
    for name in ("hd95", "hd", "assd"):
        assert math.isnan(out[name]) and np.isnan(out[name + "_per_class"]).all()
    empty = A.surface_distance_scores(np.zeros((0, 2, 3, 8), dtype=np.int64))
    assert empty["images"] == 0 and math.isnan(empty["hd95"]) and empty["unmatched"].tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="shape"):
        A.surface_distance_scores(np.zeros((2, 3, 8), dtype=np.int64))


def test_percentile_is_read_exactly():
    import pytorch_camvid_amd as A
    assert A.surface_percentile(95) == (19, 20) and A.surface_percentile("97.5") == (39, 40) and A.surface_percentile(97.5) == (39, 40)
    assert A.surface_percentile(0) == (0, 1) and A.surface_percentile(100) == (1, 1) and A.surface_percentile("99.99") == (9999, 10000)
    for bad in (-1, 100.5, "99.999", "x", None, True, float("nan")):
        with pytest.raises(ValueError):
            A.surface_percentile(bad)
    with pytest.raises(ValueError):
        A.SurfaceDistanceMeter(percentile=101)
    with pytest.raises(ValueError):
        A.SurfaceDistanceMeter(num_classes=33)


def test_argument_validation_without_gpu():
    import pytorch_camvid_amd as A
    lib = A.load_library()
    assert lib.cvk_surface_record_slots() == 8

    def call(pred=16, label=16, N=1, H=8, W=8, C=12, qnum=95, qden=100, ws=16, d2=16, rec=16):
        rc = lib.cvk_surface_distances(pred, label, N, H, W, C, 11, qnum, qden, ws, d2, rec, None)
        return rc, lib.cvk_last_error_string()

    for kw, word in (({"pred": None}, b"null"), ({"label": None}, b"null"), ({"ws": None}, b"null"), ({"d2": None}, b"null"),
                     ({"rec": None}, b"null"), ({"C": 0}, b"classes"), ({"C": 33}, b"classes"), ({"N": 0}, b"positive"),
                     ({"H": 5000, "W": 5000}, b"2^24"), ({"N": 1 << 20, "H": 64, "W": 64}, b"2^31"), ({"qnum": 101}, b"percentile"),
                     ({"qnum": -1}, b"percentile"), ({"qden": 0, "qnum": 0}, b"percentile"), ({"qden": 10001}, b"percentile"),
                     ({"ws": 24}, b"16-byte"), ({"d2": 18}, b"misaligned"), ({"rec": 20}, b"misaligned")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)


def test_workspace_bytes():
    import pytorch_camvid_amd as A
    lib = A.load_library()
    assert lib.cvk_surface_workspace_bytes(8, 360, 480, 12) > 0
    assert lib.cvk_surface_workspace_bytes(8, 360, 480, 12) % 16 == 0
    for N, H, W, C in ((0, 8, 8, 12), (1, 8, 8, 0), (1, 8, 8, 33), (1, 5000, 5000, 12), (1, 65535, 1, 12), (1 << 20, 64, 64, 12)):
        assert lib.cvk_surface_workspace_bytes(N, H, W, C) == 0, (N, H, W, C)


def test_evaluate_report_keeps_its_signature():
    """`tta` stays the last parameter of evaluate_report (tests/test_tta_cpu.py and tests/test_boundary_cpu.py hold it there), so the
    surface meter reaches the report through `boundary`, alone or next to a BoundaryMeter."""
    import pytorch_camvid_amd as A
    params = list(inspect.signature(A.evaluate_report).parameters.values())
    assert [p.name for p in params] == ["net", "batches", "num_classes", "ignore_index", "loss_fn", "window", "boundary", "tta"]
    assert all(p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params)
    sd, bf = A.SurfaceDistanceMeter(), A.BoundaryMeter()
    for good in (None, bf, sd, (bf, sd), [sd], []):
        with pytest.raises(ValueError, match="no batches"):                  # the meters pass; the empty set of batches does not
            A.evaluate_report(torch.nn.Identity(), [], boundary=good)
    for bad in (A.ConfusionMeter(12, 11, "cpu"), (bf, 3), "hd95"):
        with pytest.raises(ValueError, match="BoundaryMeter or None"):
            A.evaluate_report(torch.nn.Identity(), [], boundary=bad)
    with pytest.raises(ValueError, match="two meters of one kind"):
        A.evaluate_report(torch.nn.Identity(), [], boundary=(sd, A.SurfaceDistanceMeter(percentile=50)))
