"""CPU-side checks of the boundary F1 measure: the numpy restatement of tests/boundary_ref.py against scipy's exact Euclidean distance
transform and against hand-worked cases, cvk.boundary_tolerance, the host aggregation (cvk.boundary_scores, what
BoundaryMeter.compute() applies to its counts), the checks of cvk_boundary_counts / cvk_boundary_map before any launch, and the
defaults of the workflow."""
import inspect
import math

import numpy as np
import pytest
import torch

from tests import boundary_ref as R

K, IGN = 12, 11
# (seed, H, W, r2): the random cases; the first three share one size, where r2 0 / 2 / 5 match about 10 % / 30 % / 85 %
RANDOM_CASES = [(1, 37, 70, 0), (1, 37, 70, 2), (1, 37, 70, 5), (2, 41, 77, 9), (3, 45, 83, 16)]


@pytest.mark.parametrize("seed,H,W,r2", RANDOM_CASES)
def test_reference_matches_scipy_distance_transform(seed, H, W, r2):
    ndi = pytest.importorskip("scipy.ndimage")
    pred, label = R.blocky_maps(seed, 2, H, W)
    got = R.counts(pred, label, K, IGN, r2)
    want = np.zeros_like(got)
    for n in range(2):
        bP, bG = R.boundary_map(pred[n], label[n], K, IGN), R.boundary_map(label[n], label[n], K, IGN)
        for c in range(K):
            for row, (a, b) in ((0, (bP, bG)), (2, (bG, bP))):
                want[n, row, c] = (a == c).sum()
                if (b == c).any():
                    d = ndi.distance_transform_edt(b != c)             # distance to the nearest pixel of b's class-c boundary
                    want[n, row + 1, c] = ((a == c) & (np.rint(d * d) <= r2)).sum()
    print(f"{H}x{W} r2 {r2}: counts summed over classes {got.sum(axis=2).tolist()}")
    assert np.array_equal(got, want)


def test_random_cases_discriminate():
    """Every class that occurs has boundaries in both maps, and at r2 0 / 2 / 5 most classes match some but not all of them."""
    for seed, H, W, r2 in RANDOM_CASES:
        pred, label = R.blocky_maps(seed, 2, H, W)
        c = R.counts(pred, label, K, IGN, r2).sum(axis=0)
        present = [k for k in range(K) if k != IGN and ((label == k).any() or (pred == k).any())]
        assert present and all(c[0, k] > 0 and c[2, k] > 0 for k in present), (H, W, r2)
        if r2 <= 5:
            strictly = [k for k in present if 0 < c[1, k] < c[0, k] and 0 < c[3, k] < c[2, k]]
            print(f"{H}x{W} r2 {r2}: matched {c[1].sum()} of {c[0].sum()} / {c[3].sum()} of {c[2].sum()}; strictly between: {len(strictly)} of {len(present)}")
            assert len(strictly) * 4 >= len(present) * 3


def test_one_class_everywhere_has_no_boundary():
    import pytorch_camvid_amd as A
    m = np.full((1, 6, 9), 3, dtype=np.int64)
    c = R.counts(m, m, K, IGN, 5)
    assert not c.any()
    for s in (R.scores(c, IGN), A.boundary_scores(c, IGN)):
        assert math.isnan(s["bf"]) and math.isnan(s["pooled"]) and s["images"] == 0 and np.isnan(s["bf_per_class"]).all()


def test_identical_maps_score_one_at_radius_zero():
    _, label = R.blocky_maps(4, 2, 23, 31)
    c = R.counts(label, label, K, IGN, 0)
    assert np.array_equal(c[:, 0], c[:, 1]) and np.array_equal(c[:, 0], c[:, 2]) and np.array_equal(c[:, 0], c[:, 3]) and c.any()
    s = R.scores(c, IGN)
    present = c[:, 0].sum(axis=0) > 0
    assert s["bf"] == 1.0 and s["pooled"] == 1.0 and (s["bf_per_class"][present] == 1.0).all()
    assert np.isnan(s["bf_per_class"][~present]).all()


def test_class_only_in_the_prediction_scores_zero_and_counts():
    label = np.zeros((1, 8, 8), dtype=np.int64)
    label[0, :, 4:] = 1
    pred = label.copy()
    pred[0, 2:4, 0:2] = 5                                      # class 5 exists in the prediction only
    c = R.counts(pred, label, K, IGN, 2)
    assert c[0, 0, 5] == 4 and c[0, 1, 5] == 0 and c[0, 2, 5] == 0 and c[0, 3, 5] == 0
    s = R.scores(c, IGN)
    assert s["bf_per_class"][5] == 0.0 and s["precision"][5] == 0.0 and s["recall"][5] == 0.0
    f0, f1 = s["bf_per_class"][0], s["bf_per_class"][1]
    assert s["bf"] == (f0 + f1 + 0.0) / 3                      # class 5 is evaluated: it pulls the image score down


def test_offset_one_two_matches_at_five_not_at_four():
    """A lone pixel of class 2 in each map, at offset (1, 2): each is its class's whole boundary."""
    label = np.zeros((1, 9, 9), dtype=np.int64)
    pred = np.zeros((1, 9, 9), dtype=np.int64)
    label[0, 3, 3] = 2
    pred[0, 4, 5] = 2
    for r2, m in ((4, 0), (5, 1)):
        c = R.counts(pred, label, K, IGN, r2)
        assert c[0, :, 2].tolist() == [1, m, 1, m], (r2, c[0, :, 2])


def test_void_stripe_separates_without_a_boundary():
    label = np.zeros((1, 5, 7), dtype=np.int64)
    label[0, :, 3] = IGN
    label[0, :, 4:] = 1
    pred = label.copy()
    pred[0, :, 3] = 0                                          # whatever is predicted under the void stripe is void
    assert (R.boundary_map(label[0], label[0], K, IGN) == R.NONE).all()
    assert (R.boundary_map(pred[0], label[0], K, IGN) == R.NONE).all()
    assert not R.counts(pred, label, K, IGN, 4).any()


def test_predicted_ignore_index_is_different_but_no_boundary_of_its_own():
    label = np.zeros((1, 5, 5), dtype=np.int64)
    pred = label.copy()
    pred[0, 2, 2] = IGN
    b = R.boundary_map(pred[0], label[0], K, IGN)
    want = np.full((5, 5), R.NONE, dtype=np.uint8)
    want[1, 2] = want[3, 2] = want[2, 1] = want[2, 3] = 0
    assert np.array_equal(b, want)
    c = R.counts(pred, label, K, IGN, 0)
    assert c[0, 0].tolist() == [4] + [0] * 11 and not c[0, 1:].any()


def test_out_of_range_values_index_nothing():
    label = np.zeros((1, 5, 5), dtype=np.int64)
    pred = label.copy()
    label[0, 1, 1] = 200
    pred[0, 3, 3] = -3
    pred[0, 0, 4] = 2 ** 32 + 1
    bG, bP = R.boundary_map(label[0], label[0], K, IGN), R.boundary_map(pred[0], label[0], K, IGN)
    assert bG[1, 1] == R.NONE and bG[0, 1] == 0 and bG[1, 0] == 0 and bG[2, 1] == 0 and bG[1, 2] == 0 and (bG != R.NONE).sum() == 4
    assert bP[3, 3] == R.NONE and bP[0, 4] == R.NONE and bP[0, 3] == 0 and bP[1, 4] == 0 and (bP != R.NONE).sum() == 6
    c = R.counts(pred, label, K, IGN, 1)
    assert c[0, 0, 0] == 6 and c[0, 2, 0] == 4 and not c[0, :, 1:].any()


def test_boundary_tolerance():
    import pytorch_camvid_amd as A
    assert A.boundary_tolerance(360, 480) == 20 and A.boundary_tolerance(720, 960) == 81 and A.boundary_tolerance(1, 1) == 0
    assert A.boundary_tolerance(360, 480, 0.0075) == 20 and A.boundary_tolerance(300, 400, 0.01) == 25      # exactly 5 pixels: no epsilon
    assert A.boundary_tolerance(1200, 1600, 0.008) == 256
    with pytest.raises(ValueError, match="256"):
        A.boundary_tolerance(1440, 1920)
    with pytest.raises(ValueError, match="256"):
        A.BoundaryMeter(radius2=257)
    with pytest.raises(ValueError, match="radius2"):
        A.BoundaryMeter(radius2=-1)
    with pytest.raises(ValueError, match="1 to 32 classes"):
        A.BoundaryMeter(num_classes=33)
    assert A.BoundaryMeter(radius2=256).radius2 == 256 and A.BoundaryMeter().radius2 is None


def test_host_aggregation_from_hand_made_counts():
    import pytorch_camvid_amd as A
    c = np.zeros((3, 4, 4), dtype=np.int64)                    # K = 4, class 3 ignored
    c[0, :, 0] = [10, 5, 8, 8]                                 # P 0.5, R 1.0, F 2/3
    c[0, :, 1] = [4, 0, 0, 0]                                  # prediction only: F 0
    c[1, :, 0] = [2, 2, 2, 2]                                  # F 1
    c[1, :, 2] = [0, 0, 6, 3]                                  # label only: P 0 -> F 0
    # image 2 has no boundary at all: not scored
    s = A.boundary_scores(c, 3)
    f00 = 2 * 0.5 * 1.0 / 1.5
    assert s["images"] == 2 and s["bf"] == ((f00 + 0.0) / 2 + (1.0 + 0.0) / 2) / 2
    assert s["bf_per_class"][0] == (f00 + 1.0) / 2 and s["bf_per_class"][1] == 0.0 and s["bf_per_class"][2] == 0.0
    assert math.isnan(s["bf_per_class"][3])
    assert s["precision"][0] == 0.75 and s["recall"][0] == 1.0 and s["recall"][2] == 0.5 and s["precision"][2] == 0.0
    pp, pr = 7 / 12, 1.0                                       # pooled class 0: nP 12, mP 7, nG 10, mG 10
    assert s["pooled"] == (2 * pp * pr / (pp + pr) + 0.0 + 0.0) / 3
    want = R.scores(c, 3)
    for k in ("bf", "pooled", "images"):
        assert s[k] == want[k], k
    for k in ("bf_per_class", "precision", "recall"):
        assert np.array_equal(s[k], want[k], equal_nan=True) and s[k].dtype == np.float64, k
    empty = A.boundary_scores(np.zeros((0, 4, 4), dtype=np.int64), 3)
    assert math.isnan(empty["bf"]) and math.isnan(empty["pooled"]) and empty["images"] == 0
    m = A.BoundaryMeter(4, 3)                                  # a meter that saw nothing
    assert tuple(m.counts().shape) == (0, 4, 4) and math.isnan(m.compute()["bf"])
    with pytest.raises(ValueError, match=r"\[images, 4, K\]"):
        A.boundary_scores(np.zeros((4, 4)))


def test_random_counts_aggregate_like_the_loops():
    import pytorch_camvid_amd as A
    pred, label = R.blocky_maps(5, 3, 37, 70)
    c = R.counts(pred, label, K, IGN, 2)
    s, want = A.boundary_scores(c, IGN), R.scores(c, IGN)
    assert abs(s["bf"] - want["bf"]) < 1e-15 and abs(s["pooled"] - want["pooled"]) < 1e-15 and s["images"] == 3
    for k in ("bf_per_class", "precision", "recall"):
        assert np.allclose(s[k], want[k], rtol=0, atol=1e-15, equal_nan=True), k


def test_entry_points_validate_before_any_launch():
    from pytorch_camvid_amd import _lib
    lib = _lib.load()
    p = 256                                                    # a non-null "pointer": never dereferenced on these paths
    bc, bm = lib.cvk_boundary_counts, lib.cvk_boundary_map
    #          pred label counts N  H   W   K  ignore r2 stream
    for args in ((None, p, p, 1, 17, 23, 12, 11, 4, None), (p, None, p, 1, 17, 23, 12, 11, 4, None), (p, p, None, 1, 17, 23, 12, 11, 4, None)):
        assert bc(*args) == -1 and b"null pointer" in lib.cvk_last_error_string(), args
    for k in (0, 33, -1):
        assert bc(p, p, p, 1, 17, 23, k, 11, 4, None) == -1 and b"classes" in lib.cvk_last_error_string(), k
        assert bm(p, None, p, 1, 17, 23, k, 11, None) == -1 and b"classes" in lib.cvk_last_error_string(), k
    for r2 in (-1, 257):
        assert bc(p, p, p, 1, 17, 23, 12, 11, r2, None) == -1 and b"0..256" in lib.cvk_last_error_string(), r2
    for n, h, w in ((0, 17, 23), (1, 0, 23), (1, 17, -4)):
        assert bc(p, p, p, n, h, w, 12, 11, 4, None) == -1 and b"positive" in lib.cvk_last_error_string(), (n, h, w)
        assert bm(p, p, p, n, h, w, 12, 11, None) == -1 and b"positive" in lib.cvk_last_error_string(), (n, h, w)
    assert bc(p, p, p, 8, 16384, 16384, 12, 11, 4, None) == -1 and b"2^31" in lib.cvk_last_error_string()
    assert bm(p, None, p, 8, 16384, 16384, 12, 11, None) == -1 and b"2^31" in lib.cvk_last_error_string()
    assert bm(None, p, p, 1, 17, 23, 12, 11, None) == -1 and b"null pointer" in lib.cvk_last_error_string()
    assert bm(p, p, None, 1, 17, 23, 12, 11, None) == -1 and b"null pointer" in lib.cvk_last_error_string()


def test_python_surface_validates_and_defaults():
    import pytorch_camvid_amd as A
    for name in ("BoundaryMeter", "label_boundaries", "boundary_tolerance"):
        assert name in A.__all__ and hasattr(A, name), name
    sig = inspect.signature(A.evaluate_report).parameters
    assert sig["boundary"].default is None and list(sig)[-3:] == ["window", "boundary", "tta"]      # `tta` stays the last one
    assert "boundary" not in inspect.signature(A.evaluate).parameters
    init = inspect.signature(A.BoundaryMeter.__init__).parameters
    assert [(k, v.default) for k, v in init.items() if k != "self"] == [("num_classes", 12), ("ignore_index", 11), ("tolerance", 0.0075),
                                                                         ("radius2", None)]
    m = A.BoundaryMeter()
    z = torch.zeros((1, 4, 4), dtype=torch.int64)
    for pred, label in ((z, z), (z.int(), z.int()), (z[0], z[0]), (z, torch.zeros((1, 4, 5), dtype=torch.int64))):
        with pytest.raises(ValueError):
            m.update(pred, label)                              # CPU tensors, another dtype, no batch axis, another shape
    with pytest.raises(ValueError):
        A.label_boundaries(z)
    with pytest.raises(ValueError, match="BoundaryMeter or None"):
        A.evaluate_report(torch.nn.Identity(), [], boundary=A.ConfusionMeter(12, 11, "cpu"))
