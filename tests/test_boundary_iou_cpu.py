"""Boundary IoU and the trimap curve without a GPU: the numpy restatement of tests/boundary_iou_ref.py against scipy's binary erosion
(the identity that makes the chessboard depth the right primitive), boundary_dilation, the host score functions on hand-made counts,
the meter's constructor refusals and the C entry points' argument errors."""
import math

import numpy as np
import pytest
import torch

from tests import boundary_iou_ref as R
from tests.boundary_ref import blocky_maps

K, IGN = 12, 11


def _pairs():
    out = dict(R.special_maps(23, 31))
    out["blocky"] = blocky_maps(3, 1, 23, 31, cell=(6, 7), shift=(1, -2), noise=0.02, void=0.04)
    return out


@pytest.mark.parametrize("name", sorted(_pairs()))
def test_restatement_against_scipy_erosion(name):
    """m & ~binary_erosion(m, ones((3,3)), iterations=d, border_value=b) == m & (depth_b <= d): b = 0 is Cheng's zero pad (depth1),
    b = 1 leaves the image border out (depth0).  Both maps, every class."""
    ndi = pytest.importorskip("scipy.ndimage")
    pred, label = _pairs()[name]
    for x in (pred, label):
        code = R.code_bytes(x, label, K, IGN)[0]
        for b in (0, 1):
            dep = R.depth(code, border=(b == 0))
            assert ((dep == 0) == (code >= 32)).all()
            for d in (1, 2, 3, 5, 9):
                for c in range(K):
                    m = code == c
                    band = m & ~ndi.binary_erosion(m, np.ones((3, 3), dtype=bool), iterations=d, border_value=b)
                    assert np.array_equal(band, m & (dep <= d)), (name, b, d, c)


def test_depth_saturates_and_clamps():
    one = np.zeros((300, 270), dtype=np.uint8)
    d0 = R.depth(one, border=False)
    assert (d0 == 255).all()
    d1 = R.depth(one, border=True)
    assert d1.max() == 135 and d1[0, 0] == 1 and d1[150, 134] == 135
    assert R.depth(one, border=False, max_depth=24).max() == 25 and R.depth(one, border=True, max_depth=24).max() == 25
    two = one.copy()
    two[:, 260:] = 1                                      # a boundary 260 columns away from the left edge
    d = R.depth(two, border=False)
    assert d[7, 259] == 1 and d[7, 6] == 254 and d[7, 5] == 255 and d[7, 0] == 255


def test_boundary_dilation_values_and_refusals():
    import pytorch_camvid_amd as A
    assert A.boundary_dilation(360, 480) == 12 and A.boundary_dilation(720, 960) == 24
    assert A.boundary_dilation(96, 128) == 3 and A.boundary_dilation(32, 48) == 1
    assert A.boundary_dilation(1, 1) == 1 and A.boundary_dilation(360, 480, 0) == 1
    assert A.boundary_dilation(30, 40, "0.05") == 3       # 2.5 exactly: the half rounds up, round(2.5) would give 2
    assert A.boundary_dilation(30, 40, 0.03) == 2         # 1.5 exactly
    assert A.boundary_dilation(360, 480, "0.4233") == 254
    for H, W, r in ((360, 480, 0.02), (97, 131, 0.02), (513, 1025, 0.013), (45, 60, 0.1)):
        x = r * math.hypot(H, W)
        if abs(x - math.floor(x) - 0.5) > 1e-6:
            assert A.boundary_dilation(H, W, r) == max(1, round(x)), (H, W, r)
    for bad in (-0.01, "-1", "x", None, True):
        with pytest.raises(ValueError):
            A.boundary_dilation(360, 480, bad)
    with pytest.raises(ValueError, match="254"):
        A.boundary_dilation(360, 480, 0.5)                # 300 pixels
    with pytest.raises(ValueError, match="254"):
        A.boundary_dilation(360, 480, "0.425")            # 255 exactly


def test_boundary_iou_scores_on_hand_made_counts():
    import pytorch_camvid_amd as A
    c = np.zeros((3, 6, 4), dtype=np.int64)
    #            bG  bP  bI  aG   aP   aI
    c[0, :, 0] = [10, 12, 6, 100, 110, 90]
    c[1, :, 0] = [8, 4, 2, 50, 40, 30]
    c[0, :, 1] = [5, 0, 0, 20, 0, 0]                       # predicted nowhere in image 0
    c[2, :, 1] = [4, 4, 4, 9, 9, 9]                        # perfect in image 2
    c[1, :, 3] = [7, 7, 7, 7, 7, 7]                        # counts at the ignore index are not scored
    s = A.boundary_iou_scores(c, ignore_index=3)
    b0, b1 = 8 / (18 + 16 - 8), 4 / (9 + 4 - 4)
    assert np.allclose(s["biou_per_class"][:2], [b0, b1], rtol=0, atol=1e-15)
    assert np.isnan(s["biou_per_class"][2]) and np.isnan(s["biou_per_class"][3])
    assert s["biou"] == pytest.approx((b0 + b1) / 2, abs=1e-15)
    img = [(6 / 16 + 0.0) / 2, 2 / 10, 1.0]
    assert s["biou_image"] == pytest.approx(sum(img) / 3, abs=1e-15) and s["images"] == 3
    m0, m1 = 120 / (150 + 150 - 120), 9 / (29 + 9 - 9)
    assert np.allclose(s["min_iou_per_class"][:2], [min(b0, m0), min(b1, m1)], rtol=0, atol=1e-15)
    assert np.isnan(s["min_iou_per_class"][2:]).all()
    ref = R.scores(c, 3)
    for k in ("biou", "biou_image"):
        assert s[k] == pytest.approx(ref[k], abs=1e-15)
    for k in ("biou_per_class", "min_iou_per_class"):
        assert np.allclose(s[k], ref[k], rtol=0, atol=1e-15, equal_nan=True)
    # without ignore_index class 3 is scored like any other
    assert A.boundary_iou_scores(c)["biou_per_class"][3] == 1.0
    # no images
    e = A.boundary_iou_scores(np.zeros((0, 6, 4), dtype=np.int64), 3)
    assert math.isnan(e["biou"]) and math.isnan(e["biou_image"]) and e["images"] == 0 and np.isnan(e["biou_per_class"]).all()
    with pytest.raises(ValueError, match=r"\[images, 6, K\]"):
        A.boundary_iou_scores(np.zeros((2, 4, 4), dtype=np.int64))


def test_trimap_scores_on_hand_made_bins():
    import pytorch_camvid_amd as A
    b = np.zeros((3, 3, 3), dtype=np.int64)
    b[0] = [[3, 1, 0], [0, 2, 0], [0, 0, 0]]
    b[2] = [[1, 0, 0], [2, 5, 0], [0, 0, 9]]               # bin 1 is empty: width 2 adds nothing to width 1
    s = A.trimap_scores(b, (1, 2, 6), ignore_index=2)
    assert s["widths"] == (1, 2, 6) and s["trimap_pixels"].dtype == np.int64 and s["trimap_pixels"].tolist() == [6, 6, 23]
    i0 = (3 / 4 + 2 / 3) / 2
    assert np.allclose(s["trimap_miou"], [i0, i0, (4 / 7 + 7 / 10) / 2], rtol=0, atol=1e-15)
    assert np.allclose(s["trimap_accuracy"], [5 / 6, 5 / 6, 20 / 23], rtol=0, atol=1e-15)
    ref = R.trimap_scores(b, (1, 2, 6), 2)
    for k in ("trimap_miou", "trimap_accuracy"):
        assert np.allclose(s[k], ref[k], rtol=0, atol=1e-15, equal_nan=True)
    e = A.trimap_scores(np.zeros((2, 3, 3), dtype=np.int64), (1, 2))
    assert np.isnan(e["trimap_miou"]).all() and np.isnan(e["trimap_accuracy"]).all() and e["trimap_pixels"].tolist() == [0, 0]
    for bins, widths in ((b, (1, 2)), (b[:, :2], (1, 2, 6)), (b, (1, 1, 2)), (b, (0, 1, 2)), (b, (1, 2, 255))):
        with pytest.raises(ValueError):
            A.trimap_scores(bins, widths)


def test_meter_refusals():
    import pytorch_camvid_amd as A
    for kw in (dict(num_classes=0), dict(num_classes=33), dict(num_classes=True), dict(ratio=-0.1), dict(ratio="x"), dict(dilation=0),
               dict(dilation=255), dict(dilation=2.0), dict(dilation=True), dict(trimap_widths=(0, 1)), dict(trimap_widths=(2, 2)),
               dict(trimap_widths=(3, 1)), dict(trimap_widths=(1, 255)), dict(trimap_widths=tuple(range(1, 10))),
               dict(trimap_widths=(1.5,)), dict(trimap_widths=4)):
        with pytest.raises(ValueError):
            A.BoundaryIoUMeter(**kw)
    m = A.BoundaryIoUMeter(trimap_widths=[1, 2, 4, 8, 16, 32, 64, 254], dilation=254)
    assert m.trimap_widths == (1, 2, 4, 8, 16, 32, 64, 254)
    assert tuple(m.counts().shape) == (0, 6, 12) and tuple(m.trimap_counts().shape) == (8, 12, 12)
    s = m.compute()
    assert math.isnan(s["biou"]) and s["images"] == 0 and set(s) >= {"trimap_miou", "trimap_accuracy", "trimap_pixels", "widths"}
    assert "trimap_miou" not in A.BoundaryIoUMeter().compute()
    cpu = torch.zeros((1, 4, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU"):
        A.BoundaryIoUMeter().update(cpu, cpu)
    with pytest.raises(ValueError, match="GPU"):
        A.chessboard_depth(cpu)
    with pytest.raises(ValueError, match="int64"):
        A.chessboard_depth(cpu.int())


def test_evaluate_report_takes_the_meter():
    import pytorch_camvid_amd as A
    bi, sd, bf = A.BoundaryIoUMeter(), A.SurfaceDistanceMeter(), A.BoundaryMeter()
    for good in (bi, (bi,), [bf, sd, bi], (bi, sd)):
        with pytest.raises(ValueError, match="no batches"):
            A.evaluate_report(torch.nn.Identity(), [], boundary=good)
    with pytest.raises(ValueError, match="two meters of one kind"):
        A.evaluate_report(torch.nn.Identity(), [], boundary=(bi, A.BoundaryIoUMeter(dilation=3)))
    with pytest.raises(ValueError, match="BoundaryMeter or None"):
        A.evaluate_report(torch.nn.Identity(), [], boundary=(bi, 3))


def test_argument_validation_without_gpu():
    import ctypes
    import pytorch_camvid_amd as A
    lib = A.load_library()
    assert lib.cvk_cheb_workspace_bytes(8, 360, 480) == 8 * 360 * 480 and lib.cvk_cheb_workspace_bytes(1, 5, 7) == 48
    for N, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1, 8, 32769), (1 << 20, 64, 64)):
        assert lib.cvk_cheb_workspace_bytes(N, H, W) == 0, (N, H, W)

    def depth(map=16, void=None, code=16, dep=16, ws=16, N=1, H=8, W=8, C=12, max_depth=254, border=1):
        rc = lib.cvk_cheb_depth(map, void, code, dep, ws, N, H, W, C, 11, max_depth, border, None)
        return rc, lib.cvk_last_error_string()

    for kw, word in (({"map": None}, b"null"), ({"code": None}, b"null"), ({"dep": None}, b"null"), ({"ws": None}, b"null"),
                     ({"C": 0}, b"classes"), ({"C": 33}, b"classes"), ({"N": 0}, b"positive"), ({"W": 0}, b"positive"),
                     ({"N": 1 << 20, "H": 64, "W": 64}, b"2^31"), ({"W": 40000}, b"32768"), ({"max_depth": 0}, b"max_depth"),
                     ({"max_depth": 255}, b"max_depth"), ({"border": 2}, b"border")):
        rc, msg = depth(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)

    def arr(*w):
        return (ctypes.c_int * len(w))(*w)

    def count(cp=16, dp=16, cl=16, dl=16, cnt=16, tri=None, widths=None, nw=0, N=1, H=8, W=8, C=12, d=3):
        rc = lib.cvk_boundary_iou_counts(cp, dp, cl, dl, cnt, tri, widths, nw, N, H, W, C, d, None)
        return rc, lib.cvk_last_error_string()

    for kw, word in (({"cp": None}, b"null"), ({"dp": None}, b"null"), ({"cl": None}, b"null"), ({"dl": None}, b"null"),
                     ({"cnt": None}, b"null"), ({"C": 0}, b"classes"), ({"C": 33}, b"classes"), ({"H": 0}, b"positive"),
                     ({"N": 1 << 20, "H": 64, "W": 64}, b"2^31"), ({"d": 0}, b"dilation"), ({"d": 255}, b"dilation"),
                     ({"tri": 16, "widths": arr(*range(1, 10)), "nw": 9}, b"widths"), ({"nw": -1}, b"widths"),
                     ({"tri": 16, "widths": None, "nw": 2}, b"without widths"), ({"tri": 16, "widths": arr(1), "nw": 0}, b"without widths"),
                     ({"tri": 16, "widths": arr(0, 2), "nw": 2}, b"outside"), ({"tri": 16, "widths": arr(1, 255), "nw": 2}, b"outside"),
                     ({"tri": 16, "widths": arr(2, 2), "nw": 2}, b"increasing"), ({"tri": 16, "widths": arr(1, 4, 3), "nw": 3}, b"increasing")):
        rc, msg = count(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
