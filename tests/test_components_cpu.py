"""Connected components and small-region removal without a GPU: the scipy restatement (tests/components_ref.py) against a plain
breadth-first search, its vote rules on hand-made maps, the C entry points' argument checks (no launch), the Python refusals, and the
meter's place in evaluate_report."""
import inspect
import math

import numpy as np
import pytest
import torch

from tests import components_ref as R


@pytest.mark.parametrize("connectivity", [4, 8])
def test_restatement_matches_a_breadth_first_search(connectivity):
    rng = np.random.default_rng(5)
    for H, W, K, p_void in ((1, 1, 2, 0.0), (1, 7, 2, 0.2), (7, 1, 3, 0.2), (9, 11, 2, 0.0), (13, 17, 3, 0.15), (20, 23, 5, 0.1)):
        for _ in range(3):
            m = rng.integers(0, K, size=(H, W)).astype(np.int64)
            m[rng.random((H, W)) < p_void] = rng.choice([-1, K, K + 5, 2 ** 40])
            c = R.codes(m, K, 1 if K > 2 else -100)
            lab, area = R.label_image(c, connectivity)
            blab, barea = R.bfs_labels(c, connectivity)
            assert np.array_equal(lab, blab) and np.array_equal(area, barea), (H, W, K)
            assert (lab.ravel() <= np.arange(H * W)).all()
            roots = lab.ravel() == np.arange(H * W)
            assert roots.sum() == len(np.unique(lab)) and area.ravel()[roots].sum() == H * W
    for maker in (R.spiral, R.serpentine, R.comb, R.checkerboard):
        m = maker(9, 14)
        assert np.array_equal(R.label_image(m, connectivity)[0], R.bfs_labels(m, connectivity)[0]), maker.__name__


def test_special_maps_are_what_their_names_say():
    for H, W in ((65, 97), (9, 13)):
        lab, area = R.label_image(R.spiral(H, W), 4)
        assert len(np.unique(lab)) == 2 and lab[0, 0] == 0
        lab, _ = R.label_image(R.serpentine(H, W), 4)
        assert (lab[R.serpentine(H, W) == 1] == 0).all()
    lab, _ = R.label_image(R.comb(70, 130), 4)
    assert (lab[R.comb(70, 130) == 1] == 0).all() and len(np.unique(lab)) == 1 + 130 // 2
    cb = R.checkerboard(37, 53)
    assert len(np.unique(R.label_image(cb, 4)[0])) == 37 * 53 and len(np.unique(R.label_image(cb, 8)[0])) == 2


def test_tie_goes_to_the_smallest_class():
    # one pixel of class 2 between class 1 (left, above) and class 0 (right, below): two votes each
    m = np.array([[[1, 1, 1, 0, 0],
                   [1, 1, 2, 0, 0],
                   [1, 1, 0, 0, 0]]], dtype=np.int64)
    m[0, 0, 2] = 1
    out, rec = R.filter_regions(m, 3, -100, 4, 2, "neighbor")
    assert out[0, 1, 2] == 0 and (np.delete(out.ravel(), 7) == np.delete(m.ravel(), 7)).all()
    assert rec[0, 2].tolist() == [1, 1, 1, 1, 1, 1, 0, 0] and rec[0, 0, 6] == 1 and rec[0, 1, 6] == 0
    # three votes against one: the majority wins although its class is larger
    m2 = np.array([[[2, 2, 2], [2, 0, 2], [1, 1, 1], [1, 1, 1]]], dtype=np.int64)
    out, rec = R.filter_regions(m2, 3, -100, 4, 2, "neighbor")
    assert out[0, 1, 1] == 2 and rec[0, 2, 6] == 1
    # under 8 the diagonals vote too: 5 of class 2, 3 of class 1
    out8, _ = R.filter_regions(m2, 3, -100, 8, 2, "neighbor")
    assert out8[0, 1, 1] == 2


def test_isolated_components_stay_and_void_never_votes():
    K, ig = 3, 2
    m = np.full((1, 5, 6), ig, dtype=np.int64)              # void everywhere, the only large region
    m[0, 1, 1] = 0
    m[0, 3, 3:5] = 1
    m[0, 0, 5] = 7                                          # out of range: void as well, and kept bit for bit
    out, rec = R.filter_regions(m, K, ig, 4, 3, "neighbor")
    assert np.array_equal(out, m)
    assert rec[0, 0].tolist() == [1, 1, 1, 1, 1, 0, 0, 1] and rec[0, 1].tolist() == [1, 2, 2, 1, 2, 0, 0, 1] and not rec[0, 2].any()
    out, rec = R.filter_regions(m, K, ig, 4, 3, "fill")
    assert (out[0, 1, 1], out[0, 3, 3], out[0, 0, 5]) == (ig, ig, 7) and rec[0, :, 5].tolist() == [1, 1, 0] and not rec[0, :, 6].any()
    out, rec = R.filter_regions(m, K, ig, 4, 3, "fill", fill_value=0)
    assert out[0, 3, 4] == 0 and out[0, 1, 1] == 0 and rec[0, :, 5].tolist() == [0, 1, 0] and rec[0, :, 6].tolist() == [2, 0, 0]
    out, rec = R.filter_regions(m, K, ig, 4, 1, "neighbor")
    assert np.array_equal(out, m) and not rec[0, :, 3:].any()


def test_one_round_only_small_components_do_not_vote():
    # a 1-pixel class-2 speck whose only class neighbours are a small class-1 component: no vote, although after the filter the
    # neighbours are class 0; the small class-1 component itself goes to class 0
    ig = 9
    m = np.array([[[0, 0, 0, 0, 0, 0],
                   [0, 0, 0, 0, 0, 0],
                   [0, 1, 1, 1, 0, 0],
                   [0, 1, 2, 1, 0, 0],
                   [0, 1, 1, 1, 0, 0],
                   [0, 0, 0, 0, 0, 0]]], dtype=np.int64)
    out, rec = R.filter_regions(m, 3, ig, 4, 9, "neighbor")
    assert out[0, 3, 2] == 2 and rec[0, 2, 7] == 1
    assert ((out == 0) == (m != 2)).all() and rec[0, 1, 5] == 1 and rec[0, 0, 6] == 8
    again, _ = R.filter_regions(out, 3, ig, 4, 9, "neighbor")
    assert again[0, 3, 2] == 0                               # a second round would take it: the filter does not run one


def test_entry_points_validate_before_any_launch():
    import pytorch_camvid_amd as A
    lib = A.load_library()
    assert lib.cvk_cc_record_slots() == 8
    M = 8 * 360 * 480
    assert lib.cvk_cc_workspace_bytes(8, 360, 480, 12) == 4 * M + M + 4 * M * 12
    assert lib.cvk_cc_workspace_bytes(1, 1, 7, 3) == 32 + 16 + 84
    for N, H, W, C in ((0, 8, 8, 12), (1, 0, 8, 12), (1, 8, -1, 12), (1, 8, 8, 0), (1, 8, 8, 33), (1 << 20, 64, 32, 12)):
        assert lib.cvk_cc_workspace_bytes(N, H, W, C) == 0, (N, H, W, C)
    assert lib.cvk_cc_workspace_bytes(1 << 19, 64, 32, 1) > 0          # 2^30 pixels

    def label(map=16, lab=16, area=32, N=1, H=8, W=8, C=12, conn=4, ws=16):
        rc = lib.cvk_cc_label(map, lab, area, N, H, W, C, 11, conn, ws, None)
        return rc, lib.cvk_last_error_string()

    for kw, word in (({"map": None}, b"null"), ({"lab": None}, b"null"), ({"area": None}, b"null"), ({"ws": None}, b"null"),
                     ({"C": 0}, b"classes"), ({"C": 33}, b"classes"), ({"N": 0}, b"positive"), ({"H": -1}, b"positive"),
                     ({"N": 1 << 20, "H": 64, "W": 32}, b"2^31"), ({"conn": 6}, b"connectivity"), ({"conn": 0}, b"connectivity"),
                     ({"area": 16}, b"one buffer")):
        rc, msg = label(**kw)
        assert rc == -1 and msg.startswith(b"cvk_cc_label") and word in msg, (kw, rc, msg)

    def filt(map=4096, lab=16, area=32, out=8192, rec=None, N=1, H=8, W=8, C=12, conn=4, min_area=2, mode=1, fill=11, ws=16):
        rc = lib.cvk_cc_filter(map, lab, area, out, rec, N, H, W, C, 11, conn, min_area, mode, fill, ws, None)
        return rc, lib.cvk_last_error_string()

    for kw, word in (({"map": None}, b"null"), ({"lab": None}, b"null"), ({"area": None}, b"null"), ({"out": None}, b"null"),
                     ({"ws": None}, b"null"), ({"C": 0}, b"classes"), ({"C": 33}, b"classes"), ({"W": 0}, b"positive"),
                     ({"N": 1 << 20, "H": 64, "W": 32}, b"2^31"), ({"conn": 5}, b"connectivity"), ({"min_area": 0}, b"min_area"),
                     ({"min_area": -3}, b"min_area"), ({"mode": 2}, b"mode"), ({"mode": -1}, b"mode"), ({"out": 4096}, b"alias"),
                     ({"out": 4096 + 8 * 63}, b"alias"), ({"out": 4096 - 8 * 63}, b"alias")):
        rc, msg = filt(**kw)
        assert rc == -1 and msg.startswith(b"cvk_cc_filter") and word in msg, (kw, rc, msg)


def test_python_surface_and_refusals():
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd import functional
    for name in ("connected_components", "remove_small_regions", "RegionFilter", "RegionMeter"):
        assert getattr(A, name) is getattr(functional, name), name
    sig = inspect.signature(A.connected_components).parameters
    assert [(k, v.default) for k, v in sig.items()][1:] == [("num_classes", 12), ("ignore_index", 11), ("connectivity", 4)]
    sig = inspect.signature(A.remove_small_regions).parameters
    assert [(k, v.default) for k, v in sig.items()][2:] == [("num_classes", 12), ("ignore_index", 11), ("connectivity", 4),
                                                            ("mode", "neighbor"), ("fill_value", None)]
    sig = inspect.signature(A.RegionMeter.__init__).parameters
    assert [(k, v.default) for k, v in sig.items() if k != "self"] == [("num_classes", 12), ("ignore_index", 11), ("min_area", 64),
                                                                       ("connectivity", 4), ("mode", "neighbor")]
    assert A.RegionFilter(5, mode="fill").fill_value == 11 and A.RegionFilter(5, ignore_index=3, mode="fill", fill_value=0).fill_value == 0
    for kw in (dict(min_area=0), dict(min_area=-1), dict(min_area=2.5), dict(min_area=True), dict(min_area=4, connectivity=6),
               dict(min_area=4, connectivity=True), dict(min_area=4, mode="nearest"), dict(min_area=4, num_classes=33),
               dict(min_area=4, num_classes=0), dict(min_area=4, fill_value=3), dict(min_area=4, mode="fill", fill_value=1.5),
               dict(min_area=4, mode="fill", fill_value=2 ** 63)):
        with pytest.raises(ValueError):
            A.RegionFilter(**kw)
    for kw in (dict(min_area=0), dict(connectivity=5), dict(mode="fil"), dict(num_classes=33)):
        with pytest.raises(ValueError):
            A.RegionMeter(**kw)
    cpu = torch.zeros((1, 4, 4), dtype=torch.int64)
    for call in (lambda: A.connected_components(cpu), lambda: A.remove_small_regions(cpu, 4), lambda: A.RegionFilter(4)(cpu[0]),
                 lambda: A.RegionMeter().update(cpu, cpu)):
        with pytest.raises(ValueError, match="GPU"):
            call()
    for bad in (cpu.int(), cpu[0, 0], torch.zeros((1, 1, 4, 4), dtype=torch.int64), torch.zeros((0, 4, 4), dtype=torch.int64), "map"):
        with pytest.raises(ValueError, match="int64"):
            A.connected_components(bad)
        with pytest.raises(ValueError, match="int64"):
            A.remove_small_regions(bad, 4)
    with pytest.raises(ValueError, match="connectivity"):
        A.connected_components(cpu, connectivity=6)
    with pytest.raises(ValueError, match="32 classes"):
        A.connected_components(cpu, num_classes=40)
    with pytest.raises(ValueError, match="2\\^31"):
        A.connected_components(torch.empty((1, 1 << 16, 1 << 15), dtype=torch.int64, device="meta"))
    with pytest.raises(RuntimeError, match="not been called"):
        A.RegionFilter(4).last_record


def test_region_scores_on_hand_made_sums():
    import pytorch_camvid_amd as A
    rp, rl = np.zeros((4, 8), dtype=np.int64), np.zeros((4, 8), dtype=np.int64)
    rp[:, 0], rl[:, 0], rp[:, 3] = [6, 2, 0, 5], [2, 2, 0, 1], [4, 0, 0, 5]
    hist = np.array([[30, 10, 0, 0], [40, 20, 0, 7], [50, 10, 0, 3]], dtype=np.int64)
    s = A.region_scores(rp, rl, hist, ignore_index=3)
    assert s["regions_pred"].tolist() == [6, 2, 0, 5] and s["regions_label"].tolist() == [2, 2, 0, 1] and s["small_regions_pred"].tolist() == [4, 0, 0, 5]
    assert s["fragmentation_per_class"][:2].tolist() == [3.0, 1.0] and np.isnan(s["fragmentation_per_class"][2:]).all()
    assert s["fragmentation"] == 2.0
    assert np.allclose(s["iou_filtered"][:2], [0.5, 0.5], rtol=0, atol=1e-15) and np.isnan(s["iou_filtered"][2:]).all() and s["miou_filtered"] == 0.5
    e = A.RegionMeter(num_classes=4, ignore_index=3).compute()
    assert math.isnan(e["fragmentation"]) and math.isnan(e["miou_filtered"]) and e["images"] == 0 and not e["regions_pred"].any()


def test_evaluate_report_takes_the_meter_and_keeps_its_refusals():
    import pytorch_camvid_amd as A
    rm, bi, sd, bf = A.RegionMeter(), A.BoundaryIoUMeter(), A.SurfaceDistanceMeter(), A.BoundaryMeter()
    for good in (rm, (rm,), [bf, rm], (bf, sd, bi, rm), None, bf, (bf, sd)):
        with pytest.raises(ValueError, match="no batches"):
            A.evaluate_report(torch.nn.Identity(), [], boundary=good)
        with pytest.raises(ValueError, match="no batches"):
            A.evaluate_report(torch.nn.Identity(), [], boundary=good, window=A.SlidingWindow((32, 32), (16, 16)))
        with pytest.raises(ValueError, match="no batches"):
            A.evaluate_report(torch.nn.Identity(), [], boundary=good, tta=A.TestTimeAugmentation(scales=(1.0,), flip=False))
    with pytest.raises(ValueError, match="two meters of one kind"):
        A.evaluate_report(torch.nn.Identity(), [], boundary=(rm, A.RegionMeter(min_area=3)))
    for bad in (3, "bf", (bf, 3), [rm, object()], A.RegionFilter(4)):
        with pytest.raises(ValueError, match="BoundaryMeter or None"):
            A.evaluate_report(torch.nn.Identity(), [], boundary=bad)
    sig = inspect.signature(A.evaluate_report).parameters
    assert list(sig) == ["net", "batches", "num_classes", "ignore_index", "loss_fn", "window", "boundary", "tta"]
    assert list(inspect.signature(A.predict).parameters) == ["net", "image_u8", "out_size", "mean", "std", "window", "tta"]
    assert list(inspect.signature(A.evaluate).parameters) == ["net", "batches", "num_classes", "ignore_index", "window", "tta"]
