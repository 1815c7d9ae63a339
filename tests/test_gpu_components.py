"""Connected components and small-region removal on the GPU: cvk_cc_label / cvk_cc_filter through cvk.connected_components,
cvk.RegionFilter and cvk.RegionMeter against the scipy restatement of tests/components_ref.py.  Every output is an integer and every
comparison a torch.equal; each prints what differs before it asserts.  The maps are the smallest at which each mechanism can go
wrong: tiles are 32 x 64 pixels, so 65 x 97 has 3 x 2 of them and 130 x 200 has 5 x 4."""
import functools

import numpy as np
import pytest
import torch

from tests import components_ref as R
from tests.boundary_ref import blocky_maps

pytestmark = pytest.mark.gpu

K, IGN = 12, 11
MIN_AREAS = (1, 2, 9, 10 ** 6)


def dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.array(a)).to(dev())


def _blocky():
    pred, label = blocky_maps(3, 2, 96, 128, cell=(7, 9), shift=(2, -2), noise=0.03, void=0.0)
    m = pred.copy()
    m[:, 20:23, :] = IGN                                   # void stripes, both ways, across every tile seam
    m[:, :, 60:67] = IGN
    m[0, 40:44, 10:90] = -1                                # values outside [0, K): void too, and kept bit for bit
    m[1, 70:90, 100] = K
    m[1, 5, 5:9] = 2 ** 32 + 3
    return m


def _tiny(H, W):
    rng = np.random.default_rng(H * 10 + W)
    m = rng.integers(0, 3, size=(2, H, W)).astype(np.int64)
    m[1].flat[0] = IGN
    return m


def _void_only_large():
    m = np.full((2, 40, 70), IGN, dtype=np.int64)          # the only large region is void: every small component is isolated
    rng = np.random.default_rng(2)
    for n in range(2):
        for _ in range(30):
            y, x = rng.integers(1, 38), rng.integers(1, 67)
            m[n, y, x:x + rng.integers(1, 3)] = rng.integers(0, 4)
    return m


MAPS = {
    "1x1": lambda: (_tiny(1, 1), 3, IGN),
    "1x7": lambda: (_tiny(1, 7), 3, IGN),
    "7x1": lambda: (_tiny(7, 1), 3, IGN),
    "solid": lambda: (np.full((2, 67, 131), 4, dtype=np.int64), K, IGN),
    "checkerboard": lambda: (R.checkerboard(37, 53)[None], 2, -100),
    "spiral": lambda: (R.spiral(65, 97)[None], 2, -100),
    "serpentine": lambda: (R.serpentine(65, 97)[None], 2, -100),
    "comb": lambda: (R.comb(70, 130)[None], 2, -100),
    "random_p50": lambda: (R.random_two_class(11, 3, 130, 200, 0.5), 2, -100),
    "random_p41": lambda: (R.random_two_class(12, 3, 130, 200, 0.41), 2, -100),
    "random3_odd": lambda: (np.random.default_rng(4).integers(0, 3, size=(2, 33, 66)).astype(np.int64), 3, -100),
    "blocky": lambda: (_blocky(), K, IGN),
    "speckled": lambda: (R.speckled(6, 2, 70, 150), K, IGN),
    "identical3": lambda: (np.repeat(R.speckled(8, 1, 45, 75), 3, axis=0), K, IGN),
    "void_only_large": lambda: (_void_only_large(), K, IGN),
}


@functools.lru_cache(maxsize=None)
def _map(name):
    m, k, ig = MAPS[name]()
    m.setflags(write=False)
    return m, k, ig


@functools.lru_cache(maxsize=None)
def _ref_labels(name, conn):
    m, k, ig = _map(name)
    return R.connected_components(m, k, ig, conn)


def _same(what, got, want):
    got = got.cpu()
    want = torch.from_numpy(np.ascontiguousarray(want))
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        print(f"{what}: {bad.shape[0]} of {want.numel()} differ; first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()}, "
              f"want {want[tuple(bad[0])].item()}")
    assert got.dtype == want.dtype and torch.equal(got, want), what


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", list(MAPS))
def test_labels_and_areas(name, conn):
    import pytorch_camvid_amd as A
    m, k, ig = _map(name)
    want_l, want_a = _ref_labels(name, conn)
    lab, area = A.connected_components(_t(m), k, ig, conn)
    assert lab.dtype == torch.int32 and area.dtype == torch.int32 and tuple(lab.shape) == m.shape
    _same(f"{name} labels", lab, want_l)
    _same(f"{name} area", area, want_a)
    first = lab.clone()
    lab2, area2 = A.connected_components(_t(m), k, ig, conn)          # the same buffers again: the same bits
    assert lab2.data_ptr() == lab.data_ptr() and torch.equal(lab2, first)
    _same(f"{name} area, second call", area2, want_a)
    if name == "identical3":
        assert torch.equal(lab[0], lab[1]) and torch.equal(lab[0], lab[2]) and torch.equal(area[0], area[2])
        assert int(lab.max()) < m.shape[1] * m.shape[2]
    if name == "1x7":
        one_l, one_a = A.connected_components(_t(m[1]), k, ig, conn)    # [H, W] in, [H, W] out
        assert tuple(one_l.shape) == (1, 7)
        _same("2-D labels", one_l, want_l[1])
        _same("2-D area", one_a, want_a[1])


@pytest.mark.parametrize("mode", ["neighbor", "fill"])
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", list(MAPS))
def test_filtered_map_and_record(name, conn, mode):
    import pytorch_camvid_amd as A
    m, k, ig = _map(name)
    x = _t(m)
    for min_area in MIN_AREAS:
        want, want_rec = R.filter_regions(m, k, ig, conn, min_area, mode)
        rf = A.RegionFilter(min_area, k, ig, conn, mode)
        out = rf(x)
        assert out.dtype == torch.int64 and out.data_ptr() != x.data_ptr()
        _same(f"{name} {mode} min_area {min_area}: map", out, want)
        _same(f"{name} {mode} min_area {min_area}: record", rf.last_record, want_rec)
        if min_area == 1:
            assert torch.equal(out, x)
        if name == "void_only_large" and mode == "neighbor" and min_area >= 9:
            assert want_rec[:, :, 2].max() < 9             # every class component is small: nobody votes, nothing changes
            assert torch.equal(out, x) and torch.equal(rf.last_record[:, :, 7], rf.last_record[:, :, 3])
        assert torch.equal(x.cpu(), torch.from_numpy(np.array(m)))      # the input is left alone


def test_fill_values_and_the_function_form():
    import pytorch_camvid_amd as A
    m, k, ig = _map("speckled")
    x = _t(m)
    for fill in (0, 5, -1, 2 ** 40, ig):
        want, want_rec = R.filter_regions(m, k, ig, 4, 9, "fill", fill_value=fill)
        rf = A.RegionFilter(9, k, ig, 4, "fill", fill_value=fill)
        _same(f"fill {fill}: map", rf(x), want)
        _same(f"fill {fill}: record", rf.last_record, want_rec)
    want, _ = R.filter_regions(m, k, ig, 8, 9, "neighbor")
    _same("remove_small_regions", A.remove_small_regions(x, 9, k, ig, connectivity=8), want)
    _same("remove_small_regions, [H, W]", A.remove_small_regions(x[1], 9, k, ig, connectivity=8), want[1])
    a, b = A.remove_small_regions(x, 9, k, ig), A.remove_small_regions(x, 9, k, ig)
    assert torch.equal(a, b)


def test_vote_slots_past_2_31_elements():
    """8192 x 8192 pixels and 32 classes: the vote slots of a component whose first pixel is the image's last lie past 2^31 elements of
    the workspace (2^26 pixels x 32 classes), the one index of these kernels that leaves 32 bits.  One class everywhere but the first
    pixel (class 31) and the last (class 1), so the expected maps need no restatement: both single pixels go to class 0, the region
    beside them, and the large component spans every tile seam."""
    import pytorch_camvid_amd as A
    H = W = 8192
    m = torch.zeros((1, H, W), device=dev(), dtype=torch.int64)
    m[0, 0, 0], m[0, -1, -1] = 31, 1
    for conn in (4, 8):
        lab, area = A.connected_components(m, 32, -100, conn)
        assert int(lab[0, 0, 0]) == 0 and int(lab[0, -1, -1]) == H * W - 1 and bool(lab.view(-1)[1:-1].eq(1).all())
        assert int(area[0, 0, 0]) == 1 and int(area[0, -1, -1]) == 1 and bool(area.view(-1)[1:-1].eq(H * W - 2).all())
        rf = A.RegionFilter(2, 32, -100, conn)
        out = rf(m)
        assert bool(out.eq(0).all())
        rec = rf.last_record[0].cpu()
        assert rec[0].tolist() == [1, H * W - 2, H * W - 2, 0, 0, 0, 2, 0]
        assert rec[1].tolist() == [1, 1, 1, 1, 1, 1, 0, 0] and rec[31].tolist() == [1, 1, 1, 1, 1, 1, 0, 0] and not rec[2:31].any()
    A.meters._workspaces.clear()                            # 9.5 GB of workspace: not kept for the rest of the session


def test_region_meter_against_the_restatement():
    import pytorch_camvid_amd as A
    pred, label = blocky_maps(21, 2, 96, 128, cell=(7, 9), shift=(1, -1), noise=0.05, void=0.03)
    pred2, label2 = blocky_maps(22, 2, 96, 128, cell=(9, 7), shift=(-2, 1), noise=0.02, void=0.03)
    for conn, mode, min_area in ((4, "neighbor", 9), (8, "fill", 4)):
        meter = A.RegionMeter(K, IGN, min_area=min_area, connectivity=conn, mode=mode)
        meter.update(_t(pred), _t(label))
        meter.update(_t(pred2), _t(label2))
        s = meter.compute()
        rp, rl, hist = (a + b for a, b in zip(R.meter_sums(pred, label, K, IGN, conn, min_area, mode),
                                              R.meter_sums(pred2, label2, K, IGN, conn, min_area, mode)))
        want = A.region_scores(rp, rl, hist, IGN)
        print("fragmentation", s["fragmentation"], "miou_filtered", s["miou_filtered"], "regions", s["regions_pred"], s["regions_label"])
        assert s["images"] == 4
        for key in ("regions_pred", "regions_label", "small_regions_pred"):
            assert s[key].dtype == np.int64 and np.array_equal(s[key], want[key]), key
        for key in ("fragmentation_per_class", "iou_filtered"):
            assert np.array_equal(s[key], want[key], equal_nan=True), key
        assert s["fragmentation"] == want["fragmentation"] and s["miou_filtered"] == want["miou_filtered"]
        cm = A.ConfusionMeter(K, IGN, dev())
        cm.update(A.remove_small_regions(_t(pred), min_area, K, IGN, conn, mode), _t(label))
        cm.update(A.remove_small_regions(_t(pred2), min_area, K, IGN, conn, mode), _t(label2))
        _, cm_iou, cm_miou = cm.compute()
        assert np.array_equal(cm_iou.numpy()[:IGN], s["iou_filtered"][:IGN], equal_nan=True)       # one division per class: the same bits
        # the two means add the same eleven values of [0, 1] in different orders: ten additions each, partial sums below 16, so at
        # most 2^-50 per addition; then one division by 11 and its rounding
        assert abs(cm_miou - s["miou_filtered"]) <= 2 * 10 * 2.0 ** -50 / 11 + 2.0 ** -52
        meter.reset()
        assert meter.compute()["images"] == 0


def test_evaluate_report_with_the_region_meter():
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.get_model("unet", 3, K).to(dev())
    g = torch.Generator().manual_seed(7)
    batches = [(torch.randn(2, 3, 48, 64, generator=g).to(dev()), torch.randint(0, K, (2, 48, 64), generator=g).to(dev()))]
    old = A.evaluate_report(net, batches, K, IGN, boundary=A.BoundaryMeter())
    meter = A.RegionMeter(K, IGN, min_area=4)
    new = A.evaluate_report(net, batches, K, IGN, boundary=(A.BoundaryMeter(), meter))
    assert set(new) == set(old) | {"fragmentation", "miou_filtered", "regions_pred"}
    for key in old:
        a, b = torch.as_tensor(old[key]), torch.as_tensor(new[key])
        assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num()), key
    net.eval()
    with torch.no_grad():
        pred = A.argmax_channels(net(batches[0][0])).cpu().numpy()
    rp, rl, hist = R.meter_sums(pred, batches[0][1].cpu().numpy(), K, IGN, 4, 4, "neighbor")
    want = A.region_scores(rp, rl, hist, IGN)
    assert np.array_equal(new["regions_pred"], want["regions_pred"]) and new["miou_filtered"] == want["miou_filtered"]
    assert new["fragmentation"] == want["fragmentation"] or (np.isnan(new["fragmentation"]) and np.isnan(want["fragmentation"]))
    alone = A.evaluate_report(net, batches, K, IGN, boundary=A.RegionMeter(K, IGN, min_area=4))
    assert alone["miou_filtered"] == new["miou_filtered"] and "bf" not in alone
    for kw in (dict(window=A.SlidingWindow(crop=(32, 32), stride=(16, 32))), dict(tta=A.TestTimeAugmentation(scales=(1.0,), flip=True))):
        rep = A.evaluate_report(net, batches, K, IGN, boundary=A.RegionMeter(K, IGN, min_area=4), **kw)
        assert {"fragmentation", "miou_filtered", "regions_pred"} <= set(rep), kw
