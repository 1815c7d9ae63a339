"""Surface distances on the GPU: cvk_surface_distances at the C ABI against the numpy restatement of tests/surface_ref.py (integers,
compared with torch.equal, never with a tolerance), at the shapes where a strip, a row tile or a histogram level can go wrong, and
cvk.surface_distances / cvk.SurfaceDistanceMeter / evaluate_report(boundary=<the meter>) end to end.  Every comparison prints how many entries
differ before it asserts."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import boundary_ref as B
from tests import surface_ref as S

pytestmark = pytest.mark.gpu

K, IGN = 12, 11
PERCENTILES = (0, 50, 95, 100, "97.5")


def dev():
    return torch.device("cuda:0")


def _frac(percentile):
    import pytorch_camvid_amd as A
    return A.surface_percentile(percentile)


def _raw(pred, label, percentile=95, K=K, ignore=IGN, ws=None):
    """cvk_surface_distances on numpy int64 maps [N,H,W] -> (d2 int32 [2,N,H,W], record int64 [N,2,K,8]) on the host.  The workspace
    and both outputs start out as 0xFF bytes: the entry point clears what it needs and writes every output element."""
    import pytorch_camvid_amd as A
    lib = A.load_library()
    p, l = torch.from_numpy(pred).to(dev()), torch.from_numpy(label).to(dev())
    N, H, W = pred.shape
    nbytes = lib.cvk_surface_workspace_bytes(N, H, W, K)
    assert nbytes > 0
    if ws is None:
        ws = torch.empty(nbytes, device=dev(), dtype=torch.uint8)
    assert ws.numel() == nbytes
    ws.fill_(0xFF)
    d2 = torch.full((2, N, H, W), -1, device=dev(), dtype=torch.int32)
    rec = torch.full((N, 2, K, lib.cvk_surface_record_slots()), -1, device=dev(), dtype=torch.int64)
    qnum, qden = _frac(percentile)
    rc = lib.cvk_surface_distances(p.data_ptr(), l.data_ptr(), N, H, W, K, ignore, qnum, qden, ws.data_ptr(), d2.data_ptr(),
                                   rec.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.cvk_last_error_string()
    return d2.cpu(), rec.cpu()


def _same(tag, got, want):
    """got, want = (d2, record): prints how many entries of either differ, then asserts exact equality."""
    want = tuple(torch.as_tensor(w) for w in want)
    nd, nr = int((got[0] != want[0]).sum()), int((got[1] != want[1]).sum())
    ev = int(((want[1][..., 0] > 0) & (want[1][..., 1] > 0)).sum())
    print(f"{tag}: {nd} of {want[0].numel()} d2 entries and {nr} of {want[1].numel()} record entries differ; "
          f"{int((want[0] >= 0).sum())} distances, {ev} evaluated segments, largest d2 {int(want[0].max())}")
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.int64
    assert torch.equal(got[0], want[0]), (tag, nd)
    assert torch.equal(got[1], want[1]), (tag, nr)


def _check(tag, pred, label, percentile=95, K=K, ignore=IGN):
    got = _raw(pred, label, percentile, K, ignore)
    want = S.surface(pred, label, K, ignore, *_frac(percentile))
    _same(tag, got, want)
    return got, want


@functools.lru_cache(maxsize=None)
def _maps(H, W):
    """Three different blocky images of one size (small images get small cells, so that they hold contours at all)."""
    cell = (7, 9) if H >= 16 and W >= 16 else (2, 3)
    return B.blocky_maps(100 * H + W, 3, H, W, cell=cell)


@functools.lru_cache(maxsize=None)
def _ref(H, W, percentile):
    return S.surface(*_maps(H, W), K, IGN, *_frac(percentile))


# 1x1; smaller than a strip; one past the 16-column strip and the 8-row batch of the column walk; one past the 256-pixel row tile; one past
# 32 and 64 either way; odd sizes over several strips and tiles
SHAPES = [(1, 1), (5, 7), (9, 17), (8, 257), (3, 300), (33, 65), (65, 33), (67, 131)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_distances_and_records_match_the_reference(H, W):
    _same(f"{H}x{W}", _raw(*_maps(H, W)), _ref(H, W, 95))


@pytest.mark.parametrize("percentile", PERCENTILES)
def test_percentiles(percentile):
    H, W = 33, 65
    d2, rec = _raw(*_maps(H, W), percentile)
    want = _ref(H, W, percentile)
    _same(f"percentile {percentile}", (d2, rec), want)
    ev = (rec[..., 0] > 0) & (rec[..., 1] > 0)
    assert int(ev.sum()) > 10
    if percentile == 100:
        assert torch.equal(rec[..., 6][ev], rec[..., 2][ev]) and torch.equal(rec[..., 7][ev], rec[..., 2][ev])
    if percentile == 0:
        ref_d2, _ = want
        bP, bG = (B.boundary_map(m, _maps(H, W)[1], K, IGN) for m in _maps(H, W))
        for n, d, c in zip(*np.nonzero(ev.numpy())):
            seg = ref_d2[d, n][(bP, bG)[d][n] == c]
            assert int(rec[n, d, c, 6]) == int(seg.min()) == int(rec[n, d, c, 7]) and int(rec[n, d, c, 4]) == 0


def test_row_search_in_global_memory_when_the_row_does_not_fit_lds():
    """32 classes at W = 520: the row's column distances (4 W C bytes) no longer fit 64 KiB of LDS next to the other tables, the kernel
    searches them where they lie.  W = 370 is the widest row that fits at 32 classes, 371 the first that does not."""
    pred, label = B.blocky_maps(7, 2, 3, 520, K=32, ignore=31, cell=(2, 5), shift=(1, -3))
    _check("3x520, 32 classes", pred, label, 95, K=32, ignore=31)
    for W in (370, 371):
        pred, label = B.blocky_maps(8 + W, 2, 9, W, K=32, ignore=31, cell=(3, 7), shift=(1, 4))
        _check(f"9x{W}, 32 classes", pred, label, 50, K=32, ignore=31)


def test_identical_maps_have_zero_distances():
    import pytorch_camvid_amd as A
    _, label = _maps(33, 65)
    (d2, rec), _ = _check("pred == label", label.copy(), label)
    assert int((d2 > 0).sum()) == 0 and int((d2 == 0).sum()) > 100 and int((d2 == -1).sum()) == 0
    out = A.surface_distance_scores(rec.numpy(), IGN)
    assert out["hd"] == 0.0 and out["hd95"] == 0.0 and out["assd"] == 0.0 and out["images"] == 3 and int(out["unmatched"].sum()) == 0


def _background(N, H, W, c=0):
    return np.full((N, H, W), c, dtype=np.int64)


def test_class_with_a_contour_in_one_map_only():
    import pytorch_camvid_amd as A
    label, pred = _background(1, 20, 30), _background(1, 20, 30)
    label[0, 4:9, 5:11] = 1
    pred[0, 5:10, 6:12] = 1
    pred[0, 14:17, 20:25] = 2                                   # class 2: the prediction alone
    (d2, rec), _ = _check("one map only", pred, label)
    at2 = torch.from_numpy(B.boundary_map(pred, label, K, IGN) == 2)
    assert int(at2.sum()) == 12 and bool((d2[0][at2] == -1).all()) and int((d2 == -1).sum()) == 12
    assert rec[0, 0, 2].tolist() == [12, 0, -1, 0, -1, -1, -1, -1] and rec[0, 1, 2].tolist() == [0, 12, -1, 0, -1, -1, -1, -1]
    meter = A.SurfaceDistanceMeter(K, IGN)
    meter.update(torch.from_numpy(pred).to(dev()), torch.from_numpy(label).to(dev()))
    out = meter.compute()
    assert out["unmatched"].tolist() == [0, 0, 1] + [0] * 9 and out["images"] == 1 and math.isnan(out["hd_per_class"][2])
    assert out["hd"] > 0 and not math.isnan(out["hd_per_class"][1])


@pytest.mark.parametrize("what", ["void", "one class"])
def test_nothing_evaluated(what):
    import pytorch_camvid_amd as A
    label = _background(2, 9, 17, IGN if what == "void" else 3)
    pred = _background(2, 9, 17, 3)
    (d2, rec), _ = _check(what, pred, label)
    assert bool((d2 == -2).all()) and int(rec[..., 0].sum()) == 0
    out = A.surface_distance_scores(rec.numpy(), IGN)
    assert out["images"] == 0 and all(math.isnan(out[k]) for k in ("hd", "hd95", "assd")) and int(out["unmatched"].sum()) == 0


def test_blobs_in_opposite_corners():
    """The search runs the full width and d2 lands in a high bin of the first histogram level."""
    label, pred = _background(1, 40, 300), _background(1, 40, 300)
    label[0, 2:5, 2:5] = 1
    pred[0, 35:38, 295:298] = 1
    for percentile in (50, 95):
        (d2, rec), _ = _check(f"corner blobs, percentile {percentile}", pred, label, percentile)
    assert int(rec[0, 0, 1, 2]) == 33 * 33 + 293 * 293 and int(rec[0, 0, 1, 6]) >> 12 >= 20


def test_rank_edge_cases():
    """Image 0: n = 1 either way.  Image 1: n = 2, both distances equal.  Image 2: two lines, every distance equal."""
    label, pred = _background(3, 24, 20), _background(3, 24, 20)
    label[0, 10, 10] = 1
    pred[0, 10, 14] = 1
    label[1, 10, 10:12] = 1
    pred[1, 20, 10:12] = 1
    label[2, :, 5] = 1
    pred[2, :, 9] = 1
    for percentile in PERCENTILES:
        (d2, rec), _ = _check(f"rank edge cases, percentile {percentile}", pred, label, percentile)
        assert rec[0, 0, 1, [0, 1, 2, 6, 7]].tolist() == [1, 1, 16, 16, 16] and rec[1, 1, 1, [0, 1, 2, 6, 7]].tolist() == [2, 2, 100, 100, 100]
        assert rec[2, 0, 1, [0, 2, 6, 7]].tolist() == [24, 16, 16, 16] and int(rec[2, 0, 1, 3]) == 24 * 4 * 65536


def test_two_clusters_inside_one_top_level_bin():
    """Image 0: distances near 70 and near 80 pixels, d2 in 4096..8191: one bin of the first level, the second level tells them apart."""
    label, pred = _background(2, 64, 200), _background(2, 64, 200)
    label[:, 5:7, 10:13] = 1
    label[:, 50:52, 10:13] = 1
    pred[:, 5:8, 80:84] = 1
    pred[0, 48:52, 90:93] = 1
    pred[1, 48:52, 110:113] = 1                                 # image 1: near 70 and near 100 pixels, two bins of the first level
    for percentile in PERCENTILES:
        (d2, rec), _ = _check(f"two clusters, percentile {percentile}", pred, label, percentile)
    at = d2[0][d2[0] >= 0]
    seg = d2[0, 0][torch.from_numpy(B.boundary_map(pred, label, K, IGN)[0] == 1)]
    assert bool(((seg >> 12) == 1).all()) and len(torch.unique(seg)) > 6 and len(at) > len(seg)


def test_values_that_are_no_class_in_the_prediction():
    pred, label = (m.copy() for m in _maps(33, 65))
    rng = np.random.default_rng(3)
    odd = np.array([-5, -1, 12, 99, IGN, (1 << 32) + 3, -(1 << 40)], dtype=np.int64)
    hit = rng.random(pred.shape) < 0.06
    pred[hit] = odd[rng.integers(0, len(odd), size=int(hit.sum()))]
    assert int(((pred == IGN) & (label != IGN)).sum()) > 5
    _check("no-class values", pred, label)


def test_an_image_scores_in_a_batch_what_it_scores_alone():
    pred, label = _maps(33, 65)
    d2, rec = _raw(pred, label)
    for n in range(3):
        d2n, recn = _raw(pred[n:n + 1], label[n:n + 1])
        assert torch.equal(recn[0], rec[n]) and torch.equal(d2n[:, 0], d2[:, n]), n


def test_two_runs_agree_bit_for_bit_on_a_poisoned_workspace():
    import pytorch_camvid_amd as A
    pred, label = _maps(67, 131)
    ws = torch.empty(A.load_library().cvk_surface_workspace_bytes(3, 67, 131, K), device=dev(), dtype=torch.uint8)
    a = _raw(pred, label, ws=ws)
    b = _raw(pred, label, ws=ws)                               # _raw fills the workspace with 0xFF before every call
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _same("second run", b, _ref(67, 131, 95))


def test_functional_and_meter():
    import pytorch_camvid_amd as A
    (p1, l1), (p2, l2) = _maps(33, 65), _maps(65, 33)
    tp1, tl1, tp2, tl2 = (torch.from_numpy(m).to(dev()) for m in (p1, l1, p2, l2))
    d2, rec = A.surface_distances(tp1, tl1, K, IGN, percentile="97.5")
    assert d2.is_cuda and rec.is_cuda
    _same("surface_distances", (d2.cpu(), rec.cpu()), _ref(33, 65, "97.5"))
    meter = A.SurfaceDistanceMeter(K, IGN)
    assert meter.records().shape == (0, 2, K, 8) and math.isnan(meter.compute()["hd95"])
    meter.update(tp1, tl1)
    meter.update(tp2, tl2)
    meter.update(tp1, tl1)                                      # the kept workspace of the first shape, used again
    want = np.concatenate([_ref(33, 65, 95)[1], _ref(65, 33, 95)[1], _ref(33, 65, 95)[1]])
    got = meter.records()
    print(f"meter: {int((got != torch.from_numpy(want)).sum())} of {want.size} record entries differ")
    assert torch.equal(got, torch.from_numpy(want))
    out, ref = meter.compute(), A.surface_distance_scores(want, IGN)
    print(f"  hd95 {out['hd95']!r}, hd {out['hd']!r}, assd {out['assd']!r}, unmatched {out['unmatched'].tolist()}")
    assert set(out) == {"hd95", "hd", "assd", "hd95_per_class", "hd_per_class", "assd_per_class", "unmatched", "images", "percentile"}
    for k in out:
        assert np.array_equal(out[k], ref[k], equal_nan=True), k
    assert out["images"] == 9 and out["percentile"] == 95.0 and 0 < out["assd"] <= out["hd95"] <= out["hd"]
    meter.reset()
    assert meter.records().shape[0] == 0
    for bad in ((tp1.cpu(), tl1), (tp1, tl2), (tp1.int(), tl1), (tp1[0], tl1[0])):
        with pytest.raises(ValueError):
            meter.update(*bad)
    with pytest.raises(ValueError):
        A.surface_distances(tp1, tl1, 33)


def test_evaluate_report_with_a_surface_meter():
    import pytorch_camvid_amd as A
    torch.manual_seed(42)
    net = A.UNet(3, 12).to(dev()).eval()
    g = torch.Generator().manual_seed(41)
    batches = [(torch.randn((2, 3, 32, 48), generator=g).to(dev()), torch.from_numpy(B.blocky_maps(60 + i, 2, 32, 48)[1]).to(dev()))
               for i in range(2)]
    sw = A.SlidingWindow(crop=(32, 48), stride=(8, 8))
    tta = A.TestTimeAugmentation(scales=(1.0, 1.25), flip=True)
    meter = A.SurfaceDistanceMeter(K, IGN)
    meter.update(batches[0][1], batches[0][1])                  # left-over state: evaluate_report resets the meter
    parent_keys = {"miou", "precision", "recall", "loss", "accuracy", "iou"}
    for path, kw in (("plain", {}), ("window", {"window": sw}), ("tta", {"tta": tta})):
        with torch.no_grad():
            preds = [{"plain": lambda x: A.argmax_channels(net(x)), "window": lambda x: sw(net, x)[1].clone(),
                      "tta": lambda x: tta(net, x)[1].clone()}[path](x) for x, _ in batches]
        base = A.evaluate_report(net, batches, **kw)
        rep = A.evaluate_report(net, batches, boundary=meter, **kw)
        by_hand = A.SurfaceDistanceMeter(K, IGN)
        for p, (_, m) in zip(preds, batches):
            by_hand.update(p, m)
        want = by_hand.compute()
        ref_rec = np.concatenate([S.surface(p.cpu().numpy(), m.cpu().numpy(), K, IGN, 19, 20)[1] for p, (_, m) in zip(preds, batches)])
        print(f"evaluate_report {path}: hd95 {rep['hd95']!r}, hd {rep['hd']!r}, assd {rep['assd']!r}; "
              f"{int((meter.records() != torch.from_numpy(ref_rec)).sum())} record entries differ from the reference")
        assert torch.equal(meter.records(), torch.from_numpy(ref_rec)) and meter.records().shape[0] == 4
        assert set(base) == parent_keys
        assert set(rep) == parent_keys | {"hd95", "hd", "assd", "hd95_per_class", "hd_per_class", "assd_per_class"}
        for k in set(rep) - parent_keys:
            assert np.array_equal(rep[k], want[k], equal_nan=True), k
        for k in parent_keys - {"iou"}:
            assert rep[k] == base[k], k
        assert torch.equal(torch.nan_to_num(rep["iou"]), torch.nan_to_num(base["iou"]))
    bf = A.BoundaryMeter(K, IGN, radius2=2)
    both = A.evaluate_report(net, batches, boundary=(bf, meter))
    alone = A.evaluate_report(net, batches, boundary=bf)
    rep = A.evaluate_report(net, batches, boundary=[meter])
    assert set(both) == set(alone) | set(rep) and both["bf"] == alone["bf"] and both["hd95"] == rep["hd95"] and both["assd"] == rep["assd"]
    assert not net.training
