"""Boundary IoU and the trimap bins on the GPU: cvk_cheb_depth / cvk_boundary_iou_counts through cvk.chessboard_depth and
cvk.BoundaryIoUMeter against the brute-force numpy restatement of tests/boundary_iou_ref.py.  Every output is an integer and every
comparison a torch.equal; each prints what differs before it asserts."""
import functools

import numpy as np
import pytest
import torch

from tests import boundary_iou_ref as R
from tests.boundary_ref import blocky_maps

pytestmark = pytest.mark.gpu

K, IGN = 12, 11
SHAPES = ((1, 1, 1), (1, 1, 7), (1, 9, 1), (2, 5, 7), (2, 37, 53), (1, 70, 130), (1, 20, 300), (1, 5, 1100), (3, 96, 128))
WIDTHS = (1, 2, 4, 8)


def dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@functools.lru_cache(maxsize=None)
def _cases(shape):
    """Named (pred, label) int64 [N, H, W] pairs of a shape: blocky maps with shifts of 1 to 3 px and noise, the special maps, and at
    20 x 300 and 5 x 1100 a single run that crosses every chunk edge of its row (256 pixels, 1024 where a thread takes four)."""
    N, H, W = shape
    out = {}
    for i, shift in enumerate(((1, -1), (2, 3), (-3, 1))):
        out[f"blocky{i}"] = blocky_maps(10 + i, N, H, W, cell=(7, 9), shift=shift, noise=0.03, void=0.05)
    for name, (p, l) in R.special_maps(H, W).items():
        out[name] = (np.repeat(p, N, axis=0), np.repeat(l, N, axis=0))
    if W >= 300:
        lab = np.zeros((N, H, W), dtype=np.int64)
        lab[:, :, :3] = 1                                  # one run of class 0 from column 3 to the row's end, across the edges
        lab[:, H // 2, 290] = 2                            # and one pixel that ends it in one row only
        prd = lab.copy()
        prd[:, :, :3] = 0
        for edge in (256, 1024):
            if W > edge + 1:
                prd[:, 3, edge - 1:edge + 1] = 4           # a two-pixel run that straddles the chunk edge
        out["long_run"] = (prd, lab)
    return out


@functools.lru_cache(maxsize=None)
def _ref_depths(shape, name, border, max_depth=254):
    pred, label = _cases(shape)[name]
    return R.depth_maps(pred, label, K, IGN, border, max_depth), R.depth_maps(label, label, K, IGN, border, max_depth)


def _same(tag, got, want):
    want = torch.as_tensor(want)
    got = got.cpu()
    diff = int((got != want).sum()) if got.shape == want.shape else -1
    print(f"{tag}: {diff} of {want.numel()} entries differ")
    assert got.dtype == want.dtype and torch.equal(got, want), (tag, diff)


@pytest.mark.parametrize("border", (False, True))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_codes_and_depths(shape, border):
    import pytorch_camvid_amd as A
    for name, (pred, label) in _cases(shape).items():
        (cP, dP), (cG, dG) = _ref_depths(shape, name, border)
        code, depth = A.chessboard_depth(_t(pred), K, IGN, void_from=_t(label), border=border)
        _same(f"{name} prediction codes", code, cP)
        _same(f"{name} prediction depth", depth, dP)
        code, depth = A.chessboard_depth(_t(label), K, IGN, border=border)
        _same(f"{name} label codes", code, cG)
        _same(f"{name} label depth", depth, dG)


@pytest.mark.parametrize("max_depth", (1, 3, 12))
def test_depth_clamped_to_max_depth(max_depth):
    import pytorch_camvid_amd as A
    shape = (2, 37, 53)
    for name in ("blocky0", "one_class", "void_blocks"):
        pred, label = _cases(shape)[name]
        for border in (False, True):
            (cP, dP), _ = _ref_depths(shape, name, border, max_depth)
            code, depth = A.chessboard_depth(_t(pred), K, IGN, void_from=_t(label), border=border, max_depth=max_depth)
            _same(f"{name} codes", code, cP)
            _same(f"{name} depth clamped to {max_depth} + 1", depth, dP)


def test_one_class_520_saturates():
    """270 k pixels of one class: depth0 is 255 everywhere, depth1 the border term; with max_depth 24 deep pixels store 25."""
    import pytorch_camvid_amd as A
    H = W = 520
    x = torch.full((1, H, W), 3, device=dev(), dtype=torch.int64)
    bt = torch.from_numpy(R.border_term(H, W))[None]
    code, depth = A.chessboard_depth(x, K, IGN, border=False)
    _same("codes", code, torch.full((1, H, W), 3, dtype=torch.uint8))
    _same("depth0", depth, torch.full((1, H, W), 255, dtype=torch.uint8))
    _, depth = A.chessboard_depth(x, K, IGN, border=True)
    _same("depth1", depth, bt.clamp(max=255).to(torch.uint8))
    assert int(depth.max()) == 255 and int(depth[0, 259, 259]) == 255 and int(depth[0, 100, 300]) == 101
    _, depth = A.chessboard_depth(x, K, IGN, border=False, max_depth=24)
    _same("depth0, max_depth 24", depth, torch.full((1, H, W), 25, dtype=torch.uint8))
    _, depth = A.chessboard_depth(x, K, IGN, border=True, max_depth=24)
    _same("depth1, max_depth 24", depth, bt.clamp(max=25).to(torch.uint8))
    m = A.BoundaryIoUMeter(K, IGN, dilation=12, trimap_widths=(24,))
    m.update(x, x)
    band = int((bt <= 12).sum())
    want = torch.zeros((1, 6, K), dtype=torch.int64)
    want[0, :, 3] = torch.tensor([band, band, band, H * W, H * W, H * W])
    _same("counts", m.counts(), want)
    _same("trimap bins", m.trimap_counts(), torch.zeros((1, K, K), dtype=torch.int64))


@functools.lru_cache(maxsize=None)
def _ref_counts(shape, name, d):
    pred, label = _cases(shape)[name]
    return R.counts(pred, label, K, IGN, d)


@functools.lru_cache(maxsize=None)
def _ref_bins(shape, name, widths):
    pred, label = _cases(shape)[name]
    return R.trimap_bins(pred, label, K, IGN, widths)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_counts_and_trimap_bins(shape):
    import pytorch_camvid_amd as A
    N, H, W = shape
    for d in (1, 2, 3, 12):
        if d > 3 and max(H, W) < 2 * d:                    # a band wider than anything the shape can hold
            continue
        widths = WIDTHS if d != 2 else (3,)
        for name, (pred, label) in _cases(shape).items():
            if d == 12 and not name.startswith(("blocky0", "one_class", "void_blocks", "long_run", "bad_pred")):
                continue
            m = A.BoundaryIoUMeter(K, IGN, dilation=d, trimap_widths=widths)
            m.update(_t(pred), _t(label))
            _same(f"{name} d={d} counts", m.counts(), _ref_counts(shape, name, d))
            _same(f"{name} d={d} trimap bins {widths}", m.trimap_counts(), _ref_bins(shape, name, widths))
            if d == 3:                                     # the count pass without trimap bins
                m0 = A.BoundaryIoUMeter(K, IGN, dilation=d)
                m0.update(_t(pred), _t(label))
                _same(f"{name} d={d} counts, no trimap", m0.counts(), _ref_counts(shape, name, d))


def test_thirty_two_classes_and_other_ignore_index():
    import pytorch_camvid_amd as A
    pred, label = blocky_maps(5, 2, 37, 53, K=32, ignore=0, cell=(5, 6), shift=(1, 2), noise=0.05, void=0.05)
    m = A.BoundaryIoUMeter(32, 0, dilation=2, trimap_widths=(1, 2, 3, 4, 5, 6, 7, 8))
    m.update(_t(pred), _t(label))
    _same("counts", m.counts(), R.counts(pred, label, 32, 0, 2))
    _same("trimap bins", m.trimap_counts(), R.trimap_bins(pred, label, 32, 0, (1, 2, 3, 4, 5, 6, 7, 8)))


def test_meter_accumulates_resets_and_repeats():
    import pytorch_camvid_amd as A
    shape = (3, 96, 128)
    pred, label = _cases(shape)["blocky1"]
    p, l = _t(pred), _t(label)
    whole = A.BoundaryIoUMeter(K, IGN, trimap_widths=WIDTHS)
    assert whole.dilation is None and A.boundary_dilation(96, 128) == 3
    whole.update(p, l)
    _same("ratio 0.02 -> d = 3", whole.counts(), _ref_counts(shape, "blocky1", 3))
    parts = A.BoundaryIoUMeter(K, IGN, trimap_widths=WIDTHS)
    parts.update(p[:1], l[:1])
    parts.update(p[1:], l[1:])
    _same("two updates, counts", parts.counts(), whole.counts())
    _same("two updates, trimap bins", parts.trimap_counts(), whole.trimap_counts())
    again = A.BoundaryIoUMeter(K, IGN, trimap_widths=WIDTHS)
    again.update(p, l)
    _same("second run, counts", again.counts(), whole.counts())
    _same("second run, trimap bins", again.trimap_counts(), whole.trimap_counts())
    s, ref = whole.compute(), R.scores(whole.counts().numpy(), IGN)
    assert s["biou"] == ref["biou"] or abs(s["biou"] - ref["biou"]) < 1e-15
    assert np.allclose(s["biou_per_class"], ref["biou_per_class"], rtol=0, atol=1e-15, equal_nan=True) and s["images"] == 3
    tref = R.trimap_scores(whole.trimap_counts().numpy(), WIDTHS, IGN)
    assert np.allclose(s["trimap_miou"], tref["trimap_miou"], rtol=0, atol=1e-15) and s["widths"] == WIDTHS
    whole.reset()
    assert tuple(whole.counts().shape) == (0, 6, K) and int(whole.trimap_counts().sum()) == 0
    whole.update(p[:1], l[:1])
    _same("after reset", whole.counts(), _ref_counts(shape, "blocky1", 3)[:1])


def test_perfect_prediction_scores_one():
    import pytorch_camvid_amd as A
    _, label = _cases((2, 37, 53))["blocky0"]
    l = _t(label)
    m = A.BoundaryIoUMeter(K, IGN, dilation=2, trimap_widths=(1, 3))
    m.update(l, l)
    s = m.compute()
    present = [c for c in range(K) if c != IGN and (label == c).any()]
    assert present and all(s["biou_per_class"][c] == 1.0 for c in present) and s["biou"] == 1.0 and s["biou_image"] == 1.0
    assert all(np.isnan(s["biou_per_class"][c]) for c in range(K) if c not in present)
    assert (s["trimap_accuracy"] == 1.0).all() and (s["trimap_miou"] == 1.0).all()


def test_compute_against_scipy_erosions():
    """Boundary IoU taken directly from scipy erosions with Cheng's zero pad, in float64: the counts are integers, so only the division
    differs."""
    ndi = pytest.importorskip("scipy.ndimage")
    import pytorch_camvid_amd as A
    shape, d = (2, 37, 53), 2
    pred, label = _cases(shape)["blocky1"]
    m = A.BoundaryIoUMeter(K, IGN, dilation=d)
    m.update(_t(pred), _t(label))
    s = m.compute()
    void = label == IGN
    inter, union = np.zeros(K), np.zeros(K)
    for n in range(shape[0]):
        for c in range(K):
            if c == IGN:
                continue
            g, p = (label[n] == c) & ~void[n], (pred[n] == c) & ~void[n]
            bg = g & ~ndi.binary_erosion(g, np.ones((3, 3), dtype=bool), iterations=d, border_value=0)
            bp = p & ~ndi.binary_erosion(p, np.ones((3, 3), dtype=bool), iterations=d, border_value=0)
            inter[c] += (bg & bp).sum()
            union[c] += (bg | bp).sum()
    want = np.where(union > 0, inter / np.maximum(union, 1), np.nan)
    print("boundary IoU per class:", s["biou_per_class"], "scipy:", want)
    assert np.allclose(s["biou_per_class"], want, rtol=0, atol=1e-12, equal_nan=True)
    assert abs(s["biou"] - np.nanmean(want)) < 1e-12


def _batches(seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(2, 3, 32, 48, generator=g).to(dev()), torch.randint(0, K, (2, 32, 48), generator=g).to(dev())) for _ in range(2)]


def test_evaluate_report_with_the_three_meters():
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.get_model("unet", 3, K).to(dev())
    batches = _batches(7)
    plain = A.evaluate_report(net, batches, K, IGN)
    assert set(plain) == {"miou", "precision", "recall", "loss", "accuracy", "iou"}
    two = A.evaluate_report(net, batches, K, IGN, boundary=(A.BoundaryMeter(), A.SurfaceDistanceMeter()))
    assert set(two) == set(plain) | {"bf", "bf_per_class"} | set(A.functional.SURFACE_REPORT_KEYS)
    meter = A.BoundaryIoUMeter(trimap_widths=(1, 2))
    three = A.evaluate_report(net, batches, K, IGN, boundary=(A.BoundaryMeter(), A.SurfaceDistanceMeter(), meter))
    assert set(three) == set(two) | {"biou", "biou_per_class", "trimap_miou"}
    for k in two:
        a, b = torch.as_tensor(two[k]), torch.as_tensor(three[k])
        assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num()), k
    alone = A.evaluate_report(net, batches, K, IGN, boundary=A.BoundaryIoUMeter())
    assert set(alone) == set(plain) | {"biou", "biou_per_class"} and alone["biou"] == three["biou"]
    assert three["biou"] == meter.compute()["biou"] and tuple(meter.counts().shape) == (4, 6, K)
    # the report's numbers are those of the predictions the confusion meter saw
    net.eval()
    with torch.no_grad():
        preds = [A.argmax_channels(net(x)) for x, _ in batches]
    cnt = np.concatenate([R.counts(p.cpu().numpy(), t.cpu().numpy(), K, IGN, A.boundary_dilation(32, 48)) for p, (_, t) in zip(preds, batches)])
    _same("report counts", meter.counts(), cnt)
    for kw in (dict(window=A.SlidingWindow(crop=(32, 32), stride=(16, 16))), dict(tta=A.TestTimeAugmentation(scales=(1.0,), flip=True))):
        rep = A.evaluate_report(net, batches, K, IGN, boundary=A.BoundaryIoUMeter(trimap_widths=(1, 2)), **kw)
        assert {"biou", "biou_per_class", "trimap_miou"} <= set(rep) and len(rep["trimap_miou"]) == 2, kw
    with pytest.raises(ValueError, match="two meters of one kind"):
        A.evaluate_report(net, batches, K, IGN, boundary=(A.BoundaryIoUMeter(), A.BoundaryIoUMeter(dilation=2)))
