"""The boundary F1 measure on the GPU: cvk_boundary_counts / cvk_boundary_map at the C ABI against the numpy restatement of
tests/boundary_ref.py (integer counts, compared exactly), at the shapes where a tiled kernel can go wrong, and cvk.BoundaryMeter /
cvk.label_boundaries / evaluate_report(boundary=) end to end.  Every comparison prints its counts before it asserts."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import boundary_ref as R

pytestmark = pytest.mark.gpu

K, IGN = 12, 11
R2S = (0, 1, 2, 5, 16, 20, 81, 256)


def dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _raw_counts(pred, label, r2, K=K, ignore=IGN, into=None):
    """cvk_boundary_counts on numpy int64 maps [N,H,W] -> (counts int64 [N,4,K] on the host, the device buffer)."""
    import pytorch_camvid_amd as A
    lib = A.load_library()
    p, l = torch.from_numpy(pred).to(dev()), torch.from_numpy(label).to(dev())
    N, H, W = pred.shape
    out = torch.zeros((N, 4, K), device=dev(), dtype=torch.int64) if into is None else into
    rc = lib.cvk_boundary_counts(p.data_ptr(), l.data_ptr(), out.data_ptr(), N, H, W, K, ignore, r2, _stream())
    assert rc == 0, lib.cvk_last_error_string()
    return out.cpu(), out


def _raw_map(x, void_from, K=K, ignore=IGN):
    import pytorch_camvid_amd as A
    lib = A.load_library()
    m = torch.from_numpy(x).to(dev())
    v = None if void_from is None else torch.from_numpy(void_from).to(dev())
    N, H, W = x.shape
    out = torch.full((N, H, W), 77, device=dev(), dtype=torch.uint8)
    rc = lib.cvk_boundary_map(m.data_ptr(), None if v is None else v.data_ptr(), out.data_ptr(), N, H, W, K, ignore, _stream())
    assert rc == 0, lib.cvk_last_error_string()
    return out.cpu()


def _same_counts(tag, got, want):
    """Prints both count tables summed over classes and how many entries differ, then asserts exact equality."""
    want = torch.as_tensor(want)
    diff = int((got != want).sum())
    print(f"{tag}: {diff} of {want.numel()} counts differ; kernel {got.sum(dim=2).tolist()}, reference {want.sum(dim=2).tolist()}")
    assert got.dtype == torch.int64 and torch.equal(got, want), (tag, diff)


@functools.lru_cache(maxsize=None)
def _maps(H, W, seed=0):
    """Three different blocky images of one size (small images get small cells, so that they hold boundaries at all)."""
    cell = (7, 9) if H >= 16 and W >= 16 else (2, 3)
    return R.blocky_maps(100 * H + W + seed, 3, H, W, cell=cell)


@functools.lru_cache(maxsize=None)
def _ref_counts(H, W, r2):
    """The reference counts of _maps(H, W), image by image: each image alone, so nothing of its neighbours in the batch can enter."""
    pred, label = _maps(H, W)
    return np.concatenate([R.counts(pred[n:n + 1], label[n:n + 1], K, IGN, r2) for n in range(3)])


# 1x1; smaller than any tile and halo; one past 32 and 64 either way; the prototype's blocky size; odd widths, several tiles, rows that
# are not 16-byte aligned
SHAPES = [(1, 1), (5, 7), (33, 65), (65, 33), (37, 70), (45, 83), (67, 131)]


@pytest.mark.parametrize("H,W", SHAPES)
def test_counts_match_the_reference(H, W):
    pred, label = _maps(H, W)
    for r2 in R2S:                                             # r2 256 on every shape: the disc is wider than the small images
        got, _ = _raw_counts(pred, label, r2)
        _same_counts(f"{H}x{W} r2 {r2}", got, _ref_counts(H, W, r2))


@pytest.mark.parametrize("H,W", SHAPES)
def test_boundary_maps_match_the_reference(H, W):
    pred, label = _maps(H, W)
    for tag, got, want in (("label", _raw_map(label, None), R.boundary_map(label, label, K, IGN)),
                           ("label, void_from itself", _raw_map(label, label), R.boundary_map(label, label, K, IGN)),
                           ("prediction", _raw_map(pred, label), R.boundary_map(pred, label, K, IGN)),
                           ("prediction alone", _raw_map(pred, None), R.boundary_map(pred, pred, K, IGN))):
        diff = int((got.numpy() != want).sum())
        print(f"{H}x{W} {tag}: {diff} of {want.size} bytes differ, {int((want != R.NONE).sum())} boundary pixels")
        assert diff == 0, tag


def test_the_blocky_cases_discriminate():
    """On the reference's own counts: every class that occurs has boundary pixels in both maps, and at r2 0 / 2 / 5 the matched counts
    of at least three classes in four lie strictly between none and all: a kernel matching everything, nothing, or a pixel too far fails."""
    pred, label = _maps(37, 70)
    present = [k for k in range(K) if k != IGN and ((label == k).any() or (pred == k).any())]
    for r2 in (0, 2, 5):
        c = _ref_counts(37, 70, r2).sum(axis=0)
        assert present and all(c[0, k] > 0 and c[2, k] > 0 for k in present)
        strictly = [k for k in present if 0 < c[1, k] < c[0, k] and 0 < c[3, k] < c[2, k]]
        print(f"37x70 r2 {r2}: matched {c[1].sum()} of {c[0].sum()} and {c[3].sum()} of {c[2].sum()}; strictly between in {len(strictly)} of {len(present)} classes")
        assert len(strictly) * 4 >= len(present) * 3
        assert not np.array_equal(_ref_counts(37, 70, r2), _ref_counts(37, 70, {0: 1, 2: 4, 5: 8}[r2]))       # the next disc differs


@pytest.mark.parametrize("Rr", [1, 2, 4, 9, 16])
def test_pairs_across_every_tile_seam(Rr):
    """67x131 under any tile of 32 / 64 pixels has seams at rows 32, 64 and columns 64, 128.  A lone label pixel and a lone prediction
    pixel of one class straddle each seam at offset (0, R) or (R, 0): matched at r2 = R^2, not at R^2 - 1."""
    H, W = 67, 131
    label = np.zeros((1, H, W), dtype=np.int64)
    pred = np.zeros((1, H, W), dtype=np.int64)
    cls = 1
    for s, y in ((64, 10), (128, 50)):                         # columns: offset (0, R)
        x1 = min(s - (Rr + 1) // 2 + Rr, W - 1)
        x0 = x1 - Rr
        assert x0 < s <= x1
        label[0, y, x0], pred[0, y, x1] = cls, cls
        cls += 1
    for s, x in ((32, 20), (64, 100)):                         # rows: offset (R, 0)
        y1 = min(s - (Rr + 1) // 2 + Rr, H - 1)
        y0 = y1 - Rr
        assert y0 < s <= y1
        label[0, y0, x], pred[0, y1, x] = cls, cls
        cls += 1
    for r2, m in ((Rr * Rr, 1), (Rr * Rr - 1, 0)):
        got, _ = _raw_counts(pred, label, r2)
        _same_counts(f"seams R {Rr} r2 {r2}", got, R.counts(pred, label, K, IGN, r2))
        print(f"  classes 1..4: {got[0, :, 1:5].t().tolist()}")
        assert got[0, :, 1:5].t().tolist() == [[1, m, 1, m]] * 4


def test_the_entry_point_adds_and_repeats_bitwise():
    pred, label = _maps(45, 83)
    once, buf = _raw_counts(pred, label, 5)
    twice, _ = _raw_counts(pred, label, 5, into=buf)
    again, _ = _raw_counts(pred, label, 5)
    print(f"once {once.sum().item()}, twice into one buffer {twice.sum().item()}, a second run {again.sum().item()}")
    assert once.sum() > 0 and torch.equal(twice, 2 * once) and torch.equal(again, once)


def test_out_of_range_values_and_predicted_ignore():
    pred, label = (a.copy() for a in _maps(45, 83))
    rng = np.random.default_rng(7)
    bad_p = np.array([-3, -1, 2 ** 32 + 1, 2 ** 32 + IGN, 200, IGN, K, 2 ** 63 - 1, -2 ** 63], dtype=np.int64)
    bad_l = np.array([200, -1, 2 ** 32 + 5, 2 ** 32 + IGN, K], dtype=np.int64)
    sel = rng.random(pred.shape) < 0.04
    pred[sel] = bad_p[rng.integers(0, len(bad_p), size=int(sel.sum()))]
    sel = rng.random(label.shape) < 0.02
    label[sel] = bad_l[rng.integers(0, len(bad_l), size=int(sel.sum()))]
    for r2 in (0, 5, 20):
        got, _ = _raw_counts(pred, label, r2)
        _same_counts(f"out of range, r2 {r2}", got, R.counts(pred, label, K, IGN, r2))
    assert np.array_equal(_raw_map(pred, label).numpy(), R.boundary_map(pred, label, K, IGN))
    assert np.array_equal(_raw_map(label, None).numpy(), R.boundary_map(label, label, K, IGN))
    got, _ = _raw_counts(pred, label, 5, K=3, ignore=-100)    # few classes, an ignore index that is no class
    _same_counts("K 3, ignore -100", got, R.counts(pred, label, 3, -100, 5))
    torch.cuda.synchronize()                                   # nothing faulted behind the results


HAND = [  # name, label edits, prediction edits on a 9x9 map of class 0, r2, {class: [nP, mP, nG, mG]}
    ("one class", [], [], 5, {0: [0, 0, 0, 0]}),
    ("offset (1, 2) at r2 4", [((3, 3), 2)], [((4, 5), 2)], 4, {2: [1, 0, 1, 0]}),
    ("offset (1, 2) at r2 5", [((3, 3), 2)], [((4, 5), 2)], 5, {2: [1, 1, 1, 1]}),
    ("class only in the prediction", [], [((4, 4), 5)], 2, {5: [1, 0, 0, 0], 0: [4, 0, 0, 0]}),
    ("predicted ignore index", [], [((4, 4), IGN)], 0, {0: [4, 0, 0, 0], IGN: [0, 0, 0, 0]}),
    ("label 200, prediction -3", [((2, 2), 200)], [((6, 6), -3)], 1, {0: [4, 0, 4, 0]}),
]


@pytest.mark.parametrize("name,ledit,pedit,r2,want", HAND, ids=[h[0] for h in HAND])
def test_hand_worked_cases(name, ledit, pedit, r2, want):
    label = np.zeros((1, 9, 9), dtype=np.int64)
    pred = np.zeros((1, 9, 9), dtype=np.int64)
    for (y, x), v in ledit:
        label[0, y, x] = v
    for (y, x), v in pedit:
        pred[0, y, x] = v
    got, _ = _raw_counts(pred, label, r2)
    _same_counts(name, got, R.counts(pred, label, K, IGN, r2))
    for c, col in want.items():
        assert got[0, :, c].tolist() == col, (name, c, got[0, :, c].tolist())


def test_void_stripe_on_the_device():
    label = np.zeros((1, 5, 7), dtype=np.int64)
    label[0, :, 3] = IGN
    label[0, :, 4:] = 1
    pred = label.copy()
    pred[0, :, 3] = 0
    got, _ = _raw_counts(pred, label, 4)
    print(f"void stripe: {got.sum().item()} boundary pixels")
    assert not got.any() and (_raw_map(pred, label) == 255).all() and (_raw_map(label, None) == 255).all()


def test_meter_over_batches_of_two_sizes():
    import pytorch_camvid_amd as A
    b1, b2 = R.blocky_maps(11, 2, 37, 70), R.blocky_maps(12, 3, 45, 83)
    for kw, r2s in (({"tolerance": 0.05}, (15, 22)), ({"radius2": 5}, (5, 5))):
        if "tolerance" in kw:
            assert (A.boundary_tolerance(37, 70, 0.05), A.boundary_tolerance(45, 83, 0.05)) == r2s
        meter = A.BoundaryMeter(K, IGN, **kw)
        for _ in range(2):                                     # reset() starts over
            meter.reset()
            for pred, label in (b1, b2):
                meter.update(torch.from_numpy(pred).to(dev()), torch.from_numpy(label).to(dev()))
        want = np.concatenate([R.counts(*b1, K, IGN, r2s[0]), R.counts(*b2, K, IGN, r2s[1])])
        got = meter.counts()
        assert tuple(got.shape) == (5, 4, K) and not got.is_cuda
        _same_counts(f"meter {kw}", got, want)
        s, ref, loops = meter.compute(), A.boundary_scores(want, IGN), R.scores(want, IGN)
        print(f"  bf {s['bf']!r} (loops {loops['bf']!r}), pooled {s['pooled']!r}, images {s['images']}")
        assert set(s) == {"bf", "bf_per_class", "precision", "recall", "pooled", "images"} and s["images"] == 5
        assert s["bf"] == ref["bf"] and s["pooled"] == ref["pooled"] and 0.0 < s["bf"] < 1.0
        assert abs(s["bf"] - loops["bf"]) < 1e-15 and abs(s["pooled"] - loops["pooled"]) < 1e-15
        for k in ("bf_per_class", "precision", "recall"):
            assert np.array_equal(s[k], ref[k], equal_nan=True) and np.allclose(s[k], loops[k], rtol=0, atol=1e-15, equal_nan=True), k
        assert math.isnan(s["bf_per_class"][IGN])
    pred, label = (torch.from_numpy(a).to(dev()) for a in b1)
    assert torch.equal(A.label_boundaries(label).cpu(), torch.from_numpy(R.boundary_map(b1[1], b1[1], K, IGN)))
    assert torch.equal(A.label_boundaries(pred, void_from=label).cpu(), torch.from_numpy(R.boundary_map(b1[0], b1[1], K, IGN)))
    strided = torch.stack([pred, pred], dim=-1)[..., 0]        # a view that is not contiguous
    m2 = A.BoundaryMeter(K, IGN, radius2=5)
    m2.update(strided, label)
    _same_counts("strided prediction", m2.counts(), R.counts(*b1, K, IGN, 5))
    with pytest.raises(ValueError):
        m2.update(pred.int(), label.int())
    with pytest.raises(ValueError):
        m2.update(pred, label[:, :, :-1])
    with pytest.raises(ValueError):
        m2.update(pred.cpu(), label)


def _report_batches():
    """Two batches at the smallest size the sliding-window evaluation tests run (2x3x40x56), with blocky masks holding void pixels."""
    g = torch.Generator().manual_seed(41)
    out = []
    for i in range(2):
        _, label = R.blocky_maps(50 + i, 2, 40, 56)
        out.append((torch.randn((2, 3, 40, 56), generator=g).to(dev()), torch.from_numpy(label).to(dev())))
    return out


def _same_report(a, b):
    assert set(a) == set(b), (set(a), set(b))
    for k in a:
        if k == "iou":
            assert torch.equal(torch.isnan(a[k]), torch.isnan(b[k])) and torch.equal(torch.nan_to_num(a[k]), torch.nan_to_num(b[k]))
        else:
            assert a[k] == b[k], (k, a[k], b[k])


def test_evaluate_report_with_a_boundary_meter():
    import pytorch_camvid_amd as A
    torch.manual_seed(42)
    net = A.UNet(3, 12).to(dev()).eval()
    batches = _report_batches()
    sw = A.SlidingWindow(crop=(32, 48), stride=(8, 8))
    tta = A.TestTimeAugmentation(scales=(1.0, 1.25), flip=True)
    with torch.no_grad():
        preds = {"plain": [A.argmax_channels(net(x)) for x, _ in batches], "window": [sw(net, x)[1].clone() for x, _ in batches],
                 "tta": [tta(net, x)[1].clone() for x, _ in batches]}
    meter = A.BoundaryMeter(K, IGN, radius2=2)
    meter.update(batches[0][1], batches[0][1])                 # left-over state: evaluate_report resets the meter
    for path, kw in (("plain", {}), ("window", {"window": sw}), ("tta", {"tta": tta})):
        base = A.evaluate_report(net, batches, **kw)
        rep = A.evaluate_report(net, batches, boundary=meter, **kw)
        want = np.concatenate([R.counts(p.cpu().numpy(), m.cpu().numpy(), K, IGN, 2) for p, (_, m) in zip(preds[path], batches)])
        _same_counts(f"evaluate_report {path}", meter.counts(), want)
        ref = A.boundary_scores(want, IGN)
        print(f"  bf {rep['bf']!r}, from the reference counts {ref['bf']!r}, miou {rep['miou']!r}")
        assert set(base) == {"miou", "precision", "recall", "loss", "accuracy", "iou"} and set(rep) == set(base) | {"bf", "bf_per_class"}
        assert rep["bf"] == ref["bf"] and 0.0 <= rep["bf"] <= 1.0 and abs(rep["bf"] - R.scores(want, IGN)["bf"]) < 1e-15
        assert np.array_equal(rep["bf_per_class"], ref["bf_per_class"], equal_nan=True)
        _same_report({k: v for k, v in rep.items() if k not in ("bf", "bf_per_class")}, base)
    assert not net.training
