"""The references of tests/eval_io_ref.py checked without a GPU, so that tests/test_gpu_eval_io.py compares the kernels with
something that is itself known to be right: the arg-max restatements against torch on the CPU and against the winner each planted
row was built to have, the confusion counts against the oracle and its committed fixture, the float32 restatements of the
preprocess expression against the derived bound, and the argument validation of the six entry points (refused before any launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import np_ops as O
from pytorch_camvid_amd import _lib, functional as F
from tests import eval_io_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P = 4096                              # a fake, 16-byte aligned device address: every call below is refused before a launch
ARGMAX_C = (1, 2, 3, 11, 12, 13, 32, 64, 130)
MEAN_STD = ((F.CAMVID_MEAN, F.CAMVID_STD), ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0.5, -0.25, 0.9), (0.05, 0.05, 2.0)))


# ------------------------------------------------------------------------------------------------ layout
def test_layout_references_on_a_hand_written_case():
    src = np.arange(2 * 3 * 2 * 2, dtype=np.int32).reshape(2, 3, 2, 2) + 1
    got = R.import_nchw_ref(src, 4)
    assert got.shape == (2, 2, 2, 4)
    assert got[1, 0, 1].tolist() == [src[1, 0, 0, 1], src[1, 1, 0, 1], src[1, 2, 0, 1], 0]
    assert np.array_equal(R.export_nchw_ref(got, 3), src)
    assert np.array_equal(R.import_nchw_ref(src[:, ::2, :, 1:], 2), np.ascontiguousarray(src[:, ::2, :, 1:].transpose(0, 2, 3, 1)))
    buf = np.arange(1 * 3 * 4 * 3, dtype=np.int32).reshape(1, 3, 4, 3) + 1
    z = R.zero_frame_ref(buf, 2, 1, 1, 1, 2)
    assert np.array_equal(z[..., 2], buf[..., 2])                                  # channel 2 is outside C = 2
    assert np.array_equal(z[0, 1, 1:3, :2], buf[0, 1, 1:3, :2])                    # the window
    assert int((z[..., :2] != 0).sum()) == 4                                       # and nothing else of channels 0, 1
    assert np.array_equal(R.zero_frame_ref(buf, 3, 0, 0, 3, 4), buf)
    assert not R.zero_frame_ref(buf, 3, 1, 1, 0, 2).any() and not R.zero_frame_ref(buf, 3, 1, 1, 2, 0).any()


# ------------------------------------------------------------------------------------------------ arg-max
@pytest.mark.parametrize("C", ARGMAX_C)
def test_argmax_ref_on_every_planted_case(C):
    base = np.random.default_rng(C).uniform(-4, 4, size=C).astype(np.float32)
    seen = 0
    for name in R.ARGMAX_CASES:
        made = R.argmax_case_row(name, C, base)
        if made is None:
            assert C < 3
            continue
        row, want = made
        seen += 1
        assert R.argmax_ref_loop(row[None])[0] == want, name
        assert R.argmax_ref(row[None])[0] == want, name
        assert int(torch.argmax(torch.from_numpy(row))) == want, name
    assert seen == (len(R.ARGMAX_CASES) if C >= 3 else 11 if C == 2 else 4)


@pytest.mark.parametrize("C", ARGMAX_C)
def test_argmax_ref_against_torch_on_the_gpu_tests_rows(C):
    for M in (1, 255, 256, 257, 4099):
        for ld in (C, C + 3):
            rows, planted = R.argmax_rows(M, C, ld, seed=1000 * C + M)
            assert 0 in planted and M - 1 in planted and (M <= 256 or (255 in planted and 256 in planted))
            if ld > C:
                assert np.isinf(rows[:, C]).all() and np.isnan(rows[:, C + 1]).all()
            got = R.argmax_ref(rows[:, :C])
            assert np.array_equal(got, torch.argmax(torch.from_numpy(rows[:, :C].copy()), dim=-1).numpy())
            if M <= 257:
                assert np.array_equal(got, R.argmax_ref_loop(rows[:, :C]))
            for p, (name, want) in planted.items():
                assert got[p] == want, (p, name)
    if C >= 3:                                            # with 4099 rows every case is planted, and ties occur at random too
        assert {name for name, _ in planted.values()} == set(R.ARGMAX_CASES)
        srt = np.sort(rows[:, :C], axis=1)
        assert int((srt[:, -1] == srt[:, -2]).sum()) > len(planted)


def test_argmax_rows_of_one_row_reach_every_case():
    for k, name in enumerate(R.ARGMAX_CASES):
        rows, planted = R.argmax_rows(1, 12, 15, seed=k, shift=k)
        assert planted == {0: (name, R.argmax_ref(rows[:, :12])[0])}


# ------------------------------------------------------------------------------------------------ confusion counts
def test_confusion_ref_against_the_oracle_and_its_fixture():
    d = np.load(os.path.join(GOLDEN, "miou_intersect_union.npz"))
    for t in "ab":
        preds, labels = d[f"{t}_pred"].astype(np.int64), d[f"{t}_label"].astype(np.int64)
        hist = sum(R.confusion_ref(p, l, 12, 11) for p, l in zip(preds, labels))
        assert np.array_equal(hist[0], d[f"{t}_inter"]) and np.array_equal(hist[1] + hist[2] - hist[0], d[f"{t}_union"])
        acc_o, iou_o, miou_o = O.mean_iou(list(preds), list(labels), 12, 11)
        acc, iou, miou = R.miou_ref(hist, 11)
        assert abs(acc - acc_o) < 1e-12 and abs(miou - miou_o) < 1e-12
        assert np.allclose(iou, iou_o, rtol=0, atol=1e-12, equal_nan=True)
    for K, ignore in ((1, -100), (2, 1), (12, 11), (12, -100), (12, 255), (13, 0), (256, 255)):
        pred, label = R.confusion_inputs(1025, K, ignore, seed=K)
        pred[::7], label[::5] = 255, 255                  # out of range upwards: the oracle's bincount takes no negative value
        pred[::11], label[::13] = K, K
        inter, union, ap, al = O.intersect_and_union(pred, label, K, ignore)
        assert np.array_equal(R.confusion_ref(pred, label, K, ignore), np.stack([inter, ap, al]).astype(np.int64))
        assert np.array_equal(union, ap + al - inter)


def test_confusion_ref_on_hand_counted_pixels():
    K, ign = 4, 3
    pred = np.array([0, 1, 1, 2, 3, 3, -1, 4, R.TWO32 + 1, 1, 2, R.TWO32 + 3], dtype=np.int64)
    label = np.array([0, 1, 2, 3, 3, 0, 1, 2, 1, R.TWO32 + 1, R.TWO32 + 3, 3], dtype=np.int64)
    # kept (label != 3): pixels 0 1 2 5 6 7 8 9 10
    want = np.array([[1, 1, 0, 0],        # pred == label in range: pixels 0 and 1
                     [1, 3, 1, 1],        # pred in range among the kept: 0 | 1 2 9 | 10 | 5
                     [2, 3, 2, 0]])       # label in range among the kept: 0 5 | 1 6 8 | 2 7
    assert np.array_equal(R.confusion_ref(pred, label, K, ign), want)
    acc, iou, miou = R.miou_ref(want, ign)
    assert acc == 2 / 7 and np.allclose(iou[:3], [1 / 2, 1 / 5, 0 / 3]) and abs(miou - (0.5 + 0.2 + 0.0) / 3) < 1e-15
    prec, rec = R.precision_recall_ref(want, ign)
    assert abs(prec - (1 + 1 / 3 + 0) / 3) < 1e-12 and abs(rec - (1 / 2 + 1 / 3 + 0) / 3) < 1e-12
    # nothing counted: NaN mIoU, accuracy 0 and no division error; an absent class is left out of the mean
    acc, iou, miou = R.miou_ref(np.zeros((3, 4), dtype=np.int64), ign)
    assert acc == 0.0 and np.isnan(iou).all() and np.isnan(miou)
    assert abs(R.miou_ref(np.array([[2, 0, 1], [2, 0, 3], [4, 0, 1]]), -100)[2] - (2 / 4 + 1 / 3) / 2) < 1e-15
    # every planted pair of the GPU test: a 64-bit value is no class and not the ignore index
    for K, ignore in ((12, 11), (12, -100), (13, 0)):
        for p, l in R.confusion_planted_pairs(K, ignore):
            h = R.confusion_ref([p], [l], K, ignore)
            assert h[0].sum() == int(p == l and 0 <= p < K and l != ignore)
            assert h[1].sum() == int(0 <= p < K and l != ignore) and h[2].sum() == int(0 <= l < K and l != ignore)
    for kind in ("random", "planted", "constant", "ignored", "absent"):
        pred, label = R.confusion_inputs(1023, 12, 11, 5, kind)
        h = R.confusion_ref(pred, label, 12, 11)
        assert (h[0] <= np.minimum(h[1], h[2])).all()
        assert h[2].sum() == int(((label >= 0) & (label < 12) & (label != 11)).sum())
        assert (kind == "ignored") == (not h.any())
        if kind == "absent":
            assert h[:, 6].sum() == 0 and np.isnan(R.miou_ref(h, 11)[1][6])
        if kind == "constant":
            assert h[:, 0].tolist() == [1023, 1023, 1023]


# ------------------------------------------------------------------------------------------------ preprocess
@pytest.mark.parametrize("mean,std", MEAN_STD)
def test_preprocess_bound_holds_for_both_float32_evaluation_orders(mean, std):
    u8 = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)             # all 256 values x 3 channels
    ref, bound = R.preprocess_ref(u8, mean, std), R.preprocess_bound(u8, mean, std)
    assert ref.dtype == np.float64 and ref.shape == (256, 3)
    m32, s32 = np.float32(mean).astype(np.float64), np.float32(std).astype(np.float64)
    assert np.array_equal(ref[255], (1.0 - m32) / s32) and np.array_equal(ref[0], (0.0 - m32) / s32)
    for fn in (R.preprocess_f32_rounded, R.preprocess_f32_fused):
        got = fn(u8, mean, std)
        assert got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
        assert (np.diff(got.astype(np.float64), axis=0) >= 0).all()                # monotonic in v
    # the bound is not slack by orders of magnitude: some value comes within a factor 12 of it (half a ulp of six)
    worst = np.abs(R.preprocess_f32_rounded(u8, mean, std).astype(np.float64) - ref) / np.maximum(bound, 1e-300)
    assert worst.max() > 1.0 / 24.0


def test_preprocess_all_values_layout():
    img, perms = R.preprocess_all_values()
    assert img.shape == (1, 16, 16, 3) and img.dtype == np.uint8
    flat = img.reshape(256, 3)
    for c in range(3):
        assert np.array_equal(np.sort(flat[:, c]), np.arange(256)) and np.array_equal(flat[:, c], perms[c])
    assert (flat[:, 0] != flat[:, 1]).sum() > 250 and (flat[:, 1] != flat[:, 2]).sum() > 250 and (flat[:, 0] != flat[:, 2]).sum() > 250


# ------------------------------------------------------------------------------------------------ argument validation
def _refused(rc, name):
    """a non-zero status whose message names the entry point"""
    msg = _lib.load().cvk_last_error_string()
    return rc != 0 and msg is not None and name in msg


def test_import_export_argument_validation_without_gpu():
    lib = _lib.load()
    imp, exp = lib.cvk_import_nchw, lib.cvk_export_nchw
    #           src   sN   sC  sH sW dst  ld N  C  H  W  stream
    assert _refused(imp(None, 105, 35, 7, 1, P, 4, 2, 3, 5, 7, None), b"cvk_import_nchw")
    assert _refused(imp(P, 105, 35, 7, 1, None, 4, 2, 3, 5, 7, None), b"cvk_import_nchw")
    for N, C, H, W in ((0, 3, 5, 7), (2, 0, 5, 7), (2, 3, 0, 7), (2, 3, 5, 0), (-1, 3, 5, 7), (2, 3, 5, -7)):
        assert _refused(imp(P, 105, 35, 7, 1, P, 4, N, C, H, W, None), b"cvk_import_nchw")
    assert _refused(imp(P, 105, 35, 7, 1, P, 2, 2, 3, 5, 7, None), b"cvk_import_nchw")             # ld < C
    assert _refused(imp(P, 175, 35, 7, 1, P, 4, 2, 5, 5, 7, None), b"cvk_import_nchw")
    #           src   ld dst  dN   dC  dH dW N  C  H  W  stream
    assert _refused(exp(None, 4, P, 105, 35, 7, 1, 2, 3, 5, 7, None), b"cvk_export_nchw")
    assert _refused(exp(P, 4, None, 105, 35, 7, 1, 2, 3, 5, 7, None), b"cvk_export_nchw")
    for N, C, H, W in ((0, 3, 5, 7), (2, 0, 5, 7), (2, 3, 0, 7), (2, 3, 5, 0), (2, -3, 5, 7)):
        assert _refused(exp(P, 4, P, 105, 35, 7, 1, N, C, H, W, None), b"cvk_export_nchw")
    assert _refused(exp(P, 2, P, 105, 35, 7, 1, 2, 3, 5, 7, None), b"cvk_export_nchw")             # ld < C
    assert _refused(exp(P, 0, P, 105, 35, 7, 1, 2, 3, 5, 7, None), b"cvk_export_nchw")


def test_zero_frame_argument_validation_without_gpu():
    lib = _lib.load()
    zf = lib.cvk_zero_frame
    good = _lib.View(P, 5 * 7 * 4, 7 * 4, 4)
    #                view                  N  H  W  C  y0 x0 h  w  stream
    assert _refused(zf(_lib.View(None, 140, 28, 4), 2, 5, 7, 4, 1, 1, 2, 2, None), b"cvk_zero_frame")
    for N, H, W, C in ((0, 5, 7, 4), (2, 0, 7, 4), (2, 5, 0, 4), (2, 5, 7, 0), (2, 5, -7, 4)):
        assert _refused(zf(good, N, H, W, C, 0, 0, 0, 0, None), b"cvk_zero_frame")
    assert _refused(zf(good, 2, 5, 7, 4, 3, 1, 3, 2, None), b"cvk_zero_frame")                     # y0 + h > H
    assert _refused(zf(good, 2, 5, 7, 4, 1, 6, 2, 2, None), b"cvk_zero_frame")                     # x0 + w > W
    assert _refused(zf(good, 2, 5, 7, 4, 1, -1, 2, 2, None), b"cvk_zero_frame")                    # negative x0
    assert _refused(zf(good, 2, 5, 7, 4, -1, 1, 2, 2, None), b"cvk_zero_frame")                    # negative y0
    assert _refused(zf(good, 2, 5, 7, 4, 0, 0, 6, 7, None), b"cvk_zero_frame")


def test_preprocess_argument_validation_without_gpu():
    lib = _lib.load()
    pre = lib.cvk_preprocess_u8
    f3 = ctypes.c_float * 3
    mean, std = f3(*F.CAMVID_MEAN), f3(*F.CAMVID_STD)
    #            src   dst N  H  W  mean  std  stream
    assert _refused(pre(None, P, 2, 5, 7, mean, std, None), b"cvk_preprocess_u8")
    assert _refused(pre(P, None, 2, 5, 7, mean, std, None), b"cvk_preprocess_u8")
    assert _refused(pre(P, P, 2, 5, 7, None, std, None), b"cvk_preprocess_u8")
    assert _refused(pre(P, P, 2, 5, 7, mean, None, None), b"cvk_preprocess_u8")
    for N, H, W in ((0, 5, 7), (2, 0, 7), (2, 5, 0), (2, -5, 7)):
        assert _refused(pre(P, P, N, H, W, mean, std, None), b"cvk_preprocess_u8")
    for off in (4, 8, 12):                                                                          # dst takes 16-byte stores
        assert _refused(pre(P, P + off, 2, 5, 7, mean, std, None), b"cvk_preprocess_u8")
    for c in range(3):
        s = list(F.CAMVID_STD)
        s[c] = 0.0
        assert _refused(pre(P, P, 2, 5, 7, mean, f3(*s), None), b"zero std")
    assert _refused(pre(P, P, 2, 5, 7, mean, f3(0.3, -0.0, 0.3), None), b"zero std")


def test_argmax_and_confusion_argument_validation_without_gpu():
    lib = _lib.load()
    am, cf = lib.cvk_argmax_channels, lib.cvk_confusion_accumulate
    #           logits ld out M     C   stream
    assert _refused(am(None, 12, P, 1024, 12, None), b"cvk_argmax_channels")
    assert _refused(am(P, 12, None, 1024, 12, None), b"cvk_argmax_channels")
    assert _refused(am(P, 12, P, 0, 12, None), b"cvk_argmax_channels")
    assert _refused(am(P, 12, P, -1, 12, None), b"cvk_argmax_channels")
    assert _refused(am(P, 12, P, 1024, 0, None), b"cvk_argmax_channels")
    assert _refused(am(P, 12, P, 1024, -12, None), b"cvk_argmax_channels")
    assert _refused(am(P, 11, P, 1024, 12, None), b"cvk_argmax_channels")                          # ld < C
    #           pred  label hist M    K   ignore stream
    assert _refused(cf(None, P, P, 1024, 12, 11, None), b"cvk_confusion_accumulate")
    assert _refused(cf(P, None, P, 1024, 12, 11, None), b"cvk_confusion_accumulate")
    assert _refused(cf(P, P, None, 1024, 12, 11, None), b"cvk_confusion_accumulate")
    assert _refused(cf(P, P, P, 0, 12, 11, None), b"cvk_confusion_accumulate")
    assert _refused(cf(P, P, P, -5, 12, 11, None), b"cvk_confusion_accumulate")
    for K in (0, -1, 4097):
        assert _refused(cf(P, P, P, 1024, K, 11, None), b"cvk_confusion_accumulate")
