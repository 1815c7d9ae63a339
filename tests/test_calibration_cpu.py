"""The calibration meter and the temperature fit without a GPU: the fp64 restatement (tests/calibration_ref.py) against a plain loop
over pixels and against torch.softmax, the host arithmetic of calibration_scores on hand-made tables, the refusals of the Python
front ends and of the C entry points (no launch), the place of a CalibrationMeter in evaluate_report, and the bracketed Newton rule
on the inputs the GPU tests use."""
import math

import numpy as np
import pytest
import torch

from tests import calibration_ref as R


@pytest.mark.parametrize("name,tau,B", [("small", 1.0, 15), ("two_groups", 0.5, 15), ("wide", 1.0, 10), ("small", 1.7, 1)])
def test_restatement_equals_a_loop_over_pixels(name, tau, B):
    x, t = R.case(name)
    rows, tt = R.rows_of(x), t.reshape(-1)
    C = rows.shape[1]
    p = R.pixel_terms(rows, tt, tau)
    hist, valid, bad, s_nll, s_brier = R.pixel_loop(rows, tt, tau, B)
    v = p["valid"]
    b = R.bins_fp64(p["conf"], B)
    ref = np.zeros((C, B, 3), dtype=np.int64)
    np.add.at(ref[:, :, 0], (p["pred"][v], b[v]), 1)
    np.add.at(ref[:, :, 1], (p["pred"][v], b[v]), p["correct"][v].astype(np.int64))
    np.add.at(ref[:, :, 2], (p["pred"][v], b[v]), np.floor(p["conf"][v] * R.Q_SCALE).astype(np.int64))
    assert np.array_equal(ref[:, :, :2], hist[:, :, :2])
    assert np.abs(ref[:, :, 2] - hist[:, :, 2]).max() <= 2 * max(1, hist[:, :, 0].max())     # exp summed in another order: an ulp per pixel
    assert valid == int(v.sum()) and bad == int(p["bad"].sum()) and bad >= 3 and 0 < valid < len(tt)
    assert abs(p["nll"].sum() - s_nll) <= 1e-12 * s_nll and abs(p["brier"].sum() - s_brier) <= 1e-12 * s_brier
    acc = p["correct"][v].mean()
    assert 0.05 < acc < 0.95, acc                                   # neither all right nor all wrong


def test_restatement_equals_torch_softmax():
    x, t = R.case("two_groups")
    rows, tt = R.rows_of(x), t.reshape(-1)
    for tau in (1.0, 0.37):
        p = R.pixel_terms(rows, tt, tau)
        prob = torch.softmax(torch.from_numpy(rows).double() * tau, dim=1)
        conf, pred = prob.max(dim=1)
        assert np.abs(conf.numpy() - p["conf"]).max() < 1e-14 and np.array_equal(pred.numpy(), p["pred"])
        v = p["valid"]
        tv = torch.from_numpy(tt[v])
        nll = torch.nn.functional.nll_loss(torch.log(prob[v]), tv, reduction="none").numpy()
        assert np.abs(nll - p["nll"][v]).max() < 1e-12
        brier = ((prob[v] - torch.nn.functional.one_hot(tv, rows.shape[1]).double()) ** 2).sum(dim=1).numpy()
        assert np.abs(brier - p["brier"][v]).max() < 1e-14
        assert (p["nll"][~v] == 0).all() and (p["conf"] <= 1.0).all()


def test_float32_binning_rule_and_the_edge_excuse():
    """tables_from_conf is the kernel's float32 rule; on the shared inputs the fp64 reference's own share of confidences within 1e-5 B
    of a bin edge is far inside the 1 % the GPU test allows (expected about 2e-5 B of the valid pixels)."""
    conf = np.array([1.0, 0.2, 0.2000001, 1e-9, 0.5, 1.0 / 3.0], dtype=np.float32)
    hist, valid, bad = R.tables_from_conf(conf, np.zeros(6, dtype=np.int64), np.array([0, 0, 1, 0, R.IGNORE, 99]), 5, 15)
    assert valid == 4 and bad == 1 and hist[0, :, 0].sum() == 4
    assert hist[0, 14, 0] == 1 and hist[0, 2, 0] == 1 and hist[0, 3, 0] == 1 and hist[0, 0, 0] == 1      # 0.2 = 3/15 closes bin 2
    assert hist[0, 14, 2] == 1 << 30 and hist[0, 3, 1] == 0
    for name in R.CASES:
        x, t = R.case(name)
        p = R.pixel_terms(R.rows_of(x), t.reshape(-1))
        for B in (10, 15):
            share = R.near_bin_edge(p["conf"], B)[p["valid"]].mean()
            assert share <= 0.002, (name, B, share)


def test_calibration_scores_on_hand_made_tables():
    import pytorch_camvid_amd as A
    q = lambda c: int(math.floor(c * R.Q_SCALE))
    hist = np.zeros((3, 4, 3), dtype=np.int64)
    hist[0, 3] = [6, 6, 6 * q(0.875)]             # bin 3: 10 pixels, accuracy 0.9, mean confidence (6 * 0.875 + 4 * 1.0) / 10 = 0.925
    hist[1, 3] = [4, 3, 4 * q(1.0)]
    hist[1, 1] = [10, 2, 10 * q(0.5)]             # bin 1: 10 pixels, accuracy 0.2, confidence 0.5
    s = A.calibration_scores(hist, [20, 3, 20 * 0.25, 20 * 0.5])
    assert s["ece"] == pytest.approx(0.5 * 0.025 + 0.5 * 0.3, abs=1e-12) and s["mce"] == pytest.approx(0.3, abs=1e-12)
    assert s["nll"] == 0.25 and s["brier"] == 0.5 and s["accuracy"] == pytest.approx(11 / 20) and s["out_of_range"] == 3
    assert s["mean_confidence"] == pytest.approx((9.25 + 5.0) / 20, abs=1e-12)
    assert list(s["bins"]["count"]) == [0, 10, 0, 10] and np.isnan(s["bins"]["accuracy"][0]) and s["bins"]["accuracy"][3] == 0.9
    assert list(s["count_per_class"]) == [6, 14, 0] and np.isnan(s["ece_per_class"][2])
    assert s["ece_per_class"][0] == pytest.approx(0.125, abs=1e-12)
    assert s["ece_per_class"][1] == pytest.approx((4 * 0.25 + 10 * 0.3) / 14, abs=1e-12)
    # the record as the meter keeps it: an int64 tensor whose last two words are fp64 bit patterns
    rec = torch.zeros(4, dtype=torch.int64)
    rec[0], rec[1] = 20, 3
    rec[2:4].view(torch.float64)[:] = torch.tensor([5.0, 10.0], dtype=torch.float64)
    s2 = A.calibration_scores(torch.from_numpy(hist), rec)
    assert s2["nll"] == 0.25 and s2["brier"] == 0.5 and s2["ece"] == s["ece"]
    # n = 0: every score NaN, no exception
    z = A.calibration_scores(np.zeros((3, 4, 3), dtype=np.int64), [0, 2, 0.0, 0.0])
    assert all(math.isnan(z[k]) for k in ("ece", "mce", "nll", "brier", "accuracy", "mean_confidence")) and z["out_of_range"] == 2
    assert np.isnan(z["ece_per_class"]).all() and z["bins"]["count"].sum() == 0
    # a single full bin, perfectly calibrated
    one = np.zeros((1, 1, 3), dtype=np.int64)
    one[0, 0] = [8, 6, 8 * q(0.75)]
    s = A.calibration_scores(one, [8, 0, 1.0, 1.0])
    assert s["ece"] == 0.0 and s["mce"] == 0.0 and s["accuracy"] == 0.75 and s["mean_confidence"] == 0.75
    with pytest.raises(ValueError):
        A.calibration_scores(np.zeros((3, 4), dtype=np.int64), [0, 0, 0.0, 0.0])


def test_names_are_attributes_and_not_in_all():
    import pytorch_camvid_amd as A
    for name in ("CalibrationMeter", "TemperatureScaler", "calibration_scores", "confidence_map"):
        assert hasattr(A, name) and name not in A.__all__, name


def test_python_refusals():
    import pytorch_camvid_amd as A
    for kw in ({"bins": 0}, {"bins": 65}, {"bins": 2.5}, {"num_classes": 0}, {"num_classes": 129}, {"num_classes": 128, "bins": 17},
               {"temperature": 0.0}, {"temperature": -1.0}, {"temperature": float("inf")}, {"temperature": "hot"}):
        with pytest.raises(ValueError):
            A.CalibrationMeter(device="cpu", **kw)
    A.CalibrationMeter(num_classes=128, bins=16, device="cpu")                     # C * B = 2048 is served
    for kw in ({"iterations": 0}, {"iterations": 2.0}, {"init": 0.0}, {"init": -2.0}, {"init": 100.0}, {"init": 0.001}):
        with pytest.raises(ValueError):
            A.TemperatureScaler(**kw)
    m = A.CalibrationMeter(num_classes=5, bins=15, temperature=2.0, device="cpu")
    assert float(m._tau) == 0.5 and m.hist.shape == (5, 15, 3) and m.hist.dtype == torch.int64 and m.record.shape == (4,)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.update(torch.zeros(1, 5, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.confidence_map(torch.zeros(1, 5, 4, 4))
    s = m.compute()                                                               # an untouched meter: NaN scores, no exception
    assert math.isnan(s["ece"]) and math.isnan(s["nll"]) and s["valid"] == 0


def test_dtype_and_shape_refusals():
    """_check_calib_shapes is what update, confidence_map and fit run right after their device check, before any launch"""
    from pytorch_camvid_amd.functional import _check_calib_shapes
    ok, lab = torch.zeros(1, 5, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    _check_calib_shapes("CalibrationMeter", ok, lab)
    with pytest.raises(ValueError, match="float32"):
        _check_calib_shapes("CalibrationMeter", torch.zeros(1, 5, 4, 4, dtype=torch.float64), lab)
    with pytest.raises(ValueError, match="int64"):
        _check_calib_shapes("CalibrationMeter", ok, torch.zeros(1, 4, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="label size"):
        _check_calib_shapes("CalibrationMeter", ok, torch.zeros(1, 4, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match="N, C, H, W"):
        _check_calib_shapes("confidence_map", torch.zeros(5, 4, 4))
    with pytest.raises(ValueError, match="classes"):
        _check_calib_shapes("confidence_map", torch.zeros(1, 129, 2, 2))


def test_c_entry_points_refuse_bad_arguments_without_a_launch():
    from pytorch_camvid_amd import _lib
    lib = _lib.load()
    err = lambda: lib.cvk_last_error_string()
    P = 4096                                                 # stands for a device pointer: refused calls never dereference it
    assert lib.cvk_calib_accumulate(None, 12, P, None, P, P, P, None, None, 100, 12, 15, 11, None) == -1 and b"null" in err()
    assert lib.cvk_calib_accumulate(P, 12, None, None, P, P, P, None, None, 100, 12, 15, 11, None) == -1 and b"go together" in err()
    assert lib.cvk_calib_accumulate(P, 12, P, None, None, P, P, P, P, 100, 12, 15, 11, None) == -1 and b"go together" in err()
    assert lib.cvk_calib_accumulate(P, 12, None, None, None, None, None, None, None, 100, 12, 15, 11, None) == -1 and b"no map" in err()
    for C, B, what in ((0, 15, b"1 <= C <= 128"), (129, 15, b"1 <= C <= 128"), (12, 0, b"bins <= 64"), (12, 65, b"bins <= 64"),
                       (128, 17, b"exceeds 2048"), (70, 30, b"exceeds 2048")):
        assert lib.cvk_calib_accumulate(P, 128, P, None, P, P, P, None, None, 100, C, B, 11, None) == -1 and what in err(), (C, B, err())
    assert lib.cvk_calib_accumulate(P, 12, P, None, P, P, P, None, None, 0, 12, 15, 11, None) == -1 and b"M > 0" in err()
    assert lib.cvk_calib_accumulate(P, 11, P, None, P, P, P, None, None, 100, 12, 15, 11, None) == -1 and b"stride" in err()
    assert lib.cvk_calib_accumulate(P, 12, None, None, None, None, None, P, None, 100, 129, 15, 11, None) == -1 and b"C <= 128" in err()
    assert lib.cvk_calib_newton_accumulate(P, 12, P, None, P, 100, 12, 11, None) == -1 and b"null" in err()
    assert lib.cvk_calib_newton_accumulate(P, 12, None, P, P, 100, 12, 11, None) == -1 and b"null" in err()
    assert lib.cvk_calib_newton_accumulate(P, 200, P, P, P, 100, 129, 11, None) == -1 and b"C <= 128" in err()
    assert lib.cvk_calib_newton_accumulate(P, 5, P, P, P, 100, 12, 11, None) == -1 and b"stride" in err()
    assert lib.cvk_calib_newton_accumulate(P, 12, P, P, P, -3, 12, 11, None) == -1 and b"M > 0" in err()
    assert lib.cvk_calib_newton_step(None, P, 21, 0, None) == -1 and b"null" in err()
    assert lib.cvk_calib_newton_step(P, None, 21, 0, None) == -1 and b"null" in err()
    assert lib.cvk_calib_newton_step(P, P, 0, 0, None) == -1 and b"log_rows" in err()


def test_a_calibration_meter_is_a_fifth_kind_of_evaluate_report():
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd.functional import _contour_meters
    m = A.CalibrationMeter(device="cpu")
    assert _contour_meters(m) == [m]
    both = _contour_meters((A.BoundaryMeter(), m))
    assert both[1] is m
    with pytest.raises(ValueError, match="two meters of one kind"):
        _contour_meters([m, A.CalibrationMeter(device="cpu")])
    with pytest.raises(ValueError, match="CalibrationMeter"):
        _contour_meters(["nope"])
    with pytest.raises(ValueError, match="tta="):
        A.evaluate_report(None, [], boundary=m, tta=A.TestTimeAugmentation())
    with pytest.raises(ValueError, match="tta="):
        A.evaluate_report(None, [], boundary=(A.BoundaryMeter(), m), tta=A.TestTimeAugmentation())


@pytest.mark.parametrize("name", ["two_groups", "small", "wide", "many_groups"])
def test_newton_restatement_converges_and_honours_the_bracket(name):
    x, t = R.case(name)
    rows, tt = R.rows_of(x), t.reshape(-1)
    log = R.newton_fit([(rows, tt)], iterations=20)
    assert log.shape == (21, 8)
    assert (log[:, 0] >= R.TAU_LO).all() and (log[:, 0] <= R.TAU_HI).all()
    assert (np.diff(log[:, 6]) >= 0).all() and (np.diff(log[:, 7]) <= 0).all() and (log[:, 6] < log[:, 7]).all()
    inside = (log[:-1, 5] >= log[:-1, 6]) & (log[:-1, 5] <= log[:-1, 7])       # after rounding to float32 an end may be met, not passed
    assert inside.all()
    assert (log[:-1, 5] == log[:-1, 5].astype(np.float32)).all(), "tau next is a float32 value"
    star = R.minimiser(rows, tt)
    assert R.TAU_LO < star < R.TAU_HI and abs(log[-1, 0] - star) <= 2e-7 * star, (log[-1, 0], star)
    n, L, g, h = R.newton_sums(rows, tt, star)
    assert h >= 0.01 and abs(g) < 1e-10, (g, h)            # the curvature the GPU test's bound of the fitted tau needs
    assert log[-1, 2] - L <= 1e-12 and log[-1, 5] == log[-1, 0]
    # the scaled problem has the scaled answer
    star2 = R.minimiser(2.0 * rows.astype(np.float64), tt)
    assert abs(star2 - 0.5 * star) <= 1e-11 * star


def test_newton_rule_on_a_separable_set_and_on_nothing():
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((200, 4)).astype(np.float32)
    tt = rows.argmax(axis=1)
    log = R.newton_fit([(rows, tt)], iterations=20)          # labels = arg-max: the NLL decreases in tau all the way
    assert (log[:, 3] < 0).all() and log[-1, 7] == R.TAU_HI and (np.diff(log[:, 0]) > 0).all()
    assert R.TAU_HI * (1 - 1e-3) <= log[-1, 0] <= R.TAU_HI    # Newton steps grow tau geometrically, then the bracket is halved
    assert R.minimiser(rows, tt) == R.TAU_HI
    # with a margin d between the label's logit and the rest the NLL falls like exp(-tau d) and a Newton step is about 1 / d: still
    # upwards every iteration and never past the bracket, but 20 iterations do not reach its end
    wide = rows.copy()
    wide[np.arange(200), tt] += 0.5
    log = R.newton_fit([(wide, tt)], iterations=20)
    assert (log[:, 3] < 0).all() and log[-1, 7] == R.TAU_HI and (np.diff(log[:, 0]) > 0).all() and log[-1, 0] < R.TAU_HI * (1 - 1e-3)
    # h too small: the geometric mean of the bracket; a candidate outside the bracket likewise
    assert R.newton_rule(1.0, R.TAU_LO, R.TAU_HI, 10, -1.0, 0.0) == (8.0, 1.0, R.TAU_HI)
    assert R.newton_rule(1.0, R.TAU_LO, R.TAU_HI, 10, 1.0, 0.001) == (0.125, R.TAU_LO, 1.0)
    assert R.newton_rule(1.0, 0.5, 2.0, 10, 0.25, 1.0) == (0.75, 0.5, 1.0)
    assert R.newton_rule(1.0, 0.5, 2.0, 0, float("nan"), float("nan")) == (1.0, 0.5, 2.0)
    empty = R.newton_fit([(rows, np.full(200, R.IGNORE))], iterations=3)
    assert (empty[:, 0] == 1.0).all() and (empty[:, 1] == 0).all()
