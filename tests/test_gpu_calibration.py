"""cvk.CalibrationMeter, cvk.confidence_map and cvk.TemperatureScaler on the device against the fp64 numpy restatement of
include/cvk.h (tests/calibration_ref.py).

Bounds.  conf, and the sums of nll and brier (relative), within 1e-5 of fp64: the project's bound for the fused losses.  The tables are
compared bit for bit with the kernel's binning rule applied on the host to the kernel's own conf map; against the fp64 binning a pixel
may differ only where the fp64 conf * B lies within 1e-5 B of an integer, and at most 1 % of the valid pixels may lie there (the
reference alone: about 2e-5 B of them, tests/test_calibration_cpu.py).  The fit: every log row's NLL, g and h within 1e-5 x (1, s, s^2)
of fp64 at the row's tau, s = the mean of max_c |x_c|; tau next = the restated rule on the kernel's own sums to 1e-12; the fp64 NLL at
the fitted tau exceeds the fp64 minimum by at most (1e-5 s)^2 / (2 h*): an error of 1e-5 s in g moves tau by 1e-5 s / h*.
Every case prints its measured figures before it asserts.  Shapes: tests/calibration_ref.py CASES."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import calibration_ref as R

pytestmark = pytest.mark.gpu

BINS = 15
BOUND = 1e-5


def dev():
    return torch.device("cuda:0")


def nhwc_logits(x, ld=None):
    """float32 [N,C,H,W] numpy -> a device tensor of that logical shape whose memory is NHWC rows of pitch ld (default C: dense)"""
    N, C, H, W = x.shape
    rows = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1)))
    if ld is None:
        return rows.to(dev()).permute(0, 3, 1, 2)
    buf = torch.full((N, H, W, ld), float("nan"), dtype=torch.float32)           # the padding is never read as a class
    buf[..., :C] = rows
    return buf.to(dev())[..., :C].permute(0, 3, 1, 2)


def labels(t):
    return torch.from_numpy(np.array(t)).to(dev())


@functools.lru_cache(maxsize=None)
def reference(name):
    x, t = R.case(name)
    return R.pixel_terms(R.rows_of(x), t.reshape(-1))


def fed_meter(name, ld=None, temperature=None, scale=None, maps=False):
    import pytorch_camvid_amd as A
    x, t = R.case(name)
    if scale is not None:
        x = x * np.float32(scale)
    lg, lab = nhwc_logits(x, ld), labels(t)
    N, C, H, W = x.shape
    meter = A.CalibrationMeter(num_classes=C, ignore_index=R.IGNORE, bins=BINS, temperature=temperature, device=dev())
    conf = torch.empty((N, H, W), device=dev(), dtype=torch.float32) if maps else None
    pred = torch.empty((N, H, W), device=dev(), dtype=torch.int64) if maps else None
    meter.update(lg, lab, conf=conf, pred=pred)
    return meter, lg, lab, conf, pred


def record_numbers(meter):
    r = meter.record.cpu()
    s = r[2:4].view(torch.float64)
    return int(r[0]), int(r[1]), float(s[0]), float(s[1])


@pytest.mark.parametrize("name,ld", [("two_groups", None), ("two_groups", 16), ("small", None), ("wide", None), ("many_groups", None)])
def test_maps_tables_and_sums_against_fp64(name, ld):
    import pytorch_camvid_amd as A
    x, t = R.case(name)
    N, C, H, W = x.shape
    ref = reference(name)
    meter, lg, lab, conf, pred = fed_meter(name, ld, maps=True)
    if ld is not None:
        assert A.functional._as_nhwc(lg)[1] == ld, "the padded buffer was copied: the case would not run at this pitch"
    conf_h, pred_h = conf.cpu().numpy().reshape(-1), pred.cpu().numpy().reshape(-1)
    # 1. conf against fp64, pred against argmax_channels
    err = np.abs(conf_h.astype(np.float64) - ref["conf"]).max()
    print(f"{name} ld={ld}: max |conf - fp64| = {err:.3e}")
    assert err <= BOUND and (conf_h <= 1.0).all()
    assert torch.equal(pred, A.argmax_channels(lg)) and np.array_equal(pred_h, ref["pred"])
    # 2. the tables on the kernel's own conf, bit for bit
    hist, valid, bad = R.tables_from_conf(conf_h, pred_h, t, C, BINS)
    got_valid, got_bad, s_nll, s_brier = record_numbers(meter)
    assert np.array_equal(meter.hist.cpu().numpy(), hist) and got_valid == valid and got_bad == bad and bad >= 3
    assert valid == int(ref["valid"].sum()) and hist[:, :, 0].sum() == valid
    # 3. the binning against fp64: differences only beside a bin edge, and few pixels there
    v = ref["valid"]
    mine = np.clip(np.ceil(conf_h * np.float32(BINS)).astype(np.int64) - 1, 0, BINS - 1)
    differ = (mine != R.bins_fp64(ref["conf"], BINS)) & v
    near = R.near_bin_edge(ref["conf"], BINS, BOUND) & v
    print(f"{name} ld={ld}: {differ.sum()} of {v.sum()} valid pixels binned otherwise than fp64, {near.sum()} beside an edge")
    assert not (differ & ~near).any() and near.sum() <= 0.01 * v.sum()
    # 4. the sums
    e_nll, e_brier = abs(s_nll / ref["nll"].sum() - 1), abs(s_brier / ref["brier"].sum() - 1)
    print(f"{name} ld={ld}: relative error of sum nll {e_nll:.3e}, of sum brier {e_brier:.3e}")
    assert e_nll <= BOUND and e_brier <= BOUND
    s = meter.compute()
    acc = ref["correct"][v].mean()
    assert s["accuracy"] == pytest.approx(acc, abs=1e-12) and 0.05 < acc < 0.95
    assert s["nll"] == s_nll / valid and s["out_of_range"] == bad and abs(s["mean_confidence"] - ref["conf"][v].mean()) <= BOUND
    # 16. confidence_map: the same kernel without tables, bitwise the maps of update; a layout that is copied gives the same
    c2, p2 = A.confidence_map(lg)
    assert torch.equal(c2, conf) and torch.equal(p2, pred)
    c3, p3 = A.confidence_map(lg.contiguous())
    assert torch.equal(c3, conf) and torch.equal(p3, pred)


@pytest.mark.parametrize("name,T", [("many_groups", 0.37), ("small", 0.37), ("many_groups", 3.87), ("wide", 1.0 / 3.0)])
def test_maps_and_tables_at_a_temperature_that_is_no_power_of_two(name, T):
    """tau = 1 / T is not dyadic, so tau x_c is rounded: were the product contracted into the subtraction of the maximum, the maximum's
    own term would not be exp(0) and conf would exceed 1 on sure pixels (T = 0.37 sharpens 3 * randn logits: many of them).  The fp64
    reference takes the float tau the meter holds and does not round z; |z| stays below 64 here, so that costs at most 64 x 2^-24 =
    3.8e-6 in the exponent, inside the 1e-5 bound on conf."""
    import pytorch_camvid_amd as A
    x, t = R.case(name)
    N, C, H, W = x.shape
    meter, lg, lab, conf, pred = fed_meter(name, temperature=T, maps=True)
    tau = float(meter._tau)
    assert tau == float(np.float32(1.0 / T)) and math.frexp(tau)[0] != 0.5
    ref = R.pixel_terms(R.rows_of(x), t.reshape(-1), tau)
    assert np.abs(tau * R.rows_of(x)).max() < 64
    conf_h, pred_h = conf.cpu().numpy().reshape(-1), pred.cpu().numpy().reshape(-1)
    err = np.abs(conf_h.astype(np.float64) - ref["conf"]).max()
    sure = int((ref["conf"] > 1 - 1e-6).sum())
    print(f"{name} T={T:g}: max |conf - fp64| = {err:.3e}, max conf = {conf_h.max():.9g}, {sure} pixels with fp64 conf > 1 - 1e-6")
    assert (conf_h <= 1.0).all() and err <= BOUND
    assert np.array_equal(pred_h, ref["pred"])
    hist, valid, bad = R.tables_from_conf(conf_h, pred_h, t, C, BINS)
    got_valid, got_bad, s_nll, s_brier = record_numbers(meter)
    assert np.array_equal(meter.hist.cpu().numpy(), hist) and got_valid == valid and got_bad == bad
    assert hist[:, :, 2].max() <= hist[:, :, 0].max() * (1 << 30) and (hist[:, :, 2] <= hist[:, :, 0] * (1 << 30)).all()
    e_nll, e_brier = abs(s_nll / ref["nll"].sum() - 1), abs(s_brier / ref["brier"].sum() - 1)
    print(f"{name} T={T:g}: relative error of sum nll {e_nll:.3e}, of sum brier {e_brier:.3e}")
    assert e_nll <= BOUND and e_brier <= BOUND
    c2, p2 = A.confidence_map(lg, temperature=T)
    assert torch.equal(c2, conf) and torch.equal(p2, pred)


def test_planted_pixels():
    import pytorch_camvid_amd as A
    C = 5
    rows = np.full((4, C), -100.0, np.float32)
    rows[0, 2] = 100.0                                        # one class certain: conf == 1, the top bin
    rows[1] = 0.75                                            # all equal: conf = 1/5 = 3/15 closes bin 2; the first class wins
    rows[2] = [-1.0, 2.5, 0.0, 2.5, -3.0]                     # two equal maxima: the first wins
    rows[3] = [0.0, 0.0, 0.0, 0.0, 30.0]
    t = np.array([2, 0, 3, R.IGNORE], np.int64)
    lg, lab = nhwc_logits(rows.reshape(1, 2, 2, C).transpose(0, 3, 1, 2)), labels(t.reshape(1, 2, 2))
    meter = A.CalibrationMeter(num_classes=C, ignore_index=R.IGNORE, bins=BINS, device=dev())
    conf = torch.empty((1, 2, 2), device=dev(), dtype=torch.float32)
    pred = torch.empty((1, 2, 2), device=dev(), dtype=torch.int64)
    meter.update(lg, lab, conf=conf, pred=pred)
    conf_h, pred_h, hist = conf.cpu().numpy().reshape(-1), pred.cpu().numpy().reshape(-1), meter.hist.cpu().numpy()
    assert conf_h[0] == 1.0 and conf_h[1] == np.float32(0.2) and list(pred_h) == [2, 0, 1, 4]
    assert list(hist[2, 14]) == [1, 1, 1 << 30]
    assert list(hist[0, 2]) == [1, 1, int(math.floor(float(np.float32(0.2)) * R.Q_SCALE))]
    assert hist[1, :, 0].sum() == 1 and hist[1, :, 1].sum() == 0 and hist[:, :, 0].sum() == 3 and hist[4].sum() == 0
    assert record_numbers(meter)[:2] == (3, 0)
    with pytest.raises(ValueError, match="5 classes"):
        meter.update(torch.zeros(1, 12, 2, 2, device=dev()), lab)
    # an all-ignored batch: NaN scores, untouched tables
    meter.reset()
    meter.update(lg, torch.full_like(lab, R.IGNORE))
    s = meter.compute()
    assert not meter.hist.any() and not meter.record.any()
    assert all(math.isnan(s[k]) for k in ("ece", "mce", "nll", "brier", "accuracy"))


def test_accumulation_reproducibility_and_power_of_two_temperature():
    import pytorch_camvid_amd as A
    x, t = R.case("many_groups")
    C = x.shape[1]
    whole, lg, lab, _, _ = fed_meter("many_groups")
    # 6. two updates = one update on the concatenation (the first part ends inside a workgroup: 1600 pixels)
    parts = A.CalibrationMeter(num_classes=C, ignore_index=R.IGNORE, bins=BINS, device=dev())
    parts.update(nhwc_logits(x[:1]), labels(t[:1]))
    parts.update(nhwc_logits(x[1:]), labels(t[1:]))
    assert torch.equal(parts.hist, whole.hist)
    a, b = record_numbers(parts), record_numbers(whole)
    print(f"two updates against one: sums differ by {abs(a[2] / b[2] - 1):.3e}, {abs(a[3] / b[3] - 1):.3e} relative")
    assert a[:2] == b[:2] and abs(a[2] / b[2] - 1) <= 1e-12 and abs(a[3] / b[3] - 1) <= 1e-12
    # 7. the same update twice from reset: bitwise, record included
    again = A.CalibrationMeter(num_classes=C, ignore_index=R.IGNORE, bins=BINS, device=dev())
    again.update(lg, lab)
    first_hist, first_record = again.hist.clone(), again.record.clone()
    again.reset()
    again.update(lg, lab)
    assert torch.equal(again.hist, first_hist) and torch.equal(again.record, first_record)
    assert torch.equal(first_hist, whole.hist) and torch.equal(first_record, whole.record)
    # 8. T = 2 on x is T = 1 on x / 2: scaling by a power of two is exact in fp32
    t2 = fed_meter("many_groups", temperature=2.0)[0]
    half = fed_meter("many_groups", scale=0.5)[0]
    assert torch.equal(t2.hist, half.hist) and torch.equal(t2.record, half.record)
    assert not torch.equal(t2.hist, whole.hist)


@functools.lru_cache(maxsize=None)
def fitted(name, scale=1.0):
    import pytorch_camvid_amd as A
    x, t = R.case(name)
    scaler = A.TemperatureScaler(iterations=20, ignore_index=R.IGNORE, device=dev())
    scaler.fit([nhwc_logits(x * np.float32(scale))], [labels(t)])
    return scaler, scaler.log().cpu().numpy()


@pytest.mark.parametrize("name", ["two_groups", "small", "wide"])
def test_fit_rows_rule_and_fitted_tau(name):
    x, t = R.case(name)
    rows, tt = R.rows_of(x), t.reshape(-1)
    scaler, log = fitted(name)
    s = R.logit_scale(rows, tt)
    assert log.shape == (21, 8)
    lo, hi = R.TAU_LO, R.TAU_HI
    worst = [0.0, 0.0, 0.0]
    for k, (tau, n, L, g, h, nxt, row_lo, row_hi) in enumerate(log):
        # 9. the sums at the row's tau
        rn, rL, rg, rh = R.newton_sums(rows, tt, tau)
        assert n == rn and tau == np.float32(tau)
        worst = [max(worst[0], abs(L - rL)), max(worst[1], abs(g - rg) / s), max(worst[2], abs(h - rh) / s ** 2)]
        # 10. the update rule on the kernel's own sums
        if k < 20:
            want, lo, hi = R.newton_rule(tau, lo, hi, n, g, h)
        else:
            want = tau
        assert abs(nxt - want) <= 1e-12 * want and row_lo == lo and row_hi == hi, (k, nxt, want, row_lo, lo, row_hi, hi)
        if k:
            assert tau == log[k - 1, 5]
    print(f"{name}: s = {s:.3f}; worst |NLL - fp64| = {worst[0]:.3e}, |g - fp64| / s = {worst[1]:.3e}, |h - fp64| / s^2 = {worst[2]:.3e}")
    assert worst[0] <= BOUND and worst[1] <= BOUND and worst[2] <= BOUND
    # 11. the fitted tau
    star = R.minimiser(rows, tt)
    _, L_star, _, h_star = R.newton_sums(rows, tt, star)
    assert h_star >= 0.01
    tau = float(scaler.tau)
    assert tau == log[20, 0] and scaler.temperature == 1.0 / tau
    excess = R.newton_sums(rows, tt, tau)[1] - L_star
    print(f"{name}: tau = {tau:.9g}, fp64 minimiser {star:.9g}; NLL excess {excess:.3e}, allowed {(BOUND * s) ** 2 / (2 * h_star):.3e}")
    assert excess <= (BOUND * s) ** 2 / (2 * h_star)
    assert scaler.converged and not scaler.at_bound


def test_fit_known_answers():
    import pytorch_camvid_amd as A
    # 12. the fit on 2 x is half the fit on x
    one, two = float(fitted("two_groups")[0].tau), float(fitted("two_groups", 2.0)[0].tau)
    print(f"tau on x {one:.9g}, on 2 x {two:.9g}: ratio off one half by {abs(2 * two / one - 1):.3e}")
    assert abs(2 * two / one - 1) <= BOUND
    # labels drawn from softmax(x0), logits 4 x0: T is clearly above 1 (about 4), and scaling lowers the ECE
    rng = np.random.default_rng(12)
    N, C, H, W = 2, 12, 19, 27
    x0 = rng.standard_normal((N, C, H, W)).astype(np.float32)
    r = R.rows_of(x0).astype(np.float64)
    p = np.exp(r - r.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    t = np.minimum((np.cumsum(p, axis=1) < rng.random(len(r))[:, None]).sum(axis=1), C - 1).reshape(N, H, W)
    lg, lab = nhwc_logits(4.0 * x0), labels(t)
    scaler = A.TemperatureScaler(iterations=20, ignore_index=R.IGNORE, device=dev()).fit([lg], [lab])
    star = R.minimiser(R.rows_of(4.0 * x0), t.reshape(-1))
    T = scaler.temperature
    print(f"over-confident by 4: fitted T = {T:.4f}, fp64 {1 / star:.4f}")
    assert T > 2.0
    before = A.CalibrationMeter(num_classes=C, ignore_index=R.IGNORE, bins=BINS, device=dev())
    after = A.CalibrationMeter(num_classes=C, ignore_index=R.IGNORE, bins=BINS, temperature=scaler, device=dev())
    by_value = A.CalibrationMeter(num_classes=C, ignore_index=R.IGNORE, bins=BINS, device=dev())
    before.update(lg, lab)
    after.update(lg, lab)
    scaled = scaler(lg)
    assert scaled.stride() == lg.stride()
    # the maps at the fitted (non-dyadic) tau, from the scaler's device value: conf <= 1, within 1e-5 of fp64, tables on the kernel's conf
    tau = float(scaler.tau)
    conf, pred = A.confidence_map(lg, temperature=scaler)
    conf_h, pred_h = conf.cpu().numpy().reshape(-1), pred.cpu().numpy().reshape(-1)
    ref = R.pixel_terms(R.rows_of(4.0 * x0), t.reshape(-1), tau)
    err = np.abs(conf_h.astype(np.float64) - ref["conf"]).max()
    print(f"maps at the fitted tau {tau:.9g}: max |conf - fp64| = {err:.3e}, max conf = {conf_h.max():.9g}")
    assert (conf_h <= 1.0).all() and err <= BOUND and math.frexp(tau)[0] != 0.5
    want = R.tables_from_conf(conf_h, pred_h, t, C, BINS)[0]
    assert np.array_equal(after.hist.cpu().numpy(), want)
    by_value.update(scaled, lab)
    e0, e1, e2 = before.compute()["ece"], after.compute()["ece"], by_value.compute()["ece"]
    print(f"ECE before {e0:.4f}, after {e1:.4f} (on scaler(logits): {e2:.4f})")
    assert e1 < e0 and e2 < e0 and after.compute()["nll"] < before.compute()["nll"]
    assert torch.equal(after.hist.sum(dim=(0, 1))[:2], before.hist.sum(dim=(0, 1))[:2])       # the same pixels, as right as before


def test_fit_on_a_separable_set_ends_at_the_bracket():
    """The rule takes a candidate only strictly inside (lo, hi), and hi stays 64 here, so tau approaches 64 by halvings of the bracket in
    the logarithm and cannot equal it after a finite number of steps: `at_bound` means within 1e-3 relative of the bracket's end, and
    that is what is asserted.  On these logits (labels = the arg-max of 3 * randn, some margins tiny) the fp64 restatement ends at
    63.99; a separable set with a wide margin climbs by about 1 / margin per step and ends short of it with neither flag set
    (tests/test_calibration_cpu.py)."""
    import pytorch_camvid_amd as A
    x, _ = R.case("two_groups")
    t = R.rows_of(x).argmax(axis=1).reshape(x.shape[0], x.shape[2], x.shape[3])
    scaler = A.TemperatureScaler(iterations=20, ignore_index=R.IGNORE, device=dev()).fit([nhwc_logits(x)], [labels(t)])
    log = scaler.log().cpu().numpy()
    tau = float(scaler.tau)
    print(f"separable: tau = {tau:.6f}, last bracket [{log[20, 6]:.6f}, {log[20, 7]:.6f}]")
    assert np.isfinite(log).all() and (log[:, 3] < 0).all() and log[20, 7] == R.TAU_HI
    assert scaler.at_bound and not scaler.converged and R.TAU_HI * (1 - 1e-3) <= tau <= R.TAU_HI


def test_fit_is_reproducible_and_batches_add_up():
    import pytorch_camvid_amd as A
    x, t = R.case("many_groups")
    lg, lab = nhwc_logits(x), labels(t)
    scaler = A.TemperatureScaler(iterations=20, ignore_index=R.IGNORE, device=dev())
    first = scaler.fit([lg], [lab]).log()
    first_tau = scaler.tau.clone()
    again = scaler.fit([lg], [lab]).log()
    assert torch.equal(first, again) and torch.equal(first_tau, scaler.tau)
    split = A.TemperatureScaler(iterations=20, ignore_index=R.IGNORE, device=dev())
    split.fit([nhwc_logits(x[:1]), nhwc_logits(x[1:])], [labels(t[:1]), labels(t[1:])])
    print(f"one batch tau {float(first_tau):.9g}, two batches {float(split.tau):.9g}")
    assert abs(float(split.tau) / float(first_tau) - 1) <= 1e-6
    assert split.log()[20, 1] == first[20, 1]


def test_evaluate_report_feeds_a_calibration_meter():
    import pytorch_camvid_amd as A
    torch.manual_seed(21)
    net = A.UNet(3, 12).to(dev())
    images = torch.randn(2, 3, 48, 64, generator=torch.Generator().manual_seed(22)).to(dev())
    masks = torch.randint(0, 12, (2, 48, 64), generator=torch.Generator().manual_seed(23)).to(dev())
    batches = [(images, masks), (torch.flip(images, dims=(3,)), masks)]
    meter = A.CalibrationMeter(device=dev())
    meter.update(torch.zeros(1, 12, 4, 4, device=dev()), torch.zeros(1, 4, 4, dtype=torch.int64, device=dev()))    # reset must drop this
    net.train()
    rep = A.evaluate_report(net, batches, loss_fn=A.CrossEntropyLoss(ignore_index=11), boundary=(A.BoundaryMeter(), meter))
    assert net.training
    by_hand = A.CalibrationMeter(device=dev())
    net.eval()
    with torch.no_grad():
        for im, m in batches:
            by_hand.update(net(im), m)
    assert torch.equal(meter.hist, by_hand.hist) and torch.equal(meter.record, by_hand.record)
    scores = by_hand.compute()
    for k in ("ece", "mce", "nll", "brier"):
        assert rep[k] == scores[k] and math.isfinite(rep[k]), k
    assert "bf" in rep and rep["nll"] == pytest.approx(rep["loss"], rel=1e-5)          # both are the mean cross-entropy of the labelled pixels
    base = A.evaluate_report(net, batches)
    assert set(rep) - set(base) == {"ece", "mce", "nll", "brier", "bf", "bf_per_class"} and rep["miou"] == base["miou"]
    sw = A.SlidingWindow(crop=(32, 48), stride=(16, 16))
    rep = A.evaluate_report(net, batches, window=sw, boundary=meter)
    by_hand.reset()
    for im, m in batches:
        by_hand.update(A.SlidingWindow(crop=(32, 48), stride=(16, 16)).logits(net, im), m)
    assert torch.equal(meter.hist, by_hand.hist) and rep["ece"] == by_hand.compute()["ece"]
    with pytest.raises(ValueError, match="tta="):
        A.evaluate_report(net, batches, boundary=meter, tta=A.TestTimeAugmentation())
    # fit_network: the logits of one eval-mode forward per batch
    net.train()
    a = A.TemperatureScaler(iterations=5, device=dev()).fit_network(net, batches)
    assert net.training
    net.eval()
    with torch.no_grad():
        kept = [net(im) for im, _ in batches]
    b = A.TemperatureScaler(iterations=5, device=dev()).fit(kept, [m for _, m in batches])
    assert torch.equal(a.log(), b.log()) and a.log().shape == (6, 8)
