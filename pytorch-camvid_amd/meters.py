"""Evaluation meters of the hot path on HIP tensors: integer counts on the device, scores in float64 on the host.  The losses are in
losses.py, the inference drivers in inference.py, the evaluation loops in functional.py; every name here is importable from
functional as before.

  ClassFrequencyMeter, class_weights
                    <- median-frequency (SegNet) / ENet class weights from device-side class histograms of the masks
  ConfusionMeter    <- utils.intersect_and_union / mean_iou (utils.py:162-228) accumulated on device, with the
                       np.float crash (utils.py:210) and the per-batch-sum bug of train.py:192-206 not reproduced
                       (SURVEY.md §0.5): IoU = sum(intersection)/sum(union) per class over the whole set.
  BoundaryMeter, label_boundaries, boundary_tolerance, boundary_scores
                    <- the boundary F1 measure (BF score, Csurka et al. BMVC 2013; not in the reference): per-image, per-class
                       contour counts from one launch, scores on the host
  SurfaceDistanceMeter, surface_distances, surface_percentile, surface_distance_scores
                    <- Hausdorff distance, its percentile and the average symmetric surface distance between the same contours
                       (not in the reference): exact integer records per image, direction and class, scores on the host
  BoundaryIoUMeter, chessboard_depth, boundary_dilation, boundary_iou_scores, trimap_scores
                    <- Boundary IoU (Cheng et al. CVPR 2021) and the trimap curve (not in the reference) on a device chessboard
                       depth map: integer counts per image and class, scores on the host
  connected_components, remove_small_regions, RegionFilter, RegionMeter, region_scores
                    <- connected components of a class map (canonical labels and areas from a union-find over tiles) and the
                       removal of small regions (not in the reference); fragmentation and the mIoU after despeckling
  CalibrationMeter, calibration_scores, confidence_map, TemperatureScaler
                    <- expected calibration error, reliability tables, NLL and Brier score of the top-label probability, and
                       temperature scaling (Guo et al. ICML 2017; not in the reference): one pass over the logits per batch into
                       integer tables, and a Newton fit of 1 / T that runs on the device without a host sync

The meters share one front end: `_map_pair` and `_check_classes` (what every update asks of its maps and its class count),
`_workspace` / `_new_workspace` / `_kept` (the device buffers kept per kind of call and shape), `_Parts` (per-image results until the
one host copy) and the host arithmetic of the scores, `_masked_mean`, `_nan_ratio`, `_nan_at`, `_mean_of`.  A meter that
`evaluate_report` takes says what its `update` is fed (`update_takes`: "pred" or "logits") and which keys of its `compute()` go into
the report (`report_keys`).
"""
import numpy as np
import torch

from . import _lib
from ._lib import check
from .losses import _as_nhwc, _stream, EDT_MAX_CLASSES
from .inference import _check_window


def _map_pair(who, pred, label):
    """The check of two int64 maps [N,H,W] on one GPU; returns them contiguous (one map given twice is made contiguous once)."""
    ok = all(isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.dim() == 3 for t in (pred, label))
    if not ok or pred.shape != label.shape or pred.numel() == 0:
        raise ValueError(f"{who}: expected int64 tensors of one shape [N, H, W]")
    if not (pred.is_cuda and label.is_cuda) or pred.device != label.device:
        raise ValueError(f"{who}: expected both tensors on one GPU (no CPU fallback)")
    p = pred.contiguous()
    return p, p if label is pred else label.contiguous()


def _check_classes(who, num_classes, most=32):
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= most:
        raise ValueError(f"{who} serves 1 to {most} classes. Got: {num_classes}")
    return num_classes


_workspaces = {}        # (kind, N, H, W, classes or None, str(device)) -> {"ws": the uint8 workspace, name: a tensor `_kept` made}


def _workspace(kind, N, H, W, C, device):
    return _workspaces.get((kind, N, H, W, C, str(device)))


def _new_workspace(kind, N, H, W, C, device, nbytes, refusal):
    """Fills the cache for one shape.  `nbytes` is what the kind's cvk_*_workspace_bytes returned: <= 0 for a shape it refuses."""
    if nbytes <= 0:
        raise ValueError(refusal)
    ent = _workspaces[(kind, N, H, W, C, str(device))] = {"ws": torch.empty(nbytes, device=device, dtype=torch.uint8)}
    return ent


def _kept(ent, name, shape, dtype):
    """The tensor a workspace entry keeps under `name`, made on first request."""
    t = ent.get(name)
    if t is None:
        t = ent[name] = torch.empty(shape, device=ent["ws"].device, dtype=dtype)
    return t


class _Parts:
    """The per-image int64 device results of a meter's updates, [images of the batch, *tail] each; no host sync until `host()`."""

    def __init__(self, *tail):
        self.tail, self.parts = tail, []

    def append(self, part):
        self.parts.append(part)

    def clear(self):
        self.parts = []

    def host(self):
        """int64 [images, *tail] on the host, in the order of the updates: one device->host copy"""
        if not self.parts:
            return torch.zeros((0,) + self.tail, dtype=torch.int64)
        return (self.parts[0] if len(self.parts) == 1 else torch.cat(self.parts)).cpu()


def _masked_mean(v, ev, axis):
    """the mean of `v` over `axis` where `ev`; NaN where `ev` selects nothing"""
    n = ev.sum(axis=axis)
    return np.divide(np.where(ev, v, 0.0).sum(axis=axis), n, out=np.full(n.shape, np.nan), where=n > 0)


def _nan_ratio(num, den):
    """num / den where den > 0, NaN elsewhere"""
    return np.divide(num, den, out=np.full(den.shape, np.nan), where=den > 0)


def _nan_at(ignore_index, *per_class):
    """NaN at `ignore_index` of the last axis of each array, when it is one of its classes"""
    for a in per_class:
        if ignore_index is not None and 0 <= ignore_index < a.shape[-1]:
            a[..., ignore_index] = np.nan


def _mean_of(v, selected):
    """the mean of the selected values as a float; NaN when none is"""
    return float(v[selected].mean()) if selected.any() else float("nan")


class ConfusionMeter:
    """Device-side accumulation of per-class intersection / prediction / label pixel counts (utils.py:162-190)."""

    def __init__(self, num_classes=12, ignore_index=11, device="cuda"):
        self.num_classes, self.ignore_index = num_classes, ignore_index
        self.hist = torch.zeros((3, num_classes), device=device, dtype=torch.int64)

    def reset(self):
        self.hist.zero_()

    def update(self, pred, label):
        lib = _lib.load()
        p = pred.contiguous(); l = label.contiguous()
        if p.dtype != torch.int64 or l.dtype != torch.int64 or p.shape != l.shape:
            raise ValueError("pred and label must be int64 tensors of the same shape")
        check(lib.cvk_confusion_accumulate(p.data_ptr(), l.data_ptr(), self.hist.data_ptr(), p.numel(), self.num_classes,
                                           self.ignore_index, _stream(p)), "cvk_confusion_accumulate")

    def compute(self):
        """(overall accuracy, per-class IoU tensor, mIoU over the non-ignored classes) — one device->host copy."""
        h = self.hist.cpu().double()
        inter, pred, lab = h[0], h[1], h[2]
        union = pred + lab - inter
        iou = inter / union
        valid = [c for c in range(self.num_classes) if c != self.ignore_index]
        acc = float(inter.sum() / lab.sum().clamp(min=1))
        return acc, iou, float(torch.nanmean(iou[valid]))

    def precision_recall(self):
        """Mean precision and recall over the non-ignored classes (the two extra numbers reference eval.py:70-79 prints;
        legacy/metrics.py:33-57: diag / column sums and diag / row sums of the confusion matrix).  Pixels whose label is
        ignore_index are left out of every count, as in utils.intersect_and_union (utils.py:170-172)."""
        h = self.hist.cpu().double()
        valid = [c for c in range(self.num_classes) if c != self.ignore_index]
        prec = (h[0] / (h[1] + 1e-15))[valid].mean()
        rec = (h[0] / (h[2] + 1e-15))[valid].mean()
        return float(prec), float(rec)


BOUNDARY_MAX_RADIUS2 = 256       # include/cvk.h: cvk_boundary_counts serves squared tolerances up to 16 * 16 pixels


def boundary_tolerance(H, W, tolerance=0.0075):
    """Squared matching distance of the boundary F1 measure for an H x W image, in pixels: floor((tolerance * diagonal)^2), in exact
    rational arithmetic (`tolerance` is read through its decimal string).  The default is 0.75 % of the diagonal (Csurka et al., the
    SegNet paper): 360 x 480 -> 20, 720 x 960 -> 81."""
    from fractions import Fraction
    q = Fraction(str(tolerance))
    if q < 0:
        raise ValueError(f"tolerance must not be negative. Got: {tolerance!r}")
    r2 = (q * q * (int(H) * int(H) + int(W) * int(W))).__floor__()
    if r2 > BOUNDARY_MAX_RADIUS2:
        raise ValueError(f"a tolerance of {tolerance!r} on {H} x {W} pixels is a squared distance of {r2}; the kernel serves at most "
                         f"{BOUNDARY_MAX_RADIUS2} (16 pixels)")
    return int(r2)


def _check_radius2(r2):
    if isinstance(r2, bool) or not isinstance(r2, int) or r2 < 0:
        raise ValueError(f"radius2 must be a non-negative integer. Got: {r2!r}")
    if r2 > BOUNDARY_MAX_RADIUS2:
        raise ValueError(f"radius2 {r2} is above the limit of {BOUNDARY_MAX_RADIUS2} (16 pixels)")
    return r2


def boundary_scores(counts, ignore_index=None):
    """The boundary F1 scores of per-image, per-class counts [images, 4, K] (rows: prediction boundary pixels nP, those matched mP,
    label boundary pixels nG, those matched mG), in float64 on the host.  A class is evaluated in an image iff nP + nG > 0;
    P = mP / nP, R = mG / nG, F = 2 P R / (P + R), each 0 where its denominator is.  Returns
      "bf": the mean over the images with an evaluated class of the image's mean F over its evaluated classes (NaN without one),
      "bf_per_class", "precision", "recall": float64 [K], per class the mean F / P / R over the images where it is evaluated (NaN
          where it never is, and at ignore_index),
      "pooled": the image score of the counts summed over all images,
      "images": how many images had an evaluated class."""
    c = np.asarray(counts, dtype=np.int64)
    if c.ndim != 3 or c.shape[1] != 4:
        raise ValueError(f"expected counts of shape [images, 4, K], got {list(c.shape)}")

    def prf(c4):
        nP, mP, nG, mG = (c4[..., r, :].astype(np.float64) for r in range(4))
        ev = (nP + nG) > 0
        P = np.divide(mP, nP, out=np.zeros_like(nP), where=nP > 0)
        R = np.divide(mG, nG, out=np.zeros_like(nG), where=nG > 0)
        F = np.divide(2.0 * P * R, P + R, out=np.zeros_like(P), where=(P + R) > 0)
        return ev, P, R, F

    ev, P, R, F = prf(c)
    image = _masked_mean(F, ev, 1)                        # [images], NaN where nothing is evaluated
    scored = ~np.isnan(image)
    per_class, prec, rec = _masked_mean(F, ev, 0), _masked_mean(P, ev, 0), _masked_mean(R, ev, 0)
    _nan_at(ignore_index, per_class, prec, rec)
    evp, _, _, Fp = prf(c.sum(axis=0))
    return {"bf": _mean_of(image, scored), "bf_per_class": per_class, "precision": prec, "recall": rec, "pooled": _mean_of(Fp, evp),
            "images": int(scored.sum())}


class BoundaryMeter:
    """Boundary F1 measure (BF score; Csurka et al., BMVC 2013; MATLAB's bfscore) of predictions against labels: per image and class,
    the 4-connected contour pixels of both maps and how many of them have a contour pixel of the same class in the other map within
    the tolerance, counted on the device by one launch per batch (cvk_boundary_counts, exact integers), no host sync until
    `counts()` / `compute()`.  The tolerance is `tolerance` times the image diagonal of each batch (`boundary_tolerance`), or the
    squared pixel distance `radius2`.  Pixels whose label is `ignore_index` are void in both maps."""

    update_takes, report_keys = "pred", ("bf", "bf_per_class")

    def __init__(self, num_classes=12, ignore_index=11, tolerance=0.0075, radius2=None):
        self.num_classes = _check_classes("BoundaryMeter", num_classes)
        self.ignore_index, self.tolerance = int(ignore_index), tolerance
        self.radius2 = None if radius2 is None else _check_radius2(radius2)
        if radius2 is None:
            boundary_tolerance(1, 1, tolerance)           # a bad tolerance fails here, not in the first batch
        self._parts = _Parts(4, self.num_classes)

    def reset(self):
        self._parts.clear()

    def update(self, pred, label):
        p, l = _map_pair("BoundaryMeter.update", pred, label)
        lib = _lib.load()
        N, H, W = p.shape
        r2 = self.radius2 if self.radius2 is not None else boundary_tolerance(H, W, self.tolerance)
        part = torch.zeros((N, 4, self.num_classes), device=p.device, dtype=torch.int64)
        check(lib.cvk_boundary_counts(p.data_ptr(), l.data_ptr(), part.data_ptr(), N, H, W, self.num_classes, self.ignore_index, r2,
                                      _stream(p)), "cvk_boundary_counts")
        self._parts.append(part)

    def counts(self):
        """int64 [images, 4, num_classes] on the host (rows nP, mP, nG, mG), in the order of the updates — one device->host copy."""
        return self._parts.host()

    def compute(self):
        """`boundary_scores` of `counts()`: {"bf", "bf_per_class", "precision", "recall", "pooled", "images"}."""
        return boundary_scores(self.counts().numpy(), self.ignore_index)


def label_boundaries(labels, num_classes=12, ignore_index=11, void_from=None):
    """uint8 [N,H,W]: the class whose 4-connected boundary each pixel of the int64 map `labels` carries under BoundaryMeter's rule, 255
    where it carries none.  `void_from` is the label map whose `ignore_index` pixels are void (for a prediction map); None: the map's
    own.  The kernel shares the rule's device function with the counting kernel."""
    m, v = _map_pair("label_boundaries", labels, labels if void_from is None else void_from)
    _check_classes("label_boundaries", num_classes)
    lib = _lib.load()
    N, H, W = m.shape
    out = torch.empty((N, H, W), device=m.device, dtype=torch.uint8)
    check(lib.cvk_boundary_map(m.data_ptr(), None if void_from is None else v.data_ptr(), out.data_ptr(), N, H, W, int(num_classes),
                               int(ignore_index), _stream(m)), "cvk_boundary_map")
    return out


SURFACE_RECORD_SLOTS = 8         # include/cvk.h: n, m, max d2, Q, k, r, d2_lo, d2_hi
SURFACE_MAX_DENOMINATOR = 10000


def surface_percentile(percentile=95):
    """The percentile of the surface-distance meter as the fraction (qnum, qden) = percentile / 100 in lowest terms, in exact rational
    arithmetic (`percentile` is read through its decimal string, as `boundary_tolerance` reads its tolerance): 95 -> (19, 20),
    "97.5" -> (39, 40).  It must lie in [0, 100] and the denominator must not exceed 10000."""
    from fractions import Fraction
    try:
        if isinstance(percentile, bool):
            raise ValueError
        q = Fraction(str(percentile)) / 100
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"percentile must be a number in [0, 100]. Got: {percentile!r}") from None
    if not 0 <= q <= 1:
        raise ValueError(f"percentile must lie in [0, 100]. Got: {percentile!r}")
    if q.denominator > SURFACE_MAX_DENOMINATOR:
        raise ValueError(f"percentile {percentile!r} / 100 has denominator {q.denominator}; the kernel serves at most "
                         f"{SURFACE_MAX_DENOMINATOR}")
    return int(q.numerator), int(q.denominator)


def surface_distance_scores(records, ignore_index=None, percentile=95):
    """Hausdorff distance, its percentile and the average symmetric surface distance from the records of `surface_distances` /
    `SurfaceDistanceMeter.records()`, int64 [images, 2, K, 8] (include/cvk.h: n, m, max d2, Q, k, r, d2_lo, d2_hi per image, direction
    and class), in float64 on the host.  `percentile` must be the one the records were made with (their slots hold k and r, not the
    denominator; a percentile that does not fit them raises ValueError).  A class is evaluated in an image iff both maps have a contour of it; then
      hd   = the larger sqrt(max d2) of the two directions,
      hdq  = the larger a + (b - a) r / qden of the two directions, a = sqrt(d2_lo), b = sqrt(d2_hi): numpy's default "linear"
             percentile of the distances per direction, then the larger one (MONAI's rule),
      assd = (Q_PG + Q_GP) / 65536 / (n_P + n_G).
    A class with a contour in exactly one map of an image is unmatched: it is counted and takes part in no mean (public libraries
    return inf or NaN there).  An image's score is the mean over its evaluated classes, the set's score the mean over the images that
    have one (NaN without one).  Returns "hd95" (the percentile score, whatever `percentile` is), "hd", "assd", "hd95_per_class",
    "hd_per_class", "assd_per_class" (float64 [K]: the mean over the images where the class is evaluated, NaN where it never is and at
    ignore_index), "unmatched" (int64 [K]), "images" (how many images had an evaluated class) and "percentile"."""
    from fractions import Fraction
    qnum, qden = surface_percentile(percentile)
    rec = np.asarray(records, dtype=np.int64)
    if rec.ndim != 4 or rec.shape[1] != 2 or rec.shape[3] != SURFACE_RECORD_SLOTS:
        raise ValueError(f"expected records of shape [images, 2, K, {SURFACE_RECORD_SLOTS}], got {list(rec.shape)}")
    nP, nG = rec[:, 0, :, 0], rec[:, 1, :, 0]
    ev = (nP > 0) & (nG > 0)                                            # [images, K]
    unmatched = ((nP > 0) ^ (nG > 0)).sum(axis=0).astype(np.int64)
    n1 = rec[..., 0] - 1
    if (np.where(ev[:, None, :], rec[..., 4] * qden + rec[..., 5] - n1 * qnum, 0) != 0).any():
        raise ValueError(f"these records were not made with percentile {percentile!r}: their ranks k, r do not satisfy "
                         f"k * {qden} + r = (n - 1) * {qnum}")
    f = np.where(ev[:, None, :, None], rec, 0).astype(np.float64)      # unevaluated slots (-1) must not reach a root
    hd = np.sqrt(f[..., 2]).max(axis=1)
    a, b = np.sqrt(f[..., 6]), np.sqrt(f[..., 7])
    hdq = (a + (b - a) * f[..., 5] / float(qden)).max(axis=1)
    assd = np.divide((f[:, 0, :, 3] + f[:, 1, :, 3]) / 65536.0, (nP + nG).astype(np.float64), out=np.zeros(ev.shape), where=ev)
    out = {}
    scored = ev.any(axis=1)
    for name, v in (("hd95", hdq), ("hd", hd), ("assd", assd)):
        image = _masked_mean(v, ev, 1)
        per_class = _masked_mean(v, ev, 0)
        _nan_at(ignore_index, per_class)
        out[name] = _mean_of(image, scored)
        out[name + "_per_class"] = per_class
    out["unmatched"], out["images"] = unmatched, int(scored.sum())
    out["percentile"] = float(Fraction(qnum, qden) * 100)
    return out


def _surface_call(who, pred, label, num_classes, ignore_index, frac, d2):
    """One cvk_surface_distances call; d2 None: the kept planes of this shape.  Returns (d2, record)."""
    p, l = _map_pair(who, pred, label)
    lib = _lib.load()
    N, H, W = p.shape
    ent = _workspace("surface", N, H, W, num_classes, p.device) or _new_workspace(
        "surface", N, H, W, num_classes, p.device, lib.cvk_surface_workspace_bytes(N, H, W, num_classes),
        f"surface distances serve 1 to {EDT_MAX_CLASSES} classes, H <= 65534, (H - 1)^2 + (W - 1)^2 < 2^24 and fewer than 2^31 pixels, "
        f"got N = {N}, H = {H}, W = {W}, classes = {num_classes}")
    if d2 is None:
        d2 = _kept(ent, "d2", (2, N, H, W), torch.int32)
    record = torch.empty((N, 2, num_classes, SURFACE_RECORD_SLOTS), device=p.device, dtype=torch.int64)
    check(lib.cvk_surface_distances(p.data_ptr(), l.data_ptr(), N, H, W, num_classes, ignore_index, frac[0], frac[1], ent["ws"].data_ptr(),
                                    d2.data_ptr(), record.data_ptr(), _stream(p)), "cvk_surface_distances")
    return d2, record


def surface_distances(pred, label, num_classes=12, ignore_index=11, percentile=95):
    """Contour-to-contour distances of int64 maps [N,H,W] on the GPU, per image and class, under BoundaryMeter's contour rule
    (include/cvk.h, cvk_surface_distances): `d2` int32 [2,N,H,W], plane 0 the exact squared Euclidean distance from each contour pixel
    of the prediction to the nearest contour pixel of its class in the label map (-1: the label map has none), plane 1 the same from
    the label's contour pixels to the prediction's, -2 at every other pixel; `record` int64 [N,2,num_classes,8], per (image, direction,
    class): n, m, max d2, Q (the sum of the distances in 2^-16 pixels, by integers), and the ranks and values of the `percentile`:
    k, r, d2_lo, d2_hi.  Both are new device tensors; no host sync.  `surface_distance_scores` turns records into scores."""
    _check_classes("surface_distances", num_classes, EDT_MAX_CLASSES)
    frac = surface_percentile(percentile)
    p, l = _map_pair("surface_distances", pred, label)
    d2 = torch.empty((2,) + tuple(p.shape), device=p.device, dtype=torch.int32)
    return _surface_call("surface_distances", p, l, num_classes, int(ignore_index), frac, d2)


class SurfaceDistanceMeter:
    """Hausdorff distance (HD), its percentile (HD95 by default; MONAI's compute_hausdorff_distance(percentile=95), medpy's hd95) and
    the average symmetric surface distance (ASSD) of predictions against labels, per image and class, between the 4-connected contours
    of BoundaryMeter's rule.  Distances, sums and the exact order statistics are made on the device by one cvk_surface_distances call
    per batch (integers only: two runs agree bit for bit); no host sync until `records()` / `compute()`.  Pixels whose label is
    `ignore_index` are void in both maps.  A class whose contour exists in only one map of an image is counted as unmatched and enters
    no mean."""

    update_takes, report_keys = "pred", ("hd95", "hd", "assd", "hd95_per_class", "hd_per_class", "assd_per_class")

    def __init__(self, num_classes=12, ignore_index=11, percentile=95):
        self.num_classes = _check_classes("SurfaceDistanceMeter", num_classes, EDT_MAX_CLASSES)
        self.ignore_index, self.percentile = int(ignore_index), percentile
        self._frac = surface_percentile(percentile)
        self._parts = _Parts(2, self.num_classes, SURFACE_RECORD_SLOTS)

    def reset(self):
        self._parts.clear()

    def update(self, pred, label):
        _, record = _surface_call("SurfaceDistanceMeter.update", pred, label, self.num_classes, self.ignore_index, self._frac, None)
        self._parts.append(record)

    def records(self):
        """int64 [images, 2, num_classes, 8] on the host, in the order of the updates — one device->host copy."""
        return self._parts.host()

    def compute(self):
        """`surface_distance_scores` of `records()`."""
        return surface_distance_scores(self.records().numpy(), self.ignore_index, self.percentile)


CHEB_MAX_DEPTH = 254             # include/cvk.h: depths, dilations and trimap widths of the chessboard depth map
CHEB_MAX_WIDTHS = 8
BIOU_ROWS = 6                    # include/cvk.h: bG, bP, bI, aG, aP, aI


def boundary_dilation(H, W, ratio=0.02):
    """The dilation of Boundary IoU (Cheng et al., CVPR 2021) for an H x W image, in pixels: max(1, round(ratio * diagonal)), in exact
    rational arithmetic (`ratio` is read through its decimal string, as `boundary_tolerance` reads its tolerance): the largest d with
    (2 d - 1)^2 <= 4 ratio^2 (H^2 + W^2), and at least 1.  An exact half rounds up, where Python's round() of the float product goes to
    the even neighbour.  The default is 2 % of the diagonal: 360 x 480 -> 12, 720 x 960 -> 24."""
    import math
    from fractions import Fraction
    try:
        if isinstance(ratio, bool):
            raise ValueError
        q = Fraction(str(ratio))
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"ratio must be a non-negative number. Got: {ratio!r}") from None
    if q < 0:
        raise ValueError(f"ratio must not be negative. Got: {ratio!r}")
    d = max(1, (math.isqrt((4 * q * q * (int(H) * int(H) + int(W) * int(W))).__floor__()) + 1) // 2)
    if d > CHEB_MAX_DEPTH:
        raise ValueError(f"a ratio of {ratio!r} on {H} x {W} pixels is a dilation of {d}; the kernels serve at most {CHEB_MAX_DEPTH}")
    return int(d)


def _check_depth(name, d):
    if isinstance(d, bool) or not isinstance(d, int) or not 1 <= d <= CHEB_MAX_DEPTH:
        raise ValueError(f"{name} must be an integer in 1..{CHEB_MAX_DEPTH}. Got: {d!r}")
    return d


def _cheb_workspace(lib, N, H, W, device):
    """The buffers of cvk_cheb_depth / cvk_boundary_iou_counts: the workspace, and under "maps" the meter's four byte maps."""
    return _workspace("cheb", N, H, W, None, device) or _new_workspace(
        "cheb", N, H, W, None, device, lib.cvk_cheb_workspace_bytes(N, H, W),
        f"the chessboard depth serves rows of up to 32768 pixels and fewer than 2^31 pixels, got N = {N}, H = {H}, W = {W}")


def _cheb_call(lib, m, v, code, depth, ws, num_classes, ignore_index, max_depth, border):
    N, H, W = m.shape
    check(lib.cvk_cheb_depth(m.data_ptr(), None if v is None else v.data_ptr(), code.data_ptr(), depth.data_ptr(), ws.data_ptr(), N, H, W,
                             num_classes, ignore_index, max_depth, 1 if border else 0, _stream(m)), "cvk_cheb_depth")


def chessboard_depth(labels, num_classes=12, ignore_index=11, void_from=None, border=True, max_depth=254):
    """(code, depth), uint8 [N,H,W] each, of the int64 map `labels` on the GPU (include/cvk.h, cvk_cheb_depth).  `code` is the pixel's
    class, 254 for a value that is no class, 255 where `void_from` (the label map of a prediction; None: the map's own) is
    `ignore_index`.  `depth` of a class pixel is how many 3 x 3 erosions of its class's mask it survives, plus one: the smallest k for
    which the (2k+1)-square around it holds another code, void and 254 included; with `border` the image border counts as outside too
    (Cheng's zero pad), without it the border bounds nothing.  Pixels deeper than `max_depth` hold `max_depth + 1`; a pixel that is no
    class holds 0.  The class-c mask eroded d <= max_depth times is (code == c) & (depth > d).  No host sync."""
    m, v = _map_pair("chessboard_depth", labels, labels if void_from is None else void_from)
    _check_classes("chessboard_depth", num_classes)
    _check_depth("max_depth", max_depth)
    lib = _lib.load()
    N, H, W = m.shape
    ws = _cheb_workspace(lib, N, H, W, m.device)["ws"]
    code = torch.empty((N, H, W), device=m.device, dtype=torch.uint8)
    depth = torch.empty((N, H, W), device=m.device, dtype=torch.uint8)
    _cheb_call(lib, m, None if void_from is None else v, code, depth, ws, num_classes, int(ignore_index), max_depth, border)
    return code, depth


def boundary_iou_scores(counts, ignore_index=None):
    """Boundary IoU (Cheng et al., CVPR 2021) from per-image, per-class counts [images, 6, K] (rows: bG, bP, bI the band pixels of the
    label, of the masked prediction and of both; aG, aP, aI the same of the whole masks), in float64 on the host.  Returns
      "biou": per class sum bI / (sum bG + sum bP - sum bI) over all images (pooled over the set, as the mIoU is), then the mean over
          the classes with a non-zero denominator (NaN without one),
      "biou_per_class": float64 [K], NaN where the denominator is 0 and at ignore_index,
      "biou_image": the mean over the images with an evaluated class of the image's mean boundary IoU over its classes with
          bG + bP > 0 (as the boundary F1 averages),
      "min_iou_per_class": min(mask IoU, boundary IoU) of the pooled counts, the quantity Boundary AP / PQ use,
      "images": how many images had an evaluated class."""
    c = np.asarray(counts, dtype=np.int64)
    if c.ndim != 3 or c.shape[1] != BIOU_ROWS:
        raise ValueError(f"expected counts of shape [images, {BIOU_ROWS}, K], got {list(c.shape)}")

    def ratio(i, a, b):
        return _nan_ratio(i.astype(np.float64), (a + b - i).astype(np.float64))

    pooled = c.sum(axis=0)
    per_class = ratio(pooled[2], pooled[0], pooled[1])
    mask_iou = ratio(pooled[5], pooled[3], pooled[4])
    per_image = ratio(c[:, 2], c[:, 0], c[:, 1])          # [images, K], NaN where bG + bP == 0 (the union is then 0 too)
    _nan_at(ignore_index, per_class, mask_iou, per_image)
    ev, evi = ~np.isnan(per_class), ~np.isnan(per_image)
    image = _masked_mean(per_image, evi, 1)
    scored = evi.any(axis=1)
    return {"biou": _mean_of(per_class, ev), "biou_per_class": per_class, "biou_image": _mean_of(image, scored),
            "min_iou_per_class": np.where(np.isnan(per_class) | np.isnan(mask_iou), np.nan, np.fmin(per_class, mask_iou)),
            "images": int(scored.sum())}


def _check_widths(widths):
    try:
        ws = tuple(widths)
    except TypeError:
        raise ValueError(f"trimap_widths must be a sequence of integers. Got: {widths!r}") from None
    if len(ws) > CHEB_MAX_WIDTHS:
        raise ValueError(f"at most {CHEB_MAX_WIDTHS} trimap widths. Got: {len(ws)}")
    for w in ws:
        _check_depth("a trimap width", w)
    if any(b <= a for a, b in zip(ws, ws[1:])):
        raise ValueError(f"trimap widths must be strictly increasing. Got: {ws!r}")
    return ws


def trimap_scores(conf, widths, ignore_index=None):
    """The trimap curve (Kohli et al.; DeepLab) from the bins of `BoundaryIoUMeter.trimap_counts()`, int64 [nw, K, K]: bin i holds the
    confusion matrix [label, prediction] of the non-void pixels whose chessboard depth in the label map is above widths[i - 1] and at
    most widths[i]; the band of width widths[i] is the running sum.  In float64 on the host, per width: "trimap_miou" the mean over
    the classes other than ignore_index with a non-zero union of diag / (row sum + column sum - diag) (NaN without one),
    "trimap_accuracy" trace / total (NaN for an empty band), "trimap_pixels" the band's total (int64), and "widths"."""
    ws = _check_widths(widths)
    b = np.asarray(conf, dtype=np.int64)
    if b.ndim != 3 or b.shape[0] != len(ws) or b.shape[1] != b.shape[2]:
        raise ValueError(f"expected bins of shape [{len(ws)}, K, K], got {list(b.shape)}")
    K = b.shape[1]
    cum = np.cumsum(b, axis=0)
    miou, acc = np.full(len(ws), np.nan), np.full(len(ws), np.nan)
    pixels = cum.sum(axis=(1, 2)).astype(np.int64)
    for i in range(len(ws)):
        diag = np.diagonal(cum[i]).astype(np.float64)
        union = cum[i].sum(axis=1) + cum[i].sum(axis=0) - np.diagonal(cum[i])
        ev = union > 0
        if ignore_index is not None and 0 <= ignore_index < K:
            ev[ignore_index] = False
        if ev.any():
            miou[i] = (diag[ev] / union[ev]).mean()
        if pixels[i] > 0:
            acc[i] = diag.sum() / float(pixels[i])
    return {"trimap_miou": miou, "trimap_accuracy": acc, "trimap_pixels": pixels, "widths": ws}


class BoundaryIoUMeter:
    """Boundary IoU (Cheng et al., CVPR 2021) and the trimap curve (mIoU inside bands of growing width around the label boundaries;
    Kohli et al., DeepLab) of predictions against labels.  Both read one device map: the chessboard depth of every pixel inside its
    own region (`chessboard_depth`), made by two launches per map; one more launch counts per image and class the band and mask
    pixels of both maps and of their intersection, and per width the confusion matrix of the band (exact integers: two runs agree
    bit for bit).  No host sync until `counts()` / `trimap_counts()` / `compute()`.  The dilation is `ratio` times the image diagonal
    of each batch (`boundary_dilation`; Cheng's default 0.02), or `dilation` pixels; the band of a mask is what `dilation` 3 x 3
    erosions with a zero pad remove.  `trimap_widths`: up to 8 strictly increasing widths in 1..254; the image border bounds no
    trimap band.  Pixels whose label is `ignore_index` are void in both maps and bound the regions beside them."""

    update_takes = "pred"

    def __init__(self, num_classes=12, ignore_index=11, ratio=0.02, dilation=None, trimap_widths=()):
        self.num_classes = _check_classes("BoundaryIoUMeter", num_classes)
        self.ignore_index, self.ratio = int(ignore_index), ratio
        self.dilation = None if dilation is None else _check_depth("dilation", dilation)
        if dilation is None:
            boundary_dilation(1, 1, ratio)                # a bad ratio fails here, not in the first batch
        self.trimap_widths = _check_widths(trimap_widths)
        import ctypes
        self._widths = (ctypes.c_int * max(1, len(self.trimap_widths)))(*self.trimap_widths)
        self._parts = _Parts(BIOU_ROWS, self.num_classes)
        self.reset()

    @property
    def report_keys(self):
        return ("biou", "biou_per_class") + (("trimap_miou",) if self.trimap_widths else ())

    def reset(self):
        self._parts.clear()
        self._trimap = None

    def update(self, pred, label):
        p, l = _map_pair("BoundaryIoUMeter.update", pred, label)
        lib = _lib.load()
        N, H, W = p.shape
        K, nw = self.num_classes, len(self.trimap_widths)
        d = self.dilation if self.dilation is not None else boundary_dilation(H, W, self.ratio)
        max_depth = max((d,) + self.trimap_widths)
        ent = _cheb_workspace(lib, N, H, W, p.device)
        ws, maps = ent["ws"], _kept(ent, "maps", (4, N, H, W), torch.uint8)     # code and depth of the prediction, then of the label
        _cheb_call(lib, p, l, maps[0], maps[1], ws, K, self.ignore_index, max_depth, False)
        _cheb_call(lib, l, None, maps[2], maps[3], ws, K, self.ignore_index, max_depth, False)
        part = torch.zeros((N, BIOU_ROWS, K), device=p.device, dtype=torch.int64)
        if nw and (self._trimap is None or self._trimap.device != p.device):
            if self._trimap is not None:
                raise ValueError("BoundaryIoUMeter.update: the batches of one meter must be on one device")
            self._trimap = torch.zeros((nw, K, K), device=p.device, dtype=torch.int64)
        check(lib.cvk_boundary_iou_counts(maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(), maps[3].data_ptr(), part.data_ptr(),
                                          self._trimap.data_ptr() if nw else None, self._widths if nw else None, nw, N, H, W, K, d,
                                          _stream(p)), "cvk_boundary_iou_counts")
        self._parts.append(part)

    def counts(self):
        """int64 [images, 6, num_classes] on the host (rows bG, bP, bI, aG, aP, aI), in the order of the updates — one device->host
        copy."""
        return self._parts.host()

    def trimap_counts(self):
        """int64 [widths, num_classes, num_classes] on the host: per width the confusion matrix [label, prediction] of the pixels whose
        depth in the label map falls into that width's bin (`trimap_scores` takes the running sum)."""
        K = self.num_classes
        if self._trimap is None:
            return torch.zeros((len(self.trimap_widths), K, K), dtype=torch.int64)
        return self._trimap.cpu()

    def compute(self):
        """`boundary_iou_scores` of `counts()`, and with widths `trimap_scores` of `trimap_counts()` too."""
        out = boundary_iou_scores(self.counts().numpy(), self.ignore_index)
        if self.trimap_widths:
            out.update(trimap_scores(self.trimap_counts().numpy(), self.trimap_widths, self.ignore_index))
        return out


CC_RECORD_SLOTS = 8              # include/cvk.h: components, pixels, largest, small, small pixels, changed, received, isolated
CC_MODES = ("fill", "neighbor")


def _check_region_options(who, num_classes, connectivity, mode="neighbor", min_area=1):
    _check_classes(who, num_classes)
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"{who}: connectivity must be 4 or 8. Got: {connectivity!r}")
    if mode not in CC_MODES:
        raise ValueError(f"{who}: mode must be one of {CC_MODES}. Got: {mode!r}")
    if isinstance(min_area, bool) or not isinstance(min_area, int) or min_area < 1:
        raise ValueError(f"{who}: min_area must be an integer of at least 1. Got: {min_area!r}")


def _check_region_map(who, m):
    if not isinstance(m, torch.Tensor) or m.dtype != torch.int64 or m.dim() not in (2, 3) or m.numel() == 0:
        raise ValueError(f"{who}: expected an int64 tensor [N, H, W] or [H, W]")
    if m.numel() >= 2 ** 31:
        raise ValueError(f"{who}: {m.numel()} pixels, the kernels serve fewer than 2^31")
    if not m.is_cuda:
        raise ValueError(f"{who}: expected a tensor on a GPU (no CPU fallback)")
    return (m if m.dim() == 3 else m.unsqueeze(0)).contiguous()


def _region_workspace(lib, N, H, W, C, device):
    """The buffers of cvk_cc_label / cvk_cc_filter: the workspace, under "public" the (labels, area) maps `connected_components`
    returns, and under "maps" two such pairs for the callers that keep the maps to themselves (the filter and the meter)."""
    return _workspace("region", N, H, W, C, device) or _new_workspace(
        "region", N, H, W, C, device, lib.cvk_cc_workspace_bytes(N, H, W, C),
        f"connected components serve 1 to 32 classes and fewer than 2^31 pixels, got N = {N}, H = {H}, W = {W}, {C} classes")


def _cc_label(lib, m, labels, area, ws, num_classes, ignore_index, connectivity):
    N, H, W = m.shape
    check(lib.cvk_cc_label(m.data_ptr(), labels.data_ptr(), area.data_ptr(), N, H, W, num_classes, ignore_index, connectivity,
                           ws.data_ptr(), _stream(m)), "cvk_cc_label")


def _cc_filter(lib, m, labels, area, out, record, ws, num_classes, ignore_index, connectivity, min_area, mode, fill_value):
    N, H, W = m.shape
    check(lib.cvk_cc_filter(m.data_ptr(), labels.data_ptr(), area.data_ptr(), out.data_ptr(), None if record is None else record.data_ptr(),
                            N, H, W, num_classes, ignore_index, connectivity, min(min_area, 2 ** 31 - 1), CC_MODES.index(mode),
                            int(fill_value), ws.data_ptr(), _stream(m)), "cvk_cc_filter")


def connected_components(labels, num_classes=12, ignore_index=11, connectivity=4):
    """(labels, area), int32 [N,H,W] each ([H,W] for an [H,W] map), of the int64 class map `labels` on the GPU (include/cvk.h,
    cvk_cc_label).  A pixel's code is its value when that is a class other than `ignore_index`, and void, one code, for anything else;
    a component is a maximal set of equal codes of one image connected under `connectivity` (4 or 8), void components included.
    `labels` of a pixel is y * W + x of the first pixel of its component in row-major order, `area` the component's size, at every
    pixel.  Exact and canonical: nothing depends on the order in which the device works.  The two maps are buffers kept per shape and
    device and are overwritten by the next call of the same shape.  No host sync."""
    _check_region_options("connected_components", num_classes, connectivity)
    m = _check_region_map("connected_components", labels)
    lib = _lib.load()
    N, H, W = m.shape
    ent = _region_workspace(lib, N, H, W, num_classes, m.device)
    lab, area = _kept(ent, "public", (2, N, H, W), torch.int32)
    _cc_label(lib, m, lab, area, ent["ws"], num_classes, int(ignore_index), connectivity)
    return (lab, area) if labels.dim() == 3 else (lab[0], area[0])


class RegionFilter:
    """Removes the regions of a class map that are smaller than `min_area` pixels: `rf(pred)` returns a new int64 map of the shape of
    `pred` ([N,H,W] or [H,W]), e.g. `cls = rf(cvk.predict(net, img, window=sw))`.  A region is a component of `connected_components`
    whose code is a class; void is never removed.  mode "fill": its pixels become `fill_value` (default: `ignore_index`).  mode
    "neighbor": it becomes the class most of its neighbouring pixels have, counting pairs (pixel of the region, neighbour under the same
    connectivity) whose neighbour is a class pixel of a region that is not small itself; ties go to the smallest class, a region
    without any such neighbour stays as it is.  One round, so the result does not depend on any order; `min_area=1` returns the input's
    values.  `last_record` is a view of the device record int64 [N, num_classes, 8] of the last call: components, pixels, largest area,
    small components, their pixels, small components changed, pixels received from other classes, small components without a vote.
    Five to seven launches, no host sync."""

    def __init__(self, min_area, num_classes=12, ignore_index=11, connectivity=4, mode="neighbor", fill_value=None):
        _check_region_options("RegionFilter", num_classes, connectivity, mode, min_area)
        self.min_area, self.num_classes, self.ignore_index = min_area, num_classes, int(ignore_index)
        self.connectivity, self.mode = connectivity, mode
        if fill_value is not None and mode != "fill":
            raise ValueError('RegionFilter: fill_value belongs to mode="fill"')
        if fill_value is not None and (isinstance(fill_value, bool) or not isinstance(fill_value, int) or not -2 ** 63 <= fill_value < 2 ** 63):
            raise ValueError(f"RegionFilter: fill_value must be an int64 value. Got: {fill_value!r}")
        self.fill_value = self.ignore_index if fill_value is None else fill_value
        self._record = None

    @property
    def last_record(self):
        if self._record is None:
            raise RuntimeError("RegionFilter.last_record: the filter has not been called yet")
        return self._record

    def _run(self, m, pair):
        """the filtered map and the record of the contiguous [N,H,W] map `m`; `pair` chooses the (labels, area) buffers"""
        lib = _lib.load()
        N, H, W = m.shape
        ent = _region_workspace(lib, N, H, W, self.num_classes, m.device)
        lab, area = _kept(ent, "maps", (2, 2, N, H, W), torch.int32)[pair]
        _cc_label(lib, m, lab, area, ent["ws"], self.num_classes, self.ignore_index, self.connectivity)
        out = torch.empty_like(m)
        record = torch.zeros((N, self.num_classes, CC_RECORD_SLOTS), device=m.device, dtype=torch.int64)
        _cc_filter(lib, m, lab, area, out, record, ent["ws"], self.num_classes, self.ignore_index, self.connectivity, self.min_area,
                   self.mode, self.fill_value)
        return out, record

    def __call__(self, pred):
        m = _check_region_map("RegionFilter", pred)
        out, self._record = self._run(m, 0)
        return out if pred.dim() == 3 else out[0]


def remove_small_regions(pred, min_area, num_classes=12, ignore_index=11, connectivity=4, mode="neighbor", fill_value=None):
    """`RegionFilter(min_area, ...)(pred)`: the int64 map `pred` without its class regions of fewer than `min_area` pixels."""
    return RegionFilter(min_area, num_classes, ignore_index, connectivity, mode, fill_value)(pred)


def region_scores(records_pred, records_label, hist, ignore_index=None):
    """The scores of `RegionMeter` from its sums, in float64 on the host: `records_pred` / `records_label` int64 [K, 8] pooled over the
    images, `hist` int64 [3, K] the confusion counts of the filtered prediction (intersection, prediction, label)."""
    rp, rl, h = (np.asarray(a, dtype=np.int64) for a in (records_pred, records_label, hist))
    frag = _nan_ratio(rp[:, 0].astype(np.float64), rl[:, 0])
    iou = _nan_ratio(h[0].astype(np.float64), (h[1] + h[2] - h[0]).astype(np.float64))
    _nan_at(ignore_index, frag, iou)
    return {"regions_pred": rp[:, 0].copy(), "regions_label": rl[:, 0].copy(), "small_regions_pred": rp[:, 3].copy(),
            "fragmentation_per_class": frag, "fragmentation": _mean_of(frag, ~np.isnan(frag)),
            "iou_filtered": iou, "miou_filtered": _mean_of(iou, ~np.isnan(iou))}


class RegionMeter:
    """Fragmentation of predictions against labels, and the mIoU after despeckling.  `update(pred, label)` labels the components of
    both maps, filters the prediction as `RegionFilter(min_area, ..., mode)` does (the labels take no part in that, as at deployment;
    void is the prediction's own `ignore_index` pixels) and adds the filtered prediction's confusion counts against the label and both
    maps' records, all on the device.  `compute()` (one device->host copy) returns "regions_pred", "regions_label",
    "small_regions_pred" (int64 per class, pooled over the images; the prediction's are those before the filter),
    "fragmentation_per_class" (predicted regions over label regions; NaN for a class without a label region and at `ignore_index`),
    "fragmentation" (its mean over the classes that occur), "iou_filtered", "miou_filtered" and "images"."""

    update_takes, report_keys = "pred", ("fragmentation", "miou_filtered", "regions_pred")

    def __init__(self, num_classes=12, ignore_index=11, min_area=64, connectivity=4, mode="neighbor"):
        self._filter = RegionFilter(min_area, num_classes, ignore_index, connectivity, mode)
        self._count = RegionFilter(1, num_classes, ignore_index, connectivity, "fill")       # removes nothing: the label's record
        self.num_classes, self.ignore_index, self.min_area = num_classes, int(ignore_index), min_area
        self.connectivity, self.mode = connectivity, mode
        self.reset()

    def reset(self):
        self._sums, self.images = None, 0

    def update(self, pred, label):
        p, l = _map_pair("RegionMeter.update", pred, label)
        if p.numel() >= 2 ** 31:
            raise ValueError(f"RegionMeter.update: {p.numel()} pixels, the kernels serve fewer than 2^31")
        lib = _lib.load()
        K = self.num_classes
        if self._sums is None:
            self._sums = torch.zeros(2 * K * CC_RECORD_SLOTS + 3 * K, device=p.device, dtype=torch.int64)
        elif self._sums.device != p.device:
            raise ValueError("RegionMeter.update: the batches of one meter must be on one device")
        filtered, rec_p = self._filter._run(p, 0)
        _, rec_l = self._count._run(l, 1)
        rec = self._sums[:2 * K * CC_RECORD_SLOTS].view(2, K, CC_RECORD_SLOTS)
        rec[0] += rec_p.sum(0)
        rec[1] += rec_l.sum(0)
        hist = self._sums[2 * K * CC_RECORD_SLOTS:]
        check(lib.cvk_confusion_accumulate(filtered.data_ptr(), l.data_ptr(), hist.data_ptr(), filtered.numel(), K, self.ignore_index,
                                           _stream(p)), "cvk_confusion_accumulate")
        self.images += p.shape[0]

    def compute(self):
        K = self.num_classes
        if self._sums is None:
            s = torch.zeros(2 * K * CC_RECORD_SLOTS + 3 * K, dtype=torch.int64).numpy()
        else:
            s = self._sums.cpu().numpy()
        rec = s[:2 * K * CC_RECORD_SLOTS].reshape(2, K, CC_RECORD_SLOTS)
        out = region_scores(rec[0], rec[1], s[2 * K * CC_RECORD_SLOTS:].reshape(3, K), self.ignore_index)
        out["images"] = self.images
        return out


WEIGHT_METHODS = ("median_frequency", "enet")


def weights_from_counts(pixels, image_pixels, method="median_frequency"):
    """Class weights from per-class counts (numpy float64 [C]); classes with no pixel get weight 0.
      median_frequency (SegNet, Eigen & Fergus): freq(c) = pixels[c] / image_pixels[c] (the counted pixels of the images that
        contain c), w_c = median over the present classes of freq / freq(c);
      enet (ENet, Paszke et al.): p_c = pixels[c] / all counted pixels, w_c = 1 / ln(1.02 + p_c)."""
    pix = np.asarray(pixels, dtype=np.float64)
    img = np.asarray(image_pixels, dtype=np.float64)
    present = pix > 0
    w = np.zeros_like(pix)
    if not present.any():
        return w
    if method == "median_frequency":
        freq = pix[present] / img[present]
        w[present] = np.median(freq) / freq
    elif method == "enet":
        w[present] = 1.0 / np.log(1.02 + pix[present] / pix.sum())
    else:
        raise ValueError(f"method must be one of {WEIGHT_METHODS}, got {method!r}")
    return w


class ClassFrequencyMeter:
    """Device-side class statistics of label masks for class weights (`weights()`), one launch per batch and no host sync
    until `weights()` / `counts()`.  Labels equal to `ignore_index` are skipped; labels outside [0, num_classes) are counted
    apart (`counts()[2]`).  The default counts every class, as the reference's loss trains Void (train.py:105)."""

    def __init__(self, num_classes=12, ignore_index=-100, device="cuda"):
        self.num_classes, self.ignore_index = num_classes, ignore_index
        self.hist = torch.zeros(2 * num_classes + 1, device=device, dtype=torch.int64)

    def reset(self):
        self.hist.zero_()

    def update(self, masks):
        """masks: uint8 or int64 HIP tensor [N, H, W] (or one [H, W] mask)."""
        lib = _lib.load()
        m = masks.contiguous()
        if m.dtype not in (torch.uint8, torch.int64) or m.dim() not in (2, 3) or not m.is_cuda:
            raise ValueError("expected uint8 or int64 HIP masks of shape [N, H, W] or [H, W]")
        if m.device != self.hist.device:
            raise ValueError(f"masks are on {m.device}, the meter on {self.hist.device}")
        if m.dim() == 2:
            m = m.unsqueeze(0)
        N = m.shape[0]
        if m.numel() == 0:
            return
        check(lib.cvk_class_histogram(m.data_ptr(), m.element_size(), N, m.numel() // N, self.num_classes, int(self.ignore_index),
                                      self.hist.data_ptr(), _stream(m)), "cvk_class_histogram")

    def counts(self):
        """(pixels per class, counted pixels of the images containing each class, labels out of range) — one device->host copy."""
        h = self.hist.cpu().numpy()
        K = self.num_classes
        return h[:K].copy(), h[K:2 * K].copy(), int(h[2 * K])

    def weights(self, method="median_frequency"):
        """float32 [num_classes] class weights on the meter's device (see `weights_from_counts`)."""
        if method not in WEIGHT_METHODS:
            raise ValueError(f"method must be one of {WEIGHT_METHODS}, got {method!r}")
        pix, img, _ = self.counts()
        return torch.tensor(weights_from_counts(pix, img, method), dtype=torch.float32).to(self.hist.device)


def class_weights(mask_batches, num_classes, ignore_index=-100, method="median_frequency", device="cuda"):
    """Class weights of a data set: `mask_batches` yields uint8 or int64 masks [N, H, W] (HIP tensors, or CPU tensors / numpy
    arrays, which are uploaded to `device`).  Returns float32 [num_classes] on the device, for CrossEntropyLoss(weight=...)."""
    if method not in WEIGHT_METHODS:
        raise ValueError(f"method must be one of {WEIGHT_METHODS}, got {method!r}")
    meter = None
    for m in mask_batches:
        m = torch.as_tensor(m)
        if not m.is_cuda:
            m = m.to(device)
        if meter is None:
            meter = ClassFrequencyMeter(num_classes, ignore_index, m.device)
        meter.update(m)
    if meter is None:
        raise ValueError("class_weights(): no batches")
    return meter.weights(method)


CALIB_MAX_CLASSES, CALIB_MAX_BINS, CALIB_MAX_CELLS = 128, 64, 2048     # include/cvk.h: the limits of cvk_calib_accumulate
CALIB_Q_SCALE = float(1 << 30)                                         # hist[..., 2] holds sum floor(conf * 2^30)
CALIB_LOG_COLUMNS = ("tau", "n", "nll", "g", "h", "tau_next", "lo", "hi")
CALIB_TAU_BRACKET = (1.0 / 64.0, 64.0)
CALIBRATION_REPORT_KEYS = ("ece", "mce", "nll", "brier")


def _check_calib_logits(who, logits, label=None):
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or (label is not None and not label.is_cuda):
        raise RuntimeError(f"pytorch_camvid_amd.{who} needs HIP tensors (no CPU fallback)")
    if label is not None and label.device != logits.device:
        raise ValueError(f"{who}: the logits are on {logits.device}, the label on {label.device}")
    _check_calib_shapes(who, logits, label)


def _check_calib_shapes(who, logits, label=None):
    """dtype, rank, class count and label shape: everything about the tensors but where they live"""
    if logits.dim() != 4:
        raise ValueError("expected logits of shape [N, C, H, W]")
    if logits.dtype != torch.float32:
        raise ValueError(f"{who}: expected float32 logits, got {logits.dtype}")
    N, C, H, W = logits.shape
    if not 1 <= C <= CALIB_MAX_CLASSES:
        raise ValueError(f"{who} serves 1 to {CALIB_MAX_CLASSES} classes, got C = {C}")
    if N * H * W == 0:
        raise ValueError(f"{who}: empty logits")
    if label is not None:
        if label.dtype != torch.int64:
            raise ValueError(f"{who}: expected an int64 label, got {label.dtype}")
        if tuple(label.shape) != (N, H, W):
            raise ValueError(f"Expected label size {[N, H, W]}, got {list(label.shape)}")


def _check_calib_classes(who, num_classes, bins=1):
    if not isinstance(num_classes, int) or not 1 <= num_classes <= CALIB_MAX_CLASSES:
        raise ValueError(f"{who}: num_classes must be an integer in [1, {CALIB_MAX_CLASSES}], got {num_classes!r}")
    if not isinstance(bins, int) or isinstance(bins, bool) or not 1 <= bins <= CALIB_MAX_BINS:
        raise ValueError(f"{who}: bins must be an integer in [1, {CALIB_MAX_BINS}], got {bins!r}")
    if num_classes * bins > CALIB_MAX_CELLS:
        raise ValueError(f"{who}: num_classes * bins = {num_classes * bins} exceeds {CALIB_MAX_CELLS} (the work-group's table in LDS)")


def _calib_tau(who, temperature, device):
    """The device float the kernel reads as tau = 1 / T: None (tau = 1), a TemperatureScaler's live value, or a new tensor."""
    if temperature is None:
        return None
    if isinstance(temperature, TemperatureScaler):
        return temperature.tau
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not 0.0 < float(temperature) < float("inf"):
        raise ValueError(f"{who}: temperature must be None, a positive finite number or a TemperatureScaler, got {temperature!r}")
    return torch.full((), 1.0 / float(temperature), device=device, dtype=torch.float32)


def calibration_scores(hist, record):
    """The host arithmetic of CalibrationMeter.compute(): `hist` int64 [C][B][3] = {count, correct, sum floor(conf 2^30)} by predicted
    class and bin, `record` the four words {valid, out of range, sum nll, sum brier} (an int64 tensor whose last two words are fp64 bit
    patterns, as the meter keeps it, or a sequence of four numbers).  ECE = sum_b n_b / n |acc_b - conf_b| over Guo's right-closed
    bins, MCE the maximum gap over the non-empty bins; "ece_per_class" is the same sum within the pixels PREDICTED as a class.  With no
    valid pixel every score is NaN."""
    h = np.asarray(hist.cpu() if isinstance(hist, torch.Tensor) else hist).astype(np.int64)
    if h.ndim != 3 or h.shape[2] != 3:
        raise ValueError(f"calibration_scores: hist must be [C][B][3], got {list(h.shape)}")
    if isinstance(record, torch.Tensor):
        r = record.cpu()
        sums = r[2:4].view(torch.float64) if r.dtype == torch.int64 else r[2:4].double()
        valid, bad, s_nll, s_brier = int(r[0]), int(r[1]), float(sums[0]), float(sums[1])
    else:
        valid, bad, s_nll, s_brier = int(record[0]), int(record[1]), float(record[2]), float(record[3])

    def gaps(t):                                  # t: [..., B, 3] -> per-bin count, accuracy, confidence, |acc - conf| (NaN where empty)
        cnt = t[..., 0].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            acc = t[..., 1] / cnt
            conf = t[..., 2] / CALIB_Q_SCALE / cnt
        return cnt, acc, conf, np.abs(acc - conf)

    top = h.sum(axis=0)
    cnt, acc, conf, gap = gaps(top)
    n = float(cnt.sum())
    nan = float("nan")
    with np.errstate(invalid="ignore", divide="ignore"):
        ece = float(np.nansum(cnt * gap) / n) if n > 0 else nan
        ccnt, _, _, cgap = gaps(h)
        per_n = ccnt.sum(axis=1)
        ece_c = np.where(per_n > 0, np.nansum(ccnt * cgap, axis=1) / per_n, np.nan)
    return {"ece": ece, "mce": float(np.nanmax(gap)) if n > 0 else nan,
            "nll": s_nll / valid if valid > 0 else nan, "brier": s_brier / valid if valid > 0 else nan,
            "accuracy": float(top[:, 1].sum() / n) if n > 0 else nan,
            "mean_confidence": float(top[:, 2].sum() / CALIB_Q_SCALE / n) if n > 0 else nan,
            "bins": {"count": top[:, 0].copy(), "accuracy": acc, "confidence": conf},
            "ece_per_class": ece_c, "count_per_class": per_n.astype(np.int64), "valid": valid, "out_of_range": bad}


class CalibrationMeter:
    """Expected calibration error and reliability tables of the top-label probability (Guo et al., ICML 2017), accumulated on the
    device in one pass over the logits per batch (cvk_calib_accumulate; the definitions are in include/cvk.h):

      meter = CalibrationMeter(num_classes=12, ignore_index=11, bins=15, temperature=None)
      meter.update(logits, masks)          # float32 [N,C,H,W] (channels_last is read in place), int64 [N,H,W]
      meter.compute()                      # one device->host copy: "ece", "mce", "nll", "brier", "accuracy", "mean_confidence",
                                           # "bins" (count / accuracy / confidence per bin), "ece_per_class", "count_per_class"
                                           # (by predicted class), "valid", "out_of_range"

    `temperature` is None, a float T (the probabilities are softmax(logits / T)), or a TemperatureScaler, whose device value is read at
    every update without a sync.  `hist` (int64 [C][bins][3]) and `record` (int64 [4]: valid, out of range, and the fp64 bit patterns
    of sum nll and sum brier) are the device tensors; every word of `hist` is an integer sum, so the tables do not depend on the order
    of the pixels or of the updates.  Limits: 1 <= C <= 128, 1 <= bins <= 64, C * bins <= 2048."""

    update_takes, report_keys = "logits", CALIBRATION_REPORT_KEYS

    def __init__(self, num_classes=12, ignore_index=11, bins=15, temperature=None, device="cuda"):
        _check_calib_classes("CalibrationMeter", num_classes, bins)
        self.num_classes, self.ignore_index, self.bins = num_classes, int(ignore_index), bins
        self.temperature = temperature
        self._tau = _calib_tau("CalibrationMeter", temperature, device)
        self.hist = torch.zeros((num_classes, bins, 3), device=device, dtype=torch.int64)
        self.record = torch.zeros(4, device=device, dtype=torch.int64)
        self._part = None

    def reset(self):
        self.hist.zero_()
        self.record.zero_()

    def update(self, logits, label, conf=None, pred=None):
        """Adds one batch.  `conf` (float32 [N,H,W]) and `pred` (int64 [N,H,W]), when given, receive the maps of every pixel."""
        _check_calib_logits("CalibrationMeter", logits, label)
        N, C, H, W = logits.shape
        if C != self.num_classes:
            raise ValueError(f"CalibrationMeter: the meter has {self.num_classes} classes, the logits {C}")
        for name, m, dt in (("conf", conf, torch.float32), ("pred", pred, torch.int64)):
            if m is not None and (m.dtype != dt or tuple(m.shape) != (N, H, W) or not m.is_contiguous() or m.device != logits.device):
                raise ValueError(f"CalibrationMeter: {name} must be a contiguous {dt} tensor of shape {[N, H, W]} on the logits' device")
        tau = self._tau
        if logits.device != self.hist.device or (tau is not None and tau.device != logits.device):
            raise ValueError(f"CalibrationMeter: the logits are on {logits.device}, the meter's tables on {self.hist.device}"
                             + (f", its temperature on {tau.device}" if tau is not None else ""))
        lib = _lib.load()
        lg, ld = _as_nhwc(logits.detach())
        lab = label.contiguous()
        M = N * H * W
        need = 4 * lib.cvk_ce_blocks(M)
        if self._part is None or self._part.numel() < need or self._part.device != logits.device:
            self._part = torch.empty(need, device=logits.device, dtype=torch.float64)
        check(lib.cvk_calib_accumulate(lg.data_ptr(), ld, lab.data_ptr(), tau.data_ptr() if tau is not None else None,
                                       self.hist.data_ptr(), self._part.data_ptr(), self.record.data_ptr(),
                                       conf.data_ptr() if conf is not None else None, pred.data_ptr() if pred is not None else None,
                                       M, C, self.bins, self.ignore_index, _stream(logits)), "cvk_calib_accumulate")

    def compute(self):
        both = torch.cat([self.record, self.hist.reshape(-1)]).cpu()                 # one device->host copy
        return calibration_scores(both[4:].reshape(self.num_classes, self.bins, 3), both[:4])


def confidence_map(logits, temperature=None):
    """(conf float32 [N,H,W], pred int64 [N,H,W]): the top-label probability of softmax(logits / T) and its class (the first maximum,
    as argmax_channels), from the meter's kernel without its tables: one launch.  The input of confidence-thresholded
    pseudo-labelling.  `temperature` as in CalibrationMeter."""
    _check_calib_logits("confidence_map", logits)
    lib = _lib.load()
    N, C, H, W = logits.shape
    tau = _calib_tau("confidence_map", temperature, logits.device)
    if tau is not None and tau.device != logits.device:
        raise ValueError(f"confidence_map: the logits are on {logits.device}, the temperature on {tau.device}")
    lg, ld = _as_nhwc(logits.detach())
    conf = torch.empty((N, H, W), device=logits.device, dtype=torch.float32)
    pred = torch.empty((N, H, W), device=logits.device, dtype=torch.int64)
    check(lib.cvk_calib_accumulate(lg.data_ptr(), ld, None, tau.data_ptr() if tau is not None else None, None, None, None,
                                   conf.data_ptr(), pred.data_ptr(), N * H * W, C, 1, 0, _stream(logits)), "cvk_calib_accumulate")
    return conf, pred


class TemperatureScaler:
    """Temperature scaling (Guo et al., ICML 2017): one scalar T fitted by minimising the NLL of softmax(logits / T) on held-out
    batches.  The fit is a bracketed Newton iteration on tau = 1 / T that runs on the device as a fixed chain of launches
    (cvk_calib_newton_accumulate per batch, cvk_calib_newton_step per iteration) with no host sync:

      scaler = TemperatureScaler(iterations=20, init=1.0, ignore_index=11)
      scaler.fit(logits_list, labels_list)        # stored float32 [N,C,H,W] / int64 [N,H,W] tensors; or
      scaler.fit_network(net, batches)            # an eval-mode forward per batch, logits kept
      scaler.temperature                          # host float T (one copy);  scaler.tau: 0-dim device view of 1 / T
      scaler(logits)                              # logits * tau, layout preserved
      scaler.log()                                # float64 [iterations + 1, 8]: tau, n, nll, g, h, tau_next, lo, hi per iteration

    tau is kept inside [1/64, 64].  `converged`: the last row's Newton step would move tau by less than 1e-5 of its value;
    `at_bound`: the fit ran into an end of the bracket (the NLL has no minimum inside it: a perfectly separable set, say)."""

    def __init__(self, iterations=20, init=1.0, ignore_index=11, device="cuda"):
        if not isinstance(iterations, int) or isinstance(iterations, bool) or not 1 <= iterations <= 1000:
            raise ValueError(f"TemperatureScaler: iterations must be an integer in [1, 1000], got {iterations!r}")
        if isinstance(init, bool) or not isinstance(init, (int, float)) or not 1.0 / 64.0 <= 1.0 / float(init or float("nan")) <= 64.0:
            raise ValueError(f"TemperatureScaler: the initial temperature must lie in [1/64, 64], got {init!r}")
        self.iterations, self.init, self.ignore_index = iterations, float(init), int(ignore_index)
        self._state = torch.zeros(9, device=device, dtype=torch.float64)
        self._log = torch.zeros((iterations + 1, len(CALIB_LOG_COLUMNS)), device=device, dtype=torch.float64)
        self._part = None
        self._reset_state()

    def _reset_state(self):
        tau0 = float(torch.tensor(1.0 / self.init, dtype=torch.float32))
        host = torch.tensor([tau0, CALIB_TAU_BRACKET[0], CALIB_TAU_BRACKET[1], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64)
        host[8:9].view(torch.float32)[0] = tau0
        self._state.copy_(host)                 # one host-to-device copy; the kernels own the state from here
        self._log.zero_()

    @property
    def tau(self):
        """0-dim float32 device view of the fitted inverse temperature; the step kernel writes it"""
        return self._state[8:9].view(torch.float32)[0]

    @property
    def temperature(self):
        return 1.0 / float(self.tau)

    def log(self):
        return self._log.clone()

    def _last(self):
        return [float(v) for v in self._log[self.iterations].cpu()]

    @property
    def at_bound(self):
        tau, _, _, _, _, _, lo, hi = self._last()
        return bool((hi == CALIB_TAU_BRACKET[1] and tau >= hi * (1.0 - 1e-3)) or (lo == CALIB_TAU_BRACKET[0] and tau <= lo * (1.0 + 1e-3)))

    @property
    def converged(self):
        tau, n, _, g, h, _, _, _ = self._last()
        return bool(n > 0 and not self.at_bound and h > 1e-12 and abs(g / h) <= 1e-5 * tau)

    def fit(self, logits_list, labels_list):
        """Fits on stored batches: every iteration walks every batch, then steps; a last pass leaves the NLL of the fitted tau in the
        log's last row.  Labels that are `ignore_index` or outside [0, C) are skipped (a CalibrationMeter counts the latter as
        "out_of_range"; the fit does not report them).  Returns self."""
        if isinstance(logits_list, torch.Tensor):
            logits_list, labels_list = [logits_list], [labels_list]
        logits_list, labels_list = list(logits_list), list(labels_list)
        if not logits_list or len(logits_list) != len(labels_list):
            raise ValueError("TemperatureScaler.fit: expected as many label tensors as logits tensors, and at least one")
        lib = _lib.load()
        calls = []
        for logits, label in zip(logits_list, labels_list):
            _check_calib_logits("TemperatureScaler", logits, label)
            if logits.device != self._state.device:
                raise ValueError(f"TemperatureScaler: the logits are on {logits.device}, the scaler on {self._state.device}")
            lg, ld = _as_nhwc(logits.detach())
            calls.append((lg, ld, label.contiguous(), lg.shape[0] * lg.shape[1] * lg.shape[2], logits.shape[1]))
        need = 4 * max(lib.cvk_ce_blocks(c[3]) for c in calls)
        if self._part is None or self._part.numel() < need:
            self._part = torch.empty(need, device=self._state.device, dtype=torch.float64)
        self._reset_state()
        stream = _stream(logits_list[0])
        state, log, part = self._state.data_ptr(), self._log.data_ptr(), self._part.data_ptr()
        for it in range(self.iterations + 1):
            for lg, ld, lab, M, C in calls:
                check(lib.cvk_calib_newton_accumulate(lg.data_ptr(), ld, lab.data_ptr(), state, part, M, C, self.ignore_index, stream),
                      "cvk_calib_newton_accumulate")
            check(lib.cvk_calib_newton_step(state, log, self.iterations + 1, int(it == self.iterations), stream), "cvk_calib_newton_step")
        return self

    def fit_network(self, net, batches, window=None):
        """Runs `net` once over `batches` ((images, masks) on the GPU) in eval mode under no_grad, keeps the logits and fits on them.
        Memory: the kept logits, 4 C M bytes per batch (C classes, M = N H W pixels; 66 MB at 8 x 12 x 360 x 480).  With `window` (a
        SlidingWindow) the logits are the windows' merged ones.  `net.training` is restored."""
        _check_window(window)
        was_training = net.training
        net.eval()
        kept, masks_kept = [], []
        try:
            with torch.no_grad():
                for images, masks in batches:
                    kept.append(net(images) if window is None else window(net, images)[0])
                    masks_kept.append(masks)
        finally:
            net.train(was_training)
        return self.fit(kept, masks_kept)

    def __call__(self, logits):
        return logits * self.tau
