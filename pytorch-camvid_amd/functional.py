"""Evaluation operators of the hot path on HIP tensors: meters, class weights, image ingest and the inference drivers.  The losses are
in losses.py; their public names and constants are importable from here as before.

  ClassFrequencyMeter, class_weights
                    <- median-frequency (SegNet) / ENet class weights from device-side class histograms of the masks
  argmax_channels   <- preds.argmax(dim=1) of train.py:191
  ConfusionMeter    <- utils.intersect_and_union / mean_iou (utils.py:162-228) accumulated on device, with the
                       np.float crash (utils.py:210) and the per-batch-sum bug of train.py:192-206 not reproduced
                       (SURVEY.md §0.5): IoU = sum(intersection)/sum(union) per class over the whole set.
  BoundaryMeter, label_boundaries, boundary_tolerance, boundary_scores
                    <- the boundary F1 measure (BF score, Csurka et al. BMVC 2013; not in the reference): per-image, per-class
                       contour counts from one launch, scores on the host
  BoundaryIoUMeter, chessboard_depth, boundary_dilation, boundary_iou_scores, trimap_scores
                    <- Boundary IoU (Cheng et al. CVPR 2021) and the trimap curve (not in the reference) on a device chessboard
                       depth map: integer counts per image and class, scores on the host
  connected_components, remove_small_regions, RegionFilter, RegionMeter, region_scores
                    <- connected components of a class map (canonical labels and areas from a union-find over tiles) and the
                       removal of small regions (not in the reference); fragmentation and the mIoU after despeckling
  LocalCRF, crf_refine, crf_coefficients, crf_tile
                    <- local-window mean-field CRF refinement of a prediction under the network's own input as the guide image
                       (ConvCRF's form with a dilation; not in the reference): one stencil launch per iteration
  CalibrationMeter, calibration_scores, confidence_map, TemperatureScaler
                    <- expected calibration error, reliability tables, NLL and Brier score of the top-label probability, and
                       temperature scaling (Guo et al. ICML 2017; not in the reference): one pass over the logits per batch into
                       integer tables, and a Newton fit of 1 / T that runs on the device without a host sync
"""
import torch

from . import _lib
from ._lib import check
from .losses import (_as_nhwc, _stream, BDL_RECORD_HEAD, DICE_AVERAGES, EDT_MAX_CLASSES, KD_RECORD, LOVASZ_CLASSES,  # noqa: F401
                     LOVASZ_CLASS_SLOTS, LOVASZ_RECORD_HEAD, LOVASZ_SORT_TILE, OHEM_RECORD, REDUCTIONS, SEG_RECORD_HEAD,
                     BoundaryLoss, CrossEntropyLoss, DiceLoss, DistillationLoss, FocalLoss, LovaszSoftmaxLoss, OhemCrossEntropyLoss,
                     SegmentationLoss, boundary_loss, cross_entropy, distillation_loss, distillation_scales, last_ce_status,
                     lovasz_softmax, ohem_cross_entropy, ohem_loss_threshold, segmentation_loss, signed_distance_maps,
                     squared_distance_maps)


def argmax_channels(logits):
    """preds.argmax(dim=1) (train.py:191): int64 [N,H,W]; first maximum wins."""
    lib = _lib.load()
    N, C, H, W = logits.shape
    lg, ld = _as_nhwc(logits.detach())
    out = torch.empty((N, H, W), device=logits.device, dtype=torch.int64)
    check(lib.cvk_argmax_channels(lg.data_ptr(), ld, out.data_ptr(), N * H * W, C, _stream(logits)), "cvk_argmax_channels")
    return out


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
    import numpy as np
    c = np.asarray(counts, dtype=np.int64)
    if c.ndim != 3 or c.shape[1] != 4:
        raise ValueError(f"expected counts of shape [images, 4, K], got {list(c.shape)}")
    K = c.shape[2]

    def prf(c4):
        nP, mP, nG, mG = (c4[..., r, :].astype(np.float64) for r in range(4))
        ev = (nP + nG) > 0
        P = np.divide(mP, nP, out=np.zeros_like(nP), where=nP > 0)
        R = np.divide(mG, nG, out=np.zeros_like(nG), where=nG > 0)
        F = np.divide(2.0 * P * R, P + R, out=np.zeros_like(P), where=(P + R) > 0)
        return ev, P, R, F

    def masked_mean(v, ev, axis):
        n = ev.sum(axis=axis)
        return np.divide(np.where(ev, v, 0.0).sum(axis=axis), n, out=np.full(n.shape, np.nan), where=n > 0)

    ev, P, R, F = prf(c)
    image = masked_mean(F, ev, 1)                         # [images], NaN where nothing is evaluated
    scored = ~np.isnan(image)
    per_class, prec, rec = masked_mean(F, ev, 0), masked_mean(P, ev, 0), masked_mean(R, ev, 0)
    if ignore_index is not None and 0 <= ignore_index < K:
        per_class[ignore_index] = prec[ignore_index] = rec[ignore_index] = np.nan
    evp, _, _, Fp = prf(c.sum(axis=0))
    return {"bf": float(image[scored].mean()) if scored.any() else float("nan"), "bf_per_class": per_class, "precision": prec,
            "recall": rec, "pooled": float(Fp[evp].mean()) if evp.any() else float("nan"), "images": int(scored.sum())}


def _check_boundary_maps(who, pred, label):
    ok = all(isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.dim() == 3 for t in (pred, label))
    if not ok or pred.shape != label.shape or pred.numel() == 0:
        raise ValueError(f"{who}: expected int64 tensors of one shape [N, H, W]")
    if not (pred.is_cuda and label.is_cuda) or pred.device != label.device:
        raise ValueError(f"{who}: expected both tensors on one GPU (no CPU fallback)")


class BoundaryMeter:
    """Boundary F1 measure (BF score; Csurka et al., BMVC 2013; MATLAB's bfscore) of predictions against labels: per image and class,
    the 4-connected contour pixels of both maps and how many of them have a contour pixel of the same class in the other map within
    the tolerance, counted on the device by one launch per batch (cvk_boundary_counts, exact integers), no host sync until
    `counts()` / `compute()`.  The tolerance is `tolerance` times the image diagonal of each batch (`boundary_tolerance`), or the
    squared pixel distance `radius2`.  Pixels whose label is `ignore_index` are void in both maps."""

    def __init__(self, num_classes=12, ignore_index=11, tolerance=0.0075, radius2=None):
        if not 1 <= num_classes <= 32:
            raise ValueError(f"BoundaryMeter serves 1 to 32 classes. Got: {num_classes}")
        self.num_classes, self.ignore_index, self.tolerance = int(num_classes), int(ignore_index), tolerance
        self.radius2 = None if radius2 is None else _check_radius2(radius2)
        if radius2 is None:
            boundary_tolerance(1, 1, tolerance)           # a bad tolerance fails here, not in the first batch
        self._parts = []

    def reset(self):
        self._parts = []

    def update(self, pred, label):
        _check_boundary_maps("BoundaryMeter.update", pred, label)
        lib = _lib.load()
        N, H, W = pred.shape
        r2 = self.radius2 if self.radius2 is not None else boundary_tolerance(H, W, self.tolerance)
        p = pred.contiguous(); l = label.contiguous()
        part = torch.zeros((N, 4, self.num_classes), device=p.device, dtype=torch.int64)
        check(lib.cvk_boundary_counts(p.data_ptr(), l.data_ptr(), part.data_ptr(), N, H, W, self.num_classes, self.ignore_index, r2,
                                      _stream(p)), "cvk_boundary_counts")
        self._parts.append(part)

    def counts(self):
        """int64 [images, 4, num_classes] on the host (rows nP, mP, nG, mG), in the order of the updates — one device->host copy."""
        if not self._parts:
            return torch.zeros((0, 4, self.num_classes), dtype=torch.int64)
        return (self._parts[0] if len(self._parts) == 1 else torch.cat(self._parts)).cpu()

    def compute(self):
        """`boundary_scores` of `counts()`: {"bf", "bf_per_class", "precision", "recall", "pooled", "images"}."""
        return boundary_scores(self.counts().numpy(), self.ignore_index)


def label_boundaries(labels, num_classes=12, ignore_index=11, void_from=None):
    """uint8 [N,H,W]: the class whose 4-connected boundary each pixel of the int64 map `labels` carries under BoundaryMeter's rule, 255
    where it carries none.  `void_from` is the label map whose `ignore_index` pixels are void (for a prediction map); None: the map's
    own.  The kernel shares the rule's device function with the counting kernel."""
    _check_boundary_maps("label_boundaries", labels, labels if void_from is None else void_from)
    if not 1 <= num_classes <= 32:
        raise ValueError(f"label_boundaries serves 1 to 32 classes. Got: {num_classes}")
    lib = _lib.load()
    m = labels.contiguous()
    v = None if void_from is None else void_from.contiguous()
    N, H, W = m.shape
    out = torch.empty((N, H, W), device=m.device, dtype=torch.uint8)
    check(lib.cvk_boundary_map(m.data_ptr(), None if v is None else v.data_ptr(), out.data_ptr(), N, H, W, int(num_classes),
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
    import numpy as np
    from fractions import Fraction
    qnum, qden = surface_percentile(percentile)
    rec = np.asarray(records, dtype=np.int64)
    if rec.ndim != 4 or rec.shape[1] != 2 or rec.shape[3] != SURFACE_RECORD_SLOTS:
        raise ValueError(f"expected records of shape [images, 2, K, {SURFACE_RECORD_SLOTS}], got {list(rec.shape)}")
    K = rec.shape[2]
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

    def masked_mean(v, axis):
        n = ev.sum(axis=axis)
        return np.divide(np.where(ev, v, 0.0).sum(axis=axis), n, out=np.full(n.shape, np.nan), where=n > 0)

    out = {}
    scored = ev.any(axis=1)
    for name, v in (("hd95", hdq), ("hd", hd), ("assd", assd)):
        image = masked_mean(v, 1)
        per_class = masked_mean(v, 0)
        if ignore_index is not None and 0 <= ignore_index < K:
            per_class[ignore_index] = np.nan
        out[name] = float(image[scored].mean()) if scored.any() else float("nan")
        out[name + "_per_class"] = per_class
    out["unmatched"], out["images"] = unmatched, int(scored.sum())
    out["percentile"] = float(Fraction(qnum, qden) * 100)
    return out


class _SurfaceBuffers:
    """The device buffers of cvk_surface_distances, kept per (N, H, W, classes, device): the workspace and the meter's d2 planes."""

    _buffers = {}

    @staticmethod
    def get(lib, N, H, W, C, device, want_d2):
        key = (N, H, W, C, str(device))
        ent = _SurfaceBuffers._buffers.get(key)
        if ent is None:
            nbytes = lib.cvk_surface_workspace_bytes(N, H, W, C)
            if nbytes <= 0:
                raise ValueError(f"surface distances serve 1 to {EDT_MAX_CLASSES} classes, H <= 65534, (H - 1)^2 + (W - 1)^2 < 2^24 and "
                                 f"fewer than 2^31 pixels, got N = {N}, H = {H}, W = {W}, classes = {C}")
            ent = _SurfaceBuffers._buffers[key] = [torch.empty(nbytes, device=device, dtype=torch.uint8), None]
        if want_d2 and ent[1] is None:
            ent[1] = torch.empty((2, N, H, W), device=device, dtype=torch.int32)
        return ent


def _surface_call(who, pred, label, num_classes, ignore_index, frac, d2):
    """One cvk_surface_distances call; d2 None: the kept planes of this shape.  Returns (d2, record)."""
    _check_boundary_maps(who, pred, label)
    lib = _lib.load()
    N, H, W = pred.shape
    ws, kept = _SurfaceBuffers.get(lib, N, H, W, num_classes, pred.device, d2 is None)
    if d2 is None:
        d2 = kept
    p = pred.contiguous(); l = label.contiguous()
    record = torch.empty((N, 2, num_classes, SURFACE_RECORD_SLOTS), device=p.device, dtype=torch.int64)
    check(lib.cvk_surface_distances(p.data_ptr(), l.data_ptr(), N, H, W, num_classes, ignore_index, frac[0], frac[1], ws.data_ptr(),
                                    d2.data_ptr(), record.data_ptr(), _stream(p)), "cvk_surface_distances")
    return d2, record


def _check_surface_classes(who, num_classes):
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= EDT_MAX_CLASSES:
        raise ValueError(f"{who} serves 1 to {EDT_MAX_CLASSES} classes. Got: {num_classes}")
    return num_classes


def surface_distances(pred, label, num_classes=12, ignore_index=11, percentile=95):
    """Contour-to-contour distances of int64 maps [N,H,W] on the GPU, per image and class, under BoundaryMeter's contour rule
    (include/cvk.h, cvk_surface_distances): `d2` int32 [2,N,H,W], plane 0 the exact squared Euclidean distance from each contour pixel
    of the prediction to the nearest contour pixel of its class in the label map (-1: the label map has none), plane 1 the same from
    the label's contour pixels to the prediction's, -2 at every other pixel; `record` int64 [N,2,num_classes,8], per (image, direction,
    class): n, m, max d2, Q (the sum of the distances in 2^-16 pixels, by integers), and the ranks and values of the `percentile`:
    k, r, d2_lo, d2_hi.  Both are new device tensors; no host sync.  `surface_distance_scores` turns records into scores."""
    _check_surface_classes("surface_distances", num_classes)
    frac = surface_percentile(percentile)
    _check_boundary_maps("surface_distances", pred, label)
    d2 = torch.empty((2,) + tuple(pred.shape), device=pred.device, dtype=torch.int32)
    return _surface_call("surface_distances", pred, label, num_classes, int(ignore_index), frac, d2)


class SurfaceDistanceMeter:
    """Hausdorff distance (HD), its percentile (HD95 by default; MONAI's compute_hausdorff_distance(percentile=95), medpy's hd95) and
    the average symmetric surface distance (ASSD) of predictions against labels, per image and class, between the 4-connected contours
    of BoundaryMeter's rule.  Distances, sums and the exact order statistics are made on the device by one cvk_surface_distances call
    per batch (integers only: two runs agree bit for bit); no host sync until `records()` / `compute()`.  Pixels whose label is
    `ignore_index` are void in both maps.  A class whose contour exists in only one map of an image is counted as unmatched and enters
    no mean."""

    def __init__(self, num_classes=12, ignore_index=11, percentile=95):
        self.num_classes = _check_surface_classes("SurfaceDistanceMeter", num_classes)
        self.ignore_index, self.percentile = int(ignore_index), percentile
        self._frac = surface_percentile(percentile)
        self._parts = []

    def reset(self):
        self._parts = []

    def update(self, pred, label):
        _, record = _surface_call("SurfaceDistanceMeter.update", pred, label, self.num_classes, self.ignore_index, self._frac, None)
        self._parts.append(record)

    def records(self):
        """int64 [images, 2, num_classes, 8] on the host, in the order of the updates — one device->host copy."""
        if not self._parts:
            return torch.zeros((0, 2, self.num_classes, SURFACE_RECORD_SLOTS), dtype=torch.int64)
        return (self._parts[0] if len(self._parts) == 1 else torch.cat(self._parts)).cpu()

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


def _check_cheb_classes(who, num_classes):
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= 32:
        raise ValueError(f"{who} serves 1 to 32 classes. Got: {num_classes}")
    return num_classes


def _check_depth(name, d):
    if isinstance(d, bool) or not isinstance(d, int) or not 1 <= d <= CHEB_MAX_DEPTH:
        raise ValueError(f"{name} must be an integer in 1..{CHEB_MAX_DEPTH}. Got: {d!r}")
    return d


class _ChebBuffers:
    """The device buffers of cvk_cheb_depth / cvk_boundary_iou_counts, kept per (N, H, W, device): the workspace and the meter's four
    byte maps (code and depth of the prediction, code and depth of the label)."""

    _buffers = {}

    @staticmethod
    def get(lib, N, H, W, device, want_maps):
        key = (N, H, W, str(device))
        ent = _ChebBuffers._buffers.get(key)
        if ent is None:
            nbytes = lib.cvk_cheb_workspace_bytes(N, H, W)
            if nbytes <= 0:
                raise ValueError(f"the chessboard depth serves rows of up to 32768 pixels and fewer than 2^31 pixels, got N = {N}, "
                                 f"H = {H}, W = {W}")
            ent = _ChebBuffers._buffers[key] = [torch.empty(nbytes, device=device, dtype=torch.uint8), None]
        if want_maps and ent[1] is None:
            ent[1] = torch.empty((4, N, H, W), device=device, dtype=torch.uint8)
        return ent


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
    _check_boundary_maps("chessboard_depth", labels, labels if void_from is None else void_from)
    _check_cheb_classes("chessboard_depth", num_classes)
    _check_depth("max_depth", max_depth)
    lib = _lib.load()
    m = labels.contiguous()
    v = None if void_from is None else void_from.contiguous()
    N, H, W = m.shape
    ws, _ = _ChebBuffers.get(lib, N, H, W, m.device, False)
    code = torch.empty((N, H, W), device=m.device, dtype=torch.uint8)
    depth = torch.empty((N, H, W), device=m.device, dtype=torch.uint8)
    _cheb_call(lib, m, v, code, depth, ws, num_classes, int(ignore_index), max_depth, border)
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
    import numpy as np
    c = np.asarray(counts, dtype=np.int64)
    if c.ndim != 3 or c.shape[1] != BIOU_ROWS:
        raise ValueError(f"expected counts of shape [images, {BIOU_ROWS}, K], got {list(c.shape)}")
    K = c.shape[2]

    def ratio(i, a, b):
        den = (a + b - i).astype(np.float64)
        return np.divide(i.astype(np.float64), den, out=np.full(den.shape, np.nan), where=den > 0)

    pooled = c.sum(axis=0)
    per_class = ratio(pooled[2], pooled[0], pooled[1])
    mask_iou = ratio(pooled[5], pooled[3], pooled[4])
    if ignore_index is not None and 0 <= ignore_index < K:
        per_class[ignore_index] = mask_iou[ignore_index] = np.nan
    ev = ~np.isnan(per_class)
    per_image = ratio(c[:, 2], c[:, 0], c[:, 1])          # [images, K], NaN where bG + bP == 0 (the union is then 0 too)
    if ignore_index is not None and 0 <= ignore_index < K:
        per_image[:, ignore_index] = np.nan
    evi = ~np.isnan(per_image)
    ni = evi.sum(axis=1)
    image = np.divide(np.where(evi, per_image, 0.0).sum(axis=1), ni, out=np.full(ni.shape, np.nan), where=ni > 0)
    scored = ni > 0
    return {"biou": float(per_class[ev].mean()) if ev.any() else float("nan"), "biou_per_class": per_class,
            "biou_image": float(image[scored].mean()) if scored.any() else float("nan"),
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
    import numpy as np
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

    def __init__(self, num_classes=12, ignore_index=11, ratio=0.02, dilation=None, trimap_widths=()):
        self.num_classes = _check_cheb_classes("BoundaryIoUMeter", num_classes)
        self.ignore_index, self.ratio = int(ignore_index), ratio
        self.dilation = None if dilation is None else _check_depth("dilation", dilation)
        if dilation is None:
            boundary_dilation(1, 1, ratio)                # a bad ratio fails here, not in the first batch
        self.trimap_widths = _check_widths(trimap_widths)
        import ctypes
        self._widths = (ctypes.c_int * max(1, len(self.trimap_widths)))(*self.trimap_widths)
        self.reset()

    def reset(self):
        self._parts, self._trimap = [], None

    def update(self, pred, label):
        _check_boundary_maps("BoundaryIoUMeter.update", pred, label)
        lib = _lib.load()
        N, H, W = pred.shape
        K, nw = self.num_classes, len(self.trimap_widths)
        d = self.dilation if self.dilation is not None else boundary_dilation(H, W, self.ratio)
        max_depth = max((d,) + self.trimap_widths)
        p = pred.contiguous(); l = label.contiguous()
        ws, maps = _ChebBuffers.get(lib, N, H, W, p.device, True)
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
        if not self._parts:
            return torch.zeros((0, BIOU_ROWS, self.num_classes), dtype=torch.int64)
        return (self._parts[0] if len(self._parts) == 1 else torch.cat(self._parts)).cpu()

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
    _check_cheb_classes(who, num_classes)
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


class _RegionBuffers:
    """The device buffers of cvk_cc_label / cvk_cc_filter, kept per (N, H, W, classes, device): the workspace, and two pairs of
    (labels, area) for the callers that keep the maps to themselves (the filter and the meter)."""

    _buffers = {}

    @staticmethod
    def get(lib, N, H, W, C, device):
        key = (N, H, W, C, str(device))
        ent = _RegionBuffers._buffers.get(key)
        if ent is None:
            nbytes = lib.cvk_cc_workspace_bytes(N, H, W, C)
            if nbytes <= 0:
                raise ValueError(f"connected components serve 1 to 32 classes and fewer than 2^31 pixels, got N = {N}, H = {H}, W = {W}, "
                                 f"{C} classes")
            ent = _RegionBuffers._buffers[key] = {"ws": torch.empty(nbytes, device=device, dtype=torch.uint8),
                                                  "maps": torch.empty((2, 2, N, H, W), device=device, dtype=torch.int32)}
        return ent


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
    ent = _RegionBuffers.get(lib, N, H, W, num_classes, m.device)
    if "public" not in ent:
        ent["public"] = torch.empty((2, N, H, W), device=m.device, dtype=torch.int32)
    lab, area = ent["public"][0], ent["public"][1]
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
        ent = _RegionBuffers.get(lib, N, H, W, self.num_classes, m.device)
        lab, area = ent["maps"][pair][0], ent["maps"][pair][1]
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
    import numpy as np
    rp, rl, h = (np.asarray(a, dtype=np.int64) for a in (records_pred, records_label, hist))
    K = rp.shape[0]
    frag = np.divide(rp[:, 0].astype(np.float64), rl[:, 0], out=np.full(K, np.nan), where=rl[:, 0] > 0)
    union = (h[1] + h[2] - h[0]).astype(np.float64)
    iou = np.divide(h[0].astype(np.float64), union, out=np.full(K, np.nan), where=union > 0)
    if ignore_index is not None and 0 <= ignore_index < K:
        frag[ignore_index] = iou[ignore_index] = np.nan
    ev, evi = ~np.isnan(frag), ~np.isnan(iou)
    return {"regions_pred": rp[:, 0].copy(), "regions_label": rl[:, 0].copy(), "small_regions_pred": rp[:, 3].copy(),
            "fragmentation_per_class": frag, "fragmentation": float(frag[ev].mean()) if ev.any() else float("nan"),
            "iou_filtered": iou, "miou_filtered": float(iou[evi].mean()) if evi.any() else float("nan")}


class RegionMeter:
    """Fragmentation of predictions against labels, and the mIoU after despeckling.  `update(pred, label)` labels the components of
    both maps, filters the prediction as `RegionFilter(min_area, ..., mode)` does (the labels take no part in that, as at deployment;
    void is the prediction's own `ignore_index` pixels) and adds the filtered prediction's confusion counts against the label and both
    maps' records, all on the device.  `compute()` (one device->host copy) returns "regions_pred", "regions_label",
    "small_regions_pred" (int64 per class, pooled over the images; the prediction's are those before the filter),
    "fragmentation_per_class" (predicted regions over label regions; NaN for a class without a label region and at `ignore_index`),
    "fragmentation" (its mean over the classes that occur), "iou_filtered", "miou_filtered" and "images"."""

    def __init__(self, num_classes=12, ignore_index=11, min_area=64, connectivity=4, mode="neighbor"):
        self._filter = RegionFilter(min_area, num_classes, ignore_index, connectivity, mode)
        self._count = RegionFilter(1, num_classes, ignore_index, connectivity, "fill")       # removes nothing: the label's record
        self.num_classes, self.ignore_index, self.min_area = num_classes, int(ignore_index), min_area
        self.connectivity, self.mode = connectivity, mode
        self.reset()

    def reset(self):
        self._sums, self.images = None, 0

    def update(self, pred, label):
        _check_boundary_maps("RegionMeter.update", pred, label)
        if pred.numel() >= 2 ** 31:
            raise ValueError(f"RegionMeter.update: {pred.numel()} pixels, the kernels serve fewer than 2^31")
        lib = _lib.load()
        p, l = pred.contiguous(), label.contiguous()
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
    import numpy as np
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


# reference conf/settings.py:8-9 (BGR order, as cv2 decodes)
CAMVID_MEAN = (0.42019099703461577, 0.41323568513979647, 0.4010048431259079)
CAMVID_STD = (0.30598050258519743, 0.3089986932156864, 0.3054061869915674)


def preprocess_uint8(images_u8, mean=CAMVID_MEAN, std=CAMVID_STD):
    """Device-side ToTensor + Normalize (reference transforms.py:485-538): uint8 [N,H,W,3] on the GPU -> float32
    logical [N,3,H,W] (a channels_last view of an NHWC-4 buffer).  Replaces the per-sample CPU float conversion and the
    pageable `images.cuda()` copy of 4 bytes/value (train.py:126) by a 1 byte/value upload + one kernel."""
    import ctypes
    lib = _lib.load()
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3 or not images_u8.is_cuda:
        raise ValueError("expected a uint8 HIP tensor of shape [N, H, W, 3]")
    src = images_u8.contiguous()
    N, H, W, _ = src.shape
    dst = torch.empty((N, H, W, 4), device=src.device, dtype=torch.float32)
    m = (ctypes.c_float * 3)(*mean); sd = (ctypes.c_float * 3)(*std)
    check(lib.cvk_preprocess_u8(src.data_ptr(), dst.data_ptr(), N, H, W, m, sd, _stream(src)), "cvk_preprocess_u8")
    return dst[..., :3].permute(0, 3, 1, 2)


def _check_images(who, images):
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.float32:
        raise ValueError("expected float32 images of shape [N, 3, H, W]")
    if not images.is_cuda:
        raise RuntimeError(f"pytorch_camvid_amd.{who} needs HIP tensors (no CPU fallback)")


def _int_pair(name, v):
    ok = isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(e, int) and not isinstance(e, bool) and e >= 1 for e in v)
    if not ok:
        raise ValueError(f"{name} must be a pair of positive integers (height, width). Got: {v!r}")
    return int(v[0]), int(v[1])


class SlidingWindow:
    """Sliding-window inference: the network runs on overlapping crops of an image of any size and the windows' logits are averaged
    where they overlap, merged on the device (cvk_window_merge).

      sw = SlidingWindow(crop=(360, 480), stride=(240, 320))
      logits, pred = sw(net, images)

    The grid is the one of mmseg's mode='slide' (include/cvk.h): for images [N,3,H,W] the windows are hw x ww = min(crop, image) per
    side, (max(H - hc, 0) + sy - 1) // sy + 1 rows of them starting at min(i * sy, H - hw) (columns likewise), visited in row-major
    order; the last row and column are pulled back inside the image, never padded.  A window's network input is the view
    images[:, :, y1:y1+hw, x1:x1+ww] (no copy: the network's import reads any strides).  One launch per window adds its logits into
    the full-size map; the launch of the last window that covers a pixel divides by the pixel's window count and takes the arg-max:
    logits = ((l_1 + l_2) + ...) / float32(count) in visiting order, pred = its first-maximum arg-max
    (`torch.equal(pred, argmax_channels(logits))`).  No count matrix, cleared buffer, atomics or host synchronisation, so two runs
    agree bitwise, and where one window covers a pixel the value is that window's logit bit for bit.

    `logits` is float32 [N,C,H,W], a channels_last view of the buffer this object keeps per (N, C, H, W, device): the next call with
    that shape overwrites it (clone it to keep it).  `pred` is a fresh int64 [N,H,W].  The network runs in eval mode under no_grad and
    gets its `training` flag back.  Networks in bf16 mode or with split operands work unchanged (their logits are float32 at the module
    boundary), and so does a call inside `opt.swap_ema()`.  At most 32 classes.  One cached plan of the network, at the window size,
    serves every image size.  A size the network cannot run raises whatever the network raises."""

    def __init__(self, crop=(360, 480), stride=(240, 320)):
        self.crop, self.stride = _int_pair("crop", crop), _int_pair("stride", stride)
        if self.stride[0] > self.crop[0] or self.stride[1] > self.crop[1]:
            raise ValueError(f"stride must not exceed crop (pixels between two windows would be skipped). Got: stride {self.stride}, "
                             f"crop {self.crop}")
        self._out = {}

    def _grid(self, H, W):
        """(hw, ww, [y1 per grid row], [x1 per grid column])."""
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError(f"an image of {H} x {W} has no pixel")
        (hc, wc), (sy, sx) = self.crop, self.stride
        hw, ww = min(hc, H), min(wc, W)
        gy, gx = (H - hw + sy - 1) // sy + 1, (W - ww + sx - 1) // sx + 1
        return hw, ww, [min(i * sy, H - hw) for i in range(gy)], [min(j * sx, W - ww) for j in range(gx)]

    def windows(self, H, W):
        """[(y1, x1, hw, ww), ...] in visiting order (row-major) for an image size (H, W).  Host arithmetic only."""
        hw, ww, ys, xs = self._grid(H, W)
        return [(y1, x1, hw, ww) for y1 in ys for x1 in xs]

    def counts(self, H, W):
        """int64 [H, W]: how many windows cover each pixel.  Host arithmetic only."""
        hw, ww, ys, xs = self._grid(H, W)
        cy, cx = torch.zeros(int(H), dtype=torch.int64), torch.zeros(int(W), dtype=torch.int64)
        for y1 in ys:
            cy[y1:y1 + hw] += 1
        for x1 in xs:
            cx[x1:x1 + ww] += 1
        return cy[:, None] * cx[None, :]

    def _merge(self, net, images, want_pred):
        lib = _lib.load()
        _check_images("SlidingWindow", images)
        N, _, H, W = images.shape
        hw, ww, ys, xs = self._grid(H, W)
        (hc, wc), (sy, sx) = self.crop, self.stride
        out = pred = None
        C = None
        was_training = net.training
        net.eval()
        try:
            with torch.no_grad():
                for iy, y1 in enumerate(ys):
                    for ix, x1 in enumerate(xs):
                        logits = net(images[:, :, y1:y1 + hw, x1:x1 + ww])
                        if not isinstance(logits, torch.Tensor) or logits.dim() != 4:
                            raise ValueError("the network must return logits of shape [N, C, h, w]")
                        if logits.dtype != torch.float32 or not logits.is_cuda:
                            raise RuntimeError(f"expected float32 logits on a HIP device, got {logits.dtype} on {logits.device}")
                        if out is None:
                            C = logits.shape[1]
                            if not 1 <= C <= 32:
                                raise ValueError(f"pytorch_camvid_amd.SlidingWindow serves 1 to 32 classes, got C = {C}")
                            key = (N, C, H, W, logits.device)
                            out = self._out.get(key)
                            if out is None:
                                out = self._out[key] = torch.empty((N, H, W, C), device=logits.device, dtype=torch.float32)
                            if want_pred:
                                pred = torch.empty((N, H, W), device=logits.device, dtype=torch.int64)
                        if tuple(logits.shape) != (N, C, hw, ww) or logits.device != out.device:
                            raise ValueError(f"window ({iy}, {ix}) at ({y1}, {x1}): the network returned logits {list(logits.shape)} on "
                                             f"{logits.device}, the merge expects {[N, C, hw, ww]} on {out.device}")
                        lg, ld = _as_nhwc(logits.detach())
                        check(lib.cvk_window_merge(lg.data_ptr(), ld, out.data_ptr(), pred.data_ptr() if want_pred else None, N, H, W, C,
                                                   hc, wc, sy, sx, iy, ix, _stream(logits)), "cvk_window_merge")
        finally:
            net.train(was_training)
        return out.permute(0, 3, 1, 2), pred

    def __call__(self, net, images):
        """(logits float32 [N,C,H,W], pred int64 [N,H,W]) of one batch; see the class."""
        return self._merge(net, images, True)

    def logits(self, net, images):
        """The merged logits alone (float32 [N,C,H,W], the same buffer `sw(net, images)` returns): no arg-max is taken."""
        return self._merge(net, images, False)[0]


def _check_window(window):
    if window is not None and not isinstance(window, SlidingWindow):
        raise ValueError(f"window must be a pytorch_camvid_amd.SlidingWindow or None. Got: {window!r}")


class TestTimeAugmentation:
    """Multi-scale and horizontal-flip test-time inference, merged on the device (cvk_tta_accumulate, cvk_tta_resize_input).

      tta = TestTimeAugmentation(scales=(0.75, 1.0, 1.25), flip=True, size_divisor=1)
      probs, pred = tta(net, images)

    For images [N,3,H,W] the views are, in this order, `for s in scales: unflipped, then mirrored (if flip)`, each at
    h = size_divisor * ceil(floor(H * s + 0.5) / size_divisor) (w likewise), resampled bilinearly (align_corners=False).  Every
    view's logits, of whatever spatial size the network returns, are resampled to H x W, soft-maxed, mirrored back where the view
    was mirrored, and averaged: probs = ((p_1 + p_2) + ... + p_K) * float32(1 / K) in view order, pred = its first-maximum arg-max
    (`torch.equal(pred, argmax_channels(probs))`).  One launch per view does all of that; no resized, soft-maxed or flipped tensor
    is written, nothing synchronises with the host and no atomics are used, so two runs agree bitwise.  Bilinear weights come from
    integer arithmetic (include/cvk.h), so they are correctly rounded at any size.

    `probs` is float32 [N,C,H,W], a channels_last view of the accumulator this object keeps per output shape: the next call with
    that shape overwrites it (clone it to keep it).  `pred` is a fresh int64 [N,H,W].  The network runs in eval mode under no_grad
    and gets its `training` flag back.  Networks in bf16 mode or with split operands work unchanged (their logits are float32 at
    the module boundary), and so does a call inside `opt.swap_ema()`.  At most 32 classes.  Every distinct view size is one more
    cached plan of the network (DESIGN.md states the memory).  A size the network cannot run raises whatever the network raises.

    With `window` (a SlidingWindow) every view's logits are `window.logits(net, view)` instead of `net(view)`: the network runs on
    crops of the view and the merged map, dense logits at the view's size, goes through everything above unchanged (evaluate_report's
    loss view sees the merged logits).  One plan at the crop size then serves every scale."""

    __test__ = False                    # the name starts with "Test": not a pytest class

    def __init__(self, scales=(0.75, 1.0, 1.25), flip=True, size_divisor=1, window=None):
        import math
        try:
            scales = tuple(float(s) for s in scales)
        except (TypeError, ValueError):
            raise ValueError(f"scales must be a non-empty sequence of positive finite numbers. Got: {scales!r}") from None
        if not scales or not all(math.isfinite(s) and s > 0.0 for s in scales):
            raise ValueError(f"scales must be a non-empty sequence of positive finite numbers. Got: {scales!r}")
        if isinstance(size_divisor, bool) or not isinstance(size_divisor, int) or size_divisor < 1:
            raise ValueError(f"size_divisor must be an integer >= 1. Got: {size_divisor!r}")
        _check_window(window)
        self.scales, self.flip, self.size_divisor, self.window = scales, bool(flip), size_divisor, window
        self._acc = {}

    def _plan(self, H, W):
        """[(scale, h, w, flipped)] in view order."""
        import math
        d = self.size_divisor
        out = []
        for s in self.scales:
            h = d * math.ceil(math.floor(H * s + 0.5) / d)
            w = d * math.ceil(math.floor(W * s + 0.5) / d)
            if h < 1 or w < 1:
                raise ValueError(f"scale {s} of a {H} x {W} image leaves no pixel")
            out.append((s, h, w, False))
            if self.flip:
                out.append((s, h, w, True))
        return out

    def view_sizes(self, H, W):
        """[(h, w, flipped), ...] in view order for a label size (H, W).  Host arithmetic only."""
        return [(h, w, f) for _, h, w, f in self._plan(int(H), int(W))]

    def loss_view(self, H, W):
        """Index of the view evaluate_report takes its loss from: scale 1.0, not mirrored, at the label size; None when there is none."""
        for i, (s, h, w, f) in enumerate(self._plan(int(H), int(W))):
            if s == 1.0 and not f and (h, w) == (H, W):
                return i
        return None

    @staticmethod
    def _check_images(images):
        _check_images("TestTimeAugmentation", images)

    def views(self, images):
        """The network inputs, in view order (what `tta(net, images)` feeds the network): the scale-1.0 unmirrored view at the image
        size is `images` itself, every other one a fresh float32 [N,3,h,w] view of an NHWC-4 buffer (as `preprocess_uint8` returns),
        written by one launch."""
        self._check_images(images)
        lib = _lib.load()
        N, _, H, W = images.shape
        src = images.detach()
        for s, h, w, flipped in self._plan(H, W):
            if s == 1.0 and not flipped and (h, w) == (H, W):
                yield images
                continue
            dst = torch.empty((N, h, w, 4), device=images.device, dtype=torch.float32)
            check(lib.cvk_tta_resize_input(src.data_ptr(), *src.stride(), dst.data_ptr(), N, H, W, h, w, int(flipped), _stream(images)),
                  "cvk_tta_resize_input")
            yield dst[..., :3].permute(0, 3, 1, 2)

    def _merge(self, net, images, on_logits=None):
        lib = _lib.load()
        self._check_images(images)
        N, _, H, W = images.shape
        plan = self._plan(H, W)
        K = len(plan)
        import numpy as np
        inv_k = float(np.float32(1.0) / np.float32(K))
        acc = pred = None
        C = None
        was_training = net.training
        net.eval()
        try:
            with torch.no_grad():
                for i, ((s, h, w, flipped), x) in enumerate(zip(plan, self.views(images))):
                    logits = net(x) if self.window is None else self.window.logits(net, x)
                    if not isinstance(logits, torch.Tensor) or logits.dim() != 4:
                        raise ValueError("the network must return logits of shape [N, C, h, w]")
                    if logits.dtype != torch.float32 or not logits.is_cuda:
                        raise RuntimeError(f"expected float32 logits on a HIP device, got {logits.dtype} on {logits.device}")
                    if acc is None:
                        C = logits.shape[1]
                        if not 1 <= C <= 32:
                            raise ValueError(f"pytorch_camvid_amd.TestTimeAugmentation serves 1 to 32 classes, got C = {C}")
                        key = (N, C, H, W, logits.device)
                        acc = self._acc.get(key)
                        if acc is None:
                            acc = self._acc[key] = torch.empty((N, H, W, C), device=logits.device, dtype=torch.float32)
                        pred = torch.empty((N, H, W), device=logits.device, dtype=torch.int64)
                    if logits.shape[0] != N or logits.shape[1] != C or logits.device != acc.device:
                        raise ValueError(f"view {i} ({h} x {w}{', mirrored' if flipped else ''}): the network returned logits "
                                         f"{list(logits.shape)} on {logits.device}, the accumulator is {[N, C, H, W]} on {acc.device}")
                    if on_logits is not None:
                        on_logits(i, logits)
                    lg, ld = _as_nhwc(logits.detach())
                    lh, lw = lg.shape[1], lg.shape[2]
                    check(lib.cvk_tta_accumulate(lg.data_ptr(), ld, lh, lw, acc.data_ptr(), pred.data_ptr(), N, H, W, C, int(flipped),
                                                 int(i == 0), int(i == K - 1), inv_k, _stream(logits)), "cvk_tta_accumulate")
        finally:
            net.train(was_training)
        return acc.permute(0, 3, 1, 2), pred

    def __call__(self, net, images):
        """(probs float32 [N,C,H,W], pred int64 [N,H,W]) of one batch; see the class."""
        return self._merge(net, images)


CRF_MAX_RADIUS, CRF_MAX_DILATION = 5, 4          # include/cvk.h: the window of cvk_crf_step


def _crf_numbers(name, v, n, positive_from):
    import math
    try:
        out = tuple(float(e) for e in v)
    except (TypeError, ValueError):
        out = ()
    ok = len(out) == n and all(math.isfinite(e) for e in out) and out[0] >= 0.0 and all(e > 0.0 for e in out[positive_from:])
    if not ok:
        raise ValueError(f"{name} must be {n} finite numbers, a weight >= 0 followed by widths > 0. Got: {v!r}")
    return out


def _crf_window(radius, dilation):
    for name, v, hi in (("radius", radius, CRF_MAX_RADIUS), ("dilation", dilation, CRF_MAX_DILATION)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= hi:
            raise ValueError(f"{name} must be an integer in 1..{hi}. Got: {v!r}")
    return radius, dilation


def crf_coefficients(radius=3, dilation=1, appearance=(4.0, 8.0, 13.0), smoothness=(3.0, 3.0)):
    """(ga, gs, cb, wa, ws): exactly the numbers cvk_crf_step gets.  ga, gs are float32 numpy arrays [2r+1, 2r+1] over the offsets
    (d i, d j) in row-major (i, j): ga = float32(exp(-|o|^2 / (2 theta_alpha^2))), gs the same with theta_gamma; cb =
    float32(-1 / (2 theta_beta^2)); wa, ws the two weights as float32.  Each is evaluated in double and rounded once.  The centre
    entry of a table (offset (0, 0)) is never read."""
    import numpy as np
    r, d = _crf_window(radius, dilation)
    wa, theta_alpha, theta_beta = _crf_numbers("appearance", appearance, 3, 1)
    ws, theta_gamma = _crf_numbers("smoothness", smoothness, 2, 1)
    i = np.arange(-r, r + 1, dtype=np.float64) * d
    o2 = i[:, None] ** 2 + i[None, :] ** 2
    ga = np.exp(-o2 / (2.0 * theta_alpha * theta_alpha)).astype(np.float32)
    gs = np.exp(-o2 / (2.0 * theta_gamma * theta_gamma)).astype(np.float32)
    cb = float(np.float32(-1.0 / (2.0 * theta_beta * theta_beta)))
    if not (np.isfinite(np.float32(wa)) and np.isfinite(np.float32(ws)) and np.isfinite(cb)):
        raise ValueError("appearance / smoothness leave float32's range")
    return ga, gs, cb, float(np.float32(wa)), float(np.float32(ws))


def crf_tile(num_classes, radius=3, dilation=1):
    """(tile height, tile width, staged) of cvk_crf_step for a class count and a window: the pixels one work-group produces and
    whether their neighbourhood is staged in LDS (True) or read from global memory (False).  No GPU needed."""
    import ctypes
    lib = _lib.load()
    th, tw, st = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.cvk_crf_tile(int(num_classes), int(radius), int(dilation), ctypes.byref(th), ctypes.byref(tw), ctypes.byref(st))
    if rc != 0:
        raise ValueError(lib.cvk_last_error_string().decode())
    return th.value, tw.value, bool(st.value)


class LocalCRF:
    """Local-window mean-field CRF refinement of a prediction, on the device (cvk_crf_step; the definition is in include/cvk.h).

      crf = LocalCRF(iterations=5, radius=3, dilation=1, appearance=(4.0, 8.0, 13.0), smoothness=(3.0, 3.0))
      probs, pred = crf.refine(logits, images)     # logits [N,C,H,W], images the network's float input [N,3,H,W]
      probs, pred = crf(net, images)               # eval-mode forward under no_grad, then the refinement

    This is the ConvCRF form (Teichmann & Cipolla) with a dilation for reach: every pixel hears the (2 radius + 1)^2 - 1 pixels at
    offsets (dilation i, dilation j) around it, not the whole image; the fully connected permutohedral CRF is not provided.
    `appearance = (wa, theta_alpha in pixels, theta_beta in grey levels of 0..255)`, `smoothness = (ws, theta_gamma)`; the defaults
    are DeepLab's dense-CRF values with theta_alpha scaled to a 7 x 7 window.  `compat` is None (Potts, mu = -I) or a float32 [C,C]
    device tensor mu.  `mean` / `std` are the normalisation of the network's input, undone on load (I = 255 (std x + mean)), so the
    guide is the network input itself, of any strides: no second image tensor exists.  uint8 frames [N,H,W,3] are taken as they are.

    `inner` decides what `crf(net, images)` refines: None, the network's logits; a SlidingWindow, `inner.logits(net, images)`; a
    TestTimeAugmentation, its mean probabilities (a probability unary enters as log(max(p, FLT_MIN))).

    One launch per iteration, no atomics: two runs agree bitwise.  `probs` is float32 [N,C,H,W], a channels_last view of one of the
    two buffers this object keeps per (N, C, H, W, device): the next call with that shape overwrites it (clone it to keep it).
    `pred` is a fresh int64 [N,H,W], the first-maximum arg-max of `probs` (`torch.equal(pred, argmax_channels(probs))`).  Channels_last
    logits are read in place, other layouts copied once.  At most 32 classes.  A LocalCRF has TestTimeAugmentation's return
    contract: `evaluate`, `evaluate_report` and `predict` take it as `tta=`; "loss" is then `loss_fn` of the unrefined logits (with a
    TestTimeAugmentation inside, of its loss view)."""

    def __init__(self, iterations=5, radius=3, dilation=1, appearance=(4.0, 8.0, 13.0), smoothness=(3.0, 3.0), compat=None,
                 mean=CAMVID_MEAN, std=CAMVID_STD, inner=None):
        import ctypes
        import math
        import numpy as np
        if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 1:
            raise ValueError(f"iterations must be an integer >= 1. Got: {iterations!r}")
        self.iterations = iterations
        self.radius, self.dilation = _crf_window(radius, dilation)
        self.ga, self.gs, self.cb, self.wa, self.ws = crf_coefficients(radius, dilation, appearance, smoothness)
        if compat is not None and (not isinstance(compat, torch.Tensor) or compat.dim() != 2 or compat.shape[0] != compat.shape[1]
                                   or compat.dtype != torch.float32):
            raise ValueError("compat must be None or a float32 tensor of shape [C, C]")
        self.compat = None if compat is None else compat.detach().contiguous()
        try:
            mean, std = tuple(float(e) for e in mean), tuple(float(e) for e in std)
        except (TypeError, ValueError):
            mean = std = ()
        if len(mean) != 3 or len(std) != 3 or not all(math.isfinite(e) for e in mean + std) or not all(e > 0.0 for e in std):
            raise ValueError("mean and std must be three finite numbers each, std > 0")
        if inner is not None and not isinstance(inner, (SlidingWindow, TestTimeAugmentation)):
            raise ValueError(f"inner must be None, a SlidingWindow or a TestTimeAugmentation. Got: {inner!r}")
        self.inner = inner
        self.guide_scale = np.array([255.0 * s for s in std], dtype=np.float32)       # a_k, b_k of include/cvk.h, rounded once
        self.guide_offset = np.array([255.0 * m for m in mean], dtype=np.float32)
        taps = (2 * self.radius + 1) ** 2
        self._ga = (ctypes.c_float * taps)(*self.ga.ravel().tolist())
        self._gs = (ctypes.c_float * taps)(*self.gs.ravel().tolist())
        self._a = (ctypes.c_float * 3)(*self.guide_scale.tolist())
        self._b = (ctypes.c_float * 3)(*self.guide_offset.tolist())
        self._buf = {}

    def refine(self, unary, images, unary_is_prob=False):
        """(probs float32 [N,C,H,W], pred int64 [N,H,W]) of a unary [N,C,H,W] (logits, or probabilities with `unary_is_prob`) under
        the guide `images` (float32 [N,3,H,W] of any strides, or uint8 [N,H,W,3]); see the class."""
        lib = _lib.load()
        if not isinstance(unary, torch.Tensor) or unary.dim() != 4 or unary.dtype != torch.float32:
            raise ValueError("expected a float32 unary of shape [N, C, H, W]")
        if not unary.is_cuda:
            raise RuntimeError("pytorch_camvid_amd.LocalCRF needs HIP tensors (no CPU fallback)")
        N, C, H, W = unary.shape
        if not 1 <= C <= 32:
            raise ValueError(f"pytorch_camvid_amd.LocalCRF serves 1 to 32 classes, got C = {C}")
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.device != unary.device:
            raise ValueError("expected the guide images as a 4-D tensor on the unary's device")
        if images.dtype == torch.uint8:
            if tuple(images.shape) != (N, H, W, 3):
                raise ValueError(f"uint8 guide frames must be {[N, H, W, 3]}, got {list(images.shape)}")
            guide, u8, strides = images.contiguous(), 1, (0, 0, 0, 0)
        elif images.dtype == torch.float32:
            if tuple(images.shape) != (N, 3, H, W):
                raise ValueError(f"the float guide must be {[N, 3, H, W]}, got {list(images.shape)}")
            guide, u8, strides = images.detach(), 0, tuple(images.stride())
        else:
            raise ValueError(f"the guide must be float32 [N,3,H,W] or uint8 [N,H,W,3], got {images.dtype}")
        compat = self.compat
        if compat is not None:
            if tuple(compat.shape) != (C, C):
                raise ValueError(f"compat is {list(compat.shape)}, the unary has {C} classes")
            if compat.device != unary.device:
                raise ValueError(f"compat is on {compat.device}, the unary on {unary.device}")
        key = (N, C, H, W, unary.device)
        bufs = self._buf.get(key)
        if bufs is None:
            bufs = self._buf[key] = (torch.empty((N, H, W, C), device=unary.device, dtype=torch.float32),
                                     torch.empty((N, H, W, C), device=unary.device, dtype=torch.float32))
        lg, ld = _as_nhwc(unary.detach())
        if lg.data_ptr() in (bufs[0].data_ptr(), bufs[1].data_ptr()):
            lg, ld = lg.clone(), C                            # an earlier result of this object as the unary: it would be overwritten
        pred = torch.empty((N, H, W), device=unary.device, dtype=torch.int64)
        T, s = self.iterations, _stream(unary)
        for t in range(T):
            q_out, q_in = bufs[t & 1], bufs[(t + 1) & 1]
            check(lib.cvk_crf_step(lg.data_ptr(), ld, int(bool(unary_is_prob)), q_in.data_ptr(), q_out.data_ptr(),
                                   pred.data_ptr() if t == T - 1 else None, guide.data_ptr(), u8, *strides, self._a, self._b, self._ga,
                                   self._gs, self.cb, self.wa, self.ws, None if compat is None else compat.data_ptr(), N, H, W, C,
                                   self.radius, self.dilation, int(t == 0), int(t == T - 1), s), "cvk_crf_step")
        return bufs[(T - 1) & 1].permute(0, 3, 1, 2), pred

    def loss_view(self, H, W):
        """Index of the logits evaluate_report takes its loss from: the inner TestTimeAugmentation's own rule, else 0 (the unrefined
        logits)."""
        return self.inner.loss_view(H, W) if isinstance(self.inner, TestTimeAugmentation) else 0

    def _merge(self, net, images, on_logits=None):
        _check_images("LocalCRF", images)
        if isinstance(self.inner, TestTimeAugmentation):
            probs, _ = self.inner._merge(net, images, on_logits)
            return self.refine(probs, images, unary_is_prob=True)
        if isinstance(self.inner, SlidingWindow):
            logits = self.inner.logits(net, images)
        else:
            was_training = net.training
            net.eval()
            try:
                with torch.no_grad():
                    logits = net(images)
            finally:
                net.train(was_training)
            if not isinstance(logits, torch.Tensor) or logits.dim() != 4:
                raise ValueError("the network must return logits of shape [N, C, h, w]")
            if logits.dtype != torch.float32 or not logits.is_cuda:
                raise RuntimeError(f"expected float32 logits on a HIP device, got {logits.dtype} on {logits.device}")
        if on_logits is not None:
            on_logits(0, logits)
        with torch.no_grad():
            return self.refine(logits.detach(), images)

    def __call__(self, net, images):
        """(probs float32 [N,C,H,W], pred int64 [N,H,W]) of one batch; see the class."""
        return self._merge(net, images)


def crf_refine(logits, images, iterations=5, radius=3, dilation=1, appearance=(4.0, 8.0, 13.0), smoothness=(3.0, 3.0), compat=None,
               mean=CAMVID_MEAN, std=CAMVID_STD, unary_is_prob=False):
    """`LocalCRF(...).refine(logits, images, unary_is_prob)` in one call: (probs, pred), fresh buffers."""
    return LocalCRF(iterations, radius, dilation, appearance, smoothness, compat, mean, std).refine(logits, images, unary_is_prob)


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
    import numpy as np
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


def _evaluate_tta(net, batches, num_classes, ignore_index, tta, loss_fn=None, contour_meters=()):
    """evaluate / evaluate_report with test-time augmentation: (meter, the per-batch losses of the loss view: empty without one).
    `contour_meters` (BoundaryMeter, SurfaceDistanceMeter, BoundaryIoUMeter, RegionMeter) see the predictions the ConfusionMeter sees."""
    meter, losses = None, []

    def keep_loss(masks, want):
        def on_logits(i, logits):
            if i == want:
                losses.append(loss_fn(logits, masks).detach())
        return on_logits

    for images, masks in batches:
        want = tta.loss_view(images.shape[2], images.shape[3]) if loss_fn is not None else None
        _, pred = tta._merge(net, images, keep_loss(masks, want) if want is not None else None)
        if meter is None:
            meter = ConfusionMeter(num_classes, ignore_index, pred.device)
        meter.update(pred, masks)
        for m in contour_meters:
            m.update(pred, masks)
    return meter, losses


def _check_tta_window(who, tta, window):
    _check_window(window)
    if tta is not None and window is not None:
        raise ValueError(f"{who}(): pass tta= or window=, not both; for sliding windows under test-time augmentation pass "
                         "tta=TestTimeAugmentation(..., window=window)")


@torch.no_grad()
def evaluate(net, batches, num_classes=12, ignore_index=11, window=None, tta=None):
    """Validation pass of reference train.py:169-206 / eval.py:44-80 without their bugs: eval-mode forward, device-side
    argmax and histogram accumulation over the WHOLE set, one host copy at the end.
    `batches` yields (images [N,3,H,W] float32, masks [N,H,W] int64) on the GPU.  Returns (accuracy, per-class IoU, mIoU).
    With `tta` (a TestTimeAugmentation) the prediction of a batch is the arg-max of the views' mean probabilities; with `window` (a
    SlidingWindow) it is the arg-max of the windows' merged logits.  One of the two: TestTimeAugmentation(..., window=) combines them."""
    _check_tta_window("evaluate", tta, window)
    if tta is not None:
        meter, _ = _evaluate_tta(net, batches, num_classes, ignore_index, tta)
        if meter is None:
            raise ValueError("evaluate(): no batches")
        return meter.compute()
    was_training = net.training
    net.eval()
    meter = None
    for images, masks in batches:
        if window is None:
            logits = net(images)
            pred = argmax_channels(logits)
        else:
            logits, pred = window(net, images)
        if meter is None:
            meter = ConfusionMeter(num_classes, ignore_index, logits.device)
        meter.update(pred, masks)
    net.train(was_training)
    if meter is None:
        raise ValueError("evaluate(): no batches")
    return meter.compute()


SURFACE_REPORT_KEYS = ("hd95", "hd", "assd", "hd95_per_class", "hd_per_class", "assd_per_class")


def _contour_meters(boundary):
    """The meters behind evaluate_report's `boundary`: None, one meter, or a tuple / list with at most one meter of each kind."""
    meters = list(boundary) if isinstance(boundary, (tuple, list)) else [] if boundary is None else [boundary]
    for m in meters:
        if not isinstance(m, (BoundaryMeter, SurfaceDistanceMeter, BoundaryIoUMeter, RegionMeter, CalibrationMeter)):
            raise ValueError("boundary must be a BoundaryMeter or None, or a SurfaceDistanceMeter, or a tuple or list of one of each. "
                             "A BoundaryIoUMeter, a RegionMeter and a CalibrationMeter are taken the same way. "
                             f"Got: {type(m).__name__}")
    if len({type(m) for m in meters}) != len(meters):
        raise ValueError("boundary holds two meters of one kind: their scores would share the report's keys")
    return meters


def _with_boundary(report, contour_meters):
    for m in contour_meters:
        scores = m.compute()
        if isinstance(m, CalibrationMeter):
            keys = CALIBRATION_REPORT_KEYS
        elif isinstance(m, RegionMeter):
            keys = ("fragmentation", "miou_filtered", "regions_pred")
        elif isinstance(m, BoundaryIoUMeter):
            keys = ("biou", "biou_per_class") + (("trimap_miou",) if m.trimap_widths else ())
        else:
            keys = SURFACE_REPORT_KEYS if isinstance(m, SurfaceDistanceMeter) else ("bf", "bf_per_class")
        for k in keys:
            report[k] = scores[k]
    return report


def evaluate_report(net, batches, num_classes=12, ignore_index=11, loss_fn=None, window=None, boundary=None, tta=None):
    """The report of reference eval.py:44-80: {"miou", "precision", "recall", "loss" (mean over batches), "accuracy",
    "iou" (per class)} for a set of (images, masks) batches on the GPU; eval-mode forward under no_grad, argmax and
    histograms on the device, one host copy at the end (the reference copies N*H*W int64 per batch, eval.py:60-62).
    With `tta` (a TestTimeAugmentation) the predictions are the merged ones and "loss" is `loss_fn` of the logits of the
    scale-1.0 unmirrored view at the label size: None when that view is not among the views.  With `window` (a SlidingWindow) the
    predictions and the logits `loss_fn` sees are the windows' merged ones.  One of the two: TestTimeAugmentation(..., window=) combines
    them.  With `boundary` (a BoundaryMeter) the meter is reset, sees every batch's predictions and masks, and the report gains "bf"
    (the boundary F1 measure) and "bf_per_class"; the meter keeps its counts for `boundary.compute()`.  `boundary` also takes a
    SurfaceDistanceMeter, or a tuple or list with one meter of either kind: a SurfaceDistanceMeter is reset and fed the same way, and
    the report gains "hd95", "hd", "assd" and their "_per_class" arrays; the meter's `compute()` has the rest (unmatched classes,
    images).  A BoundaryIoUMeter is a third kind, alone or beside one of each of the others: the report gains "biou" and
    "biou_per_class", and "trimap_miou" when the meter has trimap widths.  A RegionMeter is a fourth kind: the report gains
    "fragmentation", "miou_filtered" and "regions_pred".  A CalibrationMeter is a fifth kind: it is fed the logits `loss_fn` sees
    (with `window`, the merged ones) and the masks, and the report gains "ece", "mce", "nll" and "brier"; with `tta` it raises
    ValueError (the calibration of merged views is not provided)."""
    _check_tta_window("evaluate_report", tta, window)
    contour_meters = _contour_meters(boundary)
    if tta is not None and any(isinstance(m, CalibrationMeter) for m in contour_meters):
        raise ValueError("evaluate_report(): a CalibrationMeter with tta= is not provided: the merged views have probabilities but no "
                         "logits to calibrate; pass window= or neither")
    loss_fn = loss_fn or CrossEntropyLoss()
    for m in contour_meters:
        m.reset()
    if tta is not None:
        meter, losses = _evaluate_tta(net, batches, num_classes, ignore_index, tta, loss_fn, contour_meters)
        if meter is None:
            raise ValueError("evaluate_report(): no batches")
        acc, iou, miou = meter.compute()
        prec, rec = meter.precision_recall()
        loss = None
        if losses:
            loss_sum = losses[0]
            for l in losses[1:]:
                loss_sum = loss_sum + l
            loss = float(loss_sum) / len(losses)
        return _with_boundary({"miou": miou, "precision": prec, "recall": rec, "loss": loss, "accuracy": acc, "iou": iou}, contour_meters)
    was_training = net.training
    net.eval()
    meter, loss_sum, n = None, None, 0
    with torch.no_grad():
        for images, masks in batches:
            if window is None:
                logits = net(images)
                pred = argmax_channels(logits)
            else:
                logits, pred = window(net, images)
            if meter is None:
                meter = ConfusionMeter(num_classes, ignore_index, logits.device)
            l = loss_fn(logits, masks).detach()
            loss_sum = l if loss_sum is None else loss_sum + l
            n += 1
            meter.update(pred, masks)
            for m in contour_meters:
                m.update(logits if isinstance(m, CalibrationMeter) else pred, masks)
    net.train(was_training)
    if meter is None:
        raise ValueError("evaluate_report(): no batches")
    acc, iou, miou = meter.compute()
    prec, rec = meter.precision_recall()
    return _with_boundary({"miou": miou, "precision": prec, "recall": rec, "loss": float(loss_sum) / n, "accuracy": acc, "iou": iou},
                          contour_meters)


def predict(net, image_u8, out_size=None, mean=CAMVID_MEAN, std=CAMVID_STD, window=None, tta=None):
    """reference predict.py:35-57 from the decoded image onward: `image_u8` is one uint8 [H, W, 3] frame (BGR, as cv2
    decodes; a CPU or GPU tensor or a numpy array) already at the network's input size; normalisation, eval-mode forward
    and channel argmax run on the device.  Returns the int64 class map [H, W]; with out_size=(h, w) it is resized by
    nearest neighbour the way `cv2.resize(..., INTER_NEAREST)` does (predict.py:55; source index floor(dst * in / out)).
    Image decoding / PIL resizing to IMAGE_SIZE stay on the host side (cv2 / PIL are not part of this package).
    With `tta` (a TestTimeAugmentation) the class map is the arg-max of the views' mean probabilities; with `window` (a SlidingWindow)
    the frame may have any size and the class map is the arg-max of the windows' merged logits.  One of the two."""
    _check_tta_window("predict", tta, window)
    dev = next(net.parameters()).device
    img = torch.as_tensor(image_u8)
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[-1] != 3:
        raise ValueError("expected one uint8 image of shape [H, W, 3]")
    x = preprocess_uint8(img.to(dev).unsqueeze(0), mean, std)
    if tta is not None:
        cls = tta(net, x)[1][0]
    elif window is not None:
        cls = window(net, x)[1][0]
    else:
        was_training = net.training
        net.eval()
        with torch.no_grad():
            cls = argmax_channels(net(x))[0]
        net.train(was_training)
    if out_size is not None:
        h, w = out_size
        H, W = cls.shape
        yi = torch.clamp((torch.arange(h, device=dev, dtype=torch.float64) * (H / h)).floor().long(), max=H - 1)
        xi = torch.clamp((torch.arange(w, device=dev, dtype=torch.float64) * (W / w)).floor().long(), max=W - 1)
        cls = cls[yi][:, xi]
    return cls


class DevicePrefetcher:
    """the reference converts every frame to float on the CPU (transforms.py:485-538) and uploads 4 bytes per
    value from pageable memory inside the step (`images.cuda()`, train.py:126-127).  This iterator takes (uint8 frames
    [N,H,W,3] BGR, int64 masks [N,H,W]) batches from any host iterable (numpy arrays or CPU tensors), stages them in
    pinned buffers and uploads 1 byte per value on a side stream one batch ahead of the consumer; normalisation to the
    network's float NHWC layout happens on the device (`preprocess_uint8`).  Yields (images float32 [N,3,H,W] view, masks).
    The yielded tensors are safe to use on the current stream (the side stream's work is awaited before they are handed out).
    With `transforms` (a `transforms.Compose`, e.g. `transforms.train_transforms()`) each batch's augmentation parameters are
    drawn while it is staged, in batch order, and go up with its frames (pinned records, same side stream); the frames then pass
    through `cvk_augment_u8` instead of `preprocess_uint8` (masks uint8 or int64; uint8 ones travel at 1 byte per pixel) and the
    masks come back int64 at the transforms' output size.  `transforms` supplies its own Normalize mean / std.
    A `transforms.CropCompose` (e.g. `transforms.crop_transforms()`) is served the same way: its records (`cvk_crop_record`) are
    drawn while the batch is staged and go up from the pinned slot; `cvk_crop_select` and `cvk_crop_augment_u8` run on the
    consumer's stream and the batch comes back at the crop size."""

    def __init__(self, batches, device="cuda", mean=CAMVID_MEAN, std=CAMVID_STD, transforms=None):
        self.it = iter(batches)
        self.dev = torch.device(device)
        self.mean, self.std = mean, std
        self.transforms = transforms
        self.stream = torch.cuda.Stream(self.dev)
        self._pin = [None, None]        # two pinned staging slots (frames, masks[, records]), reused when shapes repeat
        self._busy = [None, None]       # per slot: event recorded after the H2D copies that READ its pinned buffers
        self._slot = 0
        self._next = None
        self._stage()

    def _pinned(self, slot, which, like):
        cur = self._pin[slot]
        buf = None if cur is None else cur[which]
        if buf is None or buf.shape != like.shape or buf.dtype != like.dtype:
            buf = torch.empty(like.shape, dtype=like.dtype, pin_memory=True)
            if cur is None:
                self._pin[slot] = [None, None, None]
            self._pin[slot][which] = buf
        return buf

    def _stage(self):
        try:
            frames, masks = next(self.it)
        except StopIteration:
            self._next = None
            return
        frames, masks = torch.as_tensor(frames), torch.as_tensor(masks)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError("expected uint8 frames of shape [N, H, W, 3]")
        slot = self._slot
        self._slot ^= 1
        if self._busy[slot] is not None:
            self._busy[slot].synchronize()              # the upload that last read this slot must be done before the host overwrites it
        pf = self._pinned(slot, 0, frames); pf.copy_(frames)
        pm = self._pinned(slot, 1, masks); pm.copy_(masks)
        pr = None
        if self.transforms is not None:
            from .transforms import RECORD, CROP_RECORD, CropCompose
            N = frames.shape[0]
            if isinstance(self.transforms, CropCompose):        # the draws need the source size; everything else is the same
                pr = self._pinned(slot, 2, torch.empty(N * CROP_RECORD.itemsize, dtype=torch.uint8))
                self.transforms.pack([self.transforms.draw(frames.shape[1], frames.shape[2]) for _ in range(N)],
                                     out=pr.numpy().view(CROP_RECORD))
            else:
                pr = self._pinned(slot, 2, torch.empty(N * RECORD.itemsize, dtype=torch.uint8))
                self.transforms.pack([self.transforms.draw() for _ in range(N)], out=pr.numpy().view(RECORD))
        with torch.cuda.stream(self.stream):
            gf = pf.to(self.dev, non_blocking=True)
            gm = pm.to(self.dev, non_blocking=True)
            gr = pr.to(self.dev, non_blocking=True) if pr is not None else None
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._busy[slot] = ev
        self._next = (gf, gm, gr, ev)

    def __iter__(self):
        return self

    def __next__(self):
        if self._next is None:
            raise StopIteration
        gf, gm, gr, ev = self._next
        cur = torch.cuda.current_stream(self.dev)
        cur.wait_event(ev)
        gf.record_stream(cur); gm.record_stream(cur)
        self._stage()                                   # upload of the following batch overlaps the consumer's step
        if self.transforms is not None:
            from .transforms import augment_u8, CropCompose
            gr.record_stream(cur)
            t = self.transforms
            if isinstance(t, CropCompose):
                return t.apply(gf, gm, gr)                      # cvk_crop_select + cvk_crop_augment_u8 on the consumer's stream
            return augment_u8(gf, gm, gr, t.out_hw(gf.shape[1], gf.shape[2]), t.mean, t.std)
        return preprocess_uint8(gf, self.mean, self.std), gm
