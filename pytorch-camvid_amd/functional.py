"""Evaluation loops of the hot path on HIP tensors: evaluate, evaluate_report and predict, one pass over a set with the network, a
ConfusionMeter and any further meters.  The losses are in losses.py, the inference drivers in inference.py, the meters in meters.py;
their public names and constants are importable from here as before.

  evaluate, evaluate_report
                    <- the validation pass of train.py:169-206 / eval.py:44-80 without their bugs, plain, under a SlidingWindow or
                       under test-time augmentation: one loop (`_run`) that feeds each meter what it says it takes
  predict           <- predict.py:35-57 from the decoded image onward
"""
import torch

from .losses import (_as_nhwc, _stream, BDL_RECORD_HEAD, DICE_AVERAGES, EDT_MAX_CLASSES, KD_RECORD, LOVASZ_CLASSES,  # noqa: F401
                     LOVASZ_CLASS_SLOTS, LOVASZ_RECORD_HEAD, LOVASZ_SORT_TILE, OHEM_RECORD, REDUCTIONS, SEG_RECORD_HEAD,
                     BoundaryLoss, CrossEntropyLoss, DiceLoss, DistillationLoss, FocalLoss, LovaszSoftmaxLoss, OhemCrossEntropyLoss,
                     SegmentationLoss, boundary_loss, cross_entropy, distillation_loss, distillation_scales, last_ce_status,
                     lovasz_softmax, ohem_cross_entropy, ohem_loss_threshold, segmentation_loss, signed_distance_maps,
                     squared_distance_maps)
from .inference import (CAMVID_MEAN, CAMVID_STD, CRF_MAX_DILATION, CRF_MAX_RADIUS, DevicePrefetcher, LocalCRF, SlidingWindow,  # noqa: F401
                        TestTimeAugmentation, _check_window, argmax_channels, crf_coefficients, crf_refine, crf_tile, preprocess_uint8)
from .meters import (BIOU_ROWS, BOUNDARY_MAX_RADIUS2, CALIB_LOG_COLUMNS, CALIB_MAX_BINS, CALIB_MAX_CELLS, CALIB_MAX_CLASSES,  # noqa: F401
                     CALIB_Q_SCALE, CALIB_TAU_BRACKET, CALIBRATION_REPORT_KEYS, CC_MODES, CC_RECORD_SLOTS, CHEB_MAX_DEPTH,
                     CHEB_MAX_WIDTHS, SURFACE_MAX_DENOMINATOR, SURFACE_RECORD_SLOTS, WEIGHT_METHODS, BoundaryIoUMeter, BoundaryMeter,
                     CalibrationMeter, ClassFrequencyMeter, ConfusionMeter, RegionFilter, RegionMeter, SurfaceDistanceMeter,
                     TemperatureScaler, _check_calib_shapes, boundary_dilation, boundary_iou_scores, boundary_scores, boundary_tolerance,
                     calibration_scores, chessboard_depth, class_weights, confidence_map, connected_components, label_boundaries,
                     region_scores, remove_small_regions, surface_distance_scores, surface_distances, surface_percentile,
                     trimap_scores, weights_from_counts)


def _check_tta_window(who, tta, window):
    _check_window(window)
    if tta is not None and window is not None:
        raise ValueError(f"{who}(): pass tta= or window=, not both; for sliding windows under test-time augmentation pass "
                         "tta=TestTimeAugmentation(..., window=window)")


def _run(who, net, batches, num_classes, ignore_index, window, tta, loss_fn=None, meters=()):
    """The one evaluation loop: eval-mode forward under no_grad over `batches`, the network's `training` flag restored whatever
    happens.  A batch's (logits or None, pred) come from `tta._merge` (which shows `loss_fn` the logits of its loss view, when it has
    one), from `window(net, images)` or from the plain forward; they feed a ConfusionMeter, `loss_fn` and `meters`, each by its
    `update_takes`.  Returns (the ConfusionMeter, the mean of the batch losses: None when none was taken)."""
    confusion, loss_sum, n = None, None, 0

    def add_loss(logits, masks):
        nonlocal loss_sum, n
        l = loss_fn(logits, masks).detach()
        loss_sum = l if loss_sum is None else loss_sum + l
        n += 1

    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            for images, masks in batches:
                if tta is not None:
                    want = tta.loss_view(images.shape[2], images.shape[3]) if loss_fn is not None else None
                    on_logits = None if want is None else lambda i, lg: add_loss(lg, masks) if i == want else None
                    logits, pred = None, tta._merge(net, images, on_logits)[1]
                elif window is not None:
                    logits, pred = window(net, images)
                else:
                    logits = net(images)
                    pred = argmax_channels(logits)
                if confusion is None:
                    confusion = ConfusionMeter(num_classes, ignore_index, pred.device)
                if loss_fn is not None and logits is not None:
                    add_loss(logits, masks)
                confusion.update(pred, masks)
                for m in meters:
                    m.update(logits if m.update_takes == "logits" else pred, masks)
    finally:
        net.train(was_training)
    if confusion is None:
        raise ValueError(f"{who}(): no batches")
    return confusion, float(loss_sum) / n if n else None


def evaluate(net, batches, num_classes=12, ignore_index=11, window=None, tta=None):
    """Validation pass of reference train.py:169-206 / eval.py:44-80 without their bugs: eval-mode forward, device-side
    argmax and histogram accumulation over the WHOLE set, one host copy at the end.
    `batches` yields (images [N,3,H,W] float32, masks [N,H,W] int64) on the GPU.  Returns (accuracy, per-class IoU, mIoU).
    With `tta` (a TestTimeAugmentation) the prediction of a batch is the arg-max of the views' mean probabilities; with `window` (a
    SlidingWindow) it is the arg-max of the windows' merged logits.  One of the two: TestTimeAugmentation(..., window=) combines them."""
    _check_tta_window("evaluate", tta, window)
    return _run("evaluate", net, batches, num_classes, ignore_index, window, tta)[0].compute()


SURFACE_REPORT_KEYS = SurfaceDistanceMeter.report_keys


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
    ValueError (the calibration of merged views is not provided).  What a meter is fed and which of its scores the report takes are
    the meter's own `update_takes` and `report_keys`."""
    _check_tta_window("evaluate_report", tta, window)
    meters = _contour_meters(boundary)
    if tta is not None and any(m.update_takes == "logits" for m in meters):
        raise ValueError("evaluate_report(): a CalibrationMeter with tta= is not provided: the merged views have probabilities but no "
                         "logits to calibrate; pass window= or neither")
    loss_fn = loss_fn or CrossEntropyLoss()
    for m in meters:
        m.reset()
    confusion, loss = _run("evaluate_report", net, batches, num_classes, ignore_index, window, tta, loss_fn, meters)
    acc, iou, miou = confusion.compute()
    prec, rec = confusion.precision_recall()
    report = {"miou": miou, "precision": prec, "recall": rec, "loss": loss, "accuracy": acc, "iou": iou}
    for m in meters:
        scores = m.compute()
        report.update((k, scores[k]) for k in m.report_keys)
    return report


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
