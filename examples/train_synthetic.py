#!/usr/bin/env python3
"""The training loop of the reference (train.py:100-134 + validation :169-206) on synthetic CamVid-shaped data,
driving the MI355X-native network.  Frames are synthesised at the network's input size; for the reference's own
augmentation of 960x720 frames on the device see examples/train_augmented.py.  Everything from the tensors onward is the product path.

  python examples/train_synthetic.py --net unet --epochs 2 --iters 20 -b 8
  python examples/train_synthetic.py --graphed      # each iteration (step, AdamW, log line) as ONE graph replay
  python examples/train_synthetic.py --graphed --clip-grad-norm 1.0     # global-norm clipping inside the captured AdamW step
  python examples/train_synthetic.py --graphed --ema-decay 0.999 --ema-warmup   # weight EMA inside the captured AdamW step, validated too
  python examples/train_synthetic.py --graphed --optimizer sgd -lr 0.05 -wd 1e-4 --clip-grad-norm 1.0   # momentum SGD (cvk.FlatSGD), captured
  python examples/train_synthetic.py --net segnet --teacher unet --teacher-weights unet.pth --kd-temperature 4   # distil the UNet into SegNet
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/train_synthetic.py   # data parallel
"""
import argparse
import os
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pytorch_camvid_amd as cvk  # noqa: E402


def validate(net, batches, tta, window, boundary, surface=None, biou=None, region=None):
    """(accuracy, mIoU, the contour scores of one validation pass: boundary F1, HD95 and ASSD, Boundary IoU and the trimap mIoU,
    fragmentation and the mIoU without small regions, each with its meter; None without a meter)."""
    if boundary is None and surface is None and biou is None and region is None:
        acc, _, miou = cvk.evaluate(net, batches, num_classes=12, ignore_index=11, tta=tta, window=window)
        return acc, miou, None
    rep = cvk.evaluate_report(net, batches, num_classes=12, ignore_index=11, tta=tta, window=window,
                              boundary=[m for m in (boundary, surface, biou, region) if m is not None])
    return rep["accuracy"], rep["miou"], {k: rep[k] for k in ("bf", "hd95", "assd", "biou", "trimap_miou", "fragmentation", "miou_filtered")
                                      if k in rep}


def calibration_text(net, batches, fit):
    """--calibration / --fit-temperature: ECE and NLL of the validation batches (cvk.CalibrationMeter through evaluate_report), and
    with `fit` the temperature fitted on the same batches (cvk.TemperatureScaler) with the ECE after scaling."""
    batches = list(batches)
    before = cvk.evaluate_report(net, batches, num_classes=12, ignore_index=11, boundary=cvk.CalibrationMeter(12, 11, 15))
    out = f"calibration: ECE {before['ece']:.4f}  MCE {before['mce']:.4f}  NLL {before['nll']:.4f}  Brier {before['brier']:.4f}"
    if fit:
        scaler = cvk.TemperatureScaler(iterations=20, ignore_index=11).fit_network(net, batches)
        after = cvk.evaluate_report(net, batches, num_classes=12, ignore_index=11, boundary=cvk.CalibrationMeter(12, 11, 15, temperature=scaler))
        state = "converged" if scaler.converged else "at the bracket's end" if scaler.at_bound else "not converged"
        out += f"\n{'':10s}temperature T {scaler.temperature:.4f} ({state}): ECE {before['ece']:.4f} -> {after['ece']:.4f}  NLL {before['nll']:.4f} -> {after['nll']:.4f}"
    return out


def bf_text(scores, percentile=95):
    if scores is None:
        return ""
    out = f"  BF {scores['bf']:.4f}" if "bf" in scores else ""
    if "hd95" in scores:
        out += f"  HD{percentile:g} {scores['hd95']:.2f} px  ASSD {scores['assd']:.2f} px"
    if "biou" in scores:
        out += f"  BIoU {scores['biou']:.4f}"
    if "trimap_miou" in scores:
        out += "  trimap mIoU " + " ".join(f"{v:.4f}" for v in scores["trimap_miou"])
    if "miou_filtered" in scores:
        out += f"  mIoU without small regions {scores['miou_filtered']:.4f}  fragmentation {scores['fragmentation']:.2f}"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-net", "--net", default="unet")
    ap.add_argument("-b", type=int, default=8)                 # reference default 10 (train.py:22)
    ap.add_argument("-lr", type=float, default=5e-4)           # train.py:23
    ap.add_argument("--epochs", type=int, default=2)           # reference 120 (train.py:24)
    ap.add_argument("--iters", type=int, default=20, help="synthetic batches per epoch")
    ap.add_argument("-wd", type=float, default=0.0)            # train.py:25
    ap.add_argument("--flat-adamw", action="store_true", help="one fused optimizer kernel (cvk.FlatAdamW; with --optimizer sgd: cvk.FlatSGD)")
    ap.add_argument("--optimizer", default="adamw", choices=["adamw", "sgd"],
                    help="adamw: the reference's optimizer; sgd: momentum SGD as the U-Net and SegNet papers trained (cvk.FlatSGD with "
                    "--flat-adamw / --graphed, torch.optim.SGD otherwise); -lr is the schedule's peak, -wd the coupled L2 weight decay")
    ap.add_argument("--momentum", type=float, default=0.9, help="--optimizer sgd: the momentum (OneCycleLR cycles it between 0.85 and this)")
    ap.add_argument("--nesterov", action="store_true", help="--optimizer sgd: Nesterov momentum")
    ap.add_argument("--graphed", action="store_true", help="the whole iteration (forward, loss, backward, FlatAdamW, the log line) as one "
                    "captured graph (cvk.GraphedStep); the log is read once per epoch.  Implies --flat-adamw")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--class-weights", default="none", choices=["none", "median_frequency", "enet"],
                    help="class-weighted loss, weights from the training masks (cvk.class_weights)")
    ap.add_argument("--label-smoothing", type=float, default=0.0)
    ap.add_argument("--loss", default="ce", choices=["ce", "focal", "dice", "ce+dice", "ohem", "lovasz", "ce+lovasz", "boundary", "ce+boundary"],
                    help="ce: cvk.CrossEntropyLoss (the reference's loss); focal, dice, ce+dice: cvk.SegmentationLoss, one fused pass; "
                         "ohem: cvk.OhemCrossEntropyLoss, online hard example mining; lovasz, ce+lovasz: cvk.LovaszSoftmaxLoss, the "
                         "Jaccard surrogate alone or added to the (weighted) cross-entropy; boundary, ce+boundary: cvk.BoundaryLoss, Kervadec's "
                         "boundary loss on distance maps computed on the device, alone or added to the (weighted) cross-entropy")
    ap.add_argument("--focal-gamma", type=float, default=2.0, help="--loss focal: the focusing exponent")
    ap.add_argument("--dice-weight", type=float, default=0.5, help="--loss ce+dice: the Dice term's coefficient")
    ap.add_argument("--ohem-thresh", type=float, default=0.7, help="--loss ohem: keep the pixels whose target probability is below this")
    ap.add_argument("--ohem-min-kept", type=int, default=100000, help="--loss ohem: never keep fewer than this many of the hardest pixels")
    ap.add_argument("--lovasz-weight", type=float, default=1.0, help="--loss lovasz, ce+lovasz: the Lovász term's coefficient")
    ap.add_argument("--lovasz-per-image", action="store_true", help="--loss lovasz, ce+lovasz: one Lovász loss per image, averaged")
    ap.add_argument("--lovasz-classes", default="present", choices=["present", "all"],
                    help="--loss lovasz, ce+lovasz: average over the classes that occur in a segment, or over all of them")
    ap.add_argument("--boundary-weight", type=float, default=1.0,
                    help="--loss boundary, ce+boundary: the boundary term's coefficient (with --boundary-ramp: in the first epoch)")
    ap.add_argument("--boundary-ramp", type=float, default=0.0, metavar="X",
                    help="--loss boundary, ce+boundary: add X to the coefficient every epoch, up to 1 (Kervadec's schedule); the coefficient "
                         "lives in a device buffer, so a --graphed step follows it without a re-capture")
    ap.add_argument("--teacher", default=None, choices=["unet", "segnet"],
                    help="knowledge distillation: train --net under this network's logits with cvk.DistillationLoss (cross-entropy on the "
                         "labels + --kd-weight * temperature-softened KL towards the teacher); the teacher runs in eval mode under no_grad")
    ap.add_argument("--teacher-weights", default=None, metavar="FILE",
                    help="with --teacher: its state_dict; without it the teacher is freshly initialised, good for a smoke run only")
    ap.add_argument("--kd-weight", type=float, default=1.0, help="with --teacher: the KL term's coefficient")
    ap.add_argument("--kd-temperature", type=float, default=4.0, help="with --teacher: the temperature T (the KL term carries T^2)")
    ap.add_argument("--kd-ignored", action="store_true", help="with --teacher: distil on the pixels the labels ignore too")
    ap.add_argument("--split-operands", type=int, default=0, choices=[0, 2, 3],
                    help="opt-in for fp32: matrix products on the 16-bit matrix pipe with split fp32 operands (cvk.set_split_operands; 2 = fp16 x 2)")
    ap.add_argument("--clip-grad-norm", type=float, default=None, metavar="X",
                    help="clip the global gradient 2-norm to X: fused into the step with --flat-adamw / --graphed (FlatAdamW(max_grad_norm=X)), "
                    "cvk.clip_grad_norm_ before torch's AdamW otherwise; prints the epoch's largest norm and the share of clipped steps")
    ap.add_argument("--accumulate", type=int, default=1, metavar="K",
                    help="gradient accumulation: one optimizer update per K batches on their mean gradient (cvk.GradAccumulator; with --graphed "
                    "the whole window of K batches is one captured graph).  --iters must be a multiple of K")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="X",
                    help="keep an exponential moving average of the weights inside the fused step (FlatAdamW(ema_decay=X); needs --flat-adamw or "
                    "--graphed); every epoch validates the live and, inside opt.swap_ema(), the averaged weights")
    ap.add_argument("--ema-warmup", action="store_true", help="with --ema-decay: decay min(X, (1 + k) / (10 + k)) at the k-th update")
    ap.add_argument("--tta-scales", default=None, metavar="S,S,...",
                    help="validate with multi-scale test-time augmentation at these scales, e.g. 0.75,1.0,1.25 (cvk.TestTimeAugmentation)")
    ap.add_argument("--tta-flip", action="store_true", help="also validate on the mirrored views (alone: scale 1.0 and its mirror image)")
    ap.add_argument("--window-crop", default=None, metavar="H,W",
                    help="validate by sliding-window inference with crops of this size, e.g. 360,480 (cvk.SlidingWindow); with --tta-scales / "
                    "--tta-flip every view is evaluated in windows")
    ap.add_argument("--window-stride", default=None, metavar="H,W", help="with --window-crop: the step between windows (default: two thirds of the crop)")
    ap.add_argument("--boundary-f1", action="store_true", help="also report the boundary F1 measure (BF score) of the validation pass (cvk.BoundaryMeter)")
    ap.add_argument("--bf-tolerance", type=float, default=0.0075, metavar="X",
                    help="with --boundary-f1: the matching distance as a fraction of the image diagonal (default 0.75 %%)")
    ap.add_argument("--surface-distance", action="store_true",
                    help="also report HD95 and the average symmetric surface distance of the validation pass, in pixels (cvk.SurfaceDistanceMeter)")
    ap.add_argument("--hd-percentile", type=float, default=95.0, metavar="Q",
                    help="with --surface-distance: the percentile of the Hausdorff distance, 0..100 (default 95; 100 is the Hausdorff distance)")
    ap.add_argument("--boundary-iou", action="store_true",
                    help="also report Boundary IoU (Cheng et al., CVPR 2021) of the validation pass (cvk.BoundaryIoUMeter)")
    ap.add_argument("--biou-ratio", type=float, default=0.02, metavar="X",
                    help="with --boundary-iou: the dilation as a fraction of the image diagonal (default 2 %%)")
    ap.add_argument("--trimap-widths", default=None, metavar="W,W,...",
                    help="also report the mIoU inside bands of these widths around the label boundaries, e.g. 1,2,4,8,16 (up to 8 increasing "
                    "widths in 1..254; cvk.BoundaryIoUMeter)")
    ap.add_argument("--min-region", type=int, default=None, metavar="A",
                    help="also report the mIoU after regions of fewer than A pixels went to their neighbours' class, and the fragmentation "
                    "(predicted regions over label regions; cvk.RegionMeter)")
    ap.add_argument("--region-connectivity", type=int, default=4, choices=(4, 8), help="with --min-region: 4- or 8-connected regions")
    ap.add_argument("--calibration", action="store_true",
                    help="also report the expected calibration error, NLL and Brier score of the validation pass (cvk.CalibrationMeter)")
    ap.add_argument("--fit-temperature", action="store_true",
                    help="fit a temperature T on the validation batches (cvk.TemperatureScaler) and report T and the ECE before and after")
    ap.add_argument("--crf", action="store_true",
                    help="also validate with a local-window mean-field CRF on top of the predictions (cvk.LocalCRF; the guide image is the "
                    "network's own input) and print the mIoU with and without it; with --tta-* / --window-crop it refines their result")
    ap.add_argument("--crf-iterations", type=int, default=5, help="with --crf: mean-field iterations")
    ap.add_argument("--crf-radius", type=int, default=3, help="with --crf: the window is (2 radius + 1)^2 pixels, radius in 1..5")
    ap.add_argument("--crf-dilation", type=int, default=1, help="with --crf: the step between the window's pixels, 1..4")
    a = ap.parse_args()
    tta = window = boundary = surface = biou = region = None
    if a.min_region is not None:
        try:
            region = cvk.RegionMeter(num_classes=12, ignore_index=11, min_area=a.min_region, connectivity=a.region_connectivity)
        except ValueError as e:
            ap.error(f"--min-region: {e}")
    if a.boundary_iou or a.trimap_widths:
        try:
            widths = tuple(int(v) for v in a.trimap_widths.split(",")) if a.trimap_widths else ()
            biou = cvk.BoundaryIoUMeter(num_classes=12, ignore_index=11, ratio=a.biou_ratio, trimap_widths=widths)
        except ValueError as e:
            ap.error(f"--biou-ratio / --trimap-widths: {e}")
    if a.surface_distance:
        try:
            surface = cvk.SurfaceDistanceMeter(num_classes=12, ignore_index=11, percentile=a.hd_percentile)
        except ValueError as e:
            ap.error(f"--hd-percentile: {e}")
    if a.boundary_f1:
        try:
            boundary = cvk.BoundaryMeter(num_classes=12, ignore_index=11, tolerance=a.bf_tolerance)
        except ValueError as e:
            ap.error(f"--bf-tolerance: {e}")
    if a.window_stride and not a.window_crop:
        ap.error("--window-stride needs --window-crop")
    if a.window_crop:
        try:
            crop = tuple(int(v) for v in a.window_crop.split(","))
            stride = tuple(int(v) for v in a.window_stride.split(",")) if a.window_stride else tuple(max(1, 2 * c // 3) for c in crop)
            window = cvk.SlidingWindow(crop=crop, stride=stride)
        except ValueError as e:
            ap.error(f"--window-crop / --window-stride: {e}")
    if a.tta_scales or a.tta_flip:
        try:
            tta = cvk.TestTimeAugmentation(scales=[float(v) for v in (a.tta_scales or "1.0").split(",")], flip=a.tta_flip, window=window)
        except ValueError as e:
            ap.error(f"--tta-scales: {e}")
        window = None                   # the views are evaluated in windows: evaluate() takes tta= or window=, not both
    crf = None
    if a.crf:
        try:
            crf = cvk.LocalCRF(iterations=a.crf_iterations, radius=a.crf_radius, dilation=a.crf_dilation,
                               inner=tta if tta is not None else window)
        except ValueError as e:
            ap.error(f"--crf-iterations / --crf-radius / --crf-dilation: {e}")
    a.flat_adamw = a.flat_adamw or a.graphed
    if (a.ema_decay is not None or a.ema_warmup) and not a.flat_adamw:
        ap.error("--ema-decay / --ema-warmup need --flat-adamw or --graphed (the average lives in FlatAdamW's flat buffers)")
    if a.ema_warmup and a.ema_decay is None:
        ap.error("--ema-warmup needs --ema-decay")
    K = a.accumulate
    if K < 1 or a.iters % K:
        ap.error("--accumulate K needs K >= 1 and --iters a multiple of K")
    updates = a.iters // K
    if a.teacher is None and (a.teacher_weights or a.kd_ignored):
        ap.error("--teacher-weights / --kd-ignored need --teacher")
    if a.teacher is not None and (a.loss != "ce" or a.label_smoothing):
        ap.error("--teacher distils next to the plain cross-entropy: --loss ce without --label-smoothing")
    if a.teacher is not None and a.graphed and K > 1:
        ap.error("--teacher with --graphed and --accumulate is not provided: the bound teacher-logits buffer holds one batch, not a window; "
                 "drop --graphed (the eager accumulation loop passes each micro-batch's teacher logits)")

    world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        cvk.ddp.init_process_group("nccl", device_id=dev)      # RCCL with the channel count / CU reservation this path is tuned for

    torch.manual_seed(0)
    net = cvk.get_model(a.net, 3, 12).to(dev)                              # utils.get_model (utils.py:147-160)
    cvk.set_conv_precision(net, a.precision)
    cvk.set_split_operands(net, a.split_operands)
    model = cvk.ddp.DataParallel(net) if world > 1 else net
    fused = dict(max_grad_norm=a.clip_grad_norm, ema_decay=a.ema_decay, ema_warmup=a.ema_warmup)
    if a.optimizer == "sgd":
        sgd = dict(lr=a.lr, momentum=a.momentum, weight_decay=a.wd, nesterov=a.nesterov)
        opt = cvk.FlatSGD(net, **sgd, **fused) if a.flat_adamw else torch.optim.SGD(net.parameters(), **sgd)
    else:
        opt = cvk.FlatAdamW(net, lr=a.lr, weight_decay=a.wd, **fused) if a.flat_adamw else \
            torch.optim.AdamW(net.parameters(), lr=a.lr, weight_decay=a.wd)     # train.py:100
    cycle = dict(max_momentum=a.momentum, base_momentum=min(0.85, a.momentum)) if a.optimizer == "sgd" and a.momentum > 0 else \
        dict(cycle_momentum=a.optimizer != "sgd")
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=a.lr, steps_per_epoch=updates, epochs=a.epochs, **cycle)  # :103-104
    if K > 1 and a.graphed and world > 1:
        ap.error("--accumulate with --graphed runs on one GPU (a window with captured collectives is not supported)")
    accum = cvk.GradAccumulator(model, steps=K) if K > 1 else None           # folds the flat gradient buffers of K backward passes
    g = torch.Generator().manual_seed(1234 + rank)
    # a fixed synthetic "dataset": uint8 HWC frames like cv2 delivers + 12-class masks; smooth blobs so it is learnable
    base = torch.rand(a.iters, a.b, 45, 60, generator=g)
    masks = torch.nn.functional.interpolate((base * 12).floor().clamp(0, 11), size=(360, 480), mode="nearest").long()
    weight = None if a.class_weights == "none" else cvk.class_weights(masks, 12, method=a.class_weights, device=dev)
    if a.loss == "ce":
        loss_fn = cvk.CrossEntropyLoss(weight=weight, label_smoothing=a.label_smoothing)   # train.py:105
    else:
        if a.label_smoothing:
            raise SystemExit("--label-smoothing belongs to --loss ce")
        if a.loss == "ohem":
            loss_fn = cvk.OhemCrossEntropyLoss(a.ohem_thresh, a.ohem_min_kept, weight=weight)
        elif a.loss in ("lovasz", "ce+lovasz"):
            if a.loss == "lovasz" and weight is not None:
                raise SystemExit("--class-weights enter the cross-entropy term: use --loss ce+lovasz")
            loss_fn = cvk.LovaszSoftmaxLoss(a.lovasz_weight, 1.0 if a.loss == "ce+lovasz" else 0.0, classes=a.lovasz_classes,
                                            per_image=a.lovasz_per_image, weight=weight)
        elif a.loss in ("boundary", "ce+boundary"):
            if a.loss == "boundary" and weight is not None:
                raise SystemExit("--class-weights enter the cross-entropy term: use --loss ce+boundary")
            if a.boundary_weight < 0 or a.boundary_ramp < 0 or a.boundary_weight + a.boundary_ramp <= 0:
                raise SystemExit("--boundary-weight and --boundary-ramp must not be negative, and one of them must be positive")
            # which terms exist is fixed here; the coefficient itself is set at the start of every epoch
            loss_fn = cvk.BoundaryLoss(1.0, 1.0 if a.loss == "ce+boundary" else 0.0, weight=weight).to(dev)
        else:
            ce, dice = {"focal": (1.0, 0.0), "dice": (0.0, 1.0), "ce+dice": (1.0, a.dice_weight)}[a.loss]
            loss_fn = cvk.SegmentationLoss(ce, dice, focal_gamma=a.focal_gamma if a.loss == "focal" else 0.0, weight=weight)
    teacher = kd = kd_buf = None
    if a.teacher is not None:
        teacher = cvk.get_model(a.teacher, 3, 12).to(dev)
        if a.teacher_weights:
            teacher.load_state_dict(torch.load(a.teacher_weights, map_location=dev))
        elif rank == 0:
            print("--teacher without --teacher-weights: the teacher is freshly initialised; that is good for a smoke run only")
        teacher.eval().requires_grad_(False)
        kd = cvk.DistillationLoss(1.0, a.kd_weight, a.kd_temperature, weight=weight, distill_ignored=a.kd_ignored)
    step = None
    for epoch in range(1, a.epochs + 1):
        net.train()
        if isinstance(loss_fn, cvk.BoundaryLoss):                           # a fill of the device buffer on this stream, no sync
            loss_fn.boundary = min(1.0, a.boundary_weight + a.boundary_ramp * (epoch - 1)) if a.boundary_ramp else a.boundary_weight
        t0 = time.time()
        norms = []                                                          # device scalars: read once per epoch
        pending = []                                                        # --graphed --accumulate: the open window's batches
        for it in range(a.iters):
            m = masks[it].to(dev)
            frames = ((m.unsqueeze(-1) * torch.tensor([20, 15, 10], device=dev)) % 256 +
                      torch.randint(0, 30, (a.b, 360, 480, 3), device=dev)).clamp(0, 255).to(torch.uint8)
            images = cvk.preprocess_uint8(frames)                           # transforms.ToTensor + Normalize on device
            z = None
            if teacher is not None:
                with torch.no_grad():
                    z = teacher(images)                                     # the teacher's logits: a constant of this step
            if a.graphed:
                if accum is not None:                                       # a window of K batches: [K, N, 3, H, W], [K, N, H, W]
                    pending.append((images, m))
                    if len(pending) < K:
                        continue
                    images, m = torch.stack([w[0] for w in pending]), torch.stack([w[1] for w in pending])
                    pending = []
                if step is None:                                            # capture once, on the first batch of the geometry
                    if kd is not None:                                      # the captured kernels read the teacher's logits from kd_buf
                        kd_buf = z.clone()
                        loss_fn = kd.bind(kd_buf)
                    step = cvk.GraphedStep(net, loss_fn, images, m, allow_grad_sync=world > 1, optimizer=opt, scheduler=sched,
                                           log_capacity=updates, accumulator=accum)
                if kd is not None:
                    kd_buf.copy_(z)
                loss = step.replay(images, m)                               # train.py:124-134 + the log line, one launch
                continue
            if accum is None or accum.micro_step == 0:
                opt.zero_grad()                                             # train.py:124
            preds = model(images)                                           # :128
            loss = loss_fn(preds, m) if kd is None else kd(preds, m, z)     # :130
            loss.backward()                                                 # :131
            if accum is not None and not accum.ready:                       # the window is still open: .grad is None, nothing to step
                continue
            if a.clip_grad_norm is not None and not a.flat_adamw:
                norms.append(cvk.clip_grad_norm_(net, a.clip_grad_norm))    # reduction, finish, in-place scale: no host sync
            opt.step(); sched.step()                                        # :133-134
            if a.clip_grad_norm is not None and a.flat_adamw:
                norms.append(opt.grad_norm.clone())                         # the fused step's record
        torch.cuda.synchronize()
        dt = time.time() - t0
        if step is not None and rank == 0:
            rows, dropped = step.log()                                      # the epoch's per-iteration lines: one D2H copy
            if a.clip_grad_norm is not None:                                # 7 columns: ..., global norm, clip coefficient
                norms = list(torch.from_numpy(rows[:, 5].copy()))
            col2 = "Momentum" if a.optimizer == "sgd" else "Beta1"          # column 2 of the log: what the scheduler cycles
            for i, (l, lr, beta, gw, gb) in enumerate(rows[:, :5]):         # train.py:135-143 + utils.visulaize_lastlayer
                print(("Training Epoch:{epoch} [{trained_samples}/{total_samples}] Lr:{lr:0.6f} Loss:{loss:0.4f} " + col2 + ":{beta:0.4f} "
                       "grad_norm2_weights:{gw:0.4e} grad_norm2_bias:{gb:0.4e}").format(
                    epoch=epoch, trained_samples=(dropped + i + 1) * a.b * K, total_samples=a.iters * a.b, lr=lr, loss=l, beta=beta,
                    gw=gw, gb=gb))
        if rank == 0:
            print(f"epoch {epoch}: loss {loss.item():.4f}  lr {sched.get_last_lr()[0]:.6f}  "
                  f"{world * a.b * a.iters / dt:.1f} img/s (incl. data synthesis + optimizer)")
            if kd is not None:                                          # device views of the last step's record
                kd_h, kd_k = kd.last_terms.tolist()
                print(f"          distillation: H {kd_h:.4f}  K {kd_k:.4f}  arg-max agreement with the teacher {kd.last_agreement.item():.4f}  "
                      f"(T {a.kd_temperature:g}, kd weight {a.kd_weight:g})")
            if isinstance(loss_fn, cvk.BoundaryLoss):                   # device views of the last step's record
                bl_b, bl_h = loss_fn.last_terms.tolist()
                print(f"          boundary loss: B {bl_b:.4f}  H {bl_h:.4f}  (coefficient {loss_fn.boundary:g})")
            if norms:
                n = torch.stack([v.detach().float().cpu() for v in norms])
                print(f"          grad norm max {n.max().item():.4e}  clipped {(n > a.clip_grad_norm).float().mean().item() * 100:.0f} % of "
                      f"{n.numel()} steps (max_norm {a.clip_grad_norm:g})")
        # validation (train.py:169-206) on two of the batches
        batches = []
        for it in range(2):
            m = masks[it].to(dev)
            frames = ((m.unsqueeze(-1) * torch.tensor([20, 15, 10], device=dev)) % 256).clamp(0, 255).to(torch.uint8)
            batches.append((cvk.preprocess_uint8(frames), m))
        acc, miou, bf = validate(net, batches, tta, window, boundary, surface, biou, region)
        miou_crf = cvk.evaluate(net, batches, num_classes=12, ignore_index=11, tta=crf)[2] if crf is not None else None
        if rank == 0:
            print(f"          val acc {acc:.4f}  mIoU(11 classes) {miou:.4f}{bf_text(bf, a.hd_percentile)}")
            if crf is not None:
                print(f"          with the CRF refinement mIoU {miou_crf:.4f}, without {miou:.4f}  ({crf.iterations} iterations, radius "
                      f"{crf.radius}, dilation {crf.dilation})")
        if a.calibration or a.fit_temperature:
            text = calibration_text(net, batches, a.fit_temperature)
            if rank == 0:
                print(f"          {text}")
        if a.ema_decay is not None:
            with opt.swap_ema():                                            # the averaged weights (BatchNorm statistics stay the live ones)
                acc_e, miou_e, bf_e = validate(net, batches, tta, window, boundary, surface, biou, region)
                miou_crf_e = cvk.evaluate(net, batches, num_classes=12, ignore_index=11, tta=crf)[2] if crf is not None else None
            if rank == 0:
                print(f"          EMA acc {acc_e:.4f}  mIoU(11 classes) {miou_e:.4f}{bf_text(bf_e, a.hd_percentile)}  ({opt.ema_updates} updates, decay {a.ema_decay:g})")
                if crf is not None:
                    print(f"          EMA with the CRF refinement mIoU {miou_crf_e:.4f}, without {miou_e:.4f}")
    if rank == 0:
        torch.save(net.state_dict(), "/tmp/cvk_synthetic.pth")             # train.py:232-240; loads into the reference too
        if a.ema_decay is not None:
            torch.save(opt.ema_state_dict(), "/tmp/cvk_synthetic_ema.pth")  # the averaged weights, same keys and layout
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
