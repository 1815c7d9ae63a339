"""The losses of the hot path as autograd nodes on HIP tensors (the meters are in meters.py, the inference drivers in inference.py).

  CrossEntropyLoss, cross_entropy
                    <- nn.CrossEntropyLoss() of reference train.py:105 (mean over N*H*W, no ignored class); also torch's
                       weight / reduction / label_smoothing options
  SegmentationLoss, FocalLoss, DiceLoss, segmentation_loss
                    <- ce * focal + dice * soft Dice, one fused pass over the logits each way (not in the reference)
  OhemCrossEntropyLoss, ohem_cross_entropy
                    <- cross-entropy over the hard pixels, chosen by an on-device k-th-largest select (not in the reference)
  LovaszSoftmaxLoss, lovasz_softmax
                    <- the Lovász-softmax surrogate of the Jaccard index over an on-device segmented radix sort (not in the reference)
  BoundaryLoss, boundary_loss, squared_distance_maps, signed_distance_maps
                    <- Kervadec's boundary loss over an exact on-device Euclidean distance transform (not in the reference)
  DistillationLoss, distillation_loss
                    <- ce * cross-entropy + kd * temperature KL to a teacher's logits (not in the reference)

Every node goes through one front end: `_check_inputs` (the input rules), `_launch` (one profiled call of a cvk_* entry point),
`_ptr`, `_grad_buffers` (what every backward allocates) and, for the modules, `_LastRecord`.
"""
import torch
import torch.nn as nn

from . import _lib, engine
from ._lib import check


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def _as_nhwc(logits):
    """[N,C,H,W] logical -> (tensor whose memory is dense NHWC rows, ld).  Zero-copy for channels_last producers
    (our networks return channels_last strides), one copy otherwise."""
    if logits.dim() != 4:
        raise ValueError("expected logits of shape [N, C, H, W]")
    p = logits.permute(0, 2, 3, 1)
    if p.is_contiguous():
        return p, logits.shape[1]
    st = p.stride()
    N, H, W, C = p.shape
    if st[3] == 1 and st[2] >= C and st[1] == st[2] * W and st[0] == st[1] * H:
        return p, st[2]                                   # padded pixel stride (ld > C)
    return p.contiguous(), C


def _check_weight_option(weight):
    if weight is not None and (not isinstance(weight, torch.Tensor) or weight.dim() != 1):
        raise ValueError("weight must be a 1-D tensor of one value per class")


def _check_inputs(who, logits, target, weight, target_optional=False):
    """The input rules of every loss node (`who`: the module's name), before anything is launched: HIP tensors, [N, C, H, W] float32
    logits, an int64 [N, H, W] target, a float32 weight of one value per class on the logits' device.  With `target_optional` the
    target may be None.  Returns the logits' NHWC view and its pixel stride (`_as_nhwc`), the contiguous target (or None), the
    detached contiguous weight (or None) and (N, C, H, W)."""
    if not logits.is_cuda:
        raise RuntimeError(f"pytorch_camvid_amd.{who} needs HIP tensors (no CPU fallback)")
    if logits.dim() != 4:
        raise ValueError("expected logits of shape [N, C, H, W]")
    if target_optional and logits.dtype != torch.float32:      # a loss that can do without a target names the logits alone
        raise RuntimeError(f"expected float32 logits, got {logits.dtype}")
    labelled = not (target_optional and target is None)
    if labelled and (logits.dtype != torch.float32 or target.dtype != torch.int64):
        raise RuntimeError(f"expected float32 logits and int64 target, got {logits.dtype} / {target.dtype}")
    N, C, H, W = logits.shape
    if labelled and tuple(target.shape) != (N, H, W):
        raise ValueError(f"Expected target size {[N, H, W]}, got {list(target.shape)}")
    if weight is not None:
        if weight.dim() != 1 or weight.numel() != C:
            raise RuntimeError(f"weight tensor should be defined either for all {C} classes or no classes but got weight tensor "
                               f"of shape: {list(weight.shape)}")
        if weight.device != logits.device:
            raise RuntimeError(f"weight is on {weight.device} but the logits are on {logits.device} (no implicit copy: the loss "
                               "stays capturable); move the loss module with .to(device)")
        if weight.dtype != torch.float32:
            raise RuntimeError(f"expected a float32 weight, got {weight.dtype}")
        weight = weight.detach().contiguous()
    lg, ld = _as_nhwc(logits)
    return lg, ld, target.contiguous() if labelled else None, weight, (N, C, H, W)


def _launch(kname, nbytes, fn, *args):
    """One call of the entry point `fn` (a `lib.cvk_*`), its status checked, as the kernel `kname` of `nbytes` algorithmic HBM bytes in
    the profile list (`engine.PROF`, read at the call)."""
    return engine._timed(None, kname, nbytes, lambda: check(fn(*args), fn.__name__), "byte")


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _grad_buffers(lg, gout, N, C, H, W):
    """What every backward starts from: the float32 [N, H, W, C] gradient (returned to autograd as its [N, C, H, W] view) and the
    contiguous incoming gradient."""
    return torch.empty((N, H, W, C), device=lg.device, dtype=torch.float32), gout.contiguous()


class _LastRecord:
    """Mixin of the loss modules that keep the device record of their most recent forward in `self._record`."""

    _record = None

    def _rec(self):
        if self._record is None:
            raise RuntimeError("no forward has run yet")
        return self._record

    @property
    def last_record(self):
        """The device record of the most recent forward (float32, no sync; its layout is in the module's docstring)."""
        return self._rec()


class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, grad_scale, ignore_index=-100):
        lib = _lib.load()
        lg, ld, tg, _, (N, C, H, W) = _check_inputs("CrossEntropyLoss", logits, target, None)
        M = N * H * W
        part = torch.empty(3 * lib.cvk_ce_blocks(M), device=logits.device, dtype=torch.float32)
        loss3 = torch.empty(3, device=logits.device, dtype=torch.float32)     # mean loss | valid pixels | out-of-range targets
        _launch("k_ce_fwd", 4.0 * M * ld + 8.0 * M, lib.cvk_softmax_ce_fwd,
                lg.data_ptr(), ld, tg.data_ptr(), part.data_ptr(), loss3.data_ptr(), M, C, int(ignore_index), _stream(logits))
        ctx.save_for_backward(lg, tg, loss3)
        ctx.meta = (N, C, H, W, ld, grad_scale, int(ignore_index))
        _CrossEntropy.last_status = loss3
        return loss3[0].clone()     # not a view: loss3 is saved for backward (its divisor) and published as the status

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        lg, tg, loss3 = ctx.saved_tensors
        N, C, H, W, ld, grad_scale, ignore_index = ctx.meta
        M = N * H * W
        d, g = _grad_buffers(lg, gout, N, C, H, W)
        _launch("k_ce_bwd", 4.0 * M * ld + 8.0 * M + 4.0 * M * C, lib.cvk_softmax_ce_bwd,
                lg.data_ptr(), ld, tg.data_ptr(), loss3.data_ptr(), g.data_ptr(), float(grad_scale), d.data_ptr(), C, M, C, ignore_index,
                _stream(lg))
        return d.permute(0, 3, 1, 2), None, None, None


REDUCTIONS = {k: _lib.DEFINES["CVK_REDUCTION_" + k.upper()] for k in ("none", "mean", "sum")}


class _CrossEntropyEx(torch.autograd.Function):
    """Class weights / label smoothing / reduction 'none' | 'sum' (cvk_softmax_ce_fwd_ex / _bwd_ex)."""

    @staticmethod
    def forward(ctx, logits, target, weight, grad_scale, ignore_index, reduction, label_smoothing):
        lib = _lib.load()
        lg, ld, tg, weight, (N, C, H, W) = _check_inputs("CrossEntropyLoss", logits, target, weight)
        red = REDUCTIONS[reduction]
        M = N * H * W
        part = torch.empty(lib.cvk_ce_ex_part_floats(M), device=logits.device, dtype=torch.float32)
        loss4 = torch.empty(4, device=logits.device, dtype=torch.float32)   # loss | valid pixels | out-of-range targets | divisor
        px = torch.empty((N, H, W), device=logits.device, dtype=torch.float32) if red == 0 else None
        _launch("k_ce_fwd_ex", 4.0 * M * ld + 8.0 * M, lib.cvk_softmax_ce_fwd_ex,
                lg.data_ptr(), ld, tg.data_ptr(), _ptr(weight), float(label_smoothing), red, part.data_ptr(), loss4.data_ptr(), _ptr(px),
                M, C, int(ignore_index), _stream(logits))
        ctx.save_for_backward(lg, tg, loss4, weight)
        ctx.meta = (N, C, H, W, ld, grad_scale, int(ignore_index), red, float(label_smoothing))
        _CrossEntropy.last_status = loss4
        return px if px is not None else loss4[0].clone()

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        lg, tg, loss4, weight = ctx.saved_tensors
        N, C, H, W, ld, grad_scale, ignore_index, red, eps = ctx.meta
        M = N * H * W
        d, g = _grad_buffers(lg, gout, N, C, H, W)
        _launch("k_ce_bwd_ex", 4.0 * M * ld + 8.0 * M + 4.0 * M * C, lib.cvk_softmax_ce_bwd_ex,
                lg.data_ptr(), ld, tg.data_ptr(), _ptr(weight), eps, red, loss4.data_ptr(), g.data_ptr(), float(grad_scale), d.data_ptr(),
                C, M, C, ignore_index, _stream(lg))
        return d.permute(0, 3, 1, 2), None, None, None, None, None, None


def _check_ce_options(weight, reduction, label_smoothing):
    if reduction not in REDUCTIONS:
        raise ValueError(f"{reduction} is not a valid value for reduction")
    if not 0.0 <= float(label_smoothing) <= 1.0:
        raise ValueError(f"label_smoothing must be between 0.0 and 1.0. Got: {label_smoothing}")
    _check_weight_option(weight)


def _ce(logits, target, weight, grad_scale, ignore_index, reduction, label_smoothing):
    if weight is None and reduction == "mean" and float(label_smoothing) == 0.0:
        return _CrossEntropy.apply(logits, target, grad_scale, ignore_index)       # the default loss: k_ce_fwd -> k_ce_finish -> k_ce_bwd
    return _CrossEntropyEx.apply(logits, target, weight, grad_scale, ignore_index, reduction, float(label_smoothing))


class CrossEntropyLoss(nn.Module):
    """Drop-in for the reference's `nn.CrossEntropyLoss()` (train.py:105); targets are int64 class indices in [0, C) or
    `ignore_index` (default -100 as in torch: such pixels are left out of the loss and get no gradient).  Any other
    out-of-range target makes the loss NaN — torch raises a device-side assert there; raising here would need a host sync
    in every step — and `last_ce_status()` reports the count.  `grad_scale` multiplies the backward only (data-parallel
    training can fold 1/world_size in here).
    Keyword options as in torch: `weight` (float32 [C] on the logits' device; a registered buffer, so it follows .to() and
    is in state_dict), `reduction` ('mean' divides by the sum of the targets' weights, 'sum', or 'none' for an [N, H, W]
    loss map) and `label_smoothing` in [0, 1].  With all three at their defaults the loss runs the unweighted kernels."""

    def __init__(self, grad_scale=1.0, ignore_index=-100, *, weight=None, reduction="mean", label_smoothing=0.0):
        super().__init__()
        _check_ce_options(weight, reduction, label_smoothing)
        self.grad_scale = grad_scale
        self.ignore_index = ignore_index
        self.reduction = reduction
        self.label_smoothing = float(label_smoothing)
        self.register_buffer("weight", weight)

    def forward(self, logits, target):
        return _ce(logits, target, self.weight, self.grad_scale, self.ignore_index, self.reduction, self.label_smoothing)


def cross_entropy(logits, target, weight=None, ignore_index=-100, reduction="mean", label_smoothing=0.0):
    """torch.nn.functional.cross_entropy's options on the HIP kernels.  An int in the third position is read as
    `ignore_index`, what that position meant before `weight` existed."""
    if isinstance(weight, int) and not isinstance(weight, bool):
        weight, ignore_index = None, weight
    _check_ce_options(weight, reduction, label_smoothing)
    return _ce(logits, target, weight, 1.0, ignore_index, reduction, label_smoothing)


DICE_AVERAGES = {k: _lib.DEFINES["CVK_DICE_" + k.upper()] for k in ("present", "all")}
SEG_RECORD_HEAD = 7                                # loss | valid | out of range | sum w[t] | F | D | K, then dice_c, a_c, b_c


class _SegLoss(torch.autograd.Function):
    """ce * focal + dice * soft Dice in one forward and one backward pass over the logits (cvk_seg_loss_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, logits, target, weight, opts):
        ce, dice, gamma, smooth, average, ignore_index, grad_scale = opts
        lib = _lib.load()
        lg, ld, tg, weight, (N, C, H, W) = _check_inputs("SegmentationLoss", logits, target, weight)
        M = N * H * W
        nfloats = lib.cvk_seg_loss_part_floats(M, C)
        if nfloats <= 0:
            raise RuntimeError(f"pytorch_camvid_amd.SegmentationLoss serves 1 to 128 classes and a non-empty batch, got C = {C}, M = {M}")
        part = torch.empty(nfloats, device=logits.device, dtype=torch.float32)
        rec = torch.empty(lib.cvk_seg_loss_record_floats(C), device=logits.device, dtype=torch.float32)
        _launch("k_seg_fwd", 4.0 * M * ld + 8.0 * M, lib.cvk_seg_loss_fwd,
                lg.data_ptr(), ld, tg.data_ptr(), _ptr(weight), ce, dice, gamma, smooth, DICE_AVERAGES[average], part.data_ptr(),
                rec.data_ptr(), M, C, int(ignore_index), _stream(logits))
        ctx.save_for_backward(lg, tg, rec, weight)
        ctx.meta = (N, C, H, W, ld, ce, dice, gamma, float(grad_scale), int(ignore_index))
        _CrossEntropy.last_status = rec
        return rec[0].clone()           # not a view: rec is saved for backward (divisor, a_c, b_c) and published as the status

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        lg, tg, rec, weight = ctx.saved_tensors
        N, C, H, W, ld, ce, dice, gamma, grad_scale, ignore_index = ctx.meta
        M = N * H * W
        d, g = _grad_buffers(lg, gout, N, C, H, W)
        _launch("k_seg_bwd", 4.0 * M * ld + 8.0 * M + 4.0 * M * C, lib.cvk_seg_loss_bwd,
                lg.data_ptr(), ld, tg.data_ptr(), _ptr(weight), ce, dice, gamma, rec.data_ptr(), g.data_ptr(), grad_scale, d.data_ptr(),
                C, M, C, ignore_index, _stream(lg))
        return d.permute(0, 3, 1, 2), None, None, None


def _nonneg(name, v):
    v = float(v)
    if not 0.0 <= v < float("inf"):
        raise ValueError(f"{name} must be a finite number >= 0. Got: {v}")
    return v


def _check_seg_options(ce, dice, focal_gamma, weight, dice_smooth, dice_average):
    ce, dice = _nonneg("ce", ce), _nonneg("dice", dice)
    if ce == 0.0 and dice == 0.0:
        raise ValueError("ce and dice must not both be 0")
    if dice_average not in DICE_AVERAGES:
        raise ValueError(f"{dice_average} is not a valid value for dice_average (one of {sorted(DICE_AVERAGES)})")
    _check_weight_option(weight)
    return ce, dice, _nonneg("focal_gamma", focal_gamma), _nonneg("dice_smooth", dice_smooth)


class SegmentationLoss(_LastRecord, nn.Module):
    """`ce * Focal_gamma + dice * Dice` as one autograd node: one HIP pass over the logits forward (plus a one-workgroup finish), one
    backward.  With p = softmax(logits) over the classes and every sum over the pixels of the whole batch whose target is not
    `ignore_index`:
      focal  F = sum w[t] (1 - p[t])^focal_gamma (-log p[t]) / sum w[t]      (focal_gamma = 0: torch's weighted mean cross-entropy)
      Dice   D = 1 - mean over S of (2 I_c + s) / (P_c + T_c + s), I_c = sum p[c] [t = c], P_c = sum p[c], T_c = sum [t = c],
             s = `dice_smooth`; S = the classes that occur in the batch (`dice_average="present"`) or all of them (`"all"`)
    `weight` (float32 [C] on the logits' device, a registered buffer as in CrossEntropyLoss) enters the focal term only.  A term whose
    coefficient is 0 is not computed.  Conventions of CrossEntropyLoss hold: float32 logits [N, C, H, W] (C <= 128) and int64 targets
    [N, H, W] on the GPU, a 0-dim loss, an out-of-range target makes the loss NaN and `last_ce_status()` reports it, with every pixel
    ignored the focal term is 0/0 = NaN and the Dice term 0; `grad_scale` multiplies the backward only.  All sums run in a fixed order
    without float atomics: the loss and its gradient are bitwise reproducible.
    After a forward, `last_terms` ([F, D]) and `last_dice` (per class, 0 outside S) are views of the device record (`last_record`: [loss,
    valid, out of range, sum w[t], F, D, K, then dice_c, a_c, b_c]), read without a
    sync (a module captured by `GraphedStep` keeps viewing the record the replays rewrite, until it is called eagerly again).  Under `ddp.DataParallel` every rank takes the Dice sums I_c, P_c, T_c (and the focal divisor) over its own part of the
    batch: the averaged gradient is the mean of the per-rank losses' gradients, not the gradient of a Dice over the global batch."""

    def __init__(self, ce=1.0, dice=0.0, *, focal_gamma=0.0, weight=None, ignore_index=-100, dice_smooth=1.0, dice_average="present",
                 grad_scale=1.0):
        super().__init__()
        self.ce, self.dice, self.focal_gamma, self.dice_smooth = _check_seg_options(ce, dice, focal_gamma, weight, dice_smooth,
                                                                                    dice_average)
        self.dice_average = dice_average
        self.ignore_index = ignore_index
        self.grad_scale = grad_scale
        self.register_buffer("weight", weight)
        self._record = None

    def forward(self, logits, target):
        loss = _SegLoss.apply(logits, target, self.weight, (self.ce, self.dice, self.focal_gamma, self.dice_smooth, self.dice_average,
                                                            self.ignore_index, self.grad_scale))
        self._record = _CrossEntropy.last_status
        return loss

    @property
    def last_terms(self):
        """[F, D] of the most recent forward (device tensor, no sync)."""
        return self._rec()[4:6]

    @property
    def last_dice(self):
        """dice_c of the most recent forward, [C], 0 for the classes outside S (device tensor, no sync)."""
        r = self._rec()
        return r[SEG_RECORD_HEAD:SEG_RECORD_HEAD + (r.numel() - SEG_RECORD_HEAD) // 3]


class FocalLoss(SegmentationLoss):
    """SegmentationLoss(1.0, 0.0, focal_gamma=gamma): the class-weighted focal loss (Lin et al.), mean over the valid pixels."""

    def __init__(self, gamma=2.0, weight=None, ignore_index=-100):
        super().__init__(1.0, 0.0, focal_gamma=gamma, weight=weight, ignore_index=ignore_index)


class DiceLoss(SegmentationLoss):
    """SegmentationLoss(0.0, 1.0): the soft Dice loss over the whole batch."""

    def __init__(self, smooth=1.0, average="present", ignore_index=-100):
        super().__init__(0.0, 1.0, dice_smooth=smooth, dice_average=average, ignore_index=ignore_index)


def segmentation_loss(logits, target, ce=1.0, dice=0.0, *, focal_gamma=0.0, weight=None, ignore_index=-100, dice_smooth=1.0,
                      dice_average="present"):
    """Functional form of SegmentationLoss (same kernels)."""
    opts = _check_seg_options(ce, dice, focal_gamma, weight, dice_smooth, dice_average)
    return _SegLoss.apply(logits, target, weight, (opts[0], opts[1], opts[2], opts[3], dice_average, ignore_index, 1.0))


OHEM_RECORD = 8                                    # loss | V | out of range | sum_kept w[t] | kept | L | lambda | k


def ohem_loss_threshold(thresh):
    """The loss boundary of a probability threshold: float32(-log(thresh)), the logarithm taken in double and rounded once.  A pixel
    whose target probability is below `thresh` has a loss above it."""
    import math
    import numpy as np
    thresh = float(thresh)
    if not 0.0 < thresh <= 1.0:
        raise ValueError(f"thresh must be a probability in (0, 1]. Got: {thresh}")
    return float(np.float32(-math.log(thresh)))


def _check_ohem_options(thresh, min_kept, weight):
    lam = ohem_loss_threshold(thresh)
    if isinstance(min_kept, bool) or not isinstance(min_kept, int) or min_kept < 1:
        raise ValueError(f"min_kept must be an integer >= 1. Got: {min_kept!r}")
    _check_weight_option(weight)
    return lam, min(min_kept, 2 ** 31 - 1)


class _OhemCrossEntropy(torch.autograd.Function):
    """Online hard example mining over the per-pixel cross-entropy (cvk_ohem_ce_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, logits, target, weight, opts):
        lam, min_kept, ignore_index, grad_scale = opts
        lib = _lib.load()
        lg, ld, tg, weight, (N, C, H, W) = _check_inputs("OhemCrossEntropyLoss", logits, target, weight)
        M = N * H * W
        nbytes = lib.cvk_ohem_scratch_bytes(M)
        if nbytes <= 0 or not 1 <= C <= 128:
            raise RuntimeError(f"pytorch_camvid_amd.OhemCrossEntropyLoss serves 1 to 128 classes and a non-empty batch, got C = {C}, M = {M}")
        scratch = torch.empty(nbytes, device=logits.device, dtype=torch.uint8)
        rec = torch.empty(lib.cvk_ohem_record_floats(), device=logits.device, dtype=torch.float32)
        px = torch.empty((N, H, W), device=logits.device, dtype=torch.float32)
        _launch("k_ohem_fwd", 4.0 * M * ld + 8.0 * M + 16.0 * M, lib.cvk_ohem_ce_fwd,
                lg.data_ptr(), ld, tg.data_ptr(), _ptr(weight), lam, min_kept, scratch.data_ptr(), rec.data_ptr(), px.data_ptr(), M, C,
                int(ignore_index), _stream(logits))
        ctx.save_for_backward(lg, tg, rec, px, weight)
        ctx.meta = (N, C, H, W, ld, float(grad_scale), int(ignore_index))
        _CrossEntropy.last_status = rec
        _OhemCrossEntropy.last_pixel_loss = px
        return rec[0].clone()           # not a view: rec is saved for backward (divisor, L, lambda) and published as the status

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        lg, tg, rec, px, weight = ctx.saved_tensors
        N, C, H, W, ld, grad_scale, ignore_index = ctx.meta
        M = N * H * W
        d, g = _grad_buffers(lg, gout, N, C, H, W)
        _launch("k_ohem_bwd", 4.0 * M * ld + 12.0 * M + 4.0 * M * C, lib.cvk_ohem_ce_bwd,
                lg.data_ptr(), ld, tg.data_ptr(), _ptr(weight), rec.data_ptr(), px.data_ptr(), g.data_ptr(), grad_scale, d.data_ptr(),
                C, M, C, ignore_index, _stream(lg))
        return d.permute(0, 3, 1, 2), None, None, None


class OhemCrossEntropyLoss(_LastRecord, nn.Module):
    """Cross-entropy with online hard example mining as one autograd node (the rule of HRNet/OCR's OhemCrossEntropy and mmseg's
    OHEMPixelSampler): train on the pixels whose target probability is below `thresh`, and never on fewer than the `min_kept` hardest.
    With l = lse(x) - x[t] the unweighted fp32 loss of a valid pixel (t != `ignore_index`), V the number of valid pixels,
    lambda = `ohem_loss_threshold(thresh)` and L the min(min_kept, V)-th largest l, a valid pixel is kept iff l > lambda or l >= L:
      loss = sum_kept w[t] l / sum_kept w[t]
    Ties at the boundary are all kept, so at least min(min_kept, V) pixels always are.  (HRNet and mmseg take element `min_kept` of the
    ascending sort and compare strictly: a batch whose losses are all equal keeps nothing there and gives NaN; the two rules differ by
    at most the ties at the boundary.)  L is found on the device by an exact three-level radix select over the bit patterns of the
    losses: no sort, no compaction, no host sync, so the loss can be captured by `GraphedStep`; every float sum has one fixed order, so
    the loss and its gradient are bitwise reproducible.  The backward re-evaluates the predicate from the forward's saved loss map.
    Conventions of CrossEntropyLoss hold: float32 logits [N, C, H, W] (C <= 128), int64 targets [N, H, W], a 0-dim loss, `weight`
    (float32 [C], a registered buffer) weighs the kept pixels' mean, an out-of-range target makes the loss NaN and `last_ce_status()`
    reports it, no valid pixel gives 0/0 = NaN with a zero gradient, `grad_scale` multiplies the backward only.
    After a forward, device views for logging without a sync: `last_record` ([loss, V, out of range, sum_kept w[t], kept, L, lambda,
    k]), `last_kept`, `last_threshold` (min(lambda, L): a valid pixel is kept iff its loss reaches it, up to the strictness at lambda) and
    `last_pixel_loss` ([N, H, W], -1 where ignored).  Under `ddp.DataParallel` every rank selects over its own part of the batch, as
    the Dice sums of SegmentationLoss are per rank."""

    def __init__(self, thresh=0.7, min_kept=100000, *, weight=None, ignore_index=-100, grad_scale=1.0):
        super().__init__()
        self.loss_threshold, self.min_kept = _check_ohem_options(thresh, min_kept, weight)
        self.thresh = float(thresh)
        self.ignore_index = ignore_index
        self.grad_scale = grad_scale
        self.register_buffer("weight", weight)
        self._record = self._px = None

    def forward(self, logits, target):
        loss = _OhemCrossEntropy.apply(logits, target, self.weight, (self.loss_threshold, self.min_kept, self.ignore_index,
                                                                     self.grad_scale))
        self._record, self._px = _CrossEntropy.last_status, _OhemCrossEntropy.last_pixel_loss
        return loss

    @property
    def last_kept(self):
        """Number of kept pixels of the most recent forward (0-dim device view, no sync)."""
        return self._rec()[4]

    @property
    def last_threshold(self):
        """The effective loss boundary min(lambda, L) of the most recent forward (0-dim device tensor, no sync)."""
        r = self._rec()
        return torch.minimum(r[5], r[6])

    @property
    def last_pixel_loss(self):
        """The unweighted per-pixel losses of the most recent forward: [N, H, W], -1 where ignored, NaN where out of range."""
        self._rec()
        return self._px


def ohem_cross_entropy(logits, target, thresh, min_kept, weight=None, ignore_index=-100):
    """Functional form of OhemCrossEntropyLoss (same kernels)."""
    lam, min_kept = _check_ohem_options(thresh, min_kept, weight)
    return _OhemCrossEntropy.apply(logits, target, weight, (lam, min_kept, ignore_index, 1.0))


LOVASZ_CLASSES = {k: _lib.DEFINES["CVK_LOVASZ_" + k.upper()] for k in ("present", "all")}
LOVASZ_RECORD_HEAD = 8                             # loss | V | out of range | J | H | evaluated pairs | counted segments | sum w[t]
LOVASZ_CLASS_SLOTS = 128                           # L_c at [8 + c], G_c at [8 + 128 + c]
LOVASZ_SORT_TILE = _lib.DEFINES["CVK_LOVASZ_SORT_TILE"]   # elements a sort work-group covers


def _check_lovasz_options(lovasz, ce, classes, per_image, weight):
    lovasz, ce = _nonneg("lovasz", lovasz), _nonneg("ce", ce)
    if lovasz == 0.0:
        raise ValueError("lovasz must be greater than 0 (ce alone is CrossEntropyLoss)")
    if classes not in LOVASZ_CLASSES:
        raise ValueError(f"{classes} is not a valid value for classes (one of {sorted(LOVASZ_CLASSES)})")
    if not isinstance(per_image, bool):
        raise ValueError(f"per_image must be a bool. Got: {per_image!r}")
    _check_weight_option(weight)
    if weight is not None and ce == 0.0:
        raise ValueError("weight enters the cross-entropy term only and needs ce > 0 (class weights do not enter the Lovász term)")
    return lovasz, ce


class _LovaszSoftmax(torch.autograd.Function):
    """lovasz * Lovász-softmax + ce * weighted cross-entropy (cvk_lovasz_softmax_fwd / _bwd)."""

    _buffers = {}                                  # (M, C, segments, device) -> the workspace (sort buffers, g map, tables)

    @staticmethod
    def workspace(lib, M, C, S, device):
        key = (M, C, S, str(device))
        ws = _LovaszSoftmax._buffers.get(key)
        if ws is None:
            nbytes = lib.cvk_lovasz_workspace_bytes(M, C, S)
            if nbytes <= 0:
                raise RuntimeError(f"pytorch_camvid_amd.LovaszSoftmaxLoss serves 1 to 128 classes, segments of fewer than 2^30 pixels and "
                                   f"at most 65535 (segment, class) pairs, got C = {C}, M = {M}, segments = {S}")
            ws = _LovaszSoftmax._buffers[key] = torch.empty(nbytes, device=device, dtype=torch.uint8)
        return ws

    @staticmethod
    def forward(ctx, logits, target, weight, opts):
        lovasz, ce, classes, per_image, ignore_index, grad_scale = opts
        lib = _lib.load()
        lg, ld, tg, weight, (N, C, H, W) = _check_inputs("LovaszSoftmaxLoss", logits, target, weight)
        M, S = N * H * W, (N if per_image else 1)
        if not 1 <= C <= 128 or M <= 0:
            raise RuntimeError(f"pytorch_camvid_amd.LovaszSoftmaxLoss serves 1 to 128 classes and a non-empty batch, got C = {C}, M = {M}")
        ws = _LovaszSoftmax.workspace(lib, M, C, S, logits.device)
        gmap = ws[16 * M * C:20 * M * C].view(torch.float32).view(M, C)        # the room include/cvk.h reserves for a dense g map
        rec = torch.empty(lib.cvk_lovasz_record_floats(), device=logits.device, dtype=torch.float32)
        # bytes: the logits, the targets, the elements written once, 4 passes reading them twice and writing them once, the weight
        # pass reading them twice (8 B each) and scattering g (4 B)
        _launch("k_lovasz_fwd", 4.0 * M * ld + 8.0 * M + 8.0 * M * C * (1 + 3 * 4 + 2) + 4.0 * M * C, lib.cvk_lovasz_softmax_fwd,
                lg.data_ptr(), ld, tg.data_ptr(), _ptr(weight), lovasz, ce, LOVASZ_CLASSES[classes], int(per_image), N, H * W, ws.data_ptr(),
                rec.data_ptr(), gmap.data_ptr(), C, C, int(ignore_index), _stream(logits))
        ctx.save_for_backward(lg, tg, rec, weight)
        ctx.ws = ws                                # shared by every call of this size: backward must run before the next forward
        ctx.meta = (N, C, H, W, ld, lovasz, ce, int(per_image), float(grad_scale), int(ignore_index))
        _CrossEntropy.last_status = rec
        _LovaszSoftmax.last_sorted = (ws, S, C, M // S)
        return rec[0].clone()           # not a view: rec is saved for backward (H's divisor) and published as the status

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        lg, tg, rec, weight = ctx.saved_tensors
        N, C, H, W, ld, lovasz, ce, per_image, grad_scale, ignore_index = ctx.meta
        M = N * H * W
        ws = ctx.ws
        gmap = ws[16 * M * C:20 * M * C]
        d, g = _grad_buffers(lg, gout, N, C, H, W)
        _launch("k_lovasz_bwd", 4.0 * M * ld + 8.0 * M + 8.0 * M * C, lib.cvk_lovasz_softmax_bwd,
                lg.data_ptr(), ld, tg.data_ptr(), _ptr(weight), lovasz, ce, per_image, N, H * W, ws.data_ptr(), rec.data_ptr(),
                gmap.data_ptr(), C, g.data_ptr(), grad_scale, d.data_ptr(), C, C, ignore_index, _stream(lg))
        return d.permute(0, 3, 1, 2), None, None, None


class LovaszSoftmaxLoss(_LastRecord, nn.Module):
    """`lovasz * J + ce * H` as one autograd node: J the Lovász-softmax loss (Berman, Triki and Blaschko, CVPR 2018; mmseg's `LovaszLoss`
    with `loss_type="multi_class"`), the convex surrogate of the Jaccard index this project reports, and H the weighted mean
    cross-entropy of CrossEntropyLoss(weight=) it is usually added to.  Per segment (the whole batch, or one image with `per_image=True`)
    and class c, over the valid pixels (t != `ignore_index`) in memory order i, with p = softmax(logits) in fp32:
      e_i = p_i[c] where t_i != c and 1 - p_i[c] where t_i = c (as the other classes' share of the sum, so it does not cancel)
      the pixels are ordered by e descending, ties by ascending i; with G the class's pixel count, n a pixel's position and F the
      foreground pixels before it, U = G + n - F and I = G - F, its weight is g = 1 / U (foreground) or I / (U (U + 1)) (background),
      which is the step of the Jaccard loss 1 - I / U along the order (G = 0: g = 1 at n = 0, 0 elsewhere)
      L_c = sum e_i g_i in fp64
    A segment's loss is the mean of L_c over the classes that occur in it (`classes="present"`) or over all of them (`"all"`); a segment
    without a valid pixel is not counted; J is the mean over the counted segments, 0 when there is none (never NaN).  `weight` (float32
    [C] on the logits' device, a registered buffer) enters H only and needs `ce > 0`; with `ce == 0` H is not computed.
    The order comes from a stable segmented LSD radix sort on the device (8 bits a pass over a 32-bit key, one 64-bit element per pixel
    and class): no torch.sort, no allocation after the first call of a size, no host sync, so the loss can be captured by `GraphedStep`
    (with `optimizer=` and `accumulator=`); every histogram is an integer count and every float sum has one fixed order, so the loss and
    its gradient are bitwise reproducible, ties included.
    Conventions of CrossEntropyLoss hold: float32 logits [N, C, H, W] (C <= 128; channels_last is read in place), int64 targets
    [N, H, W], a 0-dim loss, an out-of-range target makes the loss NaN and `last_ce_status()` reports it, `grad_scale` multiplies the
    backward only.  The workspace (two sort buffers of 8 bytes per pixel and class, the g map of 4, small tables) is kept per (pixels,
    classes, segments, device) and shared by every loss of that size: run a forward's backward before the next forward of the same size.
    After a forward, device views for logging without a sync: `last_record` ([loss, V, out of range, J, H, evaluated (segment, class)
    pairs, counted segments, sum w[t], then L_c at 8 + c and G_c at 136 + c]), `last_terms` ([J, H]), `last_class_loss` ([C], NaN
    where no segment evaluated the class) and `sorted_view()`.  Under `ddp.DataParallel` every rank sorts its own part of the batch:
    the averaged gradient is the mean of the per-rank losses' gradients, not the gradient of a Lovász loss over the global batch, as
    the Dice sums of SegmentationLoss and the selection of OhemCrossEntropyLoss are per rank.
    Not provided: the binary Lovász hinge, per-class weights on the Lovász term, segments of 2^30 pixels or more, a sort shared across
    ranks."""

    def __init__(self, lovasz=1.0, ce=0.0, *, classes="present", per_image=False, weight=None, ignore_index=-100, grad_scale=1.0):
        super().__init__()
        self.lovasz, self.ce = _check_lovasz_options(lovasz, ce, classes, per_image, weight)
        self.classes = classes
        self.per_image = per_image
        self.ignore_index = ignore_index
        self.grad_scale = grad_scale
        self.register_buffer("weight", weight)
        self._record = self._sorted = None
        self._C = 0

    def forward(self, logits, target):
        loss = _LovaszSoftmax.apply(logits, target, self.weight, (self.lovasz, self.ce, self.classes, self.per_image, self.ignore_index,
                                                                   self.grad_scale))
        self._record, self._sorted, self._C = _CrossEntropy.last_status, _LovaszSoftmax.last_sorted, logits.shape[1]
        return loss

    @property
    def last_terms(self):
        """[J, H] of the most recent forward (device tensor, no sync)."""
        return self._rec()[3:5]

    @property
    def last_class_loss(self):
        """L_c of the most recent forward, [C], NaN for a class no segment evaluated (device tensor, no sync)."""
        return self._rec()[LOVASZ_RECORD_HEAD:LOVASZ_RECORD_HEAD + self._C]

    @property
    def last_class_pixels(self):
        """G_c of the most recent forward, [C] (device tensor, no sync)."""
        o = LOVASZ_RECORD_HEAD + LOVASZ_CLASS_SLOTS
        return self._rec()[o:o + self._C]

    def sorted_view(self):
        """The sorted buffer of the most recent forward as (keys uint32, pixel index int64, fg bool), each [S, C, segment length]:
        keys is a view of the workspace, the other two are unpacked from its payload words.  Position n of segment (s, c) holds the
        pixel with the n-th largest error of class c; key = 0x3f800000 - bits(e), 0xffffffff for a pixel that is not valid.  The
        workspace is shared: read it before another loss of the same size runs."""
        self._rec()
        ws, S, C, P = self._sorted
        words = ws[:8 * S * C * P].view(torch.int32).view(S, C, P, 2)          # little endian: payload word, then key word
        payload = words[..., 0].to(torch.int64) & 0xFFFFFFFF
        return words[..., 1].view(torch.uint32), payload >> 1, (payload & 1).bool()


def lovasz_softmax(logits, target, lovasz=1.0, ce=0.0, *, classes="present", per_image=False, weight=None, ignore_index=-100):
    """Functional form of LovaszSoftmaxLoss (same kernels)."""
    lovasz, ce = _check_lovasz_options(lovasz, ce, classes, per_image, weight)
    return _LovaszSoftmax.apply(logits, target, weight, (lovasz, ce, classes, per_image, ignore_index, 1.0))


BDL_RECORD_HEAD = 8                                # loss | |V| | out of range | B | H | boundary coef | ce coef | sum w[t], then B's class shares
EDT_MAX_CLASSES = 32


class _DistanceMaps:
    """The device buffers of the distance transform, kept per (N, H, W, classes, device): the uint16 column maps (+ presence words) that
    both entry points use as workspace, and the float32 phi maps the boundary loss reads."""

    _buffers = {}

    @staticmethod
    def get(lib, N, H, W, C, device, want_phi):
        key = (N, H, W, C, str(device))
        ent = _DistanceMaps._buffers.get(key)
        if ent is None:
            nbytes = lib.cvk_edt_workspace_bytes(N, H, W, C)
            if nbytes <= 0:
                raise ValueError(f"the distance transform serves 1 to {EDT_MAX_CLASSES} classes, H <= 65534, (H - 1)^2 + (W - 1)^2 < 2^24 "
                                 f"and fewer than 2^31 pixels, got N = {N}, H = {H}, W = {W}, classes = {C}")
            ent = _DistanceMaps._buffers[key] = [torch.empty(nbytes, device=device, dtype=torch.uint8), None]
        if want_phi and ent[1] is None:
            ent[1] = torch.empty((N, H, W, C), device=device, dtype=torch.float32)
        return ent

    @staticmethod
    def signed(lib, labels, C, ignore_index):
        """phi of `labels` (contiguous int64 [N,H,W] on the GPU) in the shared [N,H,W,C] buffer of its shape."""
        N, H, W = labels.shape
        ws, phi = _DistanceMaps.get(lib, N, H, W, C, labels.device, True)
        M = N * H * W
        # bytes: the labels read by both passes, the column maps written and read, phi written
        _launch("k_edt_signed", 16.0 * M + 4.0 * M * (C + 1) + 4.0 * M * C, lib.cvk_edt_signed,
                labels.data_ptr(), N, H, W, C, int(ignore_index), ws.data_ptr(), phi.data_ptr(), _stream(labels))
        return phi


def _check_label_maps(who, labels, num_classes):
    if not (isinstance(labels, torch.Tensor) and labels.dtype == torch.int64 and labels.dim() == 3 and labels.numel() > 0):
        raise ValueError(f"{who}: expected an int64 tensor of shape [N, H, W]")
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= EDT_MAX_CLASSES:
        raise ValueError(f"{who} serves 1 to {EDT_MAX_CLASSES} classes. Got: {num_classes}")
    if not labels.is_cuda:
        raise ValueError(f"{who}: expected a tensor on the GPU (no CPU fallback)")


def squared_distance_maps(labels, num_classes=12, ignore_index=11):
    """The exact squared Euclidean distance transform of an int64 label batch [N,H,W] on the GPU, per image:
    `to_class` int32 [N,H,W,C], the squared distance to the nearest pixel whose label is c (-1 where the image has none), and `to_other`
    int32 [N,H,W], the squared distance to the nearest pixel whose label differs from this pixel's (-1 where there is none).  A label
    that is `ignore_index` or outside [0, num_classes) is void: such a pixel belongs to no class but is a pixel, so it is "not class c"
    for every c and differs from every class pixel.  Two launches (columns, then rows), no host sync; the result tensors are new."""
    _check_label_maps("squared_distance_maps", labels, num_classes)
    lib = _lib.load()
    m = labels.contiguous()
    N, H, W = m.shape
    ws, _ = _DistanceMaps.get(lib, N, H, W, num_classes, m.device, False)
    to_class = torch.empty((N, H, W, num_classes), device=m.device, dtype=torch.int32)
    to_other = torch.empty((N, H, W), device=m.device, dtype=torch.int32)
    check(lib.cvk_edt_squared(m.data_ptr(), N, H, W, num_classes, int(ignore_index), ws.data_ptr(), to_class.data_ptr(),
                              to_other.data_ptr(), _stream(m)), "cvk_edt_squared")
    return to_class, to_other


def signed_distance_maps(labels, num_classes=12, ignore_index=11):
    """Kervadec's signed distance maps phi of an int64 label batch [N,H,W] on the GPU, float32 [N,C,H,W] (a channels_last view of a new
    tensor): +sqrt(to_class) where the pixel is not of class c, -(sqrt(to_other) - 1) where it is, 0 where the needed distance does not
    exist (the class is absent from the image, or the image is all one class).  The integers are those of `squared_distance_maps`; the
    root is the correctly rounded fp32 root."""
    _check_label_maps("signed_distance_maps", labels, num_classes)
    lib = _lib.load()
    m = labels.contiguous()
    return _DistanceMaps.signed(lib, m, num_classes, ignore_index).clone().permute(0, 3, 1, 2)


def _check_boundary_loss_options(boundary, ce, classes, weight):
    boundary, ce = _nonneg("boundary", boundary), _nonneg("ce", ce)
    if boundary == 0.0 and ce == 0.0:
        raise ValueError("boundary and ce are both 0: the loss has no term")
    if classes is not None:
        classes = tuple(classes)
        if not classes or any(isinstance(c, bool) or not isinstance(c, int) or not 0 <= c < EDT_MAX_CLASSES for c in classes):
            raise ValueError(f"classes must be None or a non-empty sequence of class indices in [0, {EDT_MAX_CLASSES}). Got: {classes!r}")
        if len(set(classes)) != len(classes):
            raise ValueError(f"classes must be distinct. Got: {classes!r}")
        if boundary == 0.0:
            raise ValueError("classes selects the classes of the boundary term, and boundary is 0")
    _check_weight_option(weight)
    if weight is not None and ce == 0.0:
        raise ValueError("weight enters the cross-entropy term only and needs ce > 0 (class weights do not enter the boundary term)")
    return boundary, ce, classes


class _BoundaryLoss(torch.autograd.Function):
    """coef[0] * boundary loss + coef[1] * weighted cross-entropy (cvk_edt_signed, cvk_boundary_loss_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, logits, target, weight, coef, opts):
        want_b, want_ce, classes, ignore_index, grad_scale = opts
        lib = _lib.load()
        lg, ld, tg, weight, (N, C, H, W) = _check_inputs("BoundaryLoss", logits, target, weight)
        M = N * H * W
        if not 1 <= C <= EDT_MAX_CLASSES or M <= 0:
            raise RuntimeError(f"pytorch_camvid_amd.BoundaryLoss serves 1 to {EDT_MAX_CLASSES} classes and a non-empty batch, got C = {C}, "
                               f"M = {M}")
        if classes is not None and max(classes) >= C:
            raise ValueError(f"classes names class {max(classes)} but the logits have {C} channels")
        if coef.device != logits.device or coef.dtype != torch.float32 or coef.numel() != 2:
            raise RuntimeError(f"the coefficient buffer must be 2 float32 values on {logits.device}")
        if ld > 63:                                # the kernels stage a pixel row of at most 63 floats
            lg, ld = lg.contiguous(), C
        cmask = sum(1 << c for c in (range(C) if classes is None else classes)) if want_b else 0
        phi = _DistanceMaps.signed(lib, tg, C, ignore_index) if want_b else None
        part = torch.empty(lib.cvk_boundary_loss_part_floats(M, C), device=logits.device, dtype=torch.float32)
        rec = torch.empty(lib.cvk_boundary_loss_record_floats(), device=logits.device, dtype=torch.float32)
        _launch("k_bdl_fwd", 4.0 * M * ld + 8.0 * M + (4.0 * M * C if want_b else 0.0), lib.cvk_boundary_loss_fwd,
                lg.data_ptr(), ld, tg.data_ptr(), _ptr(phi), _ptr(weight), coef.data_ptr(), want_b, want_ce, cmask, part.data_ptr(),
                rec.data_ptr(), M, C, int(ignore_index), _stream(logits))
        ctx.save_for_backward(lg, tg, rec, weight)
        ctx.phi = phi                              # shared by every call of this shape: backward must run before the next forward
        ctx.meta = (N, C, H, W, ld, want_b, want_ce, cmask, float(grad_scale), int(ignore_index))
        _CrossEntropy.last_status = rec
        _BoundaryLoss.last_maps = phi
        return rec[0].clone()           # not a view: rec is saved for backward and published as the status

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        lg, tg, rec, weight = ctx.saved_tensors
        N, C, H, W, ld, want_b, want_ce, cmask, grad_scale, ignore_index = ctx.meta
        M = N * H * W
        d, g = _grad_buffers(lg, gout, N, C, H, W)
        _launch("k_bdl_bwd", 4.0 * M * ld + 8.0 * M + (4.0 * M * C if want_b else 0.0) + 4.0 * M * C, lib.cvk_boundary_loss_bwd,
                lg.data_ptr(), ld, tg.data_ptr(), _ptr(ctx.phi), _ptr(weight), want_b, want_ce, cmask, rec.data_ptr(), g.data_ptr(),
                grad_scale, d.data_ptr(), C, M, C, ignore_index, _stream(lg))
        return d.permute(0, 3, 1, 2), None, None, None, None


class BoundaryLoss(_LastRecord, nn.Module):
    """`boundary * B + ce * H` as one autograd node: B the boundary loss of Kervadec et al. ("Boundary loss for highly unbalanced
    segmentation", MIDL 2019) and H the weighted mean cross-entropy of CrossEntropyLoss(weight=) it is usually ramped in next to.
      B = 1 / |V| sum over the pixels q of V of sum over the classes c of S of phi_c(q) softmax(logits)_c(q)
    V = the pixels whose target is not `ignore_index`, S = `classes` (Kervadec's `idc`; None: every class), phi_c = the signed Euclidean
    distance map of the target's class-c region, computed per image on the device at every call by an exact distance transform
    (`signed_distance_maps`: positive outside the region, -(distance - 1) inside, 0 where the class is absent from the image or fills
    it).  Ignored pixels are void: they belong to no class, get a zero gradient row, and bound the regions next to them.  V empty
    gives B = 0 and a zero gradient (H alone is 0/0 = NaN there, as CrossEntropyLoss).  `weight` (float32 [C] on the logits' device, a
    registered buffer) enters H only and needs `ce > 0`.
    The two coefficients live in a registered 2-float device buffer (`coef`) that the kernels read: `loss.boundary = 0.02` and
    `loss.ce = ...` fill it on the current stream without a sync, so a captured `GraphedStep` follows a schedule without a re-capture.
    Which terms exist is fixed at construction: a coefficient that was 0 there is never computed, and raising it later is a ValueError.
    Conventions of CrossEntropyLoss hold: float32 logits [N, C, H, W] (C <= 32; channels_last is read in place), int64 targets
    [N, H, W], a 0-dim loss, an out-of-range target makes the loss NaN and `last_ce_status()` reports it, `grad_scale` multiplies the
    backward only.  No float atomic, allocation after the first call of a shape, or host sync: the loss is bitwise reproducible and
    can be captured (with `optimizer=` and `accumulator=`).  The column maps (2 bytes per pixel and class + 1) and phi (4 bytes per pixel
    and class) are kept per (shape, classes, device) and shared by every loss of that shape: run a forward's backward before the next
    forward of the same shape.  After a forward, device views without a sync: `last_record` ([loss, |V|, out of range, B, H, the two
    coefficients used, sum w[t], then each class's share of B]), `last_terms` ([B, H]), `last_class_terms` ([C]) and `last_maps` (phi,
    [N, C, H, W]).  Under `ddp.DataParallel` |V| is per rank, as for the other losses.
    Not provided: 3-D or anisotropic spacing, a Hausdorff / HD95 loss, chamfer approximations, per-class weights on B, maps cached
    across epochs."""

    def __init__(self, boundary=1.0, ce=0.0, *, classes=None, weight=None, ignore_index=-100, grad_scale=1.0):
        super().__init__()
        self._boundary, self._ce, self.classes = _check_boundary_loss_options(boundary, ce, classes, weight)
        self._terms = (int(self._boundary > 0.0), int(self._ce > 0.0))          # fixed here
        self.ignore_index = ignore_index
        self.grad_scale = grad_scale
        self.register_buffer("weight", weight)
        self.register_buffer("coef", torch.tensor([self._boundary, self._ce], dtype=torch.float32))
        self._record = self._maps = None
        self._C = 0

    def _set(self, slot, name, v):
        v = _nonneg(name, v)
        if v > 0.0 and not self._terms[slot]:
            raise ValueError(f"{name} was 0 at construction, so that term is not computed: construct the loss with {name} > 0")
        self.coef[slot:slot + 1].fill_(v)          # on the current stream, no sync: the kernels read it from there
        return v

    @property
    def boundary(self):
        return self._boundary

    @boundary.setter
    def boundary(self, v):
        self._boundary = self._set(0, "boundary", v)

    @property
    def ce(self):
        return self._ce

    @ce.setter
    def ce(self, v):
        self._ce = self._set(1, "ce", v)

    def forward(self, logits, target):
        if self.coef.device != logits.device and logits.is_cuda:
            self.coef = self.coef.to(logits.device)        # once, at the first call (before any capture)
        loss = _BoundaryLoss.apply(logits, target, self.weight, self.coef,
                                   (self._terms[0], self._terms[1], self.classes, self.ignore_index, self.grad_scale))
        self._record, self._maps, self._C = _CrossEntropy.last_status, _BoundaryLoss.last_maps, logits.shape[1]
        return loss

    @property
    def last_terms(self):
        """[B, H] of the most recent forward (device tensor, no sync)."""
        return self._rec()[3:5]

    @property
    def last_class_terms(self):
        """Each class's share of B in the most recent forward, [C]; they sum to B (device tensor, no sync)."""
        return self._rec()[BDL_RECORD_HEAD:BDL_RECORD_HEAD + self._C]

    @property
    def last_maps(self):
        """phi of the most recent forward, float32 [N, C, H, W] (a channels_last view of the shared buffer; None without the boundary
        term).  Read it before another loss of the same shape runs."""
        self._rec()
        return None if self._maps is None else self._maps.permute(0, 3, 1, 2)


def boundary_loss(logits, target, boundary=1.0, ce=0.0, *, classes=None, weight=None, ignore_index=-100):
    """Functional form of BoundaryLoss (same kernels; the two coefficients are copied to the device at every call)."""
    boundary, ce, classes = _check_boundary_loss_options(boundary, ce, classes, weight)
    coef = torch.tensor([boundary, ce], dtype=torch.float32).to(logits.device)
    return _BoundaryLoss.apply(logits, target, weight, coef, (int(boundary > 0.0), int(ce > 0.0), classes, ignore_index, 1.0))


KD_RECORD = 9                                      # loss | valid | out of range | sum w[t] | H | K | |D| | agree | agree / |D|


def distillation_scales(temperature):
    """(tau, t2) = (float32(1 / T), float32(T * T)) of a temperature T > 0: each evaluated in double and rounded once, the two numbers
    the distillation kernels take."""
    import numpy as np
    T = float(temperature)
    if not 0.0 < T < float("inf"):
        raise ValueError(f"temperature must be a finite number > 0. Got: {T}")
    if not 1e-18 <= T <= 1e18:
        raise ValueError(f"temperature {T} leaves float32's range as 1 / T or T * T")
    return float(np.float32(1.0 / T)), float(np.float32(T * T))


def _check_kd_options(ce, kd, temperature, weight):
    ce, kd = _nonneg("ce", ce), _nonneg("kd", kd)
    if ce == 0.0 and kd == 0.0:
        raise ValueError("ce and kd must not both be 0")
    _check_weight_option(weight)
    return (ce, kd) + distillation_scales(temperature)


class _Distillation(torch.autograd.Function):
    """ce * cross-entropy + kd * T^2 KL(teacher || student) at temperature T in one forward and one backward pass over both logit
    tensors (cvk_kd_loss_fwd / _bwd).  The teacher is a constant: its gradient is None."""

    @staticmethod
    def forward(ctx, logits, target, teacher, weight, opts):
        ce, kd, tau, t2, distill_ignored, ignore_index, grad_scale = opts
        lib = _lib.load()
        lg, ld, tg, weight, (N, C, H, W) = _check_inputs("DistillationLoss", logits, target, weight, target_optional=True)
        if target is None:
            if ce > 0.0:
                raise ValueError("target=None needs ce == 0 (distillation on unlabelled frames)")
        elif target.device != logits.device:
            raise RuntimeError(f"target is on {target.device} but the logits are on {logits.device}")
        if teacher is None:
            if kd > 0.0:
                raise ValueError("teacher_logits=None needs kd == 0")
        elif tuple(teacher.shape) != tuple(logits.shape) or teacher.dtype != logits.dtype or teacher.device != logits.device:
            raise ValueError(f"the teacher's logits must match the student's: student {list(logits.shape)} {logits.dtype} on "
                             f"{logits.device}, teacher {list(teacher.shape)} {teacher.dtype} on {teacher.device}")
        M = N * H * W
        if not 1 <= C <= 128 or M <= 0:
            raise RuntimeError(f"pytorch_camvid_amd.DistillationLoss serves 1 to 128 classes and a non-empty batch, got C = {C}, M = {M}")
        tc, ld_t = _as_nhwc(teacher.detach()) if teacher is not None and kd > 0.0 else (None, 0)
        part = torch.empty(lib.cvk_kd_loss_part_floats(M), device=logits.device, dtype=torch.float32)
        rec = torch.empty(lib.cvk_kd_loss_record_floats(), device=logits.device, dtype=torch.float32)
        _launch("k_kd_fwd", 4.0 * M * (ld + ld_t) + 8.0 * M, lib.cvk_kd_loss_fwd,
                lg.data_ptr(), ld, _ptr(tc), ld_t, _ptr(tg), _ptr(weight), ce, kd, tau, t2, int(bool(distill_ignored)), part.data_ptr(),
                rec.data_ptr(), M, C, int(ignore_index), _stream(logits))
        ctx.save_for_backward(lg, tc, tg, rec, weight)
        ctx.meta = (N, C, H, W, ld, ld_t, ce, kd, tau, t2, int(bool(distill_ignored)), float(grad_scale), int(ignore_index))
        _CrossEntropy.last_status = rec
        return rec[0].clone()           # not a view: rec is saved for backward (the two divisors) and published as the status

    @staticmethod
    def backward(ctx, gout):
        lib = _lib.load()
        lg, tc, tg, rec, weight = ctx.saved_tensors
        N, C, H, W, ld, ld_t, ce, kd, tau, t2, distill_ignored, grad_scale, ignore_index = ctx.meta
        M = N * H * W
        d, g = _grad_buffers(lg, gout, N, C, H, W)
        _launch("k_kd_bwd", 4.0 * M * (ld + ld_t) + 8.0 * M + 4.0 * M * C, lib.cvk_kd_loss_bwd,
                lg.data_ptr(), ld, _ptr(tc), ld_t, _ptr(tg), _ptr(weight), ce, kd, tau, t2, distill_ignored, rec.data_ptr(), g.data_ptr(),
                grad_scale, d.data_ptr(), C, M, C, ignore_index, _stream(lg))
        return d.permute(0, 3, 1, 2), None, None, None, None


class _BoundDistillation:
    """`DistillationLoss.bind(buf)`: the two-argument `loss_fn(logits, target)` over a persistent teacher-logits buffer; `.loss` is the
    module, `.teacher_logits` the buffer."""

    def __init__(self, loss, buf):
        self.loss, self.teacher_logits = loss, buf

    def __call__(self, logits, target):
        return self.loss(logits, target, self.teacher_logits)


class DistillationLoss(_LastRecord, nn.Module):
    """Pixel-wise knowledge distillation (Hinton et al.) as one autograd node: `ce * H + kd * K`, one HIP pass over the student's and
    the teacher's logits forward (plus a one-workgroup finish), one backward.  With x a pixel's student logits, z the teacher's,
    T = `temperature`, tau = float32(1 / T) and t2 = float32(T * T) (`distillation_scales`):
      H = sum w[t] (lse(x) - x[t]) / sum w[t] over the valid pixels (t != `ignore_index`): torch's weighted mean cross-entropy
      K = t2 / |D| * sum over D of KL(softmax(tau z) || softmax(tau x))
    D = the valid pixels, or every pixel of the batch with `distill_ignored=True` (CamVid's void class has no label, but the teacher
    still has an opinion there).  `weight` (float32 [C] on the logits' device, a registered buffer) enters H only.  A term whose
    coefficient is 0 is not computed: `kd=0` needs no teacher and is the weighted cross-entropy, `ce=0` needs no target
    (`loss(logits, None, teacher_logits)`: unlabelled frames, every pixel in D).  The gradient goes to the student only; the teacher's
    logits are a constant even if they require a gradient.  They must have the student's shape, dtype and device; channels_last (as the
    package's networks return them, padded pixel stride included) is read in place, any other layout is copied once.
    Conventions of CrossEntropyLoss hold: float32 logits [N, C, H, W] (C <= 128), int64 targets [N, H, W], a 0-dim loss, an out-of-range
    target makes the loss NaN (such a pixel is in neither set) and `last_ce_status()` reports it, no valid pixel gives H = 0/0 = NaN,
    `grad_scale` multiplies the backward only.  All sums run in a fixed order without float atomics: loss and gradient are bitwise
    reproducible.  `ce`, `kd`, `temperature` and `distill_ignored` are read at every call, so a temperature schedule is an assignment
    (a captured `GraphedStep` keeps the values it was captured with).
    After a forward, device views for logging without a sync: `last_terms` ([H, K]), `last_agreement` (the share of D where student
    and teacher agree on the arg-max, first maximum as `argmax_channels`) and `last_record` ([loss, valid, out of range, sum w[t], H,
    K, |D|, agree, agree / |D|]).
    `bind(buf)` gives the two-argument form every `loss_fn(logits, target)` interface takes (`GraphedStep`, `evaluate_report`,
    `GradAccumulator`'s eager loop): `buf` is a persistent tensor of the logits' shape, and before each `step.replay(x, t)` the caller
    writes `buf.copy_(teacher(x))` under `no_grad` on the same stream.  Not provided: the teacher's forward inside the captured
    graph; the bound form together with `GraphedStep(accumulator=)` (one buffer cannot hold a window: the eager accumulation loop,
    which passes each micro-batch's teacher logits, does work); per-class temperatures; feature- or attention-map distillation; an
    EMA ("mean") teacher.  Under `ddp.DataParallel` the sums (and |D|) are per rank, as the Dice sums of SegmentationLoss are."""

    def __init__(self, ce=1.0, kd=1.0, temperature=4.0, *, weight=None, ignore_index=-100, distill_ignored=False, grad_scale=1.0):
        super().__init__()
        self.ce, self.kd, _, _ = _check_kd_options(ce, kd, temperature, weight)
        self.temperature = float(temperature)
        self.distill_ignored = bool(distill_ignored)
        self.ignore_index = ignore_index
        self.grad_scale = grad_scale
        self.register_buffer("weight", weight)
        self._record = None

    def forward(self, logits, target, teacher_logits=None):
        ce, kd, tau, t2 = _check_kd_options(self.ce, self.kd, self.temperature, self.weight)
        loss = _Distillation.apply(logits, target, teacher_logits, self.weight,
                                   (ce, kd, tau, t2, self.distill_ignored, self.ignore_index, self.grad_scale))
        self._record = _CrossEntropy.last_status
        return loss

    def bind(self, buf):
        """`(logits, target) -> self(logits, target, buf)` over the persistent teacher-logits tensor `buf`."""
        if not isinstance(buf, torch.Tensor) or buf.dim() != 4:
            raise ValueError("bind() takes the persistent teacher-logits tensor, [N, C, H, W]")
        return _BoundDistillation(self, buf)

    @property
    def last_terms(self):
        """[H, K] of the most recent forward (device tensor, no sync)."""
        return self._rec()[4:6]

    @property
    def last_agreement(self):
        """Share of the pixels of D where student and teacher agree on the arg-max (0-dim device view, no sync)."""
        return self._rec()[8]


def distillation_loss(logits, target, teacher_logits, ce=1.0, kd=1.0, temperature=4.0, *, weight=None, ignore_index=-100,
                      distill_ignored=False):
    """Functional form of DistillationLoss (same kernels)."""
    ce, kd, tau, t2 = _check_kd_options(ce, kd, temperature, weight)
    return _Distillation.apply(logits, target, teacher_logits, weight, (ce, kd, tau, t2, bool(distill_ignored), ignore_index, 1.0))


def last_ce_status():
    """(valid pixels, out-of-range targets) of the most recent cross-entropy forward — one device->host copy; raises
    IndexError like torch's `Target out of bounds` when the second number is not zero."""
    st = getattr(_CrossEntropy, "last_status", None)
    if st is None:
        raise RuntimeError("no cross-entropy forward has run yet")
    _, valid, bad = st.cpu().tolist()[:3]
    if bad:
        raise IndexError(f"Target out of bounds: {int(bad)} pixels have a class index outside [0, C) that is not ignore_index")
    return int(valid), int(bad)
