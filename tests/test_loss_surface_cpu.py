"""The public surface of the losses after their move from functional.py to losses.py: every loss name and loss constant
`pytorch_camvid_amd.functional` exposed before the move is still there and is the object losses.py defines, the package's `__all__` is
the list it was, the five record-bearing modules refuse `last_record` before a forward, and the six option checkers refuse a weight
that is not 1-D.  No compute calls (no GPU here)."""
import pytest
import torch

import pytorch_camvid_amd as A
from pytorch_camvid_amd import functional, losses

# what functional.py exposed of the losses before the move (its public names, and the two helpers tools and tests import from it)
LOSS_NAMES = [
    "_as_nhwc", "_stream",
    "REDUCTIONS", "CrossEntropyLoss", "cross_entropy",
    "DICE_AVERAGES", "SEG_RECORD_HEAD", "SegmentationLoss", "FocalLoss", "DiceLoss", "segmentation_loss",
    "OHEM_RECORD", "ohem_loss_threshold", "OhemCrossEntropyLoss", "ohem_cross_entropy",
    "LOVASZ_CLASSES", "LOVASZ_RECORD_HEAD", "LOVASZ_CLASS_SLOTS", "LOVASZ_SORT_TILE", "LovaszSoftmaxLoss", "lovasz_softmax",
    "BDL_RECORD_HEAD", "EDT_MAX_CLASSES", "squared_distance_maps", "signed_distance_maps", "BoundaryLoss", "boundary_loss",
    "KD_RECORD", "distillation_scales", "DistillationLoss", "distillation_loss",
    "last_ce_status",
]

PACKAGE_ALL = [
    "UNet", "SegNet", "BasicConv2d", "BasicConv", "UpSample2d", "get_model", "set_conv_precision", "set_split_operands", "CrossEntropyLoss",
    "SegmentationLoss", "FocalLoss", "DiceLoss", "segmentation_loss", "OhemCrossEntropyLoss", "ohem_cross_entropy", "ohem_loss_threshold",
    "LovaszSoftmaxLoss", "lovasz_softmax", "BoundaryLoss", "boundary_loss", "squared_distance_maps", "signed_distance_maps",
    "DistillationLoss", "distillation_loss", "distillation_scales", "cross_entropy", "last_ce_status", "argmax_channels", "ConfusionMeter",
    "BoundaryMeter", "label_boundaries", "boundary_tolerance", "boundary_scores", "SurfaceDistanceMeter", "surface_distances",
    "surface_distance_scores", "surface_percentile", "ClassFrequencyMeter", "class_weights", "weights_from_counts", "evaluate",
    "evaluate_report", "predict", "TestTimeAugmentation", "SlidingWindow", "preprocess_uint8", "DevicePrefetcher", "transforms",
    "FlatAdamW", "FlatSGD", "clip_grad_norm_", "ema_alpha", "GradAccumulator", "ddp", "GraphedStep", "mark_weights_dirty",
    "save_checkpoint", "load_checkpoint", "latest_checkpoint", "checkpoint_epoch", "resume", "save_policy", "reference_state_dict",
    "build_library", "load_library", "CvkError",
]


@pytest.mark.parametrize("name", LOSS_NAMES)
def test_functional_still_exposes_the_loss_name(name):
    assert getattr(functional, name) is getattr(losses, name)


def test_package_all_is_unchanged():
    assert A.__all__ == PACKAGE_ALL
    for name in PACKAGE_ALL:
        assert hasattr(A, name), name
    for name in LOSS_NAMES:
        if name in PACKAGE_ALL:
            assert getattr(A, name) is getattr(losses, name), name


@pytest.mark.parametrize("make", [
    lambda: A.SegmentationLoss(1, .5),
    lambda: A.OhemCrossEntropyLoss(0.7, 4),
    lambda: A.LovaszSoftmaxLoss(1, .5),
    lambda: A.BoundaryLoss(1, .5),
    lambda: A.DistillationLoss(1, 1),
], ids=["seg", "ohem", "lovasz", "boundary", "distill"])
def test_last_record_before_a_forward(make):
    with pytest.raises(RuntimeError, match="^no forward has run yet$"):
        make().last_record


@pytest.mark.parametrize("checker", [
    lambda w: losses._check_ce_options(w, "mean", 0.0),
    lambda w: losses._check_seg_options(1.0, 0.5, 0.0, w, 1.0, "present"),
    lambda w: losses._check_ohem_options(0.7, 4, w),
    lambda w: losses._check_lovasz_options(1.0, 0.5, "present", False, w),
    lambda w: losses._check_boundary_loss_options(1.0, 0.5, None, w),
    lambda w: losses._check_kd_options(1.0, 1.0, 4.0, w),
], ids=["ce", "seg", "ohem", "lovasz", "boundary", "kd"])
def test_option_checkers_refuse_a_weight_that_is_not_1d(checker):
    checker(torch.ones(3))
    with pytest.raises(ValueError, match="1-D"):
        checker(torch.ones(2, 3))
