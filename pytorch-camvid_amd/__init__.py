"""pytorch_camvid_amd — MI355X-native (gfx950) execution of the pytorch-camvid UNet/SegNet training hot path.

Import name: `pytorch_camvid_amd` (the directory is `pytorch-camvid_amd/`; `pytorch_camvid_amd.py` at the repository
root aliases it).  Public surface mirrors the reference (models/unet.py, models/segnet.py, utils.get_model,
train.py's loss): UNet, SegNet, BasicConv2d, BasicConv, UpSample2d, get_model, CrossEntropyLoss.
"""
from ._lib import CvkError, build as build_library, load as load_library          # noqa: F401
from .modules import BasicConv, BasicConv2d, SegNet, UNet, UpSample2d, get_model, set_conv_precision, set_split_operands   # noqa: F401
from .losses import (CrossEntropyLoss, cross_entropy, last_ce_status, SegmentationLoss, FocalLoss,  # noqa: F401
                     DiceLoss, segmentation_loss, OhemCrossEntropyLoss, ohem_cross_entropy, ohem_loss_threshold,
                     LovaszSoftmaxLoss, lovasz_softmax,
                     BoundaryLoss, boundary_loss, squared_distance_maps, signed_distance_maps,
                     DistillationLoss, distillation_loss, distillation_scales)
from .inference import (argmax_channels, preprocess_uint8, DevicePrefetcher, TestTimeAugmentation, SlidingWindow,  # noqa: F401
                        LocalCRF, crf_refine, crf_coefficients, crf_tile)
from .meters import (ConfusionMeter, ClassFrequencyMeter, class_weights, weights_from_counts, BoundaryMeter, label_boundaries,  # noqa: F401
                     boundary_tolerance, boundary_scores, SurfaceDistanceMeter, surface_distances, surface_distance_scores,
                     surface_percentile, BoundaryIoUMeter, chessboard_depth, boundary_dilation, boundary_iou_scores,
                     trimap_scores, connected_components, remove_small_regions, RegionFilter, RegionMeter, region_scores,
                     CalibrationMeter, TemperatureScaler, calibration_scores, confidence_map)
from .functional import evaluate, evaluate_report, predict  # noqa: F401
from .optim import FlatAdamW, FlatSGD, clip_grad_norm_, ema_alpha  # noqa: F401
from .accumulate import GradAccumulator  # noqa: F401
from . import ddp  # noqa: F401
from . import transforms  # noqa: F401
from .graph import GraphedStep  # noqa: F401
from .engine import mark_weights_dirty  # noqa: F401
from .checkpoint import (save_checkpoint, load_checkpoint, latest_checkpoint, checkpoint_epoch, resume,   # noqa: F401
                         save_policy, reference_state_dict)

__all__ = ["UNet", "SegNet", "BasicConv2d", "BasicConv", "UpSample2d", "get_model", "set_conv_precision", "set_split_operands", "CrossEntropyLoss",
           "SegmentationLoss", "FocalLoss", "DiceLoss", "segmentation_loss", "OhemCrossEntropyLoss", "ohem_cross_entropy", "ohem_loss_threshold", "LovaszSoftmaxLoss", "lovasz_softmax", "BoundaryLoss", "boundary_loss", "squared_distance_maps", "signed_distance_maps", "DistillationLoss", "distillation_loss", "distillation_scales", "cross_entropy", "last_ce_status", "argmax_channels", "ConfusionMeter", "BoundaryMeter", "label_boundaries", "boundary_tolerance", "boundary_scores", "SurfaceDistanceMeter", "surface_distances", "surface_distance_scores", "surface_percentile", "ClassFrequencyMeter", "class_weights", "weights_from_counts", "evaluate", "evaluate_report", "predict", "TestTimeAugmentation", "SlidingWindow", "preprocess_uint8", "DevicePrefetcher", "transforms", "FlatAdamW", "FlatSGD", "clip_grad_norm_", "ema_alpha", "GradAccumulator", "ddp", "GraphedStep", "mark_weights_dirty", "save_checkpoint", "load_checkpoint", "latest_checkpoint", "checkpoint_epoch", "resume", "save_policy",
           "reference_state_dict", "build_library", "load_library", "CvkError"]
