"""The public surface of the meters and the inference drivers after their move from functional.py to meters.py and inference.py: every
public name and upper-case constant `pytorch_camvid_amd.functional` exposed before the move (outside the loss names, which
tests/test_loss_surface_cpu.py pins) is still there and is the object its home module defines, the package resolves its `__all__` to
the same objects, imports run losses <- inference <- meters <- functional only, the meters evaluate_report takes say what they are fed
and what they report, and the evaluation loop gives the network its `training` flag back when a batch raises.  No GPU call and no
library call."""
import ast
import os

import pytest
import torch

import pytorch_camvid_amd as A
from pytorch_camvid_amd import functional, inference, losses, meters

# dir(functional) before the move, without the loss names: by home module
METER_NAMES = [
    "BIOU_ROWS", "BOUNDARY_MAX_RADIUS2", "BoundaryIoUMeter", "BoundaryMeter", "CALIBRATION_REPORT_KEYS", "CALIB_LOG_COLUMNS",
    "CALIB_MAX_BINS", "CALIB_MAX_CELLS", "CALIB_MAX_CLASSES", "CALIB_Q_SCALE", "CALIB_TAU_BRACKET", "CC_MODES", "CC_RECORD_SLOTS",
    "CHEB_MAX_DEPTH", "CHEB_MAX_WIDTHS", "CalibrationMeter", "ClassFrequencyMeter", "ConfusionMeter", "RegionFilter", "RegionMeter",
    "SURFACE_MAX_DENOMINATOR", "SURFACE_RECORD_SLOTS", "SurfaceDistanceMeter", "TemperatureScaler", "WEIGHT_METHODS",
    "boundary_dilation", "boundary_iou_scores", "boundary_scores", "boundary_tolerance", "calibration_scores", "chessboard_depth",
    "class_weights", "confidence_map", "connected_components", "label_boundaries", "region_scores", "remove_small_regions",
    "surface_distance_scores", "surface_distances", "surface_percentile", "trimap_scores", "weights_from_counts",
]
INFERENCE_NAMES = [
    "CAMVID_MEAN", "CAMVID_STD", "CRF_MAX_DILATION", "CRF_MAX_RADIUS", "DevicePrefetcher", "LocalCRF", "SlidingWindow",
    "TestTimeAugmentation", "argmax_channels", "crf_coefficients", "crf_refine", "crf_tile", "preprocess_uint8",
]
FUNCTIONAL_NAMES = ["SURFACE_REPORT_KEYS", "_check_tta_window", "evaluate", "evaluate_report", "predict"]       # these stayed
HOMES = ([(n, meters) for n in METER_NAMES] + [(n, inference) for n in INFERENCE_NAMES] + [(n, functional) for n in FUNCTIONAL_NAMES])


def test_the_list_is_the_sixty_names():
    assert len(HOMES) == 60 and len({n for n, _ in HOMES}) == 60


@pytest.mark.parametrize("name,home", HOMES, ids=[n for n, _ in HOMES])
def test_functional_still_exposes_the_name(name, home):
    obj = getattr(home, name)
    assert getattr(functional, name) is obj
    if hasattr(obj, "__module__"):                          # a class or a function: defined there, not passed through
        assert obj.__module__ == home.__name__


def test_the_private_check_a_test_imports_from_functional_is_still_there():
    assert functional._check_calib_shapes is meters._check_calib_shapes         # tests/test_calibration_cpu.py


def test_the_report_keys_of_the_surface_meter_are_the_old_constant():
    assert functional.SURFACE_REPORT_KEYS == ("hd95", "hd", "assd", "hd95_per_class", "hd_per_class", "assd_per_class")
    assert functional.CALIBRATION_REPORT_KEYS == ("ece", "mce", "nll", "brier")


def test_package_names_are_their_home_modules_objects():
    home = dict(HOMES)
    for name in A.__all__:
        assert hasattr(A, name), name
        if name in home:
            assert getattr(A, name) is getattr(home[name], name), name
    assert sum(name in home for name in A.__all__) == 20
    for name in ("BoundaryIoUMeter", "RegionMeter", "CalibrationMeter", "LocalCRF", "TemperatureScaler"):       # exported, not in __all__
        assert getattr(A, name) is getattr(home[name], name), name


def _imports(module):
    """every module name an import statement of `module`'s file names, nested ones included: (level, "a.b", [names])"""
    with open(os.path.splitext(module.__file__)[0] + ".py") as f:
        tree = ast.parse(f.read())
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            out += [(0, a.name, []) for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            out.append((node.level, node.module or "", [a.name for a in node.names]))
    return out


@pytest.mark.parametrize("module,forbidden", [(inference, {"meters", "functional"}), (meters, {"functional"}),
                                              (losses, {"inference", "meters", "functional"})], ids=["inference", "meters", "losses"])
def test_import_direction(module, forbidden):
    found = _imports(module)
    assert found, "the walk saw no import at all"
    for level, mod, names in found:
        if level > 0 or "pytorch_camvid_amd" in mod:        # an import from this package: neither the path nor a name is a later module
            assert not (set(mod.split(".")) | set(names)) & forbidden, (module.__name__, level, mod, names)
    if module is meters:
        from_inference = [names for level, mod, names in found if level > 0 and mod == "inference"]
        assert from_inference == [["_check_window"]]


def test_meters_declare_what_they_take_and_report():
    made = {
        "BoundaryMeter": (A.BoundaryMeter(), "pred", ("bf", "bf_per_class")),
        "SurfaceDistanceMeter": (A.SurfaceDistanceMeter(), "pred", functional.SURFACE_REPORT_KEYS),
        "BoundaryIoUMeter": (A.BoundaryIoUMeter(), "pred", ("biou", "biou_per_class")),
        "RegionMeter": (A.RegionMeter(), "pred", ("fragmentation", "miou_filtered", "regions_pred")),
        "CalibrationMeter": (A.CalibrationMeter(device="cpu"), "logits", functional.CALIBRATION_REPORT_KEYS),
    }
    for name, (m, takes, keys) in made.items():
        assert functional._contour_meters(m) == [m], name
        assert m.update_takes == takes and type(m).update_takes == takes, name
        assert tuple(m.report_keys) == tuple(keys), name
    with_widths = A.BoundaryIoUMeter(trimap_widths=(1, 3))
    assert with_widths.report_keys == ("biou", "biou_per_class", "trimap_miou")
    assert "trimap_miou" not in A.BoundaryIoUMeter(trimap_widths=()).report_keys
    empty = with_widths.compute()                                   # a meter that saw nothing: the keys it reports exist
    assert all(k in empty for k in with_widths.report_keys)
    for m, _, _ in made.values():
        if m.update_takes == "pred":
            assert all(k in m.compute() for k in m.report_keys), type(m).__name__


class _Raises(torch.nn.Module):
    def forward(self, x):
        raise RuntimeError("this batch does not run")


@pytest.mark.parametrize("call", [
    lambda net, batches: A.evaluate(net, batches),
    lambda net, batches: A.evaluate_report(net, batches),
    lambda net, batches: A.evaluate_report(net, batches, boundary=(A.BoundaryMeter(), A.RegionMeter())),
], ids=["evaluate", "evaluate_report", "with_meters"])
@pytest.mark.parametrize("training", [True, False])
def test_the_loop_restores_training_when_a_batch_raises(call, training):
    net = _Raises().train(training)
    batches = [(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))]
    with pytest.raises(RuntimeError, match="this batch does not run"):
        call(net, batches)
    assert net.training is training
    with pytest.raises(ValueError, match="no batches"):
        call(net, [])
    assert net.training is training
