"""The exact Euclidean distance transform on the GPU (cvk.squared_distance_maps / cvk.signed_distance_maps) against the scipy
restatement of tests/edt_ref.py: the integer maps with torch.equal, phi bit by bit.  Every image's reference is computed alone, so
nothing can leak across a batch.  Shapes: one pixel; smaller than a tile; rows of 65 and 131 and columns of 65 and 67 (not multiples of
anything); 2x517 and 517x2 (rows and columns longer than a 256-pixel tile, rows that are not 16-byte aligned)."""
import numpy as np
import pytest
import torch

from tests import edt_ref as R
from tests.boundary_ref import blocky_maps
from tests.test_gpu_ce_options import dev

pytestmark = pytest.mark.gpu

K, IGN = 12, 11
SHAPES = [(1, 1), (5, 7), (33, 65), (65, 33), (37, 70), (67, 131), (2, 517), (517, 2)]
_cache = {}


def _reference(key, labels, C=K, ign=IGN):
    """(to_class, to_other, phi) of tests/edt_ref.py for the int64 numpy batch, computed once per key and left unchanged."""
    if key not in _cache:
        _cache[key] = tuple(torch.from_numpy(a) for a in R.batch_maps(labels, C, ign))
    return _cache[key]


def _blocky(H, W):
    return blocky_maps(1000 * H + W, 3, H, W, cell=(3, 4), void=0.05)[1]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(labels, key, C=K, ign=IGN):
    import pytorch_camvid_amd as A
    want_c, want_o, want_phi = _reference(key, labels, C, ign)
    lab = torch.from_numpy(labels).to(dev())
    to_class, to_other = A.squared_distance_maps(lab, C, ign)
    phi = A.signed_distance_maps(lab, C, ign)
    N, H, W = labels.shape
    assert to_class.dtype == torch.int32 and tuple(to_class.shape) == (N, H, W, C) and to_class.is_contiguous()
    assert to_other.dtype == torch.int32 and tuple(to_other.shape) == (N, H, W)
    assert phi.dtype == torch.float32 and tuple(phi.shape) == (N, C, H, W) and phi.permute(0, 2, 3, 1).is_contiguous()
    to_class, to_other, phi = to_class.cpu(), to_other.cpu(), phi.cpu()
    bad_c, bad_o = int((to_class != want_c).sum()), int((to_other != want_o).sum())
    bad_p = int((_bits(phi.abs()) != _bits(want_phi.abs())).sum()) + int((torch.sign(phi) != torch.sign(want_phi)).sum())
    print(f"{key}: {N}x{H}x{W}, largest squared distance {int(want_c.max())}, absent (image, class) pairs "
          f"{int((want_c.reshape(N, -1, C).max(dim=1).values < 0).sum())}; differing to_class {bad_c}, to_other {bad_o}, phi {bad_p}")
    assert torch.equal(to_class, want_c) and torch.equal(to_other, want_o)
    assert bad_p == 0 and torch.equal(phi, want_phi)
    return to_class, to_other, phi


@pytest.mark.parametrize("H,W", SHAPES)
def test_blocky_maps_are_exact(H, W):
    labels = _blocky(H, W)
    to_class, to_other, phi = _check(labels, f"blocky {H}x{W}")
    if H * W > 1:
        assert (to_class > 0).any() and (to_other > 0).any() and (phi < 0).any() and (phi > 0).any()


def test_special_maps_at_67x131():
    H, W = 67, 131
    sp = R.special_maps(H, W, K, IGN)
    # one batch: nothing may leak between an image of one class, an all-void image and the others
    names = ["one_class", "corner_pixel", "all_void", "checkerboard", "void_stripe", "out_of_range"]
    labels = np.stack([sp[n] for n in names])
    to_class, to_other, phi = _check(labels, "special 67x131")
    i = {n: k for k, n in enumerate(names)}
    assert (to_other[i["one_class"]] == -1).all() and (to_class[i["one_class"], :, :, 3] == 0).all() and not phi[i["one_class"]].any()
    assert (to_class[i["all_void"]] == -1).all() and (to_other[i["all_void"]] == -1).all() and not phi[i["all_void"]].any()
    # the single pixel in the corner: the longest search and the largest value
    assert to_class[i["corner_pixel"], 0, 0, 5].item() == (H - 1) ** 2 + (W - 1) ** 2
    assert to_other[i["corner_pixel"], H - 1, W - 1].item() == 1 and to_other[i["corner_pixel"], 0, 0].item() == (H - 1) ** 2 + (W - 1) ** 2
    assert (to_other[i["checkerboard"]] == 1).all()
    # the void stripe: class 2 on both sides, its pixels next to the stripe are at distance 1 from "another label"
    assert (to_other[i["void_stripe"], :, W // 2] == 1).all() and (to_other[i["void_stripe"], :, 0] == (W // 2) ** 2).all()
    # out-of-range labels are void: present nowhere as a class, but they bound their neighbours
    assert to_other[i["out_of_range"], 0, 1].item() == 1 and (to_class[i["out_of_range"], :, :, 2:] == -1).all()


def test_class_absent_from_the_first_image_only():
    labels = np.zeros((2, 33, 65), dtype=np.int64)
    labels[:, :, 40:] = 1
    labels[1, 10:14, 3:9] = 7
    to_class, _, phi = _check(labels, "absent in image 0")
    assert (to_class[0, :, :, 7] == -1).all() and not phi[0, 7].any()
    assert (to_class[1, :, :, 7] >= 0).all() and to_class[1, 10, 3, 7].item() == 0 and phi[1, 7, 11, 4].item() == 0.0 - (2.0 - 1.0)


def test_other_class_counts_and_ignore_index():
    """32 classes with ignore_index -100, and one class: the channel count and the void rule are arguments, not constants."""
    lab32 = blocky_maps(77, 3, 37, 70, K=32, ignore=-100, cell=(3, 4), void=0.05)[1]
    _check(lab32, "32 classes", C=32, ign=-100)
    lab1 = (np.random.default_rng(3).random((3, 37, 70)) < 0.3).astype(np.int64)           # class 0 and "class 1", which is void at C = 1
    _check(lab1, "1 class", C=1, ign=-100)


def test_a_size_above_the_limit_is_refused_without_a_launch():
    import pytorch_camvid_amd as A
    lab = torch.zeros((1, 1, 4097), dtype=torch.int64, device=dev())                        # (W - 1)^2 = 2^24
    for f in (A.squared_distance_maps, A.signed_distance_maps):
        with pytest.raises(ValueError, match=r"\(W - 1\)\^2 < 2\^24"):
            f(lab)
    at_limit = torch.zeros((1, 1, 4096), dtype=torch.int64, device=dev())
    at_limit[0, 0, 0] = 1
    to_class, to_other = A.squared_distance_maps(at_limit)
    assert to_class[0, 0, 4095, 1].item() == 4095 ** 2 and to_other[0, 0, 0].item() == 1
    assert A.signed_distance_maps(at_limit)[0, 1, 0, 4095].item() == 4095.0


def test_a_second_call_gives_the_same_bits():
    import pytorch_camvid_amd as A
    lab = torch.from_numpy(_blocky(67, 131)).to(dev())
    a = A.squared_distance_maps(lab) + (A.signed_distance_maps(lab),)
    other = torch.from_numpy(_blocky(37, 70)).to(dev())
    A.signed_distance_maps(other)                                                           # another shape in between
    b = A.squared_distance_maps(lab) + (A.signed_distance_maps(lab),)
    for u, v in zip(a, b):
        assert u.data_ptr() != v.data_ptr() and torch.equal(_bits(u), _bits(v))
