"""The local-window CRF without a GPU: the sliced numpy restatement (tests/crf_ref.py) against a loop over pixels and offsets and on
the cases whose answer is known, the coefficients' rounding, the C entry points' argument checks (no launch), the Python refusals
and the place of a LocalCRF in evaluate / evaluate_report / predict."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import crf_ref as R


def coeffs(radius=2, dilation=1, appearance=(4.0, 8.0, 13.0), smoothness=(3.0, 3.0)):
    import pytorch_camvid_amd as A
    return A.crf_coefficients(radius, dilation, appearance, smoothness)


def case(N, H, W, C, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    U = (scale * rng.standard_normal((N, H, W, C))).astype(np.float32)
    I = R.blocky_frames(N, H, W, seed + 1, cell=(3, 2)).astype(np.float64)
    return U, I


@pytest.mark.parametrize("radius,dilation,compat", [(1, 1, False), (2, 1, False), (2, 2, True), (1, 3, False)])
def test_restatement_equals_a_loop_over_pixels_and_offsets(radius, dilation, compat):
    U, I = case(2, 5, 6, 3, 11)
    ga, gs, cb, wa, ws = coeffs(radius, dilation)
    mu = np.random.default_rng(3).standard_normal((3, 3)).astype(np.float32) if compat else None
    a = R.crf_reference(U, I, ga, gs, cb, wa, ws, radius, dilation, 3, compat=mu)
    b = R.crf_brute(U, I, ga, gs, cb, wa, ws, radius, dilation, 3, compat=mu)
    assert np.abs(a - b).max() < 1e-13
    assert np.abs(a.sum(-1) - 1).max() < 1e-14
    assert np.abs(a - R.softmax(U, np.float64)).max() > 1e-3, "the refinement did nothing: the comparison would be vacuous"


def test_one_pixel_and_zero_weights_give_the_softmax():
    ga, gs, cb, wa, ws = coeffs(3, 1)
    U, I = case(1, 1, 1, 4, 2)
    assert np.array_equal(R.crf_reference(U, I, ga, gs, cb, wa, ws, 3, 1, 4), R.softmax(U, np.float64))
    U, I = case(1, 6, 7, 4, 3)
    q = R.crf_reference(U, I, ga, gs, cb, 0.0, 0.0, 3, 1, 4)
    assert np.array_equal(q, R.softmax(U, np.float64))
    assert np.array_equal(q, R.crf_reference(U, I[:, ::-1].copy(), ga, gs, cb, 0.0, 0.0, 3, 1, 4))
    # a probability unary with exact zeros: log(max(p, FLT_MIN)) keeps everything finite, and softmax(log p) is p again
    P = R.softmax(U, np.float64).astype(np.float32)
    P[..., 0] = 0.0
    P /= P.sum(-1, keepdims=True)
    q = R.crf_reference(P, I, ga, gs, cb, 0.0, 0.0, 3, 1, 2, unary_is_prob=True)
    assert np.isfinite(q).all() and np.abs(q - P).max() < 1e-7


def test_on_a_constant_image_appearance_is_smoothness_with_theta_alpha():
    U, _ = case(1, 8, 9, 3, 5)
    I = np.full((1, 8, 9, 3), 77.0)
    ga, gs, cb, _, _ = coeffs(2, 2, (4.0, 2.5, 13.0), (3.0, 2.5))
    assert np.array_equal(ga, gs)
    Q = R.softmax(U, np.float64)
    ma, ms = R.messages(Q, I, ga, gs, cb, 2, 2, np.float64)
    assert np.abs(ma - ms).max() < 1e-15
    ga2, gs2, _, _, _ = coeffs(2, 2, (4.0, 2.5, 13.0), (3.0, 1.0))
    ma2, ms2 = R.messages(Q, I, ga2, gs2, cb, 2, 2, np.float64)
    assert np.abs(ma2 - ma).max() < 1e-15 and np.abs(ms2 - ms).max() > 1e-4


def test_the_potts_matrix_is_the_default():
    U, I = case(1, 6, 7, 4, 8)
    ga, gs, cb, wa, ws = coeffs(2, 1)
    a = R.crf_reference(U, I, ga, gs, cb, wa, ws, 2, 1, 3)
    b = R.crf_reference(U, I, ga, gs, cb, wa, ws, 2, 1, 3, compat=-np.eye(4, dtype=np.float32))
    assert np.abs(a - b).max() < 1e-15


def test_fp32_restatement_is_near_the_fp64_one():
    U, I = case(1, 12, 13, 5, 4)
    ga, gs, cb, wa, ws = coeffs(2, 1)
    a = R.crf_reference(U, I, ga, gs, cb, wa, ws, 2, 1, 5)
    b = R.crf_reference(U, I, ga, gs, cb, wa, ws, 2, 1, 5, dtype=np.float32)
    assert b.dtype == np.float32 and 0 < np.abs(a - b).max() < 5e-6


def test_coefficients_are_rounded_once_from_double():
    import pytorch_camvid_amd as A
    ga, gs, cb, wa, ws = A.crf_coefficients(3, 2, (4.1, 8.0, 13.0), (3.3, 3.0))
    assert ga.dtype == np.float32 and gs.dtype == np.float32 and ga.shape == gs.shape == (7, 7)
    for i in range(-3, 4):
        for j in range(-3, 4):
            o2 = 4.0 * (i * i + j * j)
            assert ga[i + 3, j + 3] == np.float32(np.exp(-o2 / (2.0 * 64.0)))
            assert gs[i + 3, j + 3] == np.float32(np.exp(-o2 / (2.0 * 9.0)))
    assert cb == float(np.float32(-1.0 / (2.0 * 169.0))) and wa == float(np.float32(4.1)) and ws == float(np.float32(3.3))
    assert ga[3, 3] == 1.0
    for bad in (dict(radius=0), dict(radius=6), dict(dilation=0), dict(dilation=5), dict(radius=True), dict(appearance=(4.0, 0.0, 13.0)),
                dict(appearance=(-1.0, 8.0, 13.0)), dict(appearance=(4.0, 8.0)), dict(smoothness=(3.0, float("inf"))),
                dict(smoothness="ab")):
        with pytest.raises(ValueError):
            A.crf_coefficients(**bad)


def step(lib, C=12, r=3, d=1, ld=None, first=1, last=1, pred=16, q_in=32, q_out=48, unary=64, cb=-0.003, wa=4.0, ws=3.0):
    tab = (ctypes.c_float * 121)()
    ab = (ctypes.c_float * 3)()
    return lib.cvk_crf_step(unary, C if ld is None else ld, 0, q_in, q_out, pred, 80, 0, 0, 0, 0, 0, ab, ab, tab, tab, cb, wa, ws, None,
                            1, 8, 8, C, r, d, first, last, None)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    from pytorch_camvid_amd import _lib
    lib = _lib.load()
    EINVAL = -1
    for kw in (dict(C=0), dict(C=33), dict(r=0), dict(r=6), dict(d=0), dict(d=5), dict(C=12, ld=11), dict(last=1, pred=None),
               dict(first=0, q_in=48), dict(first=1, q_in=48), dict(q_in=None), dict(unary=None), dict(cb=0.5), dict(wa=-1.0),
               dict(ws=float("nan"))):
        assert step(lib, **kw) == EINVAL, kw
        assert lib.cvk_last_error_string().startswith(b"cvk_crf_step"), kw
    th, tw, st = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    for C, r, d in ((0, 3, 1), (33, 3, 1), (12, 0, 1), (12, 6, 1), (12, 3, 0), (12, 3, 5)):
        assert lib.cvk_crf_tile(C, r, d, ctypes.byref(th), ctypes.byref(tw), ctypes.byref(st)) == EINVAL


def test_tile_query_names_both_paths():
    import pytorch_camvid_amd as A
    th, tw, staged = A.crf_tile(12, 3, 1)
    assert th >= 1 and tw >= 1 and staged is True
    assert A.crf_tile(12, 5, 4)[2] is False, "r d = 20 fits no tile"
    for C in (1, 2, 3, 12, 16):
        for r, d in ((1, 1), (3, 1), (3, 2), (5, 1)):
            assert A.crf_tile(C, r, d)[2] is True, (C, r, d)
    assert A.crf_tile(32, 3, 1)[2] is True and A.crf_tile(32, 3, 2)[2] is False      # 32 classes: the halo of 6 no longer fits
    with pytest.raises(ValueError):
        A.crf_tile(33)


def test_constructor_refusals():
    import pytorch_camvid_amd as A
    A.LocalCRF()
    A.LocalCRF(iterations=1, radius=5, dilation=4, inner=A.SlidingWindow(), compat=torch.zeros(3, 3))
    A.LocalCRF(inner=A.TestTimeAugmentation())
    for bad in (dict(iterations=0), dict(iterations=2.0), dict(iterations=True), dict(radius=6), dict(dilation=0),
                dict(appearance=(4.0, 8.0, -1.0)), dict(smoothness=(3.0,)), dict(compat=torch.zeros(3, 4)),
                dict(compat=torch.zeros(3, 3, dtype=torch.float64)), dict(compat=[[0.0]]), dict(mean=(0.4, 0.4)),
                dict(std=(0.3, 0.0, 0.3)), dict(inner=object()), dict(inner="window")):
        with pytest.raises(ValueError):
            A.LocalCRF(**bad)
    crf = A.LocalCRF()
    with pytest.raises(ValueError):
        crf.refine(torch.zeros(1, 3, 4, 4, dtype=torch.float64), torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crf.refine(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4))


def test_pinned_signatures_and_all_are_unchanged_and_a_crf_passes_as_tta():
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd import functional as F
    from tests.test_loss_surface_cpu import PACKAGE_ALL
    assert str(inspect.signature(A.evaluate)) == "(net, batches, num_classes=12, ignore_index=11, window=None, tta=None)"
    assert str(inspect.signature(A.evaluate_report)) == ("(net, batches, num_classes=12, ignore_index=11, loss_fn=None, window=None, "
                                                         "boundary=None, tta=None)")
    assert list(inspect.signature(A.predict).parameters) == ["net", "image_u8", "out_size", "mean", "std", "window", "tta"]
    assert A.__all__ == PACKAGE_ALL
    for name in ("LocalCRF", "crf_refine", "crf_coefficients", "crf_tile"):
        assert hasattr(A, name) and name not in A.__all__
    crf = A.LocalCRF()
    F._check_tta_window("evaluate", crf, None)
    with pytest.raises(ValueError, match="not both"):
        F._check_tta_window("evaluate", crf, A.SlidingWindow())
    assert crf.loss_view(360, 480) == 0
    tta = A.TestTimeAugmentation(scales=(0.5, 1.0), flip=True)
    assert A.LocalCRF(inner=tta).loss_view(360, 480) == tta.loss_view(360, 480) == 2
    assert A.LocalCRF(inner=A.TestTimeAugmentation(scales=(0.5,))).loss_view(360, 480) is None
