"""CPU-side checks of the captured training iteration (GraphedStep(optimizer=, scheduler=, log_capacity=)): the host fill of the AdamW
record against glibc's powf, argument validation of the three new entry points before any launch, the constructor's refusals, and
which parameters the per-iteration log reads.  No compute calls (no GPU here)."""
import ctypes
import ctypes.util

import numpy as np
import pytest
import torch

import pytorch_camvid_amd as A
from pytorch_camvid_amd import _lib
from pytorch_camvid_amd.graph import last_layer_params

P = 4096                              # a fake, 16-byte aligned device address: every call below is refused before a launch


def _err():
    return _lib.load().cvk_last_error_string()


def _libm():
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    for name, nargs in (("powf", 2), ("sqrtf", 1)):
        fn = getattr(m, name)
        fn.restype = ctypes.c_float
        fn.argtypes = [ctypes.c_float] * nargs
    return m


@pytest.mark.parametrize("beta1", [0.85, 0.9, 0.95])
def test_hyper_fill_bias_corrections_are_the_host_powf_expressions(beta1):
    """bc1 = 1.f - powf(beta1, (float)step), bc2_sqrt = sqrtf(1.f - powf(beta2, (float)step)): the expressions cvk_adamw_step evaluates,
    re-evaluated here through glibc in fp32, bit for bit, for steps 1..10000."""
    lib, m = _lib.load(), _libm()
    one = np.float32(1.0)
    b1, b2 = np.float32(beta1), np.float32(0.999)
    h = _lib.AdamwHyper()
    for step in range(1, 10001):
        assert lib.cvk_adamw_hyper_fill(2e-3, beta1, 0.999, 1e-8, 1e-2, step, ctypes.addressof(h)) == 0
        bc1 = one - np.float32(m.powf(b1, float(step)))
        bc2s = np.float32(m.sqrtf(one - np.float32(m.powf(b2, float(step)))))
        assert np.float32(h.bc1).tobytes() == bc1.tobytes(), step
        assert np.float32(h.bc2_sqrt).tobytes() == bc2s.tobytes(), step
    assert (h.lr, h.beta1, h.beta2, h.eps, h.weight_decay) == tuple(float(np.float32(v)) for v in (2e-3, beta1, 0.999, 1e-8, 1e-2))
    assert ctypes.sizeof(_lib.AdamwHyper) == 4 * 7


def test_new_entry_points_validate_arguments_without_gpu():
    lib = _lib.load()
    h = _lib.AdamwHyper()
    assert lib.cvk_adamw_hyper_fill(1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None) == -1
    assert b"cvk_adamw_hyper_fill" in _err()
    assert lib.cvk_adamw_hyper_fill(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, ctypes.addressof(h)) == -1        # step < 1
    assert lib.cvk_adamw_hyper_fill(1e-3, 0.9, 0.999, 1e-8, 0.0, -5, ctypes.addressof(h)) == -1

    step = lib.cvk_adamw_step_ranges_dev
    #           param grad m  v  ema   n    ranges nr nb hyper nh rec  alpha a_host stream
    good = [P, P, P, P, None, 100, P, 1, 1, P, 1, None, None, 0.0, None]
    for i in (0, 1, 2, 3, 6, 9):                                                                       # every pointer that may not be null
        args = list(good)
        args[i] = None
        assert step(*args) == -1
        assert b"null" in _err()
    for n in (0, -7):                                                                                  # n <= 0
        args = list(good)
        args[5] = n
        assert step(*args) == -1
        assert b"bad arguments" in _err()

    log = lib.cvk_step_log
    #      loss hyper gw nw gb nb  rec   ring cap counter stream
    good = [P, P, P, 12, P, 12, None, P, 8, P, None]
    for i in (0, 1, 2, 4, 7, 9):                                                                       # every pointer but the clip record
        args = list(good)
        args[i] = None
        assert log(*args) == -1
        assert b"null" in _err()
    for i, bad in ((8, 0), (8, -1), (3, 0), (3, -4), (5, 0), (5, -4)):                                # capacity, nw, nb
        args = list(good)
        args[i] = bad
        assert log(*args) == -1
        assert b"bad arguments" in _err()


def test_graphed_step_refuses_other_optimizers_and_bad_log_arguments():
    net = A.UNet(3, 12)
    lossf = A.CrossEntropyLoss()
    x, t = torch.zeros(1, 3, 32, 32), torch.zeros(1, 32, 32, dtype=torch.int64)
    with pytest.raises(TypeError, match="only FlatAdamW"):
        A.GraphedStep(net, lossf, x, t, optimizer=torch.optim.AdamW(net.parameters(), lr=1e-3))
    with pytest.raises(TypeError):
        A.GraphedStep(net, lossf, x, t, optimizer=torch.optim.SGD(net.parameters(), lr=1e-3))
    with pytest.raises(ValueError, match="needs optimizer="):
        A.GraphedStep(net, lossf, x, t, log_capacity=4)
    sched_opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="scheduler"):
        A.GraphedStep(net, lossf, x, t, scheduler=torch.optim.lr_scheduler.StepLR(sched_opt, 10))


def _reference_last_layer(net):
    """utils._get_lastlayer_params of the reference (utils.py:15-30), restated."""
    w = b = None
    for name, p in net.named_parameters():
        if "weight" in name:
            w = name
        if "bias" in name:
            b = name
    return w, b


@pytest.mark.parametrize("model,names", [("unet", ("output.conv.1.weight", "output.conv.1.bias")),
                                         ("segnet", ("decoder1.1.bn.weight", "decoder1.1.bn.bias"))])
def test_log_reads_the_reference_last_layer(model, names):
    """The reference logs the gradient norms of the LAST parameters named '*weight*' / '*bias*': for both networks that is the final
    block's BatchNorm affine pair (12 values each), not the classifier convolution."""
    from oracle import torch_ref as R
    net = A.get_model(model, 3, 12)
    (wn, w), (bn, b) = last_layer_params(net)
    assert (wn, bn) == names
    assert _reference_last_layer(R.build(model, 3, 12)) == names
    assert w is dict(net.named_parameters())[wn] and b is dict(net.named_parameters())[bn]
    assert w.numel() == 12 and b.numel() == 12
