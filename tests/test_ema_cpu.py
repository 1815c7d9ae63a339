"""The weight EMA of FlatAdamW, the parts that need no GPU: the per-update weight `ema_alpha`, the option check of the constructor and the
argument checks of the two range-step entry points with an EMA buffer (refused on the host, before any launch)."""
import numpy as np
import pytest


def test_ema_alpha_values():
    """alpha_k = float32(1 - d_k), d_k = decay or min(decay, (1 + k) / (10 + k)), evaluated in double precision and rounded once.

    The warm-up term reaches the decay 0.999 when 9 / (10 + k) <= 0.001, that is from k = 8990 on: 9 / 9000 is exactly 0.001 and
    8991 / 9000 divides to the double 0.999 itself.  (The feature request quotes 8981 for this point; at k = 8981 its own formula gives
    1 - 8982 / 8991 = 0.001001..., so the formula is kept and the point is the one that follows from it.)  The test pins the switch at
    both sides: strictly above float32(0.001) up to k = 8989, equal to it from k = 8990 on."""
    from pytorch_camvid_amd.optim import ema_alpha
    for decay in (0.0, 0.5, 0.9, 0.999, 0.9999):
        want = np.float32(1.0 - decay)
        for k in (1, 2, 17, 10 ** 6):
            got = ema_alpha(decay, False, k)
            assert isinstance(got, np.float32) and got.tobytes() == want.tobytes(), (decay, k, got, want)
    first = ema_alpha(0.999, True, 1)
    assert isinstance(first, np.float32) and first.tobytes() == np.float32(1.0 - 2.0 / 11.0).tobytes()
    alphas = np.array([ema_alpha(0.999, True, k) for k in range(1, 12001)], np.float32)
    assert np.all(alphas[1:] <= alphas[:-1])                             # monotone non-increasing in k
    floor = np.float32(0.001)
    assert floor.tobytes() == np.float32(1.0 - 0.999).tobytes()
    assert np.all(alphas[8990 - 1:] == floor) and np.all(alphas[:8990 - 1] > floor)
    for k in (1, 5, 100, 8989):                                          # the double-precision expression, rounded once
        assert alphas[k - 1].tobytes() == np.float32(1.0 - (1.0 + k) / (10.0 + k)).tobytes(), k
    # a small decay is never raised by the warm-up
    assert ema_alpha(0.1, True, 1).tobytes() == np.float32(0.9).tobytes()


def test_ema_decay_is_checked_before_the_device():
    import pytorch_camvid_amd as A
    net = A.UNet(3, 12)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            A.FlatAdamW(net, ema_decay=bad)
    with pytest.raises(RuntimeError, match="GPU"):                       # valid options: the next check is the device
        A.FlatAdamW(A.UNet(3, 12), ema_decay=0.0, ema_warmup=True)
    with pytest.raises(RuntimeError, match="GPU"):
        A.FlatAdamW(A.UNet(3, 12), ema_decay=0.999)


def _refused(lib, rc, name, word):
    msg = lib.cvk_last_error_string().decode()
    assert rc == -1 and msg.startswith(name + ":") and word in msg, (name, rc, msg)


def test_ema_entry_points_refuse_bad_arguments_before_any_launch():
    from pytorch_camvid_amd import _lib as L
    lib = L.load()
    p = 4096                                                  # never dereferenced: every call is refused on the host
    eager, captured = "cvk_adamw_step_ranges", "cvk_adamw_step_ranges_dev"
    # null pointers.  A null ema buffer itself is the step without an average (as a null clip record is the unclipped step), so it is not
    # refused; every other buffer still is, with and without an average, and so is an average whose device alpha is null
    _refused(lib, lib.cvk_adamw_step_ranges(p, p, p, None, None, 8, p, 1, 1, p, 1, None, 0.1, None), eager, "null")
    _refused(lib, lib.cvk_adamw_step_ranges(p, None, p, p, p, 8, p, 1, 1, p, 1, p, 0.1, None), eager, "null")
    _refused(lib, lib.cvk_adamw_step_ranges_dev(p, p, p, None, None, 8, p, 1, 1, p, 1, None, p, 0.1, None), captured, "null")
    _refused(lib, lib.cvk_adamw_step_ranges_dev(p, p, p, p, p, 8, p, 1, 1, p, 1, p, None, 0.1, None), captured, "null")
    # alpha outside (0, 1], with and without a clip record
    for alpha in (0.0, 1.5, -0.25, float("nan")):
        for rec in (None, p):
            _refused(lib, lib.cvk_adamw_step_ranges(p, p, p, p, p, 8, p, 1, 1, p, 1, rec, alpha, None), eager, "alpha")
            _refused(lib, lib.cvk_adamw_step_ranges_dev(p, p, p, p, p, 8, p, 1, 1, p, 1, rec, p, alpha, None), captured, "alpha")
    # the record limit of the kernel-argument form; an empty table in both
    _refused(lib, lib.cvk_adamw_step_ranges(p, p, p, p, p, 8, p, 1, 1, p, L.ADAMW_ARG_RECORDS + 1, None, 0.1, None), eager, "records")
    assert L.ADAMW_ARG_RECORDS + 1 == 17
    _refused(lib, lib.cvk_adamw_step_ranges(p, p, p, p, p, 8, p, 0, 0, p, 1, None, 0.1, None), eager, "bad arguments")
    _refused(lib, lib.cvk_adamw_step_ranges_dev(p, p, p, p, p, 8, p, 0, 0, p, 1, None, p, 0.1, None), captured, "bad arguments")
