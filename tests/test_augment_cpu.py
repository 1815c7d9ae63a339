"""CPU checks of the device transforms (pytorch_camvid_amd.transforms): the host-side sampler makes the reference's augmentation
decisions under a seed (tests/golden/aug_params.npz, recorded from the reference's transforms.py by make_aug_params.py), the
packed records hold the right taps and LUTs, cvk_augment_u8 validates its arguments, and unsupported pipelines are refused
when they are built."""
import ctypes
import math
import os
import random

import numpy as np
import pytest

from pytorch_camvid_amd import _lib
from pytorch_camvid_amd import transforms as T

MEAN = (0.42019099703461577, 0.41323568513979647, 0.4010048431259079)
STD = (0.30598050258519743, 0.3089986932156864, 0.3054061869915674)


@pytest.fixture(scope="module")
def params(golden_dir):
    return np.load(os.path.join(golden_dir, "aug_params.npz"))


def _pipelines():
    bc = T.Compose([T.Resize((480, 360)), T.RandomRotation(15, fill=11), T.RandomGaussianBlur(), T.RandomHorizontalFlip(),
                    T.ColorJitter(0.0, 0.4, 0.4), T.ToTensor(), T.Normalize(MEAN, STD)])
    return {"train": T.train_transforms(), "bc": bc}


@pytest.mark.parametrize("name", ["train", "bc"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sampler_reproduces_the_reference_draws(params, name, seed):
    pipe = _pipelines()[name]
    key = f"{name}_s{seed}_"
    random.seed(seed)
    drawn = [pipe.draw() for _ in range(len(params[key + "flipped"]))]
    assert not params[key + "rotated"].any()
    assert [p["flip"] for p in drawn] == params[key + "flipped"].tolist()
    assert [p["blur"] is not None for p in drawn] == params[key + "blurred"].tolist()
    assert [p["blur"][0] if p["blur"] else 0 for p in drawn] == params[key + "ksize"].tolist()
    sig = np.array([p["blur"][1] if p["blur"] else 0.0 for p in drawn], dtype=np.float64)
    assert np.array_equal(sig.view(np.uint64), params[key + "sigma"].view(np.uint64))           # bitwise
    assert [bool(p["jitter"]) for p in drawn] == params[key + "jittered"].tolist()
    assert [len(p["jitter"] or []) for p in drawn] == params[key + "nlut"].tolist()
    rec = T.Compose.pack(drawn)
    assert np.array_equal(rec["lut"][rec["use_lut"] != 0], params[key + "lut"][params[key + "jittered"]])
    assert (params[key + "lut"][~params[key + "jittered"]] == np.arange(256)).all()
    version, state, gauss = random.getstate()
    assert version == int(params[key + "state_version"]) and list(state) == params[key + "state"].tolist()
    assert gauss is None and math.isnan(float(params[key + "gauss_next"]))


def test_reference_frequencies_and_bucket_rule(params):
    fl = np.concatenate([params[f"train_s{s}_flipped"] for s in range(3)])
    bl = np.concatenate([params[f"train_s{s}_blurred"] for s in range(3)])
    lu = np.concatenate([params[f"train_s{s}_jittered"] for s in range(3)])
    assert 0.44 < fl.mean() < 0.56 and 0.44 < bl.mean() < 0.56 and 0.54 < lu.mean() < 0.67
    assert set(np.concatenate([params[f"train_s{s}_ksize"] for s in range(3)]).tolist()) <= {0, 3, 5, 7, 9}
    two = params["bc_s0_nlut"] == 2
    assert two.all()


def _taps64(k, sigma):
    """cv2.getGaussianKernel restated independently"""
    if sigma <= 0 and k <= 7:
        from math import comb
        return np.array([comb(k - 1, i) for i in range(k)], dtype=np.float64) / 2 ** (k - 1)
    s = sigma if sigma > 0 else ((k - 1) * 0.5 - 1) * 0.3 + 0.8
    x = np.arange(k, dtype=np.float64) - (k - 1) / 2
    g = np.exp(-x * x / (2 * s * s))
    return g / g.sum()


def test_packed_records_match_an_fp64_restatement():
    assert T.RECORD.itemsize == ctypes.sizeof(_lib.AugmentRecord) == _lib.load().cvk_augment_record_bytes()
    params = [{"flip": True, "blur": (3, 0.95), "jitter": [("brightness", 1.3)]},
              {"flip": False, "blur": (9, 2.9), "jitter": [("contrast", 0.7), ("brightness", 1.1)]},
              {"flip": False, "blur": (5, 0.0), "jitter": None},
              {"flip": True, "blur": None, "jitter": [("brightness", 0.61), ("contrast", 1.39)]}]
    rec = T.Compose.pack(params)
    assert rec["flip"].tolist() == [1, 0, 0, 1] and rec["ksize"].tolist() == [3, 9, 5, 0] and rec["use_lut"].tolist() == [1, 1, 0, 1]
    for r, p in zip(rec, params):
        if p["blur"]:
            k, s = p["blur"]
            ref = _taps64(k, s)
            assert np.array_equal(r["taps"][:k], ref.astype(np.float32)) or np.abs(r["taps"][:k] - ref).max() < 1e-7
            assert (r["taps"][k:] == 0).all()
        lut = np.arange(256, dtype=np.float64)
        for name, f in p["jitter"] or []:
            lut = np.floor(np.clip(lut * f if name == "brightness" else (lut - 74) * f + 74, 0, 255))
        assert np.array_equal(r["lut"], lut.astype(np.uint8)) or not p["jitter"]
    # sigma <= 0 takes cv2's fixed small kernels; (5, 0.0) is the binomial one
    assert np.array_equal(rec[2]["taps"][:5], np.array([1, 4, 6, 4, 1], np.float32) / 16)


def test_augment_argument_validation_without_gpu():
    lib = _lib.load()
    m = (ctypes.c_float * 3)(*MEAN)
    sd = (ctypes.c_float * 3)(*STD)
    z = (ctypes.c_float * 3)(1.0, 0.0, 1.0)
    p = 4096                                         # a fake, 16-byte aligned device address: every call below is refused first
    assert lib.cvk_augment_u8(None, p, 1, 2, 720, 960, 360, 480, p, m, sd, p, p, None, None) == -1
    assert b"null" in lib.cvk_last_error_string()
    assert lib.cvk_augment_u8(p, p, 4, 2, 720, 960, 360, 480, p, m, sd, p, p, None, None) == -1          # mask_bytes
    assert b"bad arguments" in lib.cvk_last_error_string()
    assert lib.cvk_augment_u8(p, p, 1, 0, 720, 960, 360, 480, p, m, sd, p, p, None, None) == -1          # N
    assert lib.cvk_augment_u8(p, p, 1, 2, 720, 960, 360, 0, p, m, sd, p, p, None, None) == -1            # W
    assert lib.cvk_augment_u8(p, p, 1, 2, 720, 960, 360, 480, p, m, sd, p + 4, p, None, None) == -1      # unaligned out
    assert b"bad arguments" in lib.cvk_last_error_string()
    assert lib.cvk_augment_u8(p, p, 8, 70000, 720, 960, 360, 480, p, m, sd, p, p, None, None) == -1     # grid
    assert b"grid" in lib.cvk_last_error_string()
    assert lib.cvk_augment_u8(p, p, 1, 2, 720, 960, 360, 480, p, m, z, p, p, None, None) == -1           # zero std
    assert b"zero std" in lib.cvk_last_error_string()


def test_unsupported_pipelines_are_refused_when_built():
    with pytest.raises(NotImplementedError):
        T.RandomRotation(0.5)                                   # could rotate
    T.RandomRotation(15, fill=11)                               # train.py's: never does
    with pytest.raises(NotImplementedError):
        T.ColorJitter(0.4, 0.4, 0.0, 0.4)                       # saturation
    with pytest.raises(NotImplementedError):
        T.ColorJitter(0.4, 0.4, hue=0.1)
    with pytest.raises(NotImplementedError):
        T.RandomScale()
    with pytest.raises(NotImplementedError):
        T.Compose([T.Resize((480, 360)), T.RandomHorizontalFlip(), T.RandomGaussianBlur(), T.ToTensor()])
    with pytest.raises(NotImplementedError):
        T.Compose([T.Resize((480, 360)), T.ToTensor(), T.Resize((240, 180))])
    with pytest.raises(NotImplementedError):
        T.Compose([T.Resize((480, 360)), T.Normalize(MEAN, STD)])                   # no ToTensor
    with pytest.raises(NotImplementedError):
        T.RandomGaussianBlur(sigma=(0.0, 5.0))                  # more than 9 taps
    # reference argument checks kept
    with pytest.raises(ValueError):
        T.RandomRotation(15, angle=0)
    with pytest.raises(TypeError):
        T.Resize((1, 2, 3))
    v = T.valid_transforms()
    assert v.size == (480, 360) and v.out_hw(720, 960) == (360, 480) and v.mean == MEAN and v.std == STD
    random.seed(5)
    before = random.getstate()
    assert v.draw() == {"flip": False, "blur": None, "jitter": None}
    assert random.getstate() == before                          # the validation pipeline draws nothing
