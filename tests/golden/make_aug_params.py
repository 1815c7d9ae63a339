#!/usr/bin/env python3
"""Record the augmentation decisions of the reference's transforms.py (train.py:61-75) per seed -> tests/golden/aug_params.npz.

Run in the build container only (needs the read-only reference checkout; cv2 and torchvision are absent, so recording stand-ins
take their place and only the random draws and the arguments the reference passes to cv2 are kept):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_aug_params.py [/path/to/reference]

Pipelines, per seed 0, 1, 2 x 256 samples (random.seed(seed), then one call per sample, as a DataLoader with num_workers=0):
  "train":   Resize((480, 360)), RandomRotation(15, fill=11), RandomGaussianBlur(), RandomHorizontalFlip(), ColorJitter(0.4, 0.4),
             ToTensor(), Normalize(MEAN, STD)
  "bc":      the same with ColorJitter(0.0, 0.4, 0.4): brightness and contrast both on, so random.shuffle draws
Per sample: rotated / blurred / flipped / jittered flags, blur ksize and sigma, and the composition of the tables passed to
cv2.LUT (identity when none); per seed: random.getstate() after the last sample."""
import importlib.util
import os
import random
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "aug_params.npz")
SEEDS, SAMPLES = (0, 1, 2), 256
MEAN = (0.42019099703461577, 0.41323568513979647, 0.4010048431259079)
STD = (0.30598050258519743, 0.3089986932156864, 0.3054061869915674)

LOG = []          # calls of the current sample


def _cv2_stub():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_NEAREST, cv2.BORDER_CONSTANT = 0, 0

    def resize(img, size, interpolation=None, **kw):
        LOG.append(("resize", tuple(size), interpolation))
        return np.zeros((2, 2) + img.shape[2:], dtype=img.dtype)     # content is irrelevant: only the draws are recorded

    def GaussianBlur(img, ksize, sigmaX, sigmaY=0, **kw):
        LOG.append(("blur", tuple(ksize), sigmaX, sigmaY))
        return img

    def flip(img, code):
        LOG.append(("flip", code))
        return img

    def LUT(img, table):
        LOG.append(("lut", np.asarray(table).copy()))
        return img

    def getRotationMatrix2D(*a):
        LOG.append(("rotate",))
        return np.eye(2, 3)

    def warpAffine(img, *a, **kw):
        LOG.append(("warp",))
        return img

    for f in (resize, GaussianBlur, flip, LUT, getRotationMatrix2D, warpAffine):
        setattr(cv2, f.__name__, f)
    return cv2


def load_reference():
    sys.modules["cv2"] = _cv2_stub()
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tvf = types.ModuleType("torchvision.transforms.functional")
    tv.transforms, tvt.functional = tvt, tvf
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})
    spec = importlib.util.spec_from_file_location("ref_transforms", os.path.join(REF, "transforms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pipelines(T):
    def make(jitter):
        return T.Compose([T.Resize((480, 360)), T.RandomRotation(15, fill=11), T.RandomGaussianBlur(), T.RandomHorizontalFlip(),
                          jitter, T.ToTensor(), T.Normalize(MEAN, STD)])
    return {"train": make(T.ColorJitter(0.4, 0.4)), "bc": make(T.ColorJitter(0.0, 0.4, 0.4))}


def main():
    T = load_reference()
    out = {}
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    mask = np.zeros((4, 4), dtype=np.uint8)
    for name, pipe in pipelines(T).items():
        for seed in SEEDS:
            random.seed(seed)
            rows = {"rotated": [], "blurred": [], "flipped": [], "jittered": [], "ksize": [], "sigma": [], "nlut": [], "lut": []}
            for _ in range(SAMPLES):
                LOG.clear()
                pipe(img, mask)
                blur = [c for c in LOG if c[0] == "blur"]
                luts = [c[1] for c in LOG if c[0] == "lut"]
                flips = [c for c in LOG if c[0] == "flip"]
                assert len(flips) in (0, 2) and len(blur) <= 1
                assert all(c[1] == 1 for c in flips)
                assert not blur or (blur[0][1][0] == blur[0][1][1] and blur[0][2] == blur[0][3])
                table = np.arange(256, dtype=np.uint8)
                for t in luts:
                    table = t.astype(np.uint8)[table]
                rows["rotated"].append(any(c[0] in ("rotate", "warp") for c in LOG))
                rows["blurred"].append(bool(blur))
                rows["flipped"].append(bool(flips))
                rows["jittered"].append(bool(luts))
                rows["ksize"].append(blur[0][1][0] if blur else 0)
                rows["sigma"].append(blur[0][2] if blur else 0.0)
                rows["nlut"].append(len(luts))
                rows["lut"].append(table)
            key = f"{name}_s{seed}_"
            for k, v in rows.items():
                dt = {"ksize": np.int32, "nlut": np.int32, "sigma": np.float64, "lut": np.uint8}.get(k, np.bool_)
                out[key + k] = np.array(v, dtype=dt)
            version, state, gauss = random.getstate()
            out[key + "state"] = np.array(state, dtype=np.int64)
            out[key + "state_version"] = np.array(version, dtype=np.int64)
            out[key + "gauss_next"] = np.array(np.nan if gauss is None else gauss, dtype=np.float64)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: train seed 0 blur {out['train_s0_blurred'].mean():.2f} flip {out['train_s0_flipped'].mean():.2f} "
          f"lut {out['train_s0_jittered'].mean():.2f} rotation {out['train_s0_rotated'].mean():.2f}; "
          f"bc seed 0 two-LUT samples {(out['bc_s0_nlut'] == 2).mean():.2f}")


if __name__ == "__main__":
    main()
