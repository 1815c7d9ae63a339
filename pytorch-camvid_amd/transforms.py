"""The reference's training / validation transforms (transforms.py, composed in train.py:61-75) on the device, ONE HIP launch per
batch (`cvk_augment_u8`).  Class names and constructor signatures are the reference's, positional quirks included:

  Resize((480, 360)) -> RandomRotation(15, fill=...) -> RandomGaussianBlur() -> RandomHorizontalFlip() -> ColorJitter(0.4, 0.4)
    -> ToTensor() -> Normalize(MEAN, STD)

Every random parameter is drawn on the host from the module-level `random`, in the reference's order, so a seeded run makes the
same augmentation decisions as the reference's `Compose` (a DataLoader with num_workers=0).  Quirks reproduced:
  * RandomRotation(15, ...) binds 15 to p and skips when random() < p: it never rotates but draws one random() per sample.
  * ColorJitter(0.4, 0.4) is p = 0.4, brightness = 0.4; it fires when random() >= p.  Brightness / contrast are uint8 LUTs
    (truncating astype); with both enabled random.shuffle decides their order.  The LUTs of one sample are composed on the host
    into one table (exact: every stage maps uint8 to uint8).
  * RandomGaussianBlur: ksize from 3.3 * sigma (at least 3, made odd), taps by cv2.getGaussianKernel's formula in fp64.
Not supported (NotImplementedError when the pipeline is built): a RandomRotation that can fire (p < 1), saturation / hue jitter,
RandomScale, stages out of train.py's order."""
import math
import numbers
import random
from collections.abc import Iterable

import numpy as np
import torch

from . import _lib
from ._lib import check
from .functional import CAMVID_MEAN, CAMVID_STD, _stream

RECORD = np.dtype(_lib.AugmentRecord)       # one cvk_augment_record per sample
IDENTITY_LUT = np.arange(256, dtype=np.uint8)

# cv2.getGaussianKernel's fixed kernels for sigma <= 0 and ksize <= 7
_SMALL_GAUSSIAN = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
                   7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


def gaussian_taps(ksize, sigma):
    """cv2.getGaussianKernel(ksize, sigma) in fp64."""
    if ksize % 2 == 1 and ksize <= 7 and sigma <= 0:
        return np.array(_SMALL_GAUSSIAN[ksize], dtype=np.float64)
    s = sigma if sigma > 0 else ((ksize - 1) * 0.5 - 1) * 0.3 + 0.8
    scale2 = -0.5 / (s * s)
    t = np.array([math.exp(scale2 * (i - (ksize - 1) * 0.5) ** 2) for i in range(ksize)], dtype=np.float64)
    return t * (1.0 / t.sum())


def brightness_lut(factor):
    """reference adjust_brightness's table"""
    return np.array([i * factor for i in range(0, 256)]).clip(0, 255).astype("uint8")


def contrast_lut(factor):
    """reference adjust_contrast's table"""
    return np.array([(i - 74) * factor + 74 for i in range(0, 256)]).clip(0, 255).astype("uint8")


def compose_luts(stages):
    """One table for a sample's jitter stages [(name, factor), ...] applied in order."""
    table = IDENTITY_LUT.copy()
    for name, factor in stages:
        table = (brightness_lut if name == "brightness" else contrast_lut)(factor)[table]
    return table


class Resize:
    def __init__(self, size):
        if isinstance(size, int):
            self.size = (size, size)
        elif isinstance(size, Iterable) and len(size) == 2:
            self.size = size
        else:
            raise TypeError('size should be iterable with size 2 or int')

    def _draw(self, p):
        pass


class RandomScale:
    def __init__(self, scale=(0.5, 2.0), value=0):
        raise NotImplementedError("RandomScale is not supported by the device transforms")


class RandomRotation:
    def __init__(self, p=0.5, angle=10, fill=0):
        if not (isinstance(angle, numbers.Number) and angle > 0):
            raise ValueError('angle must be a positive number.')
        if not p >= 1:
            raise NotImplementedError(f"RandomRotation(p={p}) can rotate (it skips only when random() < p); "
                                      "the device transforms have no rotation")
        self.angle, self.value, self.p = angle, fill, p

    def _draw(self, p):
        random.random()         # always < p: the reference returns the sample unchanged


class RandomHorizontalFlip:
    def __init__(self, p=0.5):
        self.p = p

    def _draw(self, p):
        p["flip"] = random.random() < self.p


class RandomGaussianBlur:
    def __init__(self, p=0.5, sigma=(0.0, 3.0)):
        if not isinstance(sigma, Iterable) and len(sigma) == 2:
            raise TypeError('sigma should be iterable with length 2')
        if not sigma[1] >= sigma[0] >= 0:
            raise ValueError('sigma shoule be an iterval of nonegative real number')
        if self._compute_gaussian_blur_ksize(sigma[1]) > 9:
            raise NotImplementedError(f"RandomGaussianBlur(sigma={sigma}) can need more than 9 taps; the device kernel has at most 9")
        self.sigma, self.p = sigma, p

    @staticmethod
    def _compute_gaussian_blur_ksize(sigma):
        if sigma < 3.0:
            ksize = 3.3 * sigma
        elif sigma < 5.0:
            ksize = 2.9 * sigma
        else:
            ksize = 2.6 * sigma
        ksize = int(max(ksize, 3))
        if not ksize % 2:
            ksize += 1
        return ksize

    def _draw(self, p):
        if random.random() < self.p:
            sigma = random.uniform(*self.sigma)
            p["blur"] = (self._compute_gaussian_blur_ksize(sigma), sigma)


class ColorJitter:
    def __init__(self, p=0.5, brightness=0, contrast=0, saturation=0, hue=0):
        self.brightness = self._check_input(brightness, 'brightness')
        self.contrast = self._check_input(contrast, 'contrast')
        self.saturation = self._check_input(saturation, 'saturation')
        self.hue = self._check_input(hue, 'hue', center=0, bound=(-0.5, 0.5), clip_first_on_zero=False)
        if self.saturation is not None or self.hue is not None:
            raise NotImplementedError("saturation / hue jitter (PIL-based in the reference) is not supported by the device transforms")
        self.p = p

    @staticmethod
    def _check_input(value, name, center=1, bound=(0, float('inf')), clip_first_on_zero=True):
        if isinstance(value, numbers.Number):
            if value < 0:
                raise ValueError("If {} is a single number, it must be non negative.".format(name))
            value = [center - value, center + value]
            if clip_first_on_zero:
                value[0] = max(value[0], 0)
        elif isinstance(value, (tuple, list)) and len(value) == 2:
            if not bound[0] <= value[0] <= value[1] <= bound[1]:
                raise ValueError("{} values should be between {}".format(name, bound))
        else:
            raise TypeError("{} should be a single number or a list/tuple with length 2.".format(name))
        if value[0] == value[1] == center:
            value = None
        return value

    def _draw(self, p):
        if random.random() < self.p:
            return
        stages = []
        if self.brightness is not None:
            stages.append(("brightness", random.uniform(self.brightness[0], self.brightness[1])))
        if self.contrast is not None:
            stages.append(("contrast", random.uniform(self.contrast[0], self.contrast[1])))
        random.shuffle(stages)
        p["jitter"] = stages


class ToTensor:
    def _draw(self, p):
        pass


class Normalize:
    def __init__(self, mean, std, inplace=False):
        self.mean, self.std, self.inplace = mean, std, inplace

    def _draw(self, p):
        pass


_ORDER = (Resize, RandomRotation, RandomGaussianBlur, RandomHorizontalFlip, ColorJitter, ToTensor, Normalize)


class Compose:
    """A train.py-ordered pipeline.  Called on GPU uint8 frames [N,Hs,Ws,3] (BGR) and masks [N,Hs,Ws] (uint8, or int64) it draws
    N samples' parameters and returns (float32 [N,3,H,W] channels_last view, int64 [N,H,W]); out_u8=True adds the augmented
    uint8 frames [N,H,W,3] (before ToTensor / Normalize) as a third item."""

    def __init__(self, transforms):
        self.transforms = list(transforms)
        last = -1
        for t in self.transforms:
            kind = next((i for i, c in enumerate(_ORDER) if type(t) is c), None)
            if kind is None:
                raise NotImplementedError(f"{type(t).__name__} is not supported by the device transforms")
            if kind <= last:
                raise NotImplementedError("stages out of train.py's order (Resize, RandomRotation, RandomGaussianBlur, "
                                          "RandomHorizontalFlip, ColorJitter, ToTensor, Normalize)")
            last = kind
        if not any(type(t) is ToTensor for t in self.transforms):
            raise NotImplementedError("the device transforms end in ToTensor (optionally followed by Normalize)")
        rs = [t for t in self.transforms if type(t) is Resize]
        self.size = tuple(rs[0].size) if rs else None          # (w, h) as cv2.resize takes it
        nm = [t for t in self.transforms if type(t) is Normalize]
        self.mean = tuple(nm[0].mean) if nm else (0.0, 0.0, 0.0)
        self.std = tuple(nm[0].std) if nm else (1.0, 1.0, 1.0)

    def draw(self):
        """One sample's parameters from `random`, in the reference's order: {"flip": bool, "blur": (ksize, sigma) or None,
        "jitter": [(name, factor), ...] in applied order, or None}."""
        p = {"flip": False, "blur": None, "jitter": None}
        for t in self.transforms:
            t._draw(p)
        return p

    @staticmethod
    def pack(params, out=None):
        """Records (numpy array of cvk_augment_record) for a list of drawn parameters; `out` may be a RECORD array to fill."""
        rec = np.zeros(len(params), dtype=RECORD) if out is None else out
        rec[...] = np.zeros((), dtype=RECORD)
        for i, p in enumerate(params):
            rec[i]["flip"] = int(bool(p["flip"]))
            if p["blur"] is not None:
                k, sigma = p["blur"]
                rec[i]["ksize"] = k
                rec[i]["taps"][:k] = gaussian_taps(k, sigma).astype(np.float32)
            if p["jitter"]:
                rec[i]["use_lut"] = 1
                rec[i]["lut"] = compose_luts(p["jitter"])
        return rec

    def out_hw(self, Hs, Ws):
        return (Hs, Ws) if self.size is None else (int(self.size[1]), int(self.size[0]))

    def __call__(self, frames, masks, out_u8=False):
        rec = self.pack([self.draw() for _ in range(frames.shape[0])])
        grec = torch.from_numpy(rec.view(np.uint8)).to(frames.device)
        return augment_u8(frames, masks, grec, self.out_hw(frames.shape[1], frames.shape[2]), self.mean, self.std, out_u8)

    def __repr__(self):
        return "Compose(" + "".join(f"\n    {type(t).__name__}" for t in self.transforms) + "\n)"


def augment_u8(frames, masks, records, size, mean=CAMVID_MEAN, std=CAMVID_STD, out_u8=False):
    """One `cvk_augment_u8` launch: frames uint8 [N,Hs,Ws,3] and masks [N,Hs,Ws] (uint8 or int64) on the GPU, `records` a device
    uint8 tensor of N packed cvk_augment_record (Compose.pack), size = (H, W) of the output.  No host synchronisation."""
    import ctypes
    lib = _lib.load()
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or not frames.is_cuda:
        raise ValueError("expected uint8 HIP frames of shape [N, H, W, 3]")
    N, Hs, Ws, _ = frames.shape
    if masks.dtype not in (torch.uint8, torch.int64) or tuple(masks.shape) != (N, Hs, Ws) or masks.device != frames.device:
        raise ValueError("expected uint8 or int64 masks of shape [N, H, W] on the frames' device")
    if records.dtype != torch.uint8 or records.numel() != N * RECORD.itemsize or records.device != frames.device:
        raise ValueError(f"expected {N} packed records ({N * RECORD.itemsize} bytes) on the frames' device")
    H, W = size
    frames, masks, records = frames.contiguous(), masks.contiguous(), records.contiguous()
    out = torch.empty((N, H, W, 4), device=frames.device, dtype=torch.float32)
    out_masks = torch.empty((N, H, W), device=frames.device, dtype=torch.int64)
    u8 = torch.empty((N, H, W, 3), device=frames.device, dtype=torch.uint8) if out_u8 else None
    m = (ctypes.c_float * 3)(*mean); sd = (ctypes.c_float * 3)(*std)
    check(lib.cvk_augment_u8(frames.data_ptr(), masks.data_ptr(), masks.element_size(), N, Hs, Ws, H, W, records.data_ptr(), m, sd,
                             out.data_ptr(), out_masks.data_ptr(), u8.data_ptr() if u8 is not None else None, _stream(frames)),
          "cvk_augment_u8")
    x = out[..., :3].permute(0, 3, 1, 2)
    return (x, out_masks, u8) if out_u8 else (x, out_masks)


def train_transforms(image_size=(480, 360), ignore_index=11, mean=CAMVID_MEAN, std=CAMVID_STD):
    """train.py:61-69 (IMAGE_SIZE is (w, h); CamVid's ignore_index is Void = 11)."""
    return Compose([
        Resize(image_size),
        RandomRotation(15, fill=ignore_index),
        RandomGaussianBlur(),
        RandomHorizontalFlip(),
        ColorJitter(0.4, 0.4),
        ToTensor(),
        Normalize(mean, std),
    ])


def valid_transforms(image_size=(480, 360), mean=CAMVID_MEAN, std=CAMVID_STD):
    """train.py:71-75"""
    return Compose([Resize(image_size), ToTensor(), Normalize(mean, std)])


__all__ = ["Compose", "Resize", "RandomRotation", "RandomGaussianBlur", "RandomHorizontalFlip", "ColorJitter", "ToTensor",
           "Normalize", "RandomScale", "train_transforms", "valid_transforms", "augment_u8", "gaussian_taps", "RECORD"]
