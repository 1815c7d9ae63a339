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
RandomScale inside a `Compose`, stages out of train.py's order.

Crop training (`CropCompose`, `crop_transforms()`; two launches per batch, `cvk_crop_select` + `cvk_crop_augment_u8`):

  RandomResize(ratio_range) -> RandomCrop(crop_size, cat_max_ratio) -> [RandomGaussianBlur] -> RandomHorizontalFlip -> [ColorJitter]
    -> ToTensor() -> Normalize(MEAN, STD)            (mmseg's RandomResize + RandomCrop + RandomFlip + Pad)
  ScaleJitter(scale, value) -> ...the same tail...   (the reference's own RandomScale, transforms.py:63-127, as a draw rule)

The host draws a ratio and ALWAYS eleven candidate offsets per sample (one when cat_max_ratio is 1), so the random stream never
depends on device data; the device counts the labels of every candidate window and takes the first whose largest class holds
less than cat_max_ratio of its counted pixels, else the eleventh.  The resized image is never materialised.
Not supported by the crop pipeline either: rotation, saturation / hue jitter, PhotoMetricDistortion's HSV stages, per-class crop
sampling, labels >= 256 taking part in the ratio (they pass through to the output mask but are not counted)."""
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


# ---- crop training: random rescale, class-balanced crop, pad ---------------------------------------------------------------------------
CROP_RECORD = np.dtype(_lib.CropRecord)     # one cvk_crop_record per sample
MAX_CANDIDATES = 11                         # mmseg's RandomCrop: ten tries, the eleventh box is taken as it is


def resized_hw(Hs, Ws, r, scale=None):
    """(Hr, Wr) of a frame rescaled by ratio r.  scale=None: round half up of each side, at least 1.  scale=(a, b): mmcv's
    keep-ratio rule on the box (a, b) * r: the largest size that fits its long and its short edge."""
    if scale is None:
        return max(int(Hs * r + 0.5), 1), max(int(Ws * r + 0.5), 1)
    L, S = int(max(scale) * r), int(min(scale) * r)
    sf = min(L / max(Hs, Ws), S / min(Hs, Ws))
    return max(int(Hs * sf + 0.5), 1), max(int(Ws * sf + 0.5), 1)


class RandomResize:
    def __init__(self, ratio_range=(0.5, 2.0), scale=None):
        if not (isinstance(ratio_range, Iterable) and len(ratio_range) == 2 and 0 < ratio_range[0] <= ratio_range[1]):
            raise ValueError('ratio_range should be two positive numbers (min, max)')
        if scale is not None and not (isinstance(scale, Iterable) and len(scale) == 2 and min(scale) > 0):
            raise ValueError('scale should be None or two positive numbers')
        self.ratio_range, self.scale = tuple(ratio_range), None if scale is None else tuple(scale)


class RandomCrop:
    def __init__(self, crop_size, cat_max_ratio=0.75, ignore_index=11):
        if not (isinstance(crop_size, Iterable) and len(crop_size) == 2 and crop_size[0] > 0 and crop_size[1] > 0):
            raise ValueError('crop_size should be (h, w), both positive')
        if not 0 < cat_max_ratio <= 1:
            raise ValueError('cat_max_ratio should be in (0, 1]')
        self.crop_size, self.cat_max_ratio, self.ignore_index = (int(crop_size[0]), int(crop_size[1])), float(cat_max_ratio), ignore_index


class ScaleJitter:
    """The reference's RandomScale (transforms.py:63-127): rescale by a factor, pad centred with black / `value` up to the source
    size, crop the source size at a random place.  One candidate, no selection rule."""

    def __init__(self, scale=(0.5, 2.0), value=11):
        if not (isinstance(scale, Iterable) and len(scale) == 2 and 0 < scale[0] <= scale[1]):
            raise ValueError('scale should be two positive numbers (min, max)')
        self.scale, self.value = tuple(scale), value


_CROP_TAIL = (RandomGaussianBlur, RandomHorizontalFlip, ColorJitter, ToTensor, Normalize)


class CropCompose:
    """A crop-training pipeline (the module docstring has the two accepted forms).  Called like `Compose`: GPU uint8 frames
    [N,Hs,Ws,3] and masks [N,Hs,Ws] (uint8 or int64) -> (float32 [N,3,hc,wc] channels_last view, int64 [N,hc,wc]) and, with
    out_u8=True, the uint8 crops.  `last_selection` is the device table int32 [N,4] = (candidate, offy, offx, passed) of the last
    call; reading it on the host is the caller's synchronisation, the pipeline itself never does."""

    def __init__(self, transforms):
        self.transforms = list(transforms)
        t = self.transforms
        if t and type(t[0]) is ScaleJitter:
            self.jitter_stage, self.resize, self.crop, tail = t[0], None, None, t[1:]
        elif len(t) >= 2 and type(t[0]) is RandomResize and type(t[1]) is RandomCrop:
            self.jitter_stage, self.resize, self.crop, tail = None, t[0], t[1], t[2:]
        else:
            raise NotImplementedError("a crop pipeline starts with RandomResize, RandomCrop or with ScaleJitter")
        last = -1
        for st in tail:
            kind = next((i for i, c in enumerate(_CROP_TAIL) if type(st) is c), None)
            if kind is None:
                raise NotImplementedError(f"{type(st).__name__} is not supported at this place of a crop pipeline")
            if kind <= last:
                raise NotImplementedError("stages out of order (RandomResize, RandomCrop, RandomGaussianBlur, RandomHorizontalFlip, "
                                          "ColorJitter, ToTensor, Normalize)")
            last = kind
        if not any(type(st) is ToTensor for st in tail):
            raise NotImplementedError("the device transforms end in ToTensor (optionally followed by Normalize)")
        self._tail = tail
        nm = [st for st in tail if type(st) is Normalize]
        self.mean = tuple(nm[0].mean) if nm else (0.0, 0.0, 0.0)
        self.std = tuple(nm[0].std) if nm else (1.0, 1.0, 1.0)
        if self.crop is not None:
            self.cat_max_ratio, self.ignore_index = self.crop.cat_max_ratio, int(self.crop.ignore_index)
            self.pad_label, self.pad_normalized = int(self.crop.ignore_index), 0
        else:
            self.cat_max_ratio, self.ignore_index = 1.0, int(self.jitter_stage.value)
            self.pad_label, self.pad_normalized = int(self.jitter_stage.value), 1
        self.last_selection = None
        self._tables = {}

    def out_hw(self, Hs, Ws):
        return (Hs, Ws) if self.crop is None else self.crop.crop_size

    def draw(self, Hs, Ws):
        """One sample's parameters from `random`, in stage order: the ratio, the K candidate offsets (y then x each), then the blur,
        flip and jitter draws of the existing classes.  {"r", "Hr", "Wr", "sy", "sx", "cands": [(offy, offx), ...], "flip", "blur",
        "jitter"}."""
        hc, wc = self.out_hw(Hs, Ws)
        if self.crop is not None:
            r = random.uniform(*self.resize.ratio_range)
            Hr, Wr = resized_hw(Hs, Ws, r, self.resize.scale)
            sy, sx = Hs / Hr, Ws / Wr
            K = MAX_CANDIDATES if self.cat_max_ratio < 1 else 1
            cands = []
            for _ in range(K):
                oy = random.randint(0, max(Hr - hc, 0))
                ox = random.randint(0, max(Wr - wc, 0))
                cands.append((oy, ox))
        else:
            r = random.uniform(*self.jitter_stage.scale)
            Hr, Wr = max(round(r * Hs), 1), max(round(r * Ws), 1)          # cv2's fx rule (unverified against cv2 itself)
            sy = sx = 1.0 / r
            dh, dw = max(0, Hs - Hr), max(0, Ws - Wr)
            y1 = random.randint(0, max(Hr, Hs) - Hs)
            x1 = random.randint(0, max(Wr, Ws) - Ws)
            cands = [(y1 - dh // 2, x1 - dw // 2)]
        p = {"r": r, "Hr": Hr, "Wr": Wr, "sy": sy, "sx": sx, "flip": False, "blur": None, "jitter": None}
        for st in self._tail:
            st._draw(p)
        if self.crop is not None and p["flip"] and Wr < wc:
            cands = [(oy, Wr - wc) for oy, _ in cands]      # content at the left after the canvas flip, as mmseg's flip-then-pad
        p["cands"] = cands
        return p

    @staticmethod
    def pack(params, out=None):
        """Records (numpy array of cvk_crop_record) for a list of drawn parameters; `out` may be a CROP_RECORD array to fill."""
        rec = np.zeros(len(params), dtype=CROP_RECORD) if out is None else out
        rec[...] = np.zeros((), dtype=CROP_RECORD)
        for i, p in enumerate(params):
            rec[i]["sy"], rec[i]["sx"], rec[i]["Hr"], rec[i]["Wr"] = p["sy"], p["sx"], p["Hr"], p["Wr"]
            k = len(p["cands"])
            if not 1 <= k <= MAX_CANDIDATES:
                raise ValueError(f"a record holds 1 to {MAX_CANDIDATES} candidates, got {k}")
            rec[i]["ncand"] = k
            rec[i]["offy"][:k] = [c[0] for c in p["cands"]]
            rec[i]["offx"][:k] = [c[1] for c in p["cands"]]
            rec[i]["flip"] = int(bool(p["flip"]))
            if p["blur"] is not None:
                ks, sigma = p["blur"]
                rec[i]["ksize"] = ks
                rec[i]["taps"][:ks] = gaussian_taps(ks, sigma).astype(np.float32)
            if p["jitter"]:
                rec[i]["use_lut"] = 1
                rec[i]["lut"] = compose_luts(p["jitter"])
        return rec

    def tables(self, N, device):
        """The count (uint32 [N,11,256], as int32 storage) and selection (int32 [N,4]) tables, cached per (N, device)."""
        key = (N, str(device))
        if key not in self._tables:
            self._tables[key] = (torch.empty((N, MAX_CANDIDATES, 256), device=device, dtype=torch.int32),
                                 torch.empty((N, 4), device=device, dtype=torch.int32))
        return self._tables[key]

    def apply(self, frames, masks, records, out_u8=False):
        """The two launches for device records (uint8 tensor of N packed cvk_crop_record).  No host synchronisation."""
        counts, sel = self.tables(frames.shape[0], frames.device)
        crop_select(masks, records, frames.shape[1:3], self.out_hw(frames.shape[1], frames.shape[2]), self.ignore_index,
                    self.cat_max_ratio, counts, sel)
        self.last_selection = sel
        return crop_augment_u8(frames, masks, records, sel, self.out_hw(frames.shape[1], frames.shape[2]), self.mean, self.std,
                               self.pad_label, self.pad_normalized, out_u8)

    def __call__(self, frames, masks, out_u8=False):
        N, Hs, Ws = frames.shape[:3]
        rec = self.pack([self.draw(Hs, Ws) for _ in range(N)])
        return self.apply(frames, masks, torch.from_numpy(rec.view(np.uint8)).to(frames.device), out_u8)

    def __repr__(self):
        return "CropCompose(" + "".join(f"\n    {type(t).__name__}" for t in self.transforms) + "\n)"


def _check_crop_inputs(masks, records, N, Hs, Ws):
    if masks.dtype not in (torch.uint8, torch.int64) or tuple(masks.shape) != (N, Hs, Ws) or not masks.is_cuda:
        raise ValueError("expected uint8 or int64 HIP masks of shape [N, H, W]")
    if records.dtype != torch.uint8 or records.numel() != N * CROP_RECORD.itemsize or records.device != masks.device:
        raise ValueError(f"expected {N} packed records ({N * CROP_RECORD.itemsize} bytes) on the masks' device")


def crop_select(masks, records, src_hw, crop_hw, ignore_index, cat_max_ratio, counts, selection):
    """`cvk_crop_select`: fills counts (int32 storage [N,11,256]) and selection (int32 [N,4]) for device records."""
    N = masks.shape[0]
    _check_crop_inputs(masks, records, N, src_hw[0], src_hw[1])
    for t, shape in ((counts, (N, MAX_CANDIDATES, 256)), (selection, (N, 4))):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or t.device != masks.device or not t.is_contiguous():
            raise ValueError(f"expected a contiguous int32 table of shape {shape} on the masks' device")
    masks, records = masks.contiguous(), records.contiguous()
    check(_lib.load().cvk_crop_select(masks.data_ptr(), masks.element_size(), N, src_hw[0], src_hw[1], crop_hw[0], crop_hw[1],
                                      records.data_ptr(), int(ignore_index), float(cat_max_ratio), counts.data_ptr(),
                                      selection.data_ptr(), _stream(masks)), "cvk_crop_select")


def crop_augment_u8(frames, masks, records, selection, size, mean=CAMVID_MEAN, std=CAMVID_STD, pad_label=11, pad_normalized=0,
                    out_u8=False):
    """One `cvk_crop_augment_u8` launch for device records and a device selection table; size = (hc, wc)."""
    import ctypes
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or not frames.is_cuda:
        raise ValueError("expected uint8 HIP frames of shape [N, H, W, 3]")
    N, Hs, Ws, _ = frames.shape
    _check_crop_inputs(masks, records, N, Hs, Ws)
    if selection.dtype != torch.int32 or tuple(selection.shape) != (N, 4) or selection.device != frames.device:
        raise ValueError("expected an int32 selection table of shape [N, 4] on the frames' device")
    hc, wc = size
    frames, masks, records, selection = frames.contiguous(), masks.contiguous(), records.contiguous(), selection.contiguous()
    out = torch.empty((N, hc, wc, 4), device=frames.device, dtype=torch.float32)
    out_masks = torch.empty((N, hc, wc), device=frames.device, dtype=torch.int64)
    u8 = torch.empty((N, hc, wc, 3), device=frames.device, dtype=torch.uint8) if out_u8 else None
    m = (ctypes.c_float * 3)(*mean); sd = (ctypes.c_float * 3)(*std)
    check(_lib.load().cvk_crop_augment_u8(frames.data_ptr(), masks.data_ptr(), masks.element_size(), N, Hs, Ws, hc, wc,
                                          records.data_ptr(), selection.data_ptr(), m, sd, int(pad_label), int(pad_normalized),
                                          out.data_ptr(), out_masks.data_ptr(), u8.data_ptr() if u8 is not None else None,
                                          _stream(frames)), "cvk_crop_augment_u8")
    x = out[..., :3].permute(0, 3, 1, 2)
    return (x, out_masks, u8) if out_u8 else (x, out_masks)


def crop_transforms(crop_size=(360, 480), ratio_range=(0.5, 2.0), cat_max_ratio=0.75, ignore_index=11, blur=False, jitter=True,
                    mean=CAMVID_MEAN, std=CAMVID_STD):
    """The crop-training recipe (mmseg's RandomResize + RandomCrop + RandomFlip + Pad, the reference's brightness / contrast
    jitter in place of PhotoMetricDistortion); crop_size is (h, w)."""
    stages = [RandomResize(ratio_range), RandomCrop(crop_size, cat_max_ratio, ignore_index)]
    if blur:
        stages.append(RandomGaussianBlur())
    stages.append(RandomHorizontalFlip())
    if jitter:
        stages.append(ColorJitter(0.4, 0.4))
    return CropCompose(stages + [ToTensor(), Normalize(mean, std)])


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
           "Normalize", "RandomScale", "train_transforms", "valid_transforms", "augment_u8", "gaussian_taps", "RECORD",
           "CropCompose", "RandomResize", "RandomCrop", "ScaleJitter", "crop_transforms", "resized_hw", "crop_select", "crop_augment_u8",
           "CROP_RECORD", "MAX_CANDIDATES"]
