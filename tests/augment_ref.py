"""fp64 numpy restatement of the device transforms (cvk_augment_u8) for the tests: cv2's INTER_LINEAR / INTER_NEAREST resize
mappings, a separable Gaussian with REFLECT_101 borders, the LUT and the flip.  Not an oracle of the reference's numerics:
OpenCV's own 8-bit fixed-point paths are not restated (cv2 is not available to check them)."""
import numpy as np


def _linear_coords(dst, src):
    f = (np.arange(dst, dtype=np.float64) + 0.5) * (src / dst) - 0.5
    i = np.floor(f).astype(np.int64)
    a = f - i
    lo = i < 0
    i[lo], a[lo] = 0, 0.0
    hi = i >= src - 1
    i[hi], a[hi] = src - 1, 0.0
    return i, np.minimum(i + 1, src - 1), a


def resize_linear(img, H, W):
    """uint8 [Hs,Ws,3] -> uint8 [H,W,3], bilinear in fp64, rounded half-up."""
    Hs, Ws = img.shape[:2]
    y0, y1, ay = _linear_coords(H, Hs)
    x0, x1, ax = _linear_coords(W, Ws)
    f = img.astype(np.float64)
    ax = ax[None, :, None]
    top = (1 - ax) * f[y0][:, x0] + ax * f[y0][:, x1]
    bot = (1 - ax) * f[y1][:, x0] + ax * f[y1][:, x1]
    ay = ay[:, None, None]
    return np.clip(np.floor((1 - ay) * top + ay * bot + 0.5), 0, 255).astype(np.uint8)


def resize_nearest(mask, H, W):
    Hs, Ws = mask.shape[:2]
    yi = np.minimum(np.floor(np.arange(H) * (Hs / H)).astype(np.int64), Hs - 1)
    xi = np.minimum(np.floor(np.arange(W) * (Ws / W)).astype(np.int64), Ws - 1)
    return mask[yi][:, xi]


def blur(img, taps):
    """separable Gaussian (rows, then columns) in fp64 with REFLECT_101 borders, rounded half-up"""
    k = len(taps)
    r = (k - 1) // 2
    f = np.pad(img.astype(np.float64), ((r, r), (r, r), (0, 0)), mode="reflect")     # numpy 'reflect' = REFLECT_101
    H, W = img.shape[:2]
    h = sum(taps[t] * f[:, t:t + W] for t in range(k))
    v = sum(taps[t] * h[t:t + H] for t in range(k))
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def augment(frame, mask, H, W, ksize=0, taps=None, flip=False, lut=None):
    """one sample: (uint8 [H,W,3], mask [H,W])"""
    x = resize_linear(frame, H, W)
    if ksize:
        x = blur(x, np.asarray(taps, dtype=np.float64)[:ksize])
    if lut is not None:
        x = np.asarray(lut, dtype=np.uint8)[x]
    m = resize_nearest(mask, H, W)
    if flip:
        x, m = x[:, ::-1], m[:, ::-1]
    return np.ascontiguousarray(x), np.ascontiguousarray(m)
