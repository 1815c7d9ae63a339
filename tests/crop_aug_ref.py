"""fp64 numpy restatement of crop training on the device (cvk_crop_select, cvk_crop_augment_u8; DESIGN.md "Crop training") for the
tests: the virtual resized image with explicit steps (cv2's INTER_LINEAR / INTER_NEAREST mappings), the separable Gaussian with
REFLECT_101 at the resized image's borders, the LUT, the window with its pad, the canvas flip, the per-candidate class counts and the
selection rule.  Not an oracle of OpenCV's numerics: its 8-bit fixed-point resize and its fx rounding are not restated (no cv2 here)."""
import numpy as np

from tests import augment_ref as R

MAX_CAND = 11


def linear_coords(dst, src, step):
    f = (np.arange(dst, dtype=np.float64) + 0.5) * np.float64(step) - 0.5
    i = np.floor(f).astype(np.int64)
    a = f - i
    lo = i < 0
    i[lo], a[lo] = 0, 0.0
    hi = i >= src - 1
    i[hi], a[hi] = src - 1, 0.0
    return i, np.minimum(i + 1, src - 1), a


def resize_linear_pre(img, Hr, Wr, sy, sx):
    """uint8 [Hs,Ws,3] -> float64 [Hr,Wr,3]: the bilinear value before rounding"""
    Hs, Ws = img.shape[:2]
    y0, y1, ay = linear_coords(Hr, Hs, sy)
    x0, x1, ax = linear_coords(Wr, Ws, sx)
    f = img.astype(np.float64)
    ax = ax[None, :, None]
    top = (1 - ax) * f[y0][:, x0] + ax * f[y0][:, x1]
    bot = (1 - ax) * f[y1][:, x0] + ax * f[y1][:, x1]
    ay = ay[:, None, None]
    return (1 - ay) * top + ay * bot


def round_u8(v):
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def resize_nearest(mask, Hr, Wr, sy, sx):
    Hs, Ws = mask.shape[:2]
    yi = np.minimum(np.floor(np.arange(Hr) * np.float64(sy)).astype(np.int64), Hs - 1)
    xi = np.minimum(np.floor(np.arange(Wr) * np.float64(sx)).astype(np.int64), Ws - 1)
    return mask[yi][:, xi]


def blur_pre(img, taps):
    """separable Gaussian (rows, then columns) in fp64 with REFLECT_101 borders: the value before rounding"""
    k = len(taps)
    r = (k - 1) // 2
    f = np.pad(img.astype(np.float64), ((r, r), (r, r), (0, 0)), mode="reflect")
    H, W = img.shape[:2]
    h = sum(taps[t] * f[:, t:t + W] for t in range(k))
    return sum(taps[t] * h[t:t + H] for t in range(k))


def near_half(pre, delta):
    """values whose distance to a half-integer is below delta: where fp32 and fp64 may round to different levels"""
    return np.abs(pre - np.floor(pre) - 0.5) < delta


def window(img, hc, wc, offy, offx, fill):
    """the hc x wc window at a signed offset of a [Hr,Wr,...] array; (crop, inside): outside the array the crop holds `fill`"""
    Hr, Wr = img.shape[:2]
    out = np.full((hc, wc) + img.shape[2:], fill, dtype=img.dtype)
    inside = np.zeros((hc, wc), dtype=bool)
    y0, y1 = max(0, -offy), min(hc, Hr - offy)
    x0, x1 = max(0, -offx), min(wc, Wr - offx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = img[y0 + offy:y1 + offy, x0 + offx:x1 + offx]
        inside[y0:y1, x0:x1] = True
    return out, inside


def resized(frame, Hr, Wr, sy, sx, ksize=0, taps=None, lut=None):
    """the blurred and LUT-mapped resized image, uint8 [Hr,Wr,3]"""
    x = round_u8(resize_linear_pre(frame, Hr, Wr, sy, sx))
    if ksize:
        x = R.blur(x, np.asarray(taps, dtype=np.float64)[:ksize])
    if lut is not None:
        x = np.asarray(lut, dtype=np.uint8)[x]
    return x


def crop_augment(frame, mask, Hr, Wr, sy, sx, hc, wc, offy, offx, ksize=0, taps=None, flip=False, lut=None, pad_label=11):
    """one sample: (uint8 [hc,wc,3] with 0 at the pad, mask [hc,wc] with pad_label at the pad, inside bool [hc,wc])"""
    x, inside = window(resized(frame, Hr, Wr, sy, sx, ksize, taps, lut), hc, wc, offy, offx, 0)
    m, _ = window(resize_nearest(mask, Hr, Wr, sy, sx).astype(np.int64), hc, wc, offy, offx, pad_label)
    if flip:
        x, m, inside = x[:, ::-1], m[:, ::-1], inside[:, ::-1]
    return np.ascontiguousarray(x), np.ascontiguousarray(m), np.ascontiguousarray(inside)


def candidate_counts(mask, Hr, Wr, sy, sx, hc, wc, offy, offx, ignore_index):
    """uint32 [256]: the resized labels inside (window ∩ resized image) per value; ignore_index and values outside [0, 256) not counted"""
    m, inside = window(resize_nearest(mask, Hr, Wr, sy, sx).astype(np.int64), hc, wc, offy, offx, 0)
    v = m[inside]
    v = v[(v != ignore_index) & (v >= 0) & (v < 256)]
    return np.bincount(v, minlength=256).astype(np.uint32)


def select(counts, ncand, cat_max_ratio):
    """(candidate, passed) of a count table uint32 [>= ncand, 256]: candidates 0 .. ncand - 2 in order, the first with more than
    one value counted and float64(max) / float64(sum) < cat_max_ratio; else (ncand - 1, 0)"""
    for c in range(ncand - 1):
        row = counts[c]
        if np.count_nonzero(row) > 1 and np.float64(row.max()) / np.float64(row.sum(dtype=np.uint64)) < np.float64(cat_max_ratio):
            return c, 1
    return ncand - 1, 0


def selection_tables(masks, records, hc, wc, ignore_index, cat_max_ratio):
    """(counts uint32 [N,11,256], selection int32 [N,4] = candidate, offy, offx, passed) for packed records"""
    N = len(records)
    counts = np.zeros((N, MAX_CAND, 256), dtype=np.uint32)
    sel = np.zeros((N, 4), dtype=np.int32)
    for n, r in enumerate(records):
        k = int(r["ncand"])
        for c in range(k):
            counts[n, c] = candidate_counts(masks[n], int(r["Hr"]), int(r["Wr"]), float(r["sy"]), float(r["sx"]), hc, wc,
                                            int(r["offy"][c]), int(r["offx"][c]), ignore_index)
        c, passed = select(counts[n], k, cat_max_ratio)
        sel[n] = (c, r["offy"][c], r["offx"][c], passed)
    return counts, sel


# ---- inputs and bands shared by tests/test_crop_aug_cpu.py (which asserts the share of values inside a band from the restatement
# alone) and tests/test_gpu_crop_aug.py (which lets the kernel differ inside the band only) ---------------------------------------
N, HS, WS, HC, WC = 3, 45, 83, 33, 70           # odd source; one full + one partial 64-wide tile, three 16-high tiles (last partial)
RATIOS = (0.61, 1.37, 1.93)
BLURS = ((3, 0.8), (9, 2.7))                    # radii 1 and 4; sigma > 0: generic (non-dyadic) taps

# fp32 roundings between the three source bytes and the rounded resized value (aug_coord / crop_tile stage A), each at most
# 2^-24 relative on a magnitude of at most 255:
#   2  double -> float casts of the weights ax, ay
#   2  the complements 1 - ax, 1 - ay
#   6  top and bot: two products and one sum each
#   3  the vertical blend: two products and one sum
#   1  v + 0.5f inside the rounding
RESIZE_ROUNDINGS = 14
DELTA_RESIZE = 2 * RESIZE_ROUNDINGS * 2.0 ** -24 * 255


def blur_delta(ksize):
    """the two passes: ksize FMAs each (one rounding per FMA; the taps are fp32 in the record and in the restatement alike, the
    inputs are uint8 values: exact), and v + 0.5f inside the rounding"""
    return 2 * (2 * ksize + 1) * 2.0 ** -24 * 255


def frames_masks(n=N, Hs=HS, Ws=WS, seed=0):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (n, Hs, Ws, 3), dtype=np.uint8), g.integers(0, 12, (n, Hs, Ws), dtype=np.uint8)


def step_cases(Hs=HS, Ws=WS):
    """(name, Hr, Wr, sy, sx) for every ratio under both step rules: cv2's dsize rule (steps Hs / Hr, Ws / Wr) and its fx rule
    (steps 1 / r, size round-half-even of r * n)"""
    out = []
    for r in RATIOS:
        Hr, Wr = max(int(Hs * r + 0.5), 1), max(int(Ws * r + 0.5), 1)
        out.append((f"dsize{r}", Hr, Wr, Hs / Hr, Ws / Wr))
        out.append((f"fx{r}", max(round(r * Hs), 1), max(round(r * Ws), 1), 1.0 / r, 1.0 / r))
    return out
