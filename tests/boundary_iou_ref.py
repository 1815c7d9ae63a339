"""Plain numpy restatement of the chessboard depth, the Boundary IoU counts (Cheng et al., CVPR 2021) and the trimap bins as
include/cvk.h defines them for cvk_cheb_depth / cvk_boundary_iou_counts, written from the brute-force definition: squares around a
pixel, no rows, no columns, no tiles.  Everything is integer and exact; the scores are plain loops in float64.

  depth0(z), for a pixel whose code is a class: the smallest k >= 1 for which the (2k+1) x (2k+1) square around z, clipped to the image,
  holds a pixel of another code (void and "other" are codes like any other); 255 if there is no such k below 255.  0 where the code is
  no class.  depth1 = min(depth0, 1 + min(x, W-1-x, y, H-1-y)).
"""
import math

import numpy as np

from tests.boundary_ref import codes

OTHER, VOID, LIMIT = 254, 255, 255


def code_bytes(x, void_from, K, ignore):
    """uint8 [..., H, W]: the class, 254 for a non-void value that is no class, 255 for void."""
    c = codes(x, void_from, K, ignore)
    return np.where(c == -2, VOID, np.where(c == -1, OTHER, c)).astype(np.uint8)


_DEPTH0 = {}


def depth0(code):
    """depth0 of one image's code bytes, int64 [H, W] (read-only: each distinct map is computed once and shared)."""
    key = (code.shape, code.tobytes())
    if key not in _DEPTH0:
        _DEPTH0[key] = _depth0(code)
        _DEPTH0[key].setflags(write=False)
    return _DEPTH0[key]


def _depth0(code):
    """int64 [H, W] of one image's code bytes.  Whether the clipped square of half-width k around a pixel of class c holds another code
    is read off a summed-area table of (code != c): the definition itself, one k after the other."""
    H, W = code.shape
    out = np.zeros((H, W), dtype=np.int64)
    for c in np.unique(code):
        if c >= 32:
            continue
        S = np.zeros((H + 1, W + 1), dtype=np.int64)
        S[1:, 1:] = np.cumsum(np.cumsum(code != c, axis=0), axis=1)
        ys, xs = np.nonzero(code == c)
        d = np.full(len(ys), LIMIT, dtype=np.int64)
        alive = np.arange(len(ys))
        for k in range(1, LIMIT):
            if alive.size == 0 or k > max(H, W):           # past that the square is the whole image for every pixel
                break
            y, x = ys[alive], xs[alive]
            y0, y1, x0, x1 = np.maximum(y - k, 0), np.minimum(y + k + 1, H), np.maximum(x - k, 0), np.minimum(x + k + 1, W)
            hit = (S[y1, x1] - S[y0, x1] - S[y1, x0] + S[y0, x0]) > 0
            d[alive[hit]] = k
            alive = alive[~hit]
        out[ys, xs] = d
    return out


def border_term(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return 1 + np.minimum(np.minimum(x, W - 1 - x), np.minimum(y, H - 1 - y))


def depth(code, border, max_depth=254):
    """What cvk_cheb_depth stores for one image: min(depth0, max_depth + 1), and the border term too with `border`; 0 off the classes."""
    d = np.minimum(depth0(code), max_depth + 1)
    if border:
        d = np.minimum(d, border_term(*code.shape))
    return np.where(code < 32, d, 0).astype(np.uint8)


def depth_maps(x, void_from, K, ignore, border, max_depth=254):
    """(code, depth) uint8 [N, H, W] of an int64 batch."""
    code = code_bytes(x, void_from, K, ignore)
    return code, np.stack([depth(c, border, max_depth) for c in code])


def counts(pred, label, K, ignore, d):
    """int64 [N, 6, K]: rows bG, bP, bI, aG, aP, aI (each image on its own)."""
    pred, label = np.asarray(pred, dtype=np.int64), np.asarray(label, dtype=np.int64)
    assert pred.shape == label.shape and pred.ndim == 3 and 1 <= K <= 32 and 1 <= d <= 254
    out = np.zeros((pred.shape[0], 6, K), dtype=np.int64)
    cP, cG = code_bytes(pred, label, K, ignore), code_bytes(label, label, K, ignore)
    for n in range(pred.shape[0]):
        bt = border_term(*cP[n].shape)
        dP, dG = np.minimum(depth0(cP[n]), bt), np.minimum(depth0(cG[n]), bt)
        for c in range(K):
            mP, mG = cP[n] == c, cG[n] == c
            bP, bG = mP & (dP <= d), mG & (dG <= d)
            out[n, :, c] = [bG.sum(), bP.sum(), (bG & bP).sum(), mG.sum(), mP.sum(), (mG & mP).sum()]
    return out


def trimap_bins(pred, label, K, ignore, widths):
    """int64 [nw, K, K]: a pixel whose label and masked prediction are classes adds 1 at [i, label, pred] for the smallest i with
    depth0 of the label <= widths[i]."""
    pred, label = np.asarray(pred, dtype=np.int64), np.asarray(label, dtype=np.int64)
    out = np.zeros((len(widths), K, K), dtype=np.int64)
    cP, cG = code_bytes(pred, label, K, ignore), code_bytes(label, label, K, ignore)
    for n in range(pred.shape[0]):
        dG = depth0(cG[n])
        ok = (cG[n] < K) & (cP[n] < K)
        lo = 0
        for i, w in enumerate(widths):
            sel = ok & (dG > lo) & (dG <= w)
            np.add.at(out[i], (cG[n][sel].astype(np.int64), cP[n][sel].astype(np.int64)), 1)
            lo = w
    return out


def _iou(i, a, b):
    return i / (a + b - i) if a + b - i > 0 else float("nan")


def scores(cnt, ignore):
    """{"biou", "biou_per_class", "biou_image", "min_iou_per_class", "images"} by loops in float64."""
    cnt = np.asarray(cnt, dtype=np.int64)
    K = cnt.shape[2]
    pooled = cnt.sum(axis=0) if len(cnt) else np.zeros((6, K), dtype=np.int64)
    per, mn = np.full(K, np.nan), np.full(K, np.nan)
    for c in range(K):
        if c == ignore:
            continue
        per[c] = _iou(int(pooled[2, c]), int(pooled[0, c]), int(pooled[1, c]))
        m = _iou(int(pooled[5, c]), int(pooled[3, c]), int(pooled[4, c]))
        if not math.isnan(per[c]) and not math.isnan(m):
            mn[c] = min(per[c], m)
    have = [v for v in per if not math.isnan(v)]
    image = []
    for c6 in cnt:
        vs = [_iou(int(c6[2, c]), int(c6[0, c]), int(c6[1, c])) for c in range(K) if c != ignore and c6[0, c] + c6[1, c] > 0]
        if vs:
            image.append(sum(vs) / len(vs))
    return {"biou": sum(have) / len(have) if have else float("nan"), "biou_per_class": per,
            "biou_image": sum(image) / len(image) if image else float("nan"), "min_iou_per_class": mn, "images": len(image)}


def trimap_scores(bins, widths, ignore):
    """{"trimap_miou", "trimap_accuracy", "trimap_pixels"} of the bins, by loops."""
    bins = np.asarray(bins, dtype=np.int64)
    K = bins.shape[1]
    miou, acc, pix = [], [], []
    for i in range(len(widths)):
        m = bins[:i + 1].sum(axis=0)
        ious = []
        for c in range(K):
            union = int(m[c, :].sum() + m[:, c].sum() - m[c, c])
            if c != ignore and union > 0:
                ious.append(int(m[c, c]) / union)
        tot = int(m.sum())
        miou.append(sum(ious) / len(ious) if ious else float("nan"))
        acc.append(int(np.trace(m)) / tot if tot else float("nan"))
        pix.append(tot)
    return {"trimap_miou": np.array(miou), "trimap_accuracy": np.array(acc), "trimap_pixels": np.array(pix, dtype=np.int64)}


def special_maps(H, W, K=12, ignore=11):
    """Named (pred, label) int64 [1, H, W] pairs that exercise the corners of the definition."""
    y, x = np.mgrid[0:H, 0:W]
    out = {}
    one = np.full((1, H, W), 3, dtype=np.int64)
    out["one_class"] = (one.copy(), one.copy())
    out["all_void"] = (one.copy(), np.full((1, H, W), ignore, dtype=np.int64))
    chk = ((x + y) % 2)[None].astype(np.int64)
    out["checkerboard"] = (1 - chk, chk)
    corner = np.zeros((1, H, W), dtype=np.int64)
    corner[0, H - 1, W - 1] = 5
    corner2 = np.zeros((1, H, W), dtype=np.int64)
    corner2[0, 0, 0] = 5
    out["corner_pixel"] = (corner2, corner)
    for w in (1, 2, 3):
        out[f"vstripes{w}"] = ((((x + 1) // w) % 3)[None].astype(np.int64), ((x // w) % 3)[None].astype(np.int64))
        out[f"hstripes{w}"] = ((((y + 1) // w) % 3)[None].astype(np.int64), ((y // w) % 3)[None].astype(np.int64))
    lab = ((x // 5 + y // 4) % 4)[None].astype(np.int64)
    prd = np.roll(lab, (1, 2), axis=(1, 2)).copy()
    lab[0, :max(1, H // 4), :max(1, W // 3)] = ignore                                 # a void block at the border
    lab[0, H // 2:H // 2 + max(1, H // 5), W // 2:W // 2 + max(1, W // 5)] = ignore   # and one inside
    out["void_blocks"] = (prd, lab)
    lab2 = ((x // 4 + y // 3) % 5)[None].astype(np.int64)
    bad = lab2.copy()
    vals = np.array([-1, K, 2 ** 32 + 3, ignore], dtype=np.int64)
    sel = ((x * 7 + y * 3) % 5 == 0)[None]
    bad[sel] = vals[((x + 2 * y) % 4)[None][sel]]
    out["bad_pred"] = (bad, lab2)
    return out
