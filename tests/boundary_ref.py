"""Plain numpy restatement of the boundary F1 measure (BF score; Csurka et al., BMVC 2013) as include/cvk.h defines it for
cvk_boundary_counts / cvk_boundary_map, written from the definition: no kernel code, no tiles.  Everything is integer and exact.

  A pixel is void iff label == ignore_index, in both maps.  A non-void pixel z of a map X is a boundary pixel of class c iff X(z) = c,
  0 <= c < K, c != ignore_index, and a 4-neighbour inside the image is non-void with X != c.  Any other non-void value carries no
  boundary and is "different" for its neighbours.  A boundary pixel of class c of map A is matched iff map B has a boundary pixel of
  class c at an integer offset (dy, dx) with dy^2 + dx^2 <= r2 inside the image.
"""
import math

import numpy as np

NONE = 255          # boundary byte of a pixel that carries no boundary
_OTHER, _VOID = -1, -2


def codes(x, void_from, K, ignore):
    """int64 maps [..., H, W] -> int16 codes: the class, _OTHER for a non-void value that is no class, _VOID."""
    x, v = np.asarray(x, dtype=np.int64), np.asarray(void_from, dtype=np.int64)
    is_class = (x >= 0) & (x < K) & (x != ignore)
    c = np.where(is_class, x, _OTHER).astype(np.int16)
    return np.where(v == ignore, np.int16(_VOID), c)


def _shift(a, dy, dx, fill):
    """out[..., y, x] = a[..., y + dy, x + dx], `fill` where that lies outside the image."""
    H, W = a.shape[-2:]
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if abs(dy) < H and abs(dx) < W:
        out[..., yd, xd] = a[..., ys, xs]
    return out


def boundary_map(x, void_from, K, ignore):
    """uint8 [..., H, W]: the class whose boundary each pixel of the int64 map x carries, NONE (255) where it carries none.
    `void_from`: the label map whose ignore pixels are void (x itself for a label map)."""
    c = codes(x, void_from, K, ignore)
    diff = np.zeros(c.shape, dtype=bool)
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        nb = _shift(c, dy, dx, _VOID)
        diff |= (nb != _VOID) & (nb != c)
    return np.where((c >= 0) & diff, c, NONE).astype(np.uint8)


def disc(r2):
    R = math.isqrt(r2)
    return [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if dy * dy + dx * dx <= r2]


def matched(bA, bB, r2):
    """bool [..., H, W]: boundary pixels of bA with a boundary pixel of the same class in bB within the disc."""
    hit = np.zeros(bA.shape, dtype=bool)
    for dy, dx in disc(r2):
        hit |= _shift(bB, dy, dx, NONE) == bA
    return hit & (bA != NONE)


def counts(pred, label, K, ignore, r2):
    """int64 [N, 4, K] of int64 maps [N, H, W]: rows nP, mP, nG, mG (each image on its own)."""
    pred, label = np.asarray(pred, dtype=np.int64), np.asarray(label, dtype=np.int64)
    assert pred.shape == label.shape and pred.ndim == 3 and 1 <= K <= 32 and 0 <= r2
    out = np.zeros((pred.shape[0], 4, K), dtype=np.int64)
    for n in range(pred.shape[0]):
        bP, bG = boundary_map(pred[n], label[n], K, ignore), boundary_map(label[n], label[n], K, ignore)
        mP, mG = matched(bP, bG, r2), matched(bG, bP, r2)
        for c in range(K):
            out[n, 0, c], out[n, 1, c] = (bP == c).sum(), (mP & (bP == c)).sum()
            out[n, 2, c], out[n, 3, c] = (bG == c).sum(), (mG & (bG == c)).sum()
    return out


def _f(nP, mP, nG, mG):
    P = mP / nP if nP else 0.0
    R = mG / nG if nG else 0.0
    return P, R, (2.0 * P * R / (P + R) if P + R > 0 else 0.0)


def _image_score(c4):
    fs = [_f(*[int(c4[r, c]) for r in range(4)])[2] for c in range(c4.shape[1]) if c4[0, c] + c4[2, c] > 0]
    return sum(fs) / len(fs) if fs else float("nan")


def scores(cnt, ignore):
    """The host aggregation, by loops in float64: {"bf", "bf_per_class", "precision", "recall", "pooled", "images"}."""
    cnt = np.asarray(cnt, dtype=np.int64)
    K = cnt.shape[2]
    image = [_image_score(c4) for c4 in cnt]
    image = [s for s in image if not math.isnan(s)]
    per = np.full((3, K), np.nan)
    for c in range(K):
        if c == ignore:
            continue
        rows = [_f(*[int(c4[r, c]) for r in range(4)]) for c4 in cnt if c4[0, c] + c4[2, c] > 0]
        if rows:
            per[:, c] = [sum(r[k] for r in rows) / len(rows) for k in range(3)]
    return {"bf": sum(image) / len(image) if image else float("nan"), "bf_per_class": per[2], "precision": per[0], "recall": per[1],
            "pooled": _image_score(cnt.sum(axis=0)) if len(cnt) else float("nan"), "images": len(image)}


def blocky_maps(seed, N, H, W, K=12, ignore=11, cell=(7, 9), shift=(2, -2), noise=0.03, void=0.05):
    """(pred, label) int64 [N, H, W]: label = a coarse random class grid enlarged by `cell`; pred = the label shifted by `shift` with
    `noise` of its pixels redrawn; then `void` of the label pixels become `ignore`.  Classes are drawn from the non-ignored ones."""
    rng = np.random.default_rng(seed)
    classes = np.array([c for c in range(K) if c != ignore])
    gh, gw = -(-H // cell[0]) + 1, -(-W // cell[1]) + 1
    coarse = classes[rng.integers(0, len(classes), size=(N, gh, gw))]
    label = np.repeat(np.repeat(coarse, cell[0], axis=1), cell[1], axis=2)[:, :H, :W].astype(np.int64)
    pred = np.roll(label, shift, axis=(1, 2)).copy()
    redraw = rng.random((N, H, W)) < noise
    pred[redraw] = classes[rng.integers(0, len(classes), size=int(redraw.sum()))]
    label = label.copy()
    label[rng.random((N, H, W)) < void] = ignore
    return pred, label
