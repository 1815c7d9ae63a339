"""Restatement of connected-component labelling and small-region removal (include/cvk.h, cvk_cc_label / cvk_cc_filter) in numpy and
scipy, for the tests: scipy.ndimage.label per code with the 4- or 8-structure, canonicalised to the row-major index of a component's
first pixel, areas from bincount; the filter and the record by brute force over the components.  `bfs_labels` is a second, plain
restatement of the labelling that the CPU tests hold this one against.  Map makers for the GPU tests are at the end."""
import numpy as np
from scipy import ndimage

VOID = -1
RECORD_SLOTS = 8
NEIGHBOURS = {4: ((-1, 0), (0, -1), (0, 1), (1, 0)), 8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}
STRUCTURE = {4: np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]]), 8: np.ones((3, 3), dtype=int)}


def codes(x, K, ignore):
    """int64 maps -> int64 codes: the class, VOID (-1) for every other value."""
    x = np.asarray(x, dtype=np.int64)
    return np.where((x >= 0) & (x < K) & (x != ignore), x, VOID)


def label_image(c, connectivity):
    """(labels, area) int32 [H, W] of one image of codes."""
    H, W = c.shape
    index = np.arange(H * W, dtype=np.int64).reshape(H, W)
    labels = np.zeros((H, W), dtype=np.int64)
    for code in np.unique(c):
        lab, n = ndimage.label(c == code, structure=STRUCTURE[connectivity])
        if n == 0:
            continue
        first = np.asarray(ndimage.minimum(index, lab, np.arange(1, n + 1)), dtype=np.int64).reshape(-1)
        labels = np.where(lab > 0, first[np.maximum(lab, 1) - 1], labels)
    area = np.bincount(labels.ravel(), minlength=H * W)[labels]
    return labels.astype(np.int32), area.astype(np.int32)


def connected_components(x, K, ignore, connectivity):
    """(labels, area) int32 [N, H, W] of int64 maps [N, H, W]."""
    c = codes(x, K, ignore)
    pairs = [label_image(c[n], connectivity) for n in range(c.shape[0])]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def bfs_labels(c, connectivity):
    """(labels, area) of one image of codes by a breadth-first search from every pixel in row-major order."""
    H, W = c.shape
    labels = np.full((H, W), -1, dtype=np.int64)
    area = np.zeros((H, W), dtype=np.int64)
    for y0 in range(H):
        for x0 in range(W):
            if labels[y0, x0] >= 0:
                continue
            labels[y0, x0] = y0 * W + x0
            todo, seen = [(y0, x0)], [(y0, x0)]
            while todo:
                y, x = todo.pop()
                for dy, dx in NEIGHBOURS[connectivity]:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and labels[yy, xx] < 0 and c[yy, xx] == c[y0, x0]:
                        labels[yy, xx] = y0 * W + x0
                        todo.append((yy, xx))
                        seen.append((yy, xx))
            for y, x in seen:
                area[y, x] = len(seen)
    return labels.astype(np.int32), area.astype(np.int32)


def filter_regions(x, K, ignore, connectivity, min_area, mode, fill_value=None):
    """(out int64 [N, H, W], record int64 [N, K, 8]) of int64 maps [N, H, W]; slots: components, pixels, largest area, small components,
    small pixels, small components changed, pixels received from other classes, isolated small components.  Every ordered pair (pixel
    of a small class component, neighbour inside the image that is a class pixel of a component that is not small) is one vote."""
    assert mode in ("fill", "neighbor") and min_area >= 1
    x = np.asarray(x, dtype=np.int64)
    fill_value = ignore if fill_value is None else fill_value
    c = codes(x, K, ignore)
    labels, area = connected_components(x, K, ignore, connectivity)
    out = x.copy()
    N, H, W = x.shape
    record = np.zeros((N, K, RECORD_SLOTS), dtype=np.int64)
    fill_code = int(codes(np.array([fill_value]), K, ignore)[0])
    for n in range(N):
        cn, ln, an = c[n], labels[n].astype(np.int64), area[n].astype(np.int64)
        is_class = cn >= 0
        small = is_class & (an < min_area)
        voter = is_class & ~small
        votes = np.zeros((H * W, K), dtype=np.int64)
        for dy, dx in NEIGHBOURS[connectivity]:
            ps = (slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx)))
            qs = (slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx)))
            pair = small[ps] & voter[qs]
            np.add.at(votes, (ln[ps][pair], cn[qs][pair]), 1)
        roots = np.nonzero((ln.ravel() == np.arange(H * W)) & is_class.ravel())[0]
        rk, ra = cn.ravel()[roots], an.ravel()[roots]
        rec = record[n]
        np.add.at(rec[:, 0], rk, 1)
        np.add.at(rec[:, 1], rk, ra)
        np.maximum.at(rec[:, 2], rk, ra)
        sm = ra < min_area
        np.add.at(rec[:, 3], rk[sm], 1)
        np.add.at(rec[:, 4], rk[sm], ra[sm])
        target = np.full(H * W, -1, dtype=np.int64)        # per root: the value its component takes, -1: it stays
        if mode == "fill":
            changed = sm & (rk != fill_value)
            target[roots[changed]] = fill_value
            received = np.full(roots.shape, fill_code)
        else:
            v = votes[roots]
            changed = sm & (v.max(axis=1) > 0)
            received = v.argmax(axis=1)                    # the first maximum: ties go to the smallest class
            target[roots[changed]] = received[changed]
            np.add.at(rec[:, 7], rk[sm & ~changed], 1)
        np.add.at(rec[:, 5], rk[changed], 1)
        got = changed & (received >= 0)
        np.add.at(rec[:, 6], received[got], ra[got])
        moved = small & (target[ln] >= 0 if mode == "neighbor" else np.isin(ln, roots[changed]))
        out[n][moved] = target[ln][moved]
    return out, record


def meter_sums(pred, label, K, ignore, connectivity, min_area, mode):
    """(record of the prediction pooled over the images [K, 8], the label's, confusion counts [3, K] of the filtered prediction)."""
    filtered, rec_p = filter_regions(pred, K, ignore, connectivity, min_area, mode)
    _, rec_l = filter_regions(label, K, ignore, connectivity, 1, "fill")
    rp, rl = rec_p.sum(0), rec_l.sum(0)
    rp[:, 2], rl[:, 2] = rec_p[:, :, 2].max(0), rec_l[:, :, 2].max(0)
    hist = np.zeros((3, K), dtype=np.int64)
    keep = label != ignore
    for k in range(K):
        hist[0, k] = ((filtered == k) & (label == k) & keep).sum()
        hist[1, k] = ((filtered == k) & keep).sum()
        hist[2, k] = ((label == k) & keep).sum()
    return rp, rl, hist


# ---- maps ---------------------------------------------------------------------------------------------------------------------------

def spiral(H, W):
    """a one-pixel-wide spiral of class 1 on class 0 from the top left corner inwards, its turns one pixel apart: a walker turns right
    when the pixel ahead is outside or the one after it is already on the path"""
    m = np.zeros((H, W), dtype=np.int64)
    y, x, d = 0, 0, 0
    step = ((0, 1), (1, 0), (0, -1), (-1, 0))
    m[0, 0] = 1

    def free(y, x, d):
        y1, x1, y2, x2 = y + step[d][0], x + step[d][1], y + 2 * step[d][0], x + 2 * step[d][1]
        if not (0 <= y1 < H and 0 <= x1 < W) or m[y1, x1]:
            return False
        return not (0 <= y2 < H and 0 <= x2 < W) or not m[y2, x2]

    turns = 0
    while turns < 2:
        if free(y, x, d):
            y, x = y + step[d][0], x + step[d][1]
            m[y, x] = 1
            turns = 0
        else:
            d = (d + 1) % 4
            turns += 1
    return m


def serpentine(H, W):
    """class 1 on every other row, joined alternately at the right and the left end: one long path from the first pixel to the last"""
    m = np.zeros((H, W), dtype=np.int64)
    m[0::2] = 1
    for i, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if i % 2 == 0 else 0] = 1
    return m


def comb(H, W):
    """teeth of class 1 on every other column that join only in the last row"""
    m = np.zeros((H, W), dtype=np.int64)
    m[:, 0::2] = 1
    m[H - 1, :] = 1
    return m


def checkerboard(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return ((y + x) & 1).astype(np.int64)


def random_two_class(seed, N, H, W, p):
    return (np.random.default_rng(seed).random((N, H, W)) < p).astype(np.int64)


def speckled(seed, N, H, W, K=12, ignore=11, cell=(24, 32), speck=0.02):
    """large class cells with single-pixel and small-blob specks of other classes: what an arg-max map looks like"""
    rng = np.random.default_rng(seed)
    classes = np.array([c for c in range(K) if c != ignore])
    gh, gw = -(-H // cell[0]) + 1, -(-W // cell[1]) + 1
    coarse = classes[rng.integers(0, len(classes), size=(N, gh, gw))]
    m = np.repeat(np.repeat(coarse, cell[0], axis=1), cell[1], axis=2)[:, :H, :W].astype(np.int64)
    hit = rng.random((N, H, W)) < speck
    hit |= np.roll(hit, 1, axis=2) & (rng.random((N, H, W)) < 0.5)
    m[hit] = classes[rng.integers(0, len(classes), size=int(hit.sum()))]
    return m
