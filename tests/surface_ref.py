"""Plain numpy restatement of the surface distances as include/cvk.h defines them for cvk_surface_distances, written from the
definition: no kernel code, no tiles, no histograms.  Everything is integer and exact; each image is computed alone.

  The contour pixels of class c of a map are those of tests/boundary_ref.boundary_map (the prediction masked by the label's void
  pixels).  For a contour pixel z of class c of map A, d2(z) = min over the contour pixels z' of class c of map B of |z - z'|^2, -1
  when B has none.  Per (image, direction, class): n, m, max d2, Q = sum isqrt(d2 << 32), k = (n - 1) qnum // qden,
  r = (n - 1) qnum % qden, d2_lo = sorted[k], d2_hi = sorted[min(k + 1, n - 1)] if r else d2_lo; a segment is evaluated iff n, m > 0.
"""
import math

import numpy as np

from tests import boundary_ref as B

SLOTS = 8


def nearest_d2_scipy(src, dst):
    """int64 squared distances from the True pixels of `src` to the nearest True pixel of `dst` ([H, W] bool), in src's row-major order;
    scipy's exact Euclidean feature transform names the nearest pixel, the squared distance is made from its integer coordinates."""
    from scipy import ndimage
    ys, xs = np.nonzero(src)
    if not dst.any():
        return np.full(len(ys), -1, dtype=np.int64)
    iy, ix = ndimage.distance_transform_edt(~dst, return_distances=False, return_indices=True)
    dy, dx = iy[ys, xs].astype(np.int64) - ys, ix[ys, xs].astype(np.int64) - xs
    return dy * dy + dx * dx


def nearest_d2_brute(src, dst):
    """The same by the O((H W)^2) definition."""
    ys, xs = np.nonzero(src)
    ty, tx = np.nonzero(dst)
    if len(ty) == 0:
        return np.full(len(ys), -1, dtype=np.int64)
    out = np.empty(len(ys), dtype=np.int64)
    for i, (y, x) in enumerate(zip(ys.tolist(), xs.tolist())):
        out[i] = min((y - int(a)) ** 2 + (x - int(b)) ** 2 for a, b in zip(ty, tx))
    return out


def segment_record(d2, m, qnum, qden):
    """The eight slots of a segment from its distances (int64 [n]) and the other map's count."""
    n = len(d2)
    rec = np.array([n, m, -1, 0, -1, -1, -1, -1], dtype=np.int64)
    if n > 0 and m > 0:
        s = np.sort(d2)
        k, r = divmod((n - 1) * qnum, qden)
        rec[2] = s[-1]
        rec[3] = sum(math.isqrt(int(v) << 32) for v in d2)
        rec[4], rec[5], rec[6] = k, r, s[k]
        rec[7] = s[min(k + 1, n - 1)] if r > 0 else s[k]
    return rec


def surface(pred, label, K, ignore, qnum, qden, nearest=nearest_d2_scipy):
    """(d2 int32 [2, N, H, W], record int64 [N, 2, K, 8]) of int64 maps [N, H, W]."""
    pred, label = np.asarray(pred, dtype=np.int64), np.asarray(label, dtype=np.int64)
    assert pred.shape == label.shape and pred.ndim == 3 and 1 <= K <= 32 and 0 <= qnum <= qden
    N, H, W = pred.shape
    d2 = np.full((2, N, H, W), -2, dtype=np.int32)
    rec = np.zeros((N, 2, K, SLOTS), dtype=np.int64)
    for n in range(N):
        maps = (B.boundary_map(pred[n], label[n], K, ignore), B.boundary_map(label[n], label[n], K, ignore))
        for direction in range(2):
            src, dst = maps[direction], maps[1 - direction]
            for c in range(K):
                v = nearest(src == c, dst == c)
                d2[direction, n][src == c] = v
                rec[n, direction, c] = segment_record(v, int((dst == c).sum()), qnum, qden)
    return d2, rec
