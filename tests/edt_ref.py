"""Plain numpy / scipy restatement of the exact Euclidean distance transform of a label batch and of the boundary loss (Kervadec et
al., MIDL 2019) as include/cvk.h defines them for cvk_edt_squared / cvk_edt_signed / cvk_boundary_loss_fwd / _bwd, written from the
definition: no kernel code, no passes.

  Everything is per image.  A pixel's category is its label when 0 <= label < C and label != ignore_index, else void (-1).  A void
  pixel belongs to no class but is a pixel: it is "not class c" for every c, and it differs from every class pixel.
  to_class[y, x, c] = the squared distance from (y, x) to the nearest pixel of category c, -1 where the image has none.
  to_other[y, x]    = the squared distance to the nearest pixel of another category, -1 where there is none.
  phi[c, y, x]      = +sqrt(to_class) where the pixel's category is not c, -(sqrt(to_other) - 1) where it is, 0 where the needed
                      distance is -1; the root is the correctly rounded fp32 root of the integer.
  B = 1 / |V| sum_{q in V} sum_{c in S} phi_c(q) softmax(x)_c(q), V = the pixels whose target is not ignore_index; 0 for an empty V.
"""
import numpy as np


def categories(label, C, ignore):
    label = np.asarray(label, dtype=np.int64)
    return np.where((label >= 0) & (label < C) & (label != ignore), label, -1)


def _nearest_sq(present):
    """int32 [H, W]: squared distance to the nearest True pixel of the bool map `present` (which has one), via scipy."""
    from scipy import ndimage as ndi
    d = ndi.distance_transform_edt(~present)
    return np.rint(d * d).astype(np.int32)


def squared_maps(label, C, ignore):
    """(to_class int32 [H, W, C], to_other int32 [H, W]) of one image's int64 label map [H, W]."""
    k = categories(label, C, ignore)
    H, W = k.shape
    to_class = np.full((H, W, C), -1, dtype=np.int32)
    for c in range(C):
        if (k == c).any():
            to_class[:, :, c] = _nearest_sq(k == c)
    to_other = np.full((H, W), -1, dtype=np.int32)
    for v in np.unique(k):
        if (k != v).any():
            to_other[k == v] = _nearest_sq(k != v)[k == v]
    return to_class, to_other


def squared_maps_brute(label, C, ignore):
    """The same by the O((HW)^2) definition, for tiny maps."""
    k = categories(label, C, ignore)
    H, W = k.shape
    ys, xs = np.mgrid[0:H, 0:W]
    d2 = (ys.reshape(-1, 1) - ys.reshape(1, -1)) ** 2 + (xs.reshape(-1, 1) - xs.reshape(1, -1)) ** 2      # [from, to]
    kf = k.reshape(-1)
    big = np.iinfo(np.int64).max
    to_class = np.full((H * W, C), -1, dtype=np.int32)
    for c in range(C):
        if (kf == c).any():
            to_class[:, c] = np.where(kf[None, :] == c, d2, big).min(axis=1)
    differs = kf[:, None] != kf[None, :]
    best = np.where(differs, d2, big).min(axis=1)
    to_other = np.where(differs.any(axis=1), best, -1).astype(np.int32)
    return to_class.reshape(H, W, C), to_other.reshape(H, W)


def signed_from_squared(label, to_class, to_other, C, ignore):
    """float32 [C, H, W] phi of one image from its integer maps."""
    k = categories(label, C, ignore)
    out = np.sqrt(np.maximum(to_class, 0).astype(np.float32))
    out[to_class < 0] = 0.0
    inside = -(np.sqrt(np.maximum(to_other, 0).astype(np.float32)) - np.float32(1.0))
    inside[to_other < 0] = 0.0
    for c in range(C):
        out[:, :, c] = np.where(k == c, inside, out[:, :, c])
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def batch_maps(labels, C, ignore, brute=False):
    """(to_class [N,H,W,C], to_other [N,H,W], phi [N,C,H,W]) of an int64 batch [N,H,W]; every image is computed alone."""
    f = squared_maps_brute if brute else squared_maps
    tc, to, phi = [], [], []
    for lab in np.asarray(labels):
        a, b = f(lab, C, ignore)
        tc.append(a); to.append(b); phi.append(signed_from_squared(lab, a, b, C, ignore))
    return np.stack(tc), np.stack(to), np.stack(phi)


def _softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def loss_and_grad(logits, target, phi, boundary=1.0, ce=0.0, classes=None, weight=None, ignore=-100):
    """fp64: {"loss", "B", "H", "class_terms" [C], "mag" (1 / |V| sum |phi_c| p_c over V and S), "grad" [N,C,H,W], "valid"} of logits
    [N,C,H,W], int64 target [N,H,W] (every target a class or `ignore`) and phi [N,C,H,W], with the analytic gradient of the contract."""
    x = np.asarray(logits, dtype=np.float64)
    t = np.asarray(target, dtype=np.int64)
    f = np.asarray(phi, dtype=np.float64)
    N, C, H, W = x.shape
    S = np.zeros(C, dtype=bool)
    S[list(range(C)) if classes is None else list(classes)] = True
    w = np.ones(C) if weight is None else np.asarray(weight, dtype=np.float64)
    p = _softmax64(x)
    valid = t != ignore
    V = int(valid.sum())
    vm = valid[:, None, :, :]
    fs = f * S[None, :, None, None]
    grad = np.zeros_like(x)
    if V > 0 and boundary > 0:
        class_terms = (fs * p * vm).sum(axis=(0, 2, 3)) / V
        mag = (np.abs(fs) * p * vm).sum() / V
        dot = (fs * p).sum(axis=1, keepdims=True)
        grad += boundary * p * (fs - dot) * vm / V
    else:
        class_terms, mag = np.zeros(C), 0.0
    B = float(class_terms.sum())
    Hce = 0.0
    if ce > 0:
        tt = np.where(valid, t, 0)
        pt = np.take_along_axis(p, tt[:, None], axis=1)[:, 0]
        wt = w[tt] * valid
        div = wt.sum()
        Hce = float((-(np.log(pt)) * wt).sum() / div) if V > 0 else float("nan")
        onehot = np.zeros_like(x)
        np.put_along_axis(onehot, tt[:, None], 1.0, axis=1)
        if V > 0:
            grad += ce * wt[:, None] * (p - onehot) / div
    return {"loss": boundary * B + (ce * Hce if ce > 0 else 0.0), "B": B, "H": Hce, "class_terms": class_terms, "mag": float(mag),
            "grad": grad, "valid": V}


def special_maps(H, W, C=12, ignore=11):
    """Named int64 maps [H, W] that take the distance transform's special paths."""
    one = np.full((H, W), 3, dtype=np.int64)
    corner = np.zeros((H, W), dtype=np.int64)
    corner[H - 1, W - 1] = 5
    ys, xs = np.mgrid[0:H, 0:W]
    checker = ((ys + xs) % 2).astype(np.int64)
    stripe = np.full((H, W), 2, dtype=np.int64)
    stripe[:, W // 2] = ignore
    allvoid = np.full((H, W), ignore, dtype=np.int64)
    out_of_range = np.zeros((H, W), dtype=np.int64)
    out_of_range[H // 2:, :] = 1
    out_of_range[0, 0] = C + 5
    out_of_range[H - 1, 0] = -3
    out_of_range[H // 2, W // 2] = 2 ** 40
    return {"one_class": one, "corner_pixel": corner, "checkerboard": checker, "void_stripe": stripe, "all_void": allvoid,
            "out_of_range": out_of_range}
