"""Plain numpy restatements of the image-ingest and evaluation entry points, written from their definitions for the tests
(include/cvk.h: cvk_import_nchw, cvk_export_nchw, cvk_zero_frame, cvk_preprocess_u8, cvk_argmax_channels, cvk_confusion_accumulate;
meters.py: ConfusionMeter.compute / precision_recall), and the seeded inputs the CPU and the GPU tests share.  Nothing here
touches a GPU or imports the package.

  import       dst[n][y][x][c] = src[n][c][y][x] for c < C, +0.0 for C <= c < ld          pure data movement: any dtype, so the
  export       dst[n][c][y][x] = src[n][y][x][c] for c < C; the pad channels go nowhere   tests hand over int32 BIT PATTERNS
  zero frame   channels [0, C) of every pixel outside [y0, y0+h) x [x0, x0+w) become +0.0
  preprocess   (v/255 - mean[c]) / std[c] in fp64, mean and std rounded to float32 first (the ABI takes float)
  arg-max      first maximum; the first NaN beats everything (ATen's rule)
  confusion    pixels with label == ignore dropped; intersection = #(pred == label, 0 <= pred < K) per class, prediction area =
               #(pred in [0, K)), label area = #(label in [0, K)), all compared as 64-bit integers
  metrics      iou = inter / (pred + label - inter), mIoU = nanmean over the classes != ignore, acc = inter.sum() / max(label.sum(), 1),
               precision = mean inter / (pred + 1e-15), recall = mean inter / (label + 1e-15) over the classes != ignore"""
import numpy as np

U32 = 2.0 ** -24                      # unit roundoff of fp32
TWO32 = 2 ** 32


# ------------------------------------------------------------------------------------------------ layout
def import_nchw_ref(src, ld):
    """src: logical [N,C,H,W] array of any strides -> dense [N,H,W,ld], channels [C, ld) zero (bit pattern 0 = +0.0)."""
    N, C, H, W = src.shape
    assert ld >= C
    out = np.zeros((N, H, W, ld), dtype=src.dtype)
    for c in range(C):
        out[:, :, :, c] = src[:, c, :, :]
    return out


def export_nchw_ref(nhwc, C):
    """nhwc: dense [N,H,W,ld] -> logical [N,C,H,W] (a fresh dense array); channels [C, ld) are dropped."""
    N, H, W, ld = nhwc.shape
    assert ld >= C
    out = np.empty((N, C, H, W), dtype=nhwc.dtype)
    for c in range(C):
        out[:, c, :, :] = nhwc[:, :, :, c]
    return out


def zero_frame_ref(buf, C, y0, x0, h, w):
    """buf: [N,H,W,>=C] -> copy with channels [0, C) zeroed (bit pattern 0) at every pixel outside the window; the window and the
    channels from C on keep their values."""
    N, H, W, _ = buf.shape
    out = buf.copy()
    for y in range(H):
        for x in range(W):
            if not (y0 <= y < y0 + h and x0 <= x < x0 + w):
                out[:, y, x, :C] = 0
    return out


# ------------------------------------------------------------------------------------------------ preprocess
def _f32_as_f64(v3):
    return np.asarray(v3, dtype=np.float32).astype(np.float64)


def preprocess_ref(u8, mean3, std3):
    """u8: uint8 [..., 3] -> float64 [..., 3]: (v/255 - mean[c]) / std[c] with the float32-rounded constants, exact otherwise."""
    assert u8.dtype == np.uint8 and u8.shape[-1] == 3
    return (u8.astype(np.float64) / 255.0 - _f32_as_f64(mean3)) / _f32_as_f64(std3)


def preprocess_bound(u8, mean3, std3):
    """|fp32 result - preprocess_ref| <= 6 u (v/255 + |mean_c|) / std_c, u = 2^-24, for the expression
    ((float)v * (1.f/255.f) - m) * (1.f/std) evaluated in float32 with or without the multiply-subtract fused.

    With q = v/255 and every |e_i| <= u:  fl(1/255) = (1+e1)/255,  t1 = fl(v * fl(1/255)) = q (1+e1)(1+e2),  t2 = fl(t1 - m) =
    (t1 - m)(1+e3),  r = fl(1/std) = (1+e4)/std,  result = fl(t2 r) = t2 r (1+e5).  To first order
        result - (q - m)/std = [q (e1 + e2) + (q - m)(e3 + e4 + e5)] / std,
    at most (2 q + 3 |q - m|) u / std <= 5 u (q + |m|) / std; the sixth u covers the second-order terms.  A fused
    multiply-subtract drops e2.  Nothing under- or overflows: q - m is either 0 or at least one ulp of a number near 1."""
    q = u8.astype(np.float64) / 255.0
    return 6.0 * U32 * (q + np.abs(_f32_as_f64(mean3))) / np.abs(_f32_as_f64(std3))


def preprocess_f32_rounded(u8, mean3, std3):
    """The kernel's expression in float32 numpy, rounded after every operation."""
    m, s = np.asarray(mean3, dtype=np.float32), np.asarray(std3, dtype=np.float32)
    c255 = np.float32(1.0) / np.float32(255.0)
    r = np.float32(1.0) / s
    return (u8.astype(np.float32) * c255 - m) * r


def preprocess_f32_fused(u8, mean3, std3):
    """The same with v * (1/255) - m evaluated in fp64 and rounded once: what an FMA contraction computes (v * fl(1/255) is exact
    in fp64: 8 x 24 bits)."""
    m, s = np.asarray(mean3, dtype=np.float32), np.asarray(std3, dtype=np.float32)
    c255 = np.float32(1.0) / np.float32(255.0)
    r = np.float32(1.0) / s
    t = (u8.astype(np.float64) * np.float64(c255) - m.astype(np.float64)).astype(np.float32)
    return t * r


def preprocess_all_values():
    """uint8 [1,16,16,3] holding each of the 256 values once per channel, in a different order per channel (a kernel that swaps
    or repeats a channel cannot pass), and the three orders."""
    perms = [np.arange(256), (np.arange(256) * 37 + 11) % 256, (np.arange(256) * 91 + 200) % 256]
    for p in perms:
        assert np.array_equal(np.sort(p), np.arange(256))
    img = np.stack(perms, axis=-1).astype(np.uint8).reshape(1, 16, 16, 3)
    return img, perms


# ------------------------------------------------------------------------------------------------ arg-max
def argmax_ref_loop(rows):
    """rows: [M, C] float -> int64 [M].  The definition, row by row."""
    M, C = rows.shape
    out = np.zeros(M, dtype=np.int64)
    for m in range(M):
        best, bi = rows[m, 0], 0
        for c in range(1, C):
            v = rows[m, c]
            if np.isnan(best):
                break                                     # the first NaN is final
            if np.isnan(v) or v > best:
                best, bi = v, c
        out[m] = bi
    return out


def argmax_ref(rows):
    """The same, vectorised: the index of the first NaN where a row has one, else of the first element equal to the row maximum."""
    nan = np.isnan(rows)
    clean = np.where(nan, -np.inf, rows)
    first_max = (clean == clean.max(axis=1, keepdims=True)).argmax(axis=1)     # argmax of booleans: the first True
    return np.where(nan.any(axis=1), nan.argmax(axis=1), first_max).astype(np.int64)


ARGMAX_CASES = ("all_equal", "dup2", "dup3", "negzero_first", "poszero_first", "inf_once", "inf_twice", "all_neginf",
                "nan_first", "nan_middle", "nan_last", "nan_twice", "nan_after_inf")


def argmax_case_row(name, C, base):
    """One planted row of C channels over `base` (finite float32 [C] in (-4, 4)) and the index that must win, or None when C is
    too small for the case."""
    r = base.astype(np.float32).copy()
    a, mid, hi = C // 3, C // 2, C - 1                    # a < hi whenever C >= 2
    if name == "all_equal":
        r[:] = 1.5
        return r, 0
    if name == "inf_once":
        r[mid] = np.inf
        return r, mid
    if name == "all_neginf":
        r[:] = -np.inf
        return r, 0
    if name == "nan_first":
        r[0] = np.nan
        return r, 0
    if C < 2:
        return None
    if name == "dup2":
        r[[a, hi]] = 9.0
        return r, a
    if name in ("negzero_first", "poszero_first"):
        r = -np.abs(r) - 0.5
        r[a], r[hi] = (-0.0, 0.0) if name == "negzero_first" else (0.0, -0.0)
        return r, a                                        # -0.0 == +0.0: the first of the two wins either way
    if name == "inf_twice":
        r[[a, hi]] = np.inf
        return r, a
    if name == "nan_last":
        r[hi] = np.nan
        return r, hi
    if name == "nan_twice":
        r[[a, hi]] = np.nan
        return r, a
    if name == "nan_after_inf":
        r[a], r[hi] = np.inf, np.nan
        return r, hi
    if C < 3:
        return None
    if name == "dup3":
        r[[0, mid, hi]] = 9.0
        return r, 0
    if name == "nan_middle":
        r[mid] = np.nan
        return r, mid
    raise KeyError(name)


ARGMAX_PADS = (np.inf, np.nan, np.inf)
ARGMAX_GRID_CAP = 8192 * 256           # rows one sweep of cvk_argmax_channels' capped grid covers


def argmax_rows(M, C, ld, seed, shift=0):
    """float32 [M, ld] rows and {row index: (case, winning index)} of the planted ones.  Values are multiples of 1/4 in [-4, 4], so
    ties also occur at random; the pad columns [C, ld) hold +inf, NaN, +inf, ...; the planted rows sit at 0, M-1, 255, 256 and
    8192*256 (where M reaches them) and at every ~M/61-th row, cycling through ARGMAX_CASES from case number `shift` on."""
    rng = np.random.default_rng(seed)
    rows = (np.round(rng.uniform(-4.0, 4.0, size=(M, ld)) * 4.0) / 4.0).astype(np.float32)
    for j in range(C, ld):
        rows[:, j] = ARGMAX_PADS[(j - C) % 3]
    where = [p for p in (0, M - 1, 255, 256, ARGMAX_GRID_CAP) if 0 <= p < M]
    where += list(range(3, M, max(1, M // 61)))
    planted, k = {}, shift
    for p in where:
        if p in planted:
            continue
        for _ in range(len(ARGMAX_CASES)):
            name = ARGMAX_CASES[k % len(ARGMAX_CASES)]
            k += 1
            made = argmax_case_row(name, C, rows[p, :C])
            if made is not None:
                rows[p, :C] = made[0]
                planted[p] = (name, made[1])
                break
    return rows, planted


# ------------------------------------------------------------------------------------------------ confusion counts and metrics
def confusion_ref(pred, label, K, ignore):
    """int64 [3][K]: intersection, prediction area, label area."""
    p = np.asarray(pred, dtype=np.int64).ravel()
    l = np.asarray(label, dtype=np.int64).ravel()
    keep = l != np.int64(ignore)
    p, l = p[keep], l[keep]
    p_in = (p >= 0) & (p < K)
    l_in = (l >= 0) & (l < K)
    hist = np.zeros((3, K), dtype=np.int64)
    hist[0] = np.bincount(p[p_in & (p == l)], minlength=K)
    hist[1] = np.bincount(p[p_in], minlength=K)
    hist[2] = np.bincount(l[l_in], minlength=K)
    return hist


def _valid(K, ignore):
    return [c for c in range(K) if c != ignore]


def miou_ref(hist, ignore):
    """(acc, iou float64 [K], mIoU) of ConfusionMeter.compute's docstring; a class in neither pred nor label has IoU NaN and is
    left out of the mean; with no class left the mean is NaN."""
    h = np.asarray(hist, dtype=np.float64)
    inter, pred, lab = h[0], h[1], h[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / (pred + lab - inter)
    v = iou[_valid(h.shape[1], ignore)]
    v = v[~np.isnan(v)]
    miou = float(v.mean()) if v.size else float("nan")
    return float(inter.sum() / max(lab.sum(), 1.0)), iou, miou


def precision_recall_ref(hist, ignore):
    h = np.asarray(hist, dtype=np.float64)
    valid = _valid(h.shape[1], ignore)
    return float((h[0] / (h[1] + 1e-15))[valid].mean()), float((h[0] / (h[2] + 1e-15))[valid].mean())


def confusion_planted_pairs(K, ignore):
    """(pred, label) pixels outside the everyday range: values just outside [0, K), the usual ignore codes, and 64-bit values whose
    low 32 bits are a class or the ignore index.  c and d are two classes (equal when K == 1)."""
    c, d = K // 2, K - 1
    odd = [-1, K, 255, -100, TWO32 + c, TWO32 + ignore, -TWO32 + c]
    pairs = []
    for v in odd:
        pairs += [(v, d), (d, v), (v, v)]
    pairs += [(c, TWO32 + c), (TWO32 + c, c), (-TWO32 + c, c), (c, -TWO32 + c),      # low words agree, the values do not
              (c, TWO32 + ignore), (d, TWO32 + ignore), (ignore, TWO32 + ignore),   # not the ignore index: pred still counts
              (c, ignore), (TWO32 + c, ignore)]                                     # the ignore index: nothing counts
    return pairs


def confusion_inputs(M, K, ignore, seed, kind="random"):
    """int64 pred, label [M].  random: classes in [0, K), agreeing about half the time; planted: the same with
    confusion_planted_pairs spread over the image (all of them when M allows, else the first M); constant: one class (not the ignored one) everywhere;
    ignored: every label is `ignore`; absent: class K//2 occurs in neither (K >= 2)."""
    rng = np.random.default_rng(seed)
    label = rng.integers(0, K, size=M, dtype=np.int64)
    pred = rng.integers(0, K, size=M, dtype=np.int64)
    agree = rng.random(M) < 0.5
    pred[agree] = label[agree]
    if kind == "planted":
        pairs = confusion_planted_pairs(K, ignore)[:M]
        at = np.linspace(0, M - 1, num=len(pairs)).astype(np.int64)
        assert len(set(at.tolist())) == len(pairs)
        for i, (p, l) in zip(at, pairs):
            pred[i], label[i] = p, l
    elif kind == "constant":
        c = K - 1 if K - 1 != ignore else 0
        pred[:] = c
        label[:] = c
    elif kind == "ignored":
        label[:] = ignore
    elif kind == "absent":
        assert K >= 2
        pred[pred == K // 2] = 0
        label[label == K // 2] = 0
    else:
        assert kind == "random", kind
    return pred, label
