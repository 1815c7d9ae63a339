"""Plain numpy fp64 restatement of the Lovász-softmax loss (cvk.LovaszSoftmaxLoss), written from the definition in include/cvk.h.
Two formulations that share nothing but the errors and the order: the closed-form weights g the kernels use, and the cumulative
Jaccard formulation of the paper's `lovasz_grad` (J_n = 1 - (G - F_n) / (G + n - F_n), g_n = J_{n+1} - J_n)."""
import numpy as np


def softmax64(x):
    """x: [M, C] -> p, and q = 1 - p computed as the other classes' share (no cancellation), both fp64."""
    x = np.asarray(x, np.float64)
    ex = np.exp(x - x.max(axis=1, keepdims=True))
    se = ex.sum(axis=1, keepdims=True)
    rest = np.stack([np.delete(ex, c, axis=1).sum(axis=1) for c in range(x.shape[1])], axis=1)
    return ex / se, rest / se


def errors(x, t, c):
    """Errors of class c over the rows of x (all valid): p[c] where t != c, 1 - p[c] where t == c; and the foreground mask."""
    p, q = softmax64(x)
    fg = t == c
    return np.where(fg, q[:, c], p[:, c]), fg


def stable_order(e):
    """Descending by e, ties by ascending index."""
    return np.argsort(-np.asarray(e), kind="stable")


def weights_closed_form(fg_sorted):
    """g at every position of the sorted order, from integers: 1 / U (foreground), I / (U (U + 1)) (background)."""
    fg_sorted = np.asarray(fg_sorted, bool)
    V = fg_sorted.size
    G = int(fg_sorted.sum())
    g = np.zeros(V, np.float64)
    if V == 0:
        return g
    if G == 0:
        g[0] = 1.0
        return g
    n = np.arange(V, dtype=np.int64)
    F = np.cumsum(fg_sorted) - fg_sorted                    # foreground strictly before
    U = G + n - F
    I = G - F
    return np.where(fg_sorted, 1.0 / U, I / (U * (U + 1.0)))


def weights_cumulative_jaccard(fg_sorted):
    """The published lovasz_grad: jaccard = 1 - (G - cumsum(fg)) / (G + cumsum(1 - fg)), then first differences."""
    fg = np.asarray(fg_sorted, np.float64)
    if fg.size == 0:
        return fg
    G = fg.sum()
    inter = G - np.cumsum(fg)
    union = G + np.cumsum(1.0 - fg)
    jac = 1.0 - inter / union
    jac[1:] = jac[1:] - jac[:-1]
    return jac


def class_loss(e, fg, order=None, weights=weights_closed_form):
    """(L_c, g in pixel order) of one segment and class.  `order`: a permutation to use instead of the stable order (the kernel's)."""
    order = stable_order(e) if order is None else np.asarray(order)
    gs = weights(np.asarray(fg)[order])
    g = np.zeros(len(e), np.float64)
    g[order] = gs
    return float(np.dot(np.asarray(e, np.float64)[order], gs)), g


def lovasz_softmax(x, t, ignore_index=-100, classes="present", per_image=False, weights=weights_closed_form, orders=None):
    """x: [N, C, H, W], t: [N, H, W] (numpy).  Returns a dict: loss J, class_loss [C] (mean over the evaluating segments, NaN: none),
    pairs, counted, dlogits [N, C, H, W] of J (fp64).  `orders[(s, c)]`: the order of the valid pixels of segment s for class c, as
    indices into the segment's valid pixels, to use instead of the stable one."""
    x = np.asarray(x, np.float64)
    t = np.asarray(t)
    N, C, H, W = x.shape
    rows = x.transpose(0, 2, 3, 1).reshape(N, H * W, C)
    tt = t.reshape(N, H * W)
    if not per_image:
        rows, tt = rows.reshape(1, N * H * W, C), tt.reshape(1, N * H * W)
    S = rows.shape[0]
    seg_losses, pairs = [], 0
    cl_sum, cl_n = np.zeros(C), np.zeros(C, int)
    gsign = np.zeros(rows.shape)                           # s_c before the 1 / (K counted) factor
    Ks = np.zeros(S, int)
    for s in range(S):
        valid = tt[s] != ignore_index
        xs, ts = rows[s][valid], tt[s][valid]
        if xs.shape[0] == 0:
            continue
        ls = []
        gv = np.zeros((xs.shape[0], C))
        for c in range(C):
            e, fg = errors(xs, ts, c)
            if classes == "present" and not fg.any():
                continue
            L, g = class_loss(e, fg, None if orders is None else orders[(s, c)], weights)
            ls.append(L)
            cl_sum[c] += L
            cl_n[c] += 1
            gv[:, c] = np.where(fg, -g, g)
        if ls:
            seg_losses.append(np.mean(ls))
            pairs += len(ls)
            Ks[s] = len(ls)
            gsign[s][valid] = gv
    counted = len(seg_losses)
    loss = float(np.mean(seg_losses)) if counted else 0.0
    d = np.zeros(rows.shape)
    for s in range(S):
        if Ks[s] == 0:
            continue
        p, _ = softmax64(rows[s])
        sc = gsign[s] / (Ks[s] * counted)
        d[s] = p * (sc - (sc * p).sum(axis=1, keepdims=True))
        d[s][tt[s] == ignore_index] = 0.0
    d = d.reshape(N, H, W, C).transpose(0, 3, 1, 2)
    with np.errstate(invalid="ignore"):
        cl = np.where(cl_n > 0, cl_sum / np.maximum(cl_n, 1), np.nan)
    return {"loss": loss, "class_loss": cl, "pairs": pairs, "counted": counted, "dlogits": d}


def radix_sort_emulation(keys, tile, bits, dest, count_index, segments=1):
    """The sort's index arithmetic on the host: `keys` [segments, P] unsigned, stable LSD passes of `bits` bits with work-groups of
    `tile` elements; every table index comes from `count_index(nwg, seg, digit, wg)` and every destination from
    `dest(P, seg, digit_base, wg_base, rank)` (the library's own functions).  Returns the permutation [segments, P] (source index at
    every sorted position); raises AssertionError on an index out of range or written twice."""
    keys = np.asarray(keys, np.uint64).reshape(segments, -1)
    P = keys.shape[1]
    nwg = (P + tile - 1) // tile
    bins = 1 << bits
    perm = np.tile(np.arange(P), (segments, 1))
    cur = keys.copy()
    for shift in range(0, 32, bits):
        counts = np.zeros(segments * bins * nwg, np.int64)
        digits = (cur >> np.uint64(shift)) & np.uint64(bins - 1)
        for s in range(segments):
            for w in range(nwg):
                h = np.bincount(digits[s, w * tile:(w + 1) * tile].astype(np.int64), minlength=bins)
                for d in range(bins):
                    at = count_index(nwg, s, d, w)
                    assert 0 <= at < counts.size
                    counts[at] = h[d]
        out_k = np.full(segments * P, -1, np.int64).astype(np.uint64)
        out_p = np.full(segments * P, -1, np.int64)
        for s in range(segments):
            rows = np.array([[counts[count_index(nwg, s, d, w)] for w in range(nwg)] for d in range(bins)])
            tot = rows.sum(axis=1)
            dbase = np.cumsum(tot) - tot
            wbase = np.cumsum(rows, axis=1) - rows
            for w in range(nwg):
                seen = np.zeros(bins, np.int64)
                for k in range(w * tile, min(P, (w + 1) * tile)):
                    d = int(digits[s, k])
                    to = dest(P, s, int(dbase[d]), int(wbase[d, w]), int(seen[d]))
                    seen[d] += 1
                    assert s * P <= to < (s + 1) * P, (s, k, to)
                    assert out_p[to] == -1, (s, k, to)
                    out_k[to], out_p[to] = cur[s, k], perm[s, k]
        cur, perm = out_k.reshape(segments, P), out_p.reshape(segments, P)
    return perm
