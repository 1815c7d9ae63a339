"""fp64 numpy restatement of the calibration meter and of the temperature fit (include/cvk.h: cvk_calib_accumulate,
cvk_calib_newton_accumulate, cvk_calib_newton_step), and the inputs the calibration tests share.  Pixel rows are [M, C]."""
import functools

import numpy as np

Q_SCALE = float(1 << 30)
TAU_LO, TAU_HI = 1.0 / 64.0, 64.0
CASES = {                     # name: (N, H, W, C, seed); the shapes of tests/test_gpu_calibration.py
    "two_groups": (2, 19, 27, 12, 1),          # M = 1026: two workgroups, the second with 2 rows
    "small": (1, 7, 9, 5, 2),                  # M = 63: less than one chunk, ld = 5 takes the scalar loads
    "wide": (1, 5, 53, 70, 3),                 # M = 265: rows wider than CE_MAX_LD are walked in global memory
    "many_groups": (3, 40, 40, 12, 4),         # M = 4800: five workgroups on the global table
}
IGNORE = 11


def rows_of(logits_nchw):
    """[N, C, H, W] -> [M, C]"""
    a = np.asarray(logits_nchw)
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1).reshape(-1, a.shape[1]))


def make_logits_labels(N, H, W, C, seed, ignore_index=IGNORE, scale=3.0, sharpen=1.0):
    """logits = scale * randn (float32 [N, C, H, W]); labels drawn from softmax(sharpen * (logits + randn)), so that the accuracy is
    neither 0 nor 1; about 10 % of the labels are ignore_index and a few are out of range (-1, C, C + 7, 2^32 + 1)."""
    rng = np.random.default_rng(seed)
    x = (scale * rng.standard_normal((N, C, H, W))).astype(np.float32)
    r = rows_of(x).astype(np.float64)
    z = sharpen * (r + rng.standard_normal(r.shape))
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    u = rng.random(len(r))
    t = np.minimum((np.cumsum(p, axis=1) < u[:, None]).sum(axis=1), C - 1).astype(np.int64)
    t[rng.random(len(r)) < 0.10] = ignore_index
    bad = rng.choice(len(r), size=min(4, len(r)), replace=False)
    t[bad] = np.array([-1, C, C + 7, (1 << 32) + 1], dtype=np.int64)[:len(bad)]
    return x, t.reshape(N, H, W)


@functools.lru_cache(maxsize=None)
def case(name):
    N, H, W, C, seed = CASES[name]
    x, t = make_logits_labels(N, H, W, C, seed)
    x.setflags(write=False)
    t.setflags(write=False)
    return x, t


def valid_mask(t, C, ignore_index):
    t = np.asarray(t).reshape(-1)
    return (t != ignore_index) & (t >= 0) & (t < C)


def pixel_terms(x, t, tau=1.0, ignore_index=IGNORE):
    """The definitions in fp64 on rows x [M, C] (float32 values) and targets t [M]: a dict of per-pixel arrays.  nll and brier are 0
    on pixels that are not valid."""
    x = np.asarray(x, dtype=np.float64)
    t = np.asarray(t).reshape(-1)
    M, C = x.shape
    z = float(tau) * x
    m = z.max(axis=1)
    e = np.exp(z - m[:, None])
    se = e.sum(axis=1)
    conf = 1.0 / se
    pred = x.argmax(axis=1)                                    # numpy: the first maximum
    valid = valid_mask(t, C, ignore_index)
    bad = (t != ignore_index) & ~valid
    tc = np.where(valid, t, 0)
    nll = np.where(valid, (m + np.log(se)) - z[np.arange(M), tc], 0.0)
    p = e * conf[:, None]
    onehot = np.zeros_like(p)
    onehot[np.arange(M), tc] = 1.0
    brier = np.where(valid, ((p - onehot) ** 2).sum(axis=1), 0.0)
    return {"conf": conf, "pred": pred, "valid": valid, "bad": bad, "nll": nll, "brier": brier, "correct": valid & (pred == t)}


def bins_fp64(conf, B):
    return np.clip(np.ceil(np.asarray(conf, dtype=np.float64) * B).astype(np.int64) - 1, 0, B - 1)


def near_bin_edge(conf, B, eps=1e-5):
    """where the fp64 conf * B lies within eps * B of an integer: a conf off by eps may fall into the neighbouring bin"""
    v = np.asarray(conf, dtype=np.float64) * B
    return np.abs(v - np.rint(v)) <= eps * B


def tables_from_conf(conf32, pred, t, C, B, ignore_index=IGNORE):
    """The kernel's binning rule applied, in float32 arithmetic, to a float32 conf map: (hist int64 [C][B][3], valid, out of range).
    bin = clamp((int)ceilf(conf * (float)B) - 1, 0, B - 1), q = floor(conf * 2^30)."""
    conf32 = np.asarray(conf32, dtype=np.float32).reshape(-1)
    pred = np.asarray(pred).reshape(-1)
    t = np.asarray(t).reshape(-1)
    valid = valid_mask(t, C, ignore_index)
    prod = conf32 * np.float32(B)                              # one float32 multiply
    assert prod.dtype == np.float32
    b = np.clip(np.ceil(prod).astype(np.int64) - 1, 0, B - 1)
    q = np.floor(conf32.astype(np.float64) * Q_SCALE).astype(np.int64)     # a power-of-two scale: exact in either format
    hist = np.zeros((C, B, 3), dtype=np.int64)
    v = np.nonzero(valid)[0]
    np.add.at(hist[:, :, 0], (pred[v], b[v]), 1)
    np.add.at(hist[:, :, 1], (pred[v], b[v]), (pred[v] == t[v]).astype(np.int64))
    np.add.at(hist[:, :, 2], (pred[v], b[v]), q[v])
    return hist, int(valid.sum()), int(((t != ignore_index) & ~valid).sum())


def pixel_loop(x, t, tau, B, ignore_index=IGNORE):
    """The same definitions as a plain loop over pixels and classes in Python floats (fp64): hist with q from the fp64 conf, valid, out
    of range, sum nll, sum brier."""
    import math
    x = np.asarray(x, dtype=np.float64)
    M, C = x.shape
    hist = np.zeros((C, B, 3), dtype=np.int64)
    valid = bad = 0
    s_nll = s_brier = 0.0
    for i in range(M):
        ti = int(t[i])
        if ti == ignore_index:
            continue
        if not 0 <= ti < C:
            bad += 1
            continue
        z = [float(tau) * float(v) for v in x[i]]
        m = max(z)
        se = 0.0
        for v in z:
            se += math.exp(v - m)
        pred = 0
        for c in range(1, C):
            if x[i, c] > x[i, pred]:
                pred = c
        conf = 1.0 / se
        b = min(max(int(math.ceil(conf * B)) - 1, 0), B - 1)
        hist[pred, b, 0] += 1
        hist[pred, b, 1] += int(pred == ti)
        hist[pred, b, 2] += int(math.floor(conf * Q_SCALE))
        valid += 1
        s_nll += (m + math.log(se)) - z[ti]
        s_brier += sum((math.exp(z[c] - m) * conf - (1.0 if c == ti else 0.0)) ** 2 for c in range(C))
    return hist, valid, bad, s_nll, s_brier


# ---- the temperature fit ----------------------------------------------------------------------------------------------------------------
def newton_sums(x, t, tau, ignore_index=IGNORE):
    """(n, NLL, g, h) of the valid pixels at tau in fp64: means of lse(tau x) - tau x_t, E_p[x] - x_t and Var_p[x] = sum_c p_c (x_c -
    E_p[x])^2, p = softmax(tau x)."""
    x = np.asarray(x, dtype=np.float64)
    t = np.asarray(t).reshape(-1)
    v = valid_mask(t, x.shape[1], ignore_index)
    x, t = x[v], t[v]
    n = len(x)
    if n == 0:
        return 0, float("nan"), float("nan"), float("nan")
    z = float(tau) * x
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    se = e.sum(axis=1, keepdims=True)
    p = e / se
    xt = x[np.arange(n), t]
    mean = (p * x).sum(axis=1)
    var = (p * (x - mean[:, None]) ** 2).sum(axis=1)
    nll = (m[:, 0] + np.log(se[:, 0])) - float(tau) * xt
    return n, float(nll.mean()), float((mean - xt).mean()), float(var.mean())


def newton_rule(tau, lo, hi, n, g, h):
    """One bracketed Newton update in fp64: (tau next rounded to float32, lo, hi)."""
    if not n > 0:
        return tau, lo, hi
    if g < 0.0:
        lo = tau
    elif g > 0.0:
        hi = tau
    newton = h > 1e-12
    cand = tau - g / h if newton else 0.0
    if not newton or not (lo < cand < hi):
        cand = float(np.sqrt(lo * hi))
    return float(np.float32(cand)), lo, hi


def newton_fit(batches, iterations=20, init=1.0, ignore_index=IGNORE):
    """The fit in fp64 over `batches` = [(rows, targets), ...]: the log, [iterations + 1][8] = tau, n, NLL, g, h, tau next, lo, hi."""
    x = np.concatenate([np.asarray(b[0], dtype=np.float64) for b in batches])
    t = np.concatenate([np.asarray(b[1]).reshape(-1) for b in batches])
    tau, lo, hi = float(np.float32(1.0 / init)), TAU_LO, TAU_HI
    log = np.zeros((iterations + 1, 8))
    for k in range(iterations + 1):
        n, L, g, h = newton_sums(x, t, tau, ignore_index)
        if k < iterations:
            nxt, lo, hi = newton_rule(tau, lo, hi, n, g, h)
        else:
            nxt = tau
        log[k] = [tau, n, L, g, h, nxt, lo, hi]
        tau = nxt
    return log


def minimiser(x, t, ignore_index=IGNORE, tol=1e-13):
    """The tau in [1/64, 64] that minimises the fp64 NLL, by bisection on the sign of g (g is increasing: the NLL is convex); an end of
    the bracket when g does not change sign inside it."""
    lo, hi = TAU_LO, TAU_HI
    if newton_sums(x, t, lo, ignore_index)[2] >= 0.0:
        return lo
    if newton_sums(x, t, hi, ignore_index)[2] <= 0.0:
        return hi
    while hi - lo > tol * hi:
        mid = 0.5 * (lo + hi)
        if newton_sums(x, t, mid, ignore_index)[2] < 0.0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def logit_scale(x, t, ignore_index=IGNORE):
    """s: the mean over the valid pixels of max_c |x_c|; NLL, g and h scale as 1, s and s^2"""
    x = np.asarray(x, dtype=np.float64)
    v = valid_mask(t, x.shape[1], ignore_index)
    return float(np.abs(x[v]).max(axis=1).mean())
