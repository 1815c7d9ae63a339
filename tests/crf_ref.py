"""numpy restatement of the local-window mean-field CRF of include/cvk.h (cvk_crf_step), from shifted slices, in fp64 or in fp32.

It takes the fp32-rounded tables ga, gs and cb as the kernel gets them (`crf_coefficients`).  In fp64 it is the reference; run in
fp32 it gives the rounding error of a legal fp32 evaluation, from which tests/test_gpu_crf.py takes its bound.  No torch, no GPU."""
import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)


def softmax(v, dtype):
    v = v.astype(dtype)
    e = np.exp(v - v.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(dtype)


def guide_levels(x_nchw, a, b, dtype=np.float64):
    """I [N,H,W,3] = a_k x_k + b_k of a float32 network input [N,3,H,W] and the float32 a, b the kernel gets."""
    x = np.asarray(x_nchw).transpose(0, 2, 3, 1).astype(dtype)
    return (x * np.asarray(a, dtype=np.float32).astype(dtype) + np.asarray(b, dtype=np.float32).astype(dtype)).astype(dtype)


def offsets(radius, dilation):
    """[(tap index, dy, dx)] in row-major (i, j), the centre left out."""
    side = 2 * radius + 1
    return [((i + radius) * side + (j + radius), dilation * i, dilation * j)
            for i in range(-radius, radius + 1) for j in range(-radius, radius + 1) if (i, j) != (0, 0)]


def _views(H, W, dy, dx):
    """slices (of p, of p + o) over the pixels p whose neighbour p + o lies inside the image; None when there is none"""
    y0, y1 = max(0, -dy), H - max(0, dy)
    x0, x1 = max(0, -dx), W - max(0, dx)
    if y1 <= y0 or x1 <= x0:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def messages(Q, I, ga, gs, cb, radius, dilation, dtype):
    """(Sa / na, Ss / ns) [N,H,W,C] each, 0 where the normaliser is 0: the two normalised messages before their weights."""
    N, H, W, C = Q.shape
    ga, gs = np.asarray(ga, dtype=np.float32).ravel().astype(dtype), np.asarray(gs, dtype=np.float32).ravel().astype(dtype)
    cb = dtype(np.float32(cb))
    Sa, Ss = np.zeros((N, H, W, C), dtype), np.zeros((N, H, W, C), dtype)
    na, ns = np.zeros((N, H, W), dtype), np.zeros((N, H, W), dtype)
    for tap, dy, dx in offsets(radius, dilation):
        v = _views(H, W, dy, dx)
        if v is None:
            continue
        (py, px), (qy, qx) = v
        diff = I[:, py, px] - I[:, qy, qx]
        ka = (ga[tap] * np.exp(cb * (diff * diff).sum(axis=-1, dtype=dtype))).astype(dtype)
        qn = Q[:, qy, qx]
        Sa[:, py, px] += ka[..., None] * qn
        Ss[:, py, px] += gs[tap] * qn
        na[:, py, px] += ka
        ns[:, py, px] += gs[tap]
    with np.errstate(divide="ignore", invalid="ignore"):
        ra = np.where(na > 0, dtype(1) / na, dtype(0)).astype(dtype)
        rs = np.where(ns > 0, dtype(1) / ns, dtype(0)).astype(dtype)
    return Sa * ra[..., None], Ss * rs[..., None]


def crf_reference(U, I, ga, gs, cb, wa, ws, radius, dilation, iterations, compat=None, unary_is_prob=False, dtype=np.float64):
    """probs [N,H,W,C] = Q_T of the unary U [N,H,W,C] under the guide I [N,H,W,3] (grey levels)."""
    dtype = np.dtype(dtype).type
    U, I = np.asarray(U).astype(dtype), np.asarray(I).astype(dtype)
    if unary_is_prob:
        U = np.log(np.maximum(U, dtype(FLT_MIN))).astype(dtype)
    wa, ws = dtype(np.float32(wa)), dtype(np.float32(ws))
    mu = None if compat is None else np.asarray(compat, dtype=np.float32).astype(dtype)
    Q = softmax(U, dtype)
    for _ in range(iterations):
        ma, ms = messages(Q, I, ga, gs, cb, radius, dilation, dtype)
        m = (wa * ma + ws * ms).astype(dtype)
        Q = softmax(U + m if mu is None else U - m @ mu.T, dtype)
    return Q


def crf_brute(U, I, ga, gs, cb, wa, ws, radius, dilation, iterations, compat=None):
    """the same by a loop over pixels and offsets, fp64: what the sliced restatement is held against"""
    U, I = np.asarray(U, dtype=np.float64), np.asarray(I, dtype=np.float64)
    N, H, W, C = U.shape
    ga, gs = np.asarray(ga, dtype=np.float64).ravel(), np.asarray(gs, dtype=np.float64).ravel()
    mu = -np.eye(C) if compat is None else np.asarray(compat, dtype=np.float64)
    Q = softmax(U, np.float64)
    for _ in range(iterations):
        Qn = np.empty_like(Q)
        for n in range(N):
            for y in range(H):
                for x in range(W):
                    Sa, Ss, na, ns = np.zeros(C), np.zeros(C), 0.0, 0.0
                    for tap, dy, dx in offsets(radius, dilation):
                        yy, xx = y + dy, x + dx
                        if not (0 <= yy < H and 0 <= xx < W):
                            continue
                        ka = ga[tap] * np.exp(float(np.float32(cb)) * ((I[n, y, x] - I[n, yy, xx]) ** 2).sum())
                        Sa += ka * Q[n, yy, xx]; na += ka
                        Ss += gs[tap] * Q[n, yy, xx]; ns += gs[tap]
                    m = np.zeros(C)
                    if na > 0:
                        m += wa * Sa / na
                    if ns > 0:
                        m += ws * Ss / ns
                    Qn[n, y, x] = softmax(U[n, y, x] - mu @ m, np.float64)
        Q = Qn
    return Q


def blocky_frames(N, H, W, seed, cell=(7, 9), noise=6):
    """uint8 [N,H,W,3]: cells of random colour with +-noise levels on top, the standard guide of the tests"""
    rng = np.random.default_rng(seed)
    gy, gx = -(-H // cell[0]), -(-W // cell[1])
    base = rng.integers(noise, 256 - noise, size=(N, gy, gx, 3))
    img = np.repeat(np.repeat(base, cell[0], axis=1), cell[1], axis=2)[:, :H, :W]
    return (img + rng.integers(-noise, noise + 1, size=img.shape)).astype(np.uint8)


def normalise(frames_u8, mean, std):
    """float32 [N,3,H,W]: the network input of uint8 frames, (v / 255 - mean) / std in fp32"""
    v = frames_u8.astype(np.float32) / np.float32(255.0)
    x = (v - np.asarray(mean, dtype=np.float32)) / np.asarray(std, dtype=np.float32)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32)


def top2_margin(P):
    s = np.sort(P, axis=-1)
    return s[..., -1] - s[..., -2] if P.shape[-1] > 1 else np.full(P.shape[:-1], np.inf)
