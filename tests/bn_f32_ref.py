"""High-precision restatements of what the fp32 BatchNorm passes (csrc/bn.hip) compute beyond tests/elem_bf16_ref.py, whose apply,
pool2x2, bn_bwd_terms and bn_bwd_dy work for any storage type and are used as they are.  Here: the statistics finalisation, the eval
parameters, the E planes of the transposed F(4,3) weight gradient, and the row index of the padded plane layout.  Nothing here touches a
GPU or imports the package.

  partial layout   float[2][P][C]: per granule p of n_p rows the sum s_p and q_p = sum (y - s_p/n_p)^2 (the M2 about the granule's OWN mean)
  finalisation     S = sum s_p, mean = S/M, m2 = sum q_p + sum s_p^2/n_p - S^2/M (Chan's combination), var = m2/M (biased, normalises),
                   rstd = 1/sqrt(var + eps), scale = gamma*rstd, shift = beta - mean*scale,
                   running = (1 - m)*old + m*new with new = mean and the UNBIASED m2/(M - 1) (the biased one for M = 1)
  eval parameters  mean = running_mean, rstd = 1/sqrt(running_var + eps), scale and shift as above
  E planes         per group of four columns d0..d3 of dy (a missing column counts as 0): E_k = sum_i p_k^i d_i at the points
                   p = (1, -1, 2, -2) for E1..E4, E0 = d0 and E5 = d3 (the points 0 and infinity)
  padded layout    prow = Wtp + (n*(H + 2) + y + 1)*Wtp + xt with Wtp = ceil(ceil(W/4)/8)*8; (N*(H + 2) + 2)*Wtp rows per plane

The statistics are evaluated in numpy.longdouble (64 significant bits on x86: sums of a few thousand fp32 values and their squares
lose nothing that matters beside 2^-52) from the fp32 partials AS THE KERNEL GETS THEM, so kernel and restatement differ by the
kernel's fp64 arithmetic and one rounding to fp32; `magnitudes` returns the sums of absolute values the error bounds are written in."""
import numpy as np
import torch

LD = np.longdouble
STAT_ROWS = 64                        # include/cvk.h CVK_STAT_ROWS
U32 = 2.0 ** -24


def granule_counts(M, rows=STAT_ROWS):
    """rows per granule: full granules and a ragged last one"""
    return [min(rows, M - p) for p in range(0, M, rows)]


def partials(y, counts, dtype=np.float32):
    """y [M, C] (fp64) -> [2][P][C]: sum and M2 about the granule's own mean, formed in fp64, rounded to `dtype`"""
    y = np.asarray(y, dtype=np.float64)
    assert sum(counts) == y.shape[0]
    out = np.empty((2, len(counts), y.shape[1]), dtype=np.float64)
    m = 0
    for p, n in enumerate(counts):
        blk = y[m:m + n]
        out[0, p] = blk.sum(0)
        out[1, p] = ((blk - blk.mean(0)) ** 2).sum(0)
        m += n
    return out.astype(dtype)


def finalize(stats, counts, M, gamma, beta, eps, momentum=None, running_mean=None, running_var=None):
    """The finalisation of the partials `stats` [2][P][C] in longdouble.  eps and momentum are the fp32 values the kernel gets.
    Returns a dict of longdouble [C] arrays: mean, var, unbiased, rstd, scale, shift, running_mean / running_var (when given), and
    the magnitudes abs_s = sum|s_p|, var_mag = sum q_p + sum s_p^2/n_p + S^2/M, round_mag = sum q_p + 2 sum s_p^2/n_p."""
    s, q = np.asarray(stats[0], dtype=LD), np.asarray(stats[1], dtype=LD)
    n = np.asarray(counts, dtype=LD)[:, None]
    assert s.shape[0] == len(counts) and int(sum(counts)) == M
    S = s.sum(0)
    between = (s * s / n).sum(0)
    m2 = q.sum(0) + between - S * S / LD(M)
    m2 = np.maximum(m2, LD(0))
    r = {"mean": S / LD(M), "var": m2 / LD(M), "unbiased": m2 / LD(M - 1) if M > 1 else m2 / LD(M)}
    eps = LD(np.float32(eps))
    r["rstd"] = LD(1) / np.sqrt(r["var"] + eps)
    r["scale"] = np.asarray(gamma, dtype=LD) * r["rstd"]
    r["shift"] = np.asarray(beta, dtype=LD) - r["mean"] * r["scale"]
    r["abs_s"] = np.abs(s).sum(0)
    r["var_mag"] = q.sum(0) + between + S * S / LD(M)
    r["round_mag"] = q.sum(0) + 2 * between
    if running_mean is not None:
        m = LD(np.float32(momentum))
        r["running_mean"] = (LD(1) - m) * np.asarray(running_mean, dtype=LD) + m * r["mean"]
        r["running_var"] = (LD(1) - m) * np.asarray(running_var, dtype=LD) + m * r["unbiased"]
    return r


def eval_params(gamma, beta, running_mean, running_var, eps):
    """mean, rstd, scale, shift from the running statistics, longdouble"""
    rm = np.asarray(running_mean, dtype=LD)
    rstd = LD(1) / np.sqrt(np.asarray(running_var, dtype=LD) + LD(np.float32(eps)))
    scale = np.asarray(gamma, dtype=LD) * rstd
    return {"mean": rm, "rstd": rstd, "scale": scale, "shift": np.asarray(beta, dtype=LD) - rm * scale}


E_POINTS = (1.0, -1.0, 2.0, -2.0)
# rows E0..E5 over the four columns d0..d3 of a group
E_COEF = torch.tensor([[1.0, 0.0, 0.0, 0.0]] + [[p ** i for i in range(4)] for p in E_POINTS] + [[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)


def e_planes(dy, coef=E_COEF):
    """dy [N,H,W,C] fp64 -> [len(coef)][N][H][ceil(W/4)][C]; columns past W count as zero.  With coef.abs() and |dy| (or a bound of
    dy's error) it gives the sums of absolute terms the error bounds use."""
    assert dy.dtype == torch.float64
    N, H, W, C = dy.shape
    Wt = -(-W // 4)
    d = torch.zeros(N, H, 4 * Wt, C, dtype=torch.float64)
    d[:, :, :W] = dy
    return torch.einsum("ki,nhtic->knhtc", coef, d.view(N, H, Wt, 4, C))


def padded_layout(N, H, W):
    """(Wtp, rows per plane, prow [N][H][ceil(W/4)]) of the padded plane layout of csrc/wgradp.hip"""
    Wt = -(-W // 4)
    Wtp = -(-Wt // 8) * 8
    rows = (N * (H + 2) + 2) * Wtp
    n = torch.arange(N).view(N, 1, 1)
    y = torch.arange(H).view(1, H, 1)
    xt = torch.arange(Wt).view(1, 1, Wt)
    return Wtp, rows, Wtp + (n * (H + 2) + y + 1) * Wtp + xt
