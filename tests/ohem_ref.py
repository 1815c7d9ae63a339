"""fp64 restatement of the OHEM cross-entropy (include/cvk.h, cvk_ohem_ce_fwd) in torch / numpy, with no selection tricks: a full sort
for L, the two predicates, the weighted mean, autograd for the gradient.

  l_i  = lse(x_i) - x_i[t_i]                      unweighted loss of a valid pixel (t_i != ignore_index)
  V    = number of valid pixels, k = min(min_kept, V), L = the k-th largest l_i
  kept = valid and (l_i > lam or l_i >= L)
  loss = sum_kept w[t_i] l_i / sum_kept w[t_i]    (V = 0: NaN)
"""
import numpy as np
import torch


def loss_threshold(thresh):
    return np.float32(-np.log(np.float64(thresh)))


def pixel_losses(logits, target, ignore_index=-100):
    """fp64 [N, H, W] losses (-1 where ignored) and the valid mask; logits [N, C, H, W] of any float dtype, may require grad."""
    x = logits.double()
    valid = target != ignore_index
    tc = target.clamp(0, x.shape[1] - 1)
    l = torch.logsumexp(x, dim=1) - x.gather(1, tc.unsqueeze(1)).squeeze(1)
    return torch.where(valid, l, torch.full_like(l, -1.0)), valid


def kth_largest(values, k):
    """The k-th largest (1-based) of a 1-D array by a full sort."""
    return np.sort(np.asarray(values))[::-1][k - 1]


def select(loss_map_fp32, lam, min_kept):
    """The selection rule on a given fp32 loss map, compared in fp32: negative entries are ignored pixels, NaN out-of-range targets.
    Returns (kept mask, L as float32 (0 when V = 0), V, k)."""
    m = np.asarray(loss_map_fp32, dtype=np.float32)
    lam = np.float32(lam)
    valid = m >= 0                                       # false for NaN
    V = int(valid.sum())
    k = min(int(min_kept), V)
    if V == 0:
        return np.zeros(m.shape, bool), np.float32(0), 0, 0
    L = np.float32(kth_largest(m[valid], k))
    kept = valid & ((m > lam) | (m >= L))
    return kept, L, V, k


def weighted_mean(logits, target, kept, weight=None):
    """fp64 loss over a given kept set (a bool tensor [N, H, W]); differentiable in the logits."""
    x = logits.double()
    C = x.shape[1]
    tc = target.clamp(0, C - 1)
    l = torch.logsumexp(x, dim=1) - x.gather(1, tc.unsqueeze(1)).squeeze(1)
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.double()
    wt = w[tc] * kept.double()
    return (wt * l).sum() / wt.sum()


def ohem(logits, target, thresh, min_kept, weight=None, ignore_index=-100):
    """(loss, kept mask, L, V, per-pixel losses), everything in fp64; the loss is differentiable in the logits."""
    l, valid = pixel_losses(logits, target, ignore_index)
    lam = float(loss_threshold(thresh))
    V = int(valid.sum())
    if V == 0:
        kept = torch.zeros_like(valid)
        return weighted_mean(logits, target, kept, weight), kept, float("nan"), 0, l.detach()
    k = min(int(min_kept), V)
    L = float(kth_largest(l.detach()[valid].numpy(), k))
    kept = valid & ((l.detach() > lam) | (l.detach() >= L))
    return weighted_mean(logits, target, kept, weight), kept, L, V, l.detach()
