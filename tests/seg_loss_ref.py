"""Plain-torch restatement of the fused focal + soft-Dice loss (include/cvk.h, cvk_seg_loss_fwd), written from its definition; the
tests run it in fp64 on the CPU as the reference of the HIP kernels, and in fp32 as the loss of the reference graph.

  x [N, C, H, W] logits, t [N, H, W] int64, p = softmax(x) over C, w[C] (ones when absent); sums over the pixels with t != ignore_index
  F = sum w[t] (1 - p[t])^gamma (-log p[t]) / sum w[t]
  I_c = sum p[c] [t = c], P_c = sum p[c], T_c = sum [t = c], dice_c = (2 I_c + s) / (P_c + T_c + s)
  D = 1 - (1 / K) sum_{c in S} dice_c, S = {c: T_c > 0} ("present") or every class ("all"), K = |S|; K = 0: D = 0
  L = ce F + dice D; a term whose coefficient is 0 is left out
"""
import torch


def _pieces(x, t, weight, ignore_index):
    C = x.shape[1]
    valid = t != ignore_index
    tc = torch.where(valid, t, torch.zeros_like(t))
    onehot = torch.nn.functional.one_hot(tc, C).permute(0, 3, 1, 2).to(x.dtype) * valid.unsqueeze(1).to(x.dtype)
    w = torch.ones(C, dtype=x.dtype, device=x.device) if weight is None else weight.to(x.dtype)
    wt = w[tc] * valid.to(x.dtype)
    return valid, onehot, wt


def seg_loss(x, t, ce=1.0, dice=0.0, *, focal_gamma=0.0, weight=None, ignore_index=-100, dice_smooth=1.0, dice_average="present"):
    """(L, F, D, dice_c[C]) in x's dtype; differentiable in x.  dice_c is 0 outside S."""
    valid, onehot, wt = _pieces(x, t, weight, ignore_index)
    logp = torch.log_softmax(x, dim=1)
    p = logp.exp()
    logpt = (logp * onehot).sum(1)
    focal_px = -logpt * wt
    if focal_gamma != 0:
        pt = (p * onehot).sum(1)
        focal_px = focal_px * (1 - pt).clamp(min=0) ** focal_gamma
    F = focal_px.sum() / wt.sum()
    pv = p * valid.unsqueeze(1).to(x.dtype)
    I = (pv * onehot).sum((0, 2, 3))
    P = pv.sum((0, 2, 3))
    T = onehot.sum((0, 2, 3))
    S = T > 0 if dice_average == "present" else torch.ones_like(T, dtype=torch.bool)
    assert dice_average in ("present", "all")
    K = int(S.sum())
    den = P + T + dice_smooth
    ratio = torch.where(den > 0, (2 * I + dice_smooth) / torch.where(den > 0, den, torch.ones_like(den)), torch.ones_like(den))
    dice_c = torch.where(S, ratio, torch.zeros_like(ratio))
    D = 1 - dice_c.sum() / K if K > 0 else dice_c.sum() * 0            # K = 0: a zero that still backpropagates (to zeros)
    L = x.new_zeros(())
    if ce > 0:
        L = L + ce * F
    if dice > 0:
        L = L + dice * D
    return L, F, D, dice_c


def seg_loss_grad_closed_form(x, t, ce=1.0, dice=0.0, *, focal_gamma=0.0, weight=None, ignore_index=-100, dice_smooth=1.0,
                              dice_average="present"):
    """dL/dx by the closed form the kernel implements (no autograd):
      Dice part  p_k (g_k - sum_c g_c p_c), g_c = b_c + a_c [t = c], a_c = -2 / (K den_c), b_c = (2 I_c + s) / (K den_c^2) on S
      focal part w[t] / sum w (delta_kt - p_k) (gamma p_t (1 - p_t)^(gamma - 1) log p_t - (1 - p_t)^gamma)
    with 1 - p_t summed from the other classes' probabilities and the gamma product taken as (1 - p_t)^gamma (log p_t / (1 - p_t))."""
    x = x.detach()
    valid, onehot, wt = _pieces(x, t, weight, ignore_index)
    vf = valid.unsqueeze(1).to(x.dtype)
    logp = torch.log_softmax(x, dim=1)
    p = logp.exp()
    g = torch.zeros_like(x)
    if ce > 0:
        logpt = (logp * onehot).sum(1)
        pt = (p * onehot).sum(1)
        q = (p * (vf - onehot)).sum(1)                       # 1 - p_t from the other classes
        qg = q ** focal_gamma if focal_gamma != 0 else torch.ones_like(q)
        ratio = torch.where(q > 0, logpt / torch.where(q > 0, q, torch.ones_like(q)), -torch.ones_like(q))
        B = qg * (focal_gamma * pt * ratio - 1)
        g = g + ce * (wt / wt.sum() * B).unsqueeze(1) * (onehot - p * vf)
    if dice > 0:
        pv = p * vf
        I = (pv * onehot).sum((0, 2, 3))
        P = pv.sum((0, 2, 3))
        T = onehot.sum((0, 2, 3))
        S = T > 0 if dice_average == "present" else torch.ones_like(T, dtype=torch.bool)
        K = int(S.sum())
        if K > 0:
            den = P + T + dice_smooth
            ok = S & (den > 0)
            dsafe = torch.where(ok, den, torch.ones_like(den))
            a = torch.where(ok, -2 / (K * dsafe), torch.zeros_like(den))
            b = torch.where(ok, (2 * I + dice_smooth) / (K * dsafe * dsafe), torch.zeros_like(den))
            gc = b.view(1, -1, 1, 1) + a.view(1, -1, 1, 1) * onehot
            g = g + dice * pv * (gc - (gc * p).sum(1, keepdim=True))
    return g
