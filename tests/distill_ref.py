"""fp64 restatement of the knowledge-distillation loss (cvk.DistillationLoss, include/cvk.h cvk_kd_loss_*) in plain torch ops on the
CPU: autograd-differentiable in the student's logits, and the closed-form gradient the backward kernel implements.

  L = ce H + kd K,  H = sum_valid w[t] (lse(x) - x[t]) / sum_valid w[t],  K = t2 sum_D KL(softmax(tau z) || softmax(tau x)) / |D|

`tau` and `t2` are taken as given (the float32-rounded values of `cvk.distillation_scales`), so the kernels and this file compute with
the same numbers.  A pixel is labelled when its target is in [0, C); D = the labelled pixels, plus the ignored ones when
`distill_ignored`; `t=None` labels nothing and puts every pixel into D; an out-of-range target is in neither set and makes L NaN."""
import torch


def _rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).double()


def pixel_sets(t, M, C, ignore_index, distill_ignored):
    """(labelled, in D, out of range): three bool [M] masks."""
    if t is None:
        none = torch.zeros(M, dtype=torch.bool)
        return none, ~none, none
    tt = t.reshape(-1)
    ign = tt == ignore_index
    lab = (tt >= 0) & (tt < C) & ~ign
    bad = ~ign & ~lab
    return lab, (lab | ign) if distill_ignored else lab, bad


def distill_loss(x, z, t, ce, kd, tau, t2, weight=None, ignore_index=-100, distill_ignored=False):
    """x, z: [N, C, H, W] (z may be None when kd == 0), t: int64 [N, H, W] or None (when ce == 0).  Returns (L, H, K, |D|, agree):
    three 0-dim fp64 tensors (a term whose coefficient is 0 is 0) and two ints; agree counts the pixels of D whose student and teacher
    arg-max (first maximum) coincide, 0 when kd == 0."""
    C = x.shape[1]
    xr = _rows(x)
    M = xr.shape[0]
    lab, in_d, bad = pixel_sets(t, M, C, ignore_index, distill_ignored)
    H = K = torch.zeros((), dtype=torch.float64)
    agree = 0
    if ce > 0:
        tl = t.reshape(-1)[lab]
        xl = xr[lab]
        w = torch.ones(C, dtype=torch.float64) if weight is None else weight.double()
        wt = w[tl]
        H = (wt * (torch.logsumexp(xl, 1) - xl.gather(1, tl[:, None])[:, 0])).sum() / wt.sum()
    if kd > 0:
        la = torch.log_softmax(tau * xr[in_d], 1)
        zd = _rows(z)[in_d]
        lb = torch.log_softmax(tau * zd, 1)
        K = t2 * (lb.exp() * (lb - la)).sum() / int(in_d.sum())
        agree = int((xr[in_d].argmax(1) == zd.argmax(1)).sum())
    L = (ce * H if ce > 0 else 0.0) + (kd * K if kd > 0 else 0.0)
    if bad.any():
        L = L * float("nan")
    return L, H, K, int(in_d.sum()), agree


def distill_grad(x, z, t, ce, kd, tau, t2, weight=None, ignore_index=-100, distill_ignored=False, g=1.0):
    """The closed form of include/cvk.h: dx_k = g (ce w[t] / sum w[t] (p_k - [k = t]) on labelled pixels + kd t2 tau / |D| (ps_k - qs_k)
    on pixels of D), as [N, C, H, W] fp64."""
    N, C, Hh, Ww = x.shape
    xr = _rows(x.detach())
    M = xr.shape[0]
    lab, in_d, _ = pixel_sets(t, M, C, ignore_index, distill_ignored)
    d = torch.zeros(M, C, dtype=torch.float64)
    if ce > 0:
        tl = t.reshape(-1)[lab]
        w = torch.ones(C, dtype=torch.float64) if weight is None else weight.double()
        wt = w[tl]
        onehot = torch.zeros(int(lab.sum()), C, dtype=torch.float64).scatter_(1, tl[:, None], 1.0)
        d[lab] += ce * (wt / wt.sum())[:, None] * (torch.softmax(xr[lab], 1) - onehot)
    if kd > 0:
        zr = _rows(z.detach())
        d[in_d] += kd * t2 * tau / int(in_d.sum()) * (torch.softmax(tau * xr[in_d], 1) - torch.softmax(tau * zr[in_d], 1))
    return (g * d).reshape(N, Hh, Ww, C).permute(0, 3, 1, 2)
