"""Plain-torch fp64 restatements of the elementwise passes of the bf16-storage mode (csrc/elem_bf16.hip; include/cvk.h from
cvk_import_nchw_bf16 on), written from their definitions for the tests.  Everything is NHWC (channels last, per-channel vectors
broadcast over the last axis) and float64; nothing here touches a GPU or imports the package, and the functions are plain tensor
expressions, so they also run on device tensors where a host reference would be too slow.

  apply        out = max(0, y*scale + shift)                                      BatchNorm2d + ReLU, models/unet.py:12-13
  backward     z = y*scale + shift, g = dout [z > 0], xhat = (y - mean)*rstd
               dbeta = sum g, dgamma = sum g*xhat
               dy = scale*(g - dbeta/M - xhat*dgamma/M)     (batch statistics)    dy = scale*g   (running statistics)
  pool         2x2 maximum, floor output size; arg-max = first maximum in scan order (0,0),(0,1),(1,0),(1,1)   models/unet.py:92
  bilinear x2  align_corners=True: src = dst*(n-1)/(2n-1), taps i0 = floor(src), i1 = min(i0+1, n-1), weights 1-f, f   models/unet.py:25

scale, shift, mean, rstd, dgamma and dbeta are INPUTS: the fp32 values the kernel gets, widened to fp64.  Nothing is recomputed from
statistics here, so a difference between kernel and restatement is the kernel's arithmetic and nothing else."""
import torch

U32 = 2.0 ** -24                      # unit roundoff of fp32
BF16_MIN_NORMAL_EXP = -126            # smallest normal bf16 = 2^-126 (the exponent range of fp32)


def _f64(*ts):
    for t in ts:
        assert t.dtype == torch.float64, t.dtype


def rne_bf16(t):
    """Round to nearest even to bf16: torch's conversion."""
    return t.to(torch.bfloat16)


def bf16_half_ulp(ref):
    """Half the spacing of bf16 numbers at |ref| (fp64): bf16 keeps 8 significant bits, so for |ref| in [2^(e-1), 2^e) — e as frexp
    returns it — the spacing is 2^(e-8) and half of it 2^(e-9).  Below the normal range (zero included) the spacing of the smallest
    normal binade is used.  The power of two is assembled as an fp64 bit pattern: exact on every device."""
    a = ref.detach().abs().to(torch.float64)
    _, e = torch.frexp(a)
    e = torch.where(a < 2.0 ** BF16_MIN_NORMAL_EXP, torch.full_like(e, BF16_MIN_NORMAL_EXP + 1), e).to(torch.int64)
    return ((e - 9 + 1023) << 52).view(torch.float64)


def apply(y, scale, shift):
    _f64(y, scale, shift)
    return (y * scale + shift).clamp_min(0.0)


def pool2x2(a):
    """[N,H,W,C] -> [N,H//2,W//2,C]: the maximum of every full 2x2 cell; an odd trailing row / column feeds no cell."""
    N, H, W, C = a.shape
    Ho, Wo = H // 2, W // 2
    return a[:, :2 * Ho, :2 * Wo].reshape(N, Ho, 2, Wo, 2, C).amax(dim=(2, 4))


def pool2x2_scatter(v, x):
    """MaxPool2d(2,2) backward / MaxUnpool2d(2) forward: v [N,H//2,W//2,C] goes to the arg-max pixel of its cell of x [N,H,W,C]
    (first maximum in scan order), every other pixel gets 0."""
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    cells = x[:, :2 * Ho, :2 * Wo].reshape(N, Ho, 2, Wo, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, Ho, Wo, 4, C)
    k = cells.argmax(dim=3, keepdim=True)                      # torch.argmax: the first of several maxima
    s = torch.zeros(N, Ho, Wo, 4, C, dtype=v.dtype, device=v.device).scatter_(3, k, v.unsqueeze(3))
    out = torch.zeros(N, H, W, C, dtype=v.dtype, device=v.device)
    out[:, :2 * Ho, :2 * Wo] = s.reshape(N, Ho, Wo, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * Ho, 2 * Wo, C)
    return out


def bn_bwd_terms(dout, y, scale, shift, mean, rstd):
    """(mask, g, g*xhat, band).  mask = z > 0 (strictly, as torch's ReLU backward: z == 0 passes nothing).  band marks the elements
    whose mask an fp32 evaluation of z may legitimately decide the other way: |z| <= 4 * 2^-24 * (|y*scale| + |shift|) — fp32 computes
    z with at most two roundings (one with a fused multiply-add), each at most 2^-24 of a term that |y*scale| + |shift| bounds; 4 is
    that with a factor 2 to spare.  Where both terms are exactly 0, z is exactly 0 in every precision: not in the band."""
    _f64(dout, y, scale, shift, mean, rstd)
    ys = y * scale
    z = ys + shift
    mask = z > 0
    g = torch.where(mask, dout, torch.zeros_like(dout))
    xhat = (y - mean) * rstd
    mag = ys.abs() + shift.abs()
    band = (z.abs() <= 4.0 * U32 * mag) & (mag > 0)
    return mask, g, g * xhat, band


def bn_bwd_dy(dout, y, scale, shift, mean, rstd, dgamma, dbeta, M, use_batch_stats):
    """Gradient with respect to the conv output y (unrounded).  dgamma / dbeta may be None when use_batch_stats is 0."""
    _, g, _, _ = bn_bwd_terms(dout, y, scale, shift, mean, rstd)
    if not use_batch_stats:
        return scale * g
    _f64(dgamma, dbeta)
    xhat = (y - mean) * rstd
    return scale * (g - dbeta / M - xhat * dgamma / M)


def bilinear_taps(n, device="cpu"):
    """[2n, n] fp64 interpolation matrix of one axis, align_corners=True (ATen: src = dst * (n-1)/(2n-1))."""
    dst = torch.arange(2 * n, dtype=torch.float64, device=device)
    src = dst * (n - 1) / (2 * n - 1)
    i0 = src.floor().clamp_max(n - 1).to(torch.int64)
    i1 = (i0 + 1).clamp_max(n - 1)
    f = src - i0.to(torch.float64)
    A = torch.zeros(2 * n, n, dtype=torch.float64, device=device)
    rows = torch.arange(2 * n, device=device)
    A.index_put_((rows, i0), 1.0 - f, accumulate=True)
    A.index_put_((rows, i1), f, accumulate=True)
    return A


def bilinear_up2(x):
    """[N,H,W,C] -> [N,2H,2W,C]"""
    _f64(x)
    Ay, Ax = bilinear_taps(x.shape[1], x.device), bilinear_taps(x.shape[2], x.device)
    return torch.einsum("ph,qw,nhwc->npqc", Ay, Ax, x)


def bilinear_up2_adjoint(g):
    """[N,2H,2W,C] -> [N,H,W,C]: the transpose of bilinear_up2 (its backward).  All weights are >= 0, so the adjoint of |g| is the
    sum of |weight * g| that the error bounds use."""
    _f64(g)
    Ay, Ax = bilinear_taps(g.shape[1] // 2, g.device), bilinear_taps(g.shape[2] // 2, g.device)
    return torch.einsum("ph,qw,npqc->nhwc", Ay, Ax, g)
