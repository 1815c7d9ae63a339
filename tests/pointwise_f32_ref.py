"""Plain references of the fp32 data-movement passes of csrc/pointwise.hip, for tests/test_gpu_pointwise_f32.py.  What
tests/elem_bf16_ref.py (pool2x2, pool2x2_scatter, bilinear_taps, bilinear_up2, bilinear_up2_adjoint: they work for any storage type)
and tests/eval_io_ref.py (import_nchw_ref, export_nchw_ref, zero_frame_ref) already state is imported from there; this file adds the
rest.  tests/test_pointwise_f32_ref_cpu.py checks all of it against torch without a GPU.  Everything is NHWC.

  arg-max code   0..3 = the position (0,0), (0,1), (1,0), (1,1) inside the 2x2 cell; the scan takes a later element when it is
                 strictly greater or a NaN (ATen's `val > maxval || isnan(val)`): the first of several maxima wins, -0.0 and +0.0
                 are equal, a NaN wins against everything before it
  torch index    (2 yo + k/2) * W + 2 xo + k%2, laid out [N,C,H/2,W/2] as MaxPool2d(return_indices=True) returns it
  unpool         forward: v goes to the coded pixel of its cell, everything else (an odd trailing row / column too) is zero;
                 its adjoint reads the coded pixel back.  The pool's backward is the unpool's forward with the code of x.
  bilinear x2    exact taps in fp64 (elem_bf16_ref.bilinear_taps: src = dst (n-1)/(2n-1)), and the 6-wide candidate window
                 [2i-2, 2i+3] of the backward's error bound."""
import torch

from tests.elem_bf16_ref import U32, bilinear_taps, bilinear_up2, bilinear_up2_adjoint, pool2x2, pool2x2_scatter  # noqa: F401
from tests.eval_io_ref import export_nchw_ref, import_nchw_ref, zero_frame_ref  # noqa: F401


def cells(x):
    """[N,H,W,C] -> [N,H//2,W//2,4,C]: the full 2x2 cells in scan order; an odd trailing row / column belongs to no cell"""
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    return x[:, :2 * Ho, :2 * Wo].reshape(N, Ho, 2, Wo, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, Ho, Wo, 4, C)


def uncells(s, H, W):
    """[N,H//2,W//2,4,C] -> [N,H,W,C], zero where no cell is"""
    N, Ho, Wo, _, C = s.shape
    out = torch.zeros(N, H, W, C, dtype=s.dtype, device=s.device)
    out[:, :2 * Ho, :2 * Wo] = s.reshape(N, Ho, Wo, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * Ho, 2 * Wo, C)
    return out


def pool_code(x):
    """(pooled [N,H//2,W//2,C] in x's dtype, code uint8 of the same shape).  The pooled value is the coded element itself, so its
    bits (the sign of a zero, a NaN's payload) are the input's."""
    c = cells(x)
    best = c[:, :, :, 0]
    code = torch.zeros(best.shape, dtype=torch.uint8, device=x.device)
    for k in (1, 2, 3):
        a = c[:, :, :, k]
        take = (a > best) | (a != a)
        best = torch.where(take, a, best)
        code = torch.where(take, torch.full_like(code, k), code)
    return best, code


def pool_index(code, W):
    """code [N,Ho,Wo,C] -> int64 [N,C,Ho,Wo]: the flat index into the H x W plane that torch's max_pool2d returns"""
    N, Ho, Wo, C = code.shape
    k = code.to(torch.int64)
    yo = torch.arange(Ho, dtype=torch.int64, device=code.device).view(1, Ho, 1, 1)
    xo = torch.arange(Wo, dtype=torch.int64, device=code.device).view(1, 1, Wo, 1)
    return ((2 * yo + k // 2) * W + 2 * xo + k % 2).permute(0, 3, 1, 2).contiguous()


def unpool_fwd(v, code, H, W):
    """v, code [N,H//2,W//2,C] -> [N,H,W,C]"""
    N, Ho, Wo, C = v.shape
    assert (Ho, Wo) == (H // 2, W // 2) and code.shape == v.shape
    s = torch.zeros(N, Ho, Wo, 4, C, dtype=v.dtype, device=v.device).scatter_(3, code.to(torch.int64).unsqueeze(3), v.unsqueeze(3))
    return uncells(s, H, W)


def unpool_bwd(dout, code):
    """dout [N,H,W,C], code [N,H//2,W//2,C] -> [N,H//2,W//2,C]: the adjoint of unpool_fwd"""
    return cells(dout).gather(3, code.to(torch.int64).unsqueeze(3)).squeeze(3)


def candidate_window(n, device="cpu"):
    """[2n, n] fp64 matrix of ones where output index p lies in the candidate window [2i-2, 2i+3] of input index i (every output
    whose taps can touch i lies there, csrc/pointwise.hip k_bilinear_bwd), zero elsewhere"""
    p = torch.arange(2 * n, device=device).view(-1, 1)
    i = torch.arange(n, device=device).view(1, -1)
    return ((p >= 2 * i - 2) & (p <= 2 * i + 3)).to(torch.float64)


def window_abs_sum(g):
    """[N,2H,2W,C] fp64 -> [N,H,W,C]: the sum of |g| over each input pixel's 6x6 candidate window"""
    assert g.dtype == torch.float64
    By, Bx = candidate_window(g.shape[1] // 2, g.device), candidate_window(g.shape[2] // 2, g.device)
    return torch.einsum("ph,qw,npqc->nhwc", By, Bx, g.abs())


def bilinear_fwd_bound(x, ref):
    """8 max(H,W) u max|x| + u |ref|: the tap position scale * dst is an fp32 product of magnitude up to max(H,W), so a weight
    carries an absolute error of up to 2u max(H,W) per axis (the quotient's rounding and the product's), times a difference of two
    inputs (2 max|x|), two axes; u |ref| covers the sums' own roundings and the store."""
    H, W = x.shape[1], x.shape[2]
    return 8 * max(H, W) * U32 * float(x.abs().max()) + U32 * ref.abs()


def bilinear_bwd_bound(g, H, W):
    """40u sum|w g| + 4 max(H,W) u sum_window|g|.  The first term is the general bound of a sum of at most 36 products in any order;
    the second the weights' own error: 2u max(H,W) per axis and weight (see bilinear_fwd_bound), the product of two weights <= 1
    is off by the sum of the two, and every gradient the sum can reach lies in the 6x6 candidate window."""
    return 40 * U32 * bilinear_up2_adjoint(g.abs()) + 4 * max(H, W) * U32 * window_abs_sum(g)
