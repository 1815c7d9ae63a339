"""tests/pointwise_f32_ref.py is right, and the bilinear bounds of tests/test_gpu_pointwise_f32.py are neither too tight nor idle:
  * the references against torch (max_pool2d with indices, max_unpool2d, bilinear interpolate in fp64 and autograd's adjoints) at the
    shapes and with the inputs of the GPU cases;
  * a float32 numpy emulation of the kernels' arithmetic (scale = (n-1)/(2n-1), src = scale * dst, i0 = (int)src, l1 = src - i0,
    l0 = 1 - l1, products and sums in float32, nothing fused) in both summation orders of the backward — the 6 x 6 gather and the
    separable walk — must stay inside the bounds at every GPU case, and its worst case must use more than a hundredth of them: a
    bound used less than that would not notice a swapped weight.  The worst used fractions are printed (profiles/
    pointwise_f32_margins.txt keeps them beside the device's).
The largest backward case is emulated at its H and W with N = 1 and 8 of its 2048 channels: channels do not interact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pointwise_f32_ref as P
from tests import test_gpu_pointwise_f32 as G

f32 = np.float32


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ references against torch
@pytest.mark.parametrize("name", list(G.POOL_CASES))
def test_pool_code_and_index_match_torch(name):
    x, _, _ = G.pool_case(name)
    N, H, W, C = x.shape
    pooled, code = P.pool_code(x)
    tv, ti = F.max_pool2d(nchw(x), 2, 2, return_indices=True)
    assert torch.equal(nchw(pooled).view(torch.int32) & 0x7FFFFFFF, tv.view(torch.int32) & 0x7FFFFFFF)     # torch may pick either zero
    assert torch.equal(torch.isnan(nchw(pooled)), torch.isnan(tv))
    assert torch.equal(P.pool_index(code, W), ti)
    plant = G.POOL_CASES[name][3]
    if plant is None:
        assert torch.equal(pooled, P.pool2x2(x))
        v = torch.randn(pooled.shape, generator=torch.Generator().manual_seed(1))
        assert torch.equal(P.unpool_fwd(v, code, H, W), P.pool2x2_scatter(v, x))


@pytest.mark.parametrize("name", list(G.UNPOOL_CASES))
def test_unpool_and_its_adjoint_match_torch(name):
    (N, H, W, C), _, _ = G.UNPOOL_CASES[name]
    g = torch.Generator().manual_seed(G.case_seed(name) + 2)
    x = (torch.randint(-2, 4, (N, H, W, C), generator=g).double() * 0.5).clamp_min(0.0)
    v = torch.randn(N, H // 2, W // 2, C, generator=g, dtype=torch.float64).requires_grad_(True)
    r = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    _, code = P.pool_code(x)
    out = F.max_unpool2d(nchw(v), P.pool_index(code, W), 2, 2, output_size=(H, W))
    assert torch.equal(P.unpool_fwd(v.detach(), code, H, W), nhwc(out.detach()))
    out.backward(nchw(r))
    assert torch.equal(P.unpool_bwd(r, code), v.grad)
    assert torch.equal(P.unpool_bwd(P.unpool_fwd(v.detach(), code, H, W), code), v.detach())


def bilinear_shapes():
    fwd = sorted({(2, hw[0], hw[1], min(C, 8)) for C, hw, _ in G.BILINEAR_FWD})
    bwd = sorted({(min(s[0], 2), s[1], s[2], min(s[3], 8)) for s in G.BILINEAR_BWD + [G.BILINEAR_BWD_LARGE]})
    return sorted(set(fwd + bwd))


@pytest.mark.parametrize("shape", bilinear_shapes())
def test_bilinear_references_match_torch(shape):
    N, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    r = torch.randn(N, 2 * H, 2 * W, C, generator=g, dtype=torch.float64)
    xt = nchw(x).requires_grad_(True)
    y = F.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=True)
    y.backward(nchw(r))
    assert float((P.bilinear_up2(x) - nhwc(y.detach())).abs().max()) <= 1e-12 * float(x.abs().max())
    assert float((P.bilinear_up2_adjoint(r) - nhwc(xt.grad)).abs().max()) <= 1e-12 * 36 * float(r.abs().max())
    for n in (H, W):                                          # every output a tap of input i comes from lies in i's candidate window
        assert bool(((P.bilinear_taps(n) > 0) <= (P.candidate_window(n) > 0)).all())
    assert torch.equal(P.window_abs_sum(r), torch.einsum("ph,qw,npqc->nhwc", P.candidate_window(H), P.candidate_window(W), r.abs()))


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic in float32
def taps_f32(n):
    """make_tap for every output index of an axis of n inputs: (i0, i1, l0, l1), the weights float32"""
    scale = f32(n - 1) / f32(2 * n - 1) if n > 1 else f32(0)
    src = scale * np.arange(2 * n, dtype=f32)
    assert src.dtype == f32
    i0 = np.minimum(src.astype(np.int64), n - 1)
    i1 = i0 + (i0 < n - 1)
    l1 = src - i0.astype(f32)
    l0 = f32(1) - l1
    return i0, i1, l0, l1


def emulate_fwd(x):
    N, H, W, C = x.shape
    y0, y1, ly0, ly1 = taps_f32(H)
    x0, x1, lx0, lx1 = taps_f32(W)
    lx0, lx1 = lx0[None, None, :, None], lx1[None, None, :, None]
    top = lx0 * x[:, y0][:, :, x0] + lx1 * x[:, y0][:, :, x1]
    bot = lx0 * x[:, y1][:, :, x0] + lx1 * x[:, y1][:, :, x1]
    out = ly0[None, :, None, None] * top + ly1[None, :, None, None] * bot
    assert out.dtype == f32
    return out


def candidate_weights(n):
    """[n, 6] float32: the weight of output 2i - 2 + k on input i, as the backward kernels form it; zero outside the image"""
    i0, i1, l0, l1 = taps_f32(n)
    w = np.zeros((n, 6), dtype=f32)
    for i in range(n):
        for k in range(6):
            o = 2 * i - 2 + k
            if 0 <= o < 2 * n:
                w[i, k] = (l0[o] if i0[o] == i else f32(0)) + (l1[o] if i1[o] == i else f32(0))
    return w


def emulate_bwd_gather(g):
    N, Ho, Wo, C = g.shape
    H, W = Ho // 2, Wo // 2
    wy, wx = candidate_weights(H), candidate_weights(W)
    acc = np.zeros((N, H, W, C), dtype=f32)
    for ky in range(6):
        yo = np.clip(2 * np.arange(H) - 2 + ky, 0, Ho - 1)
        for kx in range(6):
            xo = np.clip(2 * np.arange(W) - 2 + kx, 0, Wo - 1)
            w = wy[:, ky][:, None] * wx[:, kx][None, :]
            acc = acc + w[None, :, :, None] * g[:, yo][:, :, xo]
    assert acc.dtype == f32
    return acc


def emulate_bwd_walk(g):
    """returns (dx, whether the walk met a tap clamped at the last row)"""
    N, Ho, Wo, C = g.shape
    H, W = Ho // 2, Wo // 2
    wx = candidate_weights(W)
    h = np.zeros((N, Ho, W, C), dtype=f32)
    for k in range(6):
        xo = np.clip(2 * np.arange(W) - 2 + k, 0, Wo - 1)
        h = h + wx[:, k][None, None, :, None] * g[:, :, xo]
    i0, i1, l0, l1 = taps_f32(H)
    acc = np.zeros((N, H, W, C), dtype=f32)
    clamped = False
    for yo in range(Ho):
        if i1[yo] > i0[yo]:
            acc[:, i0[yo]] = acc[:, i0[yo]] + l0[yo] * h[:, yo]
            acc[:, i1[yo]] = acc[:, i1[yo]] + l1[yo] * h[:, yo]
        else:
            clamped = True
            acc[:, i0[yo]] = acc[:, i0[yo]] + (l0[yo] + l1[yo]) * h[:, yo]
    assert acc.dtype == f32 and h.dtype == f32
    return acc, clamped


def used(got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref.numpy())
    b = bound.numpy()
    assert ((b > 0) | (err == 0)).all()
    return float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0)))


def test_bilinear_forward_bound_holds_the_float32_emulation():
    worst = 0.0
    for C, hw, _ in G.BILINEAR_FWD:
        x = G.bilinear_fwd_input(C, hw)
        ref = P.bilinear_up2(x.double())
        frac = used(emulate_fwd(x.numpy()), ref, P.bilinear_fwd_bound(x.double(), ref))
        print(f"[pointwise_f32 emulation] forward C={C} {hw[0]}x{hw[1]}: {frac:.3f} of its bound")
        assert frac <= 1.0
        worst = max(worst, frac)
    print(f"[pointwise_f32 emulation] cvk_bilinear_up2_fwd: worst used fraction {worst:.3f}")
    assert worst >= 0.01


def test_bilinear_backward_bound_holds_both_summation_orders():
    worst = {"gather": 0.0, "walk": 0.0}
    clamp_seen = False
    for shape in G.BILINEAR_BWD + [(1,) + G.BILINEAR_BWD_LARGE[1:3] + (8,)]:
        N, H, W, C = shape
        go = G.bilinear_bwd_input(shape)
        ref = P.bilinear_up2_adjoint(go.double())
        bound = P.bilinear_bwd_bound(go.double(), H, W)
        walk, clamped = emulate_bwd_walk(go.numpy())
        clamp_seen |= clamped and H >= 2 and C % 4 == 0
        for order, got in (("gather", emulate_bwd_gather(go.numpy())), ("walk", walk)):
            frac = used(got, ref, bound)
            print(f"[pointwise_f32 emulation] backward {order} {'x'.join(map(str, shape))}: {frac:.3f} of its bound")
            assert frac <= 1.0
            worst[order] = max(worst[order], frac)
    print(f"[pointwise_f32 emulation] cvk_bilinear_up2_bwd: worst used fraction gather {worst['gather']:.3f}, walk {worst['walk']:.3f}")
    assert min(worst.values()) >= 0.01
    assert clamp_seen, "no walk case reaches the tap that is clamped at the last row"
