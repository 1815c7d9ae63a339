"""tests/elem_bf16_ref.py is right: the fp64 restatements that tests/test_gpu_elem_bf16.py holds the HIP kernels of
csrc/elem_bf16.hip against are themselves checked here, in fp64 on the CPU, against torch's operators and autograd (the reference's
nn.BatchNorm2d + ReLU, MaxPool2d(2,2), bilinear x2 with align_corners=True: models/unet.py:12-13,25,92).  fp64 against fp64, two
orders of evaluation: 1e-12 relative to the tensors' scale.  The GPU file's input generators run here too: no case may hold an
element whose ReLU mask is ambiguous in fp32 (the exclusion band), and every case must hold the exact-zero edge."""
import pytest
import torch
import torch.nn.functional as F

from tests import elem_bf16_ref as R
from tests import test_gpu_elem_bf16 as G

EPS = 1e-5
TIGHT = 1e-12


def close(a, b):
    return float((a - b).abs().max()) <= TIGHT * max(1.0, float(b.abs().max()))


def _bn_problem(M, C, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(M, C, generator=g, dtype=torch.float64) * 1.3 + 0.2
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    dout = torch.randn(M, C, generator=g, dtype=torch.float64)
    return y, gamma, beta, dout


@pytest.mark.parametrize("M,C", [(70, 12), (71, 64), (15, 8)])
def test_bn_backward_matches_autograd_in_training_mode(M, C):
    y, gamma, beta, dout = _bn_problem(M, C, M + C)
    yr, gr, br = y.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    F.relu(F.batch_norm(yr, None, None, gr, br, training=True, eps=EPS)).backward(dout)
    mean, rstd = y.mean(0), (y.var(0, unbiased=False) + EPS).rsqrt()
    scale = gamma * rstd
    shift = beta - mean * scale
    mask, g, gx, band = R.bn_bwd_terms(dout, y, scale, shift, mean, rstd)
    assert not bool(band.any())
    assert close(g.sum(0), br.grad) and close(gx.sum(0), gr.grad)
    dy = R.bn_bwd_dy(dout, y, scale, shift, mean, rstd, gx.sum(0), g.sum(0), M, 1)
    assert close(dy, yr.grad)
    assert close(R.apply(y, scale, shift), F.relu(F.batch_norm(y, None, None, gamma, beta, training=True, eps=EPS)))


def test_bn_backward_matches_autograd_with_running_statistics():
    M, C = 70, 24
    y, gamma, beta, dout = _bn_problem(M, C, 3)
    g0 = torch.Generator().manual_seed(4)
    rm, rv = 0.2 * torch.randn(C, generator=g0, dtype=torch.float64), torch.rand(C, generator=g0, dtype=torch.float64) + 0.5
    yr, gr, br = y.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    F.relu(F.batch_norm(yr, rm, rv, gr, br, training=False, eps=EPS)).backward(dout)
    rstd = (rv + EPS).rsqrt()
    scale = gamma * rstd
    shift = beta - rm * scale
    _, g, gx, _ = R.bn_bwd_terms(dout, y, scale, shift, rm, rstd)
    assert close(g.sum(0), br.grad) and close(gx.sum(0), gr.grad)
    assert close(R.bn_bwd_dy(dout, y, scale, shift, rm, rstd, None, None, M, 0), yr.grad)


def test_relu_mask_is_strict_and_exact_zeros_are_outside_the_band():
    """z == 0 passes no gradient (torch's ReLU backward), and an exact zero from y = 0, shift = 0 is exact in every precision: it is
    not an ambiguous element, while a z within fp32 rounding of zero is."""
    y = torch.tensor([[0.0, 1.0, 1.0]], dtype=torch.float64)
    scale = torch.tensor([1.5, 2.0, 2.0], dtype=torch.float64)
    shift = torch.tensor([0.0, -2.0, -2.0 - 1e-9], dtype=torch.float64)
    zero, one = torch.zeros(3, dtype=torch.float64), torch.ones(3, dtype=torch.float64)
    dout = torch.ones(1, 3, dtype=torch.float64)
    mask, g, _, band = R.bn_bwd_terms(dout, y, scale, shift, zero, one)
    assert mask.tolist() == [[False, False, False]] and g.tolist() == [[0.0, 0.0, 0.0]]
    assert band.tolist() == [[False, True, True]]
    yr = y.clone().requires_grad_(True)
    F.relu(yr * scale + shift).backward(dout)
    assert yr.grad.tolist() == [[0.0, 0.0, 0.0]]


def test_pool2x2_and_its_scatter_match_torch():
    g = torch.Generator().manual_seed(2)
    x = (torch.randint(-2, 4, (2, 5, 7, 8), generator=g).double() * 0.5).clamp_min(0.0)          # ties and dead cells
    v, idx = F.max_pool2d(x.permute(0, 3, 1, 2), 2, return_indices=True)
    assert torch.equal(R.pool2x2(x), v.permute(0, 2, 3, 1))
    r = torch.randn(2, 2, 3, 8, generator=g, dtype=torch.float64)
    want = F.max_unpool2d(r.permute(0, 3, 1, 2).contiguous(), idx, 2, output_size=(5, 7)).permute(0, 2, 3, 1)
    assert torch.equal(R.pool2x2_scatter(r, x), want)


SIZES = [(h, w) for h in (1, 2, 3, 5) for w in (1, 2, 3, 5)] + [(9, 16)]


@pytest.mark.parametrize("H,W", SIZES)
def test_bilinear_up2_and_its_adjoint(H, W):
    g = torch.Generator().manual_seed(10 * H + W)
    x = torch.randn(2, H, W, 3, generator=g, dtype=torch.float64)
    go = torch.randn(2, 2 * H, 2 * W, 3, generator=g, dtype=torch.float64)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    want = F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=True)
    up = R.bilinear_up2(x)
    assert close(up, want.detach().permute(0, 2, 3, 1))
    adj = R.bilinear_up2_adjoint(go)
    assert abs(float((up * go).sum()) - float((x * adj).sum())) <= TIGHT * float(up.abs().sum() + 1)
    want.backward(go.permute(0, 3, 1, 2))
    assert close(adj, xr.grad.permute(0, 2, 3, 1))
    for n in (H, W):                                  # interpolation weights: non-negative, rows sum to 1
        A = R.bilinear_taps(n)
        assert bool((A >= 0).all()) and close(A.sum(1), torch.ones(2 * n, dtype=torch.float64))


def test_bf16_half_ulp():
    for k in (-126, -20, -1, 0, 1, 7, 100, 127):
        p = torch.tensor([2.0 ** k], dtype=torch.float64)
        below, above = torch.nextafter(p, torch.zeros_like(p)), torch.nextafter(p, 2 * p)
        assert float(R.bf16_half_ulp(p)) == 2.0 ** (k - 8) and float(R.bf16_half_ulp(-p)) == 2.0 ** (k - 8)
        assert float(R.bf16_half_ulp(above)) == 2.0 ** (k - 8)
        assert float(R.bf16_half_ulp(below)) == 2.0 ** (max(k, -125) - 9)
    for tiny in (0.0, 2.0 ** -140, 2.0 ** -127):      # below the normal range: the spacing of the smallest normal binade
        assert float(R.bf16_half_ulp(torch.tensor([tiny], dtype=torch.float64))) == 2.0 ** -134
    # it is what round-to-nearest commits: never more, and a tie commits exactly that much
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0), dtype=torch.float64) * 37.0
    assert bool(((R.rne_bf16(x).double() - x).abs() <= R.bf16_half_ulp(x)).all())
    tie = torch.tensor([1.0 + 2.0 ** -8, 3.0 + 3 * 2.0 ** -7], dtype=torch.float64)
    assert torch.equal((R.rne_bf16(tie).double() - tie).abs(), R.bf16_half_ulp(tie))
    assert R.rne_bf16(tie).double().tolist() == [1.0, 3.0 + 2.0 ** -5]              # ties go to the even significand (down, then up)


@pytest.mark.parametrize("name", list(G.BN_CASES) + list(G.APPLY_CASES))
def test_gpu_generators_hold_no_ambiguous_element_and_the_zero_edge(name):
    """What test_gpu_elem_bf16.py assumes of its inputs, checked without a GPU: zero elements in the exclusion band (the cap is 1e-5 of
    the elements and at most 8; for these sizes that is 0, or 1 for the one of 156 000 elements), and in channel 0 elements with z == 0 exactly."""
    if name in G.BN_CASES:
        shape, _, f32, _, _ = G.BN_CASES[name]
    else:
        shape, f32 = G.APPLY_CASES[name][0], 0
    inp = G.bn_inputs(shape, G.case_seed(name), f32)
    q = {k: v.double() for k, v in inp.items()}
    mask, g, gx, band = R.bn_bwd_terms(q["dout"], q["y"], q["scale"], q["shift"], q["mean"], q["rstd"])
    assert int(band.sum()) == 0 and G.excluded_cap(band.numel()) <= 1
    z0 = (q["y"][:, 0] * q["scale"][0] + q["shift"][0]) == 0
    assert int(z0.sum()) >= q["y"].shape[0] // 3 and not bool(mask[:, 0][z0].any())
    assert all(v.dtype == (torch.float32 if k != "y" and (k != "dout" or f32) else torch.bfloat16) for k, v in inp.items())


def test_generator_at_four_million_elements_stays_under_the_cap():
    """The generator of the 128 MiB case at 1/16 of its size (the device draws other numbers from the same distributions; the GPU
    test asserts the cap on its own inputs)."""
    shape = (1, 256, 256, 64)
    inp = G.bn_inputs(shape, 9, 0)
    q = {k: v.double() for k, v in inp.items()}
    _, _, _, band = R.bn_bwd_terms(q["dout"], q["y"], q["scale"], q["shift"], q["mean"], q["rstd"])
    assert int(band.sum()) == 0 and G.excluded_cap(band.numel()) == 8
