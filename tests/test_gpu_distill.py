"""The knowledge-distillation loss (cvk.DistillationLoss on cvk_kd_loss_fwd / _bwd) against its fp64 restatement on the CPU
(tests/distill_ref.py): loss, terms, record and dlogits over class counts and pairs of pixel strides on both sides of the staging
bound ((ld_s + 1) + (ld_t + 1) <= 64 stages both tiles in LDS, beyond it a thread walks its rows in global memory), crossed with
weights, ignore indices, temperatures, coefficients and both pixel sets; the gradient's padding columns at the C ABI; the degenerate
forms (kd = 0 is the weighted cross-entropy, ce = 0 needs no target, the student as its own teacher); the out-of-range and
all-ignored conventions; refusals; bitwise reproducibility; the bound form under GraphedStep and evaluate_report; one bf16-mode step.

Bound: the project's standing one for these losses, 1e-5 relative on the loss and on each term and 1e-5 of the largest gradient
magnitude.  On the CPU, torch's own fp32 arithmetic stays within 1.8e-7 on the loss and 8.0e-7 of the largest gradient over these
inputs, and the smallest K of the grid is 3.07, so relative bounds on K are meaningful (the test asserts K >= 0.1 on the reference).
Measured on an MI355X over the whole grid: at most 8.0e-8 on the loss and 8.7e-7 of the largest gradient magnitude; the student as its
own teacher gives K = 0 and a zero gradient exactly."""
import numpy as np
import pytest
import torch

from tests import distill_ref as R
from tests.test_gpu_ce_options import _logits, _targets, dev

pytestmark = pytest.mark.gpu

TOL = 1e-5
N, H, W = 2, 24, 30                                      # 1440 pixels: two workgroups, the second one partly filled
# (C, ld_s, ld_t): the first three are staged (ld_s + ld_t + 2 <= 64), the last two walk their rows in global memory
STRIDES = [(5, 5, 8), (12, 16, 12), (12, 12, 12), (33, 36, 36), (100, 100, 104)]


def _weight(C, weighted):
    gw = torch.Generator().manual_seed(7 * C)
    return (torch.rand(C, generator=gw) * 2 + 0.1).to(dev()) if weighted else None


def _pair(C, ld_s, ld_t, n=N, h=H, w=W):
    """Student and teacher logits drawn independently, each with its own pixel stride."""
    return _logits(n, C, h, w, ld_s, seed=C + ld_s), _logits(n, C, h, w, ld_t, seed=1000 + C + ld_t)


def _check_against_fp64(lf, x, z, t, w, case, gout=None):
    """One forward + backward of `lf` on the GPU against the fp64 restatement; prints the figures before it asserts."""
    import pytorch_camvid_amd as A
    ign = lf.ignore_index
    tau, t2 = A.distillation_scales(lf.temperature)
    x.grad = None
    loss = lf(x, t, z)
    g = torch.tensor(1.0) if gout is None else gout
    loss.backward(g.to(dev()))
    xr = x.detach().cpu().double().requires_grad_(True)
    tc = None if t is None else t.cpu()
    L, Hh, K, nD, agree = R.distill_loss(xr, None if z is None else z.detach().cpu().double(), tc, lf.ce, lf.kd, tau, t2,
                                         None if w is None else w.cpu().double(), ign, lf.distill_ignored)
    if lf.kd > 0:
        assert K.item() >= 0.1, (case, K.item())         # a relative bound on K needs a K that is no difference of near-equal numbers
    L.backward(g.double())
    dref = xr.grad
    assert loss.dim() == 0
    got = loss.item()
    rec = lf.last_record.cpu().double()
    d = x.grad.cpu().double()
    e_l = abs(got - L.item()) / abs(L.item())
    e_g = ((d - dref).abs().max() / dref.abs().max()).item()
    print(f"{case}: loss {got:.7f} ref {L.item():.7f} rel {e_l:.2e}; H {rec[4].item():.7f} ref {Hh.item():.7f}; K {rec[5].item():.7f} "
          f"ref {K.item():.7f}; grad rel-to-max {e_g:.2e}")
    assert np.isfinite(got) and torch.isfinite(d).all(), case
    assert e_l <= TOL, (case, got, L.item())
    assert e_g <= TOL, (case, e_g)
    lab, in_d, _ = R.pixel_sets(tc, x.shape[0] * x.shape[2] * x.shape[3], x.shape[1], ign, lf.distill_ignored)
    # the record: [L, valid, out of range, sum w[t], H, K, |D|, agree, agree / |D|]; the integers exactly
    assert rec.numel() == 9 and rec[0].item() == got, case
    assert rec[1].item() == (int(lab.sum()) if t is not None else lab.numel()) and rec[2].item() == 0, (case, rec)
    assert rec[6].item() == nD == int(in_d.sum()), (case, rec, nD)
    assert torch.equal(lf.last_terms.cpu().double(), rec[4:6]) and lf.last_agreement.item() == rec[8].item(), case
    if lf.ce > 0:
        assert abs(rec[4].item() - Hh.item()) <= TOL * abs(Hh.item()), (case, rec, Hh)
    else:
        assert rec[4].item() == 0.0, case
    if t is not None:
        wsum = float(lab.sum()) if w is None else w.cpu().double()[tc.reshape(-1)[lab]].sum().item()
        assert abs(rec[3].item() - wsum) <= TOL * wsum, (case, rec, wsum)
    if lf.kd > 0:
        assert abs(rec[5].item() - K.item()) <= TOL * abs(K.item()), (case, rec, K)
        assert rec[7].item() == agree, (case, rec, agree)
        assert rec[8].item() == float(np.float32(agree / nD)), (case, rec)
    else:
        assert rec[5].item() == 0.0 and rec[7].item() == 0.0 and rec[8].item() == 0.0, case
    # rows that enter neither term are exactly 0
    active = (lab if lf.ce > 0 else torch.zeros_like(lab)) | (in_d if lf.kd > 0 else torch.zeros_like(in_d))
    idle = (~active).reshape(x.shape[0], 1, x.shape[2], x.shape[3]).expand_as(d)
    assert (d[idle] == 0).all(), case
    return e_l, e_g


@pytest.mark.parametrize("ignore_index", [-100, 11])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C,ld_s,ld_t", STRIDES)
def test_loss_terms_record_and_grad_match_fp64(C, ld_s, ld_t, weighted, ignore_index):
    import pytorch_camvid_amd as A
    x, z = _pair(C, ld_s, ld_t)
    x.requires_grad_(True)
    t = _targets(N, H, W, C, ignore_index, seed=C).to(dev())
    w = _weight(C, weighted)
    gg = torch.Generator().manual_seed(11 * C + ld_t)
    worst = [0.0, 0.0]
    for T in (1.0, 2.0, 4.0):
        for ce, kd in ((1.0, 0.0), (0.0, 1.0), (1.0, 0.5)):
            for ignored in (False, True):
                gout = torch.rand((), generator=gg) + 0.5
                lf = A.DistillationLoss(ce, kd, T, weight=w, ignore_index=ignore_index, distill_ignored=ignored)
                e = _check_against_fp64(lf, x, z if kd > 0 else None, t, w, (C, ld_s, ld_t, weighted, ignore_index, T, ce, kd, ignored),
                                        gout)
                worst = [max(a, b) for a, b in zip(worst, e)]
                assert A.last_ce_status() == (int((t != ignore_index).sum()), 0)
    print(f"worst over the case: loss rel {worst[0]:.2e}, grad rel-to-max {worst[1]:.2e}")


@pytest.mark.parametrize("C,ld_s,ld_t", STRIDES)
def test_padding_columns_at_the_c_abi(C, ld_s, ld_t):
    """dlogits asked for at a wider pixel stride than the logits': columns [C, ld_d) exactly 0 over a NaN prefill, everything finite,
    and the first C columns bitwise the autograd path's gradient."""
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd.functional import _as_nhwc
    x, z = _pair(C, ld_s, ld_t)
    x.requires_grad_(True)
    t = _targets(N, H, W, C, 11, seed=C).to(dev())
    w = _weight(C, True)
    tau, t2 = A.distillation_scales(2.0)
    lg, ls = _as_nhwc(x.detach())
    zg, lt = _as_nhwc(z)
    assert (ls, lt) == (ld_s, ld_t)
    M = N * H * W
    lib = A.load_library()
    rec = torch.empty(lib.cvk_kd_loss_record_floats(), device=dev())
    part = torch.empty(lib.cvk_kd_loss_part_floats(M), device=dev())
    s = torch.cuda.current_stream().cuda_stream
    assert lib.cvk_kd_loss_fwd(lg.data_ptr(), ld_s, zg.data_ptr(), ld_t, t.data_ptr(), w.data_ptr(), 1.0, 0.5, tau, t2, 1, part.data_ptr(),
                               rec.data_ptr(), M, C, 11, s) == 0
    ld_d = ld_s + 3
    dl = torch.full((M, ld_d), float("nan"), device=dev())
    assert lib.cvk_kd_loss_bwd(lg.data_ptr(), ld_s, zg.data_ptr(), ld_t, t.data_ptr(), w.data_ptr(), 1.0, 0.5, tau, t2, 1, rec.data_ptr(),
                               None, 1.0, dl.data_ptr(), ld_d, M, C, 11, s) == 0
    assert (dl[:, C:] == 0).all() and torch.isfinite(dl).all()
    lf = A.DistillationLoss(1.0, 0.5, 2.0, weight=w, ignore_index=11, distill_ignored=True)
    lf(x, t, z).backward()
    assert torch.equal(lf.last_record, rec)
    assert torch.equal(dl[:, :C].view(N, H, W, C).permute(0, 3, 1, 2), x.grad)


def _run(lf, x, *args):
    x.grad = None
    l = lf(x, *args)
    l.backward()
    return l.detach().clone(), x.grad.clone()


@pytest.mark.parametrize("C,ld_s,ld_t", [(12, 16, 12), (33, 36, 36)])
def test_degenerate_forms(C, ld_s, ld_t):
    import pytorch_camvid_amd as A
    x, z = _pair(C, ld_s, ld_t)
    x.requires_grad_(True)
    t = _targets(N, H, W, C, 11, seed=C).to(dev())
    w = _weight(C, True)
    # kd = 0: the weighted cross-entropy, with or without a teacher tensor
    for weight in (None, w):
        l0, d0 = _run(A.CrossEntropyLoss(weight=weight, ignore_index=11), x, t)
        for teacher in (None, z):
            l1, d1 = _run(A.DistillationLoss(1.0, 0.0, weight=weight, ignore_index=11), x, t, teacher)
            print(f"kd = 0: loss rel {abs(l1.item() - l0.item()) / abs(l0.item()):.2e}, grad rel-to-max "
                  f"{((d1 - d0).abs().max() / d0.abs().max()).item():.2e}")
            assert abs(l1.item() - l0.item()) <= TOL * abs(l0.item())
            assert (d1 - d0).abs().max().item() <= TOL * d0.abs().max().item()
    # ce = 0 needs no target: bitwise the loss, the terms and the gradient of an all-valid target
    lf_a, lf_b = A.DistillationLoss(0.0, 1.0, 2.0), A.DistillationLoss(0.0, 1.0, 2.0)
    la, da = _run(lf_a, x, None, z)
    lb, db = _run(lf_b, x, torch.zeros_like(t), z)
    assert torch.equal(la, lb) and torch.equal(da, db) and torch.isfinite(la).item()
    assert torch.equal(lf_a.last_record[4:], lf_b.last_record[4:]) and lf_a.last_record[6].item() == N * H * W
    assert A.last_ce_status() == (N * H * W, 0)
    # the student as its own teacher (the same values at the teacher's stride): K and the gradient vanish
    own = _logits(N, C, H, W, ld_t, seed=5)
    own.copy_(x.detach())
    lf = A.DistillationLoss(0.0, 1.0, 4.0)
    l_ind, d_ind = _run(lf, x, None, z)
    l_own, d_own = _run(lf, x, None, own)
    print(f"own teacher: |K| {abs(l_own.item()):.2e} of {l_ind.item():.4f}, grad max {d_own.abs().max().item():.2e} of "
          f"{d_ind.abs().max().item():.2e}; agreement {lf.last_agreement.item()}")
    assert abs(l_own.item()) <= TOL * abs(l_ind.item())
    assert d_own.abs().max().item() <= TOL * d_ind.abs().max().item()
    assert lf.last_agreement.item() == 1.0
    # the module, the functional form and the bound form return the same bits
    lf = A.DistillationLoss(1.0, 0.5, 2.0, weight=w, ignore_index=11, distill_ignored=True)
    l1 = lf(x, t, z)
    l2 = A.distillation_loss(x, t, z, 1.0, 0.5, 2.0, weight=w, ignore_index=11, distill_ignored=True)
    bound = lf.bind(z)
    l3 = bound(x, t)
    assert torch.equal(l1, l2) and torch.equal(l1, l3) and bound.loss is lf
    # the attributes are read at every call: a temperature schedule is an assignment
    lf.temperature = 4.0
    assert torch.equal(lf(x, t, z), A.DistillationLoss(1.0, 0.5, 4.0, weight=w, ignore_index=11, distill_ignored=True)(x, t, z))
    assert not torch.equal(lf(x, t, z), l1)
    # a teacher that requires a gradient gets none, and grad_scale multiplies the backward only
    zr = z.detach().clone().requires_grad_(True)
    l4, d4 = _run(A.DistillationLoss(1.0, 0.5, 2.0, weight=w, ignore_index=11, distill_ignored=True, grad_scale=0.25), x, t, zr)
    assert zr.grad is None and torch.equal(l4, l1)
    _, d1 = _run(A.DistillationLoss(1.0, 0.5, 2.0, weight=w, ignore_index=11, distill_ignored=True), x, t, z)
    assert (d4 - 0.25 * d1).abs().max().item() <= 1e-6 * d1.abs().max().item()
    # a teacher in another memory layout (plain NCHW) is copied once and gives the same bits
    assert torch.equal(lf.bind(z.contiguous())(x, t), lf(x, t, z))


@pytest.mark.parametrize("C,ld_s,ld_t", [(12, 16, 12), (33, 36, 36)])
def test_out_of_range_targets_and_all_ignored(C, ld_s, ld_t):
    import pytorch_camvid_amd as A
    x, z = _pair(C, ld_s, ld_t, 2, 16, 20)
    w = torch.rand(C, device=dev()) + 0.5
    t = _targets(2, 16, 20, C, -100, seed=2).to(dev())
    t[0, 0, :3] = C                                      # three targets past the last class
    t[1, 5, 7] = -1
    for ce, kd in ((1.0, 0.0), (0.0, 1.0), (1.0, 0.5)):
        for ignored in (False, True):
            xg = x.detach().clone().requires_grad_(True)
            lf = A.DistillationLoss(ce, kd, 2.0, weight=w, distill_ignored=ignored)
            l = lf(xg, t, z)
            assert torch.isnan(l).item()
            assert lf.last_record[2].item() == 4
            with pytest.raises(IndexError, match="4 pixels"):
                A.last_ce_status()
            l.backward()
            bad = ((t == C) | (t == -1)).unsqueeze(1).expand_as(xg)
            assert (xg.grad[bad] == 0).all() and torch.isfinite(xg.grad).all() and (xg.grad != 0).any()
    # every pixel ignored: H is 0/0 = NaN as the cross-entropy's mean; K too unless the ignored pixels are distilled
    t_ign = torch.full_like(t, -100)
    xg = x.detach().clone().requires_grad_(True)
    for ce, kd, ignored in ((1.0, 0.0, False), (1.0, 0.5, False), (1.0, 0.5, True)):
        lf = A.DistillationLoss(ce, kd, 2.0, weight=w, distill_ignored=ignored)
        l = lf(xg, t_ign, z)
        assert torch.isnan(l).item() and torch.isnan(lf.last_terms[0]).item()
        assert A.last_ce_status() == (0, 0)
    lf = A.DistillationLoss(0.0, 1.0, 2.0)
    assert torch.isnan(lf(xg, t_ign, z)).item() and lf.last_record[6].item() == 0          # D is empty
    lf = A.DistillationLoss(0.0, 1.0, 2.0, distill_ignored=True)
    l = lf(xg, t_ign, z)
    assert torch.isfinite(l).item() and lf.last_record[6].item() == t.numel() and lf.last_terms[0].item() == 0.0
    l.backward()
    assert torch.isfinite(xg.grad).all() and (xg.grad != 0).any()


def test_refusals():
    import pytorch_camvid_amd as A
    C = 12
    x, z = _pair(C, 16, 12, 2, 16, 20)
    t = _targets(2, 16, 20, C, -100, seed=2).to(dev())
    lf = A.DistillationLoss()
    with pytest.raises((ValueError, RuntimeError), match=r"student \[2, 12, 16, 20\].*teacher \[2, 12, 16, 24\]"):
        lf(x, t, torch.zeros(2, C, 16, 24, device=dev()))
    with pytest.raises((ValueError, RuntimeError), match=r"student \[2, 12, 16, 20\].*teacher \[2, 11, 16, 20\]"):
        lf(x, t, z[:, :11])
    with pytest.raises((ValueError, RuntimeError), match="float64"):
        lf(x, t, z.double())
    with pytest.raises((ValueError, RuntimeError), match="teacher .* on cpu"):
        lf(x, t, z.cpu())
    with pytest.raises(ValueError, match="target=None needs ce == 0"):
        lf(x, None, z)
    with pytest.raises(ValueError, match="needs kd == 0"):
        lf(x, t)
    with pytest.raises(RuntimeError, match="float32 logits"):
        lf(x.double(), t, z.double())
    with pytest.raises(RuntimeError, match="int64 target"):
        lf(x, t.int(), z)
    with pytest.raises(ValueError, match="Expected target size"):
        lf(x, t[:, :-1], z)
    with pytest.raises(RuntimeError, match="all 12 classes"):
        A.DistillationLoss(weight=torch.ones(11, device=dev()))(x, t, z)
    with pytest.raises(RuntimeError, match="no implicit copy"):
        A.DistillationLoss(weight=torch.ones(C))(x, t, z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lf(x.cpu(), t.cpu(), z.cpu())
    big = torch.zeros(1, 129, 4, 4, device=dev())
    with pytest.raises(RuntimeError, match="1 to 128 classes"):
        lf(big, torch.zeros(1, 4, 4, dtype=torch.int64, device=dev()), big.clone())


@pytest.mark.parametrize("shape,ld_s,ld_t", [((2, 12, 24, 30), 12, 12), ((4, 12, 48, 64), 16, 16), ((2, 33, 24, 30), 36, 36)])
def test_runs_are_bitwise_reproducible(shape, ld_s, ld_t):
    import pytorch_camvid_amd as A
    n, C, h, w_ = shape
    x, z = _pair(C, ld_s, ld_t, n, h, w_)
    x.requires_grad_(True)
    t = _targets(n, h, w_, C, -100, seed=4).to(dev())
    w = torch.rand(C, device=dev()) + 0.1
    lf = A.DistillationLoss(1.0, 0.5, 4.0, weight=w, distill_ignored=True)

    def run():
        x.grad = None
        l = lf(x, t, z)
        l.backward()
        return l.detach().clone(), lf.last_record.clone(), x.grad.clone()

    a, b = run(), run()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.isfinite(a[0]).item() and torch.isfinite(a[1]).all()


def _batch(seed):
    gb = torch.Generator().manual_seed(seed)
    return torch.randn(2, 3, 48, 64, generator=gb).to(dev()), torch.randint(0, 12, (2, 48, 64), generator=gb).to(dev())


def _loss_fn():
    import pytorch_camvid_amd as A
    w = (torch.rand(12, generator=torch.Generator().manual_seed(8)) + 0.2).to(dev())
    return A.DistillationLoss(1.0, 0.5, 2.0, weight=w, ignore_index=11, distill_ignored=True)


def _teacher():
    import pytorch_camvid_amd as A
    torch.manual_seed(5)
    return A.UNet(3, 12).to(dev()).eval()


def _teacher_logits(teacher, x):
    with torch.no_grad():
        return teacher(x)


@pytest.mark.parametrize("with_optimizer", [False, True])
def test_graphed_step_with_the_bound_loss_is_bitwise_the_eager_loop(with_optimizer):
    """The student's step captured with kd.bind(buf); the teacher runs outside the graph and its logits are copied into buf before each
    replay.  Three replays against the eager loop: gradients (no optimizer) or parameters and momentum (FlatSGD) bitwise."""
    import pytorch_camvid_amd as A
    teacher = _teacher()
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    opt = A.FlatSGD(net, lr=0.01, momentum=0.9) if with_optimizer else None
    st0 = {k: v.clone() for k, v in net.state_dict().items()}
    lossf, eager = _loss_fn(), _loss_fn()                  # two modules: the views are of a module's own last record
    x0, t0 = _batch(1)
    buf = _teacher_logits(teacher, x0).clone(memory_format=torch.channels_last)
    bound = lossf.bind(buf)
    gs = A.GraphedStep(net, bound, x0, t0, optimizer=opt)
    net.load_state_dict(st0)                               # the capture's warm-up passes advanced the BatchNorm statistics
    torch.manual_seed(0)
    ref = A.UNet(3, 12).to(dev()).train()
    opt_ref = A.FlatSGD(ref, lr=0.01, momentum=0.9) if with_optimizer else None
    ref.load_state_dict(st0)
    for it in range(3):
        x, t = _batch(10 + it)
        zt = _teacher_logits(teacher, x)
        buf.copy_(zt)
        la = gs.replay(x, t)
        if opt_ref is not None:
            opt_ref.zero_grad()
        else:
            for p in ref.parameters():
                p.grad = None
        lb = eager(ref(x), t, zt)
        lb.backward()
        if opt_ref is not None:
            opt_ref.step()
        assert torch.equal(la, lb), (it, la.item(), lb.item())
        assert torch.isfinite(la).item()
        assert torch.equal(lossf.last_record, eager.last_record), it
        for (k, p), q in zip(net.named_parameters(), ref.parameters()):
            assert torch.equal(p, q) if with_optimizer else torch.equal(p.grad, q.grad), (it, k)
    if with_optimizer:
        assert torch.equal(opt._buf, opt_ref._buf) and not torch.equal(st0["output.conv.0.weight"], net.state_dict()["output.conv.0.weight"])


def test_evaluate_report_takes_the_bound_loss():
    import pytorch_camvid_amd as A
    teacher = _teacher()
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev())
    batches = [_batch(20), ]
    lf = _loss_fn()
    buf = _teacher_logits(teacher, batches[0][0])
    rep = A.evaluate_report(net, batches, loss_fn=lf.bind(buf))
    net.eval()
    with torch.no_grad():
        want = lf(net(batches[0][0]), batches[0][1], buf).item()
    assert np.isfinite(rep["loss"]) and abs(rep["loss"] - want) <= 1e-6 * abs(want)


def test_one_step_in_bf16_mode():
    import pytorch_camvid_amd as A
    teacher = _teacher()
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    A.set_conv_precision(net, "bf16")
    x, t = _batch(3)
    y = net(x)
    assert y.dtype == torch.float32                        # the logits stay fp32 in bf16 mode
    lf = _loss_fn()
    loss = lf(y, t, _teacher_logits(teacher, x))
    loss.backward()
    assert torch.isfinite(loss).item() and torch.isfinite(lf.last_record).all()
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
