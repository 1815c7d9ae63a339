"""The fused focal + soft-Dice loss (cvk.SegmentationLoss on cvk_seg_loss_fwd / _bwd) against its fp64 restatement on the CPU
(tests/seg_loss_ref.py): loss, terms, per-class Dice and dlogits over the grid of class counts, pixel strides, weights and ignore
indices of test_gpu_ce_options.py crossed with gamma, the coefficients, both averages and the smoothing; gamma = 0 / dice = 0 against
cvk.CrossEntropyLoss; saturated pixels; the out-of-range and all-ignored conventions; bitwise reproducibility; a short UNet training
run against the reference graph; the step replayed from a captured graph; one step in bf16 mode.

Bound: 1e-5 of the largest reference magnitude for the loss and the gradient, the bound test_gpu_ce_options.py holds the _ex kernels
to (a plain fp32 torch restatement of this loss stays within 8.4e-7 of fp64 on these inputs).  Measured on an MI355X over the whole
grid: at most 1.5e-7 on the loss and 7.5e-7 of the largest gradient magnitude."""
import numpy as np
import pytest
import torch

from tests import seg_loss_ref as R
from tests.test_gpu_ce_options import _logits, _targets, _task, _train, dev

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _check_against_fp64(lf, x, t, w, case, gout=None):
    """One forward + backward of `lf` on the GPU against the fp64 restatement; prints the figures before it asserts."""
    ign = lf.ignore_index
    x.grad = None
    loss = lf(x, t)
    g = torch.tensor(1.0) if gout is None else gout
    loss.backward(g.to(dev()))
    xr = x.detach().cpu().double().requires_grad_(True)
    L, F, D, dc = R.seg_loss(xr, t.cpu(), lf.ce, lf.dice, focal_gamma=lf.focal_gamma, weight=None if w is None else w.cpu().double(),
                             ignore_index=ign, dice_smooth=lf.dice_smooth, dice_average=lf.dice_average)
    L.backward(g.double())
    dref = xr.grad
    assert loss.dim() == 0
    got = loss.item()
    e_l = abs(got - L.item()) / max(abs(L.item()), 1e-30)
    d = x.grad.cpu().double()
    e_g = ((d - dref).abs().max() / dref.abs().max()).item()
    terms = lf.last_terms.cpu().double()
    dice = lf.last_dice.cpu().double()
    print(f"{case}: loss {got:.7f} ref {L.item():.7f} rel {e_l:.2e}; grad rel-to-max {e_g:.2e}")
    assert np.isfinite(got) and torch.isfinite(d).all(), case
    assert e_l <= TOL, (case, got, L.item())
    assert e_g <= TOL, (case, e_g)
    if lf.ce > 0:
        assert abs(terms[0].item() - F.item()) <= TOL * abs(F.item()), (case, terms, F)
    else:
        assert terms[0].item() == 0.0, case
    if lf.dice > 0:
        assert abs(terms[1].item() - D.item()) <= TOL * max(abs(D.item()), dc.abs().max().item()), (case, terms, D)
        assert dice.shape == dc.shape and (dice - dc.detach()).abs().max() <= TOL * dc.abs().max(), (case, dice, dc)
        assert ((dice == 0) == (dc == 0)).all(), case
    else:
        assert terms[1].item() == 0.0 and (dice == 0).all(), case
    assert (d[(t.cpu() == ign).unsqueeze(1).expand_as(d)] == 0).all(), case


@pytest.mark.parametrize("ignore_index", [-100, 11])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C,ld", [(5, 5), (5, 8), (12, 16), (33, 36), (100, 100), (100, 104)])
def test_loss_terms_and_grad_match_fp64(C, ld, weighted, ignore_index):
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd.functional import _as_nhwc
    N, H, W = 2, 24, 30                                  # 1440 pixels: two workgroups, the second one partly filled
    x = _logits(N, C, H, W, ld, seed=C + ld).requires_grad_(True)
    t = _targets(N, H, W, C, ignore_index, seed=C)
    t[t == 1] = 0                                        # class 1 never occurs: "present" and "all" differ
    t = t.to(dev())
    gw = torch.Generator().manual_seed(7 * C)
    w = (torch.rand(C, generator=gw) * 2 + 0.1).to(dev()) if weighted else None
    for gamma in (0.0, 0.5, 2.0):
        for ce, dice in ((1.0, 0.0), (0.0, 1.0), (1.0, 0.5)):
            for average in ("present", "all"):
                for s in (0.0, 1.0):
                    gout = torch.rand((), generator=gw) + 0.5
                    lf = A.SegmentationLoss(ce, dice, focal_gamma=gamma, weight=w, ignore_index=ignore_index, dice_smooth=s,
                                            dice_average=average)
                    _check_against_fp64(lf, x, t, w, (C, ld, weighted, ignore_index, gamma, ce, dice, average, s), gout)
                    assert A.last_ce_status() == (int((t != ignore_index).sum()), 0)
    # the padding columns [C, ld) of the gradient's storage are exactly 0: ask for the gradient at the padded pixel stride
    lg, _ = _as_nhwc(x.detach())
    M = N * H * W
    lib = A.load_library()
    rec = torch.empty(lib.cvk_seg_loss_record_floats(C), device=dev())
    part = torch.empty(lib.cvk_seg_loss_part_floats(M, C), device=dev())
    s = torch.cuda.current_stream().cuda_stream
    wp = w.data_ptr() if w is not None else None
    assert lib.cvk_seg_loss_fwd(lg.data_ptr(), ld, t.data_ptr(), wp, 1.0, 0.5, 2.0, 1.0, 0, part.data_ptr(), rec.data_ptr(), M, C,
                                ignore_index, s) == 0
    ld_d = ld + 3
    dl = torch.full((M, ld_d), float("nan"), device=dev())
    assert lib.cvk_seg_loss_bwd(lg.data_ptr(), ld, t.data_ptr(), wp, 1.0, 0.5, 2.0, rec.data_ptr(), None, 1.0, dl.data_ptr(), ld_d, M, C,
                                ignore_index, s) == 0
    assert (dl[:, C:] == 0).all() and torch.isfinite(dl).all()
    x.grad = None
    A.SegmentationLoss(1.0, 0.5, focal_gamma=2.0, weight=w, ignore_index=ignore_index)(x, t).backward()
    assert torch.equal(dl[:, :C].view(N, H, W, C).permute(0, 3, 1, 2), x.grad)
    # the functional form and the two conveniences take the same path
    l1 = A.segmentation_loss(x, t, 1.0, 0.5, focal_gamma=2.0, weight=w, ignore_index=ignore_index)
    l2 = A.SegmentationLoss(1.0, 0.5, focal_gamma=2.0, weight=w, ignore_index=ignore_index)(x, t)
    assert torch.equal(l1, l2)
    assert torch.equal(A.FocalLoss(2.0, w, ignore_index)(x, t), A.SegmentationLoss(1.0, 0.0, focal_gamma=2.0, weight=w,
                                                                                 ignore_index=ignore_index)(x, t))
    assert torch.equal(A.DiceLoss(0.0, "all", ignore_index)(x, t), A.SegmentationLoss(0.0, 1.0, dice_smooth=0.0, dice_average="all",
                                                                                     ignore_index=ignore_index)(x, t))


@pytest.mark.parametrize("weighted", [False, True])
def test_gamma_0_without_dice_is_the_cross_entropy(weighted):
    import pytorch_camvid_amd as A
    C = 12
    x = _logits(4, C, 48, 64, 16, seed=3).requires_grad_(True)
    t = _targets(4, 48, 64, C, -100, seed=4).to(dev())
    w = (torch.rand(C, generator=torch.Generator().manual_seed(5)) + 0.1).to(dev()) if weighted else None

    def run(lf):
        x.grad = None
        l = lf(x, t)
        l.backward()
        return l.detach().clone(), x.grad.clone()

    l0, d0 = run(A.CrossEntropyLoss(weight=w))
    l1, d1 = run(A.SegmentationLoss(1.0, 0.0, weight=w))
    print(f"loss rel {abs(l1.item() - l0.item()) / abs(l0.item()):.2e}, grad rel-to-max {((d1 - d0).abs().max() / d0.abs().max()).item():.2e}")
    assert abs(l1.item() - l0.item()) <= 1e-6 * abs(l0.item())
    assert (d1 - d0).abs().max().item() <= 1e-6 * d0.abs().max().item()


@pytest.mark.parametrize("gamma", [0.5, 2.0])
def test_saturated_pixels_stay_finite_and_inside_the_bound(gamma):
    """A few pixels with a logit margin of +20 on the target (p_t rounds to 1 in fp32) and a few with -20."""
    import pytorch_camvid_amd as A
    C, ld, N, H, W = 12, 16, 2, 24, 30
    x = _logits(N, C, H, W, ld, seed=21).detach()
    t = _targets(N, H, W, C, -100, seed=22).to(dev())
    for k, (n, h, w_) in enumerate(((0, 0, 0), (0, 3, 7), (1, 23, 29), (1, 10, 2), (0, 12, 12), (1, 1, 1))):
        c = k % C
        t[n, h, w_] = c
        x[n, :, h, w_] = torch.randn(C, device=dev()) * 0.1
        x[n, c, h, w_] += 20.0 if k % 2 == 0 else -20.0
    xs = x[0, :, 0, 0]
    assert (torch.softmax(xs, 0)[0] == 1.0).item()                       # p_t rounds to 1 in fp32
    x.requires_grad_(True)
    w = (torch.rand(C, generator=torch.Generator().manual_seed(9)) + 0.2).to(dev())
    for ce, dice in ((1.0, 0.0), (1.0, 0.5)):
        for weight in (None, w):
            lf = A.SegmentationLoss(ce, dice, focal_gamma=gamma, weight=weight)
            _check_against_fp64(lf, x, t, weight, ("saturated", gamma, ce, dice, weight is not None))


def test_out_of_range_targets_all_ignored_and_refusals():
    import pytorch_camvid_amd as A
    C = 12
    x = _logits(2, C, 16, 20, 16, seed=1)
    w = torch.rand(C, device=dev()) + 0.5
    t = _targets(2, 16, 20, C, -100, seed=2).to(dev())
    t[0, 0, :3] = C                                      # three targets past the last class
    t[1, 5, 7] = -1
    for ce, dice in ((1.0, 0.0), (0.0, 1.0), (1.0, 0.5)):
        xg = x.detach().clone().requires_grad_(True)
        l = A.SegmentationLoss(ce, dice, focal_gamma=2.0, weight=w)(xg, t)
        assert torch.isnan(l).item()
        with pytest.raises(IndexError, match="4 pixels"):
            A.last_ce_status()
        l.backward()
        bad = ((t == C) | (t == -1)).unsqueeze(1).expand_as(xg)
        assert (xg.grad[bad] == 0).all()
    # every pixel ignored: the focal term is 0/0 = NaN as the cross-entropy's mean; the Dice term 0 with a zero gradient
    t_ign = torch.full_like(t, -100)
    xg = x.detach().clone().requires_grad_(True)
    for ce, dice in ((1.0, 0.0), (1.0, 0.5)):
        l = A.SegmentationLoss(ce, dice, weight=w)(xg, t_ign)
        assert torch.isnan(l).item()
        assert A.last_ce_status() == (0, 0)
    for average in ("present", "all"):
        lf = A.SegmentationLoss(0.0, 1.0, dice_average=average)
        l = lf(xg, t_ign)
        assert l.item() == 0.0 and lf.last_terms.tolist() == [0.0, 0.0]
        xg.grad = None
        l.backward()
        assert (xg.grad == 0).all()
    # a weight of the wrong size or on another device, CPU logits and other dtypes are refused
    with pytest.raises(RuntimeError, match="all 12 classes"):
        A.SegmentationLoss(weight=torch.ones(11, device=dev()))(x, t_ign)
    with pytest.raises(RuntimeError, match="no implicit copy"):
        A.SegmentationLoss(weight=torch.ones(C))(x, t_ign)
    with pytest.raises(RuntimeError, match="float32 logits and int64 target"):
        A.SegmentationLoss()(x.double(), t_ign)
    with pytest.raises(RuntimeError, match="float32 logits and int64 target"):
        A.SegmentationLoss()(x, t_ign.int())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.SegmentationLoss()(x.cpu(), t_ign.cpu())


@pytest.mark.parametrize("shape,ld", [((4, 12, 48, 64), 16), ((8, 12, 180, 240), 12), ((2, 100, 48, 64), 104)])
def test_runs_are_bitwise_reproducible(shape, ld):
    import pytorch_camvid_amd as A
    N, C, H, W = shape
    x = _logits(N, C, H, W, ld, seed=3).requires_grad_(True)
    t = _targets(N, H, W, C, -100, seed=4).to(dev())
    w = torch.rand(C, device=dev()) + 0.1
    lf = A.SegmentationLoss(1.0, 0.5, focal_gamma=2.0, weight=w)

    def run():
        x.grad = None
        l = lf(x, t)
        l.backward()
        return l.detach().clone(), lf.last_terms.clone(), lf.last_dice.clone(), x.grad.clone()

    a, b = run(), run()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.isfinite(a[0]).item()


def test_evaluate_report_takes_the_loss():
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev())
    g = torch.Generator().manual_seed(2)
    batches = [(torch.randn(2, 3, 48, 64, generator=g).to(dev()), torch.randint(0, 12, (2, 48, 64), generator=g).to(dev()))
               for _ in range(2)]
    lf = A.SegmentationLoss(1.0, 0.5, ignore_index=11)
    rep = A.evaluate_report(net, batches, loss_fn=lf)
    net.eval()
    with torch.no_grad():
        want = sum(lf(net(x), t).item() for x, t in batches) / 2
    assert np.isfinite(rep["loss"]) and abs(rep["loss"] - want) <= 1e-6 * abs(want)


def test_training_tracks_the_reference_graph():
    """20 AdamW steps of the UNet at 2x3x96x128 on the imbalanced blob task with SegmentationLoss(1.0, 0.5, weight=w), against the
    reference graph (oracle/torch_ref.py on ATen/MIOpen) trained with the fp32 restatement of the loss."""
    import pytorch_camvid_amd as A
    from oracle import torch_ref as Rf
    images, masks = _task(4, 2, 96, 128, seed=5)
    w = A.class_weights((m for m in masks), 12)
    steps = 20
    l_a = _train(lambda: A.get_model("unet", 3, 12), A.SegmentationLoss(1.0, 0.5, weight=w), steps, images, masks)
    l_r = _train(lambda: Rf.build("unet", 3, 12), lambda y, t: R.seg_loss(y, t, 1.0, 0.5, weight=w)[0], steps, images, masks)
    print(f"first loss {l_a[0]:.6f} vs {l_r[0]:.6f}; first-5 max diff {np.abs(l_a[:5] - l_r[:5]).max():.2e}; "
          f"last-5 {l_a[-5:].mean():.4f} vs {l_r[-5:].mean():.4f}")
    assert abs(l_a[0] - l_r[0]) <= 2e-5 * abs(l_r[0])       # identical initialisation and first forward
    assert np.abs(l_a[:5] - l_r[:5]).max() < 2e-2           # the first steps track each other
    assert l_a[-5:].mean() < 0.8 * l_a[0] and l_r[-5:].mean() < 0.8 * l_r[0]          # both learn
    assert abs(l_a[-5:].mean() - l_r[-5:].mean()) < 0.05


def _batch(seed):
    gb = torch.Generator().manual_seed(seed)
    return torch.randn(2, 3, 48, 64, generator=gb).to(dev()), torch.randint(0, 12, (2, 48, 64), generator=gb).to(dev())


def _loss_fn():
    import pytorch_camvid_amd as A
    w = (torch.rand(12, generator=torch.Generator().manual_seed(8)) + 0.2).to(dev())
    return A.SegmentationLoss(1.0, 0.5, focal_gamma=2.0, weight=w, ignore_index=11)


def test_graphed_step_is_bitwise_the_eager_step():
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    ref = A.UNet(3, 12).to(dev()).train()
    ref.load_state_dict(net.state_dict())
    lossf, eager = _loss_fn(), _loss_fn()                  # two modules: last_terms / last_dice are views of a module's own last record,
    x0, t0 = _batch(1)                                     # which for the captured one is the record the replays rewrite
    gs = A.GraphedStep(net, lossf, x0, t0)
    net.load_state_dict(ref.state_dict())                  # the capture's warm-up passes advanced the BN statistics
    for it in range(2):
        x, t = _batch(10 + it)
        la = gs.replay(x, t)
        for p in ref.parameters():
            p.grad = None
        lb = eager(ref(x), t)
        lb.backward()
        assert la.item() == lb.item(), it
        assert torch.equal(lossf.last_terms, eager.last_terms) and torch.equal(lossf.last_dice, eager.last_dice), it
        for (k, p), q in zip(net.named_parameters(), ref.parameters()):
            assert torch.equal(p.grad, q.grad), (it, k)


def test_graphed_step_with_the_optimizer_is_bitwise_the_eager_loop():
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    opt = A.FlatAdamW(net, lr=1e-3, weight_decay=1e-2)
    st0 = {k: v.clone() for k, v in net.state_dict().items()}
    lossf = _loss_fn()
    gs = A.GraphedStep(net, lossf, *_batch(1), optimizer=opt)
    net.load_state_dict(st0)                               # the capture's warm-up passes advanced the BatchNorm statistics
    torch.manual_seed(0)
    ref = A.UNet(3, 12).to(dev()).train()
    opt_ref = A.FlatAdamW(ref, lr=1e-3, weight_decay=1e-2)
    ref.load_state_dict(net.state_dict())
    for it in range(2):
        x, t = _batch(10 + it)
        la = gs.replay(x, t)
        opt_ref.zero_grad()
        lb = lossf(ref(x), t)
        lb.backward()
        opt_ref.step()
        assert torch.equal(la, lb), (it, la.item(), lb.item())
        for (k, p), q in zip(net.named_parameters(), ref.parameters()):
            assert torch.equal(p, q), (it, k)
    assert torch.equal(opt._m, opt_ref._m) and torch.equal(opt._v, opt_ref._v)


def test_graphed_window_with_an_accumulator_is_bitwise_the_eager_window():
    import pytorch_camvid_amd as A
    K = 2
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    ref = A.UNet(3, 12).to(dev()).train()
    ref.load_state_dict(net.state_dict())
    lossf, eager = _loss_fn(), _loss_fn()
    acc = A.GradAccumulator(net, steps=K)
    acc_ref = A.GradAccumulator(ref, steps=K)

    def window(seed):
        xs, ts = zip(*[_batch(seed + k) for k in range(K)])
        return torch.stack(xs), torch.stack(ts)

    gs = A.GraphedStep(net, lossf, *window(20), accumulator=acc)
    net.load_state_dict(ref.state_dict())                  # the capture's warm-up passes advanced the BN statistics
    x, t = window(30)
    la = gs.replay(x, t)
    for p in ref.parameters():
        p.grad = None
    losses = []
    for k in range(K):
        l = eager(ref(x[k]), t[k])
        l.backward()
        losses.append(l.detach())
    assert acc_ref.ready and acc.micro_step == 0
    assert torch.equal(la, torch.stack(losses).mean())
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        assert torch.equal(p.grad, q.grad), k


def test_one_step_in_bf16_mode():
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    A.set_conv_precision(net, "bf16")
    x, t = _batch(3)
    y = net(x)
    assert y.dtype == torch.float32                        # the logits stay fp32 in bf16 mode
    lf = _loss_fn()
    loss = lf(y, t)
    loss.backward()
    assert torch.isfinite(loss).item() and torch.isfinite(lf.last_terms).all()
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
