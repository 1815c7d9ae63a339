"""cvk.BoundaryLoss / cvk.boundary_loss on the GPU against the fp64 restatement of tests/edt_ref.py, evaluated on the kernel's own phi
(tests/test_gpu_edt.py checks phi bit by bit).  Bounds: the loss within 1e-5 of (1 / |V|) sum |phi_c| p_c (B itself can cancel to 0),
the gradient within 1e-5 of the restatement's largest gradient.  Then the options, the special inputs, reproducibility and GraphedStep
with the coefficient changed between replays."""
import numpy as np
import pytest
import torch

from tests import edt_ref as R
from tests.boundary_ref import blocky_maps
from tests.test_gpu_ce_options import _logits, dev

pytestmark = pytest.mark.gpu

TOL = 1e-5
# (N, C, H, W), ld: 5180 and 6435 pixels are 6 and 7 work-groups of 1024, the last one partly filled
CASES = [((2, 12, 37, 70), 12), ((2, 12, 37, 70), 16), ((3, 5, 33, 65), 5), ((3, 5, 33, 65), 8)]


def _labels(shape, seed, ign=-100):
    N, C, H, W = shape
    return torch.from_numpy(blocky_maps(seed, N, H, W, K=C, ignore=ign, cell=(5, 6), void=0.1)[1]).to(dev())


def _run(lf, x, t):
    x.grad = None
    loss = lf(x, t)
    loss.backward()
    return loss.detach().clone(), lf.last_record.clone(), x.grad.clone()


def _compare(tag, lf, x, t, **ref_kw):
    loss, rec, grad = _run(lf, x, t)
    phi = lf.last_maps.cpu().numpy() if lf.last_maps is not None else np.zeros(x.shape, dtype=np.float32)
    want = R.loss_and_grad(x.detach().cpu().numpy(), t.cpu().numpy(), phi, ignore=lf.ignore_index, **ref_kw)
    scale = want["mag"] * ref_kw.get("boundary", 1.0) + abs(want["H"]) * ref_kw.get("ce", 0.0)
    e_l = abs(loss.item() - want["loss"]) / scale
    e_b = abs(rec[3].item() - want["B"]) / want["mag"] if want["mag"] > 0 else abs(rec[3].item())
    e_c = np.abs(rec[8:8 + x.shape[1]].cpu().numpy() - want["class_terms"]).max() / want["mag"] if want["mag"] > 0 else 0.0
    gmax = np.abs(want["grad"]).max()
    e_g = np.abs(grad.cpu().numpy() - want["grad"]).max() / gmax
    print(f"{tag}: loss {loss.item():.7f} want {want['loss']:.7f} (sum of magnitudes {want['mag']:.4f}) dev {e_l:.2e}; B dev {e_b:.2e}; "
          f"class terms dev {e_c:.2e}; grad dev rel-to-max {e_g:.2e} (max {gmax:.3e})")
    assert rec[1].item() == want["valid"] and rec[2].item() == 0
    assert e_l <= TOL and e_b <= TOL and e_c <= TOL and e_g <= TOL
    return loss, rec, grad, want


@pytest.mark.parametrize("shape,ld", CASES)
def test_loss_and_gradient_match_fp64(shape, ld):
    import pytorch_camvid_amd as A
    x = _logits(*shape, ld, seed=sum(shape) + ld).requires_grad_(True)
    t = _labels(shape, seed=ld)
    lf = A.BoundaryLoss()
    loss, rec, grad, want = _compare(f"{shape} ld {ld}", lf, x, t)
    assert 0 < want["valid"] < t.numel() and want["mag"] > 1.0
    assert (grad.permute(0, 2, 3, 1)[t == -100] == 0).all()                     # ignored pixels: exactly zero rows
    assert torch.equal(lf.last_terms, rec[3:5]) and rec[4].item() == 0.0 and rec[5].item() == 1.0 and rec[6].item() == 0.0
    assert torch.equal(lf.last_class_terms, rec[8:8 + shape[1]])
    # the functional form runs the same kernels
    assert torch.equal(A.boundary_loss(x.detach(), t), loss)


def test_class_subset_weighted_cross_entropy_and_grad_scale():
    import pytorch_camvid_amd as A
    shape, ld = (2, 12, 37, 70), 16
    x = _logits(*shape, ld, seed=3).requires_grad_(True)
    t = _labels(shape, seed=4)
    sub = [0, 2, 3, 7, 10]
    _, rec, _, _ = _compare("classes subset", A.BoundaryLoss(classes=sub), x, t, classes=sub)
    assert not rec[8:20][[c for c in range(12) if c not in sub]].any() and rec[8:20][sub].any()
    w = (torch.rand(12, generator=torch.Generator().manual_seed(3)) * 2 + 0.1).to(dev())
    both = A.BoundaryLoss(0.3, 0.8, classes=sub, weight=w)
    lb, rec, db, want = _compare("boundary + weighted ce", both, x, t, boundary=0.3, ce=0.8, classes=sub, weight=w.cpu().numpy())
    assert rec[5].item() == pytest.approx(0.3) and rec[6].item() == pytest.approx(0.8)
    assert rec[7].item() == pytest.approx(w[t[t != -100]].sum().item(), rel=1e-5)
    # H is the existing weighted cross-entropy
    lh = A.CrossEntropyLoss(weight=w)(x.detach(), t)
    assert abs(rec[4].item() - lh.item()) <= TOL * lh.item()
    # ce alone: no maps are computed, the loss is ce * H
    only_h = A.BoundaryLoss(0.0, 0.8, weight=w)
    lo, reco, _ = _run(only_h, x, t)
    assert only_h.last_maps is None and reco[3].item() == 0.0 and abs(lo.item() - 0.8 * lh.item()) <= TOL * lh.item()
    # grad_scale multiplies the backward only
    scaled = A.BoundaryLoss(0.3, 0.8, classes=sub, weight=w, grad_scale=128.0)
    ls, _, ds = _run(scaled, x, t)
    assert torch.equal(ls, lb) and torch.equal(ds, db * 128.0)
    with pytest.raises(RuntimeError, match="no implicit copy"):
        A.BoundaryLoss(1.0, 1.0, weight=torch.ones(12))(x, t)
    with pytest.raises(RuntimeError, match="float32 logits and int64 target"):
        A.BoundaryLoss()(x, t.int())
    with pytest.raises(ValueError, match="names class 12"):
        A.BoundaryLoss(classes=[0, 12])(x, t)


def test_every_pixel_ignored_and_out_of_range_targets():
    import pytorch_camvid_amd as A
    shape = (2, 12, 37, 70)
    x = _logits(*shape, 12, seed=7).requires_grad_(True)
    t = _labels(shape, seed=8)
    lf = A.BoundaryLoss()
    loss, rec, grad = _run(lf, x, torch.full_like(t, -100))
    assert loss.item() == 0.0 and (grad == 0).all() and rec[1].item() == 0 and rec[3].item() == 0.0
    assert A.last_ce_status() == (0, 0)
    tb = t.clone()
    tb[1, 5, 7] = 12
    tb[0, 2, 2] = -1
    loss, rec, grad = _run(lf, x, tb)
    assert torch.isnan(loss).item() and rec[2].item() == 2 and (grad[1, :, 5, 7] == 0).all() and (grad[0, :, 2, 2] == 0).all()
    assert rec[1].item() == int(((tb >= 0) & (tb < 12)).sum()) and torch.isfinite(grad).all()
    with pytest.raises(IndexError, match="2 pixels"):
        A.last_ce_status()


def test_the_one_hot_optimum_is_not_positive():
    """With softmax(logits) = the target's one-hot, B is the mean of phi at each pixel's own class: -(distance - 1) <= 0."""
    import pytorch_camvid_amd as A
    shape = (2, 12, 37, 70)
    t = _labels(shape, seed=9)
    onehot = torch.nn.functional.one_hot(t.clamp(min=0), 12).permute(0, 3, 1, 2).float()
    x = (40.0 * onehot).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    lf = A.BoundaryLoss()
    loss, rec, _ = _run(lf, x, t)
    valid = t != -100
    own = lf.last_maps.gather(1, t.clamp(min=0)[:, None])[:, 0][valid].double()
    print(f"one-hot optimum: B {loss.item():.6f}, mean of phi at the own class {own.mean().item():.6f}")
    assert loss.item() <= 0.0 and (own <= 0).all() and abs(loss.item() - own.mean().item()) <= TOL * own.abs().mean().item()
    # and the opposite prediction (all mass on a class that is far away) is worse
    worse = A.boundary_loss(torch.roll(x.detach(), 1, dims=1), t)
    assert worse.item() > 0.0


def test_two_runs_give_the_same_bits():
    import pytorch_camvid_amd as A
    shape = (2, 12, 37, 70)
    x = _logits(*shape, 16, seed=11).requires_grad_(True)
    t = _labels(shape, seed=12)
    w = torch.ones(12, device=dev())
    a = _run(A.BoundaryLoss(0.5, 0.5, weight=w), x, t)
    b = _run(A.BoundaryLoss(0.5, 0.5, weight=w), x, t)
    for u, v in zip(a, b):
        assert torch.equal(u.contiguous().view(torch.int32), v.contiguous().view(torch.int32))


def _batch(seed):
    gb = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 3, 48, 64, generator=gb).to(dev())
    t = torch.from_numpy(blocky_maps(seed, 2, 48, 64, cell=(6, 7), void=0.05)[1]).to(dev())
    return x, t


def _loss_fn(boundary=0.01):
    import pytorch_camvid_amd as A
    w = (torch.rand(12, generator=torch.Generator().manual_seed(8)) * 2 + 0.1).to(dev())
    return A.BoundaryLoss(boundary, 1.0, weight=w, ignore_index=11).to(dev())


def _optimizer(name, net):
    import pytorch_camvid_amd as A
    return A.FlatAdamW(net, lr=1e-3, weight_decay=1e-2) if name == "adamw" else A.FlatSGD(net, lr=1e-2, momentum=0.9)


@pytest.mark.parametrize("optimizer", ["adamw", "sgd"])
def test_graphed_step_follows_the_coefficient_without_a_recapture(optimizer):
    """Two optimizer steps of the eager loop and of GraphedStep(optimizer=) are bitwise equal, with both flat optimizers; `boundary`
    changes between the steps through the property, and the captured graph reads the new value from the device buffer."""
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    opt = _optimizer(optimizer, net)
    st0 = {k: v.clone() for k, v in net.state_dict().items()}
    lossf = _loss_fn()
    gs = A.GraphedStep(net, lossf, *_batch(1), optimizer=opt)
    net.load_state_dict(st0)                               # the capture's warm-up passes advanced the BatchNorm statistics
    torch.manual_seed(0)
    ref = A.UNet(3, 12).to(dev()).train()
    opt_ref = _optimizer(optimizer, ref)
    ref.load_state_dict(net.state_dict())
    eager = _loss_fn()
    used = []
    for it, coef in enumerate((0.01, 0.5)):
        lossf.boundary = coef
        eager.boundary = coef
        x, t = _batch(10 + it)
        la = gs.replay(x, t)
        opt_ref.zero_grad()
        lb = eager(ref(x), t)
        lb.backward()
        opt_ref.step()
        assert torch.equal(la, lb), (it, la.item(), lb.item())
        assert torch.equal(lossf.last_record.view(torch.int32), eager.last_record.view(torch.int32)), it
        used.append(lossf.last_record[5].item())
        for (k, p), q in zip(net.named_parameters(), ref.parameters()):
            assert torch.equal(p, q), (it, k)
    assert used == pytest.approx([0.01, 0.5]) and lossf.last_record[3].item() != 0.0


def test_graphed_accumulation_window_is_bitwise_the_eager_window():
    import pytorch_camvid_amd as A
    torch.manual_seed(3)
    a, b = A.UNet(3, 12).to(dev()).train(), A.UNet(3, 12).to(dev()).train()
    b.load_state_dict(a.state_dict())
    n = 2
    xs, ts = zip(*[_batch(30 + k) for k in range(n)])
    acc_a, acc_b = A.GradAccumulator(a, steps=n), A.GradAccumulator(b, steps=n)
    gs = A.GraphedStep(b, _loss_fn(0.1), torch.stack(xs), torch.stack(ts), accumulator=acc_b)
    la = gs.replay()
    eager, losses = _loss_fn(0.1), []
    for x, t in zip(xs, ts):                               # the same window through the eager accumulator
        l = eager(a(x), t)
        l.backward()
        losses.append(l.detach())
    assert acc_a.ready and torch.equal(la, torch.stack(losses).mean())
    for (k, p), q in zip(b.named_parameters(), a.parameters()):
        assert torch.equal(p.grad, q.grad), k


def test_evaluate_report_and_one_step_in_bf16_mode():
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev())
    batches = [_batch(20), _batch(21)]
    lf = A.BoundaryLoss(ignore_index=11)
    rep = A.evaluate_report(net, batches, loss_fn=lf)
    net.eval()
    with torch.no_grad():
        want = sum(lf(net(x), t).item() for x, t in batches) / 2
    assert np.isfinite(rep["loss"]) and abs(rep["loss"] - want) <= 1e-6 * abs(want)
    net.train()
    A.set_conv_precision(net, "bf16")
    x, t = _batch(3)
    y = net(x)
    assert y.dtype == torch.float32                        # the logits stay fp32 in bf16 mode
    lf = _loss_fn()
    loss = lf(y, t)
    loss.backward()
    assert torch.isfinite(loss).item() and torch.isfinite(lf.last_record[:8]).all()
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
