"""nn.CrossEntropyLoss's weight / label_smoothing / reduction options on the HIP kernels (cvk_softmax_ce_fwd_ex / _bwd_ex) and
the class-statistics meter (cvk_class_histogram): loss and dlogits against torch.nn.functional.cross_entropy in fp64 on the
CPU over a grid of class counts, pixel strides, reductions, weights, smoothing and ignore indices; the out-of-range and
all-ignored conventions; bitwise reproducibility; a short weighted + smoothed UNet training run against the reference graph;
and the step replayed from a captured graph."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _logits(N, C, H, W, ld, seed):
    """[N, C, H, W] logits on the GPU whose NHWC rows have pixel stride ld (a channel slice of a channels_last tensor, the layout
    our networks return)."""
    g = torch.Generator().manual_seed(seed)
    big = (3 * torch.randn(N, ld, H, W, generator=g)).to(dev()).contiguous(memory_format=torch.channels_last)
    x = big[:, :C]
    from pytorch_camvid_amd.functional import _as_nhwc
    assert _as_nhwc(x)[1] == ld
    return x


def _targets(N, H, W, C, ignore_index, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, C, (N, H, W), generator=g)
    t[torch.rand(N, H, W, generator=g) < 0.15] = ignore_index
    return t


def _torch_ref(x, t, w, reduction, eps, ignore_index, gout):
    xr = x.detach().cpu().double().requires_grad_(True)
    l = torch.nn.functional.cross_entropy(xr, t.cpu(), weight=None if w is None else w.cpu().double(), ignore_index=ignore_index,
                                          reduction=reduction, label_smoothing=eps)
    l.backward(gout.cpu().double())
    return l.detach(), xr.grad


@pytest.mark.parametrize("ignore_index", [-100, 11])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C,ld", [(5, 5), (5, 8), (12, 16), (33, 36), (100, 100), (100, 104)])
def test_loss_and_grad_match_torch_fp64(C, ld, weighted, ignore_index):
    import pytorch_camvid_amd as A
    N, H, W = 2, 24, 30                                  # 1440 pixels: two workgroups, the second one partly filled
    x = _logits(N, C, H, W, ld, seed=C + ld).requires_grad_(True)
    t = _targets(N, H, W, C, ignore_index, seed=C).to(dev())
    gw = torch.Generator().manual_seed(7 * C)
    w = (torch.rand(C, generator=gw) * 2 + 0.1).to(dev()) if weighted else None
    for reduction in ("mean", "sum", "none"):
        for eps in (0.0, 0.1, 1.0):
            if w is None and reduction == "mean" and eps == 0.0:
                continue                                 # the default loss: its own kernels, tested elsewhere
            gout = torch.rand((N, H, W) if reduction == "none" else (), generator=gw) + 0.5
            x.grad = None
            lf = A.CrossEntropyLoss(ignore_index=ignore_index, weight=w, reduction=reduction, label_smoothing=eps)
            loss = lf(x, t)
            loss.backward(gout.to(dev()))
            lref, dref = _torch_ref(x, t, w, reduction, eps, ignore_index, gout)
            case = (C, ld, weighted, ignore_index, reduction, eps)
            assert loss.shape == lref.shape, case
            got = loss.detach().cpu().double()
            assert (got - lref).abs().max() <= 1e-5 * lref.abs().max(), (case, got, lref)
            if reduction == "none":
                assert (got[t.cpu() == ignore_index] == 0).all(), case
            d = x.grad.cpu().double()
            assert (d - dref).abs().max() <= 1e-5 * dref.abs().max(), (case, (d - dref).abs().max().item(), dref.abs().max().item())
            assert (d[(t.cpu() == ignore_index).unsqueeze(1).expand_as(d)] == 0).all(), case
            assert A.last_ce_status() == (int((t != ignore_index).sum()), 0)
    # the functional form takes the same path
    l1 = A.cross_entropy(x, t, weight=w, ignore_index=ignore_index, reduction="sum", label_smoothing=0.1)
    l2 = A.CrossEntropyLoss(ignore_index=ignore_index, weight=w, reduction="sum", label_smoothing=0.1)(x, t)
    assert torch.equal(l1, l2)


def test_out_of_range_targets_and_all_ignored():
    import pytorch_camvid_amd as A
    C = 12
    x = _logits(2, C, 16, 20, 16, seed=1)
    w = torch.rand(C, device=dev()) + 0.5
    t = _targets(2, 16, 20, C, -100, seed=2).to(dev())
    t[0, 0, :3] = C                                      # three targets past the last class
    t[1, 5, 7] = -1
    for reduction in ("mean", "sum"):
        l = A.CrossEntropyLoss(weight=w, reduction=reduction, label_smoothing=0.1)(x, t)
        assert torch.isnan(l).item()
        with pytest.raises(IndexError, match="4 pixels"):
            A.last_ce_status()
    lmap = A.cross_entropy(x, t, weight=w, reduction="none")
    bad = (t == C) | (t == -1)
    assert torch.isnan(lmap[bad]).all() and torch.isfinite(lmap[~bad]).all()
    with pytest.raises(IndexError):
        A.last_ce_status()
    # every pixel ignored: the mean is 0/0 = NaN as in torch, the sum 0, the gradient 0
    t_ign = torch.full_like(t, -100)
    xg = x.detach().clone().requires_grad_(True)
    l = A.CrossEntropyLoss(weight=w, label_smoothing=0.1)(xg, t_ign)
    assert torch.isnan(l).item()
    assert torch.isnan(torch.nn.functional.cross_entropy(x.detach().cpu(), t_ign.cpu(), weight=w.cpu(), label_smoothing=0.1)).item()
    assert A.last_ce_status() == (0, 0)
    l = A.CrossEntropyLoss(weight=w, reduction="sum", label_smoothing=0.1)(xg, t_ign)
    assert l.item() == 0.0
    l.backward()
    assert (xg.grad == 0).all()
    # a weight of the wrong size or on another device is refused, not copied
    with pytest.raises(RuntimeError, match="all 12 classes"):
        A.CrossEntropyLoss(weight=torch.ones(11, device=dev()))(x, t_ign)
    with pytest.raises(RuntimeError, match="no implicit copy"):
        A.CrossEntropyLoss(weight=torch.ones(C))(x, t_ign)


def test_unit_weight_matches_the_unweighted_loss_and_runs_are_bitwise_reproducible():
    import pytorch_camvid_amd as A
    C = 12
    x = _logits(4, C, 48, 64, 16, seed=3).requires_grad_(True)
    t = _targets(4, 48, 64, C, -100, seed=4).to(dev())

    def run(lf):
        x.grad = None
        l = lf(x, t)
        l.backward()
        return l.detach().clone(), x.grad.clone()

    l0, d0 = run(A.CrossEntropyLoss())
    l1, d1 = run(A.CrossEntropyLoss(weight=torch.ones(C, device=dev())))
    assert abs(l1.item() - l0.item()) <= 1e-6 * abs(l0.item())
    assert (d1 - d0).abs().max().item() <= 1e-6 * d0.abs().max().item()
    w = torch.rand(C, device=dev()) + 0.1
    for reduction in ("mean", "sum"):
        lf = A.CrossEntropyLoss(weight=w, reduction=reduction, label_smoothing=0.1)
        la, da = run(lf)
        lb, db = run(lf)
        assert torch.equal(la, lb) and torch.equal(da, db), reduction


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
def test_class_frequency_meter_matches_bincount(dtype):
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd.functional import weights_from_counts
    C, ignore = 12, 11
    rng = np.random.default_rng(5)
    meter = A.ClassFrequencyMeter(C, ignore_index=ignore, device=dev())
    pix = np.zeros(C, np.int64); img = np.zeros(C, np.int64); bad = 0
    batches = []
    for b in range(3):
        m = rng.integers(0, C, size=(3, 45, 61))
        m[m == 4] = 0                                    # class 4 never occurs
        if b == 1:
            m[0][m[0] == 7] = 3                          # class 7 missing from one image
            m[2, :2] = 200                               # out of range
        batches.append(m)
        meter.update(torch.as_tensor(m).to(dtype).to(dev()))
        for im in m:
            v = im[(im != ignore) & (im < C)]
            cnt = np.bincount(v, minlength=C)
            pix += cnt
            img += np.where(cnt > 0, cnt.sum(), 0)
            bad += int((im >= C).sum())
    got_pix, got_img, got_bad = meter.counts()
    assert (got_pix == pix).all() and (got_img == img).all() and got_bad == bad
    assert got_pix[4] == 0 and got_pix[ignore] == 0 and got_img[7] < got_img[3]
    for method in ("median_frequency", "enet"):
        w = meter.weights(method)
        assert w.device == dev() and w.dtype == torch.float32
        np.testing.assert_allclose(w.cpu().numpy(), weights_from_counts(pix, img, method), rtol=1e-6)
        np.testing.assert_allclose(A.class_weights(batches, C, ignore, method).cpu().numpy(), w.cpu().numpy(), rtol=0)
    meter.reset()
    meter.update(torch.as_tensor(batches[0][0]).to(dtype).to(dev()))    # one [H, W] mask
    p1, _, _ = meter.counts()
    im = batches[0][0]
    assert (p1 == np.bincount(im[im != ignore], minlength=C)).all()


PALETTE = torch.randn(11, 3, generator=torch.Generator().manual_seed(99))


def _task(n_batches, n, h, w, seed):
    """Blobs of 11 classes with very unequal areas (class c drawn with probability ~ 1/(c+1)); colour determines class up to noise."""
    g = torch.Generator().manual_seed(seed)
    p = 1.0 / torch.arange(1, 12, dtype=torch.float64)
    coarse = torch.multinomial(p / p.sum(), n_batches * n * (h // 8) * (w // 8), replacement=True, generator=g)
    coarse = coarse.view(n_batches, n, h // 8, w // 8).float()
    masks = torch.nn.functional.interpolate(coarse, size=(h, w), mode="nearest").long()
    images = PALETTE[masks].permute(0, 1, 4, 2, 3).contiguous() + 0.3 * torch.randn(n_batches, n, 3, h, w, generator=g)
    return images, masks


def _train(make_net, loss_fn, steps, images, masks):
    torch.manual_seed(0)
    net = make_net().to(dev()).train()
    opt = torch.optim.AdamW(net.parameters(), lr=2e-3, weight_decay=0.0)
    losses = []
    for it in range(steps):
        x = images[it % len(images)].to(dev()); t = masks[it % len(masks)].to(dev())
        opt.zero_grad()
        loss = loss_fn(net(x), t)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return np.array(losses)


def test_weighted_smoothed_training_tracks_the_reference_graph():
    """20 AdamW steps of the UNet at 2x3x96x128 with median-frequency class weights and label smoothing 0.1, against the
    reference graph (oracle/torch_ref.py on ATen/MIOpen) trained with nn.CrossEntropyLoss(weight=w, label_smoothing=0.1)."""
    import pytorch_camvid_amd as A
    from oracle import torch_ref as R
    images, masks = _task(4, 2, 96, 128, seed=5)
    w = A.class_weights((m for m in masks), 12)
    assert w[11] == 0 and (w[:11] > 0).all() and w[10] > w[0]           # class 11 never occurs; rare classes weigh more
    steps = 20
    l_a = _train(lambda: A.get_model("unet", 3, 12), A.CrossEntropyLoss(weight=w, label_smoothing=0.1), steps, images, masks)
    l_r = _train(lambda: R.build("unet", 3, 12), torch.nn.CrossEntropyLoss(weight=w, label_smoothing=0.1), steps, images, masks)
    print(f"first loss {l_a[0]:.6f} vs {l_r[0]:.6f}; first-5 max diff {np.abs(l_a[:5] - l_r[:5]).max():.2e}; "
          f"last-5 {l_a[-5:].mean():.4f} vs {l_r[-5:].mean():.4f}")
    assert abs(l_a[0] - l_r[0]) <= 2e-5 * abs(l_r[0])       # identical initialisation and first forward
    assert np.abs(l_a[:5] - l_r[:5]).max() < 2e-2           # the first steps track each other
    assert l_a[-5:].mean() < 0.8 * l_a[0] and l_r[-5:].mean() < 0.8 * l_r[0]          # both learn
    assert abs(l_a[-5:].mean() - l_r[-5:].mean()) < 0.05


def test_graphed_step_with_weighted_smoothed_loss_is_bitwise_the_eager_step():
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    ref = A.UNet(3, 12).to(dev()).train()
    ref.load_state_dict(net.state_dict())
    g = torch.Generator().manual_seed(8)
    w = (torch.rand(12, generator=g) + 0.2).to(dev())
    lossf = A.CrossEntropyLoss(weight=w, label_smoothing=0.1)

    def batch(seed):
        gb = torch.Generator().manual_seed(seed)
        return torch.randn(2, 3, 48, 64, generator=gb).to(dev()), torch.randint(0, 12, (2, 48, 64), generator=gb).to(dev())

    x0, t0 = batch(1)
    gs = A.GraphedStep(net, lossf, x0, t0)
    net.load_state_dict(ref.state_dict())                  # the capture's warm-up passes advanced the BN statistics
    for it in range(2):
        x, t = batch(10 + it)
        la = gs.replay(x, t)
        for p in ref.parameters():
            p.grad = None
        lb = lossf(ref(x), t)
        lb.backward()
        assert la.item() == lb.item(), it
        for (k, p), q in zip(net.named_parameters(), ref.parameters()):
            assert torch.equal(p.grad, q.grad), (it, k)
