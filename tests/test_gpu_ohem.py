"""The OHEM cross-entropy (cvk.OhemCrossEntropyLoss on cvk_ohem_ce_fwd / _bwd) on the GPU against its fp64 restatement on the CPU
(tests/ohem_ref.py): the per-pixel loss map, the loss and dlogits over a grid of class counts, pixel strides, weights, ignore indices
and two sizes, at the raw entry points and through the module; the selection (L, the counts, the set of zero gradient rows) bitwise
against the rule applied to the kernel's own loss map; the out-of-range / all-ignored conventions; bitwise reproducibility; the step
replayed from a captured graph; evaluate_report and one step in bf16 mode.

Bound: 1e-5 of the largest reference magnitude for the loss map, the loss and the gradient, the bound test_gpu_ce_options.py and
test_gpu_seg_loss.py hold these kernels' siblings to.  The loss and the gradient are compared over the kernel's own kept set (the
rule of ohem_ref.select applied to the kernel's fp32 map): whether a pixel within rounding of the boundary is kept is decided in fp32
and checked bitwise, apart from the arithmetic.  Measured on an MI355X over the whole grid: at most 8.5e-8 of
the largest loss on the map, 1.2e-7 on the loss and 8.4e-7 of the largest gradient magnitude."""
import numpy as np
import pytest
import torch

from tests import ohem_ref as R
from tests.test_gpu_ce_options import _logits, _targets, dev

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _weights(C, seed):
    return (torch.rand(C, generator=torch.Generator().manual_seed(seed)) * 2 + 0.1).to(dev())


def _run(lf, x, t, gout=None):
    """Forward + backward of the module: (loss, record, loss map, dlogits), all on the CPU."""
    x.grad = None
    loss = lf(x, t)
    loss.backward(None if gout is None else gout.to(dev()))
    return loss.detach().cpu(), lf.last_record.cpu().numpy().copy(), lf.last_pixel_loss.cpu().numpy().copy(), x.grad.cpu().clone()


def _check_against_fp64(lf, x, t, w, case, gout):
    """The module's map, loss and gradient against fp64 over the kernel's own kept set; prints the figures before it asserts."""
    loss, rec, px, d = _run(lf, x, t, gout)
    tc = t.cpu()
    lref, valid = R.pixel_losses(x.detach().cpu(), tc, lf.ignore_index)
    e_px = (np.abs(px.astype(np.float64) - lref.numpy())[valid.numpy()].max() / lref[valid].abs().max()).item()
    kept, L, V, k = R.select(px, lf.loss_threshold, lf.min_kept)
    xr = x.detach().cpu().double().requires_grad_(True)
    want = R.weighted_mean(xr, tc, torch.from_numpy(kept), None if w is None else w.cpu())
    want.backward(gout.double())
    dref = xr.grad
    e_l = abs(loss.item() - want.item()) / abs(want.item())
    e_g = ((d.double() - dref).abs().max() / dref.abs().max()).item()
    print(f"{case}: V {V} k {k} kept {int(kept.sum())}; map rel-to-max {e_px:.2e}; loss {loss.item():.7f} ref {want.item():.7f} "
          f"rel {e_l:.2e}; grad rel-to-max {e_g:.2e}")
    assert loss.dim() == 0 and np.isfinite(loss.item()) and torch.isfinite(d).all(), case
    assert (px[~valid.numpy()] == -1).all(), case
    assert e_px <= TOL and e_l <= TOL and e_g <= TOL, (case, e_px, e_l, e_g)
    assert rec[0] == loss.item() and rec[1] == V and rec[2] == 0 and rec[4] == kept.sum() and rec[7] == k, (case, rec)
    return e_px, e_l, e_g


def _raw(x, t, w, lam, min_kept, ignore_index, gout, ld_d):
    """The raw entry points on the same tensors: (record, loss map, dlogits [M, ld_d]) on the device."""
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd.functional import _as_nhwc
    lib = A.load_library()
    lg, ld = _as_nhwc(x.detach())
    N, C, H, W = x.shape
    M = N * H * W
    s = torch.cuda.current_stream().cuda_stream
    scratch = torch.full((lib.cvk_ohem_scratch_bytes(M),), 0xA5, dtype=torch.uint8, device=dev())     # the call must not rely on zeros
    rec = torch.empty(lib.cvk_ohem_record_floats(), device=dev())
    px = torch.empty(M, device=dev())
    wp = w.data_ptr() if w is not None else None
    assert lib.cvk_ohem_ce_fwd(lg.data_ptr(), ld, t.data_ptr(), wp, lam, min_kept, scratch.data_ptr(), rec.data_ptr(), px.data_ptr(), M, C,
                               ignore_index, s) == 0
    dl = torch.full((M, ld_d), float("nan"), device=dev())
    g = gout.to(dev())
    assert lib.cvk_ohem_ce_bwd(lg.data_ptr(), ld, t.data_ptr(), wp, rec.data_ptr(), px.data_ptr(), g.data_ptr(), 1.0, dl.data_ptr(), ld_d,
                               M, C, ignore_index, s) == 0
    return rec, px, dl


@pytest.mark.parametrize("ignore_index", [-100, 11])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C,ld", [(5, 5), (5, 8), (12, 12), (12, 16), (33, 36), (100, 104)])
def test_map_loss_and_grad_match_fp64(C, ld, weighted, ignore_index):
    import pytorch_camvid_amd as A
    w = _weights(C, 7 * C) if weighted else None
    gg = torch.Generator().manual_seed(C + ld)
    # 782 pixels: one partly filled workgroup; 4551: five workgroups, the last chunk partial.  The first setting lets the threshold
    # decide (most pixels of 3 * randn logits are harder than p = 0.7), the second the rank (lambda = 3.9 is rarely reached).
    for (N, H, W), thresh, frac in (((2, 17, 23), 0.7, 4), ((3, 37, 41), 0.02, 3)):
        M = N * H * W
        x = _logits(N, C, H, W, ld, seed=C + ld + N).requires_grad_(True)
        t = _targets(N, H, W, C, ignore_index, seed=C + N).to(dev())
        gout = torch.rand((), generator=gg) + 0.5
        lf = A.OhemCrossEntropyLoss(thresh, M // frac, weight=w, ignore_index=ignore_index)
        case = (C, ld, weighted, ignore_index, M)
        _check_against_fp64(lf, x, t, w, case, gout)
        assert A.last_ce_status() == (int((t != ignore_index).sum()), 0)
        loss, grad = lf(x, t).detach(), x.grad.clone()
        # the raw entry points, the gradient asked for at a padded pixel stride: the same bits, zeros in the padding columns
        rec, px, dl = _raw(x, t, w, lf.loss_threshold, lf.min_kept, ignore_index, gout, ld + 3)
        assert torch.equal(rec, lf.last_record) and torch.equal(px.view(N, H, W), lf.last_pixel_loss), case
        assert rec[0].item() == loss.item() and rec[6].item() == lf.loss_threshold, case
        assert (dl[:, C:] == 0).all() and torch.isfinite(dl).all(), case
        assert torch.equal(dl[:, :C].view(N, H, W, C).permute(0, 3, 1, 2), grad), case
        l2 = A.ohem_cross_entropy(x, t, thresh, M // frac, weight=w, ignore_index=ignore_index)
        assert torch.equal(l2.detach(), loss), case


def _assert_selection_exact(lf, x, t, case):
    """L, the counts and the set of zero gradient rows, bitwise against the rule applied to the kernel's own loss map."""
    loss, rec, px, d = _run(lf, x, t)
    kept, L, V, k = R.select(px, lf.loss_threshold, lf.min_kept)
    print(f"{case}: V {V} k {k} kept {int(kept.sum())} L {L!r} lambda {lf.loss_threshold!r}")
    assert rec[5:6].view(np.uint32)[0] == np.array([L], np.float32).view(np.uint32)[0], (case, rec[5], L)
    assert rec[1] == V and rec[4] == kept.sum() and rec[7] == k and rec[6] == np.float32(lf.loss_threshold), (case, rec)
    assert kept.sum() >= min(lf.min_kept, V)
    assert lf.last_kept.item() == kept.sum() and lf.last_threshold.item() == min(L, np.float32(lf.loss_threshold))
    # precondition: a kept row's gradient cannot underflow (its target entry is g w[t] / sum w (p_t - 1), 1 - p_t >= 1 - exp(-1e-4))
    assert px[kept].min() > 1e-4, case
    nonzero = (d != 0).any(dim=1).numpy()
    assert (nonzero == kept).all(), (case, int((nonzero != kept).sum()))
    return px, kept, L, V, k


def test_selection_is_exact():
    import pytorch_camvid_amd as A
    C, ld, (N, H, W) = 12, 16, (3, 37, 41)
    M = N * H * W
    w = _weights(C, 5)
    x = _logits(N, C, H, W, ld, seed=31).requires_grad_(True)
    t = _targets(N, H, W, C, 11, seed=32).to(dev())
    # (a) lambda low: more than min_kept pixels exceed it, the threshold decides
    lf = A.OhemCrossEntropyLoss(0.9, 50, weight=w, ignore_index=11)
    px, kept, L, V, k = _assert_selection_exact(lf, x, t, "a")
    assert (px > lf.loss_threshold).sum() > 50 and kept.sum() == (px > lf.loss_threshold).sum() and L > lf.loss_threshold
    # (b) lambda high: the rank lands in the middle of the distribution and decides
    lf = A.OhemCrossEntropyLoss(1e-4, M // 2, weight=w, ignore_index=11)
    px, kept, L, V, k = _assert_selection_exact(lf, x, t, "b")
    assert k == M // 2 < V and (px > lf.loss_threshold).sum() < k and L < lf.loss_threshold
    # (c) logits from {-2..2}: losses repeat and the boundary is a tie of several pixels, all kept
    # (three classes: 375 distinct (row, target) pairs over some 3900 valid pixels)
    gi = torch.Generator().manual_seed(33)
    xi = torch.randint(-2, 3, (N, 3, H, W), generator=gi).float().to(dev()).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ti = _targets(N, H, W, 3, 11, seed=35).to(dev())
    lf = A.OhemCrossEntropyLoss(1e-4, M // 3, weight=_weights(3, 6), ignore_index=11)
    px, kept, L, V, k = _assert_selection_exact(lf, xi, ti, "c")
    assert (px == L).sum() >= 2 and kept.sum() > k
    # (d) min_kept >= V: everything is kept and the loss is the class-weighted mean cross-entropy
    lf = A.OhemCrossEntropyLoss(1e-4, M + 5, weight=w, ignore_index=11)
    xs = (_logits(N, C, H, W, ld, seed=34) / 3).requires_grad_(True)       # randn: no pixel is so easy that its gradient could underflow
    px, kept, L, V, k = _assert_selection_exact(lf, xs, t, "d")
    assert k == V == kept.sum() == int((t != 11).sum())
    want = A.CrossEntropyLoss(weight=w, ignore_index=11)(xs, t).item()
    got = lf(xs, t).item()
    print(f"d: loss {got:.7f} against CrossEntropyLoss {want:.7f}")
    assert abs(got - want) <= TOL * abs(want)
    # (e) min_kept = 1: only the hardest pixel (and its ties)
    lf = A.OhemCrossEntropyLoss(1e-30, 1, weight=w, ignore_index=11)       # lambda = 69: no loss of these logits reaches it
    px, kept, L, V, k = _assert_selection_exact(lf, x, t, "e")
    assert k == 1 and (px > lf.loss_threshold).sum() == 0 and L == px[px >= 0].max() and kept.sum() == (px == L).sum()


def test_third_radix_digit_decides():
    """(f) 96 pixels share a logit row but for the first logit, which steps by one ulp around 2.0: their losses differ in the last
    bits only, and the rank is chosen inside the cluster."""
    import pytorch_camvid_amd as A
    C, ld, (N, H, W) = 12, 16, (3, 37, 41)
    x = _logits(N, C, H, W, ld, seed=41).detach()
    t = _targets(N, H, W, C, 11, seed=42)
    g = torch.Generator().manual_seed(43)
    pos = torch.randperm(N * H * W, generator=g)[:96]
    n, h, w_ = pos // (H * W), (pos // W) % H, pos % W
    row = torch.randn(C, generator=g)
    first = torch.from_numpy((np.float32(2.0).view(np.int32) + np.arange(-48, 48, dtype=np.int32)).view(np.float32).copy())
    for j in range(96):
        r = row.clone()
        r[0] = first[j]
        x[n[j], :, h[j], w_[j]] = r.to(dev())
        t[n[j], h[j], w_[j]] = 3
    t = t.to(dev())
    x.requires_grad_(True)
    # the loss map does not depend on min_kept: take it once, put the rank on the cluster's median value, run again
    probe = A.OhemCrossEntropyLoss(1e-6, 1, ignore_index=11)
    probe(x, t)
    px0 = probe.last_pixel_loss.cpu().numpy()
    cluster = px0[n.numpy(), h.numpy(), w_.numpy()]
    assert len(np.unique(cluster)) >= 8, np.unique(cluster)
    mid = np.sort(cluster)[48]
    k = int((px0 >= mid).sum())
    lf = A.OhemCrossEntropyLoss(1e-6, k, ignore_index=11)
    px, kept, L, V, k2 = _assert_selection_exact(lf, x, t, "f")
    assert L == mid and k2 == k and 0 < (cluster >= L).sum() < 96
    keys = px[px >= 0].view(np.uint32)
    lkey = np.array([L], np.float32).view(np.uint32)[0]
    bin1 = np.unique(keys[(keys >> 20) == (lkey >> 20)])
    bin2 = np.unique(keys[(keys >> 10) == (lkey >> 10)])
    print(f"f: distinct values in the boundary's level-1 bin {len(bin1)}, level-2 bin {len(bin2)}")
    assert len(bin1) >= 2 and len(bin2) >= 2             # else the case proves nothing about the later digits


def test_conventions():
    import pytorch_camvid_amd as A
    C, ld, (N, H, W) = 12, 16, (2, 16, 20)
    w = _weights(C, 3)
    x = _logits(N, C, H, W, ld, seed=1).requires_grad_(True)
    t = _targets(N, H, W, C, -100, seed=2).to(dev())
    lf = A.OhemCrossEntropyLoss(0.7, 100, weight=w)
    # ignored pixels: -1 in the map, zero gradient rows
    loss, rec, px, d = _run(lf, x, t)
    ign = (t == -100).cpu()
    assert ign.any() and (px[ign.numpy()] == -1).all() and (px[~ign.numpy()] >= 0).all()
    assert (d[ign.unsqueeze(1).expand_as(d)] == 0).all() and np.isfinite(loss.item())
    # one out-of-range target: NaN, counted, reported; its gradient row is zero
    tb = t.clone()
    tb[1, 5, 7] = C
    loss, rec, px, d = _run(lf, x, tb)
    assert torch.isnan(loss).item() and rec[2] == 1 and np.isnan(px[1, 5, 7]) and (d[1, :, 5, 7] == 0).all()
    with pytest.raises(IndexError, match="1 pixels"):
        A.last_ce_status()
    # every pixel ignored: NaN (0/0) and zero gradients
    loss, rec, px, d = _run(lf, x, torch.full_like(t, -100))
    assert torch.isnan(loss).item() and (d == 0).all() and (px == -1).all() and rec[1] == 0 and rec[4] == 0 and rec[7] == 0
    assert A.last_ce_status() == (0, 0)
    # refusals at call time, with CrossEntropyLoss's messages
    with pytest.raises(RuntimeError, match="all 12 classes"):
        A.OhemCrossEntropyLoss(weight=torch.ones(11, device=dev()))(x, t)
    with pytest.raises(RuntimeError, match="no implicit copy"):
        A.OhemCrossEntropyLoss(weight=torch.ones(C))(x, t)
    with pytest.raises(RuntimeError, match="float32 logits and int64 target"):
        A.OhemCrossEntropyLoss()(x.double(), t)
    with pytest.raises(RuntimeError, match="float32 logits and int64 target"):
        A.OhemCrossEntropyLoss()(x, t.int())


@pytest.mark.parametrize("shape,ld", [((4, 12, 48, 64), 16), ((2, 100, 48, 64), 104)])
def test_runs_are_bitwise_reproducible(shape, ld):
    import pytorch_camvid_amd as A
    N, C, H, W = shape
    x = _logits(N, C, H, W, ld, seed=3).requires_grad_(True)
    t = _targets(N, H, W, C, -100, seed=4).to(dev())
    lf = A.OhemCrossEntropyLoss(0.7, N * H * W // 3, weight=_weights(C, 9))
    a, b = _run(lf, x, t), _run(lf, x, t)
    assert torch.equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and torch.equal(a[3], b[3])
    assert np.isfinite(a[0].item())


def _batch(seed):
    gb = torch.Generator().manual_seed(seed)
    return torch.randn(2, 3, 48, 64, generator=gb).to(dev()), torch.randint(0, 12, (2, 48, 64), generator=gb).to(dev())


def _loss_fn():
    import pytorch_camvid_amd as A
    return A.OhemCrossEntropyLoss(0.7, 2000, weight=_weights(12, 8), ignore_index=11)


def test_graphed_step_is_bitwise_the_eager_step():
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    ref = A.UNet(3, 12).to(dev()).train()
    ref.load_state_dict(net.state_dict())
    lossf, eager = _loss_fn(), _loss_fn()                  # the captured module keeps viewing the record the replays rewrite
    x0, t0 = _batch(1)
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
        assert torch.equal(lossf.last_record, eager.last_record), (it, lossf.last_record, eager.last_record)
        assert 2000 <= lossf.last_kept.item() <= 2 * 48 * 64
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
    eager = _loss_fn()
    x, t = _batch(10)
    la = gs.replay(x, t)
    opt_ref.zero_grad()
    lb = eager(ref(x), t)
    lb.backward()
    opt_ref.step()
    assert torch.equal(la, lb), (la.item(), lb.item())
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        assert torch.equal(p, q), k


def test_evaluate_report_takes_the_loss():
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev())
    g = torch.Generator().manual_seed(2)
    batches = [(torch.randn(2, 3, 48, 64, generator=g).to(dev()), torch.randint(0, 12, (2, 48, 64), generator=g).to(dev()))
               for _ in range(2)]
    lf = A.OhemCrossEntropyLoss(0.7, 1000, ignore_index=11)
    rep = A.evaluate_report(net, batches, loss_fn=lf)
    net.eval()
    with torch.no_grad():
        want = sum(lf(net(x), t).item() for x, t in batches) / 2
    assert np.isfinite(rep["loss"]) and abs(rep["loss"] - want) <= 1e-6 * abs(want)


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
    assert torch.isfinite(loss).item() and torch.isfinite(lf.last_record).all()
    for k, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
