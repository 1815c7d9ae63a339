"""Multi-scale / flip test-time augmentation on the GPU: cvk_tta_accumulate and cvk_tta_resize_input at the C ABI and
cvk.TestTimeAugmentation end to end, against the fp64 restatement of tests/tta_ref.py; the exact properties (pred is the arg-max of the
stored probabilities, bitwise reproducibility, the one-view TTA is the plain evaluation) and the evaluate / evaluate_report / predict /
swap_ema workflow.

Tolerance on the probabilities: 4x the yardstick, never more than 1e-5 (tta_ref.tolerance).  The yardstick is the largest deviation of
torch's own fp32 CPU composition (interpolate, softmax, flip, ordered sum, * float32(1/K): tta_ref.torch_fp32_merge) from the fp64
restatement on the very inputs of a case; the values below were measured that way and are kept as constants.  The end-to-end tests
measure theirs at run time as well (their logits come from the network) and print both.
Predictions equal the restatement's except where its two largest mean probabilities are within twice that tolerance; such pixels are at
most 0.2 % of a case (tests/test_tta_cpu.py checks the seeds against that cap without a GPU).

Measured on an MI355X, largest |probs - restatement| (tolerance): six views 7.3e-8 (2.5e-6) at 2 x 12 x 17 x 23 with ld 12 and 16, 6.0e-8
(2.8e-7) at C = 5, 7.1e-8 (3.4e-7) at C = 21, 8.6e-8 (5.9e-6) at 2 x 12 x 45 x 60; one view 2.1e-7 / 1.6e-7 / 3.5e-7 (1e-5 / 6.1e-7 / 1e-5);
two views 1.2e-7 / 1.1e-7 / 1.5e-7 (2.6e-6 / 3.7e-7 / 1e-5); the symmetric map 2.1e-7 (8.3e-7); the input resampling at most 3.9e-7 (1e-5)
and exact at the identity size; UNet end to end 2.1e-8 (8.5e-8), SegNet 1.9e-8 (7.2e-8).  No prediction differed from the restatement's."""
import numpy as np
import pytest
import torch

from tests import tta_ref as R

pytestmark = pytest.mark.gpu

# yardsticks: max |torch fp32 CPU composition - fp64 restatement| on each case's own inputs (tta_ref.yardstick)
YARD_SIX = {"c12_17x23": 6.251e-07, "c12_17x23_ld16": 6.251e-07, "c5_16x16": 6.893e-08, "c21_16x16": 8.579e-08, "c12_45x60": 1.484e-06}
YARD_SINGLE = {"c12_17x23": 3.185e-06, "c5_16x16": 1.527e-07, "c12_45x60": 8.892e-06}      # the last view of the six alone (mirrored, down-scaling)
YARD_TWO = {"c12_17x23": 6.463e-07, "c5_16x16": 9.134e-08, "c12_45x60": 2.925e-06}         # views 1 and 2: mirrored up-scaling, identity
YARD_SYMMETRIC = 2.077e-07
# the input side: max |F.interpolate fp32 - restatement| over the three destination sizes of an image size, images drawn as randn
YARD_INPUT = {(17, 23): 3.400e-06, (16, 16): 3.014e-06, (45, 60): 1.625e-05}
# end to end the logits come from the network on the GPU: measured on an MI355X on the tests' own logits (each test prints it again)
YARD_UNET_E2E = 2.113e-08
YARD_SEGNET_E2E = 1.807e-08


def dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _upload_nhwc(x, ld):
    """[N,C,h,w] CPU -> device NHWC rows of pixel stride ld, the padding filled with NaN (the kernel must not read it into a result)."""
    N, C, h, w = x.shape
    buf = torch.full((N, h, w, ld), float("nan"), dtype=torch.float32)
    buf[..., :C] = x.permute(0, 2, 3, 1)
    return buf.to(dev())


def _accumulate(logits, flips, H, W, ld):
    """The views through cvk_tta_accumulate in order -> (probs [N,C,H,W], pred [N,H,W]) on the CPU."""
    import pytorch_camvid_amd as A
    lib = A.load_library()
    N, C = logits[0].shape[:2]
    K = len(logits)
    acc = torch.full((N, H, W, C), float("nan"), device=dev())          # never cleared: the first view must not read it
    pred = torch.full((N, H, W), -7, device=dev(), dtype=torch.int64)
    inv_k = float(np.float32(1.0) / np.float32(K))
    for i, (lg, fl) in enumerate(zip(logits, flips)):
        d = _upload_nhwc(lg, ld)
        rc = lib.cvk_tta_accumulate(d.data_ptr(), ld, lg.shape[2], lg.shape[3], acc.data_ptr(), pred.data_ptr(), N, H, W, C, int(fl),
                                    int(i == 0), int(i == K - 1), inv_k, _stream())
        assert rc == 0, lib.cvk_last_error_string()
        if i < K - 1:
            assert (pred == -7).all()                                   # only the last view writes predictions
    return acc.permute(0, 3, 1, 2).cpu(), pred.cpu(), acc


def _check(case, probs, pred, ref_probs, ref_pred, yard):
    """Prints the figures, then asserts the probability tolerance and the prediction rule."""
    tol = R.tolerance(yard)
    err = float((probs.double() - ref_probs).abs().max())
    ties = R.near_ties(ref_probs, 2 * tol)
    diff = pred != ref_pred
    print(f"{case}: max |probs - fp64| {err:.3e} (yardstick {yard:.3e}, tolerance {tol:.3e}); predictions differing {int(diff.sum())}, "
          f"near ties {int(ties.sum())} of {pred.numel()}")
    assert torch.isfinite(probs).all(), case
    assert err <= tol, (case, err, tol)
    assert not (diff & ~ties).any(), (case, int((diff & ~ties).sum()))
    assert int(ties.sum()) <= 0.002 * pred.numel(), (case, int(ties.sum()))


def _exact_argmax(acc_dev, pred):
    import pytorch_camvid_amd as A
    assert torch.equal(A.argmax_channels(acc_dev.permute(0, 3, 1, 2)).cpu(), pred)


@pytest.mark.parametrize("name", list(R.CASES))
def test_accumulate_six_views_match_fp64(name):
    seed, N, C, (H, W), sources, ld = R.CASES[name]
    logits, flips = R.draw_views(seed, N, C, sources)
    ref_probs, ref_pred = R.merge(logits, flips, H, W)
    probs, pred, acc = _accumulate(logits, flips, H, W, ld)
    _check(name, probs, pred, ref_probs, ref_pred, YARD_SIX[name])
    _exact_argmax(acc, pred)
    probs2, pred2, _ = _accumulate(logits, flips, H, W, ld)
    assert torch.equal(probs, probs2) and torch.equal(pred, pred2)      # no atomics: bitwise reproducible


@pytest.mark.parametrize("name", list(YARD_SINGLE))
def test_accumulate_one_and_two_views(name):
    """first && last is a plain softmax + arg-max pass, first-then-last has no middle view: both take their own code."""
    seed, N, C, (H, W), sources, ld = R.CASES[name]
    logits, flips = R.draw_views(seed, N, C, sources)
    for tag, sel, yard in (("one view", slice(5, 6), YARD_SINGLE[name]), ("two views", slice(1, 3), YARD_TWO[name])):
        lg, fl = logits[sel], flips[sel]
        ref_probs, ref_pred = R.merge(lg, fl, H, W)
        probs, pred, acc = _accumulate(lg, fl, H, W, ld)
        _check(f"{name} {tag}", probs, pred, ref_probs, ref_pred, yard)
        _exact_argmax(acc, pred)
    # one view at the output size: the softmax of the map itself
    ident = [logits[2]]
    probs, pred, _ = _accumulate(ident, [False], H, W, ld)
    ref = R.softmax(ident[0])
    err = float((probs.double() - ref).abs().max())
    yard = R.yardstick(ident, [False], H, W)                            # torch's fp32 softmax alone, on this map
    print(f"{name} identity view: max |probs - softmax| {err:.3e} (yardstick {yard:.3e})")
    assert err <= R.tolerance(yard) and torch.equal(pred, R.argmax_first(ref))


def test_flip_only_of_a_symmetric_map_is_its_softmax():
    g = torch.Generator().manual_seed(4)
    r = 3.0 * torch.randn((2, 12, 17, 23), generator=g)
    sym = torch.maximum(r, r.flip(-1))                                  # mirror-symmetric along W
    probs, pred, _ = _accumulate([sym, sym], [False, True], 17, 23, 12)
    ref = R.softmax(sym)
    err = float((probs.double() - ref).abs().max())
    print(f"symmetric map: max |probs - softmax| {err:.3e} (yardstick {YARD_SYMMETRIC:.3e})")
    assert err <= R.tolerance(YARD_SYMMETRIC)
    assert torch.equal(probs, probs.flip(-1))                           # (p + flip p) / 2 is symmetric bit for bit
    assert not ((pred != R.argmax_first(ref)) & ~R.near_ties(ref, 2 * R.tolerance(YARD_SYMMETRIC))).any()


@pytest.mark.parametrize("size,dsts", [((17, 23), ((12, 16), (17, 23), (23, 31))), ((16, 16), ((8, 8), (16, 16), (33, 29))),
                                       ((45, 60), ((34, 45), (45, 60), (56, 75)))])
def test_resize_input_matches_fp64(size, dsts):
    import pytorch_camvid_amd as A
    lib = A.load_library()
    H, W = size
    N = 2
    g = torch.Generator().manual_seed(5)
    img = torch.randn((N, 3, H, W), generator=g)
    wide = torch.randn((N, 5, H + 2, W + 3), generator=g)
    wide[:, 1:4, 1:H + 1, 2:W + 2] = img
    layouts = {"channels_last": img.to(dev()).contiguous(memory_format=torch.channels_last),
               "sliced": wide.to(dev())[:, 1:4, 1:H + 1, 2:W + 2]}
    assert not layouts["sliced"].is_contiguous() and not layouts["channels_last"].is_contiguous()
    tol = R.tolerance(YARD_INPUT[size])
    for h, w in dsts:
        for flipped in (False, True):
            ref = R.input_view(img, h, w, flipped)
            for tag, src in layouts.items():
                dst = torch.full((N, h, w, 4), float("nan"), device=dev())
                rc = lib.cvk_tta_resize_input(src.data_ptr(), *src.stride(), dst.data_ptr(), N, H, W, h, w, int(flipped), _stream())
                assert rc == 0, lib.cvk_last_error_string()
                out = dst.cpu()
                err = float((out[..., :3].permute(0, 3, 1, 2).double() - ref).abs().max())
                print(f"input {size} -> {(h, w)} {'mirrored ' if flipped else ''}{tag}: max |view - fp64| {err:.3e} (tolerance {tol:.1e})")
                assert err <= tol and (out[..., 3] == 0).all()
                if (h, w) == (H, W):
                    assert torch.equal(out[..., :3].permute(0, 3, 1, 2), img.flip(-1) if flipped else img)     # weights (1, 0): a copy


def _end_to_end(A, net, tta, images, yard_const, tag):
    net.eval()
    H, W = images.shape[2:]
    sizes = tta.view_sizes(H, W)
    with torch.no_grad():
        views = list(tta.views(images))
        logits = [net(v).cpu() for v in views]
    assert [(v.shape[2], v.shape[3]) for v in views] == [(h, w) for h, w, _ in sizes]
    img = images.cpu()
    for v, (h, w, fl) in zip(views, sizes):                             # the inputs themselves are the restatement's views
        assert float((v.cpu().double() - R.input_view(img, h, w, fl)).abs().max()) <= 1e-5
    flips = [fl for _, _, fl in sizes]
    ref_probs, ref_pred = R.merge(logits, flips, H, W)
    yard = R.yardstick(logits, flips, H, W)
    print(f"{tag}: yardstick measured now {yard:.3e}, constant {yard_const:.3e}")
    net.train()
    probs, pred = tta(net, images)
    assert net.training                                                 # the flag comes back
    assert probs.shape == (images.shape[0], logits[0].shape[1], H, W) and probs.dtype == torch.float32
    assert pred.shape == (images.shape[0], H, W) and pred.dtype == torch.int64
    assert probs.permute(0, 2, 3, 1).is_contiguous()                    # a channels_last view of the accumulator
    keep_p, keep_y = probs.clone(), pred.clone()
    _check(tag, probs.cpu(), pred.cpu(), ref_probs, ref_pred, yard_const)
    assert torch.equal(pred, A.argmax_channels(probs))
    probs2, pred2 = tta(net, images)
    assert torch.equal(probs2, keep_p) and torch.equal(pred2, keep_y)
    assert probs2.data_ptr() == probs.data_ptr()                        # one accumulator per output shape


def test_unet_end_to_end_three_scales_and_flip():
    import pytorch_camvid_amd as A
    torch.manual_seed(11)
    net = A.UNet(3, 12).to(dev())
    images = torch.randn((2, 3, 32, 48), generator=torch.Generator().manual_seed(12)).to(dev())
    tta = A.TestTimeAugmentation(scales=(0.5, 1.0, 1.5), flip=True)
    assert tta.view_sizes(32, 48) == [(16, 24, False), (16, 24, True), (32, 48, False), (32, 48, True), (48, 72, False), (48, 72, True)]
    _end_to_end(A, net, tta, images, YARD_UNET_E2E, "unet 2x3x32x48")


def test_segnet_end_to_end_size_divisor_32():
    import pytorch_camvid_amd as A
    torch.manual_seed(13)
    net = A.SegNet(3, 12).to(dev())
    images = torch.randn((2, 3, 64, 96), generator=torch.Generator().manual_seed(14)).to(dev())
    tta = A.TestTimeAugmentation(scales=(0.5, 1.0), size_divisor=32)
    assert tta.view_sizes(64, 96) == [(32, 64, False), (32, 64, True), (64, 96, False), (64, 96, True)]
    _end_to_end(A, net, tta, images, YARD_SEGNET_E2E, "segnet 2x3x64x96")


def _batches(n=2, N=2, H=32, W=48, seed=20):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn((N, 3, H, W), generator=g).to(dev()), torch.randint(0, 12, (N, H, W), generator=g).to(dev())) for _ in range(n)]


def test_one_view_tta_is_the_plain_evaluation():
    import pytorch_camvid_amd as A
    torch.manual_seed(15)
    net = A.UNet(3, 12).to(dev()).eval()
    batches = _batches()
    one = A.TestTimeAugmentation(scales=(1.0,), flip=False)
    assert one.view_sizes(32, 48) == [(32, 48, False)]
    images = batches[0][0]
    assert next(one.views(images)) is images                            # passed through untouched
    with torch.no_grad():
        logits = net(images)
    probs, pred = one(net, images)
    assert torch.equal(pred, A.argmax_channels(logits))
    yard = R.yardstick([logits.cpu()], [False], 32, 48)
    err = float((probs.cpu().double() - R.softmax(logits.cpu())).abs().max())
    print(f"one view: max |probs - softmax| {err:.3e} (yardstick {yard:.3e})")
    assert err <= R.tolerance(yard)
    plain, with_tta = A.evaluate(net, batches), A.evaluate(net, batches, tta=one)
    assert plain[0] == with_tta[0] and plain[2] == with_tta[2]
    assert torch.allclose(plain[1], with_tta[1], rtol=0.0, atol=0.0, equal_nan=True)       # the ignored class has no IoU: NaN on both sides


def test_workflow_evaluate_report_predict_and_swap_ema():
    import pytorch_camvid_amd as A
    torch.manual_seed(16)
    net = A.UNet(3, 12).to(dev())
    opt = A.FlatAdamW(net, lr=1e-3, ema_decay=0.9)
    batches = _batches()
    loss_fn = A.CrossEntropyLoss()
    for images, masks in batches:                                       # two steps, so the average differs from the weights
        net.train()
        for p in net.parameters():
            p.grad = None
        loss_fn(net(images), masks).backward()
        opt.step()
    tta = A.TestTimeAugmentation(scales=(0.5, 1.0), flip=True)
    before = [p.detach().clone() for p in net.parameters()]
    plain = A.evaluate(net, batches, tta=tta)
    with opt.swap_ema():
        inside = [p.detach().clone() for p in net.parameters()]
        ema = A.evaluate(net, batches, tta=tta)
    assert any(not torch.equal(a, b) for a, b in zip(before, inside))
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, net.parameters()))        # the weights are back
    assert net.training
    assert 0.0 <= plain[2] <= 1.0 and 0.0 <= ema[2] <= 1.0 and plain[1].shape == (12,)
    assert A.evaluate(net, batches, tta=tta)[2] == plain[2]
    base = A.evaluate_report(net, batches)
    rep = A.evaluate_report(net, batches, tta=tta)
    assert set(rep) == set(base) and rep["loss"] == base["loss"] and rep["miou"] == plain[2]
    assert A.evaluate_report(net, batches, tta=A.TestTimeAugmentation(scales=(0.5, 1.5)))["loss"] is None
    with pytest.raises(ValueError, match="no batches"):
        A.evaluate(net, [], tta=tta)
    frame = torch.randint(0, 256, (32, 48, 3), generator=torch.Generator().manual_seed(17), dtype=torch.uint8)
    cls = A.predict(net, frame, tta=tta)
    assert cls.shape == (32, 48) and cls.dtype == torch.int64 and cls.is_cuda and int(cls.min()) >= 0 and int(cls.max()) < 12
    big = A.predict(net, frame, out_size=(50, 70), tta=tta)
    assert big.shape == (50, 70) and big.dtype == torch.int64
    assert torch.equal(big[0, 0], cls[0, 0]) and torch.equal(big[-1, -1], cls[-1, -1])


def test_bf16_mode_and_split_operand_networks():
    """Their logits are float32 at the module boundary: the merge takes them as they are."""
    import pytorch_camvid_amd as A
    images = torch.randn((2, 3, 32, 48), generator=torch.Generator().manual_seed(18)).to(dev())
    tta = A.TestTimeAugmentation(scales=(0.5, 1.0), flip=True)
    for tag in ("bf16", "split2", "split3"):
        torch.manual_seed(19)
        net = A.UNet(3, 12).to(dev())
        if tag == "bf16":
            A.set_conv_precision(net, "bf16")
        else:
            A.set_split_operands(net, int(tag[-1]))
        with torch.no_grad():
            logits = [net.eval()(v).cpu() for v in tta.views(images)]
        assert all(lg.dtype == torch.float32 for lg in logits)
        ref_probs, ref_pred = R.merge(logits, [False, True, False, True], 32, 48)
        probs, pred = tta(net, images)
        _check(f"unet {tag}", probs.cpu(), pred.cpu(), ref_probs, ref_pred, R.yardstick(logits, [False, True, False, True], 32, 48))
        assert torch.equal(pred, A.argmax_channels(probs))


def test_validation_on_the_device():
    import pytorch_camvid_amd as A

    class Fewer(torch.nn.Module):                                       # another class count on the second view
        def __init__(self):
            super().__init__()
            self.calls = 0

        def forward(self, x):
            self.calls += 1
            return torch.zeros((x.shape[0], 12 if self.calls == 1 else 11, x.shape[2], x.shape[3]), device=x.device)

    class OtherBatch(torch.nn.Module):
        def forward(self, x):
            return torch.zeros((x.shape[0] + 1, 12, x.shape[2], x.shape[3]), device=x.device)

    class Half(torch.nn.Module):
        def forward(self, x):
            return torch.zeros((x.shape[0], 12, x.shape[2], x.shape[3]), device=x.device, dtype=torch.float16)

    class Wide(torch.nn.Module):
        def forward(self, x):
            return torch.zeros((x.shape[0], 33, x.shape[2], x.shape[3]), device=x.device)

    images = torch.zeros((1, 3, 16, 16), device=dev())
    tta = A.TestTimeAugmentation(scales=(1.0,), flip=True)
    with pytest.raises(ValueError, match="accumulator"):
        tta(Fewer(), images)
    with pytest.raises(ValueError, match="accumulator"):
        tta(OtherBatch(), images)
    with pytest.raises(RuntimeError, match="float32 logits"):
        tta(Half(), images)
    with pytest.raises(ValueError, match="1 to 32 classes"):
        tta(Wide(), images)
    m = Half().train()
    with pytest.raises(RuntimeError):
        tta(m, images)
    assert m.training                                                   # restored after an error as well
