"""Sliding-window inference on the GPU: cvk_window_merge at the C ABI against tests/window_ref.merge_fp32, bitwise (the kernel does the
same IEEE fp32 additions in the same order and one correctly rounded division), and cvk.SlidingWindow end to end against the same window
views merged by hand with torch operators on the GPU, bitwise as well; the evaluate / evaluate_report / predict / TestTimeAugmentation /
swap_ema workflow.  Every comparison prints its figures before it asserts."""
import functools

import pytest
import torch

from tests import window_ref as R

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(tag, got, want):
    """Prints the deviation, then asserts bitwise equality of two fp32 tensors."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (tag, got.shape, want.shape)
    diff = int((_bits(got) != _bits(want)).sum())
    err = float((got.double() - want.double()).abs().max())
    print(f"{tag}: {diff} of {got.numel()} values differ in bits, max |difference| {err:.3e}")
    assert diff == 0, (tag, diff, err)


def _draw(seed, N, C, H, W, crop, stride):
    g = torch.Generator().manual_seed(seed)
    return [3.0 * torch.randn((N, C, h, w), generator=g) for _, _, h, w in R.windows(H, W, crop, stride)]


def _upload_nhwc(x, ld, offset=0):
    """[N,C,h,w] CPU -> device NHWC rows of pixel stride ld, the padding filled with NaN (the kernel must not read it into a result);
    `offset` floats into a larger allocation, for a pointer that is not 16-byte aligned."""
    N, C, h, w = x.shape
    buf = torch.full((N, h, w, ld), float("nan"), dtype=torch.float32)
    buf[..., :C] = x.permute(0, 2, 3, 1)
    flat = torch.full((buf.numel() + offset,), float("nan"), dtype=torch.float32)
    flat[offset:] = buf.reshape(-1)
    return flat.to(dev())[offset:]


def _last_window(H, W, crop, stride):
    """int64 [H, W]: the visiting index of the last window that covers each pixel (brute force)."""
    last = torch.full((H, W), -1, dtype=torch.int64)
    for k, (y1, x1, h, w) in enumerate(R.windows(H, W, crop, stride)):
        last[y1:y1 + h, x1:x1 + w] = k
    return last


def _merge(window_logits, H, W, crop, stride, ld, offset=0, with_pred=True):
    """The windows through cvk_window_merge in visiting order -> (out [N,C,H,W] CPU, pred [N,H,W] CPU, out on the device).  out starts
    as NaN and pred as -7: the kernel never reads out before a pixel's first window and writes pred only where a pixel is finished."""
    import pytorch_camvid_amd as A
    lib = A.load_library()
    N, C = window_logits[0].shape[:2]
    out = torch.full((N, H, W, C), float("nan"), device=dev())
    pred = torch.full((N, H, W), -7, device=dev(), dtype=torch.int64)
    wins = R.windows(H, W, crop, stride)
    gx = len({x1 for _, x1, _, _ in wins})
    last = _last_window(H, W, crop, stride)
    for k, lg in enumerate(window_logits):
        d = _upload_nhwc(lg, ld, offset)
        rc = lib.cvk_window_merge(d.data_ptr(), ld, out.data_ptr(), pred.data_ptr() if with_pred else None, N, H, W, C, crop[0], crop[1],
                                  stride[0], stride[1], k // gx, k % gx, _stream())
        assert rc == 0, lib.cvk_last_error_string()
        if with_pred:
            p = pred.cpu()
            done = (last <= k).expand(N, H, W)
            assert (p[~done] == -7).all(), f"window {k}: an unfinished pixel has a prediction"
            assert ((p[done] >= 0) & (p[done] < C)).all(), f"window {k}: a finished pixel has none"
    return out.permute(0, 3, 1, 2).cpu(), pred.cpu(), out


# name: (seed, N, C, (H, W), crop, stride, ld, pointer offset in floats)
CASES = {
    "c12_17x23": (1, 2, 12, (17, 23), (8, 12), (3, 7), 12, 0),                 # counts reach 3 x 2; a workgroup straddles rows and images
    "c12_17x23_ld16": (1, 2, 12, (17, 23), (8, 12), (3, 7), 16, 0),            # NaN padding
    "c12_17x23_unaligned": (1, 2, 12, (17, 23), (8, 12), (3, 7), 12, 1),       # C % 4 == 0 but no 16-byte alignment: the scalar path
    "c12_17x23_n5": (2, 5, 12, (17, 23), (8, 12), (3, 7), 12, 0),              # 480 window pixels: two workgroups, the second partial
    "c5_16x16": (3, 2, 5, (16, 16), (8, 8), (5, 5), 5, 0),                     # scalar paths, ragged last window
    "c21_16x16_ld24": (4, 2, 21, (16, 16), (8, 8), (5, 5), 24, 0),
    "c12_9x10_stride1": (5, 2, 12, (9, 10), (4, 4), (1, 1), 12, 0),            # counts reach 16
}


@pytest.mark.parametrize("name", list(CASES))
def test_merge_matches_fp32_composition_bitwise(name):
    import pytorch_camvid_amd as A
    seed, N, C, (H, W), crop, stride, ld, offset = CASES[name]
    logits = _draw(seed, N, C, H, W, crop, stride)
    ref, ref_pred = R.merge_fp32(logits, H, W, crop, stride)
    out, pred, out_dev = _merge(logits, H, W, crop, stride, ld, offset)
    assert torch.isfinite(out).all() and (pred >= 0).all()                       # nothing left over
    _same_bits(name, out, ref)
    assert torch.equal(pred, ref_pred)
    assert torch.equal(A.argmax_channels(out_dev.permute(0, 3, 1, 2)).cpu(), pred)
    out2, pred2, _ = _merge(logits, H, W, crop, stride, ld, offset)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(pred, pred2)     # no atomics: bitwise reproducible
    out3, pred3, _ = _merge(logits, H, W, crop, stride, ld, offset, with_pred=False)
    assert torch.equal(_bits(out), _bits(out3)) and (pred3 == -7).all()          # pred is optional and then untouched


@pytest.mark.parametrize("H,W,crop,stride", [(16, 24, (8, 12), (8, 12)), (17, 23, (32, 32), (16, 16))])
def test_single_coverage_is_the_input_bitwise(H, W, crop, stride):
    """Stride equal to the crop on an exact tiling, and a crop at least the image (a single window): cnt == 1 everywhere."""
    assert int(R.counts(H, W, crop, stride).max()) == 1
    logits = _draw(6, 2, 12, H, W, crop, stride)
    out, pred, _ = _merge(logits, H, W, crop, stride, 12)
    whole = torch.empty((2, 12, H, W))
    for (y1, x1, h, w), l in zip(R.windows(H, W, crop, stride), logits):
        whole[:, :, y1:y1 + h, x1:x1 + w] = l
    _same_bits(f"{H}x{W} crop {crop}", out, whole)
    assert torch.equal(pred, R.argmax_first(whole))
    if crop[0] >= H and crop[1] >= W:
        assert len(logits) == 1


def test_a_nan_logit_reaches_its_pixel_only_and_wins_the_argmax():
    seed, N, C, (H, W), crop, stride, ld, _ = CASES["c12_17x23"]
    logits = _draw(seed, N, C, H, W, crop, stride)
    wins = R.windows(H, W, crop, stride)
    k, n, c, wy, wx = 4, 1, 7, 4, 2                                              # window 4 = grid (1, 1) at (3, 7); pixel (7, 9) has 3 x 2 windows
    logits[k][n, c, wy, wx] = float("nan")
    y, x = wins[k][0] + wy, wins[k][1] + wx
    assert int(R.counts(H, W, crop, stride)[y, x]) == 6
    ref, ref_pred = R.merge_fp32(logits, H, W, crop, stride)
    out, pred, _ = _merge(logits, H, W, crop, stride, ld)
    where = torch.isnan(out).nonzero().tolist()
    print(f"NaN at {where}, expected {[[n, c, y, x]]}; pred there {int(pred[n, y, x])}")
    assert where == [[n, c, y, x]] and torch.equal(torch.isnan(ref), torch.isnan(out))
    assert int(pred[n, y, x]) == c and torch.equal(pred, ref_pred)
    _same_bits("values beside the NaN", torch.nan_to_num(out, nan=0.0), torch.nan_to_num(ref, nan=0.0))


def test_bad_arguments_return_an_error():
    import pytorch_camvid_amd as A
    lib = A.load_library()
    lg = torch.zeros((1, 8, 12, 12), device=dev())
    out = torch.zeros((1, 17, 23, 12), device=dev())

    def args(**kw):
        return [kw.get("logits", lg.data_ptr()), kw.get("ld", 12), kw.get("out", out.data_ptr()), None, 1, 17, 23, kw.get("C", 12), 8, 12,
                kw.get("sy", 3), 7, kw.get("iy", 0), 0, _stream()]

    for kw, msg in (({"logits": None}, b"null pointer"), ({"out": None}, b"null pointer"), ({"sy": 9}, b"stride"), ({"iy": 4}, b"outside the 4 x 3 grid"),
                    ({"ld": 8}, b"bad arguments"), ({"C": 33, "ld": 33}, b"33 classes")):
        assert lib.cvk_window_merge(*args(**kw)) == -1 and msg in lib.cvk_last_error_string(), kw
    assert lib.cvk_window_merge(*args()) == 0
    torch.cuda.synchronize()


# ---- end to end -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _net(kind):
    """One network per kind for the tests that only run it in eval mode (they leave its weights and flags as they found them)."""
    import pytorch_camvid_amd as A
    torch.manual_seed(21)
    return (A.UNet if kind == "unet" else A.SegNet)(3, 12).to(dev())


def _images(N, H, W, seed):
    return torch.randn((N, 3, H, W), generator=torch.Generator().manual_seed(seed)).to(dev())


def _by_hand(net, images, sw):
    """The same window views through `net`, merged with torch operators on the GPU in visiting order: (logits [N,C,H,W], counts)."""
    N, _, H, W = images.shape
    out = None
    with torch.no_grad():
        for y1, x1, h, w in sw.windows(H, W):
            l = net(images[:, :, y1:y1 + h, x1:x1 + w])
            if out is None:
                out = torch.zeros((N, l.shape[1], H, W), device=images.device)
            out[:, :, y1:y1 + h, x1:x1 + w] += l
    return out / sw.counts(H, W).to(images.device).to(torch.float32)


def _end_to_end(net, sw, images, tag, nwin):
    import pytorch_camvid_amd as A
    N, _, H, W = images.shape
    assert len(sw.windows(H, W)) == nwin
    net.eval()
    want = _by_hand(net, images, sw)
    net.train()
    logits, pred = sw(net, images)
    assert net.training                                                          # the flag comes back
    net.eval()
    assert logits.shape == (N, 12, H, W) and logits.dtype == torch.float32 and logits.permute(0, 2, 3, 1).is_contiguous()
    assert pred.shape == (N, H, W) and pred.dtype == torch.int64
    _same_bits(tag, logits, want)
    assert torch.equal(pred, A.argmax_channels(logits)) and torch.equal(pred.cpu(), R.argmax_first(want.cpu()))
    keep_l, keep_p = logits.clone(), pred.clone()
    only = sw.logits(net, images)
    assert only.data_ptr() == logits.data_ptr() and torch.equal(_bits(only), _bits(keep_l))      # one buffer per output shape
    logits2, pred2 = sw(net, images)
    assert torch.equal(_bits(logits2), _bits(keep_l)) and torch.equal(pred2, keep_p) and pred2.data_ptr() != pred.data_ptr()


def test_unet_end_to_end_four_windows():
    import pytorch_camvid_amd as A
    sw = A.SlidingWindow(crop=(32, 48), stride=(8, 8))
    assert sw.windows(40, 56) == [(0, 0, 32, 48), (0, 8, 32, 48), (8, 0, 32, 48), (8, 8, 32, 48)]
    _end_to_end(_net("unet"), sw, _images(2, 40, 56, 22), "unet 2x3x40x56", 4)


def test_segnet_end_to_end():
    import pytorch_camvid_amd as A
    sw = A.SlidingWindow(crop=(32, 64), stride=(32, 32))
    assert sw.windows(64, 96) == [(0, 0, 32, 64), (0, 32, 32, 64), (32, 0, 32, 64), (32, 32, 32, 64)]
    _end_to_end(_net("segnet"), sw, _images(2, 64, 96, 23), "segnet 2x3x64x96", 4)


def _batches(n=2, N=2, H=40, W=56, seed=24):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn((N, 3, H, W), generator=g).to(dev()), torch.randint(0, 12, (N, H, W), generator=g).to(dev())) for _ in range(n)]


def _same_metrics(a, b):
    return a[0] == b[0] and a[2] == b[2] and torch.allclose(a[1], b[1], rtol=0.0, atol=0.0, equal_nan=True)


def test_crop_at_least_the_image_is_the_plain_forward():
    import pytorch_camvid_amd as A
    net = _net("unet").eval()
    batches = _batches()
    sw = A.SlidingWindow(crop=(64, 64), stride=(32, 32))
    images = batches[0][0]
    assert sw.windows(40, 56) == [(0, 0, 40, 56)]
    with torch.no_grad():
        plain = net(images).clone()
    logits, pred = sw(net, images)
    _same_bits("one window", logits, plain)
    assert torch.equal(pred, A.argmax_channels(plain))
    assert _same_metrics(A.evaluate(net, batches), A.evaluate(net, batches, window=sw))
    a, b = A.evaluate_report(net, batches), A.evaluate_report(net, batches, window=sw)
    assert a["loss"] == b["loss"] and a["miou"] == b["miou"]


def test_workflow_evaluate_report_and_predict():
    import pytorch_camvid_amd as A
    net = _net("unet").eval()
    batches = _batches()
    sw = A.SlidingWindow(crop=(32, 48), stride=(8, 8))
    loss_fn = A.CrossEntropyLoss()
    meter = A.ConfusionMeter(12, 11, dev())
    losses = []
    for images, masks in batches:
        logits, pred = sw(net, images)
        losses.append(loss_fn(logits, masks).detach())
        meter.update(pred, masks)
    want = meter.compute()
    assert _same_metrics(A.evaluate(net, batches, window=sw), want)
    rep = A.evaluate_report(net, batches, window=sw)
    print(f"report loss {rep['loss']!r}, loss_fn of the merged logits {float(losses[0] + losses[1]) / 2!r}")
    assert rep["loss"] == float(losses[0] + losses[1]) / 2 and rep["miou"] == want[2] and rep["accuracy"] == want[0]
    assert set(rep) == set(A.evaluate_report(net, batches))
    with pytest.raises(ValueError, match="no batches"):
        A.evaluate(net, [], window=sw)
    # predict: the frame goes through preprocess_uint8, whose result is a channels_last view of an NHWC-4 buffer; the windows are views of it
    frame = torch.randint(0, 256, (40, 56, 3), generator=torch.Generator().manual_seed(25), dtype=torch.uint8)
    x = A.preprocess_uint8(frame.to(dev()).unsqueeze(0))
    assert x.stride() == (40 * 56 * 4, 1, 56 * 4, 4)
    lg4, pr4 = sw(net, x)
    lg4 = lg4.clone()
    lgc, prc = sw(net, x.contiguous())                                           # the same values as plain NCHW
    _same_bits("NHWC-4 view against NCHW copy", lg4, lgc)
    cls = A.predict(net, frame, window=sw)
    assert cls.shape == (40, 56) and cls.dtype == torch.int64 and torch.equal(cls, pr4[0]) and torch.equal(cls, prc[0])
    big = A.predict(net, frame, out_size=(50, 70), window=sw)
    assert big.shape == (50, 70) and torch.equal(big[0, 0], cls[0, 0]) and torch.equal(big[-1, -1], cls[-1, -1])


def _tta_by_hand(net, tta, images, view_logits):
    """The views of `tta`, their logits from `view_logits(view)`, through cvk_tta_accumulate at the C ABI: (probs NHWC on the device, pred)."""
    import numpy as np
    import pytorch_camvid_amd as A
    lib = A.load_library()
    N, _, H, W = images.shape
    sizes = tta.view_sizes(H, W)
    K = len(sizes)
    inv_k = float(np.float32(1.0) / np.float32(K))
    acc = torch.full((N, H, W, 12), float("nan"), device=dev())
    pred = torch.full((N, H, W), -7, device=dev(), dtype=torch.int64)
    with torch.no_grad():
        for i, (view, (h, w, flipped)) in enumerate(zip(tta.views(images), sizes)):
            lg = view_logits(view).permute(0, 2, 3, 1).contiguous()
            assert lg.shape == (N, h, w, 12)
            rc = lib.cvk_tta_accumulate(lg.data_ptr(), 12, h, w, acc.data_ptr(), pred.data_ptr(), N, H, W, 12, int(flipped), int(i == 0),
                                        int(i == K - 1), inv_k, _stream())
            assert rc == 0, lib.cvk_last_error_string()
    return acc.permute(0, 3, 1, 2), pred


def test_tta_over_sliding_windows_and_tta_alone():
    import pytorch_camvid_amd as A
    net = _net("unet").eval()
    images = _images(2, 40, 56, 26)
    sw = A.SlidingWindow(crop=(32, 48), stride=(16, 24))
    tta = A.TestTimeAugmentation(scales=(1.0, 1.25), flip=True, window=sw)
    assert tta.view_sizes(40, 56) == [(40, 56, False), (40, 56, True), (50, 70, False), (50, 70, True)]
    assert len(sw.windows(40, 56)) == 4 and len(sw.windows(50, 70)) == 6
    want, want_pred = _tta_by_hand(net, tta, images, lambda v: _by_hand(net, v, sw))
    probs, pred = tta(net, images)
    _same_bits("TTA over windows", probs, want)
    assert torch.equal(pred, want_pred)
    # evaluate_report's loss view (scale 1.0, not mirrored) sees the merged logits
    masks = torch.randint(0, 12, (2, 40, 56), generator=torch.Generator().manual_seed(27)).to(dev())
    loss_fn = A.CrossEntropyLoss()
    rep = A.evaluate_report(net, [(images, masks)], loss_fn=loss_fn, tta=tta)
    assert rep["loss"] == float(loss_fn(sw.logits(net, images), masks))
    # without a window nothing changes: the views through the network itself and the unchanged entry point
    alone = A.TestTimeAugmentation(scales=(1.0, 1.25), flip=True)
    assert alone.window is None
    want, want_pred = _tta_by_hand(net, alone, images, lambda v: net(v))
    probs, pred = alone(net, images)
    _same_bits("TTA alone", probs, want)
    assert torch.equal(pred, want_pred)


def test_inside_swap_ema():
    import pytorch_camvid_amd as A
    torch.manual_seed(28)
    net = A.UNet(3, 12).to(dev())
    opt = A.FlatAdamW(net, lr=1e-3, ema_decay=0.9)
    batches = _batches(seed=29)
    loss_fn = A.CrossEntropyLoss()
    for images, masks in batches:                                                # two steps, so the average differs from the weights
        net.train()
        for p in net.parameters():
            p.grad = None
        loss_fn(net(images), masks).backward()
        opt.step()
    sw = A.SlidingWindow(crop=(32, 48), stride=(8, 8))
    images = batches[0][0]
    live = sw(net, images)[0].clone()
    before = [p.detach().clone() for p in net.parameters()]
    with opt.swap_ema():
        inside = sw(net, images)[0].clone()
        want = _by_hand(net.eval(), images, sw)
        net.train()
        ema = A.evaluate(net, batches, window=sw)
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, net.parameters()))        # the weights are back
    assert net.training
    _same_bits("inside swap_ema", inside, want)
    assert not torch.equal(inside, live) and 0.0 <= ema[2] <= 1.0


@pytest.mark.parametrize("mode", ["bf16", "split2"])
def test_bf16_mode_and_split_operand_networks(mode):
    """Their logits are float32 at the module boundary: the merge takes them as they are."""
    import pytorch_camvid_amd as A
    torch.manual_seed(30)
    net = A.UNet(3, 12).to(dev())
    if mode == "bf16":
        A.set_conv_precision(net, "bf16")
    else:
        A.set_split_operands(net, 2)
    sw = A.SlidingWindow(crop=(32, 48), stride=(8, 8))
    logits, pred = sw(net, _images(2, 40, 56, 31))
    assert logits.dtype == torch.float32 and torch.isfinite(logits).all()
    assert torch.equal(pred, A.argmax_channels(logits))


def test_validation_on_the_device():
    import pytorch_camvid_amd as A

    class Fake(torch.nn.Module):
        def __init__(self, second=None, dtype=torch.float32, classes=12):
            super().__init__()
            self.calls, self.second, self.dtype, self.classes = 0, second, dtype, classes

        def forward(self, x):
            self.calls += 1
            N, C, h, w = x.shape[0], self.classes, x.shape[2], x.shape[3]
            if self.calls == 2 and self.second is not None:
                N, C, h, w = self.second(N, C, h, w)
            return torch.zeros((N, C, h, w), device=x.device, dtype=self.dtype)

    images = torch.zeros((1, 3, 16, 16), device=dev())
    sw = A.SlidingWindow(crop=(8, 8), stride=(8, 8))
    for second in (lambda N, C, h, w: (N, 11, h, w), lambda N, C, h, w: (N + 1, C, h, w), lambda N, C, h, w: (N, C, h, w - 1)):
        with pytest.raises(ValueError, match=r"window \(0, 1\) at \(0, 8\)"):
            sw(Fake(second), images)
    with pytest.raises(RuntimeError, match="float32 logits"):
        sw(Fake(dtype=torch.float16), images)
    with pytest.raises(ValueError, match="1 to 32 classes"):
        sw(Fake(classes=33), images)
    m = Fake(dtype=torch.float16).train()
    with pytest.raises(RuntimeError):
        sw(m, images)
    assert m.training                                                            # restored after an error as well
    ok = Fake()
    logits, pred = sw(ok, images)
    assert ok.calls == 4 and (logits == 0).all() and (pred == 0).all()
