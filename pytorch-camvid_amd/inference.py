"""Inference operators of the hot path on HIP tensors: image ingest, the arg-max and the inference drivers.  The losses are in
losses.py, the meters in meters.py, the evaluation loops in functional.py; every name here is importable from functional as before.

  argmax_channels   <- preds.argmax(dim=1) of train.py:191
  preprocess_uint8, DevicePrefetcher
                    <- ToTensor + Normalize of reference transforms.py:485-538 on the device, fed by 1 byte/value uploads from pinned
                       memory one batch ahead (the reference's `images.cuda()`, train.py:126)
  SlidingWindow, TestTimeAugmentation
                    <- sliding-window and multi-scale / flip test-time inference (not in the reference), merged on the device by one
                       launch per window or view
  LocalCRF, crf_refine, crf_coefficients, crf_tile
                    <- local-window mean-field CRF refinement of a prediction under the network's own input as the guide image
                       (ConvCRF's form with a dilation; not in the reference): one stencil launch per iteration
"""
import torch

from . import _lib
from ._lib import check
from .losses import _as_nhwc, _stream


def argmax_channels(logits):
    """preds.argmax(dim=1) (train.py:191): int64 [N,H,W]; first maximum wins."""
    lib = _lib.load()
    N, C, H, W = logits.shape
    lg, ld = _as_nhwc(logits.detach())
    out = torch.empty((N, H, W), device=logits.device, dtype=torch.int64)
    check(lib.cvk_argmax_channels(lg.data_ptr(), ld, out.data_ptr(), N * H * W, C, _stream(logits)), "cvk_argmax_channels")
    return out


# reference conf/settings.py:8-9 (BGR order, as cv2 decodes)
CAMVID_MEAN = (0.42019099703461577, 0.41323568513979647, 0.4010048431259079)
CAMVID_STD = (0.30598050258519743, 0.3089986932156864, 0.3054061869915674)


def preprocess_uint8(images_u8, mean=CAMVID_MEAN, std=CAMVID_STD):
    """Device-side ToTensor + Normalize (reference transforms.py:485-538): uint8 [N,H,W,3] on the GPU -> float32
    logical [N,3,H,W] (a channels_last view of an NHWC-4 buffer).  Replaces the per-sample CPU float conversion and the
    pageable `images.cuda()` copy of 4 bytes/value (train.py:126) by a 1 byte/value upload + one kernel."""
    import ctypes
    lib = _lib.load()
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3 or not images_u8.is_cuda:
        raise ValueError("expected a uint8 HIP tensor of shape [N, H, W, 3]")
    src = images_u8.contiguous()
    N, H, W, _ = src.shape
    dst = torch.empty((N, H, W, 4), device=src.device, dtype=torch.float32)
    m = (ctypes.c_float * 3)(*mean); sd = (ctypes.c_float * 3)(*std)
    check(lib.cvk_preprocess_u8(src.data_ptr(), dst.data_ptr(), N, H, W, m, sd, _stream(src)), "cvk_preprocess_u8")
    return dst[..., :3].permute(0, 3, 1, 2)


def _check_images(who, images):
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.float32:
        raise ValueError("expected float32 images of shape [N, 3, H, W]")
    if not images.is_cuda:
        raise RuntimeError(f"pytorch_camvid_amd.{who} needs HIP tensors (no CPU fallback)")


def _int_pair(name, v):
    ok = isinstance(v, (tuple, list)) and len(v) == 2 and all(isinstance(e, int) and not isinstance(e, bool) and e >= 1 for e in v)
    if not ok:
        raise ValueError(f"{name} must be a pair of positive integers (height, width). Got: {v!r}")
    return int(v[0]), int(v[1])


def _check_logits(who, logits, C=None):
    """What a merge asks of every output of the network.  Returns the class count the merge runs with: `C`, or for the first output
    (`C` None) the logits' own, of which `who` serves 1 to 32."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 4:
        raise ValueError("the network must return logits of shape [N, C, h, w]")
    if logits.dtype != torch.float32 or not logits.is_cuda:
        raise RuntimeError(f"expected float32 logits on a HIP device, got {logits.dtype} on {logits.device}")
    if C is None:
        C = logits.shape[1]
        if not 1 <= C <= 32:
            raise ValueError(f"pytorch_camvid_amd.{who} serves 1 to 32 classes, got C = {C}")
    return C


def _kept_output(cache, N, C, H, W, device):
    """The float32 [N,H,W,C] buffer `cache` keeps per (N, C, H, W, device), made on first request."""
    key = (N, C, H, W, device)
    buf = cache.get(key)
    if buf is None:
        buf = cache[key] = torch.empty((N, H, W, C), device=device, dtype=torch.float32)
    return buf


class SlidingWindow:
    """Sliding-window inference: the network runs on overlapping crops of an image of any size and the windows' logits are averaged
    where they overlap, merged on the device (cvk_window_merge).

      sw = SlidingWindow(crop=(360, 480), stride=(240, 320))
      logits, pred = sw(net, images)

    The grid is the one of mmseg's mode='slide' (include/cvk.h): for images [N,3,H,W] the windows are hw x ww = min(crop, image) per
    side, (max(H - hc, 0) + sy - 1) // sy + 1 rows of them starting at min(i * sy, H - hw) (columns likewise), visited in row-major
    order; the last row and column are pulled back inside the image, never padded.  A window's network input is the view
    images[:, :, y1:y1+hw, x1:x1+ww] (no copy: the network's import reads any strides).  One launch per window adds its logits into
    the full-size map; the launch of the last window that covers a pixel divides by the pixel's window count and takes the arg-max:
    logits = ((l_1 + l_2) + ...) / float32(count) in visiting order, pred = its first-maximum arg-max
    (`torch.equal(pred, argmax_channels(logits))`).  No count matrix, cleared buffer, atomics or host synchronisation, so two runs
    agree bitwise, and where one window covers a pixel the value is that window's logit bit for bit.

    `logits` is float32 [N,C,H,W], a channels_last view of the buffer this object keeps per (N, C, H, W, device): the next call with
    that shape overwrites it (clone it to keep it).  `pred` is a fresh int64 [N,H,W].  The network runs in eval mode under no_grad and
    gets its `training` flag back.  Networks in bf16 mode or with split operands work unchanged (their logits are float32 at the module
    boundary), and so does a call inside `opt.swap_ema()`.  At most 32 classes.  One cached plan of the network, at the window size,
    serves every image size.  A size the network cannot run raises whatever the network raises."""

    def __init__(self, crop=(360, 480), stride=(240, 320)):
        self.crop, self.stride = _int_pair("crop", crop), _int_pair("stride", stride)
        if self.stride[0] > self.crop[0] or self.stride[1] > self.crop[1]:
            raise ValueError(f"stride must not exceed crop (pixels between two windows would be skipped). Got: stride {self.stride}, "
                             f"crop {self.crop}")
        self._out = {}

    def _grid(self, H, W):
        """(hw, ww, [y1 per grid row], [x1 per grid column])."""
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError(f"an image of {H} x {W} has no pixel")
        (hc, wc), (sy, sx) = self.crop, self.stride
        hw, ww = min(hc, H), min(wc, W)
        gy, gx = (H - hw + sy - 1) // sy + 1, (W - ww + sx - 1) // sx + 1
        return hw, ww, [min(i * sy, H - hw) for i in range(gy)], [min(j * sx, W - ww) for j in range(gx)]

    def windows(self, H, W):
        """[(y1, x1, hw, ww), ...] in visiting order (row-major) for an image size (H, W).  Host arithmetic only."""
        hw, ww, ys, xs = self._grid(H, W)
        return [(y1, x1, hw, ww) for y1 in ys for x1 in xs]

    def counts(self, H, W):
        """int64 [H, W]: how many windows cover each pixel.  Host arithmetic only."""
        hw, ww, ys, xs = self._grid(H, W)
        cy, cx = torch.zeros(int(H), dtype=torch.int64), torch.zeros(int(W), dtype=torch.int64)
        for y1 in ys:
            cy[y1:y1 + hw] += 1
        for x1 in xs:
            cx[x1:x1 + ww] += 1
        return cy[:, None] * cx[None, :]

    def _merge(self, net, images, want_pred):
        lib = _lib.load()
        _check_images("SlidingWindow", images)
        N, _, H, W = images.shape
        hw, ww, ys, xs = self._grid(H, W)
        (hc, wc), (sy, sx) = self.crop, self.stride
        out = pred = None
        C = None
        was_training = net.training
        net.eval()
        try:
            with torch.no_grad():
                for iy, y1 in enumerate(ys):
                    for ix, x1 in enumerate(xs):
                        logits = net(images[:, :, y1:y1 + hw, x1:x1 + ww])
                        C = _check_logits("SlidingWindow", logits, C)
                        if out is None:
                            out = _kept_output(self._out, N, C, H, W, logits.device)
                            if want_pred:
                                pred = torch.empty((N, H, W), device=logits.device, dtype=torch.int64)
                        if tuple(logits.shape) != (N, C, hw, ww) or logits.device != out.device:
                            raise ValueError(f"window ({iy}, {ix}) at ({y1}, {x1}): the network returned logits {list(logits.shape)} on "
                                             f"{logits.device}, the merge expects {[N, C, hw, ww]} on {out.device}")
                        lg, ld = _as_nhwc(logits.detach())
                        check(lib.cvk_window_merge(lg.data_ptr(), ld, out.data_ptr(), pred.data_ptr() if want_pred else None, N, H, W, C,
                                                   hc, wc, sy, sx, iy, ix, _stream(logits)), "cvk_window_merge")
        finally:
            net.train(was_training)
        return out.permute(0, 3, 1, 2), pred

    def __call__(self, net, images):
        """(logits float32 [N,C,H,W], pred int64 [N,H,W]) of one batch; see the class."""
        return self._merge(net, images, True)

    def logits(self, net, images):
        """The merged logits alone (float32 [N,C,H,W], the same buffer `sw(net, images)` returns): no arg-max is taken."""
        return self._merge(net, images, False)[0]


def _check_window(window):
    if window is not None and not isinstance(window, SlidingWindow):
        raise ValueError(f"window must be a pytorch_camvid_amd.SlidingWindow or None. Got: {window!r}")


class TestTimeAugmentation:
    """Multi-scale and horizontal-flip test-time inference, merged on the device (cvk_tta_accumulate, cvk_tta_resize_input).

      tta = TestTimeAugmentation(scales=(0.75, 1.0, 1.25), flip=True, size_divisor=1)
      probs, pred = tta(net, images)

    For images [N,3,H,W] the views are, in this order, `for s in scales: unflipped, then mirrored (if flip)`, each at
    h = size_divisor * ceil(floor(H * s + 0.5) / size_divisor) (w likewise), resampled bilinearly (align_corners=False).  Every
    view's logits, of whatever spatial size the network returns, are resampled to H x W, soft-maxed, mirrored back where the view
    was mirrored, and averaged: probs = ((p_1 + p_2) + ... + p_K) * float32(1 / K) in view order, pred = its first-maximum arg-max
    (`torch.equal(pred, argmax_channels(probs))`).  One launch per view does all of that; no resized, soft-maxed or flipped tensor
    is written, nothing synchronises with the host and no atomics are used, so two runs agree bitwise.  Bilinear weights come from
    integer arithmetic (include/cvk.h), so they are correctly rounded at any size.

    `probs` is float32 [N,C,H,W], a channels_last view of the accumulator this object keeps per output shape: the next call with
    that shape overwrites it (clone it to keep it).  `pred` is a fresh int64 [N,H,W].  The network runs in eval mode under no_grad
    and gets its `training` flag back.  Networks in bf16 mode or with split operands work unchanged (their logits are float32 at
    the module boundary), and so does a call inside `opt.swap_ema()`.  At most 32 classes.  Every distinct view size is one more
    cached plan of the network (DESIGN.md states the memory).  A size the network cannot run raises whatever the network raises.

    With `window` (a SlidingWindow) every view's logits are `window.logits(net, view)` instead of `net(view)`: the network runs on
    crops of the view and the merged map, dense logits at the view's size, goes through everything above unchanged (evaluate_report's
    loss view sees the merged logits).  One plan at the crop size then serves every scale."""

    __test__ = False                    # the name starts with "Test": not a pytest class

    def __init__(self, scales=(0.75, 1.0, 1.25), flip=True, size_divisor=1, window=None):
        import math
        try:
            scales = tuple(float(s) for s in scales)
        except (TypeError, ValueError):
            raise ValueError(f"scales must be a non-empty sequence of positive finite numbers. Got: {scales!r}") from None
        if not scales or not all(math.isfinite(s) and s > 0.0 for s in scales):
            raise ValueError(f"scales must be a non-empty sequence of positive finite numbers. Got: {scales!r}")
        if isinstance(size_divisor, bool) or not isinstance(size_divisor, int) or size_divisor < 1:
            raise ValueError(f"size_divisor must be an integer >= 1. Got: {size_divisor!r}")
        _check_window(window)
        self.scales, self.flip, self.size_divisor, self.window = scales, bool(flip), size_divisor, window
        self._acc = {}

    def _plan(self, H, W):
        """[(scale, h, w, flipped)] in view order."""
        import math
        d = self.size_divisor
        out = []
        for s in self.scales:
            h = d * math.ceil(math.floor(H * s + 0.5) / d)
            w = d * math.ceil(math.floor(W * s + 0.5) / d)
            if h < 1 or w < 1:
                raise ValueError(f"scale {s} of a {H} x {W} image leaves no pixel")
            out.append((s, h, w, False))
            if self.flip:
                out.append((s, h, w, True))
        return out

    def view_sizes(self, H, W):
        """[(h, w, flipped), ...] in view order for a label size (H, W).  Host arithmetic only."""
        return [(h, w, f) for _, h, w, f in self._plan(int(H), int(W))]

    def loss_view(self, H, W):
        """Index of the view evaluate_report takes its loss from: scale 1.0, not mirrored, at the label size; None when there is none."""
        for i, (s, h, w, f) in enumerate(self._plan(int(H), int(W))):
            if s == 1.0 and not f and (h, w) == (H, W):
                return i
        return None

    @staticmethod
    def _check_images(images):
        _check_images("TestTimeAugmentation", images)

    def views(self, images):
        """The network inputs, in view order (what `tta(net, images)` feeds the network): the scale-1.0 unmirrored view at the image
        size is `images` itself, every other one a fresh float32 [N,3,h,w] view of an NHWC-4 buffer (as `preprocess_uint8` returns),
        written by one launch."""
        self._check_images(images)
        lib = _lib.load()
        N, _, H, W = images.shape
        src = images.detach()
        for s, h, w, flipped in self._plan(H, W):
            if s == 1.0 and not flipped and (h, w) == (H, W):
                yield images
                continue
            dst = torch.empty((N, h, w, 4), device=images.device, dtype=torch.float32)
            check(lib.cvk_tta_resize_input(src.data_ptr(), *src.stride(), dst.data_ptr(), N, H, W, h, w, int(flipped), _stream(images)),
                  "cvk_tta_resize_input")
            yield dst[..., :3].permute(0, 3, 1, 2)

    def _merge(self, net, images, on_logits=None):
        lib = _lib.load()
        self._check_images(images)
        N, _, H, W = images.shape
        plan = self._plan(H, W)
        K = len(plan)
        import numpy as np
        inv_k = float(np.float32(1.0) / np.float32(K))
        acc = pred = None
        C = None
        was_training = net.training
        net.eval()
        try:
            with torch.no_grad():
                for i, ((s, h, w, flipped), x) in enumerate(zip(plan, self.views(images))):
                    logits = net(x) if self.window is None else self.window.logits(net, x)
                    C = _check_logits("TestTimeAugmentation", logits, C)
                    if acc is None:
                        acc = _kept_output(self._acc, N, C, H, W, logits.device)
                        pred = torch.empty((N, H, W), device=logits.device, dtype=torch.int64)
                    if logits.shape[0] != N or logits.shape[1] != C or logits.device != acc.device:
                        raise ValueError(f"view {i} ({h} x {w}{', mirrored' if flipped else ''}): the network returned logits "
                                         f"{list(logits.shape)} on {logits.device}, the accumulator is {[N, C, H, W]} on {acc.device}")
                    if on_logits is not None:
                        on_logits(i, logits)
                    lg, ld = _as_nhwc(logits.detach())
                    lh, lw = lg.shape[1], lg.shape[2]
                    check(lib.cvk_tta_accumulate(lg.data_ptr(), ld, lh, lw, acc.data_ptr(), pred.data_ptr(), N, H, W, C, int(flipped),
                                                 int(i == 0), int(i == K - 1), inv_k, _stream(logits)), "cvk_tta_accumulate")
        finally:
            net.train(was_training)
        return acc.permute(0, 3, 1, 2), pred

    def __call__(self, net, images):
        """(probs float32 [N,C,H,W], pred int64 [N,H,W]) of one batch; see the class."""
        return self._merge(net, images)


CRF_MAX_RADIUS, CRF_MAX_DILATION = 5, 4          # include/cvk.h: the window of cvk_crf_step


def _crf_numbers(name, v, n, positive_from):
    import math
    try:
        out = tuple(float(e) for e in v)
    except (TypeError, ValueError):
        out = ()
    ok = len(out) == n and all(math.isfinite(e) for e in out) and out[0] >= 0.0 and all(e > 0.0 for e in out[positive_from:])
    if not ok:
        raise ValueError(f"{name} must be {n} finite numbers, a weight >= 0 followed by widths > 0. Got: {v!r}")
    return out


def _crf_window(radius, dilation):
    for name, v, hi in (("radius", radius, CRF_MAX_RADIUS), ("dilation", dilation, CRF_MAX_DILATION)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= hi:
            raise ValueError(f"{name} must be an integer in 1..{hi}. Got: {v!r}")
    return radius, dilation


def crf_coefficients(radius=3, dilation=1, appearance=(4.0, 8.0, 13.0), smoothness=(3.0, 3.0)):
    """(ga, gs, cb, wa, ws): exactly the numbers cvk_crf_step gets.  ga, gs are float32 numpy arrays [2r+1, 2r+1] over the offsets
    (d i, d j) in row-major (i, j): ga = float32(exp(-|o|^2 / (2 theta_alpha^2))), gs the same with theta_gamma; cb =
    float32(-1 / (2 theta_beta^2)); wa, ws the two weights as float32.  Each is evaluated in double and rounded once.  The centre
    entry of a table (offset (0, 0)) is never read."""
    import numpy as np
    r, d = _crf_window(radius, dilation)
    wa, theta_alpha, theta_beta = _crf_numbers("appearance", appearance, 3, 1)
    ws, theta_gamma = _crf_numbers("smoothness", smoothness, 2, 1)
    i = np.arange(-r, r + 1, dtype=np.float64) * d
    o2 = i[:, None] ** 2 + i[None, :] ** 2
    ga = np.exp(-o2 / (2.0 * theta_alpha * theta_alpha)).astype(np.float32)
    gs = np.exp(-o2 / (2.0 * theta_gamma * theta_gamma)).astype(np.float32)
    cb = float(np.float32(-1.0 / (2.0 * theta_beta * theta_beta)))
    if not (np.isfinite(np.float32(wa)) and np.isfinite(np.float32(ws)) and np.isfinite(cb)):
        raise ValueError("appearance / smoothness leave float32's range")
    return ga, gs, cb, float(np.float32(wa)), float(np.float32(ws))


def crf_tile(num_classes, radius=3, dilation=1):
    """(tile height, tile width, staged) of cvk_crf_step for a class count and a window: the pixels one work-group produces and
    whether their neighbourhood is staged in LDS (True) or read from global memory (False).  No GPU needed."""
    import ctypes
    lib = _lib.load()
    th, tw, st = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.cvk_crf_tile(int(num_classes), int(radius), int(dilation), ctypes.byref(th), ctypes.byref(tw), ctypes.byref(st))
    if rc != 0:
        raise ValueError(lib.cvk_last_error_string().decode())
    return th.value, tw.value, bool(st.value)


class LocalCRF:
    """Local-window mean-field CRF refinement of a prediction, on the device (cvk_crf_step; the definition is in include/cvk.h).

      crf = LocalCRF(iterations=5, radius=3, dilation=1, appearance=(4.0, 8.0, 13.0), smoothness=(3.0, 3.0))
      probs, pred = crf.refine(logits, images)     # logits [N,C,H,W], images the network's float input [N,3,H,W]
      probs, pred = crf(net, images)               # eval-mode forward under no_grad, then the refinement

    This is the ConvCRF form (Teichmann & Cipolla) with a dilation for reach: every pixel hears the (2 radius + 1)^2 - 1 pixels at
    offsets (dilation i, dilation j) around it, not the whole image; the fully connected permutohedral CRF is not provided.
    `appearance = (wa, theta_alpha in pixels, theta_beta in grey levels of 0..255)`, `smoothness = (ws, theta_gamma)`; the defaults
    are DeepLab's dense-CRF values with theta_alpha scaled to a 7 x 7 window.  `compat` is None (Potts, mu = -I) or a float32 [C,C]
    device tensor mu.  `mean` / `std` are the normalisation of the network's input, undone on load (I = 255 (std x + mean)), so the
    guide is the network input itself, of any strides: no second image tensor exists.  uint8 frames [N,H,W,3] are taken as they are.

    `inner` decides what `crf(net, images)` refines: None, the network's logits; a SlidingWindow, `inner.logits(net, images)`; a
    TestTimeAugmentation, its mean probabilities (a probability unary enters as log(max(p, FLT_MIN))).

    One launch per iteration, no atomics: two runs agree bitwise.  `probs` is float32 [N,C,H,W], a channels_last view of one of the
    two buffers this object keeps per (N, C, H, W, device): the next call with that shape overwrites it (clone it to keep it).
    `pred` is a fresh int64 [N,H,W], the first-maximum arg-max of `probs` (`torch.equal(pred, argmax_channels(probs))`).  Channels_last
    logits are read in place, other layouts copied once.  At most 32 classes.  A LocalCRF has TestTimeAugmentation's return
    contract: `evaluate`, `evaluate_report` and `predict` take it as `tta=`; "loss" is then `loss_fn` of the unrefined logits (with a
    TestTimeAugmentation inside, of its loss view)."""

    def __init__(self, iterations=5, radius=3, dilation=1, appearance=(4.0, 8.0, 13.0), smoothness=(3.0, 3.0), compat=None,
                 mean=CAMVID_MEAN, std=CAMVID_STD, inner=None):
        import ctypes
        import math
        import numpy as np
        if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 1:
            raise ValueError(f"iterations must be an integer >= 1. Got: {iterations!r}")
        self.iterations = iterations
        self.radius, self.dilation = _crf_window(radius, dilation)
        self.ga, self.gs, self.cb, self.wa, self.ws = crf_coefficients(radius, dilation, appearance, smoothness)
        if compat is not None and (not isinstance(compat, torch.Tensor) or compat.dim() != 2 or compat.shape[0] != compat.shape[1]
                                   or compat.dtype != torch.float32):
            raise ValueError("compat must be None or a float32 tensor of shape [C, C]")
        self.compat = None if compat is None else compat.detach().contiguous()
        try:
            mean, std = tuple(float(e) for e in mean), tuple(float(e) for e in std)
        except (TypeError, ValueError):
            mean = std = ()
        if len(mean) != 3 or len(std) != 3 or not all(math.isfinite(e) for e in mean + std) or not all(e > 0.0 for e in std):
            raise ValueError("mean and std must be three finite numbers each, std > 0")
        if inner is not None and not isinstance(inner, (SlidingWindow, TestTimeAugmentation)):
            raise ValueError(f"inner must be None, a SlidingWindow or a TestTimeAugmentation. Got: {inner!r}")
        self.inner = inner
        self.guide_scale = np.array([255.0 * s for s in std], dtype=np.float32)       # a_k, b_k of include/cvk.h, rounded once
        self.guide_offset = np.array([255.0 * m for m in mean], dtype=np.float32)
        taps = (2 * self.radius + 1) ** 2
        self._ga = (ctypes.c_float * taps)(*self.ga.ravel().tolist())
        self._gs = (ctypes.c_float * taps)(*self.gs.ravel().tolist())
        self._a = (ctypes.c_float * 3)(*self.guide_scale.tolist())
        self._b = (ctypes.c_float * 3)(*self.guide_offset.tolist())
        self._buf = {}

    def refine(self, unary, images, unary_is_prob=False):
        """(probs float32 [N,C,H,W], pred int64 [N,H,W]) of a unary [N,C,H,W] (logits, or probabilities with `unary_is_prob`) under
        the guide `images` (float32 [N,3,H,W] of any strides, or uint8 [N,H,W,3]); see the class."""
        lib = _lib.load()
        if not isinstance(unary, torch.Tensor) or unary.dim() != 4 or unary.dtype != torch.float32:
            raise ValueError("expected a float32 unary of shape [N, C, H, W]")
        if not unary.is_cuda:
            raise RuntimeError("pytorch_camvid_amd.LocalCRF needs HIP tensors (no CPU fallback)")
        N, C, H, W = unary.shape
        if not 1 <= C <= 32:
            raise ValueError(f"pytorch_camvid_amd.LocalCRF serves 1 to 32 classes, got C = {C}")
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.device != unary.device:
            raise ValueError("expected the guide images as a 4-D tensor on the unary's device")
        if images.dtype == torch.uint8:
            if tuple(images.shape) != (N, H, W, 3):
                raise ValueError(f"uint8 guide frames must be {[N, H, W, 3]}, got {list(images.shape)}")
            guide, u8, strides = images.contiguous(), 1, (0, 0, 0, 0)
        elif images.dtype == torch.float32:
            if tuple(images.shape) != (N, 3, H, W):
                raise ValueError(f"the float guide must be {[N, 3, H, W]}, got {list(images.shape)}")
            guide, u8, strides = images.detach(), 0, tuple(images.stride())
        else:
            raise ValueError(f"the guide must be float32 [N,3,H,W] or uint8 [N,H,W,3], got {images.dtype}")
        compat = self.compat
        if compat is not None:
            if tuple(compat.shape) != (C, C):
                raise ValueError(f"compat is {list(compat.shape)}, the unary has {C} classes")
            if compat.device != unary.device:
                raise ValueError(f"compat is on {compat.device}, the unary on {unary.device}")
        key = (N, C, H, W, unary.device)
        bufs = self._buf.get(key)
        if bufs is None:
            bufs = self._buf[key] = (torch.empty((N, H, W, C), device=unary.device, dtype=torch.float32),
                                     torch.empty((N, H, W, C), device=unary.device, dtype=torch.float32))
        lg, ld = _as_nhwc(unary.detach())
        if lg.data_ptr() in (bufs[0].data_ptr(), bufs[1].data_ptr()):
            lg, ld = lg.clone(), C                            # an earlier result of this object as the unary: it would be overwritten
        pred = torch.empty((N, H, W), device=unary.device, dtype=torch.int64)
        T, s = self.iterations, _stream(unary)
        for t in range(T):
            q_out, q_in = bufs[t & 1], bufs[(t + 1) & 1]
            check(lib.cvk_crf_step(lg.data_ptr(), ld, int(bool(unary_is_prob)), q_in.data_ptr(), q_out.data_ptr(),
                                   pred.data_ptr() if t == T - 1 else None, guide.data_ptr(), u8, *strides, self._a, self._b, self._ga,
                                   self._gs, self.cb, self.wa, self.ws, None if compat is None else compat.data_ptr(), N, H, W, C,
                                   self.radius, self.dilation, int(t == 0), int(t == T - 1), s), "cvk_crf_step")
        return bufs[(T - 1) & 1].permute(0, 3, 1, 2), pred

    def loss_view(self, H, W):
        """Index of the logits evaluate_report takes its loss from: the inner TestTimeAugmentation's own rule, else 0 (the unrefined
        logits)."""
        return self.inner.loss_view(H, W) if isinstance(self.inner, TestTimeAugmentation) else 0

    def _merge(self, net, images, on_logits=None):
        _check_images("LocalCRF", images)
        if isinstance(self.inner, TestTimeAugmentation):
            probs, _ = self.inner._merge(net, images, on_logits)
            return self.refine(probs, images, unary_is_prob=True)
        if isinstance(self.inner, SlidingWindow):
            logits = self.inner.logits(net, images)
        else:
            was_training = net.training
            net.eval()
            try:
                with torch.no_grad():
                    logits = net(images)
            finally:
                net.train(was_training)
            if not isinstance(logits, torch.Tensor) or logits.dim() != 4:
                raise ValueError("the network must return logits of shape [N, C, h, w]")
            if logits.dtype != torch.float32 or not logits.is_cuda:
                raise RuntimeError(f"expected float32 logits on a HIP device, got {logits.dtype} on {logits.device}")
        if on_logits is not None:
            on_logits(0, logits)
        with torch.no_grad():
            return self.refine(logits.detach(), images)

    def __call__(self, net, images):
        """(probs float32 [N,C,H,W], pred int64 [N,H,W]) of one batch; see the class."""
        return self._merge(net, images)


def crf_refine(logits, images, iterations=5, radius=3, dilation=1, appearance=(4.0, 8.0, 13.0), smoothness=(3.0, 3.0), compat=None,
               mean=CAMVID_MEAN, std=CAMVID_STD, unary_is_prob=False):
    """`LocalCRF(...).refine(logits, images, unary_is_prob)` in one call: (probs, pred), fresh buffers."""
    return LocalCRF(iterations, radius, dilation, appearance, smoothness, compat, mean, std).refine(logits, images, unary_is_prob)


class DevicePrefetcher:
    """the reference converts every frame to float on the CPU (transforms.py:485-538) and uploads 4 bytes per
    value from pageable memory inside the step (`images.cuda()`, train.py:126-127).  This iterator takes (uint8 frames
    [N,H,W,3] BGR, int64 masks [N,H,W]) batches from any host iterable (numpy arrays or CPU tensors), stages them in
    pinned buffers and uploads 1 byte per value on a side stream one batch ahead of the consumer; normalisation to the
    network's float NHWC layout happens on the device (`preprocess_uint8`).  Yields (images float32 [N,3,H,W] view, masks).
    The yielded tensors are safe to use on the current stream (the side stream's work is awaited before they are handed out).
    With `transforms` (a `transforms.Compose`, e.g. `transforms.train_transforms()`) each batch's augmentation parameters are
    drawn while it is staged, in batch order, and go up with its frames (pinned records, same side stream); the frames then pass
    through `cvk_augment_u8` instead of `preprocess_uint8` (masks uint8 or int64; uint8 ones travel at 1 byte per pixel) and the
    masks come back int64 at the transforms' output size.  `transforms` supplies its own Normalize mean / std.
    A `transforms.CropCompose` (e.g. `transforms.crop_transforms()`) is served the same way: its records (`cvk_crop_record`) are
    drawn while the batch is staged and go up from the pinned slot; `cvk_crop_select` and `cvk_crop_augment_u8` run on the
    consumer's stream and the batch comes back at the crop size."""

    def __init__(self, batches, device="cuda", mean=CAMVID_MEAN, std=CAMVID_STD, transforms=None):
        self.it = iter(batches)
        self.dev = torch.device(device)
        self.mean, self.std = mean, std
        self.transforms = transforms
        self.stream = torch.cuda.Stream(self.dev)
        self._pin = [None, None]        # two pinned staging slots (frames, masks[, records]), reused when shapes repeat
        self._busy = [None, None]       # per slot: event recorded after the H2D copies that READ its pinned buffers
        self._slot = 0
        self._next = None
        self._stage()

    def _pinned(self, slot, which, like):
        cur = self._pin[slot]
        buf = None if cur is None else cur[which]
        if buf is None or buf.shape != like.shape or buf.dtype != like.dtype:
            buf = torch.empty(like.shape, dtype=like.dtype, pin_memory=True)
            if cur is None:
                self._pin[slot] = [None, None, None]
            self._pin[slot][which] = buf
        return buf

    def _stage(self):
        try:
            frames, masks = next(self.it)
        except StopIteration:
            self._next = None
            return
        frames, masks = torch.as_tensor(frames), torch.as_tensor(masks)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError("expected uint8 frames of shape [N, H, W, 3]")
        slot = self._slot
        self._slot ^= 1
        if self._busy[slot] is not None:
            self._busy[slot].synchronize()              # the upload that last read this slot must be done before the host overwrites it
        pf = self._pinned(slot, 0, frames); pf.copy_(frames)
        pm = self._pinned(slot, 1, masks); pm.copy_(masks)
        pr = None
        if self.transforms is not None:
            from .transforms import RECORD, CROP_RECORD, CropCompose
            N = frames.shape[0]
            if isinstance(self.transforms, CropCompose):        # the draws need the source size; everything else is the same
                pr = self._pinned(slot, 2, torch.empty(N * CROP_RECORD.itemsize, dtype=torch.uint8))
                self.transforms.pack([self.transforms.draw(frames.shape[1], frames.shape[2]) for _ in range(N)],
                                     out=pr.numpy().view(CROP_RECORD))
            else:
                pr = self._pinned(slot, 2, torch.empty(N * RECORD.itemsize, dtype=torch.uint8))
                self.transforms.pack([self.transforms.draw() for _ in range(N)], out=pr.numpy().view(RECORD))
        with torch.cuda.stream(self.stream):
            gf = pf.to(self.dev, non_blocking=True)
            gm = pm.to(self.dev, non_blocking=True)
            gr = pr.to(self.dev, non_blocking=True) if pr is not None else None
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._busy[slot] = ev
        self._next = (gf, gm, gr, ev)

    def __iter__(self):
        return self

    def __next__(self):
        if self._next is None:
            raise StopIteration
        gf, gm, gr, ev = self._next
        cur = torch.cuda.current_stream(self.dev)
        cur.wait_event(ev)
        gf.record_stream(cur); gm.record_stream(cur)
        self._stage()                                   # upload of the following batch overlaps the consumer's step
        if self.transforms is not None:
            from .transforms import augment_u8, CropCompose
            gr.record_stream(cur)
            t = self.transforms
            if isinstance(t, CropCompose):
                return t.apply(gf, gm, gr)                      # cvk_crop_select + cvk_crop_augment_u8 on the consumer's stream
            return augment_u8(gf, gm, gr, t.out_hw(gf.shape[1], gf.shape[2]), t.mean, t.std)
        return preprocess_uint8(gf, self.mean, self.std), gm
