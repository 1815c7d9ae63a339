"""Static-plan executor for the conv/BN/ReLU/pool/upsample/concat hot path.

A network's `forward` (reference models/unet.py:94-156, models/segnet.py:82-119) is recorded ONCE per input shape as
a list of ops over NHWC fp32 activation buffers, then replayed: forward launches the libcvk kernels in order on the
current HIP stream, backward replays the list in reverse with explicit gradient buffers.  The whole network is ONE
autograd node (`_PlanFunction`), so PyTorch autograd sees `(input, *parameters) -> logits` and nothing in between:
no per-layer Python autograd overhead, no tensor version counters on the in-place concat writes, and the executor
knows exactly when each parameter gradient is final (the hook data-parallel bucketing uses, see ddp.py).

Buffers are torch tensors (caching allocator); concat is zero-copy: the upsample branch and the encoder stage write
into the two channel halves of one pre-sized buffer through strided views (cvk_view).
"""
import ctypes

import torch

from . import _lib
from ._lib import View, ViewH, check
from .route import W2D, conv_route, pad4, split_fmt
from .route import layer_tile, wgrad2d_pays, wino2d_ok, wino2d_pays, wino4_pays  # noqa: F401  (engine.<predicate> stays importable)

_F32 = torch.float32


_BF16 = torch.bfloat16


class ActBuf:
    """Logical NHWC activation buffer [N,H,W,C] stored with pixel stride ld: fp32 with ld = pad4(C), or (bf16-storage
    plans) bf16 with ld = C rounded up to 8, at least 32 — the K-slice of the bf16 convolution kernels."""
    __slots__ = ("id", "N", "H", "W", "C", "ld", "name", "dtype")

    def __init__(self, id_, N, H, W, C, name="", dtype=_F32):
        self.id, self.N, self.H, self.W, self.C, self.name, self.dtype = id_, N, H, W, C, name, dtype
        self.ld = pad4(C) if dtype == _F32 else max(32, (C + 7) // 8 * 8)

    @property
    def esize(self):
        return 4 if self.dtype == _F32 else 2

    @property
    def M(self):
        return self.N * self.H * self.W

    def full_view(self):
        return BufView(self, 0, self.C, 0, 0, self.H, self.W)

    def __repr__(self):
        return f"ActBuf({self.name}#{self.id} {self.N}x{self.H}x{self.W}x{self.C}/{self.ld})"


class BufView:
    """Channel slice [c0, c0+C) and spatial window [y0,y0+H) x [x0,x0+W) of an ActBuf."""
    __slots__ = ("buf", "c0", "C", "y0", "x0", "H", "W")

    def __init__(self, buf, c0, C, y0, x0, H, W):
        assert 0 <= c0 and c0 + C <= buf.ld and 0 <= y0 and y0 + H <= buf.H and 0 <= x0 and x0 + W <= buf.W
        self.buf, self.c0, self.C, self.y0, self.x0, self.H, self.W = buf, c0, C, y0, x0, H, W

    def cview(self, tensor):
        b = self.buf
        ptr = tensor.data_ptr() + 4 * ((self.y0 * b.W + self.x0) * b.ld + self.c0)
        return View(ptr, b.H * b.W * b.ld, b.W * b.ld, b.ld)

    def hview(self, tensor):
        """cvk_viewh (strides in elements of the buffer's dtype) — the bf16-storage kernels' view type."""
        b = self.buf
        ptr = tensor.data_ptr() + b.esize * ((self.y0 * b.W + self.x0) * b.ld + self.c0)
        return ViewH(ptr, b.H * b.W * b.ld, b.W * b.ld, b.ld)

    @property
    def is_full(self):
        b = self.buf
        return self.c0 == 0 and self.C == b.C and self.y0 == 0 and self.x0 == 0 and self.H == b.H and self.W == b.W


class RunState:
    """Per-forward-call tensors: activations, saved-for-backward, gradient buffers."""

    def __init__(self, params, training, need_grad):
        self.params = params
        self.training = training
        self.need_grad = need_grad
        self.act = {}      # buf.id -> tensor [N,H,W,ld]
        self.saved = {}    # op index -> tuple
        self.routes = None  # op index -> route.ConvRoute of the conv blocks (fp32 plans: Runner.routes)
        self.grad = {}     # buf.id -> grad tensor
        self.gflat = None
        self.stream = None
        self.sync = None   # optional gradient synchroniser (ddp.GradSync)
        self.pooled_by_block = {}   # op index of a conv block -> True when its BN-apply pass also wrote the max pool behind it
        self.colsums = []           # queued column-sum finalisations (Runner.defer_colsum)
        self.wreduces = []          # queued weight-gradient slab reductions of the bf16 path (Runner.defer_wreduce)
        self.pass_token = 0         # derived-weight cache token of this pass (Runner.forward)
        self.bnred = {}             # op index of a conv block -> (partials, count): its BN-backward sums, left by the consumer's data-grad
        self.amax = {}              # buf.id -> amax block (device int32 words): the largest magnitude written into the buffer, left by the passes
                                    # that write it (opt-in fp16 split-operand layers scale by it: Runner.plan_amax)
        self.amax_spare = []        # zeroed amax blocks for the backward pass (|dy| maxima)
        self.scratch = []           # dgamma / dbeta temporaries of blocks with frozen BatchNorm parameters (ConvBnRelu._grad_targets)
        self.fold = None            # the gradient-accumulation fold of this backward pass (accumulate.GradAccumulator), or None


def _empty(n, dev, dtype=_F32):
    return torch.empty(n, device=dev, dtype=dtype)


import os

# Runner switches (Runner.kernel_config); what each one selects is decided per layer in route.py
WINO_DEFAULT = os.environ.get("CVK_WINO", "1") != "0"   # 1-D Winograd F(2,3) for eligible layers (Cin % 64 == 0, > 32 columns)
# F(4,3) instead of F(2,3) for the forward / data-grad GEMMs of the layers where it pays (route.wino4_pays); "always": every eligible layer (tests)
WINO4_DEFAULT = {"0": False, "1": True, "always": "always"}[os.environ.get("CVK_WINO4", "1")]
# 2-D F(4x4,3x3) (csrc/wino2d.hip) for the channel-heavy layers: 2.25 multiplies per output and input channel instead of
# the 4.5 of the 1-D kernels, paid for with three HBM passes over transform-domain planes.  "0": off, "1": where it pays,
# "always": every eligible layer (tests).
WINO2D_DEFAULT = {"0": False, "1": True, "always": "always"}[os.environ.get("CVK_WINO2D", "1")]
# Output tile of the 2-D path: 6 = F(6x6,3x3) (64 GEMMs, 1.78 multiplies per output, planes 1.78x the activation), 4 = F(4x4,3x3)
# (36 GEMMs, 2.25 / 2.25x).  Both are the same kernels of csrc/wino2d.hip; F(6x6) rounds about twice as coarsely (5e-6 relative L2
# at 256 input channels, tests/test_gpu_w6.py).  "auto" (default): 6, except for networks with MaxUnpool2d (SegNet): their five
# pool/unpool pairs are discontinuous in the arg-max, rounding differences flip single arg-maxes and the logits behind them, and
# the full-size SegNet parity test (distance to the reference <= 2x the reference's own distance to its 1e-6-perturbed twin) holds
# with F(4x4) (18 % of the sampled logits move by > 1e-3, the twin: 11 %) but not with F(6x6) (26 %).
W2TILE_DEFAULT = {"auto": None, "4": 4, "6": 6}[os.environ.get("CVK_W2D_TILE", "auto")]
# fused F(4,3) (csrc/wino4f.hip) instead of the per-index F(4,3) kernels + output pass: "0" off, "1" on
WINO4F_DEFAULT = os.environ.get("CVK_WINO4F", "1") != "0"
# transposed F(4,3) weight-grad through transform-domain planes (csrc/wgradp.hip): "0" off, "1" where it pays, "always" (tests)
WGRADP_DEFAULT = {"0": False, "1": True, "always": "always"}[os.environ.get("CVK_WGRADP", "1")]
# Round 6: the fused F(4,3) forward launch also writes the weight-grad's V planes (cvk_conv3x3_wino4f_vplanes, slice-major) — the plane GEMM then
# takes every F(4,3) weight-grad, not only the 64-input-channel ones, and the x -> V pass is gone.  "0" off, "1" on.
VPLANES_DEFAULT = os.environ.get("CVK_VPLANES", "1") != "0"


def w2fn(lib, tile, name):
    """Entry point `name` of the 2-D Winograd family for output tile `tile`: cvk_w2d_<name> (4) or cvk_w6_<name> (6)."""
    return getattr(lib, ("cvk_w6_" if tile == 6 else "cvk_w2d_") + name)


def w2ws(lib, tile, N, H, W, k_ch, cout):
    return (lib.cvk_conv3x3_w6_workspace_bytes if tile == 6 else lib.cvk_conv3x3_w2d_workspace_bytes)(N, H, W, k_ch, cout)


def amax_blocks(lib, n, dev):
    """n zeroed "amax blocks" (csrc/cvk_common.h: the largest magnitude of a tensor in device memory, a few slots one cache line apart): a list of
    int32 views, one fill for all of them."""
    nw = lib.cvk_amax_block_words()
    t = torch.zeros(n * nw, device=dev, dtype=torch.int32)
    return [t[i * nw:(i + 1) * nw] for i in range(n)]


def absmax(R, t, rows, cols, ld, s, what):
    """A new amax block holding the largest magnitude of t[rows][cols] (pitch ld), measured by its own pass."""
    a = amax_blocks(R.lib, 1, t.device)[0]
    _timed(R, "k_absmax", 4.0 * rows * cols, lambda: check(
        R.lib.cvk_absmax_f32(t.data_ptr(), rows, cols, ld, a.data_ptr(), s), "cvk_absmax_f32(%s)" % what), "byte")
    return a


class WinoConv:
    """y[N,H,W,ldy] = conv3x3(x[N,H,W,k_ch], w[cout][3][3][k_ch]) (+bias, +BN statistics partials at sp) through the Winograd family the
    route names: a block's forward pass, or its data-grad (dgrad_of = (forward weights [Cout_f][3][3][Cin_f], Cout_f, Cin_f); `w` then returns
    the rotated / transposed pack).  Transformed filters are cached under key ck as functions of the parameter wsrc (Runner.derived).
    After run: v, v_amax = the input transform kept for the weight-grad (keep); bnred_sums = (partials, count) a fused data-grad left."""

    def __init__(self, R, s, x, w, bias, y, sp, N, H, W, k_ch, cout, ldy, flops, wsrc, ck, what="", dgrad_of=None):
        self.R, self.lib, self.s, self.x, self.w, self.bias, self.y, self.sp = R, R.lib, s, x, w, bias, y, sp
        self.N, self.H, self.W, self.M, self.k_ch, self.cout, self.ldy = N, H, W, N * H * W, k_ch, cout, ldy
        self.flops, self.wsrc, self.ck, self.what, self.dgrad_of = flops, wsrc, ck, what, dgrad_of
        self.wt = dgrad_of[0] if dgrad_of is not None else w        # the filter the F(4,3) / split transforms read (data-grad: they rotate it)
        self.v = self.v_amax = self.bnred_sums = None

    def run(self, fam, tile=0, fmt=0, keep=False, v_pre=None, x_amax=None, bnred=None):
        """v_pre: 2-D input planes already made with this tile (dy transformed once for both gradients); x_amax: the amax block of x (fp16 split
        operands; measured when None); bnred: (y, scale, shift, mean, rstd) pointers of the block whose BatchNorm-backward sums a fused
        data-grad leaves.  Returns (partial count, counts pointer) when the partials carry pixel counts (cvk_bn_finalize_counts), else None."""
        if fam == "w2d":
            return self.w2d(tile, keep, v_pre)
        if fam == "w2d_split":
            return self.w2d_split(tile, fmt, keep, v_pre, x_amax)
        if fam in ("w4f", "w4f_vplanes", "w4h"):
            return self.w4f(fam == "w4f_vplanes", bnred, fam == "w4h", x_amax)
        return self.w4() if fam == "w4" else self.w2()

    def _filter(self, kind, build, job=None):
        """The cached transformed filter `kind`.  job = (family, floats, rows, cols, tile, dgrad): how prebuild_fp32's batched launch rebuilds it,
        recorded only when the transform reads the parameter itself (no packed or channel-padded copy in between)."""
        d = self.dgrad_of
        straight = self.wt.data_ptr() == self.wsrc.data_ptr() and (d is None or (d[1] == self.k_ch and d[2] == self.cout))
        return self.R.derived((self.ck, kind), self.wsrc, build, job if straight else None)

    def _amax_w(self):
        """The largest magnitude of the filter (fp16 split operands), cached with the layer's filters (shared by its forward and data-grad)."""
        wt = self.wt
        return self.R.derived(((self.ck[0], "a"), "amaxw"), self.wsrc, lambda: absmax(self.R, wt, wt.numel() // 4, 4, 4, self.s, "w"))

    def _counts(self, P):
        return self.sp + 4 * 2 * P * self.cout if self.sp is not None else None

    def w2d(self, tile, keep, v_pre):
        """2-D F(4x4,3x3) / F(6x6,3x3) (csrc/wino2d.hip)."""
        R, lib, s, x, d = self.R, self.lib, self.s, self.x, self.dgrad_of
        N, H, W, M, k_ch, cout, ldy = self.N, self.H, self.W, self.M, self.k_ch, self.cout, self.ldy
        NX = 64 if tile == 6 else 36

        dg = d is not None and d[1] == k_ch and d[2] == cout          # data-grad without channel padding: straight from the forward weights
        rows, cols = (d[1], d[2]) if dg else (cout, k_ch)

        def build():
            u, wt = _empty(NX * cout * k_ch, x.device), d[0] if dg else (self.w() if callable(self.w) else self.w)
            kind = "weight_transform_dgrad" if dg else "weight_transform"
            _timed(R, "k_w2d_weight_dgrad" if dg else "k_w2d_weight", 4.0 * (9 + NX) * cout * k_ch, lambda: check(
                w2fn(lib, tile, kind)(wt.data_ptr(), u.data_ptr(), rows, cols, s), "cvk_w2d_" + kind), "byte")
            return u
        U = self._filter("w2d%d" % tile, build, ("w2d", NX * cout * k_ch, rows, cols, tile, int(d is not None)))
        T = w2fn(lib, tile, "tiles")(N, H, W)
        vfl = NX * lib.cvk_w2d_tpad(T) * k_ch + 128          # V planes + 512 bytes of slack
        if keep:        # the weight-grad of this layer reuses V: its own tensor instead of the shared workspace
            self.v = _empty(vfl, x.device)
        Vt = v_pre if v_pre is not None else self.v
        ws = R.workspace(w2ws(lib, tile, N, H, W, k_ch, cout) - (4 * vfl if Vt is not None else 0), x.device)
        V, Mo = (Vt.data_ptr(), ws.data_ptr()) if Vt is not None else (ws.data_ptr(), ws.data_ptr() + 4 * vfl)
        P2 = w2fn(lib, tile, "stat_partials")(N, H, W)
        cnt = self._counts(P2)
        if v_pre is None:
            _timed(R, "k_w2d_input", 4.0 * (M + NX * T) * k_ch, lambda: check(
                w2fn(lib, tile, "input_transform")(x.data_ptr(), V, N, H, W, k_ch, s), "cvk_w2d_input_transform" + self.what), "byte")
        _timed(R, "k_w2d_gemm<128, 32, 2, 2>", self.flops, lambda: check(
            w2fn(lib, tile, "gemm")(V, U.data_ptr(), Mo, T, k_ch, cout, s), "cvk_w2d_gemm" + self.what),
            executed=2.0 * NX * T * k_ch * cout)   # NX GEMMs of T x k_ch x cout really run on the matrix pipe
        _timed(R, "k_w2d_output", 4.0 * (NX * T + M) * cout, lambda: check(
            w2fn(lib, tile, "output")(Mo, self.bias, self.y.data_ptr(), self.sp, cnt, N, H, W, k_ch, cout, ldy, s), "cvk_w2d_output" + self.what), "byte")
        return (P2, cnt) if self.sp is not None else None

    def w2d_split(self, tile, fmt, keep, v_pre, x_amax):
        """OPT-IN (runner.w2d_split = 3 | 2): the 2-D path with its GEMM stage on the 16-bit matrix pipe with split fp32
        operands (csrc/split_fmt.h: three bf16 terms / six cross-products, or two fp16 terms / three cross-products scaled by an exact power of
        two from the source tensors' largest magnitudes) — the transforms write split planes, cvk_w2d_gemm_split multiplies them, the plain
        output pass finishes.  With v_pre, x_amax is the amax block those planes were scaled by."""
        R, lib, s, x, d = self.R, self.lib, self.s, self.x, self.dgrad_of
        N, H, W, M, k_ch, cout, ldy = self.N, self.H, self.W, self.M, self.k_ch, self.cout, self.ldy
        NX = 64 if tile == 6 else 36
        pdt = _BF16 if fmt == 3 else torch.float16
        tag = "split3" if fmt == 3 else "split2h"
        T = w2fn(lib, tile, "tiles")(N, H, W)
        Tp = lib.cvk_split3_rows_pad(T, 256)
        Cp = lib.cvk_split3_rows_pad(cout, 128)
        wt = self.wt
        am_w = self._amax_w() if fmt == 2 else None

        def build():
            u3 = torch.empty(NX * (k_ch // 32) * fmt * Cp * 32, device=x.device, dtype=pdt)
            amp = am_w.data_ptr() if am_w is not None else None
            rows, cols = (d[1], d[2]) if d is not None else (cout, k_ch)
            _timed(R, ("k_w2d_weight_dgrad+" if d is not None else "k_w2d_weight+") + tag, 4.0 * 9 * cout * k_ch + 2.0 * fmt * NX * cout * k_ch,
                   lambda: check(lib.cvk_w2d_weight_transform_split(fmt, tile, wt.data_ptr(), u3.data_ptr(), amp, rows, cols, int(d is not None), s),
                                 "cvk_w2d_weight_transform_split" + ("(dgrad)" if d is not None else "")), "byte")
            return u3
        U3 = self._filter("w2ds%d_%d" % (fmt, tile), build)
        am_x = x_amax
        if v_pre is not None:
            V3 = v_pre
        else:
            V3 = torch.empty(NX * (k_ch // 32) * fmt * Tp * 32, device=x.device, dtype=pdt)
            if fmt == 2 and am_x is None:       # left by the passes that wrote x (Runner.plan_amax), else measured here
                am_x = absmax(R, x, M, k_ch, k_ch, s, "x")
            if keep:            # the planes travel with the word they were scaled by (weight-grad GEMM)
                self.v, self.v_amax = V3, am_x
            _timed(R, "k_w2d_input<%s>" % tag, (4.0 * M + 2.0 * fmt * NX * T) * k_ch, lambda: check(
                lib.cvk_w2d_input_transform_split(fmt, tile, x.data_ptr(), V3.data_ptr(), am_x.data_ptr() if am_x is not None else None,
                                                  N, H, W, k_ch, s), "cvk_w2d_input_transform_split" + self.what), "byte")
        ws = R.workspace(4 * NX * T * cout + 1024, x.device)
        _timed(R, "k_gemm_" + tag, self.flops, lambda: check(
            lib.cvk_w2d_gemm_split(fmt, tile, V3.data_ptr(), U3.data_ptr(), ws.data_ptr(), am_x.data_ptr() if am_x is not None else None,
                                   am_w.data_ptr() if am_w is not None else None, NX, T, Tp, k_ch, cout, Cp, s), "cvk_w2d_gemm_split" + self.what),
            executed=2.0 * (6 if fmt == 3 else 3) * NX * Tp * k_ch * Cp)     # six bf16 / three fp16 MFMA products per fp32 product
        P2 = w2fn(lib, tile, "stat_partials")(N, H, W)
        cnt = self._counts(P2)
        _timed(R, "k_w2d_output", 4.0 * (NX * T + M) * cout, lambda: check(
            lib.cvk_w2d_output_plain(tile, ws.data_ptr(), self.bias, self.y.data_ptr(), self.sp, cnt, N, H, W, cout, ldy, s),
            "cvk_w2d_output_plain" + self.what), "byte")
        return (P2, cnt) if self.sp is not None else None

    def w4f(self, vplanes=False, bnred=None, h2=False, x_amax=None):
        """Fused F(4,3) (csrc/wino4f.hip): all six transform indices in one workgroup, output transform + bias + statistics in registers — no
        product planes, no output pass.  vplanes: the forward launch also leaves V = B^T d behind as six slice-major planes, the input of the
        layer's plane-GEMM weight-grad (csrc/wgradp.hip); bnred: the data-grad also sums the producing block's BatchNorm backward.
        h2: the OPT-IN fp16 split-operand form (runner.w2d_split = 2): two scaled fp16 terms per operand, 18 fp16 MFMAs per K step instead of
        48 fp32 ones; needs the largest magnitudes of x (left by the pass that wrote it, else measured here) and of w."""
        R, lib, s, x, d, wt = self.R, self.lib, self.s, self.x, self.dgrad_of, self.wt
        N, H, W, M, k_ch, cout, ldy, flops = self.N, self.H, self.W, self.M, self.k_ch, self.cout, self.ldy, self.flops
        floats, dg, f = lib.cvk_wino4f_weight_floats(cout, k_ch), int(d is not None), "h" if h2 else "f"
        am_w = self._amax_w() if h2 else None

        def build():
            u = _empty(floats, x.device)
            if h2:
                _timed(R, "k_wino4h_weight", 4.0 * (9 + 18) * cout * k_ch, lambda: check(lib.cvk_wino4h_weight_transform(
                    wt.data_ptr(), u.data_ptr(), am_w.data_ptr(), cout, k_ch, dg, s), "cvk_wino4h_weight_transform"), "byte")
            else:
                _timed(R, "k_wino4f_weight", 4.0 * (9 + 18) * cout * k_ch, lambda: check(lib.cvk_wino4f_weight_transform(
                    wt.data_ptr(), u.data_ptr(), cout, k_ch, dg, s), "cvk_wino4f_weight_transform" + ("(dgrad)" if dg else "")), "byte")
            return u
        U = self._filter("w4" + f, build, None if h2 else ("w4f", floats, cout, k_ch, 0, dg))
        am = ()
        if h2:
            am_x = x_amax if x_amax is not None else absmax(R, x, M, k_ch, k_ch, s, "x")
            am = (am_x.data_ptr(), am_w.data_ptr())
        executed = (1.5 if h2 else 0.5) * flops        # 3 fp16 products per fp32 product / the F(4,3) saving
        Pf = lib.cvk_wino4f_stat_partials(N, H, W)
        cnt = self._counts(Pf)
        if bnred is not None:
            bpart = _empty(2 * Pf * cout, x.device)
            name = "cvk_conv3x3_wino4%s_bnred" % f
            _timed(R, "k_conv3x3_wino4%s<bnred>" % f, flops, lambda: check(getattr(lib, name)(
                x.data_ptr(), U.data_ptr(), self.y.data_ptr(), *am, N, H, W, k_ch, cout, ldy, *bnred, bpart.data_ptr(), R.launch_wgs(), s), name),
                executed=executed)
            self.bnred_sums = (bpart, Pf)
            return None
        if vplanes:
            self.v = _empty(6 * lib.cvk_wgradp_plane_rows(N, H, W) * k_ch, x.device)
            check(lib.cvk_wgradp_zero_pads_sm(self.v.data_ptr(), N, H, W, k_ch, s), "cvk_wgradp_zero_pads_sm")
            _timed(R, "k_conv3x3_wino4f<vplanes>", flops, lambda: check(
                lib.cvk_conv3x3_wino4f_vplanes(x.data_ptr(), U.data_ptr(), self.bias, self.y.data_ptr(), self.sp, cnt, self.v.data_ptr(), N, H, W,
                                               k_ch, cout, ldy, R.launch_wgs(), s), "cvk_conv3x3_wino4f_vplanes" + self.what), executed=executed)
        else:
            name = "cvk_conv3x3_wino4" + f
            _timed(R, "k_conv3x3_wino4" + f, flops, lambda: check(getattr(lib, name)(
                x.data_ptr(), U.data_ptr(), self.bias, self.y.data_ptr(), self.sp, cnt, *am, N, H, W, k_ch, cout, ldy, R.launch_wgs(), s),
                name + self.what), executed=executed)
        return (Pf, cnt) if self.sp is not None else None

    def w4(self):
        """Per-index F(4,3) GEMMs (csrc/wino4.hip) + output pass."""
        R, lib, s, x, d = self.R, self.lib, self.s, self.x, self.dgrad_of
        N, H, W, M, k_ch, cout, ldy = self.N, self.H, self.W, self.M, self.k_ch, self.cout, self.ldy

        dg = d is not None and d[1] == k_ch and d[2] == cout          # no channel padding on either side: straight from the forward weights

        def build():
            u, wt = _empty(6 * cout * 3 * k_ch, x.device), d[0] if dg else (self.w() if callable(self.w) else self.w)
            kind = "weight_transform_dgrad" if dg else "weight_transform"
            _timed(R, "k_wino4_weight_dgrad" if dg else "k_wino4_weight", 4.0 * (9 + 18) * cout * k_ch, lambda: check(getattr(lib, "cvk_wino4_" + kind)(
                wt.data_ptr(), u.data_ptr(), *((d[1], d[2]) if dg else (cout, k_ch)), s), "cvk_wino4_" + kind), "byte")
            return u
        U = self._filter("w4", build)
        ws = R.workspace(lib.cvk_conv3x3_wino4_workspace_bytes(N, H, W, k_ch, ldy), x.device)
        ksplit = lib.cvk_conv3x3_wino4_ksplit(N, H, W, k_ch, ldy)
        _timed(R, conv_kernel_name("wino4", ldy), self.flops, lambda: check(
            lib.cvk_conv3x3_wino4_gemm(x.data_ptr(), U.data_ptr(), ws.data_ptr(), N, H, W, k_ch, cout, ldy, s), "cvk_conv3x3_wino4_gemm" + self.what))
        _timed(R, "k_wino4_output", (4.0 + 6.0 * ksplit) * M * ldy, lambda: check(
            lib.cvk_wino4_output(ws.data_ptr(), self.bias, self.y.data_ptr(), self.sp, N, H, W, cout, ldy, ksplit, s), "cvk_wino4_output"), "byte")

    def w2(self):
        """F(2,3) GEMMs (csrc/wino.hip) + output pass."""
        R, lib, s, x = self.R, self.lib, self.s, self.x
        N, H, W, M, k_ch, cout, ldy = self.N, self.H, self.W, self.M, self.k_ch, self.cout, self.ldy

        def build():
            wt = self.w() if callable(self.w) else self.w
            u = _empty(4 * cout * 3 * k_ch, x.device)
            _timed(R, "k_wino_weight", 4.0 * (9 + 12) * cout * k_ch, lambda: check(
                lib.cvk_wino_weight_transform(wt.data_ptr(), u.data_ptr(), cout, k_ch, s), "cvk_wino_weight_transform"), "byte")
            return u
        U = self._filter("w", build)
        ws = R.workspace(lib.cvk_conv3x3_wino_workspace_bytes(N, H, W, ldy), x.device)
        _timed(R, conv_kernel_name("wino", ldy), self.flops, lambda: check(
            lib.cvk_conv3x3_wino_gemm(x.data_ptr(), U.data_ptr(), ws.data_ptr(), N, H, W, k_ch, cout, ldy, s), "cvk_conv3x3_wino_gemm" + self.what))
        _timed(R, "k_wino_output", 12.0 * M * ldy, lambda: check(
            lib.cvk_wino_output(ws.data_ptr(), self.bias, self.y.data_ptr(), self.sp, N, H, W, cout, ldy, s), "cvk_wino_output"), "byte")


def conv_kernel_name(kind, n_cols, k_ch=32):
    """Mirror of the tile dispatch in csrc/conv3x3.hip / wino.hip: the kernel-trace name."""
    if kind == "wino4":
        return "k_conv3x3_wino4<128, 128, 2, 2>" if n_cols > 64 else ("k_conv3x3_wino4<128, 64, 2, 2>" if n_cols > 32 else "k_conv3x3_wino4<128, 32, 4, 1>")
    if kind == "wino":
        return "k_conv3x3_wino<128, 128, 2, 2>" if n_cols > 64 else ("k_conv3x3_wino<128, 64, 2, 2>" if n_cols > 32 else "k_conv3x3_wino<128, 32, 4, 1>")
    if kind == "wgrad":
        if n_cols <= 16 and k_ch == 64:
            return "k_wgrad_smallco"
        t = "128, 128, 2, 2" if n_cols > 64 else ("64, 128, 2, 2" if n_cols > 32 else "32, 256, 1, 4")
        if 32 < n_cols <= 64 and k_ch * 9 <= 64:
            t = "64, 64, 2, 2"
        return f"k_conv3x3_wgrad<{t}>"
    t = "128, 128, 2, 2" if n_cols > 64 else ("128, 64, 2, 2" if n_cols > 32 else "256, 32, 4, 1")
    return f"k_conv3x3_igemm<{t}, {'true' if kind == 'fwd' else 'false'}, {'true' if k_ch % 32 == 0 else 'false'}>"


def bf16_kernel_name(lib, N, H, W, cin_ld, cout, stats):
    """The kernel cvk_conv3x3_bf16s(_wg) dispatches for this geometry, as a kernel trace names it (the library answers:
    cvk_conv3x3_bf16s_kernel is a query of the same dispatch code; csrc/conv_bf16s.hip, csrc/conv_bf16p.hip)."""
    k = lib.cvk_conv3x3_bf16s_kernel(N, H, W, cin_ld, cout, 1 if stats else 0)
    st = "true" if stats else "false"
    if k == 1:
        return f"k_conv_bf16q<{st}>"
    if k in (2, 3):
        return f"k_conv_bf16h<{st}, 0, {'true' if k == 3 else 'false'}>"
    if k in (4, 5):
        return f"k_conv_bf16s_strip<{1 if cin_ld == 32 else 2}, {st}>" + (" x2" if k == 5 else "")
    return f"k_conv_bf16s<{128 if cout > 64 else 64}, {st}>"


# ---- derived-weight cache ---------------------------------------------------------------------------------------------
# Winograd-domain filters, data-grad packs and bf16 copies are functions of the conv weights only; a step used to rebuild
# all of them (~55 launches, 0.5 ms, also in eval mode).  They are now kept per layer and rebuilt when the weights may have
# changed.  A raw-pointer optimizer or a `p.data` write does not touch the parameter's version counter, so validity is
# explicit: an entry is valid while (global optimizer epoch, runner epoch, storage pointer, tensor version) are unchanged.
#   * any torch.optim optimizer step      -> global epoch (torch.optim.optimizer.register_optimizer_step_post_hook)
#   * FlatAdamW.step, load_state_dict, ddp.DataParallel's broadcast, mark_weights_dirty(net) -> runner epoch
#   * .to() / .cuda() / in-place autograd-visible ops -> storage pointer / version counter
# FAIL-SAFE in training: a TRAINING pass (forward with a backward to follow) never trusts entries of earlier passes — its
# signature carries a per-pass token, so the tensors are built once per pass (one batched launch in bf16 mode) and shared by that
# pass's forward and backward only.  Writes nobody can see (`p.data.copy_()` of an EMA swap, manual re-initialisation, a foreign
# kernel, a freed-and-reallocated parameter at the same address) are therefore always picked up in training, as stock torch
# picks them up.  Only eval / no-grad passes reuse entries across calls; THERE an invisible in-place write needs
# `mark_weights_dirty(net)`.
# Never used while a stream capture is running: a replayed graph must recompute the derived tensors from the live weights.
WEIGHT_EPOCH = [0]
WCACHE_DEFAULT = os.environ.get("CVK_WEIGHT_CACHE", "1") != "0"


def _bump_epoch(*_a, **_k):
    WEIGHT_EPOCH[0] += 1


try:
    from torch.optim.optimizer import register_optimizer_step_post_hook as _reg_opt_hook
    _reg_opt_hook(_bump_epoch)
except ImportError:                      # very old torch: no global hook, the cache stays off
    WCACHE_DEFAULT = False


def mark_weights_dirty(module):
    """Tell the executor that the parameters of `module` were changed behind its back (p.data writes, custom kernels):
    every derived weight tensor (Winograd-domain filters, data-grad packs, bf16 copies) is rebuilt on next use."""
    from .modules import runner_of
    runner_of(module).wepoch += 1


PROF = None     # bench.py sets this to a list: every _timed call then appends (kernel name, work, start event, end event, unit, executed)
PROF_OPS = None  # a list beside PROF (tests): every _timed call also appends (op index, "fwd" | "bwd" | None) of the op that launched it
_CUR_OP = [None]


def _timed(R, name, work, fn, unit="flop", executed=None, nbytes=None):
    """Run fn(); when a profile list is attached (bench.py sets engine.PROF), bracket it with HIP events on the launch
    stream.  `work` is the ALGORITHMIC work of the call: FLOPs for the conv kernels, HBM bytes (each input read once,
    each output written once, at the storage dtype) for the memory-bound kernels.  `executed`: FLOPs the kernel really
    issues to the matrix pipe when that is not a fixed share of `work` (bench.py knows the fixed shares by kernel name).
    `nbytes`: for conv kernels that sit near the HBM side of the ridge (the 3-channel stem, the 12-class head: SURVEY §8d) their
    algorithmic bytes as well — bench.py then reports BOTH roofline fractions for them."""
    if PROF is None:
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    PROF.append((name, work, e0, e1, unit, executed, nbytes))
    if PROF_OPS is not None:
        PROF_OPS.append(_CUR_OP[0])
    return r


# ===================================================================================================== ops
class Op:
    idx = -1

    def fwd(self, R, st):
        raise NotImplementedError

    def bwd(self, R, st):
        pass


class ConvBnRelu(Op):
    """ReLU(BN(conv3x3(x)+b)) — reference BasicConv2d (models/unet.py:5-17) / BasicConv (models/segnet.py:5-17)."""

    def __init__(self, src, dst, pslot, holder, cin, cout, src_needs_grad, bn_train=True, req=(True, True, True, True)):
        self.src, self.dst, self.pslot, self.holder = src, dst, pslot, holder
        self.cin, self.cout, self.src_needs_grad = cin, cout, src_needs_grad
        # fixed when the plan is recorded (part of the plan-cache key, modules._run): the BatchNorm child's own mode, and which of
        # [conv weight, conv bias, gamma, beta] need a gradient.  src_needs_grad: something upstream of the input needs its gradient.
        self.bn_train = bool(bn_train)
        self.w_req, self.b_req, self.g_req, self.be_req = (bool(r) for r in req)
        self.name = None            # the block's module name (modules._run), for error messages
        self.pool_dst = None        # the ActBuf of a MaxPool2d(2,2) of this block's output, written by the BN-apply pass
        self.pool_op = None
        assert src.C == cin and dst.C == cout and dst.H == src.H and dst.W == src.W

    @property
    def trainable(self):
        """A parameter of this block receives a gradient."""
        return self.w_req or self.b_req or self.g_req or self.be_req

    @property
    def active(self):
        """The block runs any backward work: its own parameters' gradients, or the gradient of its input."""
        return self.trainable or self.src_needs_grad

    @property
    def label(self):
        return self.name or "conv block #%d" % self.pslot

    def _grad_targets(self, R, st, ld):
        """(dW, dbias, dgamma, dbeta) pointers: the flat gradient buffer's segments of the trainable parameters; None for a frozen conv weight or
        bias (nothing writes their segments); a scratch pair for frozen BatchNorm parameters (the BatchNorm-backward passes need the two sums
        as temporaries in training mode, and the E-plane passes always take the pointers)."""
        gw, gb, gg, gbe = R.grad_ptrs(st, self.pslot)
        if not (self.g_req and self.be_req):
            sc = _empty(2 * ld, st.device)
            st.scratch.append(sc)
            gg = gg if self.g_req else sc.data_ptr()
            gbe = gbe if self.be_req else sc.data_ptr() + 4 * ld
        return (gw if self.w_req else None), (gb if self.b_req else None), gg, gbe

    def _weight_fwd(self, R, st, w):
        """[Cout][9][ld_in]: the parameter itself when it is channels_last and needs no channel padding."""
        ldx = self.src.ld
        if ldx == self.cin and w.is_contiguous(memory_format=torch.channels_last):
            return w
        wc = w if w.is_contiguous(memory_format=torch.channels_last) else w.contiguous(memory_format=torch.channels_last)
        def build():
            out = _empty(self.cout * 9 * ldx, w.device)
            check(R.lib.cvk_pack_weight_fwd(wc.data_ptr(), out.data_ptr(), self.cout, self.cin, ldx, st.stream), "cvk_pack_weight_fwd")
            return out
        return R.derived(((self.pslot, "f"), "pack"), w, build)

    def _conv(self, R, st, rt, X, wk, b, y, stats):
        """y = conv3x3(X, wk) + b (+ BN statistics partials) through the route's forward family.  Returns (counts, kept): (count, pointer)
        when the partials carry pixel counts; (V, its amax block) when the route keeps the input transform for the weight-grad."""
        lib, s, src = R.lib, st.stream, self.src
        N, H, W, M, C, ldy = src.N, src.H, src.W, src.M, self.cout, pad4(self.cout)
        sp = stats.data_ptr() if stats is not None else None
        flops = 18.0 * M * C * self.cin
        if rt.fwd == "thin":
            Pt = lib.cvk_thin_stat_partials(N, H, W, src.ld)
            cnt = sp + 4 * 2 * Pt * C if sp is not None else None
            head = src.ld == 64
            _timed(R, "k_thin_co_fwd" if head else "k_thin_ci_fwd", flops, lambda: check(
                lib.cvk_conv3x3_thin_fwd(X.data_ptr(), wk.data_ptr(), b.data_ptr(), y.data_ptr(), sp, cnt, N, H, W, src.ld, C, ldy, s),
                "cvk_conv3x3_thin_fwd"), executed=18.0 * M * (16 * self.cin if head else C * src.ld), nbytes=4.0 * M * (src.ld + ldy))
            return ((Pt, cnt) if sp is not None else None), None
        if rt.fwd == "direct":
            _timed(R, conv_kernel_name("fwd", ldy, src.ld), flops, lambda: check(
                lib.cvk_conv3x3_fwd(X.data_ptr(), wk.data_ptr(), b.data_ptr(), y.data_ptr(), sp, N, H, W, src.ld, C, ldy, s),
                "cvk_conv3x3_fwd"))
            return None, None
        c = WinoConv(R, s, X, wk, b.data_ptr(), y, sp, N, H, W, src.ld, C, ldy, flops, st.params[4 * self.pslot], (self.pslot, "f"))
        counted = c.run(rt.fwd, rt.tile, rt.split, keep=rt.keeps_v, x_amax=st.amax.get(src.id))
        return counted, ((c.v, c.v_amax) if rt.keeps_v else None)

    def fwd(self, R, st):
        if st.plan.bf16:
            return self._fwd_bf16(R, st)
        lib, s = R.lib, st.stream
        src, dst = self.src, self.dst
        rt = st.routes[self.idx]
        X = st.act[src.id]
        w, b, gamma, beta = st.params[4 * self.pslot:4 * self.pslot + 4]
        dev = X.device
        N, H, W = src.N, src.H, src.W
        M, C, ldy = src.M, self.cout, pad4(self.cout)
        wk = self._weight_fwd(R, st, w)
        y = _empty(M * ldy, dev)
        bnp = _empty(4 * ldy, dev)                      # mean | rstd | scale | shift
        pm, pr, psc, psh = (bnp.data_ptr() + 4 * ldy * i for i in range(4))
        conv, bn = self.holder.conv_bn()
        if self.bn_train:
            P = (M + _lib.CVK_STAT_ROWS - 1) // _lib.CVK_STAT_ROWS
            Pm = max(P, lib.cvk_w2d_stat_partials(N, H, W), lib.cvk_w6_stat_partials(N, H, W), lib.cvk_thin_stat_partials(N, H, W, src.ld))   # room for any partial layout (+ counts)
            stats = _empty(2 * Pm * C + Pm, dev)
            if M <= 1:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size {[N, C, H, W]}")
            counted, kept = self._conv(R, st, rt, X, wk, b, y, stats)
            wsb = lib.cvk_bn_finalize_workspace_bytes(Pm, C)
            ws = R.workspace(wsb, dev)
            track = bn.track_running_stats and bn.running_mean is not None
            mom = 0.1 if bn.momentum is None else float(bn.momentum)
            run = (bn.running_mean.data_ptr() if track else None, bn.running_var.data_ptr() if track else None,
                   bn.num_batches_tracked.data_ptr() if track else None)
            if counted is None:
                check(lib.cvk_bn_finalize(stats.data_ptr(), P, M, C, gamma.data_ptr(), beta.data_ptr(), pm, pr, psc, psh, *run,
                                          mom, float(bn.eps), ws.data_ptr(), wsb, s), "cvk_bn_finalize")
            else:       # partials with explicit pixel counts (2-D Winograd path: P2 <= P partials in the same buffer)
                check(lib.cvk_bn_finalize_counts(stats.data_ptr(), counted[1], counted[0], M, C, gamma.data_ptr(), beta.data_ptr(),
                                                 pm, pr, psc, psh, *run, mom, float(bn.eps), ws.data_ptr(), wsb, s),
                      "cvk_bn_finalize_counts")
        else:
            _, kept = self._conv(R, st, rt, X, wk, b, y, None)
            check(lib.cvk_bn_eval_params(gamma.data_ptr(), beta.data_ptr(), bn.running_mean.data_ptr(),
                                         bn.running_var.data_ptr(), pm, pr, psc, psh, C, float(bn.eps), s), "cvk_bn_eval_params")
        out = R.alloc_act(st, dst.buf, dev)
        pooled = False
        if self.pool_dst is not None and C % 4 == 0:
            # the 2x2 max pool behind this block is written by the same pass (csrc/bn.hip k_bn_relu_apply_pool)
            pool = R.alloc_act(st, self.pool_dst, dev)
            code = None
            if self.pool_op.keep_code:
                code = torch.empty(self.pool_dst.M * self.pool_dst.ld, device=dev, dtype=torch.uint8)
            aw, ap = st.amax.get(dst.buf.id), st.amax.get(self.pool_dst.id)
            if aw is not None or ap is not None:
                rc = _timed(R, "k_bn_relu_apply<pool>", (8.0 + 1.0 + (0.25 if code is not None else 0.0)) * M * C, lambda: lib.cvk_bn_relu_apply_pool_amax(
                    y.data_ptr(), ldy, psc, psh, dst.cview(out), pool.data_ptr(), code.data_ptr() if code is not None else None,
                    N, H, W, C, aw.data_ptr() if aw is not None else None, ap.data_ptr() if ap is not None else None, s), "byte")
            else:
                rc = _timed(R, "k_bn_relu_apply<pool>", (8.0 + 1.0 + (0.25 if code is not None else 0.0)) * M * C, lambda: lib.cvk_bn_relu_apply_pool(
                    y.data_ptr(), ldy, psc, psh, dst.cview(out), pool.data_ptr(), code.data_ptr() if code is not None else None,
                    N, H, W, C, s), "byte")
            pooled = rc == 0
            if not pooled and ap is not None:
                st.amax.pop(self.pool_dst.id)          # the separate pool pass writes that buffer: its reader measures it itself
            if pooled and code is not None:
                st.saved[self.pool_op.idx] = code
        st.pooled_by_block[self.idx] = pooled
        if not pooled:
            aw = st.amax.get(dst.buf.id)
            if aw is not None:
                _timed(R, "k_bn_relu_apply", 8.0 * M * C, lambda: check(
                    lib.cvk_bn_relu_apply_amax(y.data_ptr(), ldy, psc, psh, dst.cview(out), N, H, W, C, aw.data_ptr(), s), "cvk_bn_relu_apply_amax"), "byte")
            else:
                _timed(R, "k_bn_relu_apply", 8.0 * M * C, lambda: check(
                    lib.cvk_bn_relu_apply(y.data_ptr(), ldy, psc, psh, dst.cview(out), N, H, W, C, s), "cvk_bn_relu_apply"), "byte")
        if st.need_grad and self.active:
            st.saved[self.idx] = (y, bnp, rt, kept)

    # BatchNorm-backward passes that also write the weight-grad's transformed dy (route bn_bwd): mode of cvk_bn_bwd_dx_e_amax, the entry point
    # without the amax word, plane bytes written per 4-column group and channel
    _BN_E = {"dx+E": (0, "cvk_bn_bwd_dx_e", 16.0), "dx+E6": (1, "cvk_bn_bwd_dx_e6", 24.0), "dx+E4p": (2, "cvk_bn_bwd_dx_e4p", 16.0)}

    def _bn_bwd(self, R, st, kind, head, part, PB, gb, want_amax):
        """BatchNorm + ReLU backward (csrc/bn.hip): dy from dO and, for kind != "dx" (route bn_bwd), the weight-grad's E planes in the same pass.
        head: cvk_bn_bwd_dx's arguments before the partials.  Returns (planes, amax block of dy if want_amax); planes None after the plain
        pass, which also runs when a planes pass refuses the layout (rc != 0: a strided view) — the weight-grad then transforms dy itself."""
        lib, s, src = R.lib, st.stream, self.src
        N, H, W, M, C, ldy = src.N, src.H, src.W, src.M, self.cout, pad4(self.cout)
        tail = (part.data_ptr(), N, H, W, C, 1 if self.bn_train else 0)
        if kind != "dx":
            mode, plain, eb = self._BN_E[kind]
            if kind == "dx+E":
                E = _empty(4 * N * H * ((W + 3) // 4) * ldy, st.device)
            else:
                E = _empty((4 if mode == 2 else 6) * lib.cvk_wgradp_plane_rows(N, H, W) * C, st.device)
                check((lib.cvk_wgradp_zero_pads4 if mode == 2 else lib.cvk_wgradp_zero_pads)(E.data_ptr(), N, H, W, C, s), "cvk_wgradp_zero_pads")
            blk = st.amax_spare[-1] if want_amax else None
            rc = _timed(R, "k_bn_bwd<%s>" % kind, (12.0 * M + eb * N * H * ((W + 3) // 4)) * C, lambda: (
                lib.cvk_bn_bwd_dx_e_amax(mode, *head, E.data_ptr(), *tail, blk.data_ptr(), s) if blk is not None
                else getattr(lib, plain)(*head, E.data_ptr(), *tail, s)), "byte")
            if rc == 0:
                if gb is not None:      # conv bias grad: finalised with the others, in one launch
                    R.defer_colsum(st, part, lib.cvk_bn_bwd_e_blocks(N, H, W), C, gb)
                return E, (st.amax_spare.pop() if blk is not None else None)
        am = st.amax_spare.pop() if want_amax else None         # a zeroed word: the pass that writes dy leaves its largest magnitude there
        fn, extra = ("cvk_bn_bwd_dx_amax", (am.data_ptr(),)) if am is not None else ("cvk_bn_bwd_dx", ())
        _timed(R, "k_bn_bwd<dx>", 12.0 * M * C, lambda: check(getattr(lib, fn)(*head, *tail, *extra, s), fn), "byte")
        if gb is not None:
            R.defer_colsum(st, part, PB, C, gb)
        return None, am

    def bwd(self, R, st):
        if st.plan.bf16:
            return self._bwd_bf16(R, st)
        lib, s = R.lib, st.stream
        src, dst = self.src, self.dst
        saved = st.saved.pop(self.idx, None)
        if not self.active:         # frozen block with nothing upstream that needs a gradient: no backward work at all
            return
        y, bnp, rt, kept = saved
        X = st.act[src.id]
        dev = X.device
        N, H, W = src.N, src.H, src.W
        M, C, ldy = src.M, self.cout, pad4(self.cout)
        flops = 18.0 * M * C * self.cin
        pm, pr, psc, psh = (bnp.data_ptr() + 4 * ldy * i for i in range(4))
        w = st.params[4 * self.pslot]
        gw, gb, gg, gbe = self._grad_targets(R, st, ldy)
        dO = dst.cview(st.grad[dst.buf.id])
        PB = lib.cvk_bn_bwd_blocks(M)
        part = _empty(2 * PB * C, dev)
        pre = st.bnred.pop(self.idx, None)
        if pre is not None:     # the data-grad that wrote dO summed it already (csrc/wino4f.hip BNR epilogue)
            check(lib.cvk_colsum_finalize(pre[0].data_ptr(), pre[1], C, gbe, gg, s), "cvk_colsum_finalize")
        elif self.bn_train or self.g_req or self.be_req:        # eval-mode BatchNorm with frozen gamma / beta needs neither sum
            _timed(R, "k_bn_bwd<reduce>", 8.0 * M * C, lambda: check(
                lib.cvk_bn_bwd_reduce(dO, y.data_ptr(), ldy, psc, psh, pm, pr, part.data_ptr(), N, H, W, C, s), "cvk_bn_bwd_reduce"), "byte")
            check(lib.cvk_colsum_finalize(part.data_ptr(), PB, C, gbe, gg, s), "cvk_colsum_finalize")   # dbeta, dgamma
        del pre
        if not (self.w_req or self.b_req or self.src_needs_grad):     # only gamma / beta train: dy is not needed
            R.grads_ready(st, self.pslot)
            return
        if rt.bn_bwd == "dx+E4p":
            # the plane GEMM reads E0 / E5 (columns of dy) from dy itself: dy carries a zeroed slack behind its last row (cvk_wgradp_gemm_sm_dy)
            dyb = _empty(M * ldy + lib.cvk_wgradp_dy_slack(W) * ldy, dev)
            dyb[M * ldy:].zero_()
            dy = dyb[:M * ldy]
        else:
            dy = torch.zeros(M * ldy, device=dev, dtype=_F32) if ldy != C else _empty(M * ldy, dev)
        E, am_dy = self._bn_bwd(R, st, rt.bn_bwd, (dO, y.data_ptr(), ldy, psc, psh, pm, pr, gg, gbe, dy.data_ptr(), ldy), part, PB, gb,
                                rt.dy_amax and bool(st.amax_spare))
        del y
        V, am_v = kept if kept is not None else (None, None)
        # 2-D data-grad and weight-grad with the same tile: dy is transformed for both in ONE launch (csrc/wino2d.hip k_w2d_dy_both): E for
        # the weight-grad, V' for the data-grad; dy crosses the fabric once
        Eb = Vb = None
        if rt.dy_both:
            tile, fmt = rt.tile, rt.split
            NX = 64 if tile == 6 else 36
            T = w2fn(lib, tile, "tiles")(N, H, W)
            n, pdt = (NX * (C // 32) * fmt * lib.cvk_split3_rows_pad(T, 256) * 32, _BF16 if fmt == 3 else torch.float16) if fmt else \
                (NX * lib.cvk_w2d_tpad(T) * C + 128, _F32)
            Eb, Vb = torch.empty(n, device=dev, dtype=pdt), torch.empty(n, device=dev, dtype=pdt)
            if fmt:
                if fmt == 2 and am_dy is None:
                    am_dy = absmax(R, dy, M, C, ldy, s, "dy")
                _timed(R, "k_w2d_dy<both,%s>" % ("split3" if fmt == 3 else "split2h"), (4.0 * M + 4.0 * fmt * NX * T) * C, lambda: check(
                    lib.cvk_w2d_dy_transform_both_split(fmt, tile, dy.data_ptr(), ldy, Vb.data_ptr(), Eb.data_ptr(), 1,
                                                        am_dy.data_ptr() if am_dy is not None else None, N, H, W, C, s),
                    "cvk_w2d_dy_transform_both_split"), "byte")
            else:
                _timed(R, "k_w2d_dy<both>", 4.0 * (M + 2 * NX * T) * C, lambda: check(
                    w2fn(lib, tile, "dy_transform_both")(dy.data_ptr(), ldy, Vb.data_ptr(), Eb.data_ptr(), N, H, W, C, s),
                    "cvk_w2d_dy_transform_both"), "byte")
        if self.src_needs_grad:
            if src.id in st.grad:
                raise NotImplementedError("conv data-grad must be the first writer of its input's gradient buffer")
            wc = w if w.is_contiguous(memory_format=torch.channels_last) else w.contiguous(memory_format=torch.channels_last)

            def packed():       # [Cin_pad][9][Cout_pad] rotated + transposed filter for the data-grad-as-forward kernels
                wd_ = _empty(src.ld * 9 * ldy, dev)
                _timed(R, "k_pack_weight_dgrad", 4.0 * 9 * (C * self.cin + src.ld * ldy), lambda: check(
                    lib.cvk_pack_weight_dgrad(wc.data_ptr(), wd_.data_ptr(), C, self.cin, src.ld, ldy, s), "cvk_pack_weight_dgrad"), "byte")
                return wd_
            dX = _empty(M * src.ld, dev).view(N, H, W, src.ld)
            wd = R.derived(((self.pslot, "d"), "pack"), w, packed) if rt.dgrad in ("thin", "direct") else None
            if rt.dgrad == "thin":          # the head's data-grad: 12 -> 64 (csrc/thin.hip)
                _timed(R, "k_thin_ci_fwd(dgrad)", flops, lambda: check(
                    lib.cvk_conv3x3_thin_fwd(dy.data_ptr(), wd.data_ptr(), None, dX.data_ptr(), None, None, N, H, W, ldy, src.ld, src.ld, s),
                    "cvk_conv3x3_thin_fwd(dgrad)"), executed=18.0 * M * ldy * src.ld, nbytes=4.0 * M * (src.ld + ldy))
            elif rt.dgrad == "direct":
                _timed(R, conv_kernel_name("dgrad", src.ld, ldy), flops, lambda: check(
                    lib.cvk_conv3x3_fwd(dy.data_ptr(), wd.data_ptr(), None, dX.data_ptr(), None, N, H, W, ldy, src.ld, src.ld, s),
                    "cvk_conv3x3_fwd(dgrad)"))
            else:
                # dX is the whole gradient of the producing block's activation when this conv is its only reader: the fused kernel then sums
                # it for that block's BatchNorm backward on the way out (training-mode statistics only)
                prod = st.plan.sole_producer(src) if rt.dgrad_bnred else None
                bnred = None
                if prod is not None and prod.bn_train and prod.idx in st.saved and pad4(prod.cout) == prod.cout == src.ld:
                    pb = st.saved[prod.idx][1].data_ptr()
                    bnred = (st.saved[prod.idx][0].data_ptr(), pb + 8 * src.ld, pb + 12 * src.ld, pb, pb + 4 * src.ld)
                c = WinoConv(R, s, dy, packed, None, dX, None, N, H, W, ldy, src.ld, src.ld, flops, w, (self.pslot, "d"), "(dgrad)",
                             dgrad_of=(wc, C, self.cin))
                c.run(rt.dgrad, rt.dgrad_tile, rt.split, v_pre=Vb, x_amax=am_dy, bnred=bnred)
                if c.bnred_sums is not None:
                    st.bnred[prod.idx] = c.bnred_sums
            st.grad[src.id] = dX
        if rt.wgrad is None:        # frozen conv weight: no weight-grad launch
            pass
        elif rt.wgrad in W2D:
            tile = rt.tile
            NX = 64 if tile == 6 else 36
            T = w2fn(lib, tile, "tiles")(N, H, W)
            if rt.wgrad == "w2d_split":
                fmt = rt.split
                Tp = lib.cvk_split3_rows_pad(T, 256)
                f = lib.cvk_w2d_gemm_tn_split3_ksplit(NX, Tp, src.ld, C)
                ws = R.workspace(4 * f * NX * C * src.ld, dev)
                _timed(R, "k_gemm_tn_" + ("split3" if fmt == 3 else "split2h"), flops, lambda: check(
                    lib.cvk_w2d_gemm_tn_split(fmt, tile, Eb.data_ptr(), V.data_ptr(), ws.data_ptr(), am_dy.data_ptr() if am_dy is not None else None,
                                              am_v.data_ptr() if am_v is not None else None, NX, Tp, src.ld, C, s), "cvk_w2d_gemm_tn_split"),
                    executed=2.0 * (6 if fmt == 3 else 3) * NX * Tp * src.ld * C)
                _timed(R, "k_w2d_wgrad_out", 4.0 * (NX * f + 9) * C * self.cin, lambda: check(
                    lib.cvk_w2d_wgrad_output_f(tile, ws.data_ptr(), gw, self.cin, src.ld, C, f, s), "cvk_w2d_wgrad_output_f"), "byte")
            else:
                Tp = lib.cvk_w2d_tpad(T)
                vfl, efl = NX * Tp * src.ld + 128, NX * Tp * C + 128
                f = w2fn(lib, tile, "wgrad_ksplit")(T, src.ld, C)
                if V is None:           # the forward pass ran another family: transform x now
                    V = _empty(vfl, dev)
                    _timed(R, "k_w2d_input", 4.0 * (M + NX * T) * src.ld, lambda: check(
                        w2fn(lib, tile, "input_transform")(X.data_ptr(), V.data_ptr(), N, H, W, src.ld, s), "cvk_w2d_input_transform(wgrad)"), "byte")
                ws = R.workspace(4 * ((0 if Eb is not None else efl) + f * NX * C * src.ld), dev)
                Ep, Pp = (Eb.data_ptr(), ws.data_ptr()) if Eb is not None else (ws.data_ptr(), ws.data_ptr() + 4 * efl)
                if Eb is None:          # else E came with the data-grad's V'
                    _timed(R, "k_w2d_dy", 4.0 * (M + NX * T) * C, lambda: check(
                        w2fn(lib, tile, "dy_transform")(dy.data_ptr(), ldy, Ep, N, H, W, C, s), "cvk_w2d_dy_transform"), "byte")
                _timed(R, "k_w2d_gemm_tn", flops, lambda: check(
                    w2fn(lib, tile, "gemm_tn")(Ep, V.data_ptr(), Pp, T, src.ld, C, s), "cvk_w2d_gemm_tn"), executed=2.0 * NX * Tp * src.ld * C)
                _timed(R, "k_w2d_wgrad_out", 4.0 * (NX * f + 9) * C * self.cin, lambda: check(
                    w2fn(lib, tile, "wgrad_output")(Pp, gw, T, self.cin, src.ld, C, s), "cvk_w2d_wgrad_output"), "byte")
        elif rt.wgrad in ("wgradp", "wgradp_sm"):
            # transposed F(4,3) through transform-domain planes (csrc/wgradp.hip): V from the forward launch ("wgradp_sm", slice-major) or from
            # a pass over x; E from the BatchNorm-backward pass, or from a pass over dy when that one fell back
            own_v = rt.wgrad == "wgradp"
            rows6 = lib.cvk_wgradp_plane_rows(N, H, W)
            wsb = lib.cvk_wgradp_gemm_workspace_bytes(N, H, W, src.ld, C)
            nE = 0 if E is not None else 6 * rows6 * C
            nV = 6 * rows6 * src.ld if own_v else 0
            ws = R.workspace(4 * (nV + nE) + wsb, dev)
            V6p = ws.data_ptr() if own_v else V.data_ptr()
            E6p = E.data_ptr() if E is not None else ws.data_ptr() + 4 * nV
            slabp = ws.data_ptr() + 4 * (nV + nE)
            if own_v:
                _timed(R, "k_wgradp_planes", 4.0 * (M + 6.0 * rows6) * src.ld, lambda: check(
                    lib.cvk_wgradp_planes(X.data_ptr(), src.ld, V6p, N, H, W, src.ld, 0, s), "cvk_wgradp_planes(x)"), "byte")
            if E is None:
                _timed(R, "k_wgradp_planes", 4.0 * (M + 6.0 * rows6) * C, lambda: check(
                    lib.cvk_wgradp_planes(dy.data_ptr(), ldy, E6p, N, H, W, C, 1, s), "cvk_wgradp_planes(dy)"), "byte")
            sm_dy = rt.bn_bwd == "dx+E4p" and E is not None          # E0 / E5 read from dy
            fn = "cvk_wgradp_gemm_sm_dy" if sm_dy else ("cvk_wgradp_gemm" if own_v else "cvk_wgradp_gemm_sm")
            ev = (E6p, dy.data_ptr(), V6p) if sm_dy else (E6p, V6p)
            _timed(R, "k_wgradp_gemm", flops, lambda: check(getattr(lib, fn)(*ev, gw, N, H, W, self.cin, src.ld, C, slabp, wsb, s), fn),
                   executed=9.0 * M * C * self.cin)
        elif rt.wgrad == "w4":
            # transposed F(4,3): fastest weight-grad on every layer with >= 64 input channels (tools/bench_conv.py wgrad wwino wwino4)
            wsb = lib.cvk_conv3x3_wgrad_wino4_workspace_bytes(N, H, W, src.ld, C, ldy)
            ws = R.workspace(wsb, dev)
            _timed(R, f"k_wgrad_wino4<{'128' if C > 64 else '64'}, 128, 2, 2>", flops, lambda: check(
                lib.cvk_conv3x3_wgrad_wino4(X.data_ptr(), dy.data_ptr(), E.data_ptr() if E is not None else None, gw, N, H, W,
                                            self.cin, src.ld, C, ldy, ws.data_ptr(), wsb, s),
                "cvk_conv3x3_wgrad_wino4"))
        else:       # thin (the stem, the head: csrc/thin.hip), F(2,3) or the direct kernel: one entry-point signature
            fn = {"thin": "cvk_conv3x3_thin_wgrad", "w2": "cvk_conv3x3_wgrad_wino", "direct": "cvk_conv3x3_wgrad"}[rt.wgrad]
            wsb = getattr(lib, fn + "_workspace_bytes")(N, H, W, src.ld, C)
            ws = R.workspace(wsb, dev)
            head = src.ld == 64
            name, kw = {"thin": ("k_thin_co_wgrad" if head else "k_thin_ci_wgrad",
                                 dict(executed=18.0 * M * (16 * self.cin if head else C * 16 / 3.0), nbytes=4.0 * M * (src.ld + ldy))),
                        "w2": (f"k_wgrad_wino<{'128' if C > 64 else '64'}, 128, 2, 2>", {}), "direct": (conv_kernel_name("wgrad", C, src.ld), {})}[rt.wgrad]
            _timed(R, name, flops, lambda: check(getattr(lib, fn)(
                X.data_ptr(), dy.data_ptr(), gw, N, H, W, self.cin, src.ld, C, ldy, ws.data_ptr(), wsb, s), fn), **kw)
        R.grads_ready(st, self.pslot)

    # ---- bf16-storage mode (BASELINE.json configs[3]; csrc/conv_bf16s.hip, csrc/elem_bf16.hip) ------------------------
    def _thin_bf16_mode(self, R, lib, dgrad, ld_dy=0):
        """csrc/thin_bf16.hip mode of this layer's forward (dgrad=False) / data-grad launch, 0 = the general kernels (also with CVK_THIN=0)."""
        if not R.thin or self.src.H * self.src.W * max(self.src.ld, self.cout, ld_dy, 64) * 2 >= 2 ** 31:
            return 0
        if dgrad:
            return lib.cvk_thin_bf16_mode(self.cin, self.cout, ld_dy, self.src.ld, 1) if self.src.ld == 64 and self.cin == 64 else 0
        return lib.cvk_thin_bf16_mode(self.cin, self.cout, self.src.ld, self.cout, 0)

    def _fwd_bf16(self, R, st):
        """bf16 NHWC activations in HBM: conv (bf16 MFMA, fp32 accumulate, fp32 statistics from the accumulators) writes
        the pre-BN tensor y as bf16; ONE elementwise pass applies BN + ReLU, writes the bf16 activation through the
        (concat) view and, for encoder stages, the 2x2 max-pooled tensor as well."""
        lib, s = R.lib, st.stream
        src, dst = self.src, self.dst
        X = st.act[src.id]
        w, b, gamma, beta = st.params[4 * self.pslot:4 * self.pslot + 4]
        dev = X.device
        N, H, W, M, C = src.N, src.H, src.W, src.M, self.cout
        if C % 4:
            raise NotImplementedError("bf16 mode needs output channel counts that are multiples of 4")
        wc = w if w.is_contiguous(memory_format=torch.channels_last) else w.contiguous(memory_format=torch.channels_last)
        def build_wb():
            t = torch.empty(lib.cvk_bf16s_rows_pad(C) * 9 * src.ld, device=dev, dtype=_BF16)
            check(lib.cvk_pack_weight_fwd_bf16(wc.data_ptr(), t.data_ptr(), C, self.cin, src.ld, s), "cvk_pack_weight_fwd_bf16")
            return t
        # the stem (3 -> 64) and the head (64 -> 12) run the register-only thin kernels (csrc/thin_bf16.hip, round 5)
        tmode = self._thin_bf16_mode(R, lib, False)

        def build_thin():
            t = torch.empty(lib.cvk_thin_bf16_pack_elems(tmode), device=dev, dtype=_BF16)
            check(lib.cvk_pack_weight_thin_bf16(wc.data_ptr(), t.data_ptr(), C, self.cin, tmode, s), "cvk_pack_weight_thin_bf16")
            return t
        wb = R.derived(((self.pslot, "f"), "thinb"), w, build_thin) if tmode else R.derived(((self.pslot, "f"), "bf16"), w, build_wb)
        y = torch.empty(M * C, device=dev, dtype=_BF16)
        bnp = _empty(4 * C, dev)
        pm, pr, psc, psh = (bnp.data_ptr() + 4 * C * i for i in range(4))
        conv, bn = self.holder.conv_bn()
        flops = 18.0 * M * C * self.cin
        tname = {1: "k_thinb_head_fwd", 2: "k_thinb_wide<1>"}.get(tmode)
        if self.bn_train:
            if M <= 1:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size {[N, C, H, W]}")
            P = lib.cvk_thin_bf16_stat_partials(N, H, W) if tmode else lib.cvk_bf16s_stat_partials_c(N, H, W, src.ld, C)
            stats = _empty(2 * P * C + P, dev)
            cnt = stats.data_ptr() + 4 * 2 * P * C
            if tmode:
                _timed(R, tname, flops, lambda: check(
                    lib.cvk_conv3x3_thin_bf16(X.data_ptr(), wb.data_ptr(), b.data_ptr(), y.data_ptr(), stats.data_ptr(), cnt, N, H, W, src.ld, C, C,
                                              tmode, s), "cvk_conv3x3_thin_bf16"), nbytes=2.0 * M * (src.ld + C))
            else:
                _timed(R, bf16_kernel_name(lib, N, H, W, src.ld, C, True), flops, lambda: check(
                    lib.cvk_conv3x3_bf16s_wg(X.data_ptr(), wb.data_ptr(), b.data_ptr(), y.data_ptr(), stats.data_ptr(), cnt, N, H, W, src.ld, C, C,
                                             R.launch_wgs(), s), "cvk_conv3x3_bf16s"))
            wsb = lib.cvk_bn_finalize_workspace_bytes(P, C)
            ws = R.workspace(wsb, dev)
            track = bn.track_running_stats and bn.running_mean is not None
            mom = 0.1 if bn.momentum is None else float(bn.momentum)
            check(lib.cvk_bn_finalize_counts(stats.data_ptr(), cnt, P, M, C, gamma.data_ptr(), beta.data_ptr(), pm, pr, psc, psh,
                                             bn.running_mean.data_ptr() if track else None,
                                             bn.running_var.data_ptr() if track else None,
                                             bn.num_batches_tracked.data_ptr() if track else None,
                                             mom, float(bn.eps), ws.data_ptr(), wsb, s), "cvk_bn_finalize_counts")
        else:
            if tmode:
                _timed(R, tname, flops, lambda: check(
                    lib.cvk_conv3x3_thin_bf16(X.data_ptr(), wb.data_ptr(), b.data_ptr(), y.data_ptr(), None, None, N, H, W, src.ld, C, C, tmode, s),
                    "cvk_conv3x3_thin_bf16"), nbytes=2.0 * M * (src.ld + C))
            else:
                _timed(R, bf16_kernel_name(lib, N, H, W, src.ld, C, False), flops, lambda: check(
                    lib.cvk_conv3x3_bf16s(X.data_ptr(), wb.data_ptr(), b.data_ptr(), y.data_ptr(), None, None, N, H, W, src.ld, C, C, s),
                    "cvk_conv3x3_bf16s"))
            check(lib.cvk_bn_eval_params(gamma.data_ptr(), beta.data_ptr(), bn.running_mean.data_ptr(),
                                         bn.running_var.data_ptr(), pm, pr, psc, psh, C, float(bn.eps), s), "cvk_bn_eval_params")
        out = R.alloc_act(st, dst.buf, dev)
        out_f32 = 1 if dst.buf.dtype == _F32 else 0
        pool = None
        if self.pool_dst is not None:
            pool = R.alloc_act(st, self.pool_dst, dev)
        nbytes = (2.0 + (4.0 if out_f32 else 2.0)) * M * C + (0.5 * M * C if pool is not None else 0.0)
        _timed(R, "k_apply_bf16" + ("<pool>" if pool is not None else ""), nbytes, lambda: check(
            lib.cvk_bn_relu_apply_bf16(y.data_ptr(), C, psc, psh, dst.hview(out), out_f32, pool.data_ptr() if pool is not None else None,
                                       N, H, W, C, s), "cvk_bn_relu_apply_bf16"), "byte")
        if st.need_grad and self.active:
            st.saved[self.idx] = (y, bnp)

    def _bwd_bf16(self, R, st):
        lib, s = R.lib, st.stream
        src, dst = self.src, self.dst
        saved = st.saved.pop(self.idx, None)
        if not self.active:
            return
        y, bnp = saved
        X = st.act[src.id]
        dev = X.device
        N, H, W, M, C = src.N, src.H, src.W, src.M, self.cout
        pm, pr, psc, psh = (bnp.data_ptr() + 4 * C * i for i in range(4))
        w = st.params[4 * self.pslot]
        gw, gb, gg, gbe = self._grad_targets(R, st, C)
        G = st.grad[dst.buf.id]
        dO = dst.hview(G)
        do_f32 = 1 if dst.buf.dtype == _F32 else 0
        esz = 4.0 if do_f32 else 2.0
        PB = lib.cvk_bn_bwd_blocks_bf16(M)
        part = _empty(2 * PB * C, dev)
        pre = st.bnred.pop(self.idx, None)
        if pre is not None:     # the pass that wrote dO last summed it already (csrc/elem_bf16.hip k_pool_bwd_bnred_bf16)
            check(lib.cvk_colsum_finalize(pre[0].data_ptr(), pre[1], C, gbe, gg, s), "cvk_colsum_finalize")
        elif self.bn_train or self.g_req or self.be_req:
            _timed(R, "k_bnbwd_bf16<reduce>", (esz + 2.0) * M * C, lambda: check(
                lib.cvk_bn_bwd_reduce_bf16(dO, do_f32, y.data_ptr(), C, psc, psh, pm, pr, part.data_ptr(), N, H, W, C, s),
                "cvk_bn_bwd_reduce_bf16"), "byte")
            check(lib.cvk_colsum_finalize(part.data_ptr(), PB, C, gbe, gg, s), "cvk_colsum_finalize")   # dbeta, dgamma
        del pre
        if not (self.w_req or self.b_req or self.src_needs_grad):
            R.grads_ready(st, self.pslot)
            return
        ld_dy = max(32, C)                              # the data-grad GEMM reads dy in 32-channel K slices
        dy = torch.empty(M * ld_dy, device=dev, dtype=_BF16)
        _timed(R, "k_bnbwd_bf16<dx>", (esz + 4.0) * M * C, lambda: check(
            lib.cvk_bn_bwd_dx_bf16(dO, do_f32, y.data_ptr(), C, psc, psh, pm, pr, gg, gbe, dy.data_ptr(), ld_dy, part.data_ptr(),
                                   N, H, W, C, 1 if self.bn_train else 0, s), "cvk_bn_bwd_dx_bf16"), "byte")
        if gb is not None:
            R.defer_colsum(st, part, PB, C, gb)         # conv bias grad: finalised with the others, in one launch
        del y
        wc = w if w.is_contiguous(memory_format=torch.channels_last) else w.contiguous(memory_format=torch.channels_last)
        flops = 18.0 * M * C * self.cin
        if self.src_needs_grad:
            if src.id in st.grad:
                raise NotImplementedError("conv data-grad must be the first writer of its input's gradient buffer")
            def build_wd():
                t = torch.empty(lib.cvk_bf16s_rows_pad(self.cin) * 9 * ld_dy, device=dev, dtype=_BF16)
                check(lib.cvk_pack_weight_dgrad_bf16(wc.data_ptr(), t.data_ptr(), C, self.cin, ld_dy, s), "cvk_pack_weight_dgrad_bf16")
                return t
            dmode = self._thin_bf16_mode(R, lib, True, ld_dy)

            def build_thin_d():
                t = torch.empty(lib.cvk_thin_bf16_pack_elems(dmode), device=dev, dtype=_BF16)
                check(lib.cvk_pack_weight_thin_bf16(wc.data_ptr(), t.data_ptr(), C, self.cin, dmode, s), "cvk_pack_weight_thin_bf16")
                return t
            dX = torch.empty((N, H, W, src.ld), device=dev, dtype=_BF16)
            if dmode:
                wd = R.derived(((self.pslot, "d"), "thinb"), w, build_thin_d)
                _timed(R, "k_thinb_wide<3>(dgrad)", flops, lambda: check(
                    lib.cvk_conv3x3_thin_bf16(dy.data_ptr(), wd.data_ptr(), None, dX.data_ptr(), None, None, N, H, W, ld_dy, C, src.ld, dmode, s),
                    "cvk_conv3x3_thin_bf16(dgrad)"), nbytes=2.0 * M * (ld_dy + src.ld))
            else:
                wd = R.derived(((self.pslot, "d"), "bf16"), w, build_wd)
                _timed(R, bf16_kernel_name(lib, N, H, W, ld_dy, self.cin, False), flops, lambda: check(
                    lib.cvk_conv3x3_bf16s_wg(dy.data_ptr(), wd.data_ptr(), None, dX.data_ptr(), None, None, N, H, W, ld_dy, self.cin, src.ld,
                                             R.launch_wgs(), s), "cvk_conv3x3_bf16s(dgrad)"))
            st.grad[src.id] = dX
        if gw is None:          # frozen conv weight: no weight-grad launch
            R.grads_ready(st, self.pslot)
            return
        # partial slabs now, the sum over the slabs with every other layer's in ONE launch (Runner.flush_wreduces): nobody reads a weight
        # gradient before the end of backward (or the all-reduce of its bucket); 23 reductions of ~11 us were 0.26 ms of a 21 ms step
        S = lib.cvk_conv3x3_wgrad_bf16s_splits(N, H, W, self.cin, C)
        n = C * 9 * self.cin
        slab = None if S == 1 else _empty(S * n, dev)           # one slab: it is the gradient itself, written in place
        _timed(R, "k_wgrad_bf16r", flops, lambda: check(
            lib.cvk_conv3x3_wgrad_bf16s_slabs(X.data_ptr(), dy.data_ptr(), gw if slab is None else slab.data_ptr(), N, H, W, self.cin, src.ld, C,
                                              ld_dy, 4 * S * n, s), "cvk_conv3x3_wgrad_bf16s_slabs"))
        if slab is not None:
            R.defer_wreduce(st, slab, S, n, gw)
        R.grads_ready(st, self.pslot)


class MaxPool(Op):
    """nn.MaxPool2d(2,2) (models/unet.py:92) / with indices (models/segnet.py:79)."""

    def __init__(self, src_view, dst_buf, keep_code):
        self.src, self.dst, self.keep_code = src_view, dst_buf, keep_code
        self.fused = False          # produced by the preceding block's BN-apply pass
        self.producer_idx = -1
        self.wants = True           # something upstream of the pooled view needs a gradient (Plan._needs_grad)
        if src_view.H < 2 or src_view.W < 2:
            raise RuntimeError(f"max_pool2d: input {src_view.H}x{src_view.W} is too small for a 2x2 window")

    def fwd(self, R, st):
        v, d = self.src, self.dst
        X = st.act[v.buf.id]
        if st.plan.bf16:
            if not self.fused:
                raise NotImplementedError("bf16 mode: a max pool must directly follow a conv block (it is fused into its BN pass)")
            return                                      # the producing block's BN-apply pass already wrote st.act[d.id]
        if self.fused and st.pooled_by_block.get(self.producer_idx, False):
            return                                      # the producing block's BN-apply pass already wrote st.act[d.id] (and the code)
        out = R.alloc_act(st, d, X.device)
        code = None
        if self.keep_code:
            code = torch.empty(d.M * d.ld, device=X.device, dtype=torch.uint8)
            st.saved[self.idx] = code
        _timed(R, "k_maxpool_fwd", 5.0 * v.buf.N * v.H * v.W * v.C, lambda: check(
            R.lib.cvk_maxpool2x2_fwd(v.cview(X), out.data_ptr(), code.data_ptr() if code is not None else None,
                                     v.buf.N, v.H, v.W, v.C, st.stream), "cvk_maxpool2x2_fwd"), "byte")

    def bwd(self, R, st):
        v, d = self.src, self.dst
        if not self.wants or d.id not in st.grad:
            st.grad.pop(d.id, None)
            return
        X = st.act[v.buf.id]
        acc = v.buf.id in st.grad
        if not acc:
            if not v.is_full:
                st.grad[v.buf.id] = torch.zeros_like(X)
            else:
                st.grad[v.buf.id] = torch.empty_like(X)
        # round 6: when the pool directly follows a conv block (its BN-apply pass pooled) this pass is the LAST writer of the block's output
        # gradient — the consumers behind it in the plan ran earlier in backward — and touches every element of it: it then also leaves the block's
        # BatchNorm-backward sums (csrc/pointwise.hip k_pool_scatter_bnred, csrc/elem_bf16.hip k_pool_bwd_bnred_bf16) and the block's reduce pass is
        # not launched
        prod = st.plan.ops[self.producer_idx] if (self.fused and self.producer_idx >= 0) else None
        fuse_sums = (prod is not None and st.training and R.pool_bnred and isinstance(prod, ConvBnRelu) and prod.bn_train and prod.idx in st.saved
                     and prod.idx not in st.bnred and prod.dst.buf is v.buf
                     and (prod.dst.c0, prod.dst.C, prod.dst.y0, prod.dst.x0, prod.dst.H, prod.dst.W) == (v.c0, v.C, v.y0, v.x0, v.H, v.W)
                     and prod.cout == v.C and st.plan.last_gradient_writer(v, prod.idx) == self.idx)
        if st.plan.bf16:
            PBp = R.lib.cvk_maxpool2x2_bwd_bnred_blocks_bf16(v.buf.N, v.H, v.W, v.C) if fuse_sums else 0
            if PBp > 0:
                py, pbnp = st.saved[prod.idx][0], st.saved[prod.idx][1]
                part = _empty(2 * PBp * v.C, X.device)
                rc = _timed(R, "k_pool_bwd_bf16(+bnred)", (2.0 * 0.25 + 2.0 + (4.0 if acc else 2.0) + 2.0) * v.buf.N * v.H * v.W * v.C,
                            lambda: R.lib.cvk_maxpool2x2_bwd_bnred_bf16(
                                st.grad[d.id].data_ptr(), v.hview(X), v.hview(st.grad[v.buf.id]), 1 if acc else 0, v.buf.N, v.H, v.W, v.C,
                                py.data_ptr(), v.C, pbnp.data_ptr() + 8 * v.C, pbnp.data_ptr() + 12 * v.C, pbnp.data_ptr(), pbnp.data_ptr() + 4 * v.C,
                                part.data_ptr(), st.stream), "byte")
                if rc == 0:
                    st.bnred[prod.idx] = (part, PBp)
                    st.grad.pop(d.id)
                    return
            _timed(R, "k_pool_bwd_bf16", (2.0 * 0.25 + 2.0 + (4.0 if acc else 2.0)) * v.buf.N * v.H * v.W * v.C, lambda: check(
                R.lib.cvk_maxpool2x2_bwd_bf16(st.grad[d.id].data_ptr(), v.hview(X), v.hview(st.grad[v.buf.id]), 1 if acc else 0,
                                              v.buf.N, v.H, v.W, v.C, st.stream), "cvk_maxpool2x2_bwd_bf16"), "byte")
            st.grad.pop(d.id)
            return
        code = st.saved.get(self.idx)
        if fuse_sums and pad4(prod.cout) == prod.cout:
            PBp = R.lib.cvk_maxpool2x2_bwd_bnred_blocks(v.buf.N, v.H, v.W, v.C)
            if PBp > 0:
                py, pbnp = st.saved[prod.idx][0], st.saved[prod.idx][1]
                ldp = pad4(prod.cout)
                part = _empty(2 * PBp * v.C, X.device)
                rc = _timed(R, "k_pool_scatter(bwd+bnred)", (1.0 + (0.25 if code is not None else 4.0) + (8.0 if acc else 4.0) + 4.0) * v.buf.N * v.H * v.W * v.C,
                            lambda: R.lib.cvk_maxpool2x2_bwd_bnred(
                                st.grad[d.id].data_ptr(), v.cview(X), code.data_ptr() if code is not None else None, v.cview(st.grad[v.buf.id]),
                                1 if acc else 0, v.buf.N, v.H, v.W, v.C, py.data_ptr(), ldp, pbnp.data_ptr() + 8 * ldp, pbnp.data_ptr() + 12 * ldp,
                                pbnp.data_ptr(), pbnp.data_ptr() + 4 * ldp, part.data_ptr(), st.stream), "byte")
                if rc == 0:
                    st.bnred[prod.idx] = (part, PBp)
                    st.grad.pop(d.id)
                    return
        # bytes per input element: the pooled gradient (1) + the arg-max source (the activations, 4, or the 1-byte codes, 0.25) + the
        # gradient written (4) or accumulated (8)
        _timed(R, "k_pool_scatter(bwd)", (1.0 + (0.25 if code is not None else 4.0) + (8.0 if acc else 4.0)) * v.buf.N * v.H * v.W * v.C, lambda: check(
            R.lib.cvk_maxpool2x2_bwd(st.grad[d.id].data_ptr(), v.cview(X), code.data_ptr() if code is not None else None,
                                     v.cview(st.grad[v.buf.id]), 1 if acc else 0, v.buf.N, v.H, v.W, v.C, st.stream),
            "cvk_maxpool2x2_bwd"), "byte")
        st.grad.pop(d.id)


class Unpool(Op):
    """nn.MaxUnpool2d(2)(x, idx, output_size) (models/segnet.py:80,104-116)."""

    def __init__(self, src_buf, pool_op, dst_buf):
        self.src, self.pool, self.dst = src_buf, pool_op, dst_buf
        self.wants = True

    def fwd(self, R, st):
        V = st.act[self.src.id]
        d = self.dst
        out = R.alloc_act(st, d, V.device)
        if st.plan.bf16:
            # bf16 plans keep no index tensor: the arg-max is recomputed from the pooling layer's stored input, and the forward unpool
            # is the pool's backward kernel without accumulation (a scatter of the pooled values; every other pixel 0)
            pv = self.pool.src
            X = st.act[pv.buf.id]
            assert d.ld == d.C and self.src.ld == d.C, "bf16 unpool: dense tensors (C % 8 == 0, C >= 32)"
            _timed(R, "k_unpool_fwd_bf16", (2.0 * 0.25 + 2.0 + 2.0) * d.M * d.ld, lambda: check(
                R.lib.cvk_maxpool2x2_bwd_bf16(V.data_ptr(), pv.hview(X), d.full_view().hview(out), 0, d.N, d.H, d.W, d.C, st.stream),
                "cvk_maxpool2x2_bwd_bf16(unpool)"), "byte")
            return
        code = st.saved[self.pool.idx]
        _timed(R, "k_unpool_fwd", 5.25 * d.M * d.ld, lambda: check(        # reads pooled values + 1-byte codes, writes the full frame
            R.lib.cvk_maxunpool2x2_fwd(V.data_ptr(), code.data_ptr(), out.data_ptr(), d.N, d.H, d.W, d.ld, st.stream),
            "cvk_maxunpool2x2_fwd"), "byte")

    def bwd(self, R, st):
        d = self.dst
        g = st.grad.pop(d.id, None)
        if not self.wants or g is None:
            return
        dv = torch.empty_like(st.act[self.src.id])
        if st.plan.bf16:
            pv = self.pool.src
            X = st.act[pv.buf.id]
            _timed(R, "k_unpool_bwd_bf16", (2.0 + 2.0 + 2.0 * 0.25) * d.M * d.ld, lambda: check(
                R.lib.cvk_maxunpool2x2_bwd_bf16(g.data_ptr(), pv.hview(X), dv.data_ptr(), d.N, d.H, d.W, d.C, st.stream),
                "cvk_maxunpool2x2_bwd_bf16"), "byte")
            assert self.src.id not in st.grad
            st.grad[self.src.id] = dv
            return
        code = st.saved[self.pool.idx]
        _timed(R, "k_unpool_bwd", 5.25 * d.M * d.ld, lambda: check(
            R.lib.cvk_maxunpool2x2_bwd(g.data_ptr(), code.data_ptr(), dv.data_ptr(), d.N, d.H, d.W, d.ld, st.stream),
            "cvk_maxunpool2x2_bwd"), "byte")
        assert self.src.id not in st.grad
        st.grad[self.src.id] = dv


class Upsample(Op):
    """nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) (models/unet.py:25)."""

    def __init__(self, src_buf, dst_buf):
        self.src, self.dst = src_buf, dst_buf
        self.wants = True

    def fwd(self, R, st):
        X = st.act[self.src.id]
        out = R.alloc_act(st, self.dst, X.device)
        b = self.src
        if st.plan.bf16:
            _timed(R, "k_bilinear_fwd_bf16", 10.0 * b.M * b.ld, lambda: check(
                R.lib.cvk_bilinear_up2_fwd_bf16(X.data_ptr(), out.data_ptr(), b.N, b.H, b.W, b.ld, st.stream), "cvk_bilinear_up2_fwd_bf16"), "byte")
            return
        _timed(R, "k_bilinear_fwd", 20.0 * b.M * b.ld, lambda: check(
            R.lib.cvk_bilinear_up2_fwd(X.data_ptr(), out.data_ptr(), b.N, b.H, b.W, b.ld, st.stream), "cvk_bilinear_up2_fwd"), "byte")
        aw = st.amax.get(self.dst.id)
        if aw is not None:          # align_corners interpolation is a convex combination: |out| <= max |in| (an upper bound serves the scale)
            aw.copy_(st.amax[b.id])

    def bwd(self, R, st):
        g = st.grad.pop(self.dst.id, None)
        if not self.wants or g is None:
            return
        b = self.src
        dx = torch.empty_like(st.act[b.id])
        if st.plan.bf16:
            _timed(R, "k_bilinear_bwd_bf16", 10.0 * b.M * b.ld, lambda: check(
                R.lib.cvk_bilinear_up2_bwd_bf16(g.data_ptr(), dx.data_ptr(), b.N, b.H, b.W, b.ld, st.stream), "cvk_bilinear_up2_bwd_bf16"), "byte")
        else:
            _timed(R, "k_bilinear_bwd", 20.0 * b.M * b.ld, lambda: check(
                R.lib.cvk_bilinear_up2_bwd(g.data_ptr(), dx.data_ptr(), b.N, b.H, b.W, b.ld, st.stream), "cvk_bilinear_up2_bwd"), "byte")
        assert b.id not in st.grad
        st.grad[b.id] = dx


class ZeroFrame(Op):
    """The F.pad border of models/unet.py:120-123, written in place into the concat buffer (forward only)."""

    def __init__(self, view):
        self.view = view

    def fwd(self, R, st):
        v = self.view
        b = v.buf
        t = R.alloc_act(st, b, st.device)
        chan = BufView(b, v.c0, v.C, 0, 0, b.H, b.W)
        if st.plan.bf16:
            check(R.lib.cvk_zero_frame_bf16(chan.hview(t), b.N, b.H, b.W, v.C, v.y0, v.x0, v.H, v.W, st.stream), "cvk_zero_frame_bf16")
            return
        check(R.lib.cvk_zero_frame(chan.cview(t), b.N, b.H, b.W, v.C, v.y0, v.x0, v.H, v.W, st.stream), "cvk_zero_frame")


# ===================================================================================================== plan
class Plan:
    """Recorded op list for one (N, H, W) input geometry."""

    def __init__(self, N, cin, H, W, bf16=False):
        self.N, self.cin, self.H, self.W = N, cin, H, W
        self.bf16 = bool(bf16)      # bf16-storage plan: activation buffers are bf16 (the logits buffer stays fp32)
        self.bufs, self.ops, self.holders = [], [], []
        self.convs = []             # the ConvBnRelu ops by parameter slot
        self._writers = {}          # buffer id -> [(c0, C, op)]: the ops that write channels [c0, c0 + C) of it (gradient reachability)
        self._producer = {}         # (buffer id, first channel) -> the ConvBnRelu op that writes that view
        self._readers = {}          # buffer id -> number of ops that read the buffer (each one adds to its gradient)
        self.routes = {}            # (Runner.kernel_config(), training, need_grad) -> {op index: ConvRoute} (Runner.routes)
        self.input = self.new_buf(cin, H, W, "input")
        self.output = None
        self.input_needs_grad = False

    def new_buf(self, C, H, W, name="", f32=False):
        b = ActBuf(len(self.bufs), self.N, H, W, C, name, _BF16 if (self.bf16 and not f32) else _F32)
        self.bufs.append(b)
        return b

    def add(self, op):
        op.idx = len(self.ops)
        self.ops.append(op)
        return op

    def _reads(self, buf):
        self._readers[buf.id] = self._readers.get(buf.id, 0) + 1

    def _writes(self, buf, c0, C, op):
        self._writers.setdefault(buf.id, []).append((c0, C, op))

    def _needs_grad(self, buf, c0=0, C=None):
        """Does anything upstream of channels [c0, c0 + C) of `buf` need a gradient: a writer of those channels with a trainable parameter or
        whose own input needs one, or the network input when it requires a gradient?  Writers precede readers in the plan, so the flags of
        every writer are final here.  Per channel range: the two halves of a zero-copy concat buffer (a frozen encoder's skip tensor, a
        trainable upsample branch) answer separately."""
        if buf is self.input:
            return bool(self.input_needs_grad)
        C = buf.C if C is None else C
        for w0, wC, op in self._writers.get(buf.id, ()):
            if w0 < c0 + C and c0 < w0 + wC and (op.active if isinstance(op, ConvBnRelu) else op.wants):
                return True
        return False

    def last_gradient_writer(self, view, producer_idx):
        """Index of the op whose backward pass writes LAST into the gradient of `view` (channels [c0, c0 + C) of its buffer): backward runs the plan
        in reverse, so it is the FIRST op behind the producer that reads any of those channels."""
        for op in self.ops[producer_idx + 1:]:
            s = getattr(op, "src", None)
            if s is None:
                continue
            if isinstance(s, BufView):
                if s.buf is view.buf and s.c0 < view.c0 + view.C and view.c0 < s.c0 + s.C:
                    return op.idx
            elif s is view.buf:
                return op.idx
        return -1

    def sole_producer(self, buf):
        """The ConvBnRelu block whose output is exactly `buf` when `buf` has ONE reader — that reader's data-grad is then
        the complete dL/d(activation) of the block, and may carry the block's BatchNorm-backward sums (csrc/wino4f.hip BNR)."""
        op = self._producer.get((buf.id, 0))
        if op is None or not op.dst.is_full or op.dst.buf is not buf or self._readers.get(buf.id, 0) != 1 or self.output is None \
                or self.output.buf is buf:
            return None
        return op

    # ---- builders used by the modules -----------------------------------------------------------------------
    def conv_bn_relu(self, src_buf, holder, dst_view=None):
        cin, cout = holder.in_channels, holder.out_channels
        if src_buf.C != cin:
            raise RuntimeError(f"Given groups=1, weight of size [{cout}, {cin}, 3, 3], expected input[{src_buf.N}, {src_buf.C}, "
                               f"{src_buf.H}, {src_buf.W}] to have {cin} channels, but got {src_buf.C} channels instead")
        if dst_view is None:
            dst_view = self.new_buf(cout, src_buf.H, src_buf.W, holder.tag).full_view()
        pslot = len(self.holders)
        self.holders.append(holder)
        conv, bn = holder.conv_bn()
        req = (conv.weight.requires_grad, conv.bias is not None and conv.bias.requires_grad, bn.weight is not None and bn.weight.requires_grad,
               bn.bias is not None and bn.bias.requires_grad)
        needs = self._needs_grad(src_buf)
        self._reads(src_buf)
        op = self.add(ConvBnRelu(src_buf, dst_view, pslot, holder, cin, cout, needs, bn.training, req))
        self.convs.append(op)
        self._producer[(dst_view.buf.id, dst_view.c0)] = op
        self._writes(dst_view.buf, dst_view.c0, dst_view.C, op)
        return dst_view

    def maxpool(self, src_view, keep_code=False):
        dst = self.new_buf(src_view.C, src_view.H // 2, src_view.W // 2, "pool")
        self._reads(src_view.buf)
        op = self.add(MaxPool(src_view, dst, keep_code))
        op.wants = self._needs_grad(src_view.buf, src_view.c0, src_view.C)
        self._writes(dst, 0, dst.C, op)
        prod = self._producer.get((src_view.buf.id, src_view.c0))
        if prod is not None and prod.dst.C == src_view.C and prod.pool_dst is None \
                and prod.dst.H == src_view.H and prod.dst.W == src_view.W and prod.dst.y0 == src_view.y0 and prod.dst.x0 == src_view.x0:
            prod.pool_dst = dst         # the block's BN-apply pass writes the pooled tensor too (csrc/elem_bf16.hip, csrc/bn.hip)
            prod.pool_op = op
            op.fused = True
            op.producer_idx = prod.idx
        return op

    def unpool(self, src_buf, pool_op):
        v = pool_op.src
        dst = self.new_buf(v.C, v.H, v.W, "unpool")
        self._reads(src_buf)
        op = self.add(Unpool(src_buf, pool_op, dst))
        op.wants = self._needs_grad(src_buf)
        self._writes(dst, 0, dst.C, op)
        return dst

    def upsample(self, src_buf):
        dst = self.new_buf(src_buf.C, 2 * src_buf.H, 2 * src_buf.W, "up")
        self._reads(src_buf)
        op = self.add(Upsample(src_buf, dst))
        op.wants = self._needs_grad(src_buf)
        self._writes(dst, 0, dst.C, op)
        return dst

    def zero_frame(self, view):
        self.add(ZeroFrame(view))

    def seal(self, thin=True):
        """Called once after recording.  bf16-storage plans hand their result (the logits) to the caller and to the loss
        in fp32: the buffer of the output view becomes an fp32 buffer (written by the last block's BN-apply pass).
        Their imported input keeps a pixel pitch of 8 instead of 32 channels when every reader is a stem the thin kernel serves
        (csrc/thin_bf16.hip mode 2: <= 4 real channels -> 64; the weight-grad kernel reads any pitch % 8 == 0): a 3-channel image
        was 64 bytes per pixel — 177 MB written by the import pass and read twice per step at 4 x 720 x 960, 133 MB of it padding."""
        if self.bf16:
            b = self.output.buf
            if not self.output.is_full:
                raise NotImplementedError("bf16 mode: the network output must be a whole buffer")
            b.dtype = _F32
            b.ld = pad4(b.C)
            readers = [op for op in self.ops if getattr(op, "src", None) is self.input]
            if (thin and not self.input_needs_grad and self.input.C <= 4 and readers and self.input is not self.output.buf
                    and all(isinstance(op, ConvBnRelu) and op.cout == 64 for op in readers)
                    and self.input.H * self.input.W * 64 * 2 < 2 ** 31):
                self.input.ld = 8


_SPLIT_ENV_LOGGED = False


def _split_mode_from_env():
    """CVK_W2D_SPLIT (unset | 0 | 1 = 3 | 2 | 3) selects the OPT-IN split-operand arithmetic for every network of the process.  Anything else is
    an error that names the variable; a non-zero value is reported once on stderr, because it moves the fp32 products onto 16-bit MFMAs."""
    global _SPLIT_ENV_LOGGED
    raw = os.environ.get("CVK_W2D_SPLIT")
    if raw is None:
        return 0
    modes = {"0": 0, "1": 3, "3": 3, "2": 2}
    if raw.strip() not in modes:
        raise ValueError(f"CVK_W2D_SPLIT={raw!r}: allowed values are 0 (off, the default), 2 (two fp16 terms) and 3 or 1 (three bf16 terms); "
                         "or leave it unset and call pytorch_camvid_amd.set_split_operands(net, mode)")
    mode = modes[raw.strip()]
    if mode and not _SPLIT_ENV_LOGGED:
        _SPLIT_ENV_LOGGED = True
        import sys
        print(f"pytorch_camvid_amd: CVK_W2D_SPLIT={raw} — fp32 convolution products run as split {'fp16 x 2' if mode == 2 else 'bf16 x 3'} operands "
              "(opt-in, not the exact-fp32 default)", file=sys.stderr)
    return mode


class Runner:
    """Executes a Plan.  One Runner per module instance; plans are cached per input geometry."""

    def __init__(self):
        self.lib = _lib.load()
        self._ws = None
        self._dp_wgs = None
        self._collectives_in_flight = False     # a gradient bucket's all-reduce has been issued and backward is still running
        self.grad_sync = None       # set by ddp.DataParallel
        self.accumulator = None     # set by accumulate.GradAccumulator: folds the flat gradient buffers of a window of micro-batches
        self.wino = WINO_DEFAULT
        self.wino4 = WINO4_DEFAULT
        self.wino4f = WINO4F_DEFAULT
        self.wgradp = WGRADP_DEFAULT
        self.vplanes = VPLANES_DEFAULT      # fused forward launches leave the weight-grad's V planes behind (round 6)
        self.thin = os.environ.get("CVK_THIN", "1") != "0"    # csrc/thin.hip for the stem and the classifier head
        self.pool_bnred = os.environ.get("CVK_POOL_BNRED", "1") != "0"   # BN-backward sums in the max-pool backward pass behind a conv block (round 6)
        self.wino2d = WINO2D_DEFAULT
        # OPT-IN split-operand modes (cvk.set_split_operands): the matrix products of the fp32 convolutions on the 16-bit
        # matrix pipe with split fp32 operands (csrc/split_fmt.h).  Not the product default; bench.py names the mode in `dtype` when it is on.
        self.w2d_split = _split_mode_from_env()      # 0 off | 3: bf16 x 3 | 2: fp16 x 2
        self.w2tile_cfg = W2TILE_DEFAULT    # None = auto (see W2TILE_DEFAULT), 4 or 6 = forced
        self.w2tile = 6                     # the tile of the plan being routed (set by routes)
        self.w2tile_dgrad = 6               # ... of its data-grad launches
        self.bf16 = False           # opt-in: bf16-storage mode (modules.set_conv_precision; BASELINE.json configs[3])
        self.wcache = WCACHE_DEFAULT
        self.wepoch = 0             # bumped by mark_weights_dirty / FlatAdamW.step / load_state_dict
        self._wc = {}               # (layer slot, kind) -> (signature, tensor)
        self._wjobs, self._wjobs_cfg = {}, None      # batchable builds recorded by the last pass (prebuild_fp32)
        self._pass_token = 0        # 0: eval / no-grad passes (entries shared across calls); > 0: the training pass being executed
        self._passes = 0
        self.wcache_builds = 0      # derived tensors built since creation (tests / diagnostics)

    def persistent_wgs(self):
        """Workgroup cap of the persistent (one-workgroup-per-CU) kernels: 0 = every CU.  Under data-parallel training
        CVK_DP_RESERVE_CUS (default 8) CUs are left to RCCL's all-reduce kernels, which run beside backward."""
        gs = self.grad_sync
        if gs is None or (getattr(gs, "world", 1) <= 1 and not getattr(gs, "always_issue", False)):
            return 0
        if self._dp_wgs is None:
            cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
            self._dp_wgs = max(8, cus - int(os.environ.get("CVK_DP_RESERVE_CUS", "8")))
        return self._dp_wgs

    def launch_wgs(self):
        """Workgroup cap for a persistent-kernel launch NOW: the data-parallel cap only while a collective can be in flight — from the
        first gradient bucket's all-reduce to the end of backward (round 5).  The forward pass and the part of backward before the
        first bucket run on every CU: a capped grid changes the tile rounds of the persistent walk (768 tiles = 3 rounds of 256
        workgroups but 4 of 240: measured +7-8 % on the whole bf16 step at world 1 for ANY channel count between 2 and 16, so the cost
        was the lost fit, not the CUs), and there is nothing to leave CUs to before the first bucket is issued.  Results are bitwise
        independent of the cap (tests/test_gpu_wino4f.py, tests/test_gpu_bf16.py)."""
        return self.persistent_wgs() if self._collectives_in_flight else 0

    def derived(self, key, src, build, job=None):
        """The derived weight tensor `key` of parameter `src`: cached while the weights are provably unchanged.
        job = (family, floats, rows, cols, tile, dgrad): how a batched launch can build it straight from `src` (prebuild_fp32 then builds
        it with every other recorded tensor of the network at the start of the next pass)."""
        if not self.wcache or key is None or torch.cuda.is_current_stream_capturing():
            self.wcache_builds += 1
            return build()
        if job is not None:
            self._wjobs[key] = (src, job)
        sig = (WEIGHT_EPOCH[0], self.wepoch, src.data_ptr(), src._version, self._pass_token)
        ent = self._wc.get(key)
        if ent is not None and ent[0] == sig:
            return ent[1]
        t = build()
        self.wcache_builds += 1
        self._wc[key] = (sig, t)
        return t

    def prebuild_fp32(self, plan, st, need_grad):
        """fp32 plans: the Winograd-domain filters the previous pass over this plan asked for (fused F(4,3): 16 per UNet step; 2-D forward
        and data-grad filters: 26), rebuilt in TWO launches (cvk_wino4f_weight_transform_batch, cvk_w2d_weight_transform_batch) instead
        of 42 of 5-15 us each.  Which filters a layer needs follows from its route (WinoConv); the launcher records a job with
        every cached tensor it builds straight from a parameter, and this pass replays the record."""
        if not self.wcache or torch.cuda.is_current_stream_capturing():
            return
        cfg = (id(plan),) + self.kernel_config()
        if cfg != self._wjobs_cfg:          # another plan or other kernel knobs: the record starts over with this pass
            self._wjobs, self._wjobs_cfg = {}, cfg
            return
        live = {p.data_ptr() for p in st.params}
        lib, fam_jobs = self.lib, {"w4f": [], "w2d": []}
        for key, (src, (fam, floats, rows, cols, tile, dgrad)) in self._wjobs.items():
            if src.data_ptr() not in live or (dgrad and not need_grad):
                continue
            sig = (WEIGHT_EPOCH[0], self.wepoch, src.data_ptr(), src._version, self._pass_token)
            ent = self._wc.get(key)
            if ent is not None and ent[0] == sig:
                continue
            t = _empty(floats, src.device)
            fam_jobs[fam].append((_lib.WtJob(src.data_ptr(), t.data_ptr(), rows, cols, tile, dgrad), 4.0 * (src.numel() + floats)))
            self._wc[key] = (sig, t)
            self.wcache_builds += 1
        for fam, fn in (("w4f", lib.cvk_wino4f_weight_transform_batch), ("w2d", lib.cvk_w2d_weight_transform_batch)):
            jobs = fam_jobs[fam]
            for i in range(0, len(jobs), _lib.WT_BATCH_MAX):
                chunk = jobs[i:i + _lib.WT_BATCH_MAX]
                arr = (_lib.WtJob * len(chunk))(*[j for j, _ in chunk])
                _timed(self, "k_weight_transform_batch", sum(b for _, b in chunk),           # filter read + transformed filter written
                       lambda: check(fn(ctypes.addressof(arr), len(chunk), st.stream), "cvk_%s_weight_transform_batch" % fam), "byte")

    def prepack_bf16(self, plan, st, need_grad):
        """bf16 plans: every weight pack the step will ask for and the cache does not hold (forward packs; data-grad packs when a
        backward pass follows) in ONE launch (cvk_pack_weights_bf16_batch) instead of one ~9 us launch per layer and direction."""
        if not self.wcache or torch.cuda.is_current_stream_capturing():
            return
        lib, jobs, keep = self.lib, [], []
        for op in plan.ops:
            if not isinstance(op, ConvBnRelu):
                continue
            w = st.params[4 * op.pslot]
            sig = (WEIGHT_EPOCH[0], self.wepoch, w.data_ptr(), w._version, self._pass_token)
            want = []
            if not op._thin_bf16_mode(self, lib, False):        # thin layers pack their own (tiny) filter formats where they run
                want.append((((op.pslot, "f"), "bf16"), 0, op.cout, op.src.ld))
            if need_grad and op.src_needs_grad and not op._thin_bf16_mode(self, lib, True, max(32, op.cout)):
                want.append((((op.pslot, "d"), "bf16"), 1, op.cin, max(32, op.cout)))
            for key, dgrad, rows, kpad in want:
                ent = self._wc.get(key)
                if ent is not None and ent[0] == sig:
                    continue
                wc = w if w.is_contiguous(memory_format=torch.channels_last) else w.contiguous(memory_format=torch.channels_last)
                t = torch.empty(lib.cvk_bf16s_rows_pad(rows) * 9 * kpad, device=w.device, dtype=_BF16)
                jobs.append(_lib.PackJob(wc.data_ptr(), t.data_ptr(), op.cout, op.cin, kpad, dgrad))
                keep.append(wc)
                self._wc[key] = (sig, t)
                self.wcache_builds += 1
        for i in range(0, len(jobs), _lib.PACK_BATCH_MAX):
            chunk = jobs[i:i + _lib.PACK_BATCH_MAX]
            arr = (_lib.PackJob * len(chunk))(*chunk)
            check(lib.cvk_pack_weights_bf16_batch(ctypes.addressof(arr), len(chunk), st.stream), "cvk_pack_weights_bf16_batch")

    def workspace(self, nbytes, dev):
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != dev:
            self._ws = torch.empty(max(nbytes, 1 << 20), device=dev, dtype=torch.uint8)
        return self._ws

    def alloc_act(self, st, buf, dev):
        t = st.act.get(buf.id)
        if t is None:
            shape = (buf.N, buf.H, buf.W, buf.ld)
            t = torch.zeros(shape, device=dev, dtype=buf.dtype) if buf.ld != buf.C else torch.empty(shape, device=dev, dtype=buf.dtype)
            st.act[buf.id] = t
        return t

    # ---- flat gradient buffer: parameter grads are views, laid out in REVERSE execution order --------------------
    def layout_grads(self, plan, params):
        return layout_grads(params)

    def grad_ptrs(self, st, slot):
        base = st.gflat.data_ptr()
        return tuple(base + 4 * st.goffs[4 * slot + j] for j in range(4))

    def defer_colsum(self, st, part, PB, C, out_ptr):
        """Queue a column-sum finalisation whose result nobody reads before the end of backward (or the all-reduce of its
        gradient bucket): flushed in ONE launch by flush_colsums."""
        st.colsums.append((part, PB, C, out_ptr))
        if len(st.colsums) >= _lib.COLSUM_BATCH_MAX:
            self.flush_colsums(st)

    def defer_wreduce(self, st, slab, splits, n, dw_ptr):
        st.wreduces.append((slab, splits, n, dw_ptr))
        if len(st.wreduces) >= _lib.WREDUCE_BATCH_MAX:
            self.flush_wreduces(st)

    def flush_wreduces(self, st):
        if not st.wreduces:
            return
        arr = (_lib.WReduceJob * len(st.wreduces))(*[_lib.WReduceJob(sl.data_ptr(), dw, n, sp, 0) for sl, sp, n, dw in st.wreduces])
        check(self.lib.cvk_wgrad_reduce_bf16s_batch(ctypes.addressof(arr), len(st.wreduces), st.stream), "cvk_wgrad_reduce_bf16s_batch")
        st.wreduces.clear()

    def flush_colsums(self, st):
        if not st.colsums:
            return
        arr = (_lib.ColsumJob * len(st.colsums))(*[_lib.ColsumJob(p.data_ptr(), o, pb, c) for p, pb, c, o in st.colsums])
        check(self.lib.cvk_colsum_finalize_batch(ctypes.addressof(arr), len(st.colsums), st.stream), "cvk_colsum_finalize_batch")
        st.colsums.clear()

    def grads_ready(self, st, slot):
        if st.sync is not None and st.plan.convs[slot].trainable:
            if st.sync.closes_bucket():     # this layer completes a bucket that is handed to the all-reduce now: its queued bias and
                self.flush_colsums(st)      # weight gradient finalisations must have run (round 5: only then — flushing after every
                self.flush_wreduces(st)     # layer turned the two batched launches of a backward pass into 23 + 23 under data parallel)
            st.sync.layer_done(st, slot)
            self._collectives_in_flight = st.sync.in_flight()

    def begin_sync(self, st, plan, fold=None):
        """The gradient synchroniser's per-call state for this backward pass, or None: no synchroniser, one switched off
        (ddp.DataParallel.no_sync), or a micro-step that does not close its accumulation window.  A skipped pass issues no collective and
        leaves `grad_sync.launched` empty."""
        gs = self.grad_sync
        if gs is None:
            return None
        if not gs.enabled or (fold is not None and not fold.closing):
            gs.launched = []
            return None
        return gs.begin(st, plan)

    # ---- forward / backward -------------------------------------------------------------------------------------
    def plan_amax(self, plan, st):
        """fp16 split-operand mode (w2d_split = 2): the transforms of a split layer scale by the EXACT largest magnitude of the tensor they
        read (csrc/split_fmt.h).  Where every pass that writes a layer's input can leave that maximum on its way (BN-apply passes: csrc/bn.hip
        *_amax; bilinear upsampling: bounded by its input's maximum; the zero frame), the input's buffer gets a device word here and no extra
        pass runs; any other input is measured by cvk_absmax_f32 in WinoConv.  One zero fill per step for all words."""
        if split_fmt(self) != 2 or plan.bf16 or not (st.training and st.need_grad):
            return
        # every conv block that can run a split form: the 2-D split layers (route.split) and the fused F(4,3) of the 64/128-channel levels
        routes = self.routes(plan, True, True)
        layers = [op for op in plan.ops if isinstance(op, ConvBnRelu) and (routes[op.idx].split or (op.src.ld % 32 == 0 and op.cout % 4 == 0))]
        if not layers:
            return

        def writers(buf):
            out = []
            for op in plan.ops:
                if isinstance(op, ConvBnRelu) and (op.dst.buf is buf or (op.pool_dst is buf and op.cout % 4 == 0)):
                    out.append(op)
                elif isinstance(op, (MaxPool, Unpool, Upsample)) and op.dst is buf and not (isinstance(op, MaxPool) and op.fused):
                    out.append(op)
                elif isinstance(op, ZeroFrame) and op.view.buf is buf:
                    out.append(op)
            return out

        want, ok = [], {}

        def fusable(buf):
            if buf.id in ok:
                return ok[buf.id]
            ok[buf.id] = False                      # (cycles cannot occur; guards the recursion anyway)
            ws = writers(buf)
            good = bool(ws) and buf is not plan.input
            for op in ws:
                if isinstance(op, Upsample):
                    good = good and fusable(op.src)
                elif not isinstance(op, (ConvBnRelu, ZeroFrame)):
                    good = False
            ok[buf.id] = good
            if good:
                want.append(buf)
            return good
        for op in layers:
            fusable(op.src)
        blocks = amax_blocks(self.lib, len(want) + len(layers), st.device)
        for i, buf in enumerate(want):
            st.amax[buf.id] = blocks[i]
        st.amax_spare = blocks[len(want):]

    def kernel_config(self):
        """Every switch that changes which kernels run: the route cache, prebuild_fp32's job record and GraphedStep's signature key on it."""
        return (self.wino, self.wino4, self.wino4f, self.wino2d, self.wgradp, self.vplanes, self.thin, self.pool_bnred, self.w2d_split,
                self.w2tile_cfg)

    def routes(self, plan, training, need_grad):
        """{op index: route.ConvRoute} of the conv blocks of an fp32 plan, computed once per configuration and pass kind."""
        key = (self.kernel_config(), training, need_grad)
        r = plan.routes.get(key)
        if r is None:
            if split_fmt(self):
                check_bn_modes(plan, training, "set_split_operands")
            self.w2tile, self.w2tile_dgrad = self.tile_for(plan)
            r = plan.routes[key] = {op.idx: conv_route(self, op, training, need_grad) for op in plan.ops if isinstance(op, ConvBnRelu)}
        return r

    def tile_for(self, plan):
        """(forward / weight-grad tile, data-grad tile) of the 2-D path for a plan."""
        if self.w2tile_cfg in (4, 6):
            return self.w2tile_cfg, self.w2tile_cfg
        return (4, 6) if any(isinstance(op, Unpool) for op in plan.ops) else (6, 6)

    def forward(self, plan, x, params, training, need_grad):
        dev = x.device
        self._collectives_in_flight = False     # finish() of the previous backward waited for every collective
        st = RunState(params, training, need_grad)
        st.device = dev
        st.plan = plan
        if training and need_grad:          # a training pass: derived weights are rebuilt for it (fail-safe, see the cache notes above)
            self._passes += 1
            st.pass_token = self._passes
        self._pass_token = st.pass_token
        st.stream = torch.cuda.current_stream(dev).cuda_stream
        inb = plan.input
        xp = x.permute(0, 2, 3, 1)
        if plan.bf16:
            t = torch.empty((inb.N, inb.H, inb.W, inb.ld), device=dev, dtype=_BF16)
            sN, sC, sH, sW = x.stride()
            check(self.lib.cvk_import_nchw_bf16(x.data_ptr(), sN, sC, sH, sW, t.data_ptr(), inb.ld, inb.N, inb.C, inb.H, inb.W,
                                                st.stream), "cvk_import_nchw_bf16")
            st.act[inb.id] = t
        elif inb.ld == inb.C and xp.is_contiguous():
            st.act[inb.id] = xp                               # already dense NHWC: zero-copy
        else:
            t = torch.empty((inb.N, inb.H, inb.W, inb.ld), device=dev, dtype=_F32)
            sN, sC, sH, sW = x.stride()
            check(self.lib.cvk_import_nchw(x.data_ptr(), sN, sC, sH, sW, t.data_ptr(), inb.ld, inb.N, inb.C, inb.H, inb.W,
                                           st.stream), "cvk_import_nchw")
            st.act[inb.id] = t
        if plan.bf16:
            check_bn_modes(plan, training, "bf16 mode", need_grad, forward_only_ok=True)
            self.prepack_bf16(plan, st, need_grad)
        else:
            st.routes = self.routes(plan, training, need_grad)
            self.prebuild_fp32(plan, st, need_grad)
            self.plan_amax(plan, st)
        for op in plan.ops:
            _CUR_OP[0] = (op.idx, "fwd")
            op.fwd(self, st)
        _CUR_OP[0] = None
        ov = plan.output
        out = st.act[ov.buf.id][..., :ov.buf.C].permute(0, 3, 1, 2)    # logical NCHW, channels_last strides
        if not need_grad:
            st.act.clear()
            st.saved.clear()
        return out, st

    def backward(self, plan, st, gout):
        dev = gout.device
        st.stream = torch.cuda.current_stream(dev).cuda_stream
        self._pass_token = st.pass_token
        params = st.params
        st.goffs, total = self.layout_grads(plan, params)
        # A FRESH flat buffer per backward call (caching allocator: the block freed by `p.grad = None` comes straight
        # back).  The returned .grad tensors are views of it and autograd may hold them for as long as it likes (a
        # second pass through the same network inside one graph, torch.autograd.grad results the caller keeps, manual
        # accumulation across zero_grad(set_to_none=True)): no later backward ever writes into memory handed out here.
        st.gflat = torch.empty(total, device=dev, dtype=_F32)
        # Gradient accumulation (accumulate.GradAccumulator, steps > 1): the micro-steps before the last of a window fold this pass's buffer
        # into the accumulator's own and hand out nothing; the last one folds the accumulator into this pass's fresh buffer, bucket by
        # bucket before each leaves for the all-reduce (ddp._SyncCall.layer_done) or in one launch at the end.  The accumulator's buffer is
        # never handed to autograd, so the promise above holds.
        fold = st.fold = self.accumulator.open_pass(st, plan, total) if self.accumulator is not None else None
        st.sync = self.begin_sync(st, plan, fold)
        self._collectives_in_flight = False
        ob = plan.output.buf
        gp = gout.permute(0, 2, 3, 1)
        if ob.ld == ob.C and gp.is_contiguous():
            st.grad[ob.id] = gp
        else:
            g = torch.zeros((ob.N, ob.H, ob.W, ob.ld), device=dev, dtype=_F32) if ob.ld != ob.C else \
                torch.empty((ob.N, ob.H, ob.W, ob.ld), device=dev, dtype=_F32)
            sN, sC, sH, sW = gout.stride()
            check(self.lib.cvk_import_nchw(gout.data_ptr(), sN, sC, sH, sW, g.data_ptr(), ob.ld, ob.N, ob.C, ob.H, ob.W,
                                           st.stream), "cvk_import_nchw")
            st.grad[ob.id] = g
        for op in reversed(plan.ops):
            _CUR_OP[0] = (op.idx, "bwd")
            op.bwd(self, st)
        _CUR_OP[0] = None
        self.flush_colsums(st)
        self.flush_wreduces(st)
        if fold is not None and st.sync is None:        # with a synchroniser every bucket was folded before it left
            fold.whole(st)
        dx = None
        if plan.input_needs_grad:
            gi = st.grad[plan.input.id]
            dx = gi[..., :plan.input.C].permute(0, 3, 1, 2)
            if plan.bf16:                   # the stem's data-grad is stored as bf16 like every other dX; x.grad is fp32 like x
                dx = dx.float()
        grads = []
        hand_out = fold is None or fold.closing
        for i, p in enumerate(params):
            op = plan.convs[i // 4]
            if not hand_out or not (op.w_req, op.b_req, op.g_req, op.be_req)[i % 4]:
                grads.append(None)          # frozen when the plan was recorded: its segment was never written
                continue
            n = p.numel()
            seg = st.gflat[st.goffs[i]:st.goffs[i] + n]
            if p.dim() == 4:   # [Cout][3][3][Cin] storage -> logical OIHW with channels_last strides
                co, ci, kh, kw = p.shape
                seg = seg.view(co, kh, kw, ci).permute(0, 3, 1, 2)
            else:
                seg = seg.view(p.shape)
            grads.append(seg)
        if st.sync is not None:
            st.sync.finish(st)
        self._collectives_in_flight = False
        st.act.clear(); st.saved.clear(); st.grad.clear(); st.scratch.clear()
        if fold is not None:
            fold.done()
            st.fold = None
            if not hand_out:        # nothing views this pass's buffer: it goes back to the allocator now
                st.gflat = None
        return dx, grads


def check_bn_modes(plan, training, what, need_grad=True, forward_only_ok=False):
    """The bf16 kernels and the split-operand routes serve one BatchNorm mode per pass: a block whose BatchNorm child is in the other mode
    (a sub-module's eval() inside a training pass, or the reverse) is refused by name rather than run in the wrong mode.  forward_only_ok (bf16):
    such a block is served when it runs no backward (a frozen encoder in eval mode: the inference forward pass of the block)."""
    for op in plan.convs:
        if forward_only_ok and not (need_grad and op.active):
            continue
        if op.bn_train != bool(training):
            raise NotImplementedError(f"{what}: BatchNorm of {op.label} is in {'training' if op.bn_train else 'eval'} mode inside a "
                                      f"{'training' if training else 'eval'} pass; per-block BatchNorm modes run in the fp32 mode only")


def layout_grads(params):
    """Offsets (in floats) of every parameter inside the flat gradient buffer.  `params` is the executor's flat list
    [w, b, gamma, beta] per conv block in execution order; the LAST-executed block comes first in the buffer, so the
    buffer fills front to back during backward and contiguous prefixes can be all-reduced early (ddp.GradSync)."""
    offs = [0] * len(params)
    o = 0
    for slot in range(len(params) // 4 - 1, -1, -1):
        for j in range(4):
            i = 4 * slot + j
            offs[i] = o
            o += (params[i].numel() + 3) // 4 * 4     # keep every view 16-byte aligned
    return offs, o


class _PlanFunction(torch.autograd.Function):
    """The whole recorded network as one autograd node: (x, *parameters) -> logits."""

    @staticmethod
    def forward(ctx, runner, plan, training, x, *params):
        out, st = runner.forward(plan, x, params, training, True)
        ctx.runner, ctx.plan, ctx.st = runner, plan, st
        return out

    @staticmethod
    def backward(ctx, gout):
        st = ctx.st
        if st is None:
            raise RuntimeError("Trying to backward through the plan a second time (activations were already freed)")
        ctx.st = None
        dx, grads = ctx.runner.backward(ctx.plan, st, gout)
        return (None, None, None, dx, *grads)


def run_plan(runner, plan, training, x, params):
    need = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
    if not need:
        out, _ = runner.forward(plan, x, params, training, False)
        return out
    return _PlanFunction.apply(runner, plan, training, x, *params)
