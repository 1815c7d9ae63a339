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
import os
from collections import namedtuple

import torch

from . import _lib
from ._lib import View, ViewH, check
from .route import conv_route, pad4, split_fmt
from .route import layer_tile, wgrad2d_pays, wino2d_ok, wino2d_pays, wino4_pays  # noqa: F401  (engine.<predicate> stays importable)

_F32, _BF16 = torch.float32, torch.bfloat16


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
        self.side = False           # this backward pass forks its weight-grads onto the side stream (Runner.side_allowed)
        self.side_open = False      # ... and has launches there that no join covers yet
        self.side_keep = []         # what those launches touch, referenced until the join (Runner.side_begin)


def _empty(n, dev, dtype=_F32):
    return torch.empty(n, device=dev, dtype=dtype)


def channels_last(w):
    """The [Cout][3][3][Cin] storage of a conv weight: the parameter itself when it is channels_last, else a copy."""
    return w if w.is_contiguous(memory_format=torch.channels_last) else w.contiguous(memory_format=torch.channels_last)


class Saved(namedtuple("Saved", "y bnp rt kept", defaults=(None, None))):
    """What a conv block keeps for its backward pass: y (pre-BN), bnp = mean | rstd | scale | shift, the pass's route, what its forward family kept."""
    def pointers(self, ld):
        """(y, scale, shift, mean, rstd) pointers, as the BatchNorm-backward entry points take them; ld: the pitch of the bnp vectors."""
        pb = self.bnp.data_ptr()
        return self.y.data_ptr(), pb + 8 * ld, pb + 12 * ld, pb, pb + 4 * ld


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
# CVK_WGRAD_SIDE: "1" runs the fp32 weight-grads on the library's side stream beside the next block's passes, "0" keeps the single-stream order
WGRAD_SIDE_DEFAULT = "1"
# ... for the weight-grad families (route.ConvRoute.wgrad) measured to gain from it together (the plane GEMM, the transposed 2-D GEMM,
# the thin stem / head kernels); the families nobody measured (w4, w2, direct, the split-operand GEMMs) stay on the pass's stream
WGRAD_SIDE_FAMILIES = frozenset(("wgradp", "wgradp_sm", "w2d", "thin"))


def amax_blocks(lib, n, dev):
    """n zeroed "amax blocks" (csrc/cvk_common.h: the largest magnitude of a tensor in device memory, a few slots one cache line apart): a list of
    int32 views, one fill for all of them."""
    nw = lib.cvk_amax_block_words()
    t = torch.zeros(n * nw, device=dev, dtype=torch.int32)
    return [t[i * nw:(i + 1) * nw] for i in range(n)]


# ---- derived-weight cache ---------------------------------------------------------------------------------------------
# Winograd-domain filters, data-grad packs and bf16 copies are functions of the conv weights only; a step used to rebuild
# all of them (~55 launches, 0.5 ms, also in eval mode).  They are now kept per layer and rebuilt when the weights may have
# changed.  A raw-pointer optimizer or a `p.data` write does not touch the parameter's version counter, so validity is
# explicit: an entry is valid while (global optimizer epoch, runner epoch, storage pointer, tensor version) are unchanged.
#   * any torch.optim optimizer step      -> global epoch (torch.optim.optimizer.register_optimizer_step_post_hook)
#   * FlatAdamW.step, FlatAdamW.swap_ema (entry and exit), load_state_dict, ddp.DataParallel's broadcast, mark_weights_dirty(net) -> runner epoch
#   * .to() / .cuda() / in-place autograd-visible ops -> storage pointer / version counter
# FAIL-SAFE in training: a TRAINING pass (forward with a backward to follow) never trusts entries of earlier passes — its
# signature carries a per-pass token, so the tensors are built once per pass (one batched launch in bf16 mode) and shared by that
# pass's forward and backward only.  Writes nobody can see (`p.data.copy_()` of a hand-written EMA swap, manual re-initialisation, a foreign
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
                py, *pbn = st.saved[prod.idx].pointers(v.C)
                part = _empty(2 * PBp * v.C, X.device)
                rc = _timed(R, "k_pool_bwd_bf16(+bnred)", (2.0 * 0.25 + 2.0 + (4.0 if acc else 2.0) + 2.0) * v.buf.N * v.H * v.W * v.C,
                            lambda: R.lib.cvk_maxpool2x2_bwd_bnred_bf16(
                                st.grad[d.id].data_ptr(), v.hview(X), v.hview(st.grad[v.buf.id]), 1 if acc else 0, v.buf.N, v.H, v.W, v.C,
                                py, v.C, *pbn, part.data_ptr(), st.stream), "byte")
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
                ldp = pad4(prod.cout)
                py, *pbn = st.saved[prod.idx].pointers(ldp)
                part = _empty(2 * PBp * v.C, X.device)
                rc = _timed(R, "k_pool_scatter(bwd+bnred)", (1.0 + (0.25 if code is not None else 4.0) + (8.0 if acc else 4.0) + 4.0) * v.buf.N * v.H * v.W * v.C,
                            lambda: R.lib.cvk_maxpool2x2_bwd_bnred(
                                st.grad[d.id].data_ptr(), v.cview(X), code.data_ptr() if code is not None else None, v.cview(st.grad[v.buf.id]),
                                1 if acc else 0, v.buf.N, v.H, v.W, v.C, py, ldp, *pbn, part.data_ptr(), st.stream), "byte")
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
        op = self.add((ConvBnReluBf16 if self.bf16 else ConvBnRelu)(src_buf, dst_view, pslot, holder, cin, cout, needs, bn.training, req))
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
        # fp32 weight-grads on the library's side stream, beside the next block's bandwidth-bound passes (csrc/side.cpp): the weight-grad
        # families (route.ConvRoute.wgrad) that gained in the probe (tools/bench_wgrad_side.py); the others stay on the pass's stream
        self.wgrad_side = os.environ.get("CVK_WGRAD_SIDE", WGRAD_SIDE_DEFAULT) != "0"
        self.side_families = WGRAD_SIDE_FAMILIES

    def side_allowed(self, fold):
        """This backward pass may fork weight-grads onto the side stream: switched on, and none of the cases that keep the single-stream order:
        a stream capture, a gradient synchroniser attached (its buckets leave in layer order), gradient accumulation, a recording profile."""
        return (self.wgrad_side and not self.bf16 and self.grad_sync is None and self.accumulator is None and fold is None and PROF is None
                and not torch.cuda.is_current_stream_capturing())

    def side_begin(self, st, *keep):
        """Fork: the side stream, ordered behind everything queued on the pass's stream so far.  `keep`: what the side launches read or write;
        referenced until the join, so that the caching allocator cannot hand their blocks to work on the pass's stream meanwhile."""
        s = self.lib.cvk_side_begin(st.stream)
        if not s:
            check(-1, "cvk_side_begin")
        st.side_keep.extend(k for k in keep if k is not None)
        st.side_open = True
        return s

    def side_join(self, st):
        """Join: whatever is queued on the pass's stream from now on runs after the side stream's launches (no-op when nothing was forked)."""
        if st.side_open:
            check(self.lib.cvk_side_join(st.stream), "cvk_side_join")
            st.side_open = False
            st.side_keep.clear()

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
        return self._cache(key, src, build)

    def _cache(self, key, src, build=None):
        """The entry `key` while built from the present state of parameter `src` (cache notes above); else build() becomes it (None without)."""
        sig = (WEIGHT_EPOCH[0], self.wepoch, src.data_ptr(), src._version, self._pass_token)
        ent = self._wc.get(key)
        if (ent is None or ent[0] != sig) and build is not None:
            ent = self._wc[key] = (sig, build())
            self.wcache_builds += 1
        return ent[1] if ent is not None and ent[0] == sig else None

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
            if self._cache(key, src) is not None:
                continue
            t = self._cache(key, src, lambda: _empty(floats, src.device))
            fam_jobs[fam].append((_lib.WtJob(src.data_ptr(), t.data_ptr(), rows, cols, tile, dgrad), 4.0 * (src.numel() + floats)))
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
            for key, dgrad, rows, kpad in op.packs_wanted(self, need_grad):
                if self._cache(key, w) is not None:
                    continue
                wc = channels_last(w)
                t = self._cache(key, w, lambda: torch.empty(lib.cvk_bf16s_rows_pad(rows) * 9 * kpad, device=w.device, dtype=_BF16))
                jobs.append(_lib.PackJob(wc.data_ptr(), t.data_ptr(), op.cout, op.cin, kpad, dgrad))
                keep.append(wc)
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
    def import_nchw(self, st, x, buf, dtype, zero_pad=False):
        """The NCHW tensor x as the NHWC tensor of `buf`: x itself when fp32 and dense NHWC already, else a copy (zero_pad: padding channels 0)."""
        xp = x.permute(0, 2, 3, 1)
        if dtype == _F32 and buf.ld == buf.C and xp.is_contiguous():
            return xp
        t = (torch.zeros if zero_pad and buf.ld != buf.C else torch.empty)((buf.N, buf.H, buf.W, buf.ld), device=x.device, dtype=dtype)
        fn = "cvk_import_nchw_bf16" if dtype == _BF16 else "cvk_import_nchw"
        check(getattr(self.lib, fn)(x.data_ptr(), *x.stride(), t.data_ptr(), buf.ld, buf.N, buf.C, buf.H, buf.W, st.stream), fn)
        return t

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
        st.act[plan.input.id] = self.import_nchw(st, x, plan.input, _BF16 if plan.bf16 else _F32)
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
        st.goffs, total = layout_grads(params)
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
        st.side = self.side_allowed(fold)
        st.grad[plan.output.buf.id] = self.import_nchw(st, gout, plan.output.buf, _F32, zero_pad=True)
        try:
            for op in reversed(plan.ops):
                _CUR_OP[0] = (op.idx, "bwd")
                op.bwd(self, st)
        finally:
            _CUR_OP[0] = None
            # the last blocks' weight-grads: before anything reads the flat gradient buffer — and, when an op raised, before the pass's
            # tensors are released while side-stream kernels may still read them
            self.side_join(st)
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


from .conv_fp32 import ConvBnRelu, conv_kernel_name  # noqa: E402,F401  (below what they import from here; engine.<name> stays importable)
from .conv_bf16 import ConvBnReluBf16  # noqa: E402
