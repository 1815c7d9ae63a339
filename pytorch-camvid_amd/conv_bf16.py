"""The bf16-storage conv block (BASELINE.json configs[3]; csrc/conv_bf16s.hip, csrc/thin_bf16.hip, csrc/elem_bf16.hip), created by Plan.conv_bn_relu
for bf16 plans: ConvBnRelu's passes (conv_fp32.py) with the stages that differ in entry points, element sizes and pitches."""
import torch

from ._lib import check
from .conv_fp32 import ConvBnRelu
from .engine import _BF16, _F32, _empty, _timed, channels_last


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


class ConvBnReluBf16(ConvBnRelu):
    """bf16 NHWC activations in HBM: conv (bf16 MFMA, fp32 accumulate, fp32 statistics from the accumulators) writes
    the pre-BN tensor y as bf16; ONE elementwise pass applies BN + ReLU, writes the bf16 activation through the
    (concat) view and, for encoder stages, the 2x2 max-pooled tensor as well."""
    _pitch, _ydt = staticmethod(int), _BF16
    _BN = ("cvk_bn_bwd_blocks_bf16", "cvk_bn_bwd_reduce_bf16", "k_bnbwd_bf16<reduce>")

    def thin_mode(self, R, dgrad, ld_dy=0):
        """csrc/thin_bf16.hip mode of this layer's forward (dgrad=False) / data-grad launch, 0 = the general kernels (also with CVK_THIN=0)."""
        if not R.thin or self.src.H * self.src.W * max(self.src.ld, self.cout, ld_dy, 64) * 2 >= 2 ** 31:
            return 0
        if dgrad:
            return R.lib.cvk_thin_bf16_mode(self.cin, self.cout, ld_dy, self.src.ld, 1) if self.src.ld == 64 and self.cin == 64 else 0
        return R.lib.cvk_thin_bf16_mode(self.cin, self.cout, self.src.ld, self.cout, 0)

    def packs_wanted(self, R, need_grad):
        """[(cache key, dgrad, rows, K pitch)] of the general kernels' filter packs a pass over this layer asks for (Runner.prepack_bf16)."""
        want = []
        if not self.thin_mode(R, False):        # thin layers pack their own (tiny) filter formats where they run
            want.append((((self.pslot, "f"), "bf16"), 0, self.cout, self.src.ld))
        if need_grad and self.src_needs_grad and not self.thin_mode(R, True, max(32, self.cout)):
            want.append((((self.pslot, "d"), "bf16"), 1, self.cin, max(32, self.cout)))
        return want

    def _pack(self, R, st, w, side, mode, kpad):
        """The cached bf16 filter of the forward ("f") or data-grad ("d") launch: the thin kernels' format `mode`, or (0) the general pack."""
        lib, s, dev, wc = R.lib, st.stream, st.device, channels_last(w)

        def build_thin():
            t = torch.empty(lib.cvk_thin_bf16_pack_elems(mode), device=dev, dtype=_BF16)
            check(lib.cvk_pack_weight_thin_bf16(wc.data_ptr(), t.data_ptr(), self.cout, self.cin, mode, s), "cvk_pack_weight_thin_bf16")
            return t

        def build():
            fn = "cvk_pack_weight_%s_bf16" % ("fwd" if side == "f" else "dgrad")
            t = torch.empty(lib.cvk_bf16s_rows_pad(self.cout if side == "f" else self.cin) * 9 * kpad, device=dev, dtype=_BF16)
            check(getattr(lib, fn)(wc.data_ptr(), t.data_ptr(), self.cout, self.cin, kpad, s), fn)
            return t
        return R.derived(((self.pslot, side), "thinb"), w, build_thin) if mode else R.derived(((self.pslot, side), "bf16"), w, build)

    def _weight_fwd(self, R, st, w):
        """(thin mode, filter pack): the stem (3 -> 64) and the head (64 -> 12) run the register-only thin kernels (csrc/thin_bf16.hip, round 5)."""
        if self.cout % 4:
            raise NotImplementedError("bf16 mode needs output channel counts that are multiples of 4")
        tmode = self.thin_mode(R, False)
        return tmode, self._pack(R, st, w, "f", tmode, self.src.ld)

    def _stat_partials(self, R, wk):
        src = self.src
        P = R.lib.cvk_thin_bf16_stat_partials(src.N, src.H, src.W) if wk[0] else R.lib.cvk_bf16s_stat_partials_c(src.N, src.H, src.W, src.ld, self.cout)
        return P, P

    def _conv(self, R, st, rt, X, wk, b, y, stats, P):
        """y = conv3x3(X, wb) + b as bf16 (+ BN statistics partials with pixel counts when stats is given)."""
        lib, s, src, C, (tmode, wb) = R.lib, st.stream, self.src, self.cout, wk
        N, H, W, M = src.N, src.H, src.W, src.M
        flops = 18.0 * M * C * self.cin
        sp = stats.data_ptr() if stats is not None else None
        cnt = sp + 4 * 2 * P * C if stats is not None else None
        if tmode:
            _timed(R, {1: "k_thinb_head_fwd", 2: "k_thinb_wide<1>"}.get(tmode), flops, lambda: check(
                lib.cvk_conv3x3_thin_bf16(X.data_ptr(), wb.data_ptr(), b.data_ptr(), y.data_ptr(), sp, cnt, N, H, W, src.ld, C, C,
                                          tmode, s), "cvk_conv3x3_thin_bf16"), nbytes=2.0 * M * (src.ld + C))
        elif stats is not None:
            _timed(R, bf16_kernel_name(lib, N, H, W, src.ld, C, True), flops, lambda: check(
                lib.cvk_conv3x3_bf16s_wg(X.data_ptr(), wb.data_ptr(), b.data_ptr(), y.data_ptr(), sp, cnt, N, H, W, src.ld, C, C,
                                         R.launch_wgs(), s), "cvk_conv3x3_bf16s"))
        else:
            _timed(R, bf16_kernel_name(lib, N, H, W, src.ld, C, False), flops, lambda: check(
                lib.cvk_conv3x3_bf16s(X.data_ptr(), wb.data_ptr(), b.data_ptr(), y.data_ptr(), None, None, N, H, W, src.ld, C, C, s), "cvk_conv3x3_bf16s"))
        return ((P, cnt) if stats is not None else None), None

    def _bn_apply(self, R, st, y, psc, psh):
        src, dst, C = self.src, self.dst, self.cout
        out = R.alloc_act(st, dst.buf, st.device)
        out_f32 = 1 if dst.buf.dtype == _F32 else 0
        pool = R.alloc_act(st, self.pool_dst, st.device) if self.pool_dst is not None else None
        nbytes = (2.0 + (4.0 if out_f32 else 2.0)) * src.M * C + (0.5 * src.M * C if pool is not None else 0.0)
        _timed(R, "k_apply_bf16" + ("<pool>" if pool is not None else ""), nbytes, lambda: check(
            R.lib.cvk_bn_relu_apply_bf16(y.data_ptr(), C, psc, psh, dst.hview(out), out_f32, pool.data_ptr() if pool is not None else None,
                                         src.N, src.H, src.W, C, st.stream), "cvk_bn_relu_apply_bf16"), "byte")

    def _dout(self, st):
        return self.dst.hview(st.grad[self.dst.buf.id]), 1 if self.dst.buf.dtype == _F32 else 0

    def _bn_bwd(self, R, st, rt, bn, gg, gbe, part, PB, gb):
        """Stage 2: BatchNorm + ReLU backward: dy (bf16, pitch max(32, C): the data-grad GEMM reads dy in 32-channel K slices) from dO."""
        src, C, ld_dy = self.src, self.cout, max(32, self.cout)
        dy = torch.empty(src.M * ld_dy, device=st.device, dtype=_BF16)
        _timed(R, "k_bnbwd_bf16<dx>", ((4.0 if bn[1] else 2.0) + 4.0) * src.M * C, lambda: check(
            R.lib.cvk_bn_bwd_dx_bf16(*bn, gg, gbe, dy.data_ptr(), ld_dy, part.data_ptr(),
                                     src.N, src.H, src.W, C, 1 if self.bn_train else 0, st.stream), "cvk_bn_bwd_dx_bf16"), "byte")
        if gb is not None:
            R.defer_colsum(st, part, PB, C, gb)         # conv bias grad: finalised with the others, in one launch
        return dy, None, None

    def _data_grad(self, R, st, rt, dy, Vb, am_dy):
        lib, s, src, C, ld_dy = R.lib, st.stream, self.src, self.cout, max(32, self.cout)
        N, H, W, M = src.N, src.H, src.W, src.M
        flops = 18.0 * M * C * self.cin
        if src.id in st.grad:
            raise NotImplementedError("conv data-grad must be the first writer of its input's gradient buffer")
        dmode = self.thin_mode(R, True, ld_dy)
        dX = torch.empty((N, H, W, src.ld), device=st.device, dtype=_BF16)
        wd = self._pack(R, st, st.params[4 * self.pslot], "d", dmode, ld_dy)
        if dmode:
            _timed(R, "k_thinb_wide<3>(dgrad)", flops, lambda: check(
                lib.cvk_conv3x3_thin_bf16(dy.data_ptr(), wd.data_ptr(), None, dX.data_ptr(), None, None, N, H, W, ld_dy, C, src.ld, dmode, s),
                "cvk_conv3x3_thin_bf16(dgrad)"), nbytes=2.0 * M * (ld_dy + src.ld))
        else:
            _timed(R, bf16_kernel_name(lib, N, H, W, ld_dy, self.cin, False), flops, lambda: check(
                lib.cvk_conv3x3_bf16s_wg(dy.data_ptr(), wd.data_ptr(), None, dX.data_ptr(), None, None, N, H, W, ld_dy, self.cin, src.ld,
                                         R.launch_wgs(), s), "cvk_conv3x3_bf16s(dgrad)"))
        st.grad[src.id] = dX

    def _weight_grad(self, R, st, saved, dy, gw, E, Eb, am_dy):
        # partial slabs now, the sum over the slabs with every other layer's in ONE launch (Runner.flush_wreduces): nobody reads a weight
        # gradient before the end of backward (or the all-reduce of its bucket); 23 reductions of ~11 us were 0.26 ms of a 21 ms step
        lib, src, C = R.lib, self.src, self.cout
        N, H, W = src.N, src.H, src.W
        S = lib.cvk_conv3x3_wgrad_bf16s_splits(N, H, W, self.cin, C)
        n = C * 9 * self.cin
        slab = None if S == 1 else _empty(S * n, st.device)           # one slab: it is the gradient itself, written in place
        _timed(R, "k_wgrad_bf16r", 18.0 * src.M * C * self.cin, lambda: check(
            lib.cvk_conv3x3_wgrad_bf16s_slabs(st.act[src.id].data_ptr(), dy.data_ptr(), gw if slab is None else slab.data_ptr(), N, H, W, self.cin,
                                              src.ld, C, max(32, C), 4 * S * n, st.stream), "cvk_conv3x3_wgrad_bf16s_slabs"))
        if slab is not None:
            R.defer_wreduce(st, slab, S, n, gw)
