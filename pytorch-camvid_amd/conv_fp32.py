"""The conv block ConvBnRelu, its passes as lists of stages (plain values in and out: ops are shared across passes), and the launchers of what its
route names (route.ConvRoute): WinoConv for the forward and data-grad families, WeightGrad for the weight-grad families."""
import torch

from . import _lib
from ._lib import check
from .engine import _BF16, _F32, Op, Saved, _empty, _timed, amax_blocks, channels_last
from .route import pad4


def w2fn(lib, tile, name):
    """Entry point `name` of the 2-D Winograd family for output tile `tile`: cvk_w2d_<name> (4) or cvk_w6_<name> (6)."""
    return getattr(lib, ("cvk_w6_" if tile == 6 else "cvk_w2d_") + name)


_PLANE_DT = {0: _F32, 2: torch.float16, 3: _BF16}       # element type of the 2-D path's planes by split format (0: plain fp32 planes)


def planes2d(lib, tile, N, H, W, fmt=0):
    """(NX, T, Tp) of the 2-D path's transform-domain planes: NX planes per channel, T tiles, T padded to the row tile of the format's GEMM."""
    T = w2fn(lib, tile, "tiles")(N, H, W)
    return 64 if tile == 6 else 36, T, lib.cvk_split3_rows_pad(T, 256) if fmt else lib.cvk_w2d_tpad(T)


def plane_elems(NX, Tp, C, fmt=0):
    """Elements of a C-channel tensor's planes: fp32 with 512 bytes of slack, or (fmt = 2 | 3) fmt 16-bit terms in 32-channel slices."""
    return NX * (C // 32) * fmt * Tp * 32 if fmt else NX * Tp * C + 128


def absmax(R, t, rows, cols, ld, s, what):
    """A new amax block holding the largest magnitude of t[rows][cols] (pitch ld), measured by its own pass."""
    a = amax_blocks(R.lib, 1, t.device)[0]
    _timed(R, "k_absmax", 4.0 * rows * cols, lambda: check(R.lib.cvk_absmax_f32(t.data_ptr(), rows, cols, ld, a.data_ptr(), s), "cvk_absmax_f32(%s)" % what), "byte")
    return a


def amax_call(lib, name, args, blocks, s):
    """`name`(*args, s), or when a block is wanted its twin `name`_amax(*args, *block pointers, s), which leaves the largest magnitude written there."""
    if blocks.count(None) == len(blocks):
        return getattr(lib, name)(*args, s)
    return getattr(lib, name + "_amax")(*args, *(b.data_ptr() if b is not None else None for b in blocks), s)


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
        NX, T, Tp = planes2d(lib, tile, N, H, W)

        dg = d is not None and d[1] == k_ch and d[2] == cout          # data-grad without channel padding: straight from the forward weights
        rows, cols = (d[1], d[2]) if dg else (cout, k_ch)

        def build():
            u, wt = _empty(NX * cout * k_ch, x.device), d[0] if dg else (self.w() if callable(self.w) else self.w)
            kind = "weight_transform_dgrad" if dg else "weight_transform"
            _timed(R, "k_w2d_weight_dgrad" if dg else "k_w2d_weight", 4.0 * (9 + NX) * cout * k_ch, lambda: check(
                w2fn(lib, tile, kind)(wt.data_ptr(), u.data_ptr(), rows, cols, s), "cvk_w2d_" + kind), "byte")
            return u
        U = self._filter("w2d%d" % tile, build, ("w2d", NX * cout * k_ch, rows, cols, tile, int(d is not None)))
        vfl = plane_elems(NX, Tp, k_ch)          # V planes + 512 bytes of slack
        if keep:        # the weight-grad of this layer reuses V: its own tensor instead of the shared workspace
            self.v = _empty(vfl, x.device)
        Vt = v_pre if v_pre is not None else self.v
        wsb = (lib.cvk_conv3x3_w6_workspace_bytes if tile == 6 else lib.cvk_conv3x3_w2d_workspace_bytes)(N, H, W, k_ch, cout)
        ws = R.workspace(wsb - (4 * vfl if Vt is not None else 0), x.device)
        V, Mo = (Vt.data_ptr(), ws.data_ptr()) if Vt is not None else (ws.data_ptr(), ws.data_ptr() + 4 * vfl)
        P2 = w2fn(lib, tile, "stat_partials")(N, H, W)
        cnt = self._counts(P2)
        if v_pre is None:
            _timed(R, "k_w2d_input", 4.0 * (M + NX * T) * k_ch, lambda: check(
                w2fn(lib, tile, "input_transform")(x.data_ptr(), V, N, H, W, k_ch, s), "cvk_w2d_input_transform" + self.what), "byte")
        _timed(R, "k_w2d_gemm<128, 32, 2, 2>", self.flops, lambda: check(w2fn(lib, tile, "gemm")(V, U.data_ptr(), Mo, T, k_ch, cout, s), "cvk_w2d_gemm" + self.what),
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
        (NX, T, Tp), pdt = planes2d(lib, tile, N, H, W, fmt), _PLANE_DT[fmt]
        tag = "split3" if fmt == 3 else "split2h"
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
            V3 = torch.empty(plane_elems(NX, Tp, k_ch, fmt), device=x.device, dtype=pdt)
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
            u, name = _empty(floats, x.device), "cvk_wino4%s_weight_transform" % f
            _timed(R, "k_wino4%s_weight" % f, 4.0 * (9 + 18) * cout * k_ch, lambda: check(getattr(lib, name)(
                wt.data_ptr(), u.data_ptr(), *((am_w.data_ptr(),) if h2 else ()), cout, k_ch, dg, s), name + ("(dgrad)" if dg and not h2 else "")), "byte")
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
                x.data_ptr(), U.data_ptr(), self.y.data_ptr(), *am, N, H, W, k_ch, cout, ldy, *bnred, bpart.data_ptr(), R.launch_wgs(), s), name), executed=executed)
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


class WeightGrad:
    """dW[cout][3][3][cin] at gw from x[N,H,W,k_ch] and dy[N,H,W,ldy] through the weight-grad family the route names.  From earlier stages: V, am_v:
    the input transform the forward pass kept (and its amax block); E: the BatchNorm-backward pass's planes (dy_e: four of them, E0 / E5 are
    columns of dy); Eb: dy's 2-D planes from the transform shared with the data-grad; am_dy: the amax block of dy."""

    def __init__(self, R, s, x, dy, gw, N, H, W, cin, k_ch, cout, ldy, flops):
        self.R, self.lib, self.s, self.x, self.dy, self.gw = R, R.lib, s, x, dy, gw
        self.keep = []      # tensors made here that the launches still read after run() has returned (s may be the side stream)
        self.N, self.H, self.W, self.M, self.cin, self.k_ch, self.cout, self.ldy, self.flops = N, H, W, N * H * W, cin, k_ch, cout, ldy, flops

    def run(self, fam, tile=0, fmt=0, V=None, am_v=None, E=None, dy_e=False, Eb=None, am_dy=None):
        if fam == "w2d":
            return self.w2d(tile, V, Eb)
        if fam == "w2d_split":
            return self.w2d_split(tile, fmt, V, am_v, Eb, am_dy)
        if fam in ("wgradp", "wgradp_sm"):
            return self.wgradp(fam == "wgradp", V, E, dy_e and E is not None)
        return self.w4(E) if fam == "w4" else self.direct(fam)

    def w2d(self, tile, V, Eb):
        """Transposed 2-D F(4x4,3x3) / F(6x6,3x3) (csrc/wino2d.hip)."""
        R, lib, s, x, dy = self.R, self.lib, self.s, self.x, self.dy
        N, H, W, M, k_ch, C, ldy = self.N, self.H, self.W, self.M, self.k_ch, self.cout, self.ldy
        NX, T, Tp = planes2d(lib, tile, N, H, W)
        efl = plane_elems(NX, Tp, C)
        f = w2fn(lib, tile, "wgrad_ksplit")(T, k_ch, C)
        if V is None:           # the forward pass ran another family: transform x now
            V = _empty(plane_elems(NX, Tp, k_ch), x.device)
            self.keep.append(V)
            _timed(R, "k_w2d_input", 4.0 * (M + NX * T) * k_ch, lambda: check(
                w2fn(lib, tile, "input_transform")(x.data_ptr(), V.data_ptr(), N, H, W, k_ch, s), "cvk_w2d_input_transform(wgrad)"), "byte")
        ws = R.workspace(4 * ((0 if Eb is not None else efl) + f * NX * C * k_ch), x.device)
        Ep, Pp = (Eb.data_ptr(), ws.data_ptr()) if Eb is not None else (ws.data_ptr(), ws.data_ptr() + 4 * efl)
        if Eb is None:          # else E came with the data-grad's V'
            _timed(R, "k_w2d_dy", 4.0 * (M + NX * T) * C, lambda: check(
                w2fn(lib, tile, "dy_transform")(dy.data_ptr(), ldy, Ep, N, H, W, C, s), "cvk_w2d_dy_transform"), "byte")
        _timed(R, "k_w2d_gemm_tn", self.flops, lambda: check(
            w2fn(lib, tile, "gemm_tn")(Ep, V.data_ptr(), Pp, T, k_ch, C, s), "cvk_w2d_gemm_tn"), executed=2.0 * NX * Tp * k_ch * C)
        _timed(R, "k_w2d_wgrad_out", 4.0 * (NX * f + 9) * C * self.cin, lambda: check(
            w2fn(lib, tile, "wgrad_output")(Pp, self.gw, T, self.cin, k_ch, C, s), "cvk_w2d_wgrad_output"), "byte")

    def w2d_split(self, tile, fmt, V, am_v, Eb, am_dy):
        """The transposed 2-D GEMMs on split planes (WinoConv.w2d_split): V from the forward transform, E from the pass over dy."""
        R, lib, s, k_ch, C = self.R, self.lib, self.s, self.k_ch, self.cout
        NX, _, Tp = planes2d(lib, tile, self.N, self.H, self.W, fmt)
        f = lib.cvk_w2d_gemm_tn_split3_ksplit(NX, Tp, k_ch, C)
        ws = R.workspace(4 * f * NX * C * k_ch, self.x.device)
        _timed(R, "k_gemm_tn_" + ("split3" if fmt == 3 else "split2h"), self.flops, lambda: check(
            lib.cvk_w2d_gemm_tn_split(fmt, tile, Eb.data_ptr(), V.data_ptr(), ws.data_ptr(), am_dy.data_ptr() if am_dy is not None else None,
                                      am_v.data_ptr() if am_v is not None else None, NX, Tp, k_ch, C, s), "cvk_w2d_gemm_tn_split"),
            executed=2.0 * (6 if fmt == 3 else 3) * NX * Tp * k_ch * C)
        _timed(R, "k_w2d_wgrad_out", 4.0 * (NX * f + 9) * C * self.cin, lambda: check(
            lib.cvk_w2d_wgrad_output_f(tile, ws.data_ptr(), self.gw, self.cin, k_ch, C, f, s), "cvk_w2d_wgrad_output_f"), "byte")

    def wgradp(self, own_v, V, E, sm_dy):
        """Transposed F(4,3) through transform-domain planes (csrc/wgradp.hip): V from the forward launch (slice-major) or, own_v, from a pass
        over x; E from the BatchNorm-backward pass, or from a pass over dy when that one fell back.  sm_dy: E0 / E5 read from dy."""
        R, lib, s, x, dy = self.R, self.lib, self.s, self.x, self.dy
        N, H, W, M, k_ch, C, ldy = self.N, self.H, self.W, self.M, self.k_ch, self.cout, self.ldy
        rows6 = lib.cvk_wgradp_plane_rows(N, H, W)
        wsb = lib.cvk_wgradp_gemm_workspace_bytes(N, H, W, k_ch, C)
        nE = 0 if E is not None else 6 * rows6 * C
        nV = 6 * rows6 * k_ch if own_v else 0
        ws = R.workspace(4 * (nV + nE) + wsb, x.device)
        V6p = ws.data_ptr() if own_v else V.data_ptr()
        E6p = E.data_ptr() if E is not None else ws.data_ptr() + 4 * nV
        slabp = ws.data_ptr() + 4 * (nV + nE)
        if own_v:
            _timed(R, "k_wgradp_planes", 4.0 * (M + 6.0 * rows6) * k_ch, lambda: check(
                lib.cvk_wgradp_planes(x.data_ptr(), k_ch, V6p, N, H, W, k_ch, 0, s), "cvk_wgradp_planes(x)"), "byte")
        if E is None:
            _timed(R, "k_wgradp_planes", 4.0 * (M + 6.0 * rows6) * C, lambda: check(
                lib.cvk_wgradp_planes(dy.data_ptr(), ldy, E6p, N, H, W, C, 1, s), "cvk_wgradp_planes(dy)"), "byte")
        fn = "cvk_wgradp_gemm_sm_dy" if sm_dy else ("cvk_wgradp_gemm" if own_v else "cvk_wgradp_gemm_sm")
        ev = (E6p, dy.data_ptr(), V6p) if sm_dy else (E6p, V6p)
        _timed(R, "k_wgradp_gemm", self.flops, lambda: check(getattr(lib, fn)(*ev, self.gw, N, H, W, self.cin, k_ch, C, slabp, wsb, s), fn),
               executed=9.0 * M * C * self.cin)

    def w4(self, E):
        """Transposed F(4,3): fastest weight-grad on every layer with >= 64 input channels (tools/bench_conv.py wgrad wwino wwino4)."""
        R, lib, N, H, W, k_ch, C, ldy = self.R, self.lib, self.N, self.H, self.W, self.k_ch, self.cout, self.ldy
        wsb = lib.cvk_conv3x3_wgrad_wino4_workspace_bytes(N, H, W, k_ch, C, ldy)
        ws = R.workspace(wsb, self.x.device)
        _timed(R, f"k_wgrad_wino4<{'128' if C > 64 else '64'}, 128, 2, 2>", self.flops, lambda: check(
            lib.cvk_conv3x3_wgrad_wino4(self.x.data_ptr(), self.dy.data_ptr(), E.data_ptr() if E is not None else None, self.gw, N, H, W,
                                        self.cin, k_ch, C, ldy, ws.data_ptr(), wsb, self.s), "cvk_conv3x3_wgrad_wino4"))

    def direct(self, fam):
        """thin (the stem, the head: csrc/thin.hip), F(2,3) ("w2") or the direct kernel: one entry-point signature."""
        R, lib, N, H, W, M, k_ch, C, ldy = self.R, self.lib, self.N, self.H, self.W, self.M, self.k_ch, self.cout, self.ldy
        fn = {"thin": "cvk_conv3x3_thin_wgrad", "w2": "cvk_conv3x3_wgrad_wino", "direct": "cvk_conv3x3_wgrad"}[fam]
        wsb = getattr(lib, fn + "_workspace_bytes")(N, H, W, k_ch, C)
        ws = R.workspace(wsb, self.x.device)
        head = k_ch == 64
        name, kw = {"thin": ("k_thin_co_wgrad" if head else "k_thin_ci_wgrad",
                             dict(executed=18.0 * M * (16 * self.cin if head else C * 16 / 3.0), nbytes=4.0 * M * (k_ch + ldy))),
                    "w2": (f"k_wgrad_wino<{'128' if C > 64 else '64'}, 128, 2, 2>", {}), "direct": (conv_kernel_name("wgrad", C, k_ch), {})}[fam]
        _timed(R, name, self.flops, lambda: check(getattr(lib, fn)(
            self.x.data_ptr(), self.dy.data_ptr(), self.gw, N, H, W, self.cin, k_ch, C, ldy, ws.data_ptr(), wsb, self.s), fn), **kw)


def conv_kernel_name(kind, n_cols, k_ch=32):
    """Mirror of the tile dispatch in csrc/conv3x3.hip / wino.hip: the kernel-trace name."""
    if kind in ("wino4", "wino"):
        return "k_conv3x3_%s<%s>" % (kind, "128, 128, 2, 2" if n_cols > 64 else ("128, 64, 2, 2" if n_cols > 32 else "128, 32, 4, 1"))
    if kind == "wgrad":
        if n_cols <= 16 and k_ch == 64:
            return "k_wgrad_smallco"
        t = "128, 128, 2, 2" if n_cols > 64 else ("64, 128, 2, 2" if n_cols > 32 else "32, 256, 1, 4")
        if 32 < n_cols <= 64 and k_ch * 9 <= 64:
            t = "64, 64, 2, 2"
        return f"k_conv3x3_wgrad<{t}>"
    t = "128, 128, 2, 2" if n_cols > 64 else ("128, 64, 2, 2" if n_cols > 32 else "256, 32, 4, 1")
    return f"k_conv3x3_igemm<{t}, {'true' if kind == 'fwd' else 'false'}, {'true' if k_ch % 32 == 0 else 'false'}>"


class ConvBnRelu(Op):
    """ReLU(BN(conv3x3(x)+b)) — reference BasicConv2d (models/unet.py:5-17) / BasicConv (models/segnet.py:5-17)."""
    _pitch, _ydt = staticmethod(pad4), _F32         # pitch (from the channel count) and type of the pre-BN tensor y; the BatchNorm vectors share the pitch
    _BN = ("cvk_bn_bwd_blocks", "cvk_bn_bwd_reduce", "k_bn_bwd<reduce>")        # BatchNorm backward: partial-block count, reduce pass, its trace name

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
        ldx, wc = self.src.ld, channels_last(w)
        if ldx == self.cin and wc is w:
            return w
        def build():
            out = _empty(self.cout * 9 * ldx, w.device)
            check(R.lib.cvk_pack_weight_fwd(wc.data_ptr(), out.data_ptr(), self.cout, self.cin, ldx, st.stream), "cvk_pack_weight_fwd")
            return out
        return R.derived(((self.pslot, "f"), "pack"), w, build)

    def _stat_partials(self, R, wk):
        """(P, Pw): the conv's plain statistics partials, and the partial count the buffer is sized for: room for any partial layout (+ counts)."""
        lib, src = R.lib, self.src
        P = (src.M + _lib.CVK_STAT_ROWS - 1) // _lib.CVK_STAT_ROWS
        return P, max(P, lib.cvk_w2d_stat_partials(src.N, src.H, src.W), lib.cvk_w6_stat_partials(src.N, src.H, src.W),
                      lib.cvk_thin_stat_partials(src.N, src.H, src.W, src.ld))

    def _conv(self, R, st, rt, X, wk, b, y, stats, P):
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
                lib.cvk_conv3x3_fwd(X.data_ptr(), wk.data_ptr(), b.data_ptr(), y.data_ptr(), sp, N, H, W, src.ld, C, ldy, s), "cvk_conv3x3_fwd"))
            return None, None
        c = WinoConv(R, s, X, wk, b.data_ptr(), y, sp, N, H, W, src.ld, C, ldy, flops, st.params[4 * self.pslot], (self.pslot, "f"))
        counted = c.run(rt.fwd, rt.tile, rt.split, keep=rt.keeps_v, x_amax=st.amax.get(src.id))
        return counted, ((c.v, c.v_amax) if rt.keeps_v else None)

    def _bn_params(self, R, st, stats, counted, P, Pw, gamma, beta, ptrs):
        """mean | rstd | scale | shift at ptrs: from the running statistics (stats None: eval mode), else from the conv's partials, updating the running
        statistics: P plain partials, or counted = (count, pointer) with pixel counts.  Pw: the partial count the finalize workspace is sized for."""
        lib, C, bn = R.lib, self.cout, self.holder.conv_bn()[1]
        if stats is None:
            return check(lib.cvk_bn_eval_params(gamma.data_ptr(), beta.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(), *ptrs, C,
                                                float(bn.eps), st.stream), "cvk_bn_eval_params")
        wsb = lib.cvk_bn_finalize_workspace_bytes(Pw, C)
        ws = R.workspace(wsb, st.device)
        track = bn.track_running_stats and bn.running_mean is not None
        mom = 0.1 if bn.momentum is None else float(bn.momentum)
        tail = (self.src.M, C, gamma.data_ptr(), beta.data_ptr(), *ptrs, bn.running_mean.data_ptr() if track else None,
                bn.running_var.data_ptr() if track else None, bn.num_batches_tracked.data_ptr() if track else None,
                mom, float(bn.eps), ws.data_ptr(), wsb, st.stream)
        if counted is None:
            check(lib.cvk_bn_finalize(stats.data_ptr(), P, *tail), "cvk_bn_finalize")
        else:       # partials with explicit pixel counts (2-D Winograd path: P2 <= P partials in the same buffer)
            check(lib.cvk_bn_finalize_counts(stats.data_ptr(), counted[1], counted[0], *tail), "cvk_bn_finalize_counts")

    def _bn_apply(self, R, st, y, psc, psh):
        """BN + ReLU of y into the block's output view and, in the same pass, the 2x2 max pool behind the block; fills the buffers' amax blocks."""
        lib, s, src, dst = R.lib, st.stream, self.src, self.dst
        N, H, W, M, C, ldy, dev = src.N, src.H, src.W, src.M, self.cout, pad4(self.cout), st.device
        out = R.alloc_act(st, dst.buf, dev)
        pooled = False
        if self.pool_dst is not None and C % 4 == 0:
            # the 2x2 max pool behind this block is written by the same pass (csrc/bn.hip k_bn_relu_apply_pool)
            pool = R.alloc_act(st, self.pool_dst, dev)
            code = torch.empty(self.pool_dst.M * self.pool_dst.ld, device=dev, dtype=torch.uint8) if self.pool_op.keep_code else None
            ap = st.amax.get(self.pool_dst.id)
            rc = _timed(R, "k_bn_relu_apply<pool>", (8.0 + 1.0 + (0.25 if code is not None else 0.0)) * M * C, lambda: amax_call(
                lib, "cvk_bn_relu_apply_pool", (y.data_ptr(), ldy, psc, psh, dst.cview(out), pool.data_ptr(), code.data_ptr() if code is not None else None,
                                                N, H, W, C), (st.amax.get(dst.buf.id), ap), s), "byte")
            pooled = rc == 0
            if not pooled and ap is not None:
                st.amax.pop(self.pool_dst.id)          # the separate pool pass writes that buffer: its reader measures it itself
            if pooled and code is not None:
                st.saved[self.pool_op.idx] = code
        st.pooled_by_block[self.idx] = pooled
        if not pooled:
            _timed(R, "k_bn_relu_apply", 8.0 * M * C, lambda: check(amax_call(
                lib, "cvk_bn_relu_apply", (y.data_ptr(), ldy, psc, psh, dst.cview(out), N, H, W, C), (st.amax.get(dst.buf.id),), s), "cvk_bn_relu_apply"), "byte")

    def fwd(self, R, st):
        src, C, ld, dev = self.src, self.cout, self._pitch(self.cout), st.device
        rt = st.routes[self.idx] if st.routes is not None else None
        w, b, gamma, beta = st.params[4 * self.pslot:4 * self.pslot + 4]
        wk = self._weight_fwd(R, st, w)
        y = torch.empty(src.M * ld, device=dev, dtype=self._ydt)
        bnp = _empty(4 * ld, dev)                      # mean | rstd | scale | shift
        ptrs = tuple(bnp.data_ptr() + 4 * ld * i for i in range(4))
        stats, P, Pw = None, 0, 0
        if self.bn_train:
            if src.M <= 1:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size {[src.N, C, src.H, src.W]}")
            P, Pw = self._stat_partials(R, wk)
            stats = _empty(2 * Pw * C + Pw, dev)
        counted, kept = self._conv(R, st, rt, st.act[src.id], wk, b, y, stats, P)
        self._bn_params(R, st, stats, counted, P, Pw, gamma, beta, ptrs)
        self._bn_apply(R, st, y, ptrs[2], ptrs[3])
        if st.need_grad and self.active:
            st.saved[self.idx] = Saved(y, bnp, rt, kept)

    def _bn_sums(self, R, st, bn, gg, gbe):
        """Stage 1: dgamma and dbeta from the sums the pass that wrote dO left (st.bnred), else from a reduce pass; bn: the BatchNorm-backward entry
        points' leading arguments (bwd).  Returns (partials buffer, block count) for the dx pass; None when only gamma / beta train: no dy needed."""
        lib, s, src, C, (blocks, fn, name) = R.lib, st.stream, self.src, self.cout, self._BN
        PB = getattr(lib, blocks)(src.M)
        part = _empty(2 * PB * C, st.device)
        pre = st.bnred.pop(self.idx, None)
        if pre is not None:     # the pass that wrote dO last summed it already (csrc/wino4f.hip BNR epilogue, the max-pool backward passes)
            check(lib.cvk_colsum_finalize(pre[0].data_ptr(), pre[1], C, gbe, gg, s), "cvk_colsum_finalize")
        elif self.bn_train or self.g_req or self.be_req:        # eval-mode BatchNorm with frozen gamma / beta needs neither sum
            _timed(R, name, float(self.dst.buf.esize + self._ydt.itemsize) * src.M * C, lambda: check(       # dO and y, each read once
                getattr(lib, fn)(*bn, part.data_ptr(), src.N, src.H, src.W, C, s), fn), "byte")
            check(lib.cvk_colsum_finalize(part.data_ptr(), PB, C, gbe, gg, s), "cvk_colsum_finalize")   # dbeta, dgamma
        if self.w_req or self.b_req or self.src_needs_grad:
            return part, PB
        R.grads_ready(st, self.pslot)
        return None

    # BatchNorm-backward passes that also write the weight-grad's transformed dy (route bn_bwd): mode of cvk_bn_bwd_dx_e_amax, the entry point
    # without the amax word, plane bytes written per 4-column group and channel
    _BN_E = {"dx+E": (0, "cvk_bn_bwd_dx_e", 16.0), "dx+E6": (1, "cvk_bn_bwd_dx_e6", 24.0), "dx+E4p": (2, "cvk_bn_bwd_dx_e4p", 16.0)}

    def _bn_bwd(self, R, st, rt, bn, gg, gbe, part, PB, gb):
        """Stage 2: BatchNorm + ReLU backward (csrc/bn.hip): dy from dO and, for rt.bn_bwd != "dx", the weight-grad's E planes in the same pass.
        Returns (dy, planes, amax block of dy if the route wants it); planes None after the plain pass, which also runs when a planes pass refuses
        the layout (rc != 0: a strided view) — the weight-grad then transforms dy itself."""
        lib, s, src, kind = R.lib, st.stream, self.src, rt.bn_bwd
        N, H, W, M, C, ldy = src.N, src.H, src.W, src.M, self.cout, pad4(self.cout)
        if kind == "dx+E4p":
            # the plane GEMM reads E0 / E5 (columns of dy) from dy itself: dy carries a zeroed slack behind its last row (cvk_wgradp_gemm_sm_dy)
            dyb = _empty(M * ldy + lib.cvk_wgradp_dy_slack(W) * ldy, st.device)
            dyb[M * ldy:].zero_()
            dy = dyb[:M * ldy]
        else:
            dy = torch.zeros(M * ldy, device=st.device, dtype=_F32) if ldy != C else _empty(M * ldy, st.device)
        want_amax = rt.dy_amax and bool(st.amax_spare)
        head, tail = (*bn, gg, gbe, dy.data_ptr(), ldy), (part.data_ptr(), N, H, W, C, 1 if self.bn_train else 0)
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
                return dy, E, (st.amax_spare.pop() if blk is not None else None)
        am = st.amax_spare.pop() if want_amax else None         # a zeroed word: the pass that writes dy leaves its largest magnitude there
        _timed(R, "k_bn_bwd<dx>", 12.0 * M * C, lambda: check(amax_call(lib, "cvk_bn_bwd_dx", (*head, *tail), (am,), s), "cvk_bn_bwd_dx"), "byte")
        if gb is not None:
            R.defer_colsum(st, part, PB, C, gb)
        return dy, None, am

    def _dy_both(self, R, st, rt, dy, am_dy):
        """Stage 3: 2-D data-grad and weight-grad with the same tile: dy is transformed for both in ONE launch (csrc/wino2d.hip k_w2d_dy_both): E
        for the weight-grad, V' for the data-grad; dy crosses the fabric once.  Returns (E, V', the amax block of dy: measured here when the fp16
        planes need it and no pass left it); (None, None, am_dy) for every other route."""
        if rt is None or not rt.dy_both:
            return None, None, am_dy
        lib, s, src = R.lib, st.stream, self.src
        N, H, W, M, C, ldy = src.N, src.H, src.W, src.M, self.cout, pad4(self.cout)
        tile, fmt = rt.tile, rt.split
        NX, T, Tp = planes2d(lib, tile, N, H, W, fmt)
        Eb, Vb = (torch.empty(plane_elems(NX, Tp, C, fmt), device=st.device, dtype=_PLANE_DT[fmt]) for _ in range(2))
        if fmt:
            if fmt == 2 and am_dy is None:
                am_dy = absmax(R, dy, M, C, ldy, s, "dy")
            _timed(R, "k_w2d_dy<both,%s>" % ("split3" if fmt == 3 else "split2h"), (4.0 * M + 4.0 * fmt * NX * T) * C, lambda: check(
                lib.cvk_w2d_dy_transform_both_split(fmt, tile, dy.data_ptr(), ldy, Vb.data_ptr(), Eb.data_ptr(), 1,
                                                    am_dy.data_ptr() if am_dy is not None else None, N, H, W, C, s), "cvk_w2d_dy_transform_both_split"), "byte")
        else:
            _timed(R, "k_w2d_dy<both>", 4.0 * (M + 2 * NX * T) * C, lambda: check(
                w2fn(lib, tile, "dy_transform_both")(dy.data_ptr(), ldy, Vb.data_ptr(), Eb.data_ptr(), N, H, W, C, s), "cvk_w2d_dy_transform_both"), "byte")
        return Eb, Vb, am_dy

    def _data_grad(self, R, st, rt, dy, Vb, am_dy):
        """Stage 4: dX = the data-grad through the route's family (thin, direct, or a WinoConv run as a forward conv over dy with the rotated /
        transposed filter), the first writer of the input's gradient buffer."""
        lib, s, src = R.lib, st.stream, self.src
        N, H, W, M, C, ldy, dev = src.N, src.H, src.W, src.M, self.cout, pad4(self.cout), st.device
        flops = 18.0 * M * C * self.cin
        if src.id in st.grad:
            raise NotImplementedError("conv data-grad must be the first writer of its input's gradient buffer")
        # the previous block's weight-grad ran beside this block's passes; the data-grad is matrix-bound and takes the shared workspace: join first
        R.side_join(st)
        w = st.params[4 * self.pslot]
        wc = channels_last(w)

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
                lib.cvk_conv3x3_fwd(dy.data_ptr(), wd.data_ptr(), None, dX.data_ptr(), None, N, H, W, ldy, src.ld, src.ld, s), "cvk_conv3x3_fwd(dgrad)"))
        else:
            # dX is the whole gradient of the producing block's activation when this conv is its only reader: the fused kernel then sums
            # it for that block's BatchNorm backward on the way out (training-mode statistics only)
            prod = st.plan.sole_producer(src) if rt.dgrad_bnred else None
            bnred = None
            if prod is not None and prod.bn_train and prod.idx in st.saved and pad4(prod.cout) == prod.cout == src.ld:
                bnred = st.saved[prod.idx].pointers(src.ld)
            c = WinoConv(R, s, dy, packed, None, dX, None, N, H, W, ldy, src.ld, src.ld, flops, w, (self.pslot, "d"), "(dgrad)", dgrad_of=(wc, C, self.cin))
            c.run(rt.dgrad, rt.dgrad_tile, rt.split, v_pre=Vb, x_amax=am_dy, bnred=bnred)
            if c.bnred_sums is not None:
                st.bnred[prod.idx] = c.bnred_sums
        st.grad[src.id] = dX

    def _dout(self, st):
        return (self.dst.cview(st.grad[self.dst.buf.id]),)

    def _weight_grad(self, R, st, saved, dy, gw, E, Eb, am_dy):
        """Stage 5: the weight-grad through the route's family (WeightGrad)."""
        src, rt, s = self.src, saved.rt, st.stream
        x = st.act[src.id]
        side = st.side and rt.wgrad in R.side_families
        if side:        # a leaf: nothing reads gw before backward ends -> the side stream, beside the next block's passes (joined by its data-grad)
            s = R.side_begin(st, x, dy, E, Eb, am_dy, saved)
        else:           # on the pass's stream: it takes the shared workspace, which an earlier block's forked weight-grad may still hold
            R.side_join(st)
        wg = WeightGrad(R, s, x, dy, gw, src.N, src.H, src.W, self.cin, src.ld, self.cout, pad4(self.cout), 18.0 * src.M * self.cout * self.cin)
        wg.run(rt.wgrad, rt.tile, rt.split, *(saved.kept or (None, None)), E, rt.bn_bwd == "dx+E4p", Eb, am_dy)
        if side:
            st.side_keep.extend(wg.keep)                        # operands the launches above made for themselves
            st.side_keep.append(R.workspace(0, x.device))       # their slabs / partial planes

    def bwd(self, R, st):
        saved = st.saved.pop(self.idx, None)
        if not self.active:         # frozen block with nothing upstream that needs a gradient: no backward work at all
            return
        rt, ld = saved.rt, self._pitch(self.cout)
        gw, gb, gg, gbe = self._grad_targets(R, st, ld)
        yp, *bnp = saved.pointers(ld)
        bn = (*self._dout(st), yp, ld, *bnp)        # dO, y, pitch, scale, shift, mean, rstd
        sums = self._bn_sums(R, st, bn, gg, gbe)
        if sums is None:
            return
        dy, E, am_dy = self._bn_bwd(R, st, rt, bn, gg, gbe, *sums, gb)
        Eb, Vb, am_dy = self._dy_both(R, st, rt, dy, am_dy)
        if self.src_needs_grad:
            self._data_grad(R, st, rt, dy, Vb, am_dy)
        if gw is not None:          # else a frozen conv weight: no weight-grad launch
            self._weight_grad(R, st, saved, dy, gw, E, Eb, am_dy)
        R.grads_ready(st, self.pslot)
