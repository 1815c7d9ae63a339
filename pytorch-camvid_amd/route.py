"""Kernel selection for the fp32 conv blocks: which kernels run a layer's forward pass, data-grad, BatchNorm backward and weight-grad.

`conv_route` decides all of it in one place from the layer geometry, the runner's switches (Runner.kernel_config) and the pass kind, and
returns a frozen ConvRoute; conv_fp32.py launches what the route names.  Nothing here launches a kernel or allocates device memory: the
library is only asked host-side questions (cvk_thin_*_supported, cvk_wgradp_plane_rows).
"""
from dataclasses import dataclass


def pad4(c):
    return (c + 3) // 4 * 4


def wino_ok(R, k_ch, n_cols):
    return R.wino and k_ch % 64 == 0


def wino4_pays(N, H, W, k_ch, n_cols):
    """F(4,3) or F(2,3) for this layer?  Both kernels do the same work per workgroup (3*k_ch/32 K steps of a 128-row
    tile); F(4,3) needs 6 workgroups per 4 columns, F(2,3) 8, and splits its K loop when the grid is small
    (csrc/wino4.hip plan_wino4), so it wins (measured, tools/bench_conv.py wino wino4) whenever there is more than one
    wave of work.  F(2,3) — the more accurate of the two — keeps the <= 32-column head and layers whose whole F(2,3)
    grid is at most one workgroup per CU anyway (the small golden geometries)."""
    if n_cols <= 32:
        return False
    tn = -(-n_cols // 128) if n_cols > 64 else 1
    return -(-(N * H * ((W + 1) // 2)) // 128) * tn * 4 > 256


def layer_tile(R, N, H, W, dgrad=False):
    """Output tile of the 2-D path for a layer geometry (dgrad: of a data-grad launch — networks with MaxUnpool2d keep 4x4 tiles in the
    forward pass, where coarser rounding flips pool arg-maxes, but their data-grads run after the indices are fixed: 6x6).  The batched GEMM works on 128-row tiles of the tile index: at the 22x30
    bottleneck (batch 8) 6x6 tiles give 160 rows = two row tiles of which 37 % are padding (138 us, as long as F(4x4)'s three full
    row tiles) and 1.78x the filter-transform bytes (50 vs 28 us at 1024 x 1024 channels) — such layers keep 4x4 tiles."""
    if (R.w2tile_dgrad if dgrad else R.w2tile) != 6:
        return 4
    t6 = N * ((H + 5) // 6) * ((W + 5) // 6)
    t4 = N * ((H + 3) // 4) * ((W + 3) // 4)
    u6 = t6 / (128.0 * ((t6 + 127) // 128))
    u4 = t4 / (128.0 * ((t4 + 127) // 128))
    return 4 if (u6 < 0.7 and u4 > u6 + 0.2) else 6


def wino2d_ok(k_ch, cout, ldy):
    return k_ch % 32 == 0 and cout % 4 == 0 and cout >= 64 and ldy % 4 == 0


def wino2d_pays(N, H, W, k_ch, cout, tile=4):
    """Measured at the UNet batch-8 shapes (tools/bench_conv.py wino4 w2d [--rev]; tile 6: tools/bench_w6.py).  F(4x4,3x3): the 36
    batched GEMMs + transforms beat F(4,3) + its output pass by 13-31 % once Cin*Cout >= 256*256 (256->256 @ 90x120 ... 1024->512 @
    45x60), by 10-13 % for 128<->256 channels at 180x240, and lose below that (the transform passes cost more than the saved
    multiplies).  F(6x6,3x3) is 15-25 % cheaper than F(4x4) on every layer with >= 256 tiles (21 % fewer multiplies and plane
    bytes) and would also take 128->128 @180x240 (435 vs 490 us forward) and 128<->256 @90x120 (170 vs 252 / 302 us) from the fused
    1-D kernel — measured: no gain on the whole step (231.4 vs 232.9 img/s on two boxes) while the logits deviation from the
    reference grows again (headline workload, sampled logits: max 6.9e-4 and 1.2 % beyond 3e-4, against 4.6e-4 / 0.3 % with the layer
    set below; F(4x4): 2.5e-4 / none; the reference's own fp32-vs-1e-6-noise drift: 1.7e-4) — so both tile sizes take the SAME layers."""
    T = N * ((H + 3) // 4) * ((W + 3) // 4)
    return T >= 256 and (k_ch * cout >= 65536 or (k_ch * cout >= 32768 and T >= 16384))


def wgrad2d_pays(N, H, W, k_ch, cout):
    """Weight-grad through the 2-D transform: wins from 256 x 256 channels up (0.60-0.90 of the transposed F(4,3) time at the
    UNet batch-8 shapes), loses below (the dy / x transform passes dominate)."""
    T = N * ((H + 3) // 4) * ((W + 3) // 4)
    return T >= 256 and k_ch * cout >= 65536


def wino4f_ok(k_ch, cout):
    return k_ch % 32 == 0 and cout % 4 == 0 and cout >= 32


def wgradp_ok(cin_ld, cout, ldy):
    return cin_ld % 64 == 0 and cout % 64 == 0 and ldy == cout


def wgradp_pays(N, H, W, cin_ld, cout):
    return cin_ld == 64 and N * H * ((W + 3) // 4) >= 4096


def vplanes_pays(lib, N, H, W, cin_ld, cout):
    """tools/bench_vplanes.py at the headline shapes (64/128 -> 64/128/256 channels, 360x480 ... 90x120, batch 8): the forward launch costs
    +9 ... +47 us, the weight-grad gains 34 ... 370 us on every layer; bounded by the kernel's 4 GiB plane addressing (csrc/wino4f.hip: six
    planes of cvk_wgradp_plane_rows rows)."""
    rows = lib.cvk_wgradp_plane_rows(N, H, W)
    return cin_ld % 64 == 0 and cout <= 512 and N * H * ((W + 3) // 4) >= 4096 and 6 * cin_ld * 4 * rows < 2 ** 32 - 4096


def split_fmt(R):
    """runner.w2d_split as a split-plane format (csrc/split_fmt.h): 0 = off (exact-fp32 MFMA, the default), 3 = three bf16 terms (True means
    this one), 2 = two scaled fp16 terms."""
    v = getattr(R, "w2d_split", 0)
    return 3 if v is True else (int(v) if v in (2, 3) else 0)


W2D = ("w2d", "w2d_split")


@dataclass(frozen=True)
class ConvRoute:
    """The kernels of one conv block for one kind of pass.

    fwd:   "thin" (csrc/thin.hip) | "direct" (implicit GEMM) | "w2" (F(2,3)) | "w4" (per-index F(4,3)) | "w4f" (fused F(4,3)) | "w4f_vplanes"
           (... also writing the weight-grad's V planes) | "w4h" (... fp16 split operands) | "w2d" (2-D F(4x4) / F(6x6)) | "w2d_split" (split GEMMs)
    tile:  output tile (4 | 6) of the 2-D forward and weight-grad launches; split: their split-plane format (2 | 3) in the "w2d_split" family
    dgrad: the data-grad's family (the forward families without "w4f_vplanes"), None without one; dgrad_tile: its 2-D tile
    dgrad_bnred: a fused data-grad may leave the producing block's BatchNorm-backward sums (if that block is its input's sole writer)
    dy_both: one launch transforms dy for the 2-D data-grad and the 2-D weight-grad (same tile)
    bn_bwd: "dx" | "dx+E" (transposed F(4,3) planes) | "dx+E6" (plane GEMM: six planes) | "dx+E4p" (four planes, E0 / E5 read from dy)
    wgrad: "w2d" | "w2d_split" | "wgradp_sm" (plane GEMM over the forward's V planes) | "wgradp" (plane GEMM, own V pass) | "w4" (transposed
           F(4,3)) | "thin" | "w2" (F(2,3)) | "direct"; None for a frozen conv weight (no weight-grad launch)
    dy_amax: the pass that writes dy leaves its largest magnitude for the fp16 split-operand data-grad"""
    fwd: str
    tile: int = 0
    split: int = 0
    dgrad: str = None
    dgrad_tile: int = 0
    dgrad_bnred: bool = False
    dy_both: bool = False
    bn_bwd: str = "dx"
    wgrad: str = None
    dy_amax: bool = False

    @property
    def keeps_v(self):
        """The forward pass keeps its transformed input for the weight-grad: the 2-D families' V, or the fused launch's V planes."""
        return (self.fwd in W2D and self.wgrad == self.fwd) or (self.fwd == "w4f_vplanes" and self.wgrad == "wgradp_sm")


def _w2d(R, N, H, W, k_ch, cout, ldy):
    """Does a launch of k_ch -> cout channels (forward, or data-grad with k_ch = dy's pitch) take the 2-D path?"""
    return wino_ok(R, k_ch, ldy) and wino2d_ok(k_ch, cout, ldy) and (R.wino2d == "always" or (R.wino2d and wino2d_pays(N, H, W, k_ch, cout, R.w2tile)))


def _wino_1d(R, N, H, W, k_ch, cout, ldy, fused_ok, h2):
    """A 1-D Winograd launch: fused F(4,3) (h2: its fp16 split-operand form), per-index F(4,3) or F(2,3)."""
    use4 = R.wino4 == "always" or (R.wino4 and wino4_pays(N, H, W, k_ch, ldy))
    if use4 and R.wino4f and wino4f_ok(k_ch, cout) and fused_ok:
        return "w4h" if h2 else "w4f"
    return "w4" if use4 else "w2"


def conv_route(R, op, training, need_grad):
    """The route of conv block `op` (conv_fp32.ConvBnRelu) of a plan whose 2-D tiles are R.w2tile / R.w2tile_dgrad (Runner.tile_for).  The block's
    own flags decide its backward: no backward route when it is frozen with nothing upstream needing a gradient (op.active), no weight-grad
    (and no V kept by the forward pass) when its conv weight is frozen (op.w_req), no data-grad when nothing upstream needs one."""
    lib, src = R.lib, op.src
    bwd = need_grad and op.active
    wg = bwd and op.w_req
    N, H, W, k, C, cin = src.N, src.H, src.W, src.ld, op.cout, op.cin
    ldy = pad4(C)
    fmt = split_fmt(R)
    fits = H * W * max(k, ldy) * 4 < 2 ** 31            # thin kernels: one image per buffer resource
    tile, dtile = layer_tile(R, N, H, W), layer_tile(R, N, H, W, dgrad=True)
    fwd2d, dgrad2d = _w2d(R, N, H, W, k, C, ldy), _w2d(R, N, H, W, ldy, k, k)

    # weight-grad: transposed 2-D F(4x4,3x3) for the channel-heavy layers (25-40 % faster than the transposed F(4,3) from 256 x 256
    # channels up: tools/bench_conv.py ww2d); 128 <-> 256 channels at 180x240 tie on the x transform alone, but their forward pass runs the
    # 2-D path and leaves V behind (0.78 of the F(4,3) time without that pass; 6x6 tiles: 0.46)
    wgrad2d = bool(wg and R.wino and R.wino2d and k % 4 == 0 and ldy == C and k >= 32 and C >= 64
                   and (R.wino2d == "always" or wgrad2d_pays(N, H, W, k, C) or (fwd2d and k * C >= 32768)))
    # ... else the transposed F(4,3): fastest weight-grad on every layer with >= 64 input channels (tools/bench_conv.py wgrad wwino wwino4)
    wgrad4 = bool(wg and not wgrad2d and R.wino and k >= 32 and C > 32 and (R.wino4 == "always" or (R.wino4 and k >= 64)))
    # OPT-IN split-operand GEMMs (csrc/split3.hip): layers whose forward, data-grad and weight-grad ALL take the 2-D path with one tile and
    # whose channel counts the split weight-grad GEMM serves — the three GEMMs share their split planes (V from the forward transform, V'
    # and E from one pass over dy)
    split = fmt if (wg and training and fmt and op.src_needs_grad and wgrad2d and k == cin and k % 32 == 0 and C % 32 == 0 and fwd2d
                    and dgrad2d and tile == dtile and ((C % 256 == 0 and k % 128 == 0) or (k % 256 == 0 and C % 128 == 0))) else 0
    # the fused forward launch leaves the V planes of a plane-GEMM weight-grad behind (csrc/wgradp.hip)
    planes = bool(wg and R.vplanes and R.wgradp and fmt == 0 and wgrad4 and wgradp_ok(k, C, ldy) and vplanes_pays(lib, N, H, W, k, C))

    if R.thin and lib.cvk_thin_fwd_supported(k, C, ldy) and (not training or k <= 8 or k == 64) and fits:
        fwd = "thin"            # the stem (3 -> 64) and the classifier head (64 -> 12): the thin side is one side of a 16x16x4 MFMA
    elif not wino_ok(R, k, ldy):
        fwd = "direct"
    elif fwd2d:
        fwd = "w2d_split" if split else "w2d"
    else:
        fwd = _wino_1d(R, N, H, W, k, C, ldy, True, fmt == 2 and need_grad and training)
        if fwd == "w4f" and planes:
            fwd = "w4f_vplanes"
    split = split if fwd == "w2d_split" else 0
    if not bwd:
        return ConvRoute(fwd, tile if fwd in W2D else 0, split)

    # 64-input-channel layers (and every layer whose forward left V planes): both transforms outside the GEMM (csrc/wgradp.hip) — the E
    # planes come from the BatchNorm-backward pass; pays while the V pass over x is cheap (64 -> 64 @360x480 0.74x, 64 -> 128 @180x240 0.7x
    # the time of the transposed F(4,3) kernel; 128 input channels: the V pass eats the gain)
    wgradp = wgrad4 and R.wgradp and wgradp_ok(k, C, ldy) and (R.wgradp == "always" or fwd == "w4f_vplanes" or wgradp_pays(N, H, W, k, C))
    if not wg:
        wgrad = None
    elif wgrad2d:
        wgrad = "w2d_split" if split else "w2d"
    elif wgradp:
        wgrad = "wgradp_sm" if fwd == "w4f_vplanes" else "wgradp"
    elif wgrad4:
        wgrad = "w4"
    elif R.thin and lib.cvk_thin_wgrad_supported(cin, k, C, ldy) and fits:
        wgrad = "thin"
    elif R.wino and k >= 32 and C > 32 and (k > 64 or C > 64):      # 64->64 layers: the direct kernel is faster
        wgrad = "w2"
    else:
        wgrad = "direct"

    # the BatchNorm-backward pass writes the weight-grad's E planes; four with forward planes, the plane GEMM reading E0 / E5 from dy
    if wgradp:
        bn_bwd = "dx+E4p" if wgrad == "wgradp_sm" and W % 4 == 0 else "dx+E6"
    else:
        bn_bwd = "dx+E" if wgrad == "w4" and ldy == C else "dx"

    if not op.src_needs_grad:
        dgrad = None
    elif wino_ok(R, ldy, k):
        dgrad = ("w2d_split" if split else "w2d") if dgrad2d else _wino_1d(R, N, H, W, ldy, k, k, ldy == C and k == cin, fmt == 2 and training)
    elif R.thin and lib.cvk_thin_fwd_supported(ldy, k, k) and fits:
        dgrad = "thin"          # the head's data-grad: 12 -> 64
    else:
        dgrad = "direct"
    return ConvRoute(fwd, tile if (fwd in W2D or wgrad in W2D) else 0, split, dgrad, dtile if dgrad in W2D else 0,
                     training and dgrad in ("w4f", "w4h"), dgrad in W2D and wgrad in W2D and ldy == C and tile == dtile, bn_bwd, wgrad,
                     fmt == 2 and training and op.src_needs_grad)
