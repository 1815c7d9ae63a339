"""The kernel route of every conv block (route.conv_route, no GPU), pinned for the configurations the benchmark and the GPU tests run: UNet and
SegNet at 8 x 3 x 360 x 480 under the default switches and each forced mode, eval without gradients, and the golden 2 x 3 x 48 x 64 plan.
A row reads "forward  data-grad  BatchNorm-backward  weight-grad  flags" (ConvRoute fields; "@t" a 2-D tile, "/f" a split format, "-" no
data-grad).  The table was derived from the kernel choices the engine made before the route existed."""
import pytest

import pytorch_camvid_amd as A
from pytorch_camvid_amd import engine
from pytorch_camvid_amd.modules import runner_of


def _plan(kind, N, H, W):
    net = A.get_model(kind, 3, 12)
    plan = engine.Plan(N, 3, H, W)
    plan.output = net._emit(plan, plan.input)
    plan.seal()
    return runner_of(net), plan


def _row(r, need_grad):
    f = r.fwd + ("@%d" % r.tile if r.tile else "") + ("/%d" % r.split if r.split else "")
    if not need_grad:
        return f
    d = (r.dgrad or "-") + ("@%d" % r.dgrad_tile if r.dgrad_tile else "") + ("+bnred" if r.dgrad_bnred else "")
    flags = [n for n in ("dy_both", "keeps_v", "dy_amax") if getattr(r, n)]
    return " ".join([f, d, r.bn_bwd, r.wgrad] + flags)


TABLE = {
    ('unet', (8, 360, 480), None, True, True): [
        'thin - dx thin',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'thin thin dx thin',
    ],
    ('unet', (8, 360, 480), ('wino2d', 'always'), True, True): [
        'thin - dx thin',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'thin thin dx thin',
    ],
    ('unet', (8, 360, 480), ('wgradp', 'always'), True, True): [
        'thin - dx thin',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'thin thin dx thin',
    ],
    ('unet', (8, 360, 480), ('wino4', 'always'), True, True): [
        'thin - dx thin',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w2d@6 w2d@6 dx w2d dy_both keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'thin thin dx thin',
    ],
    ('unet', (8, 360, 480), ('w2d_split', 2), True, True): [
        'thin - dx thin',
        'w4h w4h+bnred dx+E6 wgradp dy_amax',
        'w4h w4h+bnred dx+E6 wgradp dy_amax',
        'w4h w4h+bnred dx+E w4 dy_amax',
        'w4h w4h+bnred dx+E w4 dy_amax',
        'w2d_split@6/2 w2d_split@6 dx w2d_split dy_both keeps_v dy_amax',
        'w2d_split@6/2 w2d_split@6 dx w2d_split dy_both keeps_v dy_amax',
        'w2d_split@6/2 w2d_split@6 dx w2d_split dy_both keeps_v dy_amax',
        'w2d_split@4/2 w2d_split@4 dx w2d_split dy_both keeps_v dy_amax',
        'w2d_split@4/2 w2d_split@4 dx w2d_split dy_both keeps_v dy_amax',
        'w2d_split@6/2 w2d_split@6 dx w2d_split dy_both keeps_v dy_amax',
        'w2d_split@6/2 w2d_split@6 dx w2d_split dy_both keeps_v dy_amax',
        'w2d_split@6/2 w2d_split@6 dx w2d_split dy_both keeps_v dy_amax',
        'w2d_split@6/2 w2d_split@6 dx w2d_split dy_both keeps_v dy_amax',
        'w2d_split@6/2 w2d_split@6 dx w2d_split dy_both keeps_v dy_amax',
        'w2d_split@6/2 w2d_split@6 dx w2d_split dy_both keeps_v dy_amax',
        'w2d_split@6/2 w2d_split@6 dx w2d_split dy_both keeps_v dy_amax',
        'w2d_split@6/2 w2d_split@6 dx w2d_split dy_both keeps_v dy_amax',
        'w4h w4h+bnred dx+E w4 dy_amax',
        'w4h w4h+bnred dx+E w4 dy_amax',
        'w4h w4h+bnred dx+E w4 dy_amax',
        'w4h w4h+bnred dx+E6 wgradp dy_amax',
        'thin thin dx thin dy_amax',
    ],
    ('unet', (8, 360, 480), ('w2d_split', 3), True, True): [
        'thin - dx thin',
        'w4f w4f+bnred dx+E6 wgradp',
        'w4f w4f+bnred dx+E6 wgradp',
        'w4f w4f+bnred dx+E w4',
        'w4f w4f+bnred dx+E w4',
        'w2d_split@6/3 w2d_split@6 dx w2d_split dy_both keeps_v',
        'w2d_split@6/3 w2d_split@6 dx w2d_split dy_both keeps_v',
        'w2d_split@6/3 w2d_split@6 dx w2d_split dy_both keeps_v',
        'w2d_split@4/3 w2d_split@4 dx w2d_split dy_both keeps_v',
        'w2d_split@4/3 w2d_split@4 dx w2d_split dy_both keeps_v',
        'w2d_split@6/3 w2d_split@6 dx w2d_split dy_both keeps_v',
        'w2d_split@6/3 w2d_split@6 dx w2d_split dy_both keeps_v',
        'w2d_split@6/3 w2d_split@6 dx w2d_split dy_both keeps_v',
        'w2d_split@6/3 w2d_split@6 dx w2d_split dy_both keeps_v',
        'w2d_split@6/3 w2d_split@6 dx w2d_split dy_both keeps_v',
        'w2d_split@6/3 w2d_split@6 dx w2d_split dy_both keeps_v',
        'w2d_split@6/3 w2d_split@6 dx w2d_split dy_both keeps_v',
        'w2d_split@6/3 w2d_split@6 dx w2d_split dy_both keeps_v',
        'w4f w4f+bnred dx+E w4',
        'w4f w4f+bnred dx+E w4',
        'w4f w4f+bnred dx+E w4',
        'w4f w4f+bnred dx+E6 wgradp',
        'thin thin dx thin',
    ],
    ('unet', (8, 360, 480), None, False, False): [
        'thin',
        'w4f',
        'w4f',
        'w4f',
        'w4f',
        'w2d@6',
        'w2d@6',
        'w2d@6',
        'w2d@4',
        'w2d@4',
        'w2d@6',
        'w2d@6',
        'w2d@6',
        'w2d@6',
        'w2d@6',
        'w2d@6',
        'w2d@6',
        'w2d@6',
        'w4f',
        'w4f',
        'w4f',
        'w4f',
        'thin',
    ],
    ('unet', (2, 48, 64), None, True, True): [
        'thin - dx thin',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'thin thin dx thin',
    ],
    ('segnet', (8, 360, 480), None, True, True): [
        'thin - dx thin',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'thin thin dx thin',
    ],
    ('segnet', (8, 360, 480), ('wino2d', 'always'), True, True): [
        'thin - dx thin',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'thin thin dx thin',
    ],
    ('segnet', (8, 360, 480), ('wgradp', 'always'), True, True): [
        'thin - dx thin',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@4 dx w2d dy_both keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w2d@4 w2d@6 dx w2d keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'w4f_vplanes w4f+bnred dx+E4p wgradp_sm keeps_v',
        'thin thin dx thin',
    ],
    ('segnet', (8, 360, 480), None, False, False): [
        'thin',
        'w4f',
        'w4f',
        'w4f',
        'w4f',
        'w2d@4',
        'w2d@4',
        'w2d@4',
        'w2d@4',
        'w2d@4',
        'w2d@4',
        'w2d@4',
        'w2d@4',
        'w2d@4',
        'w2d@4',
        'w2d@4',
        'w2d@4',
        'w2d@4',
        'w2d@4',
        'w2d@4',
        'w2d@4',
        'w4f',
        'w4f',
        'w4f',
        'w4f',
        'thin',
    ],
    ('segnet', (2, 48, 64), None, True, True): [
        'thin - dx thin',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'w2 w2 dx+E w4',
        'thin thin dx thin',
    ],
}


@pytest.mark.parametrize("key", list(TABLE), ids=lambda k: "%s-%dx%dx%d-%s-%s" % (k[0], *k[1], k[2], "train" if k[3] else "eval"))
def test_route_table(key):
    kind, (N, H, W), knob, training, need_grad = key
    R, plan = _plan(kind, N, H, W)
    if knob is not None:
        setattr(R, *knob)
    routes = R.routes(plan, training, need_grad)
    convs = [op for op in plan.ops if isinstance(op, engine.ConvBnRelu)]
    assert len(convs) == (23 if kind == "unet" else 26)
    assert [_row(routes[op.idx], need_grad) for op in convs] == TABLE[key]


def test_forward_keeps_exactly_what_the_weight_grad_reads():
    R, plan = _plan("unet", 8, 360, 480)
    for knob in (None, ("wino2d", "always"), ("wgradp", "always"), ("w2d_split", 2), ("w2d_split", 3), ("vplanes", False)):
        if knob is not None:
            setattr(R, *knob)
        for r in R.routes(plan, True, True).values():
            assert r.keeps_v == (r.wgrad in ("w2d", "w2d_split", "wgradp_sm") and r.fwd in ("w2d", "w2d_split", "w4f_vplanes"))
            assert (r.fwd == "w4f_vplanes") == (r.wgrad == "wgradp_sm") and (r.fwd == "w2d_split") == (r.wgrad == "w2d_split")


def test_routes_are_cached_per_configuration():
    R, plan = _plan("unet", 2, 48, 64)
    a = R.routes(plan, True, True)
    assert R.routes(plan, True, True) is a and R.routes(plan, False, False) is not a
    R.wino2d = "always"
    b = R.routes(plan, True, True)
    assert b is not a and b != a
    R.wino2d = True
    assert R.routes(plan, True, True) is a


def test_vplanes_bound_is_the_kernels():
    """The fused launch that writes V planes addresses six planes of cvk_wgradp_plane_rows rows with 32-bit offsets (csrc/wino4f.hip): at
    50 x 464 x 480, 64 -> 64 channels they do not fit and the layer runs the plain fused kernel; one row of pixels less, they do."""
    R, plan = _plan("unet", 50, 464, 480)
    convs = [op for op in plan.ops if isinstance(op, engine.ConvBnRelu)]
    r = R.routes(plan, True, True)[convs[1].idx]
    assert (convs[1].cin, convs[1].cout) == (64, 64)
    assert (r.fwd, r.wgrad, r.bn_bwd) == ("w4f", "wgradp", "dx+E6") and not r.keeps_v
    R, plan = _plan("unet", 50, 463, 480)
    convs = [op for op in plan.ops if isinstance(op, engine.ConvBnRelu)]
    r = R.routes(plan, True, True)[convs[1].idx]
    assert (r.fwd, r.wgrad, r.bn_bwd) == ("w4f_vplanes", "wgradp_sm", "dx+E4p") and r.keeps_v
