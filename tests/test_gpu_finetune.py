"""Fine-tuning on the GPU: frozen parameters, per-block BatchNorm modes, parameter groups and a swapped head, against stock torch
(oracle/torch_ref.py, torch.optim.AdamW) with the same freezing, in eager mode, in GraphedStep and in bf16 mode; the backward launches a
frozen region no longer makes (engine.PROF / engine.PROF_OPS); the range-table AdamW launch against cvk_adamw_step."""
import copy
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

ENCODER = ("down1", "down2", "down3", "down4", "down5")


def dev():
    return torch.device("cuda:0")


def _batch(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, h, w, generator=g), torch.randint(0, 12, (n, h, w), generator=g)


def _freeze(net, stages=ENCODER):
    for s in stages:
        m = getattr(net, s)
        m.requires_grad_(False)
        m.eval()


def _pair(seed=4, warm=True):
    """The reference network (CPU) and the device network with the same weights; one training-mode pass moves the running statistics
    away from (0, 1), so that eval-mode BatchNorm really differs from batch statistics."""
    import pytorch_camvid_amd as A
    from oracle import torch_ref as R
    torch.manual_seed(seed)
    ref = R.build("unet", 3, 12).train()
    if warm:
        with torch.no_grad():
            ref(_batch(2, 48, 64, 11)[0])
    net = A.UNet(3, 12).to(dev()).train()
    net.load_state_dict(ref.state_dict())
    return ref, net


def _grad_tolerances(ref, x, t):
    """Per trainable parameter: 4 x the reference graph's own fp32-vs-fp64 distance (ReLU masks and pool arg-maxes are discontinuous), at
    least 1e-3 (the parity bound of the small golden geometry, __graft_entry__.smoke)."""
    r64 = copy.deepcopy(ref).double()
    for p in r64.parameters():
        p.grad = None
    torch.nn.functional.cross_entropy(r64(x.double()), t).backward()
    tol = {}
    for (k, q), q64 in zip(ref.named_parameters(), r64.parameters()):
        if q.grad is not None:
            drift = float((q.grad.double() - q64.grad).norm() / q64.grad.norm())
            tol[k] = (max(4.0 * drift, 1e-3), q64.grad)
    return tol


def test_frozen_encoder_in_eval_matches_torch():
    import pytorch_camvid_amd as A
    ref, net = _pair()
    _freeze(ref); _freeze(net)
    x, t = _batch(2, 48, 64, 77)
    bn_before = {k: v.clone() for k, v in net.state_dict().items() if "running" in k or "num_batches" in k}
    out = net(x.to(dev()))
    loss = A.CrossEntropyLoss()(out, t.to(dev()))
    loss.backward()
    want = ref(x)
    lr = torch.nn.functional.cross_entropy(want, t)
    lr.backward()
    assert abs(loss.item() - lr.item()) < 5e-5, (loss.item(), lr.item())
    rel = float((out.detach().cpu() - want.detach()).norm() / want.detach().norm())
    assert rel < 1e-4, rel
    tol = _grad_tolerances(ref, x, t)
    for (k, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        if k.split(".")[0] in ENCODER:
            assert p.grad is None and q.grad is None, k
            continue
        bound, g64 = tol[k]
        r = float((p.grad.detach().cpu().double() - g64).norm() / g64.norm())
        assert r <= bound, (k, r, bound)
    sd, rsd = net.state_dict(), ref.state_dict()
    for k, v in bn_before.items():
        if k.split(".")[0] in ENCODER:      # eval-mode BatchNorm inside a training pass: statistics used, not updated
            assert torch.equal(sd[k], v), k
        else:                               # training-mode BatchNorm: updated as torch updates it
            assert not torch.equal(sd[k], v), k
            assert torch.allclose(sd[k].cpu().to(rsd[k].dtype), rsd[k], rtol=1e-4, atol=1e-5), k


def _backward_launches(net, x, t):
    """[(kernel name, op index)] of the launches of the network's backward pass (the loss's own backward launch has no op)."""
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd import engine
    loss = A.CrossEntropyLoss()(net(x), t)
    torch.cuda.synchronize()
    engine.PROF, engine.PROF_OPS = [], []
    try:
        loss.backward()
        torch.cuda.synchronize()
        rows = [(p[0], o[0]) for p, o in zip(engine.PROF, engine.PROF_OPS) if o is not None]
    finally:
        engine.PROF = engine.PROF_OPS = None
    return rows


def test_launch_accounting_frozen_encoder_and_head_only():
    import pytorch_camvid_amd as A
    from pytorch_camvid_amd import engine
    from pytorch_camvid_amd.modules import _state_of
    x, t = (v.to(dev()) for v in _batch(2, 96, 128, 5))
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    _freeze(net)
    rows = _backward_launches(net, x, t)
    plan = [p for k, p in _state_of(net)["plans"].items() if k[:4] == tuple(x.shape)][-1]
    names = {id(m): n for n, m in net.named_modules()}
    frozen = {op.idx for op in plan.convs if names[id(op.holder)].split(".")[0] in ENCODER}
    pruned = frozen | {o.idx for o in plan.ops if isinstance(o, engine.MaxPool)} | \
        {[o for o in plan.ops if isinstance(o, engine.Upsample)][0].idx}
    assert len(frozen) == 10 and rows
    hit = [(n, i) for n, i in rows if i in pruned]
    assert not hit, hit                         # no weight-grad, data-grad or BatchNorm backward in the pruned region
    up1 = [op for op in plan.convs if names[id(op.holder)] == "upsample1.conv"][0]
    assert not any("dgrad" in n for n, i in rows if i == up1.idx)
    assert any(i == up1.idx for n, i in rows)   # ... but its own weight-grad and BatchNorm backward run

    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    for n, m in net.named_children():
        if n != "output":
            m.requires_grad_(False)
    rows = _backward_launches(net, x, t)
    plan = [p for k, p in _state_of(net)["plans"].items() if k[:4] == tuple(x.shape)][-1]
    head = plan.convs[-1].idx
    assert {i for _, i in rows} == {head}, rows
    kinds = [n for n, _ in rows]
    assert any(n.startswith("k_bn_bwd") for n in kinds) and any("wgrad" in n for n in kinds) and not any("dgrad" in n for n in kinds), kinds
    assert all(p.grad is None for k, p in net.named_parameters() if not k.startswith("output."))
    assert all(p.grad is not None for k, p in net.named_parameters() if k.startswith("output."))


def _groups(named):
    """Two groups: no weight decay on BatchNorm parameters and biases, another lr for the conv weights."""
    nd = [p for k, p in named if p.dim() == 1]
    wd = [p for k, p in named if p.dim() != 1]
    return [{"params": nd, "weight_decay": 0.0, "lr": 2e-3}, {"params": wd, "weight_decay": 5e-2, "lr": 1e-3}]


def test_flat_adamw_groups_frozen_and_late_unfreezing_match_torch():
    """The same gradients into FlatAdamW and torch.optim.AdamW (two groups, encoder frozen; down5 unfrozen at step 3): trainable parameters
    follow torch (per-parameter step counts), frozen ones and their moments stay bitwise unchanged."""
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev()).train()
    twin = {k: torch.nn.Parameter(p.detach().clone()) for k, p in net.named_parameters()}
    opt = A.FlatAdamW(net, groups=_groups(list(net.named_parameters())), betas=(0.9, 0.99))
    opt_t = torch.optim.AdamW(_groups(list(twin.items())), betas=(0.9, 0.99), foreach=False)
    p0 = {k: p.detach().clone() for k, p in net.named_parameters()}
    g = torch.Generator(device=dev()).manual_seed(3)
    steps = 6
    for it in range(steps):
        frozen = ENCODER if it < 3 else ENCODER[:4]
        for k, p in net.named_parameters():
            if k.split(".")[0] in frozen:
                p.grad = twin[k].grad = None
            else:
                gr = torch.randn(p.shape, generator=g, device=dev()) * 1e-2
                p.grad, twin[k].grad = gr.clone(), gr.clone()
        opt.step()
        opt_t.step()
    for k, p in net.named_parameters():
        if k.split(".")[0] in ENCODER[:4]:
            assert torch.equal(p.detach(), p0[k]), k
        else:
            assert torch.allclose(p.detach(), twin[k].detach(), rtol=1e-5, atol=1e-7), (k, float((p - twin[k]).abs().max()))
            assert not torch.equal(p.detach(), p0[k]), k
    slot = {id(q): i for i, q in enumerate(opt._plist)}
    for k, p in net.named_parameters():
        o = opt._offs[slot[id(p)]]
        n = p.numel()
        frozen_all = k.split(".")[0] in ENCODER[:4]
        assert bool((opt._m[o:o + n] == 0).all()) == frozen_all and bool((opt._v[o:o + n] == 0).all()) == frozen_all, k
        want = 0 if frozen_all else (3 if k.startswith("down5") else steps)
        assert opt._steps[slot[id(p)]] == want == (int(opt_t.state[twin[k]]["step"]) if want else 0), k
    sd = opt.state_dict()
    opt2 = A.FlatAdamW(net, groups=_groups(list(net.named_parameters())), betas=(0.9, 0.99))
    opt2.load_state_dict(sd)
    assert opt2._steps == opt._steps and [g["lr"] for g in opt2.param_groups] == [2e-3, 1e-3]
    old = dict(sd)
    old["flat_adamw"] = {k: v for k, v in sd["flat_adamw"].items() if k != "steps"}      # the single-step format
    opt2.load_state_dict(old)
    assert opt2._steps == [opt._step] * len(opt._plist)


def test_range_launch_is_bitwise_cvk_adamw_step():
    from pytorch_camvid_amd import _lib
    lib = _lib.load()
    n = (1 << 20) + 12
    g = torch.Generator(device=dev()).manual_seed(1)
    bufs = [torch.randn(n, generator=g, device=dev()) for _ in range(2)] + [torch.rand(n, generator=g, device=dev()) * 1e-3 for _ in range(2)]
    bufs[3] = bufs[3] * bufs[3]
    a = [b.clone() for b in bufs]
    s = torch.cuda.current_stream().cuda_stream
    args = (3e-3, 0.9, 0.999, 1e-8, 1e-2, 7)
    assert lib.cvk_adamw_step(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), n, *args, s) == 0
    hyper = (_lib.AdamwHyper * 1)()
    assert lib.cvk_adamw_hyper_fill(*args, ctypes.addressof(hyper)) == 0
    hdev = torch.frombuffer(bytearray(bytes(hyper)), dtype=torch.uint8).to(dev())

    def run(ranges, dev_form):
        b = [t.clone() for t in bufs]
        tab = (_lib.AdamwRange * len(ranges))(*[_lib.AdamwRange(o, m, 0, 0) for o, m in ranges])
        nb = lib.cvk_adamw_plan_ranges(ctypes.addressof(tab), len(ranges), n, 1)
        assert nb >= len(ranges)
        tdev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev())
        ptrs = [t.data_ptr() for t in b]
        if dev_form:
            rc = lib.cvk_adamw_step_ranges_dev(*ptrs, None, n, tdev.data_ptr(), len(ranges), nb, hdev.data_ptr(), 1, None, None, 0.0, s)
        else:
            rc = lib.cvk_adamw_step_ranges(*ptrs, None, n, tdev.data_ptr(), len(ranges), nb, ctypes.addressof(hyper), 1, None, 0.0, s)
        assert rc == 0
        torch.cuda.synchronize()
        return b
    for dev_form in (False, True):
        b = run([(0, n)], dev_form)
        assert all(torch.equal(x, y) for x, y in zip(a[:1] + a[2:], b[:1] + b[2:])), dev_form
        hole = (1000, 70000)                    # a frozen range: neither read nor written, not decayed
        b = run([(0, hole[0]), (hole[1], n - hole[1])], dev_form)
        for x, y, z in zip(a, b, bufs):
            assert torch.equal(y[hole[0]:hole[1]], z[hole[0]:hole[1]])
            assert torch.equal(y[:hole[0]], x[:hole[0]]) and torch.equal(y[hole[1]:], x[hole[1]:])
    bad = (_lib.AdamwRange * 1)(_lib.AdamwRange(n - 4, 8, 0, 0))
    assert lib.cvk_adamw_plan_ranges(ctypes.addressof(bad), 1, n, 1) < 0      # outside the buffer: refused on the host

    # FlatAdamW, every parameter trainable, one group: the same update as the whole-buffer cvk_adamw_step
    import pytorch_camvid_amd as A
    torch.manual_seed(0)
    net = A.UNet(3, 12).to(dev())
    opt = A.FlatAdamW(net, lr=1e-3, weight_decay=1e-2)
    flat0 = opt._flat.clone()
    gflat = torch.randn(opt._flat.numel(), generator=g, device=dev())
    for p, o in zip(opt._plist, opt._offs):
        p.grad = (gflat[o:o + p.numel()].view(p.shape[0], p.shape[2], p.shape[3], p.shape[1]).permute(0, 3, 1, 2) if p.dim() == 4
                  else gflat[o:o + p.numel()].view(p.shape))
    opt.step()
    m, v = torch.zeros_like(flat0), torch.zeros_like(flat0)
    gl = opt._flat_grad()
    assert lib.cvk_adamw_step(flat0.data_ptr(), gl.data_ptr(), m.data_ptr(), v.data_ptr(), flat0.numel(), 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(flat0, opt._flat) and torch.equal(m, opt._m) and torch.equal(v, opt._v)


# ---- the folded range step: records as arguments / on the device x clip record or none x average or none ----------------------------------
MATRIX_N = 3072
MATRIX_RANGES = [(0, 260, 0), (512, 1028, 1), (3068, 4, 0)]      # longer than a workgroup with a tail; several workgroups; 4 floats up to the end
MATRIX_HYPER = [(3e-3, 0.9, 0.999, 1e-8, 1e-2, 7), (1e-3, 0.85, 0.99, 1e-8, 5e-2, 3)]
MATRIX_CLIP = (3.0, 0.37)                                        # {total_norm, clip_coef}
MATRIX_ALPHA = 0.1
_MATRIX = {}                                                     # the inputs and, per coefficient, the reference and the first case's result


def _matrix_inputs():
    """param, grad, exp_avg, exp_avg_sq, ema of MATRIX_N floats (never written: every case works on clones)."""
    if "bufs" not in _MATRIX:
        g = torch.Generator(device=dev()).manual_seed(23)
        bufs = [torch.randn(MATRIX_N, generator=g, device=dev()) for _ in range(2)]
        bufs += [torch.rand(MATRIX_N, generator=g, device=dev()) * 1e-3 for _ in range(2)]
        bufs[3] = bufs[3] * bufs[3]
        bufs.append(torch.randn(MATRIX_N, generator=g, device=dev()))
        _MATRIX["bufs"] = bufs
    return _MATRIX["bufs"]


def _matrix_reference(lib, coef):
    """Per range (param, exp_avg, exp_avg_sq) of cvk_adamw_step (k_adamw, whole buffer, scalars as arguments) on clones of the range's slices,
    with the range's record and the gradient multiplied by `coef` in torch fp32 (None: not multiplied)."""
    key = ("ref", coef)
    if key not in _MATRIX:
        p, g, m, v, _ = _matrix_inputs()
        s = torch.cuda.current_stream().cuda_stream
        out = []
        for o, n, r in MATRIX_RANGES:
            sl = [t[o:o + n].clone() for t in (p, g, m, v)]
            if coef is not None:
                sl[1] = sl[1] * torch.tensor(coef, dtype=torch.float32, device=dev())
            assert lib.cvk_adamw_step(*[t.data_ptr() for t in sl], n, *MATRIX_HYPER[r], s) == 0
            out.append((sl[0], sl[2], sl[3]))
        torch.cuda.synchronize()
        _MATRIX[key] = out
    return _MATRIX[key]


@pytest.mark.parametrize("with_ema", [False, True], ids=["noema", "ema"])
@pytest.mark.parametrize("with_record", [False, True], ids=["norec", "rec"])
@pytest.mark.parametrize("dev_form", [False, True], ids=["host", "device"])
def test_folded_range_step_matrix(dev_form, with_record, with_ema):
    """cvk_adamw_step_ranges / cvk_adamw_step_ranges_dev with every combination of their two nullable pointers.  Inside the ranges param and
    the moments are bitwise cvk_adamw_step on the slice; outside nothing changes, in any buffer; the average follows
    e + alpha * (p_new - e) within the bound of test_gpu_ema.py (one update: 2^-21 times the largest magnitude among p and e, which is what
    its derivation takes max|p| for); cases with the same coefficient agree bitwise."""
    from pytorch_camvid_amd import _lib
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    orig = _matrix_inputs()
    b = [t.clone() for t in orig[:4]]
    ema = orig[4].clone() if with_ema else None                     # without an average there is no buffer at all
    coef = MATRIX_CLIP[1] if with_record else None
    ref = _matrix_reference(lib, coef)

    hyper = (_lib.AdamwHyper * len(MATRIX_HYPER))()
    for r, args in enumerate(MATRIX_HYPER):
        assert lib.cvk_adamw_hyper_fill(*args, ctypes.addressof(hyper) + r * ctypes.sizeof(_lib.AdamwHyper)) == 0
    tab = (_lib.AdamwRange * len(MATRIX_RANGES))(*[_lib.AdamwRange(o, n, r, 0) for o, n, r in MATRIX_RANGES])
    nb = lib.cvk_adamw_plan_ranges(ctypes.addressof(tab), len(MATRIX_RANGES), MATRIX_N, len(MATRIX_HYPER))
    assert nb == 2 + 5 + 1 and [e.block0 for e in tab] == [0, 2, 7]
    tdev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev())
    rec = torch.tensor(MATRIX_CLIP, dtype=torch.float32, device=dev()) if with_record else None
    alpha = torch.tensor([MATRIX_ALPHA], dtype=torch.float32, device=dev())
    head = [t.data_ptr() for t in b] + [ema.data_ptr() if with_ema else None, MATRIX_N, tdev.data_ptr(), len(MATRIX_RANGES), nb]
    recp = rec.data_ptr() if with_record else None
    if dev_form:
        hdev = torch.frombuffer(bytearray(bytes(hyper)), dtype=torch.uint8).to(dev())
        rc = lib.cvk_adamw_step_ranges_dev(*head, hdev.data_ptr(), len(MATRIX_HYPER), recp, alpha.data_ptr() if with_ema else None,
                                           MATRIX_ALPHA if with_ema else 0.0, s)
    else:
        rc = lib.cvk_adamw_step_ranges(*head, ctypes.addressof(hyper), len(MATRIX_HYPER), recp, MATRIX_ALPHA if with_ema else 0.0, s)
    assert rc == 0, lib.cvk_last_error_string()
    torch.cuda.synchronize()

    inside = torch.zeros(MATRIX_N, dtype=torch.bool, device=dev())
    for (o, n, _), (rp, rm, rv) in zip(MATRIX_RANGES, ref):
        inside[o:o + n] = True
        assert torch.equal(b[0][o:o + n], rp) and torch.equal(b[2][o:o + n], rm) and torch.equal(b[3][o:o + n], rv), (o, n)
        assert not torch.equal(b[0][o:o + n], orig[0][o:o + n])
    assert int(inside.sum()) == sum(n for _, n, _ in MATRIX_RANGES) < MATRIX_N
    for got, was in zip(b, orig):                                    # outside the ranges: the original bits; the gradient: everywhere
        assert torch.equal(got[~inside], was[~inside])
    assert torch.equal(b[1], orig[1])
    if with_ema:
        assert torch.equal(ema[~inside], orig[4][~inside])
        a32 = float(alpha.item())
        e0, pn = orig[4].double(), b[0].double()
        want = e0 + a32 * (pn - e0)
        pmax = float(torch.stack([orig[0].abs().max(), b[0].abs().max(), orig[4].abs().max()]).max())
        worst, bound = float((ema.double() - want).abs()[inside].max()), 2.0 ** -21 * pmax
        print(f"folded step matrix: max |ema - fp64| = {worst:.3e}, bound {bound:.3e} (largest magnitude {pmax:.4f})")
        assert worst <= bound
        assert not torch.equal(ema[inside], orig[4][inside])
    first = _MATRIX.setdefault(("seen", coef), (b[0], b[2], b[3]))    # the cases with this coefficient that ran before: the same bits
    assert all(torch.equal(x, y) for x, y in zip(first, (b[0], b[2], b[3])))
    if ("seen", None) in _MATRIX and ("seen", MATRIX_CLIP[1]) in _MATRIX:
        assert not torch.equal(_MATRIX[("seen", None)][0], _MATRIX[("seen", MATRIX_CLIP[1])][0])     # the record really scaled the gradient


def _ft_make(A, iters, seed=0):
    torch.manual_seed(seed)
    net = A.UNet(3, 12).to(dev()).train()
    _freeze(net)
    opt = A.FlatAdamW(net, groups=_groups(list(net.named_parameters())))
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=[2e-3, 1e-3], total_steps=iters + 4, cycle_momentum=True)
    return net, opt, sched


def test_graphed_step_fine_tuning_is_bitwise_the_eager_loop():
    import pytorch_camvid_amd as A
    iters = 5
    net, opt, sched = _ft_make(A, iters)
    st0 = {k: v.clone() for k, v in net.state_dict().items()}
    lossf = A.CrossEntropyLoss()
    x0, t0 = _batch(2, 48, 64, 1)
    gs = A.GraphedStep(net, lossf, x0.to(dev()), t0.to(dev()), optimizer=opt, scheduler=sched, log_capacity=iters)
    net.load_state_dict(st0)
    ref, opt_r, sched_r = _ft_make(A, iters)
    ref.load_state_dict(net.state_dict())
    for it in range(iters):
        x, t = (v.to(dev()) for v in _batch(2, 48, 64, 100 + it))
        la = gs.replay(x, t)
        opt_r.zero_grad()
        lb = lossf(ref(x), t)
        lb.backward()
        opt_r.step()
        sched_r.step()
        assert torch.equal(la, lb), it
        for (k, p), q in zip(net.named_parameters(), ref.parameters()):
            assert torch.equal(p, q), (it, k)
        assert torch.equal(opt._m, opt_r._m) and torch.equal(opt._v, opt_r._v), it
        for (k, b), c in zip(net.named_buffers(), ref.buffers()):
            assert torch.equal(b, c), (it, k)
        assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in opt_r.param_groups]
    assert opt._steps == opt_r._steps and opt._step == opt_r._step == iters
    rows, _ = gs.log()
    assert rows.shape == (iters, 5)
    for k, p in net.named_parameters():
        if k.split(".")[0] in ENCODER:
            assert torch.equal(p, st0[k]), k
    net.down3.requires_grad_(True)
    with pytest.raises(RuntimeError, match="changed since the capture"):
        gs.replay()
    net.down3.requires_grad_(False)
    gs.replay()
    net.up1.eval()
    with pytest.raises(RuntimeError, match="changed since the capture"):
        gs.replay()


def test_head_swap_after_a_forward():
    import pytorch_camvid_amd as A
    ref, net = _pair(warm=False)
    x, t = _batch(2, 48, 64, 9)
    with torch.no_grad():
        assert net(x.to(dev())).shape[1] == 12
    torch.manual_seed(21)
    net.output = A.BasicConv2d(64, 21).to(dev())
    from oracle import torch_ref as R
    ref.output = R.build("unet", 3, 21).output
    ref.output.load_state_dict({k.split("output.", 1)[1]: v.cpu() for k, v in net.state_dict().items() if k.startswith("output.")})
    t = t % 21
    out = net(x.to(dev()))
    assert out.shape == (2, 21, 48, 64)
    loss = A.CrossEntropyLoss()(out, t.to(dev()))
    loss.backward()
    want = ref(x)
    lr = torch.nn.functional.cross_entropy(want, t)
    lr.backward()
    assert abs(loss.item() - lr.item()) < 5e-5
    assert float((out.detach().cpu() - want.detach()).norm() / want.detach().norm()) < 1e-4
    gw, gr = net.output.conv[0].weight.grad.cpu(), ref.output.conv[0].weight.grad
    assert float((gw - gr).norm() / gr.norm()) < 1e-3


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_frozen_encoder_trainable_gradients_are_the_full_backward(precision):
    """Encoder frozen (BatchNorm in training mode): every trainable gradient is bitwise what the all-trainable backward computes, in fp32 and
    in bf16 mode; frozen parameters get no gradient.  bf16 mode refuses a per-block BatchNorm mode by name where the block runs a backward."""
    import pytorch_camvid_amd as A
    x, t = (v.to(dev()) for v in _batch(2, 48, 64, 13))
    grads = []
    for frozen in (False, True):
        torch.manual_seed(0)
        net = A.set_conv_precision(A.UNet(3, 12).to(dev()).train(), precision)
        if frozen:
            for s in ENCODER:
                getattr(net, s).requires_grad_(False)
        A.CrossEntropyLoss()(net(x), t).backward()
        grads.append({k: (p.grad.clone() if p.grad is not None else None) for k, p in net.named_parameters()})
    for k, g in grads[1].items():
        if k.split(".")[0] in ENCODER:
            assert g is None, k
        else:
            assert torch.equal(g, grads[0][k]), k
    # the encoder frozen AND in eval mode: served in both modes (its blocks run the inference forward pass only), and close to each other
    losses = {}
    for prec in ("fp32", precision):
        torch.manual_seed(0)
        net = A.set_conv_precision(A.UNet(3, 12).to(dev()).train(), prec)
        _freeze(net)
        loss = A.CrossEntropyLoss()(net(x), t)
        loss.backward()
        losses[prec] = loss.item()
        assert all(p.grad is None for k, p in net.named_parameters() if k.split(".")[0] in ENCODER)
        assert all(bool(torch.isfinite(p.grad).all()) for k, p in net.named_parameters() if k.split(".")[0] not in ENCODER)
    assert abs(losses[precision] - losses["fp32"]) < 1e-2, losses
    if precision == "bf16":         # an eval-mode block that runs a backward inside a training pass: refused by name
        net.up2.eval()
        with pytest.raises(NotImplementedError, match="up2.0"):
            net(x)
