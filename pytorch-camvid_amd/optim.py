"""FlatAdamW — torch.optim.AdamW semantics (reference train.py:100,133) as ONE fused kernel over flat buffers.

The executor already writes every gradient into one flat fp32 buffer (engine.layout_grads).  FlatAdamW re-homes the
parameters into a flat buffer with the SAME layout, so a step is a single `cvk_adamw_step` launch over 34.5 M
elements (7 x 138 MB of HBM traffic) instead of ~10 multi-tensor launches over 92 tensors.  It is a
`torch.optim.Optimizer`: every group's `lr` / `betas` are read every step, so `OneCycleLR` (train.py:103-104) drives it unchanged.

Fine-tuning: `groups=` takes torch-style parameter groups (every parameter of the network in exactly one group; per-group `lr`, `betas`,
`eps`, `weight_decay`).  As torch.optim.AdamW, a parameter whose `.grad` is None is skipped and each parameter keeps its own step count (a
block unfrozen late starts its bias correction at 1).  The step is one launch over a device table of the trainable ranges of the flat
buffer (cvk_adamw_step_ranges): frozen parameters and their moments are neither read nor written.

Gradient clipping: `FlatAdamW(net, max_grad_norm=X, norm_type=2.0)` clips by the global norm inside the step.  A deterministic fp64
reduction over the exact gradient segments of the parameters that take the step (all groups together, as torch's clip is global) writes a
device record {total_norm, clip_coef}; the AdamW launch is handed that record and multiplies every gradient element by clip_coef on its
way into the update.  `.grad` is NOT rescaled — the one difference from the two-call idiom `clip_grad_norm_(...); opt.step()`,
which rewrites all gradients in place: after a clipped step `.grad` still holds what backward produced, `opt.grad_norm` its norm and
`opt.clip_coef` the factor the update applied.  `clip_grad_norm_` below is the stand-alone form with torch's contract (scaled `.grad`s).
Parameter gradients are fp32 in every mode (fp32, bf16 storage, split operands), so clipping is the same code under all of them.

Weight averaging: `FlatAdamW(net, ema_decay=d, ema_warmup=False)` keeps an exponential moving average of the parameters in one more flat
buffer, initialised to the weights the optimizer is built on (the convention of torch.optim.swa_utils.AveragedModel and timm).  The thread
of the AdamW kernel that has just stored an element's new value goes on to `ema += alpha * (p_new - ema)` with it (the `ema` buffer of
cvk_adamw_step_ranges: two more passes over the buffer instead of the three of a separate lerp, no launch, and inside the captured graph
of GraphedStep).
alpha = 1 - d, with warm-up 1 - min(d, (1 + k) / (10 + k)) at the k-th update (`ema_alpha`).  A parameter a step skips (frozen, no
gradient) keeps its average: one frozen from the start has an average equal to itself.  `with opt.swap_ema():` exchanges the weights and
the average for validation and saving (and tells the executor that its derived weights are stale); `opt.ema_state_dict()` is the
network's state_dict() with the averaged parameters, without a swap.  BatchNorm running statistics are NOT averaged: inside swap_ema()
and in ema_state_dict() they are the live ones, as with AveragedModel's default use_buffers=False; recomputing them is left to the user.

FlatSGD is the same machinery with torch.optim.SGD's update (momentum, dampening, Nesterov, coupled L2 weight decay; cvk_sgd_step_ranges):
the two classes share _FlatOptimizer and differ in what a record carries and in the launch.  What is said above of groups, frozen
parameters, clipping, the EMA and swap_ema() holds for both."""
import contextlib
import ctypes
import math

import numpy
import torch

from . import _lib, engine
from ._lib import check


def _block_params(net):
    from .modules import _Block
    out = []
    for m in net.modules():
        if isinstance(m, _Block):
            out.extend(m.block_params())
    return out


def _check_clip_options(max_norm, norm_type, what):
    """(max_norm or None, norm_type) as floats; ValueError for a negative / NaN max_norm or a norm_type other than 2 and infinity."""
    try:
        nt = float(norm_type)
    except (TypeError, ValueError):
        nt = float("nan")
    if not (nt == 2.0 or nt == math.inf):
        raise ValueError(f"{what}: norm_type {norm_type!r} is not implemented (2 and infinity are)")
    if max_norm is None:
        return None, nt
    mx = float(max_norm)
    if not mx >= 0.0:
        raise ValueError(f"{what}: max_norm {max_norm!r} must be >= 0")
    return mx, nt


def _check_ema_decay(decay, what):
    """ema_decay as a float in [0, 1), or None; ValueError for anything else (NaN included)."""
    if decay is None:
        return None
    try:
        d = float(decay)
    except (TypeError, ValueError):
        d = float("nan")
    if not 0.0 <= d < 1.0:
        raise ValueError(f"{what}: ema_decay {decay!r} must be in [0, 1)")
    return d


def ema_alpha(decay, warmup, k):
    """The weight 1 - d_k of the new parameters in the k-th EMA update (k counts the updates including this one, from 1), as the
    numpy.float32 the kernel takes: d_k = decay, with warm-up min(decay, (1 + k) / (10 + k)) so that the average follows the weights
    through the first steps.  Evaluated in double precision and rounded once."""
    d = float(decay)
    if warmup:
        k = int(k)
        d = min(d, (1.0 + k) / (10.0 + k))
    return numpy.float32(1.0 - d)


def norm_segments(pairs):
    """The segment table of a gradient norm: `pairs` = (offset, numel) of every parameter that has a gradient, in floats of the flat gradient
    buffer.  Sorted by offset; neighbours are merged only when the first ends exactly where the second begins, so no alignment padding
    (engine.layout_grads rounds every parameter up to 4 floats and the buffer is torch.empty) and no frozen parameter's segment is ever
    covered.  Overlapping entries are refused."""
    out = []
    for o, n in sorted((int(o), int(n)) for o, n in pairs):
        if n <= 0:
            continue
        if out and o < out[-1][0] + out[-1][1]:
            raise ValueError("norm_segments: overlapping gradient segments")
        if out and out[-1][0] + out[-1][1] == o:
            out[-1] = (out[-1][0], out[-1][1] + n)
        else:
            out.append((o, n))
    return out


def plan_segments(segments, n):
    """(host NormSegment array with its workgroups assigned, workgroup count) of `segments` = [(offset, length)] of a buffer of n floats
    (cvk_grad_norm_plan): the table of a norm, a scale or a fold.  `segments` must not be empty."""
    arr = (_lib.NormSegment * len(segments))(*[_lib.NormSegment(o, m, 0, 0) for o, m in segments])
    nb = _lib.load().cvk_grad_norm_plan(ctypes.addressof(arr), len(segments), n)
    if nb <= 0:
        check(nb if nb < 0 else -1, "cvk_grad_norm_plan")
    return arr, nb


class _NormPlan:
    """A planned segment table on the device, its workgroup count and the fp64 partials buffer of the reduction."""

    def __init__(self, segments, n, device):
        if not segments:
            raise RuntimeError("gradient norm: no parameter has a gradient")
        arr, nb = plan_segments(segments, n)
        self.nseg, self.n, self.blocks = len(segments), n, nb
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
        self.partials = torch.empty(nb, device=device, dtype=torch.float64)

    def norm(self, grad_ptr, norm_type, max_norm, rec, stream):
        check(_lib.load().cvk_grad_norm(grad_ptr, self.n, self.table.data_ptr(), self.nseg, self.blocks, norm_type, max_norm,
                                        self.partials.data_ptr(), rec.data_ptr(), stream), "cvk_grad_norm")

    def scale(self, grad_ptr, rec, stream):
        check(_lib.load().cvk_grad_scale(grad_ptr, self.n, self.table.data_ptr(), self.nseg, self.blocks, rec.data_ptr(), stream),
              "cvk_grad_scale")


_PLANS = {}             # clip_grad_norm_: (device, buffer floats, segments) -> _NormPlan
_PLANS_MAX = 16


def _dense(g):
    return g.is_contiguous() or (g.dim() == 4 and g.permute(0, 2, 3, 1).is_contiguous())


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False):
    """torch.nn.utils.clip_grad_norm_ (same signature, same return value: the total norm as a 0-dim fp32 device tensor; `.grad`s scaled in
    place by min(1, max_norm / (total_norm + 1e-6))) for a network, an iterable of parameters or one tensor.  Parameters without a gradient
    are skipped.  When the gradients are dense fp32 views of ONE device buffer — what backward of a UNet / SegNet of this package leaves:
    the executor's flat gradient buffer — it is three launches and no host synchronisation (unless error_if_nonfinite): the fp64 reduction
    over the exact segments, its finish, the in-place scale (cvk_grad_norm, cvk_grad_scale).  Any other gradient set goes to torch's own
    function.  Gradients are fp32 in the bf16 and split-operand modes too, so nothing differs there."""
    if isinstance(parameters, torch.nn.Module):
        parameters = parameters.parameters()
    elif isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    mx, nt = _check_clip_options(max_norm, norm_type, "clip_grad_norm_")
    if mx is None:
        raise ValueError("clip_grad_norm_: max_norm is required")
    grads = [p.grad for p in params]
    flat = bool(grads) and all(g.is_cuda and g.dtype == torch.float32 and _dense(g) for g in grads)
    if flat:
        st = grads[0].untyped_storage()
        flat = all(g.untyped_storage().data_ptr() == st.data_ptr() for g in grads) and len({id(g) for g in grads}) == len(grads)
    if not flat:
        return torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=norm_type, error_if_nonfinite=error_if_nonfinite)
    dev = grads[0].device
    n = st.nbytes() // 4
    segs = tuple(norm_segments((g.storage_offset(), g.numel()) for g in grads))
    key = (dev, n, segs)
    plan = _PLANS.get(key)
    if plan is None:
        if len(_PLANS) >= _PLANS_MAX:
            _PLANS.clear()
        plan = _PLANS[key] = _NormPlan(list(segs), n, dev)
    rec = torch.empty(2, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    plan.norm(st.data_ptr(), nt, mx, rec, stream)
    if error_if_nonfinite and not bool(torch.isfinite(rec[0])):
        raise RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot be clipped. "
                           "To disable this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")
    plan.scale(st.data_ptr(), rec, stream)
    return rec[0]


class _FlatOptimizer(torch.optim.Optimizer):
    """What FlatAdamW and FlatSGD share: the parameters re-homed into one flat buffer laid out like the executor's gradient buffer, group
    validation, the gradient buffer of a step (_flat_grad), norm plans and the clip record, the EMA buffer with swap_ema() and
    ema_state_dict(), the range table of a step and its device copies, the chunking over ADAMW_ARG_RECORDS, the state-dict frame.

    An update rule supplies its name, its record struct and state-dict key, and three things:
      _record_key(i, group)           what, besides the group, parameters must share to be updated by one record;
      _fill_record(group, i, addr)    write the 7-float record of `group` for parameter i (i None: record 0 of the captured log) at addr;
      _launch_ranges(...)             the launch over a planned range table, eager or captured.
    Around them: _count(idx) advances the per-parameter state of the parameters that take the step (after the range table was built, before
    the records are filled), _variant() is what the options as they are now choose among the rule's kernels beyond clip and EMA (a part of
    GraphedStep's signature), _rule_state() / _load_rule_state() are the rule's share of the state dict."""
    _NAME = None            # the class name the messages carry
    _STATE_KEY = None       # the optimizer's entry of state_dict()
    _HYPER = None           # ctypes struct of one record (7 floats)

    def __init__(self, net, defaults, groups, max_grad_norm, norm_type, ema_decay, ema_warmup):
        N = self._NAME
        self.max_grad_norm, self.norm_type = _check_clip_options(max_grad_norm, norm_type, N)
        self.ema_decay, self.ema_warmup = _check_ema_decay(ema_decay, N), bool(ema_warmup)
        params = _block_params(net)                       # execution order == the executor's flat parameter list
        if len(params) != len(list(net.parameters())):
            raise ValueError(f"{N} needs a network made only of conv+BN blocks (UNet / SegNet)")
        if groups is None:
            groups = params
        else:
            groups = [dict(g) for g in groups]
            for g in groups:
                if not isinstance(g, dict) or "params" not in g:
                    raise ValueError(f"{N}: groups= takes a list of dicts with a 'params' entry, like torch parameter groups")
                g["params"] = list(g["params"])
            seen = [id(p) for g in groups for p in g["params"]]
            if sorted(seen) != sorted(id(p) for p in params):
                raise ValueError(f"{N}: every parameter of the network must be in exactly one group")
        super().__init__(groups, defaults)
        self._plist = params
        self._offs, total = engine.layout_grads(params)
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError(f"{N}: move the network to the GPU first")
        self._flat = torch.zeros(total, device=dev, dtype=torch.float32)
        with torch.no_grad():
            for p, o in zip(params, self._offs):
                n = p.numel()
                seg = self._flat[o:o + n]
                if p.dim() == 4:                          # storage [Cout][3][3][Cin] == channels_last OIHW
                    co, ci, kh, kw = p.shape
                    view = seg.view(co, kh, kw, ci).permute(0, 3, 1, 2)
                else:
                    view = seg.view(p.shape)
                view.copy_(p)
                p.data = view                             # the module now owns a view of the flat buffer
        self._gbuf = None
        self._step = 0                                    # step() calls (the counter the captured step and schedulers see)
        self._tables = {}                                 # range table (host tuple) -> (device table, workgroups)
        self._clip_rec = torch.zeros(2, device=dev, dtype=torch.float32)    # {total_norm, clip_coef} of the last clipped step
        self._norm_plans = {}                             # segment table (host tuple) -> _NormPlan
        self._net = net
        self._ema = self._flat.clone() if self.ema_decay is not None else None    # the average starts at the initial weights
        self._ema_updates = 0                             # EMA updates made: its own counter (a resumed scheduler may set _step)
        self._swapped = False                             # inside swap_ema(): the flat buffer holds the average

    # ---- the update rule ------------------------------------------------------------------------------------------------------------
    def _record_key(self, i, group):
        raise NotImplementedError

    def _fill_record(self, group, i, addr):
        raise NotImplementedError

    def _launch_ranges(self, grad, table, nranges, nblocks, hyper, nrec, clipped, alpha, stream):
        raise NotImplementedError

    def _count(self, idx):
        pass

    def _variant(self):
        return ()

    def _rule_state(self):
        return {}

    def _load_rule_state(self, extra):
        pass

    # ---- clipping -------------------------------------------------------------------------------------------------------------------
    @property
    def grad_norm(self):
        """0-dim view of the device record: the gradient norm of the last clipped step (no host sync)."""
        return self._clip_rec[0]

    @property
    def clip_coef(self):
        """0-dim view of the device record: the factor the last clipped step applied to every gradient element."""
        return self._clip_rec[1]

    def _norm_plan(self, idx):
        """The norm's segment table over the parameters `idx`: exact (offset, numel) per parameter, never the padded step ranges."""
        segs = tuple(norm_segments((self._offs[i], self._plist[i].numel()) for i in idx))
        plan = self._norm_plans.get(segs)
        if plan is None:
            plan = self._norm_plans[segs] = _NormPlan(list(segs), self._flat.numel(), self._flat.device)
        return plan

    def _clip_options(self):
        return _check_clip_options(self.max_grad_norm, self.norm_type, self._NAME)

    # ---- the weight average ---------------------------------------------------------------------------------------------------------
    @property
    def ema_updates(self):
        """EMA updates made so far (steps in which something had a gradient, since construction or the loaded state)."""
        return self._ema_updates

    def _ema_options(self):
        """ema_decay as it is now (None without an EMA), checked; switching an EMA on or off after construction is refused."""
        d = _check_ema_decay(self.ema_decay, self._NAME)
        if (d is None) != (self._ema is None):
            raise RuntimeError(f"{self._NAME}: ema_decay was switched " + ("off" if d is None else "on") + " after construction; the EMA buffer "
                               + ("exists" if d is None else "was never allocated") + " — build the optimizer with the ema_decay it is to have "
                               "(the value itself may change between steps)")
        return d

    def _refuse_swapped(self, what):
        if self._swapped:
            raise RuntimeError(f"{what}: inside {self._NAME}.swap_ema() the network holds the averaged weights; leave the context before "
                               "training on")

    def _next_ema_alpha(self):
        """Count one EMA update and return its alpha (numpy.float32)."""
        self._ema_updates += 1
        return ema_alpha(self.ema_decay, self.ema_warmup, self._ema_updates)

    @contextlib.contextmanager
    def swap_ema(self):
        """Validate or save with the averaged weights: on entry the contents of the flat parameter buffer and of the EMA buffer are
        exchanged (the parameters stay views of the same memory, so net.parameters(), state_dict(), evaluate, predict, save_checkpoint
        all see the average) and the executor's derived weights are invalidated; on exit the same again.  BatchNorm running statistics
        are the live ones, not averaged.  step() and GraphedStep.replay() raise inside; nesting is refused."""
        if self._ema_options() is None:
            raise RuntimeError(f"{self._NAME}.swap_ema(): the optimizer keeps no EMA (ema_decay=None)")
        if self._swapped:
            raise RuntimeError(f"{self._NAME}.swap_ema(): already inside swap_ema()")
        self._check_homes()
        self._exchange_ema()
        self._swapped = True
        try:
            yield self
        finally:
            self._exchange_ema()
            self._swapped = False

    @torch.no_grad()
    def _exchange_ema(self):
        tmp = self._flat.clone()
        self._flat.copy_(self._ema)
        self._ema.copy_(tmp)
        engine._bump_epoch()          # the parameters changed behind the executor's back: derived weight tensors are stale

    @torch.no_grad()
    def ema_state_dict(self):
        """The network's state_dict() (same keys, shapes and memory layout) with every parameter replaced by a clone of its average.
        Buffers (BatchNorm running statistics) are the live ones.  No swap: safe between training steps."""
        if self._ema_options() is None:
            raise RuntimeError(f"{self._NAME}.ema_state_dict(): the optimizer keeps no EMA (ema_decay=None)")
        avg = self._flat if self._swapped else self._ema          # inside swap_ema() the average lives in the parameter buffer
        index = {id(p): i for i, p in enumerate(self._plist)}
        names = {name: index[id(p)] for name, p in self._net.named_parameters(remove_duplicate=False)}
        sd = self._net.state_dict()
        for k in sd:
            i = names.get(k)
            if i is None:
                continue
            p, o = self._plist[i], self._offs[i]
            seg = avg[o:o + p.numel()]
            if p.dim() == 4:
                co, ci, kh, kw = p.shape
                sd[k] = seg.view(co, kh, kw, ci).permute(0, 3, 1, 2).clone()     # preserve_format: channels_last, like the parameter
            else:
                sd[k] = seg.view(p.shape).clone()
        return sd

    # ---- one step's parameters, gradients and range table ---------------------------------------------------------------------------
    def _group_of(self):
        ids = {}
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                ids[id(p)] = gi
        return [ids[id(p)] for p in self._plist]

    def _trainable(self):
        """Indices (into the flat parameter list) of the parameters with a gradient: the ones a step updates."""
        return [i for i, p in enumerate(self._plist) if p.grad is not None]

    def _flat_grad(self, idx=None):
        """The executor's flat gradient buffer when every gradient of the parameters `idx` (default: those with a .grad) is the expected view
        of it, else a copy gathered from them.  Segments of other parameters are never read."""
        idx = self._trainable() if idx is None else idx
        if not idx:
            raise RuntimeError(f"{self._NAME}.step(): gradients missing")
        p0, o0 = self._plist[idx[0]], self._offs[idx[0]]
        base = p0.grad.data_ptr() - 4 * o0
        ok = all(self._plist[i].grad.data_ptr() == base + 4 * self._offs[i] for i in idx)
        if ok:
            st = p0.grad.untyped_storage()
            start = (base - st.data_ptr()) // 4
            if base >= st.data_ptr() and (start + self._flat.numel()) * 4 <= st.nbytes():
                return torch.empty(0, device=p0.device, dtype=torch.float32).set_(st, start, (self._flat.numel(),))
        if self._gbuf is None:
            self._gbuf = torch.zeros_like(self._flat)
        for i in idx:
            p, o = self._plist[i], self._offs[i]
            g = p.grad.permute(0, 2, 3, 1) if p.dim() == 4 else p.grad
            self._gbuf[o:o + p.numel()].view(g.shape).copy_(g)
        return self._gbuf

    def _ranges(self, idx):
        """(records, ranges) of one step over the parameters `idx`: records = [(group, a parameter the record stands for)], one per
        distinct (group, _record_key); ranges = [(offset, length, record)] in flat-buffer order, neighbours of one record merged across the
        16-byte alignment padding between them (all parameters trainable in one group with one key: the single range [0, total))."""
        gof = self._group_of()
        recs, rix, ranges = [], {}, []
        for i in sorted(idx, key=lambda i: self._offs[i]):
            k = (gof[i], self._record_key(i, gof[i]))
            if k not in rix:
                rix[k] = len(recs)
                recs.append((gof[i], i))
            o, n = self._offs[i], (self._plist[i].numel() + 3) // 4 * 4
            if ranges and ranges[-1][2] == rix[k] and ranges[-1][0] + ranges[-1][1] == o:
                ranges[-1] = (ranges[-1][0], ranges[-1][1] + n, rix[k])
            else:
                ranges.append((o, n, rix[k]))
        return recs, ranges

    def _fill(self, recs, out):
        """Write the records of `recs` into `out` (a host array of the rule's record struct or a pinned float tensor of 7 floats per
        record): every group's options as they are now and what the rule keeps per parameter (_fill_record)."""
        base = out.data_ptr() if isinstance(out, torch.Tensor) else ctypes.addressof(out)
        size = ctypes.sizeof(self._HYPER)
        for r, (gi, i) in enumerate(recs):
            self._fill_record(gi, i, base + r * size)

    def _table(self, ranges, nrec):
        """The device copy of a planned range table (cached per table) and its workgroup count."""
        key = (tuple(ranges), nrec)
        ent = self._tables.get(key)
        if ent is None:
            lib = _lib.load()
            arr = (_lib.AdamwRange * len(ranges))(*[_lib.AdamwRange(o, n, r, 0) for o, n, r in ranges])
            nb = lib.cvk_adamw_plan_ranges(ctypes.addressof(arr), len(ranges), self._flat.numel(), nrec)
            if nb <= 0:
                check(nb if nb < 0 else -1, "cvk_adamw_plan_ranges")
            dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self._flat.device)
            ent = self._tables[key] = (dev, nb)
        return ent

    def _check_homes(self):
        """The module must still read its weights from the flat buffer: net.to()/.cuda()/.float() after construction
        re-homes p.data and step() would then update memory nobody reads."""
        base = self._flat.data_ptr()
        for p, o in zip(self._plist, self._offs):
            if p.data_ptr() != base + 4 * o:
                raise RuntimeError(f"{self._NAME}: a parameter no longer lives in the optimizer's flat buffer (the network was "
                                   f"moved or cast after the optimizer was built); construct {self._NAME} after net.to(device)")

    # ---- optimizer state: the rule's buffers and counters travel with state_dict() like torch's do ------------------------------------
    def state_dict(self):
        sd = super().state_dict()           # param_groups: every group's options and its members
        own = {"step": self._step}
        own.update(self._rule_state())
        own.update(offsets=list(self._offs), max_grad_norm=self.max_grad_norm, norm_type=self.norm_type)
        if self._ema is not None:
            self._refuse_swapped(f"{self._NAME}.state_dict()")
            own.update(ema=self._ema.clone(), ema_decay=self.ema_decay, ema_warmup=self.ema_warmup, ema_updates=self._ema_updates)
        sd[self._STATE_KEY] = own
        return sd

    def load_state_dict(self, state_dict):
        """With an EMA: the saved average, decay, warm-up flag and update count are restored; a state saved without them re-initialises the
        average from the parameters as they are now (load the network first) and sets the count to 0.  Without one they are ignored."""
        N = self._NAME
        self._refuse_swapped(f"{N}.load_state_dict()")
        state_dict = dict(state_dict)
        extra = state_dict.pop(self._STATE_KEY, None)
        super().load_state_dict(state_dict)
        if extra is not None:
            if list(extra["offsets"]) != list(self._offs):
                raise ValueError(f"{N}.load_state_dict: the saved state belongs to a different network layout")
            self._load_rule_state(extra)
            self._step = int(extra["step"])
            if "max_grad_norm" in extra:    # absent in a state dict saved before clipping existed: the constructor's options stay
                self.max_grad_norm, self.norm_type = _check_clip_options(extra["max_grad_norm"], extra.get("norm_type", 2.0),
                                                                         f"{N}.load_state_dict")
        if self._ema is not None:
            if extra is not None and "ema" in extra:
                if extra["ema"].numel() != self._ema.numel():
                    raise ValueError(f"{N}.load_state_dict: the saved EMA belongs to a different network layout")
                self._ema.copy_(extra["ema"])
                self.ema_decay = _check_ema_decay(extra["ema_decay"], f"{N}.load_state_dict")
                if self.ema_decay is None:
                    raise ValueError(f"{N}.load_state_dict: the saved state carries an EMA without a decay")
                self.ema_warmup, self._ema_updates = bool(extra["ema_warmup"]), int(extra["ema_updates"])
            else:
                self._ema.copy_(self._flat)
                self._ema_updates = 0

    @torch.no_grad()
    def step(self, closure=None):
        self._refuse_swapped(f"{self._NAME}.step()")
        loss = closure() if closure is not None else None
        self._check_homes()
        ema = self._ema_options()
        idx = self._trainable()
        if not idx:                   # as torch: nothing has a gradient, nothing changes (and the EMA counts no update)
            return loss
        max_norm, norm_type = self._clip_options()
        recs, ranges = self._ranges(idx)
        self._step += 1
        self._count(idx)
        grad = self._flat_grad(idx)
        stream = torch.cuda.current_stream(self._flat.device).cuda_stream
        alpha = self._next_ema_alpha() if ema is not None else None          # every chunk with the update's one alpha
        if max_norm is not None:      # one norm over everything that takes this step, all groups together: reduction + finish
            self._norm_plan(idx).norm(grad.data_ptr(), norm_type, max_norm, self._clip_rec, stream)
        # the records travel as kernel arguments: one launch per CVK_ADAMW_ARG_RECORDS distinct records
        for c0 in range(0, len(recs), _lib.ADAMW_ARG_RECORDS):
            crecs = recs[c0:c0 + _lib.ADAMW_ARG_RECORDS]
            cranges = [(o, n, r - c0) for o, n, r in ranges if c0 <= r < c0 + len(crecs)]
            hyper = (self._HYPER * len(crecs))()
            self._fill(crecs, hyper)
            table, nb = self._table(cranges, len(crecs))
            self._launch_ranges(grad, table, len(cranges), nb, hyper, len(crecs), max_norm is not None, alpha, stream)
        engine._bump_epoch()          # the kernel wrote the parameters through raw pointers: derived weight tensors are stale
        return loss


class FlatAdamW(_FlatOptimizer):
    _NAME, _STATE_KEY, _HYPER = "FlatAdamW", "flat_adamw", _lib.AdamwHyper

    def __init__(self, net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, groups=None, max_grad_norm=None, norm_type=2.0,
                 ema_decay=None, ema_warmup=False):
        super().__init__(net, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), groups, max_grad_norm, norm_type, ema_decay,
                         ema_warmup)
        self._m = torch.zeros_like(self._flat)
        self._v = torch.zeros_like(self._flat)
        self._steps = [0] * len(self._plist)              # per parameter, as torch.optim.AdamW's state[p]["step"]

    def _record_key(self, i, group):
        """One record per (group, step count): a block unfrozen late starts its bias correction at 1."""
        return self._steps[i]

    def _count(self, idx):
        for i in idx:
            self._steps[i] += 1

    def _fill_record(self, group, i, addr):
        """The group's options as they are now and the bias corrections of parameter i's step count (cvk_adamw_hyper_fill); the log's record
        (i None) carries those of the step() count."""
        g = self.param_groups[group]
        check(_lib.load().cvk_adamw_hyper_fill(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                               float(g["weight_decay"]), self._step if i is None else self._steps[i], addr),
              "cvk_adamw_hyper_fill")

    def _launch_ranges(self, grad, table, nranges, nblocks, hyper, nrec, clipped, alpha, stream):
        """One AdamW launch over a planned range table (device tensor `table`, `nranges` entries, `nblocks` workgroups) with the gradient
        buffer `grad`.  `hyper`: the `nrec` records, a host AdamwHyper array (eager: cvk_adamw_step_ranges) or the address of device records
        (captured: cvk_adamw_step_ranges_dev).  `clipped`: the gradient is scaled by the optimizer's {total_norm, clip_coef} record.
        `alpha`: None without an EMA; else the update's weight, a host float (eager) or (device address, host value) (captured)."""
        lib = _lib.load()
        head = (self._flat.data_ptr(), grad.data_ptr(), self._m.data_ptr(), self._v.data_ptr(),
                self._ema.data_ptr() if alpha is not None else None, self._flat.numel(), table.data_ptr(), nranges, nblocks)
        rec = self._clip_rec.data_ptr() if clipped else None
        if isinstance(hyper, ctypes.Array):
            check(lib.cvk_adamw_step_ranges(*head, ctypes.addressof(hyper), nrec, rec, 0.0 if alpha is None else float(alpha), stream),
                  "cvk_adamw_step_ranges")
        else:
            adev, ahost = (None, 0.0) if alpha is None else alpha
            check(lib.cvk_adamw_step_ranges_dev(*head, hyper, nrec, rec, adev, float(ahost), stream), "cvk_adamw_step_ranges_dev")

    # exp_avg / exp_avg_sq / step travel with state_dict() like torch.optim.AdamW's do
    def _rule_state(self):
        return {"steps": list(self._steps), "exp_avg": self._m.clone(), "exp_avg_sq": self._v.clone()}

    def _load_rule_state(self, extra):
        if extra["exp_avg"].numel() != self._m.numel():
            raise ValueError("FlatAdamW.load_state_dict: the saved state belongs to a different network layout")
        steps = extra.get("steps")          # absent in the single-step format: every parameter took every step
        steps = [int(s) for s in steps] if steps is not None else [int(extra["step"])] * len(self._plist)
        if len(steps) != len(self._plist):
            raise ValueError("FlatAdamW.load_state_dict: the saved step counts belong to a different network layout")
        self._steps = steps
        self._m.copy_(extra["exp_avg"]); self._v.copy_(extra["exp_avg_sq"])


def _f32(x):
    """A hyper-parameter as the kernel sees it: rounded to float32."""
    return float(numpy.float32(x))


class FlatSGD(_FlatOptimizer):
    """torch.optim.SGD semantics (momentum, dampening, Nesterov, coupled L2 weight decay) as one fused launch over the flat buffers
    (cvk_sgd_step_ranges): everything FlatAdamW documents above — groups and frozen parameters, clipping inside the step, the weight EMA with
    swap_ema(), GraphedStep capture, accumulation — with the second update rule.  Every group's lr / momentum / dampening / weight_decay /
    nesterov are read at every step, so OneCycleLR (which cycles the momentum by default) and PolynomialLR drive it unchanged.

    As torch, a parameter gets its momentum buffer at its first step under a non-zero momentum, and that step copies the (decayed) gradient
    into it instead of applying the dampening.  The optimizer keeps one flag per parameter for it; a step's records are keyed by
    (group, has buffer), so a range table has at most two records per group and stops changing after the first step.  The flat momentum
    buffer exists from the constructor on when any group's momentum is non-zero, else from the first eager step that needs it; while every
    group's momentum is 0 the buffer-free kernel runs (3 passes over the parameters instead of 5)."""
    _NAME, _STATE_KEY, _HYPER = "FlatSGD", "flat_sgd", _lib.SgdHyper

    def __init__(self, net, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, groups=None, max_grad_norm=None,
                 norm_type=2.0, ema_decay=None, ema_warmup=False):
        if not lr >= 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not momentum >= 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if not weight_decay >= 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(net, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov), groups,
                         max_grad_norm, norm_type, ema_decay, ema_warmup)
        self._buf = None                                  # the flat momentum buffer
        self._has_buf = [False] * len(self._plist)        # per parameter: torch's `momentum_buffer is not None`
        self._fresh = frozenset()                         # the parameters whose buffer the step being launched initialises
        self._buffer()

    def _buffer(self):
        """The flat momentum buffer when any group's momentum is non-zero now (allocated on first need), else None: the buffer-free kernel."""
        if not any(_f32(g["momentum"]) != 0.0 for g in self.param_groups):
            return None
        if self._buf is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FlatSGD: the momentum buffer cannot be allocated inside a graph capture")
            self._buf = torch.zeros_like(self._flat)
        return self._buf

    def _variant(self):
        """(momentum buffer in use,): fixed at a capture.  Also makes sure that the buffer exists before one begins."""
        return (self._buffer() is not None,)

    def _record_key(self, i, group):
        return self._has_buf[i]

    def _count(self, idx):
        """torch's rule: a parameter that takes a step while its group's momentum is non-zero has a buffer from then on."""
        mom = [_f32(g["momentum"]) != 0.0 for g in self.param_groups]
        fresh = []
        if any(mom) and not all(self._has_buf[i] for i in idx):
            gof = self._group_of()
            fresh = [i for i in idx if mom[gof[i]] and not self._has_buf[i]]
        for i in fresh:
            self._has_buf[i] = True
        self._fresh = frozenset(fresh)

    def _fill_record(self, group, i, addr):
        """The group's options as they are now and whether parameter i's buffer is initialised by this step (cvk_sgd_hyper_fill); the log's
        record (i None) only lends its lr and momentum."""
        g = self.param_groups[group]
        check(_lib.load().cvk_sgd_hyper_fill(float(g["lr"]), float(g["momentum"]), float(g["dampening"]), float(g["weight_decay"]),
                                             int(bool(g["nesterov"])), int(i in self._fresh), addr), "cvk_sgd_hyper_fill")

    def _launch_ranges(self, grad, table, nranges, nblocks, hyper, nrec, clipped, alpha, stream):
        """One SGD launch over a planned range table; the arguments are FlatAdamW._launch_ranges' (cvk_sgd_step_ranges eager,
        cvk_sgd_step_ranges_dev captured).  The momentum buffer is handed over while any group's momentum is non-zero."""
        lib = _lib.load()
        buf = self._buffer()
        head = (self._flat.data_ptr(), grad.data_ptr(), buf.data_ptr() if buf is not None else None,
                self._ema.data_ptr() if alpha is not None else None, self._flat.numel(), table.data_ptr(), nranges, nblocks)
        rec = self._clip_rec.data_ptr() if clipped else None
        if isinstance(hyper, ctypes.Array):
            check(lib.cvk_sgd_step_ranges(*head, ctypes.addressof(hyper), nrec, rec, 0.0 if alpha is None else float(alpha), stream),
                  "cvk_sgd_step_ranges")
        else:
            adev, ahost = (None, 0.0) if alpha is None else alpha
            check(lib.cvk_sgd_step_ranges_dev(*head, hyper, nrec, rec, adev, float(ahost), stream), "cvk_sgd_step_ranges_dev")

    def _rule_state(self):
        return {"has_buffer": list(self._has_buf), "momentum_buffer": self._buf.clone() if self._buf is not None else None}

    def _load_rule_state(self, extra):
        flags, buf = [bool(f) for f in extra["has_buffer"]], extra["momentum_buffer"]
        if len(flags) != len(self._plist) or (buf is not None and buf.numel() != self._flat.numel()):
            raise ValueError("FlatSGD.load_state_dict: the saved state belongs to a different network layout")
        if buf is None and any(flags):
            raise ValueError("FlatSGD.load_state_dict: the saved state flags momentum buffers but carries none")
        self._has_buf = flags
        if buf is not None:
            if self._buf is None:
                self._buf = torch.zeros_like(self._flat)
            self._buf.copy_(buf)
        self._buffer()                      # the loaded groups may need one the constructor's did not
