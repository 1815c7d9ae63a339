"""GradAccumulator — gradient accumulation over micro-batches inside the executor's flat gradient buffer.

Training with an effective batch larger than what fits in one pass: `steps` forward/backward passes ("micro-steps") per optimizer
update.  The executor writes every parameter gradient of a pass into ONE fresh flat fp32 buffer with a fixed layout
(engine.layout_grads); the accumulator folds those buffers with one streaming launch per micro-step (cvk_grad_accumulate) instead of the
~100 `add_` launches autograd runs when `.grad` already exists, lets the data-parallel exchange run once per update instead of once per
micro-batch, and lets a whole window be captured as one graph (GraphedStep(..., accumulator=acc)).

    acc = cvk.GradAccumulator(net, steps=4, mean=True)     # net: UNet / SegNet of this package, or ddp.DataParallel around one
    opt = cvk.FlatAdamW(net, lr=5e-4, max_grad_norm=1.0)   # or torch.optim.AdamW: the accumulator does not care
    for x, t in loader:
        loss_fn(net(x), t).backward()
        if acc.ready:                                      # True after the steps-th backward of a window
            opt.step(); sched.step(); opt.zero_grad(set_to_none=True)

Micro-steps 1 .. steps-1 of a window fold the pass's fresh buffer into the accumulator's own persistent buffer (`acc = g`, then
`acc = acc + g`) and return None for every parameter gradient — the mechanism frozen parameters use — so `.grad` stays None, optimizer
steps are the no-ops they already are for parameters without a gradient, and no collective is issued.  The last micro-step folds the
accumulator INTO the fresh buffer of that pass, `g = (g + acc) * scale` with scale = 1/steps (mean=True) or 1, and hands out views of
it as every backward does: the bucketed all-reduce, clip_grad_norm_, the clip norm inside FlatAdamW, the AdamW launch and the log row run
unchanged on one flat buffer that holds the window's mean (or sum).  Per element the sum order is fixed, ((g1 + g2) + g3) + ..., every
add and the final multiply are single correctly rounded fp32 operations, and there are no atomics: the result is bitwise the same
expression in torch fp32, run to run, eager or captured.  The accumulator's buffer is never handed to autograd.

Do not divide the loss by `steps`: mean=True does it, after the sum, in one rounding.  The gradient of the network INPUT
(x.requires_grad) is returned on every micro-step as without an accumulator and is not accumulated.  BatchNorm running statistics are
updated per micro-batch, as torch updates them.  Input geometries may differ inside a window (the layout depends on the parameters
only); what trains may not: a requires_grad flip or a change of a block's BatchNorm mode in the middle of a window is refused by name
(between windows it is fine).  Parameter gradients are fp32 in the same flat layout in the bf16-storage mode and with
set_split_operands, so the same code serves all three.  There is no state_dict(): take checkpoints between windows, where the
accumulator holds nothing.  `steps=1` or `detach()` restores the executor's behaviour without an accumulator exactly (same launches,
same buffers)."""
import torch

from . import _lib
from ._lib import check
from .optim import norm_segments, plan_segments


def fold_segments(plan, params, goffs):
    """The segment table of a fold: exact (offset, numel) of every parameter the plan trains, merged where contiguous (optim.norm_segments)
    — the norm table of the trainable parameters.  Frozen segments and alignment padding are never covered."""
    pairs = []
    for i, p in enumerate(params):
        op = plan.convs[i // 4]
        if (op.w_req, op.b_req, op.g_req, op.be_req)[i % 4]:
            pairs.append((goffs[i], p.numel()))
    return norm_segments(pairs)


def clip_segments(segments, lo, hi):
    """`segments` intersected with [lo, hi) of the flat buffer: the fold table of one data-parallel bucket."""
    out = []
    for o, n in segments:
        a, b = max(o, lo), min(o + n, hi)
        if b > a:
            out.append((a, b - a))
    return out


def window_key(plan, params, total, device):
    """What must stay the same inside one window: the layout, the device, and per block which parameters train and its BatchNorm mode."""
    return (int(total), str(device), tuple((op.w_req, op.b_req, op.g_req, op.be_req, op.bn_train) for op in plan.convs),
            tuple(op.label for op in plan.convs))


def _describe_change(old, new):
    if old[0] != new[0] or old[1] != new[1] or len(old[2]) != len(new[2]):
        return "the parameter layout or the device changed"
    names = ("requires_grad of the conv weight", "requires_grad of the conv bias", "requires_grad of the BatchNorm weight",
             "requires_grad of the BatchNorm bias", "the BatchNorm mode (train / eval)")
    for a, b, label in zip(old[2], new[2], new[3]):
        for j in range(5):
            if a[j] != b[j]:
                return f"{names[j]} of {label} changed"
    return "the set of blocks changed"


class _Table:
    """A planned segment table on the device and its workgroup count (cvk_grad_norm_plan)."""

    def __init__(self, segments, n, device):
        arr, self.blocks = plan_table(segments, n)
        self.nseg, self.n = len(segments), n
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


def plan_table(segments, n):
    """(host NormSegment array with its workgroups assigned, workgroup count) of a fold over `segments` of a buffer of n floats."""
    if not segments:
        raise RuntimeError("GradAccumulator: no parameter of the network trains")
    return plan_segments(segments, n)


class _Fold:
    """One backward pass inside a window (engine.Runner.backward): which way this pass folds, and the launches."""

    def __init__(self, acc, mode, closing, segments, total):
        self.acc, self.mode, self.closing, self.segments, self.total = acc, mode, closing, segments, total
        self.folded = []            # (lo, hi) of the bucket folds of a closing pass under data parallel (introspection / tests)

    def _launch(self, st, table):
        acc = self.acc
        buf = acc._buffer(self.total, st.gflat.device)
        dst, src = (st.gflat, buf) if self.closing else (buf, st.gflat)
        check(_lib.load().cvk_grad_accumulate(dst.data_ptr(), src.data_ptr(), self.total, table.table.data_ptr(), table.nseg, table.blocks,
                                              self.mode, acc.scale if self.closing else 1.0, st.stream), "cvk_grad_accumulate")
        acc.launches += 1

    def whole(self, st):
        """One launch over the whole table, after the parameter gradients of the pass are complete."""
        self._launch(st, self.acc._table(tuple(self.segments), self.total, st.gflat.device))

    def bucket(self, st, lo, hi):
        """Closing pass under data parallel: fold [lo, hi) immediately before the bucket leaves for the all-reduce."""
        assert self.closing
        segs = tuple(clip_segments(self.segments, lo, hi))
        self.folded.append((lo, hi))
        if segs:
            self._launch(st, self.acc._table(segs, self.total, st.gflat.device))

    def done(self):
        self.acc._pass_done(self)


class GradAccumulator:
    def __init__(self, net, steps, mean=True):
        from . import ddp
        from .modules import runner_of
        module = net.module if isinstance(net, ddp.DataParallel) else net
        self._steps = self._check_steps(steps)
        self.mean = bool(mean)
        R = runner_of(module)
        if R.accumulator is not None:
            raise RuntimeError("GradAccumulator: this network already has an accumulator attached (detach() it first)")
        R.accumulator = self
        self._runner, self.module = R, module
        self._count = 0             # micro-batches folded into the open window
        self._ready = False
        self._key = None
        self._buf = None
        self._tables = {}           # (segments, total, device) -> _Table
        self.launches = 0           # cvk_grad_accumulate launches issued so far (tests / diagnostics)

    @staticmethod
    def _check_steps(steps):
        if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
            raise ValueError(f"GradAccumulator: steps must be an integer >= 1, got {steps!r}")
        return int(steps)

    @property
    def steps(self):
        return self._steps

    @steps.setter
    def steps(self, value):
        value = self._check_steps(value)
        if self._count and value != self._steps:
            raise RuntimeError(f"GradAccumulator: steps cannot change in the middle of a window ({self._count} of {self._steps} micro-steps "
                               "done); reset() drops the partial window")
        self._steps = value

    @property
    def scale(self):
        return 1.0 / self._steps if self.mean else 1.0

    @property
    def ready(self):
        """The last backward closed a window: `.grad` holds the window's mean (or sum) and the optimizer may step."""
        return self._ready

    @property
    def micro_step(self):
        """0-based position inside the window of the NEXT backward (= micro-batches folded so far; 0 between windows)."""
        return self._count

    @property
    def attached(self):
        return self._runner is not None and self._runner.accumulator is self

    def reset(self):
        """Drop a partial window (an epoch's end): the next backward starts a new one.  The buffer is kept; it never needs zeroing."""
        self._count, self._ready, self._key = 0, False, None

    def detach(self):
        """Take the accumulator off the network: backward behaves as it did before (same launches, same buffers)."""
        if self.attached:
            self._runner.accumulator = None
        self.reset()
        self._buf = None
        self._tables.clear()

    # ---- the executor's side (engine.Runner.backward) --------------------------------------------------------------------------------
    def open_pass(self, st, plan, total):
        """Called once per backward pass before any gradient is written.  None: steps == 1, the pass runs as without an accumulator."""
        if self._steps == 1:
            self._ready = True
            return None
        dev = st.gflat.device if getattr(st, "gflat", None) is not None else getattr(st, "device", None)
        key = window_key(plan, st.params, total, dev)
        if self._count and key != self._key:
            raise RuntimeError(f"GradAccumulator: what trains changed in the middle of a window (micro-step {self._count} of "
                               f"{self._steps}): {_describe_change(self._key, key)}.  Change it between windows, or reset() first")
        self._key = key
        closing = self._count == self._steps - 1
        mode = 2 if closing else (0 if self._count == 0 else 1)
        self._ready = False
        return _Fold(self, mode, closing, fold_segments(plan, st.params, st.goffs), total)

    def _pass_done(self, fold):
        if fold.closing:
            self._count, self._ready, self._key = 0, True, None
        else:
            self._count += 1

    def _buffer(self, total, device):
        if self._buf is None or self._buf.numel() != total or self._buf.device != device:
            self._buf = torch.empty(total, device=device, dtype=torch.float32)
        return self._buf

    def _table(self, segments, total, device):
        key = (segments, total, str(device))
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = _Table(list(segments), total, device)
        return t
