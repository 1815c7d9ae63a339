"""The training step as ONE captured HIP graph.

A step of the path is ~500 kernel launches enqueued from Python through ctypes (11-15 ms of host time per step: hidden while
the GPU needs 38 ms for the fp32 headline, the next wall for the bf16 configuration and a jitter source for 8 single-threaded
ranks).  The executor's plan is static per input geometry, every launch goes to the current HIP stream and nothing in the step
synchronises with the host, so `zero_grad -> net(x) -> loss -> backward` (reference train.py:124-131) can be captured once
with torch.cuda.CUDAGraph and replayed with a single launch: activations, saved tensors, the flat gradient buffer and the
workspace come from the graph's private pool, i.e. their addresses are the same in every replay.

    step = GraphedStep(net, lossf, x, t)       # x, t: example batch of the geometry (copied into static buffers)
    for xb, tb in loader:
        loss = step.replay(xb, tb)             # p.grad of every parameter now holds this batch's gradients
        optimizer.step()

BatchNorm running statistics and num_batches_tracked are updated by the kernels on the device, exactly as in eager mode.
Data parallel (round 4): RCCL collectives are stream-capturable, so a step of a ddp.DataParallel network is captured WITH its
bucketed all-reduces (`GraphedStep(dp_net.module, ..., allow_grad_sync=True)`): every rank replays the same graph, the
collectives run on RCCL's stream inside it, and 8 single-threaded ranks no longer sit on 11-15 ms of Python enqueue per step.
gloo groups (CPU rehearsals) cannot be captured.

The whole iteration (train.py:124-150): with `optimizer=` (a FlatAdamW or a FlatSGD; what follows says AdamW and holds for both, with the
SGD records carrying lr / momentum / dampening / weight decay / nesterov and a "first step" flag per record where AdamW's carry the bias
corrections, and log column 2 the momentum instead of beta1) the graph also runs the optimizer step after backward (after
the captured all-reduces under data parallel), and with `log_capacity=` it ends in one launch that appends the reference's log
line [loss, lr, beta1, ||last weight grad||, ||last bias grad||] to a device ring.  lr, betas, eps and weight decay of every parameter
group are read at every replay, the bias corrections computed on the host and uploaded into device records the graph reads (one per
group and step count, cvk_adamw_step_ranges_dev; the log row reads param_groups[0], as the reference prints), so a scheduler drives the
captured optimizer as it drives the eager one.  A FlatAdamW with `max_grad_norm` is captured with its norm reduction and finish between
backward and the AdamW launch (after the stream's waits for the all-reduces: every rank reduces the same averaged buffer, so no extra
collective), and the log rows gain the global norm and the clip coefficient; `max_grad_norm` / `norm_type` are baked into the graph.
A FlatAdamW with `ema_decay` is captured with its `ema` buffer in the same launch: the update's alpha travels with the hyper records, one
float behind them, so the decay may change between replays and warm-up changes it on every one; whether an EMA exists
is baked in.  Under `accumulator=` the average takes one update per window; under data parallel every rank averages the same parameters.
Frozen parameters (requires_grad False, BatchNorm children in eval mode) are captured as
they are when the GraphedStep is built; replay() refuses to run after any of that changes:

    opt = FlatAdamW(net, lr=...); sched = OneCycleLR(opt, ...)
    step = GraphedStep(net, lossf, x, t, optimizer=opt, scheduler=sched, log_capacity=len(loader))
    for epoch in ...:
        for xb, tb in loader:
            step.replay(xb, tb)                # one graph launch per iteration, no host sync
        rows, dropped = step.log()             # one D2H copy per epoch

Gradient accumulation: with `accumulator=` (the GradAccumulator attached to the network) the graph holds a whole window.  `x` and `t`
carry a leading window axis (`x: [steps, N, 3, H, W]`, `t: [steps, N, H, W]`); the capture runs the `steps` forward / loss / backward
passes back to back (each with its cvk_grad_accumulate launch), then the tail above once.  `step.loss` and the log row's loss column
are `torch.stack(micro_losses).mean()`, computed on the device inside the graph; the log gets one row per update and the scheduler
steps once per replay.  The accumulator's identity, `steps` and `mean` are baked in.  Not together with allow_grad_sync=True.
"""
import ctypes

import torch

from . import _lib, engine
from ._lib import check
from .optim import ema_alpha as _ema_alpha

HYPER_BYTES = ctypes.sizeof(_lib.AdamwHyper)   # include/cvk.h cvk_adamw_hyper: all floats; cvk_sgd_hyper has the same size with lr and
HYPER_FLOATS = HYPER_BYTES // 4                # momentum in floats 0 and 1
HYPER_SLOTS = 32                         # pinned staging records: the host may run this many replays ahead of the GPU before it waits


def last_layer_params(net):
    """(name, parameter) of the last parameter whose name contains 'weight' and of the last whose name contains 'bias', in
    named_parameters() order: the reference's utils._get_lastlayer_params (utils.py:15-30)."""
    w = b = None
    for name, p in net.named_parameters():
        if "weight" in name:
            w = (name, p)
        if "bias" in name:
            b = (name, p)
    return w, b


class GraphedStep:
    def __init__(self, net, lossf, x, t, warmup=2, allow_grad_sync=False, *, optimizer=None, scheduler=None, log_capacity=0, accumulator=None):
        from .modules import runner_of
        from .optim import _FlatOptimizer
        if optimizer is not None and not isinstance(optimizer, _FlatOptimizer):
            raise TypeError(f"GraphedStep: only FlatAdamW and FlatSGD can be captured with the step, not {type(optimizer).__name__}; step "
                            "other optimizers after replay()")
        if scheduler is not None and optimizer is None:
            raise ValueError("GraphedStep: a scheduler needs the captured optimizer it drives (optimizer=)")
        if scheduler is not None and getattr(scheduler, "optimizer", optimizer) is not optimizer:
            raise ValueError("GraphedStep: the scheduler drives another optimizer")
        log_capacity = int(log_capacity)
        if log_capacity < 0:
            raise ValueError("GraphedStep: log_capacity must be >= 0")
        if log_capacity and optimizer is None:
            raise ValueError("GraphedStep: the log records the step's lr and beta1: it needs optimizer=")
        if optimizer is not None:
            if {id(p) for p in optimizer._plist} != {id(p) for p in net.parameters()}:
                raise ValueError("GraphedStep: the optimizer was built for another network")
            optimizer._check_homes()
        R = runner_of(net)
        if accumulator is not None:
            if allow_grad_sync:
                raise NotImplementedError("GraphedStep: accumulator= together with allow_grad_sync=True is not supported (a window with "
                                          "captured collectives); run data-parallel accumulation in eager mode")
            if R.accumulator is not accumulator:
                raise ValueError("GraphedStep: accumulator= must be the GradAccumulator attached to this network")
            if accumulator.micro_step:
                raise RuntimeError("GraphedStep: the accumulator is in the middle of a window; reset() it or finish the window first")
            if x.dim() != 5 or t.dim() != 4 or x.shape[0] != accumulator.steps or t.shape[0] != accumulator.steps:
                raise ValueError(f"GraphedStep: with accumulator= the batch carries a leading window axis: x [steps, N, C, H, W], "
                                 f"t [steps, N, H, W] with steps = {accumulator.steps}; got {tuple(x.shape)}, {tuple(t.shape)}")
        elif R.accumulator is not None and R.accumulator.steps > 1:
            raise RuntimeError("GraphedStep: the network accumulates gradients over micro-batches (GradAccumulator); pass accumulator= to "
                               "capture a whole window")
        self.accumulator = accumulator
        if R.grad_sync is not None:
            if not allow_grad_sync:
                raise RuntimeError("GraphedStep: the network synchronises gradients (ddp.DataParallel); pass allow_grad_sync=True to "
                                   "capture the bucketed all-reduces with the step (RCCL only)")
            if not getattr(R.grad_sync, "_native_avg", False):
                raise RuntimeError("GraphedStep: only RCCL ('nccl') collectives can be captured; gloo groups run in eager mode")
        if not (x.is_cuda and t.is_cuda):
            raise RuntimeError("GraphedStep needs the example batch on the GPU")
        self.net, self.lossf = net, lossf
        self._runner = R
        self.optimizer, self.scheduler, self.log_capacity = optimizer, scheduler, log_capacity
        # what the captured graph bakes in: replay() refuses to run once any of it has changed
        self._sig = self._signature()
        self.x, self.t = x.clone(), t.clone()
        self.params = [p for p in net.parameters() if p.requires_grad]
        if optimizer is not None:
            # the parameters the captured step updates (those that receive a gradient) and its records: record 0 = param_groups[0] for the log,
            # then one per (group, record key) of the range table (_FlatOptimizer._ranges); rewritten before every replay from a ring of pinned slots
            self._opt_idx = [i for i, p in enumerate(optimizer._plist) if p.requires_grad]
            if not self._opt_idx:
                raise ValueError("GraphedStep: the optimizer has no trainable parameter to step")
            self._opt_recs, self._opt_ranges = optimizer._ranges(self._opt_idx)
            self._table, self._table_blocks = optimizer._table(self._opt_ranges, len(self._opt_recs))   # uploaded before the capture
            nrec = 1 + len(self._opt_recs)
            # with an EMA one more float behind the records: the update's alpha, uploaded by the same copy
            self._ema = optimizer._ema_options() is not None
            nfl = nrec * HYPER_FLOATS + (1 if self._ema else 0)
            self._hyper = torch.zeros(nfl, device=x.device, dtype=torch.float32)
            self._hyper_pin = torch.zeros(HYPER_SLOTS, nfl, dtype=torch.float32, pin_memory=True)
            self._hyper_busy = [None] * HYPER_SLOTS     # per slot: event after the H2D copy that READ it
            self._hyper_slot = 0
            # global-norm clipping (FlatAdamW(max_grad_norm=...)): the norm's segment table and partials are uploaded before the capture
            self._clip = optimizer._clip_options()
            self._norm_plan = optimizer._norm_plan(self._opt_idx) if self._clip[0] is not None else None
        self._log_cols = _lib.STEP_LOG_NORM_COLUMNS if optimizer is not None and self._clip[0] is not None else _lib.STEP_LOG_COLUMNS
        if log_capacity:
            # one buffer, so that log() is one D2H copy: int64 row counter, then capacity rows of _log_cols floats
            self._logbuf = torch.zeros(2 + log_capacity * self._log_cols, device=x.device, dtype=torch.float32)
            self._log_read = 0                  # rows the host has consumed
            (_, self._log_w), (_, self._log_b) = last_layer_params(net)
        cur = torch.cuda.current_stream(x.device)
        side = torch.cuda.Stream(device=x.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):               # warm-up off the capture: plans, workspace, allocator pools
            for _ in range(max(1, warmup)):
                self._zero()
                self._passes()
        cur.wait_stream(side)
        torch.cuda.synchronize(x.device)
        self._zero()
        self.graph = torch.cuda.CUDAGraph()
        # With a process group alive, ProcessGroupNCCL's watchdog thread polls the events of earlier collectives (hipEventQuery) at any
        # moment; under the default "global" capture mode such a call from ANOTHER thread fails with "operation not permitted when
        # stream is capturing" and the watchdog takes the process down (seen once in three full test runs).  "thread_local" restricts
        # the check to the capturing thread — what torch prescribes for capturing collectives.
        import torch.distributed as dist
        mode = "thread_local" if (R.grad_sync is not None or (dist.is_available() and dist.is_initialized())) else "global"
        if mode == "thread_local":
            # ... and the watchdog's list should be EMPTY when the capture begins: round 6 saw it die once in six suite runs with "operation not
            # permitted on an event last recorded in a capturing stream" (hipErrorCapturedEvent from WorkNCCL::isCompleted).  Every eager
            # collective has finished (synchronize above); three watchdog periods let the thread retire them before the first captured one exists.
            import time
            time.sleep(0.35)
        with torch.cuda.graph(self.graph, capture_error_mode=mode):
            self.loss = self._passes()
            if optimizer is not None or log_capacity:
                self._capture_tail(x.device)
        # every tensor a replay writes must stay alive as long as the graph: the gradients (views of the flat buffer the
        # capture allocated) and the runner's workspace (a later, larger eager call would otherwise release it)
        self.grads = [p.grad for p in self.params]
        self._keep = R._ws

    def _passes(self):
        """Forward, loss and backward of one iteration; returns the loss.  With an accumulator: the window's `steps` passes back to back and
        the mean of the micro-batch losses (device, fp32)."""
        if self.accumulator is None:
            loss = self.lossf(self.net(self.x), self.t)
            loss.backward()
            return loss
        losses = []
        for k in range(self.accumulator.steps):
            loss = self.lossf(self.net(self.x[k]), self.t[k])
            loss.backward()
            losses.append(loss.detach())
        return torch.stack(losses).mean()

    def _capture_tail(self, device):
        """Inside the capture, after backward (and after the stream's waits for the all-reduces): the AdamW step, then the log row."""
        lib, stream = _lib.load(), torch.cuda.current_stream(device).cuda_stream
        opt = self.optimizer
        if opt is not None:
            self._gflat = opt._flat_grad(self._opt_idx)     # the executor's flat gradient buffer (graph pool): same address in every replay
            if self._norm_plan is not None:
                # reduction + finish into the optimizer's {total_norm, clip_coef} record, then the AdamW launch that scales by it
                self._norm_plan.norm(self._gflat.data_ptr(), self._clip[1], self._clip[0], opt._clip_rec, stream)
            # alpha is read from the float behind the records; the host value is what the first replay uploads
            alpha = None
            if self._ema:
                alpha = (self._hyper.data_ptr() + (1 + len(self._opt_recs)) * HYPER_BYTES,
                         _ema_alpha(opt.ema_decay, opt.ema_warmup, opt._ema_updates + 1))
            opt._launch_ranges(self._gflat, self._table, len(self._opt_ranges), self._table_blocks, self._hyper.data_ptr() + HYPER_BYTES,
                               len(self._opt_recs), self._norm_plan is not None, alpha, stream)
        if self.log_capacity:
            gw, gb = self._log_w.grad, self._log_b.grad
            if gw is None or gb is None:
                raise RuntimeError("GraphedStep: the last layer's parameters received no gradient; the log cannot be captured")
            # a conv weight's gradient is a permuted view of one dense segment: the norm does not depend on the order
            for g in (gw, gb):
                if not (g.is_contiguous() or g.is_contiguous(memory_format=torch.channels_last)):
                    raise RuntimeError("GraphedStep: the last layer's gradient is not one dense block")
            rec = opt._clip_rec.data_ptr() if self._log_cols == _lib.STEP_LOG_NORM_COLUMNS else None
            check(lib.cvk_step_log(self.loss.data_ptr(), self._hyper.data_ptr(), gw.data_ptr(), gw.numel(), gb.data_ptr(), gb.numel(), rec,
                                   self._logbuf.data_ptr() + 8, self.log_capacity, self._logbuf.data_ptr(), stream), "cvk_step_log")

    def _upload_hyper(self):
        """Every group as the scheduler left it + the next step counts -> the device records, on the current stream (no host sync: the host
        waits only when it is HYPER_SLOTS replays ahead of the copies that read its pinned slots)."""
        opt = self.optimizer
        if self._ema:
            opt._ema_options()              # a decay outside [0, 1) is refused before anything is counted
        opt._step += 1
        opt._count(self._opt_idx)
        slot = self._hyper_slot
        self._hyper_slot = (slot + 1) % HYPER_SLOTS
        if self._hyper_busy[slot] is not None:
            self._hyper_busy[slot].synchronize()
        pin = self._hyper_pin[slot]
        opt._fill_record(0, None, pin.data_ptr())       # record 0: param_groups[0] as it is now, for the log row
        opt._fill(self._opt_recs, pin[HYPER_FLOATS:])
        if self._ema:
            pin[-1] = float(opt._next_ema_alpha())
        self._hyper.copy_(pin, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._hyper_busy[slot] = ev

    def log(self):
        """The log rows the replays wrote since the previous call, oldest first: (rows [k, 5] float32 numpy array of
        [loss, lr, beta1 (FlatAdamW) / momentum (FlatSGD), ||grad of the last weight||_2, ||grad of the last bias||_2], dropped).  With a clipping optimizer
        (FlatAdamW(max_grad_norm=...)) the rows have 7 columns: the five, then the step's global gradient norm and its clip coefficient.
        When more than log_capacity rows were
        written since the last call, the oldest were overwritten on the device: rows holds the newest log_capacity of them and
        dropped says how many were lost.  One device-to-host copy (waits for the replays enqueued so far)."""
        import numpy as np
        if not self.log_capacity:
            raise RuntimeError("GraphedStep.log(): built without a log (log_capacity=0)")
        buf = self._logbuf.cpu().numpy()
        written = int(buf[:2].view(np.int64)[0])
        cap = self.log_capacity
        ring = buf[2:].reshape(cap, self._log_cols)
        new = written - self._log_read
        dropped = max(0, new - cap)
        first = written - min(new, cap)
        rows = ring[[i % cap for i in range(first, written)]].copy() if written > first else np.zeros((0, self._log_cols), np.float32)
        self._log_read = written
        return rows, dropped

    def _zero(self):
        for p in self.params:
            p.grad = None

    def _signature(self):
        from .modules import plan_key_blocks
        R = self._runner
        # plan_key_blocks: every block's identity, BatchNorm mode and requires-grad pattern (what the captured plan and range table fixed)
        acc = R.accumulator
        return (id(R.grad_sync), bool(self.net.training), bool(R.bf16), R.persistent_wgs()) + R.kernel_config() + self._optimizer_signature() \
            + (plan_key_blocks(self.net),) + ((id(acc), acc.steps, acc.mean) if acc is not None else (None, 1, True))

    def _optimizer_signature(self):
        """The captured optimizer step writes the optimizer's flat buffers through raw pointers: the same optimizer, one parameter group, the
        same flat buffer, and every parameter still a view of it at its capture-time address (a rebuilt FlatAdamW re-homes them); the kernel
        variant is fixed too: clip or not, EMA or not, and what the rule adds (FlatSGD: whether a momentum buffer is in use)."""
        opt = getattr(self, "optimizer", None)
        if opt is None:
            return ()
        return (id(opt), len(opt.param_groups), tuple(opt._group_of()), opt._flat.data_ptr(), tuple(p.data_ptr() for p in opt._plist),
                opt.max_grad_norm, opt.norm_type, opt.ema_decay is not None) + opt._variant()

    def replay(self, x=None, t=None):
        """Copy a new batch into the static input buffers (optional) and replay the step.  Returns the (static) loss tensor.
        With an optimizer: the captured step uses param_groups[0] as it is now and optimizer._step + 1, then the scheduler (if any)
        steps — the order of the eager loop `replay(); optimizer.step(); scheduler.step()`."""
        if self._signature() != self._sig:
            raise RuntimeError("GraphedStep.replay: the network changed since the capture (train/eval mode of the network or of a "
                               "block's BatchNorm, a parameter's requires_grad, a swapped block, conv precision, a kernel "
                               "knob, it was wrapped in / unwrapped from ddp.DataParallel, a GradAccumulator was attached, detached or given other "
                               "steps / mean, or the captured FlatAdamW was rebuilt, re-homed, "
                               "regrouped, given another max_grad_norm / norm_type, its EMA switched on or off or a FlatSGD's momentum switched between zero and "
                               "non-zero): the "
                               "captured graph would silently run the "
                               "old configuration — build a new GraphedStep")
        if self.accumulator is not None and self.accumulator.micro_step:
            raise RuntimeError("GraphedStep.replay: the accumulator is in the middle of an eager window (micro-step "
                               f"{self.accumulator.micro_step} of {self.accumulator.steps}); the captured window starts at micro-step 0 — "
                               "finish the window or reset() the accumulator first")
        if self.optimizer is not None:
            self.optimizer._refuse_swapped("GraphedStep.replay")
        if x is not None:
            self.x.copy_(x, non_blocking=True)
        if t is not None:
            self.t.copy_(t, non_blocking=True)
        for p, g in zip(self.params, self.grads):   # zero_grad(set_to_none=True) between steps keeps working
            if p.grad is not g:
                p.grad = g
        if self.optimizer is not None:
            self._upload_hyper()
        self.graph.replay()
        if self.optimizer is not None:
            engine._bump_epoch()        # the kernel wrote the parameters through raw pointers: derived weight tensors are stale
            self.optimizer._opt_called = True   # what torch's scheduler wrapper of optimizer.step() records: a step ran before sched.step()
            if self.scheduler is not None:
                self.scheduler.step()
        return self.loss
