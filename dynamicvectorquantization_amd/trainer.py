"""Minimal trainer honouring the reference's LightningModule surface, without pytorch_lightning.

Covers what train.py + Lightning 1.5.6 do for the DQ-VAE path (train.py:227-270):
  * two-optimizer automatic optimisation: for optimizer_idx in (0, 1): training_step -> backward -> step;
  * LambdaLR schedules stepped every batch (models/stage1/utils.py:6-24);
  * data parallelism: one process per GPU, gradients averaged with bucketed RCCL all-reduce launched on a
    side stream as soon as the backward has finished (HIP kernels write .grad in place, so buckets are
    filled by `GradBuckets.reduce`, not by autograd hooks);
  * HipAdam: torch.optim.Optimizer subclass whose step() is the fused dvq_adam kernel per tensor.
"""
from __future__ import annotations

import contextlib
import math
from functools import partial

import os

import torch
import torch.distributed as dist

from . import kernels as K
from . import runtime as rt


# ---- LR schedules (models/stage1/utils.py:6-24) ----------------------------------------------------
def _fn_linear_warmup(warmup_steps, step):
    if step < warmup_steps:
        return float(step) / float(max(1, warmup_steps))
    return 1.0


def scheduler_linear_warmup(warmup_steps):
    return partial(_fn_linear_warmup, warmup_steps)


def _fn_linear_warmup_cosine_decay(warmup_steps, max_steps, multipler_min, step):
    if step < warmup_steps:
        return float(step) / float(max(1, warmup_steps))
    # (exactly the reference's expression, pinned bit for bit by tests/golden/losses.npz incl. steps past `max_steps`, where it climbs
    #  again like the reference's does: train.py keeps that from happening by sizing `training_steps` from the real loader BEFORE
    #  the schedules are built)
    multipler = 0.5 * (math.cos((step - warmup_steps) / (max_steps - warmup_steps) * math.pi) + 1)
    return max(multipler, multipler_min)


def scheduler_linear_warmup_cosine_decay(warmup_steps, max_steps, multipler_min):
    return partial(_fn_linear_warmup_cosine_decay, warmup_steps, max_steps, multipler_min)


# ---- flat parameter / gradient storage -------------------------------------------------------------------
class FlatParams:
    """One flat fp32 buffer for the parameters and one for their gradients; every Parameter's .data / .grad is
    a view into them.  The HIP kernels accumulate gradients in place into the flat buffer, which is also the
    RCCL all-reduce buffer and the operand of ONE fused Adam launch (instead of one per tensor)."""

    def __init__(self, params):
        self.params = [p for p in params if p.requires_grad]
        assert self.params, "no trainable parameters"
        dev = self.params[0].device
        total = sum(p.numel() for p in self.params)
        self.flat_p = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(total, dtype=torch.float32, device=dev)
        off = 0
        with torch.no_grad():
            for p in self.params:
                n = p.numel()
                new = self._view(self.flat_p, off, p)
                new.copy_(p.data)
                p.data = new
                p.grad = self._view(self.flat_g, off, p)
                off += n
        rt.bump_weights_epoch()      # parameter storage moved: packed copies must be rebuilt

    @staticmethod
    def _view(flat, off, p):
        """view of the flat buffer with p's logical shape; 4-D conv weights are stored channel-last
        ([Cout][KH][KW][Cin]): the wgrad kernel then accumulates with contiguous atomics and the bf16 forward
        pack is a plain cast"""
        n = p.numel()
        if p.dim() == 4 and p.shape[2] * p.shape[3] > 1:
            co, ci, kh, kw = p.shape
            return flat[off:off + n].view(co, kh, kw, ci).permute(0, 3, 1, 2)
        return flat[off:off + n].view(p.shape)

    def attach_grads(self):
        off = 0
        for p in self.params:
            n = p.numel()
            if p.grad is None or p.grad.data_ptr() != self.flat_g.data_ptr() + 4 * off:
                p.grad = self._view(self.flat_g, off, p)
            off += n

    def zero_grad(self):
        self.flat_g.zero_()
        self.attach_grads()


# ---- optimizer ------------------------------------------------------------------------------------------
def ema_decay_at(n, decay, warmup=True):
    """decay of the n-th weight-EMA update (n = 1 for the first): min(decay, (1 + n) / (10 + n)), the `num_updates` warm-up of
    tf.train.ExponentialMovingAverage and of taming / latent-diffusion's LitEma; `decay` itself with warmup=False"""
    n, decay = int(n), float(decay)
    if not warmup:
        return decay
    return min(decay, (1.0 + n) / (10.0 + n))


class HipAdam(torch.optim.Optimizer):
    """torch.optim.Adam / AdamW semantics (no amsgrad; `weight_decay` is decoupled like AdamW, 0 = plain Adam).  With
    `flatten()` (done by the Trainer) all parameter groups live in ONE flat buffer pair, each group a contiguous segment
    updated by one fused kernel launch with the group's lr / weight decay; otherwise one launch per tensor."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.flat = None
        self.flat_e = None
        self._fstate = None
        self._guard = None            # set_grad_guard: dict(clip, skip, ws, gstat)
        self._ema = None              # set_weight_ema: dict(decay, warmup, rec, last); the shadow buffer is self.flat_e
        self._norm = None             # set_norm_tracking: dict(plan, names, ws, grad / weight / update state blocks, snap, armed, ...)

    def set_weight_ema(self, decay=0.0, warmup=True):
        """Exponential moving average of this optimizer's parameters (docs/design/20-weight-ema.md): after every step()
        flat_e <- flat_e - (1 - d_n) * (flat_e - flat_p), d_n = ema_decay_at(n, decay, warmup), one launch over the whole flat buffer.
        decay == 0 switches it off and frees the shadow buffer.  `1 - d_n` is uploaded by prepare_step() into a device record, so a
        recorded step follows the schedule; with a grad guard set, a skipped step leaves flat_e untouched too (the update count still
        advances, like Adam's step count).  The buffers are allocated here, never inside step()."""
        decay = float(decay)
        if not (math.isfinite(decay) and 0.0 <= decay < 1.0):
            raise ValueError(f"EMA decay must be finite and in [0, 1) (0 = off), got {decay}")
        if self.flat is None:
            raise ValueError("set_weight_ema works on a flattened HipAdam only (call flatten() first): the per-tensor path has no "
                             "single parameter buffer to average")
        if decay == 0.0:
            self._ema, self.flat_e = None, None
            self._fstate.pop("ema_updates", None)
            return
        old = self._ema
        if old is None:
            self.flat_e = self.flat.flat_p.clone()
            self._fstate["ema_updates"] = 0
        self._ema = {"decay": decay, "warmup": bool(warmup), "last": None,
                     "rec": old["rec"] if old else torch.zeros(8, dtype=torch.float32, device=self.flat.flat_p.device)}
        self._prepared = False

    @property
    def ema_num_updates(self):
        """EMA updates applied so far (0 with the feature off)"""
        return int(self._fstate.get("ema_updates", 0)) if self._fstate else 0

    def ema_tensors(self):
        """{id(p): view of the shadow buffer with p's logical shape} (FlatParams._view: a channel-last-stored conv weight comes out
        [Cout, Cin, KH, KW]); {} with the feature off"""
        if self._ema is None:
            return {}
        out, off = {}, 0
        for p in self.flat.params:
            out[id(p)] = FlatParams._view(self.flat_e, off, p)
            off += p.numel()
        return out

    def set_grad_guard(self, clip_val=0.0, skip_nonfinite=False):
        """Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_ over ALL parameter groups of this optimizer, as Lightning's
        `gradient_clip_val` applies it) and / or a non-finite step guard (docs/design/19-gradient-clipping.md).
          clip_val > 0:    every step uses g * min(1, clip_val / (||g|| + 1e-6)); the gradient buffer itself is not rewritten;
          skip_nonfinite:  a step whose sum g^2 is not finite leaves p, m, v untouched and counts in grad_stats()["skipped"].  The step
                           count (bias corrections) and the LR schedule still advance: the host never learns of the skip.
        Norm, coefficient and flag are computed and consumed on the device (two extra launches per step, none when both are off).
        The workspace is allocated here, never inside step(): a captured step sees no allocation."""
        clip_val = float(clip_val)
        if not (math.isfinite(clip_val) and clip_val >= 0.0):
            raise ValueError(f"gradient clip value must be finite and >= 0 (0 = off), got {clip_val}")
        if self.flat is None:
            raise ValueError("set_grad_guard works on a flattened HipAdam only (call flatten() first): the per-tensor path has no "
                             "single gradient buffer to take the norm of")
        skip_nonfinite = bool(skip_nonfinite)
        if clip_val == 0.0 and not skip_nonfinite:
            self._guard = None
            return
        old = self._guard
        g = self.flat.flat_g
        self._guard = {"clip": clip_val, "skip": skip_nonfinite,
                       "ws": old["ws"] if old else torch.empty(K.grad_sqnorm_workspace_bytes(g.numel()) // 8, dtype=torch.float64, device=g.device),
                       "gstat": old["gstat"] if old else K.grad_stats_block(g.device)}

    def grad_stats(self):
        """{"norm", "coef", "finite", "skipped"} of the last step() -- a host read (synchronises): call it outside the step only.
        None when neither clipping nor the guard is enabled."""
        return K.read_grad_stats(self._guard["gstat"]) if self._guard else None

    def set_norm_tracking(self, names, track_updates=True):
        """Per-parameter gradient, weight and update norms on the device (docs/design/24-norm-tracking.md; Lightning's
        `track_grad_norm`).  `names`: {id(p): dotted name of model.named_parameters()}; None switches the feature off and frees its
        buffers.  Every step() then takes the statistics of flat_g per parameter (sum of squares, abs-max, Inf / NaN count, with
        running counts and the first offending step -- BEFORE clipping, which never rewrites flat_g); steps armed through
        arm_norm_row() also take those of flat_p after the update and, with `track_updates`, of flat_p minus a snapshot taken in
        front of Adam.  Unarmed, the weight / update launches return at once: a recorded step carries them, only row steps pay.
        Everything is allocated here, never inside step()."""
        if self.flat is None:
            raise ValueError("set_norm_tracking works on a flattened HipAdam only (call flatten() first): the per-tensor path has no "
                             "flat buffers to cut into segments")
        if names is None:
            self._norm = None
            return
        params = self.flat.params
        offsets = [0]
        for p in params:
            offsets.append(offsets[-1] + p.numel())
        dev = self.flat.flat_p.device
        plan = K.SegmentPlan(offsets, dev)
        S = plan.S
        self._norm = {"plan": plan, "names": [names.get(id(p), f"param{i}") for i, p in enumerate(params)],
                      "numel": [p.numel() for p in params], "track_updates": bool(track_updates),
                      "ws": K.segment_stats_workspace(plan.n, S, dev),
                      "grad": K.segment_stats_state(S, dev), "weight": K.segment_stats_state(S, dev),
                      "update": K.segment_stats_state(S, dev) if track_updates else None,
                      "snap": torch.empty_like(self.flat.flat_p) if track_updates else None,
                      "armed": torch.zeros(1, dtype=torch.int32, device=dev),
                      "bits": torch.tensor([0, 1], dtype=torch.int32, device=dev).view(torch.float32),      # the two values of `armed`
                      "arm_next": True}
        self._prepared = False

    def arm_norm_row(self, armed=True):
        """whether the NEXT step() takes the weight / update statistics (uploaded by prepare_step; the Trainer calls this before
        every step, a bare optimizer arms every step)"""
        if self._norm is not None:
            self._norm["arm_next"] = bool(armed)
            self._prepared = False

    def norm_stats(self):
        """{name: {numel, grad_norm, grad_absmax, grad_nonfinite, grad_nonfinite_total, first_bad_step, weight_norm, update_norm,
        update_ratio}} -- the gradient entries of the last step(), the last three of the most recent armed step (update_norm /
        update_ratio None without track_updates).  first_bad_step: the optimizer's 0-based step index, -1 = never.  A host read
        (synchronises): between steps only.  None with the feature off."""
        nt = self._norm
        if nt is None:
            return None
        S = nt["plan"].S
        g = {k: v.numpy() for k, v in K.segment_stats_views(nt["grad"].cpu(), S).items()}
        w = {k: v.numpy() for k, v in K.segment_stats_views(nt["weight"].cpu(), S).items()}
        u = {k: v.numpy() for k, v in K.segment_stats_views(nt["update"].cpu(), S).items()} if nt["update"] is not None else None
        base = int(self._fstate["step"]) - int(g["calls"][0])      # optimizer step index of the block's first launch
        out = {}
        for i, name in enumerate(nt["names"]):
            wn = math.sqrt(float(w["sumsq"][i]))
            un = math.sqrt(float(u["sumsq"][i])) if u is not None else None
            first = int(g["first_bad_call"][i])
            out[name] = {"numel": int(nt["numel"][i]), "grad_norm": math.sqrt(float(g["sumsq"][i])), "grad_absmax": float(g["absmax"][i]),
                         "grad_nonfinite": int(g["nonfinite"][i]), "grad_nonfinite_total": int(g["nonfinite_total"][i]),
                         "first_bad_step": first + base if first >= 0 else -1, "weight_norm": wn, "update_norm": un,
                         "update_ratio": (un / wn if wn > 0.0 else (0.0 if un == 0.0 else math.inf)) if un is not None else None}
        return out

    def flatten(self) -> FlatParams:
        if self.flat is None:
            allp = [p for g in self.param_groups for p in g["params"] if p.requires_grad]
            self.flat = FlatParams(allp)
            self._segments = []
            off = 0
            for g in self.param_groups:
                n = sum(p.numel() for p in g["params"] if p.requires_grad)
                self._segments.append((off, n))
                off += n
            for p in self.flat.params:
                p._dvq_group = id(self)
            self._fstate = {"step": 0, "m": torch.zeros_like(self.flat.flat_p), "v": torch.zeros_like(self.flat.flat_p)}
            # per-group hyper-parameters in DEVICE memory (dvq_adamw_dev): the launch has no step-dependent argument, so a
            # captured training step follows the LR schedule -- the host rewrites this table before each step
            self._hyper = torch.zeros(len(self.param_groups), 8, dtype=torch.float32, device=self.flat.flat_p.device)
            self._prepared = False
        return self.flat

    @torch.no_grad()
    def prepare_step(self):
        """upload the hyper-parameters of the NEXT step() (lr from the schedule, bias corrections of step count + 1).  Called
        by the Trainer at the top of every step, outside any capture; step() calls it itself when nobody did."""
        t = self._fstate["step"] + 1
        for gi, g in enumerate(self.param_groups):
            b1, b2 = g["betas"]
            lr = float(g["lr"])
            bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
            K.set_f32x8(self._hyper[gi], [lr / bc1, b1, b2, g["eps"], 1.0 / math.sqrt(bc2), 1.0 - lr * g.get("weight_decay", 0.0)])
        em = self._ema
        if em is not None:                 # 1 - d of the NEXT EMA update, in fp64 here, rounded to fp32 once on its way to the device
            em["last"] = ema_decay_at(self._fstate["ema_updates"] + 1, em["decay"], em["warmup"])
            K.set_f32x8(em["rec"], [1.0 - em["last"]])
        nt = self._norm
        if nt is not None:                 # the 4-byte `armed` record of the NEXT step: a kernel launch, like the uploads above
            K.copy_f32_armed(nt["armed"].view(torch.float32), nt["bits"][1:2] if nt["arm_next"] else nt["bits"][0:1])
        self._prepared = True

    @torch.no_grad()
    def step(self, closure=None):
        if self.flat is not None:
            st = self._fstate
            if not self._prepared:
                self.prepare_step()
            self._prepared = False
            st["step"] += 1
            gd = self._guard
            nt = self._norm
            if nt is not None:             # per-parameter gradient statistics, EVERY step (sticky counters): a NaN is localised after the fact
                K.segment_stats(self.flat.flat_g, None, nt["plan"], nt["ws"], nt["grad"], sticky=True)
            if gd is not None:             # norm / coefficient / finite flag of the WHOLE buffer (all groups), on the device
                K.grad_sqnorm(self.flat.flat_g, gd["ws"], gd["gstat"], gd["clip"], gd["skip"])
            if nt is not None and nt["snap"] is not None:      # row steps: the parameters in front of Adam
                K.copy_f32_armed(nt["snap"], self.flat.flat_p, nt["armed"])
            for gi, (off, n) in enumerate(self._segments):
                if n == 0:
                    continue
                sl = slice(off, off + n)
                if gd is not None:
                    K.adamw_clip_dev(self.flat.flat_p[sl], self.flat.flat_g[sl], st["m"][sl], st["v"][sl], self._hyper[gi], gd["gstat"])
                else:
                    K.adamw_dev(self.flat.flat_p[sl], self.flat.flat_g[sl], st["m"][sl], st["v"][sl], self._hyper[gi])
            if self._ema is not None:      # ONE launch over the whole buffer (all groups), after Adam; follows the guard's skip
                K.ema_update(self.flat_e, self.flat.flat_p, self._ema["rec"], gd["gstat"] if gd is not None else None)
                st["ema_updates"] += 1
            if nt is not None:             # row steps: weight norms of the updated parameters, update norms against the snapshot
                K.segment_stats(self.flat.flat_p, None, nt["plan"], nt["ws"], nt["weight"], armed=nt["armed"])
                if nt["snap"] is not None:
                    K.segment_stats(self.flat.flat_p, nt["snap"], nt["plan"], nt["ws"], nt["update"], armed=nt["armed"])
            rt.bump_group_epoch(id(self))      # only this optimizer's packed weights are stale
            return
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] += 1
                K.adamw_step(p.data, p.grad, st["exp_avg"], st["exp_avg_sq"], group["lr"], b1, b2, group["eps"],
                             group.get("weight_decay", 0.0), st["step"])
        rt.bump_weights_epoch()


# ---- data-parallel gradient exchange --------------------------------------------------------------------
class GradBuckets:
    """All-reduce view of a FlatParams gradient buffer: fixed-size chunks, last layers first (their gradients are
    final first), launched asynchronously on RCCL's stream."""

    def __init__(self, params_or_flat, bucket_bytes=64 << 20, process_group=None):
        self.fp = params_or_flat if isinstance(params_or_flat, FlatParams) else FlatParams(params_or_flat)
        self.pg = process_group
        n = self.fp.flat_g.numel()
        step = max(1, bucket_bytes // 4)
        self.bucket_elems = step
        self.flat = [self.fp.flat_g[i:min(n, i + step)] for i in range(0, n, step)]
        self.params = self.fp.params
        self._pending, self._done = [], []
        self.launched = 0                 # all-reduce launches so far (tests: every bucket exactly once per step)
        self._divisor = None              # tests: pre-division factor of a pretended world size in a one-rank group
        self.measure = None               # list of (start, end) event pairs around wait() while bench.py measures the exposed time

    def zero(self):
        self.fp.zero_grad()

    def _active(self):
        # DVQ_FORCE_DP=1: exchange even in a one-rank group (exercises the RCCL / capture-break path on a single GPU)
        return dist.is_available() and dist.is_initialized() and (dist.get_world_size(self.pg) > 1 or rt.force_dp())

    def reduce_range(self, lo, hi):
        """start averaging flat_g[lo:hi] over ranks NOW (asynchronously, on RCCL's stream) -- called from inside the
        backward as soon as that part of the gradient is final, so the exchange overlaps the rest of the backward"""
        if not self._active() or hi <= lo:
            return
        ws = self._divisor if self._divisor is not None else dist.get_world_size(self.pg)
        # weight gradients of eager steps are accumulated into this range by kernels on the side stream (runtime.side_wgrad):
        # the pre-division below reads the range on the CURRENT stream, so the side stream is joined first -- not only at the
        # graph break further down
        rt.join_side()
        seg = self.fp.flat_g[lo:hi]
        seg.div_(ws)
        step = max(1, self.bucket_elems)
        chunks = [self.fp.flat_g[a:min(hi, a + step)] for a in range(lo, hi, step)]

        def launch():        # eager even when the step is being captured (rt.graph_break): RCCL runs on its own stream
            if rt.switch("DVQ_DP_NOOP_COLLECTIVES") == "1":        # debugging: exchange points without the RCCL calls
                self.launched += len(chunks)
                return
            for c in chunks:
                self._pending.append(dist.all_reduce(c, op=dist.ReduceOp.SUM, group=self.pg, async_op=True))
            self.launched += len(chunks)
        rt.graph_break(launch)
        self._done.append((lo, hi))

    def reduce_params(self, params, min_bytes=1 << 20):
        """gradients of `params` are final: start the all-reduce of the contiguous flat ranges they cover (called from inside the
        backward, per block / level / segment, so that the exchange overlaps the rest of the backward).  Runs shorter than
        `min_bytes` are left to the closing reduce() -- a latency-bound collective per bias vector helps nobody."""
        if not self._active():
            return
        offs = self._offsets()
        spans = sorted((offs[id(p)], offs[id(p)] + p.numel()) for p in params if id(p) in offs)
        runs = []
        for lo, hi in spans:
            if runs and lo <= runs[-1][1]:
                runs[-1][1] = max(runs[-1][1], hi)
            else:
                runs.append([lo, hi])
        for lo, hi in runs:
            if (hi - lo) * 4 < min_bytes or any(lo < d_hi and d_lo < hi for d_lo, d_hi in self._done):
                continue
            self.reduce_range(lo, hi)

    def _offsets(self):
        offs = getattr(self, "_offs", None)
        if offs is None:
            offs, off = {}, 0
            for p in self.fp.params:
                offs[id(p)] = off
                off += p.numel()
            self._offs = offs
        return offs

    def reduce(self, async_op=True):
        """average the ranges that reduce_range() has not covered yet (no-op for world size 1); returns ALL work handles"""
        if not self._active():
            return []
        n = self.fp.flat_g.numel()
        covered = sorted(self._done)
        pos = 0
        gaps = []
        for lo, hi in covered:
            if lo > pos:
                gaps.append((pos, lo))
            pos = max(pos, hi)
        if pos < n:
            gaps.append((pos, n))
        for lo, hi in reversed(gaps):              # last layers first
            self.reduce_range(lo, hi)
        self._done = []
        return list(self._pending)

    def wait(self):
        """make the current stream wait for every exchange launched so far (eager; a graph break inside a capture)"""
        if not self._active():
            return

        def _wait():
            if self.measure is not None:              # bench.py: time the compute stream spends in this wait (HIP events around it)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            for w in self._pending:
                if w is not None:
                    w.wait()
            self._pending.clear()
            if self.measure is not None:
                e1.record()
                self.measure.append((e0, e1))
        rt.graph_break(_wait)

    def param_range(self, params):
        """[lo, hi) of the flat buffer covered by `params` (they must be contiguous in the optimizer's order)"""
        ids = {id(p) for p in params}
        off, lo, hi = 0, None, None
        for p in self.fp.params:
            if id(p) in ids:
                lo = off if lo is None else lo
                hi = off + p.numel()
            off += p.numel()
        return (lo or 0), (hi or 0)


def reference_learning_rate(model_cfg, world, batch_size, accumulate_grad_batches=1):
    """train.py:248-257 of the reference: lr = accumulate_grad_batches * ngpu * batch_size * base_learning_rate when the config gives
    a base rate (the reference pins the first factor to 1, and so does every caller here until the Trainer accumulates), else the
    absolute `learning_rate`"""
    if "base_learning_rate" in model_cfg:
        return accumulate_grad_batches * world * batch_size * model_cfg["base_learning_rate"]
    if "learning_rate" in model_cfg:
        return model_cfg["learning_rate"]
    raise NotImplementedError("Please set learning rate!")


# ---- accumulation windows (docs/design/28-gradient-accumulation.md): the host arithmetic HipAdam.set_window is fed from -------------------
def window_flags(pos, batch_in_epoch, k, batches_per_epoch=None):
    """(first, last) of a micro-batch under Lightning 1.5's accumulation: `pos` micro-batches of its window have run before it, it is
    batch `batch_in_epoch` of its epoch.  A window closes after k micro-batches or with the epoch's last batch, whichever comes
    first; batches_per_epoch None: epochs never cut a window.  From an epoch's start pos == batch_in_epoch % k, i.e. the window
    closes when (batch_in_epoch + 1) % k == 0."""
    last = pos + 1 >= k or (batches_per_epoch is not None and batch_in_epoch + 1 >= batches_per_epoch)
    return pos == 0, last


def window_schedule(n_batches, k, batches_per_epoch=None):
    """[(first, last)] of batches 0 .. n_batches - 1 of a run that starts at an epoch's start"""
    out, pos = [], 0
    for b in range(n_batches):
        first, last = window_flags(pos, b % batches_per_epoch if batches_per_epoch else b, k, batches_per_epoch)
        out.append((first, last))
        pos = 0 if last else pos + 1
    return out


def optimizer_steps_per_epoch(batches_per_epoch, k):
    """ceil(batches / k): the short last window of an epoch is an optimizer step too"""
    return -(-int(batches_per_epoch) // int(k))


def _replicated_tensors(model):
    """(name, tensor) of everything that must be IDENTICAL on all ranks: parameters and buffers, except the statistics of
    the discriminator's BatchNorm layers, which DDP keeps per rank (modules/discriminator/model.py:31)"""
    from .layers import BatchNorm2d
    skip = set()
    for mn, mod in model.named_modules():
        if isinstance(mod, BatchNorm2d):
            skip.update(f"{mn}.{bn}" for bn, _ in mod.named_buffers(recurse=False))
    for n, p in model.named_parameters():
        yield n, p.detach()
    for n, b in model.named_buffers():
        if n not in skip:
            yield n, b


def broadcast_model(model, src=0):
    """DDP's initial synchronisation: rank `src`'s parameters and buffers everywhere (one broadcast per tensor at start-up)"""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() < 2:
        return
    for _, t in _replicated_tensors(model):
        dist.broadcast(t, src)
    from .layers import ActNorm
    for m in model.modules():
        if isinstance(m, ActNorm):
            m._inited = None               # the `initialized` buffer was just overwritten in place: re-read it, do not trust the host mirror
    rt.bump_weights_epoch()


def replicas_equal(model):
    """debug check (DVQ_DP_CHECK_EVERY=k): True iff every replicated tensor has the same checksum on all ranks"""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() < 2:
        return True
    sums = torch.stack([t.double().sum() + t.double().abs().sum() * 3.0 for _, t in _replicated_tensors(model)])
    lo, hi = sums.clone(), sums.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    return bool(torch.equal(lo, hi))


class Trainer:
    """fit loop for a DualGrainVQModel-like module on batches produced by `batch_fn(step) -> dict`.

    Step capture: after `graph_after` eager steps with an unchanged signature (batch shapes, train flag, loss phase, runtime
    switches) the step is recorded once as hipGraph segments (runtime.StepGraph) and replayed from then on; collectives
    stay eager between segments, the optimizer reads its hyper-parameters from device memory, batches are copied into
    static input buffers.  `DVQ_STEP_GRAPH=0` (or use_graph=False) keeps every step eager."""

    def __init__(self, model, max_steps, log_every=0, use_graph=None, graph_after=3, gradient_clip_val=0.0, skip_nonfinite=False,
                 ema_decay=0.0, ema_warmup=True, deterministic=False, metrics_logger=None, track_grad_norm=-1, track_updates=True,
                 norm_every=50, norm_depth=0, norm_logdir=None):
        self.model, self.max_steps, self.log_every = model, max_steps, log_every
        # scalar logs (metrics.MetricsLogger, docs/design/22-metrics-logging.md): the model's logged scalars gathered on the device at the
        # end of every step, rows written every log_every_n_steps steps and at epoch ends.  None (the default): no launch, no file
        self.metrics_logger = metrics_logger
        # Lightning's Trainer(deterministic=True) (docs/design/21-reproducible-training.md): every floating-point reduction of the step in
        # a fixed order (kernels.set_deterministic, before the first launch) and every host-side draw of the step -- the dropout seeds
        # of stage 2, the restart rows of the codebooks -- a function of torch's seed and the number of draws made by THIS trainer, not
        # of what ran in the process before it.  Off (the default): nothing changes
        self.deterministic = bool(deterministic)
        if self.deterministic:
            K.set_deterministic(True)
            rt.reseed_draws(model)
        self.opts, self.scheds = model.configure_optimizers()
        self.buckets = [GradBuckets(o.flatten()) for o in self.opts]
        if metrics_logger is not None:         # its device state is allocated here, never inside a step
            metrics_logger.attach(model, self.buckets[0].fp.flat_g.device)
        # Lightning's Trainer(gradient_clip_val=...): global-norm clipping once per optimizer; skip_nonfinite: a step whose gradient
        # holds an Inf / NaN changes neither parameters nor Adam moments (HipAdam.set_grad_guard).  Both off (the default): no extra launch, dvq_adamw_dev as ever
        self.gradient_clip_val, self.skip_nonfinite = float(gradient_clip_val), bool(skip_nonfinite)
        if self.gradient_clip_val != 0.0 or self.skip_nonfinite:
            for o in self.opts:
                o.set_grad_guard(self.gradient_clip_val, self.skip_nonfinite)
        # weight EMA (docs/design/20-weight-ema.md): shadow weights of optimizer 0 -- the autoencoder in stage 1, the transformer in
        # stage 2 -- for validation, checkpoints and the tools; an averaged discriminator has no use.  Off (the default): no buffer,
        # no launch, the checkpoint as ever
        self.ema_decay, self.ema_warmup = float(ema_decay), bool(ema_warmup)
        self._in_ema_scope = False
        self._warned_no_ema = False
        broadcast_model(model)             # identical start on every rank (DDP's parameter / buffer broadcast), not just equal seeds
        if self.ema_decay != 0.0:          # after the broadcast: flat_e starts as a copy of the weights every rank holds
            self.opts[0].set_weight_ema(self.ema_decay, self.ema_warmup)
        # Lightning's Trainer(track_grad_norm=...) (docs/design/24-norm-tracking.md): per-parameter gradient / weight / update norms of
        # every optimizer on the device; -1 (the default): off -- no launch, no buffer, no file.  2 / "inf" choose what the total keys
        # report.  Rows at the metrics logger's cadence, or every `norm_every` steps without one; norms.csv in `norm_logdir` (default:
        # the metrics logger's directory; neither: statistics through norm_stats() only)
        self.norm_every = metrics_logger.log_every_n_steps if metrics_logger is not None else max(1, int(norm_every))
        self._norm_out = (norm_depth, norm_logdir or (metrics_logger.logdir if metrics_logger is not None else None))
        self.set_norm_tracking(track_grad_norm, track_updates)
        self.check_every = int(rt.switch("DVQ_DP_CHECK_EVERY"))
        import inspect
        # Lightning passes optimizer_idx only to modules that declare it (two-optimizer stage 1); stage 2 has one optimizer
        self._takes_opt_idx = "optimizer_idx" in inspect.signature(model.training_step).parameters
        if use_graph is None:
            use_graph = rt.switch("DVQ_STEP_GRAPH") != "0"
        self.use_graph = bool(use_graph) and bool(getattr(model, "GRAPH_SAFE", False))
        self.graph_after = graph_after
        self._graph = None            # dict(sg, sig, static, losses)
        self._last_sig, self._stable = None, 0
        self.graph_replays = 0

    # ---- one step ------------------------------------------------------------------------------------------------
    def train_step(self, batch, batch_idx):
        if self._in_ema_scope:
            raise RuntimeError("train_step inside ema_scope(): the parameters hold the averaged weights, a step would train those")
        lg = self.metrics_logger
        if lg is None:
            out = self._train_step(batch, batch_idx)
            self._norm_row()
        else:
            lrs = [o.param_groups[0]["lr"] for o in self.opts]       # of the step about to run: the schedulers advance inside it
            out = self._train_step(batch, batch_idx)
            self._norm_row()                                         # before the metrics row, which takes its totals
            lg.after_step(self, int(self.model.global_step) - 1, batch, lrs)
        if self.check_every and (int(self.model.global_step) % self.check_every) == 0 and not replicas_equal(self.model):
            raise RuntimeError(f"data-parallel replicas diverged at global step {self.model.global_step}")
        return out

    def _train_step(self, batch, batch_idx):
        if not self.use_graph:
            return self._eager_step(batch, batch_idx)
        sig = self._signature(batch)
        if sig is None:                            # profiled step / injected host-side noise: eager, the recording stays valid
            return self._eager_step(batch, batch_idx)
        g = self._graph
        if g is not None and g["sig"] == sig:
            return self._replay(batch)
        if g is not None:
            self._graph = None                     # the recorded control flow no longer applies
        self._stable = self._stable + 1 if sig == self._last_sig else 0
        self._last_sig = sig
        if self._stable >= self.graph_after:       # `graph_after` eager steps with this signature have run
            if self._capture(batch, batch_idx, sig):
                return self._replay(batch)
        return self._eager_step(batch, batch_idx)

    def _prepare_opts(self):
        """hyper-parameters of the step about to run -> device memory, outside any capture and before any replay; with norm tracking
        also whether it is a row step (the `armed` record the recorded weight / update launches read)"""
        if self.norm_tracker is not None:
            armed = self._is_norm_row(int(self.model.global_step))
            for o in self.opts:
                o.arm_norm_row(armed)
        for o in self.opts:
            o.prepare_step()

    def set_norm_tracking(self, track_grad_norm=-1, track_updates=True):
        """switch per-parameter norm tracking of every optimizer between steps (-1 = off: the buffers are freed, the sticky counters
        with them); a step recorded under the other setting is not replayed: the signature differs"""
        from . import normtrack
        self.track_grad_norm, self.track_updates = normtrack.parse_track_grad_norm(track_grad_norm), bool(track_updates)
        if self.track_grad_norm == -1:
            for o in self.opts:
                o.set_norm_tracking(None)
            self.norm_tracker = None
            return
        names = {id(p): n for n, p in self.model.named_parameters()}
        for o in self.opts:
            o.set_norm_tracking(names, self.track_updates)
        self.norm_tracker = normtrack.NormTracker(self.track_grad_norm, *self._norm_out)

    def _is_norm_row(self, step):
        return (step + 1) % self.norm_every == 0

    def _norm_row(self):
        """behind a row step: read the statistics (a host read, the step has been issued) and hand them to the tracker"""
        nt = self.norm_tracker
        step = int(self.model.global_step) - 1
        if nt is None or not self._is_norm_row(step):
            return
        lg = self.metrics_logger
        from .metrics import TensorBoardWriter
        tb = next((w for w in lg.writers if isinstance(w, TensorBoardWriter)), None) if lg is not None else None
        spe = max(1, int(getattr(self.model, "steps_per_epoch", 1) or 1))
        nt.row(step, step // spe, self.norm_stats(), tensorboard=tb)

    def norm_stats(self):
        """one {parameter name: {numel, grad_norm, grad_absmax, grad_nonfinite, grad_nonfinite_total, first_bad_step, weight_norm,
        update_norm, update_ratio}} per optimizer (HipAdam.norm_stats): the gradient entries of the last step, eager or replayed,
        the last three of the most recent row step.  A host read: between steps only.  None with the feature off."""
        if self.norm_tracker is None:
            return None
        return [o.norm_stats() for o in self.opts]

    def _eager_step(self, batch, batch_idx):
        self._prepare_opts()                       # hyper-parameters of this step -> device memory
        return self._step_body(batch, batch_idx)

    def _step_body(self, batch, batch_idx):
        """the capturable part: every launch of the two-optimizer step (collectives are graph breaks)"""
        m = self.model
        losses = []
        lg = self.metrics_logger
        if lg is not None:                     # collect what THIS step logs apart from what earlier steps left in the shim's dict
            logged_before, m._logged = getattr(m, "_logged", {}), {}
        K.arena_reset(self.buckets[0].fp.flat_g.device)
        # single-threaded autograd: the backward's launches come from this thread (one capture thread, no thread hops)
        with torch.autograd.set_multithreading_enabled(False):
            for oi, opt in enumerate(self.opts):
                self.buckets[oi].zero()
                self._arm_overlap(oi)
                with rt.side_wgrad():          # conv weight gradients on a second stream, joined on exit (and at graph breaks)
                    loss = m.training_step(batch, batch_idx, oi) if self._takes_opt_idx else m.training_step(batch, batch_idx)
                    if loss.requires_grad:
                        loss.backward()
                self.buckets[oi].reduce()
                self.buckets[oi].wait()
                opt.step()
                self.scheds[oi]["scheduler"].step()
                losses.append(loss.detach())
            if lg is not None:                 # the last launches of the step, recorded with it: no host read, no copy node
                lg.push(m, m._logged)
                m._logged = {**logged_before, **m._logged}
        m.global_step += 1
        return losses

    # ---- capture / replay ----------------------------------------------------------------------------------------
    def _signature(self, batch):
        """everything host-side that shapes the step's launch sequence; None = this step cannot be captured"""
        m = self.model
        if K.profiling_active() or rt.capturing():
            return None
        extra = m.graph_signature() if hasattr(m, "graph_signature") else ()
        if extra is None:
            return None
        items = []
        for k in sorted(batch):
            v = batch[k]
            if torch.is_tensor(v):
                if not v.is_cuda:
                    return None
                items.append((k, tuple(v.shape), v.dtype, v.device.index))
            else:
                items.append((k, repr(v)))
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        guard = (self.gradient_clip_val, self.skip_nonfinite)           # launch arguments of the recorded norm kernels
        sig = (tuple(items), bool(m.training), rt.compute_dtype(), rt.impl(), rt.fuse_gn_prologue(), world, extra, guard)
        if K.deterministic():                      # the ordered kernels are other launches: a recording made in one mode is not replayed in the other
            sig = sig + (("deterministic",),)
        # whether the EMA launch is part of the step; the decay is device data and not part of the signature
        sig = sig + (("ema",) if self.ema_enabled else ())
        sig = sig + (("metrics",) if self.metrics_logger is not None else ())         # likewise the scalar push
        # and the norm-tracking launches; which steps are rows is device data (`armed`) and not part of the signature
        return sig + ((("norms", self.track_grad_norm, self.track_updates),) if self.norm_tracker is not None else ())

    def _py_state(self):
        return ([o._fstate["step"] for o in self.opts], [s["scheduler"].state_dict() for s in self.scheds],
                [[g["lr"] for g in o.param_groups] for o in self.opts], int(self.model.global_step),
                [o._fstate.get("ema_updates") for o in self.opts])

    def _set_py_state(self, st):
        steps, scheds, lrs, gstep, ema_counts = st
        for o, t, lr, ne in zip(self.opts, steps, lrs, ema_counts):
            o._fstate["step"] = t
            if ne is not None:             # the capture's dry run counted an EMA update that did not happen
                o._fstate["ema_updates"] = ne
            for g, v in zip(o.param_groups, lr):
                g["lr"] = v
        for s, sd in zip(self.scheds, scheds):
            s["scheduler"].load_state_dict(sd)
        self.model.global_step = gstep

    def _capture(self, batch, batch_idx, sig) -> bool:
        """record one step (a dry run: captured kernels do not execute, the Python-side counters are put back)"""
        dev = self.buckets[0].fp.flat_g.device
        static = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
        saved = self._py_state()
        logged = dict(getattr(self.model, "_logged", {}))
        self._prepare_opts()
        sg = rt.StepGraph(dev)
        try:
            with sg.capture():
                losses = self._step_body(static, batch_idx)
        except Exception as e:          # a launch sequence that cannot be captured: stay eager, say why once
            import warnings
            warnings.warn(f"training-step capture failed ({type(e).__name__}: {e}); continuing with eager launches")
            self.use_graph = False
            self._set_py_state(saved)
            for o in self.opts:
                o._prepared = False
            return False
        self._set_py_state(saved)
        if hasattr(self.model, "_logged"):
            # the step's log tensors now live in the graph's pool and are refreshed by every replay
            self.model._logged = {**logged, **self.model._logged}
        self._graph = {"sg": sg, "sig": sig, "static": static, "losses": losses}
        if self.metrics_logger is not None:
            self._graph["metric_keys"] = self.metrics_logger.last_keys       # the keys the recorded push carries
        return True

    def _replay(self, batch):
        g = self._graph
        for k, v in batch.items():
            if torch.is_tensor(v) and v.data_ptr() != g["static"][k].data_ptr():
                g["static"][k].copy_(v, non_blocking=True)
        self._prepare_opts()
        g["sg"].replay()
        # host-side bookkeeping the recorded launches do not carry
        for o, sc in zip(self.opts, self.scheds):
            o._fstate["step"] += 1
            if o._ema is not None:
                o._fstate["ema_updates"] += 1
            o._prepared = False
            sc["scheduler"].step()
            # the replay rewrote this optimizer's parameters: whatever an EAGER forward (eval / encode / validation_step) packed
            # or prepared from them before is stale -- same invalidation an eager opt.step() / EMA update does
            rt.bump_group_epoch(id(o))
        rt.bump_codebook_epoch()
        self.model.global_step += 1
        self.graph_replays += 1
        if self.metrics_logger is not None:
            self.metrics_logger.last_keys = g["metric_keys"]
        return g["losses"]

    def drop_graph(self):
        self._graph, self._stable, self._last_sig = None, 0, None

    def set_grad_guard(self, gradient_clip_val=0.0, skip_nonfinite=False):
        """change the setting of every optimizer between steps (the skip counters survive a change of values, not switching both
        off); a recorded step with other settings is not replayed: the signature differs, the step is recorded again"""
        for o in self.opts:
            o.set_grad_guard(gradient_clip_val, skip_nonfinite)
        self.gradient_clip_val, self.skip_nonfinite = float(gradient_clip_val), bool(skip_nonfinite)

    @property
    def grad_guard_enabled(self):
        return any(getattr(o, "_guard", None) is not None for o in self.opts)

    def grad_stats(self):
        """one {"norm", "coef", "finite", "skipped"} per optimizer (None for one without clipping / guard), of the last step --
        eager or replayed.  A host read: outside the step only."""
        return [o.grad_stats() if getattr(o, "_guard", None) is not None else None for o in self.opts]

    # ---- weight EMA ------------------------------------------------------------------------------------------------
    @property
    def ema_enabled(self):
        return getattr(self.opts[0], "_ema", None) is not None

    def set_weight_ema(self, ema_decay=0.0, ema_warmup=True):
        """switch the weight EMA of optimizer 0 between steps (0 = off: the shadow buffer is freed; on again: it starts from the
        current weights).  A step recorded under the other setting is not replayed: the signature differs"""
        if self._in_ema_scope:
            raise RuntimeError("set_weight_ema inside ema_scope()")
        self.opts[0].set_weight_ema(ema_decay, ema_warmup)
        self.ema_decay, self.ema_warmup = float(ema_decay), bool(ema_warmup)

    def _swap_ema(self):
        o = self.opts[0]
        K.swap_f32(o.flat.flat_p, o.flat_e)
        rt.bump_group_epoch(id(o))         # whatever was packed or prepared from these parameters is stale
        rt.bump_codebook_epoch()

    @contextlib.contextmanager
    def ema_scope(self):
        """look through the averaged weights: the contents of flat_p and flat_e are exchanged on entry and exchanged back on exit
        (also when the body raises).  Every Parameter.data is a view of flat_p, so no pointer moves and a recorded step stays
        valid; the exchange is exact, so the training weights come back bit for bit.  Tensors the forward pass updates (the EMA
        codebook, BatchNorm statistics) are not averaged: the model sees their live values.  No-op with the feature off."""
        if not self.ema_enabled:
            yield self
            return
        if self._in_ema_scope:
            raise RuntimeError("ema_scope() does not nest")
        if rt.capturing():
            raise RuntimeError("ema_scope() inside a step capture")
        self._swap_ema()
        self._in_ema_scope = True
        try:
            yield self
        finally:
            self._in_ema_scope = False
            self._swap_ema()

    def _ema_state_dict(self):
        """{name: cpu tensor} of the averaged parameters under the names of model.state_dict(), contiguous in logical shape"""
        views = self.opts[0].ema_tensors()
        names = {id(t): k for k, t in self.model.state_dict(keep_vars=True).items()}
        return {names[i]: v.detach().cpu().contiguous().clone() for i, v in views.items() if i in names}

    def _arm_overlap(self, oi):
        """Gradient exchange overlapped with the backward: every module of the model that declares `_grad_hook` calls it with the
        parameters whose gradients just became final (decoder side / encoder heads / each encoder level of the DQ-VAE, each
        block of StackGPT); under data parallelism that starts the all-reduce of their flat ranges right away
        (GradBuckets.reduce_params), the closing reduce() covers what is left.  Only the optimizer whose backward is about to
        run is armed."""
        gb = self.buckets[oi]
        armed = gb._active() and rt.switch("DVQ_DP_NO_HOOK") != "1"
        for mod in self.model.modules():
            if hasattr(mod, "_grad_hook"):
                mod._grad_hook = gb.reduce_params if armed else None

    # ---- checkpoint / resume (train.py:153-185, 270 + `-r`) --------------------------------------------------------------------
    # Lightning's last.ckpt layout: {"state_dict", "optimizer_states": [torch Optimizer.state_dict()...], "lr_schedulers",
    # "global_step", "epoch"}.  The optimizer states are written in torch's own format (per-parameter exp_avg / exp_avg_sq in
    # the parameter's logical shape, indices over the optimizer's full parameter list, `param_groups`), so the file resumes
    # here AND under the reference; the round-1 private format ({"step","exp_avg","exp_avg_sq"} over the flat buffer) still loads.
    def _optimizer_state_dict(self, o):
        st, flat = o._fstate, o.flat
        offs, off = {}, 0
        for p in flat.params:
            offs[id(p)] = off
            off += p.numel()
        state, groups, idx = {}, [], 0
        for g in o.param_groups:
            ids = []
            for p in g["params"]:
                if id(p) in offs and st["step"] > 0:
                    state[idx] = {"step": torch.tensor(float(st["step"])),
                                  "exp_avg": FlatParams._view(st["m"], offs[id(p)], p).detach().cpu().contiguous().clone(),
                                  "exp_avg_sq": FlatParams._view(st["v"], offs[id(p)], p).detach().cpu().contiguous().clone()}
                ids.append(idx)
                idx += 1
            groups.append({**{k: v for k, v in g.items() if k != "params"}, "params": ids})
        return {"state": state, "param_groups": groups}

    def _load_optimizer_state(self, o, sd):
        st, flat = o._fstate, o.flat
        if "state" not in sd:                             # round-1 private format: flat buffers
            n = st["m"].numel()
            if sd["exp_avg"].numel() != n or sd["exp_avg_sq"].numel() != n:
                raise ValueError(f"optimizer state holds {sd['exp_avg'].numel()} elements, this optimizer has {n} "
                                 "(a different parameter set, e.g. disc_factor=0 dropping the discriminator?)")
            st["step"] = int(sd["step"])
            st["m"].copy_(sd["exp_avg"].to(st["m"].device))
            st["v"].copy_(sd["exp_avg_sq"].to(st["v"].device))
            return
        offs, off = {}, 0
        for p in flat.params:
            offs[id(p)] = off
            off += p.numel()
        full = [p for g in o.param_groups for p in g["params"]]
        n_saved = sum(len(g["params"]) for g in sd.get("param_groups", []))
        if n_saved and n_saved != len(full):
            raise ValueError(f"optimizer state lists {n_saved} parameters, this optimizer has {len(full)}")
        step = 0
        st["m"].zero_()
        st["v"].zero_()
        for idx, p in enumerate(full):
            ps = sd["state"].get(idx, sd["state"].get(str(idx)))
            if ps is None or id(p) not in offs:
                continue
            if tuple(ps["exp_avg"].shape) != tuple(p.shape):
                raise ValueError(f"optimizer state of parameter {idx}: shape {tuple(ps['exp_avg'].shape)} != {tuple(p.shape)}")
            FlatParams._view(st["m"], offs[id(p)], p).copy_(ps["exp_avg"].to(st["m"].device))
            FlatParams._view(st["v"], offs[id(p)], p).copy_(ps["exp_avg_sq"].to(st["v"].device))
            step = max(step, int(float(ps["step"])))
        st["step"] = step

    def state_dict(self):
        sd = {"state_dict": self.model.state_dict(), "global_step": int(self.model.global_step),
              "epoch": int(getattr(self.model, "current_epoch", 0)),
              "optimizer_states": [self._optimizer_state_dict(o) for o in self.opts],
              "lr_schedulers": [s["scheduler"].state_dict() for s in self.scheds]}
        if self.grad_guard_enabled:          # only then: a run without the feature writes the checkpoint it always wrote
            sd["grad_guard"] = {"skipped": [(st["skipped"] if st else 0) for st in self.grad_stats()]}
        if self.ema_enabled:                 # likewise; the reference's loaders read ["state_dict"] only
            if self._in_ema_scope:
                raise RuntimeError("state_dict() inside ema_scope(): live and averaged weights are exchanged")
            o = self.opts[0]
            sd["ema"] = {"decay": float(o._ema["decay"]), "warmup": bool(o._ema["warmup"]), "num_updates": o.ema_num_updates,
                         "state_dict": self._ema_state_dict()}
        return sd

    @torch.no_grad()
    def load_state_dict(self, ckpt, strict=True):
        """resume: parameters are written THROUGH the flat-buffer views (copy_), the packed compute-dtype copies are
        invalidated, Adam moments / step counts / LambdaLR positions restored when the checkpoint has them (torch / Lightning
        optimizer-state format or the round-1 flat format; a checkpoint whose optimizers do not match raises)"""
        self.model.load_state_dict(ckpt["state_dict"], strict=strict)
        for b in self.buckets:
            b.fp.attach_grads()
        rt.bump_weights_epoch()
        saved = ckpt.get("optimizer_states", [])
        if saved and len(saved) != len(self.opts):
            import warnings
            warnings.warn(f"checkpoint has {len(saved)} optimizer states, the model configures {len(self.opts)}: "
                          "optimizer moments are NOT restored (weights are)")
            saved = []
        for o, st in zip(self.opts, saved):
            self._load_optimizer_state(o, st)
            o._prepared = False
        for s, st in zip(self.scheds, ckpt.get("lr_schedulers", []) if saved else []):
            s["scheduler"].load_state_dict(st)
            for g, lr in zip(s["scheduler"].optimizer.param_groups, s["scheduler"].get_last_lr()):
                g["lr"] = lr
        self.model.global_step = int(ckpt.get("global_step", 0))
        # skipped-step counters of the non-finite guard: restored where this trainer has the guard's statistics block, absent key
        # (a checkpoint written without the feature) = counters stay as they are
        skipped = ckpt.get("grad_guard", {}).get("skipped", [])
        if len(skipped) == len(self.opts):
            for o, n in zip(self.opts, skipped):
                if getattr(o, "_guard", None) is not None:
                    o._guard["gstat"][4] = int(n)
        # weight EMA: the shadow weights are restored through the views and the count with them; the decay of THIS run applies (as
        # with the clipping flags).  A checkpoint written without the feature: the average starts from the loaded weights
        if self.ema_enabled:
            o = self.opts[0]
            o.flat_e.copy_(o.flat.flat_p)
            o._fstate["ema_updates"] = 0
            o._prepared = False
            ema = ckpt.get("ema")
            if ema is None:
                if not self._warned_no_ema:
                    import warnings
                    warnings.warn("checkpoint has no \"ema\" key: the weight EMA starts from the loaded weights, update count 0")
                    self._warned_no_ema = True
            else:
                names = {id(t): k for k, t in self.model.state_dict(keep_vars=True).items()}
                for i, view in o.ema_tensors().items():
                    t = ema["state_dict"].get(names.get(i))
                    if t is None:
                        if strict:
                            raise KeyError(f"checkpoint's EMA state lacks parameter {names.get(i)!r}")
                        continue
                    if tuple(t.shape) != tuple(view.shape):
                        raise ValueError(f"EMA state of {names[i]}: shape {tuple(t.shape)} != {tuple(view.shape)}")
                    view.copy_(t.to(view.device))
                o._fstate["ema_updates"] = int(ema.get("num_updates", 0))

    def save_checkpoint(self, path):
        """atomic write (temp file + rename): a crash while saving never destroys the previous last.ckpt"""
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        tmp = path + ".tmp"
        torch.save(self.state_dict(), tmp)
        os.replace(tmp, path)

    @torch.no_grad()
    def validate(self, batches, image_logger=None):
        """Lightning's validation loop (train.py:233-262 runs it every `check_val_every_n_epoch`): eval mode, `validation_step` on every
        batch, the logged scalars averaged over the batches -- and over the ranks under data parallelism (`sync_dist=True` of
        dqvae_dual_entropy.py:185-201) -- train mode restored.  -> {name: float}
        `image_logger` (imagelog.ImageLogger): offered every validation batch with split "val" (on_validation_batch_end of the
        reference's CaptionImageLogger)"""
        m = self.model
        was_training = m.training
        m.eval()
        sums, n = {}, 0
        try:
            with self.ema_scope():           # weight EMA on: metrics and pictures of the averaged model; a no-op otherwise
                for i, b in enumerate(batches):
                    m._logged = {}
                    m.validation_step(b, i)
                    if image_logger is not None:
                        image_logger.maybe_log(m, b, i, split="val")
                    for k, v in m._logged.items():
                        if torch.is_tensor(v) and v.numel() == 1 or isinstance(v, (int, float)):
                            sums[k] = sums.get(k, 0.0) + (v.detach().double() if torch.is_tensor(v) else float(v))
                    n += 1
        finally:
            m.train(was_training)
            m._logged = {}
        if n == 0:
            return {}
        keys = sorted(sums)
        dev = next(m.parameters()).device
        vec = torch.stack([torch.as_tensor(sums[k], dtype=torch.float64, device=dev).reshape(()) for k in keys]) / n
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(vec)
            vec /= dist.get_world_size()
        return {k: float(x) for k, x in zip(keys, vec.cpu())}

    def fit(self, batch_fn, ckpt_path=None, save_every=0, is_rank0=True, val_fn=None, val_every=0, save_top_k=0, image_logger=None):
        """`ckpt_path` + `save_every` (steps): rank 0 rewrites last.ckpt periodically, so a preempted run resumes with `-r`.
        `val_fn()` -> iterable of validation batches, run every `val_every` steps and after the last one; with a `monitor` on the model
        (the YAMLs say `monitor: val_rec_loss`) the `save_top_k` best checkpoints by that metric are kept next to last.ckpt as
        `epoch=<e>-<monitor>=<value>.ckpt` -- pytorch_lightning.callbacks.ModelCheckpoint(monitor, save_top_k, save_last=True, mode="min")
        of the reference's train.py:152-183.
        `image_logger` (imagelog.ImageLogger; None = no pictures, the default): offered every batch after its train step and every
        validation batch; flushed before fit returns, also when a step raises.
        With a `metrics_logger` (constructor) the validation means are written as `<key>_epoch` rows, a partial last epoch gets its
        epoch row and the log files are closed before fit returns"""
        self.model.train()
        best = []                                     # (value, path), ascending
        monitor = getattr(self.model, "monitor", None)
        if ckpt_path and is_rank0 and save_top_k and monitor:
            # a resumed run (-r) starts from the monitored checkpoints already on disk (Lightning keeps best_k_models inside the
            # checkpoint; here the file names carry the value): without this, old files were never compared or pruned again
            import glob
            import re
            pat = re.compile(r"epoch=\d+-" + re.escape(monitor) + r"=(-?\d+(?:\.\d+)?(?:[eE][-+]?\d+)?)\.ckpt$")
            for f in glob.glob(os.path.join(os.path.dirname(os.path.abspath(ckpt_path)), f"epoch=*-{glob.escape(monitor)}=*.ckpt")):
                mt = pat.search(os.path.basename(f))
                if mt:
                    best.append((float(mt.group(1)), f))
            best.sort(key=lambda t: t[0])
            for _, old in best[save_top_k:]:
                os.remove(old)
            del best[save_top_k:]

        def run_validation(step):
            metrics = self.validate(val_fn(), image_logger=image_logger if is_rank0 else None)
            self.last_val_metrics = metrics
            if self.metrics_logger is not None and is_rank0:
                self.metrics_logger.log_validation(metrics, step // max(1, int(getattr(self.model, "steps_per_epoch", 1) or 1)), step)
            if is_rank0 and metrics:
                print(f"validation @ step {step + 1}{' (EMA weights)' if self.ema_enabled else ''}: " + " ".join(f"{k}={v:.5f}" for k, v in metrics.items()), flush=True)
            if not (ckpt_path and is_rank0 and save_top_k and monitor and monitor in metrics):
                return
            val = metrics[monitor]
            if len(best) < save_top_k or val < best[-1][0]:
                epoch = step // max(1, int(getattr(self.model, "steps_per_epoch", 1) or 1))
                path = os.path.join(os.path.dirname(os.path.abspath(ckpt_path)), f"epoch={epoch}-{monitor}={val:.4f}.ckpt")
                self.save_checkpoint(path)
                best.append((val, path))
                best.sort(key=lambda t: t[0])
                for _, old in best[save_top_k:]:
                    if os.path.exists(old) and old != path:
                        os.remove(old)
                del best[save_top_k:]

        if not is_rank0:
            image_logger = None
        try:
            for step in range(int(self.model.global_step), self.max_steps):
                batch = batch_fn(step)
                losses = self.train_step(batch, step)
                if image_logger is not None:
                    image_logger.maybe_log(self.model, batch, step, split="train")
                if self.log_every and step % self.log_every == 0:
                    line = f"step {step}: " + " ".join(f"{float(l):.5f}" for l in losses)      # float(l) synchronises
                    if self.grad_guard_enabled:
                        line += "".join(f" | opt{i} gnorm={st['norm']:.4g} coef={st['coef']:.4g} skipped={st['skipped']}"
                                        for i, st in enumerate(self.grad_stats()) if st)
                    if self.ema_enabled:                  # host-side value of the step just taken: no device read
                        line += f" | ema_d={self.opts[0]._ema['last']:.6g}"
                    print(line, flush=True)
                if ckpt_path and save_every and is_rank0 and (step + 1) % save_every == 0 and step + 1 < self.max_steps:
                    self.save_checkpoint(ckpt_path)
                if val_fn is not None and val_every and ((step + 1) % val_every == 0 or step + 1 == self.max_steps):
                    run_validation(step)
            if self.metrics_logger is not None:
                self.metrics_logger.finish(self)          # the epoch row of a partial last epoch
        finally:
            if image_logger is not None:
                image_logger.flush()
            if self.metrics_logger is not None:
                self.metrics_logger.close()
        if ckpt_path and is_rank0:
            self.save_checkpoint(ckpt_path)
