"""Adam over the flat gradient bucket as one C call (include/rpnet_optim_abi.h, csrc/optim.hip).

torch.optim.Adam makes about eight element-wise passes over the bucket's parameters and keeps its step count on the host; the update
needs ONE pass (read g, p, m, v; write p, m, v) and its step count and learning rate can live in device memory, so that the step is
two launches with nothing read back: replayable in a captured graph.

The semantics are torch.optim.Adam(amsgrad=False, maximize=False) with L2 weight decay, in fp32, and the state dict is Adam's
(state[i] = {step, exp_avg, exp_avg_sq} + param_groups): a run begun under either optimizer resumes under the other.

The gradient guard (include/rpnet_guard_abi.h): FusedAdam(max_grad_norm=, skip_nonfinite=, history=) puts the gradient's 2-norm
(fp64, one more read of the bucket), torch.nn.utils.clip_grad_norm_'s coefficient and the decision to skip a step whose gradient
holds an inf or a NaN in front of the update, all in device memory: three launches, still nothing read back.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import hip

_HYPER_FIELDS = ("lr", "beta1", "beta2", "eps", "weight_decay", "grad_scale")      # struct rpnet_adam_hyper: six doubles,
_HYPER_STEP = 6                                                                    # the int64 step, ten floats: 96 bytes
_HYPER_WORDS = 12
# struct rpnet_grad_guard as ten 8-byte words: max_norm, skip_nonfinite, history_capacity | sumsq, norm, coef, (coef_f, skip), attempt,
_GUARD_WORDS = 10                                                                  # skipped, clipped: 80 bytes
_G_NORM, _G_COEF, _G_PAIR, _G_ATTEMPT, _G_SKIPPED, _G_CLIPPED = 4, 5, 6, 7, 8, 9
_HISTORY_ROW = 3                                                                   # RPNET_GUARD_HISTORY_ROW: norm, coef, skip


def clip_coefficient(norm, max_norm):
    """the factor a gradient of 2-norm `norm` is multiplied by under the threshold `max_norm`: c = max_norm / (norm + 1e-6), c when
    c <= 1 or c is NaN, else 1.  This is torch.nn.utils.clip_grad_norm_'s formula with its constant, and what the guarded step
    forms in fp64 on the device.  Host only, Python floats."""
    norm, max_norm = float(norm), float(max_norm)
    try:
        c = max_norm / (norm + 1e-6)
    except ZeroDivisionError:               # norm == -1e-6 cannot come from a norm; keep the function total
        c = math.inf
    return 1.0 if c > 1.0 else c


def _check_guard_args(max_grad_norm, skip_nonfinite, history):
    """-> (the guard's max_norm, skip_nonfinite, history) as float, bool, int, or ValueError / TypeError; no GPU call"""
    if max_grad_norm is None:
        max_norm = math.inf
    else:
        max_norm = float(max_grad_norm)
        if not max_norm > 0.0:
            raise ValueError(f"FusedAdam: max_grad_norm={max_grad_norm!r} (a threshold above 0, or None for no clipping)")
    if not isinstance(skip_nonfinite, (bool, int)):
        raise TypeError(f"FusedAdam: skip_nonfinite={skip_nonfinite!r} (True or False)")
    if isinstance(history, bool) or not isinstance(history, int):
        raise TypeError(f"FusedAdam: history={history!r} (the number of attempts the ring keeps, an int)")
    if history < 0:
        raise ValueError(f"FusedAdam: history={history} (0 for no ring)")
    return max_norm, bool(skip_nonfinite), history


def guard_block(max_norm, skip_nonfinite, history):
    """rpnet_grad_guard_init: struct rpnet_grad_guard for these settings as a float64 tensor of ten words on the host"""
    host = torch.zeros(_GUARD_WORDS, dtype=torch.float64)
    rc = hip.query("rpnet_grad_guard_init", host.data_ptr(), float(max_norm), int(bool(skip_nonfinite)), int(history))
    if rc != 0:
        raise ValueError(f"rpnet_grad_guard_init failed (rc={rc}): {hip.query('rpnet_last_error_string').decode()}")
    return host


def plan_chunks(ptrs, counts, offsets):
    """rpnet_adam_plan for parameters at device addresses `ptrs` with `counts` elements at `offsets` of the flat buffers ->
    (the chunk table as a uint8 numpy array, the number of chunks).  Host only: nothing is dereferenced, no GPU call."""
    n = len(ptrs)
    a_ptr = (C.c_void_p * n)(*ptrs)
    a_cnt = (C.c_int64 * n)(*counts)
    a_off = (C.c_int64 * n)(*offsets)
    nbytes = hip.query("rpnet_adam_plan_bytes", a_cnt, n)
    if nbytes == 0:
        raise RuntimeError(f"rpnet_adam_plan_bytes failed: {hip.query('rpnet_last_error_string').decode()}")
    table = np.zeros(nbytes, dtype=np.uint8)
    n_chunks = C.c_int64(0)
    rc = hip.query("rpnet_adam_plan", a_ptr, a_cnt, a_off, n, table.ctypes.data, nbytes, C.byref(n_chunks))
    if rc != 0:
        raise RuntimeError(f"rpnet_adam_plan failed (rc={rc}): {hip.query('rpnet_last_error_string').decode()}")
    return table, n_chunks.value


class FusedAdam(torch.optim.Optimizer):
    """Adam over the parameters of a rpnet_amd.parallel.FlatGradBucket: one param group holding [p for _, p in bucket.params].

    The gradients are read from bucket.flat (never zeroed here), the moments live in two flat buffers laid out like it, the
    parameters keep their own storage: state_dict() of the model, .to(), the weight packs and checkpoints see nothing new.
    grad_scale multiplies the gradient inside the update (1 / world behind bucket.allreduce(average=False)).

    The chunk table is planned once from the parameters' addresses; step() raises when a parameter has moved since (net.to(...),
    p.data = ...).  The learning rate is read from param_groups[0]["lr"] at every step and uploaded when it changed (8 bytes from
    pinned memory, nothing when it did not), which is what lr_scheduler.StepLR needs; the other hyper-parameters are uploaded at
    construction and by load_state_dict().  step() can be captured with torch.cuda.graph: upload a changed learning rate with
    sync_lr() between replays.

    max_grad_norm, skip_nonfinite, history: the gradient guard.  With the defaults (None, False, 0) step() is the two launches above
    and nothing is allocated for the guard.  With any of them set, step() is rpnet_adam_step_guarded, three launches:
      * the 2-norm of grad_scale * g over the whole bucket, summed in fp64 in a fixed order;
      * max_grad_norm: the gradient the update sees is clip_coefficient(norm, max_grad_norm) * (grad_scale * g), the result of
        flat.mul_(grad_scale) followed by torch.nn.utils.clip_grad_norm_(params, max_grad_norm).  Unlike clip_grad_norm_ the bucket
        is NOT rewritten: bucket.flat and every p.grad hold the unclipped gradient after the step;
      * skip_nonfinite: when the sum of squares is inf or NaN the step is not taken: p, exp_avg, exp_avg_sq and the step count stay
        as they are and guard_stats()["skipped"] goes up by one.  Without it such a gradient goes the way it goes through
        clip_grad_norm_(error_if_nonfinite=False): a NaN norm makes every parameter NaN;
      * history: a ring in device memory that keeps (norm, coef, skip) of the last `history` attempts, for guard_stats().
    Neither is a param-group key: state_dict() stays torch.optim.Adam's, the counters are not saved and start at zero after a resume.
    step_count() counts steps TAKEN.  A captured guarded step replays like the plain one; set_max_grad_norm() between replays.
    Data-parallel: behind bucket.allreduce(average=False) every rank holds the same sum, hence the same norm and the same decision."""

    def __init__(self, bucket, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0, max_grad_norm=None,
                 skip_nonfinite=False, history=0):
        max_norm, skip_nonfinite, history = _check_guard_args(max_grad_norm, skip_nonfinite, history)
        params = [p for _, p in bucket.params]
        hip.require_gpu(bucket.flat, *params)
        if not (0.0 <= lr and 0.0 <= eps and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and 0.0 <= weight_decay):
            raise ValueError(f"FusedAdam: lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        # the param group carries exactly the keys of the installed torch.optim.Adam, so that the state dicts are interchangeable
        defaults = dict(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr, betas=betas, eps=eps,
                                         weight_decay=weight_decay).defaults)
        super().__init__(params, defaults)
        self.bucket = bucket
        self.names = [n for n, _ in bucket.params]
        self.grad_scale = float(grad_scale)
        flat = bucket.flat
        if flat.dtype != torch.float32 or not flat.is_contiguous():
            raise RuntimeError("FusedAdam: the bucket's flat buffer must be contiguous fp32")
        self.counts, self.offsets, off = [], [], 0
        for n, p in bucket.params:
            if p.device != flat.device or p.dtype != torch.float32:
                raise RuntimeError(f"FusedAdam: parameter {n} is {p.dtype} on {p.device}, the bucket is fp32 on {flat.device}")
            if not p.is_contiguous():
                raise RuntimeError(f"FusedAdam: parameter {n} is not contiguous")
            if p.grad is None or p.grad.data_ptr() != flat.data_ptr() + 4 * off or p.grad.numel() != p.numel() or not p.grad.is_contiguous():
                raise RuntimeError(f"FusedAdam: the gradient of parameter {n} is not its view of the bucket's flat buffer")
            self.counts.append(p.numel())
            self.offsets.append(off)
            off += p.numel()
        self.ptrs = [p.data_ptr() for p in params]
        table, self.n_chunks = plan_chunks(self.ptrs, self.counts, self.offsets)
        self.table = torch.from_numpy(table).to(flat.device)
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        self.hyper = torch.zeros(_HYPER_WORDS, dtype=torch.float64, device=flat.device)
        self._lr_host = torch.zeros(1, dtype=torch.float64).pin_memory()
        self._lr_event = None
        self._lr_uploaded = None
        self._upload_hyper(step=0)
        self.guarded = max_grad_norm is not None or skip_nonfinite or history > 0
        self.max_grad_norm, self.skip_nonfinite, self.history = max_norm, skip_nonfinite, history
        self.partials = self.guard = self.ring = None            # the guard's buffers: made once, here or never
        self._probe = None                                       # grad_norm()'s own partial sums and guard block
        self._max_norm_host = self._max_norm_event = None
        if self.guarded:
            self.partials = torch.empty(self.n_chunks, dtype=torch.float64, device=flat.device)
            self.guard = guard_block(max_norm, skip_nonfinite, history).to(flat.device)
            self.ring = torch.zeros(history * _HISTORY_ROW, dtype=torch.float64, device=flat.device) if history else None
            self._max_norm_host = torch.zeros(1, dtype=torch.float64).pin_memory()

    # ------------------------------------------------------------------------------------------------ the device block
    def _upload_hyper(self, step):
        g = self.param_groups[0]
        host = torch.zeros(_HYPER_WORDS, dtype=torch.float64)
        vals = dict(lr=g["lr"], beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], weight_decay=g["weight_decay"],
                    grad_scale=self.grad_scale)
        for i, k in enumerate(_HYPER_FIELDS):
            host[i] = float(vals[k])
        host.view(torch.int64)[_HYPER_STEP] = int(step)
        self.hyper.copy_(host)
        self._lr_uploaded = float(g["lr"])

    def sync_lr(self):
        """upload param_groups[0]["lr"] when it differs from what the device holds (step() calls this; call it yourself
        between two replays of a captured step)"""
        lr = float(self.param_groups[0]["lr"])
        if lr == self._lr_uploaded:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdam: the learning rate changed inside a graph capture: call sync_lr() before the capture "
                               "and between replays")
        if self._lr_event is not None:
            self._lr_event.synchronize()     # the pinned word is free again once the copy that read it last has run
        self._lr_host[0] = lr
        self.hyper[0:1].copy_(self._lr_host, non_blocking=True)
        self._lr_event = torch.cuda.Event()
        self._lr_event.record()
        self._lr_uploaded = lr

    def step_count(self):
        """steps taken so far, read from the device (synchronises)"""
        return int(self.hyper.view(torch.int64)[_HYPER_STEP].item())

    # ------------------------------------------------------------------------------------------------ the guard
    def set_max_grad_norm(self, max_grad_norm):
        """a new clip threshold (None: no clipping) for an optimizer built with the guard: 8 bytes from pinned memory; between
        two replays of a captured step it takes effect without a recapture, inside a capture it is refused"""
        max_norm = _check_guard_args(max_grad_norm, False, 0)[0]
        if not self.guarded:
            raise RuntimeError("FusedAdam: built without the gradient guard (max_grad_norm=None, skip_nonfinite=False, history=0); "
                               "its step has no threshold to set")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdam: set_max_grad_norm() inside a graph capture: call it before the capture and between replays")
        if self._max_norm_event is not None:
            self._max_norm_event.synchronize()
        self._max_norm_host[0] = max_norm
        self.guard[0:1].copy_(self._max_norm_host, non_blocking=True)
        self._max_norm_event = torch.cuda.Event()
        self._max_norm_event.record()
        self.max_grad_norm = max_norm

    def guard_stats(self):
        """what the guard holds, read from the device (synchronises): norm, coef and skip of the last attempt, the counters
        attempt / skipped / clipped, and history: [(norm, coef, skip), ...] of the last min(attempt, history) attempts, oldest first"""
        if not self.guarded:
            raise RuntimeError("FusedAdam: built without the gradient guard")
        host = self.guard.cpu()
        words = host.view(torch.int64)
        attempt = int(words[_G_ATTEMPT])
        out = {"norm": float(host[_G_NORM]), "coef": float(host[_G_COEF]), "skip": int(host.view(torch.int32)[2 * _G_PAIR + 1]),
               "attempt": attempt, "skipped": int(words[_G_SKIPPED]), "clipped": int(words[_G_CLIPPED]), "history": []}
        if self.ring is not None:
            rows = self.ring.cpu().view(self.history, _HISTORY_ROW)
            for a in range(max(0, attempt - self.history), attempt):
                norm, coef, skip = rows[a % self.history].tolist()
                out["history"].append((norm, coef, int(skip)))
        return out

    def grad_norm(self):
        """the 2-norm of grad_scale * bucket.flat as the guard forms it (rpnet_grad_sumsq alone: two launches, fp64, nothing read
        back) -> a 0-dim float64 tensor on the device.  Works without the guard too; its buffers are grad_norm()'s own, so the
        counters and the ring of guard_stats() see steps only."""
        if self._probe is None:
            flat = self.bucket.flat
            self._probe = (torch.empty(self.n_chunks, dtype=torch.float64, device=flat.device),
                           guard_block(math.inf, False, 0).to(flat.device))
        partials, guard = self._probe
        hip.call("rpnet_grad_sumsq", hip.ptr(self.table), self.n_chunks, hip.ptr(self.bucket.flat), hip.ptr(partials), hip.ptr(guard),
                 None)
        return guard[_G_NORM] * abs(self.grad_scale)

    # ------------------------------------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise RuntimeError("FusedAdam.step takes no closure")
        for n, p, ptr in zip(self.names, self.param_groups[0]["params"], self.ptrs):
            if p.data_ptr() != ptr:
                raise RuntimeError(f"FusedAdam: parameter {n} has moved since the chunk table was planned (net.to(...) or an "
                                   "assignment to .data): build a new FlatGradBucket and FusedAdam")
        self.sync_lr()
        if self.guarded:
            hip.call("rpnet_adam_step_guarded", hip.ptr(self.table), self.n_chunks, hip.ptr(self.bucket.flat), hip.ptr(self.exp_avg),
                     hip.ptr(self.exp_avg_sq), hip.ptr(self.hyper), hip.ptr(self.partials), hip.ptr(self.guard), hip.ptr(self.ring))
        else:
            hip.call("rpnet_adam_step", hip.ptr(self.table), self.n_chunks, hip.ptr(self.bucket.flat), hip.ptr(self.exp_avg),
                     hip.ptr(self.exp_avg_sq), hip.ptr(self.hyper))
        return None

    def zero_grad(self, set_to_none=False):
        """the gradients are views of the bucket: one memset (setting them to None would cut the views)"""
        self.bucket.zero()

    # ------------------------------------------------------------------------------------------------ torch.optim.Adam's state dict
    def state_dict(self):
        step = self.step_count()
        if step > 0:
            for p, k, o in zip(self.param_groups[0]["params"], self.counts, self.offsets):
                self.state[p] = {"step": torch.tensor(float(step), dtype=torch.float32),
                                 "exp_avg": self.exp_avg[o:o + k].view_as(p), "exp_avg_sq": self.exp_avg_sq[o:o + k].view_as(p)}
        try:
            return super().state_dict()
        finally:
            self.state.clear()

    def load_state_dict(self, state_dict):
        for g in state_dict["param_groups"]:
            for flag in ("amsgrad", "maximize"):
                if g.get(flag, False):
                    raise RuntimeError(f"FusedAdam: the state dict was written with {flag}=True; the kernel is "
                                       "torch.optim.Adam(amsgrad=False, maximize=False)")
        super().load_state_dict(state_dict)
        params = self.param_groups[0]["params"]
        if self.state and len(self.state) != len(params):
            raise RuntimeError(f"FusedAdam: the state dict holds state for {len(self.state)} of {len(params)} parameters")
        steps = {int(float(s["step"])) for s in self.state.values()}
        if len(steps) > 1:
            raise RuntimeError(f"FusedAdam: the parameters of the state dict are at different steps {sorted(steps)}; one count is kept")
        if not self.state:
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
        for p, k, o in zip(params, self.counts, self.offsets):
            if p in self.state:
                self.exp_avg[o:o + k].copy_(self.state[p]["exp_avg"].reshape(-1))
                self.exp_avg_sq[o:o + k].copy_(self.state[p]["exp_avg_sq"].reshape(-1))
        self.state.clear()
        self._upload_hyper(steps.pop() if steps else 0)
