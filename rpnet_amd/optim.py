"""Adam over the flat gradient bucket as one C call (include/rpnet_optim_abi.h, csrc/optim.hip).

torch.optim.Adam makes about eight element-wise passes over the bucket's parameters and keeps its step count on the host; the update
needs ONE pass (read g, p, m, v; write p, m, v) and its step count and learning rate can live in device memory, so that the step is
two launches with nothing read back: replayable in a captured graph.

The semantics are torch.optim.Adam(amsgrad=False, maximize=False) with L2 weight decay, in fp32, and the state dict is Adam's
(state[i] = {step, exp_avg, exp_avg_sq} + param_groups): a run begun under either optimizer resumes under the other.
"""
import ctypes as C

import numpy as np
import torch

from . import hip

_HYPER_FIELDS = ("lr", "beta1", "beta2", "eps", "weight_decay", "grad_scale")      # struct rpnet_adam_hyper: six doubles,
_HYPER_STEP = 6                                                                    # the int64 step, ten floats: 96 bytes
_HYPER_WORDS = 12


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
    sync_lr() between replays."""

    def __init__(self, bucket, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_scale=1.0):
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
