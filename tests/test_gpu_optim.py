"""The Adam step over the flat gradient bucket (include/rpnet_optim_abi.h, csrc/optim.hip, rpnet_amd/optim.py: FusedAdam).

Yardstick of every numerical comparison: torch's own Adam.  torch.optim.Adam runs in fp32 on the CPU and in fp64 (the same
optimizer on .double() copies) on the same seeded inputs; per parameter and per tensor x of p, m, v, err_torch = max |x_torch32 -
x_64| and the kernel has to satisfy  max |x_hip - x_64| <= max(2 * err_torch, one fp32 ulp at max |x_64| of that tensor):  another,
equally valid order of the operations is one more rounding in either direction, and the ulp floor covers tensors where torch
happens to be exact.  Every check prints `PARITY optim case tensor err_hip err_torch ratio`; profiles/optim_parity.txt keeps them.

Inputs: p ~ N(0, 1), |g| log-uniform in 1e-6 .. 1e2 with random sign, so no operand is denormal.

Shapes: the smallest at which the kernel takes another path - a chunk is 4096 elements (RPNET_ADAM_CHUNK), so 4097 and 8193 put
chunk boundaries inside a parameter; behind counts 1, 3, 5 every flat offset but 0 and 4 is misaligned (element-by-element chunks;
the 5 at offset 4 is one quad and a single element); 6151 at an aligned offset is one full 16-byte chunk and one of 513 quads + 3
single elements, and the 7 behind it at flat offset 6151 go element by element.
"""
import math
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 8            # sentinel elements between and around the tensors (a multiple of 4: 16-byte alignment is kept where wanted)
SENTINEL = -777.25
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8

LISTS = {"awkward": [1, 3, 5, 64, 4096, 4097, 8193], "fast": [64, 576, 12288], "one": [1], "tail": [6151, 7]}


def _grad(rs, n):
    return (np.sign(rs.standard_normal(n)) * 10.0 ** rs.uniform(-6, 2, n)).astype(np.float32)


def _inputs(counts, seed, steps):
    rs = np.random.RandomState(seed)
    p0 = [rs.standard_normal(k).astype(np.float32) for k in counts]
    gs = [[_grad(rs, k) for k in counts] for _ in range(steps)]
    return p0, gs


def torch_adam(p0, grads, dtype, lr=LR, weight_decay=0.0, grad_scale=1.0, state=None, lrs=None):
    """torch.optim.Adam on the CPU in `dtype`; grads[step][param] (fp32, scaled by grad_scale in `dtype` first, as flat.mul_ does);
    lrs: the learning rate of each step (a scheduler's); state: an Adam state dict to resume from -> (p, m, v lists, the optimizer)"""
    ps = [torch.nn.Parameter(torch.from_numpy(a).to(dtype).clone()) for a in p0]
    opt = torch.optim.Adam(ps, lr=lr, betas=BETAS, eps=EPS, weight_decay=weight_decay)
    if state is not None:
        opt.load_state_dict(state)
    for k, gk in enumerate(grads):
        if lrs is not None:
            opt.param_groups[0]["lr"] = lrs[k]
        for p, g in zip(ps, gk):
            p.grad = torch.from_numpy(g).to(dtype) * grad_scale
        opt.step()
    return ([p.detach().numpy() for p in ps], [opt.state[p]["exp_avg"].numpy() for p in ps],
            [opt.state[p]["exp_avg_sq"].numpy() for p in ps], opt)


def yardstick(case, hip_pmv, t32, t64, names=None):
    """hold p, m, v of every parameter to the yardstick of the module docstring"""
    problems = []
    for tname, xh, x32, x64 in zip("pmv", hip_pmv, t32, t64):
        for i, (h, a, b) in enumerate(zip(xh, x32, x64)):
            b = np.asarray(b, dtype=np.float64).reshape(-1)
            err_t = float(np.abs(np.asarray(a, dtype=np.float64).reshape(-1) - b).max())
            err_h = float(np.abs(np.asarray(h, dtype=np.float64).reshape(-1) - b).max())
            ulp = float(np.spacing(np.float32(np.abs(b).max())))
            label = names[i] if names else f"param{i}[{b.size}]"
            print(f"PARITY optim {case} {tname} {label} err_hip {err_h:.3e} err_torch {err_t:.3e} "
                  f"ratio {err_h / err_t if err_t > 0 else float('nan'):.3f} ulp {ulp:.3e}")
            if not err_h <= max(2.0 * err_t, ulp):
                problems.append(f"{case} {tname} {label}: err_hip {err_h:.3e} > max(2 * {err_t:.3e}, ulp {ulp:.3e})")
    assert not problems, "\n".join(problems)


class RawAdam:
    """rpnet_adam_plan + rpnet_adam_step on buffers of the test's making: every parameter is a view into ONE larger tensor, g, m
    and v are slices of larger buffers, SENTINEL on both sides of each.  shift / flat_shift: elements by which the parameter
    storage / the three flat buffers are moved off their 16-byte alignment."""

    def __init__(self, counts, p0, weight_decay=0.0, grad_scale=1.0, lr=LR, shift=0, flat_shift=0):
        from rpnet_amd.optim import plan_chunks
        self.counts, self.offsets, self.p_at = list(counts), [], []
        off, at = 0, GAP + shift
        for k in counts:
            self.offsets.append(off)
            self.p_at.append(at)
            off += k
            at += (k + 3) // 4 * 4 + GAP            # the next parameter starts on the same 16-byte phase
        self.total = off
        self.p_buf = torch.full((at,), SENTINEL, device=DEV)
        self.lo = GAP + flat_shift
        self.g_buf, self.m_buf, self.v_buf = (torch.full((self.lo + self.total + GAP,), SENTINEL, device=DEV) for _ in range(3))
        self.p = [self.p_buf[a:a + k] for a, k in zip(self.p_at, counts)]
        self.g, self.m, self.v = (b[self.lo:self.lo + self.total] for b in (self.g_buf, self.m_buf, self.v_buf))
        for i, (view, a) in enumerate(zip(self.p, p0)):
            view.copy_(torch.from_numpy(a))
        self.m.zero_()
        self.v.zero_()
        table, self.n_chunks = plan_chunks([v.data_ptr() for v in self.p], self.counts, self.offsets)
        self.table_host = table
        self.table = torch.from_numpy(table).to(DEV)
        hyper = torch.zeros(12, dtype=torch.float64)
        hyper[:6] = torch.tensor([lr, BETAS[0], BETAS[1], EPS, weight_decay, grad_scale], dtype=torch.float64)
        self.hyper = hyper.to(DEV)

    def results(self):
        torch.cuda.synchronize()
        cut = lambda flat: [flat[o:o + k].cpu().numpy() for o, k in zip(self.offsets, self.counts)]  # noqa: E731
        return [v.cpu().numpy() for v in self.p], cut(self.m), cut(self.v)

    def sentinels_intact(self):
        keep = torch.ones_like(self.p_buf, dtype=torch.bool)
        for a, k in zip(self.p_at, self.counts):
            keep[a:a + k] = False
        ok = bool((self.p_buf[keep] == SENTINEL).all())
        for b in (self.g_buf, self.m_buf, self.v_buf):
            ok = ok and bool((b[:self.lo] == SENTINEL).all()) and bool((b[self.lo + self.total:] == SENTINEL).all())
        return ok

    def steps_taken(self):
        return int(self.hyper.view(torch.int64)[6].item())


def _step(raw, grads):
    """one rpnet_adam_step on the buffers of a RawAdam, with the gradients of this step"""
    from rpnet_amd import hip
    raw.g.copy_(torch.from_numpy(np.concatenate(grads)))
    hip.call("rpnet_adam_step", hip.ptr(raw.table), raw.n_chunks, hip.ptr(raw.g), hip.ptr(raw.m), hip.ptr(raw.v), hip.ptr(raw.hyper))


def _run_case(name, counts, steps, weight_decay, grad_scale, seed, shift=0, flat_shift=0):
    p0, grads = _inputs(counts, seed, steps)
    raw = RawAdam(counts, p0, weight_decay=weight_decay, grad_scale=grad_scale, shift=shift, flat_shift=flat_shift)
    for gk in grads:
        _step(raw, gk)
    got = raw.results()
    assert raw.sentinels_intact(), f"{name}: a sentinel beside p, g, m or v was overwritten"
    assert raw.steps_taken() == steps
    t32 = torch_adam(p0, grads, torch.float32, weight_decay=weight_decay, grad_scale=grad_scale)[:3]
    t64 = torch_adam(p0, grads, torch.float64, weight_decay=weight_decay, grad_scale=grad_scale)[:3]
    yardstick(name, got, t32, t64)
    return got, raw


@pytest.mark.parametrize("lname", list(LISTS))
def test_awkward_sizes(lname):
    """rpnet_adam_step on raw buffers: one step with weight_decay 0 / 1e-2 and grad_scale 1 / 0.5, then 20 steps with a fresh gradient each (the bias
    corrections), over every list of counts; sentinels around p, g, m, v stay intact; the path of every chunk is the expected one"""
    counts = LISTS[lname]
    for wd in (0.0, 1e-2):
        for gs in (1.0, 0.5):
            _run_case(f"{lname}/1step/wd{wd:g}/gs{gs:g}", counts, 1, wd, gs, seed=11)
    _, raw = _run_case(f"{lname}/20steps/wd0.01/gs1", counts, 20, 1e-2, 1.0, seed=12)
    vec = np.frombuffer(raw.table_host.tobytes(), dtype=np.int32).reshape(-1, 6)[:, 5]
    start = np.frombuffer(raw.table_host.tobytes(), dtype=np.int64).reshape(-1, 3)[:, 1]
    assert list(vec) == [int(s % 4 == 0) for s in start]          # the parameter views are all 16-byte aligned here
    if lname == "awkward":
        assert vec.sum() == 2 and len(vec) == 5 + 2 + 3           # flat offsets 0 and 4 (= 1 + 3) are the only multiples of 4
    if lname == "fast":
        assert vec.all()
    if lname == "tail":
        assert list(vec) == [1, 1, 0]                             # 6151 at 0: two 16-byte chunks; the 7 behind it starts at 6151


def test_misaligned_parameter_pointer():
    """rpnet_adam_step with the parameter storage at element offset 1 of its tensor (4-byte, not 16-byte aligned) while every flat
    offset is a multiple of 4: the element-by-element path chosen by the pointer; then with g, m, v themselves off the 16-byte
    grid (the launch without 16-byte accesses)"""
    counts = LISTS["fast"]
    _, raw = _run_case("misaligned_ptr/1step", counts, 1, 1e-2, 1.0, seed=13, shift=1)
    assert all(v.data_ptr() % 16 == 4 for v in raw.p)
    vec = np.frombuffer(raw.table_host.tobytes(), dtype=np.int32).reshape(-1, 6)[:, 5]
    assert not vec.any()
    _run_case("misaligned_ptr/20steps", counts, 20, 1e-2, 0.5, seed=14, shift=1)
    _run_case("misaligned_flat/20steps", LISTS["tail"], 20, 1e-2, 1.0, seed=14, flat_shift=3)


def test_zero_gradient_and_repeatability():
    counts = LISTS["awkward"]
    p0, _ = _inputs(counts, 15, 0)
    raw = RawAdam(counts, p0)
    _step(raw, [np.zeros(k, np.float32) for k in counts])
    p, m, v = raw.results()
    for a, b, mm, vv in zip(p, p0, m, v):
        assert a.tobytes() == b.tobytes()                      # bit-identical, -0.0 included
        assert mm.tobytes() == np.zeros_like(mm).tobytes() and vv.tobytes() == np.zeros_like(vv).tobytes()
    assert raw.sentinels_intact()
    runs = []
    for _ in range(2):
        p0, grads = _inputs(counts, 12, 20)
        raw = RawAdam(counts, p0, weight_decay=1e-2)
        for gk in grads:
            _step(raw, gk)
        runs.append(raw.results())
    for xa, xb in zip(runs[0], runs[1]):
        for a, b in zip(xa, xb):
            assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------ FusedAdam
class _Net(torch.nn.Module):
    def __init__(self, counts, p0):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(a).clone()) for a in p0])


def _fused(counts, p0, **kw):
    from rpnet_amd.optim import FusedAdam
    from rpnet_amd.parallel import FlatGradBucket
    net = _Net(counts, p0).to(DEV)
    bucket = FlatGradBucket(net, skip_prefixes=(), split_at=())
    return net, bucket, FusedAdam(bucket, lr=LR, betas=BETAS, eps=EPS, **kw)


def _set_grads(bucket, grads):
    bucket.flat.copy_(torch.from_numpy(np.concatenate(grads)))


def _fused_results(net, opt):
    torch.cuda.synchronize()
    cut = lambda flat: [flat[o:o + k].cpu().numpy() for o, k in zip(opt.offsets, opt.counts)]  # noqa: E731
    return [p.detach().cpu().numpy() for p in net.ps], cut(opt.exp_avg), cut(opt.exp_avg_sq)


def test_resume_from_torch_adam_and_back():
    counts = [5, 64, 4097]
    p0, grads = _inputs(counts, 16, 1003)
    p32, _, _, opt32 = torch_adam(p0, grads[:1000], torch.float32, weight_decay=1e-2)
    p64, _, _, opt64 = torch_adam(p0, grads[:1000], torch.float64, weight_decay=1e-2)
    sd = opt32.state_dict()
    assert int(sd["state"][0]["step"]) == 1000
    net, bucket, opt = _fused(counts, [a.copy() for a in p32], weight_decay=1e-2)
    opt.load_state_dict({"state": {i: {k: (v.to(DEV) if k != "step" else v.clone()) for k, v in s.items()}
                                   for i, s in sd["state"].items()}, "param_groups": sd["param_groups"]})
    assert opt.step_count() == 1000
    for gk in grads[1000:]:
        _set_grads(bucket, gk)
        opt.step()
    got = _fused_results(net, opt)
    # torch continuing, fp32 and fp64 each from its own 1000 steps
    t32 = torch_adam(p32, grads[1000:], torch.float32, weight_decay=1e-2, state=opt32.state_dict())[:3]
    t64 = torch_adam(p64, grads[1000:], torch.float64, weight_decay=1e-2, state=opt64.state_dict())[:3]
    yardstick("resume/1000+3", got, t32, t64)
    back = opt.state_dict()
    assert set(back) == {"state", "param_groups"} and set(back["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    ps = [torch.nn.Parameter(torch.from_numpy(a).clone()) for a in got[0]]
    adam = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=1e-2)
    adam.load_state_dict(back)                                                    # torch accepts it
    assert all(int(adam.state[p]["step"]) == 1003 for p in ps)
    assert all(np.array_equal(adam.state[p]["exp_avg"].numpy(), m) for p, m in zip(ps, got[1]))
    assert all(np.array_equal(adam.state[p]["exp_avg_sq"].numpy(), v) for p, v in zip(ps, got[2]))
    for p, g in zip(ps, grads[0]):
        p.grad = torch.from_numpy(g)
    adam.step()                                                                   # ... and steps from it
    assert all(int(adam.state[p]["step"]) == 1004 for p in ps)


def test_state_dict_flags_and_zero_grad():
    """a state dict written with amsgrad=True or maximize=True is refused (the kernel is neither), and leaves the optimizer as it
    was; zero_grad() clears the bucket and keeps every gradient a view of it, whatever set_to_none says"""
    counts = [5, 64]
    p0, grads = _inputs(counts, 20, 1)
    net, bucket, opt = _fused(counts, p0)
    _set_grads(bucket, grads[0])
    opt.step()
    before = _fused_results(net, opt)
    for flag in ("amsgrad", "maximize"):
        sd = opt.state_dict()
        sd["param_groups"][0][flag] = True
        with pytest.raises(RuntimeError, match=flag):
            opt.load_state_dict(sd)
    assert opt.step_count() == 1 and not opt.param_groups[0]["amsgrad"] and not opt.param_groups[0]["maximize"]
    for xa, xb in zip(before, _fused_results(net, opt)):
        for a, b in zip(xa, xb):
            assert a.tobytes() == b.tobytes()
    for set_to_none in (True, False):
        _set_grads(bucket, grads[0])
        opt.zero_grad(set_to_none=set_to_none)
        assert not bucket.flat.any()
        for p, o in zip(net.ps, opt.offsets):
            assert p.grad is not None and p.grad.data_ptr() == bucket.flat.data_ptr() + 4 * o


def test_learning_rate_through_the_scheduler():
    counts = [64, 4097]
    p0, grads = _inputs(counts, 17, 1)
    grads = [grads[0], grads[0], grads[0]]          # the same gradient: the normalised update then depends on lr alone
    net, bucket, opt = _fused(counts, p0)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.1)
    snaps = [np.concatenate(p0).astype(np.float64)]
    lrs = []
    for gk in grads:
        lrs.append(opt.param_groups[0]["lr"])
        _set_grads(bucket, gk)
        opt.step()
        sched.step()
        snaps.append(np.concatenate(_fused_results(net, opt)[0]).astype(np.float64))
    assert np.allclose(lrs, [1e-3, 1e-4, 1e-5], rtol=1e-12)
    # with a constant gradient m_hat / sqrt(v_hat) is the same at every step (= sign g, eps aside): step k moves p by lr_k
    d1, d2 = snaps[1] - snaps[0], snaps[2] - snaps[1]
    big = np.abs(d1) > 0.5 * LR
    assert big.mean() > 0.9
    assert np.abs(d2[big] / d1[big] - 0.1).max() < 2e-3          # p ~ 1: the rounding of p (6e-8) against an update of 1e-4
    t32 = torch_adam(p0, grads, torch.float32, lrs=lrs)[:3]
    t64 = torch_adam(p0, grads, torch.float64, lrs=lrs)[:3]
    yardstick("steplr/3steps", _fused_results(net, opt), t32, t64)


def test_capture_and_replay():
    """opt.step() alone in a HIP graph (one stream, no branches): 3 replays == 3 eager steps bit for bit; a learning rate changed
    between two replays through sync_lr() takes effect without a recapture"""
    counts = [5, 64, 4097]
    p0, grads = _inputs(counts, 18, 1)

    def eager(lrs):
        net, bucket, opt = _fused(counts, p0, weight_decay=1e-2)
        _set_grads(bucket, grads[0])
        for lr in lrs:
            opt.param_groups[0]["lr"] = lr
            opt.step()
        return _fused_results(net, opt), opt.step_count()

    net, bucket, opt = _fused(counts, p0, weight_decay=1e-2)
    _set_grads(bucket, grads[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    fresh = opt.state_dict()                                    # step 0: no state yet
    with torch.cuda.stream(side):                               # warm-up outside the capture (code objects, allocator)
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for p, a in zip(net.ps, p0):                                # back to the start
        p.data.copy_(torch.from_numpy(a))
    opt.load_state_dict(fresh)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    assert opt.step_count() == 0                                # a capture runs nothing
    for _ in range(3):
        graph.replay()
    got, steps = _fused_results(net, opt), opt.step_count()
    want, want_steps = eager([LR, LR, LR])
    assert steps == want_steps == 3
    for xa, xb in zip(got, want):
        for a, b in zip(xa, xb):
            assert a.tobytes() == b.tobytes()
    opt.param_groups[0]["lr"] = 10 * LR
    opt.sync_lr()
    graph.replay()
    got, steps = _fused_results(net, opt), opt.step_count()
    want, _ = eager([LR, LR, LR, 10 * LR])
    stale, _ = eager([LR, LR, LR, LR])
    assert steps == 4
    for xa, xb in zip(got, want):
        for a, b in zip(xa, xb):
            assert a.tobytes() == b.tobytes()
    assert any(a.tobytes() != b.tobytes() for a, b in zip(got[0], stale[0]))


def _real_model():
    from rpnet_amd.modules import RP_Net
    from rpnet_amd.optim import FusedAdam
    from rpnet_amd.parallel import FlatGradBucket
    from rpnet_amd.utils.seeding import seed_module_
    from tests.helpers import load_cfg
    net = RP_Net(cfg={"align": True, "backbone": "UNet"}, backbone_cfg=load_cfg(2)).to(DEV)
    seed_module_(net)
    bucket = FlatGradBucket(net)
    return net, bucket, FusedAdam(bucket, lr=LR, betas=BETAS, eps=EPS, weight_decay=1e-4)


def test_the_real_table():
    net, bucket, opt = _real_model()
    names = [n for n, _ in bucket.params]
    assert len(names) == 76 and bucket.numel == 34808000
    table = opt.table.cpu().numpy()
    assert np.frombuffer(table.tobytes(), dtype=np.int32).reshape(-1, 6)[:, 5].all()      # the whole model takes the 16-byte path
    unused = {n: p.detach().clone() for n, p in net.named_parameters() if n.startswith(("cre.w_context.", "cre.out."))}
    assert unused
    p0 = [p.detach().cpu().numpy().reshape(-1).copy() for _, p in bucket.params]
    gen = torch.Generator(device=DEV).manual_seed(19)
    grads = []
    for _ in range(3):
        mag = 10.0 ** (torch.rand(bucket.numel, generator=gen, device=DEV) * 8.0 - 6.0)
        sign = torch.where(torch.rand(bucket.numel, generator=gen, device=DEV) < 0.5, -1.0, 1.0)
        bucket.flat.copy_(mag * sign)
        grads.append(bucket.flat.cpu().numpy().copy())
        opt.step()
    torch.cuda.synchronize()
    cut = lambda flat: [flat[o:o + k] for o, k in zip(opt.offsets, opt.counts)]  # noqa: E731
    got = ([p.detach().cpu().numpy().reshape(-1) for _, p in bucket.params], cut(opt.exp_avg.cpu().numpy()),
           cut(opt.exp_avg_sq.cpu().numpy()))
    per_param = [cut(g) for g in grads]
    t32 = torch_adam(p0, per_param, torch.float32, weight_decay=1e-4)[:3]
    t64 = torch_adam(p0, per_param, torch.float64, weight_decay=1e-4)[:3]
    yardstick("real_table/3steps", got, t32, t64, names=names)
    for n, p in net.named_parameters():
        if n in unused:
            assert torch.equal(p.detach(), unused[n]), n
    moved_name, moved = bucket.params[5]
    moved.data = moved.data.clone()
    with pytest.raises(RuntimeError, match=re.escape(moved_name)):
        opt.step()


def test_driver_fused_against_torch():
    import rpnet_amd.modules as RM
    from rpnet_amd.parallel import UNUSED_PREFIXES
    from tests.helpers import load_cfg
    from train_rpnet import train
    RM._F16_MIN_PIXELS = 0
    out = {}
    for which in ("fused", "torch"):
        torch.manual_seed(0)
        net, hist = train(load_cfg(2), steps=3, batch=2, size=64, dev=torch.device(DEV), lr=1e-3, log_every=0, seed=7, optimizer=which)
        out[which] = (net, hist)
    hf, ht = out["fused"][1], out["torch"][1]
    assert hf[0] == ht[0]                                   # the same weights and episode, no update yet: bit-equal
    assert all(math.isfinite(v) for v in hf + ht) and len(hf) == len(ht) == 3
    from rpnet_amd.modules import RP_Net
    torch.manual_seed(0)
    start = dict(RP_Net(cfg={"align": True, "backbone": "UNet"}, backbone_cfg=load_cfg(2)).named_parameters())
    for n, p in out["fused"][0].named_parameters():
        same = torch.equal(p.detach().cpu(), start[n].detach())
        if n.startswith(UNUSED_PREFIXES):
            assert same, f"{n} is not in the bucket and must not move"
        else:
            assert not same, f"{n} did not move"
