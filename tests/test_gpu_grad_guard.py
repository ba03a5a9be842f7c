"""The gradient guard of the Adam step (include/rpnet_guard_abi.h, csrc/optim.hip, rpnet_amd/optim.py: FusedAdam(max_grad_norm=,
skip_nonfinite=, history=)): the gradient's 2-norm in fp64, norm clipping and the non-finite skip, all on the device.

The norm.  Reference: numpy's sqrt(sum(float64(g) ** 2)) * |grad_scale|.  Tolerance: relative 1e-12.  The squares are exact in fp64
(48 significant bits), only the fp64 additions round; the longest addition chain at these sizes is 16 per lane, 6 across the wave, 4
across the waves and at most 7 partial sums: (chain + 1) * 2^-53 < 1e-14, numpy's own pairwise sum is shorter still, so 1e-12
leaves two decades.  rpnet_grad_sumsq has no optimizer and therefore no grad_scale (its norm is sqrt(sumsq)); grad_scale 1/8 goes
through FusedAdam.grad_norm(), which is that call and one multiplication on the device, and through the norm that
rpnet_adam_step_guarded reports (test_clipping_against_torch).

Clipping.  Reference: torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam on the CPU, in fp32 and in fp64, on grad *
grad_scale.  Yardstick: that of tests/test_gpu_optim.py, max |x_hip - x_64| <= max(K * max |x_torch32 - x_64|, one fp32 ulp at max
|x_64|), with K = 3 instead of 2: the kernel's coefficient is the correctly rounded fp64 value while torch's fp32 coefficient carries
an error of unknown sign shared by every element, one more rounding than the reorderings K = 2 was sized for.  Every check prints
`PARITY guard case tensor err_hip err_torch ratio`; profiles/optim_parity.txt keeps them.

Everything else is an equality of bytes.  Inputs, shapes and the sentinel buffers are those of tests/test_gpu_optim.py."""
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_optim import (BETAS, DEV, EPS, GAP, LISTS, LR, SENTINEL, RawAdam, _fused, _fused_results, _inputs,
                                  _set_grads, _step)

pytestmark = pytest.mark.gpu
K = 3.0
NORM_RTOL = 1e-12
GUARD_WORDS, ROW = 10, 3
# (list, flat_shift): every list on the 16-byte grid, and the non-VEC instantiation with the flat buffers 1..3 elements off it
LAYOUTS = [(name, 0) for name in LISTS] + [("fast", s) for s in (1, 2, 3)]


def norm64(grads, grad_scale=1.0):
    g = np.concatenate(grads).astype(np.float64)
    return float(np.sqrt(np.sum(g ** 2)) * abs(grad_scale))


class RawGuard(RawAdam):
    """RawAdam plus the guard's three buffers, each a slice of a larger float64 tensor with SENTINEL on both sides"""

    def __init__(self, counts, p0, block, capacity=0, **kw):
        super().__init__(counts, p0, **kw)
        self.capacity = capacity
        mk = lambda n: torch.full((GAP + n + GAP,), SENTINEL, dtype=torch.float64, device=DEV)  # noqa: E731
        self.part_buf, self.guard_buf, self.ring_buf = mk(self.n_chunks), mk(GUARD_WORDS), mk(ROW * capacity)
        self.partials = self.part_buf[GAP:GAP + self.n_chunks]
        self.guard = self.guard_buf[GAP:GAP + GUARD_WORDS]
        self.ring_ptr = self.ring_buf.data_ptr() + 8 * GAP        # never null: with capacity 0 the sentinel behind it must stay
        self.guard.copy_(block)

    def stats(self):
        torch.cuda.synchronize()
        host = self.guard.cpu()
        i64, i32, f32 = host.view(torch.int64), host.view(torch.int32), host.view(torch.float32)
        ring = self.ring_buf[GAP:GAP + ROW * self.capacity].cpu().view(self.capacity, ROW).tolist()
        return dict(max_norm=float(host[0]), sumsq=float(host[3]), norm=float(host[4]), coef=float(host[5]), coef_f=float(f32[12]),
                    skip=int(i32[13]), attempt=int(i64[7]), skipped=int(i64[8]), clipped=int(i64[9]), ring=ring,
                    sumsq_bits=int(i64[3]))

    def guard_sentinels_intact(self):
        ok = True
        for buf, n in ((self.part_buf, self.n_chunks), (self.guard_buf, GUARD_WORDS), (self.ring_buf, ROW * self.capacity)):
            ok = ok and bool((buf[:GAP] == SENTINEL).all()) and bool((buf[GAP + n:] == SENTINEL).all())
        return ok and self.sentinels_intact()


def _guarded_raw(counts, p0, max_norm=math.inf, skip_nonfinite=False, capacity=0, **kw):
    from rpnet_amd.optim import guard_block
    return RawGuard(counts, p0, guard_block(max_norm, skip_nonfinite, capacity), capacity=capacity, **kw)


def _sumsq(raw, grads):
    """one rpnet_grad_sumsq on the buffers of a RawGuard"""
    from rpnet_amd import hip
    raw.g.copy_(torch.from_numpy(np.concatenate(grads)))
    hip.call("rpnet_grad_sumsq", hip.ptr(raw.table), raw.n_chunks, hip.ptr(raw.g), hip.ptr(raw.partials), hip.ptr(raw.guard),
             raw.ring_ptr)


def _gstep(raw, grads):
    """one rpnet_adam_step_guarded on the buffers of a RawGuard, with the gradients of this step"""
    from rpnet_amd import hip
    raw.g.copy_(torch.from_numpy(np.concatenate(grads)))
    hip.call("rpnet_adam_step_guarded", hip.ptr(raw.table), raw.n_chunks, hip.ptr(raw.g), hip.ptr(raw.m), hip.ptr(raw.v),
             hip.ptr(raw.hyper), hip.ptr(raw.partials), hip.ptr(raw.guard), raw.ring_ptr)


def _same_bytes(xa, xb):
    return all(a.tobytes() == b.tobytes() for ta, tb in zip(xa, xb) for a, b in zip(ta, tb))


# ---------------------------------------------------------------------------------------------------------- 1. the norm
@pytest.mark.parametrize("lname, flat_shift", LAYOUTS)
def test_norm_against_fp64(lname, flat_shift):
    counts = LISTS[lname]
    p0, (grads,) = _inputs(counts, 31, 1)
    rs = np.random.RandomState(32)
    huge = [(np.sign(rs.standard_normal(k)) * 10.0 ** rs.uniform(29, 31, k)).astype(np.float32) for k in counts]
    raw = _guarded_raw(counts, p0, flat_shift=flat_shift)
    for name, gk in (("1e-6..1e2", grads), ("1e30", huge)):
        want = norm64(gk)
        _sumsq(raw, gk)
        a = raw.stats()
        _sumsq(raw, gk)
        b = raw.stats()
        print(f"NORM guard {lname}/shift{flat_shift} {name} norm {a['norm']:.17e} fp64 {want:.17e} rel {abs(a['norm'] - want) / want:.3e}")
        assert math.isfinite(a["norm"]) and abs(a["norm"] - want) <= NORM_RTOL * want
        assert abs(math.sqrt(a["sumsq"]) - want) <= NORM_RTOL * want
        assert a["sumsq_bits"] == b["sumsq_bits"] and a["norm"] == b["norm"]          # two calls: bit-identical
        assert a["skip"] == 0 and a["coef"] == 1.0 and a["skipped"] == a["clipped"] == 0
    assert raw.stats()["attempt"] == 4
    assert raw.guard_sentinels_intact(), "a sentinel beside the partial sums, the guard block, the ring, p, g, m or v was overwritten"
    assert raw.steps_taken() == 0 and not raw.m.any() and not raw.v.any()            # the norm alone: no optimizer
    if flat_shift == 0:                                          # grad_scale: FusedAdam.grad_norm(), default-built (no guard buffers)
        for gs in (1.0, 0.125):
            net, bucket, opt = _fused(counts, p0, grad_scale=gs)
            for gk in (grads, huge):
                _set_grads(bucket, gk)
                got = opt.grad_norm()
                assert got.is_cuda and got.dim() == 0 and got.dtype == torch.float64
                want = norm64(gk, gs)
                assert abs(float(got) - want) <= NORM_RTOL * want
            assert opt.guard is None and opt.partials is None and opt.step_count() == 0


# ---------------------------------------------------------------------------------------------------------- 2. no clipping
@pytest.mark.parametrize("lname, flat_shift", LAYOUTS)
def test_no_clipping_is_bit_identical(lname, flat_shift):
    """max_norm = inf and max_norm = 2 x the largest norm: p, m, v and the step count of rpnet_adam_step, byte for byte"""
    counts = LISTS[lname]
    p0, grads = _inputs(counts, 33, 3)
    plain = RawAdam(counts, p0, weight_decay=1e-2, flat_shift=flat_shift)
    for gk in grads:
        _step(plain, gk)
    want = plain.results()
    for max_norm in (math.inf, 2.0 * max(norm64(gk) for gk in grads)):
        raw = _guarded_raw(counts, p0, max_norm=max_norm, weight_decay=1e-2, flat_shift=flat_shift)
        for gk in grads:
            _gstep(raw, gk)
        assert _same_bytes(raw.results(), want), f"{lname} shift {flat_shift} max_norm {max_norm}"
        st = raw.stats()
        assert raw.steps_taken() == plain.steps_taken() == 3
        assert st["coef"] == 1.0 and st["coef_f"] == 1.0 and st["clipped"] == 0 and st["skipped"] == 0 and st["attempt"] == 3
        assert raw.guard_sentinels_intact()


# ---------------------------------------------------------------------------------------------------------- 3. clipping
def torch_adam_clipped(p0, grads, dtype, max_norm, weight_decay, grad_scale):
    """flat.mul_(grad_scale), clip_grad_norm_(max_norm), torch.optim.Adam.step() on the CPU in `dtype` -> p, m, v lists"""
    ps = [torch.nn.Parameter(torch.from_numpy(a).to(dtype).clone()) for a in p0]
    opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=weight_decay)
    for gk in grads:
        for p, g in zip(ps, gk):
            p.grad = torch.from_numpy(g).to(dtype) * grad_scale
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
    return ([p.detach().numpy() for p in ps], [opt.state[p]["exp_avg"].numpy() for p in ps],
            [opt.state[p]["exp_avg_sq"].numpy() for p in ps])


def yardstick_guard(case, hip_pmv, t32, t64):
    problems = []
    for tname, xh, x32, x64 in zip("pmv", hip_pmv, t32, t64):
        for i, (h, a, b) in enumerate(zip(xh, x32, x64)):
            b = np.asarray(b, dtype=np.float64).reshape(-1)
            err_t = float(np.abs(np.asarray(a, dtype=np.float64).reshape(-1) - b).max())
            err_h = float(np.abs(np.asarray(h, dtype=np.float64).reshape(-1) - b).max())
            ulp = float(np.spacing(np.float32(np.abs(b).max())))
            print(f"PARITY guard {case} {tname} param{i}[{b.size}] err_hip {err_h:.3e} err_torch {err_t:.3e} "
                  f"ratio {err_h / err_t if err_t > 0 else float('nan'):.3f} ulp {ulp:.3e}")
            if not err_h <= max(K * err_t, ulp):
                problems.append(f"{case} {tname} param{i}[{b.size}]: err_hip {err_h:.3e} > max({K:g} * {err_t:.3e}, ulp {ulp:.3e})")
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("lname, flat_shift", LAYOUTS)
def test_clipping_against_torch(lname, flat_shift):
    from rpnet_amd.optim import clip_coefficient
    counts = LISTS[lname]
    p0, grads = _inputs(counts, 34, 3)
    for gs in (1.0, 0.125):
        norms = [norm64(gk, gs) for gk in grads]
        max_norm = 0.5 * norms[0]
        for wd in (0.0, 1e-4):
            raw = _guarded_raw(counts, p0, max_norm=max_norm, capacity=2, weight_decay=wd, grad_scale=gs, flat_shift=flat_shift)
            seen = []
            for gk in grads:
                _gstep(raw, gk)
                seen.append(raw.stats())
            got = raw.results()
            assert raw.guard_sentinels_intact() and raw.steps_taken() == 3
            for st, n in zip(seen, norms):
                want = clip_coefficient(n, max_norm)
                assert abs(st["norm"] - n) <= NORM_RTOL * n and abs(st["coef"] - want) <= NORM_RTOL * want
                assert st["coef_f"] == float(np.float32(st["coef"])) and st["skip"] == 0
            assert seen[-1]["clipped"] == sum(clip_coefficient(n, max_norm) < 1.0 for n in norms) >= 1
            assert seen[-1]["ring"] == [[s["norm"], s["coef"], 0.0] for s in (seen[2], seen[1])]       # attempts 2, 1 in rows 0, 1
            t32 = torch_adam_clipped(p0, grads, torch.float32, max_norm, wd, gs)
            t64 = torch_adam_clipped(p0, grads, torch.float64, max_norm, wd, gs)
            yardstick_guard(f"{lname}/shift{flat_shift}/gs{gs:g}/wd{wd:g}", got, t32, t64)


# ---------------------------------------------------------------------------------------------------------- 4. the skip
@pytest.mark.parametrize("lname, at, bad", [("tail", -1, math.nan), ("big", 2, math.inf)])
def test_nonfinite_skip(lname, at, bad):
    """A finite, B bad, C finite.  tail: a NaN in the last element of an element-by-element chunk; big ([4097]): +inf inside a quad"""
    counts = {"tail": LISTS["tail"], "big": [4097]}[lname]
    p0, (ga, gb, gc) = _inputs(counts, 35, 3)
    gb = [g.copy() for g in gb]
    gb[-1 if at < 0 else 0][at] = bad
    raw = _guarded_raw(counts, p0, skip_nonfinite=True, weight_decay=1e-2)
    _gstep(raw, ga)
    after_a, st_a = raw.results(), raw.stats()
    _gstep(raw, gb)
    after_b, st_b = raw.results(), raw.stats()
    assert _same_bytes(after_b, after_a) and raw.steps_taken() == 1
    assert st_a["skip"] == 0 and st_b["skip"] == 1 and st_b["skipped"] == 1 and st_b["attempt"] == 2
    assert st_b["coef_f"] == st_a["coef_f"] and not math.isfinite(st_b["sumsq"])
    _gstep(raw, gc)
    st_c = raw.stats()
    assert st_c["skip"] == 0 and st_c["skipped"] == 1 and st_c["attempt"] == 3 and raw.steps_taken() == 2
    only = _guarded_raw(counts, p0, skip_nonfinite=True, weight_decay=1e-2)
    _gstep(only, ga)
    _gstep(only, gc)
    assert _same_bytes(raw.results(), only.results())
    assert raw.guard_sentinels_intact()
    if math.isnan(bad):                                          # without the skip the same B poisons p
        loose = _guarded_raw(counts, p0, skip_nonfinite=False, weight_decay=1e-2)
        _gstep(loose, ga)
        _gstep(loose, gb)
        assert all(np.isnan(p).all() for p in loose.results()[0])


# ---------------------------------------------------------------------------------------------------------- 5. the ring
def test_history_ring():
    from rpnet_amd.optim import clip_coefficient
    counts = LISTS["tail"]
    p0, grads = _inputs(counts, 36, 6)
    grads[3] = [g.copy() for g in grads[3]]
    grads[3][0][17] = math.nan
    norms = [norm64(gk) for gk in grads]
    max_norm = 0.5 * norms[0]
    net, bucket, opt = _fused(counts, p0, max_grad_norm=max_norm, skip_nonfinite=True, history=4)
    for gk in grads:
        _set_grads(bucket, gk)
        opt.step()
    st = opt.guard_stats()
    assert st["attempt"] == 6 and st["skipped"] == 1 and opt.step_count() == 5
    assert st["clipped"] == sum(clip_coefficient(n, max_norm) < 1.0 for i, n in enumerate(norms) if i != 3)
    assert len(st["history"]) == 4 and [h[2] for h in st["history"]] == [0, 1, 0, 0]               # attempts 2, 3, 4, 5
    for (norm, coef, _), n, i in zip(st["history"], norms[2:], range(2, 6)):
        if i == 3:
            assert math.isnan(norm)
        else:
            assert abs(norm - n) <= NORM_RTOL * n and abs(coef - clip_coefficient(n, max_norm)) <= NORM_RTOL
    assert st["norm"] == st["history"][-1][0] and st["coef"] == st["history"][-1][1] and st["skip"] == 0
    # capacity 0 writes nothing: the sentinel behind a ring of no rows stays
    raw = _guarded_raw(counts, p0, max_norm=max_norm, capacity=0)
    for gk in grads[:2]:
        _gstep(raw, gk)
    assert raw.stats()["attempt"] == 2 and bool((raw.ring_buf == SENTINEL).all()) and raw.guard_sentinels_intact()


# ---------------------------------------------------------------------------------------------------------- 6. FusedAdam
def test_fused_adam():
    counts = [5, 64, 4097]
    p0, grads = _inputs(counts, 37, 3)
    # built as before this feature: no guard buffers, the bytes of rpnet_adam_step
    net, bucket, opt = _fused(counts, p0, weight_decay=1e-2)
    assert not opt.guarded and opt.partials is None and opt.guard is None and opt.ring is None
    plain = RawAdam(counts, p0, weight_decay=1e-2)
    for gk in grads:
        _set_grads(bucket, gk)
        opt.step()
        _step(plain, gk)
    assert _same_bytes(_fused_results(net, opt), plain.results())
    with pytest.raises(RuntimeError, match="without the gradient guard"):
        opt.guard_stats()
    with pytest.raises(RuntimeError, match="without the gradient guard"):
        opt.set_max_grad_norm(1.0)
    # the guard through FusedAdam == the raw ABI
    max_norm = 0.5 * norm64(grads[0])
    net, bucket, opt = _fused(counts, p0, weight_decay=1e-2, max_grad_norm=max_norm)
    raw = _guarded_raw(counts, p0, max_norm=max_norm, weight_decay=1e-2)
    for gk in grads:
        _set_grads(bucket, gk)
        opt.step()
        _gstep(raw, gk)
    assert _same_bytes(_fused_results(net, opt), raw.results())
    st, rs = opt.guard_stats(), raw.stats()
    assert (st["norm"], st["coef"], st["clipped"], st["attempt"]) == (rs["norm"], rs["coef"], rs["clipped"], 3) and st["clipped"] >= 1
    assert torch.equal(bucket.flat.cpu(), torch.from_numpy(np.concatenate(grads[-1])))            # the bucket is not rewritten
    # torch.optim.Adam's state dict, there and back, with the guard on
    sd = opt.state_dict()
    ps = [torch.nn.Parameter(p.detach().cpu().clone()) for p in net.ps]
    adam = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=1e-2)
    assert set(sd) == {"state", "param_groups"} and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert set(sd["param_groups"][0]) == set(adam.state_dict()["param_groups"][0])
    adam.load_state_dict({"state": {i: {k: v.cpu() for k, v in s.items()} for i, s in sd["state"].items()},
                          "param_groups": sd["param_groups"]})
    assert all(int(adam.state[p]["step"]) == 3 for p in ps)
    back = adam.state_dict()
    opt.load_state_dict({"state": {i: {k: (v.to(DEV) if k != "step" else v.clone()) for k, v in s.items()}
                                   for i, s in back["state"].items()}, "param_groups": back["param_groups"]})
    assert opt.step_count() == 3 and _same_bytes(_fused_results(net, opt)[1:], raw.results()[1:])
    _set_grads(bucket, grads[0])
    opt.step()
    _gstep(raw, grads[0])
    assert opt.step_count() == 4 and _same_bytes(_fused_results(net, opt), raw.results())
    opt.set_max_grad_norm(None)
    assert opt.guard_stats()["attempt"] == 4 and float(opt.guard[0]) == math.inf
    with pytest.raises(ValueError):
        opt.set_max_grad_norm(-2.0)


# ---------------------------------------------------------------------------------------------------------- 7. capture
def test_guarded_capture_and_replay():
    """the guarded FusedAdam.step() (rpnet_adam_step_guarded) alone in a HIP graph (one stream, no branches): 3 replays == 3 eager guarded steps bit for bit; a NaN
    in the bucket makes the replay skip, the restored gradient lets it go on; a threshold changed between two replays through
    set_max_grad_norm() takes effect without a recapture, inside a capture it is refused"""
    counts = [5, 64, 4097]
    p0, grads = _inputs(counts, 38, 1)
    c = 0.5 * norm64(grads[0])

    def eager(thresholds):
        net, bucket, opt = _fused(counts, p0, weight_decay=1e-2, max_grad_norm=c, skip_nonfinite=True)
        _set_grads(bucket, grads[0])
        for t in thresholds:
            opt.set_max_grad_norm(t)
            opt.step()
        return _fused_results(net, opt), opt.step_count()

    net, bucket, opt = _fused(counts, p0, weight_decay=1e-2, max_grad_norm=c, skip_nonfinite=True)
    _set_grads(bucket, grads[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    fresh = opt.state_dict()
    with torch.cuda.stream(side):                               # warm-up outside the capture (code objects, allocator)
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for p, a in zip(net.ps, p0):
        p.data.copy_(torch.from_numpy(a))
    opt.load_state_dict(fresh)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="capture"):
            opt.set_max_grad_norm(2 * c)
        opt.step()
    torch.cuda.synchronize()
    assert opt.step_count() == 0 and opt.guard_stats()["attempt"] == 1          # a capture runs nothing; the warm-up was attempt 0
    for _ in range(3):
        graph.replay()
    got, steps = _fused_results(net, opt), opt.step_count()
    want, want_steps = eager([c, c, c])
    assert steps == want_steps == 3 and _same_bytes(got, want)
    assert opt.guard_stats()["clipped"] == 1 + 3
    bucket.flat[70] = math.nan
    graph.replay()
    st = opt.guard_stats()
    assert st["skip"] == 1 and st["skipped"] == 1 and opt.step_count() == 3 and _same_bytes(_fused_results(net, opt), want)
    _set_grads(bucket, grads[0])
    graph.replay()
    want4, _ = eager([c, c, c, c])
    assert opt.step_count() == 4 and opt.guard_stats()["skip"] == 0 and _same_bytes(_fused_results(net, opt), want4)
    opt.set_max_grad_norm(0.5 * c)
    graph.replay()
    got = _fused_results(net, opt)
    want5, _ = eager([c, c, c, c, 0.5 * c])
    stale, _ = eager([c, c, c, c, c])
    assert opt.step_count() == 5 and _same_bytes(got, want5)
    assert any(a.tobytes() != b.tobytes() for a, b in zip(got[1], stale[1]))


# ---------------------------------------------------------------------------------------------------------- 8. the driver
def test_driver_clips_under_both_optimizers():
    """train() with clip_grad_norm under "fused" (FusedAdam(max_grad_norm=)) and "torch" (clip_grad_norm_): the threshold is half
    of FusedAdam.grad_norm() (rpnet_grad_sumsq) of the first step, so that clipping really happens.  That first step is a run of its
    own with skip_nonfinite=True on finite data: it must report skipped == 0"""
    import rpnet_amd.modules as RM
    from rpnet_amd.modules import RP_Net
    from rpnet_amd.parallel import UNUSED_PREFIXES
    from tests.helpers import load_cfg
    from train_rpnet import train
    RM._F16_MIN_PIXELS = 0
    kw = dict(batch=2, size=64, dev=torch.device(DEV), lr=1e-3, log_every=0, seed=7)
    # a first step with the skip on and finite data: nothing is skipped, and the bucket then holds that step's gradient
    probe = {}
    torch.manual_seed(0)
    train(load_cfg(2), steps=1, optimizer="fused", skip_nonfinite=True, stats=probe, **kw)
    first = probe["optimizer"].guard_stats()
    assert first["skipped"] == 0 and first["attempt"] == 1 and first["clipped"] == 0
    norm = float(probe["optimizer"].grad_norm())
    assert math.isfinite(norm) and norm > 0 and abs(norm - first["norm"]) <= NORM_RTOL * norm
    c = 0.5 * norm
    out = {}
    for which in ("fused", "torch"):
        stats = {}
        torch.manual_seed(0)
        net, hist = train(load_cfg(2), steps=3, optimizer=which, clip_grad_norm=c, stats=stats, **kw)
        out[which] = (net, hist, stats["optimizer"])
    hf, ht = out["fused"][1], out["torch"][1]
    assert hf[0] == ht[0]                                   # the same weights and episode, no update yet: bit-equal
    assert all(math.isfinite(v) for v in hf + ht) and len(hf) == len(ht) == 3
    st = out["fused"][2].guard_stats()
    assert st["clipped"] >= 1 and st["skipped"] == 0 and st["attempt"] == 3 and out["fused"][2].step_count() == 3
    torch.manual_seed(0)
    start = dict(RP_Net(cfg={"align": True, "backbone": "UNet"}, backbone_cfg=load_cfg(2)).named_parameters())
    for n, p in out["fused"][0].named_parameters():
        same = torch.equal(p.detach().cpu(), start[n].detach())
        if n.startswith(UNUSED_PREFIXES):
            assert same, f"{n} is not in the bucket and must not move"
        else:
            assert not same, f"{n} did not move"
