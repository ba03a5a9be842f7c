#!/usr/bin/env python3
"""Headline benchmark: support/query pairs per second, forward+backward, 1-way 1-shot,
256x256, T=5 refinement iterations, batch 8 per GPU (BASELINE.json configs[1]; configs[3] =
the same per-GPU work on 8 GPUs with the RCCL gradient all-reduce -> weak scaling).

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

One step = RP_Net.forward (train mode, align loss on) + the harness loss
dice_ce(output) + sum_i dice_ce(refinement[i]) + align_loss (the reference has no train
loop) + backward + the flat-bucket gradient all-reduce.  Synthetic CT-shaped
episodes are generated once and are resident in HBM before the timed region; weights are
name-seeded random init (no dataset / checkpoint exists offline).

Arithmetic of the 3x3 convolutions (`--conv-math`, default f16x2): every fp32 operand is carried as two fp16
planes of operand / (power-of-two scale from a rigorous bound) and multiplied on the fp16 matrix pipe with three
partial products into fp32 accumulators — fp32-level accuracy (dropped term <= 2^-22 |x*y|;
tests/test_gpu_ops.py::test_split_conv_accuracy measures it against fp64 next to the fp32-MFMA kernel) at 16/3 of the
fp32 matrix rate; operands without a bound run as three bf16 planes (`bf16x3`, six products).  `f32` selects the
v_mfma_f32_32x32x2_f32 kernels; the JSON line carries those figures too (`alt_math`).  `f16` = ONE fp16 plane (plain
fp16 operands, fp32 accumulation and BatchNorm statistics): the reduced-precision arithmetic of BASELINE configs[4]
(`--size 512 --iters 10 --ways 2 --batch 4 --conv-math f16`), reported with dtype "f16", never the headline.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times `--steps` steps and prints the headline (`metric`,
`value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step` = milliseconds per timed step, the per-step spread `step_ms`).
`--dump-outputs DIR` also writes what the last timed step handed its caller (loss, gradients) as .npy files (`dump_outputs`).
Everything else below (roofline, alt_math, mask_tile_skip, graph_replay, eval, conv_math_error_vs_fp64, cpu_baseline,
other_configs, the other issue mode of an N > 1 run) runs only with `--full`.  `roofline` is measured live: every C-ABI call of one extra
step is bracketed by HIP events on the launch stream; the dominant kernel is the implicit-GEMM
convolution (rpnet_conv_fwd: forward + dgrad launches).  The timed steps run with
the weight gradients on a second HIP stream (overlap on); the extra profiled step serialises the
streams so that every launch owns the GPU and its duration is the kernel's own
(RPNET_ASYNC_WGRAD=0 makes the timed steps serial too; profiles/ holds rocprofv3 stats of both).  `cpu_baseline` is
the CPU oracle in as-written mode (= the reference's operator sequence) on the host cores.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist
import yaml

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_BF16_MFMA_TFLOPS = 2500.0  # same guide: v_mfma_f32_32x32x16_bf16 dense peak
# MFMA partial products issued per algorithmic fp32 multiply-add, and the resulting ceiling in algorithmic FLOPs
# (the fp16 matrix instruction v_mfma_f32_32x32x16_f16 has the bf16 one's rate)
MATH = {"f32": (1, PEAK_F32_MFMA_TFLOPS), "bf16x3": (6, PEAK_BF16_MFMA_TFLOPS / 6), "f16x2": (3, PEAK_BF16_MFMA_TFLOPS / 3),
        "f16": (1, PEAK_BF16_MFMA_TFLOPS)}
GF_PER_PAIR = {(256, 5): 675.4, (128, 1): 138.5}  # algorithmic fwd+bwd GFLOP per pair


def algorithmic_gf_per_pair(size, T, n_shots=1, n_ways=1):
    """encoder 82.22 GF/image fwd at 256^2, CRE 10.12 GF/call, backward = 2x forward; a pair has
    ways x shots support images (one encoder pass and one CRE call each) + the query image and its T CRE calls
    (configs[4]: 3 images + 12 CRE calls at 512^2 = 4416 GF)."""
    s = (size / 256.0) ** 2
    imgs, cre_calls = n_ways * n_shots + 1, n_ways * n_shots + T
    return 3.0 * (imgs * 82.22 + cre_calls * 10.12) * s


def upconv_collapse_saved_gf_per_pair(size, n_shots=1, n_ways=1):
    """GF per pair the collapsed up_conv layers do NOT execute (Up5, Up4: 9.66 GF forward per image at 256^2 each, x 3 for forward +
    input gradient + weight gradient, 5 of 9 tap products gone); 0 with RPNET_UPCONV_COLLAPSE=0."""
    import rpnet_amd.functional as RF
    if not RF._UP4:
        return 0.0
    return 3.0 * (n_ways * n_shots + 1) * 2 * 9.664 * (5.0 / 9.0) * (size / 256.0) ** 2


def baseline_config(args, world):
    """which BASELINE.json configuration the command line is (parity-test shapes other than [1] / [3] are not headline)"""
    key = (args.ways, args.shots, args.size, args.iters)
    if key == (1, 1, 256, 5):
        return "BASELINE configs[1]" if world == 1 else "BASELINE configs[3]: the same per-GPU work, gradients all-reduced"
    if key == (1, 5, 256, 5):
        return "BASELINE configs[2]"
    if key == (2, 1, 512, 10):
        return "BASELINE configs[4]"
    if key == (1, 1, 128, 1):
        return "BASELINE configs[0] shape"
    return "not a BASELINE configuration"


def build_model(cfg, dev):
    from rpnet_amd.modules import RP_Net
    from rpnet_amd.utils.seeding import seed_module_
    net = RP_Net(cfg={"align": True, "backbone": "UNet"}, backbone_cfg=cfg).to(dev)
    seed_module_(net)
    net.train()
    return net


def make_inputs(seed, B, size, dev, n_shots=1, n_ways=1):
    from rpnet_amd.utils.synth import make_episode
    ep = make_episode(seed, B, size, n_shots=n_shots, n_ways=n_ways)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    return ([[t(s) for s in way] for way in ep["support_images"]], [[t(s) for s in way] for way in ep["support_fg"]],
            [[t(s) for s in way] for way in ep["support_bg"]], [t(ep["query_images"])], t(ep["query_labels"]),
            t(ep["appr_query_labels"]))


def step(net, bucket, inp, scaler, exposed=None):
    """exposed (N > 1): list that receives a (start, end) HIP-event pair around the part of the gradient exchange that is
    NOT hidden under backward — from the end of backward on the compute stream to the moment the averaged bucket is ready"""
    import rpnet_amd.functional as RF
    si, fg, bg, qi, ql, appr = inp
    bucket.zero()
    out = net(si, fg, bg, qi, appr_query_labels=appr)
    # dice_ce of the final output and of every refinement iteration's output, summed, + scaler * align_loss: one launch pair
    # (RF.objective: the values of `dice_ce_sum(...) + scaler * out["align_loss"]`, bit for bit)
    loss = RF.objective([out["output"], *out["refinement"].values()], ql, out["align_loss"], scaler)
    RF.backward(loss)
    if exposed is not None:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        bucket.allreduce()
        b.record()
        exposed.append((a, b))
    else:
        bucket.allreduce()
    # (detached: a loss tensor that outlives the step keeps the step's autograd nodes — among them every parameter's AccumulateGrad
    # node, stamped with the stream it first ran on — alive into a later leg that runs the same layers on another stream layout)
    return loss.detach()


DUMP_GRAD_SAMPLE = 1 << 23     # float32 gradient elements --dump-outputs writes at most (32 MiB; the whole dump stays below 64 MB)


def dump_outputs(path, loss, bucket):
    """--dump-outputs: what the timed step hands its caller, from the last timed step — the loss (`loss.npy`, float64) and the
    gradients every parameter's .grad views in the flat bucket.  The bucket (139 MB at the headline shape) is larger than the
    dump's budget: `grad_sample.npy` holds the elements at a fixed, seeded set of sorted indices (the same set for every bucket of
    the same size: numpy default_rng(0)), `grad_norms.npy` the L2 norm of every parameter's gradient (float64, bucket order)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    flat = bucket.flat
    n = flat.numel()
    if n > DUMP_GRAD_SAMPLE:
        idx = np.sort(np.random.default_rng(0).choice(n, DUMP_GRAD_SAMPLE, replace=False))
        sample = flat[torch.from_numpy(idx).to(flat.device)]
    else:
        sample = flat
    bounds = [0]
    for _, p in bucket.params:
        bounds.append(bounds[-1] + p.numel())
    norms = torch.stack([flat[a:b].double().norm() for a, b in zip(bounds[:-1], bounds[1:])])
    np.save(os.path.join(path, "loss.npy"), loss.detach().double().reshape(1).cpu().numpy())
    np.save(os.path.join(path, "grad_sample.npy"), sample.float().cpu().numpy())
    np.save(os.path.join(path, "grad_norms.npy"), norms.cpu().numpy())


def mask_skip_leg(net, bucket, inp, scaler, batch, fence, RF, dense_value):
    """The same step with the zero-tile skip of the masked CRE convolutions on (RF._MASK_SKIP: w_k(x * mask) / w_q(x * (1 - mask)),
    forward and input gradient, output tiles whose masked input / output factor is zero run no K loop; same bits as the dense
    step: tests/test_gpu_ops.py::test_masked_conv_zero_tile_skip_is_bit_identical).  NOT the headline — the metric's FLOP count is
    the dense one — but what a user of the library gets by default.  tiles: from the flag buffers of one extra step."""
    RF._MASK_SKIP = True
    try:
        for _ in range(2):
            step(net, bucket, inp, scaler)
        fence()
        t1 = time.perf_counter()
        for _ in range(10):
            step(net, bucket, inp, scaler)
        fence()
        el = time.perf_counter() - t1
        RF._SKIP_STATS = []
        step(net, bucket, inp, scaler)
        fence()
        flags = [f for f in RF._SKIP_STATS]
        RF._SKIP_STATS = None
        skipped = sum(int((f == 0).sum()) for f in flags)
        computed = sum(int((f == 1).sum()) for f in flags)
        v = batch * 10 / el
        return {"value": round(v, 3), "unit": "pairs/s", "steps": 10, "ms_per_step": round(1e3 * el / 10, 3),
                "over_dense": round(v / dense_value, 4), "launches_with_skip": len(flags), "tiles_skipped": skipped,
                "tiles_computed": computed,
                "what": "zero-tile skip of the masked CRE convolutions (forward + input gradient; weight gradients stay dense); bit-identical "
                        "results; the headline `value` and every roofline entry are measured with it OFF"}
    finally:
        RF._MASK_SKIP = False


def fp16_trained_dice_leg(dev, RF):
    """north_star's "<= 1e-3 Dice deviation" for the fp16 configuration, measured and put in the line: 150 Adam steps of
    train_rpnet.train on synthetic 2-way 512^2 episodes (T = 10, batch 4, f16x2), then configs[4]'s call free-running (every
    iteration on the loop's own thresholded mask) under the one-plane f16 arithmetic and under the fp32-equivalent f16x2:
    largest per-iteration deviation of Dice / foreground fraction, train-mode and eval-mode BatchNorm (tools/trained_f16_dice.py)."""
    import rpnet_amd.modules as RM
    import tools.trained_f16_dice as TD
    was = (RF.conv_math(), RM._F16_MIN_PIXELS, RF._ASYNC["on"])
    cur = torch.cuda.current_stream(dev)
    try:
        net, hist = TD.train_weights(150, 512, 1e-4, dev, n_ways=2, iters=10)
        out = {"trained": {"steps": 150, "size": 512, "ways": 2, "T": 10, "batch": 4, "arithmetic": "f16x2", "first_loss": round(hist[0], 3),
                           "last_loss": round(hist[-1], 3)}, "bar": 1e-3}
        for mode in (True, False):
            res = TD.free_running(net, TD.CASES["configs4_2way_512_T10_B4"], dev, mode)
            dd, df = TD.deviations(res)
            out["train_mode" if mode else "eval_mode"] = {"max_dice_dev": float(f"{max(dd):.3g}"), "max_fg_frac_dev": float(f"{max(df):.3g}"),
                                                         "dice_f16x2": [round(a[0], 4) for a in res["f16x2"]]}
        out["within_bar"] = all(out[k]["max_dice_dev"] <= 1e-3 for k in ("train_mode", "eval_mode"))
        del net
    finally:
        RF.set_conv_math(was[0])
        RM._F16_MIN_PIXELS = was[1]
        RF.set_async_wgrad(was[2])
        torch.cuda.set_stream(cur)
        torch.cuda.empty_cache()
    return out


def profile_step(net, bucket, inp, scaler):
    """One extra step with every C-ABI call bracketed by HIP events on the launch stream."""
    from rpnet_amd import hip
    records = []
    orig = hip.call

    def timed(name, *args):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        flops = nbytes = 0.0
        key = name
        if name in ("rpnet_conv_fwd", "rpnet_conv_wgrad"):
            d = args[0]._obj
            m, ci, co = d.N * d.H * d.W, d.C0 + d.C1, d.Co0 + d.Co1
            flops = 2.0 * m * ci * co * d.taps
            esz = 2.0 * d.split_planes if d.split_planes else 4.0                # operand bytes per element
            nbytes = esz * ((m >> (2 * d.upsample)) * ci + d.taps * ci * co) + 4.0 * m * co   # read x, w; write y
        elif name in ("rpnet_conv_up4", "rpnet_conv_wgrad_up4"):
            # the collapsed up_conv layers (Up5, Up4): FOUR products per (output pixel, cin, cout) are executed, not the nine the
            # reference's operator sequence implies (SURVEY.md 8d counts 9.664 GF per image and layer) — the EXECUTED count goes
            # into `achieved`, so that the roofline fraction is not flattered by work that was removed
            d = args[0]._obj
            m = d.N * d.H * d.W                                                    # high-resolution pixels
            if name == "rpnet_conv_up4" or args[1] is not None:                    # (the reduce-only phase of a weight gradient: no GEMM)
                flops = 2.0 * m * d.C0 * d.Co0 * 4
            esz = 2.0 * d.split_planes
            lo, hi = (d.C0, d.Co0) if (name == "rpnet_conv_up4" and args[1] == 1) else (d.Co0, d.C0)
            nbytes = esz * ((m >> 2) * lo + 16 * d.C0 * d.Co0) + 4.0 * m * hi if name == "rpnet_conv_up4" else 0.0
            key = "rpnet_conv_fwd" if name == "rpnet_conv_up4" else "rpnet_conv_wgrad"      # same groups as the nine-tap launches
        a.record()
        orig(name, *args)
        b.record()
        records.append((key, flops, nbytes, a, b))

    hip.call = timed
    import rpnet_amd.functional as RF
    RF.call = timed
    import rpnet_amd.modules as RM
    was_async, was_cre, was_enc = RF._ASYNC["on"], RM._CRE_STREAMS_TRAIN, RM._ENC_STREAMS
    RF.set_async_wgrad(False)   # per-kernel durations need each launch to own the GPU: streams serialised here
    RM._CRE_STREAMS_TRAIN = False   # (the CRE's second branch and the encoder's second chain too)
    RM._ENC_STREAMS = 0
    try:
        step(net, bucket, inp, scaler)
        torch.cuda.synchronize()
    finally:
        hip.call = orig
        RF.call = orig
        RF.set_async_wgrad(was_async)
        RM._CRE_STREAMS_TRAIN = was_cre
        RM._ENC_STREAMS = was_enc
    agg = {}
    for name, flops, nbytes, a, b in records:
        e = agg.setdefault(name, [0, 0.0, 0.0, 0.0])
        e[0] += 1
        e[1] += a.elapsed_time(b) * 1e-3
        e[2] += flops
        e[3] += nbytes
    return agg


def pmc_traffic(math="f16x2", size=256, batch=8):
    """HBM bytes per launch of the dominant kernel from the NEWEST committed rocprofv3 PMC passes OF THE SAME ARITHMETIC AND
    WORKLOAD (profiles/rNN_pmc_traffic[_<math>_<size>].json: separate --pmc FETCH_SIZE / WRITE_SIZE runs of this very
    command, KiB units, read side doubled per the gfx950 note of MI355X_MICROARCH.md; tools/pmc_traffic.py).
    A PMC pass cannot run inside the timed process, so this is the offline figure (its file named in `traffic_source`)
    or None when no pass of this arithmetic / size has been committed."""
    import glob
    pmc_traffic.source = None
    tag = "" if (math, size, batch) == ("f16x2", 256, 8) else f"_{math}_{size}"
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r[0-9][0-9]_pmc_traffic{tag}.json")))
    if not files:
        return None
    d = json.load(open(files[-1]))
    n = b = 0.0
    for k, v in d.items():
        if "conv_igemm" in k:
            n += v["launches"]
            b += v["launches"] * (v["fetch_bytes_per_launch"] + v["write_bytes_per_launch"])
    if not n:
        return None
    pmc_traffic.source = os.path.basename(files[-1])
    return round(b / n)


def conv_accuracy_probe(dev):
    """max |err| / max |ref| of one 3x3 convolution (2x32x32, 256 -> 256) against an fp64 CPU reference under each
    arithmetic: the evidence that the default split arithmetic is fp32-accurate (same probe as
    tests/test_gpu_ops.py::test_split_conv_accuracy, forward only)."""
    import ctypes as C
    import torch.nn.functional as F
    import rpnet_amd.functional as RF
    from rpnet_amd.hip import call
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 32, 32, 256, generator=g)
    w = torch.randn(256, 256, 3, 3, generator=g) * 0.05
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), padding=1).permute(0, 2, 3, 1)
    xd, wd = x.to(dev), w.to(dev)
    pw = RF.PackedWeight(wd)
    out = {}
    for name, planes in (("f32", 0), ("bf16x3", 3), ("f16x2", 2)):
        y = torch.empty(2, 32, 32, 256, device=dev)
        if planes == 2:      # fp16 planes of x / s, s = a power of two with max|x| / s <= 2^15 (here from the data itself)
            s_in = torch.tensor([2.0 ** (int(torch.ceil(torch.log2(x.abs().max())).item()) - 15)], device=dev)
            xs, sx = RF.split_f16(xd, s_in, planes=2)
            wps, _, t_row, _ = pw.split_packs(2)
            d = RF._desc(xs, None, wps, None, None, 0, y, None, 2, 32, 32, 9, 0)
            d.split_planes, d.acc_scale_col, d.acc_scale_x = 2, t_row.data_ptr(), sx.data_ptr()
        elif planes:
            xs = RF.split_bf16(xd, planes)
            d = RF._desc(xs[0], None, pw.split_packs(planes)[0], None, None, 0, y, None, 2, 32, 32, 9, 0)
            d.split_planes = planes
        else:
            d = RF._desc(xd, None, pw.wp, None, None, 0, y, None, 2, 32, 32, 9, 0)
        call("rpnet_conv_fwd", C.byref(d))
        out[name] = float((y.double().cpu() - ref).abs().max() / ref.abs().max())
    return out


def eval_leg(net, cfg, dev, size, RF):
    """The reference's only entry point is evaluation (test_rpnet.py:151-258: eval mode, no_grad, 2-slice batches, T = 10,
    test_rpnet.py:51,164,189-215): forward-only latency of that call, and of the same call at batch 8 (where the eval-mode
    fp16 planes pay, rpnet_amd.modules._F16_MIN_PIXELS_EVAL), with the conv launches' own roofline entry (HIP events on
    the launch stream over one extra call)."""
    was_training, old_T = net.training, net.num_iter
    net.eval()
    net.num_iter = cfg.get("n_test_iter_refinement", 10)
    out = {"workload": f"eval mode, torch.no_grad, 1-way 1-shot {size}x{size}, T={net.num_iter} "
                       "(test_rpnet.py:189-215 call shape), packs / folded BatchNorm rebuilt every call", "calls": []}
    try:
        for B in (2, 8):
            si, fg, bg, qi, ql, appr = make_inputs(77, B, size, dev)
            with torch.no_grad():
                for _ in range(3):
                    net(si, fg, bg, qi, appr_query_labels=appr)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = 20
                for _ in range(n):
                    net(si, fg, bg, qi, appr_query_labels=appr)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / n * 1e3
                # per-launch figures of the conv kernels of one more call
                recs, orig = [], RF.call

                def timed(name, *args):
                    if name != "rpnet_conv_fwd":
                        return orig(name, *args)
                    d = args[0]._obj
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    orig(name, *args)
                    b.record()
                    recs.append((2.0 * d.N * d.H * d.W * (d.C0 + d.C1) * (d.Co0 + d.Co1) * d.taps, d.split_planes, a, b))
                import rpnet_amd.modules as RM
                RF.call = timed
                RF.reset_arith()
                cre_streams, RM._CRE_STREAMS = RM._CRE_STREAMS, False   # per-launch durations: one launch at a time on the GPU
                try:
                    net(si, fg, bg, qi, appr_query_labels=appr)
                    torch.cuda.synchronize()
                finally:
                    RF.call = orig
                    RM._CRE_STREAMS = cre_streams
            # the same call replayed from a HIP graph (rpnet_amd.graph.GraphedEval: the serving form; packs and folded BatchNorm
            # affines are then made once, outside the replay)
            from rpnet_amd.graph import GraphedEval
            frozen = net.freeze_packs
            try:
                ge = GraphedEval(net)
                for _ in range(3):
                    ge(si, fg, bg, qi, appr_query_labels=appr)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    ge(si, fg, bg, qi, appr_query_labels=appr)
                torch.cuda.synchronize()
                ms_graph = (time.perf_counter() - t0) / n * 1e3
                # the same replay with the zero-tile skip of the masked CRE convolutions (the library's default; bench.py's other
                # figures are dense): the support mask and, from the second iteration on, the model's own prediction decide
                # how many tiles run
                skip_was, RF._MASK_SKIP = RF._MASK_SKIP, True
                try:
                    net._cache.clear()
                    ge2 = GraphedEval(net)
                    for _ in range(3):
                        ge2(si, fg, bg, qi, appr_query_labels=appr)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(n):
                        ge2(si, fg, bg, qi, appr_query_labels=appr)
                    torch.cuda.synchronize()
                    ms_graph_skip = (time.perf_counter() - t0) / n * 1e3
                    del ge2
                finally:
                    RF._MASK_SKIP = skip_was
            finally:
                net.freeze_packs = frozen
                net._cache.clear()
            fl = sum(r[0] for r in recs)
            tt = sum(r[2].elapsed_time(r[3]) for r in recs) * 1e-3
            planes = max((r[1] for r in recs if r[0] > 1e9), default=0)
            math = {0: "f32", 1: "f16", 2: "f16x2", 3: "bf16x3"}[planes]
            peak = MATH[math][1]
            out["calls"].append({"batch": B, "ms_per_call": round(ms, 3), "ms_per_call_graph_replay": round(ms_graph, 3),
                                 "ms_per_call_graph_replay_mask_tile_skip": round(ms_graph_skip, 3),
                                 "value": round(B / ms * 1e3, 1), "unit": "pairs/s (forward)",
                                 "conv_math": math, "launches_by_arithmetic": RF.arith_counts(),
                                 "roofline": {"bound": "mfma", "kernel": "rpnet_conv_fwd launches", "achieved": round(fl / tt / 1e12, 2),
                                              "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(fl / tt / 1e12 / peak, 4),
                                              "launches": len(recs), "conv_ms_per_call": round(tt * 1e3, 3)}})
    finally:
        net.num_iter = old_T
        net.train(was_training)
    # eval-mode fp16 planes run on scales predicted from the previous call (rpnet_amd.functional.pred_*): how many calls did,
    # and how many had to be redone on measured scales because a layer's maximum outgrew its prediction
    out["fp16_scale_prediction"] = RF.pred_stats()
    return out


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _cpu_leg(cfg, size, T, B, as_written, seconds_budget, max_steps, threads=None):
    """One CPU leg: the oracle fwd+bwd (same loss as the GPU step) on a seed-1234 synthetic episode, one warm-up step,
    then timed steps until the budget or `max_steps`; returns (leg dict, state of the last step).  `threads`: a list of
    thread counts to try first (one step each) — the leg then runs with the fastest, so that the baseline is the host's
    best, not its default (all hardware threads on operators this small is slower than a fraction of them)."""
    import statistics
    from oracle import rpnet_oracle as O
    from rpnet_amd.utils.synth import make_episode
    cfg = dict(cfg)
    cfg["n_iter_refinement"] = T
    ep = make_episode(1234, B, size)
    t = torch.from_numpy
    si, fg, bg = [[t(ep["support_images"][0][0])]], [[t(ep["support_fg"][0][0])]], [[t(ep["support_bg"][0][0])]]
    qi, ql, appr = [t(ep["query_images"])], t(ep["query_labels"]), t(ep["appr_query_labels"])
    P = O.seeded_params(cfg["mask_refinement_correlation_radius"], requires_grad=True)
    last = {}

    def one():
        for p in P.values():
            p.grad = None
        out = O.rp_net_forward(P, cfg, si, fg, bg, qi, appr, True, align=True, as_written=as_written)
        loss = O.total_loss(out, ql, cfg["align_loss_scaler"])
        loss.backward()
        last["loss"] = loss.item()

    one()  # warm-up
    tried = {}
    if threads:
        default = torch.get_num_threads()
        for n in threads:
            torch.set_num_threads(n)
            t0 = time.perf_counter()
            one()
            tried[n] = round(time.perf_counter() - t0, 3)
        best = min(tried, key=tried.get)
        torch.set_num_threads(best if tried[best] < 0.9 * tried.get(default, 1e9) else default)
    times, t_all = [], time.perf_counter()
    while True:
        t0 = time.perf_counter()
        one()
        times.append(time.perf_counter() - t0)
        if time.perf_counter() - t_all > seconds_budget or len(times) >= max_steps:
            break
    med = statistics.median(times)
    leg = {"value": round(B / med, 4), "unit": "pairs/s", "batch": B, "size": size, "T": T,
           "mode": "as-written (the reference's operator sequence: all-pairs correlation + grid_sample, explicit "
                   "bilinear up-sampling in getFeatures, prototypes per iteration)" if as_written else
                   "algorithmic (local-window correlation, adjoint-mask prototypes hoisted out of the loop)",
           "steps": len(times), "median_s_per_step": round(med, 3), "threads": torch.get_num_threads()}
    if tried:
        leg["s_per_step_by_threads"] = tried
    return leg, (P, last, (si, fg, bg, qi, ql, appr))


def _cpu_worker(argv):
    """hidden mode `bench.py --cpu-worker THREADS SIZE T SECONDS CPULIST`: one process of the concurrent CPU leg — the
    oracle's as-written fwd+bwd on its own batch-1 episode, THREADS threads pinned to the comma-separated CPULIST (a slice of
    the PARENT's allowed set, chosen by the parent so that the slices are disjoint), for about SECONDS; prints one JSON line"""
    threads, size, T, seconds = int(argv[0]), int(argv[1]), int(argv[2]), float(argv[3])
    cpus = {int(c) for c in argv[4].split(",")} if len(argv) > 4 and argv[4] else set()
    pinned = False
    try:
        if cpus:
            os.sched_setaffinity(0, cpus)
            pinned = os.sched_getaffinity(0) == cpus
    except (AttributeError, OSError):
        pass
    torch.set_num_threads(threads)
    cfg = yaml.load(open(os.path.join(ROOT, "yamls", "example.yml")), Loader=yaml.FullLoader)
    leg, _ = _cpu_leg(cfg, size, T, 1, True, seconds, 64)
    print(json.dumps({"steps": leg["steps"], "median_s_per_step": leg["median_s_per_step"], "threads": threads, "pinned": pinned}))


def _allowed_cpus():
    """the CPUs this process may run on (the lease's affinity mask / cgroup cpuset), sorted — NOT os.cpu_count(), which is the
    machine's: round 4's whole-host leg sized itself from the latter on a box whose lease was narrower, and seven of its eight
    workers fell back to the whole allowed set and fought the first one"""
    try:
        return sorted(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        return list(range(os.cpu_count() or 1))


def _cpu_aggregate_leg(size, T, threads, seconds):
    """The host's real throughput on this workload: episodes are independent, so floor(allowed CPUs / 2 / threads) processes of
    `threads` threads each run the as-written oracle CONCURRENTLY (one episode each, each pinned to its own DISJOINT, contiguous
    slice of the sorted allowed-CPU list: contiguous CPU numbers share a NUMA node / CCD on these hosts); the aggregate is the sum of
    their rates.  (One process cannot use the host: PyTorch's CPU operators at these sizes get slower beyond ~16 threads.)
    The leg is REJECTED (consistent = False; the caller then reports the single-process figure) when the processes' rates differ by
    more than 2x — the signature of workers sharing cores."""
    import subprocess
    allowed = _allowed_cpus()
    # every second allowed CPU is left idle (SMT siblings / the rest of the box's tenants): slices of 2 x threads CPUs, the
    # worker pinned to the whole slice (the kernel places its `threads` threads on it)
    width = 2 * max(threads, 1)
    procs_n = max(1, len(allowed) // width)
    slices = [allowed[i * width:(i + 1) * width] for i in range(procs_n)]
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker"]
    env = dict(os.environ, OMP_NUM_THREADS=str(threads), MKL_NUM_THREADS=str(threads))
    procs = [subprocess.Popen(cmd + [str(threads), str(size), str(T), str(seconds), ",".join(map(str, sl))], stdout=subprocess.PIPE,
                              stderr=subprocess.DEVNULL, text=True, env=env) for sl in slices]
    rates, steps, pinned = [], 0, 0
    for p in procs:
        out, _ = p.communicate(timeout=60 + 20 * seconds)
        lines = [ln for ln in out.splitlines() if ln.startswith("{")]
        if p.returncode == 0 and lines:
            r = json.loads(lines[-1])
            rates.append(1.0 / r["median_s_per_step"])
            steps += r["steps"]
            pinned += int(bool(r.get("pinned")))
    if not rates:
        return None
    return {"value": round(sum(rates), 4), "unit": "pairs/s", "processes": len(rates), "threads_per_process": threads,
            "cores": len(rates) * threads, "allowed_cpus": len(allowed), "machine_cpus": os.cpu_count(), "cpus_per_process": width,
            "processes_pinned": pinned, "steps_total": steps, "per_process_pairs_per_s": [round(r, 3) for r in rates],
            "consistent": bool(max(rates) <= 2.0 * min(rates)),
            "mode": "as-written oracle, one batch-1 episode per process, all processes concurrent, each pinned to its own contiguous "
                    "slice of the allowed CPUs"}


def cpu_baseline(cfg, size, T, seconds_budget=18.0, net=None, bucket=None, dev=None, full=False):
    """The CPU oracle fwd+bwd on the host cores, same loss.  `value` = the as-written mode (what "the
    reference CPU path" costs) at batch 1 of the benched size, a bounded sample; `legs` adds the algorithmic mode and
    BASELINE configs[0] (128^2, T=1) — and with --cpu-baseline-full batch 8 in both modes, 3 + 5 steps each (minutes).
    With `net` (the benched model: same seeded parameters) the as-written episode also goes through the HIP path under
    the arithmetic being benched and the two results are compared (`parity`) — the oracle in its checker role, at the
    headline image size."""
    default_threads = torch.get_num_threads()
    cand = sorted({default_threads, max(default_threads // 4, 1), min(default_threads, 16)}, reverse=True)
    main_leg, (P, last, (si, fg, bg, qi, ql, appr)) = _cpu_leg(cfg, size, T, 1, True, seconds_budget, 8 if not full else 5,
                                                                 threads=cand)
    res = {"value": main_leg["value"], "unit": "pairs/s", "cores": torch.get_num_threads(), "kind": "port",
           "nproc": os.cpu_count(), "cpu_model": _cpu_model(),
           "sample": f"{main_leg['steps']} fwd+bwd steps (median) of batch 1 at {size}x{size}, T={T}, oracle as-written mode "
                     f"(reference operator sequence), {main_leg['median_s_per_step']:.2f} s/step", "legs": [main_leg]}
    # the honest figure: the whole host, not one process of it
    agg = _cpu_aggregate_leg(size, T, main_leg["threads"], 12.0)
    res["allowed_cpus"] = len(_allowed_cpus())
    if agg is not None and not agg["consistent"]:
        res["note"] = ("the whole-host leg was rejected (its processes' rates differ by more than 2x: workers shared cores); `value` is "
                       "the single-process figure")
    if agg is not None and agg["consistent"] and agg["value"] > res["value"]:
        res["single_process_value"] = res["value"]
        res["value"], res["cores"] = agg["value"], agg["cores"]
        res["sample"] = (f"{agg['processes']} concurrent processes x {agg['threads_per_process']} threads, each the as-written oracle "
                         f"fwd+bwd on its own batch-1 episode at {size}x{size}, T={T} for ~12 s ({agg['steps_total']} steps in all); "
                         f"aggregate = sum of the processes' rates; one process alone: {main_leg['value']} pairs/s")
    if agg is not None:
        res["aggregate_leg"] = agg
    if net is not None:
        mv = lambda a: a.to(dev)  # noqa: E731
        loss = step(net, bucket, ([[mv(si[0][0])]], [[mv(fg[0][0])]], [[mv(bg[0][0])]], [mv(qi[0])], mv(ql), mv(appr)),
                    cfg["align_loss_scaler"])
        torch.cuda.synchronize()
        grads = {}
        for name in ("cre.w_k.0.weight", "cre.q.0.weight", "encoder.Up_conv4.conv.3.weight", "encoder.Conv5.conv.0.weight",
                     "encoder.Conv1.conv.3.weight"):
            a, b = dict(net.named_parameters())[name].grad.double().cpu(), P[name].grad.double()
            grads[name] = float((a - b).norm() / b.norm())
        res["parity"] = {"what": f"the same batch-1 {size}x{size} episode and seeded parameters through the HIP path (arithmetic of this "
                                 "run) against the CPU oracle: loss, and relative L2 error of five weight gradients (these are conditioned by "
                                 "ReLU / max-pool / 0.5-threshold switches: tests/test_gpu_model.py::test_gradients_vs_fp64_yardstick "
                                 "holds them against an fp64 oracle)",
                         "loss_hip": round(loss.item(), 6), "loss_oracle": round(last["loss"], 6),
                         "loss_rel_err": abs(loss.item() - last["loss"]) / abs(last["loss"]), "weight_grad_rel_l2_err": grads}
    del P
    extra = [(size, T, 1, False, 8.0, 5), (128, 1, 1, True, 4.0, 5)]
    if full:
        extra = [(size, T, 1, False, 60.0, 5), (size, T, 8, True, 600.0, 5), (size, T, 8, False, 300.0, 5),
                 (128, 1, 1, True, 30.0, 5), (128, 1, 1, False, 30.0, 5)]
    for sz, tt, bb, aw, budget, mx in extra:
        res["legs"].append(_cpu_leg(cfg, sz, tt, bb, aw, budget, mx)[0])      # with the thread count the main leg chose
    torch.set_num_threads(default_threads)
    return res


# N > 1: the HIP-graph form of the step is CAPTURED BEFORE dist.init_process_group — no communicator, no collective-library
# watchdog thread exists while the stream is being captured — and replayed beside the communicator afterwards (each replay followed
# by ONE all-reduce of the flat bucket).  Round 4 captured in a process that already held a one-rank RCCL group and saw a
# segmentation fault inside hipStreamEndCapture in 3 of 12 runs; profiles/r05_graph_capture_order.txt: 12 of 12 runs complete in
# either order on this round's tree, gradients bit-identical to the eager step.  The timed steps use the replay when the probe
# finds ANY rank's host unable to keep ahead of its GPU (8 Python processes on one shared host); RPNET_BENCH_DDP_GRAPH=0: never.
DDP_GRAPH = os.environ.get("RPNET_BENCH_DDP_GRAPH", "1") == "1"


def measure(w, world, rank, dev, cfg, steps, warmup, RF, ddp=None, init_group=None, full=True, dump_dir=None):
    """Times `steps` steps of workload w = dict(ways, shots, size, iters, batch, conv_math) after `warmup` untimed ones
    (barrier + synchronize on both sides, MAX over ranks); with `full`, then one extra profiled step (HIP events per C-ABI call,
    streams serialised) and (N > 1) the other way of issuing the step.  `dump_dir`: rank 0 writes the last timed step's
    outputs there (dump_outputs).  -> dict with value, ms_per_step, the per-call aggregate, the arithmetic that ran, the model."""
    from rpnet_amd.parallel import FlatGradBucket, broadcast_parameters
    ddp = (world > 1) if ddp is None else ddp      # the gradient exchange runs (N > 1, or the forced one-rank RCCL group)
    cfg = dict(cfg)
    cfg["n_iter_refinement"] = w["iters"]
    scaler = cfg["align_loss_scaler"]
    RF.set_conv_math(w["conv_math"])
    requested = math = RF.conv_math()
    torch.cuda.reset_peak_memory_stats(dev)
    net = build_model(cfg, dev)
    bucket = FlatGradBucket(net, force_active=ddp)
    inp = make_inputs(1234 + rank, w["batch"], w["size"], dev, w["shots"], w["ways"])   # resident in HBM before timing
    exposed = [] if ddp else None
    pre_gts = None
    if init_group is not None:
        # the process group does not exist yet (main() hands its creation in): capture the replay form of the step first
        if DDP_GRAPH and os.environ.get("RPNET_DIST_BACKEND", "nccl") == "nccl" and os.environ.get("RPNET_BENCH_GRAPH", "auto") != "0":
            for _ in range(2):
                step(net, bucket, inp, scaler)          # (no group yet: the bucket's exchange is a no-op)
            torch.cuda.synchronize()
            pre_gts = graphed_step(net, bucket, scaler, exposed)
            pre_gts.capture(*inp)
            torch.cuda.synchronize()
        init_group()
    broadcast_parameters(net)

    def fence():
        torch.cuda.synchronize()
        if ddp:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(warmup):
        step(net, bucket, inp, scaler)
    fence()
    # How the timed steps are issued, decided BEFORE the timed region from a probe of three untimed steps: eagerly (the
    # default: ~450 launches from Python per step, the faster way while the host keeps ahead of the GPU), or — single
    # process, when the host's enqueue time of a step has reached the GPU's time for it (a busy shared host: the boxes of
    # the pool are shared) — as replays of the step captured into a HIP graph (rpnet_amd.graph.GraphedTrainStep: one launch
    # per step from the host, bit-identical gradients).  RPNET_BENCH_GRAPH=0 / 1 forces eager / replay.
    mode, probe = "eager", None
    want = os.environ.get("RPNET_BENCH_GRAPH", "auto")
    if want != "0":
        pa, pb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hs = []
        pa.record()
        for _ in range(3):
            h0 = time.perf_counter()
            step(net, bucket, inp, scaler)
            hs.append(time.perf_counter() - h0)
        pb.record()
        fence()
        probe = {"host_enqueue_ms": round(1e3 * sorted(hs)[1], 3), "gpu_ms_per_step": round(pa.elapsed_time(pb) / 3, 3)}
        bound = want == "1" or probe["host_enqueue_ms"] > 0.95 * probe["gpu_ms_per_step"]
        if ddp:      # one decision for the job: every rank replays if ANY rank's host cannot keep ahead of its GPU
            flag = torch.tensor([1.0 if bound else 0.0], device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            probe["host_bound_ranks_any"] = bound = bool(flag.item() > 0)
        if bound and ddp and pre_gts is None:
            # under a process group only the graph captured BEFORE the group existed is replayed (see DDP_GRAPH): never a capture
            # beside a live communicator (gloo: segmentation fault or hang in round 4; profiles/r04_graph_capture_under_rccl.txt)
            bound = False
        if bound:
            mode = "hip_graph_replay"
    gts = None
    if mode == "hip_graph_replay":
        gts = pre_gts if pre_gts is not None else graphed_step(net, bucket, scaler, exposed)
        for _ in range(2):
            gts(*inp[:4], inp[4], inp[5])
        fence()
        if exposed:
            exposed.clear()
    # per-step marks (an event on the compute stream + the host clock after each step's enqueue; no synchronisation): the
    # spread of the timed steps goes into the line next to their total, so that one slow step (a busy host: the boxes are
    # shared) is visible as such
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    host = []
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(steps):
        h0 = time.perf_counter()
        loss = gts(*inp[:4], inp[4], inp[5]) if gts is not None else step(net, bucket, inp, scaler, exposed)
        marks[i + 1].record()
        host.append(time.perf_counter() - h0)
    fence()
    el = time.perf_counter() - t0
    if dump_dir is not None and rank == 0:
        dump_outputs(dump_dir, loss, bucket)       # before any later step overwrites the bucket
    gts = None
    step_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    spread = {"min": round(step_ms[0], 3), "median": round(step_ms[len(step_ms) // 2], 3), "max": round(step_ms[-1], 3),
              "host_enqueue_median": round(1e3 * sorted(host)[len(host) // 2], 3),
              "what": "per timed step: HIP events on the compute stream between the steps' ends (ms); the host's enqueue time of a step",
              "issued": mode, "probe": probe,
              "issued_what": "eager = ~450 launches per step from Python (N > 1: the gradient exchange in three segments from hooks during "
                             "backward); hip_graph_replay = the captured step replayed (N > 1: followed by ONE all-reduce of the whole bucket, "
                             "exposed) — chosen before the timed region when the probe's host enqueue time exceeds 0.95 of its GPU time per "
                             "step on any rank: a busy host"}
    if math in ("f16x2", "f16") and not RF.f16_mode():
        # a call below the fp16 threshold (rpnet_amd.modules._F16_MIN_PIXELS: small, launch-bound episodes) ran on bf16
        # planes: label the line with what ran (`requested` keeps what was asked for)
        math = "bf16x3"
    dist_info = None
    if ddp:
        tt = torch.tensor([el], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        el = float(tt.item())
        # did the collective library see every rank, and how much of the exchange is NOT hidden under backward
        ones = torch.ones(1, device=dev)
        dist.all_reduce(ones, op=dist.ReduceOp.SUM)
        ex = torch.tensor([sum(a.elapsed_time(b) for a, b in exposed) / max(len(exposed), 1)], device=dev, dtype=torch.float64)
        dist.all_reduce(ex, op=dist.ReduceOp.MAX)
        # the OTHER way of issuing the step, 5 steps, so that the line carries both (eager + overlapped exchange / graph replay
        # + exposed exchange) whichever the probe chose
        other_ex = []
        # On a real multi-GPU job the extra leg is opt-in (RPNET_BENCH_DDP_OTHER=1): graph replay beside RCCL communicators has only
        # been exercised with ONE rank here (no multi-GPU lease in any round), and a crash in an informational leg would take the
        # headline line with it.  The replay form stays captured: it is the fallback the probe above switches to when any rank's
        # host cannot keep ahead of its GPU.
        if not full or pre_gts is None or (world > 1 and os.environ.get("RPNET_BENCH_DDP_OTHER", "0") != "1" and mode == "eager"):
            # (also: no replay form without the graph captured before the group existed — gloo plumbing runs, RPNET_BENCH_DDP_GRAPH=0)
            other = None
        else:
            if mode == "eager":
                og = pre_gts
                og.exposed = other_ex
                run_other = lambda: og(*inp[:4], inp[4], inp[5])  # noqa: E731
            else:
                og = None
                run_other = lambda: step(net, bucket, inp, scaler, other_ex)  # noqa: E731
            for _ in range(2):
                run_other()
            other_ex.clear()
            fence()
            t1 = time.perf_counter()
            for _ in range(5):
                run_other()
            fence()
            to = torch.tensor([time.perf_counter() - t1], device=dev, dtype=torch.float64)
            dist.all_reduce(to, op=dist.ReduceOp.MAX)
            oex = torch.tensor([sum(a.elapsed_time(b) for a, b in other_ex) / max(len(other_ex), 1)], device=dev, dtype=torch.float64)
            dist.all_reduce(oex, op=dist.ReduceOp.MAX)
            del og
            other = {"issued": "hip_graph_replay" if mode == "eager" else "eager", "value": round(world * w["batch"] * 5 / float(to.item()), 3),
                     "unit": "pairs/s", "steps": 5, "ms_per_step": round(1e3 * float(to.item()) / 5, 3),
                     "allreduce_exposed_ms": round(float(oex.item()), 3)}
        dist_info = {"issued": mode, "other_issue_mode": other,
                     "backend": dist.get_backend() + (" (RCCL over xGMI)" if dist.get_backend() == "nccl" else " (plumbing test, not RCCL)"),
                     "rccl_ranks_seen": int(round(ones.item())), "world_size": world,
                     "allreduce_exposed_ms": round(float(ex.item()), 3),
                     "allreduce_exposed_what": "HIP events on the compute stream from the end of backward to the averaged bucket, mean "
                                               "over the timed steps, max over ranks; eager: the first two of the three bucket segments go out "
                                               "from post-accumulate hooks during backward (rpnet_amd/parallel.py); hip_graph_replay: the whole "
                                               "bucket in one collective behind the replay",
                     "bucket_segments_mb": [round((bucket.bounds[i + 1] - bucket.bounds[i]) * 4 / 1e6, 1)
                                            for i in range(len(bucket.bounds) - 1)]}
    assert torch.isfinite(loss).item()
    # The profiled extra step contains the gradient all-reduce, so EVERY rank runs it (a collective
    # issued by rank 0 alone would never complete); only rank 0 reports.
    # peak of torch's allocator over model, inputs, warm-up and the timed steps (the tensors an asynchronous weight gradient reads
    # are kept alive until the side streams are joined at the end of backward: this is what that costs)
    peak_gb = round(torch.cuda.max_memory_allocated(dev) / 2.0 ** 30, 2)
    agg = arith = None
    if full:
        RF.reset_arith()
        agg = profile_step(net, bucket, inp, scaler)
        arith = RF.arith_counts()          # which arithmetic every conv / correlation launch of that step actually ran
    return {"value": world * w["batch"] * steps / el, "el": el, "spread": spread, "agg": agg, "arith": arith, "math": math, "requested": requested,
            "peak_gb": peak_gb,
            "net": net, "bucket": bucket, "inp": inp, "scaler": scaler, "cfg": cfg, "dist": dist_info, "fence": fence}


def graphed_step(net, bucket, scaler, exposed=None):
    """the bench step (same objective as `step`) as a rpnet_amd.graph.GraphedTrainStep (N > 1: the replay is followed by one
    all-reduce of the whole bucket, bracketed by a HIP-event pair appended to `exposed`)"""
    import rpnet_amd.functional as RF
    from rpnet_amd.graph import GraphedTrainStep

    def loss_fn(out, ql):
        return RF.objective([out["output"], *out["refinement"].values()], ql, out["align_loss"], scaler)
    return GraphedTrainStep(net, bucket, loss_fn, exposed=exposed)


def graph_replay_leg(net, bucket, inp, scaler, batch, fence, steps):
    """The timed step captured once into a HIP graph (rpnet_amd.graph.GraphedTrainStep) and replayed `steps` times: the host
    then enqueues ONE launch per step, so the figure does not depend on how busy the (shared) host is."""
    gts = graphed_step(net, bucket, scaler)
    for _ in range(2):
        gts(*inp[:4], inp[4], inp[5])
    fence()
    t1 = time.perf_counter()
    for _ in range(steps):
        gts(*inp[:4], inp[4], inp[5])
    t_enq = time.perf_counter() - t1
    fence()
    t_all = time.perf_counter() - t1
    del gts
    return {"value": round(batch * steps / t_all, 3), "unit": "pairs/s", "steps": steps, "ms_per_step": round(1e3 * t_all / steps, 3),
            "host_enqueue_ms_per_step": round(1e3 * t_enq / steps, 3),
            "what": "the timed step captured once into a HIP graph and replayed (bit-identical gradients: "
                    "tests/test_gpu_model.py::test_graphed_train_step_matches_eager); `value` above is the eager step unless step_ms.issued says hip_graph_replay"}


CONV_MATH_TEXT = {
    "f32": "v_mfma_f32_32x32x2_f32 on fp32 operands",
    "bf16x3": "fp32 operands as 3 bf16 planes (exact split), 6 v_mfma_f32_32x32x16_bf16 partial "
              "products, fp32 accumulate: fp32-equivalent (dropped terms <= 2^-23 |x*y|)",
    "f16x2": "fp32 operands as 2 fp16 planes of operand / (power-of-two scale from a rigorous bound: "
             "BatchNorm outputs and gradients, weights), 3 v_mfma_f32_32x32x16_f16 partial products, "
             "fp32 accumulate (dropped term <= 2^-22 |x*y|; measured error vs fp64 = the fp32 matrix "
             "instruction's); the local correlation the same way (block-local scale for its window gradients); operands without a bound (eval mode) on 3 bf16 planes",
    "f16": "REDUCED PRECISION (BASELINE configs[4]): conv / correlation operands as ONE fp16 plane of operand / "
           "(power-of-two tensor scale), v_mfma_f32_32x32x16_f16, fp32 accumulate, fp32 BatchNorm "
           "statistics, fp32 master weights and gradients; tolerance vs the fp32 reference: "
           "tests/test_gpu_f16.py (logits 1e-2, Dice 1e-3)"}


def roofline_of(m, w, world):
    """the `roofline` object of a measured workload: the rpnet_conv_fwd launches (forward + input gradient) of the profiled step"""
    agg, math, value = m["agg"], m["math"], m["value"]
    products, peak = MATH[math]
    # (rpnet_conv_up4 / rpnet_conv_wgrad_up4, the collapsed up_conv layers, are booked into the same two groups with their
    # EXECUTED FLOPs: profile_step)
    conv = agg.get("rpnet_conv_fwd", [0, 1e-9, 0.0, 0.0])
    wg = agg.get("rpnet_conv_wgrad", [0, 1e-9, 0.0, 0.0])
    achieved = conv[2] / conv[1] / 1e12
    kern_total = sum(v[1] for v in agg.values())
    gf_pair = algorithmic_gf_per_pair(w["size"], w["iters"], w["shots"], w["ways"])
    traffic = pmc_traffic(math, w["size"], w["batch"])
    return {"bound": "mfma", "kernel": "rpnet_conv_fwd launches (conv forward + dgrad): conv_igemm"
                                       + ("_kernel" if math == "f32" else "_split*_kernel"),
            "achieved": round(achieved, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4), "traffic": traffic,
            "traffic_source": getattr(pmc_traffic, "source", None),
            "peak_basis": "157.3 TF dense fp32 MFMA" if math == "f32" else
                          "2500 TF dense fp16 MFMA" if math == "f16" else
                          f"2500 TF dense bf16 / fp16 MFMA / {products} partial products per fp32 multiply-add "
                          "(achieved counts ALGORITHMIC fp32 FLOPs, not issued MFMA FLOPs)",
            "issued_mfma_tflops": round(achieved * products, 1),
            "traffic_unit": "HBM bytes per launch (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE, offline pass of the same arithmetic and "
                            "workload; null when none is committed)",
            "algorithmic_bytes_per_launch": round(conv[3] / max(conv[0], 1)),
            "launches_per_step": conv[0], "avg_launch_ms": round(1e3 * conv[1] / max(conv[0], 1), 4),
            "algorithmic_gflop_per_step": round(conv[2] / 1e9, 1),
            "flop_accounting": "executed multiply-adds of the launches (the two up_conv layers run 4 of the 9 products per output the "
                               "reference's operator sequence implies: their taps collapse onto the 2 x 2 source pixels an output "
                               "phase reads); whole_step_frac / whole_step_tflops / gflop_per_pair likewise (the reference's sequence count: *_as_written)",
            "wgrad_tflops": round(wg[2] / wg[1] / 1e12, 2),
            # round 6: the PRIMARY whole-step figures count the multiply-adds the step EXECUTES (SURVEY.md 8d's count minus what
            # the collapsed up_conv layers skip); the reference's operator-sequence count stays beside them as *_as_written.  (Rounds 1 - 5
            # printed the as-written count under the primary names and the executed one as *_executed; both spellings are in the line.)
            "whole_step_frac": round(value / world * (gf_pair - upconv_collapse_saved_gf_per_pair(w["size"], w["shots"], w["ways"]))
                                     * 1e9 / (peak * 1e12), 4),
            "whole_step_tflops": round(value / world * (gf_pair - upconv_collapse_saved_gf_per_pair(w["size"], w["shots"], w["ways"])) / 1e3, 1),
            "gflop_per_pair": round(gf_pair - upconv_collapse_saved_gf_per_pair(w["size"], w["shots"], w["ways"]), 1),
            "whole_step_frac_as_written": round(value / world * gf_pair * 1e9 / (peak * 1e12), 4),
            "whole_step_tflops_as_written": round(value / world * gf_pair / 1e3, 1),
            "gflop_per_pair_as_written": round(gf_pair, 1),
            "gflop_per_pair_executed": round(gf_pair - upconv_collapse_saved_gf_per_pair(w["size"], w["shots"], w["ways"]), 1),
            "whole_step_frac_executed": round(value / world * (gf_pair - upconv_collapse_saved_gf_per_pair(w["size"], w["shots"], w["ways"]))
                                              * 1e9 / (peak * 1e12), 4),
            "kernel_time_share": {k: round(v[1] / kern_total, 4) for k, v in
                                  sorted(agg.items(), key=lambda kv: -kv[1][1])[:8]},
            "sum_kernel_ms_per_step": round(1e3 * kern_total, 2),
            "abi_calls_per_step": int(sum(v[0] for v in agg.values())),
            "note": "per-kernel figures from one extra step with the two HIP streams serialised; "
                    "value/ms_per_step measured with async weight gradients on"}


def stream_layout():
    """what the timed step runs beside what: the switches in force, for the record in the line"""
    import rpnet_amd.functional as RF
    import rpnet_amd.modules as RM
    return {"async_wgrad": bool(RF._ASYNC["on"]), "wgrad_released_behind_dgrad": RF._WGRAD_DEFER,
            "cre_second_branch_on_own_stream": bool(RM._CRE_STREAMS_TRAIN), "encoder_two_chains": RM._ENC_STREAMS,
            "what": "same kernels and bits as the one-stream step (tests: test_async_weight_gradients_match, "
                    "test_encoder_two_chains_match_one_stream); per-kernel roofline figures come from an extra step with all of it serialised"}


def workload_text(w, world):
    ns = argparse.Namespace(**w)
    return (f"{w['ways']}-way {w['shots']}-shot, {w['size']}x{w['size']}, T={w['iters']}, batch {w['batch']}/GPU "
            f"({baseline_config(ns, world)}), train mode, align loss on, loss = dice_ce(output)+sum dice_ce(refinement)+align_loss")


def self_launch(n, argv):
    """`python bench.py --gpus N` with no rendezvous in the environment: start the N ranks ourselves — one process per GPU
    through torch.distributed.run on 127.0.0.1 and a free port, exactly the line the driver uses — and hand its exit code
    back; rank 0's JSON line is the only thing on stdout."""
    import socket
    import subprocess
    backend = os.environ.get("RPNET_DIST_BACKEND", "nccl")
    have = torch.cuda.device_count()
    if backend == "nccl" and have < n:
        raise SystemExit(f"bench.py --gpus {n}: this host shows {have} GPU(s); RCCL needs one device per rank "
                         "(RPNET_DIST_BACKEND=gloo runs the ranks on the devices there are: plumbing only)")
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env, cwd=ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8, help="episodes (support/query pairs) per GPU")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5, help="T refinement iterations")
    ap.add_argument("--shots", type=int, default=1, help="support shots (5 with --batch 16 = BASELINE configs[2])")
    ap.add_argument("--ways", type=int, default=1, help="ways (2 with --size 512 --iters 10 --batch 4 --conv-math f16 = "
                                                        "BASELINE configs[4])")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, every informational leg as well: roofline (one extra profiled step), alt_math, "
                         "mask_tile_skip, graph_replay, eval, conv_math_error_vs_fp64, cpu_baseline, other_configs, and the other "
                         "issue mode of an N > 1 run; without it the run does only what the headline needs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's loss and gradients to DIR/*.npy (bench.dump_outputs)")
    ap.add_argument("--cpu-baseline-full", action="store_true",
                    help="with --full: all CPU legs of BASELINE.md §4 (as-written and algorithmic, B=1 and B=8, and configs[0]); minutes")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the BASELINE configs[2] / configs[4] legs the --full single-GPU command appends (`other_configs`)")
    ap.add_argument("--conv-math", choices=sorted(MATH), default=None,
                    help="arithmetic of the 3x3 convolutions (default: the library's, f16x2 = fp32-equivalent fp16 split; "
                         "f16 = plain fp16 operands, configs[4] only)")
    args = ap.parse_args()

    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs (no CPU fallback)"
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        sys.exit(self_launch(args.gpus, sys.argv[1:]))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    if os.environ.get("RPNET_DIST_BACKEND", "nccl") == "nccl":
        assert local_rank < torch.cuda.device_count(), f"LOCAL_RANK {local_rank} but {torch.cuda.device_count()} GPU(s): RCCL needs one device per rank"
    else:
        local_rank %= torch.cuda.device_count()   # > 1 rank per device: only the gloo plumbing test
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # RPNET_BENCH_FORCE_DIST=1 with --gpus 1: a process group of ONE rank, the gradient exchange forced on — the whole N > 1 code
    # path of this file (hooks, segments, RCCL's stream, exposed-time events, the replay + all-reduce leg) on a single GPU
    ddp = world > 1 or os.environ.get("RPNET_BENCH_FORCE_DIST", "0") == "1"
    if ddp:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        backend = os.environ.get("RPNET_DIST_BACKEND", "nccl")   # "nccl" IS RCCL on ROCm; gloo only for 1-GPU plumbing tests
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if "MASTER_PORT" not in os.environ:
                import socket
                sock = socket.socket()
                sock.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sock.getsockname()[1])
                sock.close()

        def init_group():
            if backend == "nccl":
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
            else:
                dist.init_process_group(backend, rank=rank, world_size=world)

    cfg = yaml.load(open(os.path.join(ROOT, "yamls", "example.yml")), Loader=yaml.FullLoader)
    import rpnet_amd.functional as RF
    RF.set_async_wgrad(os.environ.get("RPNET_ASYNC_WGRAD", "1") == "1")   # weight gradients on a second HIP stream
    w = {"ways": args.ways, "shots": args.shots, "size": args.size, "iters": args.iters, "batch": args.batch,
         "conv_math": args.conv_math or RF.conv_math()}
    headline = (args.ways, args.shots, args.size, args.iters, args.batch) == (1, 1, 256, 5, 8) and w["conv_math"] == "f16x2"
    # every timed leg that carries a roofline is DENSE: the zero-tile skip of the masked CRE convolutions (RF._MASK_SKIP, the
    # library's default) leaves out work the algorithmic FLOP count of the metric contains; it gets its own leg (mask_tile_skip)
    RF._MASK_SKIP = False
    # (N > 1: measure() creates the process group itself, AFTER it has captured the replay form of the step — see DDP_GRAPH)
    full = args.full      # the informational legs below run only with --full: a plain run is the headline and nothing else
    m = measure(w, world, rank, dev, cfg, args.steps, args.warmup, RF, ddp, init_group if ddp else None, full=full,
                dump_dir=args.dump_outputs)
    math, requested, value = m["math"], m["requested"], m["value"]
    net, bucket, inp, scaler, fence = m["net"], m["bucket"], m["inp"], m["scaler"], m["fence"]
    cfg = m["cfg"]

    result = None
    alt = None
    if full and world == 1 and not ddp and not args.no_cpu_baseline:
        # the same step under the other fp32-equivalent convolution arithmetics, for reference
        alt = {}
        for other in ("f32", "f16x2", "bf16x3"):
            if other == math or (other == "f16x2" and requested == "f16x2"):    # below the fp16 threshold f16x2 IS bf16x3
                continue
            RF.set_conv_math(other)
            for _ in range(2):
                step(net, bucket, inp, scaler)
            fence()
            t1 = time.perf_counter()
            for _ in range(5):
                step(net, bucket, inp, scaler)
            fence()
            alt[other] = {"value": round(args.batch * 5 / (time.perf_counter() - t1), 3), "unit": "pairs/s", "steps": 5}
        RF.set_conv_math(requested)
    skip_leg = None
    if full and world == 1 and not ddp:
        skip_leg = mask_skip_leg(net, bucket, inp, scaler, args.batch, fence, RF, value)
    graph_leg = None
    if full and world == 1 and not args.no_cpu_baseline:
        # the same step replayed from a HIP graph (rpnet_amd.graph.GraphedTrainStep): the host then enqueues ONE launch per step
        graph_leg = graph_replay_leg(net, bucket, inp, scaler, args.batch, fence, 10)
    if rank == 0:
        result = {
            "metric": f"support/query pairs/sec (fwd+bwd, {args.shots}-shot {args.size}x{args.size}, T={args.iters})",
            "value": round(value, 3), "unit": "pairs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * m["el"] / args.steps, 3), "step_ms": m["spread"], "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f16" if math == "f16" else "f32", "data": "synthetic",
            "conv_math": CONV_MATH_TEXT[math],
            "config": {"workload": workload_text(w, world),
                       "global_batch": world * args.batch, "parallelism": f"dp{world}", "conv_math": math,
                       "conv_math_requested": requested,
                       "streams": stream_layout(),
                       "grad_allreduce_mb": round(bucket.numel * 4 / 1e6, 1)},
            "peak_allocated_gb": m["peak_gb"],
        }
        if full:
            result["config"]["launches_by_arithmetic"] = m["arith"]
            result["roofline"] = roofline_of(m, w, world)
        if m["dist"]:
            result["distributed"] = m["dist"]
        if graph_leg:
            result["graph_replay"] = graph_leg
        if skip_leg:
            result["mask_tile_skip"] = skip_leg
        if alt:
            result["alt_math"] = alt
        if full and world == 1 and not args.no_cpu_baseline and args.ways == 1 and args.shots == 1:
            result["eval"] = eval_leg(net, cfg, dev, args.size, RF)
        if full and world == 1 and not args.no_cpu_baseline:
            result["conv_math_error_vs_fp64"] = {k: float(f"{v:.3g}") for k, v in conv_accuracy_probe(dev).items()}
        if full and world == 1 and not args.no_cpu_baseline and args.shots == 1 and args.ways == 1:
            result["cpu_baseline"] = cpu_baseline(cfg, args.size, args.iters, net=net, bucket=bucket, dev=dev,
                                                  full=args.cpu_baseline_full)
            result["cpu_baseline"]["gpu_over_cpu"] = round(value / result["cpu_baseline"]["value"], 1)
    if full and world == 1 and not ddp and headline and not args.no_other_configs:
        # the secondary BASELINE configurations that fit one GPU, timed by the same command (3 warm-up + 5 timed steps each,
        # their own roofline): configs[2] = 5-shot, batch 16; configs[4] = 2-way 512^2, T = 10, one fp16 plane, at its
        # per-GPU batch of 4 (global batch 32 across 8 GPUs)
        del net, bucket, inp, m
        torch.cuda.empty_cache()
        result["other_configs"] = {}
        for name, ow in (("configs[2]", {"ways": 1, "shots": 5, "size": 256, "iters": 5, "batch": 16, "conv_math": "f16x2"}),
                         ("configs[4]", {"ways": 2, "shots": 1, "size": 512, "iters": 10, "batch": 4, "conv_math": "f16"})):
            om = measure(ow, 1, 0, dev, cfg, 5, 3, RF)
            result["other_configs"][name] = {
                "workload": workload_text(ow, 1), "value": round(om["value"], 3), "unit": "pairs/s", "steps": 5, "warmup": 3,
                "ms_per_step": round(1e3 * om["el"] / 5, 3), "step_ms": om["spread"], "dtype": "f16" if om["math"] == "f16" else "f32",
                "conv_math": om["math"], "launches_by_arithmetic": om["arith"], "roofline": roofline_of(om, ow, 1),
                "peak_allocated_gb": om["peak_gb"]}
            if not args.no_cpu_baseline:
                result["other_configs"][name]["graph_replay"] = graph_replay_leg(om["net"], om["bucket"], om["inp"], om["scaler"],
                                                                                 ow["batch"], om["fence"], 5)
            del om
            torch.cuda.empty_cache()
        if not args.no_cpu_baseline:
            result["other_configs"]["configs[4]"]["fp16_free_running_dice_dev"] = fp16_trained_dice_leg(dev, RF)
        RF.set_conv_math(requested)
    if ddp:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(result))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-worker":
        _cpu_worker(sys.argv[2:])
    else:
        main()
