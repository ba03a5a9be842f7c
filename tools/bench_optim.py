"""The optimizer step on the real model's gradient bucket: torch.optim.Adam against rpnet_amd.optim.FusedAdam, and the two passes
over the bucket that stand beside it (flat.mul_ of the gradient mean, the bucket's memset); then the gradient guard: the norm
launch pair alone (rpnet_grad_sumsq), a guarded step (FusedAdam(max_grad_norm=, skip_nonfinite=True): three launches) and what it
replaces, torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam.step().

    python tools/bench_optim.py [--rounds 7] [--iters 20] [--out profiles/optim_step.txt] [--label TEXT] [--append]

One process, one GPU.  Each figure is a device-event time over `iters` back-to-back calls (no host wait inside the window), taken
`rounds` times with the candidates alternating inside every round; reported: the median per call, min and max over the rounds,
and the effective bandwidth.  The update is counted at 28 bytes per element (read g, p, m, v; write p, m, v), flat.mul_ at 8, the
memset at 4, the norm at 4 (one read of g), the guarded step at 32 (the norm's read and the update), beside the 6.29 TB/s of a float4 copy on this chip.  --label names the library build (its chunk size) in the output;
--append adds to the file instead of replacing it.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import yaml  # noqa: E402

from rpnet_amd import hip  # noqa: E402
from rpnet_amd.modules import RP_Net  # noqa: E402
from rpnet_amd.optim import FusedAdam  # noqa: E402
from rpnet_amd.parallel import FlatGradBucket  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_TBS = 6.29
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step.txt"))
ap.add_argument("--label", default="chunk 4096 (the shipped RPNET_ADAM_CHUNK)")
ap.add_argument("--append", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_optim.py needs the MI355X (no CPU fallback)")
dev = torch.device("cuda:0")
cfg = yaml.load(open(os.path.join(ROOT, "yamls", "example.yml")), Loader=yaml.FullLoader)


def model():
    torch.manual_seed(0)
    net = RP_Net(cfg={"align": True, "backbone": "UNet"}, backbone_cfg=cfg).to(dev)
    bucket = FlatGradBucket(net)
    bucket.flat.copy_(torch.randn(bucket.numel, device=dev) * 1e-2)
    return net, bucket


net_t, bucket_t = model()
opt_t = torch.optim.Adam([p for _, p in bucket_t.params], lr=cfg["init_lr"], weight_decay=cfg["weight_decay"])
net_f, bucket_f = model()
opt_f = FusedAdam(bucket_f, lr=cfg["init_lr"], weight_decay=cfg["weight_decay"])
n = bucket_f.numel
scratch = torch.randn(n, device=dev)
# the guard: a threshold at half the gradient's norm, so that the guarded step and clip_grad_norm_ both really clip
net_g, bucket_g = model()
half = 0.5 * float(bucket_g.flat.double().norm())
opt_g = FusedAdam(bucket_g, lr=cfg["init_lr"], weight_decay=cfg["weight_decay"], max_grad_norm=half, skip_nonfinite=True)
net_c, bucket_c = model()
params_c = [p for _, p in bucket_c.params]
opt_c = torch.optim.Adam(params_c, lr=cfg["init_lr"], weight_decay=cfg["weight_decay"])


def clip_and_adam():
    torch.nn.utils.clip_grad_norm_(params_c, half)          # rewrites the bucket (it multiplies whatever the coefficient is)
    opt_c.step()


cands = {
    "torch.optim.Adam.step()": (opt_t.step, 28),
    "FusedAdam.step()": (opt_f.step, 28),
    "flat.mul_(1 / world)": (lambda: scratch.mul_(0.5), 8),
    "bucket memset (flat.zero_())": (lambda: scratch.zero_(), 4),
    "rpnet_grad_sumsq (grad_norm())": (opt_f.grad_norm, 4),
    "FusedAdam.step() guarded": (opt_g.step, 32),
    "clip_grad_norm_ + Adam.step()": (clip_and_adam, 32),
}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / args.iters * 1e3         # us per call


for fn, _ in cands.values():                             # warm-up: code objects, torch's state tensors, the allocator
    for _ in range(5):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in cands}
order = list(cands)
for r in range(args.rounds):
    for k in (order if r % 2 == 0 else order[::-1]):     # alternate the order
        times[k].append(timed(cands[k][0]))

# the two optimizers were fed the same gradients from the same weights: how far apart are the parameters now
drift = max(float((a.detach() - b.detach()).abs().max()) for (_, a), (_, b) in zip(bucket_t.params, bucket_f.params))
med = {k: statistics.median(v) for k, v in times.items()}
lines = [f"optimizer step on the real bucket: {len(bucket_f.params)} parameters, {n} fp32 elements ({n * 4 / 1e6:.1f} MB), MI355X, "
         f"library {os.path.basename(hip.lib_path())}: {args.label}",
         f"device-event time per call over {args.iters} back-to-back calls, median (min .. max) of {args.rounds} rounds, candidates "
         f"alternating inside each round; bandwidth = bytes the operation needs / median, beside {COPY_TBS} TB/s (float4 copy)"]
for k, (_, bpe) in cands.items():
    v = times[k]
    lines.append(f"  {k:32s} {med[k]:9.1f} us  ({min(v):.1f} .. {max(v):.1f})   {bpe:2d} B/element = {n * bpe / 1e6:7.1f} MB "
                 f"-> {n * bpe / med[k] / 1e3:7.1f} GB/s = {n * bpe / med[k] / 1e6 / COPY_TBS * 100:5.1f} % of the copy rate")
lines.append(f"  torch / fused = {med['torch.optim.Adam.step()'] / med['FusedAdam.step()']:.2f} x; {n * 28 / 1e6:.0f} MB at the copy rate "
             f"would take {n * 28 / COPY_TBS / 1e6:.0f} us")
gs = opt_g.guard_stats()
lines.append(f"  guarded / plain FusedAdam = {med['FusedAdam.step() guarded'] / med['FusedAdam.step()']:.2f} x "
             f"(+{med['FusedAdam.step() guarded'] - med['FusedAdam.step()']:.1f} us); clip_grad_norm_ + Adam / guarded = "
             f"{med['clip_grad_norm_ + Adam.step()'] / med['FusedAdam.step() guarded']:.2f} x; the guard saw norm {gs['norm']:.6g}, "
             f"coef {gs['coef']:.4f}, {gs['clipped']} of {gs['attempt']} steps clipped, {gs['skipped']} skipped")
lines.append(f"  largest |p_torch - p_fused| after the same {5 + args.rounds * args.iters} steps on the same gradient: {drift:.3e}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
