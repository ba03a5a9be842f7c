"""CPU tests of the host logic: C-ABI library loads and exports what include/rpnet_abi.h
declares, module surface / state_dict parity, no-fallback behaviour, and the world-size-2
gradient exchange over gloo."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import load_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_exports_every_declared_symbol():
    from rpnet_amd import hip
    hdr = open(os.path.join(ROOT, "include", "rpnet_abi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rpnet_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 35
    assert os.path.exists(hip.lib_path()), "build librpnet_hip.so first (__graft_entry__.build())"
    lib = ctypes.CDLL(hip.lib_path())
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in rpnet_abi.h but not exported"
    assert declared == set(hip.ABI_SYMBOLS), declared ^ set(hip.ABI_SYMBOLS)
    lib.rpnet_version.restype = ctypes.c_int
    from rpnet_amd import hip as _hip
    hdr = open(os.path.join(ROOT, "include", "rpnet_abi.h")).read()
    assert lib.rpnet_version() == _hip.ABI_VERSION == int(re.search(r"#define RPNET_ABI_VERSION (\d+)", hdr).group(1))   # no compute call without a GPU


def test_index_division_of_the_passes_is_exact():
    """csrc/common.h FastDiv (round 6: the element-wise passes divide their 32-bit element index by launch constants with a host-made
    multiplier instead of hipcc's 64-bit division sequence): the library's host-only self-test — 49 divisors, edge values around their
    multiples and around powers of two, 20 000 random values each — against the C operators."""
    from rpnet_amd import hip
    lib = ctypes.CDLL(hip.lib_path())
    lib.rpnet_debug_fastdiv_selftest.restype = ctypes.c_longlong
    lib.rpnet_debug_fastdiv_selftest.argtypes = [ctypes.c_int]
    assert lib.rpnet_debug_fastdiv_selftest(20000) == 0


def test_prepack_asks_the_library_which_up_conv_layers_collapse():
    """RF.up4_layer_ok (an up_conv layer whose shape the collapsed kernel rejects belongs into the batched nine-tap prepack,
    not into a per-layer pack on first use): the answer comes from rpnet_conv_up4_supported — host logic, no GPU."""
    import torch
    from rpnet_amd import functional as RF
    w5, w4 = torch.zeros(512, 1024, 3, 3), torch.zeros(256, 512, 3, 3)
    got = {H: [RF.up4_layer_ok(w, 2, [(16, H // f, H // f)]) for w, f in ((w5, 8), (w4, 4))] for H in (64, 128, 256)}
    assert got == {64: [False, False], 128: [False, True], 256: [True, True]}
    assert not RF.up4_layer_ok(w5, 3, [(16, 32, 32)])                      # three bf16 planes: the nine-tap form
    assert not RF.up4_layer_ok(w4, 2, [(16, 64, 64), (16, 8, 8)])          # every call of the forward must fit


def test_module_surface_and_state_dict():
    from net.model import model_factory
    from oracle.rpnet_oracle import param_shapes
    cfg = load_cfg()
    net = model_factory["RP_Net"](pretrained_path=None, cfg={"align": True, "backbone": "UNet"}, backbone_cfg=cfg)
    sd = net.state_dict()
    ps = param_shapes()
    assert list(sd.keys()) == list(ps.keys()) and len(sd) == 147
    assert all(tuple(sd[k].shape) == tuple(ps[k]) for k in ps)
    assert sum(p.numel() for p in net.parameters()) == 34972800
    import inspect
    sig = inspect.signature(net.forward)
    assert list(sig.parameters) == ["supp_imgs", "fore_mask", "back_mask", "qry_imgs", "registration_field", "grid",
                                    "query_labels", "appr_query_labels"]
    for bad in ("vgg", "resnet"):
        with pytest.raises(NotImplementedError):
            model_factory["RP_Net"](cfg={"align": True, "backbone": bad}, backbone_cfg=cfg)


def test_no_cpu_fallback():
    """The product path refuses CPU tensors instead of silently computing somewhere else."""
    from rpnet_amd.modules import RP_Net
    cfg = load_cfg(1)
    net = RP_Net(cfg={"align": False, "backbone": "UNet"}, backbone_cfg=cfg)
    x = torch.zeros(1, 1, 32, 32)
    m = torch.zeros(1, 32, 32)
    with pytest.raises(RuntimeError):
        net([[x]], [[m]], [[1 - m]], [x], appr_query_labels=m)
    src = open(os.path.join(ROOT, "rpnet_amd", "functional.py")).read() + open(os.path.join(ROOT, "rpnet_amd", "modules.py")).read()
    assert "oracle" not in src.replace("CPU oracle", "").replace("oracle/", "")


def test_schedule_scope_restores_process_defaults():
    """rpnet_amd.schedule.Schedule / functional.scope (round 6): a model's own options are active only inside its forward call —
    also when the call raises — and an unset field means the process-wide default."""
    import rpnet_amd.functional as RF
    from rpnet_amd.modules import RP_Net
    from rpnet_amd.schedule import Schedule
    base = (RF.conv_math(), RF._ASYNC["on"], RF._MASK_SKIP)
    with RF.scope(conv_math="f32", async_wgrad=not base[1], mask_skip=not base[2]):
        assert (RF.conv_math(), RF._ASYNC["on"], RF._MASK_SKIP) == ("f32", not base[1], not base[2])
        with RF.scope():                                     # all None: nothing changes, nothing is restored to something else
            assert RF.conv_math() == "f32"
        assert RF.conv_math() == "f32"
    assert (RF.conv_math(), RF._ASYNC["on"], RF._MASK_SKIP) == base
    with pytest.raises(ZeroDivisionError):
        with RF.scope(conv_math="bf16x3"):
            1 / 0
    assert RF.conv_math() == base[0]
    sch = Schedule(conv_math="f16", fanin=0)
    assert sch.get("fanin", 2) == 0 and sch.get("enc_streams", 1) == 1 and sch.overrides() == {"conv_math": "f16", "fanin": 0}
    net = RP_Net(cfg={"align": False, "backbone": "UNet"}, backbone_cfg=load_cfg(1))
    assert net.schedule.overrides() == {} and net.cre.schedule is net.schedule and net.encoder.schedule is net.schedule
    assert "schedule" not in "".join(net.state_dict().keys())            # an attribute, not state
    net.schedule.conv_math = "f32"
    x, m = torch.zeros(1, 1, 32, 32), torch.zeros(1, 32, 32)
    with pytest.raises(RuntimeError):                                     # (CPU tensors: the call fails inside the scope ...)
        net([[x]], [[m]], [[1 - m]], [x], appr_query_labels=m)
    assert RF.conv_math() == base[0]                                      # ... and the process default is back


def test_environment_switch_budget():
    """at most 25 RPNET_* environment variables are read by the product (library, bench.py, train_rpnet.py, C++)."""
    import re
    names = set()
    for root in ("rpnet_amd", "bench.py", "train_rpnet.py", "__graft_entry__.py"):
        path = os.path.join(ROOT, root)
        files = [path] if os.path.isfile(path) else [os.path.join(d, f) for d, _, fs in os.walk(path) for f in fs
                                                     if f.endswith((".py", ".hip", ".h")) and "__pycache__" not in d]
        for f in files:
            src = open(f).read()
            names |= set(re.findall(r"environ(?:\.get)?\(?\[?\s*\"(RPNET_[A-Z0-9_]+)\"", src)) | set(re.findall(r"getenv\(\"(RPNET_[A-Z0-9_]+)\"", src))
    assert 0 < len(names) <= 25, sorted(names)


def _ddp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from rpnet_amd.parallel import FlatGradBucket, broadcast_parameters, shard_episodes
    torch.manual_seed(rank)                                  # different init per rank ...
    net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Linear(5, 3))
    broadcast_parameters(net)                                # ... replicated from rank 0
    bucket = FlatGradBucket(net, skip_prefixes=("1.bias",), split_at="1.")  # one tensor left out; tail = layer 1 (overlapped)
    assert bucket.split == 6 * 5 + 5 and bucket._hook is not None
    xs = torch.arange(8 * 6, dtype=torch.float32).reshape(8, 6) / 10.0
    lo, hi = shard_episodes(8, rank, world)
    bucket.zero()
    net(xs[lo:hi]).square().sum().backward()
    skipped = net[1].bias.grad.clone()
    assert bucket._tail_work is not None                     # the hook fired during backward: tail all-reduce in flight
    bucket.allreduce()
    # by value (numpy): a torch tensor travels as a shared-memory handle the parent can no longer open once the worker is gone
    q.put((rank, lo, hi, bucket.flat.numpy().copy(), net[0].weight.detach().numpy().copy(), skipped.numpy().copy(), bucket.numel))
    dist.barrier()
    dist.destroy_process_group()


def test_gradient_bucket_allreduce_gloo_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + os.getpid() % 2000
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = sorted([q.get(timeout=120) for _ in range(2)], key=lambda t: t[0])
    [p.join(60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    res = [tuple(torch.from_numpy(v) if isinstance(v, np.ndarray) else v for v in t) for t in res]
    (r0, lo0, hi0, f0, w0, s0, n0), (r1, lo1, hi1, f1, w1, s1, n1) = res
    assert (lo0, hi0, lo1, hi1) == (0, 4, 4, 8)
    assert torch.equal(w0, w1)                               # broadcast replicated the weights
    assert torch.equal(f0, f1) and n0 == 6 * 5 + 5 + 5 * 3   # identical averaged gradients, bias of layer 1 left out
    # reference: single process over all 8 episodes, gradient / world
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Linear(5, 3))
    xs = torch.arange(8 * 6, dtype=torch.float32).reshape(8, 6) / 10.0
    net(xs).square().sum().backward()
    ref = torch.cat([net[0].weight.grad.flatten(), net[0].bias.grad.flatten(), net[1].weight.grad.flatten()]) / 2
    assert torch.allclose(f0, ref, rtol=1e-5, atol=1e-6)
    assert not torch.equal(s0, s1)                           # the skipped tensor was not exchanged


def _ddp_worker3(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from rpnet_amd.parallel import FlatGradBucket, broadcast_parameters, shard_episodes
    torch.manual_seed(rank)
    net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 4), torch.nn.Tanh(), torch.nn.Linear(4, 3))
    broadcast_parameters(net)
    bucket = FlatGradBucket(net, skip_prefixes=(), split_at=("2.", "4."))      # three segments: layer 0 | layer 2 | layer 4
    assert bucket.bounds == [0, 35, 59, 74] and len(bucket._hooks) == 2
    xs = torch.arange(8 * 6, dtype=torch.float32).reshape(8, 6) / 10.0
    lo, hi = shard_episodes(8, rank, world)
    bucket.zero()
    net(xs[lo:hi]).square().sum().backward()
    launched = sorted(bucket._work)                          # segments 2 and 1 went out during backward, 0 is left
    bucket.allreduce()
    first = bucket.flat.clone()
    # the graph-replay form of the step (rpnet_amd.graph.GraphedTrainStep under a process group): hooks suspended, nothing
    # goes out during backward, ONE collective over the whole bucket behind it — the same averaged gradients
    bucket.hooks_enabled = False
    bucket.zero()
    net(xs[lo:hi]).square().sum().backward()
    assert not bucket._work
    bucket.allreduce()
    bucket.hooks_enabled = True
    assert torch.equal(bucket.flat, first)
    q.put((rank, launched, first.numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_gradient_bucket_three_segments_gloo_world2():
    """progressive exchange: the segments behind the gradient front are all-reduced while backward still runs
    (hooks), the front segment after it; the averaged gradients equal the single-process ones"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_ddp_worker3, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = sorted([q.get(timeout=120) for _ in range(2)], key=lambda t: t[0])
    [p.join(60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    (_, l0, f0), (_, l1, f1) = [(r, l, torch.from_numpy(f)) for r, l, f in res]
    assert l0 == [1, 2] and l1 == [1, 2]
    assert torch.equal(f0, f1)
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 4), torch.nn.Tanh(), torch.nn.Linear(4, 3))
    xs = torch.arange(8 * 6, dtype=torch.float32).reshape(8, 6) / 10.0
    net(xs).square().sum().backward()
    ref = torch.cat([p.grad.flatten() for p in net.parameters()]) / 2
    assert torch.allclose(f0, ref, rtol=1e-5, atol=1e-6)


def test_shard_episodes_ragged():
    from rpnet_amd.parallel import shard_episodes
    spans = [shard_episodes(10, r, 4) for r in range(4)]
    assert spans == [(0, 3), (3, 6), (6, 8), (8, 10)]
    assert shard_episodes(0, 0, 2) == (0, 0)


def test_driver_import_closure():
    """Every non-torch symbol test_rpnet.py imports exists at the reference's import path
    (test_rpnet.py:11,14,15,28,30,32) and the synthetic reader honours the item contract."""
    import numpy as np
    from dataset.few_shot_reader import FewshotRegReader
    from net.model import model_factory  # noqa: F401
    from net.registration import MSE, NCC
    from utils.util import Logger, dice_score_seperate, load_yaml  # noqa: F401
    cfg, args = load_yaml(os.path.join(ROOT, "yamls", "example.yml"))
    assert args.net == "RP_Net" and cfg["soft_mask"] is False and cfg["mask_feature_map"] is False
    ds = FewshotRegReader("/nonexistent", cfg["eval_set_name"], cfg, mode="eval", n_volumes=2, n_slices=3, size=64)
    assert len(ds) == 2
    it = ds[1]
    for k in ("support_images", "support_labels", "warped_supp", "query_images", "query_labels", "appr_query_labels",
              "grid", "class_id", "pid", "supp_pids"):
        assert k in it, k
    assert it["support_images"][0][0].shape == (3, 1, 64, 64) and it["query_labels"].dtype == torch.int64
    c, i = it["supp_pids"][0]
    assert ds.fewshot_reader.fewshot_volume_reader.data_info[c][i]["pid"].startswith("synthetic")
    a = np.zeros((1, 4, 4)); a[0, :2] = 1
    assert dice_score_seperate(a, a, num_class=1) == [1.0] and dice_score_seperate(a, a * 0, num_class=1) == [None]
    x = torch.arange(16.0).reshape(4, 4)
    assert abs(NCC(x, x).item() + 1.0) < 1e-6 and MSE(x, x).item() == 0


def test_deferred_weight_gradient_queue_order():
    """the release queue of the asynchronous weight gradients (rpnet_amd.functional._defer_wgrad / _release_wgrads /
    join_side_streams): a launch goes out behind the dgrad `depth - 1` layers further down, oldest first, and whatever is
    still queued at the end of a backward pass (or before a bucket operation) is flushed by join_side_streams"""
    import rpnet_amd.functional as RF
    st = RF._ASYNC
    saved = (st["queued"], list(st["fifo"]), set(st["pending"]))
    try:
        st["queued"] = True            # as if the engine callback of this backward pass were registered already
        st["fifo"].clear()
        st["pending"].clear()
        for depth, want in ((1, ["L3", "L2", "L1"]), (2, ["L3", "L2", "L1"]), (3, ["L3", "L2", "L1"])):
            log, held = [], []
            st["queued"] = True        # (join_side_streams re-arms the registration at the end of every pass)
            for layer in ("L3", "L2", "L1"):                      # backward runs the layers top down
                RF._defer_wgrad(lambda n=layer: log.append(n))
                RF._release_wgrads(depth - 1)                      # ... right after that layer's dgrad is enqueued
                held.append(len(st["fifo"]))
            assert held == [min(i + 1, depth - 1) for i in range(3)], (depth, held)
            assert log == want[:3 - (depth - 1)] if depth > 1 else log == want
            RF.join_side_streams()                                 # end of backward: the rest, oldest first
            assert log == want and not st["fifo"]
        st["queued"] = True
        RF._defer_wgrad(lambda: log.append("late"))
        RF.reset_async()                                           # start of the next forward / a bucket operation: flushed too
        assert log[-1] == "late" and not st["fifo"] and st["queued"] is False
    finally:
        st["queued"] = saved[0]
        st["fifo"][:] = saved[1]
        st["pending"].clear()
        st["pending"].update(saved[2])


def test_gradient_bucket_forced_one_rank_group():
    """FlatGradBucket(force_active=True) in a process group of ONE rank (what tests/test_gpu_dist.py uses to put RCCL's stream
    semantics under the real step on a single GPU): hooks fire, segments go out, sum x 1/1 — the same bits as no exchange"""
    import torch.distributed as dist
    from rpnet_amd.parallel import FlatGradBucket
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(27500 + os.getpid() % 2000))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        torch.manual_seed(3)
        net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 4), torch.nn.Tanh(), torch.nn.Linear(4, 3))
        xs = torch.arange(8 * 6, dtype=torch.float32).reshape(8, 6) / 10.0
        bucket = FlatGradBucket(net, skip_prefixes=(), split_at=("2.", "4."), force_active=False)
        bucket.zero()
        net(xs).square().sum().backward()
        assert not bucket._work and bucket.allreduce() is None
        want = bucket.flat.clone()
        bucket.force_active = True
        bucket.zero()
        net(xs).square().sum().backward()
        assert sorted(bucket._work) == [1, 2]
        bucket.allreduce()
        assert torch.equal(bucket.flat, want) and float(want.abs().max()) > 0
    finally:
        dist.destroy_process_group()


def test_dma_kernels_not_chosen_beyond_their_32_bit_range():
    """The LDS-DMA convolution kernel addresses a source through one buffer descriptor with 32-bit offsets (all planes
    below 2 GiB); the tile policy (a host function: no GPU needed) must hand larger operands to the register-staged kernels
    instead of letting the offsets wrap — and keep choosing the DMA kernel below the limit."""
    import ctypes as C
    from rpnet_amd import hip
    lib = hip.load()

    def variant(N, H, W, cin, cout, planes, tune=0):
        d = hip.ConvDesc()
        d.N, d.H, d.W, d.C0, d.C1, d.Co0, d.Co1, d.taps, d.split_planes, d.groups, d.tune = N, H, W, cin, 0, cout, 0, 9, planes, 1, tune
        return lib.rpnet_conv_tile_variant(C.byref(d))

    assert variant(8, 256, 256, 128, 128, 2) == 11 and variant(8, 128, 128, 256, 256, 1) == 13     # the step's own layers
    assert variant(16, 512, 512, 64, 128, 2) == 11                  # two planes of 512 MiB: addressable
    assert variant(32, 512, 512, 64, 128, 2) == 7                   # two planes of 1 GiB = 2^31 bytes: the register-staged patch kernel
    # 64 images of 512^2 x 64 channels: two planes = 4 GiB, one plane = 2 GiB -> no DMA variant, forced or not
    for planes in (2, 1):
        for tune in (0, 12, 13, 14):
            assert variant(64, 512, 512, 64, 128, planes, tune) not in (11, 12, 13, 14), (planes, tune)


def test_reference_driver_launcher_reaches_the_model(tmp_path):
    """tools/run_reference_driver.py with this repository on the path: a driver script that masks the device
    (`os.environ['CUDA_VISIBLE_DEVICES'] = '1'` before `import torch`), imports tensorboard (absent here), loads
    yamls/example.yml, builds the reader and the model through model_factory and moves it to the device resolves every
    import to this repository and runs.  Without a GPU (RPNET_DRIVER_ALLOW_NO_GPU=1) it stops exactly at `net = net.cuda()`;
    where the launcher could initialise a GPU first, the device mask changes nothing and the move succeeds."""
    import subprocess
    import sys
    script = tmp_path / "driver.py"
    script.write_text(
        "import os\n"
        "os.environ['CUDA_VISIBLE_DEVICES'] = '1'\n"
        "import sys\n"
        "import torch\n"
        "from torch.utils.tensorboard import SummaryWriter\n"
        "from net.model import model_factory\n"
        "from dataset.few_shot_reader import FewshotRegReader\n"
        "from utils.util import load_yaml\n"
        "config, args = load_yaml(sys.argv[1])\n"
        "ds = FewshotRegReader(args.data_dir, args.eval_set_name, config, mode='eval')\n"
        "net = model_factory[args.net](pretrained_path=config['pretrained_path'], cfg={'align': True, 'backbone': 'UNet'},\n"
        "                              backbone_cfg=config)\n"
        "print('MODEL_BUILT', type(net).__name__)\n"
        "net = net.cuda()\n"
        "print('MODEL_ON_DEVICE', next(net.parameters()).device)\n")
    env = dict(os.environ, RPNET_DRIVER_ALLOW_NO_GPU="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_reference_driver.py"), str(script),
                        os.path.join(ROOT, "yamls", "example.yml")], capture_output=True, text=True, timeout=600, env=env,
                       cwd=str(tmp_path))
    assert "ModuleNotFoundError" not in r.stderr and "ImportError" not in r.stderr, r.stderr[-1500:]
    assert "MODEL_BUILT RP_Net" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
    if "hip runtime initialised before the script" in r.stderr:
        assert r.returncode == 0 and "MODEL_ON_DEVICE cuda" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
    else:
        assert r.returncode != 0 and "No HIP GPUs are available" in r.stderr, r.stderr[-1500:]
        assert "net = net.cuda()" in r.stderr and "MODEL_ON_DEVICE" not in r.stdout
    if "tensorboard" not in sys.modules and __import__("importlib").util.find_spec("tensorboard") is None:
        assert "no-op torch.utils.tensorboard.SummaryWriter registered" in r.stderr


def test_kept_alive_tensors_outlive_a_mid_backward_join():
    """The tensors an asynchronous weight gradient reads are kept alive in RF._ASYNC["keep"] until the side streams are joined at
    the END of the backward pass; the gradient bucket's hooks join in the middle of it (`final=False`): the calling stream waits,
    the list stays — a block freed there could be handed to another stream of the pass while a weight gradient still reads it."""
    import rpnet_amd.functional as RF
    saved = (list(RF._ASYNC["keep"]), set(RF._ASYNC["pending"]), RF._ASYNC["queued"])
    try:
        RF._ASYNC["keep"][:] = [object(), object()]
        RF._ASYNC["pending"].clear()
        RF._ASYNC["queued"] = True
        RF.join_side_streams(final=False)
        assert len(RF._ASYNC["keep"]) == 2 and RF._ASYNC["queued"] is True
        RF.join_side_streams()
        assert RF._ASYNC["keep"] == [] and RF._ASYNC["queued"] is False
    finally:
        RF._ASYNC["keep"][:] = saved[0]
        RF._ASYNC["pending"].update(saved[1])
        RF._ASYNC["queued"] = saved[2]
