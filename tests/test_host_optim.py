"""The host side of the Adam step over the flat gradient bucket: the chunk table of rpnet_adam_plan against a numpy restatement, its
refusals, and the Python plumbing that needs no GPU (the library loads on a CPU box; the plan makes no GPU call and dereferences
nothing, so made-up addresses serve)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rpnet_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 4096                                     # RPNET_ADAM_CHUNK of include/rpnet_optim_abi.h
ENTRY = np.dtype([("param", "<u8"), ("flat_start", "<i8"), ("count", "<i4"), ("vec16", "<i4")])      # struct rpnet_adam_chunk
LISTS = [[1, 3, 5, 64, 4096, 4097, 8193], [64, 576, 12288], [1], [6151, 7]]
BASE = 0x7F0000000000


def _offsets(counts):
    return [int(v) for v in np.concatenate([[0], np.cumsum(counts)[:-1]])]


def _plan(ptrs, counts, offsets, table_bytes=None):
    """-> (status, table as ENTRY records or None, error string)"""
    lib = hip.load()
    n = len(counts)
    a_cnt, a_off = (C.c_int64 * n)(*counts), (C.c_int64 * n)(*offsets)
    a_ptr = (C.c_void_p * n)(*ptrs)
    need = lib.rpnet_adam_plan_bytes(a_cnt, n)
    buf = np.zeros(max(need if table_bytes is None else table_bytes, 1), dtype=np.uint8)
    k = C.c_int64(-1)
    rc = lib.rpnet_adam_plan(a_ptr, a_cnt, a_off, n, buf.ctypes.data, buf.size if table_bytes is None else table_bytes, C.byref(k))
    err = lib.rpnet_last_error_string().decode()
    if rc != 0:
        return rc, None, err
    assert k.value * ENTRY.itemsize == need
    return rc, buf[:need].view(ENTRY), err


def _numpy_plan(ptrs, counts, offsets):
    rows = []
    for ptr, k, o in zip(ptrs, counts, offsets):
        for done in range(0, k, CHUNK):
            p, s = ptr + 4 * done, o + done
            rows.append((p, s, min(CHUNK, k - done), int(s % 4 == 0 and p % 16 == 0)))
    return np.array(rows, dtype=ENTRY)


@pytest.mark.parametrize("counts", LISTS)
@pytest.mark.parametrize("ptr_phase", [0, 4])
def test_plan_matches_numpy_and_covers_every_element_once(counts, ptr_phase):
    offsets = _offsets(counts)
    ptrs, at = [], BASE + ptr_phase
    for k in counts:
        ptrs.append(at)
        at += (k + 3) // 4 * 16 + 64
    assert ENTRY.itemsize == 24
    rc, table, _ = _plan(ptrs, counts, offsets)
    assert rc == 0
    want = _numpy_plan(ptrs, counts, offsets)
    assert len(table) == len(want)
    for f in ENTRY.names:
        assert np.array_equal(table[f], want[f]), f
    # every element of every parameter exactly once, no chunk across two parameters
    seen_flat = np.zeros(sum(counts), dtype=np.int32)
    for e in table:
        assert 1 <= e["count"] <= CHUNK
        owner = [i for i, (o, k) in enumerate(zip(offsets, counts)) if o <= e["flat_start"] < o + k]
        assert len(owner) == 1
        i = owner[0]
        assert e["flat_start"] + e["count"] <= offsets[i] + counts[i]
        assert int(e["param"]) - ptrs[i] == 4 * (int(e["flat_start"]) - offsets[i])          # the pointer advanced to the chunk
        seen_flat[e["flat_start"]:e["flat_start"] + e["count"]] += 1
        assert bool(e["vec16"]) == (e["flat_start"] % 4 == 0 and int(e["param"]) % 16 == 0)
    assert (seen_flat == 1).all()
    if ptr_phase:
        assert not table["vec16"].any()
    elif counts == LISTS[1]:
        assert table["vec16"].all()


def test_plan_with_gaps_between_parameters():
    """offsets ascend and do not overlap; they need not be dense"""
    rc, table, _ = _plan([BASE, BASE + 4096], [10, 5000], [8, 100])
    assert rc == 0 and list(table["flat_start"]) == [8, 100, 100 + CHUNK] and list(table["count"]) == [10, CHUNK, 5000 - CHUNK]


@pytest.mark.parametrize("what, ptrs, counts, offsets, table_bytes", [
    ("null pointer", [BASE, 0], [4, 4], [0, 4], None),
    ("pointer not 4-byte aligned", [BASE + 2], [4], [0], None),
    ("count 0", [BASE, BASE + 64], [4, 0], [0, 4], None),
    ("count negative", [BASE], [-3], [0], None),
    ("offsets descend", [BASE, BASE + 64], [4, 4], [8, 0], None),
    ("offsets overlap", [BASE, BASE + 64], [8, 4], [0, 7], None),
    ("negative first offset", [BASE], [4], [-4], None),
    ("total 2^40", [BASE, BASE + 64], [4, 4], [0, (1 << 40) - 4], None),
    ("count 2^40", [BASE], [1 << 40], [0], None),
    ("buffer too small", [BASE], [CHUNK + 1], [0], 24),
])
def test_plan_refusals(what, ptrs, counts, offsets, table_bytes):
    _plan([BASE], [4], [0])                                   # a success in front: the error string below is this call's
    rc, table, err = _plan(ptrs, counts, offsets, table_bytes)
    assert rc != 0 and table is None, what
    assert err.startswith("adam_plan") and len(err) > 15, (what, err)


def test_plan_bytes_refusals():
    lib = hip.load()
    assert lib.rpnet_adam_plan_bytes((C.c_int64 * 2)(CHUNK, CHUNK + 1), 2) == 3 * 24
    assert lib.rpnet_adam_plan_bytes((C.c_int64 * 1)(0), 1) == 0 and lib.rpnet_last_error_string().decode().startswith("adam_plan")
    assert lib.rpnet_adam_plan_bytes(None, 1) == 0
    assert lib.rpnet_adam_plan_bytes((C.c_int64 * 1)(4), 0) == 0
    assert lib.rpnet_optim_abi_version() == hip.OPTIM_ABI_VERSION == 1


def test_fused_adam_on_a_cpu_bucket_raises():
    from rpnet_amd.optim import FusedAdam
    from rpnet_amd.parallel import FlatGradBucket
    net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Linear(5, 3))
    bucket = FlatGradBucket(net, skip_prefixes=(), split_at=())
    with pytest.raises(RuntimeError, match="CPU tensor"):
        FusedAdam(bucket, lr=1e-3)
    assert bucket.mean_scale == 1.0                              # no process group: the sum is the mean


def test_driver_lists_the_optimizer_option():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train_rpnet.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "--optimizer" in out.stdout and "fused" in out.stdout and "torch" in out.stdout
    import inspect
    from train_rpnet import train
    assert inspect.signature(train).parameters["optimizer"].default == "torch"


def _sum_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from rpnet_amd.parallel import FlatGradBucket, broadcast_parameters, shard_episodes
    torch.manual_seed(rank)
    net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Linear(5, 3))
    broadcast_parameters(net)
    bucket = FlatGradBucket(net, skip_prefixes=("1.bias",), split_at="1.")
    xs = torch.arange(8 * 6, dtype=torch.float32).reshape(8, 6) / 10.0
    lo, hi = shard_episodes(8, rank, world)
    out = []
    for average in (False, True):
        bucket.zero()
        net(xs[lo:hi]).square().sum().backward()
        if average:
            bucket.allreduce()                                   # the default call, as every existing caller makes it
        else:
            bucket.allreduce(average=False)
        out.append(bucket.flat.numpy().copy())
    assert bucket.mean_scale == 0.5                              # what the default call multiplied by, for the consumer of the sum
    q.put((rank, out[0], out[1]))
    dist.barrier()
    dist.destroy_process_group()


def test_allreduce_sum_and_mean_gloo_world2():
    """allreduce(average=False) leaves the SUM over the ranks in the bucket; the default call leaves today's mean"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + os.getpid() % 2000
    procs = [ctx.Process(target=_sum_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = sorted([q.get(timeout=120) for _ in range(2)], key=lambda t: t[0])
    [p.join(60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    (_, s0, m0), (_, s1, m1) = res
    assert np.array_equal(s0, s1) and np.array_equal(m0, m1)
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Linear(5, 3))
    xs = torch.arange(8 * 6, dtype=torch.float32).reshape(8, 6) / 10.0
    net(xs).square().sum().backward()
    total = torch.cat([net[0].weight.grad.flatten(), net[0].bias.grad.flatten(), net[1].weight.grad.flatten()]).numpy()
    assert np.allclose(s0, total, rtol=1e-5, atol=1e-6)                 # the sum over the two shards = the whole batch
    assert np.allclose(m0, total / 2, rtol=1e-5, atol=1e-6)
    assert np.array_equal(m0, s0 * np.float32(0.5))                     # the mean is the sum times 1 / world, bit for bit
