"""Label fusion on the device: one mask from the masks R raters gave one volume (csrc/fusion.hip, include/rpnet_fusion_abi.h), and the
evaluation of a data set over several runs whose masks it fuses.

Definitions (the header states them operation by operation; tests/fusion_cases.py restates them in numpy with the same bits).
R raters, 1 <= R <= 12, volumes [D,H,W] of one element kind; d_r(i) = (rater_r[i] == cls); the pattern of a voxel is
pat(i) = sum_r d_r(i) << r; hist[p] counts the voxels of pattern p.  Every rule reads a voxel only through its pattern, so a call is two
passes over the volume (patterns and histogram; patterns to labels) around one block that fills a decision table label[p], w[p]:

  vote      label[p] = popcount(p) >= min_votes (default R // 2 + 1: an even split is background); w[p] = popcount(p) / R
  weighted  s[p] = the weights of the set bits added in ascending r; label[p] = 2 s[p] > total; w[p] = s[p] / total
  staple    binary STAPLE (Warfield, Zou, Wells 2004) on the histogram: the E step of a voxel depends on its pattern alone, so the
            per-voxel sums of the M step are sums over at most 4096 bins weighted by hist, which is exact, not an approximation.
            consensus=True leaves the all-background and the all-foreground bin out of the EM (label 0 / 1, w 0.0 / 1.0).

A statistics row is int64 {n_participating, n_fused, n_all_agree_fg, n_disagree, iterations, converged}; a rater_f row float64 [R, 2]
(p_r, q_r of the EM; sensitivity and specificity against the fused mask under vote and weighted); a rater_i row int64 [R, 3]
{|rater_r and fused|, |rater_r|, |fused|}; a counts row int64 {|P and T|, |P|, |T|} of the class in the result, ADDED to what the row
holds.  Integer atomics and separately rounded fp64 only: two runs give the same bits.

Limits: binary decisions, one class at a time (no joint confusion matrix over classes); at most 12 raters; extents up to 1024.
"""
import ctypes
import math
import os
from collections import defaultdict, namedtuple

import numpy as np
import torch

from . import hip
from ._volume_checks import KINDS, WorkspaceCache, check_table, check_volume, fmt, mean_of, one_device

MAX_RATERS = 12                      # RPNET_FUSION_MAX_RATERS
MAX_ITER = 100000                    # RPNET_FUSION_MAX_ITER
METHODS = {"vote": 0, "weighted": 1, "staple": 2}       # RPNET_FUSION_VOTE / WEIGHTED / STAPLE
STATS_ROW, COUNTS_ROW = 6, 3         # RPNET_FUSION_STATS_ROW, RPNET_FUSION_COUNTS_ROW
HEAD_BYTES = 64                      # RPNET_FUSION_HEAD_BYTES
_workspaces = WorkspaceCache(by_shape=True)

FusionResult = namedtuple("FusionResult", ["mask", "prob", "counts", "stats", "rater_f", "rater_i"])


def _check_raters(fn, raters):
    if not isinstance(raters, (list, tuple)) or not 1 <= len(raters) <= MAX_RATERS:
        raise ValueError(f"{fn}: raters must be a list of 1..{MAX_RATERS} volumes")
    if not all(torch.is_tensor(t) for t in raters):
        raise ValueError(f"{fn}: every rater must be a tensor")
    hip.require_gpu(*raters)
    for r, t in enumerate(raters):
        check_volume(t, f"rater {r}", fn)
        if t.dtype != raters[0].dtype or t.shape != raters[0].shape:
            raise ValueError(f"{fn}: rater {r} is {t.dtype} {tuple(t.shape)}, rater 0 is {raters[0].dtype} {tuple(raters[0].shape)}")
    one_device(fn, *raters, what="the raters")
    return (ctypes.c_void_p * len(raters))(*[t.data_ptr() for t in raters])


def _check_class(fn, cls):
    if isinstance(cls, bool) or not isinstance(cls, (int, np.integer)) or not 1 <= int(cls) <= 255:
        raise ValueError(f"{fn}: a class is an integer 1..255, got {cls!r}")
    return int(cls)


def _workspace_layout(R, n):
    """byte offsets of (hist, w, label, patterns) inside a workspace of a call with R raters on n voxels, and its size"""
    B = 1 << R
    up16 = lambda x: (x + 15) // 16 * 16  # noqa: E731
    return (HEAD_BYTES, HEAD_BYTES + 8 * B, HEAD_BYTES + 16 * B, HEAD_BYTES + 16 * B + up16(B)), HEAD_BYTES + 16 * B + up16(B) + up16(2 * n)


def _last_table(raters_shape, R, device):
    """(hist int64 [2^R], w float64 [2^R], label uint8 [2^R], patterns int16 [D,H,W]) that the last `fuse` call of this shape and rater count
    left in its workspace, as views of the workspace (the next such call overwrites them)"""
    D, H, W = (int(s) for s in raters_shape)
    ws, _ = _workspaces.get("rpnet_fusion_workspace_bytes", torch.device(device), (D, H, W, R))
    (o_h, o_w, o_l, o_p), _ = _workspace_layout(R, D * H * W)
    B = 1 << R
    return (ws[o_h:o_h + 8 * B].view(torch.int64), ws[o_w:o_w + 8 * B].view(torch.float64), ws[o_l:o_l + B],
            ws[o_p:o_p + 2 * D * H * W].view(torch.int16).view(D, H, W))


def pattern_histogram(raters, cls=1):
    """Pass 1 alone, one `rpnet_fusion_patterns` call on the current stream -> (patterns int16 [D,H,W] with values 0 .. 2^R - 1, bit r set
    where rater r holds `cls`; hist int64 [2^R]).  Launches only: nothing is copied or synchronised."""
    fn = "pattern_histogram"
    ptrs = _check_raters(fn, raters)
    cls = _check_class(fn, cls)
    D, H, W = raters[0].shape
    patterns = torch.empty((D, H, W), device=raters[0].device, dtype=torch.int16)
    hist = torch.empty((1 << len(raters),), device=raters[0].device, dtype=torch.int64)
    hip.call("rpnet_fusion_patterns", ptrs, len(raters), KINDS[raters[0].dtype], cls, D, H, W, hip.ptr(patterns), hip.ptr(hist))
    return patterns, hist


def fuse(raters, classes=(1,), method="vote", weights=None, min_votes=None, consensus=True, max_iter=100, tol=1e-9, truth=None, counts=None,
         out=None, prob=False, stats=None, rater_f=None, rater_i=None):
    """Fuse the masks of R raters, one `rpnet_fusion_fuse` call per class on the current stream ->
    FusionResult(mask uint8 [D,H,W], prob float32 [D,H,W] or None, counts int64 [len(classes), 3] or None, stats int64 [len(classes), 6],
    rater_f float64 [len(classes), R, 2], rater_i int64 [len(classes), R, 3]); row k belongs to classes[k].
    method: "vote" (min_votes, default R // 2 + 1), "weighted" (weights: R numbers, finite, >= 0, not all zero) or "staple" (consensus,
    max_iter, tol).  The first class is written over the whole of `out` (every other voxel 0), each later class only where the result
    so far is 0, the rule of resample_labels.  prob=True (or a contiguous float32 tensor of the raters' shape to write into): the plane
    w[pat] of the LAST class.  truth: the Dice counts of each class in
    the result are ADDED to counts (made of zeros when not handed in).  out, stats, rater_f, rater_i: tensors to write into.
    Launches only: nothing is copied or synchronised.  CPU tensors raise: there is no host route."""
    fn = "fuse"
    ptrs = _check_raters(fn, raters)
    R, dev = len(raters), raters[0].device
    if method not in METHODS:
        raise ValueError(f'{fn}: method is "vote", "weighted" or "staple", got {method!r}')
    classes = [_check_class(fn, c) for c in classes]
    if not classes:
        raise ValueError(f"{fn}: no class to fuse")
    if min_votes is None:
        min_votes = R // 2 + 1
    if isinstance(min_votes, bool) or not isinstance(min_votes, (int, np.integer)) or not 1 <= int(min_votes) <= R:
        raise ValueError(f"{fn}: min_votes is an integer 1..R = {R}, got {min_votes!r}")
    wts = None
    if method == "weighted":
        if weights is None or len(weights) != R:
            raise ValueError(f"{fn}: the weighted vote needs {R} weights")
        vals = [float(v) for v in weights]
        if not all(math.isfinite(v) and v >= 0 for v in vals) or not sum(vals) > 0 or not math.isfinite(sum(vals)):
            raise ValueError(f"{fn}: weights must be finite and >= 0 with a positive total, got {vals}")
        wts = (ctypes.c_double * R)(*vals)
    elif weights is not None:
        raise ValueError(f'{fn}: weights belong to method "weighted"')
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or not 1 <= int(max_iter) <= MAX_ITER:
        raise ValueError(f"{fn}: max_iter is an integer 1..{MAX_ITER}, got {max_iter!r}")
    if not isinstance(tol, (int, float, np.floating)) or isinstance(tol, bool) or not float(tol) >= 0:
        raise ValueError(f"{fn}: tol is a number >= 0, got {tol!r}")
    hip.require_gpu(truth, counts, out, stats, rater_f, rater_i)
    shape = raters[0].shape
    if truth is not None:
        check_volume(truth, "truth", fn)
        if truth.shape != shape:
            raise ValueError(f"{fn}: the raters {tuple(shape)} and truth {tuple(truth.shape)} differ in shape")
    elif counts is not None:
        raise ValueError(f"{fn}: counts need a truth volume (there is nothing to tally without the ground truth)")
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.uint8)
    elif not torch.is_tensor(out) or out.dtype != torch.uint8 or out.shape != shape or not out.is_contiguous():
        raise ValueError(f"{fn}: out must be a contiguous uint8 tensor of shape {tuple(shape)}")
    n_rows = len(classes)
    if stats is None:
        stats = torch.zeros((n_rows, STATS_ROW), device=dev, dtype=torch.int64)
    check_table(stats, n_rows, STATS_ROW, torch.int64, "stats", fn)
    if rater_f is None:
        rater_f = torch.zeros((n_rows, R, 2), device=dev, dtype=torch.float64)
    if rater_i is None:
        rater_i = torch.zeros((n_rows, R, 3), device=dev, dtype=torch.int64)
    for t, dt, w, what in ((rater_f, torch.float64, 2, "rater_f"), (rater_i, torch.int64, 3, "rater_i")):
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != (n_rows, R, w) or not t.is_contiguous():
            raise ValueError(f"{fn}: {what} must be a contiguous {str(dt)[6:]} [{n_rows}, {R}, {w}] tensor")
    if truth is not None:
        if counts is None:
            counts = torch.zeros((n_rows, COUNTS_ROW), device=dev, dtype=torch.int64)
        check_table(counts, n_rows, COUNTS_ROW, torch.int64, "counts", fn)
    one_device(fn, raters[0], truth, out, counts, stats, rater_f, rater_i)
    if torch.is_tensor(prob):
        hip.require_gpu(prob)
        if prob.dtype != torch.float32 or prob.shape != shape or not prob.is_contiguous() or prob.device != dev:
            raise ValueError(f"{fn}: prob must be True or a contiguous float32 tensor of shape {tuple(shape)} on the raters' device")
        plane = prob
    else:
        plane = torch.empty(shape, device=dev, dtype=torch.float32) if prob else None
    D, H, W = shape
    ws, nbytes = _workspaces.get("rpnet_fusion_workspace_bytes", dev, (D, H, W, R))
    for k, c in enumerate(classes):
        hip.call("rpnet_fusion_fuse", ptrs, R, KINDS[raters[0].dtype], c, D, H, W, METHODS[method], int(min_votes), wts, int(bool(consensus)),
                 int(max_iter), float(tol), hip.ptr(out), int(k > 0), hip.ptr(plane), hip.ptr(truth),
                 KINDS[truth.dtype] if truth is not None else 0, hip.ptr(counts), k, hip.ptr(stats), hip.ptr(rater_f), hip.ptr(rater_i), k, n_rows,
                 hip.ptr(ws), nbytes)
    return FusionResult(out, plane, counts, stats, rater_f, rater_i)


_fuse_masks = fuse      # evaluate_runs has an option of that name


def evaluate_runs(net, source, config, n_runs=None, fuse=None, consensus=True, n_items=None, batch=8, **evaluate_dataset_options):
    """The reference's evaluation over runs (test_rpnet.py:112-145): `n_runs` (default config["n_runs"], 1 without that key) consecutive
    `evaluate_dataset` calls, run-major, each drawing a fresh support volume per query from the `random` generator, so that under one seed
    run r prints and returns what the r-th of n_runs plain calls would; before each, the line `<r + 1> / <n_runs>`; after the last, the
    reference's "Average performance" block from the per-run tables (mean and spread over the runs of the per-run means).
    fuse (None, "vote" or "staple"): after the last run one `fuse` call per item over that item's n_runs final masks (the end of the
    clean-up chain where one is on), class by class, with the cached query mask as the truth; consensus is STAPLE's option.  The Dice
    counts go into one int64 table [n_items, K-1, 3], the statistics and rater rows into tables of their own, all fetched ONCE after the
    last item; then one line per item
        ` fused <dice> (runs <min> .. <max>, <n_disagree> voxels disputed, <iterations> iterations)`
    and per class the means.  Memory: n_runs x n_items masks (uint8 volumes) stay on the device until the call returns.
    -> (the per-run (dsc_affine, dsc_fewshot, dsc_ref) triples, the per-run `out` dictionaries, and a dict of the fused tables
    {"counts", "stats", "rater_f", "rater_i", "masks"} or None)."""
    from .dataset_eval import evaluate_dataset
    from .volume import dice_from_counts
    if n_runs is None:
        n_runs = config.get("n_runs", 1)
    if isinstance(n_runs, bool) or not isinstance(n_runs, (int, np.integer)) or n_runs < 1:
        raise ValueError(f"evaluate_runs: n_runs is an integer >= 1, got {n_runs!r}")
    if fuse not in (None, "vote", "staple"):
        raise ValueError(f'evaluate_runs: fuse is None, "vote" or "staple", got {fuse!r}')
    if fuse and n_runs > MAX_RATERS:
        raise ValueError(f"evaluate_runs: at most {MAX_RATERS} runs can be fused, got {n_runs}")
    for key in ("out", "keep_masks"):
        if key in evaluate_dataset_options:
            raise ValueError(f"evaluate_runs: {key} is set by evaluate_runs itself")
    classes = config["eval_classes"]
    results, outs = [], []
    for r in range(n_runs):
        print(f"{r + 1} / {n_runs}")
        out = {}
        results.append(evaluate_dataset(net, source, config, n_items, batch, out=out, keep_masks=bool(fuse), **evaluate_dataset_options))
        outs.append(out)
    aff, few, ref = defaultdict(list), defaultdict(list), defaultdict(lambda: defaultdict(list))
    for d_aff, d_few, d_ref in results:
        for k in classes:
            aff[k].append(d_aff[k])
            few[k].append(d_few[k])
            for it, rows in d_ref[k].items():
                ref[k][it].append(rows)
    ref_dsc = []
    print("=======Average performance=========")
    for k in classes:
        if not few[k] or not few[k][0]:
            continue
        a, f = np.array(aff[k]), np.array(few[k])
        print(f"{k}, affine {a.mean(1).mean()} + {a.mean(1).std()}, fewshot {f.mean(1).mean()} + {f.mean(1).std()}", end=" ")
        print()
        for it, rows in ref[k].items():
            rows = np.array(rows)
            ref_dsc.append(rows.mean(1).mean())
            print(f"ref {it} {rows.mean(1).mean()} + {rows.mean(1).std()}, ", end=" ")
        print()
    print(ref_dsc)
    if not fuse:
        return results, outs, None
    n = len(outs[0]["masks"])
    dev = outs[0]["masks"][0].device
    K = 2
    counts = torch.zeros((n, K - 1, COUNTS_ROW), device=dev, dtype=torch.int64)
    stats = torch.zeros((n, K - 1, STATS_ROW), device=dev, dtype=torch.int64)
    rater_f = torch.zeros((n, K - 1, n_runs, 2), device=dev, dtype=torch.float64)
    rater_i = torch.zeros((n, K - 1, n_runs, 3), device=dev, dtype=torch.int64)
    fused = []
    for j in range(n):
        c, qv = source.reader.indices[j]
        truth = source.volume(c, qv)[1]
        res = _fuse_masks([o["masks"][j] for o in outs], classes=tuple(range(1, K)), method=fuse, consensus=consensus, truth=truth,
                          counts=counts[j], stats=stats[j], rater_f=rater_f[j], rater_i=rater_i[j])
        fused.append(res.mask)
    tables = {"counts": counts.cpu().numpy(), "stats": stats.cpu().numpy(), "rater_f": rater_f.cpu().numpy(), "rater_i": rater_i.cpu().numpy(),
              "masks": fused}
    per_class = defaultdict(list)
    for j in range(n):
        c, qv = source.reader.indices[j]
        name = classes[c]
        d = dice_from_counts(tables["counts"][j])[0]
        runs = [res[1][name][len(per_class[name])] for res in results]
        per_class[name].append((d, runs))
        st = tables["stats"][j, 0]
        seen = [v for v in runs if v is not None]
        print(f"{j} {source.reader.data_info[c][qv]['pid']} fused {d} (runs {min(seen) if seen else None} .. {max(seen) if seen else None}, "
              f"{int(st[3])} voxels disputed, {int(st[4])} iterations)")
    for name in classes:
        if per_class[name]:
            print(f"{name}, fused {fmt(mean_of([d for d, _ in per_class[name]]))}, "
                  f"runs {fmt(mean_of([mean_of(rs) for _, rs in per_class[name]]))}")
    return results, outs, tables


def save_fused(tables, source, config, directory):
    """write every fused mask of `evaluate_runs` as <directory>/<pid>_<class>.nrrd (uint8, gzip), as evaluate_dataset(save_pred=) does"""
    from .utils import nrrd
    os.makedirs(directory, exist_ok=True)
    for j, mask in enumerate(tables["masks"]):
        c, qv = source.reader.indices[j]
        nrrd.write(os.path.join(directory, f"{source.reader.data_info[c][qv]['pid']}_{config['eval_classes'][c]}.nrrd"), mask.cpu().numpy(),
                   encoding="gzip")
