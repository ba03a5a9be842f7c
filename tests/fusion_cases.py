"""The numpy restatement of include/rpnet_fusion_abi.h (patterns, histogram, the three decision tables with the header's summation
order, masks and rows), an independent per-voxel EM, and the case tables of tests/test_host_fusion.py and tests/test_gpu_fusion.py.

Every float64 operation of the header is one numpy float64 operation here, in the header's order, so the device's tables are expected
to be EQUAL to these, bit for bit.  `defect` seeds one deliberate mistake (DEFECTS) so that the host test can show each would be seen.
"""
import numpy as np

VOTE, WEIGHTED, STAPLE = 0, 1, 2
METHODS = {"vote": VOTE, "weighted": WEIGHTED, "staple": STAPLE}
LO, HI = 2.0 ** -20, 1.0 - 2.0 ** -20
P0 = 0.99999
DEFECTS = ("bit_order", "gt_min_votes", "ge_weighted", "consensus_left_in", "prior_all_bins", "no_clamp", "pq_swapped", "merge_ignored")


def patterns_of(raters, cls, defect=None):
    """pat(i) = sum_r (rater_r[i] == cls) << r, uint16, in the shape of a rater"""
    R = len(raters)
    pat = np.zeros(np.asarray(raters[0]).shape, np.uint16)
    for r, v in enumerate(raters):
        bit = R - 1 - r if defect == "bit_order" else r
        pat |= ((np.asarray(v) == cls).astype(np.uint16) << np.uint16(bit)).astype(np.uint16)
    return pat


def histogram(pat, R):
    return np.bincount(pat.ravel().astype(np.int64), minlength=1 << R).astype(np.int64)


def bits_of(R):
    """[2^R, R] bool: bit r of p"""
    return ((np.arange(1 << R)[:, None] >> np.arange(R)[None, :]) & 1).astype(bool)


def block_sum(terms):
    """SUM of the header over the last axis (bins; 0.0 where a bin takes no part): thread t of 256 adds bins t, t + 256, ... in ascending
    order from 0.0, then a stride-halving tree over the 256 partials"""
    terms = np.asarray(terms, np.float64)
    nb = terms.shape[-1]
    K = (nb + 255) // 256
    padded = np.zeros(terms.shape[:-1] + (K * 256,), np.float64)
    padded[..., :nb] = terms
    padded = padded.reshape(terms.shape[:-1] + (K, 256))
    part = np.zeros(terms.shape[:-1] + (256,), np.float64)
    for k in range(K):
        part = part + padded[..., k, :]
    s = 128
    while s > 0:
        part = part[..., :s] + part[..., s:2 * s]
        s >>= 1
    return part[..., 0]


def vote_table(R, min_votes, defect=None):
    pc = bits_of(R).sum(1)
    label = pc > min_votes if defect == "gt_min_votes" else pc >= min_votes
    return label, pc.astype(np.float64) / np.float64(R)


def weighted_table(R, weights, defect=None):
    bits = bits_of(R)
    wts = np.asarray(weights, np.float64)
    s = np.zeros(1 << R, np.float64)
    for r in range(R):
        s = np.where(bits[:, r], s + wts[r], s)
    total = s[-1]
    label = 2.0 * s >= total if defect == "ge_weighted" else 2.0 * s > total
    return label, s / total


def staple_table(hist, R, consensus=True, max_iter=100, tol=1e-9, defect=None):
    """-> None where no EM runs (n == 0 or R == 1), else dict(label, w, p, q, iterations, converged, n, g)"""
    nb = 1 << R
    bits = bits_of(R)
    part = np.ones(nb, bool)
    if consensus and defect != "consensus_left_in":
        part[0] = part[nb - 1] = False
    h = np.asarray(hist, np.int64)
    n = int(h[part].sum())
    if n == 0 or R == 1:
        return None
    pc = bits.sum(1).astype(np.int64)
    if defect == "prior_all_bins":
        g = np.float64(int((h * pc).sum())) / np.float64(R * int(h.sum()))
    else:
        g = np.float64(int((h[part] * pc[part]).sum())) / np.float64(R * n)
    hd = h.astype(np.float64)
    p = np.full(R, P0, np.float64)
    q = np.full(R, P0, np.float64)
    w = np.zeros(nb, np.float64)
    iterations, converged = 0, 0
    for it in range(max_iter):
        pe, qe = (q, p) if defect == "pq_swapped" else (p, q)
        a = np.full(nb, g, np.float64)
        b = np.full(nb, np.float64(1.0) - g, np.float64)
        for r in range(R):
            a = a * np.where(bits[:, r], pe[r], np.float64(1.0) - pe[r])
            b = b * np.where(bits[:, r], np.float64(1.0) - qe[r], qe[r])
        w = np.where(part, a / (a + b), 0.0)
        hw = np.where(part, hd * w, 0.0)
        hv = np.where(part, hd * (np.float64(1.0) - w), 0.0)
        s1, s0 = block_sum(hw), block_sum(hv)
        P = block_sum(np.where(bits.T, hw[None, :], 0.0))
        Q = block_sum(np.where(bits.T, 0.0, hv[None, :]))
        clamp = (lambda v: v) if defect == "no_clamp" else (lambda v: np.minimum(np.maximum(v, LO), HI))
        pn = clamp(P / s1) if s1 != 0.0 else p.copy()
        qn = clamp(Q / s0) if s0 != 0.0 else q.copy()
        delta = max(np.abs(pn - p).max(), np.abs(qn - q).max())
        p, q = pn, qn
        iterations = it + 1
        converged = int(delta < tol)
        if converged:
            break
    label = w >= 0.5
    if consensus and defect != "consensus_left_in":
        label[0], label[nb - 1] = False, True
        w[0], w[nb - 1] = 0.0, 1.0
    return dict(label=label, w=w, p=p, q=q, iterations=iterations, converged=converged, n=n, g=g)


def decide(hist, R, method, min_votes=None, weights=None, consensus=True, max_iter=100, tol=1e-9, defect=None):
    """the decision kernel: dict(label uint8 [2^R], w float64 [2^R], stats int64 [6], rater_f float64 [R,2], rater_i int64 [R,3])"""
    nb = 1 << R
    h = np.asarray(hist, np.int64)
    bits = bits_of(R)
    voxels = int(h.sum())
    em = staple_table(h, R, consensus, max_iter, tol, defect) if method == STAPLE else None
    if em is not None:
        label, w, n, iterations, converged = em["label"], em["w"], em["n"], em["iterations"], em["converged"]
    else:
        if method == WEIGHTED:
            label, w = weighted_table(R, weights, defect)
        else:
            label, w = vote_table(R, R if method == STAPLE else (R // 2 + 1 if min_votes is None else min_votes), defect)
        iterations, converged = 0, 1
        n = voxels
        if method == STAPLE and consensus and defect != "consensus_left_in":
            n = voxels - int(h[0]) - (int(h[nb - 1]) if nb > 1 else 0)
    n_fused = int(h[label].sum())
    both = np.array([int(h[label & bits[:, r]].sum()) for r in range(R)], np.int64)
    mine = np.array([int(h[bits[:, r]].sum()) for r in range(R)], np.int64)
    rater_i = np.stack([both, mine, np.full(R, n_fused, np.int64)], 1)
    if em is not None:
        rater_f = np.stack([em["p"], em["q"]], 1)
    else:
        not_fused = voxels - n_fused
        neither = voxels - mine - n_fused + both
        sens = both.astype(np.float64) / np.float64(n_fused) if n_fused else np.ones(R)
        spec = neither.astype(np.float64) / np.float64(not_fused) if not_fused else np.ones(R)
        rater_f = np.stack([sens, spec], 1).astype(np.float64)
    stats = np.array([n, n_fused, int(h[nb - 1]), voxels - int(h[0]) - int(h[nb - 1]), iterations, converged], np.int64)
    return dict(label=label.astype(np.uint8), w=np.asarray(w, np.float64), stats=stats, rater_f=rater_f, rater_i=rater_i)


def dice_counts(mask, truth, cls):
    P, T = np.asarray(mask) == cls, np.asarray(truth) == cls
    return np.array([int((P & T).sum()), int(P.sum()), int(T.sum())], np.int64)


def fuse(raters, classes=(1,), method="vote", weights=None, min_votes=None, consensus=True, max_iter=100, tol=1e-9, truth=None, counts=None,
         out=None, defect=None):
    """rpnet_amd.fusion.fuse restated: one decision per class, the first written with merge = 0 and the others over 0 only ->
    dict(mask, prob, counts, stats, rater_f, rater_i, patterns, hist, label, w); patterns .. w are lists, one entry per class"""
    R = len(raters)
    shape = np.asarray(raters[0]).shape
    mask = np.zeros(shape, np.uint8) if out is None else np.array(out, np.uint8)
    res = dict(mask=mask, prob=None, counts=None if truth is None else (np.zeros((len(classes), 3), np.int64) if counts is None else
                                                                        np.array(counts, np.int64)),
               stats=[], rater_f=[], rater_i=[], patterns=[], hist=[], label=[], w=[])
    for k, cls in enumerate(classes):
        pat = patterns_of(raters, cls, defect)
        hist = histogram(pat, R)
        d = decide(hist, R, METHODS[method], min_votes, weights, consensus, max_iter, tol, defect)
        fused = d["label"][pat].astype(bool)
        if k == 0 or defect == "merge_ignored":
            mask[...] = np.where(fused, cls, 0)
        else:
            mask[...] = np.where((mask == 0) & fused, cls, mask)
        res["prob"] = d["w"][pat].astype(np.float32)
        if truth is not None:
            res["counts"][k] += dice_counts(mask, truth, cls)
        for key in ("stats", "rater_f", "rater_i", "label", "w"):
            res[key].append(d[key])
        res["patterns"].append(pat)
        res["hist"].append(hist)
    for key in ("stats", "rater_f", "rater_i"):
        res[key] = np.stack(res[key])
    return res


def per_voxel_em(raters, cls, iterations, consensus=True):
    """An independent STAPLE: no patterns, one weight per voxel, sums in np.longdouble in voxel order -> (p, q, w per voxel with NaN on
    the voxels that take no part).  The clamp is not applied: use it where the clamp is not reached."""
    D = np.stack([(np.asarray(v) == cls).ravel() for v in raters])       # [R, N]
    R = D.shape[0]
    votes = D.sum(0)
    use = (votes > 0) & (votes < R) if consensus else np.ones(D.shape[1], bool)
    Du = D[:, use]
    ld = np.longdouble
    g = ld(int(Du.sum())) / ld(R * Du.shape[1])
    p = np.full(R, ld(P0))
    q = np.full(R, ld(P0))
    w = np.zeros(Du.shape[1], ld)
    for _ in range(iterations):
        a = np.full(Du.shape[1], g, ld)
        b = np.full(Du.shape[1], ld(1) - g, ld)
        for r in range(R):
            a = a * np.where(Du[r], p[r], ld(1) - p[r])
            b = b * np.where(Du[r], ld(1) - q[r], q[r])
        w = a / (a + b)
        p = np.array([(w * Du[r]).sum(dtype=ld) / w.sum(dtype=ld) for r in range(R)], ld)
        q = np.array([((ld(1) - w) * ~Du[r]).sum(dtype=ld) / (ld(1) - w).sum(dtype=ld) for r in range(R)], ld)
    full = np.full(D.shape[1], np.nan, ld)
    full[use] = w
    return p, q, full


# ------------------------------------------------------------------------------------------------------------------- volumes
def blob(shape, seed=0):
    """a uint8 {0, 1} volume with one smooth object"""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, s) if s > 1 else np.zeros(1) for s in shape], indexing="ij")
    c = rng.uniform(-0.2, 0.2, 3)
    return (((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) < 0.45).astype(np.uint8)


def perturbed(truth, miss, add, seed):
    """a rater: every object voxel missed with probability `miss`, every background voxel marked with probability `add`"""
    rng = np.random.default_rng(seed)
    u = rng.random(truth.shape)
    return np.where(truth > 0, (u >= miss), (u < add)).astype(np.uint8)


def phantom(seed=7):
    """the 6 x 40 x 40 phantom: two raters at 2-3 % misses, three with 45 % independent misses -> (truth, raters)"""
    truth = blob((6, 40, 40), seed)
    rates = ((0.02, 0.002), (0.03, 0.002), (0.45, 0.002), (0.45, 0.002), (0.45, 0.002))
    return truth, [perturbed(truth, m, a, seed + 10 + i) for i, (m, a) in enumerate(rates)]


def raters_for(shape, R, seed=0, labels=1):
    """R raters of a volume of `shape` with classes 1..labels, of mixed quality -> (truth, raters) uint8"""
    rng = np.random.default_rng(seed)
    truth = blob(shape, seed)
    if labels > 1:
        truth = truth * rng.integers(1, labels + 1, size=shape).astype(np.uint8)
    out = []
    for r in range(R):
        flip = rng.random(shape) < (0.05 + 0.3 * (r % 3) / 2)
        other = rng.integers(0, labels + 1, size=shape).astype(np.uint8)
        out.append(np.where(flip, other, truth).astype(np.uint8))
    return truth, out


# the shapes of the GPU test: one voxel; a row that is no multiple of 16; each axis of length 1; a block's 4096 voxels + 1 and two
# blocks' + 2; a line of 1024 along x
SHAPES = [(1, 1, 1), (1, 1, 17), (1, 5, 7), (5, 1, 7), (5, 7, 1), (1, 17, 241), (2, 17, 241), (1, 1, 1024), (3, 9, 13)]
assert SHAPES[5][1] * SHAPES[5][2] == 4096 + 1 and 2 * 17 * 241 == 2 * 4096 + 2
# more voxels than 1024 blocks of 4096: the second trip of a block
TWO_TRIPS = (5, 1024, 1023)
RATER_COUNTS = (1, 2, 5, 12)
