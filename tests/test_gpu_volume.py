"""rpnet_seg_tally (csrc/segtally.hip) and rpnet_amd.volume.VolumeSegmenter on the MI355X.

Counts are integers: the kernel-level bar is EQUALITY with what the driver computes on the host (`softmax(dim=1)[:, c] > 0.5`,
numpy sums).  Two correct fp32 softmax implementations can disagree only where 0 < l_c - (largest other logit) < 2^-22; every test
asserts on the host that its inputs have NO pixel in that band before it demands equality."""
import os

import numpy as np
import pytest
import torch

from tests.helpers import load_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 2.0 ** -22


def band_pixels(logits):
    """pixels of [N,K,H,W] logits where a foreground class leads the largest other logit by less than the band (K = 2: where two
    correct fp32 softmax implementations may disagree about `> 0.5`); K > 2: also where the float64 probability of a foreground
    class is within the band of 0.5"""
    l = np.asarray(logits, dtype=np.float64)
    K = l.shape[1]
    n = 0
    for c in range(1, K):
        other = np.delete(l, c, axis=1).max(axis=1)
        d = l[:, c] - other
        n += int(((d > 0) & (d < BAND)).sum())
        if K > 2:
            e = np.exp(l - l.max(axis=1, keepdims=True))
            p = e[:, c] / e.sum(axis=1)
            n += int((np.abs(p - 0.5) < BAND).sum())
    return n


def host_classes(src, kind, K):
    """the driver's predicate on the host: [N,H,W] class ids"""
    if kind == 1:
        return (np.asarray(src) > 0.5).astype(np.uint8)
    p = torch.from_numpy(np.asarray(src)).softmax(dim=1)
    cls = np.zeros(p.shape[:1] + p.shape[2:], dtype=np.uint8)
    for c in range(1, K):
        cls[(p[:, c] > 0.5).numpy()] = c
    return cls


def host_counts(sources, kinds, labels, n_valid, K):
    out = np.zeros((len(sources), K - 1, 3), dtype=np.int64)
    for s, (src, kind) in enumerate(zip(sources, kinds)):
        cls = host_classes(src, kind, K)[:n_valid]
        for c in range(1, K):
            P, T = cls == c, labels[:n_valid] == c
            out[s, c - 1] = [(P & T).sum(), P.sum(), T.sum()]
    return out


def run_tally(sources, kinds, labels, n_valid, K, want_counts=True, want_mask=True, mask_src=0, counts=None, mask_fill=7):
    from rpnet_amd.volume import seg_tally
    srcs = [torch.from_numpy(np.ascontiguousarray(s)).to(DEV) for s in sources]
    N, (H, W) = srcs[0].shape[0], srcs[0].shape[-2:]
    lab = torch.from_numpy(labels.astype(np.int32)).to(DEV) if want_counts else None
    if want_counts and counts is None:
        counts = torch.zeros((len(srcs), K - 1, 3), device=DEV, dtype=torch.int64)
    mask = torch.full((N, H, W), mask_fill, device=DEV, dtype=torch.uint8) if want_mask else None
    nv = torch.tensor([n_valid], device=DEV, dtype=torch.int32)
    seg_tally(srcs, kinds, nv, lab, counts if want_counts else None, mask, mask_src=mask_src, K=K)
    torch.cuda.synchronize()
    return counts, mask


def seeded_labels(seed, N, H, W, K):
    return np.random.RandomState(seed).randint(0, K, size=(N, H, W)).astype(np.int64)


@pytest.mark.parametrize("tag", ["m64_eval", "m128_train"])
def test_tally_of_the_reference_logits_is_exact(golden, tag):
    """the reference's own `output` / `refinement_*` tensors against a seeded synthetic mask: all counts and the mask equal the
    host's, after the host has shown that no pixel lies in the band"""
    g = golden(tag)
    names = sorted(k for k in g if k.startswith("refinement_")) + ["output"]
    sources = [g[k] for k in names]
    N, K, H, W = sources[0].shape
    assert K == 2 and sum(band_pixels(s) for s in sources) == 0
    labels = seeded_labels(11, N, H, W, K)
    kinds = [0] * len(sources)
    counts, mask = run_tally(sources, kinds, labels, N, K, mask_src=len(sources) - 1)
    want = host_counts(sources, kinds, labels, N, K)
    print(tag, "counts", counts.cpu().numpy().tolist())
    assert want[:, :, 1].min() > 0, "the fixture predicts foreground somewhere"
    assert np.array_equal(counts.cpu().numpy(), want)
    assert np.array_equal(mask.cpu().numpy(), host_classes(sources[-1], 0, K))


def test_exact_ties_are_background():
    """l0 == l1 gives softmax 0.5 exactly, and 0.5 > 0.5 is false in the reference"""
    rs = np.random.RandomState(5)
    l0 = (rs.standard_normal((1, 32, 32)) * 7).astype(np.float32)
    l1 = l0.copy()
    l1[:, :, 16:] += 1.0                       # right half: class 1 by a wide margin; left half: exact ties
    logits = np.stack([l0, l1], 1)
    assert band_pixels(logits) == 0
    labels = np.ones((1, 32, 32), dtype=np.int64)
    counts, mask = run_tally([logits], [0], labels, 1, 2)
    assert counts.cpu().numpy().tolist() == [[[512, 512, 1024]]]
    assert mask[:, :, :16].sum().item() == 0 and (mask[:, :, 16:] == 1).all()
    assert np.array_equal(mask.cpu().numpy(), host_classes(logits, 0, 2))


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("n_valid", [0, 1, 3])
def test_tally_random_logits_odd_extents(K, n_valid):
    """seeded random logits, extents that are no powers of two, a kind-1 source beside two logit sources, n_valid of 0, 1, N;
    counts only / mask only; two launches accumulate; two runs are bit-identical"""
    N, H, W = 3, 48, 80
    rs = np.random.RandomState(100 + K)
    sources = [(rs.standard_normal((N, K, H, W)) * 3).astype(np.float32) for _ in range(2)]
    sources.append((rs.rand(N, H, W) < 0.4).astype(np.float32))
    kinds = [0, 0, 1]
    assert sum(band_pixels(s) for s in sources[:2]) == 0
    labels = seeded_labels(200 + K, N, H, W, K)
    want = host_counts(sources, kinds, labels, n_valid, K)
    want_mask = np.full((N, H, W), 7, dtype=np.uint8)                 # images n >= n_valid keep what the buffer held
    want_mask[:n_valid] = host_classes(sources[1], 0, K)[:n_valid]
    counts, mask = run_tally(sources, kinds, labels, n_valid, K, mask_src=1)
    assert np.array_equal(counts.cpu().numpy(), want)
    assert np.array_equal(mask.cpu().numpy(), want_mask)
    if n_valid:
        assert want[:2, :, 0].min() > 0                               # every class of every logit source is met
    # the kind-1 source as the mask source; no labels (mask only)
    none, mask1 = run_tally(sources, kinds, labels, n_valid, K, want_counts=False, mask_src=2)
    assert none is None
    want_mask[:n_valid] = host_classes(sources[2], 1, K)[:n_valid]
    assert np.array_equal(mask1.cpu().numpy(), want_mask)
    # no mask (counts only), twice into the same table: the sum
    c2, none = run_tally(sources, kinds, labels, n_valid, K, want_mask=False)
    c2, none = run_tally(sources, kinds, labels, n_valid, K, want_mask=False, counts=c2)
    assert none is None and np.array_equal(c2.cpu().numpy(), 2 * want)
    # bit-identical runs
    again, mask_again = run_tally(sources, kinds, labels, n_valid, K, mask_src=1)
    assert torch.equal(again, counts) and torch.equal(mask_again, mask)


def test_tally_error_returns():
    from rpnet_amd import hip
    from rpnet_amd.volume import seg_tally
    nv = torch.ones(1, device=DEV, dtype=torch.int32)

    def z(*shape, dtype=torch.float32):
        return torch.zeros(shape, device=DEV, dtype=dtype)
    with pytest.raises(RuntimeError, match="K=5"):
        seg_tally([z(1, 5, 16, 16)], [0], nv, mask=z(1, 16, 16, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="multiple of 16"):
        seg_tally([z(1, 2, 16, 24)], [0], nv, mask=z(1, 16, 24, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="counts and labels come together"):
        seg_tally([z(1, 2, 16, 16)], [0], nv, counts=z(1, 1, 3, dtype=torch.int64), mask=z(1, 16, 16, dtype=torch.uint8))
    # N == 0 and H * W == 0: success without a launch
    seg_tally([z(0, 2, 16, 16)], [0], nv, mask=z(0, 16, 16, dtype=torch.uint8))
    seg_tally([z(2, 2, 0, 16)], [0], nv, mask=z(2, 0, 16, dtype=torch.uint8))
    torch.cuda.synchronize()
    assert hip.load().rpnet_last_error_string().decode().startswith("seg_tally: counts and labels")


def test_captured_launch_follows_n_valid():
    """n_valid is read on the device: one launch captured with torch.cuda.graph and replayed after n_valid changed gives the
    changed tallies and mask (the ragged last batch of a volume replays the graph of the full ones)"""
    from rpnet_amd.volume import seg_tally
    N, K, H, W = 4, 2, 32, 48
    rs = np.random.RandomState(9)
    logits = (rs.standard_normal((N, K, H, W)) * 3).astype(np.float32)
    assert band_pixels(logits) == 0
    labels = seeded_labels(10, N, H, W, K)
    src, lab = torch.from_numpy(logits).to(DEV), torch.from_numpy(labels.astype(np.int32)).to(DEV)
    counts = torch.zeros((1, K - 1, 3), device=DEV, dtype=torch.int64)
    mask = torch.zeros((N, H, W), device=DEV, dtype=torch.uint8)
    nv = torch.tensor([N], device=DEV, dtype=torch.int32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        seg_tally([src], [0], nv, lab, counts, mask)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        seg_tally([src], [0], nv, lab, counts, mask)
    for n_valid in (N, 1, 3):
        counts.zero_()
        mask.fill_(9)
        nv.fill_(n_valid)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), host_counts([logits], [0], labels, n_valid, K)), n_valid
        assert np.array_equal(mask[:n_valid].cpu().numpy(), host_classes(logits, 0, K)[:n_valid])
        assert (mask[n_valid:] == 9).all()


# ------------------------------------------------------------------------------------------------ end to end

def build_net(cfg):
    from rpnet_amd.modules import RP_Net
    from rpnet_amd.utils.seeding import seed_module_
    net = RP_Net(cfg={"align": True, "backbone": "UNet"}, backbone_cfg=cfg).to(DEV)
    seed_module_(net)
    return net.eval()


def eval_cfg():
    cfg = load_cfg()
    cfg["n_iter_refinement"] = cfg["n_test_iter_refinement"]
    return cfg


def reader(cfg, n_slices, size, n_volumes=2):
    from dataset.few_shot_reader import FewshotRegReader
    return FewshotRegReader("/nonexistent", cfg["eval_set_name"], cfg, mode="eval", n_volumes=n_volumes, n_slices=n_slices, size=size)


class Recorder:
    """hands `tools.eval_driver.evaluate` the net and keeps every call's logits (on the host)"""

    def __init__(self, net):
        self.net, self.outs = net, []

    def eval(self):
        self.net.eval()
        return self

    def __call__(self, *a, **kw):
        out = self.net(*a, **kw)
        self.outs.append({"output": out["output"].cpu().numpy(), **{k: v.cpu().numpy() for k, v in out["refinement"].items()}})
        return out


def segment(seg, item):
    return seg(item["support_images"], item["support_labels"], item["query_images"], item["appr_query_labels"], item["query_labels"])


def driver_run(cfg, item_source):
    """the parent's host loop (batch 2, eager) on a freshly seeded net: Dice values and the logits of every call"""
    from tools.eval_driver import evaluate
    rec = Recorder(build_net(cfg))
    aff, few, ref = evaluate(rec, item_source, cfg, n_items=1)
    dice = {"affine": [aff["Liver"][0]], "fewshot": [few["Liver"][0]], "refinement": {k: [v[0]] for k, v in ref["Liver"].items()}}
    return dice, rec.outs


def dice_delta(a, b):
    rows = [(a["fewshot"], b["fewshot"]), (a["affine"], b["affine"])] + [(a["refinement"][k], b["refinement"][k]) for k in a["refinement"]]
    return max(abs(x - y) for ra, rb in rows for x, y in zip(ra, rb))


class OneItem:
    """a reader that serves one prepared item (the registration pre-step of the synthetic reader runs once per test)"""

    def __init__(self, item):
        self.item = item

    def __len__(self):
        return 1

    def __getitem__(self, i):
        return self.item


@pytest.mark.parametrize("size,n_slices", [(64, 6), (256, 5)])
def test_volume_segmenter_equals_the_driver(size, n_slices):
    """batch 2, eager: the same calls as tools.eval_driver.evaluate on a net of the same seed (each run on a fresh net, so that
    both start without an fp16 scale history), hence the same logits — the rounded Dice values are EQUAL and the mask equals the
    host-thresholded output.  Then batch 8 through the captured graph against that run: |dDice| <= 1e-3 per iteration."""
    from rpnet_amd.volume import VolumeSegmenter
    cfg = eval_cfg()
    item = reader(cfg, n_slices, size)[0]
    want, outs = driver_run(cfg, OneItem(item))
    logits = np.concatenate([o["output"] for o in outs], 0)
    assert sum(band_pixels(v) for o in outs for v in o.values()) == 0
    res = segment(VolumeSegmenter(build_net(cfg), batch=2, graphed=False), item)
    print("driver", want, "\non-device", res.dice)
    assert res.counts.shape == (12, 1, 3) and res.mask.shape == (n_slices, size, size) and res.mask.dtype == torch.uint8
    assert res.dice == want
    assert np.array_equal(res.mask.cpu().numpy(), host_classes(logits, 0, 2))
    assert res.dice["fewshot"] == res.dice["refinement"][9]                      # output == refinement[T-1]
    gt = item["query_labels"].numpy()
    assert res.counts[:, 0, 2].tolist() == [int((gt == 1).sum())] * 12
    # batch 8, graphed: per-call fp16 tensor scales move the logits at the 1e-6 level
    res8 = segment(VolumeSegmenter(build_net(cfg), batch=8, graphed=True), item)
    print("batch 8 graphed", res8.dice, "differing mask pixels:", int((res8.mask != res.mask).sum().item()))
    assert dice_delta(res8.dice, res.dice) <= 1e-3
    # without labels: the mask alone
    bare = VolumeSegmenter(build_net(cfg), batch=2, graphed=False)(item["support_images"], item["support_labels"], item["query_images"],
                                                                   item["appr_query_labels"])
    assert bare.counts is None and bare.dice is None and torch.equal(bare.mask, res.mask)


def test_volume_segmenter_f32_batch_and_tail():
    """f32 conv math: eval-mode BatchNorm makes the samples independent and no per-call tensor scale exists, so the masks of batch 8
    graphed equal those of batch 2 eager, and S = 5 at batch 4 (one filler-padded tail call) equals S = 5 at batch 5, exactly"""
    import rpnet_amd.functional as RF
    from rpnet_amd.volume import VolumeSegmenter, graphed_eval
    RF.set_conv_math("f32")              # restored by tests/conftest.py
    cfg = eval_cfg()
    item = reader(cfg, 5, 64)[0]
    net = build_net(cfg)
    eager = segment(VolumeSegmenter(net, batch=2, graphed=False), item)
    seg8 = VolumeSegmenter(net, batch=8, graphed=True)
    g8 = segment(seg8, item)
    assert torch.equal(g8.mask, eager.mask) and np.array_equal(g8.counts, eager.counts)
    seg4, seg5 = VolumeSegmenter(net, batch=4, graphed=True), VolumeSegmenter(net, batch=5, graphed=True)
    b4, b5 = segment(seg4, item), segment(seg5, item)
    assert torch.equal(b4.mask, b5.mask) and np.array_equal(b4.counts, b5.counts) and b4.dice == b5.dice
    assert np.array_equal(b4.counts, eager.counts)
    # the segmenters of one net share ONE GraphedEval (a second wrapper would clear the weight packs the first one's graphs hold):
    # the graph captured first still serves after the later captures
    assert seg8._graphed_eval is seg4._graphed_eval is seg5._graphed_eval is graphed_eval(net)
    assert len(graphed_eval(net)._graphs) == 3
    again = segment(seg8, item)
    assert torch.equal(again.mask, g8.mask) and np.array_equal(again.counts, g8.counts)


def test_tallies_follow_the_redo_of_a_graphed_call():
    """fp16 planes forced on; a first volume gives the captured graph its predicted scales, a second one with images far beyond
    the prediction margin makes GraphedEval redo the call eagerly (the ordinary recovery path of the eval call): the tallies come
    from the redo's outputs, not from the stale static ones — they equal those of graphed=False on that volume within the Dice bar"""
    import rpnet_amd.functional as RF
    import rpnet_amd.modules as RM
    from rpnet_amd.volume import VolumeSegmenter
    RM._F16_MIN_PIXELS = 0               # restored by tests/conftest.py
    cfg = eval_cfg()
    item = reader(cfg, 4, 128)[0]
    big = dict(item)
    scale = 64.0 * RF.PRED_SAFETY
    big["query_images"] = item["query_images"] * scale
    big["support_images"] = [[x * scale for x in way] for way in item["support_images"]]
    seg = VolumeSegmenter(build_net(cfg), batch=2, graphed=True)
    first = segment(seg, item)
    assert RF.pred_stats()["predicted_calls"] > 0
    before = RF.pred_stats()["violations"]
    second = segment(seg, big)
    assert RF.pred_stats()["violations"] > before, "the second volume did not make GraphedEval redo a call"
    want = segment(VolumeSegmenter(build_net(cfg), batch=2, graphed=False), big)
    print("redo", second.dice, "\neager", want.dice, "\nfirst volume", first.dice)
    assert dice_delta(second.dice, want.dice) <= 1e-3
    assert np.array_equal(second.counts[:, 0, 2], want.counts[:, 0, 2])


def test_save_pred_writes_the_mask(tmp_path):
    from rpnet_amd.utils import nrrd
    from rpnet_amd.volume import VolumeSegmenter
    from tools.eval_driver import evaluate_on_device
    cfg = eval_cfg()
    item = reader(cfg, 3, 64)[0]
    aff, few, ref = evaluate_on_device(build_net(cfg), OneItem(item), cfg, batch_size=2, save_pred=str(tmp_path), graphed=False)
    res = segment(VolumeSegmenter(build_net(cfg), batch=2, graphed=False), item)
    data, header = nrrd.read(os.path.join(str(tmp_path), f"{item['pid']}_Liver.nrrd"))
    assert data.dtype == np.uint8 and header["encoding"] == "gzip"
    assert np.array_equal(data, res.mask.cpu().numpy())
    assert few["Liver"] == res.dice["fewshot"] and aff["Liver"] == res.dice["affine"]
    assert sorted(ref["Liver"].keys()) == list(range(10))
