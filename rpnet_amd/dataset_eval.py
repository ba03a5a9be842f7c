"""Evaluation of a data set with the items assembled on the device.

`DeviceEvalSource.item(idx)` reproduces `FewshotRegReader(mode="eval")[idx]` (rpnet_amd/utils/volume_reader.py) — the support
volume choice with the same consumption of the `random` generator, the k-block pairing of every query slice with a support slice,
the registration pre-step — but keeps the preprocessed volumes in HBM (the host reader decodes and preprocesses both NRRD volumes
for every item) and builds the item there: one table of S slice numbers goes up, ONE launch (`rpnet_eval_item_gather`,
csrc/evalitem.hip) writes the tensors the model takes and the two [0,1] planes the registration takes, and the registration
launches (rpnet_amd/registration.py) run without their copies to the host.  After `warm()` an item makes no device-to-host copy and
no host synchronisation.

`evaluate_dataset` walks the items: item -> `VolumeSegmenter(..., counts_out=table[j])` -> `rpnet_ncc_pairs` into `ncc[j]`.  The Dice
tallies of all items live in one int64 table and the image similarity figures in one fp64 table; both cross to the host ONCE, after
the last item, and the lines of tools/eval_driver.py:evaluate are printed from them.
"""
import os
import random
from collections import defaultdict

import numpy as np
import torch

from . import augment as A
from . import component_stats as CS
from . import components as CC
from . import morphology as MO
from . import postprocess as PP
from . import hip
from . import regions as RG
from . import registration as R
from . import surface as SF
from . import surface_spacing as SS
from .hip import call, ptr
from .utils.volume_reader import FewshotVolumeReader
from .volume import VolumeSegmenter, dice_from_counts


def eval_slice_table(n_support, n_query, k):
    """The pairing of FewshotSliceReader's eval branch (one shot) as a table: (k_effective, support_slice int32[n_query]) —
    query slice s is matched with support slice support_slice[s], the slice at the centre of the support volume's block j for every
    query slice of block j.  The numpy expressions are the host reader's own (`s_pick`, `q_edge`, `k = min(k, depths)`), so they round
    as it does.  For a few (depth, k) pairs `np.arange(0, nq, nq / k)` yields k + 1 block edges and the reader's loop over k blocks
    stops short of the last query slices (7 support / 17 query slices, k = 7: 14 of 17); the table then has as many entries as the
    loop pairs, and DeviceEvalSource refuses the item."""
    k = min([k, n_support, n_query])
    n = n_support
    s_pick = np.floor(np.arange(n / k / 2, n, n / k)).astype(np.int32)
    nq = n_query
    q_edge = np.floor(np.array(np.arange(0, nq, nq / k).tolist() + [nq])).astype(np.int32)
    counts = [int(q_edge[j + 1] - q_edge[j]) for j in range(k)]
    return k, np.repeat(s_pick[:k], counts).astype(np.int32)


def _volume(x, what):
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous float32 [D,H,W] tensor, got {x.dtype} {tuple(x.shape)}")
    return x


def eval_item_gather(s_img, s_msk, q_img, q_msk, support_slice):
    """One `rpnet_eval_item_gather` launch.  s_img, s_msk [Ds,H,W] and q_img, q_msk [S,H,W]: float32 volumes on the GPU;
    support_slice: S slice numbers in HOST memory (numpy or a CPU tensor), checked against [0, Ds) here, before the upload (the
    kernel cannot refuse a table it reads on the device).  Returns (support image, support label, query image, query label, support
    in [0,1], query in [0,1]), each [S,H,W]."""
    hip.require_gpu(s_img, s_msk, q_img, q_msk)
    s_img, s_msk, q_img, q_msk = (_volume(s_img, "support image"), _volume(s_msk, "support mask"), _volume(q_img, "query image"),
                                  _volume(q_msk, "query mask"))
    if s_img.shape != s_msk.shape or q_img.shape != q_msk.shape:
        raise ValueError(f"image and mask differ: support {tuple(s_img.shape)} / {tuple(s_msk.shape)}, query {tuple(q_img.shape)} / {tuple(q_msk.shape)}")
    if s_img.shape[1:] != q_img.shape[1:]:
        raise NotImplementedError(f"support {tuple(s_img.shape[1:])} and query {tuple(q_img.shape[1:])} slices differ in size")
    if torch.is_tensor(support_slice) and support_slice.is_cuda:
        raise TypeError("eval_item_gather: the slice table must be in host memory (it is checked before it is uploaded)")
    table = np.ascontiguousarray(np.asarray(support_slice), dtype=np.int32).reshape(-1)
    (Ds, H, W), S = s_img.shape, q_img.shape[0]
    if table.shape[0] != S:
        raise ValueError(f"eval_item_gather: {table.shape[0]} table entries for {S} query slices")
    if S and (int(table.min()) < 0 or int(table.max()) >= Ds):
        raise ValueError(f"eval_item_gather: slice table entries {int(table.min())} .. {int(table.max())} outside the support volume's [0, {Ds})")
    dev_table = A.upload(torch.from_numpy(table), q_img.device)
    outs = [torch.empty((S, H, W), device=q_img.device, dtype=torch.float32) for _ in range(6)]
    call("rpnet_eval_item_gather", ptr(s_img), ptr(s_msk), ptr(q_img), ptr(q_msk), ptr(dev_table), *[ptr(t) for t in outs], Ds, S, H, W)
    return tuple(outs)


def ncc_pairs(query, warped, affine, table, row):
    """table[row] = (NCC(query, warped), NCC(query, affine)) — net.registration.NCC over whole tensors, in fp64, bit-identical from run
    to run (csrc/evalitem.hip).  query, warped, affine: contiguous float32 GPU tensors of one element count; table: float64 [n,2] on
    the GPU.  Three launches, nothing copied."""
    hip.require_gpu(query, warped, affine, table)
    n = query.numel()
    for t, what in ((query, "query"), (warped, "warped"), (affine, "affine")):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise ValueError(f"ncc_pairs: {what} must be a contiguous float32 tensor of {n} elements, got {t.dtype} {tuple(t.shape)}")
    if table.dtype != torch.float64 or table.dim() != 2 or table.shape[1] != 2 or not table.is_contiguous():
        raise ValueError(f"ncc_pairs: the table must be a contiguous float64 [n,2] tensor, got {table.dtype} {tuple(table.shape)}")
    wb = hip.query("rpnet_ncc_pairs_workspace_bytes", n)
    ws = torch.empty((max(wb, 8),), device=query.device, dtype=torch.uint8)
    call("rpnet_ncc_pairs", ptr(query), ptr(warped), ptr(affine), n, ptr(table), int(row), table.shape[0], ptr(ws), wb)


class DeviceEvalSource:
    """config: the keys of FewshotVolumeReader / FewshotSliceReader (class_csv_dir, eval_classes, k, do_deformable, crop_size, ...);
    one way, one shot (`test_shot` 1), `use_registration_loss: True` and no `use_registration_mask` (what tools/eval_driver.py runs).
    cache_volumes=False reloads a volume every time it is used.  device_load=True builds a volume on the device from the payloads of its
    files (rpnet_amd.volume_load.DeviceVolumeLoader), the same bits as the host reader's.  `k` sticks across items, as in the host reader."""

    def __init__(self, data_dir, set_name, config, device, cache_volumes=True, device_load=False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceEvalSource runs on MI355X only (there is no CPU fallback; the host reader is "
                               "rpnet_amd.utils.volume_reader.FewshotRegReader)")
        if config["n_way"] != 1 or config["n_shot"] != 1:
            raise NotImplementedError("one way, one shot (the slice reader asserts one way)")
        if config.get("test_shot", config["n_shot"]) > 1:
            raise NotImplementedError("DeviceEvalSource pairs every query slice with ONE support slice: test_shot > 1 is not supported "
                                      "(the host reader rpnet_amd.utils.volume_reader.FewshotRegReader serves it)")
        if config.get("use_registration_mask", False):
            raise NotImplementedError("DeviceEvalSource does not build the mask channels of use_registration_mask "
                                      "(the host reader rpnet_amd.utils.volume_reader.FewshotRegReader serves them)")
        if not config.get("use_registration_loss", False):
            raise TypeError("DeviceEvalSource needs use_registration_loss: True, like FewshotRegReader")
        self.cfg, self.k = config, config["k"]
        self.reader = FewshotVolumeReader(data_dir, set_name, config, mode="eval")
        self.cache_volumes, self._volumes = cache_volumes, {}
        self.loader = None
        self.set_device_load(device_load)
        self.pre = None               # the last item's gathered tensors before registration and its slice table

    def __len__(self):
        return len(self.reader)

    def set_device_load(self, on):
        """volumes loaded from here on come from the device loader (True) or from the host reader (False); cached volumes stay, they
        hold the same bits either way"""
        if on and self.loader is None:
            from .volume_load import DeviceVolumeLoader
            self.loader = DeviceVolumeLoader(self.reader, self.device)
        elif not on:
            self.loader = None

    def volume(self, c, i):
        """(image [D,H,W], mask [D,H,W]) float32 on the device: the reader's deterministic preprocessing, once"""
        if (c, i) in self._volumes:
            return self._volumes[(c, i)]
        if self.loader is not None:
            v = self.loader.load(self.reader.data_info[c][i]["pid"], self.reader.classes[c])
        else:
            s = self.reader.load_image_and_mask(self.reader.data_info[c][i]["pid"], self.reader.classes[c])
            v = (torch.from_numpy(s["image"][0]).to(self.device), torch.from_numpy(s["mask"][0]).to(self.device))
        if self.cache_volumes:
            self._volumes[(c, i)] = v
        return v

    def warm(self):
        """load every volume and the small constants of the registration (its base grids and, with do_deformable, its smoothing
        kernel, or the DEEDS base grids with do_deformable "deeds"), so that no later item copies anything up with a blocking copy"""
        for c, i in self.reader.indices:
            img = self.volume(c, i)[0]
            R.base_grid(img.shape[2], img.device), R.base_grid(img.shape[1], img.device)
            if self.cfg.get("do_deformable", True) == "deeds":
                R.base_grid(128, img.device), R.base_grid(15, img.device)       # the keys deeds_register and deeds_warp look up
            elif self.cfg.get("do_deformable", True):
                R._device_kernel((2.0, 2.0), img.device)            # the key demons_register looks up

    def item(self, idx, support=None):
        """the item of query `idx`.  support: the index of the support volume inside the query's class instead of the drawn one; the draw
        is still made and then overridden, as FewshotVolumeReader.__getitem__(idx, supp_idx) does, so host and device stay in step"""
        rd, cfg = self.reader, self.cfg
        c, qv = rd.indices[idx]
        others = [i for i in range(rd.n_data[c]) if i != qv]
        (s,) = random.choices(others, k=1)                      # the one draw of the host item (eval mode has no elastic coin)
        if support is not None:
            if isinstance(support, bool) or not isinstance(support, (int, np.integer)) or not 0 <= int(support) < rd.n_data[c]:
                raise ValueError(f"DeviceEvalSource.item: support is the index of a volume of the class, 0..{rd.n_data[c] - 1}, got {support!r}")
            s = int(support)
        s_img, s_msk = self.volume(c, s)
        q_img, q_msk = self.volume(c, qv)
        if s_img.shape[1:] != q_img.shape[1:]:
            # make_support_query_same_size would pad here; load_image_and_mask leaves every volume at crop_size, so it never does
            raise NotImplementedError(f"support {tuple(s_img.shape[1:])} and query {tuple(q_img.shape[1:])} slices differ in size")
        self.k, table = eval_slice_table(s_img.shape[0], q_img.shape[0], self.k)       # k sticks for later items
        if table.shape[0] != q_img.shape[0]:
            raise ValueError(f"the reader's k-block loop pairs {table.shape[0]} of {q_img.shape[0]} query slices (support depth "
                             f"{s_img.shape[0]}, k = {self.k}): its block edges round to k + 1 blocks, and the host item is ragged too")
        sup, sup_l, q, lab, sup01, q01 = eval_item_gather(s_img, s_msk, q_img, q_msk, table)
        self.pre = {"support_images": sup[:, None], "support_labels": sup_l, "query_images": q[:, None], "query_labels": lab,
                    "support_slices": table}
        field, reg_pred, warped_src, aff_pred, aff_src = R.register_slices(sup01, q01, sup_l, do_deformable=cfg.get("do_deformable", True))
        # reg_pred is already 0 / 1 (thresholded at 0.1 by the warp): the host's `> 0.5` changes nothing
        return {"support_images": [[aff_src[:, None]]], "support_labels": [[aff_pred]], "query_images": q[:, None], "query_labels": lab,
                "appr_query_labels": reg_pred, "warped_supp": warped_src, "class_id": c, "pid": rd.data_info[c][qv]["pid"],
                "supp_pids": [(c, s)], "registration_field": field}


def item_spacings(source, n, spacing):
    """the spacing of each of the first n items: None, one triple for all, or "header": every item's from the NRRD header of its query
    volume (FewshotVolumeReader.volume_spacing), all read here, before any item is built"""
    if spacing is None:
        return [None] * n
    if isinstance(spacing, str):
        if spacing != "header":
            raise ValueError(f'evaluate_dataset: spacing is None, "header" or (sz, sy, sx), got {spacing!r}')
        rd = source.reader
        return [rd.volume_spacing(rd.data_info[c][qv]["pid"]) for c, qv in rd.indices[:n]]
    return [SS.check_spacing(spacing, "evaluate_dataset")] * n


def evaluate_dataset(net, source, config, n_items=None, batch=8, graphed=True, save_pred=None, out=None, surface=False, keep_largest=False,
                     spacing=None, surface_tolerance=None, fill_holes=False, hole_connectivity=None, max_hole=None, min_component=None,
                     opening=None, closing=None, morph_per_slice=False, device_load=None, keep_masks=False, regions=False,
                     components=False):
    """tools/eval_driver.py:evaluate over a DeviceEvalSource: the same printed lines (with both image similarity figures of
    test_rpnet.py:229-230: query against the fully warped and against the affine-warped support) and the same three dictionaries.
    The Dice tallies of all items are summed on the device into one int64 table [n_items, T+2, K-1, 3] and the NCC figures written into
    one fp64 table [n_items, 2]; both are copied to the host once, after the last item.  save_pred: a directory that receives every
    volume's mask as <pid>_<class>.nrrd (the masks stay on the device until the tables have crossed).  out: a dict that receives the
    host tables as out["counts"] and out["ncc"].  surface=True: two more device tables, int64 [n_items, 2, K-1, 6] and fp64
    [n_items, 2, K-1, 2], receive every volume's surface rows (rpnet_amd.surface: the final mask and the affine baseline against the
    labels) and cross with the others; every item line then ends with ` hd95 <fewshot> (<affine>) assd <fewshot> (<affine>)` (voxels,
    None where a border is empty), every class line with the means over the items where the figure is not None, and `out` receives
    out["surface_i"] and out["surface_f"].  keep_largest (False, True = 6, 6 or 26): every volume's final mask is also filtered to the
    largest connected component of its class (rpnet_amd.components); two more device tables, int64 [n_items, K-1, 3] (Dice counts of the
    filtered mask) and int64 [n_items, K-1, 4] (component statistics), and with surface=True an int64 [n_items, K-1, 6] and an fp64
    [n_items, K-1, 2] table (its surface rows), cross with the others; every item line then ends with
    ` lcc <dice> (<n_components> components, <removed> voxels removed)`, followed by ` lcc hd95 <v> assd <v>` under surface, every class
    line with their means; `out` receives out["post_counts"], out["components"] and, with surface, out["post_surface_i"] and
    out["post_surface_f"]; save_pred writes the filtered mask.  The three returned dictionaries are the same either way.
    spacing (with surface=True): None (everything above, every printed character included), (sz, sy, sx) for every item, or "header":
    every item's spacing from the header of its query volume, all headers read before the first item so that a volume without a spacing
    fails before any GPU work.  The surface tables then have the widths of rpnet_amd.surface_spacing (int64 [.., 5], fp64 [.., 5]) and
    arrive as out["surface_mm_i"], out["surface_mm_f"] (and out["post_surface_mm_i"], out["post_surface_mm_f"]), out["spacing"] holds
    the spacings used; the surface fields of every line are in millimetres and followed by `mm`.  surface_tolerance: the NSD tolerance
    in millimetres (needs a spacing); the lines then gain ` nsd <fewshot> (<affine>)`.
    fill_holes (False, True or "3d", "slice"), hole_connectivity, max_hole, min_component (voxels, or (mm3, "mm3") under a spacing, with
    "header" resolved per item; a spacing is then accepted without surface=True): the clean-up chain of VolumeSegmenter, remove small ->
    keep largest -> fill holes (rpnet_amd.postprocess).  One more device table, int64 [n_items, K-1, 8] (columns 0..3 the statistics row
    of fill_holes, 4..7 that of remove_small, zeros for a stage that is off), crosses with the others and arrives as out["post_stats"];
    the tables named under keep_largest then describe the end of the chain (out["components"] only with keep_largest); every item line
    gains ` holes <n> (<filled> voxels filled)` and ` small <n> (<removed> voxels removed)` for the stages that are on, after the lcc
    figures, every class line their means; save_pred writes the end of the chain.  With these options off nothing changes.
    opening, closing (None, a radius in voxels, ('rho', n), or (x, 'mm') under a spacing, with "header" resolved per item; a spacing is
    then accepted without surface=True), morph_per_slice: the ball morphology of VolumeSegmenter (rpnet_amd.morphology); the chain
    becomes open -> remove small -> keep largest -> close -> fill holes.  One more device table, int64 [n_items, K-1, 8] (columns 0..3
    the statistics row of the opening, 4..7 that of the closing, zeros for a stage that is off), is fetched once per data set and
    arrives as out["morph_stats"]; every item line gains ` open -<removed> +<added>` and ` close -<removed> +<added>` for the stages
    that are on, after the figures above, every class line their means.  With both None nothing changes.
    device_load (None: as the source was built; True / False): the source's volumes are built on the device from the payloads of their
    files (DeviceEvalSource.set_device_load); the tables and lines are the same either way.
    keep_masks=True: out["masks"] receives the list of every volume's final mask (uint8 [D,H,W] on the device, the end of the clean-up
    chain where one is on); nothing else changes.
    regions=True: the region statistics of VolumeSegmenter(regions=True) (rpnet_amd.regions): two more device tables, int64
    [n_items, 2, K, 20] and fp64 [n_items, 2, K, 2] (the final mask at the end of the chain, then the labels, with the query image), are
    fetched once with the others and arrive as out["regions_i"] and out["regions_f"].  A spacing (a triple or "header") is then accepted
    without surface=True (out["spacing"] holds the spacings used).  Every item line gains, after the fields above,
    ` vol <pred> (<truth>) rvd <x> cdist <x>` in voxels, under a spacing ` vol <pred> (<truth>) ml rvd <x> cdist <x> mm`; every class line
    the means over the items where the figure is not None.  With regions=False nothing changes.
    components=True | max_components: the per-component tables of VolumeSegmenter(components=...) (rpnet_amd.component_stats): two
    more device tables, int64 [n_items, 2, K-1, max_components, 24] and [n_items, 2, K-1, 4] (the final mask against the labels, then
    the labels against the final mask), are fetched once with the others and arrive as out["components_rows"] and
    out["components_head"].  A spacing is then accepted without surface=True.  Every item line gains, after the fields above,
    ` comp <Cp> (<Ct>) det <detected>/<Ct> fp <n> fpvol <voxels>`, under a spacing `fpvol <x> mL`: the components of the prediction
    (of the labels), the truth components the prediction overlaps, the predicted components that overlap no truth voxel and their
    volume; every class line the means.  With components=False nothing changes."""
    from .utils import nrrd
    from .volume import check_min_component
    if device_load is not None:
        source.set_device_load(bool(device_load))
    conn = CC.connectivity_of(keep_largest)
    holes_on, small_min = PP.holes_mode_of(fill_holes) is not None, check_min_component(min_component)
    small_on = small_min is not None
    open_r = None if opening is None else MO.check_radius(opening, "evaluate_dataset: opening")
    close_r = None if closing is None else MO.check_radius(closing, "evaluate_dataset: closing")
    morph_on = open_r is not None or close_r is not None
    morph_mm = any(r is not None and r[0] == "mm" for r in (open_r, close_r))
    if morph_mm and spacing is None:
        raise ValueError("evaluate_dataset: an opening or closing radius in mm needs a spacing (a triple or 'header')")
    chain = bool(conn) or holes_on or small_on or morph_on
    mm3 = isinstance(small_min, tuple) or morph_mm
    if isinstance(small_min, tuple) and spacing is None:
        raise ValueError("evaluate_dataset: min_component in mm3 needs a spacing (a triple or 'header')")
    classes = config["eval_classes"]
    n = len(source) if n_items is None else min(n_items, len(source))
    if ((spacing is not None and not mm3 and not regions and not components) or surface_tolerance is not None) and not surface:
        raise ValueError("evaluate_dataset: spacing and surface_tolerance act on the surface distances; give surface=True")
    if surface_tolerance is not None and spacing is None:
        raise ValueError("evaluate_dataset: surface_tolerance is a distance in millimetres; give spacing= as well")
    spacings = item_spacings(source, n, spacing)
    mm = spacing is not None
    WI, WF = (SS.IROW, SS.FROW) if mm else (SF.IROW, SF.FROW)
    seg = VolumeSegmenter(net, batch=batch, graphed=graphed, surface=surface, keep_largest=conn or False, surface_tolerance=surface_tolerance,
                          fill_holes=fill_holes, hole_connectivity=hole_connectivity, max_hole=max_hole, min_component=min_component,
                          **(dict(opening=opening, closing=closing, morph_per_slice=morph_per_slice) if morph_on else {}),
                          **(dict(regions=True) if regions else {}), **(dict(components=components) if components else {}))
    dev = next(net.parameters()).device
    T, K = net.num_iter, 2
    table = torch.zeros((n, T + 2, K - 1, 3), device=dev, dtype=torch.int64)
    ncc = torch.zeros((n, 2), device=dev, dtype=torch.float64)
    surf_i = torch.zeros((n, 2, K - 1, WI), device=dev, dtype=torch.int64) if surface else None
    surf_f = torch.zeros((n, 2, K - 1, WF), device=dev, dtype=torch.float64) if surface else None
    post_c = torch.zeros((n, K - 1, CC.COUNTS_ROW), device=dev, dtype=torch.int64) if chain else None
    post_s = torch.zeros((n, K - 1, CC.STATS_ROW), device=dev, dtype=torch.int64) if chain else None
    post_i = torch.zeros((n, K - 1, WI), device=dev, dtype=torch.int64) if chain and surface else None
    post_f = torch.zeros((n, K - 1, WF), device=dev, dtype=torch.float64) if chain and surface else None
    post_w = torch.zeros((n, K - 1, 2 * PP.STATS_ROW), device=dev, dtype=torch.int64) if holes_on or small_on else None
    post_m = torch.zeros((n, K - 1, 2 * MO.STATS_ROW), device=dev, dtype=torch.int64) if morph_on else None
    reg_i = torch.zeros((n, 2, K, RG.IROW), device=dev, dtype=torch.int64) if regions else None
    reg_f = torch.zeros((n, 2, K, RG.FROW), device=dev, dtype=torch.float64) if regions else None
    comp_n = CS.components_option(components)
    comp_rows = torch.zeros((n, 2, K - 1, comp_n, CS.COMP_ROW), device=dev, dtype=torch.int64) if comp_n else None
    comp_head = torch.zeros((n, 2, K - 1, CS.HEAD_WORDS), device=dev, dtype=torch.int64) if comp_n else None
    meta, masks = [], []
    for j in range(n):
        s = source.item(j)
        extra = {"surface_out": (surf_i[j], surf_f[j])} if surface else {}
        if mm:
            extra["spacing"] = spacings[j]
        if chain:
            extra["post_out"] = (post_c[j], post_s[j]) + (((post_i[j], post_f[j]),) if surface else ())
        if post_w is not None:
            extra["post_stats_out"] = post_w[j]
        if post_m is not None:
            extra["morph_stats_out"] = post_m[j]
        if regions:
            extra["regions_out"] = (reg_i[j], reg_f[j])
        if comp_n:
            extra["components_out"] = (comp_rows[j], comp_head[j])
        res = seg(s["support_images"], s["support_labels"], s["query_images"], s["appr_query_labels"], s["query_labels"], counts_out=table[j],
                  **extra)
        ncc_pairs(s["query_images"], s["warped_supp"], s["support_images"][0][0], ncc, j)
        meta.append((s["pid"], classes[s["class_id"]]))
        if save_pred or keep_masks:
            masks.append(res.post["mask"] if chain else res.mask)
    if keep_masks and out is not None:
        out["masks"] = masks
    counts, ncc = table.cpu().numpy(), ncc.cpu().numpy()          # the two transfers of the data set
    if out is not None:
        out["counts"], out["ncc"] = counts, ncc
    surf_few, surf_aff = defaultdict(list), defaultdict(list)
    if surface:
        surf_i, surf_f = surf_i.cpu().numpy(), surf_f.cpu().numpy()
        if out is not None:
            if mm:
                out["surface_mm_i"], out["surface_mm_f"], out["spacing"] = surf_i, surf_f, list(spacings)
            else:
                out["surface_i"], out["surface_f"] = surf_i, surf_f
    lcc_dice, lcc_fig, lcc_surf = defaultdict(list), defaultdict(list), defaultdict(list)
    holes_fig, small_fig = defaultdict(list), defaultdict(list)
    open_fig, close_fig = defaultdict(list), defaultdict(list)
    if chain:
        post_c, post_s = post_c.cpu().numpy(), post_s.cpu().numpy()
        if out is not None:
            out["post_counts"] = post_c
            if conn:
                out["components"] = post_s
        if post_w is not None:
            post_w = post_w.cpu().numpy()
            if out is not None:
                out["post_stats"] = post_w
        if post_m is not None:
            post_m = post_m.cpu().numpy()
            if out is not None:
                out["morph_stats"] = post_m
        if surface:
            post_i, post_f = post_i.cpu().numpy(), post_f.cpu().numpy()
            if out is not None:
                out["post_surface_mm_i" if mm else "post_surface_i"], out["post_surface_mm_f" if mm else "post_surface_f"] = post_i, post_f
    reg_fig = defaultdict(list)
    if regions:
        reg_i, reg_f = reg_i.cpu().numpy(), reg_f.cpu().numpy()
        if out is not None:
            out["regions_i"], out["regions_f"] = reg_i, reg_f
            if mm:
                out["spacing"] = list(spacings)
    comp_fig = defaultdict(list)
    if comp_n:
        comp_rows, comp_head = comp_rows.cpu().numpy(), comp_head.cpu().numpy()
        if out is not None:
            out["components_rows"], out["components_head"] = comp_rows, comp_head
            if mm:
                out["spacing"] = list(spacings)
    dsc_affine, dsc_fewshot, dsc_ref = defaultdict(list), defaultdict(list), defaultdict(lambda: defaultdict(list))
    if save_pred:
        os.makedirs(save_pred, exist_ok=True)
    for j, (pid, name) in enumerate(meta):
        d_aff, d_few = dice_from_counts(counts[j, T + 1])[0], dice_from_counts(counts[j, T])[0]
        dsc_affine[name].append(d_aff)
        dsc_fewshot[name].append(d_few)
        line = f"{j} {pid} affine ({ncc[j, 0]:.4f}, {ncc[j, 1]:.4f}) {d_aff}, fewshot {d_few}"
        for k in range(T):
            d = dice_from_counts(counts[j, k])[0]
            dsc_ref[name][k].append(d)
            line += f" ref {k} {d},"
        if surface:
            few, aff = (SS.spacing_figures(surf_i[j, :, 0], surf_f[j, :, 0], surface_tolerance) if mm
                        else SF.surface_figures(surf_i[j, :, 0], surf_f[j, :, 0]))
            surf_few[name].append(few)
            surf_aff[name].append(aff)
            line += SS.line_suffix_mm(few, aff, surface_tolerance is not None) if mm else SF.line_suffix(few, aff)
        if conn:
            d_lcc, fig = dice_from_counts(post_c[j])[0], CC.components_figures(post_s[j])[0]
            kept = None
            if surface:
                kept = SS.spacing_figures(post_i[j], post_f[j], surface_tolerance)[0] if mm else SF.surface_figures(post_i[j], post_f[j])[0]
            lcc_dice[name].append(d_lcc)
            lcc_fig[name].append(fig)
            lcc_surf[name].append(kept)
            line += CC.line_suffix(d_lcc, fig, kept, unit="mm" if mm else "")
        if post_w is not None:
            h = PP.holes_figures(post_w[j, :, :PP.STATS_ROW])[0] if holes_on else None
            sm = PP.small_figures(post_w[j, :, PP.STATS_ROW:])[0] if small_on else None
            holes_fig[name].append(h)
            small_fig[name].append(sm)
            line += PP.line_suffix(h, sm)
        if post_m is not None:
            op = MO.morph_figures(post_m[j, :, :MO.STATS_ROW])[0] if open_r is not None else None
            cl = MO.morph_figures(post_m[j, :, MO.STATS_ROW:])[0] if close_r is not None else None
            open_fig[name].append(op)
            close_fig[name].append(cl)
            line += MO.line_suffix(op, cl)
        if regions:
            fig = RG.region_figures(reg_i[j], reg_f[j], spacings[j])[0]
            reg_fig[name].append(fig)
            line += RG.region_line_suffix(fig, mm)
        if comp_n:
            fig = CS.detection_figures(comp_rows[j], comp_head[j], spacings[j])[0]
            comp_fig[name].append(fig)
            line += CS.detection_line_suffix(fig, mm)
        print(line)
        if save_pred:
            nrrd.write(os.path.join(save_pred, f"{pid}_{name}.nrrd"), masks[j].cpu().numpy(), encoding="gzip")
    for name in classes:
        if dsc_fewshot[name]:
            print(f"{name}, affine {np.mean(dsc_affine[name]):.4f}, fewshot {np.mean(dsc_fewshot[name]):.4f}"
                  + ((SS.mean_suffix_mm(surf_few[name], surf_aff[name], surface_tolerance is not None) if mm
                      else SF.mean_suffix(surf_few[name], surf_aff[name])) if surface else "")
                  + (CC.mean_suffix(lcc_dice[name], lcc_fig[name], lcc_surf[name] if surface else None, unit="mm" if mm else "") if conn else "")
                  + (PP.mean_suffix(holes_fig[name] if holes_on else None, small_fig[name] if small_on else None) if post_w is not None else "")
                  + (MO.mean_suffix(open_fig[name] if open_r is not None else None, close_fig[name] if close_r is not None else None)
                     if post_m is not None else "")
                  + (RG.region_mean_suffix(reg_fig[name], mm) if regions else "")
                  + (CS.detection_mean_suffix(comp_fig[name], mm) if comp_n else ""))
    return dsc_affine, dsc_fewshot, dsc_ref
