"""Segment a whole volume on the device: predicted masks and the Dice tallies of every refinement iteration.

The reference's driver (test_rpnet.py:151-258, restated in tools/eval_driver.py:evaluate) walks a volume in 2-slice calls and, per
call, runs T + 1 softmax launches, T + 1 index launches and T + 1 blocking `.cpu()` copies, then thresholds and counts in numpy —
and throws the segmentation away.  `VolumeSegmenter` runs the same model calls (`batch` slices at a time, through
`rpnet_amd.graph.GraphedEval` where it applies) and follows each with ONE launch (`rpnet_seg_tally`, csrc/segtally.hip) that
thresholds every refinement iteration's logits, the output and the affine baseline, adds their |P and T|, |P|, |T| to a counter
table in device memory and writes the predicted mask.  The counters cross to the host once per volume; the mask stays on the
device until it is asked for.
"""
import ctypes as C
import weakref
from collections import namedtuple

import numpy as np
import torch

from . import component_stats as CS
from . import components as CC
from . import hip
from . import morphology as MO
from . import postprocess as PP
from . import regions as RG
from . import surface as SF
from . import surface_spacing as SS
from .graph import GraphedEval


class VolumeResult(namedtuple("VolumeResult", ["mask", "counts", "dice"])):
    """(mask, counts, dice) of a volume; `surface` beside them: None, or the surface distances of VolumeSegmenter(surface=True);
    `post`: None, or what VolumeSegmenter(keep_largest=...) measured on the mask filtered to its largest components; `regions`: None, or
    the region statistics of VolumeSegmenter(regions=True); `components`: None, or the per-component tables of
    VolumeSegmenter(components=...)"""
    surface = None
    post = None
    regions = None
    components = None


# One GraphedEval per net, shared by every VolumeSegmenter of that net.  A captured graph holds the addresses of the net's weight
# packs, and a second `GraphedEval(net)` clears that cache (graph.py:__init__): the first wrapper's graphs would then replay on
# freed memory.  One wrapper serves every shape (one graph per shape).
_GRAPHED = weakref.WeakKeyDictionary()


def graphed_eval(net):
    """the GraphedEval that the VolumeSegmenters of `net` share (made on first use)"""
    ge = _GRAPHED.get(net)
    if ge is None:
        ge = _GRAPHED[net] = GraphedEval(net)
    return ge


def dice_from_counts(counts, decimal=4):
    """[K-1][3] rows {|P and T|, |P|, |T|} -> per-class Dice 2|P and T| / (|P| + |T|), None for a class absent from the ground
    truth, rounded as `utils.util.dice_score_seperate` rounds (the numbers the driver prints)."""
    scores = []
    for inter, p, t in ((int(r[0]), int(r[1]), int(r[2])) for r in counts):
        scores.append(round(float(2 * inter / float(t + p)), decimal) if t else None)
    return scores


def seg_tally(sources, kinds, n_valid, labels=None, counts=None, mask=None, mask_src=0, K=None, _table=None):
    """One `rpnet_seg_tally` launch on the current stream.  sources: fp32 tensors, logits [N,K,H,W] (kind 0) or 0/1 masks [N,H,W]
    (kind 1); n_valid: int32 device scalar; labels int32 [N,H,W]; counts int64 [S,K-1,3] (accumulated into); mask uint8 [N,H,W]."""
    first = sources[0]
    if kinds[0] == 0:
        N, Kk, H, W = first.shape
    else:
        (N, H, W), Kk = first.shape, K
    K = Kk if K is None else K
    hip.require_gpu(*sources, labels, counts, mask, n_valid)
    for t, kind in zip(sources, kinds):
        want = (N, K, H, W) if kind == 0 else (N, H, W)
        if tuple(t.shape) != want or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"seg_tally: a source of kind {kind} must be a contiguous fp32 tensor of shape {want}, got {tuple(t.shape)} {t.dtype}")
    for t, dt, shape, what in ((labels, torch.int32, (N, H, W), "labels"), (mask, torch.uint8, (N, H, W), "mask"),
                               (counts, torch.int64, (len(sources), K - 1, 3), "counts"), (n_valid, torch.int32, None, "n_valid")):
        if t is not None and (t.dtype != dt or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape)):
            raise ValueError(f"seg_tally: {what} must be a contiguous {dt} tensor" + (f" of shape {shape}" if shape else ""))
    S = len(sources)
    if _table is None:
        _table = ((C.c_void_p * S)(*[t.data_ptr() for t in sources]), (C.c_int32 * S)(*kinds))
    hip.call("rpnet_seg_tally", _table[0], _table[1], S, hip.ptr(labels), hip.ptr(n_valid), hip.ptr(counts), hip.ptr(mask),
             mask_src, N, K, H, W)


def surface_widths(spacing):
    """(columns of an int64 surface row, columns of an fp64 one): those of rpnet_amd.surface, or of rpnet_amd.surface_spacing under a
    spacing"""
    return (SF.IROW, SF.FROW) if spacing is None else (SS.IROW, SS.FROW)


def check_surface_out(surface_out, K, spacing=None):
    """the tables of surface rows a caller hands to VolumeSegmenter: (int64 [2, K-1, 6], float64 [2, K-1, 2]), under a spacing (int64
    [2, K-1, 5], float64 [2, K-1, 5]), both contiguous: rows of the final mask, then of the affine baseline, per foreground class"""
    wi, wf = surface_widths(spacing)
    ok = isinstance(surface_out, (tuple, list)) and len(surface_out) == 2 and all(torch.is_tensor(t) and t.is_contiguous() for t in surface_out)
    if ok:
        it, ft = surface_out
        ok = (it.dtype == torch.int64 and tuple(it.shape) == (2, K - 1, wi) and ft.dtype == torch.float64
              and tuple(ft.shape) == (2, K - 1, wf))
    if not ok:
        under = "" if spacing is None else " (the widths under a spacing: rpnet_amd.surface_spacing)"
        raise ValueError(f"surface_out must be a pair of contiguous tensors (int64 [2, {K - 1}, {wi}], float64 [2, {K - 1}, {wf}]){under}: "
                         "the rows of the final mask and of the affine baseline per foreground class")


def check_post_out(post_out, K, surface, spacing=None):
    """the tables a caller hands to VolumeSegmenter(keep_largest=...): (counts int64 [K-1, 3], stats int64 [K-1, 4]) and, with
    surface=True, a third member (int64 [K-1, 6], float64 [K-1, 2]), under a spacing (int64 [K-1, 5], float64 [K-1, 5]); all
    contiguous: one row per foreground class of the filtered mask"""
    wi, wf = surface_widths(spacing)
    want = 3 if surface else 2
    ok = isinstance(post_out, (tuple, list)) and len(post_out) == want and all(torch.is_tensor(t) and t.is_contiguous() for t in post_out[:2])
    if ok:
        counts, stats = post_out[:2]
        ok = (counts.dtype == torch.int64 and tuple(counts.shape) == (K - 1, CC.COUNTS_ROW) and stats.dtype == torch.int64
              and tuple(stats.shape) == (K - 1, CC.STATS_ROW))
    if ok and surface:
        pair = post_out[2]
        ok = isinstance(pair, (tuple, list)) and len(pair) == 2 and all(torch.is_tensor(t) and t.is_contiguous() for t in pair)
        ok = ok and (pair[0].dtype == torch.int64 and tuple(pair[0].shape) == (K - 1, wi) and pair[1].dtype == torch.float64
                     and tuple(pair[1].shape) == (K - 1, wf))
    if not ok:
        raise ValueError(f"post_out must be contiguous tensors (int64 [{K - 1}, {CC.COUNTS_ROW}], int64 [{K - 1}, {CC.STATS_ROW}]"
                         + (f", (int64 [{K - 1}, {wi}], float64 [{K - 1}, {wf}])" if surface else "")
                         + (" (the widths under a spacing)" if surface and spacing is not None else "")
                         + "): the Dice counts, the component statistics" + (" and the surface rows" if surface else "")
                         + " of the filtered mask per foreground class")


def check_counts_out(counts_out, K, T=None):
    """the tally table a caller hands to VolumeSegmenter: a contiguous int64 tensor [T+2, K-1, 3] (T is checked where it is known)"""
    if not torch.is_tensor(counts_out) or counts_out.dtype != torch.int64 or not counts_out.is_contiguous():
        raise ValueError("counts_out must be a contiguous int64 tensor [T+2, K-1, 3]")
    if counts_out.dim() != 3 or tuple(counts_out.shape[1:]) != (K - 1, 3) or (T is not None and counts_out.shape[0] != T + 2):
        rows = "T+2" if T is None else str(T + 2)
        raise ValueError(f"counts_out must have the shape [{rows}, {K - 1}, 3] (refinement 0 .. T-1, output, affine baseline), "
                         f"got {tuple(counts_out.shape)}")


def check_min_component(min_component):
    """the `min_component` option -> None (off), an int (voxels, at least 1) or (mm3, 'mm3'), resolved under a call's spacing"""
    if min_component is None or min_component is False:
        return None
    if isinstance(min_component, (tuple, list)) and len(min_component) == 2 and min_component[1] == "mm3":
        v = float(min_component[0])
        if not (v >= 0 and np.isfinite(v)):
            raise ValueError(f"min_component: the volume in mm3 must be a finite number >= 0, got {min_component[0]!r}")
        return (v, "mm3")
    if isinstance(min_component, (int, np.integer)) and not isinstance(min_component, bool) and int(min_component) >= 1:
        return int(min_component)
    raise ValueError(f"min_component must be None, a number of voxels >= 1 or (mm3, 'mm3'), got {min_component!r}")


class VolumeSegmenter:
    """`VolumeSegmenter(net, batch=8, graphed=True, surface=False, keep_largest=False, spacing=None, surface_tolerance=None)(
    support_images, support_fg, query_images, appr_query_labels, query_labels=None, counts_out=None, surface_out=None, post_out=None,
    spacing=None)` -> VolumeResult(mask, counts, dice).

    Arguments are the volume-level tensors of a `FewshotRegReader` eval item: nested lists `[way][shot]` of support images
    [S,1,H,W] and foreground masks [S,H,W] (background = 1 - foreground), query images [S,1,H,W], the approximate (affine) labels
    [S,H,W] and, optionally, the ground truth [S,H,W].
      mask    uint8 [S,H,W] on the device: the class predicted by the final output
      counts  int64 [T+2, K-1, 3] on the host, rows = refinement 0 .. T-1, output, affine baseline; columns |P and T|, |P|, |T|
      dice    {'fewshot': [..], 'affine': [..], 'refinement': {i: [..]}} per class, as the driver prints them
    (counts and dice are None without query_labels.)  The slices go through the model `batch` at a time in eval mode under
    no_grad; the last batch is filled by repeating the last slice, and the device scalar `n_valid` keeps the filler out of the
    tallies and the mask.  graphed and 1-way 1-shot: the calls go through GraphedEval — `graphed=True`: the one wrapper all
    VolumeSegmenters of this net share (`graphed_eval(net)`), or pass your own `GraphedEval(net)` to use that; a net must not get a
    second wrapper while graphs of the first are in use (graph.py clears the net's weight packs) — otherwise eager `net(...)`.  The
    only device-to-host transfer this class adds is the counter table, once per volume.
      counts_out  an int64 tensor [T+2, K-1, 3] on the net's device (needs query_labels): the tallies are ADDED to it, nothing crosses
                  to the host, and `counts` and `dice` of the result are None — for a caller that keeps the tables of many volumes
                  on the device and fetches them once (rpnet_amd.dataset_eval.evaluate_dataset).
      surface=True  (needs query_labels to do anything) the completed volume gets two surface tallies per foreground class
                  (rpnet_amd.surface.surface_tally): the final mask against the labels and appr_query_labels against the labels.  The
                  result's `surface` is {'fewshot': [..], 'affine': [..]}, per class a dict {'hd95', 'hd', 'assd'} in voxels (None
                  where a border is empty); the two small tables cross to the host once per volume.  Nothing else changes: mask,
                  counts and dice are those of surface=False.
      surface_out (int64 [2, K-1, 6], float64 [2, K-1, 2]) on the net's device (needs surface=True and query_labels): the rows are
                  written there, nothing crosses to the host for them and the result's `surface` is None.
      spacing     None (the integer path above, untouched), or (sz, sy, sx): the voxel spacing of the axes [S, H, W], here or per call
                  (a call's spacing wins).  With surface=True the tallies are rpnet_amd.surface_spacing.surface_tally_spacing: the
                  figures are {'hd95', 'hd', 'assd', 'nsd'} in the unit of the spacing (millimetres), surface_out and the third
                  member of post_out take the widths of that module (int64 [.., 5], float64 [.., 5]), and the final mask, the affine
                  baseline and the filtered mask all go through it.
      surface_tolerance  the NSD tolerance in the unit of the spacing (None: 'nsd' is None); needs a spacing.
      keep_largest  False, True (connectivity 6), 6 or 26: once the volume is complete, every foreground class of the final mask is
                  filtered to its largest connected component (rpnet_amd.components.keep_largest) into a SECOND uint8 volume.  mask,
                  counts, dice and surface of the result stay those of keep_largest=False; the result's `post` is a dict:
                    'mask'        uint8 [S,H,W] on the device: the filtered mask
                    'counts'      int64 [K-1, 3] on the host, |P and T|, |P|, |T| of the filtered classes (None without query_labels)
                    'dice'        per class, dice_from_counts of those (None without query_labels)
                    'components'  per class {'n_components', 'kept', 'removed'} (voxels)
                    'surface'     with surface=True and query_labels: per class {'hd95', 'hd', 'assd'} of the filtered mask against
                                  the labels (one more surface_tally per class), else None
                  The small tables cross to the host once per volume.
      post_out    (counts int64 [K-1, 3], stats int64 [K-1, 4]) and, with surface=True, a third member (int64 [K-1, 6],
                  float64 [K-1, 2]) on the net's device (needs keep_largest and query_labels): the counts are ADDED and the other rows
                  written there, nothing crosses to the host and every entry of `post` but 'mask' is None.
      fill_holes  False, True or '3d' (the holes of the volume), 'slice' (every slice on its own): the holes of every foreground class
                  are filled (rpnet_amd.postprocess.fill_holes; with the one foreground class of an evaluation this is
                  scipy.ndimage.binary_fill_holes).  hole_connectivity: of the background, None (6, per slice 4), 6 or 26, per slice 4
                  or 8.  max_hole: the largest hole in voxels that is filled (None: no bound).
      min_component  None, a number of voxels, or (mm3, 'mm3') under a spacing (rpnet_amd.postprocess.min_voxels_from_mm3): the
                  components of every foreground class with fewer voxels are removed (rpnet_amd.postprocess.remove_small, under the
                  connectivity of keep_largest, 6 without it).
                  The chain on the final mask is fixed: remove small -> keep largest -> fill holes, each stage reading the output of
                  the one before.  With any stage on, post['mask'], 'counts', 'dice' and 'surface' describe the end of the chain,
                  'components' is None without keep_largest, and `post` gains 'small' and 'holes': per class the figures of
                  postprocess.small_figures / holes_figures (None for a stage that is off).  With both options off nothing changes.
                  post_out is accepted with any stage on and keeps its shape rules; its statistics table [K-1, 4] belongs to keep_largest and
                  is left as it is without that stage.
      post_stats_out  int64 [K-1, 8] on the net's device (needs post_out): columns 0..3 take the statistics row of fill_holes, 4..7 that
                  of remove_small (the columns of a stage that is off are left as they are); 'holes' and 'small' of `post` are None.
      opening, closing  None, a radius in voxels, ('rho', n) for a squared voxel radius, or (x, 'mm') under a spacing: every foreground
                  class is opened / closed by the ball (rpnet_amd.morphology; outside the volume counts as object in the erosions).
                  morph_per_slice: every z slice on its own.  The fixed order of the chain becomes
                  open -> remove small -> keep largest -> close -> fill holes: opening detaches what keep_largest should drop, closing
                  seals what fill_holes should fill.  `post` gains 'opening' and 'closing': per class the figures of
                  morphology.morph_figures (None for a stage that is off).  With both None every launch and every output is what it
                  is without them.
      morph_stats_out  int64 [K-1, 8] on the net's device (needs post_out): columns 0..3 take the statistics row of the opening, 4..7
                  that of the closing (the columns of a stage that is off are left as they are); 'opening' and 'closing' of `post`
                  are None.
      regions=True  once the volume is complete (after the clean-up chain where one is on), one `rpnet_region_stats` call
                  (rpnet_amd.regions.region_stats) on the final mask and, with query_labels, one on the labels, both with the query
                  image and without the background: count, box, coordinate moments and intensity sums of every label.  The result's
                  `regions` is a dict: 'rows_i' int64 [2, K, 20] and 'rows_f' float64 [2, K, 2] on the host (prediction, then labels;
                  the second row is empty without query_labels), 'pred' and 'truth' the per-label figures of regions.derive under the
                  spacing, 'figures' per foreground class those of regions.compare (None without query_labels).  The two small tables
                  cross to the host once per volume.  Nothing else changes.
      regions_out (int64 [2, K, 20], float64 [2, K, 2]) on the net's device (needs regions=True): the rows are written there, nothing
                  crosses to the host for them and the result's `regions` is None.
      components=True | max_components  once the volume is complete (after the clean-up chain where one is on), per foreground class
                  one rpnet_amd.component_stats.component_table chain (label, renumber, tally; connectivity 6) on the final mask
                  with the labels as its `other` volume and, with query_labels, one on the labels with the final mask as theirs, both
                  with the query image at the default scale.  True stands for 4096 components per class.  The result's `components`
                  is a dict: 'rows' int64 [2, K-1, max_components, 24] and 'head' int64 [2, K-1, 4] on the host (prediction, then
                  labels; the second is zero without query_labels), 'scale_log2', and 'figures', per foreground class the dict of
                  component_stats.detection_figures (None without query_labels).  The tables cross to the host once per volume.
                  Nothing else changes.
      components_out (int64 [2, K-1, max_components, 24], int64 [2, K-1, 4]) on the net's device (needs components=...): the rows and
                  head words are written there, nothing crosses to the host for them and the result's `components` is None."""

    def __init__(self, net, batch=8, graphed=True, surface=False, keep_largest=False, spacing=None, surface_tolerance=None, fill_holes=False,
                 hole_connectivity=None, max_hole=None, min_component=None, opening=None, closing=None, morph_per_slice=False, regions=False,
                 components=False):
        if batch < 1:
            raise ValueError("batch must be >= 1")
        self.spacing = None if spacing is None else SS.check_spacing(spacing, "VolumeSegmenter")
        self.surface_tolerance = None if surface_tolerance is None else float(surface_tolerance)
        if self.surface_tolerance is not None and not self.surface_tolerance >= 0:
            raise ValueError(f"VolumeSegmenter: surface_tolerance must be a number >= 0, got {surface_tolerance!r}")
        self.net, self.batch, self.graphed, self.surface = net.eval(), int(batch), bool(graphed), bool(surface)
        self.keep_largest = CC.connectivity_of(keep_largest)
        self.fill_holes = PP.holes_mode_of(fill_holes)          # None: off, False: 3D, True: per slice
        if self.fill_holes is None and (hole_connectivity is not None or max_hole is not None):
            raise ValueError("VolumeSegmenter: hole_connectivity and max_hole need fill_holes")
        self.hole_connectivity = None if self.fill_holes is None else PP.hole_connectivity_of(hole_connectivity, self.fill_holes)
        if max_hole is not None and int(max_hole) < 1:
            raise ValueError(f"VolumeSegmenter: max_hole must be None (no bound) or at least 1 voxel, got {max_hole!r}")
        self.max_hole = None if max_hole is None else int(max_hole)
        self.min_component = check_min_component(min_component)
        self.opening = None if opening is None else MO.check_radius(opening, "VolumeSegmenter: opening")
        self.closing = None if closing is None else MO.check_radius(closing, "VolumeSegmenter: closing")
        self.morph_per_slice = bool(morph_per_slice)
        self.regions = bool(regions)
        self.components = CS.components_option(components)       # 0: off, else max_components
        if self.morph_per_slice and self.opening is None and self.closing is None:
            raise ValueError("VolumeSegmenter: morph_per_slice needs opening or closing")
        self._graphed_eval = graphed if isinstance(graphed, GraphedEval) else None
        if self._graphed_eval is not None and self._graphed_eval.net is not net:
            raise ValueError("VolumeSegmenter: the GraphedEval handed in wraps another net")
        self._tables = {}       # id(static output dict of a captured shape) -> (pointer array, kinds): built once per captured shape
        self._nv = None

    def _model(self, n_ways, n_shots):
        if not (self.graphed and n_ways == 1 and n_shots == 1):
            return self.net
        if self._graphed_eval is None:
            self._graphed_eval = graphed_eval(self.net)
        return self._graphed_eval

    def _table(self, out, appr, shape):
        """host arrays of the launch's sources: refinement 0 .. T-1, output, affine baseline.  For the static outputs of a captured
        graph the arrays are kept (only the baseline's pointer moves with the batch); outputs of an eager call are fresh tensors."""
        ge = self._graphed_eval
        entry = ge._graphs.get(shape) if ge is not None else None
        static = entry is not None and entry[2] is out
        tab = self._tables.get(id(out)) if static else None
        if tab is None:
            T = len(out["refinement"])
            srcs = [out["refinement"][i] for i in range(T)] + [out["output"]]
            for t in srcs:
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise RuntimeError("VolumeSegmenter: the model's logits must be contiguous fp32 tensors")
            S = len(srcs) + 1
            tab = ((C.c_void_p * S)(*([t.data_ptr() for t in srcs] + [0])), (C.c_int32 * S)(*([0] * (S - 1) + [1])), srcs)
            if static:
                self._tables[id(out)] = tab
        tab[0][len(tab[2])] = appr.data_ptr()
        return tab

    def _tally(self, pred, labels, it, ft, row, cls, spacing):
        if spacing is None:
            SF.surface_tally(pred, labels, it, row, ft, row, cls=cls)
        else:
            SS.surface_tally_spacing(pred, labels, spacing, it, row, ft, row, cls=cls, tau=self.surface_tolerance)

    def _figures(self, itab, ftab, spacing):
        if spacing is None:
            return SF.surface_figures(itab.cpu().numpy(), ftab.cpu().numpy())
        return SS.spacing_figures(itab.cpu().numpy(), ftab.cpu().numpy(), self.surface_tolerance)

    def _surface(self, mask, appr, labels, K, surface_out, spacing=None):
        """the rows of the final mask (0) and the affine baseline (1) against the labels, per foreground class"""
        dev = mask.device
        wi, wf = surface_widths(spacing)
        if surface_out is not None:
            itab, ftab = surface_out
        else:
            itab = torch.zeros((2, K - 1, wi), device=dev, dtype=torch.int64)
            ftab = torch.zeros((2, K - 1, wf), device=dev, dtype=torch.float64)
        it, ft = itab.view(-1, wi), ftab.view(-1, wf)
        for s, pred in enumerate((mask, appr)):
            for c in range(1, K):
                self._tally(pred, labels, it, ft, s * (K - 1) + c - 1, c, spacing)
        if surface_out is not None:
            return None
        figures = self._figures(itab, ftab, spacing)
        return {"fewshot": figures[:K - 1], "affine": figures[K - 1:]}

    def _post(self, mask, labels, K, post_out, spacing=None, post_stats_out=None, morph_stats_out=None):
        """the clean-up chain on the final mask (open -> remove small -> keep largest -> close -> fill holes, each stage that is on), and
        what is measured at its end.  Only the last stage tallies the Dice counts: they describe the end of the chain."""
        dev = mask.device
        wi, wf = surface_widths(spacing)
        with_surface = self.surface and labels is not None
        if post_out is not None:
            counts, stats = post_out[:2]
            surf = post_out[2] if with_surface else None
        else:
            counts = torch.zeros((K - 1, CC.COUNTS_ROW), device=dev, dtype=torch.int64) if labels is not None else None
            stats = torch.zeros((K - 1, CC.STATS_ROW), device=dev, dtype=torch.int64)
            surf = (torch.zeros((K - 1, wi), device=dev, dtype=torch.int64),
                    torch.zeros((K - 1, wf), device=dev, dtype=torch.float64)) if with_surface else None
        kept = torch.empty_like(mask)
        stages = [name for name, on in (("opening", self.opening is not None), ("small", self.min_component is not None),
                                        ("largest", bool(self.keep_largest)), ("closing", self.closing is not None),
                                        ("holes", self.fill_holes is not None)) if on]
        tables, src = {}, mask
        for name in stages:
            last = name == stages[-1]
            tally = dict(truth=labels if last else None, out=kept, counts=counts if last else None)
            if name == "small":
                m = self.min_component
                if isinstance(m, tuple):
                    if spacing is None:
                        raise ValueError("VolumeSegmenter: min_component in mm3 needs a spacing")
                    m = PP.min_voxels_from_mm3(m[0], spacing)
                tables[name] = PP.remove_small(src, range(1, K), m, connectivity=self.keep_largest or 6, **tally)[2]
            elif name == "largest":
                CC.keep_largest(src, classes=range(1, K), connectivity=self.keep_largest, stats=stats, **tally)
            elif name in ("opening", "closing"):
                radius = getattr(self, name)
                fn = MO.opening if name == "opening" else MO.closing
                tables[name] = fn(src, range(1, K), (radius[1], "mm") if radius[0] == "mm" else radius, spacing=spacing,
                                  per_slice=self.morph_per_slice, **tally)[2]
            else:
                tables[name] = PP.fill_holes(src, range(1, K), connectivity=self.hole_connectivity, per_slice=self.fill_holes,
                                             max_hole=self.max_hole, **tally)[2]
            src = kept                  # the later stages work in place on the output of the first
        if with_surface:
            for c in range(1, K):
                self._tally(kept, labels, surf[0], surf[1], c - 1, c, spacing)
        if post_stats_out is not None:
            for at, name in ((0, "holes"), (PP.STATS_ROW, "small")):
                if name in tables:
                    post_stats_out[:, at:at + PP.STATS_ROW].copy_(tables[name])
        if morph_stats_out is not None:
            for at, name in ((0, "opening"), (MO.STATS_ROW, "closing")):
                if name in tables:
                    morph_stats_out[:, at:at + MO.STATS_ROW].copy_(tables[name])
        post = {"mask": kept, "counts": None, "dice": None, "components": None, "surface": None}
        morph = self.opening is not None or self.closing is not None
        extended = any(name in ("small", "holes") for name in stages)
        if extended:
            post.update(holes=None, small=None)
        if morph:
            post.update(opening=None, closing=None)
        if post_out is None:
            for name in ("opening", "closing"):
                if name in tables:
                    post[name] = MO.morph_figures(tables[name].cpu().numpy())
            if self.keep_largest:
                post["components"] = CC.components_figures(stats.cpu().numpy())
            if "holes" in tables:
                post["holes"] = PP.holes_figures(tables["holes"].cpu().numpy())
            if "small" in tables:
                post["small"] = PP.small_figures(tables["small"].cpu().numpy())
            if counts is not None:
                post["counts"] = counts.cpu().numpy()
                post["dice"] = dice_from_counts(post["counts"])
            if with_surface:
                post["surface"] = self._figures(surf[0], surf[1], spacing)
        return post

    def _regions(self, final, labels, image, K, regions_out, spacing=None):
        """the region rows of the final mask (0) and of the labels (1), labels 1 .. K-1, with the query image"""
        if regions_out is not None:
            tables = tuple(regions_out)
        else:
            tables = (torch.zeros((2, K, RG.IROW), device=final.device, dtype=torch.int64),
                      torch.zeros((2, K, RG.FROW), device=final.device, dtype=torch.float64))
        RG.region_stats(final, image, n_labels=K, out=tables, row=0)
        if labels is not None:
            RG.region_stats(labels, image, n_labels=K, out=tables, row=1)
        if regions_out is not None:
            return None
        rows_i, rows_f = tables[0].cpu().numpy(), tables[1].cpu().numpy()
        return {"rows_i": rows_i, "rows_f": rows_f, "pred": RG.derive(rows_i[0], rows_f[0], spacing),
                "truth": RG.derive(rows_i[1], rows_f[1], spacing) if labels is not None else None,
                "figures": RG.region_figures(rows_i, rows_f, spacing) if labels is not None else None}

    def _components(self, final, labels, image, K, components_out, spacing=None):
        """the component tables and head words of the final mask (0) and of the labels (1), per foreground class, each with the other
        volume as its `other` and with the query image"""
        if components_out is not None:
            rows, heads = components_out
        else:
            rows = torch.zeros((2, K - 1, self.components, CS.COMP_ROW), device=final.device, dtype=torch.int64)
            heads = torch.zeros((2, K - 1, CS.HEAD_WORDS), device=final.device, dtype=torch.int64)
        for c in range(1, K):
            CS.component_table(final, cls=c, image=image, other=labels, max_components=self.components, out=rows[0], row=c - 1,
                               head_out=heads[0, c - 1])
            if labels is not None:
                CS.component_table(labels, cls=c, image=image, other=final, max_components=self.components, out=rows[1], row=c - 1,
                                   head_out=heads[1, c - 1])
        if components_out is not None:
            return None
        rows, heads = rows.cpu().numpy(), heads.cpu().numpy()
        return {"rows": rows, "head": heads, "scale_log2": CS.default_scale_log2(image),
                "figures": CS.detection_figures(rows, heads, spacing) if labels is not None else None}

    def __call__(self, support_images, support_fg, query_images, appr_query_labels, query_labels=None, counts_out=None, surface_out=None,
                 post_out=None, spacing=None, post_stats_out=None, morph_stats_out=None, regions_out=None, components_out=None):
        dev = next(self.net.parameters()).device
        morph = self.opening is not None or self.closing is not None
        chain = bool(self.keep_largest) or self.fill_holes is not None or self.min_component is not None or morph
        spacing = self.spacing if spacing is None else SS.check_spacing(spacing, "VolumeSegmenter")
        if self.surface_tolerance is not None and spacing is None and self.surface:
            raise ValueError("VolumeSegmenter: surface_tolerance is a distance in the unit of a spacing; give spacing= as well")
        n_ways, n_shots = len(support_images), len(support_images[0])
        S, B = query_images.shape[0], self.batch
        H, W = query_images.shape[-2:]
        K = n_ways + 1
        if counts_out is not None:
            if query_labels is None:
                raise ValueError("counts_out needs query_labels (there is nothing to tally without the ground truth)")
            check_counts_out(counts_out, K, getattr(self.net, "num_iter", None))
            if counts_out.device != dev:
                raise ValueError(f"counts_out is on {counts_out.device}, the net on {dev}")
        if surface_out is not None:
            if not self.surface:
                raise ValueError("surface_out needs VolumeSegmenter(surface=True)")
            if query_labels is None:
                raise ValueError("surface_out needs query_labels (a surface distance is measured against the ground truth)")
            check_surface_out(surface_out, K, spacing)
            if any(t.device != dev for t in surface_out):
                raise ValueError(f"surface_out is on {surface_out[0].device}, the net on {dev}")
        if post_out is not None:
            if not chain:
                raise ValueError("post_out needs VolumeSegmenter(keep_largest=True, 6 or 26, fill_holes=... or min_component=...)")
            if query_labels is None:
                raise ValueError("post_out needs query_labels (there is nothing to tally without the ground truth)")
            check_post_out(post_out, K, self.surface, spacing)
            flat = list(post_out[:2]) + (list(post_out[2]) if self.surface else [])
            if any(t.device != dev for t in flat):
                raise ValueError(f"post_out is on {next(t.device for t in flat if t.device != dev)}, the net on {dev}")
        if post_stats_out is not None:
            if post_out is None or (self.fill_holes is None and self.min_component is None):
                raise ValueError("post_stats_out needs post_out and VolumeSegmenter(fill_holes=... or min_component=...)")
            if not (torch.is_tensor(post_stats_out) and post_stats_out.dtype == torch.int64 and post_stats_out.is_contiguous()
                    and tuple(post_stats_out.shape) == (K - 1, 2 * PP.STATS_ROW)):
                raise ValueError(f"post_stats_out must be a contiguous int64 [{K - 1}, {2 * PP.STATS_ROW}] tensor")
            if post_stats_out.device != dev:
                raise ValueError(f"post_stats_out is on {post_stats_out.device}, the net on {dev}")
        if morph:
            for radius in (self.opening, self.closing):
                if radius is not None and radius[0] == "mm" and spacing is None:
                    raise ValueError("VolumeSegmenter: an opening or closing radius in mm needs a spacing")
        if morph_stats_out is not None:
            if post_out is None or not morph:
                raise ValueError("morph_stats_out needs post_out and VolumeSegmenter(opening=... or closing=...)")
            if not (torch.is_tensor(morph_stats_out) and morph_stats_out.dtype == torch.int64 and morph_stats_out.is_contiguous()
                    and tuple(morph_stats_out.shape) == (K - 1, 2 * MO.STATS_ROW)):
                raise ValueError(f"morph_stats_out must be a contiguous int64 [{K - 1}, {2 * MO.STATS_ROW}] tensor")
            if morph_stats_out.device != dev:
                raise ValueError(f"morph_stats_out is on {morph_stats_out.device}, the net on {dev}")
        if regions_out is not None:
            if not self.regions:
                raise ValueError("regions_out needs VolumeSegmenter(regions=True)")
            RG.check_regions_out(regions_out, K)
            if any(t.device != dev for t in regions_out):
                raise ValueError(f"regions_out is on {regions_out[0].device}, the net on {dev}")
        if components_out is not None:
            if not self.components:
                raise ValueError("components_out needs VolumeSegmenter(components=...)")
            CS.check_components_out(components_out, K, self.components)
            if any(t.device != dev for t in components_out):
                raise ValueError(f"components_out is on {components_out[0].device}, the net on {dev}")
        nb = -(-S // B)
        pad = nb * B - S

        def prep(x, dtype=torch.float32):
            x = x.to(device=dev, dtype=dtype)
            if pad:
                x = torch.cat([x, x[-1:].expand(pad, *x.shape[1:])], 0)       # the filler of the last batch: the last slice again
            return x.contiguous()

        with torch.no_grad():
            si = [[prep(x) for x in way] for way in support_images]
            fg = [[prep(x) for x in way] for way in support_fg]
            bg = [[1 - x for x in way] for way in fg]
            qi, appr = prep(query_images), prep(appr_query_labels)
            labels = prep(query_labels, torch.int32) if query_labels is not None else None
            mask = torch.empty((nb * B, H, W), device=dev, dtype=torch.uint8)
            if self._nv is None or self._nv.device != dev:
                self._nv = torch.empty(1, device=dev, dtype=torch.int32)
            model = self._model(n_ways, n_shots)
            counts, nv_now = None, None
            for i in range(nb):
                sl = slice(i * B, (i + 1) * B)
                out = model([[x[sl] for x in way] for way in si], [[x[sl] for x in way] for way in fg],
                            [[x[sl] for x in way] for way in bg], [qi[sl]], appr_query_labels=appr[sl])
                # (which tensors hold this call's logits is known only now: GraphedEval returns its static outputs after a replay,
                # fresh ones when it had to redo the call eagerly on measured fp16 scales)
                tab = self._table(out, appr[sl], tuple(si[0][0][sl].shape))
                T = len(tab[2]) - 1
                if labels is not None and counts is None:
                    if counts_out is not None:
                        check_counts_out(counts_out, K, T)
                    counts = counts_out if counts_out is not None else torch.zeros((T + 2, K - 1, 3), device=dev, dtype=torch.int64)
                n_valid = min(B, S - i * B)
                if n_valid != nv_now:
                    self._nv.fill_(n_valid)
                    nv_now = n_valid
                seg_tally(tab[2] + [appr[sl]], [0] * (T + 1) + [1], self._nv, labels[sl] if labels is not None else None, counts,
                          mask[sl], mask_src=T, K=K, _table=tab)
            surface = self._surface(mask[:S], appr[:S], labels[:S], K, surface_out, spacing) if self.surface and labels is not None else None
            post = self._post(mask[:S], labels[:S] if labels is not None else None, K, post_out, spacing, post_stats_out, morph_stats_out) if chain else None
            regions = self._regions(post["mask"] if chain else mask[:S], labels[:S] if labels is not None else None, qi[:S, 0], K, regions_out,
                                    spacing) if self.regions else None
            components = self._components(post["mask"] if chain else mask[:S], labels[:S] if labels is not None else None,
                                          qi[:S, 0], K, components_out, spacing) if self.components else None
        if counts is None or counts_out is not None:
            res = VolumeResult(mask[:S], None, None)
        else:
            host = counts.cpu().numpy()                 # the one transfer of the volume
            T = host.shape[0] - 2
            dice = {"fewshot": dice_from_counts(host[T]), "affine": dice_from_counts(host[T + 1]),
                    "refinement": {i: dice_from_counts(host[i]) for i in range(T)}}
            res = VolumeResult(mask[:S], host, dice)
        if surface is not None:
            res.surface = surface
        if post is not None:
            res.post = post
        if regions is not None:
            res.regions = regions
        if components is not None:
            res.components = components
        return res
