#!/usr/bin/env python3
"""Evaluation loop over FewshotRegReader items, in the shape of the reference's driver
(test_rpnet.py:151-258: volumes -> 2-slice batches -> net(...) -> Dice per refinement
iteration), using only the symbols that driver imports, at the reference's import paths.
The reference file itself cannot run offline (it needs tensorboard and the private data).

    python tools/eval_driver.py --yaml yamls/example.yml [--items 2] [--on-device] [--device-items] [--batch 8] [--save-pred DIR]
                                [--surface] [--keep-largest [6|26]] [--spacing header|Z,Y,X] [--surface-tolerance MM]

--on-device: the same lines from rpnet_amd.volume.VolumeSegmenter (masks and Dice tallies on the device, one transfer per volume,
`--batch` slices per model call through the captured graph); --save-pred DIR writes each volume's predicted mask as
DIR/<pid>_<class>.nrrd (uint8, gzip) and implies --on-device.  --device-items (implies --on-device; needs NRRD volumes under the
yaml's data_dir): the items too are built on the device (rpnet_amd.dataset_eval.DeviceEvalSource: volumes cached in HBM, one gather
launch and the registration launches per item) and the tallies and both image similarity figures of all volumes cross to the host
once, after the last volume (rpnet_amd.dataset_eval.evaluate_dataset).  --surface (implies --on-device; works with --device-items):
every item line ends with ` hd95 <fewshot> (<affine>) assd <fewshot> (<affine>)`, the 95th-percentile Hausdorff and the average
symmetric surface distance of the final mask and of the affine baseline in voxels (rpnet_amd.surface), every class line with their
means.  --keep-largest [6|26] (implies --on-device; works with --device-items and --surface; 6 when no number is given): every
volume's final mask is also filtered to the largest connected component of its class on the device (rpnet_amd.components) and every
item line ends with ` lcc <dice> (<n_components> components, <removed> voxels removed)`, followed by ` lcc hd95 <v> assd <v>` under
--surface, every class line with their means; --save-pred then writes the filtered mask.  --spacing header|Z,Y,X and
--surface-tolerance MM (both imply --surface; the yaml keys surface_spacing and surface_tolerance are their defaults): the surface
distances in millimetres on the voxel spacing of every query volume's NRRD header, or on one given spacing (rpnet_amd.surface_spacing),
each figure followed by `mm`, and with a tolerance the normalised surface Dice ` nsd <fewshot> (<affine>)`.
--runs R [--fuse vote|staple] [--fuse-all-voxels] (needs --device-items): the evaluation R times over, every run with a freshly drawn
support volume per query, then the reference's "Average performance" block (test_rpnet.py:112-145; rpnet_amd.fusion.evaluate_runs).
--fuse fuses every query's R final masks on the device by majority vote or STAPLE and prints the fused Dice beside the runs' own;
--fuse-all-voxels lets the voxels on which all runs agree take part in STAPLE's EM; --save-pred then writes the fused mask.
--regions (needs --device-items): every item line gains ` vol <pred> (<truth>) rvd <x> cdist <x>`, the volume of the final mask (of the
labels), their relative volume difference and the distance of their centroids, in voxels, under --spacing in ml and mm
(rpnet_amd.regions), every class line their means.
--components [N] (needs --device-items): every item line gains ` comp <Cp> (<Ct>) det <detected>/<Ct> fp <n> fpvol <voxels>`, the
connected components of the final mask (of the labels), the label components the mask overlaps, the mask components that overlap no
label voxel and their volume, in voxels, under --spacing in mL (rpnet_amd.component_stats; N components per class are tallied, 4096
without N), every class line their means.
"""
import argparse
import os
import sys
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from dataset.few_shot_reader import FewshotRegReader
from net.model import model_factory
from net.registration import NCC
from utils.util import dice_score_seperate, load_yaml


def evaluate(net, loader, config, n_items=None, batch_size=2):
    net.eval()
    classes = config["eval_classes"]
    dsc_affine, dsc_fewshot, dsc_ref = defaultdict(list), defaultdict(list), defaultdict(lambda: defaultdict(list))
    for j in range(len(loader) if n_items is None else min(n_items, len(loader))):
        s = loader[j]
        with torch.no_grad():
            si = [[x.float().cuda() for x in way] for way in s["support_images"]]
            fg = [[x.float().cuda() for x in way] for way in s["support_labels"]]
            bg = [[1 - x for x in way] for way in fg]
            qi, ql, appr = s["query_images"].float().cuda(), s["query_labels"].long().cuda(), s["appr_query_labels"].cuda()
            fewshot, ref = [], defaultdict(list)
            for i in range(int(np.ceil(len(qi) / batch_size))):
                sl = slice(i * batch_size, (i + 1) * batch_size)
                out = net([[x[sl] for x in way] for way in si], [[x[sl] for x in way] for way in fg],
                          [[x[sl] for x in way] for way in bg], [qi[sl]], grid=s["grid"][sl], query_labels=ql[sl],
                          appr_query_labels=appr[sl])
                fewshot.append(out["output"].softmax(dim=1)[:, [1]].cpu())
                for k, v in out["refinement"].items():
                    ref[k].append(v.softmax(dim=1)[:, 1].cpu())
            pred = (torch.cat(fewshot, 0).permute(1, 0, 2, 3).numpy() > 0.5).astype(np.float32)
            gt = ql.cpu().numpy()[None]
            name = classes[s["class_id"]]
            d_aff = dice_score_seperate(appr.cpu().numpy()[None], gt, num_class=1)[0]
            d_few = dice_score_seperate(pred, gt, num_class=1)[0]
            ncc = NCC(qi, s["warped_supp"].unsqueeze(1).cuda()).item()
            dsc_affine[name].append(d_aff)
            dsc_fewshot[name].append(d_few)
            line = f"{j} {s['pid']} affine ({ncc:.4f}) {d_aff}, fewshot {d_few}"
            for k, v in ref.items():
                d = dice_score_seperate((torch.cat(v, 0).numpy() > 0.5).astype(np.int32)[None], gt, num_class=1)[0]
                dsc_ref[name][k].append(d)
                line += f" ref {k} {d},"
            print(line)
    for name in classes:
        if dsc_fewshot[name]:
            print(f"{name}, affine {np.mean(dsc_affine[name]):.4f}, fewshot {np.mean(dsc_fewshot[name]):.4f}")
    return dsc_affine, dsc_fewshot, dsc_ref


def parse_spacing(value):
    """None, "header" or a triple of floats from the command line / the yaml: `header`, `Z,Y,X` or a list of three numbers"""
    if value is None or value == "header":
        return value
    parts = value.split(",") if isinstance(value, str) else list(value)
    try:
        triple = tuple(float(v) for v in parts)
    except (TypeError, ValueError):
        triple = ()
    if len(triple) != 3:
        raise ValueError(f"--spacing / surface_spacing: `header` or three numbers Z,Y,X, got {value!r}")
    return triple


def parse_min_component(value):
    """--min-component: None, a number of voxels, or `<x>mm3` -> (x, "mm3"), which needs a spacing"""
    if value is None:
        return None
    text = str(value).strip()
    try:
        if text.lower().endswith("mm3"):
            return (float(text[:-3]), "mm3")
        return int(text)
    except ValueError:
        raise ValueError(f"--min-component: a number of voxels or <x>mm3, got {value!r}") from None


def parse_radius(value, flag="--opening"):
    """--opening / --closing: None, a radius in voxels, or `<x>mm` -> (x, "mm"), which needs a spacing"""
    if value is None:
        return None
    text = str(value).strip()
    try:
        if text.lower().endswith("mm"):
            return (float(text[:-2]), "mm")
        return float(text)
    except ValueError:
        raise ValueError(f"{flag}: a radius in voxels or <x>mm, got {value!r}") from None


def evaluate_on_device(net, loader, config, n_items=None, batch_size=8, save_pred=None, graphed=True, segmenter=None, surface=False,
                       keep_largest=False, spacing=None, surface_tolerance=None, fill_holes=False, hole_connectivity=None, max_hole=None,
                       min_component=None, opening=None, closing=None, morph_per_slice=False):
    """`evaluate` through rpnet_amd.volume.VolumeSegmenter: the same printed lines and return value; thresholds, Dice tallies and the
    predicted mask are formed on the device, the tallies cross to the host once per volume.  save_pred: a directory that receives
    every volume's mask as <pid>_<class>.nrrd; segmenter: a VolumeSegmenter to reuse (its captured graphs live with it); surface: the
    lines gain the surface distances of rpnet_amd.surface (a segmenter handed in must have been made with surface=True); keep_largest
    (False, True = 6, 6 or 26): the lines gain the figures of the mask filtered to its largest component (rpnet_amd.components), and
    save_pred writes that mask (a segmenter handed in must have been made with the same keep_largest).  spacing (None, "header" or a
    triple) and surface_tolerance: the surface figures in millimetres, as evaluate_dataset prints them; "header" reads the header of
    every query volume before the first item.  fill_holes, hole_connectivity, max_hole, min_component: the clean-up chain of
    VolumeSegmenter (remove small -> keep largest -> fill holes, rpnet_amd.postprocess); the lines gain ` holes <n> (<filled> voxels
    filled)` and ` small <n> (<removed> voxels removed)` for the stages that are on, the lcc figures and save_pred describe the end of the
    chain, and min_component in mm3 is resolved under every item's spacing (a segmenter handed in must have been made with the same
    options).  opening, closing (None, voxels, ('rho', n) or (x, 'mm') under a spacing), morph_per_slice: the ball morphology of
    VolumeSegmenter (rpnet_amd.morphology), the chain becoming open -> remove small -> keep largest -> close -> fill holes; the lines gain
    ` open -<removed> +<added>` and ` close -<removed> +<added>` for the stages that are on."""
    from rpnet_amd import components as CC
    from rpnet_amd import morphology as MO
    from rpnet_amd import postprocess as PP
    from rpnet_amd.volume import check_min_component
    from rpnet_amd import surface as SF
    from rpnet_amd import surface_spacing as SS
    from rpnet_amd.utils import nrrd
    from rpnet_amd.volume import VolumeSegmenter
    conn = CC.connectivity_of(keep_largest)
    if surface_tolerance is not None and spacing is None:
        raise ValueError("evaluate_on_device: surface_tolerance is a distance in millimetres; give spacing= as well")
    holes_mode, small_min = PP.holes_mode_of(fill_holes), check_min_component(min_component)
    holes_on, small_on = holes_mode is not None, small_min is not None
    open_r = None if opening is None else MO.check_radius(opening, "evaluate_on_device: opening")
    close_r = None if closing is None else MO.check_radius(closing, "evaluate_on_device: closing")
    morph_on = open_r is not None or close_r is not None
    chain = bool(conn) or holes_on or small_on or morph_on
    if isinstance(small_min, tuple) and spacing is None:
        raise ValueError("evaluate_on_device: min_component in mm3 needs a spacing (a triple or 'header')")
    if any(r is not None and r[0] == "mm" for r in (open_r, close_r)) and spacing is None:
        raise ValueError("evaluate_on_device: an opening or closing radius in mm needs a spacing (a triple or 'header')")
    seg = segmenter or VolumeSegmenter(net, batch=batch_size, graphed=graphed, surface=surface, keep_largest=conn or False,
                                       surface_tolerance=surface_tolerance, fill_holes=fill_holes, hole_connectivity=hole_connectivity,
                                       max_hole=max_hole, min_component=min_component,
                                       **(dict(opening=opening, closing=closing, morph_per_slice=morph_per_slice) if morph_on else {}))
    if morph_on and (seg.opening != open_r or seg.closing != close_r or seg.morph_per_slice != bool(morph_per_slice)):
        raise ValueError("evaluate_on_device(opening=..., closing=...) needs a VolumeSegmenter made with the same options")
    if (holes_on or small_on) and (seg.fill_holes != holes_mode or seg.min_component != small_min):
        raise ValueError("evaluate_on_device(fill_holes=..., min_component=...) needs a VolumeSegmenter made with the same options")
    n_loop = len(loader) if n_items is None else min(n_items, len(loader))
    mm, nsd = spacing is not None, surface_tolerance is not None
    if spacing == "header":
        rd = loader.fewshot_reader.fewshot_volume_reader
        spacings = [rd.volume_spacing(rd.data_info[c][qv]["pid"]) for c, qv in rd.indices[:n_loop]]
    else:
        spacings = [spacing] * n_loop
    if surface and not seg.surface:
        raise ValueError("evaluate_on_device(surface=True) needs a VolumeSegmenter(surface=True)")
    if conn and seg.keep_largest != conn:
        raise ValueError(f"evaluate_on_device(keep_largest={conn}) needs a VolumeSegmenter(keep_largest={conn})")
    lcc_dice, lcc_fig, lcc_surf = defaultdict(list), defaultdict(list), defaultdict(list)
    holes_fig, small_fig = defaultdict(list), defaultdict(list)
    open_fig, close_fig = defaultdict(list), defaultdict(list)
    surf_few, surf_aff = defaultdict(list), defaultdict(list)
    classes = config["eval_classes"]
    dsc_affine, dsc_fewshot, dsc_ref = defaultdict(list), defaultdict(list), defaultdict(lambda: defaultdict(list))
    if save_pred:
        os.makedirs(save_pred, exist_ok=True)
    for j in range(n_loop):
        s = loader[j]
        res = seg(s["support_images"], s["support_labels"], s["query_images"], s["appr_query_labels"], s["query_labels"],
                  **({"spacing": spacings[j]} if mm else {}))
        name = classes[s["class_id"]]
        d_aff, d_few = res.dice["affine"][0], res.dice["fewshot"][0]
        with torch.no_grad():
            ncc = NCC(s["query_images"].float().cuda(), s["warped_supp"].unsqueeze(1).cuda()).item()
        dsc_affine[name].append(d_aff)
        dsc_fewshot[name].append(d_few)
        line = f"{j} {s['pid']} affine ({ncc:.4f}) {d_aff}, fewshot {d_few}"
        for k, d in res.dice["refinement"].items():
            dsc_ref[name][k].append(d[0])
            line += f" ref {k} {d[0]},"
        if surface:
            few, aff = res.surface["fewshot"][0], res.surface["affine"][0]
            surf_few[name].append(few)
            surf_aff[name].append(aff)
            line += SS.line_suffix_mm(few, aff, nsd) if mm else SF.line_suffix(few, aff)
        if conn:
            d_lcc, fig = res.post["dice"][0], res.post["components"][0]
            kept = res.post["surface"][0] if surface else None
            lcc_dice[name].append(d_lcc)
            lcc_fig[name].append(fig)
            lcc_surf[name].append(kept)
            line += CC.line_suffix(d_lcc, fig, kept, unit="mm" if mm else "")
        if holes_on or small_on:
            h, sm = res.post["holes"][0] if holes_on else None, res.post["small"][0] if small_on else None
            holes_fig[name].append(h)
            small_fig[name].append(sm)
            line += PP.line_suffix(h, sm)
        if morph_on:
            op, cl = res.post["opening"][0] if open_r is not None else None, res.post["closing"][0] if close_r is not None else None
            open_fig[name].append(op)
            close_fig[name].append(cl)
            line += MO.line_suffix(op, cl)
        print(line)
        if save_pred:
            nrrd.write(os.path.join(save_pred, f"{s['pid']}_{name}.nrrd"), (res.post["mask"] if chain else res.mask).cpu().numpy(),
                       encoding="gzip")
    for name in classes:
        if dsc_fewshot[name]:
            print(f"{name}, affine {np.mean(dsc_affine[name]):.4f}, fewshot {np.mean(dsc_fewshot[name]):.4f}"
                  + ((SS.mean_suffix_mm(surf_few[name], surf_aff[name], nsd) if mm else SF.mean_suffix(surf_few[name], surf_aff[name]))
                     if surface else "")
                  + (CC.mean_suffix(lcc_dice[name], lcc_fig[name], lcc_surf[name] if surface else None, unit="mm" if mm else "") if conn else "")
                  + (PP.mean_suffix(holes_fig[name] if holes_on else None, small_fig[name] if small_on else None)
                     if holes_on or small_on else "")
                  + (MO.mean_suffix(open_fig[name] if open_r is not None else None, close_fig[name] if close_r is not None else None)
                     if morph_on else ""))
    return dsc_affine, dsc_fewshot, dsc_ref


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yaml", default="yamls/example.yml")
    ap.add_argument("--items", type=int, default=None)
    ap.add_argument("--on-device", action="store_true", help="masks and Dice tallies on the device (rpnet_amd.volume.VolumeSegmenter)")
    ap.add_argument("--batch", type=int, default=None, help="slices per model call (default: 2, or 8 with --on-device)")
    ap.add_argument("--save-pred", default=None, metavar="DIR", help="write each volume's mask as DIR/<pid>_<class>.nrrd; implies --on-device")
    ap.add_argument("--device-items", action="store_true",
                    help="build the items on the device too and fetch all tallies once (rpnet_amd.dataset_eval); implies --on-device")
    ap.add_argument("--device-load", action="store_true",
                    help="with --device-items: crop, percentile clip and normalise every volume on the device from the payloads of its "
                         "files (rpnet_amd.volume_load), the same bits as the host reader's")
    ap.add_argument("--surface", action="store_true",
                    help="HD95 and ASSD of the final mask and the affine baseline at the end of every line (rpnet_amd.surface); implies --on-device")
    ap.add_argument("--keep-largest", type=int, nargs="?", const=6, default=0, choices=(6, 26), metavar="6|26",
                    help="also keep only the largest connected component of the final mask (connectivity 6 or 26, 6 when no number is "
                         "given) and print its figures at the end of every line (rpnet_amd.components); implies --on-device")
    ap.add_argument("--spacing", default=None, metavar="header|Z,Y,X",
                    help="surface distances in millimetres: the voxel spacing of every query volume's NRRD header, or one spacing for "
                         "all (rpnet_amd.surface_spacing); implies --surface; default: the yaml key surface_spacing")
    ap.add_argument("--surface-tolerance", type=float, default=None, metavar="MM",
                    help="also the normalised surface Dice at this tolerance in millimetres; implies --surface and needs a spacing; "
                         "default: the yaml key surface_tolerance")
    ap.add_argument("--fill-holes", nargs="?", const="3d", default=None, choices=("3d", "slice"), metavar="3d|slice",
                    help="fill the holes of the final mask, of the volume (3d, also when no word is given) or of every slice on its own "
                         "(rpnet_amd.postprocess); implies --on-device")
    ap.add_argument("--max-hole", type=int, default=None, metavar="VOXELS", help="fill only holes of at most this many voxels; needs --fill-holes")
    ap.add_argument("--min-component", default=None, metavar="VOXELS|<x>mm3",
                    help="remove the components of the final mask with fewer voxels, or below <x> cubic millimetres under --spacing (with "
                         "`header` resolved per item); implies --on-device")
    ap.add_argument("--opening", default=None, metavar="R[mm]",
                    help="open the final mask by a ball of this radius in voxels, or in millimetres under --spacing (rpnet_amd.morphology), "
                         "before the component filters; implies --on-device")
    ap.add_argument("--closing", default=None, metavar="R[mm]",
                    help="close the final mask by a ball of this radius in voxels, or in millimetres under --spacing, before the holes are "
                         "filled; implies --on-device")
    ap.add_argument("--morph-slice", action="store_true", help="--opening and --closing on every slice on its own")
    ap.add_argument("--registration", choices=("affine", "demons", "deeds"), default=None,
                    help="the registration pre-step of every item (overrides the yaml key do_deformable: False, True or deeds)")
    ap.add_argument("--runs", type=int, default=None, metavar="R",
                    help="with --device-items: evaluate R times, each run with a freshly drawn support volume per query, and print the "
                         "average over the runs (rpnet_amd.fusion.evaluate_runs)")
    ap.add_argument("--fuse", choices=("vote", "staple"), default=None,
                    help="with --runs: fuse every query's masks of the R runs on the device (rpnet_amd.fusion); --save-pred writes the fused mask")
    ap.add_argument("--regions", action="store_true",
                    help="with --device-items: volume, relative volume difference and centroid distance of every final mask against the "
                         "labels (rpnet_amd.regions), in voxels, or in ml and mm under --spacing")
    ap.add_argument("--components", nargs="?", type=int, const=True, default=None, metavar="N",
                    help="with --device-items: per-component detection counts of every final mask against the labels "
                         "(rpnet_amd.component_stats), N components tallied per class (4096 without N)")
    ap.add_argument("--fuse-all-voxels", action="store_true", help="with --fuse staple: the voxels all runs agree on take part in the EM")
    return ap


def main():
    a = build_parser().parse_args()
    config, args = load_yaml(a.yaml)
    if a.registration is not None:
        from rpnet_amd.registration import REGISTRATION_STAGES
        config["do_deformable"] = REGISTRATION_STAGES[a.registration]
    config["n_iter_refinement"] = config["n_test_iter_refinement"]            # test_rpnet.py:51
    spacing = parse_spacing(a.spacing if a.spacing is not None else config.get("surface_spacing"))
    tolerance = a.surface_tolerance if a.surface_tolerance is not None else config.get("surface_tolerance")
    a.surface = a.surface or spacing is not None or tolerance is not None
    if a.device_load and not a.device_items:
        raise SystemExit("--device-load needs --device-items")
    if a.runs is not None and not a.device_items:
        raise SystemExit("--runs needs --device-items")
    if a.regions and not a.device_items:
        raise SystemExit("--regions needs --device-items")
    if a.components is not None and not a.device_items:
        raise SystemExit("--components needs --device-items")
    if (a.fuse or a.fuse_all_voxels) and a.runs is None:
        raise SystemExit("--fuse and --fuse-all-voxels need --runs")
    min_component = parse_min_component(a.min_component)
    if a.max_hole is not None and a.fill_holes is None:
        raise SystemExit("--max-hole needs --fill-holes")
    if isinstance(min_component, tuple) and spacing is None:
        raise SystemExit("--min-component <x>mm3 needs --spacing")
    opening, closing = parse_radius(a.opening, "--opening"), parse_radius(a.closing, "--closing")
    if any(isinstance(r, tuple) for r in (opening, closing)) and spacing is None:
        raise SystemExit("--opening / --closing <x>mm needs --spacing")
    if a.morph_slice and opening is None and closing is None:
        raise SystemExit("--morph-slice needs --opening or --closing")
    post = dict(fill_holes=a.fill_holes or False, max_hole=a.max_hole, min_component=min_component)
    if opening is not None or closing is not None:
        post.update(opening=opening, closing=closing, morph_per_slice=a.morph_slice)
    if a.regions:
        post.update(regions=True)
    if a.components is not None:
        post.update(components=a.components)
    loader = None if a.device_items else FewshotRegReader(args.data_dir, args.eval_set_name, config, mode="eval")
    net = model_factory[args.net](pretrained_path=config.get("pretrained_path"),
                                  cfg={"align": True, "backbone": config.get("backbone", "vgg")}, backbone_cfg=config).cuda()
    if args.ckpt:
        state = net.state_dict()
        state.update(torch.load(args.ckpt)["state_dict"])
        net.load_state_dict(state)
    if a.device_items:
        from rpnet_amd.dataset_eval import DeviceEvalSource, evaluate_dataset
        source = DeviceEvalSource(args.data_dir, args.eval_set_name, config, next(net.parameters()).device, device_load=a.device_load)
        source.warm()
        if a.runs is not None:
            from rpnet_amd.fusion import evaluate_runs, save_fused
            _, _, fused = evaluate_runs(net, source, config, a.runs, a.fuse, not a.fuse_all_voxels, a.items, a.batch or 8,
                                        save_pred=None if a.fuse else a.save_pred, surface=a.surface, keep_largest=a.keep_largest or False,
                                        spacing=spacing, surface_tolerance=tolerance, **post)
            if a.fuse and a.save_pred:
                save_fused(fused, source, config, a.save_pred)
            return
        evaluate_dataset(net, source, config, a.items, a.batch or 8, save_pred=a.save_pred, surface=a.surface,
                         keep_largest=a.keep_largest or False, spacing=spacing, surface_tolerance=tolerance, **post)
    elif a.on_device or a.save_pred or a.surface or a.keep_largest or a.fill_holes or min_component is not None or "opening" in post:
        evaluate_on_device(net, loader, config, a.items, a.batch or 8, a.save_pred, surface=a.surface, keep_largest=a.keep_largest or False,
                           spacing=spacing, surface_tolerance=tolerance, **post)
    else:
        evaluate(net, loader, config, a.items, a.batch or 2)


if __name__ == "__main__":
    main()
