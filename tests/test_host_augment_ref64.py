"""CPU self-check of tests/augment_ref_cases.py: (1) the bounds have room for a correct implementation — SimBackend, a float32 /
float64 restatement in the kernels' operation order whose pow and whose fp64 sums differ from numpy's the way a device's may, passes every
row of every table; (2) the checks see what they are there to see — each seeded defect of DEFECTS fails them; (3) every tie case has at
least half its pixels exactly on k + 1/2, and the exact maps give the same coordinate in fp32 and fp64 on every plane they run on;
(4) every drawn map keeps its excluded band within the cap from the fp64 coordinates alone; (5) the restatements are the host functions
of rpnet_amd/utils/volume_reader.py (affine_sample, gamma_apply + transform_apply, elastic_apply with scipy): on every pixel of the
power-of-two planes for the exact maps, outside the band elsewhere, interpolated values within the calibrations of tests/augment_cases.py.
A defect the checks cannot see means the checks are changed, not the list — with one exception that is stated, not hidden: leaving out the
power law's fp32 round trip changes no output of a slice in [-1, 1] (RC.UNOBSERVABLE carries the proof and its assumptions), so no check
could be written for it; test_the_round_trip_cannot_be_seen_in_an_output holds the identity instead."""
import os
import re

import numpy as np
import pytest
import torch

from rpnet_amd.utils import volume_reader as VR
from tests import augment_cases as AC
from tests import augment_ref_cases as RC

SIM = RC.SimBackend()
F32, F64 = np.float32, np.float64


def run(family, rows, check):
    recs = []
    for row in rows:
        recs += check(SIM, *row)
    RC.hold(recs, verbose=False)
    arith = [r for r in recs if not r.exact]
    if arith:
        top = max(arith, key=lambda r: r.multiple)
        print(f"{family}: {len(rows)} rows, {len(recs)} checks, closest to its bound: {top.family} {top.what} at {top.multiple:.3f} of it")
    return recs


def test_tables_hold_what_they_are_there_for():
    hw = {h * w for h, w in RC.PLANES}
    assert {1, 255, 256, 257, 1023, 1024, 1025} <= hw and any(h == 1 for h, _ in RC.PLANES) and any(w == 1 for _, w in RC.PLANES)
    for rows in (RC.EXACT_ROWS, RC.MINMAX_ROWS):
        assert {r[0] for r in rows} == set(RC.PLANES) and {r[1] for r in rows} == set(RC.S_VALUES)
    assert {p for p, *_ in RC.RANDOM_ROWS} == set(RC.ODD_PLANES) and {a for *_, a in RC.RANDOM_ROWS} == {"transform", "label"}
    for p in RC.PLANES:                                                # every map on every plane, every pair somewhere
        assert {RC.MAP_NAMES[(first + s) % 8] for q, S, first, _ in RC.EXACT_ROWS if q == p for s in range(S)} == set(RC.EXACT_MAPS)
    assert {r[3] for r in RC.EXACT_ROWS} == set(RC.PAIRS) == {r[2] for r in RC.IMAGE_ROWS}
    assert {c for c, *_ in RC.IMAGE_ROWS} == set(RC.IMAGE_CASES)
    assert RC.BIG_S[0] == 65535 and RC.BIG_S[0] * RC.BIG_S[1] * RC.BIG_S[2] == 196605
    for rows in (RC.FIELD_ROWS, RC.ELASTIC_CRAFTED, RC.ELASTIC_RANDOM):
        sizes = {r[0][0] * r[0][1] for r in rows}
        assert min(sizes) < 256 and any(256 < s < 1024 for s in sizes) and max(sizes) > 1024 and any(s % 256 for s in sizes)
    assert {r[3] for r in RC.FIELD_ROWS} == {1.0, 1000.0} and {r[1][0] for r in RC.FIELD_ROWS} == {"one", "r1", "gauss"}
    assert {(p, w) for p, w, *_ in RC.FIELD_ROWS} >= {((3, 5), ("gauss", 30)), ((1, 7), ("gauss", 30)), ((37, 19), ("gauss", 30)), ((41, 25), ("gauss", 2))}
    assert RC.field_weights(("gauss", 30))[1] == 120
    for rows in (RC.ELASTIC_CRAFTED, RC.ELASTIC_RANDOM):
        assert {r[-2] for r in rows} == {-1.0, 0.25} and {r[-1] for r in rows} == set(RC.TRIPLES) and {r[1] for r in rows} == {1, 3}
    assert {r[3] for r in RC.ELASTIC_CRAFTED} == set(RC.FIELDS) and {r[2] for r in RC.ELASTIC_CRAFTED} == set(RC.MINV)
    img, mask = RC.elastic_inputs((17, 15), 3, 0, True)
    assert not mask[1].any() and mask[0].any() and mask[2].any()
    # the crafted fields land where they say: exactly on n-1 and 2^-20 past it, exactly on 0 and 2^-20 before it
    for name, edge in (("ramp_top", 14.0), ("ramp_bottom", 0.0)):
        _, (cy, cx) = RC.elastic_coords(RC.MINV6, RC.crafted_field(name, (17, 15)), 17, 15)
        d = np.unique(cx - edge)
        assert set(np.abs(d).tolist()) == {0.0, 2.0 ** -20}, (name, d)
        assert (cy == (16.0 if name == "ramp_top" else 0.0)).any() and (np.abs(cy - (16.0 if name == "ramp_top" else 0.0)) == 2.0 ** -20).any()


def test_exact_maps_have_one_coordinate_in_fp32_and_fp64():
    """on every plane of the tables, for the eight maps: the fma chain in fp32 and the plain fp64 sum are the same numbers"""
    for plane in RC.PLANES + [(33, 64), RC.BIG_S[1:], RC.PRODUCTION[1:]]:
        t = RC.table(list(RC.EXACT_MAPS.values()))
        fy, fx = RC.affine_coords32(t, *plane)
        cy, cx = RC.affine_coords64(t, *plane)
        assert np.array_equal(fy.astype(F64), cy) and np.array_equal(fx.astype(F64), cx), plane


def test_tie_cases_meet_their_share():
    assert {m for m, _ in RC.TIE_CASES} == {"half_shift", "zoom2", "shrink", "shear"}
    run_on = {(RC.MAP_NAMES[(first + s) % 8], p) for p, S, first, _ in RC.EXACT_ROWS for s in range(S)}
    for name, plane in RC.TIE_CASES:
        share = RC.tie_share(name, plane)
        print(f"tie share {name} {plane}: {share:.1%}")
        assert share >= RC.TIE_SHARE, (name, plane, share)
        assert (name, plane) in run_on
    assert RC.tie_share("id", (37, 19)) == 0 and RC.tie_share("half_shift", (37, 19)) == 1


def test_drawn_maps_stay_within_the_band_cap():
    """from the fp64 coordinates alone: change the seed of a row that breaks it, never the cap"""
    for plane, S, seed, args in RC.RANDOM_ROWS:
        for s, m in enumerate(RC.random_maps(plane, S, seed, args)):
            share = RC.band_of(m, *plane)[2].mean()
            print(f"band share {plane} {args} seed {seed} slice {s}: {share:.3%}")
            assert share <= RC.BAND_CAP, (plane, args, seed, s, share)


def test_minmax_rows():
    run("minmax", RC.MINMAX_ROWS, RC.check_minmax)


def test_affine_rows():
    run("affine exact", RC.EXACT_ROWS, RC.check_affine_exact)
    run("affine drawn", RC.RANDOM_ROWS, RC.check_affine_random)
    RC.hold(RC.check_big_s(SIM), verbose=False)


def test_image_rows():
    run("image", RC.IMAGE_ROWS, RC.check_image)
    # the round trip does make a zero of a value that was not one, in the case that is there for it
    img, params = RC.image_inputs("near_minimum", (37, 19))
    u = (img + F32(1)) / F32(2)
    lo, hi = u.min(axis=(1, 2), keepdims=True), u.max(axis=(1, 2), keepdims=True)
    g = params[:, 6][:, None, None]
    before, after = RC.power_law(u, lo, hi, g, round_trip=False), RC.power_law(u, lo, hi, g)
    assert ((before != 0) & (after == 0)).any() and (u[u > 0].min() < 3e-8)


def test_field_rows():
    run("field", RC.FIELD_ROWS, RC.check_field)


def test_elastic_rows():
    run("elastic crafted", RC.ELASTIC_CRAFTED, RC.check_elastic_crafted)
    run("elastic drawn", RC.ELASTIC_RANDOM, RC.check_elastic_random)


def test_refusal_table_is_well_formed():
    rows, outputs = RC.refusals(lambda n: torch.full((n,), 7.0), lambda n: torch.full((n,), 7.0, dtype=torch.float64))
    assert {e for _, e, *_ in rows} == {"rpnet_slice_minmax", "rpnet_augment_affine", "rpnet_elastic_field", "rpnet_elastic_apply"}
    assert {c for *_, c, _ in rows} == {RC.SHAPE, RC.ARG} and len(rows) >= 60
    from rpnet_amd import hip
    for _, entry, args, _, words in rows:
        assert len(args) + 1 == len(hip._SIGS[entry][1]) and words, entry
    src = open(os.path.join(os.path.dirname(os.path.abspath(hip.__file__)), "csrc", "augment.hip")).read()
    # the pinned words are those of a message of THAT entry point (or of the shared plane check): its string literals, formats as wildcards
    literals = re.findall(r'"((?:[^"\\]|\\.)*)"', src)
    for _, entry, _, _, words in rows:
        own = [lit for lit in literals if lit.startswith(entry[len("rpnet_"):] + ":") or lit.startswith("%s:")]
        assert own and any(re.search(re.sub(r"%[ds]", ".*", re.escape(words.split(" ")[0] if words.startswith("radius") else words)), lit)
                           for lit in own), (entry, words)


# ----------------------------------------------------------------------------------------------- against the host functions
def _host_affine(x, m):
    return VR.affine_sample(torch.from_numpy(np.ascontiguousarray(x))[None, None], list(m))[0, 0].numpy()


def test_affine_restatement_is_the_host_sampling():
    """affine_sample (torch's normalised grid): every pixel on the power-of-two planes for the exact maps, outside the band elsewhere"""
    for plane in RC.POW2_PLANES:
        lab = RC.coded_labels(1, *plane)
        for name, m in RC.EXACT_MAPS.items():
            _, want = RC.ref_affine(None, lab, RC.table([m]), None, *plane)
            assert np.array_equal(_host_affine(lab[0], m), want[0]), (plane, name)
    differ = 0
    for plane in RC.ODD_PLANES + [(64, 48)]:
        lab = RC.coded_labels(1, *plane)
        for name, m in RC.EXACT_MAPS.items():
            _, want = RC.ref_affine(None, lab, RC.table([m]), None, *plane)
            _, _, band = RC.band_of(m, *plane)
            host = _host_affine(lab[0], m)
            assert np.array_equal(host[~band], want[0][~band]), (plane, name)
            differ += int((host != want[0]).sum())
    print(f"pixels of the exact maps on planes that are no power of two where torch's grid lands on the other side of a tie: {differ}")
    for plane, S, seed, args in RC.RANDOM_ROWS:
        lab = RC.coded_labels(1, *plane)
        for m in RC.random_maps(plane, S, seed, args):
            _, want = RC.ref_affine(None, lab, RC.table([m]), None, *plane)
            _, _, band = RC.band_of(m, *plane)
            assert np.array_equal(_host_affine(lab[0], m)[~band], want[0][~band]), (plane, seed, args)


def test_image_restatement_is_gamma_apply_and_transform_apply():
    """within 4 x the host's own fp32-against-fp64 change of the power law (the calibration of tests/test_gpu_augment.py); law off: equal"""
    for case in RC.IMAGE_CASES:
        for plane in RC.POW2_PLANES[:2] + [(37, 19)]:
            img, params = RC.image_inputs(case, plane)
            mm = RC.ref_minmax(img)
            want, _ = RC.ref_affine(img, None, params, mm, *plane)
            for s in range(img.shape[0]):
                on, gamma, m = params[s, 7] != 0, F32(params[s, 6]), params[s, :6].tolist()
                q = VR.gamma_apply(img[s], gamma) if on else img[s]
                host, _ = VR.transform_apply(torch.from_numpy(q.copy())[None, None], torch.zeros(1, *plane), m)
                host = host[0, 0].numpy()
                calib = np.abs(AC.intensity_formula(img[s], gamma if on else None, F32).astype(F64) - AC.intensity_formula(img[s], gamma if on else None, F64)).max()
                band = RC.band_of(m, *plane)[2] if plane == (37, 19) else np.zeros(plane, bool)
                err = np.abs(host - want[s])[~band].max(initial=0.0)
                assert err <= 4 * calib, (case, plane, s, err, calib)


def test_field_restatement_is_scipy():
    from scipy.ndimage import gaussian_filter
    for plane, sigma in [((3, 5), 30), ((37, 19), 30), ((41, 25), 2), ((1, 7), 30)]:
        noise = RC.field_noise(plane, "random")[0]
        w, r = RC.field_weights(("gauss", sigma))
        tmp, field = RC.ref_field(noise, w, r, 1000.0)
        want = np.stack([gaussian_filter(noise[c], sigma) * 1000 for c in range(2)])
        assert np.abs(field - want).max() <= 2e-12 * 1000 + np.spacing(np.abs(want).astype(F32)).max(), (plane, sigma)


def test_elastic_restatement_is_elastic_apply():
    """elastic_apply of the host reader (scipy map_coordinates) with the same Minv and a field that gaussian_filter(sigma -> 0) leaves as
    it is: masks equal, images within 4 x the host's own change under fp32 coordinates (tests/augment_cases.py)"""
    from scipy.ndimage import map_coordinates
    for plane, S, seed, pad, _ in RC.ELASTIC_RANDOM:
        H, W = plane
        img, mask = RC.elastic_inputs(plane, S, seed, False)
        minv, field = RC.elastic_random_inputs(plane, S, seed)
        (sy, sx), (cy, cx) = RC.elastic_coords(minv, field, H, W)
        i1, m1 = RC.ref_stage1(img, mask, minv, H, W, pad)
        i2, m2 = RC.ref_stage2(i1.astype(F32), m1, field, H, W, pad)
        for z in range(S):
            a = map_coordinates(img[z], (sy, sx), order=1, mode="constant", cval=pad)
            h_img = map_coordinates(a, (cy, cx), order=1, mode="constant", cval=pad)
            a32 = map_coordinates(img[z], (sy.astype(F32), sx.astype(F32)), order=1, mode="constant", cval=pad)
            calib = np.abs(map_coordinates(a32, (cy.astype(F32), cx.astype(F32)), order=1, mode="constant", cval=pad) - h_img).max()
            assert np.abs(i2[z] - h_img).max() <= 4 * calib, (plane, seed, z)
            k = map_coordinates(mask[z], (np.rint(sy), np.rint(sx)), order=0, mode="constant", cval=0)
            h_msk = map_coordinates(k, (cy, cx), order=0, mode="constant")
            edge = (np.abs(cy) < AC.BAND) | (np.abs(cy - (H - 1)) < AC.BAND) | (np.abs(cx) < AC.BAND) | (np.abs(cx - (W - 1)) < AC.BAND)
            assert np.array_equal(m1[z], k) and np.array_equal(m2[z][~edge], h_msk[~edge]), (plane, seed, z)
    # and through VR.elastic_apply itself with the identity field (noise 0): stage 1 alone
    plane = (37, 19)
    img, mask = RC.elastic_inputs(plane, 3, 1, False)
    minv, _ = RC.elastic_random_inputs(plane, 3, 1)
    h_img, h_msk = VR.elastic_apply(img[None], mask[None], minv.reshape(2, 3), np.zeros((2,) + plane))
    i1, m1 = RC.ref_stage1(img, mask, minv, *plane, -1.0)
    i2, m2 = RC.ref_stage2(i1.astype(F32), m1, np.zeros((2,) + plane, F32), *plane, -1.0)
    assert np.abs(i2 - h_img[0]).max() <= 2.0 ** -23 and np.array_equal(m2, h_msk[0])


def test_the_round_trip_cannot_be_seen_in_an_output():
    """the one change of the issue's list that no row can fail (RC.UNOBSERVABLE): fl(2 RT(v) - 1) == fl(2 v - 1) for every v of [0, 1],
    and RT(v) == 0 exactly where fl(2 v - 1) == -1, so a pixel that becomes zero and takes `lo` is -1 either way"""
    rs = np.random.RandomState(0)
    v = np.concatenate([rs.rand(1 << 20), rs.rand(1 << 18) * 2.0 ** -20, 2.0 ** -rs.randint(1, 60, 4096), [0.0, 1.0, 0.25, 0.5]]).astype(F32)
    v = np.concatenate([v, np.nextafter(v, F32(0)), np.nextafter(v, F32(1))])
    rt = ((v * F32(2) - F32(1)) + F32(1)) / F32(2)
    assert np.array_equal(rt * F32(2) - F32(1), v * F32(2) - F32(1))
    assert np.array_equal(rt == 0, v * F32(2) - F32(1) == -1) and ((rt == 0) & (v != 0)).any()
    for case, plane in (("near_minimum", (37, 19)), ("gammas", (41, 25)), ("min_is_minus_one", (3, 5))):
        img, params = RC.image_inputs(case, plane)
        mm = RC.ref_minmax(img)
        a, _ = RC.ref_affine(img, None, params, mm, *plane)
        b, _ = RC.ref_affine(img, None, params, mm, *plane, defect="no_round_trip")
        assert np.array_equal(RC.bits(a), RC.bits(b)), case


# -------------------------------------------------------------------------------------------------------- seeded defects
# the rows each defect is looked for in: the smallest of the tables that can show it
DEFECT_CASES = {
    "affine_half_up": lambda be: RC.check_affine_exact(be, (37, 19), 7, 0, "both"),
    "last_block_unwritten": lambda be: RC.check_affine_exact(be, (17, 15), 1, 7, "both") + RC.check_affine_exact(be, (41, 25), 2, 3, "lab"),
    "params_slice0": lambda be: RC.check_affine_exact(be, (3, 5), 2, 3, "lab"),
    "mm_slice0": lambda be: RC.check_image(be, "gammas", (37, 19), "both") + RC.check_affine_exact(be, (3, 5), 3, 5, "img"),
    "minmax_first_1024": lambda be: RC.check_minmax(be, (41, 25), *[r[1:] for r in RC.MINMAX_ROWS if r[0] == (41, 25) and r[2] == "extremes_last"][0]),
    "lo_without_law": lambda be: RC.check_image(be, "all_fill", (3, 5), "both") + RC.check_image(be, "min_is_minus_one", (37, 19), "both"),
    "law_without_1e5": lambda be: RC.check_image(be, "gammas", (37, 19), "both"),
    "inside_lt": lambda be: RC.check_affine_exact(be, (3, 5), 7, 0, "both"),
    "centre_w_both": lambda be: RC.check_affine_exact(be, (37, 19), 7, 0, "lab"),
    "flag_eq_1": lambda be: RC.check_image(be, "flag_other", (3, 5), "both"),
    "reflect_period_n": lambda be: RC.check_field(be, (3, 5), ("gauss", 30), "impulses", 1.0),
    "reflect_mirror": lambda be: RC.check_field(be, (37, 19), ("r1",), "impulses", 1.0),
    "blur_same_axis": lambda be: RC.check_field(be, (3, 5), ("gauss", 30), "random", 1000.0),
    "field_swapped": lambda be: RC.check_elastic_crafted(be, (17, 15), 1, "identity", "dx_dy_differ", -1.0, "both"),
    "blend_with_constant": lambda be: RC.check_elastic_crafted(be, (17, 15), 1, "identity", "ramp_top", 0.25, "both"),
    "stage2_rint": lambda be: RC.check_elastic_crafted(be, (17, 15), 1, "identity", "plus_half", 0.25, "both"),
    "stage1_floor_half": lambda be: RC.check_elastic_crafted(be, (17, 15), 1, "half", "zero", -1.0, "both"),
    "stage2_reads_input": lambda be: RC.check_elastic_crafted(be, (17, 15), 3, "shift", "dx_dy_differ", -1.0, "both"),
    "pad_fixed": lambda be: RC.check_elastic_crafted(be, (17, 15), 1, "partly_outside", "zero", 0.25, "both"),
}


def test_every_defect_has_its_cases():
    assert sorted(DEFECT_CASES) == sorted(RC.DEFECTS) and len(RC.DEFECTS) + len(RC.UNOBSERVABLE) >= 17


@pytest.mark.parametrize("defect", RC.DEFECTS)
def test_seeded_defect_fails_the_checks(defect):
    RC.hold(DEFECT_CASES[defect](SIM), verbose=False)                     # the same rows pass without the defect
    with np.errstate(all="ignore"):
        recs = DEFECT_CASES[defect](RC.SimBackend(defect))
    bad = [r for r in recs if not r.ok]
    assert bad, f"{defect}: no check failed"
    print(f"DEFECT {defect}: {len(bad)} of {len(recs)} checks fail: " + "; ".join(f"{r.family} {r.what} ({r.err:.3g})" for r in bad[:3]))
    with pytest.raises(AssertionError):
        RC.hold(recs, verbose=False)
