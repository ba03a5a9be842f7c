"""The DEEDS registration entry points (include/rpnet_deeds_abi.h, csrc/deeds.hip, rpnet_amd/registration.py) on the MI355X against the
float64 restatement of tests/deeds_cases.py under its comparison rule, against the reference's own run (tests/golden/
registration_deeds.npz), and through the readers, sources and drivers with `do_deformable: deeds`."""
import random
import sys

import numpy as np
import pytest
import torch

from rpnet_amd import hip
from rpnet_amd import registration as R
from tests import deeds_cases as DC
from tests.test_host_deeds import FIXTURE_CASES, fixture_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64          # floats behind every output


class HipBackend:
    """the entry points through rpnet_amd.registration; every call is made twice and the two results must be the same bits"""

    def register(self, moving, fixed, G, D, Rr, alpha):
        m, f = moving.to(DEV), fixed.to(DEV)
        pred, cost = R.deeds_register(m, f, G, Rr, D, alpha, return_cost=True)
        pred2, cost2 = R.deeds_register(m, f, G, Rr, D, alpha, return_cost=True)
        alone = R.deeds_register(m, f, G, Rr, D, alpha)
        assert torch.equal(pred, pred2) and torch.equal(cost, cost2) and torch.equal(pred, alone)
        return pred.cpu(), cost.cpu()

    def warp(self, x, pred, mode, threshold=-1.0, scale=1.0, shift=0.0):
        xd, pd = x.to(DEV), pred.to(DEV)
        out = R.deeds_warp(xd, pd, mode, threshold, scale, shift)
        assert torch.equal(out, R.deeds_warp(xd, pd, mode, threshold, scale, shift))
        return out.cpu()


@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_id)
def test_pred_and_cost_against_float64(case):
    """rpnet_deeds_register (pred and cost_out) and rpnet_deeds_warp on every row of the table"""
    DC.hold(DC.check_case(HipBackend(), case))


@pytest.mark.parametrize("shape", DC.WARP_SHAPES, ids=str)
def test_deeds_warp_against_float64_grid_sample(shape):
    """rpnet_deeds_warp on given random pred tensors: both modes, plain, scaled and shifted, thresholded"""
    DC.hold(DC.check_warps(HipBackend(), shape))


@pytest.mark.parametrize("tag", FIXTURE_CASES)
def test_fixture_cases_through_deeds_register(tag):
    """the reference's stored affine-warped image through deeds_register and deeds_warp: pred, sample grid (read back by warping the
    two coordinate images is not needed: the grid is grid + pred at the nearest index) and warped source under the rule, the label equal
    outside the exempt pixels"""
    fx, mov, fix, src, lab = fixture_inputs(tag)
    G, D = fx["G"], fx["D"]
    pred64, _ = DC.deeds_ref(mov, fix, G, D, 0.1, DC.DEF, DC.F64)
    pred = R.deeds_register(mov.to(DEV), fix.to(DEV), G, 0.1, D).cpu()
    recs = [DC.small_record(tag + " pred", pred, pred64, fx["pred_xyz"])]
    from tests.test_host_deeds import affine_warped
    aw_lab = affine_warped(lab, fx["theta"])
    given = fx["pred_xyz"]
    wsrc = R.deeds_warp(mov.to(DEV), given.to(DEV), scale=2.0, shift=-1.0).cpu()
    recs += DC.warp_records(tag + " warped_src", wsrc, mov, given, "nearest", DC.POSTS[1])
    reg = R.deeds_warp(aw_lab.to(DEV), given.to(DEV), threshold=0.1).cpu()
    recs += DC.warp_records(tag + " reg_pred", reg, aw_lab, given, "nearest", DC.POSTS[2])
    DC.hold(recs)
    assert torch.equal(reg, fx["reg_pred"].float())
    assert (wsrc - fx["warped_src"]).abs().max().item() <= 8 * DC.ULP * 2


def test_recovers_a_constructed_shift():
    """moving = fixed moved by (2, -1) displacement steps, alpha5 = 200: the margin is asserted on the float64 reference
    (tests/test_host_deeds.py::test_recovery_case_has_its_margin asserts it without a GPU too), then the device's pred is that shift
    to within half a step at the interior points"""
    mov, fix, Rr = DC.recovery_pair()
    G, D, b = DC.REC["G"], DC.REC["D"], DC.REC["border"]
    _, cost = DC.deeds_ref(mov, fix, G, D, Rr, DC.REC["alpha"], DC.F64)
    kx, ky = DC.REC["px"]
    best = (ky + D // 2) * D + (kx + D // 2)
    inner = torch.zeros(G, G, dtype=torch.bool)
    inner[b:G - b, b:G - b] = True
    c = cost[0][inner.reshape(-1)]
    others = torch.cat([c[:, :best], c[:, best + 1:]], 1).min(1).values
    assert (others - c[:, best]).min().item() >= DC.recovery_margin_needed()
    pred = R.deeds_register(mov.to(DEV), fix.to(DEV), G, Rr, D, DC.REC["alpha"]).cpu()
    step = DC.f32(Rr) * 2 / D
    err = (pred[0][inner].double() - torch.tensor([kx * step, ky * step], dtype=torch.float64)).abs().max().item()
    print(f"largest error at the interior points: {err / step:.4f} steps")
    assert err < 0.5 * step


def _guarded(n, fill=float("nan")):
    t = torch.full((n + GUARD,), fill, device=DEV, dtype=torch.float32)
    t[n:] = 12345.0
    return t


@pytest.mark.parametrize("alpha", [DC.DEF, DC.GEN], ids=["alpha3=0", "alpha3!=0"])
def test_outputs_and_workspace_prefilled_with_nan_and_guarded(alpha):
    """rpnet_deeds_register and rpnet_deeds_warp called directly: outputs and workspace start as NaN, the words behind each are left
    alone, the results are those of the Python layer, and a second call gives the same bits"""
    S, H, W, G, D = 3, 33, 65, 2 * DC.TILE + 2, 7
    mov, fix = DC.image_pair((S, H, W), 31, "smooth")
    m, f = mov.to(DEV), fix.to(DEV)
    general = int(alpha[3] != 0)
    wb = hip.query("rpnet_deeds_workspace_bytes", S, G, D, general)
    assert wb == (S * G * G * D * D * 4 if general else 0)
    p = hip.ptr
    gb, sb = R.base_grid(G, DEV), R.base_grid(D, DEV)
    runs = []
    for _ in range(2):
        pred, cost, ws, out = _guarded(S * G * G * 2), _guarded(S * G * G * D * D), _guarded(wb // 4), _guarded(S * H * W)
        hip.call("rpnet_deeds_register", p(m), p(f), p(gb), p(sb), S, H, W, G, D, 0.1, *alpha, p(pred), p(cost), p(ws) if wb else None, wb)
        hip.call("rpnet_deeds_warp", p(m), p(pred), p(gb), p(out), S, H, W, G, 1, -1.0, 2.0, -1.0)
        torch.cuda.synchronize()
        for t in (pred, cost, ws, out):
            assert (t[-GUARD:] == 12345.0).all() and torch.isfinite(t).all()
        runs.append((pred[:-GUARD].clone(), cost[:-GUARD].clone(), out[:-GUARD].clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    want_pred, want_cost = R.deeds_register(m, f, G, 0.1, D, alpha, return_cost=True)
    assert torch.equal(runs[0][0], want_pred.reshape(-1)) and torch.equal(runs[0][1], want_cost.reshape(-1))
    assert torch.equal(runs[0][2], R.deeds_warp(m, want_pred, "bilinear", scale=2.0, shift=-1.0).reshape(-1))


def test_captured_graph_of_register_and_warp_replayed():
    """deeds_register + deeds_warp captured once (both alpha3 settings in one graph) and replayed twice on new inputs"""
    S, H, W, G, D = 2, 48, 48, 24, 7
    pairs = [DC.image_pair((S, H, W), 50 + k, "smooth") for k in range(3)]
    m, f = pairs[0][0].to(DEV), pairs[0][1].to(DEV)
    eager = []
    for mov, fix in pairs:
        pa = R.deeds_register(mov.to(DEV), fix.to(DEV), G, 0.1, D)
        pb = R.deeds_register(mov.to(DEV), fix.to(DEV), G, 0.1, D, DC.GEN)
        eager.append((pa, pb, R.deeds_warp(mov.to(DEV), pa, threshold=0.1), R.deeds_warp(mov.to(DEV), pb, "bilinear")))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            pa = R.deeds_register(m, f, G, 0.1, D)
            pb = R.deeds_register(m, f, G, 0.1, D, DC.GEN)
            outs = (pa, pb, R.deeds_warp(m, pa, threshold=0.1), R.deeds_warp(m, pb, "bilinear"))
    for k in (1, 2):
        m.copy_(pairs[k][0])
        f.copy_(pairs[k][1])
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager[k]):
            assert torch.equal(got, want), k


def test_refusals_launch_nothing():
    """every refusal of rpnet_deeds_register, rpnet_deeds_warp and rpnet_deeds_workspace_bytes, with its message"""
    S, H, W, G, D = 1, 16, 16, 8, 5
    x = torch.rand(S, H, W, device=DEV)
    pred = torch.full((S, G, G, 2), 7.0, device=DEV)
    gb, sb = R.base_grid(G, DEV), R.base_grid(D, DEV)
    p = hip.ptr
    ws = torch.empty(1 << 20, device=DEV, dtype=torch.uint8)

    def reg(moving=x, fixed=x, g=gb, s=sb, S=S, H=H, W=W, G=G, D=D, Rr=0.1, alpha=DC.DEF, out=pred, ws_=ws, wb=1 << 20):
        hip.call("rpnet_deeds_register", p(moving), p(fixed), p(g), p(s), S, H, W, G, D, Rr, *alpha, p(out), None, p(ws_), wb)

    def warp(x_=x, pr=pred, g=gb, out=x, S=S, H=H, W=W, G=G, mode=0):
        hip.call("rpnet_deeds_warp", p(x_), p(pr), p(g), p(out), S, H, W, G, mode, -1.0, 1.0, 0.0)

    for kw in (dict(moving=None), dict(fixed=None), dict(g=None), dict(s=None), dict(out=None)):
        with pytest.raises(RuntimeError, match="deeds_register: null pointer"):
            reg(**kw)
    for kw, msg in [(dict(S=-1), "S=-1 H=16 W=16"), (dict(H=1), "S=1 H=1 W=16"), (dict(W=1), "S=1 H=16 W=1"),
                    (dict(H=32768, W=32768), "S=1 H=32768 W=32768"),
                    (dict(G=0), r"G=0 D=5 \(G 1..512, D odd 1..31\)"), (dict(G=513), "G=513 D=5"), (dict(D=4), "G=8 D=4"),
                    (dict(D=33), "G=8 D=33"), (dict(D=0), "G=8 D=0"), (dict(D=-1), "G=8 D=-1")]:
        with pytest.raises(RuntimeError, match="deeds_register: " + msg):
            reg(**kw)
    for kw in (dict(Rr=float("nan")), dict(Rr=float("inf")), dict(alpha=(1, .1, 1, 0, .1, float("inf"))), dict(alpha=(float("nan"), .1, 1, 0, .1, 10))):
        with pytest.raises(RuntimeError, match="deeds_register: disp_range or alpha is not finite"):
            reg(**kw)
    need = G * G * D * D * 4
    with pytest.raises(RuntimeError, match=f"deeds_register: workspace of {need - 1} bytes, {need} needed"):
        reg(alpha=DC.GEN, wb=need - 1)
    with pytest.raises(RuntimeError, match=f"deeds_register: workspace of 0 bytes, {need} needed"):
        reg(alpha=DC.GEN, ws_=None)
    for kw in (dict(x_=None), dict(pr=None), dict(g=None), dict(out=None)):
        with pytest.raises(RuntimeError, match="deeds_warp: null pointer"):
            warp(**kw)
    for kw, msg in [(dict(S=-1), "S=-1 H=16 W=16"), (dict(H=1), "S=1 H=1 W=16"), (dict(G=0), r"G=0 \(1..512\)"), (dict(G=513), "G=513"),
                    (dict(mode=2), r"mode=2 \(0 nearest, 1 bilinear\)"), (dict(mode=-1), "mode=-1")]:
        with pytest.raises(RuntimeError, match="deeds_warp: " + msg):
            warp(**kw)
    lib = hip.load()
    for bad in ((-1, 8, 5), (1, 0, 5), (1, 513, 5), (1, 8, 4), (1, 8, 33)):
        assert hip.query("rpnet_deeds_workspace_bytes", *bad, 1) == 0
        assert lib.rpnet_last_error_string().decode().startswith("deeds_workspace_bytes: S=%d G=%d D=%d" % bad)
    # S = 0 is RPNET_OK, with or without a workspace; a3 == 0 needs none
    reg(S=0)
    reg(S=0, alpha=DC.GEN, ws_=None, wb=0)
    warp(S=0)
    reg(ws_=None, wb=0)
    with pytest.raises(ValueError, match="deeds_warp: mode"):
        R.deeds_warp(x, pred, "cubic")
    with pytest.raises(ValueError, match="displacement_width=4"):
        R.deeds_register(x, x, 8, 0.1, 4)
    with pytest.raises(RuntimeError, match="MI355X only"):
        R.deeds_register(x.cpu(), x.cpu())
    torch.cuda.synchronize()
    assert (pred[..., 0] != 7.0).all()           # the last, accepted call wrote it; nothing before it did
    assert torch.isfinite(pred).all()


def _episode(seed, S, size):
    from rpnet_amd.utils.synth import make_episode
    ep = make_episode(seed, S, size)
    src = torch.from_numpy((ep["support_images"][0][0][:, 0] + 1) / 2.0).float().to(DEV)
    dst = torch.from_numpy((ep["query_images"][:, 0] + 1) / 2.0).float().to(DEV)
    return src, dst, torch.from_numpy(ep["support_fg"][0][0]).float().to(DEV)


def test_register_slices_deeds_is_the_entry_points_composed():
    """register_slices(..., "deeds") bit for bit against the functions composed by hand; True and False give what the branches they
    always took give; get_registration_field packs (theta, pred); the classes of net.registration run the same launches"""
    src, dst, lab = _episode(91, 3, 64)
    theta, _ = R.affine_register(src, dst)
    aw_lab, aw_src = R.affine_warp(lab, theta), R.affine_warp(src, theta)
    pred = R.deeds_register(aw_src, dst)
    want = ((theta, pred), R.deeds_warp(aw_lab, pred, threshold=0.1), R.deeds_warp(aw_src, pred, scale=2.0, shift=-1.0),
            R.affine_warp(lab, theta, threshold=0.1), R.affine_warp(src, theta, scale=2.0, shift=-1.0))
    got = R.register_slices(src, dst, lab, "deeds")
    assert torch.equal(got[0][0], theta) and torch.equal(got[0][1], pred) and tuple(pred.shape) == (3, 128, 128, 2)
    for g, w in zip(got[1:], want[1:]):
        assert torch.equal(g, w)
    assert set(got[1].unique().tolist()) <= {0.0, 1.0} and got[1].sum() > 100 and pred.abs().max() > 1e-4
    with pytest.raises(ValueError, match="do_deformable 'demons'"):
        R.register_slices(src, dst, lab, "demons")
    # False: the affine branch, bit for bit
    f_field, f_reg, f_src, f_areg, f_asrc = R.register_slices(src, dst, lab, False)
    assert torch.equal(f_field, theta) and torch.equal(f_reg, R.identity_grid_warp(aw_lab, threshold=0.1))
    assert torch.equal(f_src, R.identity_grid_warp(aw_src, scale=2.0, shift=-1.0)) and torch.equal(f_areg, want[3]) and torch.equal(f_asrc, want[4])
    # True: the demons branch (its backward scatters with fp32 atomics: tests/test_gpu_dataset_eval.py holds two runs to these figures)
    (t_theta, t_flow), t_reg, t_src, t_areg, t_asrc = R.register_slices(src, dst, lab, True)
    flow, disp, _ = R.demons_register(aw_src, dst)
    assert torch.equal(t_theta, theta) and tuple(t_flow.shape) == (3, 2, 64, 64) and (t_flow - flow).abs().max().item() < 5e-3
    assert (t_src - R.displacement_warp(aw_src, disp, scale=2.0, shift=-1.0)).abs().max().item() < 1e-2
    assert torch.equal(t_areg, want[3]) and torch.equal(t_asrc, want[4])
    # the host-facing wrapper and the drop-in classes
    ep_q, ep_s = (dst * 2 - 1)[:, None].cpu(), (src * 2 - 1)[:, None].cpu()
    field, reg, wsrc, areg, asrc = R.get_registration_field(ep_q, [[ep_s]], [[lab.cpu()]], do_deformable="deeds", device=DEV)
    assert isinstance(field, tuple) and tuple(field[1].shape) == (3, 128, 128, 2) and not field[1].is_cuda
    assert tuple(reg.shape) == (3, 1, 64, 64) and isinstance(wsrc, np.ndarray) and wsrc.shape == (3, 64, 64)
    from net.registration import AffineDEEDSRegistration, DEEDSRegistration
    mod = AffineDEEDSRegistration((64, 64))
    mod.train_registraion(src[:, None], dst[:, None])
    assert torch.equal(mod.theta, theta) and torch.equal(mod.deeds.pred_xyz, pred)
    assert torch.equal(mod(src[:, None])[:, 0], R.deeds_warp(aw_src, pred))
    small = DEEDSRegistration(grid_size=24, displacement_width=7, mode="bilinear")
    small.train_registraion(aw_src[:, None], dst[:, None])
    assert torch.equal(small.pred_xyz, R.deeds_register(aw_src, dst, 24, 0.1, 7))
    assert torch.equal(small(lab[:, None])[:, 0], R.deeds_warp(lab, small.pred_xyz, "bilinear"))


def test_readers_sources_and_drivers_with_deeds(tmp_path, capsys, monkeypatch):
    """a tiny synthetic NRRD data set with do_deformable: "deeds": the host reader's eval items equal DeviceEvalSource's bit for bit (the
    same launches on equal inputs, no atomics), a DeviceEpisodeSource item is get_registration_field on its own pre-registration
    tensors, evaluate_dataset runs and differs from the affine setting in its registered figures only, and the eval driver takes
    --registration deeds"""
    from rpnet_amd import dataset_eval as DE
    from rpnet_amd.episodes import DeviceEpisodeSource
    from rpnet_amd.utils import volume_reader as VR
    from tests import augment_cases as AC
    from tests.test_gpu_augment import _dataset as train_dataset
    from tests.test_gpu_dataset_eval import _build_net, _dataset, _eval_cfg, _plain
    data_dir, set_name, cfg = _dataset(tmp_path / "data", do_deformable="deeds")
    host = VR.FewshotRegReader(data_dir, set_name, cfg, mode="eval")
    src = DE.DeviceEvalSource(data_dir, set_name, cfg, DEV)
    src.warm()
    assert R.base_grid.cache_info().currsize >= 3
    for idx in range(len(host)):
        AC.seed_all(40 + idx)
        h = host[idx]
        AC.seed_all(40 + idx)
        d = src.item(idx)
        assert d["pid"] == h["pid"] and d["supp_pids"] == h["supp_pids"]
        for key, got, want in [("support_images", d["support_images"][0][0], h["support_images"][0][0]),
                               ("support_labels", d["support_labels"][0][0], h["support_labels"][0][0]),
                               ("appr_query_labels", d["appr_query_labels"], h["appr_query_labels"]), ("warped_supp", d["warped_supp"], h["warped_supp"])]:
            assert torch.equal(got.cpu(), want), (idx, key)
        (th, pr), (hth, hpr) = d["registration_field"], h["registration_field"]
        assert torch.equal(th.cpu(), hth) and torch.equal(pr.cpu(), hpr) and tuple(pr.shape[1:]) == (128, 128, 2)
    # no host synchronisation after warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        src.item(0)
    finally:
        torch.cuda.set_sync_debug_mode("default")

    tdir, tset, tcfg = train_dataset(tmp_path / "train", do_elastic=False, do_deformable="deeds")
    esrc = DeviceEpisodeSource(tdir, tset, tcfg, DEV)
    esrc.warm()
    AC.seed_all(5)
    d = esrc.item(0)
    pre = esrc.pre
    field, reg, _, aff_pred, aff_src = R.get_registration_field(pre["query_images"].cpu(), [[pre["support_images"].cpu()]],
                                                                [[pre["support_labels"].cpu()]], do_deformable="deeds")
    assert torch.equal(d["registration_field"][0].cpu(), field[0]) and torch.equal(d["registration_field"][1].cpu(), field[1])
    assert torch.equal(d["appr_query_labels"].cpu(), reg[:, 0]) and np.array_equal(d["support_images"][:, 0].cpu().numpy(), aff_src)

    ecfg = _eval_cfg(cfg)
    tables = {}
    random.seed(77)
    capsys.readouterr()
    got = _plain(DE.evaluate_dataset(_build_net(ecfg, "f32"), src, ecfg, batch=8, graphed=False, out=tables))
    assert len(got[1]["Liver"]) == 3 and np.isfinite(tables["ncc"]).all() and tables["counts"].shape[0] == 3
    acfg = dict(ecfg, do_deformable=False)
    asrc = DE.DeviceEvalSource(data_dir, set_name, acfg, DEV)
    atables = {}
    random.seed(77)
    _plain(DE.evaluate_dataset(_build_net(acfg, "f32"), asrc, acfg, batch=8, graphed=False, out=atables))
    assert np.array_equal(tables["ncc"][:, 1], atables["ncc"][:, 1]) and not np.array_equal(tables["ncc"][:, 0], atables["ncc"][:, 0])

    from tools import eval_driver
    import train_rpnet
    assert eval_driver.build_parser().parse_args(["--registration", "deeds"]).registration == "deeds"
    assert eval_driver.build_parser().parse_args([]).registration is None
    assert R.REGISTRATION_STAGES == {"affine": False, "demons": True, "deeds": "deeds"}
    import json
    import yaml
    from tests.helpers import load_cfg
    y = dict(load_cfg(), **cfg)
    y.update(do_deformable=False, data_dir=data_dir, eval_set_name=set_name)
    path = str(tmp_path / "deeds.yml")
    with open(path, "w") as fh:
        yaml.safe_dump(json.loads(json.dumps(y)), fh)
    seen = {}
    real = DE.DeviceEvalSource

    def spy(data_dir_, set_name_, config, *a, **kw):
        seen["do_deformable"] = config.get("do_deformable")
        return real(data_dir_, set_name_, config, *a, **kw)
    monkeypatch.setattr(DE, "DeviceEvalSource", spy)
    monkeypatch.setattr(sys, "argv", ["eval_driver.py", "--yaml", path, "--device-items", "--items", "1", "--registration", "deeds"])
    capsys.readouterr()
    eval_driver.main()
    assert seen == {"do_deformable": "deeds"} and "Liver" in capsys.readouterr().out
    monkeypatch.setattr(sys, "argv", ["train_rpnet.py", "--registration", "none"])
    with pytest.raises(SystemExit):
        train_rpnet.main()
    assert "--registration" in capsys.readouterr().err
