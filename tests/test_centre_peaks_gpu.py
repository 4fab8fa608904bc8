"""GPU checks of the translation hypotheses from further centre-vote peaks (VotingPipeline.vote(centre_peaks=C), eval.py
--centre_peaks): the pipeline's state after the call, each peak's re-vote against the public stages run by hand, the constructed
case where the first maximum of the grid is a decoy and a later peak is the true centre, and eval.py end to end."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import grid_peaks_ref as GR  # noqa: E402

FIXTURE = os.path.join(GOLDEN, "example_data", "obj_000015.ply")
STATE = ("results", "counts", "top_idx", "top_cnt", "kept_count", "kept_tuple", "argmax", "peak", "world", "mask", "kept_wt",
         "kept_row0", "errs", "thr")


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _batch(dev, seed=9):
    import torch
    from cppf2_amd import ops, synth
    Ns, Ts = [900, 2048, 300, 1500, 4096, 700], [4000, 9000, 1500, 6000, 12000, 2500]
    scs = [synth.make_scene(seed, b, n) for b, n in enumerate(Ns)]
    pts = torch.from_numpy(np.concatenate([s["pc"] for s in scs])).to(dev)
    idx = torch.cat([ops.sample_tuples(n, t, 5, seed, (b,)) for b, (n, t) in enumerate(zip(Ns, Ts))])
    lg = torch.cat([torch.from_numpy(synth.teacher_logits(s["pc_canon"], idx[sum(Ts[:b]):sum(Ts[:b + 1])].cpu().numpy(), 32))
                    for b, s in enumerate(scs)]).to(dev)
    u = torch.cat([ops.philox_uniform(t, 6, seed, 1, (b,)) for b, t in enumerate(Ts)])
    scales = torch.from_numpy(np.random.default_rng(seed).random((sum(Ts), 3)).astype(np.float32)).to(dev)
    return Ns, Ts, pts, idx, lg, u, scales


def _snap(pipe, names=STATE):
    return {k: getattr(pipe, k).cpu().numpy().tobytes() for k in names}


def test_state_after_the_call_is_the_default_calls():
    """vote(centre_peaks=3) leaves every buffer byte for byte as vote() does, centre_results[0] equals results, and a callable
    pred_scales is evaluated once per peak."""
    dev = _gpu()
    from cppf2_amd.pipeline import VotingPipeline
    Ns, Ts, pts, idx, lg, u, scales = _batch(dev)
    import torch
    a = VotingPipeline(Ns, Ts, num_rots=90)
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    a.vote(pts, idx, lg, u, scales)
    torch.cuda.synchronize()
    # the default call allocates no grid buffer (nothing as large as one scene's grid); centre_peaks=3 below allocates B of them
    assert torch.cuda.memory_allocated() - m0 < a.cells_cap * 4
    want = _snap(a)
    b = VotingPipeline(Ns, Ts, num_rots=90)
    m0 = torch.cuda.memory_allocated()
    calls = []

    def sc():
        calls.append(b.kept_count.clone())
        return scales
    b.vote(pts, idx, lg, u, sc, centre_peaks=3)
    assert torch.cuda.memory_allocated() - m0 >= len(Ns) * b.cells_cap * 4
    got = _snap(b)
    for k in STATE:
        if k in ("kept_tuple", "kept_wt", "kept_row0"):          # only the kept entries of each scene's range are defined
            continue
        assert got[k] == want[k], k
    kc, off = a.kept_count.cpu().numpy(), np.concatenate([[0], np.cumsum(Ts)])
    for k in ("kept_tuple", "kept_wt", "kept_row0"):
        x, y = getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()
        for s in range(len(Ns)):
            assert x[off[s]:off[s] + kc[s]].tobytes() == y[off[s]:off[s] + kc[s]].tobytes(), (k, s)
    assert b.centre_results[0].cpu().numpy().tobytes() == want["results"]
    assert b.centre_counts[0].cpu().numpy().tobytes() == want["counts"]
    assert len(calls) == 3 and tuple(b.centre_results.shape) == (3, len(Ns), 160)
    assert np.array_equal(b.centre_idx[:, 0].cpu().numpy(), a.argmax.cpu().numpy())
    assert b.centre_n.cpu().numpy().min() >= 1 and b.centre_n.cpu().numpy().max() == 3
    # the default call again on the same object: still the same
    b.vote(pts, idx, lg, u, scales)
    assert _snap(b, ("results", "counts", "argmax", "world")) == {k: want[k] for k in ("results", "counts", "argmax", "world")}


def test_each_peak_equals_the_stages_run_by_hand_for_that_centre():
    """centre_results[c] / centre_counts[c] are what a fresh pipeline yields when its centre arrays are set to peak c by hand --
    the peaks taken from the NumPy restatement on the downloaded grid, not from the kernel -- and backvote -> rot_bins ->
    assemble are called through the public methods; a scene with fewer peaks has an empty record for the missing ones and does
    not disturb the others."""
    import torch
    dev = _gpu()
    from cppf2_amd.pipeline import RESULT_DTYPE, VotingPipeline
    Ns, Ts, pts, idx, lg, u, scales = _batch(dev, seed=4)
    C_ = 4
    # a separation of half the objects' length: no scene has four peaks that far apart
    sep = 0.12
    b = VotingPipeline(Ns, Ts, num_rots=90)
    b.vote(pts, idx, lg, u, scales, centre_peaks=C_, sep=sep)
    n = b.centre_n.cpu().numpy()
    print("peaks per scene at sep = 12 cm:", n.tolist())
    assert n.min() < C_ and n.max() >= 2
    grid = torch.zeros(len(Ns) * b.cells_cap, dtype=torch.int32, device=dev)
    goff = torch.arange(len(Ns), dtype=torch.int64, device=dev) * b.cells_cap
    for c in range(C_):
        f = VotingPipeline(Ns, Ts, num_rots=90)
        f.decode(pts, idx, lg, u)
        f.vote_center(pts, idx, grid, goff)
        grids = np.frombuffer(f.grids.cpu().numpy().tobytes(), GR.GRID_DTYPE)
        pi, pv, pw, pn = GR.grid_peaks_batch(grid.cpu().numpy(), goff.cpu().numpy(), grids, f.cells_cap, f.res, C_, round(sep / f.res))
        assert np.array_equal(pn, n)
        k_ = np.where(n > c, c, 0)                               # a scene without a peak c runs on its peak 0
        rows = np.arange(len(Ns))
        f.set_centre(torch.from_numpy(pi[rows, k_]).to(dev), torch.from_numpy(pv[rows, k_].view(np.int32)).to(dev),
                     torch.from_numpy(pw[rows, k_]).to(dev))
        f.backvote(pts, idx)
        f.rot_bins(pts, idx)
        f.assemble(scales)
        want = f.results_to_numpy()
        want["flags"][n <= c] |= 1
        got = np.frombuffer(b.centre_results[c].cpu().numpy().tobytes(), RESULT_DTYPE)
        assert got.tobytes() == want.tobytes(), c
        assert b.centre_counts[c].cpu().numpy().tobytes() == f.counts.cpu().numpy().tobytes(), c
        if c:
            assert np.all(got["argmax"][n > c] != b.centre_idx[:, 0].cpu().numpy()[n > c])
    with pytest.raises(Exception):
        b.vote(pts, idx, lg, u, scales, centre_peaks=17)


# ---- the case the feature exists for: the first maximum is a decoy ---------------------------------------------------------
VIEWS = [1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15]     # item seeds of render.item_rng(9, .): see the test's docstring
NEED = -(-len(VIEWS) * 15 // 16)                             # the share the issue asks of 16 views: at least 15 of them
OFFSET = 0.05                      # metres between the true centre and the decoy
DECOY_SHARE = 0.8                  # of the pairs vote for the decoy pose (at 0.6 the true centre still won: pairs whose line
                                   # passes near a centre put several rotations into its cell, and the true centre is the nearer)
T_PAIRS, N_POINTS, ROTS, C_PEAKS, HYP = 6000, 2048, 72, 3, 8


def _rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def _angle(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))


def _decoy_views(dev):
    """Per view: the fixture rendered at a seeded pose, its back-projected points, sampled pairs and their decoded targets placed
    directly (no network, as tests/test_verify_gpu.py builds its inputs): DECOY_SHARE of the pairs carry the targets of a decoy
    pose -- the true one turned by 180 degrees about the model's x axis, its centre OFFSET away along the longer image axis of
    the cloud's box, towards the box's middle -- the rest the true pose's."""
    import torch
    from oracle import cppf_oracle as O
    from cppf2_amd import bop, ops, render
    import test_verify_gpu as TV
    mesh = render.load_mesh(FIXTURE, 0.001)
    obj = bop.ObjectInfo.from_mesh(mesh)
    gt = np.stack([render.camera_pose(*render.sample_pose(render.item_rng(9, i), True), 1.0, obj.centre).astype(np.float64)
                   .reshape(3, 4) for i in VIEWS])
    depth = TV._render(obj, gt, dev)
    mask = depth > 0
    up, right, front = np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])
    out = []
    for j, v in enumerate(VIEWS):
        pc = TV._points(depth[j], mask[j], render.INTRINSICS, n=N_POINTS, seed=v)
        R, t = gt[j][:, :3], gt[j][:, 3]
        idx = ops.sample_tuples(len(pc), T_PAIRS, 5, 31, (v,)).cpu().numpy()
        lo, hi = pc.min(0).astype(np.float64), pc.max(0).astype(np.float64)
        ax = int(np.argmax((hi - lo)[:2]))
        e = np.zeros(3)
        e[ax] = 1.0 if (lo + hi)[ax] / 2 >= t[ax] else -1.0
        Rd, td = R @ _rot((1, 0, 0), 180.0), t + OFFSET * e
        pairs = pc[idx[:, :2]].astype(np.float64)
        decoy = np.arange(T_PAIRS) < int(DECOY_SHARE * T_PAIRS)
        tr = np.zeros((T_PAIRS, 2), np.float32)
        rot = np.zeros((T_PAIRS, 3), np.float32)
        for sel, (Rp, tp) in ((~decoy, (R, t)), (decoy, (Rd, td))):
            canon = ((pairs[sel] - tp) @ Rp).astype(np.float32)          # rows: R^T (p - t)
            tr[sel], rot[sel] = O.generate_target_pairs(canon, up, front, right)       # the reference's axis order (eval.py:237-240)
        out.append(dict(pc=pc, idx=idx, tr=tr, rot=rot, R=R, t=t, Rd=Rd, td=td))
    return dict(views=out, obj=obj, mesh=mesh, depth=depth, mask=mask, gt=gt)


def _run(dev, D, centre_peaks, icp_iters=30):
    """vote(centre_peaks) on the placed targets, the hypothesis list of eval.py, ICP and verification: the chosen records."""
    import torch
    import eval as ev
    from cppf2_amd import icp, render, verify
    from cppf2_amd.pipeline import VotingPipeline
    V = D["views"]
    B = len(V)
    pipe = VotingPipeline([len(v["pc"]) for v in V], [T_PAIRS] * B, num_rots=ROTS)
    pts = torch.from_numpy(np.concatenate([v["pc"] for v in V])).to(dev)
    idx = torch.from_numpy(np.concatenate([v["idx"] for v in V])).to(dev)
    pipe.tr.copy_(torch.from_numpy(np.concatenate([v["tr"] for v in V])))
    pipe.rot.copy_(torch.from_numpy(np.concatenate([v["rot"] for v in V])))
    pipe.decode_from_bins = lambda *a, **k: None                 # the targets are placed, not decoded
    pipe.vote(pts, idx, None, None, centre_peaks=centre_peaks)
    if centre_peaks > 1:
        hyp = np.stack([pipe.results_to_numpy(verify.hypotheses(pipe.centre_counts[c, 0], pipe.centre_counts[c, 1], pipe.sphere,
                                                                pipe.centre_results[c], HYP, pipe.up_axis, pipe.right_axis)
                                              .reshape(-1, 160)).reshape(B, HYP) for c in range(centre_peaks)])
    else:
        hyp = pipe.results_to_numpy(verify.hypotheses(pipe.counts[0], pipe.counts[1], pipe.sphere, pipe.results, HYP, pipe.up_axis,
                                                      pipe.right_axis).reshape(-1, 160)).reshape(1, B, HYP)
    sel = pipe.results_to_numpy()
    lists = [ev._instance_hypotheses(sel[b], 0, [hyp[:, b], None], (True, False), HYP) for b in range(B)]
    recs, centre = np.stack([l_[0] for l_ in lists]), np.stack([l_[1] for l_ in lists])
    off = np.cumsum([0] + [len(v["pc"]) for v in V])
    out = verify.select(D["obj"], D["depth"], D["mask"], render.INTRINSICS, recs, pts=pts, pt_off=off,
                        icp_model=icp.ModelPoints.from_mesh(D["mesh"]), icp_iters=icp_iters)
    return pipe, out, centre


def test_a_later_centre_peak_rescues_a_wrong_first_maximum():
    """Rendered views of the fixture whose vote grid has its first maximum at a decoy 5 cm from the true centre (80 % of the pairs
    vote for the decoy pose -- the true one turned by 180 degrees --, 20 % for the true one).  By the restatement alone (the
    oracle's vote grid, grid_peaks_ref) the decoy wins peak 0 in every view and the true centre is a later peak.
    Like for like, 8 hypotheses and 30 ICP iterations in both runs, only centre_peaks differs: with one centre peak the chosen
    pose is wrong on at least NEED views, with centre_peaks=3 it is within 1 degree and 2 mm of the truth on at least NEED.
    "Wrong" after ICP is judged by the rotation: more than 90 degrees from the truth, i.e. nearer the decoy's rotation than the
    true one (ICP's basin is 5-10 degrees, DESIGN.md 13, so a pose that far off is not one ICP was about to fix).  The issue's
    translation line (error > OFFSET - 1 cm) cannot hold after ICP and is asserted on the one-peak run WITHOUT ICP only, where
    every hypothesis carries the decoy's centre: ICP's inlier distance starts at 5 cm, so it drags a pose 5 cm off back onto
    the cloud -- measured 6-23 mm of translation error left after it, with the rotation still 174-180 degrees off.  A pure
    translation decoy of a few centimetres is therefore recovered by ICP alone; what the further peaks buy is the rotation that
    the wrong centre's kept pairs vote for.
    VIEWS is fixed up front: item seeds whose one-peak run reaches the true pose through a secondary rotation peak at the decoy
    centre plus ICP (0 and 8 of the first 16) cannot show a wrong baseline and are not in the list."""
    dev = _gpu()
    from oracle import cppf_oracle as O
    D = _decoy_views(dev)
    for j, v in enumerate(D["views"]):
        grid, _ = O.vote_center(v["pc"], v["tr"], 2e-3, v["idx"][:, :2], ROTS)
        c0 = v["pc"].min(0)
        pi, pv, pw, n = GR.grid_peaks(grid, grid.shape, c0, 2e-3, C_PEAKS, 10)
        assert np.abs(pw[0] - v["td"]).max() <= 2 * 2e-3, (j, pw, pv, v["td"], v["t"])
        assert n >= 2 and min(np.abs(pw[c] - v["t"]).max() for c in range(1, n)) <= 2 * 2e-3, (j, pw, v["t"])
    _, base_raw, _ = _run(dev, D, 1, icp_iters=0)
    pipe, base, _ = _run(dev, D, 1)
    pipe3, out, centre = _run(dev, D, C_PEAKS)
    shared = wrong = right = 0
    for j, v in enumerate(D["views"]):
        r0, r1, r3 = base_raw["records"][j], base["records"][j], out["records"][j]
        e0 = float(np.linalg.norm(r0["t"] - v["t"]))
        e1, a1 = float(np.linalg.norm(r1["t"] - v["t"])), _angle(r1["R"], v["R"])
        e3, a3 = float(np.linalg.norm(r3["t"] - v["t"])), _angle(r3["R"], v["R"])
        print("view %2d: one centre peak %.1f mm off (%.1f deg), with ICP %.1f mm (%.1f deg); %d peaks with ICP %.2f mm, %.2f deg, "
              "centre peak %d, chosen %d" % (VIEWS[j], e0 * 1e3, _angle(r0["R"], v["R"]), e1 * 1e3, a1, C_PEAKS, e3 * 1e3, a3,
                                             centre[j, out["chosen"][j]], out["chosen"][j]))
        shared += e0 > OFFSET - 0.01
        wrong += a1 > 90.0 and not (a1 < 1.0 and e1 < 2e-3)
        right += a3 < 1.0 and e3 < 2e-3
    assert np.array_equal(pipe3.centre_idx[:, 0].cpu().numpy(), pipe.argmax.cpu().numpy())
    assert shared >= NEED, shared
    assert wrong >= NEED, wrong
    assert right >= NEED, right


# ---- eval.py ---------------------------------------------------------------------------------------------------------------

def test_eval_main_centre_peaks(monkeypatch):
    """eval.main on the example depth / mask pair: --hypotheses=8 --centre_peaks=1 writes the report of a run without the flag;
    --centre_peaks=3 runs, reports the centre peak of the chosen hypothesis, and hypothesis 0 is unchanged."""
    _gpu()
    monkeypatch.chdir(ROOT)
    import eval as ev
    from cppf2_amd import verify
    e = json.load(open(os.path.join(GOLDEN, "full_summary.json")))["example_backproject"]
    kw = dict(data="depth", depth=os.path.join(GOLDEN, "example_data", "depth.png"), mask=os.path.join(GOLDEN, "example_data", "mask.png"),
              depth_scale=e["depth_scale"], intrinsics=e["K"], num_pairs=5000, num_rots=36, opt=False, debug=True, mesh=FIXTURE,
              mesh_scale=0.001, icp_iters=30, hypotheses=8)
    seen = []
    real = verify.select

    def spy(*a, **k):
        res = real(*a, **k)
        seen.append(res)
        return res
    monkeypatch.setattr(verify, "select", spy)
    plain = ev.main(**kw)
    one = ev.main(centre_peaks=1, **kw)
    assert json.dumps(one, sort_keys=True) == json.dumps(plain, sort_keys=True)
    assert "centre_peak" not in plain["results"][0]["verify"]
    three = ev.main(centre_peaks=3, **kw)
    v = three["results"][0]["verify"]
    assert 0 <= v["centre_peak"] < 3 and v["centre_peak"] == int(seen[2]["centre"][0, v["chosen"]])
    assert "cppf_grid_peaks" in three["verification"] and "cppf_grid_peaks" not in plain["verification"]
    # hypothesis 0 (the selected record, after ICP) is the same record in all three runs
    assert seen[2]["hypotheses"][0, 0].tobytes() == seen[0]["hypotheses"][0, 0].tobytes() == seen[1]["hypotheses"][0, 0].tobytes()
    assert v["score_first"] == plain["results"][0]["verify"]["score_first"] and v["score"] >= v["score_first"]
    assert seen[2]["centre"][0, 0] == 0
    with pytest.raises(ValueError, match="needs --hypotheses > 1"):
        ev.main(**dict(kw, hypotheses=1, centre_peaks=2))
    with pytest.raises(ValueError, match="must be >= 1"):
        ev.main(**dict(kw, centre_peaks=0))


def test_eval_bop_centre_peaks(tmp_path):
    """--data=bop --teacher_prior --hypotheses=8 --centre_peaks=3 over the generated dataset of tests/bop_data_ref.scenes: the CSV
    re-read and re-scored gives the printed report (the assertion tests/test_bop_data_gpu.py makes); the run is teacher-driven, so
    no recall is asserted."""
    _gpu()
    import bop_data_ref as DR
    import eval as ev
    from cppf2_amd import bop_data, render
    root = str(tmp_path / "gen")
    cv, cf = DR.cylinder()
    meshes = {DR.OBJ_FIXTURE: render.load_mesh(DR.FIXTURE, 0.001), DR.OBJ_CYL: render.Mesh(cv * 0.001, cf, 0.001)}
    scenes, occluders, holes = DR.scenes()
    occ = {k: [(render.Mesh(m[0], m[1]), R, t) for m, R, t in v] for k, v in occluders.items()}
    bop_data.write_dataset(root, "test", meshes, scenes, K=DR.K, height=DR.H, width=DR.W, models_info={DR.OBJ_CYL: DR.CYL_INFO},
                           occluders=occ, holes=holes)
    ds = bop_data.Dataset(root, "test")
    out_csv = str(tmp_path / "centre.csv")
    rep = ev.main(data="bop", bop_root=root, split="test", out_csv=out_csv, teacher_prior=True, num_pairs=20000, debug=True,
                  icp_iters=30, hypotheses=8, centre_peaks=3)
    print("eval --data=bop --teacher_prior --icp_iters=30 --hypotheses=8 --centre_peaks=3:",
          {k: rep["bop"][k] for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR")}, rep["skipped"])
    assert rep["rows"] == sum(t[3] for t in ds.targets())
    for item in rep["results"]:
        assert item["model"] is not None and 0 <= item["verify"]["centre_peak"] < 3 and 0 <= item["verify"]["chosen"] < 8
    scored = bop_data.score(ds, bop_data.read_results(out_csv))
    for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR", "recall", "matches", "targets", "per_object"):
        assert scored[k] == rep["bop"][k], k
    assert "cppf_grid_peaks" in rep["verification"]
