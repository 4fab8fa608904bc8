"""GPU checks of the mesh-based ICP refinement (cppf_icp_refine, cppf2_amd/icp.py): iteration-by-iteration parity with the NumPy
restatement (tests/icp_ref.py), whole-run parity, the frame contract of rendered items, recovery of perturbed poses on rendered
views, batch independence and determinism, and the eval.py --data=depth flags."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_ref as IR  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "example_data", "obj_000015.ply")
VIEWS = 40


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _records(poses):
    from cppf2_amd.pipeline import RESULT_DTYPE
    rec = np.zeros(len(poses), dtype=RESULT_DTYPE)
    for b, (R, t) in enumerate(poses):
        rec[b]["R"], rec[b]["t"] = R, t
    return rec


def _err(R, t, Rg, tg):
    c = np.clip((np.trace(R.T @ Rg) - 1) / 2, -1, 1)
    return np.degrees(np.arccos(c)), np.linalg.norm(t - tg) * 1000          # degrees, mm


def _perturb(R, t, rng):
    """R, t moved by 5-10 degrees about a random axis and by 1-2 cm in a random direction."""
    ax = rng.standard_normal(3)
    d = rng.standard_normal(3)
    return (IR.rodrigues(ax / np.linalg.norm(ax) * np.deg2rad(rng.uniform(5, 10))) @ R,
            t + d / np.linalg.norm(d) * rng.uniform(0.01, 0.02))


@pytest.fixture(scope="module")
def scene():
    """VIEWS rendered items of the fixture (uniform SO(3) poses, scale 1: the custom-object workflow) with their true poses.
    make_items back-projects pixel (r, c) along the ray through (c, r) (the reference's backproject, eval.py:185-189) while
    the rasterizer samples the surface at (c + 0.5, r + 0.5); the clouds here are moved onto those rays (x += z / 2 fx,
    y += z / 2 fy, exact up to float32 rounding) so that they lie on the mesh and the checks measure ICP, not that
    half-pixel convention (up to 2.4 mm at these depths)."""
    _gpu()
    from scipy.spatial.transform import Rotation
    from cppf2_amd import icp, render
    mesh = render.load_mesh(FIXTURE, 0.001)
    items = render.make_items(mesh, range(VIEWS), seed=3, full_rot=True)
    K = render.INTRINSICS
    pcs, gt = [], []
    for it in items:
        pc = it["pc"].astype(np.float64)
        pc[:, 0] += pc[:, 2] * (0.5 / K[0][0])
        pc[:, 1] += pc[:, 2] * (0.5 / K[1][1])
        pcs.append(pc.astype(np.float32))
        q = it["quat"].astype(np.float64)                                   # w, x, y, z
        gt.append((Rotation.from_quat(q[[1, 2, 3, 0]]).as_matrix(), it["trans"].astype(np.float64)))
    return dict(mesh=mesh, model=icp.ModelPoints.from_mesh(mesh), items=items, pcs=pcs, gt=gt)


def _batch(pcs):
    return np.concatenate(pcs), np.cumsum([0] + [len(p) for p in pcs])


def test_records_of_items_are_the_render_poses(scene):
    """Frame contract, part 1: an item's (rot, trans) is the record pose (R, t) with pc = R (v - centre) + t, v the mesh vertex
    (render._item: pc_canon = (pc - trans) @ rot / scale) -- the pose the rasterizer drew the view with."""
    from cppf2_amd import render
    mesh = scene["mesh"]
    b = mesh.bounds
    centre = (b[0] + b[1]) / 2
    for i in range(4):
        rng = render.item_rng(3, i)
        Rm, tr = render.sample_pose(rng, True)
        P = render.camera_pose(Rm, tr, 1.0, centre).astype(np.float64).reshape(3, 4)
        R, t = scene["gt"][i]
        np.testing.assert_allclose(R, P[:, :3], atol=1e-6)
        np.testing.assert_allclose(t, P[:, 3], atol=1e-6)
        assert scene["items"][i]["scale"] == np.float32((b[1] - b[0]).max())


def test_icp_at_the_items_pose_stays_there(scene):
    """Frame contract, part 2: started at the items' (rot, trans), 30 iterations move the pose by less than 0.25 degrees and
    0.3 mm (the model is 4 096 surface samples; on these views the restatement moves it by at most 0.11 degrees and 0.15 mm).
    The samples are centred like the rasterizer's views: any other frame moves it by centimetres."""
    from cppf2_amd import icp
    pts, off = _batch(scene["pcs"])
    rec = _records(scene["gt"])
    stats = icp.refine(scene["model"], pts, off, rec)
    for b, (Rg, tg) in enumerate(scene["gt"]):
        rot, tr = _err(rec[b]["R"], rec[b]["t"], Rg, tg)
        assert rot < 0.25 and tr < 0.3, (b, rot, tr)
    assert np.all(rec["flags"] == icp.REFINED)
    assert np.all(stats[:, 3] == icp.ITERS) and np.all(stats[:, 2] > 0.9) and np.all(stats[:, 1] < 1e-3)


def test_parity_iteration_by_iteration(scene):
    """iters=1 calls, each started from the GPU's previous pose, against one restatement step from that pose: the inlier count
    equal, the RMS and the pose within 1e-9."""
    from cppf2_amd import icp
    rng = np.random.default_rng(11)
    sel = [0, 5, 17, 33]
    pcs = [scene["pcs"][i] for i in sel]
    pts, off = _batch(pcs)
    rec = _records([_perturb(*scene["gt"][i], rng) for i in sel])
    for dk in IR.schedule(icp.ITERS, *icp.MAX_DIST)[:12]:
        before = rec.copy()
        stats = icp.refine(scene["model"], pts, off, rec, iters=1, max_dist=(float(dk), float(dk)))
        for b, pc in enumerate(pcs):
            R, t, cnt, rms, upd = IR.step(pc, before[b]["R"], before[b]["t"], scene["model"].pts, scene["model"].nrm, dk)
            assert upd and stats[b, 3] == 1
            assert stats[b, 0] == cnt, (b, stats[b, 0], cnt)
            assert abs(float(stats[b, 1]) - rms) <= 1e-9
            assert np.abs(rec[b]["R"] - R).max() <= 1e-9 and np.abs(rec[b]["t"] - t).max() <= 1e-9


def test_parity_whole_run(scene):
    """A 30-iteration call against the restatement's 30 iterations from the same start: poses within 1e-7 (rotation entries,
    metres), stats equal up to float32 rounding."""
    from cppf2_amd import icp
    rng = np.random.default_rng(12)
    sel = [2, 9, 21, 38]
    pcs = [scene["pcs"][i] for i in sel]
    pts, off = _batch(pcs)
    starts = [_perturb(*scene["gt"][i], rng) for i in sel]
    rec = _records(starts)
    stats = icp.refine(scene["model"], pts, off, rec)
    for b, pc in enumerate(pcs):
        R, t, st = IR.refine(pc, *starts[b], scene["model"].pts, scene["model"].nrm, icp.ITERS, *icp.MAX_DIST)
        assert np.abs(rec[b]["R"] - R).max() <= 1e-7 and np.abs(rec[b]["t"] - t).max() <= 1e-7, b
        assert stats[b, 0] == st[0] and stats[b, 3] == st[3]
        np.testing.assert_allclose(stats[b], st, rtol=1e-6)


def test_recovery_from_perturbed_poses(scene):
    """From the true pose moved by 5-10 degrees and 1-2 cm: final error < 0.5 degrees and < 2 mm on at least 90 % of the views
    (on comparable views the restatement reaches every view, at most 0.11 degrees and 0.15 mm)."""
    from cppf2_amd import icp
    rng = np.random.default_rng(13)
    pts, off = _batch(scene["pcs"])
    rec = _records([_perturb(R, t, rng) for R, t in scene["gt"]])
    icp.refine(scene["model"], pts, off, rec)
    errs = np.array([_err(rec[b]["R"], rec[b]["t"], Rg, tg) for b, (Rg, tg) in enumerate(scene["gt"])])
    ok = (errs[:, 0] < 0.5) & (errs[:, 1] < 2.0)
    assert len(ok) >= 32 and ok.mean() >= 0.9, errs


def test_batch_independence_and_determinism(scene):
    """64 instances of mixed sizes (and one record flagged empty): each record and its stats are byte-identical run alone or in
    the batch, and two runs of the batch give identical bytes; the empty record is left as it was, its stats are 0."""
    import torch
    from cppf2_amd import icp, ops
    dev = _gpu()
    rng = np.random.default_rng(14)
    pcs, poses = [], []
    for j in range(64):
        i = j % VIEWS
        pc = scene["pcs"][i]
        n = int(rng.integers(1, len(pc) + 1)) if j % 3 else len(pc)
        pcs.append(pc[:n])
        poses.append(_perturb(*scene["gt"][i], rng))
    rec0 = _records(poses)
    rec0[7]["flags"] = 1
    pts, off = _batch(pcs)
    pts_d = torch.from_numpy(pts).to(dev)
    off_d = ops._offsets([len(p) for p in pcs], dev)
    rec_d = torch.from_numpy(np.frombuffer(rec0.tobytes(), dtype=np.uint8).reshape(64, 160).copy()).to(dev)
    runs = []
    for _ in range(2):
        r = rec_d.clone()
        s = icp.refine(scene["model"], pts_d, off_d, r)
        runs.append((r.cpu().numpy().tobytes(), s.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]
    batch_rec = np.frombuffer(runs[0][0], dtype=rec0.dtype)
    batch_stats = np.frombuffer(runs[0][1], dtype=np.float32).reshape(64, 4)
    assert batch_rec[7].tobytes() == rec0[7].tobytes() and not batch_stats[7].any()
    for j in range(64):
        one = rec0[j:j + 1].copy()
        s = icp.refine(scene["model"], pcs[j], [0, len(pcs[j])], one)
        assert one.tobytes() == batch_rec[j:j + 1].tobytes(), j
        assert s.tobytes() == batch_stats[j:j + 1].tobytes(), j


def test_eval_main_depth_flags(scene, tmp_path, monkeypatch):
    """eval.main(data="depth") on a rendered depth / mask pair: --icp_iters=0 gives the report of a run without the new flags;
    --icp_iters=30 reports the pose icp.refine gives for the same cloud and the same selected record, and the stats."""
    import json
    import torch
    from PIL import Image
    from cppf2_amd import icp, ops, render
    monkeypatch.chdir(ROOT)
    sys.path.insert(0, ROOT)
    import eval as ev
    dev = _gpu()
    mesh = scene["mesh"]
    b = mesh.bounds
    Rm, tr = render.sample_pose(render.item_rng(3, 0), True)
    verts, tris = mesh.device(dev)
    pose = torch.from_numpy(render.camera_pose(Rm, tr, 1.0, (b[0] + b[1]) / 2)[None]).to(dev)
    depth = render.render_depth(verts, tris, ops._offsets([tris.shape[0]], dev), pose)[0].cpu().numpy()
    dpath, mpath = str(tmp_path / "d.png"), str(tmp_path / "m.png")
    Image.fromarray(np.round(depth * 1000).astype(np.uint16)).save(dpath)
    Image.fromarray(((depth > 0) * 255).astype(np.uint8)).save(mpath)
    kw = dict(data="depth", depth=dpath, mask=mpath, intrinsics=render.INTRINSICS.tolist(), num_pairs=5000, num_rots=36,
              opt=False, debug=True)
    base = ev.main(**kw)
    off = ev.main(mesh=FIXTURE, mesh_scale=0.001, icp_iters=0, **kw)
    assert json.dumps(off, sort_keys=True) == json.dumps(base, sort_keys=True)
    seen = []
    real = icp.refine

    def spy(model, pts, pt_off, results, **k):
        seen.append((model, pts.cpu().numpy().copy(), np.asarray(pt_off).copy(), results.copy(), k))
        return real(model, pts, pt_off, results, **k)
    monkeypatch.setattr(icp, "refine", spy)
    rep = ev.main(mesh=FIXTURE, mesh_scale=0.001, icp_iters=30, **kw)
    assert len(seen) == 1
    model, pts, pt_off, rec, k = seen[0]
    assert k == dict(iters=30) and len(rec) == 1
    RT0, RT = np.array(base["results"][0]["pred_RT"]), np.array(rep["results"][0]["pred_RT"])
    s = RT0[0, 0] / rec[0]["R"][0, 0]                                       # the scale norm eval.py multiplies R by
    assert np.array_equal(rec[0]["t"], RT0[:3, 3]) and np.allclose(rec[0]["R"] * s, RT0[:3, :3], rtol=1e-12, atol=1e-15)
    stats = real(model, pts, pt_off, rec, iters=30)
    assert np.array_equal(RT[:3, 3], rec[0]["t"]) and np.allclose(RT[:3, :3], rec[0]["R"] * s, rtol=1e-12, atol=1e-15)
    st = rep["results"][0]["icp"]
    assert st == dict(inliers=int(stats[0, 0]), rms=float(stats[0, 1]), inlier_frac=float(stats[0, 2]), updates=int(stats[0, 3]))
    assert rep["icp"] == [st] and "icp_refinement" in rep and "icp_refinement" not in base
    assert {k_: v for k_, v in rep.items() if k_ not in ("results", "icp", "icp_refinement")} == \
        {k_: v for k_, v in base.items() if k_ != "results"}
    with pytest.raises(ValueError):
        ev.main(icp_iters=30, **kw)                                         # no mesh
