"""GPU checks of the pose-hypothesis verification (cppf_verify.hip, cppf2_amd/verify.py): cppf_pose_hypotheses against the NumPy
restatement (tests/verify_ref.py) on hand-built count rows and on real pipeline counts, cppf_depth_fit_counts against it on
rendered views of the fixture, batch independence, selection among distractors with and without ICP, and eval.py
--hypotheses end to end."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import verify_ref as VR  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "example_data", "obj_000015.ply")
VIEWS = 16
COS20 = float(np.cos(np.deg2rad(20.0)))
COS45 = float(np.cos(np.deg2rad(45.0)))


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def _angle(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))


def _rand_sphere(S, rng):
    v = rng.standard_normal((S, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _random_base(B, rng):
    from cppf2_amd.pipeline import RESULT_DTYPE
    raw = rng.integers(0, 256, (B, 160), dtype=np.uint8)
    base = np.frombuffer(raw.tobytes(), dtype=RESULT_DTYPE).copy()
    base["flags"] &= ~1
    return base


def _run_hyp(cu, cr, sph, base, K, H, cos_sep, cos_perp, ua, ra, y_only):
    from cppf2_amd import verify
    from cppf2_amd.pipeline import RESULT_DTYPE
    out, pi, pc = verify.hypotheses(cu, cr, sph, base, H, ua, ra, K=K, cos_sep=cos_sep, cos_perp=cos_perp, y_only=y_only,
                                    with_peaks=True)
    rec = np.frombuffer(out.cpu().numpy().tobytes(), dtype=RESULT_DTYPE).reshape(len(base), H)
    return rec, pi.cpu().numpy(), pc.cpu().numpy()


def _check_hyp(cu, cr, sph, base, K, H, cos_sep=COS20, cos_perp=COS45, ua=1, ra=0, y_only=False):
    got, gpi, gpc = _run_hyp(cu, cr, sph, base, K, H, cos_sep, cos_perp, ua, ra, y_only)
    want, wpi, wpc = VR.hypotheses(cu, cr, sph, base, K, H, cos_sep, cos_perp, ua, ra, y_only)
    assert np.array_equal(gpi, wpi)
    assert gpc.tobytes() == wpc.tobytes()
    assert got.tobytes() == want.tobytes()
    return got


@pytest.mark.parametrize("B,S", [(1, 720), (64, 720), (1, 100), (64, 317), (3, 1)])
def test_hypotheses_match_the_restatement_on_hand_built_rows(B, S):
    """Small-integer counts (ties everywhere), all-zero rows, single-spike rows, S not a multiple of 64; K from 1 to 32, H up to
    more than the combinations; both axis orders and y_only."""
    _gpu()
    from cppf2_amd import ops
    rng = np.random.default_rng(B * 1000 + S)
    sph = ops.sphere_bins(1.0) if S == 720 else _rand_sphere(S, rng)
    cu = rng.integers(0, 4, (B, S)).astype(np.float32)
    cr = (rng.integers(0, 3, (B, S)) * rng.random((B, S))).astype(np.float32)
    cu[0] = 0.0
    if B > 2:
        cr[1] = 0.0
        cr[2] = 0.0
        cr[2, S // 2] = 7.0
    base = _random_base(B, rng)
    for K, H, ua, ra, yo in ((4, 8, 1, 0, False), (1, 1, 2, 0, False), (32, 40, 0, 2, False), (7, 1024, 1, 2, False),
                             (4, 8, 1, 0, True)):
        got = _check_hyp(cu, cr, sph, base, K, H, ua=ua, ra=ra, y_only=yo)
        # slot 0 carries the arg-max pair
        assert np.array_equal(got[:, 0]["up_idx"], np.argmax(cu, axis=1))
    # other separations, antipodes allowed to be peaks, nothing perpendicular enough
    _check_hyp(cu, cr, sph, base, 5, 9, cos_sep=-0.5, cos_perp=0.0)
    _check_hyp(cu, cr, sph, base, 5, 9, cos_sep=1.0, cos_perp=1.0)


def test_hypotheses_of_real_pipeline_counts():
    """run_ensemble(hypotheses=8) on synthetic instances with the teacher prior: each pass' hypotheses equal the restatement on
    the pass' own counts (keep=True hands them out), slot 0 is byte for byte the pass' cppf_assemble_pose record, and the
    two-stream run (keep=False) forms the same hypotheses and the same records as a run without hypotheses."""
    dev = _gpu()
    import torch
    sys.path.insert(0, ROOT)
    import eval as ev
    from cppf2_amd import synth
    for cat in ("mug", "bottle"):
        cfg, dino, shot_m = ev.load_category(cat, device=dev)
        B = 3
        scenes = [synth.make_scene(3, 60 + s, 1024) for s in range(B)]
        g = torch.Generator().manual_seed(2)
        descs = [torch.nn.functional.normalize(torch.randn((1024, 1024), generator=g), dim=-1).numpy() for _ in scenes]
        prior = ev._teacher_prior(np.concatenate([s["pc_canon"] for s in scenes]), dev)
        kw = dict(priors=prior, scale_priors=np.stack([s["extent"] for s in scenes]), up_sym=cat in ev.UP_SYM)
        ids = [60, 61, 62]
        a = ev.run_ensemble(cfg, dino, shot_m, [s["pc"] for s in scenes], descs, 5, ids, 6000, 72, keep=True, hypotheses=8, **kw)
        pipe = a["pipe"]
        for m in (0, 1):
            counts = a["kept"][m]["counts"]
            want, _, _ = VR.hypotheses(counts[0], counts[1], pipe.sphere_np, a["records"][m], 4, 8, COS20, COS45, pipe.up_axis,
                                       pipe.right_axis, kw["up_sym"])
            assert a["hypotheses"][m].tobytes() == want.tobytes(), (cat, m)
            assert a["hypotheses"][m][:, 0].tobytes() == a["records"][m].tobytes()
            assert np.count_nonzero((a["hypotheses"][m]["flags"] & 1) == 0) > B
        b = ev.run_ensemble(cfg, dino, shot_m, [s["pc"] for s in scenes], descs, 5, ids, 6000, 72, keep=False, hypotheses=8, **kw)
        c = ev.run_ensemble(cfg, dino, shot_m, [s["pc"] for s in scenes], descs, 5, ids, 6000, 72, keep=False, **kw)
        assert "hypotheses" not in c
        for m in (0, 1):
            assert b["hypotheses"][m].tobytes() == a["hypotheses"][m].tobytes()
            assert b["records"][m].tobytes() == c["records"][m].tobytes()
        assert b["selected"].tobytes() == c["selected"].tobytes()
        # with `opt` the records are refined after the hypotheses were formed: slot 0 keeps the assembled pose
        d = ev.run_ensemble(cfg, dino, shot_m, [s["pc"] for s in scenes], descs, 5, ids, 6000, 72, keep=False, hypotheses=8,
                            opt=True, **kw)
        assert d["hypotheses"][0].tobytes() == b["hypotheses"][0].tobytes()


def _render(obj, poses, dev):
    import torch
    from cppf2_amd import ops, render
    verts, faces, _ = obj.device(dev)
    n = len(poses)
    return render.render_depth(verts, faces.repeat(n, 1), ops._offsets([faces.shape[0]] * n, dev),
                               torch.from_numpy(np.asarray(poses, dtype=np.float32).reshape(n, 12)).to(dev)).cpu().numpy()


def _erode(m, k=2):
    out = m.copy()
    for dy in range(-k, k + 1):
        for dx in range(-k, k + 1):
            out &= np.roll(np.roll(m, dy, 0), dx, 1)
    return out


@pytest.fixture(scope="module")
def views():
    return make_views(_gpu())


def make_views(dev):
    """VIEWS record poses of the fixture (uniform SO(3), the rendered-item convention), their renders, and observed images: the
    render with a box in front of part of the object (view 0: 30 % of its pixels), zeroed holes, +-2 mm noise, the instance mask
    eroded by 2 px without the occluded pixels."""
    from cppf2_amd import bop, render
    mesh = render.load_mesh(FIXTURE, 0.001)
    obj = bop.ObjectInfo.from_mesh(mesh)
    gt = np.stack([render.camera_pose(*render.sample_pose(render.item_rng(9, i), True), 1.0, obj.centre).astype(np.float64)
                   .reshape(3, 4) for i in range(VIEWS)])
    dg = _render(obj, gt, dev)
    rng = np.random.default_rng(15)
    depth, mask = dg.copy(), dg > 0
    for i in range(VIEWS):
        cols = np.nonzero(mask[i].any(0))[0]
        frac = 0.3 if i == 0 else rng.uniform(0.0, 0.15)
        # the box: the first columns of the object holding `frac` of its pixels, 3 cm in front of the surface
        cum = np.cumsum(mask[i][:, cols].sum(0)) / mask[i].sum()
        c1 = cols[np.searchsorted(cum, frac)] if frac > 0 else cols[0] - 1
        box = np.zeros_like(mask[i])
        box[:, cols[0]:c1 + 1] = True
        box &= dg[i] > 0
        depth[i][box] = dg[i][box] - 0.03
        mask[i] &= ~box
    depth[rng.random(depth.shape) < 0.03] = 0.0
    noise = rng.uniform(-2e-3, 2e-3, depth.shape).astype(np.float32)
    depth = np.where(depth > 0, depth + noise, 0).astype(np.float32)
    mask = np.stack([_erode(m_) for m_ in mask])
    return dict(obj=obj, mesh=mesh, gt=gt, dg=dg, depth=depth, mask=mask, dev=dev)


def _perturb(P, rng, deg, cm):
    ax, d = rng.standard_normal(3), rng.standard_normal(3)
    Q = P.copy()
    Q[:, :3] = _rot(ax, rng.uniform(*deg)) @ P[:, :3]
    Q[:, 3] = P[:, 3] + d / np.linalg.norm(d) * rng.uniform(*cm) * 1e-2
    return Q


def test_fit_counts_match_the_restatement(views):
    """Exact counts on the rendered views at several taus: 64 hypotheses (perturbed true poses, the true pose itself) over 3
    images; each hypothesis alone gives the same row as in the batch; P = 0 launches nothing."""
    from cppf2_amd import verify
    dev = views["dev"]
    rng = np.random.default_rng(4)
    img = [0, 1, 2]
    hyp_off = np.array([0, 20, 41, 64], np.int32)
    poses = []
    for i in img:
        n = hyp_off[i + 1] - hyp_off[i]
        poses += [views["gt"][i]] + [_perturb(views["gt"][i], rng, (0, 10), (0, 3)) for _ in range(n - 1)]
    ren = _render(views["obj"], np.stack(poses), dev)
    taus = [0.002, 0.005, 0.01, 0.02, 0.05]
    d, m = views["depth"][img], views["mask"][img].astype(np.uint8)
    got = verify.fit_counts(d, m, hyp_off, ren, taus).cpu().numpy()
    want = VR.fit_counts(d, m, hyp_off, ren, taus)
    assert np.array_equal(got, want)
    assert got[:, 0].min() > 0 and got[:, 2].sum() > 0 and got[:, 3].sum() > 0 and (got[:, 4] < got[:, -1]).any()
    for p in (0, 25, 63):
        i = int(np.searchsorted(hyp_off, p, side="right") - 1)
        one = verify.fit_counts(d[i], m[i], [0, 1], ren[p:p + 1], taus).cpu().numpy()
        assert one.tobytes() == got[p:p + 1].tobytes()
    # 1 tau, one hypothesis on the last image only (the blocks of the others return at once)
    one = verify.fit_counts(d, m, [0, 0, 0, 1], ren[63:64], taus[:1]).cpu().numpy()
    assert np.array_equal(one, want[63:64, :5])
    empty = verify.fit_counts(d, m, [0, 0, 0, 0], ren[:0], taus)
    assert tuple(empty.shape) == (0, 9)


def _hypothesis_set(P, rng):
    """8 poses: the true one moved by <= 8 degrees and <= 1.5 cm first, then 180-degree flips about each model axis, 90-degree
    turns about two of them, and random rotations at least 30 degrees away (these keep the true translation)."""
    R, t = P[:, :3], P[:, 3]
    hyp = [_perturb(P, rng, (2, 8), (0.3, 1.5))]
    for ax in np.eye(3):
        hyp.append(np.hstack([R @ _rot(ax, 180), t[:, None]]))
    for ax in np.eye(3)[[0, 2]]:
        hyp.append(np.hstack([R @ _rot(ax, 90), t[:, None]]))
    while len(hyp) < 8:
        q = rng.standard_normal(4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        Rr = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                       [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                       [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        if _angle(Rr, R) >= 30:
            hyp.append(np.hstack([Rr, t[:, None]]))
    return hyp


def _points(depth, mask, K, n=3000, seed=0):
    """The masked pixels back-projected along the rays the rasterizer samples, (c + 0.5, r + 0.5)."""
    r, c = np.nonzero(mask & (depth > 0))
    z = depth[r, c].astype(np.float64)
    pts = np.stack([(c + 0.5 - K[0][2]) * z / K[0][0], (r + 0.5 - K[1][2]) * z / K[1][1], z], 1)
    if len(pts) > n:
        pts = pts[np.random.default_rng(seed).choice(len(pts), n, replace=False)]
    return pts.astype(np.float32)


def test_select_picks_the_true_hypothesis(views):
    """16 views, 8 shuffled hypotheses each (one near the truth, seven distractors): without ICP the near-true hypothesis wins on
    at least 15 views; after 30 ICP iterations the chosen pose is within 1 degree and 2 mm of the truth on at least 15, where
    hypothesis 0 alone (always a distractor here) is not.  The chosen record carries flags bit5 and its index in pad_[1]."""
    from cppf2_amd import icp, render, verify
    from cppf2_amd.pipeline import RESULT_DTYPE
    K = render.INTRINSICS
    rng = np.random.default_rng(33)
    recs = np.zeros((VIEWS, 8), dtype=RESULT_DTYPE)
    true_at = np.zeros(VIEWS, np.int64)
    for v in range(VIEWS):
        hyp = _hypothesis_set(views["gt"][v], rng)
        order = rng.permutation(8)
        if order[0] == 0:
            order = np.roll(order, 1)                           # hypothesis 0 is a distractor
        for h, j in enumerate(order):
            recs[v, h]["R"], recs[v, h]["t"] = hyp[j][:, :3], hyp[j][:, 3]
        true_at[v] = int(np.nonzero(order == 0)[0][0])
    out = verify.select(views["obj"], views["depth"], views["mask"], K, recs)
    assert np.count_nonzero(out["chosen"] == true_at) >= 15, (out["chosen"], true_at, out["scores"])
    assert np.all(out["records"]["flags"] & verify.CHOSEN) and np.array_equal(out["records"]["pad_"][:, 1], out["chosen"])
    assert out["icp"] is None and out["scores"].shape == (VIEWS, 8)
    pcs = [_points(views["depth"][v], views["mask"][v], K, seed=v) for v in range(VIEWS)]
    off = np.cumsum([0] + [len(p) for p in pcs])
    model = icp.ModelPoints.from_mesh(views["mesh"])
    out = verify.select(views["mesh"], views["depth"], views["mask"], K, recs, pts=np.concatenate(pcs), pt_off=off,
                        icp_model=model, icp_iters=30)
    assert out["icp"].shape == (VIEWS, 8, 4)
    good = first = 0
    for v in range(VIEWS):
        Rg, tg = views["gt"][v][:, :3], views["gt"][v][:, 3]
        r = out["records"][v]
        good += _angle(r["R"], Rg) < 1.0 and np.linalg.norm(r["t"] - tg) < 2e-3
        h0 = out["hypotheses"][v, 0]
        first += _angle(h0["R"], Rg) < 1.0 and np.linalg.norm(h0["t"] - tg) < 2e-3
    assert good >= 15, (good, out["chosen"], true_at)
    assert first < 15


def test_select_skips_empty_and_unrenderable_hypotheses(views):
    """An empty slot never wins, a non-finite pose and one behind the near plane score 0 and are not drawn."""
    from cppf2_amd import render, verify
    from cppf2_amd.pipeline import RESULT_DTYPE
    rec = np.zeros((1, 4), dtype=RESULT_DTYPE)
    P = views["gt"][1]
    for h in range(4):
        rec[0, h]["R"], rec[0, h]["t"] = P[:, :3], P[:, 3]
    rec[0, 0]["t"] = (0.0, 0.0, 0.01)                           # nearer than ZNEAR
    rec[0, 1]["R"] = np.nan
    rec[0, 2]["flags"] = verify.EMPTY
    out = verify.select(views["obj"], views["depth"][1], views["mask"][1], render.INTRINSICS, rec)
    assert out["chosen"].tolist() == [3]
    assert out["scores"][0, 0] == 0.0 and out["scores"][0, 1] == 0.0 and np.isnan(out["scores"][0, 2]) and out["scores"][0, 3] > 0.5
    assert np.all(out["counts"][0, :2, 0] == 0)


def test_eval_main_hypotheses(views, tmp_path, monkeypatch):
    """eval.main(data="depth", hypotheses=8, icp_iters=30, gt_pose=...) on a rendered pair: verify blocks, score >= score_first,
    the reported pose is the chosen hypothesis' record, bop_first is the bop of the same run with hypotheses=1, and a run with
    hypotheses=1 writes the report of a run without the flag."""
    import torch
    from PIL import Image
    from cppf2_amd import ops, render, verify
    monkeypatch.chdir(ROOT)
    sys.path.insert(0, ROOT)
    import eval as ev
    dev = views["dev"]
    mesh = views["mesh"]
    b = mesh.bounds
    Rm, tr = render.sample_pose(render.item_rng(3, 0), True)
    P = render.camera_pose(Rm, tr, 1.0, (b[0] + b[1]) / 2)
    verts, tris = mesh.device(dev)
    depth = render.render_depth(verts, tris, ops._offsets([tris.shape[0]], dev), torch.from_numpy(P[None]).to(dev))[0].cpu().numpy()
    dpath, mpath, ppath = str(tmp_path / "d.png"), str(tmp_path / "m.png"), str(tmp_path / "pose.txt")
    Image.fromarray(np.round(depth * 1000).astype(np.uint16)).save(dpath)
    Image.fromarray(((depth > 0) * 255).astype(np.uint8)).save(mpath)
    np.savetxt(ppath, P.astype(np.float64).reshape(3, 4))
    kw = dict(data="depth", depth=dpath, mask=mpath, intrinsics=render.INTRINSICS.tolist(), num_pairs=5000, num_rots=36,
              opt=False, debug=True, mesh=FIXTURE, mesh_scale=0.001, icp_iters=30, gt_pose=ppath)
    seen = []
    real = verify.select

    def spy(*a, **k):
        res = real(*a, **k)
        seen.append(res)
        return res
    monkeypatch.setattr(verify, "select", spy)
    rep = ev.main(hypotheses=8, **kw)
    assert len(seen) == 1
    res = rep["results"][0]
    v = res["verify"]
    sel = seen[0]
    assert v["hypotheses"] >= 2 and v["chosen"] == int(sel["chosen"][0]) and v["score"] >= v["score_first"]
    assert v["score"] == float(sel["scores"][0, v["chosen"]]) and v["score_first"] == float(sel["scores"][0, 0])
    chosen = sel["records"][0]
    assert chosen["flags"] & verify.CHOSEN and chosen["pad_"][1] == v["chosen"]
    RT = np.array(res["pred_RT"])
    assert np.array_equal(RT[:3, 3], chosen["t"])
    s = RT[0, 0] / chosen["R"][0, 0]
    assert np.allclose(RT[:3, :3], chosen["R"] * s, rtol=1e-12, atol=1e-15)
    assert "verification" in rep and "bop_first" in res and "bop_before_icp" in res
    one = ev.main(hypotheses=1, **kw)
    assert res["bop_first"] == one["results"][0]["bop"]
    assert res["bop_before_icp"] == one["results"][0]["bop_before_icp"]
    plain = ev.main(**kw)
    assert json.dumps(one, sort_keys=True) == json.dumps(plain, sort_keys=True)
    assert "verify" not in plain["results"][0] and "verification" not in plain
