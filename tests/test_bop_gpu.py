"""GPU checks of the BOP scorer (cppf_vsd_counts, cppf_mssd_mspd, cppf2_amd/bop.py): VSD counts equal to the NumPy restatement
(tests/bop_ref.py) on rendered views of the fixture, MSSD / MSPD against the float64 restatement with and without symmetries and
at edge sizes, batch independence, pose_errors, and the eval.py --gt_pose flags."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bop_ref as BR  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "example_data", "obj_000015.ply")
VIEWS = 16
TAUS = np.arange(1, 11) * 0.05


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _rot(axis, deg):
    return BR.rotation(axis, np.deg2rad(deg))


def _perturb(P, rng, deg=(1, 10), mm=(1, 20)):
    ax, d = rng.standard_normal(3), rng.standard_normal(3)
    Q = P.copy()
    Q[:, :3] = _rot(ax, rng.uniform(*deg)) @ P[:, :3]
    Q[:, 3] = P[:, 3] + d / np.linalg.norm(d) * rng.uniform(*mm) * 1e-3
    return Q


def _render(obj, poses, dev):
    import torch
    from cppf2_amd import ops, render
    verts, faces, _ = obj.device(dev)
    n = len(poses)
    if n == 0:
        return np.zeros((0, render.HEIGHT, render.WIDTH), np.float32)
    return render.render_depth(verts, faces.repeat(n, 1), ops._offsets([faces.shape[0]] * n, dev),
                               torch.from_numpy(np.asarray(poses, dtype=np.float32).reshape(n, 12)).to(dev)).cpu().numpy()


@pytest.fixture(scope="module")
def scene():
    """VIEWS record poses of the fixture (uniform SO(3), rendered-item convention), their renders, and test images made of the
    gt render plus a rendered occluder (the object again, nearer and to the side), zeroed holes and seeded 1 mm noise."""
    dev = _gpu()
    from cppf2_amd import bop, render
    mesh = render.load_mesh(FIXTURE, 0.001)
    obj = bop.ObjectInfo.from_mesh(mesh)
    gt = []
    for i in range(VIEWS):
        Rm, tr = render.sample_pose(render.item_rng(5, i), True)
        P = render.camera_pose(Rm, tr, 1.0, obj.centre).astype(np.float64).reshape(3, 4)
        gt.append(P)
    gt = np.stack(gt)
    occ = gt.copy()
    occ[:, :, 3] = gt[:, :, 3] * 0.85 + np.array([0.04, 0.02, 0.0])
    dg, do = _render(obj, gt, dev), _render(obj, occ, dev)
    rng = np.random.default_rng(21)
    test = dg.copy()
    near = (do > 0) & ((test == 0) | (do < test))
    test[near] = do[near]
    test[rng.random(test.shape) < 0.05] = 0.0
    noise = rng.normal(0, 1e-3, test.shape).astype(np.float32)
    test = np.where(test > 0, test + noise, 0).astype(np.float32)
    return dict(obj=obj, gt=gt, dg=dg, test=test, dev=dev)


def _check_counts(got, test, de, dg, obj):
    from cppf2_amd import bop
    want, near = BR.vsd_counts(test, de, dg, render_K(), bop.DELTA, obj.diameter, TAUS, near=1e-12)
    if near:
        print("VSD: %d pixels within 1e-12 of a threshold" % near)
        assert np.abs(got - want).max() <= near, (got, want, near)
    else:
        assert np.array_equal(got, want), (got, want)
    return want


def render_K():
    from cppf2_amd import render
    return render.INTRINSICS


def test_vsd_counts_equal_the_restatement(scene):
    """est = gt (error 0 at every tau), 1-10 degree / 1-20 mm estimates against occluded, holed, noisy test images, and an estimate
    off screen (error 1): the kernel's counts equal the restatement's exactly."""
    from cppf2_amd import bop
    obj, gt, dg, test = scene["obj"], scene["gt"], scene["dg"], scene["test"]
    rng = np.random.default_rng(22)
    off = gt[:1].copy()
    off[0, 0, 3] += 5.0                                                     # 5 m to the side: nothing on screen
    est = np.concatenate([gt, np.stack([_perturb(P, rng) for P in gt]), off])
    idx = np.concatenate([np.arange(VIEWS), np.arange(VIEWS), [0]])
    de = _render(obj, est, scene["dev"])
    assert not de[-1].any()
    dgs = dg[idx]
    counts = bop.vsd_counts(test, idx, de, dgs, render_K(), obj.diameter, bop.DELTA, TAUS).cpu().numpy()
    for p in range(len(est)):
        _check_counts(counts[p], test[idx[p]], de[p], dgs[p], obj)
    e = bop.vsd_errors(counts)
    assert not e[:VIEWS].any() and (counts[:VIEWS, 0] > 100).all()
    assert (e[-1] == 1).all()
    assert (e[VIEWS:-1, -1] < 1).any() and (e[VIEWS:-1, 0] > 0).all()


def _cylinder(n=315, r=0.03, h=0.1):
    from cppf2_amd import render
    a = 2 * np.pi * np.arange(n) / n
    ring = np.stack([r * np.cos(a), r * np.sin(a)], -1)
    v = np.concatenate([np.hstack([ring, np.zeros((n, 1))]), np.hstack([ring, np.full((n, 1), h)])])
    return render.Mesh(v, np.array([[0, 1, n]], dtype=np.int32))


def _pose(R, t):
    return np.hstack([R, np.asarray(t, dtype=np.float64).reshape(3, 1)])


def _check_mssd_mspd(obj, est, gt):
    from cppf2_amd import bop
    ms, mp = (x.cpu().numpy() for x in bop.mssd_mspd(obj.verts, obj.syms, est, gt, render_K()))
    for p in range(len(est)):
        wd, wp = BR.mssd_mspd(obj.verts, obj.syms, est[p], gt[p], render_K())
        assert abs(float(ms[p]) - wd) <= 1e-6 * obj.diameter, (p, ms[p], wd)
        assert (np.isinf(mp[p]) and np.isinf(wp)) or abs(float(mp[p]) - wp) <= 1e-3, (p, mp[p], wp)
    return ms, mp


def test_mssd_mspd_against_float64(scene):
    """S = 1 on the fixture (9 174 vertices), a cylinder with a continuous symmetry (S = 315) and with a 180-degree flip on top
    (S = 630): within 1e-6 x diameter and 1e-3 px of the float64 restatement."""
    from cppf2_amd import bop
    rng = np.random.default_rng(23)
    gt = scene["gt"]
    est = np.stack([_perturb(P, rng) for P in gt])
    ms, mp = _check_mssd_mspd(scene["obj"], est, gt)
    assert (ms > 0).all() and (mp > 0).all()
    cyl = _cylinder()
    flip = np.eye(4)
    flip[:3, :3] = _rot([1, 0, 0], 180)
    for info, S in (({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}, 315),
                    ({"symmetries_discrete": [flip.reshape(-1).tolist()],
                      "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}, 630)):
        obj = bop.ObjectInfo.from_mesh(cyl, info)
        assert obj.syms.shape[0] == S
        g = np.stack([_pose(_rot(rng.standard_normal(3), rng.uniform(0, 180)), [rng.uniform(-.1, .1), rng.uniform(-.1, .1), 0.8])
                      for _ in range(4)])
        e = np.stack([_perturb(P, rng) for P in g])
        _check_mssd_mspd(obj, e, g)


def test_rotation_about_the_symmetry_axis(scene):
    """An estimate turned by 37 degrees about the cylinder's axis: near 0 with the continuous symmetry, large without it."""
    from cppf2_amd import bop
    cyl = _cylinder()
    sym = bop.ObjectInfo.from_mesh(cyl, {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]})
    plain = bop.ObjectInfo.from_mesh(cyl)
    R = _rot([1, 2, 3], 50)
    gt = _pose(R, [0.05, -0.02, 0.7])[None]
    est = _pose(R @ _rot([0, 0, 1], 37), [0.05, -0.02, 0.7])[None]
    ms, mp = _check_mssd_mspd(sym, est, gt)
    assert ms[0] < 0.01 * sym.diameter and mp[0] < 0.5
    ms0, mp0 = _check_mssd_mspd(plain, est, gt)
    assert ms0[0] > 0.1 * plain.diameter and mp0[0] > 10
    assert _check_mssd_mspd(sym, gt, gt)[0][0] == 0 and _check_mssd_mspd(sym, gt, gt)[1][0] == 0


def test_mssd_mspd_edge_sizes(scene):
    """V = 1, V = 1 025 (a partial LDS tile), P = 0 (no launch), an estimate behind the camera (MSPD +inf, MSSD finite)."""
    from cppf2_amd import bop
    obj = scene["obj"]
    rng = np.random.default_rng(24)
    gt = scene["gt"][:4]
    est = np.stack([_perturb(P, rng) for P in gt])
    for V in (1, 1025):
        sub = bop.ObjectInfo(obj.verts[:V], obj.faces[:1], obj.centre, obj.diameter, obj.syms)
        _check_mssd_mspd(sub, est, gt)
    ms, mp = bop.mssd_mspd(obj.verts, obj.syms, est[:0], gt[:0], render_K())
    assert ms.numel() == 0 and mp.numel() == 0
    behind = est[:1].copy()
    behind[0, 2, 3] = -1.0
    ms, mp = _check_mssd_mspd(obj, behind, gt[:1])
    assert np.isfinite(ms[0]) and np.isinf(mp[0])


def test_batch_independence(scene):
    """64 mixed pairs with different test images: each pair's counts, MSSD and MSPD are byte-identical alone and in the batch."""
    from cppf2_amd import bop
    obj, gt, dg, test = scene["obj"], scene["gt"], scene["dg"], scene["test"]
    rng = np.random.default_rng(25)
    idx = rng.integers(0, VIEWS, 64)
    est = np.stack([gt[i] if j % 5 == 0 else _perturb(gt[i], rng) for j, i in enumerate(idx)])
    de = _render(obj, est, scene["dev"])
    counts = bop.vsd_counts(test, idx, de, dg[idx], render_K(), obj.diameter, bop.DELTA, TAUS).cpu().numpy()
    ms, mp = (x.cpu().numpy() for x in bop.mssd_mspd(obj.verts, obj.syms, est, gt[idx], render_K()))
    for j in range(64):
        one = bop.vsd_counts(test, idx[j:j + 1], de[j:j + 1], dg[idx[j:j + 1]], render_K(), obj.diameter, bop.DELTA, TAUS)
        assert one.cpu().numpy().tobytes() == counts[j:j + 1].tobytes(), j
        a, b = (x.cpu().numpy() for x in bop.mssd_mspd(obj.verts, obj.syms, est[j:j + 1], gt[idx[j:j + 1]], render_K()))
        assert a.tobytes() == ms[j:j + 1].tobytes() and b.tobytes() == mp[j:j + 1].tobytes(), j


def test_pose_errors(scene):
    """pose_errors = the kernels on its own renders: est = gt scores 0 everywhere, a NaN estimate +inf everywhere, and the rest
    equal the restatement of the same renders."""
    from cppf2_amd import bop
    obj, gt, test = scene["obj"], scene["gt"], scene["test"]
    rng = np.random.default_rng(26)
    est = np.stack([gt[0], _perturb(gt[1], rng), np.full((3, 4), np.nan), _perturb(gt[3], rng)])
    idx = np.array([0, 1, 2, 3])
    err = bop.pose_errors(obj, test, idx, est[:, :, :3], est[:, :, 3], gt[:4, :, :3], gt[:4, :, 3], render_K())
    assert not err["vsd"][0].any() and err["mssd"][0] == 0 and err["mspd"][0] == 0
    assert np.isinf(err["vsd"][2]).all() and np.isinf(err["mssd"][2]) and np.isinf(err["mspd"][2])
    de = _render(obj, est[[1, 3]], scene["dev"])
    for k, p in enumerate((1, 3)):
        want = BR.vsd_errors(BR.vsd_counts(test[p], de[k], scene["dg"][p], render_K(), bop.DELTA, obj.diameter, TAUS)[0])
        assert np.array_equal(err["vsd"][p], want)
        wd, wp = BR.mssd_mspd(obj.verts, obj.syms, est[p], gt[p], render_K())
        assert abs(err["mssd"][p] - wd) <= 1e-6 * obj.diameter and abs(err["mspd"][p] - wp) <= 1e-3
    ar = bop.average_recall(err, obj.diameter, 640)
    assert 0.25 <= ar["AR"] <= 1.0


def test_eval_main_gt_pose(scene, tmp_path, monkeypatch):
    """eval.main(data="depth") on a rendered depth / mask pair with --gt_pose and --icp_iters=30: the results' bop blocks (after
    and before ICP) equal a direct bop.pose_errors call on the reported poses, the report carries their AR, and everything else is
    the report of the same run without --gt_pose.  --gt_pose without --mesh raises.  (Untrained models: consistency, not
    accuracy.)"""
    import torch
    from PIL import Image
    from cppf2_amd import bop, ops, render
    monkeypatch.chdir(ROOT)
    sys.path.insert(0, ROOT)
    import eval as ev
    dev = scene["dev"]
    mesh = render.load_mesh(FIXTURE, 0.001)
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
              opt=False, debug=True, mesh=FIXTURE, mesh_scale=0.001, icp_iters=30)
    base = ev.main(**kw)
    seen = []
    real = bop.pose_errors

    def spy(*a, **k):
        seen.append((a, k))
        return real(*a, **k)
    monkeypatch.setattr(bop, "pose_errors", spy)
    rep = ev.main(gt_pose=ppath, **kw)
    assert len(seen) == 1
    (obj, d, idx, Re, te, Rg, tg, K), k = seen[0]
    assert k == {} and len(Re) == 2
    RT = np.array(rep["results"][0]["pred_RT"])
    s = RT[0, 0] / Re[0][0, 0]
    assert np.array_equal(RT[:3, 3], te[0]) and np.allclose(RT[:3, :3], Re[0] * s, rtol=1e-12, atol=1e-15)
    assert np.array_equal(Rg[0], P.astype(np.float64).reshape(3, 4)[:, :3])
    d_png = np.array(Image.open(dpath)).astype(np.float64) / 1000.0
    assert np.array_equal(d, d_png)
    want = real(obj, d_png, [0, 0], Re, te, Rg, tg, render.INTRINSICS)
    res = rep["results"][0]
    for key, j in (("bop", 0), ("bop_before_icp", 1)):
        assert res[key] == dict(vsd=[float(x) for x in want["vsd"][j]], mssd=float(want["mssd"][j]), mspd=float(want["mspd"][j]))
    ar = bop.average_recall({k_: v_[:1] for k_, v_ in want.items()}, obj.diameter, 640)
    assert rep["bop"] == dict(ar, delta=bop.DELTA, taus=list(bop.TAUS))
    strip = dict(rep, results=[{k_: v_ for k_, v_ in res.items() if not k_.startswith("bop")}])
    del strip["bop"]
    assert json.dumps(strip, sort_keys=True) == json.dumps(base, sort_keys=True)
    with pytest.raises(ValueError):
        ev.main(**dict(kw, mesh=None, icp_iters=0, gt_pose=ppath))
