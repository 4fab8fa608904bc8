"""GPU checks of the training-item generator: cppf_render_depth bit for bit against its NumPy mirror (tests/render_ref.py), the
depth against a float64 ray cast, batch invariance, the tile-list overflow path, the geometry and reproducibility of the
items, the CLI -> ExportedItems -> train_shot.py chain and the ShapeNet layout of dataset.py."""
import glob
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_ref as RR  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "example_data", "obj_000015.ply")
K = np.array([[591.0125, 0, 320], [0, 590.16775, 240], [0, 0, 1]])
H, W = 480, 640


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _views(meshes, poses, cull=1, dev=None, K_=K, hw=(H, W)):
    """Renders views (mesh_i, pose_i) in one call: (depth [B,H,W], tri_id [B,H,W]) as NumPy."""
    import torch
    from cppf2_amd import ops, render
    verts = np.concatenate([m[0] for m in meshes]).astype(np.float32)
    base = np.cumsum([0] + [len(m[0]) for m in meshes])
    tris = np.concatenate([m[1] + base[i] for i, m in enumerate(meshes)]).astype(np.int32)
    d, t = render.render_depth(torch.as_tensor(verts).to(dev), torch.as_tensor(tris).to(dev),
                               ops._offsets([len(m[1]) for m in meshes], dev), torch.as_tensor(np.stack(poses)).to(dev),
                               K_, hw[0], hw[1], cull=bool(cull), with_ids=True)
    return d.cpu().numpy(), t.cpu().numpy()


def _fixture():
    from cppf2_amd import render
    m = render.load_mesh(FIXTURE, 0.001)
    return m.verts, m.faces


def _fixture_poses(n, full_rot, seed=0):
    from cppf2_amd import render
    m = render.load_mesh(FIXTURE, 0.001)
    b = m.bounds
    out = []
    for i in range(n):
        R, tr = render.sample_pose(render.item_rng(seed, i), full_rot)
        out.append(render.camera_pose(R, tr, 1.0, (b[0] + b[1]) / 2))
    return out


def _assert_mirror(meshes, poses, cull, dev, K_=K, hw=(H, W)):
    d, t = _views(meshes, poses, cull, dev, K_, hw)
    for b, (m, p) in enumerate(zip(meshes, poses)):
        rd, rt, rej = RR.render(m[0], m[1], p, K_, hw[0], hw[1], cull=cull)
        assert rej == 0
        assert np.array_equal(d[b].view(np.uint32), rd.view(np.uint32)), (b, int((d[b] != rd).sum()))
        assert np.array_equal(t[b], rt), b
    return d, t


# ---- bit-exact against the mirror ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [0, 1])
def test_small_meshes_match_the_mirror(cull):
    dev = _gpu()
    rng = np.random.default_rng(1)
    sphere = RR.icosphere(3, 0.15)
    box = RR.cube(0.1)
    tri_front = (np.array([[-0.1, -0.1, 0.0], [0.1, -0.05, 0.0], [0.0, 0.12, 0.0]]), np.array([[0, 2, 1]], np.int32))
    tri_back = (tri_front[0], np.array([[0, 1, 2]], np.int32))
    # a plane reaching far off screen on every side (and a vertex 2000 px away)
    plane = (np.array([[-3.0, -3.0, 0.0], [3.0, -3.0, 0.0], [3.0, 3.0, 0.3], [-3.0, 3.0, 0.0]]),
             np.array([[0, 2, 1], [0, 3, 2]], np.int32))
    meshes, poses = [], []
    for m in (sphere, box, tri_front, tri_back, plane):
        for _ in range(2):
            R = RR.random_rotation(rng) if m is sphere or m is box else np.eye(3)
            meshes.append(m)
            poses.append(RR.look_pose(R, [rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.5, 1.5)]))
    d, t = _assert_mirror(meshes, poses, cull, dev)
    # the single back-facing triangle is drawn only without culling; the front one always
    assert (d[4] > 0).any() and (d[6] > 0).any() == (cull == 0)
    assert (d[8] > 0).all()                                 # the plane covers the whole image


def test_closed_meshes_cull_back_equals_cull_none_and_odd_sizes():
    dev = _gpu()
    rng = np.random.default_rng(2)
    meshes = [RR.icosphere(3, 0.15), RR.cube(0.1)] * 3
    poses = [RR.look_pose(RR.random_rotation(rng), [rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.4, 1.0)])
             for _ in meshes]
    d0, _ = _views(meshes, poses, 0, dev)
    d1, _ = _views(meshes, poses, 1, dev)
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    # an image whose size is not a multiple of the tile
    K2 = np.array([[250.0, 0, 50.3], [0, 260.0, 37.9], [0, 0, 1]])
    _assert_mirror(meshes[:2], poses[:2], 1, dev, K2, (75, 101))


@pytest.mark.parametrize("full_rot", [False, True])
def test_fixture_matches_the_mirror(full_rot):
    dev = _gpu()
    fx = _fixture()
    poses = _fixture_poses(8, full_rot, seed=11)
    _assert_mirror([fx] * 8, poses, 1, dev)
    _assert_mirror([fx] * 2, poses[:2], 0, dev)


# ---- physical check --------------------------------------------------------------------------------------------------
def _moller_trumbore(tri, ray):
    """Distance along `ray` (z component 1, so: the depth) to the plane of each triangle tri [n,3,3], float64."""
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    det = (e1 * np.cross(ray, e2)).sum(1)
    return (e2 * np.cross(-tri[:, 0], e1)).sum(1) / det


def test_depth_matches_a_float64_ray_cast():
    """Depth of the pixels whose 3x3 neighbourhood has one tri_id against a float64 ray cast through the sample point (c+0.5,
    r+0.5): (a) against the triangle the kernel defines -- the float32 camera-space vertices at their snapped screen positions --
    the float32 arithmetic stays within 1e-6 (measured: 2.4e-7); (b) against the unsnapped triangle all pixels are within 1e-3
    and 99.5 % within 2e-5 (measured: 4.9e-5 and 99.9 %): moving a vertex by up to 1/512 px changes the depth of a face seen at
    a grazing angle from 0.4 m by up to a few 1e-5.  The fixture's triangles span 1-3 px at the generator's distances, so few
    of its pixels qualify; the icosphere and the cube close up supply the bulk."""
    dev = _gpu()
    rng = np.random.default_rng(9)
    meshes = [_fixture()] * 4 + [RR.icosphere(2, 0.15)] * 6 + [RR.cube(0.1)] * 6
    poses = _fixture_poses(2, False, seed=3) + _fixture_poses(2, True, seed=3) + [
        RR.look_pose(RR.random_rotation(rng), [rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.4, 1.2)])
        for _ in range(12)]
    d, t = _views(meshes, poses, 1, dev)
    F = np.float32
    fx, fy, cx, cy = (float(F(K[0, 0])), float(F(K[1, 1])), float(F(K[0, 2])), float(F(K[1, 2])))
    raw, snapped = [], []
    for b, p in enumerate(poses):
        v, f = meshes[b]
        v32 = v.astype(F)
        P = p.astype(np.float64).reshape(3, 4)
        cam = v32.astype(np.float64) @ P[:, :3].T + P[:, 3]
        Pf = p.reshape(12).astype(F)
        x, y, z = v32[:, 0], v32[:, 1], v32[:, 2]
        xc = ((Pf[0] * x + Pf[1] * y) + Pf[2] * z) + Pf[3]
        yc = ((Pf[4] * x + Pf[5] * y) + Pf[6] * z) + Pf[7]
        zc = ((Pf[8] * x + Pf[9] * y) + Pf[10] * z) + Pf[11]
        su = np.rint((F(fx) * (xc / zc) + F(cx)) * F(256)).astype(np.float64) / 256
        sv = np.rint((F(fy) * (yc / zc) + F(cy)) * F(256)).astype(np.float64) / 256
        zz = zc.astype(np.float64)
        snap = np.stack([(su - cx) / fx * zz, (sv - cy) / fy * zz, zz], -1)
        tid = t[b]
        pad = np.pad(tid, 1, constant_values=-2)
        same = np.ones_like(tid, bool)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                same &= pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] == tid
        rr, cc = np.nonzero(same & (tid >= 0))
        ray = np.stack([(cc + 0.5 - cx) / fx, (rr + 0.5 - cy) / fy, np.ones(len(rr))], -1)
        got = d[b][rr, cc].astype(np.float64)
        want = _moller_trumbore(cam[f[tid[rr, cc]]], ray)
        raw.append(np.abs(got - want) / want)
        want = _moller_trumbore(snap[f[tid[rr, cc]]], ray)
        snapped.append(np.abs(got - want) / want)
    raw, snapped = np.concatenate(raw), np.concatenate(snapped)
    print("ray cast: %d interior pixels; unsnapped geometry: relative error max %.3g, 99.5th percentile %.3g, <= 1e-5: %.5f, "
          "<= 2e-5: %.5f; snapped geometry: max %.3g" % (raw.size, raw.max(), np.percentile(raw, 99.5), (raw <= 1e-5).mean(),
                                                         (raw <= 2e-5).mean(), snapped.max()))
    assert raw.size > 10000
    assert snapped.max() <= 1e-6
    assert (raw <= 2e-5).mean() >= 0.995
    assert raw.max() <= 1e-3


# ---- batch invariance, overflow ----------------------------------------------------------------------------------------
def test_views_do_not_depend_on_the_batch():
    dev = _gpu()
    fx = _fixture()
    sphere = RR.icosphere(3, 0.1)
    rng = np.random.default_rng(4)
    fposes = _fixture_poses(8, True, seed=5)
    sposes = [RR.look_pose(RR.random_rotation(rng), [rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(0.5, 1.5)])
              for _ in range(8)]
    meshes = [fx, sphere] * 8
    poses = [p for pair in zip(fposes, sposes) for p in pair]
    dB, tB = _views(meshes, poses, 1, dev)
    dB2, tB2 = _views(meshes, poses, 1, dev)
    assert np.array_equal(dB.view(np.uint32), dB2.view(np.uint32)) and np.array_equal(tB, tB2)
    for b in (0, 1, 6, 15):
        d1, t1 = _views([meshes[b]], [poses[b]], 1, dev)
        assert np.array_equal(d1[0].view(np.uint32), dB[b].view(np.uint32)) and np.array_equal(t1[0], tB[b]), b


def test_list_overflow_reports_the_need_and_the_wrapper_retries(monkeypatch):
    import ctypes as C

    import torch
    from cppf2_amd import _lib, ops, render
    dev = _gpu()
    v, f = _fixture()
    poses = _fixture_poses(4, False, seed=8)
    verts = torch.as_tensor(v.astype(np.float32)).to(dev)
    tris = torch.as_tensor(np.tile(f, (4, 1))).to(dev)
    tri_off = ops._offsets([len(f)] * 4, dev)
    P = torch.as_tensor(np.stack(poses)).to(dev)
    L = _lib.load()
    hK = (C.c_double * 4)(K[0, 0], K[1, 1], K[0, 2], K[1, 2])

    def raw(cap):
        nb = L.cppf_render_depth_workspace_bytes(4, tris.shape[0], H, W, cap)
        ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
        depth = torch.empty((4, H, W), dtype=torch.float32, device=dev)
        ids = torch.empty((4, H, W), dtype=torch.int32, device=dev)
        st = torch.empty((2,), dtype=torch.int64, device=dev)
        _lib.check(L.cppf_render_depth(4, ops._p(verts), verts.shape[0], ops._p(tris), ops._p(tri_off), tris.shape[0], ops._p(P), hK,
                                       H, W, C.c_float(0.05), C.c_float(100.0), 1, ops._p(depth), ops._p(ids), ops._p(st),
                                       ops._p(ws), nb, cap, ops._stream()), "cppf_render_depth")
        return depth.cpu().numpy(), ids.cpu().numpy(), st.cpu().numpy()
    d_big, t_big, st_big = raw(1 << 22)
    need = int(st_big[1])
    assert st_big[0] == 0 and 0 < need < (1 << 22)
    d_small, t_small, st_small = raw(100)
    assert int(st_small[1]) == need and st_small[0] == 0
    assert not d_small.any() and (t_small == -1).all()            # marked invalid: nothing written
    d_ok, t_ok, _ = raw(need)                                       # exactly enough
    assert np.array_equal(d_ok.view(np.uint32), d_big.view(np.uint32)) and np.array_equal(t_ok, t_big)
    # the wrapper: a tiny cached workspace is grown and the call issued again; the next call needs no retry
    render._WS.clear()
    monkeypatch.setattr(render, "INITIAL_CAPACITY", 64)
    d, t = render.render_depth(verts, tris, tri_off, P, K, H, W, with_ids=True)
    assert np.array_equal(d.cpu().numpy().view(np.uint32), d_big.view(np.uint32)) and np.array_equal(t.cpu().numpy(), t_big)
    cap = render._WS[render.shot._key(dev)][1]
    assert cap >= need
    render.render_depth(verts, tris, tri_off, P, K, H, W)
    assert render._WS[render.shot._key(dev)][1] == cap
    # a triangle crossing the near plane is rejected loudly
    near = torch.as_tensor(np.array([[0, 0, 0.01], [0.1, 0, 1.0], [0, 0.1, 1.0]], np.float32)).to(dev)
    with pytest.raises(_lib.CppfError):
        render.render_depth(near, torch.as_tensor(np.array([[0, 1, 2]], np.int32)).to(dev), ops._offsets([1], dev),
                            torch.as_tensor(RR.look_pose(np.eye(3), np.zeros(3))[None]).to(dev), K, H, W)


# ---- items -------------------------------------------------------------------------------------------------------------
def test_item_geometry():
    from scipy.spatial import cKDTree
    from cppf2_amd import render
    _gpu()
    m = render.load_mesh(FIXTURE, 0.001)
    items = render.make_items(m, range(32), seed=0, full_rot=True)
    c = (m.bounds[0] + m.bounds[1]) / 2
    lo, hi = m.bounds[0] - c, m.bounds[1] - c
    # dense surface samples of the centred mesh
    rng = np.random.default_rng(0)
    tri = (m.verts - c)[m.faces]
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    pick = rng.choice(len(tri), 600000, p=area / area.sum())
    a, b = rng.random((2, len(pick), 1))
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    surf = tri[pick, 0] + a * (tri[pick, 1] - tri[pick, 0]) + b * (tri[pick, 2] - tri[pick, 0])
    tree = cKDTree(surf)
    worst = 0.0
    for it in items:
        assert set(it) == {"pc", "pc_canon", "trans", "quat", "bound", "scale", "point_idxs_all", "depth", "idxs", "shot", "normal"}
        n = it["pc"].shape[0]
        assert n >= 100 and it["shot"].shape == (n, 352) and it["normal"].shape == (n, 3) and it["idxs"].shape == (n, 2)
        assert it["point_idxs_all"].shape == (10000, 5) and it["depth"].shape == (H, W)
        assert np.isfinite(it["shot"]).all() and np.isfinite(it["normal"]).all()
        from scipy.spatial.transform import Rotation
        q = it["quat"]
        rot = Rotation.from_quat([q[1], q[2], q[3], q[0]]).as_matrix()
        back = it["pc_canon"].astype(np.float64) * it["scale"] @ rot.T + it["trans"]
        assert np.abs(back - it["pc"]).max() < 1e-5
        canon = it["pc_canon"].astype(np.float64) * it["scale"]
        foot = it["pc"][:, 2:3] / K[0, 0]
        assert ((canon >= lo - foot) & (canon <= hi + foot)).all()
        dist, _ = tree.query(canon)
        frac = (dist <= foot[:, 0]).mean()
        worst = max(worst, np.median(dist))
        assert frac >= 0.9, frac
        np.testing.assert_allclose(it["bound"], m.bounds[1] - m.bounds[0], rtol=1e-6)
        assert it["scale"] == np.float32(it["bound"].max())
    print("median distance to the surface, worst item: %.3g m" % worst)


def _read_dir(d):
    out = {}
    for p in sorted(glob.glob(os.path.join(d, "*.pkl"))):
        with open(p, "rb") as f:
            out[os.path.basename(p)] = pickle.load(f)
    return out


def test_cli_items_are_batch_invariant_and_train(tmp_path):
    from cppf2_amd import render
    from cppf2_amd.training import ExportedItems
    _gpu()
    out64 = str(tmp_path / "b64")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "cppf2_amd.render", "--mesh", FIXTURE, "--mesh-scale", "0.001", "--count", "64",
                        "--out", out64, "--batch", "64"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    a = _read_dir(out64)
    assert sorted(a) == ["{:06d}.pkl".format(i) for i in range(64)]
    out1 = str(tmp_path / "b1")
    render.generate(FIXTURE, out1, 64, mesh_scale=0.001, batch=1)
    b = _read_dir(out1)
    assert sorted(a) == sorted(b)
    for k in a:
        assert set(a[k]) == {"pc", "pc_canon", "bound", "shot", "normal"} and a[k]["pc"].shape == (100, 3)
        for key in a[k]:
            assert np.array_equal(np.asarray(a[k][key]), np.asarray(b[k][key])), (k, key)
    ds = ExportedItems(out64, length=8)
    it = ds[3]
    assert it["pc"].shape == (100, 3) and it["shot"].shape == (100, 352) and "desc" not in it
    run = str(tmp_path / "run")
    r = subprocess.run([sys.executable, "train_shot.py", "category=bottle", "data_dir=%s" % out64, "max_epochs=1",
                        "iters_per_epoch=8", "hydra.run.dir=%s" % run], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("epoch 0 ")][-1]
    cls, scale = float(line.split()[3]), float(line.split()[5])
    assert np.isfinite(cls) and np.isfinite(scale), line
    assert os.path.exists(os.path.join(run, "lightning_logs", "version_0", "checkpoints", "last.ckpt"))


def _bottle_obj(path, radius, height, n=24):
    """A closed, outward-wound cylinder with a narrower neck, as an OBJ with quads and v//vn faces."""
    lines = []
    rings = [(0.0, radius), (0.7 * height, radius), (0.85 * height, 0.4 * radius), (height, 0.4 * radius)]
    for y, r in rings:
        for k in range(n):
            a = 2 * np.pi * k / n
            lines.append("v %.6f %.6f %.6f" % (r * np.cos(a), y, r * np.sin(a)))
    lines.append("v 0 0 0")
    lines.append("v 0 %.6f 0" % height)
    lines.append("vn 0 1 0")
    nv = len(rings) * n
    for i in range(len(rings) - 1):
        for k in range(n):
            a, b = i * n + k + 1, i * n + (k + 1) % n + 1
            lines.append("f %d//1 %d//1 %d//1 %d//1" % (a, a + n, b + n, b))
    for k in range(n):
        lines.append("f %d %d %d" % (nv + 1, k + 1, (k + 1) % n + 1))
        lines.append("f %d %d %d" % (nv + 2, (len(rings) - 1) * n + (k + 1) % n + 1, (len(rings) - 1) * n + k + 1))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_shapenet_layout_and_dump(tmp_path, monkeypatch):
    import dataset
    from cppf2_amd.config import load_config
    from utils.util import map_sym
    from scipy.spatial.transform import Rotation
    _gpu()
    root = tmp_path / "ShapeNetCore.v2"
    _bottle_obj(str(root / "02876657" / "m1" / "models" / "model_normalized.obj"), 0.2, 0.9)
    _bottle_obj(str(root / "02876657" / "m2" / "models" / "model_normalized.obj"), 0.3, 0.8, n=17)
    (tmp_path / "data").mkdir()
    (tmp_path / "data" / "shapenet_train.txt").write_text("1 02876657/m1\n2 02880940/other\n")
    (tmp_path / "data" / "shapenet_val.txt").write_text("1 02876657/m2\n")
    monkeypatch.chdir(tmp_path)
    cfg = load_config("config", "config", ["category=bottle"])
    ds = dataset.ShapeNetDirectDataset(cfg, shapenet_root=str(root))
    assert len(ds) == 2
    it = ds[1]
    n = it["pc"].shape[0]
    assert n >= 100 and it["pc_canon"].shape == (n, 3) and it["shot"].shape == (n, 352) and it["point_idxs_all"].shape == (10000, 5)
    assert "rgb" not in it and it["depth"].shape == (480, 640) and it["idxs"].shape == (n, 2)
    q = it["quat"]
    rot = Rotation.from_quat([q[1], q[2], q[3], q[0]]).as_matrix()
    np.testing.assert_allclose(map_sym(rot.T, 1).T, rot, atol=1e-6)          # already mapped: idempotent
    ext = ds.mesh(1).bounds[1] - ds.mesh(1).bounds[0]
    s = float(it["scale"]) / ext.max()                                        # the size drawn for the view
    assert 0.16 <= s <= 0.25                                                  # shapenet_obj_scales['02876657']
    np.testing.assert_allclose(it["bound"], ext[[2, 1, 0]] * s, rtol=1e-5)     # flip2nocs swaps x and z
    again = dataset.ShapeNetDirectDataset(cfg, shapenet_root=str(root))[1]
    for k in it:
        assert np.array_equal(np.asarray(it[k]), np.asarray(again[k])), k
    dataset.dump_data(False, categories=[1], draws=2, batch=2, shapenet_root=str(root))
    files = sorted(os.listdir(tmp_path / "data" / "category_training_data" / "1"))
    assert files == ["{:06d}.pkl".format(i) for i in range(4)]
    rd = dataset.ShapeNetExportDataset(cfg)
    assert rd[0]["pc"].shape == (100, 3)
