"""CPU checks of the training-item generator (cppf2_amd/render.py): mesh loaders, the rasterizer's arithmetic through its NumPy
mirror (tests/render_ref.py: no holes, top-left rule), map_sym against the reference, the pose samplers, and the two new C
entry points' argument checks (no GPU needed)."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_ref as RR  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "example_data", "obj_000015.ply")
K = np.array([[591.0125, 0, 320], [0, 590.16775, 240], [0, 0, 1]])


# ---- loaders ----------------------------------------------------------------------------------------------------------
def test_fixture_ply_parses():
    from cppf2_amd import render
    v, f = render.load_ply(FIXTURE)
    assert v.shape == (9174, 3) and f.shape == (15728, 3) and f.dtype == np.int32
    assert f.min() == 0 and f.max() == 9173
    np.testing.assert_allclose(v[0], [-35.7155, -91.137, 8.2525])
    m = render.load_mesh(FIXTURE, 0.001)
    assert m is render.load_mesh(FIXTURE, 0.001)                       # parsed once per process
    np.testing.assert_allclose(m.verts, v * 0.001)


def test_binary_ply_roundtrip(tmp_path):
    from cppf2_amd import render
    v, f = RR.icosphere(2)
    # binary little endian with an extra vertex property and a quad, plus an element after the faces
    quads = [(0, 1, 2, 3)]
    p = tmp_path / "m.ply"
    with open(p, "wb") as fh:
        fh.write(("ply\nformat binary_little_endian 1.0\ncomment procedural\nelement vertex %d\nproperty float x\n"
                  "property float y\nproperty float z\nproperty uchar red\nelement face %d\n"
                  "property list uchar int vertex_indices\nelement edge 1\nproperty int vertex1\nproperty int vertex2\n"
                  "end_header\n" % (len(v), len(f) + len(quads))).encode())
        for x in v:
            fh.write(struct.pack("<fffB", *x, 7))
        for t in f:
            fh.write(struct.pack("<B3i", 3, *t))
        for q in quads:
            fh.write(struct.pack("<B4i", 4, *q))
        fh.write(struct.pack("<2i", 0, 1))
    gv, gf = render.load_ply(str(p))
    np.testing.assert_array_equal(gv, v.astype(np.float32).astype(np.float64))
    np.testing.assert_array_equal(gf, np.concatenate([f, [[0, 1, 2], [0, 2, 3]]]))
    # the fast path (all triangles) too
    p2 = tmp_path / "t.ply"
    with open(p2, "wb") as fh:
        fh.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty double x\nproperty double y\n"
                  "property double z\nelement face %d\nproperty list uchar uint vertex_index\nend_header\n" % (len(v), len(f))).encode())
        fh.write(np.ascontiguousarray(v, "<f8").tobytes())
        for t in f:
            fh.write(struct.pack("<B3I", 3, *t))
    gv, gf = render.load_ply(str(p2))
    np.testing.assert_array_equal(gv, v)
    np.testing.assert_array_equal(gf, f)


def test_obj_parses_quads_slashes_negative_indices(tmp_path):
    from cppf2_amd import render
    p = tmp_path / "m.obj"
    p.write_text("# comment\nmtllib m.mtl\no thing\ng group1\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\n"
                 "usemtl a\ns off\nf 1/1/1 2/1/1 3/1/1 4/1/1\ng group2\nv 0 0 1\nv 1 0 1\nv 1 1 1\n"
                 "f -3//1 -2//1 -1//1\nf 5/1 6/1 7/1\n")
    v, f = render.load_obj(str(p))
    assert v.shape == (7, 3)
    np.testing.assert_array_equal(f, [[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 5, 6]])


# ---- the mirror's coverage rules ----------------------------------------------------------------------------------
def _convex_inside(pts2, H, W, margin=0.02):
    """Pixels whose sample point (c+0.5, r+0.5) lies strictly inside the convex hull of pts2 (by more than `margin` px)."""
    from scipy.spatial import ConvexHull
    hull = ConvexHull(pts2)
    r, c = np.mgrid[0:H, 0:W]
    q = np.stack([c.ravel() + 0.5, r.ravel() + 0.5], -1)
    eq = hull.equations                       # n . x + d <= 0 inside, |n| = 1
    return ((q @ eq[:, :2].T + eq[:, 2]) < -margin).all(1).reshape(H, W)


@pytest.mark.parametrize("k", range(4))
def test_mirror_has_no_holes_on_an_icosphere(k):
    rng = np.random.default_rng(k)
    v, f = RR.icosphere(2, 0.1)
    R = RR.random_rotation(rng)
    t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.4, 1.0)])
    H, W = 96, 128
    Kk = np.array([[300.0, 0, 61.3], [0, 290.0, 47.1], [0, 0, 1]])
    pose = RR.look_pose(R, t)
    depth, tid, rej, count = RR.render(v, f, pose, Kk, H, W, cull=1, with_count=True)
    assert rej == 0
    cam = v @ R.T + t
    uv = np.stack([Kk[0, 0] * cam[:, 0] / cam[:, 2] + Kk[0, 2], Kk[1, 1] * cam[:, 1] / cam[:, 2] + Kk[1, 2]], -1)
    inside = _convex_inside(uv, H, W)
    assert inside.sum() > 500
    assert (depth[inside] > 0).all() and (tid[inside] >= 0).all()
    assert count.max() == 1                      # front faces of a convex mesh: no pixel twice
    # without culling every inside pixel is covered exactly twice (front and back), and the front wins
    d2, t2, _, c2 = RR.render(v, f, pose, Kk, H, W, cull=0, with_count=True)
    assert (c2[inside] == 2).all() and c2.max() <= 2
    np.testing.assert_array_equal(d2, depth)


def _square(winding_front=True):
    """Two triangles with corners at pixel centres (2.5, 2.5) .. (6.5, 6.5) sharing the diagonal through (3.5, 3.5) .. ."""
    fx = 100.0
    pts = np.array([[2.5, 2.5], [6.5, 2.5], [6.5, 6.5], [2.5, 6.5]]) / fx
    v = np.concatenate([pts, np.ones((4, 1))], 1)
    f = np.array([[0, 2, 1], [0, 3, 2]] if winding_front else [[0, 1, 2], [0, 2, 3]], np.int32)
    return v, f, np.array([[fx, 0, 0], [0, fx, 0], [0, 0, 1.0]])


@pytest.mark.parametrize("front", [True, False])
def test_top_left_rule_on_a_shared_edge_through_pixel_centres(front):
    v, f, Kk = _square(front)
    depth, tid, rej, count = RR.render(v, f, RR.look_pose(np.eye(3), np.zeros(3)), Kk, 10, 10, cull=0, with_count=True)
    want = np.zeros((10, 10), bool)
    want[2:6, 2:6] = True                         # top and left edges in, bottom and right out
    np.testing.assert_array_equal(count, want.astype(np.int32))
    np.testing.assert_array_equal(depth[want], np.ones(want.sum(), np.float32))
    # the diagonal's pixels (3,3), (4,4), (5,5) go to the triangle whose top-left edge it is, exactly once
    assert all(tid[i, i] in (0, 1) for i in range(2, 6))
    # back-facing with culling: nothing
    d, _, _ = RR.render(v, f, RR.look_pose(np.eye(3), np.zeros(3)), Kk, 10, 10, cull=1)
    assert (d > 0).any() == front


def test_top_left_rule_with_a_vertex_on_a_pixel_centre():
    fx = 100.0
    v = np.array([[2.5, 2.5, 1], [2.5, 6.5, 1], [6.5, 2.5, 1]]) / np.array([fx, fx, 1])
    f = np.array([[0, 1, 2]], np.int32)
    Kk = np.array([[fx, 0, 0], [0, fx, 0], [0, 0, 1.0]])
    depth, tid, rej, count = RR.render(v, f, RR.look_pose(np.eye(3), np.zeros(3)), Kk, 10, 10, cull=1, with_count=True)
    r, c = np.mgrid[0:10, 0:10]
    want = (c >= 2) & (r >= 2) & (c + r < 8)      # the hypotenuse (a bottom-right edge) is out
    np.testing.assert_array_equal(count > 0, want)
    assert count[2, 2] == 1 and tid[2, 2] == 0


def test_mirror_rejects_triangles_crossing_the_near_plane():
    v = np.array([[0, 0, 0.01], [0.1, 0, 1.0], [0, 0.1, 1.0]])
    _, _, rej = RR.render(v, np.array([[0, 1, 2]], np.int32), RR.look_pose(np.eye(3), np.zeros(3)), K, 48, 64, cull=0)
    assert rej == 1


# ---- map_sym -------------------------------------------------------------------------------------------------------
def test_map_sym_matches_the_reference(tmp_path):
    """The reference's map_sym / map_sym_discrete (utils/util.py:66-81) run in a child process: loading the reference installs
    stub modules for its absent third-party imports, which must not leak into this test session."""
    if not os.path.isdir("/root/reference"):
        pytest.skip("the reference tree is not available")
    import subprocess
    from utils import util
    rng = np.random.default_rng(3)
    syms = np.stack([RR.random_rotation(rng) for _ in range(4)])
    rots = np.stack([RR.random_rotation(rng) for _ in range(20)])
    np.savez(tmp_path / "in.npz", syms=syms, rots=rots)
    code = ("import sys, numpy as np; sys.path.insert(0, %r); from _ref_loader import load_reference; u = load_reference().util; "
            "d = np.load(%r); s = list(d['syms']); "
            "np.savez(%r, sym=np.stack([[u.map_sym(R, a) for a in range(3)] for R in d['rots']]), "
            "disc=np.stack([u.map_sym_discrete(R, s) for R in d['rots']]))"
            % (os.path.join(ROOT, "tests", "golden"), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=str(tmp_path))
    ref = np.load(tmp_path / "out.npz")
    for i, R in enumerate(rots):
        for axis in range(3):
            np.testing.assert_array_equal(util.map_sym(R, axis), ref["sym"][i, axis])
        np.testing.assert_array_equal(util.map_sym_discrete(R, list(syms)), ref["disc"][i])


def test_map_sym_removes_the_rotation_about_the_axis():
    from utils.util import map_sym
    rng = np.random.default_rng(5)
    for axis in range(3):
        R = RR.random_rotation(rng)
        M = map_sym(R, axis)
        o = [a for a in range(3) if a != axis]
        m = M[np.ix_(o, o)]
        assert abs(m[1, 0] - m[0, 1]) < 1e-12 and abs(np.linalg.det(M) - 1) < 1e-12


# ---- pose samplers -------------------------------------------------------------------------------------------------
def test_pose_samplers_ranges_and_reproducibility():
    import dataset
    from cppf2_amd import render
    for a in (0.3, -1.2):
        np.testing.assert_allclose(render.rotx(a), dataset.rotx(a)[:3, :3])
        np.testing.assert_allclose(render.roty(a), dataset.roty(a)[:3, :3])
    for full in (False, True):
        for item in range(200):
            R, tr = render.sample_pose(render.item_rng(7, item), full)
            assert abs(np.linalg.det(R) - 1) < 1e-9 and np.allclose(R @ R.T, np.eye(3), atol=1e-9)
            assert -0.3 <= tr[0] <= 0.3 and -0.3 <= tr[1] <= 0.3 and -2.0 <= tr[2] <= -0.6
            if not full:
                # roty(yy) rotx(x) roty(y) e_y = (-sin x sin yy, cos x, sin x cos yy)
                x = np.arccos(R[1, 1])
                yy = np.arctan2(-R[0, 1], R[2, 1])
                assert np.radians(10) - 1e-9 <= x <= np.radians(80) + 1e-9
                assert abs(yy) <= np.radians(20) + 1e-9
            R2, tr2 = render.sample_pose(render.item_rng(7, item), full)
            assert np.array_equal(R, R2) and np.array_equal(tr, tr2)
        Ra, _ = render.sample_pose(render.item_rng(7, 1), full)
        Rb, _ = render.sample_pose(render.item_rng(7, 2), full)
        Rc, _ = render.sample_pose(render.item_rng(8, 1), full)
        assert not np.array_equal(Ra, Rb) and not np.array_equal(Ra, Rc)
    # uniform SO(3): the rotated z axis covers the sphere (mean near 0)
    zs = np.array([render.sample_pose(render.item_rng(0, i), True)[0][:, 2] for i in range(2000)])
    assert np.abs(zs.mean(0)).max() < 0.06


# ---- the C entry points without a GPU ------------------------------------------------------------------------------
def test_render_entry_points_load_and_validate_arguments():
    from cppf2_amd import _lib
    lib = _lib.load()
    ws = lib.cppf_render_depth_workspace_bytes
    base = ws(1, 1000, 480, 640, 4096)
    assert base > 0
    assert ws(2, 1000, 480, 640, 4096) > base and ws(1, 2000, 480, 640, 4096) > base and ws(1, 1000, 480, 640, 8192) > base
    assert ws(0, 1000, 480, 640, 4096) == -1 and ws(1, -1, 480, 640, 4096) == -1 and ws(1, 10, 0, 640, 1) == -1
    assert ws(1, 10, 480, 9000, 1) == -1 and ws(1, 10, 480, 640, -1) == -1
    hK = (C.c_double * 4)(591.0, 590.0, 320.0, 240.0)
    fake = C.c_void_p(0x1000)           # never dereferenced: every call below fails its argument check first
    good = dict(B=1, verts=fake, nv=3, tris=fake, tri_off=fake, T=1, poses=fake, hK=hK, H=48, W=64, zn=0.05, zf=100.0, cull=1,
                depth=fake, ids=None, status=fake, ws=fake, wsb=1 << 30, cap=16)

    def call(**kw):
        a = dict(good, **kw)
        return lib.cppf_render_depth(a["B"], a["verts"], a["nv"], a["tris"], a["tri_off"], a["T"], a["poses"], a["hK"], a["H"],
                                     a["W"], a["zn"], a["zf"], a["cull"], a["depth"], a["ids"], a["status"], a["ws"], a["wsb"],
                                     a["cap"], None)
    for bad in (dict(verts=None), dict(tris=None), dict(tri_off=None), dict(poses=None), dict(hK=None), dict(depth=None),
                dict(status=None), dict(ws=None), dict(wsb=16), dict(B=0), dict(H=0), dict(W=9000), dict(cull=2), dict(zn=0.0),
                dict(zf=0.01), dict(cap=-1), dict(nv=0), dict(T=-1), dict(hK=(C.c_double * 4)(0.0, 590.0, 320.0, 240.0))):
        assert call(**bad) == -1, bad
        assert b"invalid argument" in lib.cppf_last_error_string()
