"""CPU checks of mesh simplification: the NumPy restatement (tests/simplify_ref.py) on the fused sphere
of tests/fuse_ref.py, on the drill fixture and on crafted clusters -- the properties the definition promises, each crafted
representative against an independent float64 least-squares solution --, the wrapper's face rules on torch's CPU device, the
entry points' validation through ctypes and the command lines' argument errors.  The kernels themselves:
tests/test_simplify_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuse_ref  # noqa: E402
import simplify_ref as ref  # noqa: E402

VOXEL = fuse_ref.VOXEL
SPHERE_VOLUME = 4.0 / 3.0 * np.pi * fuse_ref.RADIUS ** 3
# triangles out per cell size: what the definition gives on these two meshes (DESIGN.md section 29's tables)
SPHERE_TRIANGLES = {1.0: 5956, 1.5: 2342, 2.0: 1496, 3.0: 624, 4.0: 392}
DRILL_TRIANGLES = {0.002: 14830, 0.004: 7826, 0.008: 2122}


def _volume_error(verts, faces):
    return fuse_ref.signed_volume(verts, faces) / SPHERE_VOLUME - 1.0


@pytest.mark.parametrize("cell", ref.SPHERE_CELLS)
def test_fused_sphere_stays_closed_within_one_voxel(cell):
    v, f, rep, _ = ref.sphere_cluster(cell)
    assert rep["triangles_in"] == 17852 and rep["triangles_out"] == len(f) == SPHERE_TRIANGLES[cell]
    dist, vol = fuse_ref.sphere_distance(v).max() / VOXEL, _volume_error(v, f)
    print("sphere, cell %.1f voxel: %d triangles, %d non-manifold edges, max distance %.2f voxel, volume %+.2f %%"
          % (cell, len(f), rep["nonmanifold_edges"], dist, 100 * vol))
    assert rep["boundary_edges"] == 0 and rep["multi"] == 0 and ref.euler(v, f) == 2
    assert dist <= 1.0
    assert abs(vol) <= 0.03


def test_the_quadric_keeps_the_volume_the_mean_loses():
    """lam = 1e6 makes the representative the area-weighted mean of the cell's triangles: on a convex surface it lies inside."""
    q = _volume_error(*ref.sphere_cluster(3.0)[:2])
    m = _volume_error(*ref.sphere_cluster(3.0, 1e6)[:2])
    print("sphere, cell 3 voxel: volume %+.2f %% with the quadric, %+.2f %% with the mean" % (100 * q, 100 * m))
    assert abs(q) < 0.5 * abs(m)


@pytest.mark.parametrize("cell", ref.DRILL_CELLS)
def test_drill_seams_are_welded_within_the_cell_diagonal(cell):
    v0, f0, _ = ref.drill_mesh()
    assert ref.edge_counts(f0)[0] == 2562 and len(f0) == 15728
    v, f, rep, _ = ref.drill_cluster(cell)
    a, b = ref.drill_deviation(cell)
    print("drill, cell %g mm: %d triangles, %d non-manifold edges, multi %d, deviation %.2f / %.2f cell"
          % (1e3 * cell, len(f), rep["nonmanifold_edges"], rep["multi"], a / cell, b / cell))
    assert rep["triangles_out"] == DRILL_TRIANGLES[cell]
    assert rep["boundary_edges"] == 0
    bound = np.sqrt(3.0) * cell + 1e-6
    assert a <= bound and b <= bound


# ----------------------------------------------------------------------------------------------
# crafted clusters against an independent solution of the stated minimisation
# ----------------------------------------------------------------------------------------------
def _independent(verts, faces, S, c, lam=ref.LAMBDA):
    """float64 [3]: the minimiser of sum area (u . x - d)^2 + lam area |x - centroid|^2 over the triangles of cluster c's corners
    (one term per corner), relative to the cell's centre, by numpy.linalg.lstsq on the stacked rows; clamped into the cell.  The
    mean of the corners when no triangle has area."""
    v, ctr = np.asarray(verts, dtype=np.float64), S["ctr"][c]
    rows, rhs, pts = [], [], []
    for corner in S["corners"][S["seg_off"][c]:S["seg_off"][c + 1]]:
        p = v[faces[corner // 3]] - ctr
        pts.append(p[corner % 3])
        n = np.cross(p[1] - p[0], p[2] - p[0])
        area = 0.5 * np.linalg.norm(n)
        if not area > 0:
            continue
        u = n / np.linalg.norm(n)
        rows += [np.sqrt(area) * u[None], np.sqrt(lam * area) * np.eye(3)]
        rhs += [[np.sqrt(area) * (u @ p[0])], np.sqrt(lam * area) * p.mean(0)]
    x = np.linalg.lstsq(np.concatenate(rows), np.concatenate(rhs), rcond=None)[0] if rows else np.mean(pts, 0)
    h = float(ref.CELL) / 2
    return np.clip(x, -h, h)


def _check_against_independent(name, clusters=None):
    v, f = ref.crafted()[name]
    _, _, _, S = ref.crafted_cluster(name)
    x = ref.solve(S, ref.CELL)
    worst = 0.0
    for c in range(len(S["keys"])) if clusters is None else clusters:
        worst = max(worst, np.abs(x[c] - _independent(v, f, S, c)).max())
    print("%s: largest difference to the independent solution %.2e cell" % (name, worst / float(ref.CELL)))
    assert worst <= 1e-9 * float(ref.CELL)              # the system's condition number is at most 1001
    return S, x


def test_one_triangle_in_three_cells_has_rank_one_quadrics():
    S, x = _check_against_independent("one_triangle")
    assert (np.diff(S["seg_off"]) == 1).all() and len(x) == 3
    v, f = ref.crafted()["one_triangle"]
    p = v.astype(np.float64)
    u = np.cross(p[1] - p[0], p[2] - p[0])
    u /= np.linalg.norm(u)
    # the plane term has weight 1 and the pull towards the centroid lam: the representative stays within lam x |centroid - plane| = 0 of
    # the plane, wherever the clamp is idle
    idle = (np.abs(x) < float(ref.CELL) / 2).all(1)
    assert idle.any()
    assert (np.abs((S["ctr"] + x - p[0]) @ u)[idle] <= 1e-9 * float(ref.CELL)).all()


def test_plate_representatives_lie_on_the_plate():
    S, x = _check_against_independent("plate")
    v, _ = ref.crafted()["plate"]
    idle = (np.abs(x) < float(ref.CELL) / 2).all(1)
    assert np.array_equal(v.astype(np.float64), ref._plate()[0] * float(ref.CELL))            # the vertices are exact: one plane
    off = np.abs((S["ctr"] + x - v[0].astype(np.float64)) @ ref.PLATE_NORMAL) / float(ref.CELL)
    print("plate: %d of %d clusters unclamped, farthest %.2e cell off the plate" % (idle.sum(), len(x), off[idle].max()))
    assert idle.sum() * 2 >= len(x)
    assert (off[idle] <= 1e-9).all()


def test_cube_corner_is_recovered_up_to_the_regulariser():
    """Three orthogonal faces: A = (w / 3) I, so x = (corner + 3 lam centroid) / (1 + 3 lam): the pull is 3 lam |centroid - corner|
    / (1 + 3 lam), with the mean of the three faces' centroids (1/3, 1/3, 1/3) cells from the corner: 1.7e-3 cell."""
    S, x = _check_against_independent("cube_corner")
    c = int(np.argmax(np.diff(S["seg_off"])))
    assert S["seg_off"][c + 1] - S["seg_off"][c] == 3
    v, _ = ref.crafted()["cube_corner"]
    off = np.linalg.norm(S["ctr"][c] + x[c] - v[0].astype(np.float64)) / float(ref.CELL)
    want = 3 * ref.LAMBDA * (np.sqrt(3.0) / 3.0) / (1 + 3 * ref.LAMBDA)
    print("cube corner: the representative is %.3e cell from the corner (3 lam |centroid - corner| / (1 + 3 lam) = %.3e)" % (off, want))
    assert abs(off - want) <= 1e-6


def test_zero_area_triangles_take_the_mean_of_the_corners():
    S, x = _check_against_independent("zero_area")
    assert (S["w"] == 0).all() and (S["count"] > 0).all()
    v, f = ref.crafted()["zero_area"]
    # cell 0 holds vertices 0 (corners of faces 0, 2, 2) and 3 (face 1)
    want = (3 * v[0].astype(np.float64) + v[3].astype(np.float64)) / 4 - S["ctr"][0]
    assert np.abs(x[0] - want).max() <= 1e-9 * float(ref.CELL)
    assert not np.isnan(ref.crafted_cluster("zero_area")[3]["pos"]).any()


def test_everything_in_one_cell_leaves_nothing():
    v, f, rep, S = ref.crafted_cluster("one_cell")
    assert v.shape == (0, 3) and f.shape == (0, 3) and rep["collapsed"] == 4 and rep["triangles_out"] == rep["vertices_out"] == 0
    assert len(S["keys"]) == 1 and S["seg_off"].tolist() == [0, 12]
    ev, ef, erep = ref.cluster(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), ref.CELL)
    assert ev.shape == (0, 3) and ef.shape == (0, 3) and erep["triangles_in"] == 0


@pytest.mark.parametrize("k", [64, 65, 1000])
def test_fan_around_one_vertex(k):
    S, x = _check_against_independent("fan_%d" % k)
    lens = np.diff(S["seg_off"])
    assert lens.max() == k and (lens == k).sum() == 1


def test_mirror_images_cancel_and_duplicates_count_as_multi():
    v, f, rep, _ = ref.crafted_cluster("mirror_double")
    assert (rep["cancelled"], rep["multi"], rep["collapsed"], len(f)) == (2, 1, 0, 1)
    # vertices 3, 4, 5 lie in cells (4,4,0), (6,4,0), (4,6,0): in key order vertex 5 comes before vertex 4; the winding is kept
    assert f.tolist() == [[0, 2, 1]] and len(v) == 3
    kept, counts = ref.reduce_faces(np.array([[0, 1, 2], [1, 2, 0], [2, 1, 0], [5, 4, 3], [3, 5, 4], [4, 5, 3], [7, 7, 8]]))
    # group (0,1,2): even, even, odd -> net +1, the first even one stays; group (3,4,5): odd, odd, even -> net -1, the first odd one
    assert kept.tolist() == [0, 3] and counts == dict(collapsed=1, cancelled=0, multi=0)
    kept, counts = ref.reduce_faces(np.array([[2, 1, 0], [2, 1, 0], [0, 1, 2], [1, 0, 2]]))
    assert kept.tolist() == [0] and counts == dict(collapsed=0, cancelled=0, multi=1)      # net -2: the first odd one


def test_a_vertex_outside_the_lattice_is_refused_only_when_a_face_uses_it():
    v, f = ref.crafted()["one_triangle"]
    far = np.concatenate([v, [[np.nan, 0, 0], [-1.0, 0, 0], [3e4, 0, 0]]]).astype(np.float32)       # 3e4 m / 0.01 m > 2^21 cells
    got = ref.cluster(far, f, ref.CELL, np.zeros(3, np.float32))
    want = ref.crafted_cluster("one_triangle")
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and got[2]["vertices_in"] == 6
    for bad in (3, 4, 5):
        with pytest.raises(ValueError, match="1 vertices"):
            ref.cluster(far, np.array([[0, 1, bad]]), ref.CELL, np.zeros(3, np.float32))
    assert ref.cluster(far, f, ref.CELL)[2]["triangles_out"] == 1          # the default origin looks at used vertices only


def test_key_rule():
    (a, oa, ca), (b, ob, cb) = ref.key_cases()
    ka, kb = ref.cluster_keys(a, oa, ca), ref.cluster_keys(b, ob, cb)
    cell = lambda i, j, k: i << 42 | j << 21 | k
    assert ka[:8].tolist() == [0, cell(3, 3, 3), cell(2, 2, 2), -1, -1, -1, -1, 0]        # on a boundary: the upper cell
    top = (1 << 21) - 1
    assert kb[:13].tolist() == [0, 0, cell(top, top, top), -1, -1, -1, -1, -1, -1, -1, -1, cell(top, 0, 5), cell(top, 2, 3)]
    assert (ka[8:] >= 0).any() and (ka[8:] < 0).any() and (kb[13:] >= 0).any() and (kb[13:] < 0).any()
    inside = kb >= 0
    i, j, k = kb[inside] >> 42, (kb[inside] >> 21) & top, kb[inside] & top
    assert np.array_equal(np.stack([i, j, k], 1), np.floor(b[inside].astype(np.float64)).astype(np.int64))


def test_two_runs_give_equal_bytes():
    v, f, o = ref.sphere_mesh()
    a = ref.cluster(v, f, np.float32(3 * VOXEL), o)
    b = ref.cluster(v.copy(), f.copy(), np.float32(3 * VOXEL), o.copy())
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    assert a[0].tobytes() == ref.sphere_cluster(3.0)[0].tobytes()


# ----------------------------------------------------------------------------------------------
# the wrapper's host logic on torch's CPU device
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["sphere", "drill", "mirror_double", "zero_area", "one_cell", "fan_65"])
def test_face_rules_equal_the_restatement(which):
    import torch
    from cppf2_amd import simplify
    S = (ref.sphere_cluster(1.5) if which == "sphere" else ref.drill_cluster(0.008) if which == "drill" else ref.crafted_cluster(which))[3]
    cf = S["cf"]
    if which == "drill":                               # with duplicates and mirror images of the first hundred faces
        cf = np.concatenate([cf, cf[:100], cf[:50, [0, 2, 1]], cf[:20]])
    kept, counts = simplify.reduce_faces(torch.from_numpy(cf))
    rk, rc = ref.reduce_faces(cf)
    assert kept.dtype == torch.int64 and np.array_equal(kept.numpy(), rk) and counts == rc
    if which == "drill":
        assert rc["cancelled"] > 0 and rc["multi"] > 0
    faces = torch.from_numpy(cf[rk])
    assert simplify.edge_counts(faces, int(cf.max()) + 1) == ref.edge_counts(cf[rk])
    assert simplify.edge_counts(torch.zeros((0, 3), dtype=torch.int64), 0) == (0, 0)


def test_wrappers_refuse_bad_arguments_and_have_no_cpu_fallback():
    import torch
    from cppf2_amd import render, simplify
    for cell, lam in ((0.0, 1e-3), (-1.0, 1e-3), (float("nan"), 1e-3), (float("inf"), 1e-3), (0.01, 0.0), (0.01, float("nan"))):
        with pytest.raises(ValueError):
            simplify._checked(cell, lam, None)
    with pytest.raises(ValueError):
        simplify._checked(0.01, 1e-3, [0.0, float("nan"), 0.0])
    if not torch.cuda.is_available():
        v, f = ref.crafted()["one_triangle"]
        with pytest.raises(simplify.CppfError):
            simplify.cluster(render.Mesh(v, f), 0.01)


# ----------------------------------------------------------------------------------------------
# validation: fake device addresses, never dereferenced (every refusal comes before any device work)
# ----------------------------------------------------------------------------------------------
_A, _B, _C, _D, _E, _G, _H = (0x100000 * (i + 1) for i in range(7))
_O = (C.c_double * 3)(0.0, 0.0, 0.0)
_NAN, _INF = float("nan"), float("inf")


def _keys(lib, verts=_A, n=0, origin=_O, cell=0.01, keys=_B):
    return lib.cppf_cluster_keys(verts, n, origin, cell, keys, None)


def _quadrics(lib, verts=_A, n=9, faces=_B, nf=3, corners=_C, m=9, seg_off=_D, keys=_E, nc=0, origin=_O, cell=0.01, lam=1e-3, pos=_G):
    return lib.cppf_cluster_quadrics(verts, n, faces, nf, corners, m, seg_off, keys, nc, origin, cell, lam, pos, None)


def test_cluster_keys_validation_return_codes():
    from cppf2_amd import _lib
    lib = _lib.load()
    assert _keys(lib) == 0                                   # no vertices: a valid call that launches nothing
    assert _keys(lib, verts=None, keys=None) == 0
    for kw in (dict(n=-1), dict(origin=None), dict(origin=(C.c_double * 3)(0.0, _NAN, 0.0)), dict(origin=(C.c_double * 3)(_INF, 0.0, 0.0)),
               dict(cell=0.0), dict(cell=-0.01), dict(cell=_NAN), dict(cell=_INF), dict(n=5, verts=None), dict(n=5, keys=None)):
        assert _keys(lib, **kw) == -1, kw
        assert b"invalid argument" in lib.cppf_last_error_string()


def test_cluster_quadrics_validation_return_codes():
    from cppf2_amd import _lib
    lib = _lib.load()
    assert _quadrics(lib) == 0                               # no clusters: a valid call that launches nothing
    assert _quadrics(lib, n=0, nf=0, m=0, verts=None, faces=None, corners=None, seg_off=None, keys=None, pos=None) == 0
    assert _quadrics(lib, m=0) == 0
    for kw in (dict(n=-1), dict(nf=-1, m=0), dict(nc=-1), dict(m=-1), dict(m=10), dict(nf=715827883, m=0), dict(origin=None),
               dict(origin=(C.c_double * 3)(0.0, 0.0, _NAN)), dict(cell=0.0), dict(cell=_NAN), dict(cell=_INF), dict(cell=-1.0),
               dict(lam=0.0), dict(lam=-1e-3), dict(lam=_NAN), dict(lam=_INF),
               dict(nc=2, seg_off=None), dict(nc=2, keys=None), dict(nc=2, pos=None), dict(nc=2, verts=None), dict(nc=2, faces=None),
               dict(nc=2, corners=None)):
        assert _quadrics(lib, **kw) == -1, kw
        assert b"invalid argument" in lib.cppf_last_error_string()


# ----------------------------------------------------------------------------------------------
# the command lines
# ----------------------------------------------------------------------------------------------
def test_ply_round_trip_keeps_the_float32_bits(tmp_path):
    from cppf2_amd import render, simplify
    v, f, _, _ = ref.drill_cluster(0.008)
    for scale in (0.001, 1.0, 0.0254):
        mesh = render.Mesh(v, f, scale)
        path = str(tmp_path / ("m%g.ply" % scale))
        simplify.write_mesh(path, mesh)
        back = render.load_mesh(path, scale)
        assert back.verts.astype(np.float32).tobytes() == v.tobytes() and np.array_equal(back.faces, f) and back.scale == scale


def test_cli_errors_are_loud(tmp_path, capsys):
    from cppf2_amd import fuse, simplify
    out, models = str(tmp_path / "o.ply"), tmp_path / "models"
    models.mkdir()
    for argv in (["--mesh", ref.DRILL, "--out", out],                                       # no --cell
                 ["--mesh", ref.DRILL, "--cell", "0", "--out", out],
                 ["--mesh", ref.DRILL, "--cell", "nan", "--out", out],
                 ["--mesh", ref.DRILL, "--cell", "0.004", "--lam", "0", "--out", out],
                 ["--mesh", ref.DRILL, "--cell", "0.004", "--mesh-scale", "-1", "--out", out],
                 ["--mesh", ref.DRILL, "--cell", "0.004"],                                  # no --out
                 ["--mesh", ref.DRILL, "--cell", "0.004", "--out", str(tmp_path / "o.obj")],
                 ["--mesh", ref.DRILL, "--cell", "0.004", "--out-dir", str(tmp_path)],
                 ["--mesh", str(tmp_path / "nowhere.ply"), "--cell", "0.004", "--out", out],
                 ["--mesh", ref.DRILL, "--bop-models", str(models), "--cell", "0.004", "--out", out],
                 ["--cell", "0.004", "--out", out],
                 ["--bop-models", str(models), "--cell", "0.004", "--out-dir", str(tmp_path / "eval")],       # no obj_*.ply there
                 ["--bop-models", str(tmp_path / "nowhere"), "--cell", "0.004", "--out-dir", str(tmp_path / "eval")],
                 ["--bop-models", str(models), "--cell", "0.004", "--out", out]):
        with pytest.raises(SystemExit) as e:
            simplify.main(argv)
        assert e.value.code == 2, argv
    (models / "obj_000001.ply").write_bytes(open(ref.DRILL, "rb").read())
    with pytest.raises(SystemExit) as e:
        simplify.main(["--bop-models", str(models), "--cell", "0.004", "--out-dir", str(models)])
    assert e.value.code == 2
    for cell in ("0", "-0.006", "inf"):
        with pytest.raises(SystemExit) as e:
            fuse.main(["--views", str(tmp_path), "--voxel", "0.002", "--simplify-cell", cell, "--out", out])
        assert e.value.code == 2
    capsys.readouterr()
    assert not os.path.exists(out) and not os.path.exists(tmp_path / "eval")
