"""CPU checks of the symmetry detection (cppf2_amd/symmetry.py): the NumPy restatement of
cppf_sym_deviation against an independent float64 distance, detect's host logic on small solids with the restatement injected as
the deviation function, the entry point's argument validation, the flag rules of eval.py and the --sym-axis auto decision."""
import inspect
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import symmetry_ref as ref  # noqa: E402

REL_TOL, crafted_set = ref.REL_TOL, ref.crafted_set
COUNT = 128                      # surface samples of the CPU runs of detect (the restatement is NumPy)


def _scaled_errors(q, t, d2):
    """|sqrt(d2) - the float64 distance| / the largest coordinate magnitude, for d2 float32 [N,F] of queries x triangles."""
    out = np.zeros(d2.shape)
    for i in range(len(q)):
        for j in range(len(t)):
            want = np.sqrt(ref.point_triangle_d2_f64(q[i].astype(np.float64), t[j].astype(np.float64)))
            out[i, j] = abs(np.sqrt(np.float64(d2[i, j])) - want) / max(np.abs(q[i]).max(), np.abs(t[j]).max())
    return out


def test_crafted_queries_fall_in_their_regions():
    """The crafted queries are what they are named for: the float64 reference gives the hand-computed distances, and the
    restatement gives exactly 0 on a vertex of the unposed triangle."""
    q, t, want = crafted_set(pose=False)
    for i in range(len(q)):
        got = min(ref.point_triangle_d2_f64(q[i], t[j]) for j in range(2))
        assert abs(got - want[i]) < 1e-6, (i, got, want[i])
    d2 = ref.point_triangle_d2(q, t)
    assert d2[7, 0] == 0.0 and d2[10, 0] == d2[10, 1] == np.float32(0.25)


def test_restatement_follows_the_float64_distance():
    """The float32 restatement against the independent float64 distance on 64 random points x 96 random triangles (coordinates
    in [-1, 1]; every eighth triangle a sliver, one edge 1e-3 of the others) and on the crafted queries, plain and posed.
    Measured here: the largest |d32 - d64| / largest coordinate is 2.03e-7 (random set), 7.2e-8 and 4.4e-8 (crafted sets, plain
    and posed); allowed: 4 x the largest, for the platforms' differences in rounding."""
    rng = np.random.default_rng(5)
    q = rng.uniform(-1, 1, (64, 3)).astype(np.float32)
    t = rng.uniform(-1, 1, (96, 3, 3))
    t[::8, 2] = t[::8, 1] + 1e-3 * (t[::8, 2] - t[::8, 1])
    t = t.reshape(-1, 9).astype(np.float32)
    worst = _scaled_errors(q, t, ref.point_triangle_d2(q, t)).max()
    print("random: %.3g" % worst)
    assert worst <= REL_TOL
    for pose in (False, True):
        cq, ct, want = crafted_set(pose)
        d2 = ref.point_triangle_d2(cq, ct)
        w = _scaled_errors(cq, ct, d2).max()
        print("crafted (pose %s): %.3g" % (pose, w))
        assert w <= REL_TOL
        near = np.sqrt(ref.nearest_d2(cq, ct).astype(np.float64))
        assert np.abs(near - np.sqrt(want)).max() <= REL_TOL * max(np.abs(cq).max(), np.abs(ct).max())


def test_deviation_is_the_maximum_over_queries_and_ignores_nan():
    q, t, want = crafted_set()
    eye = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12)
    d2 = ref.deviation_d2(q, t, np.stack([eye, eye]))
    assert d2.dtype == np.float32 and d2[0] == d2[1] == ref.nearest_d2(q, t).max()
    bad = eye.copy()
    bad[3] = np.nan
    assert list(np.isinf(ref.deviation_d2(q, t, np.stack([eye, bad, eye])))) == [False, True, False]
    qn = q.copy()
    qn[3, 1] = np.inf
    assert np.isinf(ref.deviation_d2(qn, t, eye[None])).all()
    # a triangle without area gives NaN distances, which a real triangle beside it outbids
    flat = np.concatenate([t, np.tile(t[:1, :3], (1, 3))])
    assert (ref.deviation_d2(q, flat, eye[None]) == ref.deviation_d2(q, t, eye[None])).all()


@pytest.fixture(scope="module")
def detected():
    """name -> (render.Mesh in metres, the entry detect() returns with the restatement as the deviation function)."""
    from cppf2_amd import render, symmetry
    out = {}
    for name, (v, f) in ref.solid_meshes().items():
        assert len(f) <= 256
        mesh = render.Mesh(v * ref.MESH_SCALE, f, ref.MESH_SCALE)
        out[name] = (mesh, symmetry.detect(mesh, count=COUNT, _deviations=ref.deviations))
    return out


@pytest.mark.parametrize("name", ["box", "square_prism", "hex_prism", "cylinder", "cone", "handled_cylinder", "cube"])
def test_detect_finds_the_solids_symmetries(detected, name):
    """box: 3 half-turns; square prism: 7 transforms; hexagonal prism: 11; 64-facet cylinder: one continuous axis and one
    half-turn; cone: one continuous axis alone; handled cylinder: one half-turn; cube: isotropic.  Each about the right axis."""
    mesh, info = detected[name]
    ref.check_entry(name, info)
    counts = dict(box=(3, 0), square_prism=(7, 0), hex_prism=(11, 0), cylinder=(1, 1), cone=(0, 1), handled_cylinder=(1, 0))
    if name in counts:
        assert (len(info.get("symmetries_discrete", [])), len(info.get("symmetries_continuous", []))) == counts[name]
    rep = info["report"]
    assert rep["tol"] == 0.01 and rep["count"] == COUNT and rep["candidates"] >= 618
    assert all(a <= rep["tol"] for a in rep["accepted"] + rep["continuous"])
    assert rep["smallest_rejected"] is None or rep["smallest_rejected"] > rep["tol"]


@pytest.mark.parametrize("name", ["box", "hex_prism", "cylinder", "cone", "handled_cylinder"])
def test_reported_transforms_map_the_surface_onto_itself(detected, name):
    """Every reported transform, expanded by bop.symmetry_transforms in the centred metre frame ObjectInfo uses, takes fresh
    surface samples onto the surface within tol x diameter; the units are pinned (millimetre file, mesh_scale 0.001)."""
    from cppf2_amd import bop, symmetry
    mesh, info = detected[name]
    centre = mesh.bounds.mean(0)
    diam_m = info["diameter"] * ref.MESH_SCALE
    assert abs(diam_m - bop.diameter(mesh.verts)) < 1e-12
    assert abs(info["size_x"] * ref.MESH_SCALE - (mesh.bounds[1, 0] - mesh.bounds[0, 0])) < 1e-12
    syms = bop.symmetry_transforms(info, ref.MESH_SCALE, centre)
    n_disc, n_cont = len(info.get("symmetries_discrete", [])), len(info.get("symmetries_continuous", []))
    assert len(syms) == ((1 + n_disc) * n_cont * bop.N_CONT if n_cont else 1 + n_disc)
    _, _, _, tri, area = symmetry.surface_frame(mesh.verts, mesh.faces)
    q = symmetry.sample_surface(tri, area, 48, 7) - centre
    dev = ref.deviations(q, (tri - centre).reshape(-1, 9), syms.reshape(-1, 12))
    assert dev.max() <= 0.01 * diam_m, dev.max() / diam_m
    obj = bop.ObjectInfo.from_mesh(mesh, models_info=info)
    assert obj.syms.shape == syms.shape and abs(obj.diameter - diam_m) < 1e-12


def test_detect_is_deterministic_and_samples_like_the_icp_model(detected):
    from cppf2_amd import icp, symmetry
    mesh, info = detected["box"]
    assert symmetry.detect(mesh, count=COUNT, _deviations=ref.deviations) == info
    _, _, _, tri, area = symmetry.surface_frame(mesh.verts, mesh.faces)
    pts = symmetry.sample_surface(tri, area, 64, 3)
    model = icp.ModelPoints.from_mesh(mesh, 64, 3)
    assert np.abs(pts - (model.pts.astype(np.float64) + model.centre)).max() < 1e-7


def test_surface_frame_matches_a_dense_sampling():
    """The closed-form centroid and second moments against 200 000 area-weighted samples of the handled cylinder."""
    from cppf2_amd import symmetry
    v, f = ref.solid_meshes()["handled_cylinder"]
    c, w, E, tri, area = symmetry.surface_frame(v, f)
    p = symmetry.sample_surface(tri, area, 200000, 1)
    assert np.abs(p.mean(0) - c).max() < 0.3                                   # millimetres; the sampling error is ~0.1
    S = (p - c).T @ (p - c) / len(p)
    assert np.abs(np.linalg.eigvalsh(S) - w).max() < 0.01 * w[2]
    assert np.allclose(E.T @ E, np.eye(3), atol=1e-12)


def test_models_info_file_round_trips(detected, tmp_path):
    from cppf2_amd import symmetry
    entries = {15: detected["hex_prism"][1], 2: detected["cone"][1]}
    path = tmp_path / "models_info.json"
    symmetry.write_models_info(str(path), entries)
    back = json.load(open(path))
    assert list(back) == ["2", "15"]
    assert back["15"] == entries[15] and back["2"] == entries[2]              # floats survive json exactly


def _untraced_lib():
    from cppf2_amd import _lib
    lib = _lib.load()
    return lib._lib if isinstance(lib, _lib._Traced) else lib


_Q, _T, _M, _OUT = (0x100000 * (i + 1) for i in range(4))       # fake device addresses, never dereferenced
_SYM_CASES = [
    (dict(nc=0), 0, None),
    (dict(nc=0, queries=None, tris=None, maps=None, out=None), 0, None),
    (dict(queries=None), -1, b"cppf_sym_deviation: invalid argument: queries && tris && maps && max_d2"),
    (dict(tris=None), -1, b"cppf_sym_deviation: invalid argument: queries && tris && maps && max_d2"),
    (dict(maps=None), -1, b"cppf_sym_deviation: invalid argument: queries && tris && maps && max_d2"),
    (dict(out=None), -1, b"cppf_sym_deviation: invalid argument: queries && tris && maps && max_d2"),
    (dict(nq=0), -1, b"cppf_sym_deviation: invalid argument: nq >= 1"),
    (dict(nq=0, nc=0), -1, b"cppf_sym_deviation: invalid argument: nq >= 1"),
    (dict(nf=0), -1, b"cppf_sym_deviation: invalid argument: nf >= 1"),
    (dict(nc=-1), -1, b"cppf_sym_deviation: invalid argument: nc >= 0 && nc <= SYM_MAX_MAPS"),
    (dict(nc=65536), -1, b"cppf_sym_deviation: invalid argument: nc >= 0 && nc <= SYM_MAX_MAPS"),
]


@pytest.mark.parametrize("kw,status,message", _SYM_CASES, ids=[str(i) for i in range(len(_SYM_CASES))])
def test_entry_point_validation(kw, status, message):
    """cppf_sym_deviation refuses null pointers and bad sizes with its message before any device work, and no maps is a valid
    call that launches nothing (this machine has no device: a launch would fail with another status)."""
    lib = _untraced_lib()
    a = dict(queries=_Q, nq=10, tris=_T, nf=5, maps=_M, nc=3, out=_OUT)
    a.update(kw)
    got = lib.cppf_sym_deviation(a["queries"], a["nq"], a["tris"], a["nf"], a["maps"], a["nc"], a["out"], None)
    assert got == status, (kw, got, lib.cppf_last_error_string())
    if message is not None:
        assert lib.cppf_last_error_string() == message


def test_eval_flag_rules(monkeypatch):
    monkeypatch.chdir(ROOT)
    import eval as ev
    from cppf2_amd import symmetry
    base = {k: p.default for k, p in inspect.signature(ev.main).parameters.items()}
    assert base["detect_symmetries"] is False and base["sym_tol"] is None
    assert ev._checked_flags(**base).sym_tol is None
    ok = dict(base, data="depth", mesh="obj.ply", gt_pose="pose.txt")
    assert ev._checked_flags(**ok).sym_tol is None
    assert ev._checked_flags(**dict(ok, detect_symmetries=True)).sym_tol == symmetry.TOL
    assert ev._checked_flags(**dict(ok, detect_symmetries=True, sym_tol="0.02")).sym_tol == 0.02
    for kw, word in ((dict(ok, sym_tol=0.02), "--sym_tol sets the tolerance of --detect_symmetries"),
                     (dict(ok, detect_symmetries=True, models_info="m.json"), "--models_info would supply"),
                     (dict(base, data="depth", detect_symmetries=True), "it needs --data=depth and --mesh"),
                     (dict(base, detect_symmetries=True), "it needs --data=depth and --mesh"),
                     (dict(ok, detect_symmetries=True, sym_tol=0), "--sym_tol is a share of the diameter > 0"),
                     (dict(ok, detect_symmetries=True, sym_tol="nan"), "--sym_tol is a share of the diameter > 0")):
        with pytest.raises(ValueError) as e:
            ev._checked_flags(**kw)
        assert word in str(e.value), (kw, str(e.value))


def _entry(axis, offset, lo=(-30.0, -30.0, -50.0), size=(60.0, 60.0, 100.0), diameter=116.6):
    e = dict(diameter=diameter, symmetries_continuous=[dict(axis=list(axis), offset=list(offset))])
    e.update({"min_" + a: lo[i] for i, a in enumerate("xyz")})
    e.update({"size_" + a: size[i] for i, a in enumerate("xyz")})
    return e


def test_sym_axis_auto_is_a_function_of_the_entry():
    from cppf2_amd import symmetry
    assert symmetry.coordinate_axis(_entry((0, 0, 1), (0, 0, 0))) == 2
    assert symmetry.coordinate_axis(_entry((0, -1, 0), (0, 7.0, 0))) == 1                    # sign and a shift along the axis
    tilt = np.radians(0.9)
    assert symmetry.coordinate_axis(_entry((np.sin(tilt), 0, np.cos(tilt)), (0, 0, 0))) == 2
    assert symmetry.coordinate_axis(_entry((0, 0, 1), (1.0, 0, 0))) == 2                     # 1 mm off: within 0.01 x 116.6
    for e, word in ((_entry((np.sin(2 * tilt), 0, np.cos(2 * tilt)), (0, 0, 0)), "1.80 deg from coordinate axis 2"),
                    (_entry((0, 0, 1), (2.0, 0, 0)), "0.0172 x diameter from the bounding-box centre"),
                    (_entry((0.6, 0, 0.8), (0, 0, 0)), "axis (0.6000, 0.0000, 0.8000)"),
                    (dict(diameter=1.0, symmetries_discrete=[[0.0] * 16]), "no continuous symmetry axis was detected (1 discrete")):
        with pytest.raises(ValueError) as err:
            symmetry.coordinate_axis(e)
        assert word in str(err.value), str(err.value)
    assert symmetry.coordinate_axis(_entry((0, 0, 1), (2.0, 0, 0)), tol=0.02) == 2


def test_sym_axis_auto_on_the_posed_and_the_upright_cylinder(detected):
    """The obliquely posed cylinder's axis is no coordinate axis: the message names it; the same cylinder upright is axis 2."""
    from cppf2_amd import render, symmetry
    with pytest.raises(ValueError) as err:
        symmetry.coordinate_axis(detected["cylinder"][1])
    assert "deg from coordinate axis" in str(err.value)
    v, f = ref.solid_meshes()["cylinder"]
    up = (v - ref.POSE_T) @ ref.POSE_R                                                       # back to its own frame
    info = symmetry.detect(render.Mesh(up * ref.MESH_SCALE, f, ref.MESH_SCALE), count=32, _deviations=ref.deviations)
    assert symmetry.coordinate_axis(info) == 2


def test_pair_table_cli_passes_the_axis_on(monkeypatch, capsys):
    """--sym-axis: an integer keeps its meaning, auto asks symmetry.detect and prints its choice or exits with the message that
    names the detected axis, anything else is a usage error.  build, load_mesh and detect are stand-ins: no table is built."""
    from cppf2_amd import pair_table, render, symmetry
    seen = []

    class Table:
        E, ncell, build_seconds, cell_off = 0, 1, 0.0, np.zeros(2, dtype=np.int32)

        def save(self, path):
            pass

    def fake_build(mesh, views, tuples, seed, sym_axis=None, name=""):
        seen.append(sym_axis)
        return Table()
    monkeypatch.setattr(pair_table, "build", fake_build)
    monkeypatch.setattr(render, "load_mesh", lambda path, scale: (path, scale))
    entry = {}
    monkeypatch.setattr(symmetry, "detect", lambda mesh: entry["info"])
    argv = ["--mesh", "can.ply", "--out", "can.npz"]
    pair_table.main(argv)
    pair_table.main(argv + ["--sym-axis", "1"])
    entry["info"] = _entry((0, 0, 1), (0, 0, 0))
    pair_table.main(argv + ["--sym-axis", "auto"])
    assert seen == [None, 1, 2] and type(seen[1]) is int
    assert "can.ply: --sym-axis auto chose coordinate axis 2" in capsys.readouterr().out
    entry["info"] = _entry((0.6, 0, 0.8), (0, 0, 0))
    with pytest.raises(SystemExit) as e:
        pair_table.main(argv + ["--sym-axis", "auto"])
    assert "can.ply: --sym-axis auto" in str(e.value) and "axis (0.6000, 0.0000, 0.8000)" in str(e.value)
    with pytest.raises(SystemExit):
        pair_table.main(argv + ["--sym-axis", "up"])
    assert seen == [None, 1, 2]
