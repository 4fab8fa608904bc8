"""GPU checks of mesh simplification: cppf_cluster_keys and cppf_cluster_quadrics bit-equal to the NumPy
restatement (tests/simplify_ref.py) at every size that takes another path, simplify.cluster and simplify.deviation end to end,
fusion with a simplification stage on a rendered scene of the fixture mesh, and the consumers on simplified meshes."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuse_ref  # noqa: E402
import simplify_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

VOXEL = fuse_ref.VOXEL
COUNTS = ("vertices_in", "vertices_out", "triangles_in", "triangles_out", "collapsed", "cancelled", "multi", "boundary_edges",
          "nonmanifold_edges")


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def assert_pos_bits(got, want, what):
    """The device's representatives carry the restatement's float32 bits; the number of coordinates that differ is printed."""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print("%s: %d of %d coordinates differ" % (what, differ, want.size))
    assert differ == 0, what


def dev_quadrics(v, f, S, cell, lam=ref.LAMBDA, clusters=None):
    from cppf2_amd import simplify
    C_ = len(S["keys"]) if clusters is None else clusters
    return simplify.cluster_quadrics(v, f, S["corners"], S["seg_off"][:C_ + 1], S["keys"][:C_], S["origin"], cell, lam).cpu().numpy()


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_keys_equal_the_restatement_bit_for_bit(which, n):
    from cppf2_amd import simplify
    v, o, c = ref.key_cases()[which]
    got = simplify.cluster_keys(v[:n], o, c).cpu().numpy()
    assert same_bits(got, ref.cluster_keys(v[:n], o, c))
    if n == 257:
        assert (got >= 0).any() and (got == -1).any()


def test_no_vertices_no_clusters():
    from cppf2_amd import simplify
    assert simplify.cluster_keys(np.zeros((0, 3), np.float32), np.zeros(3), 0.01).shape == (0,)
    z = np.zeros((0,), np.int64)
    assert simplify.cluster_quadrics(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), z, np.zeros((1,), np.int64), z,
                                     np.zeros(3), 0.01).shape == (0, 3)


@pytest.mark.parametrize("cell", ref.SPHERE_CELLS)
def test_sphere_representatives_have_the_restatement_bits(cell):
    v, f, _ = ref.sphere_mesh()
    S = ref.sphere_cluster(cell)[3]
    assert_pos_bits(dev_quadrics(v, f, S, np.float32(cell * VOXEL)), S["pos"], "sphere, cell %.1f voxel" % cell)


@pytest.mark.parametrize("cell", ref.DRILL_CELLS)
def test_drill_representatives_have_the_restatement_bits(cell):
    v, f, _ = ref.drill_mesh()
    S = ref.drill_cluster(cell)[3]
    assert_pos_bits(dev_quadrics(v, f, S, np.float32(cell)), S["pos"], "drill, cell %g mm" % (1e3 * cell))


@pytest.mark.parametrize("name", sorted(ref.crafted()))
def test_crafted_representatives_have_the_restatement_bits(name):
    v, f = ref.crafted()[name]
    S = ref.crafted_cluster(name)[3]
    assert_pos_bits(dev_quadrics(v, f, S, ref.CELL), S["pos"], name)


def test_crafted_cases_reach_the_segment_lengths():
    longest = {name: int(np.diff(ref.crafted_cluster(name)[3]["seg_off"]).max()) for name in ("one_triangle", "fan_64", "fan_65", "fan_1000")}
    assert longest == dict(one_triangle=1, fan_64=64, fan_65=65, fan_1000=1000)
    S = ref.crafted_cluster("zero_area")[3]
    assert (S["w"] == 0).all()


@pytest.mark.parametrize("clusters", [1, 63, 64, 65, 257])
def test_cluster_counts_around_one_wave_and_one_block(clusters):
    """The first C of the sphere's 314 clusters at 3 voxels; the corner list stays whole, so the later segments are simply not read."""
    v, f, _ = ref.sphere_mesh()
    S = ref.sphere_cluster(3.0)[3]
    assert len(S["keys"]) >= 257
    got = dev_quadrics(v, f, S, np.float32(3 * VOXEL), clusters=clusters)
    assert_pos_bits(got, S["pos"][:clusters], "%d clusters" % clusters)


def test_the_mean_regulariser_and_a_negative_key():
    from cppf2_amd import simplify
    v, f, _ = ref.sphere_mesh()
    S = ref.sphere_cluster(3.0, 1e6)[3]
    assert_pos_bits(dev_quadrics(v, f, S, np.float32(3 * VOXEL), lam=1e6), S["pos"], "sphere, lam 1e6")
    keys = S["keys"].copy()
    keys[5] = -1
    got = simplify.cluster_quadrics(v, f, S["corners"], S["seg_off"], keys, S["origin"], np.float32(3 * VOXEL), 1e6).cpu().numpy()
    assert np.isnan(got[5]).all() and same_bits(np.delete(got, 5, 0), np.delete(S["pos"], 5, 0))


# ----------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------
def _cluster_equals(v, f, origin, cell, want):
    from cppf2_amd import render, simplify
    mesh = render.Mesh(v, f)
    small, report = simplify.cluster(mesh, cell, origin=origin)
    again, report2 = simplify.cluster(mesh, cell, origin=origin)
    wv, wf, wrep = want[:3]
    assert same_bits(small.verts.astype(np.float32), wv) and np.array_equal(small.verts, wv.astype(np.float64))
    assert np.array_equal(small.faces, wf) and small.faces.dtype == np.int32
    assert {k: report[k] for k in COUNTS} == {k: wrep[k] for k in COUNTS}
    assert small.boundary_edges == wrep["boundary_edges"] and set(report["seconds"]) == {"keys", "sort", "quadrics", "faces"}
    assert again.verts.tobytes() == small.verts.tobytes() and again.faces.tobytes() == small.faces.tobytes()      # deterministic
    assert {k: report2[k] for k in COUNTS} == {k: report[k] for k in COUNTS}
    return small, report


def test_cluster_on_the_device_equals_the_restatement_sphere():
    v, f, o = ref.sphere_mesh()
    _, report = _cluster_equals(v, f, o, np.float32(3 * VOXEL), ref.sphere_cluster(3.0))
    assert report["triangles_out"] == 624 and report["boundary_edges"] == 0


def test_cluster_on_the_device_equals_the_restatement_drill():
    from cppf2_amd import render, simplify
    v, f, o = ref.drill_mesh()
    _, report = _cluster_equals(v, f, o, np.float32(0.004), ref.drill_cluster(0.004))
    assert report["triangles_out"] == 7826 and report["boundary_edges"] == 0
    # the default origin is the float32 minimum of the used vertices; a used vertex outside the lattice is refused with its count
    small, _ = simplify.cluster(render.Mesh(v, f), 0.004)
    wv, wf, _ = ref.cluster(v, f, np.float32(0.004))
    assert same_bits(small.verts.astype(np.float32), wv) and np.array_equal(small.faces, wf)
    far = v.copy()
    assert f[0, 0] != f[7, 1]
    far[f[0, 0]] = np.nan
    far[f[7, 1]] = 1e5
    with pytest.raises(ValueError, match="2 vertices"):
        simplify.cluster(render.Mesh(far, f), 0.004, origin=o)


def test_deviation_on_the_device_equals_the_restatement():
    from cppf2_amd import render, simplify
    v, f, _ = ref.drill_mesh()
    sv, sf, _, _ = ref.drill_cluster(0.004)
    got = simplify.deviation(render.Mesh(v, f), render.Mesh(sv, sf))
    want = ref.drill_deviation(0.004)
    print("drill, cell 4 mm: deviation %.4f / %.4f cell" % (got[0] / 0.004, got[1] / 0.004))
    assert got == want


def test_command_line_writes_the_restatement_mesh_and_a_models_eval(tmp_path):
    import json
    import shutil
    from cppf2_amd import render, simplify
    v, f, _ = ref.drill_mesh()
    wv, wf, wrep = ref.cluster(v, f, np.float32(0.004))               # the command line takes the default origin
    out, rep = str(tmp_path / "small.ply"), str(tmp_path / "report.json")
    report = simplify.main(["--mesh", ref.DRILL, "--mesh-scale", "0.001", "--cell", "0.004", "--out", out, "--report", rep])
    back = render.load_mesh(out, 0.001)
    assert same_bits(back.verts.astype(np.float32), wv) and np.array_equal(back.faces, wf)
    assert {k: report[k] for k in COUNTS} == wrep and {k: json.load(open(rep))[k] for k in COUNTS} == wrep
    models, evals = tmp_path / "models", tmp_path / "models_eval"
    models.mkdir()
    for name in ("obj_000015.ply", "obj_000002.ply", "notes.txt"):
        shutil.copy(ref.DRILL, str(models / name))
    reports = simplify.main(["--bop-models", str(models), "--cell", "0.004", "--out-dir", str(evals)])
    assert sorted(os.listdir(str(evals))) == sorted(reports) == ["obj_000002.ply", "obj_000015.ply"]
    for name in reports:
        assert open(str(evals / name), "rb").read() == open(out, "rb").read()


def test_fusion_with_a_simplification_stage(tmp_path):
    """The set-up of tests/test_fuse_gpu.py's command-line test: 32 rendered views of the fixture mesh, 160 x 120, voxel 3 mm.
    A fused vertex lies within trunc + sqrt(3) voxel + 0.1 mm of the original surface (that test's bound), and clustering moves
    no point of the surface by more than the cell's diagonal."""
    import json
    from cppf2_amd import bop_data, fuse, render, symmetry
    mesh = render.load_mesh(ref.DRILL, 0.001)
    K = render.INTRINSICS.copy()
    K[:2] *= 0.25
    dist = 2.2 * float(np.linalg.norm(mesh.bounds[1] - mesh.bounds[0]))
    P = fuse_ref.look_at(fuse_ref.fibonacci(32), centre=np.zeros(3), dist=max(dist, 0.3)).astype(np.float64).reshape(-1, 3, 4)
    root = bop_data.write_dataset(str(tmp_path / "ds"), "train", {15: mesh}, [[[(15, p[:, :3], p[:, 3])] for p in P]], K=K, height=120,
                                  width=160, targets_file=None)
    views = os.path.join(root, "train", "000000")
    voxel = 0.003
    cell = 3 * voxel
    plain, small, rep = str(tmp_path / "plain.ply"), str(tmp_path / "small.ply"), str(tmp_path / "report.json")
    common = ["--views", views, "--obj-id", "15", "--pixel-offset", "0.5", "--voxel", str(voxel)]
    before = fuse.main(common + ["--out", plain])
    report = fuse.main(common + ["--simplify-cell", str(cell), "--report", rep, "--out", small])
    assert "simplify" not in before and json.load(open(rep))["simplify"]["triangles_out"] == report["triangles"]
    # without the flag: the bytes of the stages called one by one, as the command line did before it knew the flag
    batches = fuse.read_views(views, 15)
    assert len(batches) == 1
    b = batches[0]
    vol = fuse.Volume.around(b["depths"], b["masks"], b["poses"], b["K"], voxel, pixel_offset=0.5)
    fuse.integrate(vol, b["depths"], b["poses"], b["K"], b["masks"], 0.5)
    raw = fuse.extract(vol)
    bop_data.write_ply(str(tmp_path / "stages.ply"), raw.verts / 0.001, raw.faces)
    assert open(plain, "rb").read() == open(str(tmp_path / "stages.ply"), "rb").read()
    s = report["simplify"]
    assert s["triangles_in"] == before["triangles"] == raw.faces.shape[0] and s["vertices_in"] == before["vertices"]
    assert report["triangles"] == s["triangles_out"] < before["triangles"] and report["vertices"] == s["vertices_out"]
    assert np.array_equal(np.asarray(s["origin"]), vol.origin) and s["cell"] == float(np.float32(cell))       # on the voxel lattice
    fused = render.load_mesh(small, 0.001)
    assert fused.faces.shape[0] == report["triangles"] and fused.verts.shape[0] == report["vertices"]
    tri = mesh.verts[mesh.faces].reshape(-1, 9)
    worst = float(symmetry.deviations(fused.verts, tri, ref.IDENTITY)[0])
    bound = report["trunc"] + np.sqrt(3.0) * voxel + 1e-4 + np.sqrt(3.0) * cell
    print("fixture: %d triangles unsimplified (%d boundary edges), %d at cell 3 voxel (%d boundary, %d non-manifold edges, multi %d); "
          "farthest vertex %.2f voxel (bound %.2f)" % (before["triangles"], before["boundary_edges"], report["triangles"],
                                                       report["boundary_edges"], s["nonmanifold_edges"], s["multi"], worst / voxel,
                                                       bound / voxel))
    assert worst <= bound
    assert report["boundary_edges"] == 0


# ----------------------------------------------------------------------------------------------
# the consumers take the output as it is
# ----------------------------------------------------------------------------------------------
def test_symmetry_detection_on_the_simplified_drill_still_reports_nothing():
    from cppf2_amd import render, symmetry
    sv, sf, _, _ = ref.drill_cluster(0.004)
    info = symmetry.detect(render.Mesh(sv, sf, 0.001))
    print("simplified drill: smallest rejected %s x diameter" % info["report"]["smallest_rejected"])
    assert "symmetries_discrete" not in info and "symmetries_continuous" not in info and not info["report"]["isotropic"]


def test_winding_survives_culled_render_equals_the_unculled_one():
    import torch
    from cppf2_amd import ops, render, simplify
    v, f, o = ref.sphere_mesh()
    small, report = simplify.cluster(render.Mesh(v, f), np.float32(3 * VOXEL), origin=o)
    assert report["boundary_edges"] == 0
    verts, tris = small.device(ops._dev())
    K = np.array([[150.0, 0, 80], [0, 150.0, 60], [0, 0, 1]])
    poses = torch.from_numpy(fuse_ref.look_at(fuse_ref.fibonacci(7)[[1, 5]], dist=0.3)).to(verts.device)
    off = ops._offsets([tris.shape[0]], verts.device)
    for P in poses:
        a = render.render_depth(verts, tris, off, P[None], K, fuse_ref.H, fuse_ref.W, cull=True)
        b = render.render_depth(verts, tris, off, P[None], K, fuse_ref.H, fuse_ref.W, cull=False)
        assert int((a > 0).sum()) > 1000 and torch.equal(a, b)
        flipped = render.render_depth(verts, tris[:, [0, 2, 1]].contiguous(), off, P[None], K, fuse_ref.H, fuse_ref.W, cull=True)
        assert not torch.equal(a, flipped)
