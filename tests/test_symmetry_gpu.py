"""GPU checks of the symmetry detection: cppf_sym_deviation bit-equal to the NumPy restatement (tests/symmetry_ref.py) at its
edge sizes, detect on the fixture mesh and on the solids of tests/test_symmetry.py, what the detected set is worth to the
scorer, and eval.main(detect_symmetries=True)."""
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

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, "tests", "golden", "example_data", "obj_000015.ply")
TILE = 256                       # SYM_TILE of cppf_symmetry.hip
NQ, NF, NC = 257, 2 * TILE + 3, 65


def _max_d2(q, t, m):
    """cppf_sym_deviation itself on host arrays: float32 [C] (the squared deviations, as the kernel wrote them)."""
    import torch
    from cppf2_amd import _lib, ops
    dev = ops._dev()
    qd = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 3)).to(dev)
    td = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32).reshape(-1, 9)).to(dev)
    md = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float64).reshape(-1, 12)).to(dev)
    out = torch.full((md.shape[0],), -1.0, dtype=torch.float32, device=dev)         # the entry point clears it
    _lib.check(_lib.load().cppf_sym_deviation(ops._p(qd), qd.shape[0], ops._p(td), td.shape[0], ops._p(md), md.shape[0],
                                              ops._p(out), ops._stream()), "cppf_sym_deviation")
    return out.cpu().numpy()


def _same_bits(got, want):
    return got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.fixture(scope="module")
def cloud():
    """257 queries, 515 triangles (sides 0.05 .. 0.5 in a cube of side 2) and 65 rigid maps, and the restatement's nearest
    squared distance of every (map, query) to each prefix of the triangles the cases use: computed once, read by all."""
    rng = np.random.default_rng(11)
    q = rng.uniform(-1, 1, (NQ, 3)).astype(np.float32)
    a = rng.uniform(-1, 1, (NF, 1, 3))
    t = (a + rng.uniform(-1, 1, (NF, 3, 3)) * rng.uniform(0.05, 0.5, (NF, 1, 1))).reshape(NF, 9).astype(np.float32)
    maps = np.zeros((NC, 3, 4))
    for c in range(NC):
        maps[c, :, :3] = ref._rodrigues(rng.standard_normal(3), rng.uniform(0, np.pi))
        maps[c, :, 3] = rng.uniform(-0.2, 0.2, 3)
    maps[0] = np.hstack([np.eye(3), np.zeros((3, 1))])
    return dict(q=q, t=t, maps=maps.reshape(NC, 12))


@pytest.mark.parametrize("nq,nf,nc", [(NQ, 1, 2), (NQ, TILE - 1, 2), (NQ, TILE, 2), (NQ, TILE + 1, 2), (NQ, NF, 2),
                                      (1, TILE + 1, 2), (63, TILE + 1, 2), (256, TILE + 1, 2),
                                      (63, TILE + 1, 1), (63, TILE + 1, NC)])
def test_kernel_is_bit_equal_to_the_restatement(cloud, nq, nf, nc):
    """Nq in {1, 63, 256, 257} (one lane, a partial wavefront, a full block, a second block), F in {1, tile - 1, tile, tile + 1,
    2 tile + 3}, C in {1, 2, 65}: the same bits as the restatement."""
    q, t, m = cloud["q"][:nq], cloud["t"][:nf], cloud["maps"][:nc]
    got = _max_d2(q, t, m)
    assert _same_bits(got, ref.deviation_d2(q, t, m))
    assert np.isfinite(got).all() and (got > 0).all()


def test_a_candidate_scores_the_same_alone_and_in_a_batch(cloud):
    q, t, m = cloud["q"], cloud["t"][:TILE + 1], cloud["maps"]
    batch = _max_d2(q, t, m)
    for c in (0, 37, NC - 1):
        assert _same_bits(_max_d2(q, t, m[c:c + 1]), batch[c:c + 1])
    assert _same_bits(_max_d2(q, t, m), batch)                                       # and again: no dependence on the order


def test_crafted_queries_on_the_device():
    """One query in each of the seven regions, on a vertex, on an edge, in the face and equidistant from two triangles, plain and
    posed: one query per call gives each one's own squared distance, bit-equal, and within the float64 tolerance."""
    eye = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(1, 12)
    turn = np.hstack([ref._rodrigues([0.2, 1.0, -0.4], 0.9), [[0.1], [-0.2], [0.05]]]).reshape(1, 12)
    for pose in (False, True):
        q, t, want = crafted_set(pose)
        assert _same_bits(_max_d2(q, t, np.concatenate([eye, turn])), ref.deviation_d2(q, t, np.concatenate([eye, turn])))
        for i in range(len(q)):
            got = _max_d2(q[i:i + 1], t, eye)
            assert _same_bits(got, ref.deviation_d2(q[i:i + 1], t, eye))
            scale = max(np.abs(q).max(), np.abs(t).max())
            assert abs(np.sqrt(np.float64(got[0])) - np.sqrt(want[i])) <= REL_TOL * scale, (pose, i)
    q, t, _ = crafted_set(False)
    assert _max_d2(q[7:8], t, eye)[0] == 0.0                                         # on a vertex: exactly 0


def test_non_finite_inputs_give_infinity_where_they_are(cloud):
    q, t, m = cloud["q"][:63].copy(), cloud["t"][:TILE + 1], cloud["maps"][:5].copy()
    want = ref.deviation_d2(q, t, m)
    for bad in (np.nan, np.inf, -np.inf):
        mb = m.copy()
        mb[3, 7] = bad
        got = _max_d2(q, t, mb)
        assert np.isposinf(got[3]) and _same_bits(np.delete(got, 3), np.delete(want, 3)), bad
        assert _same_bits(got, ref.deviation_d2(q, t, mb))
    for bad, at in ((np.nan, (0, 0)), (np.inf, (40, 2)), (-np.inf, (62, 1))):
        qb = q.copy()
        qb[at] = bad
        got = _max_d2(qb, t, m)
        assert np.isposinf(got).all(), (bad, got)
        assert _same_bits(got, ref.deviation_d2(qb, t, m))
    # a triangle without area is ignored beside real ones
    flat = np.concatenate([np.tile(t[:1, :3], (1, 3)), t])
    assert _same_bits(_max_d2(q, flat, m), want)


def test_deviations_wrapper_takes_the_root_and_an_empty_batch(cloud):
    import torch
    from cppf2_amd import symmetry
    q, t, m = cloud["q"][:63], cloud["t"][:TILE - 1], cloud["maps"][:2]
    got = symmetry.deviations(q, t, m.reshape(2, 3, 4))
    assert got.dtype == torch.float32 and got.is_cuda
    assert _same_bits(got.cpu().numpy(), np.sqrt(ref.deviation_d2(q, t, m)))
    assert symmetry.deviations(q, t, np.zeros((0, 12))).shape == (0,)


def test_detect_finds_no_symmetry_of_the_fixture():
    """The fixture (a drill, 15 728 triangles): nothing is accepted, and the best refused candidate deviates by at least
    5 x TOL of the diameter (a nearest-sample proxy gave 10 x before the kernel existed)."""
    from cppf2_amd import render, symmetry
    info = symmetry.detect(render.load_mesh(FIXTURE, 0.001))
    rep = info["report"]
    print("fixture:", json.dumps(rep))
    assert "symmetries_discrete" not in info and "symmetries_continuous" not in info
    assert rep["isotropic"] is False and rep["candidates"] == 618 and rep["accepted"] == [] and rep["continuous"] == []
    assert rep["smallest_rejected"] >= 5 * symmetry.TOL
    assert symmetry.detect(render.load_mesh(FIXTURE, 0.001)) == info


@pytest.fixture(scope="module")
def solids():
    from cppf2_amd import render, symmetry
    out = {}
    for name, (v, f) in ref.solid_meshes().items():
        mesh = render.Mesh(v * ref.MESH_SCALE, f, ref.MESH_SCALE)
        out[name] = (mesh, symmetry.detect(mesh))
        print(name, json.dumps(out[name][1]["report"]))
    return out


@pytest.mark.parametrize("name", ["box", "square_prism", "hex_prism", "cylinder", "cone", "handled_cylinder", "cube"])
def test_detect_on_the_solids_equals_the_cpu_sets(solids, name):
    """The device's detect at its default 2 048 samples finds what tests/test_symmetry.py's restated run finds."""
    mesh, info = solids[name]
    ref.check_entry(name, info)
    counts = dict(box=(3, 0), square_prism=(7, 0), hex_prism=(11, 0), cylinder=(1, 1), cone=(0, 1), handled_cylinder=(1, 0))
    if name in counts:
        assert (len(info.get("symmetries_discrete", [])), len(info.get("symmetries_continuous", []))) == counts[name]
    rep = info["report"]
    assert rep["count"] == 2048 and all(a <= rep["tol"] for a in rep["accepted"] + rep["continuous"])


def _box_pose():
    from cppf2_amd import render
    Rm, _ = render.sample_pose(render.item_rng(5, 0), True)
    return Rm, np.array([0.05, -0.03, -0.7])                    # OpenGL camera frame: 0.7 m in front


def test_detected_symmetries_score_a_turned_box_as_correct(solids):
    """The value of the feature: a true pose of the box composed with its half-turn about its shortest side's axis.  With the
    detected set MSSD is at most tol x diameter; without it (the identity alone, what --gt_pose without --models_info gives)
    the same pose is off by more than half the diameter."""
    from cppf2_amd import bop, ops, render
    mesh, info = solids["box"]
    with_syms = bop.ObjectInfo.from_mesh(mesh, models_info=info)
    without = bop.ObjectInfo.from_mesh(mesh)
    assert len(with_syms.syms) == 4 and len(without.syms) == 1
    Rm, tr = _box_pose()
    Rg, tg = render.GL2CV @ Rm, render.GL2CV @ tr
    S = ref.POSE_R @ ref._rodrigues([1.0, 0.0, 0.0], np.pi) @ ref.POSE_R.T         # about the centre: the centred frame's origin
    dev = ops._dev()
    errs = [bop.mssd_mspd(o.device(dev)[0], o.device(dev)[2], np.hstack([Rg @ S, tg[:, None]]).reshape(1, 12),
                          np.hstack([Rg, tg[:, None]]).reshape(1, 12), render.INTRINSICS)[0].cpu().numpy()[0]
            for o in (with_syms, without)]
    print("mssd / diameter with and without the detected set:", errs[0] / with_syms.diameter, errs[1] / without.diameter)
    assert errs[0] <= 0.01 * with_syms.diameter
    assert errs[1] > 0.5 * without.diameter


def _write_ply(path, verts, faces):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(verts))
        f.write("element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(faces))
        f.writelines("%.9g %.9g %.9g\n" % tuple(v) for v in verts)
        f.writelines("3 %d %d %d\n" % tuple(t) for t in faces)


def test_eval_main_detect_symmetries(tmp_path, monkeypatch):
    """eval.main(data="depth", mesh=<box>, gt_pose=..., detect_symmetries=True) on a rendered view of the box: the report's
    `symmetries` names three half-turns, and the BOP errors agree with those of a run given the box's hand-written models_info
    (three exact half-turns about the centre), within the restatement tolerance."""
    import torch
    from PIL import Image
    from cppf2_amd import bop, ops, render
    monkeypatch.chdir(ROOT)
    import eval as ev
    dev = ops._dev()
    v, f = ref.solid_meshes()["box"]
    ply = str(tmp_path / "box.ply")
    _write_ply(ply, v, f)
    mesh = render.load_mesh(ply, ref.MESH_SCALE)
    b = mesh.bounds
    Rm, tr = _box_pose()
    P = render.camera_pose(Rm, tr, 1.0, (b[0] + b[1]) / 2)
    verts, tris = mesh.device(dev)
    depth = render.render_depth(verts, tris, ops._offsets([tris.shape[0]], dev), torch.from_numpy(P[None]).to(dev))[0].cpu().numpy()
    assert (depth > 0).sum() > 500
    dpath, mpath, ppath, ipath = (str(tmp_path / n) for n in ("d.png", "m.png", "pose.txt", "info.json"))
    Image.fromarray(np.round(depth * 1000).astype(np.uint16)).save(dpath)
    Image.fromarray(((depth > 0) * 255).astype(np.uint8)).save(mpath)
    np.savetxt(ppath, P.astype(np.float64).reshape(3, 4))
    c = v.mean(0)                                                                   # the box's centre, millimetres
    hand = []
    for a in np.eye(3):
        T = np.eye(4)
        T[:3, :3] = ref.POSE_R @ ref._rodrigues(a, np.pi) @ ref.POSE_R.T
        T[:3, 3] = c - T[:3, :3] @ c
        hand.append(T.reshape(16).tolist())
    json.dump(dict(diameter=float(bop.diameter(v)), symmetries_discrete=hand), open(ipath, "w"))
    kw = dict(data="depth", depth=dpath, mask=mpath, intrinsics=render.INTRINSICS.tolist(), num_pairs=5000, num_rots=36,
              opt=False, debug=True, mesh=ply, mesh_scale=ref.MESH_SCALE, gt_pose=ppath)
    rep = ev.main(detect_symmetries=True, **kw)
    s = rep["symmetries"]
    assert (s["discrete"], s["continuous"], s["isotropic"]) == (3, 0, False) and s["largest_accepted"] < 1e-4
    want = ev.main(models_info=ipath, **kw)
    assert "symmetries" not in want
    got_e, want_e = rep["results"][0]["bop"], want["results"][0]["bop"]
    print("bop errors, detected and hand-written:", got_e, want_e)
    assert np.isfinite(want_e["mssd"]) and np.isfinite(want_e["mspd"])
    assert got_e["vsd"] == want_e["vsd"]
    assert abs(got_e["mssd"] - want_e["mssd"]) <= REL_TOL * max(1.0, want_e["mssd"])
    assert abs(got_e["mspd"] - want_e["mspd"]) <= REL_TOL * max(render.WIDTH, want_e["mspd"])
    assert rep["bop"].keys() == want["bop"].keys()
