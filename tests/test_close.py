"""CPU checks of closing a fused volume: the NumPy restatement (tests/close_ref.py) against
scipy.ndimage.label and on the analytic scenes -- a sphere on and sunk into a table, with and without the plane, and a sphere
with a patch of dropped readings --, the entry points' validation through ctypes, the wrapper's host logic and the command
line's argument errors.  The kernels themselves: tests/test_close_gpu.py."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import close_ref as cref  # noqa: E402
import fuse_ref as ref  # noqa: E402

VOXEL = ref.VOXEL
DOME_PZ = ref.CENTRE[2] - 0.6 * ref.RADIUS              # the sphere sunk into the table: a dome stands on it
TANGENT_PZ = ref.CENTRE[2] - ref.RADIUS                 # the sphere resting on the table


@functools.lru_cache(maxsize=None)
def fused(scene, noise=False):
    """(acc, wsum, origin, trunc) of a scene's views fused by the restatement: computed once, read by all.  scene: "dome",
    "tangent" (18 views from above the table), 10 or 20 (the 24-view bare sphere without the readings within that many degrees of
    +x).  noise: 1 mm Gaussian noise (seed 0) on every reading."""
    if scene in ("dome", "tangent"):
        depth, masks, poses = cref.table_views(cref.table_dirs(), DOME_PZ if scene == "dome" else TANGENT_PZ)
    else:
        depth, masks, poses = cref.dropout_views(scene)
    if noise:
        depth = np.where(depth > 0, depth + np.random.default_rng(0).normal(0, 0.001, depth.shape), 0).astype(np.float32)
    origin, dims, trunc = ref.sphere_volume()
    acc, wsum = ref.fuse(depth, masks, poses, origin, dims, VOXEL, trunc)
    for a in (acc, wsum):
        a.setflags(write=False)
    return acc, wsum, origin, trunc


def table_plane(pz, lift=0.0):
    return (0.0, 0.0, 1.0, -(pz + lift))


def mesh_of(acc, wsum, origin):
    tris, keys, _, _ = ref.extract(acc, wsum, origin, VOXEL)
    return ref.weld(tris, keys)


@functools.lru_cache(maxsize=None)
def closed(scene, noise=False, plane_z=None, lift=0.0):
    """dict(before: the unclosed mesh's boundary edges, verts, faces, stats, and close_ref.topology's entries) of a scene closed by
    the restatement with the table plane at plane_z + lift (None: no plane)."""
    acc, wsum, origin, trunc = fused(scene, noise)
    plane = None if plane_z is None else table_plane(plane_z, lift)
    a, w, state, stats = cref.close(acc, wsum, origin, VOXEL, trunc, 1, plane)
    verts, faces, boundary = mesh_of(a, w, origin)
    top = cref.topology(verts, faces)
    assert top["boundary"] == boundary
    return dict(top, before=mesh_of(acc, wsum, origin)[2], verts=verts, faces=faces, stats=[int(s) for s in stats], state=state)


CLOSED = dict(boundary=0, manifold=True, components=1, euler=2)


def assert_topology(m, want=CLOSED):
    assert {k: m[k] for k in want} == want


def assert_on_table(m, pz, lift, dist_measured, vol_measured):
    """The lowest vertex lies on the (lifted) plane; the farthest vertex from (sphere or plane) and the signed volume against the
    analytic cap stay within twice what the restatement measured when this test was written (DESIGN.md section 31 lists them:
    expectations, with the factor of two as the bound)."""
    z = pz + lift
    low = float(m["verts"][:, 2].astype(np.float64).min()) - z
    dist = float(cref.distance_to_sphere_or_plane(m["verts"], z).max()) / VOXEL
    vol = ref.signed_volume(m["verts"], m["faces"]) / cref.cap_volume(z) - 1
    print("lowest vertex %+.2e m from the plane, farthest vertex %.3f voxel, volume %+.2f %%, states %s" % (low, dist, 100 * vol, m["stats"]))
    assert abs(low) <= 1e-6
    assert dist <= 2 * dist_measured
    assert abs(vol) <= 2 * vol_measured


# ----------------------------------------------------------------------------------------------
# the restatement itself
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,p", [((33, 17, 9), 0.25), ((33, 17, 9), 0.4), ((20, 21, 22), 0.31), ((1, 20, 20), 0.5), ((5, 1, 7), 0.5),
                                    ((2, 2, 2), 0.5), ((1, 1, 1), 1.0)])
def test_the_flood_finds_what_scipy_labels(dims, p):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(sum(dims))
    cand = rng.random(dims) < p
    labels, n = ndimage.label(cand)                                    # the default structure is 6-connectivity
    touching = np.unique(labels[cref.faces(dims) & cand])
    want = np.isin(labels, touching[touching > 0])
    got = cref.flood(cand, cref.faces(dims))
    assert np.array_equal(got, want)
    if min(dims) > 2 and p < 0.35:
        assert (cand & ~got).any() and got.any()                       # both kinds of component occur


def test_the_restatement_follows_the_definition_on_a_small_volume():
    dims, trunc = (5, 4, 6), np.float32(0.012)
    wsum = np.ones(dims, np.int32)
    acc = np.full(dims, 0.5, np.float32)
    wsum[2, 2, 1:5] = 0                                                # an enclosed row of four unseen nodes
    wsum[0, 0, 5] = 0                                                  # an unseen corner above the plane: open
    acc[3, 1, 1], acc[3, 1, 4] = np.nan, -1.0
    origin = np.zeros(3, np.float32)
    a, w, s, stats = cref.close(acc, wsum, origin, 0.004, trunc, 1, (0, 0, 1, -0.008))       # the plane through k = 2 exactly
    assert stats.tolist() == [115, 2, 2, 1] and s[0, 0, 5] == cref.OPEN and a[0, 0, 5] == 0 and w[0, 0, 5] == 0
    assert s[2, 2].tolist() == [0, 2, 2, 1, 1, 0] and w[2, 2].tolist() == [1] * 6

    def b(k):                                                          # the plane's own value at z index k, float32 as stated
        h = np.float32(k) * np.float32(0.004) + np.float32(-0.008)
        return max(min(-h / trunc, np.float32(1)), np.float32(-1))
    # below and on the plane every decided node is >= 0 (k = 2: h == 0, b = -0.0, which is outside like +0); above it the
    # enclosed nodes are inside, sharpened to the plane within trunc of it; a known node keeps its value unless the plane's is larger
    assert b(1) > 0.3 and b(3) < -0.3 and b(4) < -0.6
    assert a[2, 2, 1] == b(1) and a[2, 2, 2] == 0 and np.signbit(a[2, 2, 2]) and a[2, 2, 3] == b(3) and a[2, 2, 4] == b(4)
    assert np.isnan(a[3, 1, 1]) and a[3, 1, 4] == b(4) and a[1, 1, 0] == b(0) > 0.5 and a[1, 1, 5] == 0.5
    a2, w2, s2, stats2 = cref.close(acc, wsum, origin, 0.004, trunc, 1, None)
    assert stats2.tolist() == [115, 4, 0, 1] and (a2[2, 2, 1:5] == -1).all() and a2[1, 1, 0] == 0.5 and a2[3, 1, 4] == -1
    a3, _, s3, stats3 = cref.close(acc, wsum * 2, origin, 0.004, trunc, 2, None)             # t = acc / wsum; min_weight
    assert np.array_equal(s3, s2) and a3[1, 1, 5] == 0.25
    assert cref.close(acc, wsum, origin, 0.004, trunc, 2, None)[3].tolist() == [0, 0, 0, 120]


# ----------------------------------------------------------------------------------------------
# what the definition does on the scenes
# ----------------------------------------------------------------------------------------------
def test_the_dome_closes_with_its_bottom_on_the_plane():
    m = closed("dome", plane_z=DOME_PZ)
    assert m["before"] == 180
    assert_topology(m)
    assert m["stats"] == [24888, 4075, 10341, 0]
    assert_on_table(m, DOME_PZ, 0.0, dist_measured=0.8112, vol_measured=0.03181)


@pytest.mark.parametrize("lift,dist_measured,vol_measured,stats", [(0.0, 0.8112, 0.03231, [24954, 4008, 10342, 0]),
                                                                  (VOXEL, 0.7586, 0.03229, [24954, 3790, 10560, 0])])
def test_the_dome_with_depth_noise_closes(lift, dist_measured, vol_measured, stats):
    m = closed("dome", noise=True, plane_z=DOME_PZ, lift=lift)
    assert m["before"] == 180
    assert_topology(m)
    assert m["stats"] == stats
    assert_on_table(m, DOME_PZ, lift, dist_measured, vol_measured)


@pytest.mark.parametrize("lift,dist_measured,vol_measured", [(VOXEL / 4, 1.0639, 0.03373), (VOXEL / 2, 1.0997, 0.03469),
                                                             (VOXEL, 1.1818, 0.03548)])
def test_the_resting_sphere_closes_into_one_component_with_a_lifted_plane(lift, dist_measured, vol_measured):
    m = closed("tangent", plane_z=TANGENT_PZ, lift=lift)
    assert m["before"] == 600
    assert_topology(m)
    assert m["stats"] == [30021, 4609, 4674, 0]
    assert_on_table(m, TANGENT_PZ, lift, dist_measured, vol_measured)


def test_without_a_lift_the_resting_sphere_closes_with_two_specks():
    """Documented, not wanted: single unseen nodes in the layer just above the plane are enclosed and filled as inside -- two
    extra components of 24 triangles and 2e-11 m^3 each.  The lift is what removes them."""
    m = closed("tangent", plane_z=TANGENT_PZ)
    assert_topology(m, dict(boundary=0, manifold=True, components=3, euler=6))
    assert m["stats"] == [30021, 4659, 4624, 0]
    assert_on_table(m, TANGENT_PZ, 0.0, dist_measured=1.0406, vol_measured=0.03237)
    verts, faces = m["verts"], m["faces"]
    low = np.nonzero(verts[:, 2] < TANGENT_PZ + 2.5 * VOXEL)[0]
    specks = [c for c in _components(faces) if len(c) == 24]
    assert len(specks) == 2
    for c in specks:
        assert np.isin(faces[c], low).all() and 0 < ref.signed_volume(verts, faces[c]) < 1e-10


def _components(faces):
    """Lists of face indices, one per connected component."""
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in faces:
        parent[find(b)] = find(a)
        parent[find(c)] = find(a)
    groups = {}
    for f, (a, _, _) in enumerate(faces):
        groups.setdefault(find(a), []).append(f)
    return list(groups.values())


@pytest.mark.parametrize("scene,before,unseen", [("dome", 180, 14416), ("tangent", 600, 9283)])
def test_without_a_plane_the_space_under_the_table_reaches_the_border_and_stays_open(scene, before, unseen):
    """The honest answer: nothing is enclosed, so nothing is filled and the mesh is the unclosed one."""
    m = closed(scene)
    acc, wsum, origin, _ = fused(scene)
    assert m["before"] == m["boundary"] == before
    assert m["stats"][1:] == [0, 0, unseen] and m["stats"][0] == int((wsum > 0).sum())
    verts, faces, _ = mesh_of(acc, wsum, origin)
    assert np.array_equal(verts, m["verts"]) and np.array_equal(faces, m["faces"])


def test_a_small_patch_no_view_measured_is_closed_without_a_plane():
    m = closed(10)
    assert m["before"] == 40
    assert_topology(m)
    assert m["stats"] == [35224, 3730, 0, 350]
    dist = float(ref.sphere_distance(m["verts"]).max()) / VOXEL
    vol = ref.signed_volume(m["verts"], m["faces"]) / (4.0 / 3.0 * np.pi * ref.RADIUS ** 3) - 1
    print("10 degrees: farthest vertex %.3f voxel, volume %+.2f %%" % (dist, 100 * vol))
    assert dist <= 2 * 1.5878 and abs(vol) <= 2 * 0.01345


def test_a_patch_whose_unseen_chimney_reaches_the_border_stays_open():
    """The stated limit: the unseen space in front of a 20 degree patch reaches the volume's border, 4 voxels away, so the
    interior it is joined to is open as well and the mesh does not close."""
    m = closed(20)
    assert m["before"] == 74 and m["boundary"] == 118 and not m["manifold"]
    assert m["stats"] == [35047, 8, 0, 4249]


# ----------------------------------------------------------------------------------------------
# the wrapper's host logic on torch's CPU device
# ----------------------------------------------------------------------------------------------
def test_planes_are_normalised_lifted_and_taken_into_the_object_frame():
    from cppf2_amd import fuse
    p = fuse.unit_plane((0, 0, 2, -0.1))
    assert p.dtype == np.float64 and np.allclose(p, [0, 0, 1, -0.05], atol=1e-15)
    assert np.allclose(fuse.unit_plane((0, 3, 4, 1), lift=0.002), [0, 0.6, 0.8, 0.2 - 0.002], atol=1e-15)
    for bad in ((0, 0, 0, 1), (0, 0, 1), (0, np.nan, 1, 0), (0, 0, np.inf, 0)):
        with pytest.raises(ValueError):
            fuse.unit_plane(bad)
    with pytest.raises(ValueError):
        fuse.unit_plane((0, 0, 1, 0), lift=-0.001)
    # a point of the object's frame on the object-frame plane lies on the camera-frame plane after the pose
    rng = np.random.default_rng(1)
    pose = ref.look_at(ref.fibonacci(5)[1:2]).astype(np.float64).reshape(3, 4)
    n_c = rng.normal(size=3)
    n_c /= np.linalg.norm(n_c)
    plane_c = np.concatenate([n_c, [-0.37]])
    plane_o = fuse.plane_to_object(plane_c, pose)
    assert abs(np.linalg.norm(plane_o[:3]) - 1) < 1e-6
    for x_o in rng.normal(size=(4, 3)):
        x_c = pose[:, :3] @ x_o + pose[:, 3]
        assert abs((plane_c[:3] @ x_c + plane_c[3]) - (plane_o[:3] @ x_o + plane_o[3])) < 1e-6


def test_close_has_no_cpu_fallback_and_checks_its_arguments():
    from cppf2_amd import fuse
    vol = fuse.Volume((0, 0, 0), VOXEL, (4, 4, 4), dev="cpu")
    with pytest.raises(fuse.CppfError):
        fuse.close(vol)
    with pytest.raises(fuse.CppfError):
        fuse.close(vol, plane=(0, 0, 1, 0))


# ----------------------------------------------------------------------------------------------
# validation: fake device addresses, 16-byte aligned and never dereferenced (every refusal comes before any device work)
# ----------------------------------------------------------------------------------------------
_A, _B, _C, _D, _E, _G, _H = (0x100000 * (i + 1) for i in range(7))
_O = (C.c_double * 3)(0.0, 0.0, 0.0)
_NAN, _INF = float("nan"), float("inf")
_NODES = 8 * 8 * 8


def _plane(*p):
    return (C.c_double * 4)(*p)


def _close(lib, acc=_A, wsum=_B, origin=_O, voxel=0.004, dims=(8, 8, 8), trunc=0.012, min_weight=1, plane=_plane(0, 0, 1, -0.01),
           acc_out=_C, wsum_out=_D, state=_E, stats=_G, ws=_H, short=0):
    need = lib.cppf_tsdf_close_workspace_bytes(*dims)
    return lib.cppf_tsdf_close(acc, wsum, origin, voxel, *dims, trunc, min_weight, plane, acc_out, wsum_out, state, stats, ws,
                               need - short, None)


def test_close_validation_return_codes():
    from cppf2_amd import _lib
    lib = _lib.load()
    assert lib.cppf_tsdf_close_workspace_bytes(34, 34, 34) == 4 * 34 ** 3
    assert lib.cppf_tsdf_close_workspace_bytes(1, 1, 1) == 4 and lib.cppf_tsdf_close_workspace_bytes(512, 512, 512) == 1 << 29
    for dims in ((0, 8, 8), (8, 8, -1), (512, 512, 513), (1 << 20, 1 << 20, 1)):
        assert lib.cppf_tsdf_close_workspace_bytes(*dims) == -1
    bad = [dict(acc=None), dict(wsum=None), dict(origin=None), dict(acc_out=None), dict(wsum_out=None), dict(state=None), dict(stats=None),
           dict(ws=None), dict(dims=(0, 8, 8)), dict(dims=(8, 8, 0)), dict(dims=(512, 512, 513)), dict(voxel=0.0), dict(voxel=_NAN),
           dict(voxel=_INF), dict(origin=(C.c_double * 3)(0.0, _NAN, 0.0)), dict(trunc=0.0), dict(trunc=-0.012), dict(trunc=_NAN),
           dict(trunc=_INF), dict(min_weight=0), dict(min_weight=-3), dict(short=1),
           # an output that aliases an input, wholly or in part, and outputs that overlap
           dict(acc_out=_A), dict(wsum_out=_B), dict(acc_out=_B), dict(wsum_out=_A), dict(state=_A), dict(stats=_B), dict(ws=_A),
           dict(acc_out=_A + 4 * _NODES - 4), dict(acc_out=_A - 4 * _NODES + 4), dict(state=_B + 4 * _NODES - 1), dict(stats=_A - 24),
           dict(wsum_out=_C), dict(state=_C + 16), dict(ws=_D), dict(stats=_H + 8),
           # the plane: not finite, not finite as float32, not a unit normal
           dict(plane=_plane(0, 0, _NAN, 0)), dict(plane=_plane(0, 0, 1, _INF)), dict(plane=_plane(_INF, 0, 0, 0)),
           dict(plane=_plane(0, 0, 1, 1e39)), dict(plane=_plane(0, 0, 0, 1)), dict(plane=_plane(0, 0, 1.001, 0)),
           dict(plane=_plane(0, 0, 0.999, 0)), dict(plane=_plane(1, 1, 0, 0))]
    for kw in bad:
        assert _close(lib, **kw) == -1, kw
        assert b"invalid argument" in lib.cppf_last_error_string()


# ----------------------------------------------------------------------------------------------
# the command line
# ----------------------------------------------------------------------------------------------
def _write_scene(d, n=2):
    import json
    from PIL import Image
    os.makedirs(os.path.join(d, "depth"))
    os.makedirs(os.path.join(d, "mask_visib"))
    cam, gt = {}, {}
    for im in range(n):
        Image.fromarray(np.full((12, 16), 4000 + im, np.uint16)).save(os.path.join(d, "depth", "%06d.png" % im))
        Image.fromarray(np.full((12, 16), 255, np.uint8)).save(os.path.join(d, "mask_visib", "%06d_000000.png" % im))
        cam[str(im)] = dict(cam_K=[150.0, 0, 8, 0, 150.0, 6, 0, 0, 1], depth_scale=0.1)
        gt[str(im)] = [dict(cam_R_m2c=list(np.eye(3).reshape(-1)), cam_t_m2c=[1.0, 2.0, 400.0 + im], obj_id=15)]
    json.dump(cam, open(os.path.join(d, "scene_camera.json"), "w"))
    json.dump(gt, open(os.path.join(d, "scene_gt.json"), "w"))
    return d


def test_cli_errors_are_loud(tmp_path, capsys, monkeypatch):
    import torch
    from cppf2_amd import fuse, segment
    out = str(tmp_path / "o.ply")
    d = _write_scene(str(tmp_path / "scene"))
    base = ["--views", d, "--voxel", "0.002", "--out", out]
    for extra in (["--support-plane", "0,0,1,-0.1"],                               # without --close
                  ["--support-plane", "auto"],
                  ["--support-lift", "0.001"],
                  ["--close", "--support-lift", "0.001"],                          # a lift without a plane
                  ["--close", "--support-plane", "0,0,0,1"],                       # a zero normal
                  ["--close", "--support-plane", "0,0,1"],
                  ["--close", "--support-plane", "0,0,nan,1"],
                  ["--close", "--support-plane", "table"],
                  ["--close", "--support-plane", "0,0,1,-0.1", "--support-lift", "-0.001"],
                  ["--close", "--support-plane", "0,0,1,-0.1", "--support-lift", "nan"]):
        with pytest.raises(SystemExit) as e:
            fuse.main(base + extra)
        assert e.value.code == 2, extra
    assert "lies this far above the table" in " ".join(_help_text(fuse, capsys).split())
    # auto with an unusable fit: refused before anything is fused
    seen = []

    def no_plane(depth, K, seeds, *a, **k):
        seen.append((np.asarray(depth).shape, seeds))
        return torch.zeros((1, 4)), torch.tensor([[-1, 0, 0, 192]], dtype=torch.int32)
    monkeypatch.setattr(segment, "fit_plane", no_plane)
    for track in ([], ["--track"]):
        with pytest.raises(fuse.ViewsError, match="--support-plane auto found no plane"):
            fuse.main(base + ["--close", "--support-plane", "auto"] + track)
    assert seen == [((1, 12, 16), 0)] * 2                                          # the first view's whole depth image, seed 0
    assert not os.path.exists(out)


def _help_text(fuse, capsys):
    capsys.readouterr()
    with pytest.raises(SystemExit):
        fuse.main(["--help"])
    return capsys.readouterr().out
