"""CPU checks of depth-view fusion: the NumPy restatement (tests/fuse_ref.py) on analytic depth images of
a sphere -- the properties the definition promises --, the wrapper's host logic on torch's CPU device, the entry points'
validation through ctypes and the command line's argument errors.  The kernels themselves: tests/test_fuse_gpu.py."""
import ctypes as C
import functools
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuse_ref as ref  # noqa: E402

VOXEL = ref.VOXEL


@functools.lru_cache(maxsize=None)
def sphere24():
    """The 24 views of the bare sphere, the volume around it and the fused (acc, wsum): computed once, read by all."""
    depth, masks, poses = ref.sphere_views(ref.fibonacci(24))
    origin, dims, trunc = ref.sphere_volume()
    acc, wsum = ref.fuse(depth, masks, poses, origin, dims, VOXEL, trunc)
    return dict(depth=depth, masks=masks, poses=poses, origin=origin, dims=dims, trunc=trunc, acc=acc, wsum=wsum)


def _mesh(acc, wsum, origin, min_weight=1):
    tris, keys, status, src = ref.extract(acc, wsum, origin, VOXEL, min_weight)
    verts, faces, boundary = ref.weld(tris, keys)
    return dict(tris=tris, keys=keys, status=status, src=src, verts=verts, faces=faces, boundary=boundary)


def _closed_manifold(faces):
    _, und = ref.edge_use(faces)
    _, dire = ref.directed_edge_use(faces)
    return bool((und == 2).all() and (dire == 1).all())


def test_case_table_follows_its_rule_and_the_kernel_holds_the_same_words():
    assert ref.derive_tet_cases() == ref.TET_CASES
    src = open(os.path.join(ROOT, "cppf2_amd", "csrc", "cppf_fuse.hip")).read()
    words = [int(w, 16) for w in re.findall(r"0x[0-9a-f]{4}", src.split("TET_CASES[16] = {")[1].split("};")[0])]
    assert len(words) == 16
    for m, edges in ref.TET_CASES.items():
        padded = edges + [edges[0]] * (4 - len(edges))
        assert words[m] == sum((lo | hi << 2) << (4 * q) for q, (lo, hi) in enumerate(padded)), m
    assert "-ffp-contract=off" in open(os.path.join(ROOT, "cppf2_amd", "build.py")).read()


def test_every_case_of_every_tetrahedron_is_wound_outwards():
    """A linear field on each of the six tetrahedra of a cell: every triangle's normal points along the gradient (from inside,
    negative, to outside), for both parities of the permutation."""
    rng = np.random.default_rng(0)
    offs = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], dtype=np.float64)
    for v1, v2, odd in ref.TETS:
        P = offs[[0, v1, v2, 7]]
        assert (np.linalg.det(P[1:] - P[0]) < 0) == odd
        for m, edges in ref.TET_CASES.items():
            t = rng.uniform(0.1, 1.0, 4) * np.where([(m >> p) & 1 for p in range(4)], -1.0, 1.0)
            g = np.linalg.solve(P[1:] - P[0], t[1:] - t[0])
            q = [P[lo] + (P[hi] - P[lo]) * (t[lo] / (t[lo] - t[hi])) for lo, hi in edges]
            for r in range(len(edges) - 2):
                b, c = (r + 2, r + 1) if odd else (r + 1, r + 2)
                assert np.cross(q[b] - q[0], q[c] - q[0]) @ g > 0, (v1, v2, m, r)


def test_closed_sphere_is_a_closed_manifold_within_one_voxel():
    s = sphere24()
    assert s["dims"] == (34, 34, 34)
    m = _mesh(s["acc"], s["wsum"], s["origin"])
    assert m["status"][0] == len(m["tris"]) > 1000
    assert m["boundary"] == 0 and _closed_manifold(m["faces"])
    V, E, Fc = len(m["verts"]), len(ref.edge_use(m["faces"])[0]), len(m["faces"])
    assert V - E + Fc == 2
    dist = ref.sphere_distance(m["verts"]).max() / VOXEL
    print("closed sphere: %d triangles, max distance %.3f voxel" % (Fc, dist))
    assert dist <= 1.0
    vol, want = ref.signed_volume(m["verts"], m["faces"]), 4.0 / 3.0 * np.pi * ref.RADIUS ** 3
    print("signed volume %+.2f %%" % (100 * (vol / want - 1)))
    assert vol > 0 and abs(vol / want - 1) <= 0.03
    # position is a function of key: weld asserts it on the raw triangles; and the keys name edges of the grid
    lo, d = m["keys"] >> 3, m["keys"] & 7
    assert (d >= 1).all() and (lo >= 0).all() and (lo < 34 ** 3).all()


def _table_views():
    d = ref.fibonacci(48)
    return d[d[:, 2] > 0.25]


def test_masks_keep_the_table_out_of_the_surface():
    """Rule 5 of the integrate definition: outside the mask a reading only carves."""
    dirs = _table_views()
    assert len(dirs) == 18
    depth, masks, poses = ref.sphere_views(dirs, plane_z=ref.CENTRE[2] - ref.RADIUS)
    assert (depth[masks == 0] > 0).mean() > 0.9                   # the table shows wherever the sphere does not
    origin, dims, trunc = ref.sphere_volume()
    with_m = _mesh(*ref.fuse(depth, masks, poses, origin, dims, VOXEL, trunc), origin)
    dist = ref.sphere_distance(with_m["verts"]) / VOXEL
    print("with masks: max %.3f voxel" % dist.max())
    assert len(with_m["verts"]) > 500 and dist.max() <= 1.0
    without = _mesh(*ref.fuse(depth, None, poses, origin, dims, VOXEL, trunc), origin)
    far = ref.sphere_distance(without["verts"]) / VOXEL
    print("without masks: %.1f %% beyond 1 voxel, max %.1f voxel" % (100 * (far > 1).mean(), far.max()))
    assert (far > 1.0).mean() > 0.20


@pytest.mark.parametrize("use_masks", [True, False])
def test_an_inconsistent_background_is_carved_away(use_masks):
    """A wall at camera depth 0.43 m behind the sphere in every view: no two views agree on it, so free space wins."""
    depth, masks, poses = ref.sphere_views(ref.fibonacci(24), wall=0.43)
    origin, dims, trunc = ref.sphere_volume()
    m = _mesh(*ref.fuse(depth, masks if use_masks else None, poses, origin, dims, VOXEL, trunc), origin)
    assert m["boundary"] == 0 and _closed_manifold(m["faces"])
    dist = ref.sphere_distance(m["verts"]).max() / VOXEL
    print("wall, masks %s: max %.3f voxel" % (use_masks, dist))
    assert dist <= 1.0


def _no_triangle_from_an_unknown_corner(m, wsum, min_weight):
    nx, ny, nz = wsum.shape
    lin = m["src"][:, 0]
    i, j, k = lin // (ny * nz), lin // nz % ny, lin % nz
    for c in range(8):
        assert (wsum[i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1)] >= min_weight).all()


def test_unknown_nodes_open_the_surface():
    s = sphere24()
    for mw in (1, 2, 4):
        m = _mesh(s["acc"], s["wsum"], s["origin"], mw)
        assert m["boundary"] == 0, mw
        _no_triangle_from_an_unknown_corner(m, s["wsum"], mw)
    m = _mesh(s["acc"], s["wsum"], s["origin"], 8)
    print("min_weight 8: %d boundary edges" % m["boundary"])
    assert m["boundary"] > 0 and len(m["faces"]) > 0
    _no_triangle_from_an_unknown_corner(m, s["wsum"], 8)
    dirs = ref.fibonacci(24)
    half = dirs[:, 2] > 0
    acc, wsum = ref.fuse(s["depth"][half], s["masks"][half], s["poses"][half], s["origin"], s["dims"], VOXEL, s["trunc"])
    m = _mesh(acc, wsum, s["origin"])
    print("one hemisphere: %d boundary edges" % m["boundary"])
    assert m["boundary"] > 0 and len(m["faces"]) > 0
    _no_triangle_from_an_unknown_corner(m, wsum, 1)


@pytest.mark.parametrize("k", [1, 23])
def test_incremental_integration_gives_the_same_bytes(k):
    s = sphere24()
    a, w = ref.fuse(s["depth"][:k], s["masks"][:k], s["poses"][:k], s["origin"], s["dims"], VOXEL, s["trunc"])
    a, w = ref.integrate(a, w, s["depth"][k:], s["masks"][k:], s["poses"][k:], ref.K4, 0.0, s["origin"], VOXEL, s["trunc"], 0.05)
    assert a.tobytes() == s["acc"].tobytes() and w.tobytes() == s["wsum"].tobytes()


# ----------------------------------------------------------------------------------------------
# the wrapper's host logic on torch's CPU device
# ----------------------------------------------------------------------------------------------
def test_weld_by_key_equals_the_restatement():
    import torch
    from cppf2_amd import fuse
    s = sphere24()
    acc = s["acc"].copy()
    acc[10:14, 10:14, 5:9] = 0.0                     # nodes of exactly 0: triangles without area
    tris, keys, _, _ = ref.extract(acc, s["wsum"], s["origin"], VOXEL)
    for drop in (True, False):
        v, f, b = fuse.weld_by_key(torch.from_numpy(tris), torch.from_numpy(keys), drop)
        rv, rf, rb = ref.weld(tris, keys, drop)
        assert np.array_equal(v.numpy().view(np.uint32), rv.view(np.uint32)) and np.array_equal(f.numpy(), rf) and b == rb
    assert len(ref.weld(tris, keys, True)[1]) < len(ref.weld(tris, keys, False)[1]) == len(tris)
    v, f, b = fuse.weld_by_key(torch.zeros((0, 9)), torch.zeros((0, 3), dtype=torch.int64))
    assert v.shape == (0, 3) and f.shape == (0, 3) and b == 0


def test_volume_around_boxes_the_masked_pixels():
    from cppf2_amd import fuse
    s = sphere24()
    K = np.array([[150.0, 0, 80], [0, 150.0, 60], [0, 0, 1]])
    b = fuse.Volume.bounds(s["depth"], s["masks"], s["poses"], K, dev="cpu")
    assert (np.abs(b[0] - (ref.CENTRE - ref.RADIUS)) < 0.002).all() and (np.abs(b[1] - (ref.CENTRE + ref.RADIUS)) < 0.002).all()
    vol = fuse.Volume.around(s["depth"], s["masks"], s["poses"], K, VOXEL, dev="cpu")
    assert abs(vol.trunc - 3 * VOXEL) < 1e-9 and vol.acc.shape == vol.dims == vol.wsum.shape
    pad = vol.trunc + vol.voxel
    assert (vol.origin <= b[0] - pad + 1e-6).all() and (vol.origin + (np.array(vol.dims) - 1) * vol.voxel >= b[1] + pad - 1e-6).all()
    assert max(vol.dims) <= 36 and vol.unknown_share == 1.0
    with pytest.raises(ValueError):
        fuse.Volume.bounds(s["depth"] * 0, s["masks"], s["poses"], K, dev="cpu")
    with pytest.raises(ValueError):
        fuse.Volume.bounds(s["depth"], s["masks"], s["poses"][:3], K, dev="cpu")
    with pytest.raises(ValueError):
        fuse.Volume((0, 0, 0), VOXEL, (0, 4, 4), dev="cpu")
    with pytest.raises(ValueError):
        fuse.Volume((0, 0, 0), VOXEL, (1024, 1024, 1024), dev="cpu")
    with pytest.raises(fuse.CppfError):             # no CPU fallback
        fuse.integrate(vol, s["depth"], s["poses"], K, s["masks"])
    with pytest.raises(fuse.CppfError):
        fuse.extract(vol)


# ----------------------------------------------------------------------------------------------
# validation: fake device addresses, 16-byte aligned and never dereferenced (every refusal comes before any device work)
# ----------------------------------------------------------------------------------------------
_A, _B, _C, _D, _E, _G = (0x100000 * (i + 1) for i in range(6))
_K = (C.c_double * 4)(150.0, 150.0, 80.0, 60.0)
_O = (C.c_double * 3)(0.0, 0.0, 0.0)
_NAN, _INF = float("nan"), float("inf")


def _integrate(lib, V=0, depth=_A, masks=_B, poses=_C, H=120, W=160, K=_K, po=0.0, origin=_O, voxel=0.004, dims=(8, 8, 8), trunc=0.012,
               znear=0.05, acc=_D, wsum=_E):
    return lib.cppf_tsdf_integrate(V, depth, masks, poses, H, W, K, po, origin, voxel, *dims, trunc, znear, acc, wsum, None)


def _extract(lib, acc=_A, wsum=_B, origin=_O, voxel=0.004, dims=(8, 8, 8), min_weight=1, capacity=16, tris=_C, keys=_D, status=_E,
             ws=_G, short=0):
    need = lib.cppf_tsdf_extract_workspace_bytes(*dims)
    return lib.cppf_tsdf_extract(acc, wsum, origin, voxel, *dims, min_weight, capacity, tris, keys, status, ws, need - short, None)


def test_integrate_validation_return_codes():
    from cppf2_amd import _lib
    lib = _lib.load()
    assert _integrate(lib) == 0                               # V == 0: a valid call that launches nothing
    assert _integrate(lib, masks=None) == 0
    assert _integrate(lib, dims=(1, 8, 8)) == 0               # an axis of length 1 is a volume
    assert _integrate(lib, dims=(512, 512, 512)) == 0         # the size limit itself
    for kw in (dict(acc=None), dict(wsum=None), dict(K=None), dict(origin=None), dict(V=1, depth=None), dict(V=1, poses=None),
               dict(V=-1), dict(dims=(0, 8, 8)), dict(dims=(8, -1, 8)), dict(dims=(8, 8, 0)), dict(dims=(512, 512, 513)),
               dict(dims=(1 << 20, 1 << 20, 1)), dict(voxel=0.0), dict(voxel=-0.004), dict(voxel=_NAN), dict(voxel=_INF),
               dict(trunc=0.0), dict(trunc=_NAN), dict(trunc=_INF), dict(znear=0.0), dict(znear=-1.0), dict(znear=_NAN),
               dict(H=0), dict(W=0), dict(po=_NAN), dict(origin=(C.c_double * 3)(0.0, _NAN, 0.0))):
        assert _integrate(lib, **kw) == -1, kw
        assert b"invalid argument" in lib.cppf_last_error_string()


def test_extract_validation_return_codes():
    from cppf2_amd import _lib
    lib = _lib.load()
    assert lib.cppf_tsdf_extract_workspace_bytes(34, 34, 34) == (2 * ((33 ** 3 + 255) // 256) + 2) * 4
    assert lib.cppf_tsdf_extract_workspace_bytes(1, 20, 20) == 8
    for dims in ((0, 8, 8), (8, 8, -1), (512, 512, 513)):
        assert lib.cppf_tsdf_extract_workspace_bytes(*dims) == -1
    for kw in (dict(acc=None), dict(wsum=None), dict(origin=None), dict(status=None), dict(ws=None), dict(tris=None), dict(keys=None),
               dict(dims=(0, 8, 8)), dict(dims=(8, 8, 0)), dict(dims=(512, 512, 513)), dict(voxel=0.0), dict(voxel=_NAN),
               dict(voxel=_INF), dict(min_weight=0), dict(min_weight=-3), dict(capacity=-1), dict(short=1)):
        assert _extract(lib, **kw) == -1, kw
        assert b"invalid argument" in lib.cppf_last_error_string()


# ----------------------------------------------------------------------------------------------
# the command line and the scene reader
# ----------------------------------------------------------------------------------------------
def _write_scene(d, n=3, obj_ids=(15,), masks=True):
    from PIL import Image
    os.makedirs(os.path.join(d, "depth"))
    os.makedirs(os.path.join(d, "mask_visib"))
    cam, gt = {}, {}
    for im in range(n):
        size = (12, 16) if im < 2 else (24, 32)                      # the third image has another size
        Image.fromarray(np.full(size, 4000 + im, np.uint16)).save(os.path.join(d, "depth", "%06d.png" % im))
        cam[str(im)] = dict(cam_K=[150.0, 0, 8, 0, 150.0, 6, 0, 0, 1], depth_scale=0.1)
        gt[str(im)] = []
        for g, o in enumerate(obj_ids):
            gt[str(im)].append(dict(cam_R_m2c=list(np.eye(3).reshape(-1)), cam_t_m2c=[1.0, 2.0, 400.0 + im], obj_id=o))
            if masks:
                Image.fromarray(np.full(size, 255 * (g == 0), np.uint8)).save(os.path.join(d, "mask_visib", "%06d_%06d.png" % (im, g)))
    json.dump(cam, open(os.path.join(d, "scene_camera.json"), "w"))
    json.dump(gt, open(os.path.join(d, "scene_gt.json"), "w"))
    return d


def test_read_views_groups_by_size_and_scales_the_poses(tmp_path):
    from cppf2_amd import fuse
    d = _write_scene(str(tmp_path / "scene"), obj_ids=(15, 7))
    with pytest.raises(fuse.ViewsError, match="--obj-id"):
        fuse.read_views(d)
    with pytest.raises(fuse.ViewsError, match="no image shows"):
        fuse.read_views(d, obj_id=3)
    b = fuse.read_views(d, obj_id=7)
    assert [x["depths"].shape for x in b] == [(2, 12, 16), (1, 24, 32)] and [x["im_ids"] for x in b] == [[0, 1], [2]]
    assert b[0]["depths"].dtype == np.float32 and abs(b[0]["depths"][1, 0, 0] - 0.4001) < 1e-7
    assert np.allclose(b[1]["poses"][0].reshape(3, 4), np.hstack([np.eye(3), [[0.001], [0.002], [0.402]]]))
    assert b[0]["masks"].dtype == np.uint8 and not b[0]["masks"].any()          # object 7 is the second instance: mask ..._000001
    assert fuse.read_views(d, obj_id=15)[0]["masks"].all()
    assert fuse.read_views(d, obj_id=15, use_masks=False)[0]["masks"] is None
    os.remove(os.path.join(d, "mask_visib", "000001_000000.png"))
    with pytest.raises(fuse.ViewsError, match="--no-masks"):
        fuse.read_views(d, obj_id=15)


def test_cli_errors_are_loud(tmp_path, capsys):
    from cppf2_amd import fuse
    out = str(tmp_path / "o.ply")
    d = _write_scene(str(tmp_path / "scene"))
    for argv in (["--views", d, "--out", out],                                     # no --voxel
                 ["--views", d, "--voxel", "0", "--out", out],
                 ["--views", d, "--voxel", "nan", "--out", out],
                 ["--views", d, "--voxel", "0.002", "--trunc", "-1", "--out", out],
                 ["--views", d, "--voxel", "0.002", "--min-weight", "0", "--out", out],
                 ["--views", d, "--voxel", "0.002", "--mesh-scale", "0", "--out", out],
                 ["--views", d, "--voxel", "0.002", "--out", str(tmp_path / "o.obj")],
                 ["--voxel", "0.002", "--out", out]):
        with pytest.raises(SystemExit) as e:
            fuse.main(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    os.remove(os.path.join(d, "scene_gt.json"))
    with pytest.raises(fuse.ViewsError, match="scene_gt.json"):
        fuse.main(["--views", d, "--voxel", "0.002", "--out", out])
    with pytest.raises(fuse.ViewsError):
        fuse.main(["--views", str(tmp_path / "nowhere"), "--voxel", "0.002", "--out", out])
    assert not os.path.exists(out)
