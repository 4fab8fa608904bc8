"""GPU checks of depth-view fusion: cppf_tsdf_integrate and cppf_tsdf_extract bit-equal to the NumPy
restatement (tests/fuse_ref.py) at every shape that takes another path, the capacity protocol, the winding against the
rasterizer's culling, and python -m cppf2_amd.fuse on a rendered BOP scene of the fixture mesh."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuse_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, "tests", "golden", "example_data", "obj_000015.ply")
VOXEL = ref.VOXEL
ZNEAR = 0.05
CANARY_F, CANARY_K = -7.25, -77


def _c3(x):
    return (C.c_double * 3)(*[float(v) for v in x])


def dev_integrate(acc, wsum, depth, masks, poses, K4, pixel_offset, origin, voxel, trunc, znear=ZNEAR):
    """cppf_tsdf_integrate itself on host arrays: (acc, wsum) as the kernel left them."""
    import torch
    from cppf2_amd import _lib, ops
    dev = ops._dev()
    a = torch.from_numpy(np.array(acc, dtype=np.float32)).to(dev)
    w = torch.from_numpy(np.array(wsum, dtype=np.int32)).to(dev)
    d = torch.from_numpy(np.array(depth, dtype=np.float32)).to(dev)
    m = None if masks is None else torch.from_numpy(np.array(masks, dtype=np.uint8)).to(dev)
    P = torch.from_numpy(np.array(poses, dtype=np.float32).reshape(-1, 12)).to(dev)
    V, H, W = d.shape
    _lib.check(_lib.load().cppf_tsdf_integrate(V, ops._p(d), ops._p(m), ops._p(P), H, W, (C.c_double * 4)(*K4), C.c_float(pixel_offset),
                                               _c3(origin), C.c_float(voxel), *a.shape, C.c_float(trunc), C.c_float(znear), ops._p(a),
                                               ops._p(w), ops._stream()), "cppf_tsdf_integrate")
    return a.cpu().numpy(), w.cpu().numpy()


def dev_extract(acc, wsum, origin, voxel, min_weight=1, capacity=None):
    """cppf_tsdf_extract itself, the workspace exactly as large as asked for, the outputs filled with canaries: (tris [capacity,9],
    keys [capacity,3], status); capacity None = what a counting call (capacity 0, NULL outputs) reports."""
    import torch
    from cppf2_amd import _lib, ops
    dev, L = ops._dev(), _lib.load()
    a = torch.from_numpy(np.array(acc, dtype=np.float32)).to(dev)
    w = torch.from_numpy(np.array(wsum, dtype=np.int32)).to(dev)
    ws = torch.empty((L.cppf_tsdf_extract_workspace_bytes(*a.shape),), dtype=torch.uint8, device=dev)
    status = torch.full((2,), -5, dtype=torch.int64, device=dev)

    def call(cap, tris, keys):
        _lib.check(L.cppf_tsdf_extract(ops._p(a), ops._p(w), _c3(origin), C.c_float(voxel), *a.shape, int(min_weight), cap, ops._p(tris),
                                       ops._p(keys), ops._p(status), ops._p(ws), ws.numel(), ops._stream()), "cppf_tsdf_extract")
        return tuple(int(x) for x in status.cpu().tolist())
    if capacity is None:
        capacity = call(0, None, None)[0]
    tris = torch.full((capacity, 9), CANARY_F, dtype=torch.float32, device=dev)
    keys = torch.full((capacity, 3), CANARY_K, dtype=torch.int64, device=dev)
    st = call(capacity, tris, keys)
    return tris.cpu().numpy(), keys.cpu().numpy(), st


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def assert_extract_equal(acc, wsum, origin, voxel, min_weight=1):
    rt, rk, rs, _ = ref.extract(acc, wsum, origin, voxel, min_weight)
    t, k, s = dev_extract(acc, wsum, origin, voxel, min_weight)
    assert s == rs, (s, rs)
    assert same_bits(k, rk), "keys"
    assert same_bits(t, rt.reshape(-1, 9)), "triangles"
    return rs


@pytest.fixture(scope="module")
def sphere():
    """The 24 analytic sphere views, the 34^3 volume around the sphere and the restatement's fusion of them: computed once."""
    depth, masks, poses = ref.sphere_views(ref.fibonacci(24))
    origin, dims, trunc = ref.sphere_volume()
    acc, wsum = ref.fuse(depth, masks, poses, origin, dims, VOXEL, trunc)
    return dict(depth=depth, masks=masks, poses=poses, origin=origin, dims=dims, trunc=trunc, acc=acc, wsum=wsum)


def _rough_views(V, seed, H=48, W=64):
    """Views that reach every skip of the integrate definition for a volume of a few centimetres at the origin: cameras 0.01 ..
    0.12 m from it (part of the volume behind the camera or nearer than znear; it projects off all four borders of the small
    image), depth readings 0.02 .. 0.2 m with holes, a negative reading, an infinite one and one NaN, random masks."""
    rng = np.random.default_rng(seed)
    dirs = ref.fibonacci(max(V, 2))[:V]
    poses = np.concatenate([ref.look_at(d[None], centre=np.array([0.03, 0.02, 0.01]), dist=r)
                            for d, r in zip(dirs, np.linspace(0.01, 0.12, V))])
    depth = rng.uniform(0.02, 0.2, (V, H, W)).astype(np.float32)
    depth[rng.random((V, H, W)) < 0.1] = 0.0
    depth[:, 3, 5], depth[:, 20, 30], depth[:, 21, 30] = -0.1, np.inf, np.nan
    masks = (rng.random((V, H, W)) < 0.6).astype(np.uint8) * 255
    return depth, masks, poses


ROUGH_K4 = (40.0, 40.0, 32.0, 24.0)


@pytest.mark.parametrize("dims,V,use_masks,po", [((33, 17, 9), 3, True, 0.5), ((33, 17, 9), 2, False, 0.0), ((1, 20, 20), 2, True, 0.0),
                                                 ((2, 2, 2), 1, False, 0.5), ((5, 1, 7), 3, True, 0.0)])
def test_rough_views_equal_the_restatement_bit_for_bit(dims, V, use_masks, po):
    depth, masks, poses = _rough_views(V, seed=sum(dims) + V)
    origin, voxel, trunc = np.array([-0.001, -0.002, -0.003], np.float32), 0.004, 0.012
    masks = masks if use_masks else None
    z = (np.zeros(dims, np.float32), np.zeros(dims, np.int32))
    ra, rw = ref.integrate(*z, depth, masks, poses, ROUGH_K4, po, origin, voxel, trunc, ZNEAR)
    a, w = dev_integrate(*z, depth, masks, poses, ROUGH_K4, po, origin, voxel, trunc)
    assert same_bits(w, rw) and same_bits(a, ra)
    if min(dims) > 2:                                   # the views really reach the skips and the updates
        assert 0 < (rw > 0).sum() and (rw < V).any()
    for mw in (1, 2):
        needed, _ = assert_extract_equal(ra, rw, origin, voxel, mw)
        assert needed > 0 or mw == 2 or min(dims) < 3


@pytest.mark.parametrize("V,use_masks,po", [(1, True, 0.0), (2, False, 0.5), (3, True, 0.5), (24, True, 0.0), (24, False, 0.0)])
def test_sphere_views_equal_the_restatement_bit_for_bit(sphere, V, use_masks, po):
    s = sphere
    masks = s["masks"][:V] if use_masks else None
    z = (np.zeros(s["dims"], np.float32), np.zeros(s["dims"], np.int32))
    if (V, use_masks, po) == (24, True, 0.0):
        ra, rw = s["acc"], s["wsum"]
    else:
        ra, rw = ref.integrate(*z, s["depth"][:V], masks, s["poses"][:V], ref.K4, po, s["origin"], VOXEL, s["trunc"], ZNEAR)
    a, w = dev_integrate(*z, s["depth"][:V], masks, s["poses"][:V], ref.K4, po, s["origin"], VOXEL, s["trunc"])
    assert same_bits(w, rw) and same_bits(a, ra)
    needed, cells = assert_extract_equal(ra, rw, s["origin"], VOXEL)
    assert needed > 1000 and 0 < cells < needed


def test_more_cells_than_one_pass_of_the_block_sum_scan(sphere):
    """(66,65,65) nodes are 65 * 64 * 64 = 266 240 cells: 1 040 block sums, 16 more than the scan's first pass of 1 024 (262 144
    cells).  The field is the analytic distance to two spheres, one of them in the cells of the second pass."""
    dims = (66, 65, 65)
    assert (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1) > ref.SCAN_PASS_CELLS
    origin, voxel = np.array([0.0003, -0.0002, 0.0001], np.float32), 0.002
    g = np.stack(np.meshgrid(*[np.arange(n) for n in dims], indexing="ij"), -1) * voxel
    d = np.minimum(np.linalg.norm(g - np.array([0.05, 0.06, 0.07]), axis=-1) - 0.03,
                   np.linalg.norm(g - np.array([0.125, 0.06, 0.06]), axis=-1) - 0.012)
    wsum = np.full(dims, 2, np.int32)
    acc = (np.clip(d / 0.006, -1, 1) * 2).astype(np.float32)
    needed, _ = assert_extract_equal(acc, wsum, origin, voxel)
    _, _, _, src = ref.extract(acc, wsum, origin, voxel)
    cell_i = src[:, 0] // (65 * 65)
    assert (cell_i * 64 * 64 >= ref.SCAN_PASS_CELLS).any() and (cell_i < 40).any()      # triangles on both sides of the pass
    depth, masks, poses = _rough_views(2, seed=5)
    z = (np.zeros(dims, np.float32), np.zeros(dims, np.int32))
    ra, rw = ref.integrate(*z, depth, masks, poses, ROUGH_K4, 0.0, origin, voxel, 0.006, ZNEAR)
    a, w = dev_integrate(*z, depth, masks, poses, ROUGH_K4, 0.0, origin, voxel, 0.006)
    assert (rw > 0).any() and same_bits(w, rw) and same_bits(a, ra)


def test_constructed_volume_with_exact_zeros_and_weights_around_min_weight():
    rng = np.random.default_rng(3)
    dims, trunc = (19, 12, 21), np.float32(0.012)
    wsum = rng.integers(0, 6, dims).astype(np.int32)
    pick = rng.integers(0, 7, dims)
    wf = wsum.astype(np.float32)
    acc = np.select([pick == 0, pick == 1, pick == 2, pick == 3, pick == 4, pick == 5],
                    [np.zeros(dims, np.float32), -np.zeros(dims, np.float32), wf, -wf, trunc * wf, -trunc * wf],
                    rng.uniform(-1, 1, dims).astype(np.float32) * wf).astype(np.float32)
    origin = np.array([0.1, -0.2, 0.3], np.float32)
    for mw in (1, 3, 5):
        needed, _ = assert_extract_equal(acc, wsum, origin, 0.004, mw)
        assert needed > 0 or mw == 5
    rt, rk, _, _ = ref.extract(acc, wsum, origin, 0.004, 3)
    ref.weld(rt, rk)                                        # position is a function of key, also at the zeros
    p = rt.reshape(-1, 3, 3)
    assert ((p[:, 0] == p[:, 1]).all(1) | (p[:, 1] == p[:, 2]).all(1)).any()      # triangles without area were emitted


def test_every_sign_pattern_of_a_cell():
    """All 256 inside masks of a cell, pattern p in the cell at k = 2 p of a (2,2,512) volume (the cells between them mix two
    patterns), and the single cell of a (2,2,2) volume."""
    rng = np.random.default_rng(9)
    acc = rng.uniform(0.1, 1.0, (2, 2, 512)).astype(np.float32)
    for p in range(256):
        for c in range(8):
            if (p >> c) & 1:
                acc[c & 1, (c >> 1) & 1, 2 * p + ((c >> 2) & 1)] *= -1
    wsum = np.ones(acc.shape, np.int32)
    origin = np.array([0.01, 0.02, -0.03], np.float32)
    needed, cells = assert_extract_equal(acc, wsum, origin, 0.005)
    assert cells >= 254
    one = np.array([-0.5, 0.25, 1, -1, 0.0, 0.75, -0.125, 1], np.float32).reshape(2, 2, 2)
    assert assert_extract_equal(one, np.ones((2, 2, 2), np.int32), origin, 0.005)[1] == 1


@pytest.mark.parametrize("k", [1, 23])
def test_incremental_integration_gives_the_same_bytes_on_the_device(sphere, k):
    s = sphere
    z = (np.zeros(s["dims"], np.float32), np.zeros(s["dims"], np.int32))
    a, w = dev_integrate(*z, s["depth"][:k], s["masks"][:k], s["poses"][:k], ref.K4, 0.0, s["origin"], VOXEL, s["trunc"])
    a, w = dev_integrate(a, w, s["depth"][k:], s["masks"][k:], s["poses"][k:], ref.K4, 0.0, s["origin"], VOXEL, s["trunc"])
    assert same_bits(a, s["acc"]) and same_bits(w, s["wsum"])


def test_capacity_protocol(sphere):
    from cppf2_amd import fuse
    s = sphere
    rt, rk, rs, _ = ref.extract(s["acc"], s["wsum"], s["origin"], VOXEL)
    needed = rs[0]
    for cap in (0, needed - 1):
        t, k, st = dev_extract(s["acc"], s["wsum"], s["origin"], VOXEL, capacity=cap)
        assert st == rs and (t == CANARY_F).all() and (k == CANARY_K).all(), cap
    t, k, st = dev_extract(s["acc"], s["wsum"], s["origin"], VOXEL, capacity=needed + 3)
    assert st == rs and same_bits(t[:needed], rt.reshape(-1, 9)) and same_bits(k[:needed], rk)
    assert (t[needed:] == CANARY_F).all() and (k[needed:] == CANARY_K).all()
    vol = fuse.Volume(s["origin"], VOXEL, s["dims"], s["trunc"])
    fuse.integrate(vol, s["depth"], s["poses"], np.array([[150.0, 0, 80], [0, 150.0, 60], [0, 0, 1]]), s["masks"])
    assert same_bits(vol.acc.cpu().numpy(), s["acc"]) and same_bits(vol.wsum.cpu().numpy(), s["wsum"]) and vol.views == 24
    for cap, calls in ((16, 2), (needed, 1), (None, 1)):
        t, k, st, n = fuse.extract_triangles(vol, capacity=cap)
        assert n == calls and st == rs and same_bits(t.cpu().numpy(), rt.reshape(-1, 9)) and same_bits(k.cpu().numpy(), rk)
    mesh = fuse.extract(vol)
    rv, rf, rb = ref.weld(rt, rk)
    assert np.array_equal(mesh.verts, rv.astype(np.float64)) and np.array_equal(mesh.faces, rf) and mesh.boundary_edges == rb == 0
    raw = fuse.extract(vol, weld=False)
    assert raw.faces.shape == (needed, 3) and raw.boundary_edges is None and mesh.cells == rs[1]


def test_a_volume_without_a_sign_change_writes_nothing():
    dims = (9, 8, 7)
    for acc, wsum in ((np.ones(dims, np.float32), np.ones(dims, np.int32)), (-np.ones(dims, np.float32), np.ones(dims, np.int32)),
                      (np.zeros(dims, np.float32), np.zeros(dims, np.int32))):
        t, k, st = dev_extract(acc, wsum, np.zeros(3, np.float32), 0.01, capacity=8)
        assert st == (0, 0) and (t == CANARY_F).all() and (k == CANARY_K).all()


def test_winding_culled_render_equals_the_unculled_one(sphere):
    """For a closed, outward-wound mesh the nearest surface along every ray is a front face: culling changes no pixel."""
    import torch
    from cppf2_amd import fuse, ops, render
    s = sphere
    vol = fuse.Volume(s["origin"], VOXEL, s["dims"], s["trunc"])
    K = np.array([[150.0, 0, 80], [0, 150.0, 60], [0, 0, 1]])
    fuse.integrate(vol, s["depth"], s["poses"], K, s["masks"])
    mesh = fuse.extract(vol)
    assert mesh.boundary_edges == 0
    verts, tris = mesh.device(ops._dev())
    poses = torch.from_numpy(ref.look_at(ref.fibonacci(7)[[1, 5]], dist=0.3)).to(verts.device)
    off = ops._offsets([tris.shape[0]], verts.device)
    for P in poses:
        a = render.render_depth(verts, tris, off, P[None], K, ref.H, ref.W, cull=True)
        b = render.render_depth(verts, tris, off, P[None], K, ref.H, ref.W, cull=False)
        assert int((a > 0).sum()) > 1000 and torch.equal(a, b)
        flipped = render.render_depth(verts, tris[:, [0, 2, 1]].contiguous(), off, P[None], K, ref.H, ref.W, cull=True)
        assert not torch.equal(a, flipped)


def test_command_line_fuses_a_rendered_scene_of_the_fixture(tmp_path):
    """32 rendered views of the fixture mesh through bop_data.write_dataset (160 x 120, depth quantised to 0.1 mm) and
    python -m cppf2_amd.fuse: every welded vertex lies within trunc + sqrt(3) voxel + 0.1 mm of the original surface -- a sign
    change needs a node with a negative observation, which is at most trunc behind a surface some view saw (along the ray's z,
    no less than the true distance), and the vertex is within one tetrahedron edge (at most the cell's diagonal) of that node."""
    import json
    from cppf2_amd import bop_data, fuse, render, symmetry
    mesh = render.load_mesh(FIXTURE, 0.001)
    K = render.INTRINSICS.copy()
    K[:2] *= 0.25
    dist = 2.2 * float(np.linalg.norm(mesh.bounds[1] - mesh.bounds[0]))
    P = ref.look_at(ref.fibonacci(32), centre=np.zeros(3), dist=max(dist, 0.3)).astype(np.float64).reshape(-1, 3, 4)
    root = bop_data.write_dataset(str(tmp_path / "ds"), "train", {15: mesh}, [[[(15, p[:, :3], p[:, 3])] for p in P]], K=K, height=120,
                                  width=160, targets_file=None)
    out, rep = str(tmp_path / "obj_000015.ply"), str(tmp_path / "report.json")
    voxel = 0.003
    report = fuse.main(["--views", os.path.join(root, "train", "000000"), "--obj-id", "15", "--pixel-offset", "0.5", "--voxel", str(voxel),
                        "--report", rep, "--out", out])
    assert report["views"] == 32 and json.load(open(rep))["triangles"] == report["triangles"] > 1000
    fused = render.load_mesh(out, 0.001)
    assert fused.faces.shape[0] == report["triangles"] and fused.verts.shape[0] == report["vertices"]
    tri = mesh.verts[mesh.faces].reshape(-1, 9)
    worst = float(symmetry.deviations(fused.verts, tri, np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(1, 12))[0])
    bound = report["trunc"] + np.sqrt(3.0) * voxel + 1e-4
    print("fixture: %d vertices, %d boundary edges, farthest vertex %.2f voxel (bound %.2f)"
          % (report["vertices"], report["boundary_edges"], worst / voxel, bound / voxel))
    assert worst <= bound
