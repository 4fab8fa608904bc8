"""GPU checks of the pose search: cppf_tsdf_pose_scores held to the NumPy restatement
(tests/relocalise_ref.py) integer for integer -- every operation of the definition is a float32 one stated in order, so there is
no tolerance -- at every point count, candidate count and volume that takes another path, on the constructed placements of
tests/test_relocalise.py, through the validation; then the full search (4 416 x 729 candidates), track.join and
python -m cppf2_amd.fuse --join end to end, judged against the geometry."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuse_ref as FR  # noqa: E402
import relocalise_ref as RR  # noqa: E402
import track_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, "tests", "golden", "example_data", "obj_000015.ply")
F = np.float32
CANARY = -77
CHUNK = 256                      # RLC_CHUNK: the offsets one block serves
VOXEL = RR.VOXEL


def dev_scores(acc, wsum, origin, voxel, trunc, min_weight, points, rotations, c, m0, offsets, tau):
    """cppf_tsdf_pose_scores itself on host arrays, 64 canaries either side of the output: int32 [NR,NT,4] as the kernel left it."""
    import torch
    from cppf2_amd import _lib, ops
    dev, L = ops._dev(), _lib.load()
    a = torch.from_numpy(np.array(acc, dtype=F)).to(dev)
    w = torch.from_numpy(np.array(wsum, dtype=np.int32)).to(dev)
    p = torch.from_numpy(np.array(points, dtype=F).reshape(-1, 3)).to(dev)
    R = torch.from_numpy(np.array(rotations, dtype=np.float64).reshape(-1, 9)).to(dev)
    off = torch.from_numpy(np.array(offsets, dtype=np.int32).reshape(-1, 3)).to(dev)
    NR, NT = R.shape[0], off.shape[0]
    buf = torch.full((64 + NR * NT * 4 + 64,), CANARY, dtype=torch.int32, device=dev)
    out = buf[64:64 + NR * NT * 4]
    cc, mm = np.array(c, dtype=F), np.array(m0, dtype=F)
    _lib.check(L.cppf_tsdf_pose_scores(ops._p(a), ops._p(w), (C.c_double * 3)(*[float(v) for v in origin]), C.c_float(voxel), *a.shape,
                                       C.c_float(trunc), min_weight, ops._p(p), p.shape[0], ops._p(R) if NR else None, NR,
                                       cc.ctypes.data_as(C.c_void_p), mm.ctypes.data_as(C.c_void_p), ops._p(off) if NT else None, NT,
                                       C.c_float(tau), out.data_ptr() if NR * NT else None, ops._stream()), "cppf_tsdf_pose_scores")
    got = buf.cpu().numpy()
    assert (got[:64] == CANARY).all() and (got[-64:] == CANARY).all(), "the output's canaries"
    return got[64:-64].reshape(NR, NT, 4)


def random_rotations(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                     2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)


def random_case(rng, dims, P, NR, NT, voxel=0.004):
    """A random volume (weights 0..4, one node in ten below 3, so min_weight 1 and 3 both find known and unknown cells), points in a ball of the volume's size
    around the camera pivot, offsets of either sign that leave some cells inside and push others off every side."""
    wsum = rng.choice(5, size=dims, p=[0.03, 0.03, 0.04, 0.45, 0.45]).astype(np.int32)
    acc = (rng.uniform(-1, 1, dims) * wsum).astype(F)
    origin = np.array([-0.05, 0.02, 0.3], F)
    side = (np.array(dims) - 1) * voxel
    c = np.array([0.01, -0.02, 0.4])
    m0 = origin + side / 2 + rng.uniform(-0.3, 0.3, 3) * voxel
    pts = (c + rng.uniform(-0.6, 0.6, (P, 3)) * max(side.max(), voxel)).astype(F)
    off = rng.integers(-(max(dims) // 2) - 1, max(dims) // 2 + 2, (NT, 3)).astype(np.int32)
    off[0] = 0
    return (acc, wsum, origin, voxel, 3 * voxel), pts, random_rotations(rng, NR), c, m0, off


@pytest.fixture(scope="module")
def scene():
    """Sequence A fused by the restatement into the coarse volume (24 x 19 x 16), the three frames from below: computed once."""
    da, ma, pa = T.box_views(RR.dirs_a())
    coarse = RR.fuse_box(da, ma, pa, 2 * VOXEL, 6 * VOXEL, 0.03)
    db, mb, pb = T.box_views(RR.dirs_below())
    return dict(a=(da, ma, pa), coarse=coarse, below=(db, mb, pb))


@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 2048])
@pytest.mark.parametrize("NR,NT", [(1, 1), (2, CHUNK - 1), (5, CHUNK + 1)])
def test_counts_equal_the_restatement_at_every_size(P, NR, NT):
    """Points: one, one below, at and above a wavefront, above a block, the most; offsets: one, one below and one above a block's
    chunk; rotations 1, 2, 5; min_weight 1 and 3 on (33, 17, 9) random nodes."""
    rng = np.random.default_rng(1000 * P + NT)
    vol, pts, rot, c, m0, off = random_case(rng, (33, 17, 9), P, NR, NT)
    for mw in (1, 3):
        want = RR.pose_scores(*vol, mw, pts, rot, c, m0, off, 0.5 * vol[4])
        assert (want.sum(2) == P).all()
        if P >= 63 and NT > 1:
            assert (want[..., :3].sum((0, 1)) > 0).all() and want[..., 3].sum() > 0, "the case has every class"
        got = dev_scores(*vol, mw, pts, rot, c, m0, off, 0.5 * vol[4])
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]


@pytest.mark.parametrize("dims", [(2, 2, 2), (5, 1, 7), (33, 17, 9)])
def test_small_and_flat_volumes(dims):
    """(2, 2, 2): one cell; (5, 1, 7): an axis of one node has no cell, every point is outside under every offset."""
    rng = np.random.default_rng(sum(dims))
    vol, pts, rot, c, m0, off = random_case(rng, dims, 130, 3, 40)
    want = RR.pose_scores(*vol, 1, pts, rot, c, m0, off, 0.5 * vol[4])
    if min(dims) < 2:
        assert (want[..., 3] == 130).all()
    else:
        assert want[..., :3].sum() > 0
    assert np.array_equal(dev_scores(*vol, 1, pts, rot, c, m0, off, 0.5 * vol[4]), want)


def test_the_fused_box_under_grid_rotations_and_lattice_offsets(scene):
    """The coarse box volume (24, 19, 16), 256 points of a frame from below, 7 rotations of the 15-degree grid and the 729
    offsets of the search (negative and positive, three blocks a rotation)."""
    from cppf2_amd import relocalise as RL
    acc, wsum, origin, voxel, trunc = scene["coarse"]
    assert acc.shape == (24, 19, 16)
    db, mb, _ = scene["below"]
    pts = RR.masked_points(db[0], mb[0], 256, 0)
    rot = RL.rotation_grid(np.deg2rad(15.0))[::700]
    off = RL.offset_lattice(0.064, 2, voxel)
    c = pts.astype(np.float64).mean(0)
    m0 = np.asarray(origin, np.float64) + 0.5 * (np.array(acc.shape) - 1) * voxel
    want = RR.pose_scores(acc, wsum, origin, voxel, trunc, 1, pts, rot, c, m0, off, 0.5 * trunc)
    assert len(rot) == 7 and len(off) == 729 and want[..., :3].max((0, 1)).min() > 50 and want[..., 3].max() > 100
    assert np.array_equal(dev_scores(acc, wsum, origin, voxel, trunc, 1, pts, rot, c, m0, off, 0.5 * trunc), want)


def test_constructed_placements_bad_points_and_offsets_off_each_side():
    """tests/test_relocalise.py's constructed cases, on the device: a point on a node, in the last cell, just outside each side,
    an unknown corner, |trunc phi| == tau exactly; NaN, infinite and huge points; offsets that push a cell off each side."""
    dims = (8, 5, 4)
    acc, wsum = RR.plane_volume(dims)
    wsum[4, 2, 2] = 1
    acc[4, 2, 2] /= 2
    g, want = RR.placements(dims)
    z3 = np.zeros(3)
    vol = (acc, wsum, RR.PO, RR.PV, 3 * RR.PV)
    tau = 1.5 * RR.PV
    per_point = np.stack([dev_scores(*vol, 2, RR.at(p), RR.EYE, z3, z3, RR.ZERO, tau)[0, 0] for p in g])
    assert per_point.argmax(1).tolist() == want and per_point.sum(1).tolist() == [1] * len(g)
    assert dev_scores(*vol, 2, RR.at(g), RR.EYE, z3, z3, RR.ZERO, tau)[0, 0].tolist() == np.bincount(want, minlength=4).tolist()
    acc, wsum = RR.plane_volume(dims)
    vol = (acc, wsum, RR.PO, RR.PV, 3 * RR.PV)
    bad = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [2.0 ** 20, 1, 1], [1, -2.0 ** 20, 1], [3e38, 1, 1]])
    with np.errstate(all="ignore"):
        pts = np.concatenate([RR.at([[2.5, 1, 1]]), (RR.PO + bad * RR.PV).astype(F), RR.at([[2.0 ** 20 - 1, 1, 1]])])
    off = np.array([[0, 0, 0], [-(1 << 20) + 2, 0, 0], [0, (1 << 20) + 1, 0], [1, 1, 1], [-(1 << 20) + 3, 0, 0],
                    [2 ** 31 - 1, 0, 0], [-2 ** 31, 0, 0], [0, 0, 2 ** 31 - 1]], np.int32)
    want = RR.pose_scores(*vol, 1, pts, RR.EYE, z3, z3, off, tau)
    assert want[0, :, 0].tolist() == [1, 1, 0, 1, 1, 0, 0, 0] and want[0, :, 3].tolist() == [7, 7, 8, 7, 7, 8, 8, 8]
    assert np.array_equal(dev_scores(*vol, 1, pts, RR.EYE, z3, z3, off, tau), want)
    off = np.array([[k if a == b else 0 for b in range(3)] for a in range(3) for k in range(-3, dims[a] + 1)], np.int32)
    want = RR.pose_scores(*vol, 1, RR.at([[2.25, 1.5, 1.75]]), RR.EYE, z3, z3, off, 100.0)
    assert want[0, :, 0].sum() == (dims[0] - 1) + (dims[1] - 1) + (dims[2] - 1)
    assert np.array_equal(dev_scores(*vol, 1, RR.at([[2.25, 1.5, 1.75]]), RR.EYE, z3, z3, off, 100.0), want)


def test_validation_and_empty_calls(scene):
    """Every CPPF_EINVAL case with real device pointers: a refused call writes nothing; NR = 0 and NT = 0 write nothing."""
    import torch
    from cppf2_amd import _lib, ops
    dev, L = ops._dev(), _lib.load()
    acc, wsum, origin, voxel, trunc = scene["coarse"]
    a, w = torch.from_numpy(acc).to(dev), torch.from_numpy(wsum).to(dev)
    p = torch.zeros((4, 3), dtype=torch.float32, device=dev)
    R = torch.from_numpy(np.tile(np.eye(3).reshape(1, 9), (2, 1))).to(dev)
    off = torch.zeros((3, 3), dtype=torch.int32, device=dev)
    out = torch.full((2, 3, 4), CANARY, dtype=torch.int32, device=dev)
    o3, f3 = (C.c_double * 3)(*[float(v) for v in origin]), (C.c_float * 3)(0, 0, 0.4)
    base = dict(acc=ops._p(a), wsum=ops._p(w), origin=o3, voxel=voxel, dims=acc.shape, trunc=trunc, mw=1, pts=ops._p(p), P=4, rot=ops._p(R),
                NR=2, c=f3, m=f3, off=ops._p(off), NT=3, tau=0.5 * trunc, out=ops._p(out))

    def call(**kw):
        k = dict(base, **kw)
        return L.cppf_tsdf_pose_scores(k["acc"], k["wsum"], k["origin"], C.c_float(k["voxel"]), *k["dims"], C.c_float(k["trunc"]), k["mw"],
                                       k["pts"], k["P"], k["rot"], k["NR"], k["c"], k["m"], k["off"], k["NT"], C.c_float(k["tau"]),
                                       k["out"], ops._stream())
    nan, inf = float("nan"), float("inf")
    cases = [dict(acc=None), dict(wsum=None), dict(origin=None), dict(pts=None), dict(rot=None), dict(c=None), dict(m=None),
             dict(off=None), dict(out=None), dict(P=0), dict(P=2049), dict(P=-1), dict(NR=-1), dict(NT=-1),
             dict(NR=1 << 15, NT=(1 << 14) + 1), dict(dims=(0, 4, 4)), dict(dims=(4, 4, -1)), dict(dims=(1 << 14, 1 << 14, 1)),
             dict(dims=(1024, 1024, 129)), dict(voxel=0.0), dict(voxel=nan), dict(voxel=inf), dict(trunc=0.0), dict(trunc=-1.0),
             dict(trunc=inf), dict(tau=0.0), dict(tau=-0.1), dict(tau=nan), dict(tau=inf), dict(mw=0),
             dict(origin=(C.c_double * 3)(0, nan, 0)), dict(c=(C.c_float * 3)(inf, 0, 0)), dict(m=(C.c_float * 3)(0, 0, nan))]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert b"invalid argument" in L.cppf_last_error_string()
    assert call(NR=0) == 0 and call(NT=0) == 0 and call(NR=0, NT=0, rot=None, off=None, out=None) == 0
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()), "a refused or empty call wrote something"
    assert dev_scores(acc, wsum, origin, voxel, trunc, 1, np.zeros((4, 3)), np.zeros((0, 9)), [0, 0, 0.4], [0, 0, 0.4], np.zeros((3, 3)), 0.01).shape == (0, 3, 4)
    assert dev_scores(acc, wsum, origin, voxel, trunc, 1, np.zeros((4, 3)), np.eye(3).reshape(1, 9), [0, 0, 0.4], [0, 0, 0.4], np.zeros((0, 3)), 0.01).shape == (1, 0, 4)
    assert call() == 0                                      # and the same arguments, untouched, are a valid call
    torch.cuda.synchronize()
    assert bool((out.sum(2) == 4).all())


def test_wrapper_equals_the_entry_point(scene):
    import torch
    from cppf2_amd import fuse, relocalise as RL
    acc, wsum, origin, voxel, trunc = scene["coarse"]
    vol = fuse.Volume(origin, voxel, acc.shape, trunc)
    vol.acc.copy_(torch.from_numpy(acc))
    vol.wsum.copy_(torch.from_numpy(wsum))
    db, mb, _ = scene["below"]
    pts = RR.masked_points(db[1], mb[1], 100, 3)
    rot, off = RL.rotation_grid(np.deg2rad(60.0)), RL.offset_lattice(0.05, 3, voxel)
    c, m0 = pts.mean(0), np.array([0.001, -0.002, 0.003])
    got = RL.pose_scores(vol, pts, rot, off, c, m0, 0.4 * trunc)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(rot), len(off), 4)
    assert np.array_equal(got.cpu().numpy(), dev_scores(acc, wsum, origin, voxel, trunc, 1, pts, rot, c, m0, off, 0.4 * trunc))
    with pytest.raises(ValueError):
        RL.pose_scores(vol, np.zeros((2049, 3), F), rot, off, c, m0, 0.01)
    with pytest.raises(ValueError):
        RL.pose_scores(vol, pts, rot, off, c, m0, 0.0)


def device_volumes(da, ma, pa):
    from cppf2_amd import fuse
    vols = []
    for k in (2, 1):
        v = fuse.Volume.around(da, ma, pa, T.K3, k * VOXEL, None, 3 * k * VOXEL)
        fuse.integrate(v, da, pa, T.K3, ma)
        vols.append(v)
    return vols


# The full search's cap is section 30's for a refined frame: 0.5 (fine) voxel RMS of the frame's masked points to the box.  The
# issue's CPU prototype measured 0.058, 0.065 and 0.088 voxel for the three frames; the device's values are printed by the test
# and recorded in DESIGN.md section 32.
RELOCALISE_RMS = 0.5


def test_the_full_search_finds_three_frames_from_below(scene):
    """4 416 rotations x 729 offsets x 256 points per frame on the device, the top 32 refined on the coarse and the fine volume:
    each kept pose is judged by the geometry (track_ref.surface_rms against the true box), not by the code under test."""
    from cppf2_amd import relocalise as RL
    vols = device_volumes(*scene["a"])
    db, mb, pb = scene["below"]
    for i in range(3):
        pose, rep = RL.relocalise(vols, db[i], T.K3, mb[i], reach=0.064)
        assert (rep["rotations"], rep["offsets"], rep["points"], rep["step_nodes"]) == (4416, 729, 256, 2)
        rms = T.surface_rms(db[i], mb[i], pose)[0] / VOXEL
        print("relocalise frame %d: %.3f voxel RMS (cap %.1f), coarse rank %d, score %s, inliers %d (runner-up %d), search %.3f s, refine %.3f s"
              % (i, rms, RELOCALISE_RMS, rep["rank"], rep["score"], rep["inliers"], rep["runner_up"], rep["seconds"]["search"],
                 rep["seconds"]["refine"]))
        assert rms <= RELOCALISE_RMS, (i, rms)
        assert sum(rep["score"]) == 256 and 0 <= rep["rank"] < 32 and rep["inliers"] >= rep["runner_up"]


# Measured once on the restatement (fuse_ref: sequence A and sequence B fused at their TRUE poses into Volume.around A at 4 mm,
# 40 x 30 x 24 nodes): the bottom face's lattice lies within 0.956 voxel of the mesh's vertices (0 boundary edges, farthest vertex
# 0.549 voxel); for A alone the largest distance is 8.09 voxel (192 boundary edges): no surface is there.
TRUE_POSE_GAP = 0.956
JOIN_RMS = 0.5                   # section 30's cap; the CPU prototype: 0.395
JOIN_FAR = 2.0                   # section 30 (b); the CPU prototype: 1.59


JOIN_TOP = 128                   # 4 x the default: the first candidate of a member that keeps the bottom down has coarse rank 50


@pytest.fixture(scope="module")
def joined():
    """track.join on the prototype's two sequences, no sweep, and sequence A alone: computed once.  The box has the symmetry group
    of its three half turns, and the two members that lay the second sequence's unseen face onto the top face, which the first
    sequence saw, fit with every point (about 1 390 inliers of 1 419 readings against about 800 for the two that keep it down:
    the default keeps one of those, every frame tracks in it within 0.293 voxel RMS and the bottom stays open, 182 boundary
    edges, gap 8.114 voxel).  So the call says what its user knows, turned_over=True, and refines JOIN_TOP candidates."""
    from cppf2_amd import fuse, track
    da, ma, pa = T.box_views(RR.dirs_a())
    db, mb, pb = T.box_views(RR.dirs_b())
    alone = fuse.Volume.around(da, ma, pa, T.K3, VOXEL)
    fuse.integrate(alone, da, pa, T.K3, ma)
    vol, poses, rep = track.join(dict(depths=da, masks=ma, K=T.K3, poses=pa), dict(depths=db, masks=mb, K=T.K3), VOXEL, reach=0.064,
                                 top=JOIN_TOP, turned_over=True)
    assert vol.dims == alone.dims == (40, 30, 24) and rep["coarse_dims"] == [25, 20, 17] and poses.shape == (36, 12) and vol.views == 56
    return dict(b=(db, mb, pb), poses=poses, report=rep, mesh=fuse.extract(vol), mesh_a=fuse.extract(alone))


def test_join_tracks_the_sequence_from_below(joined):
    """Every frame of the second sequence within 0.5 voxel RMS of the box (measured 0.460; frame 0, found by the search, 0.459:
    only the side faces hold it, the face it brings has nothing to lie on yet), every vertex of the joined mesh within 2 voxels
    (measured 0.593).  Boundary edges are recorded, not asserted: 0, against 192 for A alone (the CPU prototype: 178)."""
    db, mb, _ = joined["b"]
    rep, mesh, mesh_a = joined["report"], joined["mesh"], joined["mesh_a"]
    rms = [T.surface_rms(db[i], mb[i], joined["poses"][i])[0] / VOXEL for i in range(36)]
    far = T.box_distance(mesh.verts).max() / VOXEL
    r = rep["relocalise"]
    print("join: frame 0 %.3f voxel RMS (coarse rank %d, %d inliers, %d admitted, %d contradicted, %d unseen), largest frame RMS %.3f "
          "voxel, farthest vertex %.3f voxel, boundary edges %d (A alone %d), lost %d, max_step %.2f trunc"
          % (rms[0], r["rank"], r["inliers"], r["admitted"], r["contradicted"], r["unseen"], max(rms), far, mesh.boundary_edges,
             mesh_a.boundary_edges, rep["lost"], rep["max_step"] / rep["trunc"]))
    assert max(rms) <= JOIN_RMS
    assert far <= JOIN_FAR
    assert rep["lost"] == 0 and len(rep["frames"]) == 36 and r["offsets"] == 729 and r["turned_over"] and r["unseen"] > 0


def test_join_brings_the_bottom_face(joined):
    """The largest distance from a 4 mm lattice on the face z = -30 mm to the nearest mesh vertex: above 3 voxels for A alone (no
    surface is there: 8.094), within twice the true-pose fusion's 0.956 for the join (measured 1.098)."""
    gap_a, gap = RR.bottom_gap(joined["mesh_a"].verts) / VOXEL, RR.bottom_gap(joined["mesh"].verts) / VOXEL
    print("join: bottom gap %.3f voxel (A alone %.3f, true poses %.3f)" % (gap, gap_a, TRUE_POSE_GAP))
    assert gap_a > 3.0
    assert gap <= 2 * TRUE_POSE_GAP


def coverage(verts, of):
    """The largest distance from the points `of` to the nearest of verts, metres (on the device, in chunks)."""
    import torch
    v = torch.from_numpy(np.asarray(verts, dtype=np.float32)).cuda()
    q = torch.from_numpy(np.asarray(of, dtype=np.float32)).cuda()
    return max(float(torch.cdist(q[i:i + 1024], v).min(1).values.max()) for i in range(0, len(q), 1024))


def test_command_line_joins_rendered_views_from_below(tmp_path):
    """Rendered views of the fixture mesh (160 x 120, depth quantised to 0.1 mm, pixel_offset 0.5, voxel 3 mm): an upper-hemisphere
    set with its poses, and a lower-hemisphere orbit with EVERY pose removed from scene_gt.json, through
    python -m cppf2_amd.fuse --views A --join B: every welded vertex lies within section 28's bound (trunc + sqrt(3) voxel +
    0.1 mm) plus the second folder's largest reported RMS of the original surface, as the --track test derives it, and the
    underside, which the first folder alone leaves open, is covered as the true-pose fusion of the same images covers it.
    Measured: 29 274 vertices, boundary edges 1 168 -> 0, farthest vertex 1.10 voxel (bound 5.19, of which RMS 0.42), 1 of 96
    frames reported lost; the original's vertices within 2.61 voxel of the fused ones (A alone 10.49, true poses 1.99)."""
    from cppf2_amd import bop_data, fuse, render, symmetry
    mesh = render.load_mesh(FIXTURE, 0.001)
    K = render.INTRINSICS.copy()
    K[:2] *= 0.25
    dist = max(2.2 * float(np.linalg.norm(mesh.bounds[1] - mesh.bounds[0])), 0.3)
    up = FR.fibonacci(48)
    up = up[up[:, 2] > 0.15]
    n = 96
    a = 2 * np.pi * np.arange(n) / n
    el = -0.55 + 0.3 * np.sin(2 * a)
    down = np.stack([np.cos(a) * np.cos(el), np.sin(a) * np.cos(el), np.sin(el)], 1)
    scenes = []
    for name, dirs in (("a", up), ("b", down)):
        P = FR.look_at(dirs, centre=np.zeros(3), dist=dist).astype(np.float64).reshape(-1, 3, 4)
        root = bop_data.write_dataset(str(tmp_path / name), "train", {15: mesh}, [[[(15, p[:, :3], p[:, 3])] for p in P]], K=K, height=120,
                                      width=160, targets_file=None)
        scenes.append(os.path.join(root, "train", "000000"))
    gt_path = os.path.join(scenes[1], "scene_gt.json")
    gt = json.load(open(gt_path))
    for entries in gt.values():
        for e in entries:
            del e["cam_R_m2c"], e["cam_t_m2c"]
    out, rep = str(tmp_path / "obj_000015.ply"), str(tmp_path / "report.json")
    voxel = 0.003
    args = ["--views", scenes[0], "--obj-id", "15", "--pixel-offset", "0.5", "--voxel", str(voxel), "--report", rep, "--out", out]
    views = [fuse.read_views(s, 15)[0] for s in scenes]           # read before the second folder loses its poses
    json.dump(gt, open(gt_path, "w"))
    plain = fuse.main(args)
    assert "join" not in plain and plain["views"] == len(up)
    cover_a = coverage(render.load_mesh(out, 0.001).verts, mesh.verts)
    true = fuse.Volume.around(views[0]["depths"], views[0]["masks"], views[0]["poses"], views[0]["K"], voxel, pixel_offset=0.5)
    for b in views:
        fuse.integrate(true, b["depths"], b["poses"], b["K"], b["masks"], 0.5)
    cover_true = coverage(fuse.extract(true).verts, mesh.verts)
    report = fuse.main(args + ["--join", scenes[1]])
    jn = report["join"]
    assert report["views"] == len(up) + n and json.load(open(rep))["join"]["max_step"] == jn["max_step"]
    assert [f["recorded"] for f in jn["frames"]] == [None] * n and jn["relocalise"]["rotations"] == 4416
    fused = render.load_mesh(out, 0.001)
    assert fused.faces.shape[0] == report["triangles"] > 1000
    tri = mesh.verts[mesh.faces].reshape(-1, 9)
    worst = float(symmetry.deviations(fused.verts, tri, np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(1, 12))[0])
    rms = max(f["rms"] for f in jn["frames"])
    bound = report["trunc"] + np.sqrt(3.0) * voxel + 1e-4 + rms
    print("fixture, joined: %d vertices, %d boundary edges (A alone %d), farthest vertex %.2f voxel (bound %.2f, of which RMS %.2f); "
          "lost %d; coarse rank %d; search %.3f s"
          % (report["vertices"], report["boundary_edges"], plain["boundary_edges"], worst / voxel, bound / voxel, rms / voxel, jn["lost"],
             jn["relocalise"]["rank"], jn["relocalise"]["seconds"]["search"]))
    assert worst <= bound
    # the underside is there: the original's vertices as far from the fused mesh's as the true-pose fusion of the same images
    # leaves them, times two (the bottom-face condition of the box scene, on an object without the box's symmetry)
    cover = coverage(fused.verts, mesh.verts)
    print("fixture, joined: original vertices within %.2f voxel of the fused ones (A alone %.2f, true poses %.2f)"
          % (cover / voxel, cover_a / voxel, cover_true / voxel))
    assert cover_a > 3 * voxel
    assert cover <= 2 * cover_true
    # the same with --join-turned-over: this object has no symmetry, so nothing else fits and the same bound holds
    turned = fuse.main(args + ["--join", scenes[1], "--join-turned-over", "--join-top", "128"])
    tr = turned["join"]["relocalise"]
    fused = render.load_mesh(out, 0.001)
    worst = float(symmetry.deviations(fused.verts, tri, np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(1, 12))[0])
    bound = turned["trunc"] + np.sqrt(3.0) * voxel + 1e-4 + max(f["rms"] for f in turned["join"]["frames"])
    print("fixture, joined, turned over: %d boundary edges, farthest vertex %.2f voxel (bound %.2f); coarse rank %d, admitted %d, "
          "contradicted %d, unseen %d" % (turned["boundary_edges"], worst / voxel, bound / voxel, tr["rank"], tr["admitted"],
                                         tr["contradicted"], tr["unseen"]))
    assert tr["turned_over"] and worst <= bound
