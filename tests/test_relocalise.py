"""CPU checks of the pose search: the NumPy restatement of cppf_tsdf_pose_scores (tests/relocalise_ref.py)
on constructed volumes whose points sit at the definition's edges, the host side of cppf2_amd.relocalise (the rotation grid, the
offset lattice, the candidate's pose, the argument checks), the entry point's validation (which touches no device), and that
the score ranks the candidate nearest the truth first on the box scene."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import relocalise_ref as RR  # noqa: E402
import track_ref as T  # noqa: E402
from cppf2_amd import relocalise as RL  # noqa: E402  (fails without the feature)

F = np.float32
PV, PO, EYE, ZERO = RR.PV, RR.PO, RR.EYE, RR.ZERO
plane_volume, at, scores, placements = RR.plane_volume, RR.at, RR.scores, RR.placements


def test_the_four_counts_sum_to_the_points_and_the_placements_are_exact():
    dims = (8, 5, 4)
    acc, wsum = plane_volume(dims)
    wsum[4, 2, 2] = 1
    acc[4, 2, 2] /= 2
    g, want = placements(dims)
    per_point = np.stack([scores(acc, wsum, p, min_weight=2)[0, 0] for p in g])
    assert per_point.sum(1).tolist() == [1] * len(g)
    assert per_point.argmax(1).tolist() == want
    both = scores(acc, wsum, g, min_weight=2)[0, 0]
    assert both.tolist() == np.bincount(want, minlength=4).tolist() and both.sum() == len(g)
    assert scores(acc, wsum, g, min_weight=1)[0, 0, 2] == 0          # with min_weight 1 every node is known


def test_points_that_are_not_finite_or_huge_are_outside_for_every_offset():
    acc, wsum = plane_volume((8, 5, 4))
    bad = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [2.0 ** 20, 1, 1], [1, -2.0 ** 20, 1], [3e38, 1, 1]])
    pts = np.concatenate([at([[2.5, 1, 1]]), (PO + bad * PV).astype(F)])
    pts[5, 1] = F(PO[1] - 2.0 ** 20 * PV)
    off = np.array([[0, 0, 0], [-(1 << 20) + 2, 0, 0], [0, (1 << 20) + 1, 0], [1, 1, 1]], np.int32)
    s = RR.pose_scores(acc, wsum, PO, PV, 3 * PV, 1, pts, EYE, np.zeros(3), np.zeros(3), off, 1.5 * PV)
    assert s[0, :, 3].tolist() == [6, 7, 7, 6] and s[0, :, 0].tolist() == [1, 0, 0, 1] and s.sum(2).tolist() == [[7] * 4]
    just = (PO + np.array([[2.0 ** 20 - 1, 1, 1]]) * PV).astype(F)           # |g| < 2^20: a cell, and an offset can bring it back
    s = RR.pose_scores(acc, wsum, PO, PV, 3 * PV, 1, just, EYE, np.zeros(3), np.zeros(3), [[-(1 << 20) + 3, 0, 0]], 1.5 * PV)
    assert s[0, 0].tolist() == [1, 0, 0, 0]


def test_offsets_push_a_cell_off_each_side():
    dims = (8, 5, 4)
    acc, wsum = plane_volume(dims)
    off, want = [], []
    for a in range(3):
        for k in range(-3, dims[a] + 1):
            o = [0, 0, 0]
            o[a] = k
            off.append(o)
            want.append(0 <= [2, 1, 1][a] + k <= dims[a] - 2)
    s = scores(acc, wsum, [[2.25, 1.5, 1.75]], np.array(off, np.int32), tau=100.0)
    assert (s[0, :, 0] == 1).tolist() == want and (s[0, :, 3] == 1).tolist() == [not w for w in want]


def test_an_axis_of_one_node_has_no_cell():
    acc, wsum = plane_volume((5, 1, 7))
    s = scores(acc, wsum, [[1.5, 0.0, 2.5], [0.0, 0.0, 0.0]], np.array([[0, 0, 0], [0, -1, 0], [1, 1, 1]], np.int32))
    assert s[0, :, 3].tolist() == [2, 2, 2]


def test_candidate_pose_maps_the_model_pivot_to_the_camera_pivot():
    rot = RL.rotation_grid(np.deg2rad(40.0))
    off = RL.offset_lattice(0.05, 2, 0.008)
    c, m0 = np.array([0.01, -0.02, 0.4]), np.array([0.003, 0.001, -0.002])
    for r, j in ((0, 0), (5, 17), (len(rot) - 1, len(off) - 1)):
        P = RL.candidate_pose(rot, off, r, j, c, m0, 0.008).reshape(3, 4)
        m = m0.astype(F).astype(np.float64) + off[j] * float(F(0.008))
        assert np.abs(P[:, :3] @ m + P[:, 3] - c.astype(F)).max() <= 1e-15
        assert P[:, :3].tobytes() == rot[r].tobytes()


def test_rotation_grid_and_offset_lattice():
    for step, n in ((np.deg2rad(15.0), 184 * 24), (np.deg2rad(40.0), 26 * 9), (np.pi, 2 * 2)):
        rot = RL.rotation_grid(step)
        assert rot.shape == (n, 3, 3) and rot.dtype == np.float64
        assert np.abs(rot - RR.rotation_grid(step)).max() <= 1e-15
        assert np.abs(np.einsum("nij,nkj->nik", rot, rot) - np.eye(3)).max() <= 1e-14 and np.abs(np.linalg.det(rot) - 1).max() <= 1e-14
    rot = RL.rotation_grid(np.deg2rad(15.0))
    assert rot.tobytes() == RL.rotation_grid(np.deg2rad(15.0)).tobytes()
    # every rotation has a grid neighbour within 1.5 steps: nearest other member, by the angle of R_a^T R_b
    tr = np.einsum("aij,bij->ab", rot[::97], rot)
    ang = np.degrees(np.arccos(np.clip((tr - 1) / 2, -1, 1)))
    ang[ang < 1e-3] = 180.0
    assert ang.min(1).max() <= 22.5
    off = RL.offset_lattice(0.064, 2, 0.008)
    assert off.shape == (729, 3) and off.dtype == np.int32 and off.min() == -8 and off.max() == 8 and set(np.unique(off)) == set(range(-8, 9, 2))
    assert off[0].tolist() == [-8, -8, -8] and off[1].tolist() == [-8, -8, -6] and off[364].tolist() == [0, 0, 0]
    assert RL.offset_lattice(0.0, 1, 0.004).tolist() == [[0, 0, 0]]


def test_arguments_are_refused_loudly():
    from cppf2_amd import fuse
    for bad in (0.0, -1.0, 4.0, float("nan")):
        with pytest.raises(ValueError):
            RL.rotation_grid(bad)
    for bad in ((-1.0, 1, 0.004), (0.1, 0, 0.004), (0.1, 1, 0.0), (float("inf"), 1, 0.004)):
        with pytest.raises(ValueError):
            RL.offset_lattice(*bad)
    with pytest.raises(ValueError):
        RL.candidate_pose(EYE, ZERO, 0, 0, [0, 0], [0, 0, 0], 0.004)
    vol = fuse.Volume(np.zeros(3), 0.004, (4, 4, 4), dev="cpu")
    depth = np.ones((4, 5), F)
    mask = np.zeros((4, 5), np.uint8)
    mask[0, :5] = 1
    with pytest.raises(ValueError, match="5 readings"):
        RL.relocalise([vol], depth, T.K3, mask, score_fn=RR.ref_scores, track_fn=T.ref_track)
    depth[0, 0] = np.nan
    mask[1, 0] = 1
    with pytest.raises(ValueError, match="5 readings"):
        RL.relocalise(vol, depth, T.K3, mask, score_fn=RR.ref_scores, track_fn=T.ref_track)
    for kw in (dict(top=0), dict(points=0), dict(points=2049)):
        with pytest.raises(ValueError):
            RL.relocalise([vol], depth, T.K3, None, score_fn=RR.ref_scores, track_fn=T.ref_track, **kw)
    with pytest.raises(ValueError):
        RL.relocalise([], depth, T.K3, None)
    with pytest.raises(RL.CppfError):
        RL.pose_scores(vol, np.zeros((3, 3), F), EYE, ZERO, np.zeros(3), np.zeros(3), 0.01)          # no CPU fallback


def test_the_entry_point_validates_before_any_device_work():
    from cppf2_amd import _lib
    L = _lib.load()
    o3 = (C.c_double * 3)(0, 0, 0)
    f3 = (C.c_float * 3)(0, 0, 0)
    one = C.c_void_p(8)                    # a non-null pointer the refused calls never follow
    base = dict(acc=one, wsum=one, origin=o3, voxel=0.004, dims=(4, 4, 4), trunc=0.012, mw=1, pts=one, P=4, rot=one, NR=2, c=f3, m=f3,
                off=one, NT=3, tau=0.006, out=one)

    def call(**kw):
        a = dict(base, **kw)
        return L.cppf_tsdf_pose_scores(a["acc"], a["wsum"], a["origin"], C.c_float(a["voxel"]), *a["dims"], C.c_float(a["trunc"]), a["mw"],
                                       a["pts"], a["P"], a["rot"], a["NR"], a["c"], a["m"], a["off"], a["NT"], C.c_float(a["tau"]),
                                       a["out"], None)
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
    # no candidates: a valid call that launches nothing (and needs none of the three arrays)
    assert call(NR=0, rot=None, off=None, out=None) == 0 and call(NT=0, rot=None, off=None, out=None) == 0
    assert call(NR=1 << 15, NT=1 << 14, P=0) == -1


def test_the_candidate_nearest_the_truth_ranks_first():
    """The box fused from sequence A into the coarse volume (24 x 19 x 16 nodes of 8 mm, trunc 24 mm); a frame from below; the
    24 axis permutations composed with the true rotation times 27 offsets of 2 nodes: 648 candidates.  The box's own symmetries
    (4 of the 24: the half turns about its axes) are poses as true as the identity -- the frame shows the face A never saw, and a
    half turn lays it on the face A did see, so such a member can even score higher --, so the truth is the group: the top
    score belongs to one of its members at the offset nearest the truth under that member, and nothing outside the group
    reaches it.  The winner's pose puts the frame's points within sqrt(3) coarse voxels RMS of the box (the lattice's own
    spacing: 2 nodes per axis, so at most 1 node off per axis)."""
    da, ma, pa = T.box_views(RR.dirs_a())
    acc, wsum, origin, voxel, trunc = RR.fuse_box(da, ma, pa, 2 * RR.VOXEL, 6 * RR.VOXEL, 0.03)
    assert acc.shape == (24, 19, 16) and len(da) == 20
    db, mb, pb = T.box_views(RR.dirs_below()[:1])
    pts = RR.masked_points(db[0], mb[0], 256, 0)
    Rt, tt = pb[0].reshape(3, 4)[:, :3], pb[0].reshape(3, 4)[:, 3]
    perms = []
    for p in itertools.permutations(range(3)):
        for s in itertools.product((1.0, -1.0), repeat=3):
            Q = np.zeros((3, 3))
            Q[range(3), p] = s
            if np.linalg.det(Q) > 0:
                perms.append(Q)
    assert len(perms) == 24
    rot = np.stack([Rt @ Q for Q in perms])
    off = RL.offset_lattice(2 * voxel, 2, voxel)
    assert len(off) == 27
    c = pts.astype(np.float64).mean(0)
    m0 = np.asarray(origin, np.float64) + 0.5 * (np.array(acc.shape) - 1) * voxel
    s = RR.pose_scores(acc, wsum, origin, voxel, trunc, 1, pts, rot, c, m0, off, 0.5 * trunc)
    assert (s.sum(2) == len(pts)).all()
    value = (s[..., 0] - s[..., 1]).astype(np.int64)
    sym = [k for k, Q in enumerate(perms) if np.array_equal(np.abs(Q), np.eye(3))]
    assert len(sym) == 4 and np.array_equal(perms[sym[0]], np.eye(3))
    # the offset nearest the truth under member k of the group: (R_t Q_k)^T (c - t) = m0 + off * voxel
    near = {}
    for k in sym:
        want = (rot[k].T @ (c - tt) - m0) / voxel
        near[k] = int(np.argmin(np.abs(off - want).max(1)))
        assert np.abs(off[near[k]] - want).max() <= 1.0
    r, j = (int(x) for x in np.unravel_index(int(np.argmax(value)), value.shape))
    print("ranking: top %d at rotation %d offset %s; the group's members at their nearest offsets %s; best outside the group %d"
          % (value.max(), r, off[j].tolist(), [int(value[k, near[k]]) for k in sym], np.delete(value, sym, 0).max()))
    assert r in sym and j == near[r]
    assert np.delete(value, sym, 0).max() < value.max()
    pose = RL.candidate_pose(rot, off, r, j, c, m0, voxel)
    assert T.surface_rms(db[0], mb[0], pose)[0] <= np.sqrt(3.0) * voxel


@pytest.mark.parametrize("extra", [["--join-top", "0"], ["--join-coarse", "0"], ["--join-points", "0"], ["--join-points", "2049"],
                                   ["--join-step-deg", "0"], ["--join-step-deg", "181"]])
def test_command_line_refuses_bad_join_arguments(extra, tmp_path, capsys):
    from cppf2_amd import fuse
    with pytest.raises(SystemExit):
        fuse.main(["--views", str(tmp_path), "--join", str(tmp_path), "--voxel", "0.004", "--out", str(tmp_path / "o.ply")] + extra)
    assert "--join" in capsys.readouterr().err
    with pytest.raises(fuse.ViewsError):                    # and valid arguments reach the folders
        fuse.main(["--views", str(tmp_path), "--join", str(tmp_path), "--voxel", "0.004", "--out", str(tmp_path / "o.ply")])
