"""CPU checks of depth-frame tracking on the NumPy restatement alone (tests/track_ref.py): what the
definition of cppf_tsdf_track is able to do on analytic box scenes -- held-out views against a finished volume, an orbit of which
only the first pose is known --, the minimum-norm step on a sphere, the cases that must leave a pose's bytes alone, and
track.onboard's report with the restatement behind its two kernel calls.  The measured values stand beside each bound; the bounds
are twice what the float32 restatement gave (the runs are deterministic: the factor absorbs libm differences), capped where
DESIGN.md section 30 says so."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuse_ref as FR  # noqa: E402
import track_ref as T  # noqa: E402

from cppf2_amd import track  # noqa: E402  (the import fails without the feature)

VOXEL = T.VOXEL


def fused_box(dirs=None):
    """(acc, wsum) of the restatement's fusion of 24 Fibonacci views of the box at their true poses into the 39 x 30 x 24 volume."""
    depth, masks, poses = T.box_views(FR.fibonacci(24) if dirs is None else dirs)
    return FR.integrate(np.zeros(T.DIMS, np.float32), np.zeros(T.DIMS, np.int32), depth, masks, poses.astype(np.float32), T.K4, 0.0,
                        T.ORIGIN, VOXEL, T.TRUNC, T.ZNEAR)


@pytest.fixture(scope="module")
def box():
    acc, wsum = fused_box()
    return dict(acc=acc, wsum=wsum)


@pytest.fixture(scope="module")
def orbit():
    """The 36-frame orbit onboarded with the first pose only (no sweep), the restatement behind both kernel calls: computed once."""
    depth, masks, poses = T.box_views(T.orbit_dirs(36))
    volume, est, report = track.onboard(depth, masks, T.K3, poses[0], VOXEL, extent=0.13, sweeps=0, dev="cpu", track_fn=T.ref_track,
                                        integrate_fn=T.ref_integrate)
    return dict(depth=depth, masks=masks, poses=poses, volume=volume, est=est, report=report)


def _track(box, depth, mask, pose, iters=10, stride=1):
    return T.track(depth, mask, T.K4, 0.0, stride, pose, box["acc"], box["wsum"], T.ORIGIN, VOXEL, T.TRUNC, 1,
                   T.gates(iters, T.TRUNC, VOXEL))


def _mesh(volume):
    tris, keys, _, _ = FR.extract(volume.acc.numpy(), volume.wsum.numpy(), volume.origin, volume.voxel)
    return FR.weld(tris, keys)


HELD_OUT = (3, 9, 14, 20, 26)           # of fibonacci(29): none of them a fused direction
HELD_OUT_RMS = 0.5                      # voxel: section 30's cap; twice the largest measured (0.295) would be 0.59


def test_held_out_views_are_pulled_onto_the_volume(box):
    """(a) Five held-out views, each started 5 degrees and 10 mm off, tracked against the volume fused from 24 true poses.  The
    measure is the RMS distance of the frame's masked points, taken through the pose, to the true box (pose angles are not: a box
    seen nearly face-on leaves directions unconstrained).  Measured: 0.97-1.66 voxel before, 0.189-0.295 voxel after, 397-1 638
    inliers of 1 338-1 822 masked pixels (the view with 397 looks along a face: the free space the background carved beside the
    silhouette flattens the volume there)."""
    depth, masks, poses = T.box_views(FR.fibonacci(29)[list(HELD_OUT)])
    for i in range(len(HELD_OUT)):
        start = T.perturbed(poses[i], 5, 10, 40 + i)
        before = T.surface_rms(depth[i], masks[i], start)[0] / VOXEL
        est, st = _track(box, depth[i], masks[i], start)
        after = T.surface_rms(depth[i], masks[i], est)[0] / VOXEL
        print("view %d: %.3f -> %.3f voxel, %d inliers of %d" % (i, before, after, st[0], masks[i].sum()))
        assert before > 0.9 and after <= HELD_OUT_RMS, (i, before, after)
        assert st[0] >= 6 and st[3] == 10, st


ORBIT_RMS = 1.64                        # voxel: twice the largest tracked frame's RMS surface distance (0.820)


def test_an_orbit_with_one_known_pose_gives_a_closed_mesh_of_the_box(orbit):
    """(b) 36 frames, dirs = (cos a cos el, sin a cos el, sin el), el = 0.6 sin 2a; only frame 0's pose is given.  Measured: a
    frame at the previous frame's true pose lies up to 1.33 voxel RMS (3.61 maximum) off the box, after tracking at most 0.820
    (2.01); the extracted mesh is closed with every vertex within 1.44 voxel of the box (the same frames at true poses: 0.385;
    all at the first pose: 600 boundary edges, up to 5.04 voxel).  The condition is section 30's: closed, within 2 voxels."""
    depth, masks, poses, est = orbit["depth"], orbit["masks"], orbit["poses"], orbit["est"]
    assert np.array_equal(est[0], poses[0])
    before = max(T.surface_rms(depth[i], masks[i], poses[i - 1])[0] for i in range(1, 36)) / VOXEL
    after = max(T.surface_rms(depth[i], masks[i], est[i])[0] for i in range(36)) / VOXEL
    verts, faces, boundary = _mesh(orbit["volume"])
    far = T.box_distance(verts).max() / VOXEL
    print("orbit: %.3f -> %.3f voxel RMS; mesh %d vertices, %d boundary edges, farthest %.3f voxel" % (before, after, len(verts), boundary, far))
    assert before > 1.0 and after <= ORBIT_RMS
    assert boundary == 0 and len(faces) > 1000 and far <= 2.0


def test_fusing_the_orbit_at_its_first_pose_misses_the_condition_twice_over(orbit):
    """What (b)'s condition is worth: the same frames all integrated at frame 0's pose miss 'within 2 voxels' by a factor of 2."""
    from cppf2_amd import fuse
    v = orbit["volume"]
    vol = fuse.Volume(v.origin, v.voxel, v.dims, v.trunc, "cpu")
    T.ref_integrate(vol, orbit["depth"], np.repeat(orbit["poses"][:1], 36, 0), T.K3, orbit["masks"])
    verts, _, boundary = _mesh(vol)
    far = T.box_distance(verts).max() / VOXEL
    print("first pose for all: %d boundary edges, farthest %.3f voxel" % (boundary, far))
    assert far >= 4.0


def test_onboard_reports_lost_frames_and_the_largest_step(orbit):
    """report: per frame the four stats and lost = inlier_share < 0.5 (never frame 0, which is given); max_step = the largest
    motion of the first frame's box corners between consecutive estimates, recomputed here corner by corner.  On this orbit the
    step exceeds trunc (measured 3.2 trunc: the camera also rolls), which is what the report is there to show."""
    rep, est = orbit["report"], orbit["est"]
    assert len(rep["frames"]) == 36 and rep["sweeps"] == 0 and rep["trunc"] == T.TRUNC and rep["voxel"] == float(np.float32(VOXEL))
    assert not rep["frames"][0]["lost"] and rep["frames"][0]["inliers"] == 0
    for f in rep["frames"][1:]:
        assert f["lost"] == (f["inlier_share"] < 0.5) and f["moved"] == 10 and f["inliers"] >= 6 and f["rms"] > 0
    assert rep["lost"] == sum(f["lost"] for f in rep["frames"]) <= 2
    from cppf2_amd import fuse
    b = fuse.Volume.bounds(orbit["depth"][:1], orbit["masks"][:1], orbit["poses"][:1], T.K3, 0.0, "cpu")
    step = 0.0
    for a, c in zip(est[:-1].reshape(-1, 3, 4), est[1:].reshape(-1, 3, 4)):
        for x in (b[0, 0], b[1, 0]):
            for y in (b[0, 1], b[1, 1]):
                for z in (b[0, 2], b[1, 2]):
                    p = np.array([x, y, z])
                    step = max(step, float(np.linalg.norm((c[:, :3] @ p + c[:, 3]) - (a[:, :3] @ p + a[:, 3]))))
    assert abs(rep["max_step"] - step) <= 1e-12 and rep["max_step"] > rep["trunc"]
    # a stricter share marks more frames, nothing else changes
    strict = sum(f["inlier_share"] < 0.9 for f in rep["frames"][1:])
    assert strict > rep["lost"]


def test_a_lost_frame_is_flagged():
    """Two frames: the second one's surface lies 2 trunc in front of the first one's, outside the band that has a gradient; it
    finds no inlier, keeps the pose it was started from (frame 0's) and is reported lost."""
    depth, masks, poses = T.box_views(T.orbit_dirs(36)[:1])
    d = np.concatenate([depth, np.where(masks != 0, depth - np.float32(2 * T.TRUNC), depth)])
    _, est, rep = track.onboard(d, np.concatenate([masks, masks]), T.K3, poses[0], VOXEL, extent=0.03, sweeps=0, dev="cpu",
                                track_fn=T.ref_track, integrate_fn=T.ref_integrate)
    assert rep["frames"][1]["lost"] and rep["lost"] == 1 and rep["frames"][1]["inliers"] == 0 and rep["frames"][1]["moved"] == 0
    assert est[1].tobytes() == est[0].tobytes() == poses[0].tobytes()
    assert rep["max_step"] == 0.0


SPHERE_RMS = 0.482                      # voxel: twice the measured 0.241


def test_a_sphere_view_one_voxel_off_is_pulled_back():
    """fuse_ref's sphere volume (24 views fused) and a held-out view started one voxel off in translation.  Measured: the RMS
    distance of the frame's points to the true sphere falls from 0.556 to 0.241 voxel in 10 iterations (bound: twice that).
    The rotation does NOT stay where it was, although a sphere does not constrain it: R moves by up to 0.042 entrywise (0.08
    within the run).  The trilinear gradient of a fused volume is a noisy normal (the radial error of the fused sphere itself is
    -1.04 .. +1.78 mm at 4 mm voxels), so the rotation columns q x n do not vanish and their eigenvalues sit far above
    ICP_TAU * lambda_max = 1e-9 lambda_max: the solve keeps them.  Rotating a sphere view about the sphere's centre does not
    change its distance to the sphere, so the measure is blind to it; the minimum-norm property itself is held exactly by the
    plane below, where the normals are exact."""
    depth, masks, poses = FR.sphere_views(FR.fibonacci(24))
    origin, dims, trunc = FR.sphere_volume()
    acc, wsum = FR.fuse(depth, masks, poses, origin, dims, FR.VOXEL, trunc)
    hd, hm, hp = FR.sphere_views(FR.fibonacci(29)[[7]])
    start = hp[0].astype(np.float64)
    start[[3, 7, 11]] += np.array([0.6, -0.64, 0.48]) * FR.VOXEL            # a unit vector times one voxel
    est, st = T.track(hd[0], hm[0], FR.K4, 0.0, 1, start, acc, wsum, origin, FR.VOXEL, trunc, 1, T.gates(10, trunc, FR.VOXEL))

    def rms(pose):
        r, c = np.nonzero(hm[0])
        z = hd[0][r, c].astype(np.float64)
        p = np.stack([(c - FR.K4[2]) * z / FR.K4[0], (r - FR.K4[3]) * z / FR.K4[1], z], -1)
        P = pose.reshape(3, 4)
        return float(np.sqrt(np.mean(FR.sphere_distance((p - P[:, 3]) @ P[:, :3]) ** 2))) / FR.VOXEL
    rot = np.abs(est.reshape(3, 4)[:, :3] - start.reshape(3, 4)[:, :3]).max()
    print("sphere: %.3f -> %.3f voxel RMS, rotation moved by %.3g, stats %s" % (rms(start), rms(est), rot, st))
    assert rms(start) > 0.5 and rms(est) <= SPHERE_RMS and st[3] == 10 and st[0] == hm[0].sum()


PLANE_NORMAL = 1e-7                     # metres: float32 rounding of a 0.06 m coordinate (6e-8 / 2 per operation, a few of them)
PLANE_REST = 1e-15                      # what the unobserved directions may move: float64 rounding of values below 1


def test_minimum_norm_solve_moves_only_what_a_plane_observes():
    """A volume whose value is (x - 0.06 m) / trunc, clamped: trilinear interpolation restates it exactly and its gradient is
    exactly along x, so a face-on view of the box's +x face observes the translation along x (and the two tilts) and nothing of
    the in-plane translation and spin -- their eigenvalues are 0 or rounding, below ICP_TAU * lambda_max.  Started 4 mm off along
    the normal and 3 and 2 mm off in the plane, the pose gets its normal offset back (measured 1.4e-8 m left) and keeps the
    in-plane offsets and the rotation where they were (measured 4e-19 m and 8e-17)."""
    depth, masks, poses = T.box_views(T.orbit_dirs(36)[:1])
    x = T.ORIGIN[0] + np.arange(T.DIMS[0], dtype=np.float32) * np.float32(VOXEL)
    phi = np.clip((x - np.float32(0.06)) / np.float32(T.TRUNC), -1, 1).astype(np.float32)
    acc, wsum = np.broadcast_to(phi[:, None, None], T.DIMS).copy(), np.ones(T.DIMS, np.int32)
    true = poses[0].reshape(3, 4)
    assert np.array_equal(true[:, :3], [[0, 1, 0], [0, 0, -1], [-1, 0, 0]])      # the camera looks along -x: its z is the normal
    start = true.copy()
    start[:, 3] += [0.003, -0.002, 0.004]
    est, st = T.track(depth[0], masks[0], T.K4, 0.0, 1, start.reshape(12), acc, wsum, T.ORIGIN, VOXEL, T.TRUNC, 1,
                      T.gates(10, T.TRUNC, VOXEL))
    est = est.reshape(3, 4)
    print("plane: normal offset left %.3g m, in-plane moved %.3g m, rotation moved %.3g, stats %s"
          % (abs(est[2, 3] - true[2, 3]), np.abs(est[:2, 3] - start[:2, 3]).max(), np.abs(est[:, :3] - start[:, :3]).max(), st))
    assert st[0] == masks[0].sum() and st[3] >= 1
    assert abs(est[2, 3] - true[2, 3]) <= PLANE_NORMAL
    assert np.abs(est[:2, 3] - start[:2, 3]).max() <= PLANE_REST and np.abs(est[:, :3] - start[:, :3]).max() <= PLANE_REST


def _same_bytes(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def test_poses_that_find_too_little_keep_their_bytes(box):
    """A frame shifted by more than trunc (its surface 2 trunc in front of the volume's: value 1, no gradient), a frame without a
    reading and a frame with 5 masked pixels (5 inliers: fewer than the 6 unknowns) all come back byte for byte."""
    depth, masks, poses = T.box_views(T.orbit_dirs(36)[:1])                 # face-on: one face, no grazing side
    pose = T.perturbed(poses[0], 0.5, 0.5, 3)
    shifted = np.where(masks[0] != 0, depth[0] - np.float32(2 * T.TRUNC), depth[0])
    est, st = _track(box, shifted, masks[0], pose)
    assert _same_bytes(est, pose) and st[0] == 0 and st[2] == 0 and st[3] == 0, st
    est, st = _track(box, np.zeros_like(depth[0]), masks[0], pose)
    assert _same_bytes(est, pose) and not st.any()
    r, c = np.nonzero(masks[0])
    five = np.zeros_like(masks[0])
    pick = np.linspace(0, len(r) - 1, 9).astype(int)[2:7]
    five[r[pick], c[pick]] = 1
    est, st = _track(box, depth[0], five, pose)
    assert _same_bytes(est, pose) and st[0] == 5 and st[2] == 1 and st[3] == 0 and st[1] > 0, st
    six = five.copy()
    six[r[len(r) // 2 + 3], c[len(r) // 2 + 3]] = 1
    est, st = _track(box, depth[0], six, pose, iters=1)
    assert not _same_bytes(est, pose) and st[0] == 6 and st[3] == 1, st


def test_gates_follow_the_icp_schedule():
    import icp_ref as IR
    for iters in (1, 2, 10):
        want = np.array(IR.schedule(iters, 0.8 * T.TRUNC, VOXEL), dtype=np.float32)
        assert track.gates(iters, 0.8 * T.TRUNC, VOXEL).tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        track.gates(3, 0.0, 1.0)
