"""The pose of a depth frame against a signed distance volume with NO starting pose: what relates the
first frame of a second sequence -- the object turned over, BOP's model-free static onboarding -- to the volume of the first,
and what finds a frame again that track.track lost (its capture range is trunc).  An exhaustive search: every rotation of a grid
times every whole-node translation of a lattice is scored by where a few hundred of the frame's points fall in a coarse volume
(one launch of cppf_tsdf_pose_scores), and the best candidates are refined by track.track, coarse to fine.  The reference has no
such step.

    rotations = rotation_grid(np.deg2rad(15))                        # float64 [4416,3,3]
    offsets = offset_lattice(0.064, 2, coarse.voxel)                 # int32 [729,3]
    scores = pose_scores(coarse, points, rotations, offsets, c, m0, tau=0.5 * coarse.trunc)      # int32 [NR,NT,4], device
    pose, report = relocalise([coarse, fine], depth, K, mask)
    volume, poses_b, report = track.join(first, second, voxel=0.004)
    python -m cppf2_amd.fuse --views A --join B --voxel 0.004 --out obj.ply

The kernel is cppf_tsdf_pose_scores (include/cppf_hip_experimental.h; the definition is stated in
cppf2_amd/csrc/cppf_relocalise.hip and restated in tests/relocalise_ref.py).  Not done: no pyramid beyond the volumes given, no
use of the two sequences' support planes, no detection of symmetries: any member of a symmetric object's group is accepted
unless turned_over=True says that the frame shows what the volume has not seen.
"""
from __future__ import annotations

import ctypes as C
import math
import time

import numpy as np
import torch

from . import _lib, fuse, hostargs, ops
from ._lib import CppfError

MAX_POINTS = 2048                # points per cppf_tsdf_pose_scores call
MAX_CANDIDATES = 1 << 29         # NR * NT
MIN_READINGS = 6                 # a frame with fewer masked readings has no pose (track's own minimum)


def _count(x):
    """ceil(x) of a quotient that may exceed a whole number by rounding alone (2 pi / 15 degrees is 24.000000000000004)."""
    return int(math.ceil(x - 1e-9))


def rotation_grid(step):
    """float64 [NR,3,3], model -> camera, deterministic: nd = ceil(4 pi / step^2) directions d_i times nr = ceil(2 pi / step)
    rolls (both ceilings taken of the quotient less 1e-9), direction-major.  d_i is the Fibonacci direction z = 1 - (2 i + 1) / nd,
    s = sqrt(1 - z^2), a = i pi (3 - sqrt 5), d = (s cos a, s sin a, z): the image of the model's z axis.  With h = (1, 0, 0) if
    |d.z| > 0.9 else (0, 0, 1), u = h x d normalised and B = [u, d x u, d] as columns, rotation i * nr + k is
    B Rz(2 pi k / nr), Rz(b) = [[cos b, -sin b, 0], [sin b, cos b, 0], [0, 0, 1]].  step: radians between neighbours."""
    step = float(step)
    if not (0 < step <= math.pi):
        raise ValueError("relocalise.rotation_grid: step is an angle in (0, pi] radians, not %r" % step)
    nd, nr = _count(4 * math.pi / step ** 2), _count(2 * math.pi / step)
    i = np.arange(nd, dtype=np.float64)
    z = 1.0 - (2 * i + 1) / nd
    s = np.sqrt(1.0 - z * z)
    a = i * np.pi * (3.0 - np.sqrt(5.0))
    d = np.stack([s * np.cos(a), s * np.sin(a), z], 1)
    h = np.where((np.abs(d[:, 2]) > 0.9)[:, None], np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]))
    u = np.cross(h, d)
    u /= np.linalg.norm(u, axis=1)[:, None]
    B = np.stack([u, np.cross(d, u), d], 2)
    b = 2 * np.pi * np.arange(nr) / nr
    Rz = np.zeros((nr, 3, 3))
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = np.cos(b), -np.sin(b), np.sin(b), np.cos(b), 1.0
    return np.einsum("iab,kbc->ikac", B, Rz).reshape(nd * nr, 3, 3)


def offset_lattice(reach, step_nodes, voxel):
    """int32 [NT,3]: the whole-node offsets (a, b, c) * step_nodes with |a|, |b|, |c| <= n, n = floor(reach / (step_nodes *
    voxel)) (of the quotient plus 1e-6: a voxel rounded to float32 does not cost a step), x slowest: every translation of the model frame within reach metres per axis."""
    step_nodes, reach, voxel = int(step_nodes), float(reach), float(voxel)
    if step_nodes < 1 or not (reach >= 0 and math.isfinite(reach)) or not (0 < voxel < math.inf):
        raise ValueError("relocalise.offset_lattice: reach >= 0, step_nodes >= 1 and voxel > 0")
    n = int(math.floor(reach / (step_nodes * voxel) + 1e-6))
    k = np.arange(-n, n + 1, dtype=np.int64) * step_nodes
    out = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    if np.abs(out).max(initial=0) >= 1 << 31:
        raise ValueError("relocalise.offset_lattice: the offsets exceed int32")
    return out.astype(np.int32)


def _float3(x, who):
    v = np.asarray(x, dtype=np.float32).reshape(-1)
    if v.size != 3 or not np.isfinite(v).all():
        raise ValueError("%s: a pivot is three finite numbers, not %r" % (who, x))
    return v


def pose_scores(volume, points, rotations, offsets, pivot_cam, pivot_model, tau, min_weight=1):
    """cppf_tsdf_pose_scores: int32 device tensor [NR,NT,4] = (inliers, misses, unknown, outside) of the points float32 [P,3]
    (camera frame, 1 <= P <= 2048) under candidate (r, j): rotation rotations[r] ([NR,3,3] or [NR,9] float64, model -> camera)
    about the pivots -- pivot_cam (camera frame) is where pivot_model + offsets[j] * voxel (model frame) lands -- with offsets
    int32 [NT,3] in whole nodes of the volume.  tau: the inlier distance on the volume's value, metres.  The pivots are rounded to
    float32; candidate_pose gives the candidate's pose."""
    dev = fuse._device_of(volume)
    p = hostargs.tensor(points, torch.float32, dev).reshape(-1, 3)
    R = hostargs.tensor(rotations, torch.float64, dev).reshape(-1, 9)
    off = hostargs.tensor(offsets, torch.int32, dev).reshape(-1, 3)
    P, NR, NT = p.shape[0], R.shape[0], off.shape[0]
    if not 1 <= P <= MAX_POINTS:
        raise ValueError("relocalise.pose_scores: 1 to %d points per call, not %d" % (MAX_POINTS, P))
    if NR * NT > MAX_CANDIDATES:
        raise ValueError("relocalise.pose_scores: %d x %d candidates exceed the limit of %d" % (NR, NT, MAX_CANDIDATES))
    tau = float(np.float32(tau))
    if not (0 < tau < math.inf) or int(min_weight) < 1:
        raise ValueError("relocalise.pose_scores: tau is a positive finite length and min_weight >= 1")
    c, m0 = _float3(pivot_cam, "relocalise.pose_scores"), _float3(pivot_model, "relocalise.pose_scores")
    out = torch.zeros((NR, NT, 4), dtype=torch.int32, device=dev)
    nx, ny, nz = volume.dims
    L = _lib.load()
    _lib.check(L.cppf_tsdf_pose_scores(ops._p(volume.acc), ops._p(volume.wsum), fuse._host3(volume.origin), C.c_float(volume.voxel), nx,
                                       ny, nz, C.c_float(volume.trunc), int(min_weight), ops._p(p), P, ops._p(R), NR,
                                       c.ctypes.data_as(C.c_void_p), m0.ctypes.data_as(C.c_void_p), ops._p(off), NT, C.c_float(tau),
                                       ops._p(out), ops._stream()), "cppf_tsdf_pose_scores")
    return out


def candidate_pose(rotations, offsets, r, j, pivot_cam, pivot_model, voxel):
    """float64 [12] (row-major 3x4, model -> camera) of candidate (r, j): R = rotations[r], t = c - R (m0 + offsets[j] * voxel),
    with c, m0 and voxel rounded to float32 as the kernel has them and everything else float64."""
    R = np.asarray(rotations, dtype=np.float64).reshape(-1, 3, 3)[r]
    off = np.asarray(offsets, dtype=np.float64).reshape(-1, 3)[j]
    c, m0 = _float3(pivot_cam, "relocalise.candidate_pose").astype(np.float64), _float3(pivot_model, "relocalise.candidate_pose").astype(np.float64)
    t = c - R @ (m0 + off * float(np.float32(voxel)))
    return np.hstack([R, t[:, None]]).reshape(12)


def frame_points(depth, K, mask=None, count=256, pixel_offset=0.0, seed=0):
    """(points float32 [n,3], readings): n = min(count, readings) of the frame's masked pixels with a reading (depth > 0 and
    finite; every such pixel when mask is None), drawn without replacement by numpy's default_rng(seed) and kept in pixel order,
    back-projected through the ray of (c + pixel_offset, r + pixel_offset) in float64 and rounded once.  On the host: not hot."""
    d = depth.detach().cpu().numpy() if torch.is_tensor(depth) else np.asarray(depth)
    d = d.reshape(d.shape[-2:]).astype(np.float64)
    ok = (d > 0) & np.isfinite(d)
    if mask is not None:
        m = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
        if m.size != d.size:
            raise ValueError("relocalise: mask %s for depth %s" % (m.shape, d.shape))
        ok &= m.reshape(d.shape) != 0
    r, c = np.nonzero(ok)
    if len(r) > count:
        pick = np.sort(np.random.default_rng(seed).choice(len(r), size=int(count), replace=False))
        r, c = r[pick], c[pick]
    fx, fy, cx, cy = hostargs.camera4(K)
    z = d[r, c]
    return np.stack([(c + float(pixel_offset) - cx) * z / fx, (r + float(pixel_offset) - cy) * z / fy, z], -1).astype(np.float32), int(ok.sum())


def relocalise(volumes, depth, K, mask=None, points=256, step=math.radians(15.0), reach=None, top=32, iters=10, stride=1,
               pixel_offset=0.0, seed=0, min_weight=1, score_fn=None, track_fn=None, turned_over=False):
    """The pose of one depth frame [H,W] against volumes (one Volume or a list, coarse to fine) from nothing: (pose float64 [12],
    report).  `points` masked readings (frame_points, seed) are scored on volumes[0] under rotation_grid(step) times
    offset_lattice(reach, max(1, round(0.5 trunc / voxel)), voxel) with tau = 0.5 trunc, about the pivots c = the points' mean and
    m0 = the centre of volumes[0]'s box; reach defaults to half that box's longest side.  The candidates are ordered by
    inliers - misses, descending, then by flat index (a stable sort); the first `top` go through track.track (iters, stride,
    pixel_offset, mask), one batched call per volume with the frame repeated, and the one with the most last-iteration inliers on
    the finest volume is kept -- ties to the lower RMS, then the lower coarse rank.  Picked AFTER refinement: a nearly face-on
    view slides along its face and the coarse score cannot tell.
    report: dict(rotations, offsets, points, readings, step_nodes, reach, tau, rank, score (the kept candidate's four counts),
    inliers, runner_up (inliers of the second best, None when top = 1), stats (track's four of the kept one), seconds: dict(search,
    refine)).  ValueError when the mask has fewer than 6 readings.
    turned_over=True states what a user of track.join knows and the geometry of a symmetric object cannot: the frame shows the
    object turned over, so it shows what the volume has not seen.  Every refined candidate's points are then classed once more
    on the finest volume at its refined pose with tau just under trunc, where a miss is a point deep in space the volume saw
    EMPTY (the only value that far from zero), a contradiction.  A candidate is admitted if it is not lost by track's own measure
    (inlier share >= track.MIN_INLIER_SHARE) and has no more contradictions than the most-inliers candidate plus 2 % of the
    points; among the admitted those within 2 % of the points of the largest count in UNSEEN cells remain, and of those the order
    above decides (most inliers first).  The report gains
    turned_over, contradicted and unseen (the kept candidate's counts) and admitted; with nothing admitted (a flat object seen
    from below shows too little of what is known) the most-inliers candidate stands.  score_fn / track_fn stand for pose_scores / track.track (the
    tests pass the NumPy restatements with volumes on the CPU)."""
    from . import track
    score_fn = pose_scores if score_fn is None else score_fn
    track_fn = track.track if track_fn is None else track_fn
    volumes = [volumes] if isinstance(volumes, fuse.Volume) else list(volumes)
    top, points = int(top), int(points)
    if not volumes or top < 1 or not 1 <= points <= MAX_POINTS:
        raise ValueError("relocalise: at least one volume, top >= 1 and 1 to %d points" % MAX_POINTS)
    coarse = volumes[0]
    dev = coarse.device
    t0 = time.perf_counter()
    pts, readings = frame_points(depth, K, mask, points, pixel_offset, seed)
    if readings < MIN_READINGS:
        raise ValueError("relocalise: the mask has %d readings; a pose needs at least %d" % (readings, MIN_READINGS))
    side = (np.array(coarse.dims, dtype=np.float64) - 1) * coarse.voxel
    reach = 0.5 * float(side.max()) if reach is None else float(reach)
    step_nodes = max(1, int(math.floor(0.5 * coarse.trunc / coarse.voxel + 0.5 + 1e-6)))       # 1.4999999 of float32 lengths is 1.5
    tau = 0.5 * coarse.trunc
    rotations, offsets = rotation_grid(step), offset_lattice(reach, step_nodes, coarse.voxel)
    c = pts.astype(np.float64).mean(0).astype(np.float32)
    m0 = (coarse.origin + 0.5 * side).astype(np.float32)
    scores = score_fn(coarse, torch.from_numpy(pts).to(dev), rotations, offsets, c, m0, tau, min_weight)
    value = (scores[..., 0] - scores[..., 1]).reshape(-1)
    order = torch.sort(-value, stable=True).indices[:top].cpu().numpy()
    kept_scores = scores.reshape(-1, 4)[torch.from_numpy(order).to(scores.device)].cpu().numpy()
    NT = len(offsets)
    poses = np.stack([candidate_pose(rotations, offsets, int(f) // NT, int(f) % NT, c, m0, coarse.voxel) for f in order])
    t1 = fuse._sync(dev)
    d = hostargs.image_batch(depth, dev, "relocalise")[:1]
    n = len(poses)
    frames = d.expand(n, -1, -1).contiguous()
    masks = None if mask is None else hostargs.mask_batch(mask, d, dev, "relocalise", same_shape=True).expand(n, -1, -1).contiguous()
    P, S = torch.from_numpy(poses).to(dev), None
    for v in volumes:
        P, S = track_fn(v, frames, K, P, masks, iters=iters, stride=stride, pixel_offset=pixel_offset, min_weight=min_weight)
    P, S = P.reshape(-1, 12).cpu().numpy(), S.reshape(-1, 4).cpu().numpy().astype(np.float64)
    best = sorted(range(n), key=lambda k: (-S[k, 0], S[k, 1], k))
    k = best[0]
    extra = {}
    if turned_over:
        fine = volumes[-1]
        near = float(np.float32(fine.trunc)) * (1.0 - 2.0 ** -10)
        cls = np.zeros((n, 4), np.int64)
        for q in range(n):
            R, t = P[q].reshape(3, 4)[:, :3], P[q].reshape(3, 4)[:, 3]
            at = R.T @ (c.astype(np.float64) - t)                    # the model point that lands on c: the exact pose, offset 0
            cls[q] = score_fn(fine, torch.from_numpy(pts).to(dev), R.reshape(1, 9), np.zeros((1, 3), np.int32), c, at, near,
                              min_weight).reshape(4).cpu().numpy()
        slack = int(math.ceil(0.02 * len(pts)))
        admitted = [q for q in best if S[q, 2] >= track.MIN_INLIER_SHARE and cls[q, 1] <= cls[best[0], 1] + slack]
        if admitted:
            most = max(cls[q, 2] for q in admitted)
            k = next(q for q in admitted if cls[q, 2] >= most - slack)          # the first in best's order: the most inliers
        extra = dict(turned_over=True, contradicted=int(cls[k, 1]), unseen=int(cls[k, 2]), admitted=len(admitted))
    t2 = fuse._sync(dev)
    report = dict(rotations=len(rotations), offsets=NT, points=len(pts), readings=readings, step_nodes=step_nodes, reach=reach,
                  tau=float(np.float32(tau)), rank=int(k), score=[int(x) for x in kept_scores[k]], inliers=int(S[k, 0]),
                  runner_up=int(S[best[1], 0]) if n > 1 else None, stats=[float(x) for x in S[k]],
                  seconds=dict(search=t1 - t0, refine=t2 - t1), **extra)
    return P[k].copy(), report
