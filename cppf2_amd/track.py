"""Depth frames tracked against a signed distance volume: what lets fuse.py take a sequence of which only
the first frame's pose is known (a hand-held sequence, BOP's dynamic onboarding) or whose poses are only nominal (a turntable).
Direct alignment of the frame's points to the volume's value and gradient (Bylow et al., RSS 2013) -- no mesh, no raycast, no
nearest-neighbour search -- with the minimum-norm Gauss-Newton step of the ICP of section 13.  The reference has no such step.

    poses, stats = track(volume, depths, K, poses, masks=masks)               # B frames in one call, each from its own start
    volume, poses, report = onboard(depths, masks, K, pose0, voxel=0.004)     # frame by frame: track, then integrate
    volume, poses_b, report = join(first, second, voxel=0.004)                # a second sequence without poses (section 32)
    python -m cppf2_amd.fuse --views <dir> --track --voxel 0.004 --out obj.ply

The kernel is cppf_tsdf_track (include/cppf_hip_experimental.h; the definitions are stated in cppf2_amd/csrc/cppf_track.hip and
restated in tests/track_ref.py).  weighting= weights what is integrated, never the tracker's residuals.
Capture range: a frame whose surface lies farther than trunc from the volume's surface has no
gradient to follow; report["max_step"] beside report["trunc"] says how close a sequence came.  Not done: coarse-to-fine
pyramids, loop closure, bundle adjustment, colour, weights on the tracker's residuals.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np
import torch

from . import _lib, depthfilter, depthweights, fuse, hostargs, ops, render
from ._lib import CppfError

MAX_FRAMES = 65535               # frames per cppf_tsdf_track call
GATE_START = 0.8                 # the first iteration's inlier gate, in units of trunc; the last one's is one voxel
MIN_INLIER_SHARE = 0.5           # a frame with a smaller share of inliers among its gated pixels is reported lost

_WS = hostargs.ScratchCache("cppf_tsdf_track_workspace_bytes", CppfError)


def gates(iters, d0, d1):
    """float32 [iters]: the inlier gates d_k = d0 (d1 / d0)^(k / (iters - 1)) (d0 when iters = 1), float64 on the host and rounded
    once: cppf_icp_refine's schedule."""
    d0, d1 = float(np.float32(d0)), float(np.float32(d1))
    if not (0 < d0 < np.inf and 0 < d1 < np.inf):
        raise ValueError("track: the gates are positive and finite lengths, not (%r, %r)" % (d0, d1))
    if iters == 1:
        return np.array([d0], dtype=np.float32)
    return np.array([np.float32(d0 * (d1 / d0) ** (k / (iters - 1))) for k in range(iters)], dtype=np.float32)


def track(volume, depths, K, poses, masks=None, iters=10, gate=None, stride=1, pixel_offset=0.0, min_weight=1):
    """cppf_tsdf_track: (poses float64 [B,12], stats float32 [B,4]), device tensors, of the frames depths [B,H,W] (metres; 0 = no
    reading) started at poses [B,12] or [B,3,4] (model -> OpenCV camera; the argument is not written) against the volume, one
    batched call.  masks [B,H,W] (non-zero = the object; None: every pixel with a reading); gate = (first, last) inlier distance
    in metres on the volume's value (default 0.8 trunc down to one voxel, geometric over the iterations); the pixels (r, c) with
    r and c multiples of stride take part; pixel_offset as fuse.integrate's.  stats: inliers of the last iteration, their RMS
    distance, inliers / masked pixels with a reading, iterations that moved the pose.  A frame that finds fewer than 6 inliers
    keeps its pose byte for byte."""
    dev = fuse._device_of(volume)
    d = hostargs.image_batch(depths, dev, "track.track", max_images=MAX_FRAMES, max_dim=fuse.MAX_IMAGE)
    B, H, W = d.shape
    m = None if masks is None else hostargs.mask_batch(masks, d, dev, "track.track", same_shape=True)
    P = hostargs.tensor(poses, torch.float64, dev).reshape(-1, 12).clone()
    if P.shape[0] != B:
        raise ValueError("track.track: %d poses for %d frames" % (P.shape[0], B))
    iters, stride = int(iters), int(stride)
    if iters < 0 or stride < 1 or int(min_weight) < 1:
        raise ValueError("track.track: iters >= 0, stride >= 1 and min_weight >= 1")
    d0, d1 = (GATE_START * volume.trunc, volume.voxel) if gate is None else gate
    dk = gates(iters, d0, d1) if iters else np.zeros((0,), dtype=np.float32)
    stats = torch.zeros((B, 4), dtype=torch.float32, device=dev)
    L = _lib.load()
    ws = _WS.get(hostargs.stream_key(dev), int(L.cppf_tsdf_track_workspace_bytes(B, H, W, stride)), dev)
    nx, ny, nz = volume.dims
    _lib.check(L.cppf_tsdf_track(B, ops._p(d), ops._p(m), H, W, hostargs.camera4(K), C.c_float(pixel_offset), stride,
                                 ops._p(volume.acc), ops._p(volume.wsum), fuse._host3(volume.origin), C.c_float(volume.voxel), nx, ny,
                                 nz, C.c_float(volume.trunc), int(min_weight), iters, dk.ctypes.data_as(C.c_void_p), ops._p(P),
                                 ops._p(stats), ops._p(ws), ws.numel(), ops._stream()), "cppf_tsdf_track")
    return P, stats


def box_corners(box):
    """float64 [8,3]: the corners of the box [2,3] = (lo, hi)."""
    box = np.asarray(box, dtype=np.float64).reshape(2, 3)
    return np.array([[box[(k >> a) & 1, a] for a in range(3)] for k in range(8)])


def max_step(poses, corners):
    """The largest distance, in the camera frame, that a corner moves between two consecutive poses [V,12]: how far the object's
    surface moved from one frame to the next, the length to hold against trunc."""
    P = np.asarray(poses, dtype=np.float64).reshape(-1, 3, 4)
    x = np.einsum("vij,kj->vki", P[:, :, :3], corners) + P[:, None, :, 3]
    return float(np.linalg.norm(x[1:] - x[:-1], axis=2).max()) if len(P) > 1 else 0.0


def _weights_kw(w, weighting, a=None, b=None):
    """integrate_fn's keyword arguments for the frames a..b of a sequence's weights w (none when weighting is off: the call is
    what it always was)."""
    return {} if w is None else dict(weights=w[a:b], carve_weight=weighting.carve_weight)


def _follow(volume, d, m, K, P, S, kw, pixel_offset, znear, track_fn, integrate_fn, w=None, weighting=None):
    """The frame loop of onboard and join: frame 0 is integrated at P[0]; every later frame is tracked from the previous frame's
    result (written to P[v], its stats to S[v]) and integrated at its own.  w: the frames' weights (None: unweighted), handed to
    integrate_fn frame by frame; the tracker does not see them."""
    dev = P.device

    def sl(x, a, b):
        return None if x is None else x[a:b]
    integrate_fn(volume, d[:1], P[:1], K, sl(m, 0, 1), pixel_offset, znear, **_weights_kw(w, weighting, 0, 1))
    for v in range(1, d.shape[0]):
        p, s = track_fn(volume, d[v:v + 1], K, P[v - 1:v], sl(m, v, v + 1), **kw)
        P[v], S[v] = p.reshape(12).to(dev), s.reshape(4).to(dev)
        integrate_fn(volume, d[v:v + 1], P[v:v + 1], K, sl(m, v, v + 1), pixel_offset, znear, **_weights_kw(w, weighting, v, v + 1))


def onboard(depths, masks, K, pose0, voxel, extent=None, trunc=None, iters=10, stride=1, sweeps=1, gate=None, pixel_offset=0.0,
            min_weight=1, min_inlier_share=MIN_INLIER_SHARE, znear=render.ZNEAR, dev=None, track_fn=None, integrate_fn=None,
            condition=None, weighting=None, weights_fn=None):
    """A volume from a sequence of which only the first frame's pose is known: (volume, poses float64 [V,12] on the host, report).
    The volume is Volume.around the first frame at pose0, padded by extent (+ trunc + voxel) on every side: the first frame shows
    one side only, so extent defaults to the longest side of the first frame's box.  Frame 0 is integrated at pose0; every
    later frame is tracked from the previous frame's result and integrated at its own.  Then `sweeps` times: frames 1.. are
    tracked in ONE batched call against the finished volume, each from its own pose, and all frames are integrated into a fresh
    volume (frame 0 stays at pose0: it fixes the object's frame).
    report: dict(frames: per frame dict(inliers, rms, inlier_share, moved, lost), lost: how many, max_step: the largest motion
    of the first frame's box corners between consecutive estimates, metres, trunc, voxel, dims, sweeps, seconds).  lost =
    inlier_share < min_inlier_share; max_step above trunc means the next surface may have lain outside the band that has a
    gradient.  condition: a depthfilter.Settings record (None: the readings as they are): the frames are
    conditioned before anything sees them, and the report gains `condition`.  weighting: a
    depthweights.Settings record (None: every observation counts once): every frame gets weights by viewing angle (after
    conditioning) and is integrated with them, the same weights in the frame loop and in every sweep;
    the tracker is not weighted; the report gains `weighting` and min_weight is in units of weight.  track_fn / integrate_fn /
    weights_fn stand for track / fuse.integrate / depthweights.apply (tests/test_track.py passes the NumPy restatements and
    dev="cpu")."""
    weights_fn = depthweights.apply if weights_fn is None else weights_fn
    track_fn = track if track_fn is None else track_fn
    integrate_fn = fuse.integrate if integrate_fn is None else integrate_fn
    dev = ops._dev() if dev is None else torch.device(dev)
    t0 = time.perf_counter()
    d = hostargs.image_batch(depths, dev, "track.onboard", max_dim=fuse.MAX_IMAGE)
    d, conditioned = depthfilter.apply(d, condition, "track.onboard")
    w, weighted = weights_fn(d, K, weighting, pixel_offset, "track.onboard")
    V = d.shape[0]
    m = None if masks is None else hostargs.mask_batch(masks, d, dev, "track.onboard", same_shape=True)
    pose0 = np.asarray(pose0, dtype=np.float64).reshape(1, 12)
    sweeps = int(sweeps)
    if sweeps < 0:
        raise ValueError("track.onboard: sweeps >= 0")

    def sl(x, a, b):
        return None if x is None else x[a:b]
    box = fuse.Volume.bounds(d[:1], sl(m, 0, 1), pose0, K, pixel_offset, dev)
    extent = float((box[1] - box[0]).max()) if extent is None else float(extent)
    voxel = float(np.float32(voxel))
    trunc = float(np.float32(fuse.TRUNC_VOXELS * voxel if trunc is None else trunc))
    volume = fuse.Volume.around(d[:1], sl(m, 0, 1), pose0, K, voxel, extent + trunc + voxel, trunc, pixel_offset, dev)
    kw = dict(iters=iters, gate=gate, stride=stride, pixel_offset=pixel_offset, min_weight=min_weight)
    P = torch.zeros((V, 12), dtype=torch.float64, device=dev)
    S = torch.zeros((V, 4), dtype=torch.float32, device=dev)
    P[0] = torch.from_numpy(pose0[0]).to(dev)
    _follow(volume, d, m, K, P, S, kw, pixel_offset, znear, track_fn, integrate_fn, w, weighting)
    for _ in range(sweeps if V > 1 else 0):
        p, s = track_fn(volume, d[1:], K, P[1:], sl(m, 1, V), **kw)
        P[1:], S[1:] = p.reshape(-1, 12).to(dev), s.reshape(-1, 4).to(dev)
        volume = fuse.Volume(volume.origin, voxel, volume.dims, trunc, dev)
        integrate_fn(volume, d, P, K, m, pixel_offset, znear, **_weights_kw(w, weighting))
    poses, stats = P.cpu().numpy(), S.cpu().numpy().astype(np.float64)
    frames = _frame_reports(stats, min_inlier_share, first_fixed=True)
    report = dict(frames=frames, lost=sum(f["lost"] for f in frames), max_step=max_step(poses, box_corners(box)), trunc=trunc,
                  voxel=voxel, dims=list(volume.dims), sweeps=sweeps, seconds=time.perf_counter() - t0)
    if conditioned is not None:
        report["condition"] = conditioned
    if weighted is not None:
        report["weighting"] = weighted
    return volume, poses, report


def _frame_reports(stats, min_inlier_share, first_fixed):
    return [dict(inliers=int(s[0]), rms=float(s[1]), inlier_share=float(s[2]), moved=int(s[3]),
                 lost=bool((v > 0 or not first_fixed) and s[2] < min_inlier_share)) for v, s in enumerate(stats)]


def join(first, second, voxel, coarse=2, trunc=None, points=256, step=np.deg2rad(15.0), reach=None, top=32, iters=10, stride=1,
         sweeps=0, gate=None, pixel_offset=0.0, min_weight=1, min_inlier_share=MIN_INLIER_SHARE, znear=render.ZNEAR, seed=0, dev=None,
         track_fn=None, integrate_fn=None, score_fn=None, turned_over=False, condition=None, weighting=None, weights_fn=None):
    """A second sequence without any pose joined to a first one whose poses are known: the object turned
    over between the two, BOP's model-free static onboarding.  (volume, poses_second float64 [V,12] on the host, report).
    first = dict(depths, masks, K, poses): poses given, or onboard's result; second = dict(depths, masks, K); masks may be None.
    The fine volume is Volume.around all of first's frames at `voxel` (trunc: default 3 voxels), the coarse one at coarse * voxel
    with trunc 3 * coarse * voxel; first is integrated into both.  relocalise.relocalise finds second's frame 0 against (coarse,
    fine) -- points, step, reach, top, seed are its arguments --, then onboard's frame loop runs on the fine volume from that
    pose: every later frame is tracked from the previous one's result and integrated.  The volume only covers what first saw,
    padded by trunc + voxel: the sequences show one object.  sweeps times: all of second is tracked in ONE batched call against
    the finished volume and both sequences are integrated into a fresh one.  turned_over: relocalise's (for an object with
    symmetries, whose seen side the turned-over sequence fits as well as its own: the frame goes where it shows unseen space).
    report: dict(relocalise: relocalise's report, frames: per frame of second dict(inliers, rms, inlier_share, moved, lost) --
    frame 0's are the refinement's --, lost, max_step, trunc, voxel, dims, coarse_dims, sweeps, seconds).  condition: as
    onboard's, on both sequences (the report's `condition` sums them).  weighting: as onboard's, on both sequences and in
    every volume a frame is integrated into (fine, coarse, sweeps); the pose search and the tracker are not weighted.  track_fn,
    integrate_fn, score_fn, weights_fn stand for track, fuse.integrate, relocalise.pose_scores and depthweights.apply (the
    tests pass the NumPy restatements and dev="cpu")."""
    from . import relocalise as RL
    weights_fn = depthweights.apply if weights_fn is None else weights_fn
    track_fn = track if track_fn is None else track_fn
    integrate_fn = fuse.integrate if integrate_fn is None else integrate_fn
    dev = ops._dev() if dev is None else torch.device(dev)
    t0 = time.perf_counter()
    da = hostargs.image_batch(first["depths"], dev, "track.join", max_dim=fuse.MAX_IMAGE)
    db = hostargs.image_batch(second["depths"], dev, "track.join", max_dim=fuse.MAX_IMAGE)
    da, cond_a = depthfilter.apply(da, condition, "track.join")
    db, cond_b = depthfilter.apply(db, condition, "track.join")
    wa, weighted_a = weights_fn(da, first["K"], weighting, pixel_offset, "track.join")
    wb, weighted_b = weights_fn(db, second["K"], weighting, pixel_offset, "track.join")
    ma = None if first.get("masks") is None else hostargs.mask_batch(first["masks"], da, dev, "track.join", same_shape=True)
    mb = None if second.get("masks") is None else hostargs.mask_batch(second["masks"], db, dev, "track.join", same_shape=True)
    Ka, Kb = first["K"], second["K"]
    Pa = hostargs.tensor(first["poses"], torch.float64, dev).reshape(-1, 12)
    coarse, sweeps = int(coarse), int(sweeps)
    if Pa.shape[0] != da.shape[0] or not bool(torch.isfinite(Pa).all()):
        raise ValueError("track.join: the first sequence has one finite pose per frame")
    if coarse < 1 or sweeps < 0:
        raise ValueError("track.join: coarse >= 1 and sweeps >= 0")
    voxel = float(np.float32(voxel))
    trunc = float(np.float32(fuse.TRUNC_VOXELS * voxel if trunc is None else trunc))
    box = fuse.Volume.bounds(da, ma, Pa, Ka, pixel_offset, dev)
    volume = fuse.Volume.around(da, ma, Pa, Ka, voxel, None, trunc, pixel_offset, dev)
    rough = fuse.Volume.around(da, ma, Pa, Ka, coarse * voxel, None, fuse.TRUNC_VOXELS * coarse * voxel, pixel_offset, dev)
    integrate_fn(volume, da, Pa, Ka, ma, pixel_offset, znear, **_weights_kw(wa, weighting))
    integrate_fn(rough, da, Pa, Ka, ma, pixel_offset, znear, **_weights_kw(wa, weighting))
    pose0, found = RL.relocalise([rough, volume], db[0], Kb, None if mb is None else mb[0], points, step, reach, top, iters, stride,
                                 pixel_offset, seed, min_weight, score_fn, track_fn, turned_over)
    V = db.shape[0]
    kw = dict(iters=iters, gate=gate, stride=stride, pixel_offset=pixel_offset, min_weight=min_weight)
    P = torch.zeros((V, 12), dtype=torch.float64, device=dev)
    S = torch.zeros((V, 4), dtype=torch.float32, device=dev)
    P[0] = torch.from_numpy(pose0).to(dev)
    S[0] = torch.tensor(found["stats"], dtype=torch.float32, device=dev)
    _follow(volume, db, mb, Kb, P, S, kw, pixel_offset, znear, track_fn, integrate_fn, wb, weighting)
    for _ in range(sweeps):
        p, s = track_fn(volume, db, Kb, P, mb, **kw)
        P, S = p.reshape(-1, 12).to(dev), s.reshape(-1, 4).to(dev)
        volume = fuse.Volume(volume.origin, voxel, volume.dims, trunc, dev)
        integrate_fn(volume, da, Pa, Ka, ma, pixel_offset, znear, **_weights_kw(wa, weighting))
        integrate_fn(volume, db, P, Kb, mb, pixel_offset, znear, **_weights_kw(wb, weighting))
    poses = P.cpu().numpy()
    frames = _frame_reports(S.cpu().numpy().astype(np.float64), min_inlier_share, first_fixed=False)
    report = dict(relocalise=found, frames=frames, lost=sum(f["lost"] for f in frames), max_step=max_step(poses, box_corners(box)),
                  trunc=trunc, voxel=voxel, dims=list(volume.dims), coarse_dims=list(rough.dims), sweeps=sweeps,
                  seconds=time.perf_counter() - t0)
    if condition is not None:
        report["condition"] = depthfilter.merged([cond_a, cond_b])
    if weighting is not None:
        report["weighting"] = depthweights.merged([weighted_a, weighted_b])
    return volume, poses, report


def pose_differences(poses, recorded):
    """Per frame (rotation difference in degrees, translation difference in metres) of poses [V,12] against recorded ones; None
    where the recorded pose is not finite (the folder had none)."""
    out = []
    for p, g in zip(np.asarray(poses, dtype=np.float64).reshape(-1, 3, 4), np.asarray(recorded, dtype=np.float64).reshape(-1, 3, 4)):
        if not np.isfinite(g).all():
            out.append(None)
            continue
        c = np.clip((np.trace(p[:, :3].T @ g[:, :3]) - 1) / 2, -1, 1)
        out.append(dict(rotation_deg=float(np.degrees(np.arccos(c))), translation_m=float(np.linalg.norm(p[:, 3] - g[:, 3]))))
    return out


def onboard_scene(views_dir, voxel, obj_id=None, trunc=None, min_weight=1, use_masks=True, pixel_offset=0.0, mesh_scale=0.001,
                  simplify_cell=None, iters=10, stride=1, sweeps=1, extent=None, close=False, support_plane=None, support_lift=None,
                  condition=None, weighting=None):
    """fuse.fuse_scene for a folder of which only the first image's pose is used: (mesh in metres, report); the report gains
    `track` (onboard's report, and per frame `recorded`: the difference to the pose the folder has for it, where it has one --
    recorded, not judged).  close, support_plane, support_lift: as fuse.fuse_scene's (the first image's pose, the one that is
    known, takes an "auto" plane into the object's frame).  condition and weighting: as fuse.fuse_scene's."""
    batches, conditioned = fuse.condition_batches(fuse.read_views(views_dir, obj_id, mesh_scale, use_masks, first_pose_only=True), condition)
    if len(batches) != 1:
        raise fuse.ViewsError("%s: --track takes images of one size and camera matrix, not %d kinds" % (views_dir, len(batches)))
    b = batches[0]
    support_plane = fuse._scene_plane(support_plane, support_lift, voxel, pixel_offset, batches, views_dir)
    t0 = time.perf_counter()
    volume, poses, rep = onboard(b["depths"], b["masks"], b["K"], b["poses"][0], voxel, extent, trunc, iters, stride, sweeps,
                                 pixel_offset=pixel_offset, min_weight=min_weight, weighting=weighting)
    t1 = fuse._sync(volume.device)
    mesh, closed = fuse._surface(volume, min_weight, close, support_plane, support_lift)
    t2 = fuse._sync(volume.device)
    for f, im, diff in zip(rep["frames"], b["im_ids"], pose_differences(poses, b["poses"])):
        f["im_id"], f["recorded"] = int(im), diff
    mesh, report = fuse._conditioned(fuse._finish(volume, mesh, (0.0, t1 - t0, t2 - t1), simplify_cell, closed), conditioned)
    mesh, report = fuse._weighted((mesh, report), rep.get("weighting"))
    return mesh, dict(report, track=rep)


def join_scene(views_dir, join_dir, voxel, obj_id=None, trunc=None, min_weight=1, use_masks=True, pixel_offset=0.0, mesh_scale=0.001,
               simplify_cell=None, iters=10, stride=1, track_sweeps=None, extent=None, step=np.deg2rad(15.0), top=32, coarse=2,
               points=256, close=False, support_plane=None, support_lift=None, turned_over=False, condition=None, weighting=None):
    """fuse.fuse_scene for two folders of one object, the second (join_dir: the object turned over) read without its poses:
    (mesh in metres, report); the report gains `join` (join's report, and per frame of the second folder `recorded`, as
    onboard_scene's).  track_sweeps not None (--track): the first folder's poses come from onboard (first pose only, that many
    sweeps) and the report gains `track` too.  close, support_plane, support_lift: as fuse.fuse_scene's, on the first folder.
    condition and weighting: as fuse.fuse_scene's, on both folders."""
    tracked = track_sweeps is not None
    batches, cond_a = fuse.condition_batches(fuse.read_views(views_dir, obj_id, mesh_scale, use_masks, first_pose_only=tracked), condition)
    others, cond_b = fuse.condition_batches(fuse.read_views(join_dir, obj_id, mesh_scale, use_masks, no_poses=True), condition)
    if len(batches) != 1 or len(others) != 1:
        raise fuse.ViewsError("--join takes images of one size and camera matrix per folder, not %d and %d kinds" % (len(batches), len(others)))
    a, b = batches[0], others[0]
    support_plane = fuse._scene_plane(support_plane, support_lift, voxel, pixel_offset, batches, views_dir)
    t0 = time.perf_counter()
    extra, poses_a = {}, a["poses"]
    if tracked:
        _, poses_a, rep_a = onboard(a["depths"], a["masks"], a["K"], a["poses"][0], voxel, extent, trunc, iters, stride, track_sweeps,
                                    pixel_offset=pixel_offset, min_weight=min_weight, weighting=weighting)
        for f, im, diff in zip(rep_a["frames"], a["im_ids"], pose_differences(poses_a, a["poses"])):
            f["im_id"], f["recorded"] = int(im), diff
        extra["track"] = rep_a
    volume, poses_b, rep = join(dict(depths=a["depths"], masks=a["masks"], K=a["K"], poses=poses_a),
                                dict(depths=b["depths"], masks=b["masks"], K=b["K"]), voxel, coarse, trunc, points, step, None, top, iters,
                                stride, pixel_offset=pixel_offset, min_weight=min_weight, turned_over=turned_over, weighting=weighting)
    t1 = fuse._sync(volume.device)
    mesh, closed = fuse._surface(volume, min_weight, close, support_plane, support_lift)
    t2 = fuse._sync(volume.device)
    for f, im, diff in zip(rep["frames"], b["im_ids"], pose_differences(poses_b, b["poses"])):
        f["im_id"], f["recorded"] = int(im), diff
    conditioned = None if condition is None else depthfilter.merged([cond_a, cond_b])
    mesh, report = fuse._conditioned(fuse._finish(volume, mesh, (0.0, t1 - t0, t2 - t1), simplify_cell, closed), conditioned)
    mesh, report = fuse._weighted((mesh, report), rep.get("weighting"))
    return mesh, dict(report, join=rep, **extra)
