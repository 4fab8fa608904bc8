"""NumPy restatement of cppf_tsdf_track (cppf2_amd/csrc/cppf_track.hip): the float32 back-projection, cell lookup, trilinear value
and gradient element by element in the kernel's order, the float64 point-to-plane terms, and tests/icp_ref.py's rank-aware solve
and pose update.  The device must give these inlier counts exactly and these poses to the ICP's tolerances.  Also the box scenes
the tests of both sides share, and reference stand-ins for track.onboard's two kernel calls.  Test infrastructure only."""
import numpy as np

import fuse_ref as FR
import icp_depth_ref as DR
import icp_ref as IR

F = np.float32


def _lerp(a, b, w):
    return a + (b - a) * w


def accumulate(depth, mask, K4, pixel_offset, stride, R, t, acc, wsum, origin, voxel, trunc, min_weight, dk):
    """track_accum on one frame.  Returns (q float32 [k,3], n float32 [k,3], e float32 [k]: the inliers in pixel order; gated: the
    pixels of the stride lattice inside the mask with a reading)."""
    depth = np.asarray(depth, dtype=F)
    H, W = depth.shape
    acc, wsum = np.asarray(acc, dtype=F), np.asarray(wsum, dtype=np.int32)
    nx, ny, nz = acc.shape
    fx, fy, cx, cy = (F(v) for v in K4)
    po, voxel, trunc, dk = F(pixel_offset), F(voxel), F(trunc), F(dk)
    o = np.asarray(origin, dtype=np.float64).astype(F)
    r, c = np.mgrid[0:H:stride, 0:W:stride]
    r, c = r.reshape(-1), c.reshape(-1)
    d = depth[r, c]
    with np.errstate(all="ignore"):
        ok = (d > 0) & (d < np.inf)
        if mask is not None:
            ok &= np.asarray(mask)[r, c] != 0
        gated = int(ok.sum())
        r, c, d = r[ok], c[ok], d[ok]
        px = (((c.astype(F) + po) - cx) * d) / fx
        py = (((r.astype(F) + po) - cy) * d) / fy
        q = IR.model_frame(np.stack([px, py, d], -1), R, t)
        assert q.dtype == F
        g = [(q[:, a] - o[a]) / voxel for a in range(3)]
        n = (nx, ny, nz)
        inside = np.ones(len(d), bool)
        for a in range(3):
            inside &= (g[a] >= 0) & (g[a] < F(n[a] - 1))
        q = q[inside]
        g = [ga[inside] for ga in g]
        fl = [np.floor(ga) for ga in g]
        f = [ga - fa for ga, fa in zip(g, fl)]
        i = [fa.astype(np.int64) for fa in fl]
        tv, known = [], np.ones(len(q), bool)
        for k in range(8):
            ii, jj, kk = i[0] + (k & 1), i[1] + ((k >> 1) & 1), i[2] + ((k >> 2) & 1)
            w = wsum[ii, jj, kk]
            tv.append(acc[ii, jj, kk] / w.astype(F))
            known &= w >= min_weight
        t0, t1, t2, t3, t4, t5, t6, t7 = tv
        fx_, fy_, fz_ = f
        phi = _lerp(_lerp(_lerp(t0, t1, fx_), _lerp(t2, t3, fx_), fy_), _lerp(_lerp(t4, t5, fx_), _lerp(t6, t7, fx_), fy_), fz_)
        Gx = _lerp(_lerp(t1 - t0, t3 - t2, fy_), _lerp(t5 - t4, t7 - t6, fy_), fz_)
        Gy = _lerp(_lerp(t2 - t0, t3 - t1, fx_), _lerp(t6 - t4, t7 - t5, fx_), fz_)
        Gz = _lerp(_lerp(t4 - t0, t5 - t1, fx_), _lerp(t6 - t2, t7 - t3, fx_), fy_)
        g2 = (Gx * Gx + Gy * Gy) + Gz * Gz
        e = trunc * phi
        assert phi.dtype == g2.dtype == e.dtype == F
        inl = known & (g2 > 0) & (g2 < np.inf) & (np.abs(e) <= dk)
        s = np.sqrt(g2[inl])
        nrm = np.stack([Gx[inl] / s, Gy[inl] / s, Gz[inl] / s], -1).astype(F)
    return q[inl], nrm, e[inl], gated


def step(depth, mask, K4, pixel_offset, stride, R, t, acc, wsum, origin, voxel, trunc, min_weight, dk):
    """One iteration at the gate dk.  Returns (R, t, inliers, rms, gated, moved)."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    q, n, e, gated = accumulate(depth, mask, K4, pixel_offset, stride, R, t, acc, wsum, origin, voxel, trunc, min_weight, dk)
    Q, n, e = q.astype(np.float64), n.astype(np.float64), e.astype(np.float64)
    J = np.stack([Q[:, 1] * n[:, 2] - Q[:, 2] * n[:, 1], Q[:, 2] * n[:, 0] - Q[:, 0] * n[:, 2],
                  Q[:, 0] * n[:, 1] - Q[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]], -1)
    cnt = len(e)
    sse = float(np.sum(e * e))
    rms = float(F(np.sqrt(sse / cnt))) if cnt else 0.0
    if cnt < 6:
        return R, t, cnt, rms, gated, False
    qq = float(np.sum((Q[:, 0] * Q[:, 0] + Q[:, 1] * Q[:, 1]) + Q[:, 2] * Q[:, 2]))
    x, rank = IR._min_norm_solve(J.T @ J, J.T @ e, qq, float(cnt))
    if rank == 0 or not np.any(x != 0.0) or not np.all(np.isfinite(x)):
        return R, t, cnt, rms, gated, False
    dR = IR.rodrigues(x[:3])
    Rn = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            Rn[i, j] = (R[i, 0] * dR[j, 0] + R[i, 1] * dR[j, 1]) + R[i, 2] * dR[j, 2]
    tn = np.array([t[i] - ((Rn[i, 0] * x[3] + Rn[i, 1] * x[4]) + Rn[i, 2] * x[5]) for i in range(3)])
    return Rn, tn, cnt, rms, gated, True


def gates(iters, trunc, voxel, gate=None):
    """The gate schedule of track.track: icp_ref.schedule from 0.8 trunc to one voxel (or gate = (d0, d1))."""
    d0, d1 = (0.8 * float(F(trunc)), float(F(voxel))) if gate is None else gate
    return IR.schedule(iters, d0, d1) if iters else []


def track(depth, mask, K4, pixel_offset, stride, pose, acc, wsum, origin, voxel, trunc, min_weight, dks):
    """One frame through the gates dks.  pose: 12 float64 (row-major 3x4).  Returns (pose float64 [12], stats float32 [4]); a pose
    no iteration moved is returned as it came, byte for byte."""
    P = np.array(pose, dtype=np.float64).reshape(3, 4)
    R, t = P[:, :3].copy(), P[:, 3].copy()
    cnt, rms, gated, moves = 0, 0.0, 0, 0
    for dk in dks:
        R, t, cnt, rms, gated, moved = step(depth, mask, K4, pixel_offset, stride, R, t, acc, wsum, origin, voxel, trunc,
                                            min_weight, dk)
        moves += int(moved)
    if not len(dks):
        return P.reshape(12), np.zeros(4, F)
    return np.hstack([R, t[:, None]]).reshape(12), np.array([cnt, rms, cnt / gated if gated else 0.0, moves], dtype=F)


def track_batch(depths, masks, K4, pixel_offset, stride, poses, acc, wsum, origin, voxel, trunc, min_weight, dks):
    depths = np.asarray(depths, dtype=F)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
    out = [track(depths[b], None if masks is None else masks[b], K4, pixel_offset, stride, poses[b], acc, wsum, origin, voxel,
                 trunc, min_weight, dks) for b in range(len(depths))]
    return np.stack([o[0] for o in out]).reshape(-1, 12), np.stack([o[1] for o in out]).reshape(-1, 4)


# ----------------------------------------------------------------------------------------------
# the box scenes: icp_depth_ref's box at the origin, fuse_ref's camera and image size
# ----------------------------------------------------------------------------------------------
BOX = DR.BOX
K4 = FR.K4
K3 = np.array([[K4[0], 0.0, K4[2]], [0.0, K4[1], K4[3]], [0.0, 0.0, 1.0]])
H, W = FR.H, FR.W
VOXEL = 0.004
TRUNC = float(F(3.0 * VOXEL))
DIMS = (39, 30, 24)
ORIGIN = (-(np.array(DIMS) - 1) * VOXEL / 2 + 0.0003).astype(F)       # 0.3 mm off centre: no node on a symmetric position
ZNEAR = 0.05


def box_views(dirs):
    """(depth float32 [V,H,W] (icp_depth_ref's wall at 1.6 m off the box: it carves the free space around the object), masks
    uint8 [V,H,W], poses float64 [V,12]) of the box seen from 0.4 m along dirs.  The images are rendered at the float32 poses
    fuse_ref.look_at returns, widened."""
    poses = FR.look_at(dirs, centre=np.zeros(3)).astype(np.float64)
    depth, masks = [], []
    for P in poses.reshape(-1, 3, 4):
        d, face = DR.render_box(P[:, :3], P[:, 3], K3, H, W)
        depth.append(d)
        masks.append(face >= 0)
    return np.asarray(depth, dtype=F), np.asarray(masks).astype(np.uint8), poses


def orbit_dirs(n=36):
    a = 2 * np.pi * np.arange(n) / n
    el = 0.6 * np.sin(2 * a)
    return np.stack([np.cos(a) * np.cos(el), np.sin(a) * np.cos(el), np.sin(el)], 1)


def perturbed(pose, deg, mm, seed):
    """pose (12) moved by deg degrees about a seeded axis and by mm millimetres in a seeded direction."""
    rng = np.random.default_rng(seed)
    ax, d = rng.standard_normal(3), rng.standard_normal(3)
    P = np.asarray(pose, dtype=np.float64).reshape(3, 4)
    R = IR.rodrigues(ax / np.linalg.norm(ax) * np.deg2rad(deg)) @ P[:, :3]
    return np.hstack([R, (P[:, 3] + d / np.linalg.norm(d) * mm / 1000)[:, None]]).reshape(12)


def box_distance(x):
    """float64 [n]: the distance of the points x [n,3] (object frame) to the box's surface."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    h = BOX / 2
    outside = np.linalg.norm(np.maximum(x - h, 0.0), axis=1)
    return np.where((x <= h).all(1), (h - x).min(1), outside)


def surface_rms(depth, mask, pose, pixel_offset=0.0):
    """(rms, max) distance to the box of the frame's masked points taken through pose, float64: the capability measure."""
    r, c = np.nonzero(np.asarray(mask) != 0)
    z = np.asarray(depth, dtype=np.float64)[r, c]
    p = np.stack([(c + pixel_offset - K4[2]) * z / K4[0], (r + pixel_offset - K4[3]) * z / K4[1], z], -1)
    P = np.asarray(pose, dtype=np.float64).reshape(3, 4)
    d = box_distance((p - P[:, 3]) @ P[:, :3])
    return float(np.sqrt(np.mean(d * d))), float(d.max())


# ----------------------------------------------------------------------------------------------
# stand-ins for the two kernel calls of track.onboard (its track_fn / integrate_fn arguments), on volumes that live on the CPU
# ----------------------------------------------------------------------------------------------
def _k4(K):
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def ref_integrate(volume, depths, poses, K, masks=None, pixel_offset=0.0, znear=ZNEAR):
    import torch
    d = np.asarray(depths, dtype=F)
    acc, wsum = FR.integrate(volume.acc.numpy(), volume.wsum.numpy(), d, masks, np.asarray(poses, dtype=F).reshape(-1, 12), _k4(K),
                             pixel_offset, volume.origin, volume.voxel, volume.trunc, znear)
    volume.acc.copy_(torch.from_numpy(acc))
    volume.wsum.copy_(torch.from_numpy(wsum))
    volume.views += len(d)
    return volume


def ref_track(volume, depths, K, poses, masks=None, iters=10, gate=None, stride=1, pixel_offset=0.0, min_weight=1):
    import torch
    P, S = track_batch(np.asarray(depths, dtype=F), masks, _k4(K), pixel_offset, stride, np.asarray(poses, dtype=np.float64),
                       volume.acc.numpy(), volume.wsum.numpy(), volume.origin, volume.voxel, volume.trunc, min_weight,
                       gates(iters, volume.trunc, volume.voxel, gate))
    return torch.from_numpy(P), torch.from_numpy(S)
