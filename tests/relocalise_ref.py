"""NumPy restatement of cppf_tsdf_pose_scores (cppf2_amd/csrc/cppf_relocalise.hip): the float32 rotation of the points about the
pivot, the cell and fractions once per (rotation, point), and per whole-node offset the cell test, the eight corners and
cppf_tsdf_track's trilinear value, element by element in the kernel's order.  The device must give these counts integer for
integer.  Also relocalise.rotation_grid restated from its docstring, the prototype's scene and the
stand-in for relocalise.pose_scores on volumes that live on the CPU.  Test infrastructure only."""
import numpy as np

import fuse_ref as FR
import track_ref as T

F = np.float32
BIG = F(1048576.0)                # 2^20


def _lerp(a, b, w):
    return a + (b - a) * w


def stage(points, R, c, m0, origin, voxel):
    """(near bool [P], cell int64 [P,3], f float32 [P,3]) of the points under one rotation (9 float64, row-major)."""
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    R = np.asarray(R, dtype=np.float64).reshape(9).astype(F)
    c, m0 = np.asarray(c, dtype=F).reshape(3), np.asarray(m0, dtype=F).reshape(3)
    o, voxel = np.asarray(origin, dtype=np.float64).astype(F), F(voxel)
    with np.errstate(all="ignore"):
        dx, dy, dz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
        x = [(R[0] * dx + R[3] * dy) + R[6] * dz, (R[1] * dx + R[4] * dy) + R[7] * dz, (R[2] * dx + R[5] * dy) + R[8] * dz]
        g = np.stack([((x[a] + m0[a]) - o[a]) / voxel for a in range(3)], -1)
        assert g.dtype == F
        near = (np.abs(g) < BIG).all(1)                       # a NaN or an infinity fails
        fl = np.floor(g)
        f = g - fl
        cell = np.where(near[:, None], fl, 0).astype(np.int64)
    return near, cell, f


def pose_scores(acc, wsum, origin, voxel, trunc, min_weight, points, rotations, c, m0, offsets, tau):
    """int32 [NR,NT,4] = (inliers, misses, unknown, outside) per candidate."""
    acc, wsum = np.asarray(acc, dtype=F), np.asarray(wsum, dtype=np.int32)
    n = np.array(acc.shape, dtype=np.int64)
    rotations = np.asarray(rotations, dtype=np.float64).reshape(-1, 9)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1, 3)
    trunc, tau = F(trunc), F(tau)
    P = len(np.asarray(points).reshape(-1, 3))
    out = np.zeros((len(rotations), len(offsets), 4), np.int32)
    for r, R in enumerate(rotations):
        near, cell, f = stage(points, R, c, m0, origin, voxel)
        i = cell[None] + offsets[:, None]                                       # [NT,P,3]
        inside = near[None] & ((i >= 0) & (i <= n - 2)).all(2)
        j, p = np.nonzero(inside)
        ii, ff = i[j, p], f[p]
        tv, known = [], np.ones(len(j), bool)
        with np.errstate(all="ignore"):
            for k in range(8):
                a, b, d = ii[:, 0] + (k & 1), ii[:, 1] + ((k >> 1) & 1), ii[:, 2] + ((k >> 2) & 1)
                w = wsum[a, b, d]
                tv.append(acc[a, b, d] / w.astype(F))
                known &= w >= min_weight
            t0, t1, t2, t3, t4, t5, t6, t7 = tv
            fx, fy, fz = ff[:, 0], ff[:, 1], ff[:, 2]
            phi = _lerp(_lerp(_lerp(t0, t1, fx), _lerp(t2, t3, fx), fy), _lerp(_lerp(t4, t5, fx), _lerp(t6, t7, fx), fy), fz)
            e = trunc * phi
            assert e.dtype == F
            inl = known & (np.abs(e) <= tau)
        NT = len(offsets)
        out[r, :, 0] = np.bincount(j[inl], minlength=NT)
        out[r, :, 1] = np.bincount(j[known & ~inl], minlength=NT)
        out[r, :, 2] = np.bincount(j[~known], minlength=NT)
        out[r, :, 3] = P - out[r, :, :3].sum(1)
    return out


def rotation_grid(step):
    """relocalise.rotation_grid restated from its docstring: float64 [NR,3,3]."""
    nd = int(np.ceil(4 * np.pi / step ** 2 - 1e-9))
    nr = int(np.ceil(2 * np.pi / step - 1e-9))
    out = []
    for i in range(nd):
        z = 1.0 - (2 * i + 1) / nd
        s = np.sqrt(1.0 - z * z)
        a = i * np.pi * (3.0 - np.sqrt(5.0))
        d = np.array([s * np.cos(a), s * np.sin(a), z])
        h = np.array([1.0, 0.0, 0.0]) if abs(d[2]) > 0.9 else np.array([0.0, 0.0, 1.0])
        u = np.cross(h, d)
        u /= np.linalg.norm(u)
        B = np.stack([u, np.cross(d, u), d], 1)
        for k in range(nr):
            b = 2 * np.pi * k / nr
            out.append(B @ np.array([[np.cos(b), -np.sin(b), 0.0], [np.sin(b), np.cos(b), 0.0], [0.0, 0.0, 1.0]]))
    return np.array(out)


# ----------------------------------------------------------------------------------------------
# constructed volumes: points placed exactly (both sides' tests share them)
# ----------------------------------------------------------------------------------------------
PV = 2.0 ** -8                 # the voxel: a power of two, so that origin + g * voxel is exact in float32 for g in sixteenths
PO = np.array([-4.0, -2.0, 3.0]) * PV
EYE = np.eye(3).reshape(1, 9)
ZERO = np.zeros((1, 3), np.int32)


def plane_volume(dims, x0=2.5, trunc=3 * PV, weight=2):
    """acc / wsum of the volume whose value is (x - x0) / trunc, x0 in nodes along the first axis: exact in float32."""
    x = (PO[0] + np.arange(dims[0]) * PV - (PO[0] + x0 * PV)) / trunc
    wsum = np.full(dims, weight, np.int32)
    acc = (np.broadcast_to(x[:, None, None], dims) * weight).astype(F)
    return acc, wsum


def at(g):
    """Points that land on g (in nodes) under the identity rotation with both pivots 0."""
    return (PO + np.asarray(g, dtype=np.float64).reshape(-1, 3) * PV).astype(F)


def scores(acc, wsum, g, offsets=ZERO, tau=0.5 * 3 * PV, min_weight=1, trunc=3 * PV):
    return pose_scores(acc, wsum, PO, PV, trunc, min_weight, at(g), EYE, np.zeros(3), np.zeros(3), offsets, tau)


def placements(dims):
    """(g [n,3], the expected class per point: 0 inlier, 1 miss, 2 unknown, 3 outside) on plane_volume(dims), tau = 1.5 voxel,
    with node (4, 2, 2) made unknown by the caller: on a node, in the last cell, just outside each side, an unknown corner, and
    |trunc phi| == tau exactly."""
    n = np.array(dims, dtype=np.float64)
    g = [[2.0, 1.0, 1.0], [2.5, 1.0, 1.0], n - 1.0625, [0.0, 0.0, 0.0], [1.0, 1.5, 1.5], [1.0 - 0.0625, 1.5, 1.5]]
    want = [0, 0, 1, 1, 0, 1]              # x = 2 (0.5 off), x0 itself, the far corner (x = n - 1.0625: a miss), x = 0 (2.5 off),
    #                                        x = 1: |trunc phi| = 1.5 voxel == tau exactly, a sixteenth farther: a miss
    for a in range(3):
        for v in (-0.0625, n[a] - 1.0):
            p = np.array([2.5, 0.5, 0.5])
            p[a] = v
            g.append(p)
            want.append(3)
    g += [[3.5, 1.5, 1.5], [4.0, 2.0, 2.0], [4.5, 2.5, 2.5], [5.0, 1.5, 1.5]]
    want += [2, 2, 2, 1]                   # three cells that touch node (4, 2, 2); the cell [5, 6) does not
    return np.array(g, dtype=np.float64), want


# ----------------------------------------------------------------------------------------------
# the prototype's scene: track_ref's box and wall, sequence A from above, frames and an orbit from below
# ----------------------------------------------------------------------------------------------
VOXEL = 0.004                     # the fine volume; the coarse one has 2 VOXEL and trunc 6 VOXEL
BELOW = np.array([[0.3, 0.5, -0.8], [-0.7, 0.2, -0.5], [0.1, -0.9, -0.4]])


def dirs_a():
    """The 20 of fibonacci(48) with z > 0.15."""
    d = FR.fibonacci(48)
    return d[d[:, 2] > 0.15]


def dirs_below():
    return BELOW / np.linalg.norm(BELOW, axis=1)[:, None]


def dirs_b(n=36):
    a = 2 * np.pi * np.arange(n) / n
    el = -0.55 + 0.3 * np.sin(2 * a)
    return np.stack([np.cos(a) * np.cos(el), np.sin(a) * np.cos(el), np.sin(el)], 1)


def box_volume(voxel, trunc, pad):
    """(origin float32 [3], dims) of the volume around the box padded by pad, as fuse.Volume.around lays it out."""
    lo = -T.BOX / 2 - pad
    dims = np.ceil((T.BOX + 2 * pad) / voxel).astype(np.int64) + 1
    return lo.astype(F), tuple(int(x) for x in dims)


def fuse_box(depth, masks, poses, voxel, trunc, pad):
    """(acc, wsum, origin, voxel, trunc) of the views fused by the restatement."""
    origin, dims = box_volume(voxel, trunc, pad)
    acc, wsum = FR.integrate(np.zeros(dims, F), np.zeros(dims, np.int32), depth, masks, np.asarray(poses, F).reshape(-1, 12), T.K4, 0.0,
                             origin, F(voxel), F(trunc), T.ZNEAR)
    return acc, wsum, origin, float(F(voxel)), float(F(trunc))


def masked_points(depth, mask, count, seed):
    """float32 [count,3]: seeded masked pixels with a reading, back-projected in float64 and rounded once."""
    r, c = np.nonzero((np.asarray(mask) != 0) & (depth > 0) & np.isfinite(depth))
    pick = np.sort(np.random.default_rng(seed).choice(len(r), size=min(count, len(r)), replace=False))
    r, c = r[pick], c[pick]
    z = depth[r, c].astype(np.float64)
    return np.stack([(c - T.K4[2]) * z / T.K4[0], (r - T.K4[3]) * z / T.K4[1], z], -1).astype(F)


def bottom_gap(verts, step=0.004):
    """The largest distance from a lattice of points on the box's face z = -30 mm to the nearest of verts, metres."""
    hx, hy = T.BOX[0] / 2, T.BOX[1] / 2
    x, y = np.meshgrid(np.arange(-hx, hx + 1e-9, step), np.arange(-hy, hy + 1e-9, step), indexing="ij")
    q = np.stack([x.ravel(), y.ravel(), np.full(x.size, -T.BOX[2] / 2)], 1)
    v = np.asarray(verts, dtype=np.float64)
    if not len(v):
        return float("inf")
    d2 = ((q[:, None, :] - v[None, :, :]) ** 2).sum(2)
    return float(np.sqrt(d2.min(1).max()))


def ref_scores(volume, points, rotations, offsets, pivot_cam, pivot_model, tau, min_weight=1):
    """Stands for relocalise.pose_scores on a volume that lives on the CPU (relocalise's and track.join's score_fn)."""
    import torch
    pts = points.cpu().numpy() if torch.is_tensor(points) else points
    return torch.from_numpy(pose_scores(volume.acc.numpy(), volume.wsum.numpy(), volume.origin, volume.voxel, volume.trunc, min_weight,
                                        pts, np.asarray(rotations), pivot_cam, pivot_model, np.asarray(offsets), tau))
