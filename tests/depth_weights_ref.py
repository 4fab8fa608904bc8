"""NumPy restatement of cppf_depth_weights (cppf2_amd/csrc/cppf_depthweights.hip) and of cppf_tsdf_integrate_weighted
(cppf2_amd/csrc/cppf_fuse.hip), DESIGN.md section 34: every float32 operation in the kernels' order, so that the integers and
the bytes match; and the scenes the CPU and the GPU tests share (tilted planes, fuse_ref's sphere with angle-dependent noise).
Nothing here needs the library or a GPU."""
import functools

import numpy as np

import depth_condition_ref as DR
import fuse_ref as FR

F = np.float32


def _f(x):
    return np.asarray(x, dtype=F)


def weights(depth, K4, pixel_offset=0.0, step=1, jump=0.01, jump_rel=0.0, levels=16, cos_min=0.2):
    """(weights uint8 [I,H,W], counts int64 [I,3]) of depth [I,H,W] or [H,W]; K4 = (fx, fy, cx, cy)."""
    d = np.ascontiguousarray(depth, dtype=F)
    d = d.reshape((1,) + d.shape) if d.ndim == 2 else d
    s, L = int(step), int(levels)
    assert d.ndim == 3 and 1 <= s <= 4 and 1 <= L <= 255 and 0 <= cos_min < 1
    I, H, W = d.shape
    fx, fy, cx, cy = (F(v) for v in K4)
    po, jump, jump_rel, cos_min, fL = F(pixel_offset), F(jump), F(jump_rel), F(cos_min), F(L)
    v = DR.valid(d)
    inside = np.ones(d.shape, bool)
    with np.errstate(all="ignore"):
        z = np.where(v, d, F(0))
        tol = _f(jump + _f(jump_rel * z))

        def at(dy, dx):
            """(reading, usable) of the position (r + dy, c + dx): inside the image, valid and near the centre."""
            q = DR._shift(z, dy, dx, s, F(0))
            ok = DR._shift(v, dy, dx, s, False) & DR._shift(inside, dy, dx, s, False)
            return q, ok & (np.abs(_f(q - z)) <= tol)
        (ql, okl), (qr, okr), (qu, oku), (qd, okd) = at(0, -s), at(0, s), at(-s, 0), at(s, 0)
        usable = v & okl & okr & oku & okd

        def ux(c):
            return _f(_f(_f(c.astype(F) + po) - cx) / fx)[None, None, :]

        def uy(r):
            return _f(_f(_f(r.astype(F) + po) - cy) / fy)[None, :, None]
        cols, rows = np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64)
        ux_l, ux_c, ux_r = ux(cols - s), ux(cols), ux(cols + s)
        uy_u, uy_c, uy_d = uy(rows - s), uy(rows), uy(rows + s)
        px, py, pz = _f(ux_c * z), _f(uy_c * z), z
        txx, txy, txz = _f(_f(ux_r * qr) - _f(ux_l * ql)), _f(_f(uy_c * qr) - _f(uy_c * ql)), _f(qr - ql)
        tyx, tyy, tyz = _f(_f(ux_c * qd) - _f(ux_c * qu)), _f(_f(uy_d * qd) - _f(uy_u * qu)), _f(qd - qu)
        nx = _f(_f(txy * tyz) - _f(txz * tyy))
        ny = _f(_f(txz * tyx) - _f(txx * tyz))
        nz = _f(_f(txx * tyy) - _f(txy * tyx))

        def dot(a, b):
            return _f(_f(_f(a[0] * b[0]) + _f(a[1] * b[1])) + _f(a[2] * b[2]))
        a, nn, pp = dot((nx, ny, nz), (px, py, pz)), dot((nx, ny, nz), (nx, ny, nz)), dot((px, py, pz), (px, py, pz))
        den = _f(nn * pp)
        good = usable & (den > 0) & (den < np.inf)
        c = _f(np.sqrt(_f(_f(a * a) / np.where(good, den, F(1)))))
        good &= c >= cos_min
        t = np.floor(_f(_f(c * fL) + F(0.5)))
        assert c.dtype == t.dtype == den.dtype == F
        lev = np.where(t >= fL, L, np.where(t >= 1, np.where(good, t, F(1)).astype(np.int64), 1))
    w = np.where(good, lev, 0).astype(np.uint8)
    ax = (1, 2)
    counts = np.stack([v.sum(ax), (v & (w == 0)).sum(ax), (w == L).sum(ax)], 1).astype(np.int64)
    return w, counts


def integrate(acc, wsum, depth, masks, poses, weights, carve_weight, K4, pixel_offset, origin, voxel, trunc, znear):
    """cppf_tsdf_integrate_weighted on host arrays: fuse_ref.integrate with weights uint8 [V,H,W] and carve_weight."""
    acc, wsum = np.array(acc, dtype=F), np.array(wsum, dtype=np.int32)
    nx, ny, nz = acc.shape
    depth = np.asarray(depth, dtype=F)
    V, H, W = depth.shape if depth.ndim == 3 else (0, 1, 1)
    poses = np.asarray(poses, dtype=F).reshape(-1, 12)
    wts = np.asarray(weights, dtype=np.uint8)
    carve = int(carve_weight)
    assert 0 <= carve <= 255 and (V == 0 or wts.shape == depth.shape)
    fx, fy, cx, cy = (F(v) for v in K4)
    po, voxel, trunc, znear = F(pixel_offset), F(voxel), F(trunc), F(znear)
    o = np.asarray(origin, dtype=F)
    x = (o[0] + np.arange(nx, dtype=F) * voxel)[:, None, None]
    y = (o[1] + np.arange(ny, dtype=F) * voxel)[None, :, None]
    z = (o[2] + np.arange(nz, dtype=F) * voxel)[None, None, :]
    with np.errstate(all="ignore"):
        for v in range(V):
            P = poses[v]
            zc = ((P[8] * x + P[9] * y) + P[10] * z) + P[11]
            xc = ((P[0] * x + P[1] * y) + P[2] * z) + P[3]
            yc = ((P[4] * x + P[5] * y) + P[6] * z) + P[7]
            uf = (((fx * xc) / zc + cx) - po) + F(0.5)
            vf = (((fy * yc) / zc + cy) - po) + F(0.5)
            assert zc.dtype == uf.dtype == vf.dtype == F
            ok = (zc >= znear) & (uf >= 0) & (uf < F(W)) & (vf >= 0) & (vf < F(H))
            col = np.floor(np.where(ok, uf, F(0))).astype(np.int64)
            row = np.floor(np.where(ok, vf, F(0))).astype(np.int64)
            d = depth[v][row, col]
            ok &= (d > 0) & (d < np.inf)
            sdf = d - zc
            inm = np.ones(ok.shape, bool) if masks is None else (np.asarray(masks)[v][row, col] != 0)
            q = sdf / trunc
            carves = ~inm | ~(q < 1)
            obs = np.where(carves, F(1), q).astype(F)
            w = np.where(carves, carve, wts[v][row, col].astype(np.int32)).astype(np.int32)
            upd = ok & np.where(inm, ~(sdf < -trunc), sdf > 0) & (w != 0)
            acc = np.where(upd, acc + (w.astype(F) * obs).astype(F), acc).astype(F)
            wsum = wsum + np.where(upd, w, 0).astype(np.int32)
    return acc, wsum


# ----------------------------------------------------------------------------------------------
# tilted planes
# ----------------------------------------------------------------------------------------------
PLANE_K4 = (150.0, 150.0, 31.5, 23.5)


def tilted_plane(H, W, degrees, axis, K4=PLANE_K4, z0=0.6, pixel_offset=0.0):
    """(depth float32 [H,W], cos float64 [H,W]): the plane through (0, 0, z0) whose normal is (0, 0, -1) turned by `degrees`
    about the camera's x axis (axis = "x") or y axis ("y"), as z-depth along the ray of each pixel, and the cosine between each
    pixel's ray and the normal, both in float64 (the depth then rounded once)."""
    fx, fy, cx, cy = K4
    t = np.radians(degrees)
    n = np.array([0.0, np.sin(t), -np.cos(t)]) if axis == "x" else np.array([np.sin(t), 0.0, -np.cos(t)])
    c, r = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ray = np.stack([(c + pixel_offset - cx) / fx, (r + pixel_offset - cy) / fy, np.ones_like(c)], -1)
    den = ray @ n
    depth = (n[2] * z0) / den
    cos = np.abs(den) / np.linalg.norm(ray, axis=-1)
    return depth.astype(F), cos


def expected_levels(cos, levels):
    """(lo, hi) int64: the levels a pixel of exact cosine `cos` may take: floor(cos L + 0.5) clamped to 1..L, and either
    neighbour where cos L + 0.5 lies within 1e-3 of an integer."""
    t = cos * levels + 0.5
    lo, hi = np.floor(t - 1e-3), np.floor(t + 1e-3)
    return np.clip(lo, 1, levels).astype(np.int64), np.clip(hi, 1, levels).astype(np.int64)


# ----------------------------------------------------------------------------------------------
# fuse_ref's sphere, with Nguyen et al. 2012's axial noise
# ----------------------------------------------------------------------------------------------
N_VIEWS = 24


def noise_sigma(z, th):
    """Nguyen, Izadi, Lovell 2012, axial: metres; z metres, th radians (capped at 87 degrees by the caller)."""
    return 0.0012 + 0.0019 * (z - 0.4) ** 2 + 0.0001 / np.sqrt(z) * th ** 2 / (np.pi / 2 - th) ** 2


@functools.lru_cache(maxsize=None)
def sphere_scene(kind, noisy):
    """dict(depth, masks, poses) of fuse_ref.sphere_views(fibonacci(24)) with a wall at 1.6 m (kind "wall") or a table under
    the sphere (kind "table"; the plane z = centre.z - radius of the object's frame).  noisy: Gaussian noise of noise_sigma on
    the masked pixels only, the angle taken from the sphere's true normal and capped at 87 degrees, numpy.random.default_rng(0),
    added in float64 and rounded once.  Read-only arrays."""
    kw = dict(wall=1.6) if kind == "wall" else dict(plane_z=float(FR.CENTRE[2] - FR.RADIUS))
    depth, masks, poses = FR.sphere_views(FR.fibonacci(N_VIEWS), **kw)
    if noisy:
        fx, fy, cx, cy = FR.K4
        c, r = np.meshgrid(np.arange(FR.W, dtype=np.float64), np.arange(FR.H, dtype=np.float64))
        ray = np.stack([(c - cx) / fx, (r - cy) / fy, np.ones_like(c)], -1)
        rng = np.random.default_rng(0)
        out = depth.astype(np.float64)
        for v, P in enumerate(poses.astype(np.float64).reshape(-1, 3, 4)):
            m = masks[v] != 0
            cc = P[:, :3] @ FR.CENTRE + P[:, 3]
            p = ray[m] * out[v][m][:, None]
            n = (p - cc) / np.linalg.norm(p - cc, axis=1, keepdims=True)
            cos = np.abs((n * p).sum(1)) / np.linalg.norm(p, axis=1)
            th = np.minimum(np.arccos(np.clip(cos, 0.0, 1.0)), np.radians(87.0))
            out[v][m] += rng.standard_normal(int(m.sum())) * noise_sigma(out[v][m], th)
        depth = out.astype(F)
    res = dict(depth=depth, masks=masks, poses=poses)
    for a in res.values():
        a.setflags(write=False)
    return res


def mesh_figures(acc, wsum, origin, voxel=FR.VOXEL, min_weight=1):
    """dict(rms, max: distance of the welded mesh's vertices to the sphere in metres; triangles, boundary_edges) of a volume on
    the host, through fuse_ref's extract and weld."""
    tris, keys, _, _ = FR.extract(acc, wsum, origin, voxel, min_weight)
    verts, faces, boundary = FR.weld(tris, keys)
    return figures_of(verts, faces, boundary)


def figures_of(verts, faces, boundary):
    d = FR.sphere_distance(verts)
    return dict(rms=float(np.sqrt(np.mean(d * d))), max=float(d.max()), triangles=int(len(faces)), boundary_edges=int(boundary))


# the bounds the feature has to meet: the weighted mesh against the UNWEIGHTED fusion of the same images
RMS_RATIO = {False: 0.5, True: 0.7}             # exact depth, noisy depth
ZERO_SHARE = 0.2                                # of the masked pixels
TRIANGLE_BAND = 0.05


def check_scene(unweighted, weighted, zero_share, noisy):
    """The bounds on one scene; the figures are mesh_figures' / figures_of's."""
    print("noisy=%s unweighted %r weighted %r ratio %.3f zero_share %.3f"
          % (noisy, unweighted, weighted, weighted["rms"] / unweighted["rms"], zero_share))
    assert weighted["rms"] <= RMS_RATIO[bool(noisy)] * unweighted["rms"], (weighted, unweighted)
    assert weighted["max"] <= unweighted["max"], (weighted, unweighted)
    assert zero_share <= ZERO_SHARE, zero_share
    if unweighted["boundary_edges"] == 0:
        assert weighted["boundary_edges"] == 0, weighted
    assert abs(weighted["triangles"] - unweighted["triangles"]) <= TRIANGLE_BAND * unweighted["triangles"], (weighted, unweighted)


def masked_zero_share(w, masks, depth):
    m = (np.asarray(masks) != 0) & DR.valid(depth)
    return float((np.asarray(w)[m] == 0).mean())


# ----------------------------------------------------------------------------------------------
# stand-ins for depthweights.apply and the weighted fuse.integrate in track.onboard / track.join (their weights_fn /
# integrate_fn arguments), on volumes that live on the CPU
# ----------------------------------------------------------------------------------------------
def _k4(K):
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def ref_apply(depths, K, settings, pixel_offset=0.0, who=None):
    from cppf2_amd import depthweights
    if settings is None:
        return None, None
    w, counts = weights(np.asarray(depths, dtype=F), _k4(K), pixel_offset, *settings[:5])
    return w, depthweights.summary(settings, counts)


def ref_integrate(volume, depths, poses, K, masks=None, pixel_offset=0.0, znear=0.05, weights=None, carve_weight=1):
    import torch
    d = np.asarray(depths, dtype=F)
    m = None if masks is None else np.asarray(masks)
    args = (_k4(K), pixel_offset, volume.origin, volume.voxel, volume.trunc, znear)
    P = np.asarray(poses, dtype=F).reshape(-1, 12)
    if weights is None:
        acc, wsum = FR.integrate(volume.acc.numpy(), volume.wsum.numpy(), d, m, P, *args)
    else:
        acc, wsum = integrate(volume.acc.numpy(), volume.wsum.numpy(), d, m, P, np.asarray(weights), carve_weight, *args)
    volume.acc.copy_(torch.from_numpy(acc))
    volume.wsum.copy_(torch.from_numpy(wsum))
    volume.views += len(d)
    return volume
