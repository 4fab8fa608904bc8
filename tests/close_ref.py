"""NumPy restatement of cppf_tsdf_close (cppf2_amd/csrc/cppf_close.hip): float32 arithmetic in the order
the kernel states; the open components found by flooding from the volume's faces with repeated 6-neighbour dilation.  The device
must give these bytes.  Also the analytic scenes the tests of both sides share: fuse_ref's sphere standing on, or sunk into, a
table that hides what lies below it, and the sphere with a patch of readings dropped."""
import numpy as np

import fuse_ref as ref

F = np.float32
KNOWN, FILLED, BELOW, OPEN = 0, 1, 2, 3


def faces(dims):
    """bool [nx,ny,nz]: the nodes with an index of 0 or n-1 on any axis."""
    f = np.zeros(dims, bool)
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = (True,) * 6
    return f


def flood(cand, seed):
    """bool: the nodes of `cand` that a 6-connected path inside `cand` joins to a node of `seed & cand`."""
    cur = cand & seed
    while True:
        g = cur.copy()
        g[1:] |= cur[:-1]
        g[:-1] |= cur[1:]
        g[:, 1:] |= cur[:, :-1]
        g[:, :-1] |= cur[:, 1:]
        g[:, :, 1:] |= cur[:, :, :-1]
        g[:, :, :-1] |= cur[:, :, 1:]
        g &= cand
        if np.array_equal(g, cur):
            return cur
        cur = g


def candidates(acc, wsum, origin, voxel, trunc, min_weight=1, plane=None):
    """(candidate bool, known bool, below bool, t float32, b float32) per node: steps 1 to 3 of the definition."""
    acc, wsum = np.asarray(acc, dtype=F), np.asarray(wsum, dtype=np.int32)
    nx, ny, nz = acc.shape
    known = wsum >= min_weight
    with np.errstate(all="ignore"):
        t = np.where(known, acc / wsum.astype(F), F(-1)).astype(F)
    if plane is None:
        b, below = np.full(acc.shape, -1, F), np.zeros(acc.shape, bool)
    else:
        o, voxel, trunc = np.asarray(origin, dtype=F), F(voxel), F(trunc)
        pa, pb, pc, pd = (F(v) for v in plane)
        x = (o[0] + np.arange(nx, dtype=F) * voxel)[:, None, None]
        y = (o[1] + np.arange(ny, dtype=F) * voxel)[None, :, None]
        z = (o[2] + np.arange(nz, dtype=F) * voxel)[None, None, :]
        with np.errstate(all="ignore"):
            h = ((pa * x + pb * y) + pc * z) + pd
            q = (-h) / trunc
        assert h.dtype == q.dtype == F
        b = np.where(q < F(-1), F(-1), np.where(q > F(1), F(1), q)).astype(F)
        below = np.broadcast_to(h <= 0, acc.shape)
        b = np.broadcast_to(b, acc.shape)
    return ~known & ~below, known, below, t, b


def close(acc, wsum, origin, voxel, trunc, min_weight=1, plane=None):
    """cppf_tsdf_close on host arrays: (acc_out float32, wsum_out int32, state uint8, stats int64 [4])."""
    cand, known, below, t, b = candidates(acc, wsum, origin, voxel, trunc, min_weight, plane)
    opened = flood(cand, faces(cand.shape))
    with np.errstate(invalid="ignore"):
        acc_out = np.where(opened, F(0), np.where(b > t, b, t)).astype(F)
    wsum_out = np.where(opened, 0, 1).astype(np.int32)
    state = np.select([known, opened, cand], [KNOWN, OPEN, FILLED], BELOW).astype(np.uint8)
    stats = np.array([(state == s).sum() for s in range(4)], dtype=np.int64)
    return acc_out, wsum_out, state, stats


# ----------------------------------------------------------------------------------------------
# analytic scenes
# ----------------------------------------------------------------------------------------------
def table_dirs():
    """The 18 directions of fibonacci(48) that look down on the table."""
    d = ref.fibonacci(48)
    return d[d[:, 2] > 0.25]


def _rays(K4=ref.K4, H=ref.H, W=ref.W):
    fx, fy, cx, cy = K4
    c, r = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    return np.stack([(c - cx) / fx, (r - cy) / fy, np.ones_like(c)], -1)


def table_views(dirs, pz, centre=ref.CENTRE, radius=ref.RADIUS):
    """(depth float32 [V,H,W], masks uint8, poses float32 [V,12]): per ray the nearer of the sphere and the table z = pz of the
    object's frame, which is opaque (fuse_ref.sphere_views draws the sphere even where the table hides it); the masks are the
    pixels where the sphere is the nearer one."""
    sphere, hit, poses = ref.sphere_views(dirs, centre=centre, radius=radius)
    rays = _rays()
    table = []
    for P in poses.astype(np.float64).reshape(-1, 3, 4):
        n = P[:, :3][:, 2]                                   # object-frame z of the point ray * s: (R^T (ray s - t))_z = pz
        den = rays @ n
        s = (pz + n @ P[:, 3]) / np.where(np.abs(den) > 1e-12, den, 1.0)
        table.append(np.where((np.abs(den) > 1e-12) & (s > 0), s, 0.0))
    sphere, table = sphere.astype(np.float64), np.asarray(table)
    front = (hit != 0) & ((table <= 0) | (sphere < table))
    return np.where(front, sphere, table).astype(F), front.astype(np.uint8), poses


def dropout_views(degrees, dirs=None, axis=(1.0, 0.0, 0.0), centre=ref.CENTRE):
    """fuse_ref's bare sphere (24 views) with every reading set to 0 whose surface point lies within `degrees` of `axis` as seen
    from the centre: a patch no view measured."""
    dirs = ref.fibonacci(24) if dirs is None else dirs
    depth, masks, poses = ref.sphere_views(dirs)
    rays, axis = _rays(), np.asarray(axis, dtype=np.float64)
    depth = depth.copy()
    for v, P in enumerate(poses.astype(np.float64).reshape(-1, 3, 4)):
        p = (rays * depth[v].astype(np.float64)[..., None] - P[:, 3]) @ P[:, :3] - centre      # R^T (x - t) - centre
        n = np.linalg.norm(p, axis=-1)
        cosang = (p @ axis) / np.where(n > 0, n, 1.0)
        depth[v][(masks[v] != 0) & (cosang > np.cos(np.radians(degrees)))] = 0.0
    return depth, masks, poses


def cap_volume(pz, centre=ref.CENTRE, radius=ref.RADIUS):
    """The volume of the part of the sphere above z = pz."""
    hgt = float(np.clip(centre[2] + radius - pz, 0.0, 2 * radius))
    return np.pi * hgt * hgt * (3 * radius - hgt) / 3.0


def distance_to_sphere_or_plane(verts, pz, centre=ref.CENTRE, radius=ref.RADIUS):
    """Per vertex the smaller of its distances to the sphere's surface and to the plane z = pz."""
    v = np.asarray(verts, dtype=np.float64)
    return np.minimum(ref.sphere_distance(v, centre, radius), np.abs(v[:, 2] - pz))


def components(faces_, n_verts):
    """The number of connected components of a mesh's vertices that its faces use."""
    parent = np.arange(n_verts)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in np.asarray(faces_):
        ra, rb, rc = find(a), find(b), find(c)
        parent[rb] = ra
        parent[find(rc)] = ra
    used = np.unique(faces_)
    return len({find(x) for x in used})


def topology(verts, faces_):
    """dict(boundary, manifold, components, euler) of a welded mesh."""
    _, und = ref.edge_use(faces_)
    _, dire = ref.directed_edge_use(faces_)
    return dict(boundary=int((und == 1).sum()), manifold=bool((und == 2).all() and (dire == 1).all()),
                components=components(faces_, len(verts)), euler=int(len(verts) - len(und) + len(faces_)))
