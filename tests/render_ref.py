"""NumPy mirror of cppf_render_depth (cppf2_amd/csrc/cppf_render.hip): the same float32 operations in the same order, int64
edge functions, the top-left rule, the (z, triangle id) minimum.  One view per call, vectorised over the pixels of each
16x16 tile.  Test infrastructure only."""
import numpy as np

F32 = np.float32
GUARD = F32(2.0 ** 30)
TILE = 16


def _top_left(ax, ay, bx, by):
    dy = by - ay
    return (dy < 0) | ((dy == 0) & (bx > ax))


def setup(verts, tris, pose, K, H, W, znear=0.05, cull=1):
    """Per-triangle setup of one view: returns (records dict of the drawn triangles, number of rejected triangles)."""
    P = np.asarray(pose, dtype=F32).reshape(12)
    fx, fy, cx, cy = (F32(K[0][0]), F32(K[1][1]), F32(K[0][2]), F32(K[1][2]))
    v = np.asarray(verts, dtype=F32)[np.asarray(tris, dtype=np.int64)]         # [T,3 corners,3]
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    with np.errstate(all="ignore"):
        xc = ((P[0] * x + P[1] * y) + P[2] * z) + P[3]
        yc = ((P[4] * x + P[5] * y) + P[6] * z) + P[7]
        zc = ((P[8] * x + P[9] * y) + P[10] * z) + P[11]
        u = np.rint((fx * (xc / zc) + cx) * F32(256))
        w = np.rint((fy * (yc / zc) + cy) * F32(256))
        iz = F32(1) / zc
        bad = ~(zc >= F32(znear)) | ~(np.abs(u) < GUARD) | ~(np.abs(w) < GUARD)
    rej = bad.any(1)
    sx = np.where(rej[:, None], 0, u).astype(np.int64)
    sy = np.where(rej[:, None], 0, w).astype(np.int64)
    area = (sx[:, 1] - sx[:, 0]) * (sy[:, 2] - sy[:, 0]) - (sy[:, 1] - sy[:, 0]) * (sx[:, 2] - sx[:, 0])
    draw = ~rej & (area != 0) & ~((cull != 0) & (area > 0))
    swap = area < 0
    order = np.where(swap[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))
    sx = np.take_along_axis(sx, order, 1)
    sy = np.take_along_axis(sy, order, 1)
    iz = np.take_along_axis(iz, order, 1)
    area = np.abs(area)
    x0, x1, x2 = sx.T
    y0, y1, y2 = sy.T
    c0 = np.maximum((sx.min(1) + 127) >> 8, 0)
    c1 = np.minimum((sx.max(1) - 128) >> 8, W - 1)
    r0 = np.maximum((sy.min(1) + 127) >> 8, 0)
    r1 = np.minimum((sy.max(1) - 128) >> 8, H - 1)
    draw &= (c0 <= c1) & (r0 <= r1)
    rec = dict(x0=x0, y0=y0, x1=x1, y1=y1, x2=x2, y2=y2, iz0=iz[:, 0], iz1=iz[:, 1], iz2=iz[:, 2], area=area.astype(F32),
               tl0=_top_left(x1, y1, x2, y2), tl1=_top_left(x2, y2, x0, y0), tl2=_top_left(x0, y0, x1, y1),
               tc0=c0 // TILE, tc1=c1 // TILE, tr0=r0 // TILE, tr1=r1 // TILE)
    ids = np.nonzero(draw)[0]
    return {k: a[ids] for k, a in rec.items()} | {"id": ids.astype(np.int64)}, int(rej.sum())


def render(verts, tris, pose, K, H, W, znear=0.05, zfar=100.0, cull=1, with_count=False):
    """(depth float32 [H,W], tri_id int32 [H,W], rejected[, count int32 [H,W]: triangles covering each pixel before the depth
    range test])."""
    q, rejected = setup(verts, tris, pose, K, H, W, znear, cull)
    depth = np.zeros((H, W), F32)
    tid = np.full((H, W), -1, np.int32)
    count = np.zeros((H, W), np.int32)
    ly, lx = np.divmod(np.arange(TILE * TILE), TILE)
    znear, zfar = F32(znear), F32(zfar)
    for ty in range((H + TILE - 1) // TILE):
        rows = (q["tr0"] <= ty) & (ty <= q["tr1"])
        if not rows.any():
            continue
        for tx in range((W + TILE - 1) // TILE):
            sel = np.nonzero(rows & (q["tc0"] <= tx) & (tx <= q["tc1"]))[0]
            if sel.size == 0:
                continue
            r = ty * TILE + ly
            c = tx * TILE + lx
            px = (256 * c + 128)[None, :]
            py = (256 * r + 128)[None, :]
            g = {k: a[sel][:, None] for k, a in q.items()}
            e0 = (g["x2"] - g["x1"]) * (py - g["y1"]) - (g["y2"] - g["y1"]) * (px - g["x1"])
            e1 = (g["x0"] - g["x2"]) * (py - g["y2"]) - (g["y0"] - g["y2"]) * (px - g["x2"])
            e2 = (g["x1"] - g["x0"]) * (py - g["y0"]) - (g["y1"] - g["y0"]) * (px - g["x0"])
            cov = (e0 >= np.where(g["tl0"], 0, 1)) & (e1 >= np.where(g["tl1"], 0, 1)) & (e2 >= np.where(g["tl2"], 0, 1))
            with np.errstate(all="ignore"):
                w = e0.astype(F32) * g["iz0"]
                w = w + e1.astype(F32) * g["iz1"]
                w = w + e2.astype(F32) * g["iz2"]
                z = g["area"] / w
            ok = cov & (z >= znear) & (z <= zfar) & (z < F32(np.inf))     # the kernel's minimum starts at +inf: z = +inf never wins
            zz = np.where(ok, z, F32(np.inf))
            zmin = zz.min(0)
            best = np.where(ok & (zz == zmin[None]), g["id"], np.iinfo(np.int64).max).min(0)
            inside = (r < H) & (c < W)
            hit = inside & ok.any(0)
            depth[r[hit], c[hit]] = zmin[hit]
            tid[r[hit], c[hit]] = best[hit]
            count[r[inside], c[inside]] += cov.sum(0)[inside].astype(np.int32)
    if with_count:
        return depth, tid, rejected, count
    return depth, tid, rejected


# ---------------------------------------------------------------------------------------------
# procedural meshes
# ---------------------------------------------------------------------------------------------
def icosphere(subdiv=2, radius=1.0):
    """Outward-wound (counter-clockwise seen from outside) icosphere."""
    t = (1.0 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v) * radius, np.asarray(f, np.int32)


def cube(half=1.0):
    """Outward-wound cube of 12 triangles."""
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], float) * half
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = []
    for a, b, c, d in quads:
        f += [(a, b, c), (a, c, d)]
    f = np.asarray(f, np.int32)
    # orient outward: normal . centroid > 0
    tri = v[f]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    flip = (n * tri.mean(1)).sum(1) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return v, f


def look_pose(R, t):
    """float32 [12] of [R | t]."""
    return np.concatenate([np.asarray(R, float), np.asarray(t, float)[:, None]], 1).astype(np.float32).reshape(12)


def random_rotation(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
