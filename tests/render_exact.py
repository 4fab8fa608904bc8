"""Second reference of cppf_render_depth, written from the text of include/cppf_hip.h and not from tests/render_ref.py: it has no
tiles, no pixel boxes in the coverage, no float32 and none of the mirror's formulas.  It starts after the projection: vertices
are given as integer screen coordinates in 1/256 px plus a camera z each, so a test that uses it constructs geometry whose
projection is exact (`vertices`) and asserts that the mirror's setup lands on the same integers.

* coverage: every pixel against every triangle; edge functions in int64 (bound below); the top-left rule in Direct3D's words --
  a top edge is exactly horizontal with the interior below it (image y down), a left edge is a non-horizontal edge with the
  interior on its right; a sample point on an edge is covered only if that edge is a top or a left edge;
* depth: 1/z is linear in screen space, so z = area / (e0/z0 + e1/z1 + e2/z2) in float64 with exact integer e;
* winner: the smallest float64 z among the covering triangles with znear <= z <= zfar, ties to the lowest triangle id;
* rejected: a vertex index outside [0, V), a vertex with z < znear or NaN, a coordinate not strictly inside +-2^22 px, a triangle
  in no view's range;  need (status[1]): over the drawn triangles, the 16x16 tiles that the pixel box, clamped to the image, touches.

int64 bound: an accepted coordinate has |x| < 2^30 and a sample point 0 < p < 2^21 + 2^8 (H, W <= 8192), so every difference is
below 2^31 in magnitude, every product below 2^62 and every difference of two products below 2^63.  Test infrastructure only."""
import numpy as np

GUARD = 1 << 30          # 2^22 px in 1/256 px
FX = 128.0               # the focal length the constructed geometry assumes (cx = cy = 0, identity pose)
K = np.array([[FX, 0, 0], [0, FX, 0], [0, 0, 1.0]])
POSE = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)


def vertices(su, sv, z):
    """float32 [V,3] model points that project (identity pose, fx = fy = 128, cx = cy = 0) to exactly (su, sv) / 256 px at
    camera depth z: x = su / (256 fx) * z.  Asserts that float32 holds every coordinate exactly (z a power of two, su of at most
    24 significant bits)."""
    su, sv, z = np.asarray(su, np.float64), np.asarray(sv, np.float64), np.asarray(z, np.float64)
    v = np.stack([su / (256 * FX) * z, sv / (256 * FX) * z, z], -1)
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v, equal_nan=True), "the constructed vertices are not exact in float32"
    return v32


def _ceil_div(a, b):
    return -((-a) // b)


def render_view(su, sv, z, tris, H, W, znear, zfar, cull):
    """One view.  su, sv: Python / NumPy integers [V] (1/256 px), z float64 [V] (NaN marks an unusable vertex), tris [T,3] (any
    integers).  Returns dict(depth float64 [H,W] (0 = nothing), tri_id int64 [H,W] (-1 = nothing), count int32 [H,W] (covering
    triangles before the depth range test), cover bool [T,H,W], z float64 [T,H,W] (inf where not covered), rejected, need,
    drawn bool [T])."""
    su = [int(a) for a in su]
    sv = [int(a) for a in sv]
    z = np.asarray(z, np.float64)
    V, T = len(su), len(tris)
    py, px = np.mgrid[0:H, 0:W].astype(np.int64) * 256 + 128
    cover = np.zeros((T, H, W), bool)
    zs = np.full((T, H, W), np.inf)
    drawn = np.zeros(T, bool)
    rejected = need = 0
    for t, tri in enumerate(tris):
        idx = [int(i) for i in tri]
        if any(i < 0 or i >= V for i in idx):
            rejected += 1
            continue
        if any(not (z[i] >= znear) or not (abs(su[i]) < GUARD) or not (abs(sv[i]) < GUARD) for i in idx):
            rejected += 1
            continue
        p = [(su[i], sv[i]) for i in idx]
        zz = [float(z[i]) for i in idx]
        signed = (p[1][0] - p[0][0]) * (p[2][1] - p[0][1]) - (p[1][1] - p[0][1]) * (p[2][0] - p[0][0])
        # image y down: a positive signed area is a clockwise turn on screen, whose normal (v1-v0)x(v2-v0) has z > 0: away
        if signed == 0 or (cull and signed > 0):
            continue
        xs, ys = [q[0] for q in p], [q[1] for q in p]
        c0, c1 = max(_ceil_div(min(xs) - 128, 256), 0), min((max(xs) - 128) // 256, W - 1)
        r0, r1 = max(_ceil_div(min(ys) - 128, 256), 0), min((max(ys) - 128) // 256, H - 1)
        if c0 > c1 or r0 > r1:
            continue                                            # no sample point inside the bounding box: not drawn, not listed
        drawn[t] = True
        need += (c1 // 16 - c0 // 16 + 1) * (r1 // 16 - r0 // 16 + 1)
        inside = np.ones((H, W), bool)
        wsum = np.zeros((H, W))
        for k in range(3):                                      # edge a -> b, opposite vertex c
            a, b, c = p[(k + 1) % 3], p[(k + 2) % 3], p[k]
            side = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])          # the interior's side (never 0)
            e = np.int64(b[0] - a[0]) * (py - a[1]) - np.int64(b[1] - a[1]) * (px - a[0])
            if side < 0:
                e = -e
            if a[1] == b[1]:
                top_left = c[1] > a[1]                          # top: horizontal, the interior below
            else:
                up, dn = (a, b) if a[1] < b[1] else (b, a)      # walking down the edge, the interior lies on the right
                top_left = (dn[0] - up[0]) * (c[1] - up[1]) - (dn[1] - up[1]) * (c[0] - up[0]) < 0
            inside &= (e > 0) | ((e == 0) & top_left)
            wsum += e.astype(np.float64) / zz[k]
        cover[t] = inside
        with np.errstate(all="ignore"):
            zs[t] = np.where(inside, float(abs(signed)) / wsum, np.inf)
    zall = zs
    ok = cover & (zs >= znear) & (zs <= zfar)
    zs = np.where(ok, zs, np.inf)
    depth = zs.min(0) if T else np.full((H, W), np.inf)
    hit = np.isfinite(depth)
    tri_id = np.where(hit, (zs == depth[None]).argmax(0) if T else 0, -1).astype(np.int64)      # argmax: the first = lowest id
    return dict(depth=np.where(hit, depth, 0.0), tri_id=tri_id, count=cover.sum(0).astype(np.int32), cover=cover,
                rejected=rejected, need=need, drawn=drawn, z=zall)


def render_batch(su, sv, z, tris, tri_off, H, W, znear, zfar, cull):
    """B views in one call: view b draws tris[tri_off[b] : tri_off[b+1]]; a triangle in no view's range is rejected.  (A tri_off
    that puts a triangle into two ranges has no defined result: refused.)  Returns (list of B render_view dicts, rejected, need)."""
    tris = np.asarray(tris).reshape(-1, 3)
    tri_off = [int(a) for a in tri_off]
    B = len(tri_off) - 1
    owner = np.full(len(tris), -1)
    for b in range(B):
        for g in range(max(tri_off[b], 0), min(tri_off[b + 1], len(tris))):
            assert owner[g] < 0, "triangle %d lies in two views' ranges" % g
            owner[g] = b
    views, rejected, need = [], int((owner < 0).sum()), 0
    for b in range(B):
        sel = np.nonzero(owner == b)[0]
        assert sel.size == 0 or np.array_equal(sel, np.arange(sel[0], sel[0] + sel.size))
        views.append(render_view(su, sv, z, tris[sel], H, W, znear, zfar, cull))
        rejected += views[-1]["rejected"]
        need += views[-1]["need"]
    return views, rejected, need
