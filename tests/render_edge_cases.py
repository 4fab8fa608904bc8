"""The inputs of tests/test_render_edges.py (CPU: mirror against render_exact) and tests/test_render_edges_gpu.py (device against
both), built once per process.  Every case is exact by construction: identity pose, fx = fy = 128, cx = cy = 0, vertex z from
{0.5, 1, 2, 4}, x = su / (256 fx) z with integer su -- so the integers handed to render_exact ARE the snapped positions (each test
asserts that through render_ref.setup).  Test infrastructure only."""
import functools
from types import SimpleNamespace

import numpy as np

import render_exact as RX
import render_ref as RR

ZSET = np.array([0.5, 1.0, 2.0, 4.0])
NAN = float("nan")


def make(name, su, sv, z, tris, tri_off, H, W, znear=0.25, zfar=100.0, cull=0, override=None, **extra):
    """override: {vertex: (x, y, z)} model coordinates that replace the constructed ones (unusable vertices, whose z in the
    exact reference is NaN or below znear)."""
    su = np.asarray(su, np.int64)
    sv = np.asarray(sv, np.int64)
    z = np.asarray(z, np.float64)
    verts = RX.vertices(su, sv, z) if len(su) else np.zeros((0, 3), np.float32)
    for i, xyz in (override or {}).items():
        verts[i] = xyz
    return SimpleNamespace(name=name, su=su, sv=sv, z=z, verts=verts, tris=np.asarray(tris, np.int32).reshape(-1, 3),
                           tri_off=np.asarray(tri_off, np.int32), H=H, W=W, znear=znear, zfar=zfar, cull=cull, **extra)


def view_ranges(tri_off, total):
    """[(b, first, last)] of the non-empty views and the set of triangles that lie in no view's range."""
    left = set(range(total))
    out = []
    for b in range(len(tri_off) - 1):
        a, e = max(int(tri_off[b]), 0), min(int(tri_off[b + 1]), total)
        if a < e:
            out.append((b, a, e))
            left -= set(range(a, e))
    return out, left


# ---- the two references on a case ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact(name):
    c = case(name)
    views, rejected, need = RX.render_batch(c.su, c.sv, c.z, c.tris, c.tri_off, c.H, c.W, c.znear, c.zfar, c.cull)
    return SimpleNamespace(depth=np.stack([v["depth"] for v in views]), tri_id=np.stack([v["tri_id"] for v in views]),
                           count=np.stack([v["count"] for v in views]), views=views, rejected=rejected, need=need)


@functools.lru_cache(maxsize=None)
def mirror(name):
    """render_ref.render per view.  The mirror indexes its vertex array directly, so a triangle with an index outside [0, V) is
    pointed at an appended NaN vertex (rejected there too, numbering kept)."""
    c = case(name)
    B, V = len(c.tri_off) - 1, len(c.verts)
    verts = np.concatenate([c.verts, np.full((1, 3), np.nan, np.float32)])
    tris = c.tris.copy()
    tris[((tris < 0) | (tris >= V)).any(1)] = V
    depth = np.zeros((B, c.H, c.W), np.float32)
    tid = np.full((B, c.H, c.W), -1, np.int32)
    count = np.zeros((B, c.H, c.W), np.int32)
    ranges, left = view_ranges(c.tri_off, len(tris))
    rejected, need, snapped = len(left), 0, True
    for b, a, e in ranges:
        depth[b], tid[b], rej, count[b] = RR.render(verts, tris[a:e], RX.POSE, RX.K, c.H, c.W, c.znear, c.zfar, c.cull, with_count=True)
        q, _ = RR.setup(verts, tris[a:e], RX.POSE, RX.K, c.H, c.W, c.znear, c.cull)
        rejected += rej
        need += int(((q["tc1"] - q["tc0"] + 1) * (q["tr1"] - q["tr0"] + 1)).sum())
        # the mirror's snapped records are the constructed integers (in some corner order) with 1/z of the constructed depths
        for j, t in enumerate(q["id"]):
            want = sorted((int(c.su[i]), int(c.sv[i]), float(np.float32(1) / np.float32(c.z[i]))) for i in tris[a + t])
            got = sorted((int(q["x%d" % k][j]), int(q["y%d" % k][j]), float(q["iz%d" % k][j])) for k in range(3))
            snapped &= want == got
    return SimpleNamespace(depth=depth, tri_id=tid, count=count, rejected=rejected, need=need, snapped=snapped)


def depth_error(got, name):
    """Worst relative error of a float32 depth array against the exact depth of the case, over the pixels both draw; the
    drawn sets must agree except where the exact z lies within 1e-6 of a depth limit (returned: how many such pixels)."""
    c, x = case(name), exact(name)
    near = np.zeros(x.depth.shape, bool)
    for b, v in enumerate(x.views):
        for lim in (c.znear, c.zfar):
            near[b] |= (v["cover"] & (np.abs(v["z"] - lim) <= 1e-6 * lim)).any(0)
    both = (got > 0) & (x.depth > 0)
    assert np.array_equal((got > 0) | near, (x.depth > 0) | near), name
    err = np.abs(got.astype(np.float64) - x.depth)[both & ~near] / x.depth[both & ~near]
    return (float(err.max()) if err.size else 0.0), int(near.sum())


# ---- a. lattice triangulations -------------------------------------------------------------------------------------------
def _orient(su, sv, tris, front):
    """Winds each triangle front-facing (negative signed area on a y-down screen) where front[t], back-facing elsewhere."""
    a, b, c = tris.T
    signed = (su[b] - su[a]) * (sv[c] - sv[a]) - (sv[b] - sv[a]) * (su[c] - su[a])
    flip = (signed < 0) != front
    out = tris.copy()
    out[flip] = out[flip][:, [0, 2, 1]]
    return out


@functools.lru_cache(maxsize=None)
def lattice_mesh(seed, H, W, n, step):
    """n points with integer coordinates (1/256 px) reaching 2 px past every border -- a third on pixel centres, a third on
    pixel corners (four of them exactly 2 px outside the four borders), the rest on any multiple of `step` (128: centres, corners and the middles of pixel sides, which puts more
    sample points on edges; 1: anywhere) -- Delaunay-triangulated.  Returns (su, sv, tris, hull) with hull the convex hull's
    vertices in order; asserts that the triangles tile the hull (integer areas add up)."""
    from scipy.spatial import ConvexHull, Delaunay
    rng = np.random.default_rng(seed)
    k, m = n // 3, step
    pts = np.concatenate([
        np.stack([128 + 256 * rng.integers(-2, W + 2, k), 128 + 256 * rng.integers(-2, H + 2, k)], -1),
        np.stack([256 * rng.integers(-2, W + 3, k), 256 * rng.integers(-2, H + 3, k)], -1),
        np.stack([m * rng.integers(-512 // m, (256 * W + 512) // m + 1, n - 2 * k),
                  m * rng.integers(-512 // m, (256 * H + 512) // m + 1, n - 2 * k)], -1)])
    pts[k:k + 4] = [[pts[k, 0], -512], [pts[k + 1, 0], 256 * H + 512], [-512, pts[k + 2, 1]], [256 * W + 512, pts[k + 3, 1]]]
    pts = np.unique(pts, axis=0).astype(np.int64)
    tris = Delaunay(pts.astype(np.float64)).simplices.astype(np.int64)
    su, sv = pts[:, 0], pts[:, 1]
    a, b, c = tris.T
    area2 = np.abs((su[b] - su[a]) * (sv[c] - sv[a]) - (sv[b] - sv[a]) * (su[c] - su[a]))
    assert (area2 > 0).all()
    hull = pts[ConvexHull(pts.astype(np.float64)).vertices]
    hx, hy = hull[:, 0], hull[:, 1]
    assert area2.sum() == abs(int((hx * np.roll(hy, -1) - np.roll(hx, -1) * hy).sum()))
    return su, sv, tris, hull


def hull_sides(hull, H, W):
    """(strictly inside, strictly outside) masks of the pixels' sample points against the convex polygon `hull` (integers)."""
    py, px = np.mgrid[0:H, 0:W].astype(np.int64) * 256 + 128
    e = np.stack([(bx - ax) * (py - ay) - (by - ay) * (px - ax) for (ax, ay), (bx, by) in zip(hull, np.roll(hull, -1, 0))])
    if (e > 0).all(0).sum() < (e < 0).all(0).sum():
        e = -e
    return (e > 0).all(0), (e < 0).any(0)


def on_edge_pixels(su, sv, tris, H, W):
    """Mask of the pixels whose sample point lies exactly on an edge or a vertex of a triangle."""
    py, px = np.mgrid[0:H, 0:W].astype(np.int64) * 256 + 128
    out = np.zeros((H, W), bool)
    for t in tris:
        for k in range(3):
            ax, ay, bx, by = su[t[k]], sv[t[k]], su[t[(k + 1) % 3]], sv[t[(k + 1) % 3]]
            e = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
            out |= (e == 0) & (px >= min(ax, bx)) & (px <= max(ax, bx)) & (py >= min(ay, by)) & (py <= max(ay, by))
    return out


def _lattice(name, seed, zmode, cull, split, H=40, W=56, n=60, step=128):
    su, sv, tris, hull = lattice_mesh(seed, H, W, n, step)
    rng = np.random.default_rng(1000 + seed)
    z = np.ones(len(su)) if zmode == "flat" else rng.choice(ZSET, len(su))
    front = np.ones(len(tris), bool) if cull else rng.random(len(tris)) < 0.5
    tris = _orient(su, sv, tris, front)
    T = len(tris)
    return make(name, su, sv, z, tris, np.arange(T + 1) if split else [0, T], H, W, cull=cull, hull=hull, seed=seed)


LATTICE = ["lattice-s%d-%s-cull%d%s" % (s, zm, cu, sp) for s in range(4) for zm in ("flat", "mixed") for cu in (0, 1)
           for sp in ("", "-split")]


# ---- b. long lists and ties ----------------------------------------------------------------------------------------------
STACK_LENGTHS = (255, 256, 257, 512, 513, 600)


def stack_pair(T):
    """Ids of the two coincident nearest triangles: 300 and 10 where the list is that long, else the last one and 10."""
    return (300 if T > 300 else T - 1), 10


def _stack(name, T, mode):
    """T copies of the triangle (0.5, 0.5), (0.5, 15.5), (15.5, 0.5) px (front-facing), each with its own depth."""
    su = np.tile([128, 128, 3968], T)
    sv = np.tile([128, 3968, 128], T)
    zt = np.ones(T)
    if mode == "last":
        zt[:] = 2.0 + 2.0 * (np.arange(T) % 2)
        zt[T - 1] = 1.0
    elif mode == "pair":
        zt[:] = 2.0 + 2.0 * (np.arange(T) % 2)
        zt[list(stack_pair(T))] = 1.0
    return make(name, su, sv, np.repeat(zt, 3), np.arange(3 * T).reshape(T, 3), [0, T], 16, 16, cull=1, T=T, mode=mode)


STACK = ["stack-%d-%s" % (T, m) for T in STACK_LENGTHS for m in ("same", "last", "pair")]


# ---- c. depth range per pixel --------------------------------------------------------------------------------------------
def _range(name, variant):
    """Triangle 0 tilted (z 0.5 .. 4 from left to right; about 1 .. 3.4 inside the image), triangle 1 flat at z = 3 behind most of it; both cover every pixel.
    'literal' is the setting as first written down: znear = 0.75 makes the tilted triangle's z = 0.5 vertex a near-plane
    rejection (there is no clipping), and the flat one lies past zfar = 2, so nothing is drawn.  'raised' keeps those limits and
    lifts that vertex to z = 1; 'half' and 'far' keep the geometry and put znear on the vertex (z == znear is accepted)."""
    z_first = 1.0 if variant == "raised" else 0.5
    su = [-20000, 16000, 15000, -512, -512, 30000]
    sv = [-512, 30000, -6000, -512, 22000, -512]
    z = [z_first, 4.0, 4.0, 3.0, 3.0, 3.0]
    znear, zfar = {"literal": (0.75, 2.0), "raised": (0.75, 2.0), "half": (0.5, 2.0), "far": (0.5, 3.25)}[variant]
    return make(name, su, sv, z, [[0, 1, 2], [3, 4, 5]], [0, 2], 40, 56, znear=znear, zfar=zfar, cull=1, variant=variant)


RANGE = ["range-literal", "range-raised", "range-half", "range-far"]
RANGE_CAP = 0.02          # share of covered pixels whose exact z may lie within 1e-6 of a depth limit


# ---- d. rejections, e. silent non-draws ------------------------------------------------------------------------------
BIG = (1 << 30) - 64      # the largest float32 below the guard: u is a float32, so 2^30 - 1 cannot occur


def _two_views():
    """The batch the reject cases disturb: two lattice triangulations (seeds 0 and 1, mixed depths, front-facing)."""
    a, b = case("lattice-s0-mixed-cull1"), case("lattice-s1-mixed-cull1")
    su, sv, z = np.concatenate([a.su, b.su]), np.concatenate([a.sv, b.sv]), np.concatenate([a.z, b.z])
    return su, sv, z, a.tris, b.tris + len(a.su)


def _base(name):
    su, sv, z, ta, tb = _two_views()
    return make(name, su, sv, z, np.concatenate([ta, tb]), [0, len(ta), len(ta) + len(tb)], 40, 56, cull=1)


def _disturbed(name, kind):
    """The base batch with extra vertices and triangles: the extra triangles go to the start, the middle and the end of view 0
    (round robin); kept = positions of the base triangles in the new view 0."""
    su, sv, z, ta, tb = _two_views()
    V = len(su)
    f32 = np.float32
    xs, ys, zs, extra, override = [], [], [], [], {}

    def vert(x, y, zz, xyz=None):
        xs.append(x), ys.append(y), zs.append(zz)
        if xyz is not None:
            override[V + len(xs) - 1] = xyz
        return V + len(xs) - 1
    p, q, r = vert(2048, 1024, 1.0), vert(1024, 6144, 2.0), vert(9216, 2048, 0.5)       # a good front-facing triangle's corners
    if kind == "index-neg":
        extra = [[-1, q, r], [p, -1, r], [p, q, -1], [-(1 << 31), q, r]]
    elif kind == "index-nv":
        nv = V + 3
        extra = [[nv, q, r], [p, nv, r], [p, q, nv], [p, q, (1 << 31) - 1]]
    elif kind == "near":
        below = float(np.nextafter(f32(0.25), f32(0)))
        extra = [[vert(0, 0, below, (0, 0, below)), q, r], [p, q, vert(0, 0, below, (0, 0, below))]]
    elif kind == "nan":
        extra = [[vert(0, 0, NAN, (NAN, 0.1, 1.0)), q, r], [p, vert(0, 0, NAN, (0.1, NAN, 1.0)), r], [p, q, vert(0, 0, NAN, (0.1, 0.1, NAN))]]
    elif kind == "guard":
        g = 1 << 30
        extra = [[vert(g, 0, 1.0), q, r], [p, vert(-g, 0, 2.0), r], [p, q, vert(0, g, 0.5)], [vert(0, -g, 4.0), q, r]]
    elif kind == "inside-guard":            # drawn, in a third view: 1/4 px inside the guard on three sides, it fills the image
        extra = [[vert(-BIG, -512, 0.5), vert(0, BIG, 2.0), vert(BIG, -BIG, 4.0)]]
    elif kind == "silent":
        extra = [[p, vert(5632, 1536, 1.0), r],                            # collinear: p, the midpoint of p r, r
                 [p, p, r], [q, q, q],                                       # repeated vertices
                 [vert(129, 0, 1.0), vert(200, 5000, 1.0), vert(383, 0, 1.0)],        # between two columns of sample points
                 [vert(0, 1153, 1.0), vert(0, 1300, 1.0), vert(5000, 1407, 1.0)],     # between two rows
                 [vert(-4000, 0, 1.0), vert(-3000, 5000, 1.0), vert(-1, 0, 1.0)],     # left of the image
                 [vert(14336, 0, 1.0), vert(15000, 5000, 1.0), vert(20000, 0, 1.0)],  # right of it
                 [vert(0, -4000, 1.0), vert(5000, -129, 1.0), vert(9000, -4000, 1.0)],      # above
                 [vert(0, 10240, 1.0), vert(5000, 20000, 1.0), vert(9000, 10240, 1.0)],     # below
                 [vert(1 << 29, 1 << 29, 1.0), vert(1 << 29, BIG, 1.0), vert(BIG, 1 << 29, 1.0)],      # far away
                 [p, r, q]]                                                  # back-facing under cull = 1
    else:
        raise KeyError(kind)
    own_view = kind in ("inside-guard", "silent")        # these also (or only) get a view of their own at the end
    view0 = [list(t) for t in ta]
    marks = [False] * len(ta)
    for i, t in enumerate([] if kind == "inside-guard" else extra):
        at = [0, len(view0) // 2, len(view0)][i % 3]
        view0.insert(at, t)
        marks.insert(at, True)
    kept = np.nonzero(~np.asarray(marks))[0]
    tris = np.concatenate([np.asarray(view0, np.int64), tb])
    c = make(name, np.concatenate([su, xs]), np.concatenate([sv, ys]), np.concatenate([z, zs]), tris,
             [0, len(view0), len(view0) + len(tb)], 40, 56, cull=1, override=override, kept=kept, added=len(extra), kind=kind)
    if own_view:
        c.tris = np.concatenate([c.tris, np.asarray(extra, np.int32)])
        c.tri_off = np.concatenate([c.tri_off, [len(c.tris)]]).astype(np.int32)
    return c


REJECTS = {"rej-index-neg": 4, "rej-index-nv": 4, "rej-near": 2, "rej-nan": 3, "rej-guard": 4}       # name -> rejected triangles
DISTURBED = list(REJECTS) + ["rej-inside-guard", "silent"]


def _offsets(name, kind):
    b = case("base")
    T0, T = int(b.tri_off[1]), len(b.tris)
    if kind == "empty":               # views 0, 2 and 4 are empty; 1 and 3 are the base's
        off, tris, rejected, shown = [0, 0, T0, T0, T, T], b.tris, 0, {1: 0, 3: 1}
    elif kind == "zero":
        off, tris, rejected, shown = [0, 0], b.tris[:0], 0, {}
    elif kind == "decreasing":        # view 0 as in the base, views 1 = [T0, 2) and 2 = [2, 2) empty: view 1's triangles have no view
        off, tris, rejected, shown = [0, T0, 2, 2], b.tris, T - T0, {0: 0}
    elif kind == "short":             # the last five triangles lie past tri_off[B]
        off, tris, rejected, shown = [0, T0, T - 5], b.tris, 5, {0: 0, 1: None}
    else:
        raise KeyError(kind)
    return make(name, b.su, b.sv, b.z, tris, off, 40, 56, cull=1, want_rejected=rejected, shown=shown)


OFFSETS = ["off-empty", "off-zero", "off-decreasing", "off-short"]


# ---- f. shapes -----------------------------------------------------------------------------------------------------------
def _strip(name, H, W):
    """Two triangles (a quad 2 px larger than the image on every side) with four different vertex depths."""
    x1, y1 = 256 * W + 512, 256 * H + 512
    return make(name, [-512, x1, x1, -512], [-512, -512, y1, y1], [0.5, 4.0, 1.0, 2.0], [[0, 2, 1], [0, 3, 2]], [0, 2], H, W, cull=1)


SHAPES = {"shape-1x1": (1, 1, 12), "shape-16x16": (16, 16, 24), "shape-15x17": (15, 17, 24)}
STRIPS = {"strip-1x8192": (1, 8192), "strip-8192x1": (8192, 1)}


# ---- the depth that float32 cannot hold ------------------------------------------------------------------------------
def _huge(name):
    """A flat triangle at the largest float32 depth in front of nothing, zfar = +inf: 1/z is subnormal, and where the float32
    quotient area / w rounds past the largest float it is +inf.  The header's depth 0 / id -1 mean "nothing drawn", and a depth
    that is not a number of metres is no surface: such a pixel stays empty (the kernel's z < INFINITY never admits it)."""
    f32 = np.float32
    big = np.finfo(f32).max
    su, sv = [128, 128, 3968], [128, 3968, 128]
    override = {i: (f32(su[i] / 32768.0) * big, f32(sv[i] / 32768.0) * big, big) for i in range(3)}
    c = make(name, su, sv, [1.0] * 3, [[0, 1, 2]], [0, 1], 16, 16, zfar=np.inf, cull=1, override=override)
    c.z = np.full(3, float(big))
    return c


ALL = LATTICE + STACK + RANGE + ["base"] + DISTURBED + OFFSETS + list(SHAPES) + list(STRIPS)


@functools.lru_cache(maxsize=None)
def case(name):
    part = name.split("-")
    if part[0] == "lattice":
        return _lattice(name, int(part[1][1:]), part[2], int(part[3][-1]), len(part) == 5)
    if part[0] == "stack":
        return _stack(name, int(part[1]), part[2])
    if part[0] == "range":
        return _range(name, part[1])
    if name == "base":
        return _base(name)
    if name == "silent":
        return _disturbed(name, "silent")
    if part[0] == "rej":
        return _disturbed(name, name[4:])
    if part[0] == "off":
        return _offsets(name, part[1])
    if part[0] == "shape":
        H, W, n = SHAPES[name]
        return _lattice(name, 7, "mixed", 0, False, H, W, n, 1)
    if part[0] == "strip":
        return _strip(name, *STRIPS[name])
    if name == "huge":
        return _huge(name)
    raise KeyError(name)
