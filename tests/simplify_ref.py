"""NumPy restatement of cppf_cluster_keys, cppf_cluster_quadrics (cppf2_amd/csrc/cppf_simplify.hip) and of the face rules of
cppf2_amd.simplify.cluster: float32 keys and float64 quadrics, operation by operation in the order the kernels' header states
(NumPy fuses nothing, and its division and square root are correctly rounded), so the device is meant to give these bits.  The
clusters of one step of the serial corner loop are advanced together: each cluster still sees its own corners one after the
other, in list order.  Also the meshes both test files share (the fused sphere of tests/fuse_ref.py, the drill fixture)."""
import functools
import os

import numpy as np

import fuse_ref
import symmetry_ref

F = np.float32
KEY_RANGE = F(2097152.0)
LAMBDA = 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRILL = os.path.join(ROOT, "tests", "golden", "example_data", "obj_000015.ply")


def cluster_keys(verts, origin, cell):
    """cppf_cluster_keys: int64 [N]."""
    v = np.asarray(verts, dtype=F).reshape(-1, 3)
    o, cell = np.asarray(origin, dtype=F).reshape(3), F(cell)
    with np.errstate(all="ignore"):
        t = (v - o[None]) / cell
        assert t.dtype == F
        inside = ((t >= F(0)) & (t < KEY_RANGE)).all(1)
        i = np.floor(np.where(inside[:, None], t, F(0))).astype(np.int64)
    return np.where(inside, i[:, 0] << 42 | i[:, 1] << 21 | i[:, 2], np.int64(-1))


def corner_list(cf, C):
    """(corners int32 [M], seg_off int64 [C+1]) of the clusters cf int64 [F,3] of every corner: corner 3 f + j, sorted by cluster
    with a stable sort, so ascending within a cluster."""
    flat = np.asarray(cf, dtype=np.int64).reshape(-1)
    corners = np.argsort(flat, kind="stable").astype(np.int32)
    seg_off = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=C))]).astype(np.int64)
    return corners, seg_off


def cluster_sums(verts, faces, corners, seg_off, keys, origin, cell):
    """The running sums of cppf_cluster_quadrics after the last corner, float64: dict(ctr [C,3], count [C], vsum [C,3], A [C,6]
    (00, 01, 02, 11, 12, 22), b [C,3], w [C], m [C,3])."""
    v = np.asarray(verts, dtype=F).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    corners, seg_off = np.asarray(corners, dtype=np.int64), np.asarray(seg_off, dtype=np.int64)
    keys = np.asarray(keys, dtype=np.int64)
    C = len(keys)
    assert len(seg_off) == C + 1 and (keys >= 0).all()
    assert not len(corners) or (corners.min() >= 0 and corners.max() < 3 * len(f) and f.min() >= 0 and f.max() < len(v))
    o = np.asarray(origin, dtype=F).reshape(3).astype(np.float64)
    dcell = np.float64(F(cell))
    ijk = np.stack([(keys >> 42) & 0x1fffff, (keys >> 21) & 0x1fffff, keys & 0x1fffff], 1).astype(np.float64)
    ctr = o[None] + (ijk + 0.5) * dcell
    count, vsum = np.zeros(C), np.zeros((C, 3))
    A, b, w, m = np.zeros((C, 6)), np.zeros((C, 3)), np.zeros(C), np.zeros((C, 3))
    lens = seg_off[1:] - seg_off[:-1]
    with np.errstate(all="ignore"):
        for s in range(int(lens.max()) if C else 0):
            act = np.nonzero(lens > s)[0]
            corner = corners[seg_off[act] + s]
            face, j = corner // 3, corner % 3
            p = v[f[face]].astype(np.float64) - ctr[act][:, None, :]                 # [n,3 corners,3 axes]
            count[act] += 1.0
            vsum[act] += p[np.arange(len(act)), j]
            p0, p1, p2 = p[:, 0], p[:, 1], p[:, 2]
            e1, e2 = p1 - p0, p2 - p0
            nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            l2 = (nx * nx + ny * ny) + nz * nz
            ok = (l2 > 0.0) & (l2 < np.inf)
            at = act[ok]
            nx, ny, nz, l2, p0, p1, p2 = nx[ok], ny[ok], nz[ok], l2[ok], p0[ok], p1[ok], p2[ok]
            l = np.sqrt(l2)
            area = l / 2.0
            ux, uy, uz = nx / l, ny / l, nz / l
            d = (ux * p0[:, 0] + uy * p0[:, 1]) + uz * p0[:, 2]
            aux, auy, auz = area * ux, area * uy, area * uz
            A[at, 0] += aux * ux
            A[at, 1] += aux * uy
            A[at, 2] += aux * uz
            A[at, 3] += auy * uy
            A[at, 4] += auy * uz
            A[at, 5] += auz * uz
            ad = area * d
            b[at, 0] += ad * ux
            b[at, 1] += ad * uy
            b[at, 2] += ad * uz
            w[at] += area
            m[at] += area[:, None] * (((p0 + p1) + p2) / 3.0)
    return dict(ctr=ctr, count=count, vsum=vsum, A=A, b=b, w=w, m=m)


def cluster_quadrics(verts, faces, corners, seg_off, keys, origin, cell, lam=LAMBDA, sums=None):
    """cppf_cluster_quadrics: pos float32 [C,3]."""
    S = cluster_sums(verts, faces, corners, seg_off, keys, origin, cell) if sums is None else sums
    return (S["ctr"] + solve(S, cell, lam)).astype(F)


def solve(S, cell, lam=LAMBDA):
    """float64 [C,3]: the representatives relative to their cells' centres, after the clamp and before the final rounding."""
    lam, h = np.float64(lam), np.float64(F(cell)) / 2.0
    A, b, w, m = S["A"], S["b"], S["w"], S["m"]
    with np.errstate(all="ignore"):
        kk = lam * w
        a00, a11, a22 = A[:, 0] + kk, A[:, 3] + kk, A[:, 5] + kk
        r0, r1, r2 = b[:, 0] + lam * m[:, 0], b[:, 1] + lam * m[:, 1], b[:, 2] + lam * m[:, 2]
        l10, l20 = A[:, 1] / a00, A[:, 2] / a00
        d1 = a11 - l10 * A[:, 1]
        t21 = A[:, 4] - l20 * A[:, 1]
        l21 = t21 / d1
        d2 = (a22 - l20 * A[:, 2]) - l21 * t21
        y1 = r1 - l10 * r0
        y2 = (r2 - l20 * r0) - l21 * y1
        x2 = y2 / d2
        x1 = y1 / d1 - l21 * x2
        x0 = (r0 / a00 - l10 * x1) - l20 * x2
        x = np.stack([x0, x1, x2], 1)
        mean = np.where(S["count"][:, None] > 0.0, S["vsum"] / S["count"][:, None], 0.0)
        x = np.where(w[:, None] > 0.0, x, mean)
        return np.where(x < -h, -h, np.where(x > h, h, x))


def reduce_faces(cf):
    """The face rules of simplify.cluster on the clusters cf int64 [F,3] of every corner: (kept face indices ascending,
    dict(collapsed, cancelled, multi)).  A face two of whose corners share a cluster is dropped (collapsed).  The others are
    grouped by their sorted triple; a group's net orientation is its even minus its odd permutations; net 0 removes the whole
    group (cancelled: the faces removed so); otherwise the first face in input order with the majority orientation stays;
    multi counts the groups with |net| > 1."""
    groups, collapsed = {}, 0
    for i, (a, b, c) in enumerate(np.asarray(cf, dtype=np.int64).reshape(-1, 3).tolist()):
        if a == b or b == c or c == a:
            collapsed += 1
            continue
        odd = ((a > b) + (a > c) + (b > c)) % 2
        groups.setdefault(tuple(sorted((a, b, c))), []).append((i, -1 if odd else 1))
    kept, cancelled, multi = [], 0, 0
    for members in groups.values():
        net = sum(s for _, s in members)
        if net == 0:
            cancelled += len(members)
            continue
        multi += abs(net) > 1
        kept.append(next(i for i, s in members if s * net > 0))
    return np.asarray(sorted(kept), dtype=np.int64), dict(collapsed=collapsed, cancelled=cancelled, multi=int(multi))


def edge_counts(faces):
    """(boundary edges, non-manifold edges): undirected edges used by one face, by more than two."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if not len(faces):
        return 0, 0
    _, n = fuse_ref.edge_use(faces)
    return int((n == 1).sum()), int((n > 2).sum())


def euler(verts, faces):
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return len(verts) - len(fuse_ref.edge_use(faces)[0]) + len(faces)


def cluster(verts, faces, cell, origin=None, lam=LAMBDA, with_sums=False):
    """simplify.cluster: (verts float32 [V',3], faces int64 [F',3], report without seconds)."""
    v = np.asarray(verts, dtype=F).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    used = np.zeros(len(v), bool)
    used[f.reshape(-1)] = True
    if origin is None:
        origin = v[used].min(0) if used.any() else np.zeros(3, F)
    origin = np.asarray(origin, dtype=F).reshape(3)
    keys = cluster_keys(v, origin, cell)
    bad = int((keys[used] == -1).sum())
    if bad:
        raise ValueError("%d vertices outside the lattice" % bad)
    ukeys, inv = np.unique(keys[used], return_inverse=True)
    vc = np.full(len(v), -1, np.int64)
    vc[used] = inv.reshape(-1)
    cf = vc[f]
    corners, seg_off = corner_list(cf, len(ukeys))
    sums = cluster_sums(v, f, corners, seg_off, ukeys, origin, cell)
    pos = cluster_quadrics(v, f, corners, seg_off, ukeys, origin, cell, lam, sums)
    kept, counts = reduce_faces(cf)
    usedc, newf = np.unique(cf[kept], return_inverse=True)
    out_v, out_f = pos[usedc], newf.reshape(-1, 3).astype(np.int64)
    boundary, nonmanifold = edge_counts(out_f)
    report = dict(vertices_in=len(v), vertices_out=len(out_v), triangles_in=len(f), triangles_out=len(out_f),
                  boundary_edges=boundary, nonmanifold_edges=nonmanifold, **counts)
    if with_sums:
        return out_v, out_f, report, dict(sums, pos=pos, keys=ukeys, corners=corners, seg_off=seg_off, origin=origin, cf=cf)
    return out_v, out_f, report


def samples(verts, faces, count, seed):
    """float64 [count,3]: cppf2_amd.symmetry.sample_surface on the mesh's triangles of non-zero area."""
    tri = np.asarray(verts, dtype=np.float64).reshape(-1, 3)[np.asarray(faces, dtype=np.int64).reshape(-1, 3)]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    tri, area = tri[area > 0], area[area > 0]
    rng = np.random.default_rng(seed)
    k = rng.choice(len(tri), size=int(count), p=area / area.sum())
    r1, r2 = rng.random(int(count)), rng.random(int(count))
    s = np.sqrt(r1)
    return (1.0 - s)[:, None] * tri[k, 0] + (s * (1.0 - r2))[:, None] * tri[k, 1] + (s * r2)[:, None] * tri[k, 2]


IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(1, 12)


def one_sided(av, af, bv, bf, count=1024, seed=0):
    q = samples(av, af, count, seed).astype(F)
    t = np.asarray(bv, dtype=np.float64).reshape(-1, 3)[np.asarray(bf, dtype=np.int64).reshape(-1, 3)].reshape(-1, 9).astype(F)
    return float(symmetry_ref.deviations(q, t, IDENTITY)[0])


def deviation(av, af, bv, bf, count=1024, seed=0):
    """simplify.deviation: (a to b, b to a) in the meshes' units, by tests/symmetry_ref.py's float32 distance."""
    return one_sided(av, af, bv, bf, count, seed), one_sided(bv, bf, av, af, count, seed)


# ----------------------------------------------------------------------------------------------
# the meshes both test files use
# ----------------------------------------------------------------------------------------------
SPHERE_CELLS = (1.0, 1.5, 2.0, 3.0, 4.0)          # in voxels
DRILL_CELLS = (0.002, 0.004, 0.008)               # metres


@functools.lru_cache(maxsize=None)
def sphere_mesh():
    """(verts float32, faces int64, origin float32 [3]) of tests/fuse_ref.py's 24-view sphere: 34^3 nodes, voxel 4 mm."""
    depth, masks, poses = fuse_ref.sphere_views(fuse_ref.fibonacci(24))
    origin, dims, trunc = fuse_ref.sphere_volume()
    acc, wsum = fuse_ref.fuse(depth, masks, poses, origin, dims, fuse_ref.VOXEL, trunc)
    tris, keys, _, _ = fuse_ref.extract(acc, wsum, origin, fuse_ref.VOXEL)
    verts, faces, boundary = fuse_ref.weld(tris, keys)
    assert boundary == 0
    return verts, faces, origin


@functools.lru_cache(maxsize=None)
def drill_mesh():
    """(verts float32 in metres, faces int64, origin float32 [3] = min - 0.1 mm) of the drill fixture."""
    from cppf2_amd import render
    v, f = render.load_ply(DRILL)
    v = (v * 0.001).astype(F)
    return v, f.astype(np.int64), (v.min(0) - F(1e-4)).astype(F)


@functools.lru_cache(maxsize=None)
def sphere_cluster(cell_voxels, lam=LAMBDA):
    v, f, o = sphere_mesh()
    return cluster(v, f, F(cell_voxels * fuse_ref.VOXEL), o, lam, with_sums=True)


@functools.lru_cache(maxsize=None)
def drill_cluster(cell):
    v, f, o = drill_mesh()
    return cluster(v, f, F(cell), o, LAMBDA, with_sums=True)


@functools.lru_cache(maxsize=None)
def drill_deviation(cell):
    v, f, _ = drill_mesh()
    sv, sf, _, _ = drill_cluster(cell)
    return deviation(v, f, sv, sf)


# ----------------------------------------------------------------------------------------------
# crafted inputs: coordinates in cells of CELL on a lattice at the frame's origin
# ----------------------------------------------------------------------------------------------
CELL = F(2.0 ** -7)              # 7.8125 mm: a power of two, so that the plate's vertices are exact in float32


def fan(k, centre=(10.6, 10.3, 10.3), radius=3.0, height=1.0):
    """(verts [k+1,3] in cells, faces [k,3]): k triangles around vertex 0, the ring `radius` cells away and `height` above it,
    so that the centre's cluster owns k corners (the ring's vertices share cells where k is large)."""
    ang = 2.0 * np.pi * np.arange(k) / k
    ring = np.asarray(centre) + np.stack([radius * np.cos(ang), radius * np.sin(ang), np.full(k, height)], 1)
    faces = np.stack([np.zeros(k, np.int64), 1 + np.arange(k), 1 + (np.arange(k) + 1) % k], 1)
    return np.concatenate([[centre], ring]), faces


def _plate():
    """A flat 8 x 8 plate of 128 triangles on the plane z = 2 + x / 4 - y / 8 (cells); every coordinate a multiple of 1 / 128."""
    g = 0.25 + 0.4375 * np.arange(9)
    x, y = (a.reshape(-1) for a in np.meshgrid(g, g + 0.125, indexing="ij"))
    v = np.stack([x, y, 2.0 + x / 4 - y / 8], 1)
    q = np.array([[i * 9 + j, (i + 1) * 9 + j, (i + 1) * 9 + j + 1, i * 9 + j + 1] for i in range(8) for j in range(8)])
    return v, np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]])


PLATE_NORMAL = np.array([-0.25, 0.125, 1.0]) / np.linalg.norm([-0.25, 0.125, 1.0])
CORNER = np.array([5.7, 5.6, 5.35])


def crafted():
    """name -> (verts float32 [N,3] metres, faces int64 [F,3]); origin 0, cell CELL."""
    P = CORNER
    spread = np.array([[0.5, 0.5, 0.5], [2.5, 0.4, 0.6], [0.4, 2.5, 0.7], [4.5, 4.5, 0.5], [6.5, 4.4, 0.6], [4.4, 6.5, 0.7]])
    cases = dict(
        one_triangle=(np.array([[0.3, 0.4, 0.5], [1.6, 0.2, 0.7], [0.5, 2.3, 1.2]]), np.array([[0, 1, 2]])),
        plate=_plate(),
        cube_corner=(np.stack([P, P + [1.5, 0, 0], P + [0, 1.5, 0], P + [0, 0, 1.5]]), np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1]])),
        zero_area=(np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5], [0.25, 0.5, 0.5]]), np.array([[0, 1, 2], [3, 1, 2], [0, 0, 1]])),
        one_cell=(3.0 + np.array([[0.1, 0.1, 0.1], [0.9, 0.2, 0.1], [0.2, 0.9, 0.3], [0.4, 0.4, 0.9]]),
                  np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])),
        fan_64=fan(64), fan_65=fan(65), fan_1000=fan(1000),
        mirror_double=(spread, np.array([[0, 1, 2], [0, 2, 1], [3, 4, 5], [3, 4, 5]])),
    )
    return {k: ((np.asarray(v, dtype=np.float64) * np.float64(CELL)).astype(F), np.asarray(f, dtype=np.int64)) for k, (v, f) in cases.items()}


@functools.lru_cache(maxsize=None)
def crafted_cluster(name):
    v, f = crafted()[name]
    return cluster(v, f, CELL, np.zeros(3, F), LAMBDA, with_sums=True)


def key_cases():
    """[(verts float32 [257,3], origin float32 [3], cell)]: special rows first, random rows after.  Set A has exact boundaries
    (origin and cell are powers of two and small integers); set B reaches the upper end of the key range and the non-finite."""
    rng = np.random.default_rng(5)
    oa, ca = np.array([1.0, -2.0, 0.5], F), F(0.25)
    below = np.nextafter(oa, F(-np.inf), dtype=F)
    edge = (oa + F(3) * ca).astype(F)
    a = [oa, edge, np.nextafter(edge, F(-np.inf), dtype=F), [below[0], oa[1], oa[2]], [oa[0], below[1], oa[2]], [oa[0], oa[1], below[2]],
         [edge[0], oa[1], below[2]], oa + F(0.125)]
    a = np.concatenate([np.asarray(a, dtype=F), (oa + rng.uniform(-1, 30, (249, 3))).astype(F)])
    top, out = F(2097151.5), F(2097152.0)
    b = [[0, 0, 0], [-0.0, 0.0, -0.0], [top, top, top], [out, 1, 1], [1, out, 1], [1, 1, out], [np.nan, 1, 1], [1, np.inf, 1],
         [1, 1, -np.inf], [1e30, 1, 1], [-1e-30, 1, 1], [top, 0, 5], [np.nextafter(out, F(0), dtype=F), 2, 3]]
    b = np.concatenate([np.asarray(b, dtype=F), rng.uniform(-2, 3e6, (244, 3)).astype(F)])
    assert len(a) == len(b) == 257
    return [(a, oa, ca), (b, np.zeros(3, F), F(1.0))]
