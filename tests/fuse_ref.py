"""NumPy restatement of cppf_tsdf_integrate, cppf_tsdf_extract (cppf2_amd/csrc/cppf_fuse.hip) and of fuse.weld_by_key: float32
arithmetic in the order the kernels state, int64 indices.  The device must give these bits.  Also the analytic scenes the tests
of both sides share (a sphere seen from a Fibonacci sphere of cameras)."""
import itertools

import numpy as np

F = np.float32

# The polygon of each inside mask of a tetrahedron (bit p = corner p inside) of positive orientation, as edges (lo, hi) of
# tetrahedron corners, counter-clockwise seen from the outside: the table of cppf_fuse.hip's TET_CASES, written out.
TET_CASES = {
    1: [(0, 1), (0, 2), (0, 3)],
    2: [(0, 1), (1, 3), (1, 2)],
    3: [(0, 2), (0, 3), (1, 3), (1, 2)],
    4: [(0, 2), (1, 2), (2, 3)],
    5: [(0, 3), (0, 1), (1, 2), (2, 3)],
    6: [(0, 1), (1, 3), (2, 3), (0, 2)],
    7: [(0, 3), (1, 3), (2, 3)],
    8: [(0, 3), (2, 3), (1, 3)],
    9: [(0, 1), (0, 2), (2, 3), (1, 3)],
    10: [(1, 2), (0, 1), (0, 3), (2, 3)],
    11: [(0, 2), (2, 3), (1, 2)],
    12: [(0, 2), (1, 2), (1, 3), (0, 3)],
    13: [(0, 1), (1, 2), (1, 3)],
    14: [(0, 1), (0, 3), (0, 2)],
}
# the six tetrahedra of a cell: the axis permutations in lexicographic order as (corner code of p1, of p2, odd permutation);
# corner code = dx | dy << 1 | dz << 2, p0 = 0, p3 = 7
TETS = [(1, 3, False), (1, 5, True), (2, 3, True), (2, 6, False), (4, 5, False), (4, 6, True)]
SCAN_PASS_CELLS = 1024 * 256          # cells one pass of the block-sum scan covers (TSDF_SCAN_THREADS * TSDF_THREADS)


def derive_tet_cases():
    """TET_CASES from its rule: one corner q inside -> (q,a), (q,b), (q,c) with (q,a,b,c) the even permutation of least a; one
    corner q outside -> the same with b and c swapped; A < B inside -> (A,C), (A,D), (B,D), (B,C) with (A,B,C,D) even."""
    def odd(p):
        return sum(p[i] > p[j] for i in range(len(p)) for j in range(i + 1, len(p))) % 2

    def e(a, b):
        return (min(a, b), max(a, b))
    out = {}
    for m in range(1, 15):
        ins = [p for p in range(4) if m >> p & 1]
        outs = [p for p in range(4) if not m >> p & 1]
        if len(ins) == 2:
            (A, B), (Cc, D) = ins, outs
            if odd((A, B, Cc, D)):
                Cc, D = D, Cc
            out[m] = [e(A, Cc), e(A, D), e(B, D), e(B, Cc)]
        else:
            q = (ins if len(ins) == 1 else outs)[0]
            a, b, c = min(r for r in itertools.permutations([p for p in range(4) if p != q]) if not odd((q,) + r))
            if len(ins) == 3:
                b, c = c, b
            out[m] = [e(q, a), e(q, b), e(q, c)]
    return out


def integrate(acc, wsum, depth, masks, poses, K4, pixel_offset, origin, voxel, trunc, znear):
    """cppf_tsdf_integrate on host arrays: returns new (acc float32 [nx,ny,nz], wsum int32).  depth float32 [V,H,W], masks
    [V,H,W] or None, poses [V,12], K4 = (fx, fy, cx, cy)."""
    acc, wsum = np.array(acc, dtype=F), np.array(wsum, dtype=np.int32)
    nx, ny, nz = acc.shape
    depth = np.asarray(depth, dtype=F)
    V, H, W = depth.shape if depth.ndim == 3 else (0, 1, 1)
    poses = np.asarray(poses, dtype=F).reshape(-1, 12)
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
            obs = np.where(inm, np.where(q < 1, q, F(1)), F(1)).astype(F)
            upd = ok & np.where(inm, ~(sdf < -trunc), sdf > 0)
            acc = np.where(upd, acc + obs, acc).astype(F)
            wsum = wsum + upd.astype(np.int32)
    return acc, wsum


def extract(acc, wsum, origin, voxel, min_weight=1):
    """cppf_tsdf_extract on host arrays: (tris float32 [T,9], keys int64 [T,3], (T, cells that produced any), source) in the
    order cell, tetrahedron, triangle; source int64 [T,2] = (the triangle's cell as its first node's linear index, tetrahedron)."""
    acc, wsum = np.asarray(acc, dtype=F), np.asarray(wsum, dtype=np.int32)
    nx, ny, nz = acc.shape
    o, voxel = np.asarray(origin, dtype=F), F(voxel)
    with np.errstate(all="ignore"):
        t = (acc / wsum.astype(F)).astype(F)
    known, inside = wsum >= min_weight, t < 0
    if min(nx, ny, nz) < 2:
        return np.zeros((0, 9), F), np.zeros((0, 3), np.int64), (0, 0), np.zeros((0, 2), np.int64)
    ci, cj, ck = (a.reshape(-1) for a in np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij"))

    def corner(arr, code):
        return arr[ci + (code & 1), cj + ((code >> 1) & 1), ck + ((code >> 2) & 1)]
    processed = np.ones(ci.shape, bool)
    for code in range(8):
        processed &= corner(known, code)
    lin = (ci.astype(np.int64) * ny + cj) * nz + ck
    cell = np.arange(ci.size, dtype=np.int64)
    rows_t, rows_k, rows_o, rows_src = [], [], [], []
    for ti, (v1, v2, odd) in enumerate(TETS):
        codes = (0, v1, v2, 7)
        m = sum(corner(inside, c).astype(np.int64) << p for p, c in enumerate(codes))
        for case, edges in TET_CASES.items():
            sel = np.nonzero(processed & (m == case))[0]
            if not sel.size:
                continue
            pos, key = [], []
            for lo, hi in edges:
                clo, chi = codes[lo], codes[hi]
                d = chi ^ clo
                assert chi & clo == clo
                tl, th = corner(t, clo)[sel], corner(t, chi)[sel]
                s = tl / (tl - th)
                assert s.dtype == F
                n_lo = [ci[sel] + (clo & 1), cj[sel] + ((clo >> 1) & 1), ck[sel] + ((clo >> 2) & 1)]
                p = [o[a] + (n_lo[a].astype(F) + (s if (d >> a) & 1 else F(0))) * voxel for a in range(3)]
                pos.append(np.stack(p, 1).astype(F))
                llin = lin[sel] + (clo & 1) * ny * nz + ((clo >> 1) & 1) * nz + ((clo >> 2) & 1)
                key.append(8 * llin + d)
            for r in range(len(edges) - 2):
                b, c = (r + 2, r + 1) if odd else (r + 1, r + 2)
                rows_t.append(np.concatenate([pos[0], pos[b], pos[c]], 1))
                rows_k.append(np.stack([key[0], key[b], key[c]], 1))
                rows_o.append(cell[sel] * 12 + ti * 2 + r)
                rows_src.append(np.stack([lin[sel], np.full(sel.size, ti, np.int64)], 1))
    if not rows_t:
        return np.zeros((0, 9), F), np.zeros((0, 3), np.int64), (0, 0), np.zeros((0, 2), np.int64)
    order = np.concatenate(rows_o)
    idx = np.argsort(order, kind="stable")
    assert np.unique(order).size == order.size
    tris, keys, src = np.concatenate(rows_t)[idx], np.concatenate(rows_k)[idx], np.concatenate(rows_src)[idx]
    return tris.astype(F), keys.astype(np.int64), (int(len(tris)), int(np.unique(order // 12).size)), src


def weld(tris, keys, drop_degenerate=True):
    """fuse.weld_by_key: (verts float32 [N,3] in key order, faces int64 [F,3], boundary_edges); asserts that position is a
    function of key."""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1)
    pos = np.asarray(tris, dtype=F).reshape(-1, 3)
    if not keys.size:
        return np.zeros((0, 3), F), np.zeros((0, 3), np.int64), 0
    uniq, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    verts = pos[first]
    assert np.array_equal(verts[inverse].view(np.uint32), pos.view(np.uint32)), "two vertices of one key differ"
    faces = inverse.reshape(-1, 3).astype(np.int64)
    if drop_degenerate:
        p = verts[faces]
        same = (p[:, 0] == p[:, 1]).all(1) | (p[:, 1] == p[:, 2]).all(1) | (p[:, 2] == p[:, 0]).all(1)
        faces = faces[~same]
        used, inv = np.unique(faces, return_inverse=True)
        verts, faces = verts[used], inv.reshape(-1, 3).astype(np.int64)
    return verts, faces, int((edge_use(faces)[1] == 1).sum())


def edge_use(faces):
    """(undirected edges [E,2], the number of triangles that use each)."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    return np.unique(np.sort(e, 1), axis=0, return_counts=True)


def directed_edge_use(faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    return np.unique(e, axis=0, return_counts=True)


def signed_volume(verts, faces):
    p = np.asarray(verts, dtype=np.float64)[faces]
    return float(np.einsum("fi,fi->", p[:, 0], np.cross(p[:, 1], p[:, 2])) / 6.0)


def canonical_rows(tris, keys):
    """Each triangle rotated (the winding kept) to start at its smallest key."""
    tris, keys = np.asarray(tris).reshape(-1, 3, 3), np.asarray(keys).reshape(-1, 3)
    if not len(keys):
        return tris, keys
    r = np.argmin(keys, 1)
    idx = (r[:, None] + np.arange(3)[None]) % 3
    rows = np.arange(len(keys))[:, None]
    return tris[rows, idx], keys[rows, idx]


# ----------------------------------------------------------------------------------------------
# analytic scenes
# ----------------------------------------------------------------------------------------------
RADIUS = 0.05
CENTRE = np.array([0.003, -0.002, 0.004])
K4 = (150.0, 150.0, 80.0, 60.0)
H, W = 120, 160
CAM_DIST = 0.4
VOXEL = 0.004


def fibonacci(n):
    """float64 [n,3]: unit directions on a Fibonacci sphere."""
    i = np.arange(n) + 0.5
    zc = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - zc * zc)
    a = np.pi * (3.0 - np.sqrt(5.0)) * np.arange(n)
    return np.stack([r * np.cos(a), r * np.sin(a), zc], 1)


def look_at(dirs, centre=CENTRE, dist=CAM_DIST):
    """float32 [V,12] model -> OpenCV camera poses of cameras at centre + dist * dir looking at the centre."""
    out = []
    for d in np.asarray(dirs, dtype=np.float64).reshape(-1, 3):
        eye = centre + dist * d
        zax = -d / np.linalg.norm(d)
        up = np.array([0.0, 0.0, 1.0]) if abs(zax[2]) < 0.95 else np.array([0.0, 1.0, 0.0])
        xax = np.cross(zax, up)                       # x right, y down, z forward
        xax /= np.linalg.norm(xax)
        yax = np.cross(zax, xax)
        R = np.stack([xax, yax, zax])
        out.append(np.hstack([R, (-R @ eye)[:, None]]).reshape(12))
    return np.asarray(out, dtype=np.float32)


def sphere_views(dirs, plane_z=None, wall=None, centre=CENTRE, radius=RADIUS, K4=K4, H=H, W=W):
    """(depth float32 [V,H,W], masks uint8 [V,H,W], poses float32 [V,12]): z-depth of the ray through pixel (c, r) meeting the
    sphere; elsewhere the plane z = plane_z of the object's frame (a table), or the constant camera depth `wall`, or 0.  The
    masks are the sphere's pixels.  The rays use the float32 poses the fusion is given."""
    poses = look_at(dirs, centre)
    fx, fy, cx, cy = K4
    c, r = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ray = np.stack([(c - cx) / fx, (r - cy) / fy, np.ones_like(c)], -1)          # camera frame, z = 1
    depth, masks = [], []
    for P in poses.astype(np.float64).reshape(-1, 3, 4):
        cc = P[:, :3] @ centre + P[:, 3]                                            # the centre in the camera frame
        a = (ray * ray).sum(-1)
        b = ray @ cc
        disc = b * b - a * (cc @ cc - radius * radius)
        hit = disc > 0
        zs = (b - np.sqrt(np.where(hit, disc, 0.0))) / a
        d = np.zeros_like(c)
        if plane_z is not None:
            # object-frame z of the point ray * s: (R^T (ray s - t))_z = plane_z
            n = P[:, :3][:, 2]                                                      # R^T's third row
            den = ray @ n
            s = (plane_z + n @ P[:, 3]) / np.where(np.abs(den) > 1e-12, den, 1.0)
            d = np.where((np.abs(den) > 1e-12) & (s > 0), s, 0.0)
        if wall is not None:
            d = np.full_like(c, wall)
        d = np.where(hit, zs, d)
        depth.append(d)
        masks.append(hit)
    return np.asarray(depth, dtype=np.float32), np.asarray(masks).astype(np.uint8), poses


def sphere_volume(voxel=VOXEL, trunc=None, centre=CENTRE, radius=RADIUS, shift=0.0003):
    """(origin float32 [3], dims, trunc) of a volume around the sphere padded by trunc + voxel, the origin shifted by 0.3 mm so
    that no node falls on a symmetric position."""
    trunc = 3.0 * voxel if trunc is None else trunc
    pad = radius + trunc + voxel
    lo = centre - pad + shift
    dims = (int(np.ceil(2 * pad / voxel)) + 1,) * 3
    return lo.astype(np.float32), dims, float(np.float32(trunc))


def fuse(depth, masks, poses, origin, dims, voxel, trunc, K4=K4, pixel_offset=0.0, znear=0.05):
    return integrate(np.zeros(dims, F), np.zeros(dims, np.int32), depth, masks, poses, K4, pixel_offset, origin, voxel, trunc, znear)


def sphere_distance(verts, centre=CENTRE, radius=RADIUS):
    """|distance of each vertex to the sphere's surface|."""
    return np.abs(np.linalg.norm(np.asarray(verts, dtype=np.float64) - centre, axis=1) - radius)
