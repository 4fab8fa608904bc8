"""NumPy statements of cppf_sym_deviation (cppf2_amd/csrc/cppf_symmetry.hip) for the tests.

deviation_d2: the kernel's float32 arithmetic, operation by operation in the order its header states -- every intermediate an
np.float32 array, so each operation rounds where the kernel's does and the result is meant to be bit-equal.
point_triangle_d2_f64: an independent float64 distance (projection onto the plane and an inside test by the edge normals, else
the nearest of the three edge segments), written without the region tests the kernel uses.
"""
import numpy as np

F32 = np.float32
CHUNK = 1 << 16          # (query, triangle) pairs per block of the restatement: the intermediates stay in cache


def _dot(ux, uy, uz, wx, wy, wz):
    return (ux * wx + uy * wy) + uz * wz


def map_queries(queries, M):
    """float32 [Nq,3]: the queries through one float32 map M [12], rows ((M0*x + M1*y) + M2*z) + M3."""
    q = np.asarray(queries, dtype=F32).reshape(-1, 3)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3] for r in range(3)], 1)


def point_triangle_d2(m, tris):
    """float32 [N,F]: the kernel's squared distance of every point m [N,3] (already mapped) to every triangle [F,9]."""
    m = np.asarray(m, dtype=F32).reshape(-1, 3)
    t = np.asarray(tris, dtype=F32).reshape(-1, 9)
    one, zero = F32(1), F32(0)
    a, b, c = (t[None, :, 3 * k:3 * k + 3] for k in range(3))
    ab, ac = b - a, c - a                                   # at staging: one rounding each
    with np.errstate(all="ignore"):
        ap, bp, cp = m[:, None, :] - a, m[:, None, :] - b, m[:, None, :] - c
        abx, aby, abz = ab[..., 0], ab[..., 1], ab[..., 2]
        acx, acy, acz = ac[..., 0], ac[..., 1], ac[..., 2]
        d1 = _dot(abx, aby, abz, ap[..., 0], ap[..., 1], ap[..., 2])
        d2 = _dot(acx, acy, acz, ap[..., 0], ap[..., 1], ap[..., 2])
        d3 = _dot(abx, aby, abz, bp[..., 0], bp[..., 1], bp[..., 2])
        d4 = _dot(acx, acy, acz, bp[..., 0], bp[..., 1], bp[..., 2])
        d5 = _dot(abx, aby, abz, cp[..., 0], cp[..., 1], cp[..., 2])
        d6 = _dot(acx, acy, acz, cp[..., 0], cp[..., 1], cp[..., 2])
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        rA = (d1 <= 0) & (d2 <= 0)
        rB = (d3 >= 0) & (d4 <= d3)
        rAB = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        rC = (d6 >= 0) & (d5 <= d6)
        rAC = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        rBC = (va <= 0) & (e43 >= 0) & (e56 >= 0)
        nv, nw, den = vb, vc, (va + vb) + vc
        nw, den = np.where(rBC, e43, nw), np.where(rBC, e43 + e56, den)
        onBC = rBC
        for rule, v_, w_, d_ in ((rAC, zero, d2, d2 - d6), (rC, zero, one, one), (rAB, d1, zero, d1 - d3), (rB, one, zero, one),
                                 (rA, zero, zero, one)):
            nv, nw, den = np.where(rule, v_, nv), np.where(rule, w_, nw), np.where(rule, d_, den)
            onBC = onBC & ~rule
        r = one / den
        w = nw * r
        v = np.where(onBC, one - w, nv * r)
        ex = (ap[..., 0] - abx * v) - acx * w
        ey = (ap[..., 1] - aby * v) - acy * w
        ez = (ap[..., 2] - abz * v) - acz * w
        out = (ex * ex + ey * ey) + ez * ez
    assert out.dtype == F32
    return out


def nearest_d2(m, tris):
    """float32 [N]: min over the triangles by `d2 < best` from +inf (a NaN is ignored; np.fmin is that rule for a minimum)."""
    m = np.asarray(m, dtype=F32).reshape(-1, 3)
    t = np.asarray(tris, dtype=F32).reshape(-1, 9)
    best = np.full(len(m), np.inf, dtype=F32)
    rows = max(1, CHUNK // len(t))
    for i in range(0, len(m), rows):
        d = point_triangle_d2(m[i:i + rows], t)
        best[i:i + rows] = np.fmin(best[i:i + rows], np.fmin.reduce(d, axis=1, initial=F32(np.inf)))
    return best


def deviation_d2(queries, tris, maps):
    """float32 [C]: cppf_sym_deviation's max_d2.  maps float64 [C,12] (or [C,3,4]), rounded to float32 once."""
    M = np.asarray(maps, dtype=np.float64).reshape(-1, 12)
    with np.errstate(all="ignore"):
        M = M.astype(F32)
    out = np.zeros(len(M), dtype=F32)
    for c in range(len(M)):
        out[c] = nearest_d2(map_queries(queries, M[c]), tris).max()                  # each >= 0 or +inf, never NaN
    return out


def deviations(queries, tris, maps):
    """float32 [C]: the square roots, what cppf2_amd.symmetry.deviations returns."""
    return np.sqrt(deviation_d2(queries, tris, maps))


def point_triangle_d2_f64(p, tri):
    """float64: squared distance of one point [3] to one triangle [9] or [3,3]."""
    p = np.asarray(p, dtype=np.float64).reshape(3)
    a, b, c = np.asarray(tri, dtype=np.float64).reshape(3, 3)
    n = np.cross(b - a, c - a)
    nn = n @ n
    if nn > 0:
        h = ((p - a) @ n) / nn
        f = p - h * n                                       # the foot on the plane
        inside = all(np.cross(v1 - v0, f - v0) @ n >= 0 for v0, v1 in ((a, b), (b, c), (c, a)))
        if inside:
            return float(h * h * nn)
    best = np.inf
    for v0, v1 in ((a, b), (b, c), (c, a)):
        e = v1 - v0
        ee = e @ e
        s = min(1.0, max(0.0, ((p - v0) @ e) / ee)) if ee > 0 else 0.0
        g = p - (v0 + s * e)
        best = min(best, float(g @ g))
    return best


# ---- the solids of tests/test_symmetry.py and tests/test_symmetry_gpu.py: file units millimetres, posed obliquely -----------
MESH_SCALE = 0.001
POSE_R = None            # set below: the oblique pose x -> POSE_R x + POSE_T (mm) of every solid
POSE_T = np.array([31.0, -17.0, 23.0])


def _rodrigues(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


POSE_R = _rodrigues([0.3, -0.5, 0.81], 0.7) @ _rodrigues([1.0, 0.2, -0.1], -1.1)


def _box(sx, sy, sz, centre=(0.0, 0.0, 0.0)):
    v = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)]) * [sx, sy, sz] + centre
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]
    return v, np.array(f)


def _prism(n, r, h, apex=False):
    """A regular n-gon prism about z (or, apex: the cone over the polygon at z = -h/2 with its apex at z = +h/2)."""
    ang = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([r * np.cos(ang), r * np.sin(ang), np.full(n, -0.5 * h)], 1)
    cap = [(0, k + 1, k) for k in range(1, n - 1)]
    if apex:
        v = np.concatenate([ring, [[0.0, 0.0, 0.5 * h]]])
        side = [(k, (k + 1) % n, n) for k in range(n)]
        return v, np.array(side + cap)
    top = ring + [0.0, 0.0, h]
    v = np.concatenate([ring, top])
    side = [t for k in range(n) for t in ((k, (k + 1) % n, n + (k + 1) % n), (k, n + (k + 1) % n, n + k))]
    return v, np.array(side + cap + [(n + a, n + b, n + c) for a, c, b in cap])


def _join(parts):
    vs, fs, base = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def solid_meshes():
    """name -> (verts float64 [V,3] in millimetres, posed; faces int [F,3]); at most 256 triangles each."""
    raw = dict(box=_box(40.0, 60.0, 100.0), square_prism=_prism(4, 30.0, 100.0), hex_prism=_prism(6, 30.0, 80.0),
               cylinder=_prism(64, 30.0, 100.0), cone=_prism(64, 30.0, 100.0, apex=True),
               handled_cylinder=_join([_prism(32, 30.0, 100.0), _box(30.0, 12.0, 40.0, (40.0, 0.0, 0.0))]),
               cube=_box(50.0, 50.0, 50.0))
    return {k: (v @ POSE_R.T + POSE_T, f) for k, (v, f) in raw.items()}


def _turns(axis, n):
    return [_rodrigues(axis, 2.0 * np.pi * j / n) for j in range(1, n)]


def _dihedral(n, first_az=0.0):
    """The rotations of a regular n-gon prism about z but the identity: n - 1 about z, n half-turns across it."""
    across = [_rodrigues([np.cos(first_az + np.pi * j / n), np.sin(first_az + np.pi * j / n), 0.0], np.pi) for j in range(n)]
    return _turns([0.0, 0.0, 1.0], n) + across


# name -> (discrete rotations in the solid's own frame, continuous axes there, half-turns across a continuous axis, isotropic)
EXPECTED = dict(
    box=([_rodrigues(a, np.pi) for a in np.eye(3)], [], 0, False),
    square_prism=(_dihedral(4), [], 0, False),
    hex_prism=(_dihedral(6), [], 0, False),
    cylinder=([], [np.array([0.0, 0.0, 1.0])], 1, False),
    cone=([], [np.array([0.0, 0.0, 1.0])], 0, False),
    handled_cylinder=([_rodrigues([1.0, 0.0, 0.0], np.pi)], [], 0, False),
)


def check_entry(name, info, angle_deg=0.5):
    """Asserts that the entry `info` detect() returned for solid `name` holds exactly the expected transforms (each about the
    posed solid's centroid line, in millimetres)."""
    disc = [np.asarray(d, dtype=np.float64).reshape(4, 4) for d in info.get("symmetries_discrete", [])]
    cont = info.get("symmetries_continuous", [])
    if name == "cube":
        assert info["report"]["isotropic"] is True
        return
    want, axes, across, iso = EXPECTED[name]
    assert info["report"]["isotropic"] is iso
    assert len(cont) == len(axes), (name, cont)
    ang = lambda Ra, Rb: np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0)))
    for T in disc:
        assert np.allclose(T[3], [0, 0, 0, 1]) and np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-9)
    if axes:
        a = POSE_R @ axes[0]
        got = np.asarray(cont[0]["axis"], dtype=np.float64)
        assert np.degrees(np.arccos(min(1.0, abs(got @ a) / np.linalg.norm(got)))) < angle_deg, (name, got, a)
        assert len(disc) == across, (name, len(disc))
        for T in disc:                       # a half-turn about an axis perpendicular to the continuous one
            assert abs(np.trace(T[:3, :3]) + 1.0) < 1e-6 and np.linalg.norm(T[:3, :3] @ a + a) < 2 * np.radians(angle_deg)
        return
    assert len(disc) == len(want), (name, len(disc), len(want))
    posed = [POSE_R @ S @ POSE_R.T for S in want]
    for T in disc:
        assert min(ang(T[:3, :3], S) for S in posed) < angle_deg, (name, T)
    for S in posed:
        assert min(ang(T[:3, :3], S) for T in disc) < angle_deg, (name, S)


# ---- the crafted queries and the tolerance against float64, shared by both test files -----------------------------------
# |float32 distance - float64 distance| over the largest coordinate magnitude of the configuration: 4 x the largest value
# measured on the inputs of tests/test_symmetry.py::test_restatement_follows_the_float64_distance (2.03e-7, see its docstring)
REL_TOL = 4 * 2.03e-7

T0 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
# name -> (query, squared distance to T0): one query in each of the seven regions, then on a vertex, on an edge, in the face
CRAFTED = {
    "A": ([-0.3, -0.2, 0.5], 0.09 + 0.04 + 0.25), "B": ([1.4, -0.1, 0.3], 0.16 + 0.01 + 0.09), "C": ([-0.1, 1.5, -0.2], 0.01 + 0.25 + 0.04),
    "AB": ([0.4, -0.5, 0.2], 0.25 + 0.04), "AC": ([-0.6, 0.5, 0.1], 0.36 + 0.01), "BC": ([0.8, 0.9, -0.3], 0.245 + 0.09),
    "face": ([0.25, 0.25, 0.4], 0.16), "on_vertex": ([1.0, 0.0, 0.0], 0.0), "on_edge": ([0.5, 0.5, 0.0], 0.0),
    "in_face": ([0.25, 0.5, 0.0], 0.0),
}
TWO = np.stack([T0, T0 + [0.0, 0.0, 1.0]])          # a query at z = 0.5 above T0's inside is equidistant from both
EQUIDISTANT = [0.2, 0.2, 0.5]


def crafted_set(pose=True):
    """(queries float32 [11,3], triangles float32 [2,9], expected squared distances float64 [11]) of the crafted cases against
    the two triangles of TWO, optionally through the oblique pose of the solids (in units of 1, not millimetres)."""
    q = np.array([v[0] for v in CRAFTED.values()] + [EQUIDISTANT])
    want = np.array([v[1] for v in CRAFTED.values()] + [0.25])
    t = TWO.copy()
    if pose:
        q = q @ POSE_R.T + POSE_T / 50.0
        t = t @ POSE_R.T + POSE_T / 50.0
    return q.astype(np.float32), t.reshape(-1, 9).astype(np.float32), want
