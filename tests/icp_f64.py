"""Independent float64 reference of one point-to-plane ICP step (what cppf_icp_refine computes, not how): the transform and the
nearest model sample in float64 (brute force, the lowest index on ties), the normal equations in float64, and the minimum-norm
Gauss-Newton step of the scaled system (rotation unknowns times the inliers' RMS distance from the model origin; numpy.linalg.eigh,
eigenvalues below tau * lambda_max dropped), applied with the exact exponential map.  Also builds the degenerate test models
(plate, open cylinder, sphere cap) as render.Mesh objects.  Test infrastructure only."""
import numpy as np
from scipy.spatial.transform import Rotation

TAU = 1e-9                   # the kernel's ICP_TAU
CHUNK = 512


def model_frame(pts, R, t):
    """q = R^T (p - t), float64."""
    return (np.asarray(pts, dtype=np.float64) - np.asarray(t, dtype=np.float64).reshape(3)) @ \
        np.asarray(R, dtype=np.float64).reshape(3, 3)


def nearest(q, mp):
    """(index int64 [n], squared distance float64 [n]) of the nearest model sample, the lowest index on ties; a point with a
    non-finite coordinate gets index -1 and distance inf."""
    mp = np.asarray(mp, dtype=np.float64)
    idx = np.full(len(q), -1, dtype=np.int64)
    d2 = np.full(len(q), np.inf)
    ok = np.isfinite(q).all(1)
    qi = np.flatnonzero(ok)
    for a in range(0, len(qi), CHUNK):
        sel = qi[a:a + CHUNK]
        d = ((q[sel, None, :] - mp[None]) ** 2).sum(-1)
        i = np.argmin(d, axis=1)                                # first minimum: the lowest index
        idx[sel] = i
        d2[sel] = d[np.arange(len(sel)), i]
    return idx, d2


def normal_equations(pts, R, t, mp, mn, dk):
    """(A 6x6, b 6, sum |q|^2, inlier mask, nearest index) of the point-to-plane terms of the inliers (squared distance <= dk^2):
    e = n . (q - m), J = [q x n, n], A = J^T J, b = J^T e."""
    q = model_frame(pts, R, t)
    idx, d2 = nearest(q, mp)
    inl = d2 <= float(dk) ** 2
    Q = q[inl]
    m = np.asarray(mp, dtype=np.float64)[idx[inl]]
    n = np.asarray(mn, dtype=np.float64)[idx[inl]]
    e = np.einsum("ij,ij->i", n, Q - m)
    J = np.concatenate([np.cross(Q, n), n], 1)
    return J.T @ J, J.T @ e, float((Q * Q).sum()), inl, idx


def scale(qq, cnt):
    """The unknowns' scale S = diag(1/L, 1/L, 1/L, 1, 1, 1), L^2 = sum |q|^2 / inliers: a rotation times the inliers' RMS lever
    arm is a length, like the translation, so S A S has one unit and its eigenvalues do not depend on the model frame's axes.
    (Scaling by diag(A)^-1/2 instead would lift a rounding-level column -- the axis of a cylinder with radial normals -- to
    unit size.)  L = 0: the rotation is unobservable."""
    L2 = qq / cnt if cnt > 0 else 0.0
    r = 1.0 / np.sqrt(L2) if L2 > 0 else 0.0
    return np.array([r, r, r, 1.0, 1.0, 1.0])


def min_norm_step(A, b, s, tau=TAU):
    """(x, rank, eigenvalues of the scaled matrix, ascending): the minimum-norm solution of A x = -b in the scaled unknowns
    y = x / s, over the eigenvectors of S A S whose eigenvalue exceeds tau * lambda_max."""
    As = s[:, None] * A * s[None, :]
    lam, V = np.linalg.eigh(As)
    if not lam[-1] > 0:
        return np.zeros(6), 0, lam
    keep = lam > tau * lam[-1]
    Vk = V[:, keep]
    y = Vk @ ((Vk.T @ (-s * b)) / lam[keep])
    return s * y, int(keep.sum()), lam


def apply(R, t, x):
    """The kernel's update with the exact exponential map: R <- R exp([w]x)^T, t <- t - R v (the new R), x = [w, v]."""
    dR = Rotation.from_rotvec(x[:3]).as_matrix()
    Rn = np.asarray(R, dtype=np.float64).reshape(3, 3) @ dR.T
    return Rn, np.asarray(t, dtype=np.float64).reshape(3) - Rn @ x[3:]


def step(pts, R, t, mp, mn, dk, tau=TAU):
    """One iteration.  Returns (R, t, inliers, x, rank); with fewer than 6 inliers the pose is returned unchanged."""
    A, b, qq, inl, _ = normal_equations(pts, R, t, mp, mn, dk)
    cnt = int(inl.sum())
    if cnt < 6:
        return np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3), cnt, np.zeros(6), 0
    x, rank, _ = min_norm_step(A, b, scale(qq, cnt), tau)
    R, t = apply(R, t, x)
    return R, t, cnt, x, rank


def random_rotation(rng):
    """A uniform rotation: QR of a normal 3x3 with the signs fixed."""
    Q, Rr = np.linalg.qr(rng.standard_normal((3, 3)))
    Q = Q * np.sign(np.diag(Rr))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q


# ---------------------------------------------------------------------------------------------------------------------------
# Degenerate models (render.Mesh; ModelPoints.from_mesh gives each sample its triangle's normal)

def _grid_faces(rows, cols, wrap=False):
    """Two triangles per cell of a rows x cols vertex grid (vertex r * cols + c); wrap joins the last column to the first."""
    f = []
    for r in range(rows - 1):
        for c in range(cols if wrap else cols - 1):
            c1 = (c + 1) % cols
            a, b, d, e = r * cols + c, r * cols + c1, (r + 1) * cols + c, (r + 1) * cols + c1
            f += [(a, b, e), (a, e, d)]
    return np.asarray(f, dtype=np.int32)


def plate(Rm=None, half=0.05, cells=8):
    """A square plate of (cells x cells) quads over +-half in z = 0, turned by Rm (None: left axis-aligned, every normal exactly
    (0, 0, 1)), its vertices rounded to float32."""
    g = np.linspace(-half, half, cells + 1)
    v = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    v = np.concatenate([v, np.zeros((len(v), 1))], 1)
    if Rm is not None:
        v = v @ np.asarray(Rm).T
    from cppf2_amd import render
    return render.Mesh(v.astype(np.float32).astype(np.float64), _grid_faces(cells + 1, cells + 1))


def cylinder(facets=128, r=0.033, h=0.12):
    """An open cylinder (no caps) of `facets` side quads around the z axis."""
    a = 2 * np.pi * np.arange(facets) / facets
    ring = np.stack([r * np.cos(a), r * np.sin(a)], -1)
    v = np.concatenate([np.concatenate([ring, np.full((facets, 1), z)], 1) for z in (-h / 2, h / 2)])
    from cppf2_amd import render
    return render.Mesh(v, _grid_faces(2, facets, wrap=True))


def sphere_cap(r=0.05, cap_deg=60.0, rings=48, segs=192):
    """The cap of a sphere of radius r around +z, polar angle up to cap_deg, with the pole fanned."""
    th = np.deg2rad(cap_deg) * np.arange(1, rings + 1) / rings
    ph = 2 * np.pi * np.arange(segs) / segs
    v = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)),
                  np.outer(np.cos(th), np.ones(segs))], -1).reshape(-1, 3) * r
    v = np.concatenate([[[0.0, 0.0, r]], v])
    f = _grid_faces(rings, segs, wrap=True) + 1
    pole = np.array([(0, 1 + c, 1 + (c + 1) % segs) for c in range(segs)], dtype=np.int32)
    from cppf2_amd import render
    return render.Mesh(v, np.concatenate([pole, f]))


def smooth(model, axis_only=False):
    """The model's samples with the normals of the smooth surface the mesh approximates, radial about the mesh origin (a sphere
    centred there) or, with axis_only, about the z axis (a cylinder along it): rounded to float32 like any normal, they make
    the rotations about the centre (or the axis) unobservable up to rounding."""
    from cppf2_amd import icp
    n = model.pts.astype(np.float64) + model.centre
    if axis_only:
        n[:, 2] = 0.0
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return icp.ModelPoints(model.pts, n, model.centre)
