"""NumPy restatement of cppf_icp_refine (cppf2_amd/csrc/cppf_icp.hip): the float32 transform and distances element by element in
the kernel's order, the nearest sample by the lowest index, the normal equations, the rank-aware solve (cyclic Jacobi, minimum-norm
step) and the pose update in float64.
One instance per call.  Test infrastructure only."""
import math

import numpy as np

F32 = np.float32
CHUNK = 1024


def schedule(iters, d0, d1):
    """The inlier distances d_k (float32) of the iterations k = 0 .. iters-1, as the host of cppf_icp_refine computes them."""
    d0, d1 = float(F32(d0)), float(F32(d1))
    if iters == 1:
        return [F32(d0)]
    return [F32(d0 * (d1 / d0) ** (k / (iters - 1))) for k in range(iters)]


def model_frame(pts, R, t):
    """q = R^T (p - t) in float32: d = p - (float)t, q.x = (R00*d.x + R10*d.y) + R20*d.z, ..."""
    Rf = np.asarray(R, dtype=np.float64).reshape(9).astype(F32)
    tf = np.asarray(t, dtype=np.float64).astype(F32)
    p = np.asarray(pts, dtype=F32)
    dx, dy, dz = p[:, 0] - tf[0], p[:, 1] - tf[1], p[:, 2] - tf[2]
    qx = (Rf[0] * dx + Rf[3] * dy) + Rf[6] * dz
    qy = (Rf[1] * dx + Rf[4] * dy) + Rf[7] * dz
    qz = (Rf[2] * dx + Rf[5] * dy) + Rf[8] * dz
    return np.stack([qx, qy, qz], -1)


def nearest(q, mp):
    """(index int64 [n] of the nearest model sample, lowest on ties; its squared distance float32 [n])."""
    mp = np.asarray(mp, dtype=F32)
    idx = np.empty(q.shape[0], dtype=np.int64)
    d2 = np.empty(q.shape[0], dtype=F32)
    for a in range(0, q.shape[0], CHUNK):
        qc = q[a:a + CHUNK]
        ex = qc[:, 0:1] - mp[None, :, 0]
        ey = qc[:, 1:2] - mp[None, :, 1]
        ez = qc[:, 2:3] - mp[None, :, 2]
        d = (ex * ex + ey * ey) + ez * ez
        d = np.where(np.isnan(d), F32(np.inf), d)
        i = np.argmin(d, axis=1)
        idx[a:a + CHUNK] = i
        d2[a:a + CHUNK] = d[np.arange(d.shape[0]), i]
    return idx, d2


TAU = 1e-9          # ICP_TAU
JEPS = 1e-17        # ICP_JEPS
SWEEPS = 16         # ICP_SWEEPS


def _min_norm_solve(A, b, qq, cnt):
    """x of A x = -b (6x6) by the kernel's loops: the scale s = (r, r, r, 1, 1, 1), r = 1 / RMS |q| of the inliers, cyclic Jacobi
    of S A S, the pseudo-inverse over the eigenvalues above TAU * lambda_max.  Returns (x, rank)."""
    L2 = qq / cnt
    r = 1.0 / math.sqrt(L2) if L2 > 0.0 else 0.0
    s = [r, r, r, 1.0, 1.0, 1.0]
    a = [[(s[i] * float(A[i, j])) * s[j] for j in range(6)] for i in range(6)]
    V = [[1.0 if i == j else 0.0 for j in range(6)] for i in range(6)]
    for _ in range(SWEEPS):
        rotated = False
        for p in range(5):
            for q in range(p + 1, 6):
                apq, app, aqq = a[p][q], a[p][p], a[q][q]
                if apq == 0.0:
                    continue
                if abs(apq) <= JEPS * (abs(app) + abs(aqq)):
                    a[p][q] = a[q][p] = 0.0
                    continue
                th = (aqq - app) / (2.0 * apq)
                t = (1.0 if th >= 0.0 else -1.0) / (abs(th) + math.sqrt(th * th + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                sn = t * c
                a[p][p] = app - t * apq
                a[q][q] = aqq + t * apq
                a[p][q] = a[q][p] = 0.0
                for k in range(6):
                    if k != p and k != q:
                        akp, akq = a[k][p], a[k][q]
                        a[k][p] = a[p][k] = c * akp - sn * akq
                        a[k][q] = a[q][k] = sn * akp + c * akq
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - sn * vkq
                    V[k][q] = sn * vkp + c * vkq
                rotated = True
        if not rotated:
            break
    lmax = 0.0
    for i in range(6):
        if a[i][i] > lmax:
            lmax = a[i][i]
    y = [0.0] * 6
    rank = 0
    for i in range(6):
        lam = a[i][i]
        if not lam > TAU * lmax:
            continue
        g = 0.0
        for j in range(6):
            g += V[j][i] * (s[j] * float(b[j]))
        f = -g / lam
        for j in range(6):
            y[j] += f * V[j][i]
        rank += 1
    return np.array([s[j] * y[j] for j in range(6)]), rank


def rodrigues(w):
    w0, w1, w2 = (float(v) for v in w)
    th2 = (w0 * w0 + w1 * w1) + w2 * w2
    if th2 < 1e-8:
        a, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        th = np.sqrt(th2)
        a, c = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    K = np.array([[0.0, -w2, w1], [w2, 0.0, -w0], [-w1, w0, 0.0]])
    W = (w0, w1, w2)
    dR = np.empty((3, 3))
    for r in range(3):
        for q in range(3):
            dR[r, q] = ((1.0 - c * th2 if r == q else 0.0) + a * K[r, q]) + (c * W[r]) * W[q]
    return dR


def step(pts, R, t, mp, mn, dk):
    """One iteration at inlier distance dk (float32).  Returns (R, t, inliers, rms, updated): updated when the step is non-zero
    (and finite), which is when the kernel counts the iteration in stats[3]."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    q = model_frame(pts, R, t)
    idx, d2 = nearest(q, mp)
    dk = F32(dk)
    inl = d2 <= dk * dk
    Q = q[inl].astype(np.float64)
    m = np.asarray(mp, dtype=F32)[idx[inl]].astype(np.float64)
    n = np.asarray(mn, dtype=F32)[idx[inl]].astype(np.float64)
    r = Q - m
    e = (n[:, 0] * r[:, 0] + n[:, 1] * r[:, 1]) + n[:, 2] * r[:, 2]
    J = np.stack([Q[:, 1] * n[:, 2] - Q[:, 2] * n[:, 1], Q[:, 2] * n[:, 0] - Q[:, 0] * n[:, 2],
                  Q[:, 0] * n[:, 1] - Q[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]], -1)
    cnt = int(inl.sum())
    sse = float(np.sum(e * e))
    rms = float(F32(np.sqrt(sse / cnt))) if cnt else 0.0
    if cnt < 6:
        return R, t, cnt, rms, False
    qq = float(np.sum((Q[:, 0] * Q[:, 0] + Q[:, 1] * Q[:, 1]) + Q[:, 2] * Q[:, 2]))
    x, rank = _min_norm_solve(J.T @ J, J.T @ e, qq, float(cnt))
    if rank == 0 or not np.any(x != 0.0) or not np.all(np.isfinite(x)):
        return R, t, cnt, rms, False
    dR = rodrigues(x[:3])
    Rn = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            Rn[i, j] = (R[i, 0] * dR[j, 0] + R[i, 1] * dR[j, 1]) + R[i, 2] * dR[j, 2]
    tn = np.array([t[i] - ((Rn[i, 0] * x[3] + Rn[i, 1] * x[4]) + Rn[i, 2] * x[5]) for i in range(3)])
    return Rn, tn, cnt, rms, True


def refine(pts, R, t, mp, mn, iters, d0, d1):
    """iters iterations on the schedule of cppf_icp_refine.  Returns (R, t, stats [4]) like the kernel's record and stats."""
    updates = 0
    cnt, rms = 0, 0.0
    for dk in schedule(iters, d0, d1):
        R, t, cnt, rms, upd = step(pts, R, t, mp, mn, dk)
        updates += int(upd)
    n = len(pts)
    return R, t, np.array([cnt, rms, cnt / n if n else 0.0, updates], dtype=F32)
