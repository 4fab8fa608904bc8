"""NumPy restatement of the BOP scorer (cppf2_amd/csrc/cppf_bop.hip, cppf2_amd/bop.py): VSD counts in float64 in the kernel's
order of operations, MSSD and MSPD in float64, the symmetry expansion of a models_info entry, and the average recall.
Test infrastructure only."""
import numpy as np


def dist_factor(H, W, K):
    """f [H,W] = sqrt((x*x + y*y) + 1), x = (c - cx) / fx, y = (r - cy) / fy (float64)."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    c = np.arange(W, dtype=np.float64)[None, :]
    r = np.arange(H, dtype=np.float64)[:, None]
    x = (c - K[0, 2]) / K[0, 0]
    y = (r - K[1, 2]) / K[1, 1]
    return np.sqrt((x * x + y * y) + 1.0)


def vsd_counts(d_test, d_est, d_gt, K, delta, diameter, taus, near=0.0):
    """(counts int64 [2 + n_taus], near) of one pair: union, intersection, cost_k; `near` = the number of intersection pixels
    whose |D_g - D_e| lies within a relative `near` of some threshold (0 = not checked)."""
    dt, de, dg = (np.asarray(a, dtype=np.float32) for a in (d_test, d_est, d_gt))
    f = dist_factor(dt.shape[0], dt.shape[1], K)
    Dt, De, Dg = dt.astype(np.float64) * f, de.astype(np.float64) * f, dg.astype(np.float64) * f
    delta = float(delta)
    with np.errstate(invalid="ignore"):                  # inf - inf = NaN, which passes no comparison (as in the kernel)
        vg = (dg > 0) & ((Dg - Dt <= delta) | (dt == 0))
        ve = ((de > 0) & ((De - Dt <= delta) | (dt == 0))) | (vg & (de > 0))
        inter = vg & ve
        diff = np.abs(Dg - De)
    thr = np.asarray(taus, dtype=np.float32).astype(np.float64) * float(np.float32(diameter))
    out = [int(np.count_nonzero(vg | ve)), int(np.count_nonzero(inter))]
    close = 0
    for t in thr:
        out.append(int(np.count_nonzero(inter & (diff >= t))))
        if near:
            with np.errstate(invalid="ignore"):
                close += int(np.count_nonzero(inter & (np.abs(diff - t) <= near * t)))
    return np.array(out, dtype=np.int64), close


def vsd_errors(counts):
    c = np.asarray(counts, dtype=np.int64)
    u, i = c[..., :1], c[..., 1:2]
    num = (c[..., 2:] + u - i).astype(np.float64)
    return np.where(u > 0, num / np.maximum(u, 1), 1.0)


def mssd_mspd(verts, syms, pe, pg, K):
    """(mssd, mspd) of one pair in float64: min over s of max over v; +inf for an s with a vertex at p_z <= 0 in either pose."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    S = np.asarray(syms, dtype=np.float64).reshape(-1, 3, 4)
    pe = np.asarray(pe, dtype=np.float64).reshape(3, 4)
    pg = np.asarray(pg, dtype=np.float64).reshape(3, 4)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    e = v @ pe[:, :3].T + pe[:, 3]
    best_d = best_p = np.inf
    for s in S:
        q = (v @ s[:, :3].T + s[:, 3]) @ pg[:, :3].T + pg[:, 3]
        best_d = min(best_d, float(np.sqrt(np.max(np.sum((e - q) ** 2, 1)))))
        if (e[:, 2] > 0).all() and (q[:, 2] > 0).all():
            du = K[0, 0] * (e[:, 0] / e[:, 2] - q[:, 0] / q[:, 2])
            dv = K[1, 1] * (e[:, 1] / e[:, 2] - q[:, 1] / q[:, 2])
            best_p = min(best_p, float(np.sqrt(np.max(du * du + dv * dv))))
    return best_d, best_p


def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    c, s = np.cos(angle), np.sin(angle)
    x, y, z = a
    return np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                     [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                     [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]])


def symmetries(info, scale, centre, n=315):
    """The symmetry set as 4x4 maps of the centred metre frame: T_c^-1 . S . T_scaled, composed as matrices."""
    Sc = np.diag([scale, scale, scale, 1.0])
    Tc = np.eye(4)
    Tc[:3, 3] = -np.asarray(centre, dtype=np.float64)
    to_frame = lambda M: Tc @ Sc @ M @ np.linalg.inv(Sc) @ np.linalg.inv(Tc)      # noqa: E731
    disc = [np.eye(4)] + [np.asarray(d, dtype=np.float64).reshape(4, 4) for d in info.get("symmetries_discrete", [])]
    cont = []
    for sym in info.get("symmetries_continuous", []):
        o = np.asarray(sym["offset"], dtype=np.float64)
        for i in range(n):
            M = np.eye(4)
            M[:3, :3] = rotation(sym["axis"], 2 * np.pi * i / n)
            M[:3, 3] = o - M[:3, :3] @ o
            cont.append(M)
    mats = [C_ @ D for D in disc for C_ in cont] if cont else disc
    return np.stack([to_frame(M)[:3] for M in mats])


def average_recall(vsd, mssd, mspd, diameter, width):
    th = np.arange(1, 11) * 0.05
    r_vsd = np.mean([[np.mean(np.asarray(vsd)[:, k] < t) for t in th] for k in range(np.asarray(vsd).shape[1])])
    r_mssd = np.mean([np.mean(np.asarray(mssd) < t * diameter) for t in th])
    r_mspd = np.mean([np.mean(np.asarray(mspd) < t * width / 640.0) for t in np.arange(1, 11) * 5.0])
    return dict(AR_VSD=r_vsd, AR_MSSD=r_mssd, AR_MSPD=r_mspd, AR=(r_vsd + r_mssd + r_mspd) / 3)
