"""NumPy restatement of cppf2_amd/csrc/cppf_verify.hip: the peaks and pose hypotheses of cppf_pose_hypotheses (float32 peak
and Gram-Schmidt arithmetic, float64 combination keys) and the pixel counts of cppf_depth_fit_counts (float64 depth
differences).  Each float32 operation is one NumPy float32 operation, in the order the kernel file states."""
import numpy as np

F = np.float32
EMPTY = 1


def _dot(a, b):
    """((a0*b0 + a1*b1) + a2*b2) in float32."""
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def peaks(row, sphere, K, cos_sep):
    """(indices, counts) of up to K peaks of one float32 count row: the first maximum (larger count, then lower index; NaN
    never compares; index 0 when nothing does), then the first maxima over the bins with a count > 0 that are no earlier
    peak and that no earlier peak suppresses (dot >= cos_sep)."""
    row = np.asarray(row, dtype=F)
    sph = np.asarray(sphere, dtype=F)
    x, y, z = sph[:, 0], sph[:, 1], sph[:, 2]
    cos_sep = F(cos_sep)
    idx, cnt = [], []
    ok = ~np.isnan(row)
    for k in range(K):
        if k > 0:
            q = idx[-1]
            d = (x * sph[q, 0] + y * sph[q, 1]) + z * sph[q, 2]          # float32 arrays: one rounding per operation
            ok &= (row > 0) & ~(d >= cos_sep)
            ok[q] = False
        if not ok.any():
            if k > 0:
                break
            idx.append(0)
            cnt.append(F(-np.inf))
            continue
        best = row[ok].max()
        s = int(np.nonzero(ok & (row == best))[0][0])
        idx.append(s)
        cnt.append(row[s])
    return idx, cnt


def pose_from_bins(sphere, up_idx, right_idx, up_axis, right_axis):
    """assemble_pose_kernel's float32 Gram-Schmidt + float64 cross product: float64 [3,3]."""
    sph = np.asarray(sphere, dtype=F)
    u, r = sph[up_idx], sph[right_idx].copy()
    d = _dot(u, r)
    r = np.array([F(r[i] - F(d * u[i])) for i in range(3)], dtype=F)
    n = F(np.sqrt(F(F(F(r[0] * r[0]) + F(r[1] * r[1])) + F(r[2] * r[2]))) + F(1e-9))
    r = np.array([F(r[i] / n) for i in range(3)], dtype=F)
    R = np.eye(3)
    R[:, up_axis] = u.astype(np.float64)
    R[:, right_axis] = r.astype(np.float64)
    o = 3 - up_axis - right_axis
    c1, c2 = (o + 1) % 3, (o + 2) % 3
    R[0, o] = R[1, c1] * R[2, c2] - R[2, c1] * R[1, c2]
    R[1, o] = R[2, c1] * R[0, c2] - R[0, c1] * R[2, c2]
    R[2, o] = R[0, c1] * R[1, c2] - R[1, c1] * R[0, c2]
    return R


def combinations(up, right, sphere, cos_perp):
    """The ordered (i, j) list of one scene: (0, 0), then the others with |u.r| <= cos_perp by descending float64 key, ties by
    (i, j).  up / right: (indices, counts) of peaks()."""
    sph = np.asarray(sphere, dtype=F)
    cos_perp = F(cos_perp)
    rest = []
    for i in range(len(up[0])):
        for j in range(len(right[0])):
            if i == 0 and j == 0:
                continue
            if not abs(_dot(sph[up[0][i]], sph[right[0][j]])) <= cos_perp:
                continue
            key = float(np.float64(up[1][i]) * np.float64(right[1][j]))
            key = -np.inf if key != key else key
            rest.append((-key, i, j))
    rest.sort()
    return [(0, 0)] + [(i, j) for _, i, j in rest]


def hypotheses(counts_up, counts_right, sphere, base, K, H, cos_sep, cos_perp, up_axis, right_axis, y_only=False):
    """cppf_pose_hypotheses: (records [B,H] of base's dtype, peak_idx int32 [B,2,K], peak_count float32 [B,2,K])."""
    cu = np.asarray(counts_up, dtype=F)
    cr = np.asarray(counts_right, dtype=F)
    B = len(base)
    out = np.zeros((B, H), dtype=base.dtype)
    pi = np.full((B, 2, K), -1, dtype=np.int32)
    pc = np.zeros((B, 2, K), dtype=F)
    for b in range(B):
        up = peaks(cu[b], sphere, K, cos_sep)
        right = peaks(cr[b], sphere, 1 if y_only else K, cos_sep)
        for a, (ix, ct) in enumerate((up, right)):
            pi[b, a, :len(ix)] = ix
            pc[b, a, :len(ct)] = ct
        combos = combinations(up, right, sphere, cos_perp)
        for h in range(H):
            r = base[b].copy()
            if h < len(combos):
                i, j = combos[h]
                r["up_idx"], r["right_idx"] = up[0][i], right[0][j]
                r["up_count"], r["right_count"] = up[1][i], right[1][j]
                r["R"] = pose_from_bins(sphere, up[0][i], right[0][j], up_axis, right_axis)
            else:
                r["flags"] |= EMPTY
                r["up_idx"] = r["right_idx"] = -1
                r["up_count"] = r["right_count"] = 0
            out[b, h] = r
    return out, pi, pc


def fit_counts(depth, mask, hyp_off, renders, taus):
    """cppf_depth_fit_counts: int64 [P, 4 + n_taus] = (drawn, observed, violations, unexplained, fit_1 .. fit_n)."""
    depth = np.asarray(depth, dtype=F)
    mask = np.asarray(mask) != 0
    renders = np.asarray(renders, dtype=F)
    taus = np.asarray(taus, dtype=F).astype(np.float64).reshape(-1)
    hyp_off = np.asarray(hyp_off, dtype=np.int64)
    P = len(renders)
    out = np.zeros((P, 4 + len(taus)), dtype=np.int64)
    for i in range(len(hyp_off) - 1):
        do, m = depth[i], mask[i]
        seen = do > 0
        obs = m & seen
        for p in range(hyp_off[i], hyp_off[i + 1]):
            dh = renders[p]
            with np.errstate(invalid="ignore"):          # inf - inf = NaN, which passes no comparison (as in the kernel)
                diff = do.astype(np.float64) - dh.astype(np.float64)
            drawn = dh > 0
            out[p, 0] = np.count_nonzero(drawn)
            out[p, 1] = np.count_nonzero(obs)
            out[p, 2] = np.count_nonzero(drawn & seen & (diff > taus[0]))
            out[p, 3] = np.count_nonzero(obs & (dh == 0))
            both = obs & drawn
            for k, t in enumerate(taus):
                out[p, 4 + k] = np.count_nonzero(both & (np.abs(diff) <= t))
    return out
