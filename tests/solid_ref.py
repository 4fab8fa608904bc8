"""Restatement of cppf_support_counts and cppf_solid_overlap (cppf2_amd/csrc/cppf_solid.hip) in NumPy, one
operation per step, and of the constrained greedy selection that scene.explain_candidates(solid=True) builds from them.  Every
output is an integer count, so the GPU outputs must equal these byte for byte."""
import numpy as np

import scene_ref as SC

F = np.float32
MAX_C = 64


def reversed_faces(faces):
    """Every triangle's second and third index swapped: with cull = 1 the rasteriser then draws the nearest BACK face."""
    return np.ascontiguousarray(np.asarray(faces)[:, [0, 2, 1]])


def predicates(f, b):
    """(back, solid, open) bool of the renders f (back faces culled) and b (reversed winding), float32 of one shape.  Comparisons
    with 0 in float32: NaN compares false, -0.0 is not > 0, +inf is."""
    f, b = np.asarray(f, dtype=F), np.asarray(b, dtype=F)
    with np.errstate(invalid="ignore"):
        isf = f > F(0)
        isb = b > F(0)
    return isb, isf & isb, isf != isb


def height(b, plane, kmat):
    """float32 [...,H,W]: the height h above plane (n, d) of the point that depth b [...,H,W] puts on the ray of each pixel's
    centre (the renderer's: column + 0.5, row + 0.5), every operation a float32 one, rounded where it is written."""
    b = np.asarray(b, dtype=F)
    H, W = b.shape[-2:]
    nx, ny, nz, d = (F(v) for v in np.asarray(plane, dtype=F).reshape(4))
    fx, fy, cx, cy = (F(v) for v in np.asarray(kmat, dtype=F).reshape(4))
    with np.errstate(all="ignore"):
        rx = (np.arange(W, dtype=F) + F(0.5)) - cx
        ry = (np.arange(H, dtype=F) + F(0.5)) - cy
        x = (rx[None, :] * b) / fx
        y = (ry[:, None] * b) / fy
        h = ((nx * x + ny * y) + nz * b) + d
    assert h.dtype == F
    return h


def support_image(f, b, plane, kmat, tau):
    """int64 [C,4] = (back, sunk, solid, open) of one image's candidates f, b float32 [C,H,W]; sunk = back && h < -tau."""
    f, b = np.asarray(f, dtype=F), np.asarray(b, dtype=F)
    C, npx = f.shape[0], f.shape[-2] * f.shape[-1]
    back, solid, opn = predicates(f, b)
    with np.errstate(invalid="ignore"):
        sunk = back & (height(b, plane, kmat) < -F(tau))
    return np.stack([back.reshape(C, npx).sum(1), sunk.reshape(C, npx).sum(1), solid.reshape(C, npx).sum(1),
                     opn.reshape(C, npx).sum(1)], 1).astype(np.int64).reshape(C, 4)


def support(front, back, cand_off, planes, kmat, tau):
    """The batch: int64 [P,4]; image i has the renders cand_off[i] .. cand_off[i+1]-1, planes [I,4], kmat [I,4]."""
    planes, kmat = np.asarray(planes, dtype=F).reshape(-1, 4), np.asarray(kmat, dtype=F).reshape(-1, 4)
    per = [support_image(front[cand_off[i]:cand_off[i + 1]], back[cand_off[i]:cand_off[i + 1]], planes[i], kmat[i], tau)
           for i in range(len(cand_off) - 1)]
    return np.concatenate(per + [np.zeros((0, 4), np.int64)]).reshape(-1, 4)


def sunk_share(counts):
    """float64 [P]: sunk / back, 0 where back == 0."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    return np.where(c[:, 0] > 0, c[:, 1].astype(np.float64) / np.maximum(c[:, 0], 1).astype(np.float64), 0.0)


def overlap_image(f, b, tau):
    """int64 [C,64] of one image's C <= 64 candidates: [a, j] = the pixels where both are solid and
    (double)fmin(b_a, b_j) - (double)fmax(f_a, f_j) > (double)tau; the diagonal = solid_a; columns C .. 63 are 0."""
    f, b = np.asarray(f, dtype=F), np.asarray(b, dtype=F)
    C = f.shape[0]
    assert C <= MAX_C
    npx = f.shape[-2] * f.shape[-1]
    f, b = f.reshape(C, npx), b.reshape(C, npx)
    _, solid, _ = predicates(f, b)
    inter = np.zeros((C, MAX_C), np.int64)
    inter[np.arange(C), np.arange(C)] = solid.sum(1)
    tau_d = np.float64(F(tau))
    for a in range(C):
        for c in range(a + 1, C):
            at = np.flatnonzero(solid[a] & solid[c])      # the pixels where both are solid
            if at.size == 0:
                continue
            lo = np.fmax(f[a, at], f[c, at])
            hi = np.fmin(b[a, at], b[c, at])
            with np.errstate(invalid="ignore"):           # inf - inf: NaN, which is not > tau
                n = int((hi.astype(np.float64) - lo.astype(np.float64) > tau_d).sum())
            inter[a, c] = inter[c, a] = n
    return inter


def overlap(front, back, cand_off, tau):
    per = [overlap_image(front[cand_off[i]:cand_off[i + 1]], back[cand_off[i]:cand_off[i + 1]], tau)
           for i in range(len(cand_off) - 1)]
    return np.concatenate(per + [np.zeros((0, MAX_C), np.int64)]).reshape(-1, MAX_C)


def conflicts(inter, max_overlap):
    """bool [C,C] of one image's inter [C,64]: a and c conflict iff inter > max_overlap * min(solid_a, solid_c) in float64
    (never a candidate with itself)."""
    inter = np.asarray(inter, dtype=np.int64)
    C = inter.shape[0]
    sq = inter[:, :C]
    solid = np.diagonal(sq).astype(np.float64)
    out = sq.astype(np.float64) > np.float64(max_overlap) * np.minimum(solid[:, None], solid[None, :])
    out[np.arange(C), np.arange(C)] = False
    return out


def greedy_direct(d_o, m, d_c, tau, min_gain, viol_weight, max_rounds, conflict):
    """Section 22's greedy rounds with one more rule: a candidate is ineligible once it conflicts with an earlier winner.
    Returns (chosen [n], gain [n], net [n])."""
    d_o = np.asarray(d_o, dtype=F)
    drawn, fit, viol = SC.predicates(d_o, m, d_c, tau)
    C = fit.shape[0]
    fit, viol_n = fit.reshape(C, -1), viol.reshape(C, -1).sum(1).astype(np.int64)
    unexplained = np.ones(d_o.size, dtype=bool)
    taken = np.zeros(C, dtype=bool)
    barred = np.zeros(C, dtype=bool)
    chosen, gain, net = [], [], []
    for _ in range(int(max_rounds)):
        g = (fit & unexplained[None]).sum(1).astype(np.int64)
        n = g - np.int64(viol_weight) * viol_n
        eligible = ~taken & ~barred & (n >= np.int64(min_gain))
        if not eligible.any():
            break
        w = max(((int(n[c]) << 32) | (0xFFFFFFFF - c)) for c in range(C) if eligible[c])
        w = 0xFFFFFFFF - (w & 0xFFFFFFFF)
        chosen.append(w), gain.append(int(g[w])), net.append(int(n[w]))
        unexplained &= ~fit[w]
        taken[w] = True
        barred |= np.asarray(conflict)[w] & ~taken
    return chosen, gain, net


def greedy_loop(d_o, m, d_c, tau, min_gain, viol_weight, max_rounds, conflict):
    """The same selection from the unchanged explanation: run it, find the first chosen candidate (in chosen order) that conflicts
    with an earlier one, drop it from the list, run again; stop when no chosen pair conflicts.  Dropping a non-winner changes no
    earlier round, so every pass repeats the prefix and the result is greedy_direct's.  Returns (chosen, gain, net, refused
    [(candidate, the earlier winner it conflicts with)], passes)."""
    d_c = np.asarray(d_c, dtype=F)
    conflict = np.asarray(conflict, dtype=bool)
    alive = list(range(d_c.shape[0]))
    refused, passes = [], 0
    while True:
        passes += 1
        r = SC.explain_image(d_o, m, d_c[alive], tau, min_gain, viol_weight, max_rounds)
        n = int(r["summary"][2])
        pick = [alive[k] for k in r["chosen"][:n]]
        bad = next(((k, e) for k in range(n) for e in range(k) if conflict[pick[k], pick[e]]), None)
        if bad is None:
            return pick, r["gain"][:n].tolist(), r["net"][:n].tolist(), refused, passes
        refused.append((pick[bad[0]], pick[bad[1]]))
        alive.remove(pick[bad[0]])
