"""Plain-loop restatements for the BOP dataset layer (cppf2_amd/bop_data.py, cppf_gt_visibility) and the generated test scenes:
ground-truth visibility per pixel in NumPy (the kernel's float64 order, through tests/bop_ref.py's distance factor), the
selection and greedy matching rules of bop_data.score one threshold at a time, and the seeded two-scene dataset both the CPU
precondition check and the GPU tests use.  Test infrastructure only."""
import os

import numpy as np

import bop_ref as BR
import render_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "example_data", "obj_000015.ply")
K = np.array([[591.0125, 0, 320], [0, 590.16775, 240], [0, 0, 1]])
H, W = 480, 640
DELTA = 0.015
OBJ_FIXTURE, OBJ_CYL = 15, 2
THETAS = [round(0.05 * k, 2) for k in range(1, 11)]
MSPD_PX = [5.0 * k for k in range(1, 11)]


# ---------------------------------------------------------------------------------------------
# cppf_gt_visibility
# ---------------------------------------------------------------------------------------------
def gt_visibility(d_test, d_gt, Kmat, delta=DELTA):
    """(counts int64 [3] = (#all, #valid, #visib), bbox int32 [8] = (x, y, w, h) of all, of visib (-1 when empty), mask uint8
    [H,W]) of one instance: d_gt its render alone, d_test its image."""
    dt, dg = np.asarray(d_test, dtype=np.float32), np.asarray(d_gt, dtype=np.float32)
    f = BR.dist_factor(dt.shape[0], dt.shape[1], Kmat)
    Dt, Dg = dt.astype(np.float64) * f, dg.astype(np.float64) * f
    all_ = dg > 0
    valid = all_ & (dt > 0)
    visib = all_ & ((Dg - Dt <= float(delta)) | (dt == 0))
    box = []
    for m in (all_, visib):
        if m.any():
            r, c = np.nonzero(m)
            box += [c.min(), r.min(), c.max() - c.min() + 1, r.max() - r.min() + 1]
        else:
            box += [-1, -1, -1, -1]
    counts = np.array([all_.sum(), valid.sum(), visib.sum()], dtype=np.int64)
    return counts, np.array(box, dtype=np.int32), np.where(visib, 255, 0).astype(np.uint8)


# ---------------------------------------------------------------------------------------------
# bop_data.score's rules, one threshold at a time
# ---------------------------------------------------------------------------------------------
def select(rows, targets):
    """Rule 1.  rows: [(scene, im, obj, score)] in file order; targets: [(scene, im, obj, inst_count)].  Returns ({key: [row
    index] by descending score, ties in file order, at most inst_count}, number of rows that are no target)."""
    want = {(s, i, o): n for s, i, o, n in targets}
    kept, ignored = {}, 0
    for j, (s, i, o, _) in enumerate(rows):
        if (s, i, o) not in want:
            ignored += 1
            continue
        kept.setdefault((s, i, o), []).append(j)
    for key in kept:
        lst = kept[key]
        for a in range(1, len(lst)):                       # insertion sort: stable
            b = a
            while b > 0 and rows[lst[b - 1]][3] < rows[lst[b]][3]:
                lst[b - 1], lst[b] = lst[b], lst[b - 1]
                b -= 1
        kept[key] = lst[:want[key]]
    return kept, ignored


def match_one(err, scores, valid, thr):
    """Rule 4 at one threshold: err [n_est][n_gt], scores [n_est].  Returns [gt index or -1 per estimate]."""
    n_est = len(scores)
    order = list(range(n_est))
    for a in range(1, n_est):
        b = a
        while b > 0 and scores[order[b - 1]] < scores[order[b]]:
            order[b - 1], order[b] = order[b], order[b - 1]
            b -= 1
    taken, out = set(), [-1] * n_est
    for e in order:
        best = None
        for g in range(len(valid)):
            if valid[g] and g not in taken and err[e][g] < thr:
                if best is None or err[e][g] < err[e][best]:
                    best = g
        if best is not None:
            taken.add(best)
            out[e] = best
    return out


def report(tables):
    """Rules 3-5 over tables (bop_data.recall_report's input): dict(matches {vsd [n_taus][n_thetas], mssd, mspd}, targets)
    overall and per object."""
    acc = {}
    for tab in tables:
        n_taus = np.asarray(tab["vsd"]).shape[-1]
        n_est, n_gt = len(tab["score"]), len(tab["valid"])
        vsd = np.asarray(tab["vsd"], dtype=np.float64).reshape(n_est, n_gt, n_taus)
        for key in (tab["obj_id"], None):
            a = acc.setdefault(key, dict(vsd=np.zeros((n_taus, 10), np.int64), mssd=np.zeros(10, np.int64),
                                         mspd=np.zeros(10, np.int64), targets=0))
            a["targets"] += int(np.sum(tab["valid"]))
            for j, th in enumerate(THETAS):
                for k in range(n_taus):
                    a["vsd"][k, j] += sum(g >= 0 for g in match_one(vsd[:, :, k], tab["score"], tab["valid"], th))
                a["mssd"][j] += sum(g >= 0 for g in match_one(tab["mssd"], tab["score"], tab["valid"], th * tab["diameter"]))
                a["mspd"][j] += sum(g >= 0 for g in match_one(tab["mspd"], tab["score"], tab["valid"],
                                                              MSPD_PX[j] * (float(tab["width"]) / 640.0)))
    return acc


# ---------------------------------------------------------------------------------------------
# the generated scenes
# ---------------------------------------------------------------------------------------------
def _outward(v, f):
    """Triangles wound counter-clockwise seen from outside a convex solid centred on the origin."""
    f = np.asarray(f, dtype=np.int32).copy()
    tri = v[f]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    flip = (n * tri.mean(1)).sum(1) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return f


def cylinder(n=64, r=30.0, h=100.0):
    """(verts [2n+2,3], faces) of a closed cylinder about z, centred on the origin, model units (mm)."""
    a = 2 * np.pi * np.arange(n) / n
    ring = np.stack([r * np.cos(a), r * np.sin(a)], -1)
    v = np.concatenate([np.hstack([ring, np.full((n, 1), -h / 2)]), np.hstack([ring, np.full((n, 1), h / 2)]),
                        [[0, 0, -h / 2], [0, 0, h / 2]]])
    f = []
    for i in range(n):
        j = (i + 1) % n
        f += [(i, j, n + i), (j, n + j, n + i), (2 * n, i, j), (2 * n + 1, n + i, n + j)]
    return v, _outward(v, f)


CYL_INFO = {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}


def box(half=(0.13, 0.13, 0.02)):
    """(verts, faces) of the occluder, metres."""
    v, f = RR.cube(1.0)
    return v * np.asarray(half), f


def _pose(rng, t):
    return RR.random_rotation(rng), np.asarray(t, dtype=np.float64)


def scenes(seed=7):
    """The two generated scenes: (scenes, occluders, holes) in bop_data.write_dataset's form (occluder meshes as (verts, faces),
    metres, for the caller to wrap).  Contents by design, asserted by the tests on the restatement's output:
      scene 0 image 0: the fixture and the cylinder, both fully visible;
      scene 0 image 1: the fixture hidden behind the box (visib_fract < 0.1), the cylinder visible;
      scene 0 image 2: the fixture partly behind the box (0.3 .. 0.9);
      scene 1 image 0: two fixtures (inst_count = 2) and a cylinder cut by the right image border;
      scene 1 image 1: the fixture with 5 % seeded depth holes (px_count_valid < px_count_all) and a cylinder."""
    rng = np.random.default_rng(seed)
    flat = np.eye(3)                                             # the box faces the camera
    s0 = [[(OBJ_FIXTURE,) + _pose(rng, (-0.12, 0.02, 0.80)), (OBJ_CYL,) + _pose(rng, (0.20, -0.05, 0.70))],
          [(OBJ_FIXTURE,) + _pose(rng, (-0.10, 0.00, 0.90)), (OBJ_CYL,) + _pose(rng, (0.22, 0.08, 0.80))],
          [(OBJ_FIXTURE,) + _pose(rng, (0.05, 0.03, 0.85))]]
    s1 = [[(OBJ_FIXTURE,) + _pose(rng, (-0.18, -0.06, 0.90)), (OBJ_FIXTURE,) + _pose(rng, (0.10, 0.08, 1.00)),
           (OBJ_CYL,) + _pose(rng, (0.425, -0.10, 0.80))],
          [(OBJ_FIXTURE,) + _pose(rng, (0.00, 0.00, 0.75)), (OBJ_CYL,) + _pose(rng, (-0.20, 0.10, 0.90))]]
    occluders = {(0, 1): [(box((0.16, 0.16, 0.02)), flat, np.array([-0.07, 0.0, 0.60]))],
                 (0, 2): [(box(), flat, np.array([0.165, 0.03, 0.60]))]}
    holes = {(1, 1): np.random.default_rng(seed + 1).random((H, W)) < 0.05}
    return [s0, s1], occluders, holes


def render_alone(verts, faces, R, t):
    """tests/render_ref.py's render of one centred mesh (metres) under a record-convention pose: float32 [H,W]."""
    return RR.render(np.asarray(verts, dtype=np.float32), faces, RR.look_pose(R, t), K, H, W)[0]


def check_cases(scenes, info):
    """The cases the scenes were built for, asserted on visibility figures (a scene that stops exercising one fails here).
    info: {(scene, image): [(counts (#all, #valid, #visib), bbox [8]) per instance]}."""
    fract = {k: [c[2] / max(c[0], 1) for c, _ in v] for k, v in info.items()}
    assert info[(0, 1)][0][0][0] > 1000 and fract[(0, 1)][0] < 0.1                        # hidden behind the box
    assert 0.3 < fract[(0, 2)][0] < 0.9                                                   # partly occluded
    c, b = info[(1, 0)][2]
    assert c[0] > 500 and b[0] + b[2] == W and fract[(1, 0)][2] == 1.0                 # cut by the right border
    assert fract[(0, 0)] == [1.0, 1.0] and all(b[0] > 0 and b[0] + b[2] < W for _, b in info[(0, 0)])    # fully visible
    assert [o for o, _, _ in scenes[1][0]].count(OBJ_FIXTURE) == 2 and min(fract[(1, 0)][:2]) >= 0.1     # inst_count = 2
    c = info[(1, 1)][0][0]
    assert c[1] < c[0] and c[2] == c[0]                                                   # holes: valid < all, still visible
