"""Plain NumPy reference of the back-vote filter (eval.py:251-275; cppf_backvote_filter) and the inputs that take it through
the paths random scenes never reach: ties at the order statistic, exact-zero errors, gamma == 0 / 0.5, scenes of 1 and 2 tuples,
tuple and kept counts around the kernel's workgroup size, a hit histogram with thousands of hits per point, degenerate pairs
among the kept ones and empty scenes.

Needs neither the built library nor a GPU (no cppf2_amd.ops import).  The expected values are the oracle's
(oracle.cppf_oracle.backvote_filter: np.percentile on the float32 errors) plus what the kernel returns and the oracle does not:
the ordered kept list and each kept pair's first row in vote_rotation's compacted candidate list.  tests/test_backvote_ref.py
checks on the CPU that every case reaches the edge it is named for; tests/test_backvote_gpu.py holds the kernel to reference().

Ties are made without computing an error on the host: a scene's tuples are draws from a small pool of (indices, target) rows, so
equal rows give bit-equal errors on any implementation, and a target set to the oracle's own back-projection gives an exact 0.
"""
import collections
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import cppf_oracle as O  # noqa: E402

F32, F64 = np.float32, np.float64
BV_THREADS = 1024           # cppf_common.h: the workgroup of backvote_kernel; its compaction loops advance by this many
N_POINTS = 40               # points per scene, in a 0.2 m box
K = 5                       # indices per tuple (the filter reads the first two)
MARGIN = 0.01               # imp_wt_margin (eval.py:275)
# (up, right, front) of config/config.yaml and of config/category/camera.yaml
AXES = {"default": ([0, 1, 0], [1, 0, 0], [0, 0, 1]), "camera": ([0, 1, 0], [0, 0, 1], [1, 0, 0])}


def percentile_params(n, ratio):
    """(kq, gamma) of np.percentile(x_f32[n], ratio * 100), method 'linear', in the NumPy 2.x arithmetic that
    cppf2_amd.ops.percentile_params documents: q = (ratio * 100) / f32(100) in float32; virtual = (n - 1) * q in float32;
    kq = floor(virtual); gamma = f32(virtual - kq); an index at or past the last element is clamped to (n - 1, 0).  Only used to
    assert that a case reaches its edge and to cross-check the product's own function -- never for an expected output."""
    q = np.asanyarray(np.true_divide(ratio * 100, F32(100)))
    virt = np.asanyarray((n - 1) * q)
    prev = np.floor(virt)
    k = int(prev)
    gamma = np.asanyarray(virt - prev.astype(np.intp), dtype=virt.dtype)
    if k >= n - 1:
        return max(n - 1, 0), 0.0
    return k, float(gamma)


# T tuples drawn from a pool of P rows (P == T: each row once, no ties); `exact`: fraction of the pool whose target is the exact
# back-projection (error 0); `degenerate`: pool rows with i1 = i0; `coincident`: one more pool row whose two indices name two
# points with the same coordinates; `npts`: the pool's indices come from the first npts points (few points: many hits each);
# `edges`: names in EDGES, asserted on the reference's numbers.
Case = collections.namedtuple("Case", "name T P ratio seed exact degenerate coincident npts edges")


def _c(name, T, P, ratio, seed, edges, exact=0.0, degenerate=0, coincident=False, npts=N_POINTS):
    return Case(name, T, P, ratio, seed, exact, degenerate, coincident, npts, tuple(edges))


def _kept_is(n):
    return lambda r: r["kept"] == n


def _gamma_near(g):
    return lambda r: abs(r["gamma"] - g) < 1e-3


def _degenerate_kept(r):
    """Hundreds of kept pairs with i0 == i1, in more than one BV_THREADS chunk of the kept list, valid pairs after them (so a rank
    that counted them would show), and some point hit thousands of times."""
    i = r["idx"][r["kept_tuple"]]
    same = np.flatnonzero(i[:, 0] == i[:, 1])
    valid = r["kept_row0"] >= 0
    return (len(same) >= 200 and r["kept"] > 2 * BV_THREADS and len(np.unique(same // BV_THREADS)) >= 2
            and np.all(r["kept_row0"][same] == -1) and valid[same[0]:].sum() > BV_THREADS and r["hits"].max() >= 2000)


def _coincident_kept(r):
    i = r["idx"][r["kept_tuple"]]
    return bool(np.any((i[:, 0] != i[:, 1]) & (r["kept_row0"] == -1)))


# name -> predicate on reference()'s dictionary: s = the sorted errors, kq / gamma = percentile_params, kept = mask.sum()
EDGES = {
    "kq0": lambda r: r["kq"] == 0,
    "no_next": lambda r: r["kq"] + 1 > r["T"] - 1,                                  # there is no kq + 1
    "gamma0": lambda r: r["gamma"] == 0.0,
    "gamma0.1f": lambda r: F32(r["gamma"]) == F32(0.1),
    "gamma0.5": lambda r: r["gamma"] == 0.5,                                        # the second _lerp form, exactly at its switch
    "gamma>0.5": lambda r: r["gamma"] > 0.5,
    "gamma0.7": _gamma_near(0.7),
    "gamma0.8": _gamma_near(0.8),
    "kept0": _kept_is(0),
    "kept1": _kept_is(1),
    "kept==kq": lambda r: r["kept"] == r["kq"] > 0,
    "kept==kq+1": lambda r: r["kept"] == r["kq"] + 1,
    "kept<kq": lambda r: r["kept"] < r["kq"],
    "kept==T-1": lambda r: r["kept"] == r["T"] - 1,
    "kept1023": _kept_is(BV_THREADS - 1),
    "kept1024": _kept_is(BV_THREADS),
    "kept1025": _kept_is(BV_THREADS + 1),
    "kept>1024": lambda r: r["kept"] > BV_THREADS,                                  # the weight loop crosses a chunk
    "kept>2048": lambda r: r["kept"] > 2 * BV_THREADS,
    "tie": lambda r: r["s"][r["kq"]] == r["s"][r["kq"] + 1],                        # v_hi = v_lo: no search for the next value
    "no_tie": lambda r: r["n_le"] == r["kq"] + 1 and r["s"][r["kq"]] < r["s"][r["kq"] + 1],
    "clamped": lambda r: r["kq"] == r["T"] - 1,
    "thr==min": lambda r: r["thr"] == r["s"][0] and r["T"] > 1,
    "thr==0": lambda r: r["thr"] == 0.0 and (r["errs"] == 0).sum() > r["kq"] and (r["errs"] == 0).sum() >= 100,
    "T<1024": lambda r: r["T"] < BV_THREADS,
    "T==1024": lambda r: r["T"] == BV_THREADS,
    "T>1024": lambda r: r["T"] > BV_THREADS,
    "degenerate": _degenerate_kept,
    "coincident": _coincident_kept,
    "empty": lambda r: r["T"] == 0 and r["kept"] == 0 and np.isnan(r["thr"]),
}

# The issue's table, one scene per row.  The empty scene sits between two full ones.
CASES = [
    _c("t1", 1, 1, 0.1, 1, ["kq0", "no_next", "kept0"]),
    _c("t2", 2, 2, 0.1, 2, ["kq0", "gamma0.1f", "kept1"]),
    _c("t11", 11, 11, 0.1, 3, ["gamma0", "no_tie", "kept==kq"]),
    _c("t21", 21, 21, 0.1, 4, ["gamma0", "no_tie", "kept==kq"]),
    _c("t16_r0.5", 16, 16, 0.5, 5, ["gamma0.5", "no_tie", "kept==kq+1"]),
    _c("t16_r0.3", 16, 16, 0.3, 6, ["gamma0.5", "no_tie", "kept==kq+1"]),
    _c("t7_r0.3", 7, 7, 0.3, 7, ["gamma>0.5", "no_tie", "kept==kq+1"]),
    _c("t1023_p50", 1023, 50, 0.1, 8, ["tie", "T<1024"]),
    _c("t1024_p50", 1024, 50, 0.1, 9, ["tie", "T==1024"]),
    _c("t1025_p50_r0.3", 1025, 50, 0.3, 30, ["tie", "T>1024"]),
    _c("t2048", 2048, 2048, 0.1, 11, ["no_tie", "gamma0.7", "kept==kq+1"]),
    _c("t2049", 2049, 2049, 0.1, 12, ["no_tie", "gamma0.8", "kept==kq+1"]),
    _c("heavy_tie", 3000, 20, 0.1, 13, ["tie", "kept<kq"]),
    _c("t3000_p200_r0.5", 3000, 200, 0.5, 14, ["kept>1024"]),
    _c("ratio1", 3000, 3000, 1.0, 15, ["clamped", "gamma0", "kept==T-1"]),
    _c("empty", 0, 0, 0.1, 16, ["empty"]),
    _c("ratio0", 3000, 3000, 0.0, 17, ["kq0", "gamma0", "thr==min", "kept0"]),
    _c("thr_zero", 2500, 100, 0.1, 18, ["thr==0", "kept0"], exact=0.3),
    _c("degenerate", 5000, 7, 0.999, 19, ["degenerate", "coincident", "kept>2048"], degenerate=1, coincident=True, npts=4),
    _c("t4097", 4097, 4097, 0.1, 20, ["no_tie", "kept==kq+1"]),
    # kept counts around BV_THREADS: no ties, ratio 0.5 and an even T give gamma = 0.5 and kept = kq + 1 = T / 2
    _c("kept1023", 2046, 2046, 0.5, 21, ["no_tie", "gamma0.5", "kept1023"]),
    _c("kept1024", 2048, 2048, 0.5, 22, ["no_tie", "gamma0.5", "kept1024"]),
    _c("kept1025", 2050, 2050, 0.5, 23, ["no_tie", "gamma0.5", "kept1025"]),
]
LONE = ("heavy_tie", "thr_zero")            # launched again as B = 1

# name -> (cases, axes, num_rots).  "table": every row, 64 x B grid of backvote_errs_kernel.  "b33": the rows plus repeats with
# other seeds (compared with the reference like the rows; their edges are not asserted), B >= 32: the 16 x B grid.  "camera":
# another category's axes (they reach the kernel and must not change anything: the filter reads the translation targets only)
# and num_rots = 180, which only scales kept_row0.
_BY_NAME = {c.name: c for c in CASES}
_REPEAT = ["t1025_p50_r0.3", "heavy_tie", "thr_zero", "degenerate", "t16_r0.5", "t2049", "empty", "t11", "kept1024", "t2"]
BATCHES = {
    "table": (CASES, "default", 36),
    "b33": (CASES + [_BY_NAME[n]._replace(name=n + "_again", seed=_BY_NAME[n].seed + 100, edges=()) for n in _REPEAT], "default", 36),
    "camera": ([_BY_NAME[n] for n in ("t16_r0.3", "t1024_p50", "empty", "heavy_tie", "thr_zero", "degenerate", "kept1025", "t1")],
               "camera", 180),
}


def build_scene(case, axes="default"):
    """The inputs of one scene: pc float32 [N_POINTS, 3], centre float64 [3] (the voted centre), idx int32 [T, K],
    tr float32 [T, 2] (the translation targets the filter back-projects against)."""
    up, right, front = AXES[axes]
    rng = np.random.RandomState(1000 + case.seed)
    pc = (rng.rand(N_POINTS, 3) * 0.2).astype(F32)
    if case.coincident:
        pc[N_POINTS - 1] = pc[0]
    centre = pc.astype(F64).mean(0) + rng.randn(3) * 0.01
    if case.T == 0:
        return dict(pc=pc, centre=centre, idx=np.zeros((0, K), np.int32), tr=np.zeros((0, 2), F32))
    pool = np.zeros((0, K), np.int64)
    while len(pool) < case.P:                                    # P distinct rows
        pool = np.unique(np.concatenate([pool, rng.randint(0, case.npts, (2 * case.P + 8, K))]), axis=0)
    pool = pool[rng.permutation(len(pool))[:case.P]]
    pool[:case.degenerate, 1] = pool[:case.degenerate, 0]        # i0 == i1
    if case.coincident:
        pool[case.degenerate, :2] = (0, N_POINTS - 1)            # two indices, one position
    assert len(np.unique(pool, axis=0)) == case.P
    # the reference hands (up, front, right) to generate_target_pairs(point_pairs, up, right, front): eval.py:252-256
    tb = O.generate_target_pairs(pc[pool[:, :2]], up, front, right, centre)[0]
    tr_pool = (tb + 0.01 * rng.randn(case.P, 2)).astype(F32)
    n_exact = int(round(case.exact * case.P))
    if n_exact:
        tr_pool[case.P - n_exact:] = tb[case.P - n_exact:]       # error exactly 0
    draw = rng.permutation(case.P) if case.P == case.T else rng.randint(0, case.P, case.T)
    return dict(pc=pc, centre=centre, idx=np.ascontiguousarray(pool[draw]).astype(np.int32), tr=np.ascontiguousarray(tr_pool[draw]))


def reference(scene, ratio, num_rots, axes="default", margin=MARGIN):
    """What cppf_backvote_filter must return for one scene, and the numbers the edge predicates read.
    back_errs float32 [T], thr float32, mask bool [T], kept_tuple int32 [kept] (ascending), kept_wt float64 [kept],
    kept_row0 int32 [kept]; hits int64 [N] (the un-normalised histogram), kq, gamma, s (sorted errors), n_le, kept, T, idx."""
    up, right, front = AXES[axes]
    pc, idx, T = scene["pc"], scene["idx"], len(scene["idx"])
    if T == 0:                                                   # the oracle has no answer for an empty scene; the kernel's contract:
        return dict(back_errs=np.zeros(0, F32), thr=F32(np.nan), mask=np.zeros(0, bool), kept_tuple=np.zeros(0, np.int32),
                    kept_wt=np.zeros(0, F64), kept_row0=np.zeros(0, np.int32), hits=np.zeros(len(pc), np.int64), kq=0, gamma=0.0,
                    s=np.zeros(0, F32), n_le=0, kept=0, T=0, idx=idx, errs=np.zeros(0, F32))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)         # an empty mask: the oracle's imp_wt is 0 / 0
        mask, _, wt, errs, thr = O.backvote_filter(pc, idx, scene["tr"], up, front, right, scene["centre"], ratio, margin)
    assert errs.dtype == F32 and np.asarray(thr).dtype == F32 and wt.dtype == F64
    if not mask.any():
        wt = np.zeros(0, F64)
    kept_tuple = np.flatnonzero(mask).astype(np.int32)
    # vote_rotation's mask rule on the kept pairs (train_dino.py:223): float32 pair length > 1e-7
    valid = O._pair_frame(pc, idx[kept_tuple][:, :2].astype(np.int64))[2] > F32(1e-7)
    before = np.cumsum(valid) - valid                            # valid pairs before j
    kept_row0 = np.where(valid, before * num_rots, -1).astype(np.int32)
    kq, gamma = percentile_params(T, ratio)
    s = np.sort(errs)
    return dict(back_errs=errs, errs=errs, thr=F32(thr), mask=mask, kept_tuple=kept_tuple, kept_wt=wt, kept_row0=kept_row0,
                hits=np.bincount(idx[mask, :2].reshape(-1), minlength=len(pc)), kq=kq, gamma=gamma, s=s,
                n_le=int((errs <= s[kq]).sum()), kept=int(mask.sum()), T=T, idx=idx)


def failed_edges(case, ref):
    """The names among case.edges whose predicate does not hold on the reference's numbers."""
    return [e for e in case.edges if not EDGES[e](ref)]


def build_batch(name):
    """One launch: (cases, scenes, references, num_rots, axes name, arrays) with the arrays in the entry point's batch layout --
    pts float32 [sum N, 3], pt_off / tup_off int32 [B + 1], idx int32 [sum T, K], tr float32 [sum T, 2], centres float64 [B, 3],
    ratios [B]."""
    cases, axes, num_rots = BATCHES[name]
    scenes = [build_scene(c, axes) for c in cases]
    refs = [reference(s, c.ratio, num_rots, axes) for c, s in zip(cases, scenes)]
    return cases, scenes, refs, num_rots, axes, batch_arrays(scenes, [c.ratio for c in cases])


def batch_arrays(scenes, ratios):
    off = lambda n: np.concatenate([[0], np.cumsum(n)]).astype(np.int32)    # noqa: E731
    return dict(pts=np.concatenate([s["pc"] for s in scenes]), pt_off=off([len(s["pc"]) for s in scenes]),
                idx=np.concatenate([s["idx"] for s in scenes]), tup_off=off([len(s["idx"]) for s in scenes]),
                tr=np.concatenate([s["tr"] for s in scenes]), centres=np.stack([s["centre"] for s in scenes]),
                ratios=list(ratios))


def kept_rows(tup_off, kept_tuples, max_kept):
    """The documented rule of cppf_kept_rows / cppf_kept_rows32: [B, max_kept] global tuple rows of each scene's kept pairs,
    padded with the scene's first tuple row, or row 0 for a scene without tuples."""
    B = len(kept_tuples)
    rows = np.zeros((B, max_kept), np.int64)
    for b, kt in enumerate(kept_tuples):
        t0 = int(tup_off[b])
        rows[b] = t0 if t0 < tup_off[b + 1] else 0
        rows[b, :len(kt)] = t0 + kt
    return rows
