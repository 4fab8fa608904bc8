"""Inputs for the stand-alone rotation operators (ops.vote_rotation -> cppf_vote_rotation, ops.sphere_counts / ops.get_topk_dir ->
cppf_sphere_counts) at the sizes where their kernels change path, and the host-only reasoning those inputs rest on.

Needs neither the built library nor a GPU (no cppf2_amd.ops import).  Every expected value comes from oracle.cppf_oracle
(O.vote_rotation, O.get_topk_dir); nothing here restates an output.  tests/test_rotation_ops_ref.py checks on the CPU that each
input set has the property it is named for; tests/test_rotation_ops_gpu.py holds the kernels to the oracle on them.

vote_rotation: vr_scan_kernel is ONE workgroup of SCAN_BLOCK threads that walks the pairs SCAN_BLOCK at a time and carries the
running rank from block to block, so the cases put degenerate pairs on both sides of every block edge, make one block's total 0
and another's SCAN_BLOCK, and go up to the reference's default of 5 000 kept pairs.

sphere_counts: a chunk of bmm_size candidate rows is cut into sub-blocks of SC_ROWS rows, each bin is one thread of a 256-thread
workgroup; the cases sit on those edges.  The cone-edge set holds candidates whose dot product with a bin falls on the other side
of the cone threshold when it is summed in another order than the reference's fma(z,bz, fma(y,by, x*bx)).
"""
import collections
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import cppf_oracle as O  # noqa: E402

F32, F64 = np.float32, np.float64
SCAN_BLOCK = 1024          # BV_THREADS (cppf_common.h): pairs per step of vr_scan_kernel
EMIT_GRID = 16384 * 256    # items one pass of vr_emit_kernel's capped grid covers
SC_ROWS = 512              # candidate rows per workgroup of sphere_counts_kernel
N_POINTS = 200             # points of the one cloud every vote_rotation case uses (64 .. 300)
# the cloud's fixed points: (NEAR_INVALID) 5e-8 apart -> |ab| below the 1e-7 rule, dropped; (NEAR_VALID) 1e-6 apart -> kept;
# (X_ONLY) differ in x alone -> u = (+-1, 0, 0), the pair frame's second choice of perpendicular (train_dino.py:187-189)
NEAR_INVALID, NEAR_VALID, X_ONLY = (0, 1), (2, 3), (4, 5)
FIRST_FREE = 6             # points from here on are random


def cloud():
    """float32 [N_POINTS, 3]: random points of the unit box after the six fixed ones."""
    rng = np.random.RandomState(11)
    pc = rng.rand(N_POINTS, 3).astype(F32)
    pc[0] = (0.0, 0.0, 0.0)
    pc[1] = (5e-8, 0.0, 0.0)
    pc[2] = (0.0, 1e-3, 0.0)
    pc[3] = (0.0, 1e-3, 1e-6)
    pc[4] = (0.1, 0.2, 0.3)
    pc[5] = (0.35, 0.2, 0.3)
    return pc


def pair_norms(pc, idx):
    """The oracle's float32 |a - b| of every pair (what its mask compares with 1e-7)."""
    return O._pair_frame(np.asarray(pc, F32), np.asarray(idx))[2]


# variant: "edges" (degenerate pairs at rows 0, 1023, 1024, 2047, 2048, T-1 plus a random tenth), "block_empty" (rows 1024..2047
# all degenerate: that block's total is 0), "block_full" (rows 0..1023 all valid: that block's total is SCAN_BLOCK)
VrCase = collections.namedtuple("VrCase", "T k num_rots variant")

VR_CASES = [
    VrCase(1, 2, 1, "edges"), VrCase(1, 5, 36, "edges"),
    VrCase(1023, 2, 36, "edges"), VrCase(1023, 5, 1, "edges"),
    VrCase(1024, 5, 36, "edges"), VrCase(1024, 2, 180, "edges"),
    VrCase(1025, 2, 1, "edges"), VrCase(1025, 5, 180, "edges"),
    VrCase(2049, 2, 36, "edges"), VrCase(2049, 5, 1, "edges"),
    VrCase(5000, 5, 180, "edges"), VrCase(5000, 2, 36, "edges"),
    VrCase(2049, 5, 36, "block_empty"), VrCase(5000, 2, 1, "block_empty"),
    VrCase(2049, 2, 36, "block_full"), VrCase(5000, 5, 180, "block_full"),
]
EDGE_ROWS = (0, 1023, 1024, 2047, 2048)


def vr_id(c):
    return "T%d-k%d-R%d-%s" % c


def edge_rows(T):
    return sorted({r for r in EDGE_ROWS + (T - 1,) if 0 <= r < T})


def vr_inputs(case, seed=0):
    """(pc float32[N,3], idx int64[T,k], angle float32[T]) of one case.  Columns 2.. of idx are filler: in range (a kernel that
    read them would compute a wrong pair, not fault) and never equal to the pair's second point."""
    T, k, _, variant = case
    rng = np.random.RandomState(1000 + seed + T * 7 + k)
    pc = cloud()
    i0 = rng.randint(FIRST_FREE, N_POINTS, T)
    i1 = rng.randint(0, N_POINTS, T)
    if variant == "block_full":                      # first block: two different random points per pair
        n = min(T, SCAN_BLOCK)
        i1[:n] = FIRST_FREE + (i0[:n] - FIRST_FREE + 1 + rng.randint(0, N_POINTS - FIRST_FREE - 1, n)) % (N_POINTS - FIRST_FREE)
    idx = np.stack([i0, i1], -1)
    deg = np.zeros(T, bool)
    taken = edge_rows(T)                             # rows the variant decides about
    if variant == "edges":
        deg = rng.rand(T) < 0.1
        deg[edge_rows(T)] = True
    elif variant == "block_empty":
        deg[SCAN_BLOCK:2 * SCAN_BLOCK] = True
        taken = taken + list(range(SCAN_BLOCK, 2 * SCAN_BLOCK))
    elif variant == "block_full":
        deg[[r for r in edge_rows(T) if r >= SCAN_BLOCK]] = True
        taken = taken + list(range(SCAN_BLOCK))
    if T > 8:                                        # the fixed pairs, both ways round, on rows the variant leaves alone
        rows = rng.choice(np.setdiff1d(np.arange(T), taken), 8, replace=False)
        fixed = [NEAR_INVALID, NEAR_INVALID[::-1], NEAR_VALID, NEAR_VALID[::-1], X_ONLY, X_ONLY[::-1], NEAR_INVALID, NEAR_VALID]
        idx[rows] = np.array(fixed)
        deg[rows] = False
    idx[deg, 1] = idx[deg, 0]
    if k > 2:
        fill = (idx[:, :1] + 1 + rng.randint(0, N_POINTS - 1, (T, k - 2))) % N_POINTS
        same = fill == idx[:, 1:2]
        fill[same] = (fill[same] + 1) % N_POINTS     # may now equal column 0; filler only has to be in range
        idx = np.concatenate([idx, fill], -1)
    # angles clear of tan's pole at pi/2: (0.05, 1.5) and (1.65, 3.1)
    ang = np.where(rng.rand(T) < 0.5, rng.uniform(0.05, 1.5, T), rng.uniform(1.65, 3.1, T)).astype(F32)
    return pc, idx.astype(np.int64), ang


# ------------------------------------------------------------------------------------------------------------------
# sphere_counts
# ------------------------------------------------------------------------------------------------------------------
def sphere(S):
    """float32 [S, 3] unit bins: the reference's Fibonacci sphere from 16 bins on, hand-made axes below."""
    if S >= 16:
        return np.array(O.fibonacci_sphere(S), dtype=F32)
    axes = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0], [0, 0, -1], [-1, 0, 0], [0, -1, 0]], F32)
    assert S <= len(axes)
    return axes[:S].copy()


def candidates(M, sph, angle_tol, seed=0):
    """float32 [M, 3]: half uniformly random unit vectors, half scattered about random bins at about the cone's angular size (so
    that counts are far from zero and many candidates lie near a cone's edge); with M >= 3, one all-zero and one NaN row."""
    rng = np.random.RandomState(2000 + seed + M)
    v = rng.randn(M, 3)
    near = rng.rand(M) < 0.5
    sigma = math.sin(2 * angle_tol / 180 * math.pi) / 1.5
    b = np.asarray(sph, F64)[rng.randint(0, len(sph), M)]
    v = np.where(near[:, None], b + sigma * rng.randn(M, 3), v)
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32) if M else v.astype(F32)
    if M >= 3:
        v[M // 2] = 0.0
        v[M // 3] = np.nan
    return v


def pow2_weights(M, seed=0):
    """float64 [M, 1] divisors 2^-1 .. 2^2: every quotient and every float64 sum of them is exact, in any order."""
    return 2.0 ** np.random.RandomState(3000 + seed + M).randint(-1, 3, (M, 1)).astype(F64)


ScCase = collections.namedtuple("ScCase", "M bmm S angle_tol")
_S = (1, 64, 255, 256, 257, 720)
_TOL = (1.0, 10.0)


def _sc_cases():
    shapes = [(M, 100000) for M in (0, 1, 511, 512, 513, 1024, 1025)]
    for bmm in (1, 100, 512, 1000):
        shapes += [(min(M, 600) if bmm == 1 else M, bmm) for M in (bmm, bmm + 1, 2 * bmm, 2049)]
    # S advances by one per case and the tolerance changes every sixth: over 23 cases each S meets both tolerances
    return [ScCase(M, bmm, _S[i % 6], _TOL[(i // 6) % 2]) for i, (M, bmm) in enumerate(shapes)]


SC_CASES = _sc_cases()


def sc_id(c):
    return "M%d-bmm%d-S%d-tol%g" % c


def n_chunks(M, bmm):
    return (M + bmm - 1) // bmm


# ------------------------------------------------------------------------------------------------------------------
# cone-edge set
# ------------------------------------------------------------------------------------------------------------------
def dot_plain(a, b):
    """float32 (x*bx + y*by) + z*bz, every operation rounded: rows a[M,3] against columns b[3,S]."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return ((a[:, 0:1] * b[0:1, :] + a[:, 1:2] * b[1:2, :]).astype(F32) + a[:, 2:3] * b[2:3, :]).astype(F32)


def dot_fma_reversed(a, b):
    """The fused chain started from the other end, fma(x,bx, fma(y,by, z*bz)), through the oracle's own emulation."""
    return O._dot3_fma(np.asarray(a, F32)[:, ::-1], np.asarray(b, F32)[::-1, :])


def double_rounding_risk(a, b):
    """bool [M, S]: where O._dot3_fma's float64 emulation of a float32 FMA could round twice.  The product of two float32 is
    exact in float64; the float64 sum acc + product is then rounded to float32.  That equals the single rounding of a true FMA
    unless the float64 sum was itself inexact (TwoSum residue != 0) AND landed exactly half way between two float32."""
    a, b = np.asarray(a, F32).astype(F64), np.asarray(b, F32).astype(F64)
    acc = (a[:, 0:1] * b[0:1, :]).astype(F32)
    risk = np.zeros(acc.shape, bool)
    for j in (1, 2):
        x, p = acc.astype(F64), a[:, j:j + 1] * b[j:j + 1, :]
        s = x + p
        bb = s - x
        inexact = ((x - (s - bb)) + (p - bb)) != 0
        f = s.astype(F32)
        other = np.nextafter(f, np.where(s > f.astype(F64), F32(np.inf), F32(-np.inf)).astype(F32))
        tie = (f.astype(F64) != s) & ((f.astype(F64) + other.astype(F64)) * 0.5 == s)
        risk |= inexact & tie
        acc = f
    return risk


ConeSet = collections.namedtuple("ConeSet", "cand bins sphere angle_tol n_found n_dropped")


def cone_edge_set(S, angle_tol, per_bin=400, seed=0):
    """Candidates on the edge of a bin's cone whose hit depends on the order of the dot product.

    Search: points at the cone angle around every eighth bin, at random azimuths, rounded to float32, land within a few ulp of
    the threshold; kept are those where the reference's fused chain and the plain left-to-right float32 sum disagree about
    `> cone_threshold`.  Dropped from those: a candidate with ANY bin at risk of double rounding in the oracle's emulation.
    Returns the kept candidates, the bin each was aimed at, and the counts found / dropped."""
    rng = np.random.RandomState(4000 + seed + S)
    sph = sphere(S)
    thr = O.cone_threshold(angle_tol)
    alpha = math.acos(float(thr))
    cands, bins = [], []
    for s in range(0, S, max(S // 8, 1)):
        b = sph[s].astype(F64)
        b /= np.linalg.norm(b)
        e1 = np.cross(b, [1.0, 0.0, 0.0] if abs(b[0]) < 0.9 else [0.0, 1.0, 0.0])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(b, e1)
        phi = rng.uniform(0, 2 * math.pi, per_bin)
        c = (math.cos(alpha) * b[None] + math.sin(alpha) * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)).astype(F32)
        col = sph[s:s + 1].T
        flip = (O._dot3_fma(c, col) > thr) != (dot_plain(c, col) > thr)
        cands.append(c[flip[:, 0]])
        bins.append(np.full(int(flip.sum()), s))
    cand, bins = np.concatenate(cands), np.concatenate(bins)
    risk = double_rounding_risk(cand, sph.T).any(1)
    return ConeSet(cand[~risk], bins[~risk], sph, angle_tol, len(cand), int(risk.sum()))


def counts_with(dot, cand, sph, angle_tol):
    """Unweighted hit counts per bin under a given dot-product function (float64 integers)."""
    return (dot(cand, np.asarray(sph, F32).T) > O.cone_threshold(angle_tol)).sum(0).astype(F64)


# ------------------------------------------------------------------------------------------------------------------
# get_topk_dir: clusters of different sizes, so that the leading counts are distinct
# ------------------------------------------------------------------------------------------------------------------
def clustered_candidates(sph, angle_tol, sizes=(70, 58, 47, 35, 24, 12, 6), background=300, seed=0):
    rng = np.random.RandomState(5000 + seed)
    sph64 = np.asarray(sph, F64)
    centres = rng.choice(len(sph), len(sizes), replace=False)
    sigma = math.sin(2 * angle_tol / 180 * math.pi) / 8
    parts = [sph64[c] + sigma * rng.randn(n, 3) for c, n in zip(centres, sizes)] + [rng.randn(background, 3)]
    v = np.concatenate(parts)
    v = v[rng.permutation(len(v))]
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def leading_counts_distinct(counts, topk):
    """The topk largest counts are pairwise different and above the next one: torch.topk and the reference leave ties open."""
    top = np.sort(np.asarray(counts))[::-1][:topk + 1]
    return bool(np.all(np.diff(top) < 0))
