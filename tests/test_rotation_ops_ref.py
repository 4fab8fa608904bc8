"""The input sets of tests/rotation_ops_ref.py have the properties the GPU tests rely on -- checked without a GPU: every pair
length is clear of vote_rotation's 1e-7 rule, every case reaches the scan-block edge it is named for, the sphere-count shapes sit
on the chunk and sub-block edges, and the cone-edge set is large, free of the oracle's double-rounding cases and really separates
the dot-product orders."""
import numpy as np
import pytest

import rotation_ops_ref as R
from oracle import cppf_oracle as O

F32 = np.float32


# ------------------------------------------------------------------------------------------ vote_rotation inputs
def test_cloud_size_and_fixed_points():
    pc = R.cloud()
    assert pc.dtype == F32 and 64 <= pc.shape[0] <= 300
    n = R.pair_norms(pc, np.array([R.NEAR_INVALID, R.NEAR_VALID, R.X_ONLY]))
    assert 0 < n[0] < F32(0.9e-7) and F32(1.1e-7) < n[1] < F32(2e-6)
    d = pc[R.X_ONLY[0]] - pc[R.X_ONLY[1]]
    assert d[0] != 0 and d[1] == 0 and d[2] == 0        # u = (+-1, 0, 0): co = (0, -u_z, u_y) vanishes


@pytest.mark.parametrize("case", R.VR_CASES, ids=R.vr_id)
def test_vote_rotation_case_is_clear_of_the_threshold_and_reaches_its_edge(case):
    pc, idx, ang = R.vr_inputs(case)
    T, k, _, variant = case
    assert idx.shape == (T, k) and ang.shape == (T,) and ang.dtype == F32
    assert idx.min() >= 0 and idx.max() < pc.shape[0]
    nrm = R.pair_norms(pc, idx)
    assert np.all((nrm == 0) | (nrm < F32(0.9e-7)) | (nrm > F32(1.1e-7)))
    mask = O.vote_rotation(pc, ang, idx[:, :2], 1)[1]
    assert np.array_equal(mask, nrm > F32(1.1e-7))
    # angles keep off tan's pole and off 0 / pi
    assert np.all(((ang > 0.05) & (ang < 1.5)) | ((ang > 1.65) & (ang < 3.1)))
    if k > 2:
        assert np.all(idx[:, 2:] != idx[:, 1:2])          # a kernel that read filler for the second point would see another pair
    edges = R.edge_rows(T)
    if variant == "edges":
        assert not mask[edges].any() and np.all(idx[edges, 0] == idx[edges, 1])
    elif variant == "block_empty":
        assert T > 2 * R.SCAN_BLOCK and not mask[R.SCAN_BLOCK:2 * R.SCAN_BLOCK].any()
        assert mask[:R.SCAN_BLOCK].sum() > 0 and mask[2 * R.SCAN_BLOCK:].sum() > 0
    else:
        assert T > R.SCAN_BLOCK and mask[:R.SCAN_BLOCK].all() and not mask[[r for r in edges if r >= R.SCAN_BLOCK]].any()
    if T > 8:
        small = nrm[(nrm > 0) & (nrm < F32(1e-5))]
        assert (small < F32(0.9e-7)).sum() >= 2 and (small > F32(1.1e-7)).sum() >= 2
    if T > R.SCAN_BLOCK + 1:
        assert mask[R.SCAN_BLOCK:].sum() > 0               # rows whose rank needs the carry


def test_vote_rotation_cases_cover_the_issue_grid():
    assert {c.T for c in R.VR_CASES} == {1, 1023, 1024, 1025, 2049, 5000}     # T = 0 has a test of its own
    assert {c.k for c in R.VR_CASES} == {2, 5} and {c.num_rots for c in R.VR_CASES} == {1, 36, 180}
    assert {c.variant for c in R.VR_CASES} == {"edges", "block_empty", "block_full"}
    assert 5000 * 1000 > R.EMIT_GRID


# ------------------------------------------------------------------------------------------ sphere_counts inputs
def test_sphere_count_cases_cover_the_issue_grid():
    cs = R.SC_CASES
    assert len(cs) <= 36
    assert {c.M for c in cs if c.bmm == 100000} == {0, 1, 511, 512, 513, 1024, 1025}
    for bmm in (100, 512, 1000):
        assert {c.M for c in cs if c.bmm == bmm} == {bmm, bmm + 1, 2 * bmm, 2049}
    assert {c.M for c in cs if c.bmm == 1} == {1, 2, 600}
    for S in (1, 64, 255, 256, 257, 720):
        assert {c.angle_tol for c in cs if c.S == S} == {1.0, 10.0}
    assert max(c.M * c.S for c in cs) < 2e7
    # a sub-block cut by the chunk end, and chunks of several sub-blocks
    assert any(c.bmm < R.SC_ROWS and c.M > c.bmm for c in cs) and any(c.bmm > R.SC_ROWS and c.M > c.bmm for c in cs)


@pytest.mark.parametrize("S", [1, 64, 720])
def test_candidates_are_unit_with_one_zero_and_one_nan_row_and_hit_bins(S):
    sph = R.sphere(S)
    assert sph.shape == (S, 3) and np.allclose(np.linalg.norm(sph.astype(np.float64), axis=1), 1, atol=1e-6)
    for tol in (1.0, 10.0):
        c = R.candidates(513, sph, tol)
        assert c.dtype == F32 and c.shape == (513, 3)
        assert np.isnan(c[513 // 3]).all() and np.all(c[513 // 2] == 0)
        rest = np.delete(c, [513 // 3, 513 // 2], 0)
        assert np.allclose(np.linalg.norm(rest.astype(np.float64), axis=1), 1, atol=1e-6)
        counts = O.get_topk_dir(c, sph, 100000, tol, return_counts=True)[2]
        assert counts.sum() >= 50                          # the bins are hit: an all-zero answer would not pass by accident
    assert R.candidates(0, sph, 1.0).shape == (0, 3) and R.candidates(1, sph, 1.0).shape == (1, 3)
    w = R.pow2_weights(100)
    assert w.dtype == np.float64 and w.shape == (100, 1) and set(np.unique(w)) == {0.5, 1.0, 2.0, 4.0}


# ------------------------------------------------------------------------------------------ cone-edge set
@pytest.mark.parametrize("S,tol", [(64, 10.0), (720, 1.0)])
def test_cone_edge_set_separates_the_dot_orders(S, tol):
    cs = R.cone_edge_set(S, tol)
    thr = O.cone_threshold(tol)
    assert len(cs.cand) >= 32 and len(cs.cand) == cs.n_found - cs.n_dropped
    assert cs.n_dropped <= 0.01 * cs.n_found
    assert not R.double_rounding_risk(cs.cand, cs.sphere.T).any()
    own = cs.sphere[cs.bins].T                                                # each candidate against the bin it was aimed at
    fused = np.diagonal(O._dot3_fma(cs.cand, own))
    plain = np.diagonal(R.dot_plain(cs.cand, own))
    assert np.all((fused > thr) != (plain > thr))
    assert (fused > thr).any() and (plain > thr).any()                        # flips in both directions
    # ... and the counts, which is all the GPU returns, tell the orders apart too
    want = O.get_topk_dir(cs.cand, cs.sphere, 100000, tol, return_counts=True)[2]
    assert np.array_equal(want, R.counts_with(O._dot3_fma, cs.cand, cs.sphere, tol))
    assert not np.array_equal(want, R.counts_with(R.dot_plain, cs.cand, cs.sphere, tol))
    assert not np.array_equal(want, R.counts_with(R.dot_fma_reversed, cs.cand, cs.sphere, tol))


def test_double_rounding_detector_finds_a_constructed_tie():
    # 10610063 * 13264529 = 2^47 - 1 (both factors fit a float32), so the product below is 2^-24 - 2^-71.  With acc = 1 + 2^-23 the
    # exact sum lies just under the float32 tie 1 + 2^-23 + 2^-24: a real FMA gives 1 + 2^-23, but the float64 sum rounds ONTO the
    # tie and the second rounding goes to even, 1 + 2^-22.
    assert 10610063 * 13264529 == 2 ** 47 - 1
    a = np.array([[1.0 + 2.0 ** -23, 10610063 * 2.0 ** -35, 0.0]], F32)
    b = np.array([[1.0], [13264529 * 2.0 ** -36], [0.0]], F32)
    assert float(a[0, 1]) == 10610063 * 2.0 ** -35 and float(b[1, 0]) == 13264529 * 2.0 ** -36
    assert O._dot3_fma(a, b)[0, 0] == F32(1.0 + 2.0 ** -22)
    assert R.double_rounding_risk(a, b)[0, 0]
    assert not R.double_rounding_risk(np.array([[1.0, 0.5, 0.25]], F32), np.array([[1.0], [1.0], [1.0]], F32)).any()


# ------------------------------------------------------------------------------------------ get_topk_dir inputs
@pytest.mark.parametrize("S,tol", [(64, 10.0), (720, 1.0)])
def test_clustered_candidates_have_distinct_leading_counts(S, tol):
    sph = R.sphere(S)
    c = R.clustered_candidates(sph, tol)
    counts = O.get_topk_dir(c, sph, 100, tol, return_counts=True)[2]
    assert R.leading_counts_distinct(counts, 5) and R.leading_counts_distinct(counts, 1)
    assert not R.leading_counts_distinct(np.array([3.0, 3.0, 1.0]), 1)
    assert R.leading_counts_distinct(np.array([3.0, 2.0, 2.0]), 1) and not R.leading_counts_distinct(np.array([3.0, 2.0, 2.0]), 2)
