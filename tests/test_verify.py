"""CPU checks of the pose-hypothesis verification (cppf2_amd/verify.py, cppf_verify.hip): the NumPy restatement's peak rule and
combination order (tests/verify_ref.py), the score and the selection rule, the eval.py flag errors, and the argument checks of
the two entry points (rejected before any device work)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import verify_ref as VR  # noqa: E402

COS20 = float(np.cos(np.deg2rad(20.0)))
COS45 = float(np.cos(np.deg2rad(45.0)))


def _sphere():
    from cppf2_amd import ops
    return ops.sphere_bins(1.0)


def _near(sph, v):
    """Index of the bin nearest to the unit vector v."""
    return int(np.argmax(sph.astype(np.float64) @ np.asarray(v, dtype=np.float64)))


def test_peak_zero_is_the_first_maximum_and_ties_go_to_the_lower_index():
    sph = _sphere()
    row = np.zeros(len(sph), np.float32)
    a, b = _near(sph, (0, 0, 1)), _near(sph, (0, 0, -1))
    lo, hi = min(a, b), max(a, b)
    row[hi] = row[lo] = 5.0
    idx, cnt = VR.peaks(row, sph, 4, COS20)
    assert idx[:2] == [lo, hi] and cnt[:2] == [5.0, 5.0]          # antipodes: two peaks, the lower index first


def test_all_zero_row_has_one_peak_at_index_zero():
    sph = _sphere()
    idx, cnt = VR.peaks(np.zeros(len(sph), np.float32), sph, 8, COS20)
    assert idx == [0] and cnt == [0.0]
    idx, cnt = VR.peaks(np.full(len(sph), np.nan, np.float32), sph, 8, COS20)
    assert idx == [0] and cnt[0] == -np.inf


def test_suppression_and_k_above_the_separable_peaks():
    sph = _sphere().astype(np.float32)
    row = np.zeros(len(sph), np.float32)
    c = _near(sph, (1, 0, 0))
    d = sph.astype(np.float64) @ sph[c].astype(np.float64)
    row[d > np.cos(np.deg2rad(15))] = 1.0                          # a blob of 15 degrees, all within cos_sep of its peak
    row[c] = 9.0
    idx, cnt = VR.peaks(row, sph, 6, COS20)
    assert idx == [c] and cnt == [9.0]                             # one separable peak of six asked
    # the kernel's float32 rule: a bin is suppressed when ((x*x' + y*y') + z*z') >= cos_sep, rounded per operation
    near = [s for s in range(len(sph)) if row[s] > 0 and s != c]
    assert len(near) > 5
    for s in near:
        dot = np.float32(np.float32(sph[s, 0] * sph[c, 0]) + np.float32(sph[s, 1] * sph[c, 1])) + np.float32(sph[s, 2] * sph[c, 2])
        assert dot >= np.float32(COS20)
    far = _near(sph, (0, 1, 0))
    row[far] = 2.0
    idx, _ = VR.peaks(row, sph, 6, COS20)
    assert idx == [c, far]


def test_combinations_order_filter_and_slot_zero():
    sph = _sphere()
    up = _near(sph, (0, 1, 0))
    flip = _near(sph, (0, -1, 0))
    right = _near(sph, (1, 0, 0))
    par = _near(sph, (0, 0.98, 0.2) / np.linalg.norm((0, 0.98, 0.2)))
    cu = np.zeros(len(sph), np.float32)
    cr = np.zeros(len(sph), np.float32)
    cu[up], cu[flip] = 10.0, 6.0
    cr[right], cr[par] = 8.0, 7.0
    U, Rr = VR.peaks(cu, sph, 4, COS20), VR.peaks(cr, sph, 4, COS20)
    assert U[0] == [up, flip] and Rr[0] == [right, par]
    combos = VR.combinations(U, Rr, sph, COS45)
    # (up, par) and (flip, par) are near-parallel: dropped; (0,0) first, then (flip, right)
    assert combos == [(0, 0), (1, 0)]
    # equal keys: ties by (i, j)
    cu[flip] = 10.0
    cr[par] = 0.0
    cr[_near(sph, (0, 0, 1))] = 8.0
    U, Rr = VR.peaks(cu, sph, 4, COS20), VR.peaks(cr, sph, 4, COS20)
    combos = VR.combinations(U, Rr, sph, COS45)
    assert combos == [(0, 0), (0, 1), (1, 0), (1, 1)]


def test_slot_zero_stays_even_when_the_pair_is_not_perpendicular():
    sph = _sphere()
    a = _near(sph, (0, 1, 0))
    U = ([a], [np.float32(3.0)])
    assert VR.combinations(U, U, sph, 0.0) == [(0, 0)]


def test_hypotheses_restatement_records():
    from cppf2_amd.pipeline import RESULT_DTYPE
    sph = _sphere()
    S = len(sph)
    rng = np.random.default_rng(0)
    B, K, H = 3, 4, 6
    cu = rng.integers(0, 5, (B, S)).astype(np.float32)
    cr = rng.integers(0, 5, (B, S)).astype(np.float32)
    cr[2] = 0.0
    base = np.zeros(B, dtype=RESULT_DTYPE)
    base["t"] = rng.standard_normal((B, 3))
    base["flags"] = 8
    out, pi, pc = VR.hypotheses(cu, cr, sph, base, K, H, COS20, COS45, 1, 0)
    for b in range(B):
        assert out[b, 0]["up_idx"] == int(np.argmax(cu[b])) and out[b, 0]["right_idx"] == int(np.argmax(cr[b]))
        assert np.array_equal(out[b]["t"], np.repeat(base[b]["t"][None], H, 0))
        for h in range(H):
            r = out[b, h]
            if r["flags"] & VR.EMPTY:
                assert r["up_idx"] == -1 and r["right_idx"] == -1
                continue
            if h == 0 and abs(sph[r["up_idx"]].astype(np.float64) @ sph[r["right_idx"]]) > COS45:
                continue                                           # slot 0 is kept even for a near-parallel arg-max pair
            R = r["R"]
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-6)
            assert np.array_equal(R[:, 1], sph[r["up_idx"]].astype(np.float64))
    # an all-zero right row: one right peak (index 0), so at most K up peaks x 1
    assert pi[2, 1, 0] == 0 and np.all(pi[2, 1, 1:] == -1)
    # y_only: the right vote keeps peak 0 only
    _, pi_y, _ = VR.hypotheses(cu, cr, sph, base, K, H, COS20, COS45, 1, 0, y_only=True)
    assert np.all(pi_y[:, 1, 1:] == -1) and np.array_equal(pi_y[:, 0], pi[:, 0])


def test_fit_counts_restatement_by_hand():
    d = np.array([[[1.0, 1.0, 0.0, 2.0]]], np.float32)
    m = np.array([[[1, 1, 1, 0]]], np.uint8)
    r = np.array([[[1.005, 0.0, 1.0, 1.5]],        # fit, unexplained, drawn over a hole, drawn 0.5 m in front of an unmasked surface
                  [[1.02, 1.0, 0.0, 2.0]]], np.float32)
    c = VR.fit_counts(d, m, [0, 2], r, [0.01, 0.03])
    assert c.tolist() == [[3, 2, 1, 1, 1, 1], [3, 2, 0, 0, 1, 2]]
    r2 = np.array([[[1.0, 0.95, 0.0, 2.5]]], np.float32)    # 1.0 observed behind 0.95 drawn: a violation; behind: none
    assert VR.fit_counts(d, m, [0, 1], r2, [0.01]).tolist() == [[3, 2, 1, 0, 1]]


def test_score_and_choose():
    from cppf2_amd import verify
    c = np.array([[10, 100, 0, 5, 80], [10, 100, 20, 0, 90], [0, 0, 0, 0, 0]], np.int64)
    s = verify.score(c)
    assert s.dtype == np.float64 and s.tolist() == [0.8, 90 / 120, 0.0]
    assert verify.choose([[0.5, 0.7, 0.7]]).tolist() == [1]
    assert verify.choose([[0.5, 0.5, 0.2]]).tolist() == [0]            # hypothesis 0 wins unless beaten
    assert verify.choose([[0.0, 0.0]]).tolist() == [0]
    assert verify.choose([[0.1, 0.9, 0.3]], [[False, True, False]]).tolist() == [2]   # empty slots never win
    assert verify.choose([[0.1, 0.9]], [[True, True]]).tolist() == [-1]
    assert verify.choose([[np.nan, 0.0]]).tolist() == [1]


def test_eval_flag_errors():
    sys.path.insert(0, ROOT)
    import eval as ev
    with pytest.raises(ValueError):
        ev.main(data="synthetic", hypotheses=8)
    with pytest.raises(ValueError):
        ev.main(data="depth", hypotheses=8)
    with pytest.raises(ValueError):
        ev.main(data="depth", mesh="x.ply", hypotheses=0)


def _untraced_lib():
    from cppf2_amd import _lib
    lib = _lib.load()
    return lib._lib if isinstance(lib, _lib._Traced) else lib


_A, _Bp, _Cp, _D, _E, _F = (C.c_void_p(0x100000 * (i + 1)) for i in range(6))
COS = C.c_float


def _hyp(B=1, S=720, cu=_A, cr=_Bp, sph=_Cp, K=4, cs=0.9, cp=0.7, ua=1, ra=0, base=_D, H=8, out=_E):
    return _untraced_lib().cppf_pose_hypotheses(B, S, cu, cr, sph, K, COS(cs), COS(cp), ua, ra, 0, base, H, out, None, None, None)


def _fit(I=1, H=4, W=4, depth=_A, mask=_Bp, off=(0, 2), P=2, renders=_Cp, taus=_D, n_taus=1, counts=_E):
    o = None if off is None else (C.c_int32 * len(off))(*off)
    return _untraced_lib().cppf_depth_fit_counts(I, H, W, depth, mask, o, P, renders, taus, n_taus, counts, None)


@pytest.mark.parametrize("kw", [dict(cu=None), dict(cr=None), dict(sph=None), dict(base=None), dict(out=None), dict(K=0),
                                dict(K=33), dict(H=0), dict(H=1025), dict(S=0), dict(B=-1), dict(ua=1, ra=1), dict(ua=3),
                                dict(cs=1.5), dict(cs=float("nan")), dict(cp=-0.1), dict(cp=1.1)])
def test_pose_hypotheses_rejects_bad_arguments(kw):
    assert _hyp(**kw) == -1


def test_pose_hypotheses_zero_scenes_launch_nothing():
    assert _hyp(B=0, cu=None, cr=None, sph=None, base=None, out=None) == 0


@pytest.mark.parametrize("kw", [dict(depth=None), dict(mask=None), dict(renders=None), dict(taus=None), dict(counts=None),
                                dict(off=None), dict(n_taus=0), dict(n_taus=33), dict(I=0, off=(0,)), dict(H=0), dict(W=8193),
                                dict(I=2, off=(0, 2, 1), P=1), dict(off=(1, 2)), dict(off=(0, 3)), dict(P=-1, off=(0, -1))])
def test_depth_fit_counts_rejects_bad_arguments(kw):
    assert _fit(**kw) == -1


def test_depth_fit_counts_zero_hypotheses_launch_nothing():
    assert _fit(off=(0, 0), P=0, depth=None, mask=None, renders=None, taus=None, counts=None) == 0


def test_fit_counts_restatement_at_ties_and_special_values():
    """One pixel per decision, tau = 2^-7 so that every difference is exact: diff = tau is no violation and fits, one float32
    further out is a violation and does not fit (both signs); mask bytes 2 and 255 are set; NaN, negative and -0.0 observed
    depths are unseen; +inf observed and drawn gives diff = NaN, which neither violates nor fits; a NaN render is not drawn and
    is not 0 either (nothing unexplained)."""
    f = np.float32
    t = f(2.0 ** -7)
    nan, inf = f(np.nan), f(np.inf)
    d_o = np.array([[[1, 1, 1, 1, nan, -1, inf, -0.0]]], f)
    m = np.array([[[1, 1, 2, 255, 1, 1, 1, 1]]], np.uint8)
    d_h = np.array([[[f(1) - t, np.nextafter(f(1) - t, f(0)), f(1) + t, np.nextafter(f(1) + t, f(2)), 1, 1, inf, nan]]], f)
    assert d_h[0, 0, 1] < d_h[0, 0, 0] < 1 < d_h[0, 0, 2] < d_h[0, 0, 3]
    assert VR.fit_counts(d_o, m, [0, 1], d_h, [t, 0.0]).tolist() == [[7, 5, 1, 0, 2, 0]]
