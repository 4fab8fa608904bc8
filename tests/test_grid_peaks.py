"""CPU checks of the separated centre-vote peaks: the invariants of the NumPy restatement (tests/grid_peaks_ref.py) that
tests/test_grid_peaks_gpu.py holds cppf_grid_peaks to, and the ordering of eval.py's hypothesis list (_instance_hypotheses)
against the rule it replaces for one centre peak."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grid_peaks_ref as GR  # noqa: E402


def _cells(idx, g):
    return np.stack(np.unravel_index(np.asarray(idx, dtype=np.int64), g), -1)


def _random_grids():
    rng = np.random.default_rng(7)
    for g in ((1, 1, 1), (1, 1, 9), (9, 1, 1), (4, 5, 6), (7, 3, 11), (12, 12, 12)):
        for hi in (2, 4, 50):                                    # small ranges: ties everywhere
            for fill in (1.0, 0.3):
                v = rng.integers(0, hi, g).astype(np.uint32)
                v[rng.random(g) > fill] = 0
                yield g, v


@pytest.mark.parametrize("sep", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("K", [1, 3, 16])
def test_restatement_invariants(K, sep):
    c0 = np.array([0.1, -0.2, 0.7], np.float32)
    for g, v in _random_grids():
        idx, val, world, n = GR.grid_peaks(v, g, c0, 2e-3, K, sep)
        flat = v.reshape(-1)
        # peak 0 is the first maximum, present even on an all-zero grid
        assert idx[0] == int(np.argmax(flat)) and val[0] == flat[idx[0]] and 1 <= n <= K
        assert np.all(idx[n:] == -1) and np.all(val[n:] == 0) and np.all(np.isnan(world[n:]))
        assert np.all(idx[:n] >= 0) and np.all(val[1:n] > 0)
        assert np.array_equal(val[:n], flat[idx[:n]])
        c = _cells(idx[:n], g)
        assert np.array_equal(world[:n], c0.astype(np.float64) + c.astype(np.float64) * 2e-3)
        # values do not increase; equal values come in index order unless suppression forced otherwise
        assert np.all(np.diff(val[:n].astype(np.int64)) <= 0)
        # no two peaks within sep cells
        d2 = ((c[:, None, :] - c[None, :, :]) ** 2).sum(-1)
        assert np.all(d2[~np.eye(n, dtype=bool)] > sep * sep)
        # every positive cell no peak suppresses is at most the last peak taken -- and absent if the scene ran out
        allc = _cells(np.arange(flat.size), g)
        free = (flat > 0) & np.all(((allc[:, None, :] - c[None, :, :]) ** 2).sum(-1) > sep * sep, axis=1)
        if n < K:
            assert not free.any() or flat.max() == 0
        else:
            assert not free.any() or flat[free].max() <= val[n - 1]
            # first-maximum order: a free cell equal to the last peak has a higher index
            tie = np.nonzero(free & (flat == val[n - 1]))[0]
            assert tie.size == 0 or tie.min() > idx[n - 1]


def test_ties_go_to_the_lower_index_and_sep_zero_is_top_k():
    g = (3, 4, 5)
    v = np.zeros(g, np.uint32)
    v[2, 1, 3] = v[0, 3, 4] = v[1, 0, 0] = 9
    v[0, 0, 1] = 4
    idx, val, _, n = GR.grid_peaks(v, g, np.zeros(3, np.float32), 1.0, 8, 0)
    want = [np.ravel_multi_index(p, g) for p in ((0, 3, 4), (1, 0, 0), (2, 1, 3), (0, 0, 1))]
    assert idx[:4].tolist() == want and n == 4 and np.all(idx[4:] == -1) and val[:4].tolist() == [9, 9, 9, 4]
    rng = np.random.default_rng(1)
    v = rng.integers(0, 6, (6, 7, 8)).astype(np.uint32)
    flat = v.reshape(-1).astype(np.int64)
    order = np.lexsort((np.arange(flat.size), -flat))           # by value descending, then index ascending
    order = order[flat[order] > 0][:16]
    idx, val, _, n = GR.grid_peaks(v, v.shape, np.zeros(3, np.float32), 1.0, 16, 0)
    assert n == 16 and np.array_equal(idx, order) and np.array_equal(val, flat[order])


def test_boundary_of_the_suppression_radius():
    """Equal maxima exactly sep apart: the second is suppressed; sep + 1 apart: it is the next peak."""
    g = (20, 20, 20)
    for step in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        for sep in (1, 3, 6):
            for extra, kept in ((0, False), (1, True)):
                v = np.zeros(g, np.uint32)
                a = np.array((4, 4, 4))
                b = a + np.array(step) * (sep + extra)
                v[tuple(a)] = v[tuple(b)] = 5
                idx, _, _, n = GR.grid_peaks(v, g, np.zeros(3, np.float32), 1.0, 2, sep)
                assert idx[0] == np.ravel_multi_index(a, g)
                assert (n == 2 and idx[1] == np.ravel_multi_index(b, g)) if kept else (n == 1 and idx[1] == -1)
    # a diagonal: (2, 3, 6) has squared length 49
    for sep, kept in ((7, False), (6, True)):
        v = np.zeros(g, np.uint32)
        v[1, 1, 1] = v[3, 4, 7] = 2
        _, _, _, n = GR.grid_peaks(v, g, np.zeros(3, np.float32), 1.0, 2, sep)
        assert n == (2 if kept else 1)


def test_all_zero_and_oversized_scenes():
    idx, val, world, n = GR.grid_peaks(np.zeros((2, 3, 4), np.uint32), (2, 3, 4), np.array([1, 2, 3], np.float32), 0.5, 3, 2)
    assert idx.tolist() == [0, -1, -1] and val.tolist() == [0, 0, 0] and n == 1 and world[0].tolist() == [1.0, 2.0, 3.0]
    idx, val, world, n = GR.grid_peaks(None, (200, 200, 200), np.array([1, 2, 3], np.float32), 0.5, 2, 2, over=True)
    assert idx.tolist() == [0, -1] and val.tolist() == [GR.SENTINEL, 0] and n == 1 and world[0].tolist() == [1.0, 2.0, 3.0]


# ---- eval.py's hypothesis list -------------------------------------------------------------------------------------------

def _records(rng, n, tag):
    from cppf2_amd.pipeline import RESULT_DTYPE
    raw = rng.integers(0, 256, (n, 160), dtype=np.uint8)
    rec = np.frombuffer(raw.tobytes(), dtype=RESULT_DTYPE).copy()
    rec["flags"] &= ~1
    rec["up_idx"] = tag * 100 + np.arange(n)
    rec["R"] = 0.0                                              # (finite fields: records are compared as bytes)
    rec["t"] = 0.0
    rec["scale"] = 0.0
    rec["up_count"] = rec["right_count"] = 1.0
    return rec


def _todays_list(selected, pick, hyp, enabled, H):
    """The rule eval._verify_instances applied before centre peaks existed, restated: the selected record, the other peak
    combinations of the picked pass, then the other enabled pass'; empty records dropped; cut at H."""
    if pick < 0:
        return []
    lst = [selected] + list(hyp[pick][1:])
    if enabled[1 - pick]:
        lst += list(hyp[1 - pick])
    return [h for h in lst if not h["flags"] & 1][:H]


def test_one_centre_peak_reproduces_the_list_without_the_feature():
    sys.path.insert(0, ROOT)
    import eval as ev
    rng = np.random.default_rng(3)
    for trial in range(40):
        Hp = int(rng.integers(1, 9))
        hyp = [_records(rng, Hp, 1), _records(rng, Hp, 2)]
        for h in hyp:
            h["flags"][1:] |= (rng.random(Hp - 1) < 0.3).astype(np.int32)      # some empty slots, never slot 0
        selected = _records(rng, 1, 9)[0]
        pick = int(rng.integers(-1, 2))
        enabled = (True, bool(rng.integers(0, 2))) if pick == 0 else (bool(rng.integers(0, 2)), True)
        for H in (1, 2, Hp, 2 * Hp + 3):
            recs, centre = ev._instance_hypotheses(selected, pick, [h[None] for h in hyp], enabled, H)
            want = _todays_list(selected, pick, hyp, enabled, H)
            assert recs.shape == (H,) and centre.shape == (H,)
            for j in range(H):
                if j < len(want):
                    assert recs[j].tobytes() == want[j].tobytes() and centre[j] == 0
                else:
                    assert recs[j]["flags"] & 1 and centre[j] == -1
                    keep = recs[j].copy()
                    keep["flags"] = selected["flags"] | 1
                    assert keep.tobytes() == recs[j].tobytes()


def test_further_centre_peaks_follow_the_first_round_robin():
    sys.path.insert(0, ROOT)
    import eval as ev
    rng = np.random.default_rng(5)
    C, Hp = 3, 4
    hyp = [np.stack([_records(rng, Hp, 10 * m + c) for c in range(C)]) for m in (0, 1)]
    hyp[0]["flags"][2] |= 1                                      # pass 0 has no hypothesis at centre peak 2 ...
    selected = hyp[1][0, 0].copy()
    selected["kept"] = 77                                        # (after `opt` the selected record differs from slot 0)

    def tags(recs, centre):
        return [(int(c), int(r["up_idx"])) for r, c in zip(recs, centre) if c >= 0]
    recs, centre = ev._instance_hypotheses(selected, 1, hyp, (True, True), 64)
    first = [selected["up_idx"]] + [1000 + j for j in (1, 2, 3)] + [j for j in range(4)]
    p1 = [1100 + j for j in range(4)] + [100 + j for j in range(4)]
    p2 = [1200 + j for j in range(4)]                            # ... so peak 2 lists the picked pass only
    rr = []
    for j in range(8):
        rr += [(1, p1[j])] + ([(2, p2[j])] if j < 4 else [])
    assert tags(recs, centre) == [(0, t) for t in first] + rr
    assert recs[0].tobytes() == selected.tobytes()
    # H cuts: peak 0's part shrinks to leave one slot per further peak, never below the selected record
    recs, centre = ev._instance_hypotheses(selected, 1, hyp, (True, True), 6)
    assert tags(recs, centre) == [(0, t) for t in first[:4]] + [(1, p1[0]), (2, p2[0])]
    recs, centre = ev._instance_hypotheses(selected, 1, hyp, (True, True), 2)
    assert tags(recs, centre) == [(0, first[0]), (1, p1[0])]
    recs, centre = ev._instance_hypotheses(selected, 1, hyp, (True, True), 1)
    assert tags(recs, centre) == [(0, first[0])]
    # the other pass disabled, and no pick at all
    recs, centre = ev._instance_hypotheses(selected, 1, hyp, (False, True), 64)
    assert tags(recs, centre)[:4] == [(0, t) for t in first[:4]] and (1, 100) not in tags(recs, centre)
    recs, centre = ev._instance_hypotheses(selected, -1, hyp, (True, True), 4)
    assert np.all(centre == -1) and np.all(recs["flags"] & 1)


def test_centre_peaks_flag_errors():
    sys.path.insert(0, ROOT)
    import eval as ev
    assert ev._centre_peaks_flag(1, 1) == 1 and ev._centre_peaks_flag("3", 8) == 3
    with pytest.raises(ValueError, match="--centre_peaks must be >= 1"):
        ev._centre_peaks_flag(0, 8)
    with pytest.raises(ValueError, match="needs --hypotheses > 1"):
        ev._centre_peaks_flag(2, 1)
