"""CPU checks of tests/backvote_ref.py: every case of the back-vote filter's GPU test reaches the edge it is named for, on the
reference's numbers alone (no GPU, no built library), and the helper's own additions to the oracle are what they claim."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import backvote_ref as BR  # noqa: E402
from oracle import cppf_oracle as O  # noqa: E402

_CACHE = {}


def _batch(name):
    if name not in _CACHE:
        _CACHE[name] = BR.build_batch(name)
    return _CACHE[name]


@pytest.mark.parametrize("case", BR.CASES, ids=lambda c: c.name)
def test_case_reaches_its_edge(case):
    cases, _, refs = _batch("table")[:3]
    ref = refs[[c.name for c in cases].index(case.name)]
    assert case.edges and not BR.failed_edges(case, ref), (case.name, BR.failed_edges(case, ref), ref["kq"], ref["gamma"],
                                                           ref["kept"], ref["thr"])


def test_the_table_covers_every_named_edge_and_the_batches_their_shapes():
    assert {e for c in BR.CASES for e in c.edges} == set(BR.EDGES)
    names = [c.name for c in BR.CASES]
    e = names.index("empty")
    assert 0 < e < len(names) - 1 and BR.CASES[e - 1].T > 0 and BR.CASES[e + 1].T > 0        # an empty scene between two full ones
    assert len(BR.BATCHES["table"][0]) < 32 <= len(BR.BATCHES["b33"][0]) == 33               # both grids of backvote_errs_kernel
    assert any(c.T == 0 for c in BR.BATCHES["b33"][0]) and any(c.T == 0 for c in BR.BATCHES["camera"][0])
    assert BR.BATCHES["camera"][1:] == ("camera", 180) and BR.AXES["camera"] != BR.AXES["default"]
    assert set(BR.LONE) <= set(names)
    assert max(c.T for c in BR.CASES) == 5000


@pytest.mark.parametrize("name", sorted(BR.BATCHES))
def test_camera_axes_and_repeats_reach_the_same_edges_or_none(name):
    """Every scene of every batch that names edges reaches them (the camera batch rebuilds its scenes with other axes, which
    must not move the errors), and the repeats with other seeds are different scenes."""
    cases, scenes, refs = _batch(name)[:3]
    for c, r in zip(cases, refs):
        assert not BR.failed_edges(c, r), (name, c.name, BR.failed_edges(c, r))
    if name == "b33":
        by = {c.name: s for c, s in zip(cases, scenes)}
        for n in by:
            if n.endswith("_again") and len(by[n]["idx"]):
                assert not np.array_equal(by[n]["tr"], by[n[:-6]]["tr"])


def test_percentile_params_gives_the_order_statistics_of_np_percentile():
    """The restated (kq, gamma) reproduce np.percentile on float32 data through the two _lerp forms, bit for bit, at every size
    and ratio of the table and a sweep of small sizes -- so the edges asserted on them are edges of the reference."""
    rng = np.random.RandomState(0)
    for n, ratio in [(c.T, c.ratio) for c in BR.CASES if c.T] + [(n, r) for n in range(1, 40) for r in (0.0, 0.1, 0.3, 0.5, 0.999, 1.0)]:
        x = rng.rand(n).astype(np.float32)
        s = np.sort(x)
        kq, g = BR.percentile_params(n, ratio)
        lo, hi, g = s[kq], s[min(kq + 1, n - 1)], np.float32(g)
        want = lo + (hi - lo) * g if g < 0.5 else hi - (hi - lo) * (np.float32(1) - g)
        got = np.percentile(x, ratio * 100)
        assert got.dtype == np.float32 and np.float32(want).tobytes() == got.tobytes(), (n, ratio, kq, g)


def test_reference_additions_on_a_hand_made_scene():
    """kept_tuple, kept_row0 and the empty-mask weights on six tuples whose errors are written by hand: tuples 1, 2, 4 and 5 are
    kept (error 0), 2 has i0 == i1 and 4 joins two coincident points, so the ranks go 0, -, -, 1."""
    pc = (np.random.RandomState(3).rand(BR.N_POINTS, 3) * 0.2).astype(np.float32)
    pc[7] = pc[6]
    idx = np.array([[0, 1], [2, 3], [4, 4], [5, 8], [6, 7], [9, 10]], np.int32)
    idx = np.concatenate([idx, np.zeros((6, BR.K - 2), np.int32)], 1)
    centre = np.array([0.1, 0.1, 0.1])
    tb = O.generate_target_pairs(pc[idx[:, :2]], *np.array(BR.AXES["default"])[[0, 2, 1]], centre)[0]
    tr = tb.copy()
    tr[[0, 3], 0] += np.float32(0.05)
    ref = BR.reference(dict(pc=pc, centre=centre, idx=idx, tr=tr), 0.7, 36)
    assert np.array_equal(ref["back_errs"] == 0, [False, True, True, False, True, True])
    assert np.array_equal(ref["kept_tuple"], [1, 2, 4, 5]) and ref["kept_tuple"].dtype == np.int32
    assert np.array_equal(ref["kept_row0"], [0, -1, -1, 36])
    assert np.array_equal(ref["hits"][[2, 3, 4, 6, 7, 9, 10]], [1, 1, 2, 1, 1, 1, 1]) and ref["hits"].sum() == 8
    assert np.array_equal(ref["kept_wt"], np.array([1.0, 2.0, 1.0, 1.0]) + BR.MARGIN)
    none = BR.reference(dict(pc=pc, centre=centre, idx=idx, tr=tb), 0.5, 36)                 # all errors 0: thr 0, nothing kept
    assert none["thr"] == 0 and none["kept"] == 0 and none["kept_wt"].shape == (0,) and none["kept_row0"].shape == (0,)
    rows = BR.kept_rows(np.array([0, 6, 6, 12]), [ref["kept_tuple"], np.zeros(0, np.int32), none["kept_tuple"]], 5)
    assert np.array_equal(rows, [[1, 2, 4, 5, 0], [0] * 5, [6] * 5])
