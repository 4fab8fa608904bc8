"""CPU checks of the oriented-box IoU's NumPy restatement (tests/box_iou_ref.py, the algorithm of cppf_box_iou) against the
reference toolkit's stored values and against closed-form values on exact ties, and of the host side of the scorer's new
keyword (metrics.degree_cm_mAP(iou=), metrics.rescore)."""
import json
import os
import pickle
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import box_iou_ref as ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = 1e-9                       # the bound tests/test_host_logic.py holds the host IoU to


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "map_results.pkl"), "rb") as f:
        return pickle.load(f)


def test_restatement_matches_the_toolkit_on_the_golden_pairs(golden):
    """The 65 iou_pairs of the golden (compute_3d_iou_new: random pairs under every class rule, identical, disjoint, contained,
    face-touching): within 1e-9, exactly 0.0 wherever the toolkit has 0.0 (the matching's `iou > 0` at threshold 0 is strict),
    and no face polygon with more than ten vertices."""
    *args, want = ref.golden_pairs(golden["iou_pairs"])
    assert len(want) == 65 and set(args[6].tolist()) == {1, 36}
    got, most = ref.box_iou(*args, return_max_verts=True)
    print("worst difference to the toolkit: %.3g, most vertices %d" % (np.abs(got - want).max(), most))
    assert np.abs(got - want).max() < TOL
    assert (want == 0.0).sum() >= 2 and np.array_equal(got == 0.0, want == 0.0)
    assert most <= ref.MAX_VERTS


@pytest.mark.parametrize("turns,along_y", [(1, False), (36, True)])
def test_restatement_is_exact_on_ties(turns, along_y):
    """Planes of the two boxes that coincide exactly, under seeded random rotations, as a non-symmetric class (turns = 1, the
    shifts along every axis) and as a symmetric one (turns = 36, the shifts along y): identical boxes 1, a box shrunk by f
    against a shared face f, face-touching boxes exactly 0.0, a half shift 1/3, a quarter turn of a square-section box 1."""
    *boxes, want, kind = ref.analytic_tie_cases(seed=3, per_kind=10, along_y=along_y)
    got = ref.box_iou(*boxes, np.full(len(want), turns))
    kinds = sorted(set(kind))
    assert kinds == ["half_shift", "identical", "quarter_turn", "shrunk", "touching"]
    for k in kinds:
        m = np.array([x == k for x in kind])
        print(k, "worst error %.3g" % np.abs(got[m] - want[m]).max())
    assert np.abs(got - want).max() < TOL
    touching = np.array([x == "touching" for x in kind])
    assert (got[touching] == 0.0).all()


def _hull(R1, t1, s1, R2, t2, s2):
    from cppf2_amd import metrics
    return metrics.box_iou_3d(R1, t1, s1, R2, t2, s2)


def test_restatement_is_right_next_to_a_tie():
    """Identical, shrunk, touching, half-shifted and quarter-turned pairs with box 2 turned and / or shifted by 1e-15 .. 1e-4: within
    1e-9 of the closed form up to 1e-11 and of the host's convex hull above (planes tilted by theta meet in a line known to
    rounding / theta only; a lane of box 1 decides for both faces up to theta = 1e-5, which leaves about 1e-10 on either side of
    that threshold), and never above 1."""
    cases = ref.near_tie_cases()
    want = ref.near_tie_reference(cases, _hull)
    got = ref.box_iou(*cases[:6], np.ones(len(want), np.int32))
    err = np.abs(got - want)
    for m in ref.NEAR_TIE_MAGNITUDES:
        print("m = %.0e: worst error %.3g" % (m, err[cases[7] == m].max()))
    assert err.max() < TOL, (err.max(), cases[8][int(err.argmax())], cases[7][int(err.argmax())])
    assert got.max() <= 1.0 + 1e-12


def test_restatement_matches_the_hull_on_random_pairs():
    """200 seeded random pairs, none near a tie, against the host's convex hull: a reference that shares nothing with the
    kernel's algorithm."""
    R1, t1, s1, R2, t2, s2, _ = ref.random_pairs(200, seed=21)
    got = ref.box_iou(R1, t1, s1, R2, t2, s2, np.ones(200, np.int32))
    want = np.array([_hull(R1[i], t1[i], s1[i], R2[i], t2[i], s2[i]) for i in range(200)])
    print("worst difference to the hull: %.3g" % np.abs(got - want).max())
    assert np.abs(got - want).max() < TOL and (want > 0.05).sum() > 50


def test_restatement_scores_identical_rotated_boxes_one():
    """The issue's example: ten identical box pairs under QR rotations of RandomState(3), where the host's hull is arbitrary."""
    rng = np.random.RandomState(3)
    R = np.array([ref.rand_rot(rng) for _ in range(10)])
    t, s = rng.randn(10, 3) * 0.3, rng.uniform(0.2, 1.0, (10, 3))
    for turns in (1, 36):
        assert np.abs(ref.box_iou(R, t, s, R, t, s, np.full(10, turns)) - 1.0).max() < TOL


def test_restatement_does_not_depend_on_the_batch():
    """Each pair alone, the pairs permuted and the pairs together: the same bits (one lane per (pair, turn, face), a maximum over
    the turns)."""
    args = ref.random_pairs(12, seed=7)
    whole = ref.box_iou(*args)
    assert (whole >= 0).all() and (whole <= 1 + 1e-12).all() and (whole > 0).sum() >= 4
    perm = np.random.RandomState(0).permutation(12)
    assert np.array_equal(ref.box_iou(*(a[perm] for a in args)), whole[perm])
    for p in (0, 5, 11):
        assert ref.box_iou(*(a[p:p + 1] for a in args))[0] == whole[p]


def test_turn_table_is_the_scorers(golden):
    """The (cos, sin) table the host hands the kernel: the library's equals the restatement's, row n (n - 1) / 2 + i holds the
    angle metrics.iou_3d forms."""
    from cppf2_amd import box_iou
    tab = box_iou.turn_table(36)
    assert tab.shape == (36 * 37 // 2, 2) and np.array_equal(tab, ref.turn_table(36))
    assert np.array_equal(tab[0], [1.0, 0.0])
    for i in (0, 1, 9, 35):
        a = 2 * np.pi * i / 36.0
        assert np.array_equal(tab[36 * 35 // 2 + i], [np.cos(a), np.sin(a)])


def test_entry_point_refuses_bad_arguments_before_any_device_work():
    """Through ctypes without a device: P = 0 is a success whatever the pointers; a negative or too large P, a max_turns outside
    1 .. 64 and null pointers are CPPF_EINVAL with a message that names the condition."""
    import ctypes as C
    from cppf2_amd import _lib
    L = _lib.load()
    null, fake = C.c_void_p(0), C.c_void_p(4096)
    assert L.cppf_box_iou(*[null] * 8, 1, 0, null, null) == 0
    for ptrs, max_turns, P, what in (([fake] * 8, 36, -1, b"P >= 0"), ([fake] * 8, 36, (1 << 20) + 1, b"P <= BOX_MAX_PAIRS"),
                                     ([fake] * 8, 0, 1, b"max_turns >= 1"), ([fake] * 8, 65, 1, b"max_turns <= BOX_MAX_TURNS"),
                                     ([null] + [fake] * 7, 36, 1, b"R1"), ([fake] * 7 + [null], 36, 1, b"turn_cs")):
        assert L.cppf_box_iou(*ptrs, max_turns, P, fake, null) == -1
        msg = L.cppf_last_error_string()
        assert b"cppf_box_iou: invalid argument" in msg and what in msg, msg
    assert L.cppf_box_iou(*[fake] * 8, 36, 1, null, null) == -1


def test_scorer_keyword_and_rescore_on_the_host(golden, tmp_path):
    """iou="host" is the default's bytes; an unknown value is refused; metrics.rescore / the command line score a directory of
    saved records to the numbers of the direct call."""
    from cppf2_amd import metrics
    records = golden["results"][:4]
    thr = np.linspace(0, 1, 101)
    a = metrics.degree_cm_mAP(records, metrics.SYNSET_NAMES, (5, 10, 15), (5, 10, 15), thr, 0.1, True)
    b = metrics.degree_cm_mAP(records, metrics.SYNSET_NAMES, (5, 10, 15), (5, 10, 15), thr, 0.1, True, iou="host")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    with pytest.raises(ValueError):
        metrics.degree_cm_mAP(records, iou="gpu")
    for k, r in enumerate(records):
        with open(tmp_path / ("results_%04d.pkl" % k), "wb") as f:
            pickle.dump(r, f)
    out = tmp_path / "report.json"
    report = metrics._main(["--results", str(tmp_path), "--out", str(out)])
    assert report["images"] == 4 and report["iou"] == "host" and report["scorer_seconds"] > 0
    present = sorted({int(c) for r in records for c in list(r["gt_class_ids"]) + list(r["pred_class_ids"])})
    want = metrics.nocs_summary(a[0], a[1], present)
    assert report["pose_AP"] == want["pose_AP"] and report["iou_AP"] == want["iou_AP"]
    assert report["categories"] == [metrics.SYNSET_NAMES[c] for c in present]
    assert json.load(open(out)) == json.loads(json.dumps(report))
    with pytest.raises(ValueError):
        metrics.rescore(str(tmp_path / "missing"))
