"""GPU checks of the oriented-box IoU (cppf_box_iou, cppf2_amd/box_iou.py) and of the scorer that uses it
(metrics.degree_cm_mAP(iou="device"), python -m cppf2_amd.metrics, eval.py --data=nocs --iou_device): the kernel against the
reference toolkit's stored values, against closed-form values on exact ties, against the host's convex hull next to ties and on
random pairs, and against its NumPy restatement (tests/box_iou_ref.py); the scorer against the toolkit's AP arrays."""
import ctypes as C
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

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = 1e-9                       # the bound tests/test_host_logic.py holds the host IoU to
ROWS_PER_BLOCK = 8               # BOX_THREADS / 16 of cppf_box_iou.hip: a block is 128 threads, one row of 16 lanes per (pair, turn)
P_MAX = 1003                     # 1003 x 36 rows = 4 513 blocks and a half; 1000 x 36 = 4 500 blocks exactly
assert (1000 * 36) % ROWS_PER_BLOCK == 0 and (P_MAX * 36) % ROWS_PER_BLOCK == 4 and 67 % ROWS_PER_BLOCK == 3


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "map_results.pkl"), "rb") as f:
        return pickle.load(f)


@pytest.fixture(scope="module")
def random_set():
    """1 003 seeded random pairs, turns mixed 1 and 36, and the restatement's IoU of each -- with the mixed turns and with
    turns = 1 throughout; computed once, the cases read prefixes (the restatement does not depend on the batch:
    tests/test_box_iou.py)."""
    args = ref.random_pairs(P_MAX, seed=21)
    ones = np.ones(P_MAX, np.int32)
    return dict(args=args, mixed=ref.box_iou(*args), ones=ref.box_iou(*args[:6], ones))


def _device(*args):
    from cppf2_amd import box_iou
    return box_iou.box_iou(*args).cpu().numpy()


def test_device_matches_the_toolkit_on_the_golden_pairs(golden):
    """The 65 iou_pairs of the golden within 1e-9, exactly 0.0 where the toolkit has 0.0."""
    *args, want = ref.golden_pairs(golden["iou_pairs"])
    got = _device(*args)
    print("worst difference to the toolkit: %.3g" % np.abs(got - want).max())
    assert got.dtype == np.float64 and np.abs(got - want).max() < TOL
    assert np.array_equal(got == 0.0, want == 0.0)
    from cppf2_amd import box_iou
    batch = box_iou.iou_3d_batch([p["RT1"] for p in golden["iou_pairs"]], [p["RT2"] for p in golden["iou_pairs"]],
                                 [p["s1"] for p in golden["iou_pairs"]], [p["s2"] for p in golden["iou_pairs"]],
                                 [ref.is_symmetric(p["cls"], p["hv"]) for p in golden["iou_pairs"]]).cpu().numpy()
    assert np.array_equal(batch, got)


@pytest.mark.parametrize("turns,along_y", [(1, False), (36, True)])
def test_device_is_exact_on_ties(turns, along_y):
    """Coinciding planes under seeded random rotations, as a non-symmetric and as a symmetric class: identical boxes 1, a box
    shrunk by f against a shared face f, face-touching boxes exactly 0.0, a half shift 1/3, a quarter turn of a square section 1."""
    *boxes, want, kind = ref.analytic_tie_cases(seed=3, per_kind=10, along_y=along_y)
    got = _device(*boxes, turns)
    print("worst error on the ties: %.3g" % np.abs(got - want).max())
    assert np.abs(got - want).max() < TOL
    assert (got[np.array([k == "touching" for k in kind])] == 0.0).all()


def _hull(R1, t1, s1, R2, t2, s2):
    from cppf2_amd import metrics
    return metrics.box_iou_3d(R1, t1, s1, R2, t2, s2)


def test_device_is_right_next_to_a_tie():
    """The tie pairs with box 2 turned and / or shifted by 1e-15 .. 1e-4: within 1e-9 of the closed form up to 1e-11 and of the
    host's convex hull above, and never above 1."""
    cases = ref.near_tie_cases()
    want = ref.near_tie_reference(cases, _hull)
    got = _device(*cases[:6], 1)
    err = np.abs(got - want)
    for m in ref.NEAR_TIE_MAGNITUDES:
        print("m = %.0e: worst error %.3g" % (m, err[cases[7] == m].max()))
    assert err.max() < TOL, (err.max(), cases[8][int(err.argmax())], cases[7][int(err.argmax())])
    assert got.max() <= 1.0 + 1e-12


def test_device_matches_the_hull_on_random_pairs(random_set):
    """The first 200 random pairs, turns = 1, against the host's convex hull, which shares nothing with the kernel's algorithm."""
    R1, t1, s1, R2, t2, s2 = (a[:200] for a in random_set["args"][:6])
    got = _device(R1, t1, s1, R2, t2, s2, 1)
    want = np.array([_hull(R1[i], t1[i], s1[i], R2[i], t2[i], s2[i]) for i in range(200)])
    print("worst difference to the hull: %.3g" % np.abs(got - want).max())
    assert np.abs(got - want).max() < TOL


@pytest.mark.parametrize("P", [1, 3, 5, 67, 1000, P_MAX])
@pytest.mark.parametrize("mixed", [True, False])
def test_device_matches_the_restatement(random_set, P, mixed):
    """P = 1, 3, 5 (rows that do not fill a wavefront), 67, 1 000 and 1 003 pairs; turns mixed 1 and 36 (max_turns = 36: 36 rows per
    pair, up to 4 513.5 blocks of 8 rows, idle rows beside live ones in a wavefront) and turns = 1 throughout (one row per pair: a
    single partial block up to 125.4 blocks)."""
    args = [a[:P] for a in random_set["args"]]
    if not mixed:
        args[6] = np.ones(P, np.int32)
    want = random_set["mixed" if mixed else "ones"][:P]
    got = _device(*args)
    print("P = %d, worst difference to the restatement: %.3g" % (P, np.abs(got - want).max()))
    assert np.abs(got - want).max() < TOL
    assert np.array_equal(got == 0.0, want == 0.0)
    if P >= 67:
        assert (want > 0.05).sum() > P // 4 and (want == 0.0).sum() > 0


def test_empty_batch_and_refusals(random_set):
    """P = 0 returns success without a launch; null pointers, a negative or too large P and a max_turns outside 1 .. 64 are
    refused with a message; the wrapper refuses turns outside 1 .. 64 and ragged arguments; on the entry point itself a pair
    whose turns is outside 1 .. max_turns gets NaN and leaves its neighbours alone."""
    import torch
    from cppf2_amd import _lib, box_iou, ops
    L = _lib.load()
    dev = ops._dev()
    assert box_iou.box_iou(*(np.zeros((0, w)) for w in (9, 3, 3, 9, 3, 3)), np.zeros(0, np.int32)).shape == (0,)
    null = C.c_void_p(0)
    assert L.cppf_box_iou(null, null, null, null, null, null, null, null, 1, 0, null, ops._stream()) == 0
    a = [torch.from_numpy(np.ascontiguousarray(x[:4])).to(dev) for x in random_set["args"]]
    cs = torch.from_numpy(box_iou.turn_table(36)).to(dev)
    out = torch.full((4,), -1.0, dtype=torch.float64, device=dev)

    def call(ptrs, max_turns, P):
        return L.cppf_box_iou(*ptrs, max_turns, P, ops._p(out), ops._stream())

    good = [ops._p(x) for x in a] + [ops._p(cs)]
    for bad in ([null] + good[1:], good[:6] + [null, good[7]], good[:7] + [null]):
        assert call(bad, 36, 4) == -1 and b"invalid argument" in L.cppf_last_error_string()
    assert L.cppf_box_iou(*good, 36, 4, null, ops._stream()) == -1
    for max_turns, P in ((36, -1), (36, (1 << 20) + 1), (0, 4), (65, 4)):
        assert call(good, max_turns, P) == -1 and b"invalid argument" in L.cppf_last_error_string()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1.0).all()                       # nothing was launched
    with pytest.raises(_lib.CppfError):
        _lib.check(call(good, 65, 4), "cppf_box_iou")
    for turns in (0, 65, [1, 36, 0, 1]):
        with pytest.raises(ValueError):
            box_iou.box_iou(*[x[:4] for x in random_set["args"][:6]], turns)
    with pytest.raises(ValueError):
        box_iou.box_iou(*[x[:4] for x in random_set["args"][:6]], np.ones(3, np.int32))
    # turns outside 1 .. max_turns on the entry point: NaN for that pair alone
    a[6] = torch.tensor([1, 37, 0, 36], dtype=torch.int32, device=dev)
    assert call([ops._p(x) for x in a] + [ops._p(cs)], 36, 4) == 0
    got = out.cpu().numpy()
    want = random_set["ones"][:4].copy()
    want[3] = ref.box_iou(*(x[3:4] for x in random_set["args"][:6]), [36])[0]
    assert np.isnan(got[1]) and np.isnan(got[2]) and np.abs(got[[0, 3]] - want[[0, 3]]).max() < TOL


def test_scorer_on_the_device_matches_the_toolkit(golden):
    """degree_cm_mAP(iou="device") on the golden's 40 images, use_matches_for_pose False and True, against the toolkit's stored
    arrays at the tolerances of tests/test_host_logic.py (a positive float32 IoU of the golden is at least 8.7e-6 from every
    threshold, so a 1e-9 difference cannot flip a match)."""
    from cppf2_amd import metrics
    for matched, ki, kp in ((False, "iou_aps", "pose_aps"), (True, "iou_aps_matched", "pose_aps_matched")):
        iou_aps, pose_aps = metrics.degree_cm_mAP(golden["results"], golden["synset_names"], (5, 10, 15), (5, 10, 15),
                                                  golden["iou_thresholds"], 0.1, matched, iou="device")
        assert np.allclose(iou_aps, golden[ki], rtol=0, atol=1e-9, equal_nan=True)
        assert np.allclose(pose_aps, golden[kp], rtol=0, atol=1e-12, equal_nan=True)
    assert 0 < iou_aps[-1, 75] < iou_aps[-1, 50] < iou_aps[-1, 25] <= 1


def test_perfect_predictions_score_iou_ap_one(golden):
    """Predictions that are copies of the ground truth: IoU AP 1.0 at 0.25, 0.50 and 0.75 for every class present (the host's
    hull loses vertices on exactly coinciding planes and does not reach this)."""
    from cppf2_amd import metrics
    perfect = [metrics.make_result_record(r["gt_class_ids"], r["gt_RTs"], r["gt_scales"], None, r["gt_class_ids"], r["gt_RTs"],
                                          r["gt_scales"], r["gt_handle_visibility"]) for r in golden["results"]]
    iou_aps, _ = metrics.degree_cm_mAP(perfect, golden["synset_names"], (5, 10, 15), (5, 10, 15), golden["iou_thresholds"], 0.1,
                                       True, iou="device")
    present = sorted({int(c) for r in golden["results"] for c in r["gt_class_ids"]})
    assert present == [1, 2, 3, 4, 5, 6]
    assert (iou_aps[present][:, [25, 50, 75]] == 1.0).all()


def test_rescore_and_main_nocs_report_the_direct_call(tmp_path, monkeypatch):
    """eval.py --data=nocs --iou_device on a two-image fixture in the REAL275 layout, and python -m cppf2_amd.metrics --iou device
    on the records it saved: the summary of the direct degree_cm_mAP(iou="device") call on the same records."""
    from cppf2_amd import metrics
    monkeypatch.chdir(ROOT)
    import eval as ev
    ref.write_nocs_fixture(str(tmp_path), GOLDEN)
    rep = ev.main(data="nocs", log_dir=str(tmp_path / "log"), data_root=str(tmp_path / "real_test"), out_dir=str(tmp_path / "out"),
                  num_pairs=3000, num_rots=36, opt=False, categories="bottle,can", iou_device=True)
    assert rep["categories"] == ["bottle", "can"] and rep["scorer_seconds"] > 0
    ids = [metrics.SYNSET_NAMES.index(c) for c in rep["categories"]]
    direct = metrics.degree_cm_mAP(rep["final_results"], metrics.SYNSET_NAMES, (5, 10, 15), (5, 10, 15), np.linspace(0, 1, 101),
                                   0.1, True, iou="device")
    want = metrics.nocs_summary(direct[0], direct[1], ids)
    assert rep["pose_AP"] == want["pose_AP"] and rep["iou_AP"] == want["iou_AP"]
    assert any(v is not None for v in want["iou_AP"].values())
    out = tmp_path / "report.json"
    cli = metrics._main(["--results", str(tmp_path / "out"), "--iou", "device", "--categories", "bottle,can", "--out", str(out)])
    assert cli["images"] == 2 and cli["iou"] == "device" and cli["categories"] == ["bottle", "can"]
    assert cli["pose_AP"] == want["pose_AP"] and cli["iou_AP"] == want["iou_AP"]
    assert json.load(open(out))["iou_AP"] == want["iou_AP"]
    # the flag belongs to the NOCS mode
    with pytest.raises(ValueError):
        ev.main(data="synthetic", iou_device=True)
