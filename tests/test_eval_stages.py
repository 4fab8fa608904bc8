"""CPU checks of the record eval.py's drivers carry for the stages after the vote (cppf2_amd.ensemble.Stages): what
_checked_flags builds from the flags, and the report content stage_notes and instance_items make of it, against literal
values recorded from these functions before the record existed (they took the six settings one by one then)."""
import inspect
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_checked_flags_build_the_stages_record(monkeypatch):
    monkeypatch.chdir(ROOT)
    import eval as ev
    from cppf2_amd import verify
    from cppf2_amd.ensemble import Stages
    assert Stages._fields == ("icp_iters", "icp_depth", "icp_model_weight", "hypotheses", "verify_tau", "centre_peaks")
    base = {k: p.default for k, p in inspect.signature(ev.main).parameters.items()}
    assert ev._checked_flags(**base).stages == Stages(0, False, 1.0, 1, verify.TAU, 1)
    st = ev._checked_flags(**dict(base, data="depth", mesh="obj.ply", icp_iters="5", icp_depth=True, icp_model_weight="2",
                                  hypotheses="4", verify_tau=0.02, centre_peaks="3")).stages
    assert st == Stages(5, True, 2.0, 4, 0.02, 3)
    assert [type(x) for x in st] == [int, bool, float, int, float, int]
    # the default of verify_tau is resolved there, a given one is kept as a float
    assert ev._checked_flags(**dict(base, data="depth", mesh="obj.ply", hypotheses=2)).stages.verify_tau == verify.TAU
    assert ev._checked_flags(**dict(base, data="depth", mesh="obj.ply", hypotheses=2, verify_tau="0.015")).stages.verify_tau == 0.015


_ICP = "5 point-to-plane ICP iterations against obj.ply (cppf_icp_refine)"
_VERIFY = ("4 pose hypotheses per instance from 4 peaks per vote, rendered and compared with the depth at tau = 0.015 m "
           "(cppf_pose_hypotheses, cppf_depth_fit_counts)")


def test_stage_notes_word_the_stages_as_before():
    from cppf2_amd.ensemble import Stages, stage_notes
    off = Stages(0, False, 1.0, 1, 0.02, 1)
    assert stage_notes("obj.ply", off) == {}
    assert stage_notes("obj.ply", off._replace(icp_iters=5)) == {"icp_refinement": _ICP}
    assert stage_notes("obj.ply", off._replace(icp_iters=5, icp_depth=True, icp_model_weight=2.0)) == {
        "icp_refinement": "5 point-to-plane ICP iterations against obj.ply, observed points to model and model samples to the "
                          "depth image, model weight 2 (cppf_icp_refine_depth)"}
    assert stage_notes("obj.ply", off._replace(hypotheses=4, verify_tau=0.015)) == {"verification": _VERIFY}
    assert stage_notes("obj.ply", off._replace(hypotheses=4, verify_tau=0.015, centre_peaks=3)) == {
        "verification": _VERIFY + "; translation hypotheses from 3 separated peaks of each centre vote (cppf_grid_peaks)"}
    cleaning = dict(components=3, kept_pixels=100, valid_pixels=120)
    notes = stage_notes("obj.ply", off._replace(icp_iters=5), cleaning)
    assert notes == {"mask_cleaning": cleaning, "icp_refinement": _ICP} and list(notes) == ["mask_cleaning", "icp_refinement"]
    assert stage_notes("obj.ply", off, mask_cleaning="cleaned") == {"mask_cleaning": "cleaned"}


def _two_instances():
    """A voted batch of two as instance_items reads it: instance 0 picked pass 1, its second of two live hypotheses chosen, from
    centre peak 2, with the 8 ICP stats of the depth form; instance 1 has no pick; both carry table_hits."""
    from cppf2_amd import verify
    from cppf2_amd.pipeline import RESULT_DTYPE
    hyp = np.zeros((2, 3), dtype=RESULT_DTYPE)
    hyp["flags"][0] = [0, 0, verify.EMPTY]
    hyp["flags"][1] = [verify.EMPTY] * 3
    r = dict(pick=np.array([1, -1]), table_hits=np.array([[7, 2, 1], [0, 0, 10]], dtype=np.int64))
    ver = dict(chosen=np.array([1, -1]), hypotheses=hyp, scores=np.array([[0.25, 0.75, 0.0], [0.0, 0.0, 0.0]], dtype=np.float32),
               centre_peak=np.array([2, -1]))
    icp_stats = np.array([[120, 0.5, 0.75, 4, 60, 0.25, 0.5, 200], [0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.float32)
    return r, ver, icp_stats


def test_instance_items_report_the_stages_as_before():
    from cppf2_amd.ensemble import Stages, instance_items
    r, ver, icp_stats = _two_instances()
    one = Stages(5, True, 1.0, 3, 0.02, 1)
    icp8 = {"inliers": 120, "rms": 0.5, "inlier_frac": 0.75, "updates": 4, "model_inliers": 60, "model_rms": 0.25,
            "model_inlier_frac": 0.5, "model_visible": 200}
    first = instance_items(r, 0, icp_stats, ver, one)
    assert first == {"verify": {"hypotheses": 2, "chosen": 1, "score": 0.75, "score_first": 0.25}, "icp": icp8,
                     "table_hits": [7, 2, 1]}
    assert list(first) == ["verify", "icp", "table_hits"]
    assert [type(first["icp"][k]) for k in icp8] == [int, float, float, int, int, float, float, int]
    assert instance_items(r, 1, icp_stats, ver, one) == {"table_hits": [0, 0, 10]}
    # centre_peaks > 1: the chosen hypothesis' centre peak joins `verify`; an instance without a pick still reports neither
    peaks = one._replace(centre_peaks=3)
    assert instance_items(r, 0, icp_stats, ver, peaks) == {
        "verify": {"hypotheses": 2, "chosen": 1, "score": 0.75, "score_first": 0.25, "centre_peak": 2}, "icp": icp8,
        "table_hits": [7, 2, 1]}
    assert instance_items(r, 1, icp_stats, ver, peaks) == {"table_hits": [0, 0, 10]}
    # two model passes (no table), no verification: the 4 ICP stats alone, or nothing
    voted = dict(pick=r["pick"])
    assert instance_items(voted, 0, icp_stats[:, :4], None, one) == {
        "icp": {"inliers": 120, "rms": 0.5, "inlier_frac": 0.75, "updates": 4}}
    assert instance_items(voted, 0, None, None, one) == {}
