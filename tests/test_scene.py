"""CPU checks of scene explanation (cppf2_amd/scene.py): the restatement (tests/scene_ref.py; tests/
test_scene_gpu.py holds the kernels to it byte for byte) on hand-drawn cases, eval.py's flag rules, the wrappers' argument errors,
the return codes of cppf_scene_explain before any device work, and the pinned workspace sizes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import scene_ref as SC  # noqa: E402

F = np.float32
TAU = 0.02


def test_order_matters_and_the_remainder_decides():
    d_o, m, ren = SC.order_case()
    r = SC.explain_image(d_o, m, ren, TAU, 11, 1, 16)
    assert r["chosen"][:3].tolist() == [0, 2, -1] and r["gain"][:2].tolist() == [100, 55] and r["summary"].tolist() == [240, 155, 2]
    r = SC.explain_image(d_o, m, ren, TAU, 10, 1, 16)
    assert r["chosen"][:4].tolist() == [0, 2, 1, -1] and r["gain"][:3].tolist() == [100, 55, 10]
    assert r["net"][:3].tolist() == [100, 55, 10] and r["summary"].tolist() == [240, 165, 3]
    assert r["static"].tolist() == [[100, 100, 0], [60, 60, 0], [55, 55, 0]]
    lab = r["labels"].reshape(-1)
    assert (lab[:100] == 0).all() and (lab[100:110] == 2).all() and (lab[120:175] == 1).all() and (lab[110:120] == 255).all()
    # fewer rounds than eligible candidates: the rounds stop, the rest stays unexplained
    r = SC.explain_image(d_o, m, ren, TAU, 10, 1, 2)
    assert r["chosen"].tolist() == [0, 2] and r["summary"].tolist() == [240, 155, 2]


def test_identical_candidates_give_the_lower_index_once():
    d_o, m, ren = SC.order_case()
    r = SC.explain_image(d_o, m, np.stack([ren[1], ren[0], ren[0]]), TAU, 1, 1, 16)
    assert r["chosen"][:3].tolist() == [1, 0, -1] and r["gain"][:2].tolist() == [100, 10]
    assert 2 not in r["chosen"].tolist()


def test_a_candidate_whose_violations_outweigh_its_gain_is_never_eligible():
    d_o, m, ren = SC.order_case()
    ren = ren.copy()
    ren.reshape(3, -1)[1, 180:215] = 0.5          # B also hides 35 observed pixels by half a metre: net 60 - 2 * 35 < 0
    r = SC.explain_image(d_o, m, ren, TAU, 1, 2, 16)
    assert r["static"][1].tolist() == [95, 60, 35]
    assert r["chosen"][:3].tolist() == [0, 2, -1] and (r["net"] >= 0).all()
    r = SC.explain_image(d_o, m, ren, TAU, 1, 0, 16)      # weight 0: the violations do not count
    assert r["chosen"][:4].tolist() == [0, 2, 1, -1]
    r = SC.explain_image(d_o, m, ren[1:2], TAU, 1, 2, 16)  # alone, too: nothing is chosen, no negative net is keyed
    assert r["chosen"].tolist() == [-1] * 16 and r["summary"].tolist() == [240, 0, 0]


def test_predicates_at_the_boundaries():
    tau = F(0.02)
    near = F(1.0) + tau                           # 1.0199999809: 1.9e-8 inside tau, not on it (tau_edge_case has the exact ones)
    d_o = np.array([[1.0, 1.0, 1.0, np.nan, np.inf, -1.0, -0.0, 1.0, 1.0, 1.0]], F)
    m = np.array([[1, 1, 7, 1, 1, 1, 1, 0, 255, 1]], np.uint8)
    d_c = np.array([[[near, np.nextafter(near, F(2)), 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, np.nan, -0.0]]], F)
    drawn, fit, viol = SC.predicates(d_o, m, d_c, tau)
    assert fit[0, 0].tolist() == [True, False, True, False, False, False, False, False, False, False]
    assert drawn[0, 0].tolist() == [True] * 8 + [False, False]
    assert viol[0, 0].tolist() == [False, False, False, False, True, False, False, False, False, False]


# what tau_edge_case must give, pixel by pixel: |diff| == tau fits and does not violate; one float32 step beyond does not fit, and
# violates only when the render is the nearer one; the region gates fit, never the violation
EDGE_FIT = [True, False, True, True, False, True, False, False, False, True]
EDGE_VIOL = [False, True, False, False, False, False, False, True, True, False]


def test_a_difference_of_exactly_tau_fits_and_one_step_beyond_does_not():
    d_o, m, d_c = SC.tau_edge_case(0.02)
    diff = d_o.astype(np.float64)[0] - d_c.astype(np.float64)[0, 0]
    tau = np.float64(F(0.02))
    assert diff[0] == tau and diff[3] == -tau and diff[1] > tau > diff[2] and diff[4] < -tau < diff[5] and diff[8] > tau > diff[9]
    drawn, fit, viol = SC.predicates(d_o, m, d_c, F(0.02))
    assert drawn[0, 0].tolist() == [True] * 10
    assert fit[0, 0].tolist() == EDGE_FIT
    assert viol[0, 0].tolist() == EDGE_VIOL
    r = SC.explain_image(d_o[0:1], m[0:1], d_c[0], F(0.02), 1, 0, 4)
    assert r["static"].tolist() == [[10, 5, 3]] and r["summary"].tolist() == [8, 5, 1]
    assert r["labels"][0].tolist() == [0 if f_ else 255 for f_ in EDGE_FIT]


# ---- eval.py's flag rules ---------------------------------------------------------------------------------------------------------
_OK = dict(data="depth", depth="d.png", propose_masks=True, mesh="m.ply", hypotheses=4)


@pytest.mark.parametrize("kw,match", [
    (dict(_OK, hypotheses=1, explain_scene=True), "needs --hypotheses > 1"),
    (dict(data="depth", depth="d.png", mask="m.png", mesh="m.ply", hypotheses=4, explain_scene=True), "needs --propose_masks"),
    (dict(data="bop", bop_root="r", out_csv="o.csv", hypotheses=4, explain_scene=True), "needs --propose_masks"),
    (dict(_OK, explain_min_score=0.4), "needs --explain_scene"),
    (dict(_OK, explain_min_gain=100), "needs --explain_scene"),
    (dict(_OK, explain_viol_weight=2), "needs --explain_scene"),
    (dict(_OK, explain_max=4), "needs --explain_scene"),
    (dict(_OK, explain_scene=True, explain_min_score=float("nan")), "explain_min_score"),
    (dict(_OK, explain_scene=True, explain_min_gain=0), "explain_min_gain"),
    (dict(_OK, explain_scene=True, explain_viol_weight=-1), "explain_viol_weight"),
    (dict(_OK, explain_scene=True, explain_max=0), "explain_max"),
    (dict(_OK, explain_scene=True, explain_max=65), "explain_max"),
    (dict(_OK, models_dir="models"), "needs --explain_scene"),
    (dict(_OK, explain_scene=True, models_dir="models", pair_tables="t"), "--mesh"),
    (dict(data="depth", depth="d.png", propose_masks=True, hypotheses=4, explain_scene=True, models_dir="models", pair_tables="t",
          pair_table="t.npz"), "--pair_table"),
    (dict(data="depth", depth="d.png", propose_masks=True, hypotheses=4, explain_scene=True, models_dir="models"), "--pair_tables"),
    (dict(data="depth", depth="d.png", propose_masks=True, hypotheses=4, explain_scene=True, models_dir="models", pair_tables="t",
          obj_ids="1,x"), "obj_ids"),
    (dict(_OK, explain_scene=True, obj_ids="1"), "needs --models_dir"),
    (dict(data="depth", depth="d.png", propose_masks=True, hypotheses=4, explain_scene=True), "needs --data=depth and --mesh"),
])
def test_eval_flag_rules(kw, match, monkeypatch):
    monkeypatch.chdir(ROOT)
    import eval as ev
    with pytest.raises(ValueError, match=match):
        ev.main(**kw)


def test_eval_flags_normalise():
    import eval as ev
    import inspect
    base = {k: v.default for k, v in inspect.signature(ev.main).parameters.items()}
    f = ev._checked_flags(**dict(base, **_OK))
    assert f.explain is None
    f = ev._checked_flags(**dict(base, **dict(_OK, explain_scene=True)))
    from cppf2_amd import scene, segment, verify
    assert f.explain == dict(min_score=0.5, min_gain=segment.MIN_SEGMENT_PIXELS, viol_weight=1, max_rounds=scene.MAX_ROUNDS)
    assert scene.TAU == verify.TAU and scene.MIN_GAIN == 200
    f = ev._checked_flags(**dict(base, **dict(_OK, explain_scene=True, explain_min_score=0.25, explain_min_gain=50,
                                              explain_viol_weight=3, explain_max=2)))
    assert f.explain == dict(min_score=0.25, min_gain=50, viol_weight=3, max_rounds=2)


# ---- wrapper errors (before a device is touched) -------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,match", [
    (dict(tau=-0.01), "tau"),
    (dict(tau=float("nan")), "tau"),
    (dict(min_gain=0), "min_gain"),
    (dict(viol_weight=-1), "viol_weight"),
    (dict(max_rounds=0), "max_rounds"),
    (dict(max_rounds=65), "max_rounds"),
    (dict(cand_off=[0, 2, 1]), "never decrease"),
    (dict(cand_off=[1, 2]), "start at 0"),
    (dict(cand_off=[0]), "cand_off"),
    (dict(cand_off=[0, 65]), "at most 64"),
])
def test_wrapper_errors(kw, match):
    from cppf2_amd import scene
    a = dict(depth=np.ones((4, 4), F), region=np.ones((4, 4), np.uint8), cand_off=[0, 1], renders=np.ones((1, 4, 4), F))
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        scene.explain(**a)


# ---- the entry point's return codes, before any device work --------------------------------------------------------------------
_D, _R, _REN, _CH, _G, _N, _ST, _LAB, _SUM, _WS = (0x100000 * (i + 1) for i in range(10))
_EINVAL, _EUNSUPPORTED, _ECAPACITY = -1, -2, -4


def _lib():
    from cppf2_amd import _lib
    lib = _lib.load()
    return lib._lib if isinstance(lib, _lib._Traced) else lib


def _call(lib, off=(0, 2, 2, 5), short=0, **kw):
    a = dict(I=len(off) - 1, H=37, W=53, depth=_D, region=_R, P=off[-1], renders=_REN, tau=0.02, min_gain=200, viol_weight=1,
             max_rounds=16, chosen=_CH, gain=_G, net=_N, stat=_ST, labels=_LAB, summary=_SUM, ws=_WS)
    a.update(kw)
    h = (C.c_int32 * len(off))(*off)
    need = lib.cppf_scene_explain_workspace_bytes(a["I"], a["H"], a["W"], min(max(a["max_rounds"], 1), 64)) - short
    return lib.cppf_scene_explain(a["I"], a["H"], a["W"], a["depth"], a["region"], h, a["P"], a["renders"], a["tau"], a["min_gain"],
                                  a["viol_weight"], a["max_rounds"], a["chosen"], a["gain"], a["net"], a["stat"], a["labels"],
                                  a["summary"], a["ws"], need, None)


@pytest.mark.parametrize("kw,expected,word", [
    (dict(off=(0, 65)), _EUNSUPPORTED, b"more than 64"),
    (dict(off=(0, 3, 68, 70)), _EUNSUPPORTED, b"more than 64"),
    (dict(max_rounds=65), _EINVAL, b"max_rounds"),
    (dict(max_rounds=0), _EINVAL, b"max_rounds"),
    (dict(min_gain=0), _EINVAL, b"min_gain"),
    (dict(min_gain=-5), _EINVAL, b"min_gain"),
    (dict(viol_weight=-1), _EINVAL, b"viol_weight"),
    (dict(off=(0, 3, 2, 5)), _EINVAL, b"h_cand_off"),
    (dict(off=(1, 3, 4, 5)), _EINVAL, b"h_cand_off"),
    (dict(P=4), _EINVAL, b"h_cand_off"),
    (dict(off=(0, (1 << 24) + 1)), _EINVAL, b"P <= SCN_MAX_P"),
    (dict(short=1), _ECAPACITY, b"workspace"),
    (dict(ws=None), _EINVAL, b"workspace"),
    (dict(ws=_WS + 4), _EINVAL, b"workspace"),
    (dict(tau=-1.0), _EINVAL, b"tau"),
    (dict(tau=float("nan")), _EINVAL, b"tau"),
    (dict(H=8193), _EINVAL, b"H <= SCN_MAX_DIM"),
    (dict(H=0), _EINVAL, b"H >= 1"),
    (dict(depth=None), _EINVAL, b"depth"),
    (dict(renders=None), _EINVAL, b"renders"),
    (dict(labels=None), _EINVAL, b"labels"),
])
def test_entry_point_return_codes(kw, expected, word):
    lib = _lib()
    got = _call(lib, **kw)
    assert got == expected and word in lib.cppf_last_error_string(), (kw, got, lib.cppf_last_error_string())


# (I, H, W, max_rounds) -> cppf_scene_explain_workspace_bytes: 8 bytes per pixel rounded up to 256, then 256 per image and round
_WORKSPACE_BYTES = {
    (0, 4, 4, 16): 0, (1, 0, 4, 16): 0, (1, 4, 8193, 16): 0, (1, 4, 4, 0): 0, (1, 4, 4, 65): 0,
    (1, 1, 1, 1): 512, (1, 1, 64, 16): 512 + 4096, (1, 33, 4, 64): 1280 + 16384, (3, 37, 53, 16): 47104 + 12288,
    (1, 480, 640, 16): 2457600 + 4096, (8, 480, 640, 16): 19660800 + 32768, (129, 3, 1021, 1): 3161088 + 33024,
    (1, 8192, 8192, 64): 536870912 + 16384,
}


def test_workspace_bytes_are_pinned():
    lib = _lib()
    for args, want in _WORKSPACE_BYTES.items():
        assert lib.cppf_scene_explain_workspace_bytes(*args) == want, (args, lib.cppf_scene_explain_workspace_bytes(*args))
