"""CPU checks of the wide scene explanation (cppf2_amd/scene.py explain_wide): the restatement (tests/
scene_ref.py, which has no limit on C; tests/test_scene_wide_gpu.py holds the kernels to it byte for byte) on hand-drawn cases
with candidates above index 63, the wrappers' argument errors, the return codes of cppf_scene_explain_wide before any device
work, its pinned workspace sizes, and eval.py's rules for --explain_hypotheses."""
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


def _placed(C_, where, H=12, W=20, at=0):
    """order_case's renders A, B, C at the candidate indices `where` (a dict index -> 0, 1 or 2) among C_ empty candidates."""
    d_o, m, abc = SC.order_case(H, W, at)
    ren = np.zeros((C_, H, W), F)
    for c, which in where.items():
        ren[c] = abc[which]
    return d_o, m, ren


def test_a_winner_above_index_63():
    d_o, m, ren = _placed(200, {130: 0, 7: 2})
    r = SC.explain_image(d_o, m, ren, TAU, 1, 1, 16)
    assert r["chosen"][:3].tolist() == [130, 7, -1] and r["gain"][:2].tolist() == [100, 55] and r["summary"].tolist() == [240, 155, 2]
    assert r["static"][130].tolist() == [100, 100, 0] and (r["labels"].reshape(-1)[:100] == 0).all()


@pytest.mark.parametrize("pair,Cn", [((63, 64), 65), ((64, 320), 321)])
def test_equal_nets_across_planes_give_the_lower_index(pair, Cn):
    lo, hi = pair
    d_o, m, ren = _placed(Cn, {lo: 0, hi: 0})
    r = SC.explain_image(d_o, m, ren, TAU, 1, 1, 16)
    assert r["chosen"][:2].tolist() == [lo, -1] and r["net"][0] == 100 and hi not in r["chosen"].tolist()


@pytest.mark.parametrize("a,b", [(0, 64), (64, 0)])
def test_order_matters_with_a_and_b_in_different_planes(a, b):
    d_o, m, ren = _placed(66, {a: 0, b: 1, 65: 2})
    r = SC.explain_image(d_o, m, ren, TAU, 11, 1, 16)
    assert r["chosen"][:3].tolist() == [a, 65, -1] and r["gain"][:2].tolist() == [100, 55]
    r = SC.explain_image(d_o, m, ren, TAU, 10, 1, 16)
    assert r["chosen"][:4].tolist() == [a, 65, b, -1] and r["gain"][:3].tolist() == [100, 55, 10]
    lab = r["labels"].reshape(-1)
    assert (lab[:100] == 0).all() and (lab[100:110] == 2).all() and (lab[120:175] == 1).all()


# ---- wrapper errors (before a device is touched) -------------------------------------------------------------------------------
def _args(n):
    return dict(depth=np.ones((4, 4), F), region=np.ones((4, 4), np.uint8), cand_off=[0, n], renders=np.ones((1, 4, 4), F))


def test_wrapper_limits():
    from cppf2_amd import scene
    assert scene.MAX_CANDIDATES_WIDE == 512 and scene.MAX_CANDIDATES == 64
    with pytest.raises(ValueError, match="at most 512"):
        scene.explain_wide(**_args(513))
    with pytest.raises(ValueError, match="at most 64"):
        scene.explain(**_args(65))
    # 65 and 512 pass the wide form's argument check, which comes before any device work
    for n in (65, 512):
        off = scene._checked([0, n], TAU, 200, 1, 16, "scene.explain_wide", scene.MAX_CANDIDATES_WIDE)[0]
        assert off.tolist() == [0, n] and off.dtype == np.int32
    with pytest.raises(ValueError, match="max_rounds"):
        scene.explain_wide(max_rounds=65, **_args(65))
    with pytest.raises(ValueError, match="min_gain"):
        scene.explain_wide(min_gain=0, **_args(65))
    recs = np.zeros(65, dtype=[("x", "u1")])
    with pytest.raises(ValueError, match="at most 64"):
        scene.explain_candidates(None, np.ones((4, 4), F), np.ones((4, 4), np.uint8), np.eye(3), recs)
    with pytest.raises(ValueError, match="at most 512"):
        scene.explain_candidates(None, np.ones((4, 4), F), np.ones((4, 4), np.uint8), np.eye(3), np.zeros(513, dtype=recs.dtype),
                                 wide=True)


# ---- the entry point's return codes, before any device work --------------------------------------------------------------------
_D, _R, _REN, _CH, _G, _N, _ST, _LAB, _SUM, _WS = (0x100000 * (i + 1) for i in range(10))
_EINVAL, _EUNSUPPORTED, _ECAPACITY = -1, -2, -4


def _lib():
    from cppf2_amd import _lib
    lib = _lib.load()
    return lib._lib if isinstance(lib, _lib._Traced) else lib


def _call(lib, off=(0, 2, 2, 72), short=0, **kw):
    a = dict(I=len(off) - 1, H=37, W=53, depth=_D, region=_R, P=off[-1], renders=_REN, tau=0.02, min_gain=200, viol_weight=1,
             max_rounds=16, max_candidates=70, chosen=_CH, gain=_G, net=_N, stat=_ST, labels=_LAB, summary=_SUM, ws=_WS)
    a.update(kw)
    h = (C.c_int32 * len(off))(*off)
    need = lib.cppf_scene_explain_wide_workspace_bytes(a["I"], a["H"], a["W"], min(max(a["max_rounds"], 1), 64),
                                                       min(max(a["max_candidates"], 1), 512)) - short
    return lib.cppf_scene_explain_wide(a["I"], a["H"], a["W"], a["depth"], a["region"], h, a["P"], a["renders"], a["tau"],
                                       a["min_gain"], a["viol_weight"], a["max_rounds"], a["max_candidates"], a["chosen"], a["gain"],
                                       a["net"], a["stat"], a["labels"], a["summary"], a["ws"], need, None)


@pytest.mark.parametrize("kw,expected,word", [
    (dict(max_candidates=0), _EUNSUPPORTED, b"more than 512"),
    (dict(max_candidates=513), _EUNSUPPORTED, b"more than 512"),
    (dict(off=(0, 513), max_candidates=513), _EUNSUPPORTED, b"more than 512"),
    (dict(max_candidates=69), _EINVAL, b"70 candidates on image 2, max_candidates = 69"),
    (dict(off=(0, 65), max_candidates=64), _EINVAL, b"max_candidates"),
    (dict(short=1), _ECAPACITY, b"workspace"),
    (dict(max_rounds=65), _EINVAL, b"max_rounds"),
    (dict(max_rounds=0), _EINVAL, b"max_rounds"),
    (dict(min_gain=0), _EINVAL, b"min_gain"),
    (dict(viol_weight=-1), _EINVAL, b"viol_weight"),
    (dict(off=(0, 3, 2, 5)), _EINVAL, b"h_cand_off"),
    (dict(off=(1, 3, 4, 5)), _EINVAL, b"h_cand_off"),
    (dict(P=4), _EINVAL, b"h_cand_off"),
    (dict(off=(0, (1 << 24) + 1)), _EINVAL, b"P <= WSC_MAX_P"),
    (dict(ws=None), _EINVAL, b"workspace"),
    (dict(ws=_WS + 4), _EINVAL, b"workspace"),
    (dict(tau=-1.0), _EINVAL, b"tau"),
    (dict(tau=float("nan")), _EINVAL, b"tau"),
    (dict(H=8193), _EINVAL, b"H <= WSC_MAX_DIM"),
    (dict(H=0), _EINVAL, b"H >= 1"),
    (dict(depth=None), _EINVAL, b"depth"),
    (dict(renders=None), _EINVAL, b"renders"),
    (dict(labels=None), _EINVAL, b"labels"),
])
def test_entry_point_return_codes(kw, expected, word):
    lib = _lib()
    got = _call(lib, **kw)
    assert got == expected and word in lib.cppf_last_error_string(), (kw, got, lib.cppf_last_error_string())


def test_the_narrow_entry_point_keeps_its_limit():
    lib = _lib()
    h = (C.c_int32 * 2)(0, 65)
    need = lib.cppf_scene_explain_workspace_bytes(1, 37, 53, 16)
    got = lib.cppf_scene_explain(1, 37, 53, _D, _R, h, 65, _REN, 0.02, 200, 1, 16, _CH, _G, _N, _ST, _LAB, _SUM, _WS, need, None)
    assert got == _EUNSUPPORTED and b"more than 64" in lib.cppf_last_error_string()


# (I, H, W, max_rounds, max_candidates) -> cppf_scene_explain_wide_workspace_bytes, with G = ceil(max_candidates / 64):
# G planes of 8 bytes per pixel of the call, each rounded up to 256, then 256 G bytes per image and round
_WORKSPACE_BYTES = {
    (0, 4, 4, 16, 64): 0, (1, 0, 4, 16, 64): 0, (1, 4, 8193, 16, 64): 0, (1, 4, 4, 0, 64): 0, (1, 4, 4, 65, 64): 0,
    (1, 4, 4, 16, 0): 0, (1, 4, 4, 16, 513): 0, (1, 4, 4, 16, -1): 0,
    (1, 1, 1, 1, 1): 256 + 256, (1, 1, 1, 1, 64): 256 + 256, (1, 1, 1, 1, 65): 2 * 256 + 2 * 256,
    (1, 37, 53, 16, 64): 15872 + 4096, (1, 37, 53, 16, 128): 2 * 15872 + 2 * 4096, (1, 37, 53, 16, 512): 8 * 15872 + 8 * 4096,
    (3, 37, 53, 16, 130): 3 * 47104 + 3 * 12288,
    (1, 480, 640, 16, 64): 2457600 + 4096, (1, 480, 640, 16, 512): 8 * 2457600 + 8 * 4096,
    (129, 3, 1021, 1, 449): 8 * 3161088 + 8 * 33024,
}


def test_workspace_bytes_are_pinned():
    lib = _lib()
    for args, want in _WORKSPACE_BYTES.items():
        assert lib.cppf_scene_explain_wide_workspace_bytes(*args) == want, (args, lib.cppf_scene_explain_wide_workspace_bytes(*args))
    # one plane: what cppf_scene_explain asks for
    for I, H, W, M in ((1, 1, 1, 1), (3, 37, 53, 16), (8, 480, 640, 16)):
        assert lib.cppf_scene_explain_wide_workspace_bytes(I, H, W, M, 64) == lib.cppf_scene_explain_workspace_bytes(I, H, W, M)


def test_the_stable_interface_lists_the_two_entry_points():
    from cppf2_amd import _lib
    assert {"cppf_scene_explain_wide", "cppf_scene_explain_wide_workspace_bytes"} <= set(_lib.STABLE) and len(_lib.STABLE) == 74
    assert _lib.ABI_VERSION == 11


# ---- eval.py's flag rules ---------------------------------------------------------------------------------------------------------
_OK = dict(data="depth", depth="d.png", propose_masks=True, mesh="m.ply", hypotheses=4)


@pytest.mark.parametrize("kw,match", [
    (dict(_OK, explain_hypotheses=True), "needs --explain_scene"),
    (dict(_OK, explain_scene=True, explain_min_support=0.4), "--explain_min_support gates the hypotheses of --explain_hypotheses"),
    (dict(_OK, explain_min_support=0.4), "--explain_min_support"),
    (dict(_OK, explain_scene=True, explain_hypotheses=True, explain_min_support=1.5), "explain_min_support"),
    (dict(_OK, explain_scene=True, explain_hypotheses=True, explain_min_support=-0.1), "explain_min_support"),
    (dict(_OK, explain_scene=True, explain_hypotheses=True, explain_min_support=float("nan")), "explain_min_support"),
    (dict(_OK, explain_scene=True, explain_hypotheses=True, explain_min_score=0.4), "--explain_min_score gates one pose"),
    (dict(_OK, hypotheses=1, explain_scene=True, explain_hypotheses=True), "needs --hypotheses > 1"),
    (dict(data="depth", depth="d.png", mask="m.png", mesh="m.ply", hypotheses=4, explain_scene=True, explain_hypotheses=True),
     "needs --propose_masks"),
])
def test_eval_flag_rules(kw, match, monkeypatch):
    monkeypatch.chdir(ROOT)
    import eval as ev
    with pytest.raises(ValueError, match=match):
        ev.main(**kw)


def test_eval_flags_normalise():
    import eval as ev
    import inspect
    from cppf2_amd import scene, segment
    base = {k: v.default for k, v in inspect.signature(ev.main).parameters.items()}
    assert base["explain_hypotheses"] is False and base["explain_min_support"] is None
    narrow = dict(min_score=0.5, min_gain=segment.MIN_SEGMENT_PIXELS, viol_weight=1, max_rounds=scene.MAX_ROUNDS)
    assert ev._checked_flags(**dict(base, **dict(_OK, explain_scene=True))).explain == narrow
    f = ev._checked_flags(**dict(base, **dict(_OK, explain_scene=True, explain_hypotheses=True)))
    assert f.explain == dict(narrow, min_support=0.5, hypotheses=True)
    f = ev._checked_flags(**dict(base, **dict(_OK, explain_scene=True, explain_hypotheses=True, explain_min_support=0.25, explain_max=2)))
    assert f.explain == dict(narrow, max_rounds=2, min_support=0.25, hypotheses=True)
    multi = dict(data="depth", depth="d.png", propose_masks=True, hypotheses=4, models_dir="models", pair_tables="t", obj_ids="1,5")
    f = ev._checked_flags(**dict(base, **dict(multi, explain_scene=True, explain_hypotheses=True, explain_min_support=1.0)))
    assert f.explain["min_support"] == 1.0 and f.obj_ids == [1, 5]


def test_hypothesis_candidates():
    """_hypothesis_candidates: empty slots left out, support = fit / drawn in float64 and 0 where nothing is drawn."""
    import eval as ev
    from cppf2_amd import verify
    from cppf2_amd.pipeline import RESULT_DTYPE
    hyp = np.zeros((1, 4), dtype=RESULT_DTYPE)
    hyp["flags"][0, 2] = verify.EMPTY
    counts = np.zeros((1, 4, 5), np.int64)
    counts[0, :, 0], counts[0, :, 4] = [3, 0, 9, 7], [1, 0, 9, 7]
    ver = dict(hypotheses=hyp, counts=counts, scores=np.array([[0.25, 0.0, np.nan, 0.5]]))
    got = ev._hypothesis_candidates(ver, 0, dict(proposal=5, category="custom", obj=0))
    assert [(c["hypothesis"], c["support"], c["score"], c["proposal"]) for c in got] == \
        [(0, float(np.float64(1) / np.float64(3)), 0.25, 5), (1, 0.0, 0.0, 5), (3, 1.0, 0.5, 5)]
