"""CPU checks of the solid-interval tests (cppf2_amd/solid.py): the restatement (tests/solid_ref.py; tests/
test_solid_gpu.py holds the kernels to it byte for byte) on hand-drawn cases, the constrained greedy selection, the wrappers'
argument errors, the return codes of both entry points before any device work, and the pinned workspace sizes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import scene_ref as SC  # noqa: E402
import solid_ref as SO  # noqa: E402

F = np.float32
KMAT = np.array([8.0, 8.0, 2.0, 1.0], F)


def up(x):
    return np.nextafter(F(x), F(np.inf))


def dn(x):
    return np.nextafter(F(x), F(-np.inf))


def facing_plane_case(d=0.5, tau=0.0078125):
    """A plane facing the camera, n = (0, 0, -1), d and tau dyadic: h = d - z exactly, so a back face at z = d + tau is exactly tau
    below it (not sunk: the test is h < -tau), one float32 step farther is sunk, one step nearer is not.  Returns (f, b [1,1,6],
    plane, tau): pixels 0-2 as said; 3 the sunk depth where nothing is drawn in front (open, still sunk); 4 a front face without a
    back face (open, not back); 5 nothing."""
    z = F(d) + F(tau)
    assert np.float64(z) == np.float64(d) + np.float64(tau)
    b = np.array([[[z, up(z), dn(z), up(z), 0.0, 0.0]]], F)
    f = np.array([[[0.4, 0.4, 0.4, 0.0, 0.4, 0.0]]], F)
    return f, b, np.array([0.0, 0.0, -1.0, d], F), F(tau)


def test_a_back_face_exactly_tau_below_the_plane_is_not_sunk_and_one_step_farther_is():
    f, b, plane, tau = facing_plane_case()
    h = SO.height(b[0], plane, KMAT)
    assert h[0, 0] == -tau and h[0, 1] < -tau < h[0, 2]
    assert SO.support_image(f, b, plane, KMAT, tau).tolist() == [[4, 2, 3, 2]]
    assert SO.sunk_share([[4, 2, 3, 2]]).tolist() == [0.5] and SO.sunk_share([[0, 0, 0, 5]]).tolist() == [0.0]
    # tau = 0: everything behind the plane is sunk, a depth on it is not
    b0 = np.array([[[0.5, up(0.5), dn(0.5), 0.0, 0.0, 0.0]]], F)
    assert SO.support_image(b0, b0, plane, KMAT, 0.0).tolist() == [[3, 1, 3, 0]]


def test_a_zero_plane_and_a_nan_plane_sink_nothing():
    f, b, _, tau = facing_plane_case()
    b = b.copy()
    b[0, 0, 5] = np.inf                                   # 0 * inf = NaN: not below anything
    for plane in (np.zeros(4, F), np.full(4, np.nan, F), np.array([0, 0, -1, np.nan], F)):
        for t in (tau, 0.0):
            assert SO.support_image(f, b, plane, KMAT, t).tolist() == [[5, 0, 3, 3]]


def test_predicates_of_values_that_are_no_depth():
    vals = np.array([0.0, np.nan, np.inf, -np.inf, -1.0, -0.0, 1.0], F)
    f, b = np.meshgrid(vals, vals, indexing="ij")
    back, solid, opn = SO.predicates(f, b)
    pos = np.array([False, False, True, False, False, False, True])
    assert np.array_equal(back, np.broadcast_to(pos[None, :], (7, 7)))
    assert np.array_equal(solid, pos[:, None] & pos[None, :]) and np.array_equal(opn, pos[:, None] != pos[None, :])
    # an infinite back face in front of a tilted plane: h is -inf (sunk) or NaN (not), as IEEE gives it
    plane = np.array([0.0, 0.0, -1.0, 0.5], F)
    c = SO.support_image(f[None], b[None], plane, np.array([8.0, 8.0, 100.0, 100.0], F), 0.01)
    assert c[0, 0] == 14 and c[0, 2] == 4 and c[0, 3] == 20


def overlap_tau_case(tau=0.02):
    """Two candidates on one row of six pixels, intervals [f, b]: a = [tau / 2, 2 tau] everywhere (2 * tau and the neighbours of
    tau are float32 numbers and their differences are exact in float64).  c: 0 starts at tau: the overlap is exactly tau (does not
    count); 1 one float32 step nearer (counts); 2 one step farther; 3 c contains a (counts: 1.5 tau); 4 c is open (no back face);
    5 c lies behind a (hi < lo)."""
    t = F(tau)
    t2 = F(2) * t
    assert np.float64(t2) - np.float64(t) == np.float64(t)
    fa = np.full((1, 6), t / F(2), F)
    ba = np.full((1, 6), t2, F)
    fc = np.array([[t, dn(t), up(t), t / F(4), t, F(2.5) * t]], F)
    bc = np.array([[F(3) * t, F(3) * t, F(3) * t, F(4) * t, 0.0, F(3) * t]], F)
    return np.stack([fa, fc]), np.stack([ba, bc]), t


def test_an_overlap_of_exactly_tau_does_not_count_and_one_step_more_does():
    f, b, t = overlap_tau_case()
    inter = SO.overlap_image(f, b, t)
    assert inter.shape == (2, 64) and inter[:, :2].tolist() == [[6, 2], [2, 5]] and not inter[:, 2:].any()
    assert SO.overlap_image(f, b, 0.0)[:, :2].tolist() == [[6, 4], [4, 5]]       # every pixel with hi > lo
    assert SO.overlap_image(f[:1], b[:1], t)[:, :1].tolist() == [[6]]


def test_conflicts_compare_with_the_smaller_solid():
    inter = np.zeros((3, 64), np.int64)
    inter[:, :3] = [[100, 10, 11], [10, 1000, 0], [11, 0, 110]]
    c = SO.conflicts(inter, 0.1)                          # 10 > 0.1 * 100 is false, 11 > 0.1 * 100 is true
    assert c.tolist() == [[False, False, True], [False, False, False], [True, False, False]]
    assert not SO.conflicts(inter, 1.0).any() and SO.conflicts(inter, 0.0).sum() == 4
    from cppf2_amd import solid
    assert np.array_equal(solid.conflicts(inter, 0.1), c) and np.array_equal(solid.conflicts(inter), c)
    assert solid.sunk_share(np.array([[4, 2, 3, 2], [0, 0, 0, 0]])).tolist() == [0.5, 0.0]
    with pytest.raises(ValueError, match="max_overlap"):
        solid.conflicts(inter, float("nan"))
    with pytest.raises(ValueError, match="one image"):
        solid.conflicts(inter[:, :3], 0.1)


def test_constrained_greedy_on_the_order_case():
    """Section 22's order_case (A 100 pixels, B 60 of which 50 inside A, C 55 apart), min_gain 10: unconstrained A, C, B.  With C
    in conflict with A the successor B is chosen in C's place and the prefix A is unchanged; with B in conflict with C, B is
    dropped when it comes up third; the loop over the unchanged explanation gives what the direct selection gives."""
    d_o, m, ren = SC.order_case()
    none = np.zeros((3, 3), bool)
    assert SO.greedy_loop(d_o, m, ren, 0.02, 10, 1, 16, none) == ([0, 2, 1], [100, 55, 10], [100, 55, 10], [], 1)
    ac = none.copy()
    ac[0, 2] = ac[2, 0] = True
    assert SO.greedy_loop(d_o, m, ren, 0.02, 10, 1, 16, ac) == ([0, 1], [100, 10], [100, 10], [(2, 0)], 2)
    bc = none.copy()
    bc[1, 2] = bc[2, 1] = True
    assert SO.greedy_loop(d_o, m, ren, 0.02, 10, 1, 16, bc) == ([0, 2], [100, 55], [100, 55], [(1, 2)], 2)
    every = ~np.eye(3, dtype=bool)
    assert SO.greedy_loop(d_o, m, ren, 0.02, 10, 1, 16, every) == ([0], [100], [100], [(2, 0), (1, 0)], 3)
    rng = np.random.RandomState(3)
    for _ in range(20):                                   # random fits and conflicts: loop == direct
        C_ = 7
        r = (rng.rand(C_, 12, 20) < 0.3).astype(F)
        cf = np.triu(rng.rand(C_, C_) < 0.3, 1)
        cf = cf | cf.T
        got = SO.greedy_loop(d_o, m, r, 0.02, 5, 1, 16, cf)
        assert got[:3] == SO.greedy_direct(d_o, m, r, 0.02, 5, 1, 16, cf)
        assert got[4] == len(got[3]) + 1 and not cf[np.ix_(got[0], got[0])].any()


def test_defaults_are_the_derived_ones():
    from cppf2_amd import scene, segment, solid, verify
    assert solid.SUPPORT_TAU == segment.MIN_HEIGHT == 0.01 and solid.OVERLAP_TAU == verify.TAU == scene.TAU
    assert solid.MAX_SUNK == 0.1 and solid.MAX_OVERLAP == 0.1 and solid.MAX_CANDIDATES == scene.ROUNDS_LIMIT == 64


# ---- wrapper errors (before a device is touched) -------------------------------------------------------------------------------
@pytest.mark.parametrize("fn,kw,match", [
    ("support_counts", dict(tau=-0.01), "tau"),
    ("support_counts", dict(tau=float("nan")), "tau"),
    ("support_counts", dict(tau=float("inf")), "tau"),
    ("support_counts", dict(cand_off=[0, 2, 1]), "never decrease"),
    ("support_counts", dict(cand_off=[1, 2]), "start at 0"),
    ("support_counts", dict(cand_off=[0]), "cand_off"),
    ("overlap_counts", dict(tau=-0.01), "tau"),
    ("overlap_counts", dict(tau=float("nan")), "tau"),
    ("overlap_counts", dict(cand_off=[0, 65]), "at most 64"),
    ("overlap_counts", dict(cand_off=[0, 2, 1]), "never decrease"),
])
def test_wrapper_errors(fn, kw, match):
    from cppf2_amd import solid
    a = dict(front=np.ones((1, 4, 4), F), back=np.ones((1, 4, 4), F), cand_off=[0, 1])
    if fn == "support_counts":
        a.update(planes=np.zeros(4, F), K=KMAT)
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        getattr(solid, fn)(**a)


# ---- the entry points' return codes, before any device work --------------------------------------------------------------------
_FR, _BK, _PL, _KM, _OUT, _WS = (0x100000 * (i + 1) for i in range(6))
_OK, _EINVAL, _EUNSUPPORTED, _ECAPACITY = 0, -1, -2, -4


def _lib():
    from cppf2_amd import _lib
    lib = _lib.load()
    return lib._lib if isinstance(lib, _lib._Traced) else lib


def _call(lib, entry, off=(0, 2, 2, 5), short=0, **kw):
    a = dict(I=len(off) - 1 if off else 3, H=37, W=53, front=_FR, back=_BK, P=off[-1] if off else 5, planes=_PL, Kmat=_KM, tau=0.01, out=_OUT, ws=_WS)
    a.update(kw)
    h = (C.c_int32 * len(off))(*off) if off is not None else None
    if entry == "support":
        return lib.cppf_support_counts(a["I"], a["H"], a["W"], a["front"], a["back"], h, a["P"], a["planes"], a["Kmat"], a["tau"],
                                       a["out"], None)
    need = lib.cppf_solid_overlap_workspace_bytes(a["I"], a["H"], a["W"]) - short
    return lib.cppf_solid_overlap(a["I"], a["H"], a["W"], a["front"], a["back"], h, a["P"], a["tau"], a["out"], a["ws"], need, None)


_BOTH = [
    (dict(tau=-1.0), _EINVAL, b"tau"),
    (dict(tau=float("nan")), _EINVAL, b"tau"),
    (dict(off=(0, 3, 2, 5)), _EINVAL, b"h_cand_off"),
    (dict(off=(1, 3, 4, 5)), _EINVAL, b"h_cand_off"),
    (dict(P=4), _EINVAL, b"h_cand_off"),
    (dict(off=None), _EINVAL, b"h_cand_off"),
    (dict(off=(0, (1 << 24) + 1)), _EINVAL, b"P <= SLD_MAX_P"),
    (dict(H=8193), _EINVAL, b"H <= SLD_MAX_DIM"),
    (dict(W=8193), _EINVAL, b"W <= SLD_MAX_DIM"),
    (dict(H=0), _EINVAL, b"H >= 1"),
    (dict(I=0, off=(0,), P=0), _EINVAL, b"I >= 1"),
    (dict(front=None), _EINVAL, b"front"),
    (dict(back=None), _EINVAL, b"back"),
    (dict(out=None), _EINVAL, b"front"),
    (dict(off=(0, 0, 0, 0)), _OK, b""),                   # no candidate at all: a valid call that launches nothing
]
_CASES = [("support",) + c for c in _BOTH] + [("overlap",) + c for c in _BOTH] + [
    ("support", dict(planes=None), _EINVAL, b"planes"),
    ("support", dict(Kmat=None), _EINVAL, b"Kmat"),
    ("support", dict(off=(0, 0, 0, 0), front=None, back=None, out=None), _OK, b""),
    ("overlap", dict(off=(0, 65)), _EUNSUPPORTED, b"more than 64"),
    ("overlap", dict(off=(0, 3, 68, 70)), _EUNSUPPORTED, b"more than 64"),
    ("overlap", dict(short=1), _ECAPACITY, b"workspace"),
    ("overlap", dict(ws=None), _EINVAL, b"workspace"),
    ("overlap", dict(ws=_WS + 4), _EINVAL, b"workspace"),
    ("overlap", dict(off=(0, 65), ws=None), _EUNSUPPORTED, b"more than 64"),
]


@pytest.mark.parametrize("entry,kw,expected,word", _CASES, ids=["%s-%d" % (c[0], i) for i, c in enumerate(_CASES)])
def test_entry_point_return_codes(entry, kw, expected, word):
    lib = _lib()
    got = _call(lib, entry, **kw)
    assert got == expected, (kw, got, lib.cppf_last_error_string())
    if expected != _OK:
        assert word in lib.cppf_last_error_string(), (kw, lib.cppf_last_error_string())


# (I, H, W) -> cppf_solid_overlap_workspace_bytes: 8 bytes per pixel, rounded up to 256
_WORKSPACE_BYTES = {
    (0, 4, 4): 0, (1, 0, 4): 0, (1, 4, 8193): 0, (1, 8193, 4): 0, (-1, 4, 4): 0,
    (1, 1, 1): 256, (1, 1, 64): 512, (1, 33, 4): 1280, (3, 37, 53): 47104, (1, 480, 640): 2457600, (8, 480, 640): 19660800,
    (131, 3, 1021): 3210240, (1, 8192, 8192): 536870912,
}


def test_workspace_bytes_are_pinned():
    lib = _lib()
    for args, want in _WORKSPACE_BYTES.items():
        assert lib.cppf_solid_overlap_workspace_bytes(*args) == want, (args, lib.cppf_solid_overlap_workspace_bytes(*args))


# ---- eval.py's flag rules ---------------------------------------------------------------------------------------------------------
_FLAGS_OK = dict(data="depth", depth="d.png", propose_masks=True, mesh="m.ply", hypotheses=4)


@pytest.mark.parametrize("kw,match", [
    (dict(_FLAGS_OK, support_tau=0.01), "needs that flag"),
    (dict(_FLAGS_OK, support_max_share=0.2), "--support_max_share sets a threshold of --support_check"),
    (dict(_FLAGS_OK, solid_tau=0.01), "--solid_tau sets a threshold of --explain_solid"),
    (dict(_FLAGS_OK, explain_scene=True, solid_max_share=0.2), "needs that flag"),
    (dict(_FLAGS_OK, hypotheses=1, support_check=True), "needs --hypotheses > 1"),
    (dict(data="depth", depth="d.png", mask="m.png", mesh="m.ply", hypotheses=4, support_check=True), "needs --propose_masks"),
    (dict(data="depth", depth="d.png", propose_masks=True, hypotheses=4, support_check=True), "needs --data=depth and --mesh"),
    (dict(data="bop", bop_root="r", out_csv="o.csv", hypotheses=4, support_check=True), "needs --propose_masks"),
    (dict(_FLAGS_OK, explain_solid=True), "needs --explain_scene"),
    (dict(_FLAGS_OK, support_check=True, support_tau=-0.01), "support_tau"),
    (dict(_FLAGS_OK, support_check=True, support_tau=float("nan")), "support_tau"),
    (dict(_FLAGS_OK, support_check=True, support_tau=float("inf")), "support_tau"),
    (dict(_FLAGS_OK, support_check=True, support_max_share=1.5), "support_max_share"),
    (dict(_FLAGS_OK, support_check=True, support_max_share=float("nan")), "support_max_share"),
    (dict(_FLAGS_OK, explain_scene=True, explain_solid=True, solid_tau=-1.0), "solid_tau"),
    (dict(_FLAGS_OK, explain_scene=True, explain_solid=True, solid_max_share=-0.1), "solid_max_share"),
])
def test_eval_flag_rules(kw, match, monkeypatch):
    monkeypatch.chdir(ROOT)
    import eval as ev
    with pytest.raises(ValueError, match=match):
        ev.main(**kw)


def test_eval_flags_normalise():
    import eval as ev
    import inspect
    from cppf2_amd import solid
    base = {k: v.default for k, v in inspect.signature(ev.main).parameters.items()}
    assert ev._checked_flags(**dict(base, **_FLAGS_OK)).solid is None
    assert ev._checked_flags(**dict(base, **dict(_FLAGS_OK, explain_scene=True))).solid is None
    f = ev._checked_flags(**dict(base, **dict(_FLAGS_OK, support_check=True)))
    assert f.solid == dict(support=dict(tau=solid.SUPPORT_TAU, max_share=solid.MAX_SUNK), overlap=None)
    f = ev._checked_flags(**dict(base, **dict(_FLAGS_OK, explain_scene=True, explain_solid=True, solid_tau=0.03, solid_max_share=0.25)))
    assert f.solid == dict(support=None, overlap=dict(tau=0.03, max_share=0.25))
    f = ev._checked_flags(**dict(base, **dict(_FLAGS_OK, explain_scene=True, explain_solid=True, support_check=True, support_tau=0,
                                              support_max_share=0)))
    assert f.solid == dict(support=dict(tau=0.0, max_share=0.0), overlap=dict(tau=solid.OVERLAP_TAU, max_share=solid.MAX_OVERLAP))


def test_select_and_explain_candidates_check_their_thresholds_first():
    from cppf2_amd import scene, verify
    from cppf2_amd.pipeline import RESULT_DTYPE
    recs = np.zeros(2, dtype=RESULT_DTYPE)
    img, m = np.ones((4, 4), F), np.ones((4, 4), np.uint8)
    for kw, match in ((dict(plane=np.zeros(4), support_tau=-1.0), "support_tau"), (dict(plane=np.zeros(4), max_sunk=2.0), "max_sunk"),
                      (dict(solid=True, solid_tau=float("nan")), "solid_tau"), (dict(solid=True, max_overlap=-0.5), "max_overlap")):
        with pytest.raises(ValueError, match=match):
            scene.explain_candidates(None, img, m, np.eye(3), recs, **kw)
    with pytest.raises(ValueError, match="support_tau"):
        verify.select(None, img[None], m[None], np.eye(3), recs[None], plane=np.zeros(4), support_tau=float("inf"))


# ---- the two scenes, decided by the restatement alone ---------------------------------------------------------------------------
# What the restatement counts on the CPU renders (tests/solid_scenes.py), recorded here and in DESIGN.md section 25:
# S1  support (back, sunk, solid, open): A (8141, 1926, 8141, 0), B (8338, 0, 8338, 0), the truth (8364, 0, 8364, 0);
#     fit A 6282, B 5880; violations A 145, B 2230; region 8315 pixels.
# S2  solid pixels 5277 (front cube), 5139 (the phantom), 4494 (the cube behind); inter(front, phantom) = 2182, every other pair 0;
#     the patch 1965 pixels, 1941 of them in the region; gains 5061, 4132, 1941.
@pytest.fixture(scope="module")
def s1():
    import solid_scenes
    return solid_scenes.scene1()


@pytest.fixture(scope="module")
def s2():
    import solid_scenes
    return solid_scenes.scene2()


def test_s1_the_pose_pushed_into_the_table_wins_without_the_check_and_is_refused_with_it(s1):
    from cppf2_amd import solid
    s = s1
    print("S1 support", s["support"].tolist(), "share", s["share"].tolist(), "truth", s["truth_support"].tolist(), "plain", s["plain"],
          "supported", s["supported"], "region", int(s["region"].sum()))
    assert s["truth_support"][0, 1] == 0 and s["truth_support"][0, 0] > 5000 and s["truth_support"][0, 3] == 0
    assert SO.sunk_share(s["truth_support"]).tolist() == [0.0]
    assert s["share"][0] > solid.MAX_SUNK and s["share"][1] == 0.0 and not s["support"][:, 3].any()
    assert s["plain"][0] == [0] and s["plain"][4] == 1, "without the check A is chosen, and B adds too little beside it"
    assert s["supported"][0] == [1], "with it A is below the table and B is chosen"
    # A fits within 2 cm almost everywhere it is seen, B fits less
    fit = SC.predicates(s["d"], s["region"], s["f"], 0.02)[1].reshape(2, -1).sum(1)
    assert fit[0] > fit[1] > 0.5 * fit[0] and fit[0] > 0.75 * s["support"][0, 2]
    # A's footprint reaches the 1.5 cm it was pushed under the plane, B's and the truth's stay on it
    import solid_scenes
    low = [float(SO.height(b_, solid_scenes.PLANE, solid_scenes.KMAT)[b_ > 0].min()) for b_ in (s["b"][0], s["b"][1], s["truth_fb"][1])]
    print("S1 lowest back face", low)
    assert -0.0155 < low[0] < -0.0145 and -0.0005 < low[1] and -0.0005 < low[2]


def test_s2_the_pose_inside_the_front_cube_is_an_extra_instance_today_and_is_refused_as_inside(s2):
    from cppf2_amd import scene, solid
    s = s2
    print("S2 support", s["support"].tolist(), "inter", s["inter"][:, :3].tolist(), "plain", s["plain"], "solid", s["solid"],
          "patch", int(s["patch"].sum()), int((s["patch"] & s["region"]).sum()))
    assert s["share"].tolist() == [0.0, 0.0, 0.0], "cubes that stand on the table do not sink"
    assert not s["conflict"][0, 2] and s["inter"][0, 2] == 0, "the two true cubes do not conflict"
    assert s["conflict"][0, 1] and s["inter"][0, 1] > 0.3 * s["inter"][1, 1]
    assert (s["patch"] & s["region"]).sum() >= scene.MIN_GAIN
    assert s["plain"][0] == [0, 2, 1] and s["plain"][1][2] >= scene.MIN_GAIN, "today's greedy picks it as an extra instance"
    assert s["solid"][0] == [0, 2] and s["solid"][3] == [(1, 0)] and s["solid"][4] == 2
    assert s["solid"][1] == s["plain"][1][:2] and s["supported"][0] == [0, 2, 1]
    assert not s["support"][:, 3].any()
