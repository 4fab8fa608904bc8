"""CPU checks of the model-to-depth ICP terms (cppf_icp_refine_depth): the NumPy restatement (tests/icp_depth_ref.py) on the box
scenes of DESIGN.md section 19, its equality with tests/icp_ref.py when the model side has nothing to add, and the host-side
argument checks of icp.refine that need no device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_depth_ref as DR  # noqa: E402
import icp_ref as IR  # noqa: E402

ITERS, D0, D1 = 30, 0.05, 0.005


def test_box_scenes_are_what_the_design_section_describes():
    """Every view shows three faces of the box in front of the wall, the starts are 5-10 degrees and 1-2 cm off, and the
    one-face mask holds 1 500 points of one plane."""
    for s in range(DR.VIEWS):
        v = DR.box_view(s)
        assert len(v["faces"]) == 3, (s, v["faces"])
        rot, tr = DR.pose_err(v["R0"], v["t0"], v["R"], v["t"])
        assert 5 - 1e-6 <= rot <= 10 + 1e-6 and 10 - 1e-6 <= tr <= 20 + 1e-6
        assert v["depth"].max() == np.float32(DR.WALL) and 0.5 < v["depth"].min() < 1.1
        q = v["one_face"].astype(np.float64)
        assert len(q) == DR.MASK_POINTS
        sv = np.linalg.svd(q - q.mean(0), compute_uv=False)
        assert sv[2] < 1e-4 * sv[1]


def test_restatement_reproduces_the_three_behaviours_on_the_box_views():
    """On all 8 views, 30 iterations from the start: one-way ICP on the one-face mask stays more than FLOOR_MM off (the in-plane
    slide of the face is unobservable and keeps the start's error); with the model-to-depth terms the same mask comes within
    CEIL_DEG / CEIL_MM, and so does the run without any observed point."""
    mp, mn = DR.box_model()
    for s in range(DR.VIEWS):
        v = DR.box_view(s)
        one = IR.refine(v["one_face"], v["R0"], v["t0"], mp, mn, ITERS, D0, D1)
        two = DR.refine(v["one_face"], v["R0"], v["t0"], mp, mn, ITERS, D0, D1, v["depth"], DR.K_BOX)
        free = DR.refine(None, v["R0"], v["t0"], mp, mn, ITERS, D0, D1, v["depth"], DR.K_BOX)
        e1, e2, e0 = (DR.pose_err(r[0], r[1], v["R"], v["t"]) for r in (one, two, free))
        print("view %d: one-way %.3f deg %.3f mm, two-way %.4f deg %.4f mm, mask-free %.4f deg %.4f mm" % ((s,) + e1 + e2 + e0))
        assert e1[1] > DR.FLOOR_MM, (s, e1)
        assert e2[0] < DR.CEIL_DEG and e2[1] < DR.CEIL_MM, (s, e2)
        assert e0[0] < DR.CEIL_DEG and e0[1] < DR.CEIL_MM, (s, e0)
        assert two[2][4] > 1000 and two[2][6] > 0.8 and free[2][0] == 0 and free[2][3] == ITERS


@pytest.mark.parametrize("weight", [1.0, 0.37])
def test_equals_icp_ref_step_by_step_without_model_side_inliers(weight):
    """An all-zero depth image (no reading anywhere) and one whose surface is far behind the object give the model side nothing:
    every iteration then equals icp_ref.step bit for bit, whatever the weight, and the model-side stats say why."""
    mp, mn = DR.box_model(1000, seed=3)
    v = DR.box_view(2)
    pts = v["full"][::7]
    for depth, visible in ((np.zeros((DR.H_IMG, DR.W_IMG), np.float32), True), (np.full((DR.H_IMG, DR.W_IMG), 5.0, np.float32), True),
                           (np.full((4, 4), np.nan, np.float32), False)):
        R, t = v["R0"], v["t0"]
        Rr, tr = R, t
        for dk in IR.schedule(8, D0, D1):
            R, t, st = DR.step(pts, R, t, mp, mn, dk, depth, DR.K_BOX, weight)
            Rr, tr, cnt, rms, upd = IR.step(pts, Rr, tr, mp, mn, dk)
            assert np.array_equal(R, Rr) and np.array_equal(t, tr)
            assert st[0] == cnt and st[1] == rms and st[3] == float(upd)
            assert st[4] == 0 and st[5] == 0 and st[6] == 0 and (st[7] > 0) == visible


def test_projection_conventions():
    """A sample straight ahead lands on the pixel (cy, cx) and reads depth[row][col]; a back-facing one, one behind the camera,
    one outside the image and one whose depth is 0 / NaN / inf / negative add nothing; a pair exactly d_k apart is an inlier."""
    K = np.array([[100.0, 0, 8.0], [0, 100.0, 4.0], [0, 0, 1.0]])
    R, t = np.eye(3), np.array([0.0, 0.0, 1.0])
    mp = np.array([[0, 0, 0], [0.03, -0.02, 0], [0, 0, 0], [0, 0, -2.0], [1.0, 0, 0]], np.float32)
    mn = np.array([[0, 0, -1], [0, 0, -1], [0, 0, 1], [0, 0, -1], [0, 0, -1]], np.float32)
    depth = np.zeros((9, 17), np.float32)
    depth[4, 8] = 1.25
    depth[2, 11] = 1.0
    q, idx, vis = DR.project(R, t, mp, mn, depth, K, 0.25)
    assert idx.tolist() == [0, 1] and vis == 2
    assert np.array_equal(q[0], np.array([0, 0, 0.25], np.float32))                      # exactly d_k = 0.25 behind the sample
    assert DR.project(R, t, mp, mn, depth, K, np.float32(0.2499))[1].tolist() == [1]
    for bad in (0.0, np.nan, np.inf, -1.0):
        depth[2, 11] = bad
        assert DR.project(R, t, mp, mn, depth, K, 0.25)[1].tolist() == [0]


def test_refine_argument_checks_need_no_device():
    """What icp.refine can refuse on the host is refused before a device is asked for."""
    from cppf2_amd import icp
    from cppf2_amd.pipeline import RESULT_DTYPE
    model = icp.ModelPoints(*DR.box_model(16), np.zeros(3))
    rec = np.zeros(2, dtype=RESULT_DTYPE)
    pts, off = np.zeros((4, 3), np.float32), [0, 2, 4]
    K = DR.K_BOX
    d1, d3 = np.ones((6, 8), np.float32), np.ones((3, 6, 8), np.float32)
    bad = [
        dict(depth=d1),                                          # no K
        dict(depth=d1, K=np.eye(4)),
        dict(depth=d1, K=np.diag([0.0, 1.0, 1.0])),
        dict(depth=d1, K=np.diag([1.0, np.inf, 1.0])),
        dict(depth=d1.astype(np.float64), K=K),
        dict(depth=np.ones(8, np.float32), K=K),
        dict(depth=np.ones((0, 6, 8), np.float32), K=K),
        dict(depth=d3, K=K),                                     # 3 images, 2 instances, no img_idx
        dict(depth=d3, K=K, img_idx=[0, 1, 2]),
        dict(depth=d1, K=K, model_weight=0.0),
        dict(depth=d1, K=K, model_weight=np.nan),
        dict(depth=d1, K=K, model_weight=np.inf),
        dict(K=K),                                               # depth arguments without depth
        dict(img_idx=[0, 0]),
        dict(model_weight=2.0),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            icp.refine(model, pts, off, rec, **kw)
    with pytest.raises(ValueError):
        icp.refine(model, None, None, rec)                       # no observed points and no depth
    with pytest.raises(ValueError):
        icp.refine(model, pts, None, rec, depth=d1, K=K)
    assert not rec["flags"].any()


def test_eval_flag_errors():
    """--icp_depth without --icp_iters > 0 is the same kind of flag error --centre_peaks without --hypotheses is; the weight
    belongs to --icp_depth."""
    sys.path.insert(0, ROOT)
    import eval as ev
    for data in ("depth", "bop"):
        with pytest.raises(ValueError, match="icp_iters"):
            ev.main(data=data, icp_depth=True)
        with pytest.raises(ValueError, match="icp_model_weight"):
            ev.main(data=data, icp_depth=True, icp_iters=5, icp_model_weight=0)
        with pytest.raises(ValueError, match="icp_depth"):
            ev.main(data=data, icp_iters=5, icp_model_weight=2.0)
    with pytest.raises(ValueError, match="icp_depth"):
        ev.main(data="synthetic", icp_depth=True, icp_iters=5)


def test_new_entry_points_validate_on_the_host():
    """cppf_icp_depth_workspace_bytes and the argument rules of cppf_icp_refine_depth, none of which touches a device."""
    import ctypes as C
    from cppf2_amd import _lib
    lib = _lib.load()
    q = lib.cppf_icp_depth_workspace_bytes
    assert q(1, 0, 1) == 32 * 8 + 8 and q(3, 257, 4096) == 3 * (2 + 16) * 256 + 3 * 16 * 4
    assert q(0, 10, 10) < 0 and q(1, -1, 10) < 0 and q(1, 10, 0) < 0 and q(65536, 1, 1) < 0
    X = 0x100000
    K = (C.c_double * 9)(600, 0, 320, 0, 600, 240, 0, 0, 1)
    a = dict(B=2, pts=X, off=X, max_n=100, mp=X, mn=X, M=50, depth=X, I=2, H=4, W=4, idx=X, K=C.addressof(K), w=1.0, iters=3, d0=0.05,
             d1=0.005, rec=X, stats=X, ws=X, ws_bytes=0)

    def call(**kw):
        b = dict(a, **kw)
        return lib.cppf_icp_refine_depth(b["B"], b["pts"], b["off"], b["max_n"], b["mp"], b["mn"], b["M"], b["depth"], b["I"], b["H"],
                                         b["W"], b["idx"], b["K"], b["w"], b["iters"], b["d0"], b["d1"], b["rec"], b["stats"], b["ws"],
                                         b["ws_bytes"], None)
    assert call() == -4 and b"needed" in lib.cppf_last_error_string()            # CPPF_ECAPACITY: valid but for the workspace
    assert call(max_n=0, pts=None) == -4
    Kbad = (C.c_double * 9)(600, 0, 320, 0, float("inf"), 240, 0, 0, 1)
    for kw in (dict(depth=None), dict(idx=None), dict(K=None), dict(I=0), dict(H=0), dict(W=0), dict(w=0.0), dict(w=float("inf")),
               dict(w=float("nan")), dict(K=C.addressof(Kbad)), dict(pts=None), dict(M=0), dict(iters=0), dict(d1=0.0),
               dict(d0=0.001), dict(B=0), dict(max_n=-1), dict(ws=None), dict(off=None)):
        assert call(**kw) == -1, kw
