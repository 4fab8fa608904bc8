"""CPU checks of the BOP scorer's host side (cppf2_amd/bop.py) and of its NumPy restatement (tests/bop_ref.py): the symmetry
sets and their frame conversion, pose_from_bop, the average recall, and the VSD arithmetic on hand-built depth maps."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bop_ref as BR  # noqa: E402

K = np.array([[591.0125, 0, 320], [0, 590.16775, 240], [0, 0, 1]])


def _box_mesh(size=(40.0, 40.0, 80.0), origin=(10.0, 20.0, 5.0), scale=0.001):
    """An axis-aligned box in millimetres (corner at origin), loaded at `scale`, with its 4-fold symmetry about z."""
    from cppf2_amd import render
    o = np.asarray(origin)
    v = np.array([[x, y, z] for x in (0, size[0]) for y in (0, size[1]) for z in (0, size[2])], dtype=np.float64) + o
    f = np.array([[0, 1, 2]], dtype=np.int32)
    return render.Mesh(v * scale, f, scale), o + np.asarray(size) / 2


def _cylinder_mesh(n=315, r=30.0, h=100.0, offset=(5.0, -7.0, 12.0), scale=0.001):
    from cppf2_amd import render
    a = 2 * np.pi * np.arange(n) / n
    ring = np.stack([r * np.cos(a), r * np.sin(a)], -1)
    v = np.concatenate([np.hstack([ring, np.zeros((n, 1))]), np.hstack([ring, np.full((n, 1), h)])]) + np.asarray(offset)
    return render.Mesh(v * scale, np.array([[0, 1, n]], dtype=np.int32), scale)


def _rz(deg):
    a = np.deg2rad(deg)
    M = np.eye(4)
    M[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    return M


def _about(M, point):
    """The 4x4 map M applied about `point` (model units): x -> R (x - p) + p."""
    T = M.copy()
    T[:3, 3] = point - M[:3, :3] @ point
    return T


def _maps_onto_itself(obj, tol):
    for s in obj.syms:
        w = obj.verts @ s[:, :3].T + s[:, 3]
        d = np.sqrt(((w[:, None, :] - obj.verts[None, :, :]) ** 2).sum(-1)).min(1)
        assert d.max() <= tol, d.max()


def test_symmetry_set_sizes_and_identity():
    from cppf2_amd import bop
    mesh, c = _box_mesh()
    disc = [_about(_rz(a), c).reshape(-1).tolist() for a in (90, 180, 270)]
    for info, n in (({}, 1), ({"symmetries_discrete": disc}, 4),
                    ({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": c.tolist()}]}, 315),
                    ({"symmetries_discrete": disc[1:2], "symmetries_continuous": [{"axis": [0, 0, 1], "offset": c.tolist()}]}, 630)):
        obj = bop.ObjectInfo.from_mesh(mesh, info)
        assert obj.syms.shape == (n, 3, 4)
        assert np.array_equal(obj.syms[0], np.hstack([np.eye(3), np.zeros((3, 1))]))
    assert bop.N_CONT == 315


def test_box_symmetries_map_the_box_onto_itself():
    """A box with 90-degree steps about its vertical axis (models_info in millimetres, offset corner): every converted transform
    maps the centred metre-frame vertices onto themselves, and the set equals the restatement's matrix composition."""
    from cppf2_amd import bop
    mesh, c = _box_mesh()
    info = {"symmetries_discrete": [_about(_rz(a), c).reshape(-1).tolist() for a in (90, 180, 270)]}
    obj = bop.ObjectInfo.from_mesh(mesh, info)
    _maps_onto_itself(obj, 1e-12)
    np.testing.assert_allclose(obj.syms, BR.symmetries(info, 0.001, obj.centre), atol=1e-14)


def test_cylinder_continuous_symmetry_maps_the_cylinder_onto_itself():
    from cppf2_amd import bop
    off = np.array([5.0, -7.0, 12.0])
    mesh = _cylinder_mesh(offset=off)
    info = {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": off.tolist()}]}
    obj = bop.ObjectInfo.from_mesh(mesh, info)
    assert obj.syms.shape[0] == 315
    _maps_onto_itself(obj, 1e-12)
    np.testing.assert_allclose(obj.syms, BR.symmetries(info, 0.001, obj.centre), atol=1e-14)
    # without the offset the rotation axis misses the cylinder's own: the set no longer maps it onto itself
    bad = bop.ObjectInfo.from_mesh(mesh, {"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]})
    with pytest.raises(AssertionError):
        _maps_onto_itself(bad, 1e-6)


def test_models_info_units_and_diameter():
    from cppf2_amd import bop
    mesh, c = _box_mesh()
    obj = bop.ObjectInfo.from_mesh(mesh)
    assert obj.diameter == pytest.approx(np.sqrt(40 ** 2 + 40 ** 2 + 80 ** 2) * 1e-3, rel=1e-12)
    np.testing.assert_allclose(obj.centre, c * 1e-3, atol=1e-15)
    np.testing.assert_allclose(obj.verts.mean(0), 0, atol=1e-15)
    assert bop.ObjectInfo.from_mesh(mesh, {"diameter": 123.0}).diameter == pytest.approx(0.123, rel=1e-12)
    assert bop.ObjectInfo.from_mesh(mesh, {"diameter": 123.0}, mesh_scale=0.01).diameter == pytest.approx(1.23, rel=1e-12)
    # a translation of 10 mm along x in the model's units becomes 1 cm in the metre frame
    T = np.eye(4)
    T[0, 3] = 10.0
    s = bop.ObjectInfo.from_mesh(mesh, {"symmetries_discrete": [T.reshape(-1).tolist()]}).syms[1]
    np.testing.assert_allclose(s[:, 3], [0.01, 0, 0], atol=1e-15)
    # the chunked brute force over all vertices agrees with the hull's
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((700, 3))
    want = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1).max())
    assert bop.diameter(pts) == pytest.approx(want, rel=1e-14)
    assert bop.diameter(pts[:1]) == 0.0 and bop.diameter(pts[:2]) == pytest.approx(np.linalg.norm(pts[0] - pts[1]))


def test_pose_from_bop_round_trip_against_camera_pose():
    """A record pose from render.camera_pose (centred model, metres), written as BOP writes it (uncentred model, millimetres),
    comes back through pose_from_bop."""
    from cppf2_amd import bop, render
    mesh, c = _box_mesh()
    centre = c * 1e-3
    Rs, ts, Rb, tb = [], [], [], []
    for i in range(5):
        Rm, tr = render.sample_pose(render.item_rng(7, i), True)
        P = render.camera_pose(Rm, tr, 1.0, centre).astype(np.float64).reshape(3, 4)
        R = np.linalg.svd(P[:, :3])[0] @ np.linalg.svd(P[:, :3])[2]          # re-orthonormalised (camera_pose is float32)
        t = P[:, 3]
        Rs.append(R); ts.append(t)
        Rb.append(R); tb.append((t - R @ centre) / 1e-3)
    R1, t1 = bop.pose_from_bop(Rb[0], tb[0], 1e-3, centre)
    np.testing.assert_allclose(R1, Rs[0], atol=0)
    np.testing.assert_allclose(t1, ts[0], atol=1e-12)
    Rn, tn = bop.pose_from_bop(np.stack(Rb), np.stack(tb), 1e-3, centre)
    np.testing.assert_allclose(tn, np.stack(ts), atol=1e-12)
    # the converted pose maps the centred vertices where BOP's pose maps the uncentred millimetre ones (in metres)
    x_mm = mesh.verts / 1e-3
    cam_bop = (x_mm @ Rb[1].T + tb[1]) * 1e-3
    cam_rec = (mesh.verts - centre) @ Rn[1].T + tn[1]
    np.testing.assert_allclose(cam_rec, cam_bop, atol=1e-12)


def test_load_pose(tmp_path):
    from cppf2_amd import bop
    M = np.arange(12, dtype=np.float64).reshape(3, 4)
    np.savetxt(tmp_path / "p.txt", M)
    np.save(tmp_path / "p.npy", np.vstack([M, [0, 0, 0, 1]]))
    for p in ("p.txt", "p.npy"):
        R, t = bop.load_pose(str(tmp_path / p))
        assert np.array_equal(R, M[:, :3]) and np.array_equal(t, M[:, 3])
    np.savetxt(tmp_path / "bad.txt", np.zeros((2, 3)))
    with pytest.raises(ValueError):
        bop.load_pose(str(tmp_path / "bad.txt"))


def test_average_recall_thresholds_are_strict():
    from cppf2_amd import bop
    th = np.asarray(bop.THETAS)
    # VSD exactly at a threshold does not count: 0.05 passes 9 of 10 thresholds at every tau
    e = dict(vsd=np.full((1, 10), 0.05), mssd=np.array([0.0]), mspd=np.array([0.0]))
    ar = bop.average_recall(e, 0.1, 640)
    assert ar["AR_VSD"] == pytest.approx(0.9) and ar["AR_MSSD"] == 1.0 and ar["AR_MSPD"] == 1.0
    # MSSD at theta * diameter, MSPD at 5 px (width 640) and at 10 px with width 1280: strict
    e = dict(vsd=np.zeros((1, 10)), mssd=np.array([0.25 * 0.2]), mspd=np.array([5.0]))
    ar = bop.average_recall(e, 0.2, 640)
    assert ar["AR_MSSD"] == pytest.approx(np.mean(0.25 * 0.2 < th * 0.2)) and ar["AR_MSPD"] == pytest.approx(0.9)
    assert bop.average_recall(dict(e, mspd=np.array([10.0])), 0.2, 1280)["AR_MSPD"] == pytest.approx(0.9)
    assert bop.average_recall(dict(e, mspd=np.array([10.0])), 0.2, 640)["AR_MSPD"] == pytest.approx(0.8)
    # misses (+inf) never count; AR is the mean of the three; the restatement agrees
    rng = np.random.default_rng(3)
    vsd = rng.uniform(0, 0.6, (20, 10))
    vsd[3] = np.inf
    mssd, mspd = rng.uniform(0, 0.05, 20), rng.uniform(0, 60, 20)
    mssd[3] = mspd[3] = np.inf
    ar = bop.average_recall(dict(vsd=vsd, mssd=mssd, mspd=mspd), 0.1, 640)
    want = BR.average_recall(vsd, mssd, mspd, 0.1, 640)
    for k in want:
        assert ar[k] == pytest.approx(want[k], abs=1e-15), k
    assert ar["AR"] == pytest.approx((ar["AR_VSD"] + ar["AR_MSSD"] + ar["AR_MSPD"]) / 3)
    miss = bop.average_recall(dict(vsd=np.full((1, 10), np.inf), mssd=[np.inf], mspd=[np.inf]), 0.1, 640)
    assert miss == dict(AR_VSD=0.0, AR_MSSD=0.0, AR_MSPD=0.0, AR=0.0)
    with pytest.raises(ValueError):
        bop.average_recall(dict(vsd=np.zeros((0, 10)), mssd=[], mspd=[]), 0.1, 640)


def test_vsd_errors_from_counts():
    from cppf2_amd import bop
    c = np.array([[10, 10, 0, 0], [10, 4, 2, 1], [0, 0, 0, 0]], dtype=np.int64)
    e = bop.vsd_errors(c)
    np.testing.assert_array_equal(e, [[0.0, 0.0], [0.8, 0.7], [1.0, 1.0]])
    np.testing.assert_array_equal(e, BR.vsd_errors(c))


def _plane(H, W, z, box):
    d = np.zeros((H, W), dtype=np.float32)
    r0, r1, c0, c1 = box
    d[r0:r1, c0:c1] = z
    return d


def test_restatement_on_hand_built_depth_maps():
    H, W, taus = 24, 32, np.arange(1, 11) * 0.05
    K_ = np.array([[30.0, 0, 16], [0, 30.0, 12], [0, 0, 1]])
    gt = _plane(H, W, 1.0, (4, 14, 6, 20))
    # identical poses: every visible pixel aligned, error 0 at every tau
    c, _ = BR.vsd_counts(gt, gt, gt, K_, 0.015, 0.1, taus)
    assert c[0] == c[1] == 140 and not c[2:].any()
    assert not BR.vsd_errors(c).any()
    # disjoint masks: intersection empty, error 1
    est = _plane(H, W, 1.0, (15, 20, 22, 30))
    test = np.maximum(gt, est)
    c, _ = BR.vsd_counts(test, est, gt, K_, 0.015, 0.1, taus)
    assert c[0] == 140 + 40 and c[1] == 0 and (BR.vsd_errors(c) == 1).all()
    # an empty union: error 1
    z = np.zeros((H, W), dtype=np.float32)
    c, _ = BR.vsd_counts(gt, z, z, K_, 0.015, 0.1, taus)
    assert c[0] == 0 and (BR.vsd_errors(c) == 1).all()
    # a hole in the test depth counts as visible: occluded by a nearer surface, the gt is not visible -- unless the test
    # image has no reading there
    occ = gt.copy()
    occ[4:14, 6:13] = 0.5
    c, _ = BR.vsd_counts(occ, gt, gt, K_, 0.015, 0.1, taus)
    assert c[0] == c[1] == 70
    holed = occ.copy()
    holed[4:14, 6:9] = 0.0
    c, _ = BR.vsd_counts(holed, gt, gt, K_, 0.015, 0.1, taus)
    assert c[0] == c[1] == 100
    # an estimate 2 cm behind the truth (diameter 0.1): misaligned at tau < 0.2 (step cost), error = cost / union
    far = _plane(H, W, 1.02, (4, 14, 6, 20))
    c, near = BR.vsd_counts(gt, far, gt, K_, 0.05, 0.1, taus, near=1e-12)
    assert c[0] == c[1] == 140
    e = BR.vsd_errors(c)
    assert (e[:3] == 1).all() and (e[4:] == 0).all() and near == 0
    # the distance conversion: a pixel off the principal point sees a longer ray than its depth
    f = BR.dist_factor(H, W, K_)
    assert f[12, 16] == 1.0 and f[0, 0] == np.sqrt((16 / 30.0) ** 2 + (12 / 30.0) ** 2 + 1)


UNIT_K = np.array([[2.0 ** 40, 0, 0], [0, 2.0 ** 40, 0], [0, 0, 1]])      # dist_factor = 1 exactly: D = d


def test_dist_factor_is_one_under_the_unit_k_and_at_the_principal_point_only():
    assert (BR.dist_factor(127, 129, UNIT_K) == 1.0).all()
    f = BR.dist_factor(24, 32, np.array([[30.0, 0, 16], [0, 30.0, 12], [0, 0, 1]]))
    assert f[12, 16] == 1.0 and np.count_nonzero(f == 1.0) == 1 and (f >= 1.0).all()


def test_vsd_restatement_at_exact_ties():
    """delta = 2^-6, thresholds 2^-5 and 2^-3, every D equal to its depth: a gap equal to delta is visible and one float32 more
    is not; a difference equal to thr_0 costs and one float32 less does not."""
    f = np.float32
    one = np.ones((1, 8), f)
    dt, de = one.copy(), one.copy()
    dt[0, 0] = f(1) - f(2.0 ** -6)
    dt[0, 1] = np.nextafter(dt[0, 0], f(0))
    de[0, 2] = f(1) + f(2.0 ** -5)
    de[0, 3] = np.nextafter(de[0, 2], f(1))
    c, _ = BR.vsd_counts(dt, de, one, UNIT_K, 2.0 ** -6, 0.25, (0.125, 0.5))
    assert c.tolist() == [7, 7, 1, 0]


def test_vsd_restatement_at_special_values():
    """NaN and negative test depths hide the pixel, -0.0 and 0 are holes (visible), +inf lies behind everything (visible); a NaN,
    -0.0 or negative estimate or ground truth is not drawn; an estimate at +inf over a visible ground truth costs at every tau."""
    f = np.float32
    nan, inf = f(np.nan), f(np.inf)
    dt = np.array([[nan, -1, -0.0, inf, 0, 1, 1, 1]], f)
    de = np.array([[1, 1, 1, 1, nan, inf, -0.0, -2]], f)
    dg = np.array([[1, 1, 1, 1, 1, 1, nan, inf]], f)
    c, _ = BR.vsd_counts(dt, de, dg, UNIT_K, 2.0 ** -6, 0.25, (0.125, 0.5))
    assert c.tolist() == [4, 3, 1, 1]
