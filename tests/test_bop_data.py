"""CPU checks of the BOP dataset layer (cppf2_amd/bop_data.py): the reader on a hand-written tiny folder and its errors, the
results CSV round trip, the selection and matching rules against the plain-loop restatement (tests/bop_data_ref.py), their tie
to bop.average_recall, and the generated scenes' preconditions by the NumPy renderer and the visibility restatement."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bop_data_ref as DR  # noqa: E402

TETRA = """ply
format ascii 1.0
element vertex 4
property float x
property float y
property float z
element face 4
property list uchar int vertex_indices
end_header
0 0 0
100 0 0
0 60 0
0 0 40
3 0 2 1
3 0 1 3
3 0 3 2
3 1 2 3
"""


def _tiny(tmp_path, gt_info=True, depth_shapes=((4, 6), (4, 6))):
    """A hand-written dataset: one tetrahedron (object 3, mm), one scene (id 5) of two images."""
    from PIL import Image
    root = tmp_path / "tiny"
    (root / "models").mkdir(parents=True)
    (root / "models" / "obj_000003.ply").write_text(TETRA)
    (root / "models" / "models_info.json").write_text(json.dumps({"3": {"diameter": 123.0}}))
    sd = root / "val" / "000005"
    (sd / "depth").mkdir(parents=True)
    Kl = [500.0, 0, 3.0, 0, 510.0, 2.0, 0, 0, 1]
    (sd / "scene_camera.json").write_text(json.dumps({"0": {"cam_K": Kl, "depth_scale": 0.1}, "7": {"cam_K": Kl, "depth_scale": 1.0}}))
    Rz = [0.0, -1.0, 0, 1.0, 0, 0, 0, 0, 1.0]
    gt = {"0": [{"cam_R_m2c": [1.0, 0, 0, 0, 1, 0, 0, 0, 1], "cam_t_m2c": [10.0, 20.0, 700.0], "obj_id": 3}],
          "7": [{"cam_R_m2c": Rz, "cam_t_m2c": [0.0, 0.0, 500.0], "obj_id": 3},
                {"cam_R_m2c": Rz, "cam_t_m2c": [50.0, 0.0, 900.0], "obj_id": 3}]}
    (sd / "scene_gt.json").write_text(json.dumps(gt))
    if gt_info:
        e = dict(bbox_obj=[0, 0, 2, 2], bbox_visib=[0, 0, 2, 1], px_count_all=4, px_count_valid=4, px_count_visib=2)
        (sd / "scene_gt_info.json").write_text(json.dumps({"0": [dict(e, visib_fract=0.5)],
                                                           "7": [dict(e, visib_fract=0.05), dict(e, visib_fract=1.0)]}))
    for im, shape in zip((0, 7), depth_shapes):
        Image.fromarray((np.arange(shape[0] * shape[1], dtype=np.uint16).reshape(shape) * 1000)).save(str(sd / "depth" / ("%06d.png" % im)))
    return root


def test_reader_on_a_hand_written_folder(tmp_path):
    from cppf2_amd import bop_data
    ds = bop_data.Dataset(str(_tiny(tmp_path)), "val")
    assert ds.scene_ids == [5]
    sc = ds.scene(5)
    assert sorted(sc["gt"]) == [0, 7] and len(sc["gt"][7]) == 2
    np.testing.assert_array_equal(sc["camera"][0]["K"], [[500, 0, 3], [0, 510, 2], [0, 0, 1]])
    obj = ds.object(3)
    assert obj.diameter == pytest.approx(0.123) and obj.verts.shape == (4, 3)
    np.testing.assert_allclose(obj.centre, [0.05, 0.03, 0.02])
    # record convention: R centre + t * scale
    g = sc["gt"][0][0]
    np.testing.assert_allclose(g["t"], np.array([0.05, 0.03, 0.02]) + np.array([0.01, 0.02, 0.7]), atol=1e-15)
    g = sc["gt"][7][1]
    np.testing.assert_allclose(g["t"], np.array([-0.03, 0.05, 0.02]) + np.array([0.05, 0.0, 0.9]), atol=1e-15)
    # depth: value * depth_scale / 1000 metres
    d0, d7 = ds.depth(5, 0), ds.depth(5, 7)
    assert d0.dtype == np.float32 and d0.shape == (4, 6)
    assert d0[0, 1] == np.float32(1000 * 0.1 / 1000) and d7[1, 0] == np.float32(6000 * 1.0 / 1000)
    assert ds.depths([(5, 0), (5, 7)]).shape == (2, 4, 6)
    assert ds.gt_info(5)[7][1]["visib_fract"] == 1.0
    # default targets: valid instances only (visib_fract >= 0.1), counted per object
    assert ds.targets() == [(5, 0, 3, 1), (5, 7, 3, 1)]
    assert ds.targets(visib_gt_min=0.01) == [(5, 0, 3, 1), (5, 7, 3, 2)]
    tf = tmp_path / "targets.json"
    tf.write_text(json.dumps([{"scene_id": 5, "im_id": 7, "obj_id": 3, "inst_count": 2}]))
    assert ds.targets(str(tf)) == [(5, 7, 3, 2)]
    # pose_to_bop is the inverse of pose_from_bop
    from cppf2_amd import bop
    Rb, tb = bop.pose_to_bop(g["R"], g["t"], 0.001, obj.centre)
    np.testing.assert_allclose(tb, [50.0, 0.0, 900.0], atol=1e-10)
    np.testing.assert_array_equal(Rb, g["cam_R_m2c"])


def test_reader_errors(tmp_path):
    from cppf2_amd import bop_data
    root = _tiny(tmp_path, depth_shapes=((4, 6), (5, 6)))
    ds = bop_data.Dataset(str(root), "val")
    with pytest.raises(bop_data.BopDataError, match="differs from the batch"):
        ds.depths([(5, 0), (5, 7)])
    with pytest.raises(bop_data.BopDataError, match="no model"):
        ds.object(4)
    os.makedirs(str(root / "val" / "000006"))
    ds = bop_data.Dataset(str(root), "val")
    assert ds.scene_ids == [5, 6]
    with pytest.raises(bop_data.BopDataError, match="scene_gt.json"):
        ds.scene(6)
    # a scene_gt entry whose object has no model
    gt = json.loads((root / "val" / "000005" / "scene_gt.json").read_text())
    gt["0"][0]["obj_id"] = 9
    (root / "val" / "000005" / "scene_gt.json").write_text(json.dumps(gt))
    with pytest.raises(bop_data.BopDataError, match="object 9 has no model"):
        bop_data.Dataset(str(root), "val").scene(5)
    with pytest.raises(bop_data.BopDataError, match="no such split"):
        bop_data.Dataset(str(root), "test")
    good = "1,2,3,0.5,1 0 0 0 1 0 0 0 1,1 2 3,-1\n"
    for bad, what in (("1,2,3,0.5,1 0 0 0 1 0 0 0,1 2 3,-1\n", "R has 8"), ("1,2,3,0.5,1 0 0 0 1 0 0 0 1,1 2,-1\n", "t has 2"),
                      ("1,2,3,0.5,1 0 0 0 x 0 0 0 1,1 2 3,-1\n", "could not convert")):
        p = tmp_path / "bad.csv"
        p.write_text(bop_data.RESULTS_HEADER + "\n" + good + bad)
        with pytest.raises(bop_data.BopDataError, match="line 3.*" + what):
            bop_data.read_results(str(p))


def test_results_csv_round_trip_is_bit_equal(tmp_path):
    from cppf2_amd import bop_data
    rng = np.random.default_rng(3)
    n = 40
    res = bop_data.make_results(rng.integers(0, 50, n), rng.integers(0, 2000, n), rng.integers(1, 31, n),
                                rng.standard_normal(n) * 10.0 ** rng.integers(-12, 12, n), rng.standard_normal((n, 3, 3)),
                                rng.standard_normal((n, 3)) * 1e3, np.where(rng.random(n) < 0.3, -1.0, rng.random(n)))
    res["score"][0], res["t"][1, 2], res["R"][2, 0, 0] = np.nextafter(1.0, 2.0), 5e-324, -0.0
    p = str(tmp_path / "r.csv")
    bop_data.write_results(p, res)
    back = bop_data.read_results(p)
    assert open(p).readline().strip() == "scene_id,im_id,obj_id,score,R,t,time"
    for k in res:
        assert back[k].dtype == res[k].dtype and back[k].tobytes() == res[k].tobytes(), k
    bop_data.write_results(p, bop_data.make_results([], [], [], [], np.zeros((0, 3, 3)), np.zeros((0, 3))))
    assert len(bop_data.read_results(p)["score"]) == 0


def _random_tables(rng, n_tables=40):
    """Seeded error tables with ties (errors drawn from a few values), invalid instances and up to 3 estimates x 3 instances."""
    tables = []
    for n in range(n_tables):
        n_est, n_gt = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        diam = float(rng.choice([0.1, 0.25]))
        grid = np.array([0.0, 0.04, 0.1, 0.1, 0.26, 0.44, 0.51, 0.9, np.inf])
        tables.append(dict(obj_id=int(rng.choice([2, 15])), score=rng.choice([0.2, 0.5, 0.5, 0.9], n_est),
                           valid=rng.random(n_gt) < 0.75, vsd=rng.choice(grid, (n_est, n_gt, 10)),
                           mssd=rng.choice(grid, (n_est, n_gt)) * diam, mspd=rng.choice(grid, (n_est, n_gt)) * 100.0,
                           diameter=diam, width=int(rng.choice([640, 1280]))))
    return tables


def test_matching_equals_the_plain_loop_restatement():
    from cppf2_amd import bop_data
    rng = np.random.default_rng(11)
    tables = _random_tables(rng)
    assert any(len(t["score"]) > len(t["valid"]) > 0 for t in tables) and any(not t["valid"].all() for t in tables)
    assert any(len(set(t["score"])) < len(t["score"]) for t in tables)                     # tied scores
    got = bop_data.recall_report(tables)
    want = DR.report(tables)
    for key, w in want.items():
        g = got if key is None else got["per_object"][key]
        assert g["targets"] == w["targets"]
        for name in ("vsd", "mssd", "mspd"):
            assert np.array_equal(np.asarray(g["matches"][name]), w[name]), (key, name)
            np.testing.assert_allclose(g["AR_" + name.upper()], np.mean(w[name] / w["targets"]), rtol=0, atol=1e-15)
            np.testing.assert_allclose(np.asarray(g["recall"][name]), w[name] / w["targets"], rtol=0, atol=0)
    assert got["AR"] == (got["AR_VSD"] + got["AR_MSSD"] + got["AR_MSPD"]) / 3.0
    # the assignments, one threshold at a time
    for t in tables:
        order = np.argsort(-t["score"], kind="stable")
        m, assign = bop_data.greedy_matches(t["mssd"][order][:, None, :], np.asarray(DR.THETAS) * t["diameter"], t["valid"])
        for j, th in enumerate(DR.THETAS):
            want_a = DR.match_one(t["mssd"], t["score"], t["valid"], th * t["diameter"])
            assert [int(a) for a in assign[:, j]] == [want_a[e] for e in order]


def test_selection_keeps_the_best_inst_count_in_file_order_on_ties():
    from cppf2_amd import bop_data
    rng = np.random.default_rng(12)
    n = 60
    res = bop_data.make_results(rng.integers(0, 2, n), rng.integers(0, 3, n), rng.choice([2, 15, 30], n),
                                rng.choice([0.1, 0.5, 0.5, 0.8], n), np.tile(np.eye(3), (n, 1, 1)), np.zeros((n, 3)))
    targets = [(s, i, o, int(rng.integers(1, 3))) for s in range(2) for i in range(3) for o in (2, 15)]
    kept, counts = bop_data.select_estimates(res, targets)
    rows = list(zip(res["scene_id"].tolist(), res["im_id"].tolist(), res["obj_id"].tolist(), res["score"].tolist()))
    want, ignored = DR.select(rows, targets)
    assert kept == want
    assert counts["not_a_target"] == ignored == int(np.sum(res["obj_id"] == 30)) > 0
    assert counts["estimates"] == n and counts["kept"] == sum(len(v) for v in want.values())
    assert counts["over_inst_count"] == n - ignored - counts["kept"] > 0


def test_one_estimate_per_valid_instance_equals_average_recall_exactly():
    """One estimate per instance, one instance per (image, object), all valid: the recalls are bop.average_recall's, bit for bit."""
    from cppf2_amd import bop, bop_data
    rng = np.random.default_rng(13)
    P = 37
    diam = 0.17
    err = dict(vsd=rng.random((P, 10)) * 0.7, mssd=rng.random(P) * 0.6 * diam, mspd=rng.random(P) * 60.0)
    err["vsd"][0, 3], err["mssd"][1], err["mspd"][2] = 0.2, 0.25 * diam, 25.0           # errors on a threshold: strict '<'
    tables = [dict(obj_id=15, score=[1.0], valid=[True], vsd=err["vsd"][p][None, None], mssd=err["mssd"][p].reshape(1, 1),
                   mspd=err["mspd"][p].reshape(1, 1), diameter=diam, width=640) for p in range(P)]
    got = bop_data.recall_report(tables)
    want = bop.average_recall(err, diam, 640)
    for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR"):
        assert got[k] == want[k], k
    assert got["per_object"][15]["AR"] == want["AR"] and got["targets"] == P


def test_an_estimate_takes_the_lower_error_and_score_order_decides_who_is_left():
    from cppf2_amd import bop_data
    # estimate 0 passes the threshold against both instances: it takes instance 1 (the lower error)
    err = np.array([[[0.30, 0.10]], [[0.20, 0.90]]])                                     # [n_est, 1, n_gt]
    m, assign = bop_data.greedy_matches(err, [0.5], [True, True])
    assert m.tolist() == [2] and assign[:, 0].tolist() == [1, 0]
    # both estimates want instance 1 (errors 0.10 and 0.32); thresholds 0.2 (only the first passes) and 0.4 (both pass)
    err = np.array([[[0.90, 0.10]], [[0.90, 0.32]]])
    m, assign = bop_data.greedy_matches(err, [0.2, 0.4], [True, True])                    # the 0.10 estimate has the higher score
    assert m.tolist() == [1, 1] and assign.tolist() == [[1, 1], [-1, -1]]
    m, assign = bop_data.greedy_matches(err[::-1], [0.2, 0.4], [True, True])              # scores swapped: the 0.32 one goes first
    assert m.tolist() == [1, 1] and assign.tolist() == [[-1, 1], [1, -1]]                 # at 0.4 the other one is left unmatched
    # through recall_report the order comes from the scores, not from the file; the counts are the same either way
    tab = dict(obj_id=1, valid=[True, True], vsd=np.ones((2, 2, 1)), mspd=np.full((2, 2), np.inf), diameter=1.0, width=640,
               mssd=err[:, 0, :])
    a = bop_data.recall_report([dict(tab, score=[0.9, 0.1])])["matches"]["mssd"]
    b = bop_data.recall_report([dict(tab, score=[0.1, 0.9])])["matches"]["mssd"]
    assert a == b == [0, 0, 1, 1, 1, 1, 1, 1, 1, 1]                                      # 0.10 < theta from theta = 0.15 on
    # an invalid instance is never taken, and +inf / NaN never match
    m, _ = bop_data.greedy_matches(np.array([[[0.1, np.nan, np.inf]]]), [0.5], [False, True, True])
    assert m.tolist() == [0]


def test_generated_scenes_hold_the_cases_by_the_restatement():
    """The scenes of tests/bop_data_ref.py rendered with the NumPy mirror of the rasterizer (tests/render_ref.py) and composed
    as bop_data.write_dataset composes them: the visibility restatement finds every case the GPU tests rely on."""
    from cppf2_amd import render
    mesh = render.load_mesh(DR.FIXTURE, 0.001)
    cv, cf = DR.cylinder()
    models = {DR.OBJ_FIXTURE: (mesh.verts - mesh.bounds.mean(0), mesh.faces), DR.OBJ_CYL: (cv * 0.001, cf)}
    scenes, occluders, holes = DR.scenes()
    assert len(scenes) == 2 and sum(len(s) for s in scenes) >= 4
    info = {}
    for s, images in enumerate(scenes):
        for im, inst in enumerate(images):
            rs = [DR.render_alone(*models[o], R, t) for o, R, t in inst]
            ro = [DR.render_alone(m[0], m[1], R, t) for m, R, t in occluders.get((s, im), [])]
            stack = np.stack(rs + ro)
            d = np.where(stack > 0, stack, np.inf).min(0)
            d[np.isinf(d)] = 0
            if (s, im) in holes:
                d[holes[(s, im)]] = 0
            d = (np.rint(d.astype(np.float64) * 1e4).astype(np.uint16).astype(np.float64) * 0.1 / 1000.0).astype(np.float32)
            info[(s, im)] = [DR.gt_visibility(d, r, DR.K)[:2] for r in rs]
    DR.check_cases(scenes, info)
