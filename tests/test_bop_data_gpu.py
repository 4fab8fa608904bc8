"""GPU checks of the BOP dataset layer: cppf_gt_visibility equal to the NumPy restatement (tests/bop_data_ref.py) on every
instance of the generated scenes, alone and batched, its cross-check with cppf_vsd_counts and its edge shapes; then
bop_data.write_dataset -> Dataset -> score on ground-truth, wrong and reordered results files, and eval.py --data=bop."""
import json
import os
import shutil
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bop_data_ref as DR  # noqa: E402


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The generated dataset (tests/bop_data_ref.scenes) written with bop_data.write_dataset, read back, and every instance's
    render alone with the restatement's figures for it."""
    dev = _gpu()
    from cppf2_amd import bop_data, render
    root = str(tmp_path_factory.mktemp("bop") / "gen")
    cv, cf = DR.cylinder()
    meshes = {DR.OBJ_FIXTURE: render.load_mesh(DR.FIXTURE, 0.001), DR.OBJ_CYL: render.Mesh(cv * 0.001, cf, 0.001)}
    scenes, occluders, holes = DR.scenes()
    occ = {k: [(render.Mesh(m[0], m[1]), R, t) for m, R, t in v] for k, v in occluders.items()}
    bop_data.write_dataset(root, "test", meshes, scenes, K=DR.K, height=DR.H, width=DR.W, models_info={DR.OBJ_CYL: DR.CYL_INFO},
                           occluders=occ, holes=holes)
    ds = bop_data.Dataset(root, "test")
    inst = []                                     # (scene, image, gt index, obj id)
    for s in ds.scene_ids:
        for im, lst in sorted(ds.scene(s)["gt"].items()):
            inst += [(s, im, g, e["obj_id"]) for g, e in enumerate(lst)]
    images = sorted({(s, im) for s, im, _, _ in inst})
    depth = ds.depths(images)
    idx = np.array([images.index((s, im)) for s, im, _, _ in inst], dtype=np.int32)
    gts = [ds.scene(s)["gt"][im][g] for s, im, g, _ in inst]
    poses = [np.hstack([e["R"], e["t"][:, None]]) for e in gts]
    ren = bop_data._render_alone([ds.mesh(o) for _, _, _, o in inst], poses, DR.K, DR.H, DR.W, dev).cpu().numpy()
    want = [DR.gt_visibility(depth[idx[n]], ren[n], DR.K) for n in range(len(inst))]
    return dict(root=root, ds=ds, scenes=scenes, inst=inst, images=images, depth=depth, idx=idx, gts=gts, ren=ren, want=want, dev=dev)


def test_generated_scenes_hold_the_cases(data):
    info = {}
    for (s, im, g, _), w in zip(data["inst"], data["want"]):
        info.setdefault((s, im), []).append(w[:2])
    DR.check_cases(data["scenes"], info)
    assert len(data["ds"].scene_ids) == 2 and len(data["images"]) >= 4 and data["depth"].shape[1:] == (480, 640)


def test_gt_visibility_equals_the_restatement_alone_and_batched(data):
    """Counts, both boxes and every mask byte equal the restatement's (integers: no tolerance), for all instances in one call
    and for each alone; the two are byte-identical.  The files write_dataset wrote hold the same figures."""
    from PIL import Image
    from cppf2_amd import bop
    c, b, m = bop.gt_visibility_counts(data["depth"], data["idx"], data["ren"], DR.K, masks=True)
    c, b, m = c.cpu().numpy(), b.cpu().numpy(), m.cpu().numpy()
    for n, (s, im, g, o) in enumerate(data["inst"]):
        wc, wb, wm = data["want"][n]
        print("instance", (s, im, g, o), "counts", c[n], "want", wc, "bbox", b[n], "want", wb)
        assert np.array_equal(c[n], wc) and np.array_equal(b[n], wb), (n, c[n], wc, b[n], wb)
        assert np.array_equal(m[n], wm), (n, int((m[n] != wm).sum()))
        c1, b1, m1 = bop.gt_visibility_counts(data["depth"][data["idx"][n]], 0, data["ren"][n:n + 1], DR.K, masks=True)
        assert c1.cpu().numpy().tobytes() == c[n].tobytes() and b1.cpu().numpy().tobytes() == b[n].tobytes()
        assert m1.cpu().numpy().tobytes() == m[n].tobytes()
        c0, b0, m0 = bop.gt_visibility_counts(data["depth"], data["idx"][n:n + 1], data["ren"][n:n + 1], DR.K, masks=False)
        assert m0 is None and np.array_equal(c0.cpu().numpy()[0], wc) and np.array_equal(b0.cpu().numpy()[0], wb)
        e = data["ds"].gt_info(s)[im][g]
        assert [e["px_count_all"], e["px_count_valid"], e["px_count_visib"]] == wc.tolist()
        assert e["bbox_obj"] + e["bbox_visib"] == wb.tolist() and e["visib_fract"] == wc[2] / max(wc[0], 1)
        png = np.array(Image.open(os.path.join(data["ds"].scene_dir(s), "mask_visib", "%06d_%06d.png" % (im, g))))
        assert np.array_equal(png, wm)
    # reversed order: the same rows
    r = np.arange(len(data["inst"]))[::-1].copy()
    c2, b2, m2 = bop.gt_visibility_counts(data["depth"], data["idx"][r], data["ren"][r], DR.K, masks=True)
    assert np.array_equal(c2.cpu().numpy(), c[r]) and np.array_equal(b2.cpu().numpy(), b[r]) and np.array_equal(m2.cpu().numpy(), m[r])
    # the high-level call (renders inside, several objects per call) gives the same figures
    ds = data["ds"]
    vis = bop.gt_visibility([ds.object(o) for _, _, _, o in data["inst"]], data["depth"], data["idx"], [e["R"] for e in data["gts"]],
                            [e["t"] for e in data["gts"]], DR.K, masks=True, chunk=4)
    assert np.array_equal(vis["px_count_visib"], c[:, 2]) and np.array_equal(vis["bbox_obj"], b[:, :4])
    assert np.array_equal(vis["bbox_visib"], b[:, 4:]) and np.array_equal(vis["mask_visib"], m)
    assert np.array_equal(vis["visib_fract"], c[:, 2] / np.maximum(c[:, 0], 1))


def test_visible_count_is_the_merged_kernels_union_and_intersection(data):
    """cppf_vsd_counts with est = gt = the instance's render: union = intersection = px_count_visib."""
    from cppf2_amd import bop
    v = bop.vsd_counts(data["depth"], data["idx"], data["ren"], data["ren"], DR.K, 0.2).cpu().numpy()
    for n, w in enumerate(data["want"]):
        assert v[n, 0] == v[n, 1] == w[0][2], (n, v[n, :2], w[0])


@pytest.mark.parametrize("shape", [(37, 53), (1, 1), (3, 1021), (33, 4)])
def test_gt_visibility_edge_shapes(shape):
    """H x W that is no multiple of four or of the block's stride (instances then start at unaligned mask bytes), an all-zero
    render, an all-zero test image, an image index out of range, and the null mask pointer."""
    import torch
    _gpu()
    from cppf2_amd import bop
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    Kmat = np.array([[40.0, 0, W / 2.0], [0, 41.0, H / 2.0], [0, 0, 1]])
    G, I = 7, 3
    test = np.where(rng.random((I, H, W)) < 0.7, rng.uniform(0.5, 1.5, (I, H, W)), 0).astype(np.float32)
    test[2] = 0.0                                                  # an image without readings: everything drawn is visible
    ren = np.where(rng.random((G, H, W)) < 0.6, rng.uniform(0.5, 1.5, (G, H, W)), 0).astype(np.float32)
    ren[1] = 0.0                                                   # nothing on screen
    idx = np.array([0, 1, 2, 2, 1, 5, -1], dtype=np.int32)         # the last two: outside [0, I)
    c, b, m = bop.gt_visibility_counts(test, idx, ren, Kmat, delta=0.05, masks=True)
    c, b, m = c.cpu().numpy(), b.cpu().numpy(), m.cpu().numpy()
    c0, b0, m0 = bop.gt_visibility_counts(test, idx, ren, Kmat, delta=0.05, masks=False)
    assert m0 is None and np.array_equal(c0.cpu().numpy(), c) and np.array_equal(b0.cpu().numpy(), b)
    for g in range(G):
        if 0 <= idx[g] < I:
            wc, wb, wm = DR.gt_visibility(test[idx[g]], ren[g], Kmat, 0.05)
        else:
            wc, wb, wm = np.zeros(3, np.int64), np.full(8, -1, np.int32), np.zeros((H, W), np.uint8)
        assert np.array_equal(c[g], wc) and np.array_equal(b[g], wb) and np.array_equal(m[g], wm), (g, c[g], wc, b[g], wb)
    assert c[1].tolist() == [0, 0, 0] and b[1].tolist() == [-1] * 8 and not m[1].any()
    assert c[2][0] == c[2][2] == int((ren[2] > 0).sum())
    assert c[2][1] == 0
    # G = 0 launches nothing
    c, b, m = bop.gt_visibility_counts(test, np.zeros(0, np.int32), np.zeros((0, H, W), np.float32), Kmat, masks=True)
    assert c.shape == (0, 3) and b.shape == (0, 8) and m.shape == (0, H, W)
    torch.cuda.synchronize()


def test_off_screen_instance_has_zero_fraction(data):
    from cppf2_amd import bop
    ds = data["ds"]
    e = data["gts"][0]
    vis = bop.gt_visibility(ds.object(DR.OBJ_FIXTURE), data["depth"][0], 0, [e["R"]], [e["t"] + np.array([5.0, 0, 0])], DR.K, masks=True)
    assert vis["px_count_all"].tolist() == [0] and vis["visib_fract"].tolist() == [0.0]
    assert vis["bbox_obj"].tolist() == [[-1] * 4] and vis["bbox_visib"].tolist() == [[-1] * 4] and not vis["mask_visib"].any()


def test_reader_computes_what_the_files_hold_when_they_are_absent(data, tmp_path):
    from cppf2_amd import bop_data
    root = str(tmp_path / "bare")
    shutil.copytree(data["root"], root)
    for s in data["ds"].scene_ids:
        os.remove(os.path.join(root, "test", "%06d" % s, "scene_gt_info.json"))
        shutil.rmtree(os.path.join(root, "test", "%06d" % s, "mask_visib"))
    bare = bop_data.Dataset(root, "test")
    for s in bare.scene_ids:
        assert bare.gt_info(s) == data["ds"].gt_info(s)
    for s, im, g, _ in data["inst"]:
        assert np.array_equal(bare.mask_visib(s, im, g), data["ds"].mask_visib(s, im, g))
    assert bare.targets() == data["ds"].targets() == bop_data.read_targets(os.path.join(root, "test_targets_bop19.json"))


def _gt_results(data, rot=None):
    from cppf2_amd import bop_data
    rows = [(s, im, o, 1.0 - 0.01 * n, e["cam_R_m2c"] if rot is None else e["cam_R_m2c"] @ rot, e["cam_t_m2c"])
            for n, ((s, im, g, o), e) in enumerate(zip(data["inst"], data["gts"]))]
    return bop_data.make_results(*[[r[k] for r in rows] for k in range(4)], np.array([r[4] for r in rows]), np.array([r[5] for r in rows]))


def test_score_of_ground_truth_wrong_and_reordered_results(data, tmp_path):
    from cppf2_amd import bop_data
    ds = data["ds"]
    targets = ds.targets()
    assert (0, 1, DR.OBJ_FIXTURE, 1) not in targets and (0, 1, DR.OBJ_CYL, 1) in targets      # the hidden instance is no target
    assert (1, 0, DR.OBJ_FIXTURE, 2) in targets
    p = str(tmp_path / "gt.csv")
    bop_data.write_results(p, _gt_results(data))
    rep = bop_data.score(ds, bop_data.read_results(p), os.path.join(data["root"], "test_targets_bop19.json"))
    print("score of the ground truth:", {k: rep[k] for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR")}, rep["counts"])
    n_valid = sum(w[0][2] / max(w[0][0], 1) >= 0.1 for w in data["want"])
    assert rep["targets"] == n_valid == len(data["inst"]) - 1 == sum(t[3] for t in targets)
    assert rep["counts"]["not_a_target"] == 1 and rep["counts"]["kept"] == n_valid
    for r in [rep] + list(rep["per_object"].values()):
        assert r["AR_VSD"] == r["AR_MSSD"] == r["AR_MSPD"] == r["AR"] == 1.0
        assert np.all(np.asarray(r["recall"]["vsd"]) == 1.0) and np.all(np.asarray(r["recall"]["mspd"]) == 1.0)
    # every estimate 90 degrees off about the model's z axis: no fixture instance within half a diameter
    Rz = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    off = bop_data.score(ds, _gt_results(data, Rz))
    print("90 degrees off:", {k: off[k] for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR")})
    assert off["per_object"][DR.OBJ_FIXTURE]["AR_MSSD"] == 0.0
    assert off["per_object"][DR.OBJ_CYL]["AR_MSSD"] == 1.0                  # the cylinder's own symmetry axis
    # the two fixtures of scene 1 image 0 with their poses swapped in the file: matching is by error, not by order
    res = _gt_results(data)
    two = [n for n, (s, im, g, o) in enumerate(data["inst"]) if (s, im, o) == (1, 0, DR.OBJ_FIXTURE)]
    assert len(two) == 2
    for k in ("R", "t"):
        res[k][two] = res[k][two[::-1]].copy()
    sw = bop_data.score(ds, res)
    for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR"):
        assert sw[k] == rep[k] == 1.0
    assert sw["matches"] == rep["matches"]


def _eval(data, tmp_path, name, **kw):
    import eval as E
    out_csv = str(tmp_path / (name + ".csv"))
    rep = E.main(data="bop", bop_root=data["root"], split="test", out_csv=out_csv, teacher_prior=True, num_pairs=20000, debug=True, **kw)
    return rep, out_csv


def _same_report(a, b):
    keys = ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR", "recall", "matches", "targets", "per_object")
    return all(a[k] == b[k] for k in keys)


def test_eval_over_the_generated_dataset(data, tmp_path):
    """eval.py --data=bop --teacher_prior: one CSV row per target instance, finite poses, and the file re-read and re-scored
    gives the printed report exactly.  The AR itself is measured, not asserted (untrained networks, a teacher prior)."""
    from cppf2_amd import bop_data
    ds = data["ds"]
    n_targets = sum(t[3] for t in ds.targets())
    rep, out_csv = _eval(data, tmp_path, "plain")
    res = bop_data.read_results(out_csv)
    print("eval --data=bop --teacher_prior:", {k: rep["bop"][k] for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR")}, rep["skipped"])
    assert len(res["score"]) == rep["rows"] == n_targets
    assert np.isfinite(res["R"]).all() and np.isfinite(res["t"]).all() and np.isfinite(res["score"]).all() and (res["time"] > 0).all()
    want = {(s, im, o): n for s, im, o, n in ds.targets()}
    got = {}
    for s, im, o in zip(res["scene_id"], res["im_id"], res["obj_id"]):
        got[(int(s), int(im), int(o))] = got.get((int(s), int(im), int(o)), 0) + 1
    assert got == want
    assert _same_report(bop_data.score(ds, res), rep["bop"])
    assert json.loads(json.dumps(rep["bop"]))["AR"] == rep["bop"]["AR"]


def test_eval_with_icp_and_verification_completes(data, tmp_path):
    from cppf2_amd import bop_data
    rep, out_csv = _eval(data, tmp_path, "icp_verify", icp_iters=30, hypotheses=8)
    print("eval --data=bop --teacher_prior --icp_iters=30 --hypotheses=8:",
          {k: rep["bop"][k] for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR")}, rep["skipped"])
    assert rep["rows"] == sum(t[3] for t in data["ds"].targets())
    for item in rep["results"]:
        assert item["model"] is not None and "verify" in item and "icp" in item
        assert 1 <= item["verify"]["hypotheses"] <= 8 and 0 <= item["verify"]["chosen"] < 8
    assert _same_report(bop_data.score(data["ds"], bop_data.read_results(out_csv)), rep["bop"])
    assert "verification" in rep and "icp_refinement" in rep
