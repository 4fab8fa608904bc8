"""GPU checks of the detections path end to end: generated scenes in front of a wall (bop_data.write_dataset), detections that
are each valid instance's visible mask dilated by a few pixels plus a false positive on the wall and a low-score duplicate;
the precondition that the dilation really bleeds and that the restatement's cleaning removes exactly the bleed; the GPU
cleaning equal to the restatement; eval.py --data=bop --detections bit-equal to the ground-truth-mask run on exact masks; and
the row rules of the dirty run with --clean_masks."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bop_data_ref as DR  # noqa: E402
import mask_ref as MR  # noqa: E402
import render_ref as RR  # noqa: E402

DILATE = 4                  # pixels (4-neighbour steps): a detector's bleed
JUMP = 0.01
WALL_Z = 1.6                # metres: behind everything, several jumps away from every object
OBJ_NONE = 99               # an object id no target has


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _dilate(m, steps):
    m = m.copy()
    for _ in range(steps):
        g = m.copy()
        g[1:] |= m[:-1]; g[:-1] |= m[1:]; g[:, 1:] |= m[:, :-1]; g[:, :-1] |= m[:, 1:]
        m = g
    return m


def _scenes(seed=13):
    """One scene, three images in front of the wall: (0) the fixture and the cylinder side by side; (1) the fixture partly behind
    the box (0.25 m nearer), a cylinder; (2) two fixtures (inst_count = 2)."""
    rng = np.random.default_rng(seed)
    p = lambda t: (RR.random_rotation(rng), np.asarray(t, dtype=np.float64))        # noqa: E731
    images = [[(DR.OBJ_FIXTURE,) + p((-0.12, 0.02, 0.80)), (DR.OBJ_CYL,) + p((0.20, -0.05, 0.70))],
              [(DR.OBJ_FIXTURE,) + p((0.05, 0.03, 0.85)), (DR.OBJ_CYL,) + p((-0.22, 0.08, 0.80))],
              [(DR.OBJ_FIXTURE,) + p((-0.18, -0.06, 0.90)), (DR.OBJ_FIXTURE,) + p((0.14, 0.08, 1.00))]]
    wall = (DR.box((1.5, 1.2, 0.01)), np.eye(3), np.array([0.0, 0.0, WALL_Z]))
    occluders = {(0, 0): [wall], (0, 1): [(DR.box(), np.eye(3), np.array([0.165, 0.03, 0.60])), wall], (0, 2): [wall]}
    return [images], occluders


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("bopdet") / "gen"), _gpu())


def build(root, dev):
    """The dataset, its valid instances with their exact and dilated masks and pixel owners, and the two detections files."""
    from cppf2_amd import bop_data, masks, render
    cv, cf = DR.cylinder()
    meshes = {DR.OBJ_FIXTURE: render.load_mesh(DR.FIXTURE, 0.001), DR.OBJ_CYL: render.Mesh(cv * 0.001, cf, 0.001)}
    scenes, occluders = _scenes()
    occ = {k: [(render.Mesh(m[0], m[1]), R, t) for m, R, t in v] for k, v in occluders.items()}
    bop_data.write_dataset(root, "test", meshes, scenes, K=DR.K, height=DR.H, width=DR.W, models_info={DR.OBJ_CYL: DR.CYL_INFO},
                           occluders=occ)
    ds = bop_data.Dataset(root, "test")
    targets = ds.targets()
    inst = []                # per valid instance in target order: dict(scene, im, g, obj, visib, dirty, owner, wall (its owner index))
    for s, im, o, _ in targets:
        gts = ds.scene(s)["gt"][im]
        info = ds.gt_info(s)[im]
        # every mesh of the image rendered alone: who owns each pixel of the depth image
        poses = [np.hstack([e["R"], e["t"][:, None]]) for e in gts] + [np.hstack([R, t[:, None]]) for _, R, t in occ[(s, im)]]
        ren = bop_data._render_alone([ds.mesh(e["obj_id"]) for e in gts] + [m for m, _, _ in occ[(s, im)]], poses, DR.K, DR.H,
                                     DR.W, dev).cpu().numpy()
        owner = np.where(ren > 0, ren, np.inf).argmin(0)
        owner[~(ren > 0).any(0)] = -1
        for g, e in enumerate(gts):
            if e["obj_id"] == o and info[g]["visib_fract"] >= bop_data.VISIB_GT_MIN:
                visib = ds.mask_visib(s, im, g)
                inst.append(dict(scene=s, im=im, g=g, obj=o, visib=visib, dirty=_dilate(visib, DILATE), owner=owner,
                                 wall=len(gts) + len(occ[(s, im)]) - 1))
    H, W = DR.H, DR.W

    def det(i, mask, score):
        return dict(scene_id=i["scene"], image_id=i["im"], category_id=i["obj"], bbox=masks.bbox(mask), score=score, time=0.0,
                    size=(H, W), counts=masks.rle_encode(mask))
    exact = [det(i, i["visib"], 1.0) for i in inst]
    dirty = [det(i, i["dirty"], 0.9 - 0.01 * n) for n, i in enumerate(inst)]
    # a false positive on the wall (a disc in the top right corner of image 0, as the fixture), a low-score duplicate of the first
    # detection, one below the score threshold and one of an object no target has
    rr, cc = np.mgrid[0:H, 0:W]
    fp = (rr - 60) ** 2 + (cc - 560) ** 2 <= 40 ** 2
    extra = [det(dict(inst[0], scene=0, im=0, obj=DR.OBJ_FIXTURE), fp, 0.5), dict(dirty[0], score=0.3),
             dict(dirty[1], score=0.05), dict(dirty[0], category_id=OBJ_NONE)]
    p_exact, p_dirty = os.path.join(root, "dets_exact.json"), os.path.join(root, "dets_dirty.json")
    bop_data.write_detections(p_exact, exact)
    bop_data.write_detections(p_dirty, dirty + extra, compress=False)
    return dict(root=root, ds=ds, targets=targets, inst=inst, fp=fp, exact=p_exact, dirty=p_dirty, n_dirty=len(dirty), dev=dev)


def test_dilated_masks_bleed_and_cleaning_removes_exactly_the_bleed(data):
    """By the renders alone every dilated mask holds pixels another mesh owns (the wall, the box); by the restatement alone the
    kept component holds none of them and covers the largest depth-connected component of the exact mask up to its rim
    pixels.  Then the GPU result is the restatement's, byte for byte."""
    from cppf2_amd import masks
    ds = data["ds"]
    assert len(data["inst"]) == 6 and sum(t[3] for t in data["targets"]) == 6 and (0, 2, DR.OBJ_FIXTURE, 2) in data["targets"]
    for n, i in enumerate(data["inst"]):
        depth = ds.depth(i["scene"], i["im"])
        assert (depth > 0).all(), "the wall fills the image"
        foreign = i["dirty"] & (i["owner"] != i["g"])
        kept, stats = MR.components(i["dirty"], depth, JUMP, masks.MIN_PIXELS)
        core, cstats = MR.components(i["visib"], depth, JUMP, masks.MIN_PIXELS)
        rim = i["visib"] & _dilate(~i["visib"], 1)
        print("instance", n, (i["scene"], i["im"], i["g"], i["obj"]), "visible", int(i["visib"].sum()), "dilated", int(i["dirty"].sum()),
              "foreign", int(foreign.sum()), "kept", stats.tolist(), "core", cstats.tolist(), "rim", int(rim.sum()))
        assert foreign.sum() > 100, "the dilation does not reach another mesh"
        assert (i["dirty"] & (i["owner"] == i["wall"])).sum() > 50, "the mask does not bleed onto the wall"
        assert stats[1] >= 0 and not ((kept > 0) & foreign).any(), "bleed pixels survive the cleaning"
        assert cstats[1] >= 0
        assert not ((core > 0) & ~rim & ~(kept > 0)).any(), "the kept component misses part of the instance"
        got, gstats = masks.clean(i["dirty"][None], depth, 0, jump=JUMP)
        assert got.cpu().numpy()[0].tobytes() == kept.tobytes() and gstats.cpu().numpy()[0].tolist() == stats.tolist()
    # image 1: the fixture's mask also bleeds onto the box in front of it (the owner after the image's instances)
    i = [i_ for i_ in data["inst"] if (i_["im"], i_["obj"]) == (1, DR.OBJ_FIXTURE)][0]
    assert (i["dirty"] & (i["owner"] == len(ds.scene(0)["gt"][1]))).sum() > 50 and i["wall"] == len(ds.scene(0)["gt"][1]) + 1
    # the false positive lies on the wall alone
    assert data["inst"][0]["im"] == 0 and (data["inst"][0]["owner"][data["fp"]] == data["inst"][0]["wall"]).all()
    # all dirty masks of an image in one call, against the image they share
    for im in (0, 1, 2):
        grp = [i for i in data["inst"] if i["im"] == im]
        depth = ds.depth(0, im)
        got, gstats = masks.clean(np.stack([i["dirty"] for i in grp]), depth, 0, jump=JUMP)
        for k, i in enumerate(grp):
            kept, stats = MR.components(i["dirty"], depth, JUMP, masks.MIN_PIXELS)
            assert got.cpu().numpy()[k].tobytes() == kept.tobytes() and gstats.cpu().numpy()[k].tolist() == stats.tolist()


def _eval(data, tmp_path, name, **kw):
    import eval as E
    out_csv = str(tmp_path / (name + ".csv"))
    kw.setdefault("teacher_prior", True)
    rep = E.main(data="bop", bop_root=data["root"], split="test", out_csv=out_csv, num_pairs=20000, debug=True, seed=3,
                 batch_instances=4, **kw)
    return rep, out_csv


def test_exact_mask_detections_give_the_ground_truth_mask_run_bit_for_bit(data, tmp_path):
    """Detections that are the exact mask_visib masks at score 1 in target order, no cleaning, the teacher prior on: R and t of
    every CSV row are bit-equal to the ground-truth-mask run's with the same seed and batch size."""
    from cppf2_amd import bop_data
    rep_gt, csv_gt = _eval(data, tmp_path, "gt")
    rep_det, csv_det = _eval(data, tmp_path, "det", detections=data["exact"])
    a, b = bop_data.read_results(csv_gt), bop_data.read_results(csv_det)
    print("ground-truth masks:", {k: rep_gt["bop"][k] for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR")}, rep_gt["skipped"])
    assert rep_gt["rows"] == rep_det["rows"] == len(data["inst"]) == rep_det["detections"]
    for k in ("scene_id", "im_id", "obj_id"):
        assert np.array_equal(a[k], b[k])
    assert a["R"].tobytes() == b["R"].tobytes() and a["t"].tobytes() == b["t"].tobytes()
    assert (b["score"] == 1.0).all()
    assert rep_det["skipped"] == dict(rep_gt["skipped"], below_score=0, no_target=0, empty_after_clean=0, no_gt_for_prior=0)
    assert sorted(r_["detection"] for r_ in rep_det["results"]) == list(range(len(data["inst"])))
    assert all(r_["gt_index"] == data["inst"][r_["detection"]]["g"] for r_ in rep_det["results"])
    for k in ("AR_VSD", "AR_MSSD", "AR_MSPD"):
        assert rep_det["bop"][k] == rep_gt["bop"][k]


def _same_report(a, b):
    keys = ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR", "recall", "matches", "targets", "per_object")
    return all(a[k] == b[k] for k in keys)


@pytest.mark.parametrize("prior", [False, True])
def test_dirty_detections_with_cleaning_follow_the_row_rules(data, tmp_path, prior):
    """The file holds the dilated masks, the false positive on the wall (detection n), a duplicate (n + 1), one below
    --det_score_min (n + 2) and one of an object without a target (n + 3)."""
    from cppf2_amd import bop_data
    ds, n = data["ds"], data["n_dirty"]
    rep, out_csv = _eval(data, tmp_path, "dirty%d" % prior, detections=data["dirty"], det_score_min=0.2, clean_masks=True,
                         teacher_prior=prior)
    res = bop_data.read_results(out_csv)
    print("dirty detections, cleaned, teacher prior %s:" % prior, {k: rep["bop"][k] for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR")},
          rep["skipped"], rep["bop"]["counts"])
    sk = rep["skipped"]
    assert rep["detections"] == n + 4 and sk["below_score"] == 1 and sk["no_target"] == 1
    assert sk.get("no_gt_for_prior", 0) == (1 if prior else 0)
    ran = n + 2 - sk.get("no_gt_for_prior", 0)                        # the dilated ones, the duplicate, the false positive
    lost = sk["too_few_points"] + sk["too_large"] + sk["no_pick"] + sk["empty_after_clean"]
    assert rep["rows"] == len(res["score"]) == ran - lost and lost == 0
    seen = {r_["detection"]: r_ for r_ in rep["results"]}
    assert (n in seen) == (not prior) and n + 1 in seen and n + 2 not in seen and n + 3 not in seen
    assert all(seen[k]["model"] is not None for k in seen)
    assert seen[n + 1]["det_score"] == 0.3 and seen[n + 1]["score"] == 0.3 and seen[0]["score"] == 0.9
    if prior:
        assert seen[n + 1]["gt_index"] == seen[0]["gt_index"] == data["inst"][0]["g"]
    # the file, re-read and re-scored, is the printed report; no target keeps more than inst_count estimates
    again = bop_data.score(ds, res)
    assert _same_report(again, rep["bop"])
    kept, counts = bop_data.select_estimates(res, data["targets"])
    want = {(s, im, o): c for s, im, o, c in data["targets"]}
    assert all(len(v) <= want[k] for k, v in kept.items())
    assert counts["over_inst_count"] == (1 if prior else 2) and counts["not_a_target"] == 0
    assert rep["bop"]["counts"]["over_inst_count"] == counts["over_inst_count"]
    assert "mask_cleaning" in rep and np.isfinite(res["R"]).all() and np.isfinite(res["t"]).all()


def test_a_detection_of_another_image_size_is_refused(data, tmp_path):
    import eval as E
    from cppf2_amd import bop_data, masks
    i = data["inst"][0]
    small = np.zeros((240, 320), bool)
    small[100:140, 100:140] = True
    p = str(tmp_path / "small.json")
    bop_data.write_detections(p, [dict(scene_id=i["scene"], image_id=i["im"], category_id=i["obj"], bbox=masks.bbox(small), score=1.0,
                                       size=small.shape, counts=masks.rle_encode(small))])
    with pytest.raises(bop_data.BopDataError, match="differs"):
        E.main(data="bop", bop_root=data["root"], split="test", out_csv=str(tmp_path / "x.csv"), detections=p, num_pairs=20000)
