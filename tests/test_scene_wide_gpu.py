"""GPU checks of cppf_scene_explain_wide: every output equal to the restatement (tests/scene_ref.py) byte
for byte with up to 512 candidates per image, and to cppf_scene_explain where that takes the input; the winner's plane cleared
across the other planes at the tile edges of a round launch; winners and ties across planes; rounds, batches and depth contents
with candidates above index 63; two touching instances of one object end to end (its first test is CPU work)."""
import os
import sys

import numpy as np
import pytest

gpu = pytest.mark.gpu          # per test: test_two_touching_instances_by_the_restatement is CPU work and runs without a GPU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import scene_ref as SC  # noqa: E402
from test_scene_gpu import _case  # noqa: E402  (the random images of the 64-candidate tests, for any C)

F = np.float32
TAU = F(0.02)
SHAPES = [(1, 1), (1, 64), (33, 4), (37, 53), (3, 1021)]
COUNTS = [1, 64, 65, 127, 128, 129, 511, 512]
KEYS = ("chosen", "gain", "net", "static", "labels", "summary")


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _same(got, want, what=""):
    for k in KEYS:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape, want[k].shape)
        if g.tobytes() != want[k].tobytes():
            bad = np.flatnonzero(g.reshape(-1) != want[k].reshape(-1))
            raise AssertionError("%s %s differs at %d places, first %d: got %s, want %s (shape %s)" % (
                what, k, bad.size, bad[0], g.reshape(-1)[bad[:8]].tolist(), want[k].reshape(-1)[bad[:8]].tolist(), g.shape))


def _check(depth, region, off, renders, min_gain=3, viol_weight=1, M=16, tau=TAU):
    """scene.explain_wide against the restatement, byte for byte; returns the restatement's outputs."""
    from cppf2_amd import scene
    want = SC.explain(depth, region, off, renders, tau, min_gain, viol_weight, M)
    _same(scene.explain_wide(depth, region, off, renders, tau, min_gain, viol_weight, M), want, "explain_wide")
    return want


@pytest.mark.parametrize("C", COUNTS)
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@gpu
def test_equals_the_restatement(shape, C):
    _gpu()
    H, W = shape
    d, m, ren = _case(H, W, C, 11 * H + C)
    want = _check(d, m, [0, C], ren, min_gain=1 if H * W < 200 else 3)
    if shape == (37, 53) and C >= 65:
        planes = {int(c) // 64 for c in want["chosen"][0] if c >= 0}
        assert want["summary"][0, 2] >= 4 and (C < 127 or len(planes) >= 2), "the case no longer chooses from several planes"
        # 0, NaN, +-inf and -0.0 in candidates above index 63 and in the observed depth, region bytes 7 and 255
        hi = ren[64:].reshape(-1)
        assert np.isnan(hi).any() and np.isposinf(hi).any() and np.isneginf(hi).any() and (hi == 0).any() and np.signbit(hi[hi == 0]).any()
        assert np.isnan(d).any() and np.isinf(d).any() and np.signbit(d[d == 0]).any() and {7, 255} <= set(np.unique(m).tolist())


@gpu
def test_equals_the_restatement_at_480x640():
    _gpu()
    d, m, ren = _case(480, 640, 130, 3)
    want = _check(d, m, [0, 130], ren, min_gain=200)
    assert want["summary"][0, 2] >= 3


@pytest.mark.parametrize("C", [1, 63, 64])
@gpu
def test_equals_scene_explain_up_to_64_candidates(C):
    """The same inputs through cppf_scene_explain and cppf_scene_explain_wide: every output the same byte for byte, one image and
    a batch with an image without a candidate."""
    _gpu()
    from cppf2_amd import scene
    for H, W in SHAPES:
        d, m, ren = _case(H, W, C, 7 * H + C)
        a = scene.explain(d, m, [0, C], ren, TAU, 1, 1, 16)
        _same(scene.explain_wide(d, m, [0, C], ren, TAU, 1, 1, 16), {k: a[k].cpu().numpy() for k in KEYS}, "%dx%d" % (H, W))
    cases = [_case(37, 53, C, 50), _case(37, 53, 1, 51), _case(37, 53, 5, 52)]
    d, m = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    ren, off = np.concatenate([cases[0][2], cases[2][2]]), [0, C, C, C + 5]
    a = scene.explain(d, m, off, ren, TAU, 3, 1, 16)
    _same(scene.explain_wide(d, m, off, ren, TAU, 3, 1, 16), {k: a[k].cpu().numpy() for k in KEYS}, "batch")


@pytest.mark.parametrize("a,b", [(5, 69), (69, 5)], ids=["A0_B1", "A1_B0"])
@pytest.mark.parametrize("at", [0, 974, 1000, 1786])
@gpu
def test_the_winner_clears_the_other_planes(at, a, b):
    """order_case on 37 x 53 with A and B in different planes, at positions that straddle the 1024-pixel tile of a round launch
    and end on the image's last pixel: closing A's round clears B's 50 shared pixels in B's plane, so B's gain is its remainder of
    10 pixels, and the cleared pixels carry A's label."""
    _gpu()
    d_o, m, abc = SC.order_case(37, 53, at)
    ren = np.zeros((131, 37, 53), F)
    ren[a], ren[b], ren[130] = abc[0], abc[1], abc[2]
    want = _check(d_o, m, [0, 131], ren, min_gain=11)
    assert want["chosen"][0, :3].tolist() == [a, 130, -1] and want["gain"][0, :2].tolist() == [100, 55]
    want = _check(d_o, m, [0, 131], ren, min_gain=10)
    assert want["chosen"][0, :4].tolist() == [a, 130, b, -1] and want["gain"][0, :3].tolist() == [100, 55, 10]
    lab = want["labels"][0].reshape(-1)
    assert (lab[at:at + 100] == 0).all() and (lab[at + 100:at + 110] == 2).all() and (lab[at + 120:at + 175] == 1).all()
    assert (lab != 255).sum() == 165 and want["summary"][0].tolist() == [37 * 53, 165, 3]


@pytest.mark.parametrize("w", [64, 127, 511])
@gpu
def test_winner_index_and_ties_across_planes(w):
    """Candidate w wins the first round by one pixel over a twin in plane 0; two equal candidates in different planes: the lower
    index is chosen and the higher never."""
    _gpu()
    d_o, m, abc = SC.order_case(37, 53, 1000)
    ren = np.zeros((512, 37, 53), F)
    ren[w], ren[3], ren[300] = abc[0], abc[1], abc[2]
    ren[2] = abc[0]
    ren[2].reshape(-1)[1000] = 0                             # one pixel less than candidate w
    want = _check(d_o, m, [0, 512], ren, min_gain=10)
    assert want["chosen"][0, :4].tolist() == [w, 300, 3, -1] and want["gain"][0, :3].tolist() == [100, 55, 10]
    ren[2] = 0
    lo = {64: 1, 127: 64, 511: 448}[w]                       # the twin below w: plane 0, w's own plane, w's own plane
    ren[lo] = abc[0]
    want = _check(d_o, m, [0, 512], ren, min_gain=10)
    assert want["chosen"][0, :4].tolist() == [lo, 300, 3, -1] and w not in want["chosen"][0].tolist()
    ren[lo] = 0
    ren[min(w + 193, 511) if w < 511 else 70] = abc[0]       # the twin in another plane
    pair = sorted([w, min(w + 193, 511) if w < 511 else 70])
    want = _check(d_o, m, [0, 512], ren, min_gain=10)
    assert want["chosen"][0, :4].tolist() == [pair[0], 300, 3, -1] and pair[1] not in want["chosen"][0].tolist()


@gpu
def test_net_equal_to_min_gain_and_one_below_in_plane_1():
    _gpu()
    d, m, ren6 = _case(37, 53, 6, 31)
    ren = np.zeros((128, 37, 53), F)
    ren[[70, 3, 99, 64, 127, 20]] = ren6                     # the six candidates of the 64-candidate test, four of them in plane 1
    free = SC.explain_image(d, m, ren, TAU, 1, 1, 16)
    assert free["summary"][2] >= 3
    second = int(free["chosen"][1])
    n1 = int(free["net"][1])
    if second < 64:                                          # keep the property the test is about: the second winner in plane 1
        ren[[second, second + 64]] = ren[[second + 64, second]]
        free = SC.explain_image(d, m, ren, TAU, 1, 1, 16)
        second, n1 = int(free["chosen"][1]), int(free["net"][1])
    assert second >= 64
    at = _check(d, m, [0, 128], ren, min_gain=n1)            # net == min_gain: eligible
    assert at["chosen"][0, 1] == second and at["net"][0, 1] == n1
    below = _check(d, m, [0, 128], ren, min_gain=n1 + 1)     # net == min_gain - 1: not eligible
    assert below["chosen"][0, 1] == -1 and below["summary"][0, 2] <= 1


@gpu
def test_a_negative_net_in_plane_7():
    _gpu()
    d_o, m, abc = SC.order_case(37, 53, 1000)
    ren = np.zeros((512, 37, 53), F)
    ren[449], ren[65], ren[200] = abc[0], abc[1], abc[2]
    ren[500] = abc[1]
    ren[500].reshape(-1)[200:300] = 0.5                      # 60 fit pixels, 100 violations: net -40
    want = _check(d_o, m, [0, 512], ren, min_gain=10, viol_weight=1)
    assert want["chosen"][0, :4].tolist() == [449, 200, 65, -1] and want["static"][500].tolist() == [160, 60, 100]
    assert 500 not in want["chosen"][0].tolist() and (want["net"] >= 0).all()
    alone = _check(d_o, m, [0, 512], np.where(np.arange(512)[:, None, None] == 500, ren, 0).astype(F), min_gain=1, viol_weight=1)
    assert alone["chosen"][0].tolist() == [-1] * 16 and alone["summary"][0].tolist() == [37 * 53, 0, 0]


@pytest.mark.parametrize("M", [1, 16, 64])
@gpu
def test_round_counts_over_several_planes(M):
    """200 candidates with min_gain 1 and no violation weight: more eligible candidates than 1 and than 16 rounds, in several planes."""
    _gpu()
    d, m, ren = _case(37, 53, 200, 5)
    want = _check(d, m, [0, 200], ren, min_gain=1, viol_weight=0, M=M)
    full = int(SC.explain_image(d, m, ren, TAU, 1, 0, 64)["summary"][2])
    assert full > 16 and want["summary"][0, 2] == min(M, full)
    assert len({int(c) // 64 for c in want["chosen"][0] if c >= 0}) >= min(M, 3)


@gpu
def test_batch_of_0_70_3_and_512_candidates_alone_and_reversed():
    _gpu()
    from cppf2_amd import scene
    n = [0, 70, 3, 512]
    cases = [_case(37, 53, max(c, 1), 60 + i) for i, c in enumerate(n)]
    d, m = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    ren = np.concatenate([c[2][:k] for c, k in zip(cases, n)])
    off = np.concatenate([[0], np.cumsum(n)])
    want = _check(d, m, off, ren)
    assert want["chosen"][0].tolist() == [-1] * 16 and want["summary"][0, 0] > 0 and want["summary"][0, 1:].tolist() == [0, 0]
    assert (want["summary"][1:, 2] > 0).all() and (want["chosen"][3] >= 64).any() and (want["chosen"][1] >= 64).any()
    rren = np.concatenate([c[2][:k] for c, k in zip(cases[::-1], n[::-1])])
    roff = np.concatenate([[0], np.cumsum(n[::-1])])
    rev = scene.explain_wide(d[::-1].copy(), m[::-1].copy(), roff, rren, TAU, 3, 1, 16)
    for k in ("chosen", "gain", "net", "labels", "summary"):
        assert rev[k].cpu().numpy()[::-1].tobytes() == want[k].tobytes(), k
    rstat = rev["static"].cpu().numpy()
    for i in range(4):
        lo, hi = int(off[i]), int(off[i + 1])
        assert np.array_equal(rstat[roff[3 - i]:roff[4 - i]], want["static"][lo:hi])
        one = _check(d[i], m[i], [0, hi - lo], ren[lo:hi])
        for k in ("chosen", "gain", "net", "labels", "summary"):
            assert one[k][0].tobytes() == want[k][i].tobytes(), (i, k)
        assert np.array_equal(one["static"], want["static"][lo:hi])


@gpu
def test_more_than_128_images_in_one_call():
    """The offsets go by value 128 images at a time: 131 small images, some without a candidate, one on either side of the chunk
    edge with more than 64."""
    _gpu()
    rng = np.random.default_rng(9)
    n = rng.integers(0, 4, 131)
    n[5], n[127], n[129] = 70, 130, 65
    off = np.concatenate([[0], np.cumsum(n)])
    cases = [_case(5, 13, max(int(c), 1), 100 + i, bad=False) for i, c in enumerate(n)]
    ren = np.concatenate([c[2][:k] for c, k in zip(cases, n)])
    want = _check(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), off, ren, min_gain=1)
    assert (want["summary"][:, 2] > 0).sum() > 40 and all(want["summary"][i, 2] > 0 for i in (5, 127, 129))


# ---- end to end: two touching instances of one object on a generated table ------------------------------------------------------------
import bop_data_ref as DR  # noqa: E402
import render_ref as RR  # noqa: E402
import segment_ref as SR  # noqa: E402

PHI = np.deg2rad(55.0)       # the scene of tests/test_scene_gpu.py: a table tilted towards the camera, a wall behind
TABLE_N = np.array([0.0, -np.cos(PHI), -np.sin(PHI)])
TABLE_C = np.array([0.0, 0.10, 0.85])
SCENE_SCALE = 10000.0        # depth units per metre of the scene's PNG
SECOND_U = 0.0               # the second instance's place along the table: 0.10 in tests/test_scene_gpu.py, well apart; from 0.02
                             # downward the two stand against each other and the depth segments join (CPU, segment_ref)
DECOY_STEPS = (-3, -2, -1, 1, 2, 3)                          # times 3 cm, along and across the table: 36 decoys per instance


def _rotx(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def _rotz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


@pytest.fixture(scope="module")
def touching(tmp_path_factory):
    """The scene of tests/test_scene_gpu.py without the cylinder and with the second instance moved along the table until it
    stands against the first, every mesh rendered alone by the rasteriser's NumPy mirror; the depth is what the 16-bit PNG
    holds.  Candidates: 72 decoys first (each true pose shifted by a multiple of 3 cm, 3 to 9 cm, along and across the table),
    then per instance the true pose, the object upside down, the truth shifted by 3 cm, and a near-duplicate (1 degree, 1 mm):
    the eight real candidates are 72 .. 79, in plane 1.  Everything here is CPU work."""
    from PIL import Image
    from cppf2_amd import render, scene
    from cppf2_amd.pipeline import RESULT_DTYPE
    root = tmp_path_factory.mktemp("touching")
    ex, ds = np.array([1.0, 0, 0]), np.array([0.0, -np.sin(PHI), np.cos(PHI)])
    Rt = _rotx(np.pi / 2 + PHI)
    fixture = render.load_mesh(DR.FIXTURE, 0.001)
    b = fixture.bounds
    fv = fixture.verts - (b[0] + b[1]) / 2                      # the record convention: centred on the bounding box
    table, wall = render.Mesh(*DR.box((0.6, 0.5, 0.01))), render.Mesh(*DR.box((1.5, 1.2, 0.01)))

    def centred(mesh):
        bb = mesh.bounds
        return mesh.verts - (bb[0] + bb[1]) / 2

    def stand(verts, R, u, v):
        low = (verts @ R.T @ TABLE_N).min()                     # the lowest vertex touches the table top
        return TABLE_C + u * ex + v * ds - low * TABLE_N
    Ra, Rb = Rt @ _rotz(0.7), Rt @ _rotz(2.3)
    truth = [(Ra, stand(fv, Ra, -0.20, 0.0)), (Rb, stand(fv, Rb, SECOND_U, -0.03))]
    parts = [(fv, fixture.faces) + truth[0], (fv, fixture.faces) + truth[1],
             (centred(table), table.faces, Rt, TABLE_C - 0.01 * TABLE_N), (centred(wall), wall.faces, np.eye(3), np.array([0.0, 0.0, 1.6]))]
    ren = np.stack([RR.render(v, f, RR.look_pose(R, t), DR.K, DR.H, DR.W)[0] for v, f, R, t in parts])
    owner = np.where(ren > 0, ren, np.inf).argmin(0)
    depth = np.where(ren > 0, ren, np.inf).min(0)
    assert np.isfinite(depth).all(), "the wall fills the image"
    dpath = str(root / "depth.png")
    Image.fromarray(np.round(depth * SCENE_SCALE).astype(np.uint16)).save(dpath)
    d = (np.array(Image.open(dpath)).astype(np.float64) / SCENE_SCALE).astype(F)
    cands = [(R, t + 0.03 * (i * ex + j * ds)) for R, t in truth for i in DECOY_STEPS for j in DECOY_STEPS]
    assert len(cands) == 72
    for R, t in truth:
        cands += [(R, t), (R @ _rotx(np.pi), t), (R, t + 0.03 * ex), (R @ _rotz(np.deg2rad(1.0)), t + 0.001 * ds)]
    cren = np.stack([RR.render(fv, fixture.faces, RR.look_pose(R, t), DR.K, DR.H, DR.W)[0] for R, t in cands])
    recs = np.zeros(len(cands), dtype=RESULT_DTYPE)
    for r_, (R, t) in zip(recs, cands):
        r_["R"], r_["t"] = np.asarray(R, np.float64).reshape(r_["R"].shape), t
    ref = SR.propose(d, DR.K, 0)
    region = (ref["masks"] > 0).any(0)
    want = SC.explain(d, region, [0, len(cands)], cren, scene.TAU, scene.MIN_GAIN, scene.VIOL_WEIGHT, scene.MAX_ROUNDS)
    return dict(d=d, owner=owner, depth_png=dpath, root=root, ref=ref, region=region, cren=cren, recs=recs, want=want, truth=truth,
                fixture=fixture)


def test_two_touching_instances_by_the_restatement(touching):
    """The conditions of the scene, then, by the CPU renders and the restatement alone: exactly two instances, one per object
    instance, each the truth or its near-duplicate -- though the two share one depth segment."""
    want, owner, ref = touching["want"], touching["owner"], touching["ref"]
    vis = [owner == o for o in range(4)]
    masks = ref["masks"] > 0
    print("owners", [int(v.sum()) for v in vis], "segments", [[int((m & v).sum()) for v in vis] for m in masks],
          "static", want["static"][72:].tolist(), "chosen", want["chosen"][0].tolist(), "gain", want["gain"][0].tolist(),
          "net", want["net"][0].tolist(), "summary", want["summary"][0].tolist())
    assert vis[0].sum() > 3000 and vis[1].sum() > 3000
    assert len(masks) == 1 and (masks[0] & vis[0]).sum() > 3000 and (masks[0] & vis[1]).sum() > 3000, "one segment holds both"
    n = int(want["summary"][0, 2])
    chosen = want["chosen"][0, :n].tolist()
    assert n == 2 and all(c >= 72 for c in chosen), chosen
    assert sorted((c - 72) // 4 for c in chosen) == [0, 1] and all((c - 72) % 4 in (0, 3) for c in chosen)
    for k, c in enumerate(chosen):
        o = (c - 72) // 4
        lab = want["labels"][0] == k
        assert 2 * int((lab & vis[o]).sum()) > int(lab.sum()) and int((lab & vis[o]).sum()) > 3000


@gpu
def test_the_gpu_equals_the_restatement_on_the_touching_scene(touching):
    """cppf_scene_explain_wide on the CPU renders equals the restatement; explain_candidates(wide=True), which renders the 80
    records on the GPU, chooses the same candidates; without wide the 80 records are refused."""
    _gpu()
    from cppf2_amd import scene
    s = touching
    want = _check(s["d"], s["region"], [0, 80], s["cren"], scene.MIN_GAIN, scene.VIOL_WEIGHT, scene.MAX_ROUNDS, F(scene.TAU))
    assert want["chosen"].tobytes() == s["want"]["chosen"].tobytes()
    ex = scene.explain_candidates(s["fixture"], s["d"], s["region"], DR.K, s["recs"], wide=True)
    n = int(want["summary"][0, 2])
    print("gpu renders: chosen", ex["chosen"].tolist(), "gain", ex["gain"].tolist(), "cpu renders: gain", want["gain"][0, :n].tolist())
    assert ex["chosen"].tolist() == want["chosen"][0, :n].tolist()
    assert ex["records"].tobytes() == s["recs"][ex["chosen"]].tobytes() and ex["labels"].shape == s["d"].shape
    with pytest.raises(ValueError, match="at most 64"):
        scene.explain_candidates(s["fixture"], s["d"], s["region"], DR.K, s["recs"])


def _majority(inst, labels_of, vis):
    """Per reported instance the true instance (0 or 1) in whose visible mask more than half of its labelled pixels lie, else None."""
    out = []
    for k in range(len(inst)):
        lab = labels_of(k)
        hit = [o for o in (0, 1) if 2 * int((lab & vis[o]).sum()) > int(lab.sum())]
        out.append(hit[0] if hit else None)
    return out


@gpu
def test_eval_explains_the_touching_scene(touching, tmp_path, monkeypatch):
    """eval.py --propose_masks --explain_scene --pair_table --hypotheses=8 --centre_peaks=3 --icp_iters=10 on the touching pair:
    without --explain_hypotheses at most one instance on the joint proposal; with it two instances with the same proposal and
    different hypotheses, each with more than half of its labelled pixels inside one true instance's visible mask, the two on
    different true instances.  The rest of the report is what the run without the flag prints."""
    import json
    _gpu()
    from cppf2_amd import pair_table, scene
    monkeypatch.chdir(ROOT)
    import eval as ev
    s = touching
    table = str(tmp_path / "obj_000015.npz")
    pair_table.build(s["fixture"], views=32, seed=0, name="obj_000015.ply").save(table)
    kw = dict(data="depth", depth=s["depth_png"], depth_scale=SCENE_SCALE, intrinsics=DR.K.tolist(), num_pairs=20000, num_rots=36,
              opt=False, debug=True, hypotheses=8, centre_peaks=3, icp_iters=10, seed=0, propose_masks=True, explain_scene=True,
              mesh=DR.FIXTURE, mesh_scale=0.001, pair_table=table)
    narrow = ev.main(**kw)
    rep = ev.main(explain_hypotheses=True, **kw)
    sc = rep["scene"]
    print("narrow", [(i["proposal"], i["score"], i["gain"]) for i in narrow["scene"]["instances"]], "wide",
          [(i["proposal"], i["hypothesis"], i["support"], i["score"], i["gain"], i["net"]) for i in sc["instances"]],
          "rejected", [(r["proposal"], r["hypothesis"], round(r["support"], 3), r["reason"]) for r in sc["rejected"]],
          sc["candidates"], sc["dropped"], sc["explained_pixels"], sc["region_pixels"])
    assert json.dumps({k: v for k, v in rep.items() if k != "scene"}) == json.dumps({k: v for k, v in narrow.items() if k != "scene"})
    assert len(rep["proposals"]) == 1 and len(narrow["scene"]["instances"]) <= 1
    assert sc["parameters"] == dict(narrow["scene"]["parameters"], min_support=0.5, hypotheses=True)
    assert {r["reason"] for r in sc["rejected"]} <= {"below_min_support", "no_gain"} and sc["dropped"] == 0
    assert sc["candidates"] + sum(r["reason"] == "below_min_support" for r in sc["rejected"]) <= 8
    for e in sc["instances"] + sc["rejected"]:
        assert 0 <= e["hypothesis"] < 8 and 0.0 <= e["support"] <= 1.0 and e["proposal"] == 0
    assert all(i["support"] >= 0.5 and i["gain"] >= i["net"] >= scene.MIN_GAIN for i in sc["instances"])
    # the labels of the reported instances: the same candidates explained again by the library
    from cppf2_amd.pipeline import RESULT_DTYPE
    recs = np.zeros(len(sc["instances"]), dtype=RESULT_DTYPE)
    for r_, i in zip(recs, sc["instances"]):
        r_["R"], r_["t"] = np.asarray(i["R"], np.float64).reshape(r_["R"].shape), i["t"]
    ex = scene.explain_candidates(s["fixture"], s["d"], s["region"], DR.K, recs, wide=True)
    assert ex["chosen"].tolist() == list(range(len(recs))) and ex["gain"].tolist() == [i["gain"] for i in sc["instances"]]
    vis = [s["owner"] == o for o in range(2)]
    on = _majority(sc["instances"], lambda k: ex["labels"] == k, vis)
    print("instances lie on", on)
    assert len(sc["instances"]) == 2 and sorted(on) == [0, 1]
    assert sc["instances"][0]["hypothesis"] != sc["instances"][1]["hypothesis"]
