"""GPU checks of cppf_scene_explain: every output equal to the restatement (tests/scene_ref.py) byte for
byte on every image size, candidate count, round count and depth content; an image alone, inside a batch and in reversed order;
the static counts against cppf_depth_fit_counts; a rendered two-instance scene end to end (its first test is CPU work)."""
import os
import sys

import numpy as np
import pytest

gpu = pytest.mark.gpu          # per test: test_two_instances_by_the_restatement is CPU work and runs without a GPU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import scene_ref as SC  # noqa: E402

F = np.float32
TAU = F(0.02)
SHAPES = [(1, 1), (1, 64), (33, 4), (37, 53), (3, 1021), (480, 640)]
KEYS = ("chosen", "gain", "net", "static", "labels", "summary")


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _case(H, W, C, seed, bad=True):
    """Observed depth about a metre with a region of bytes 0, 1, 7 and 255; C candidates, each a run of pixels in row-major
    order plus a sprinkle, whose depth is the observed one shifted by 0, +-tau / 2, tau as the float32 sum rounds (within 6e-8 of
    the boundary, on either side; test_differences_of_exactly_tau has the exact ones) and one ulp beyond it, 10 cm in front (a violation) or 10 cm behind; (bad) 0, NaN, +-inf, a negative value and -0.0 in both."""
    rng = np.random.default_rng(seed)
    HW = H * W
    d_o = (1.0 + 0.1 * rng.random(HW)).astype(F)
    m = np.array([0, 1, 7, 255], np.uint8)[rng.choice(4, HW, p=[0.25, 0.5, 0.125, 0.125])]
    hi = d_o + TAU
    shifts = np.stack([d_o, d_o + TAU / 2, d_o - TAU / 2, hi, np.nextafter(hi, F(9)), d_o - TAU, np.nextafter(d_o - TAU, F(-9)),
                       d_o - F(0.1), d_o + F(0.1)]).astype(F)
    ren = np.zeros((C, HW), F)
    for c in range(C):
        n = int(rng.integers(1, max(2, HW // 2 + 1)))
        a = int(rng.integers(0, HW - n + 1))
        on = np.zeros(HW, bool)
        on[a:a + n] = True
        on |= rng.random(HW) < 0.02
        p = rng.dirichlet(np.ones(9) * 0.7)
        kind = rng.choice(9, HW, p=p)
        ren[c] = np.where(on, shifts[kind, np.arange(HW)], 0)
    if bad and HW >= 16:
        vals = np.array([0.0, np.nan, np.inf, -np.inf, -0.7, -0.0], F)
        p = rng.choice(HW, size=max(6, HW // 40), replace=False)
        d_o[p] = vals[np.arange(p.size) % 6]
        for c in range(C):
            p = rng.choice(HW, size=max(6, HW // 40), replace=False)
            ren[c, p] = vals[(np.arange(p.size) + c) % 6]
    return d_o.reshape(H, W), m.reshape(H, W), ren.reshape(C, H, W)


def _check(depth, region, off, renders, min_gain=3, viol_weight=1, M=16, tau=TAU):
    """scene.explain against the restatement, byte for byte; returns the restatement's outputs."""
    from cppf2_amd import scene
    want = SC.explain(depth, region, off, renders, tau, min_gain, viol_weight, M)
    got = scene.explain(depth, region, off, renders, tau, min_gain, viol_weight, M)
    for k in KEYS:
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (k, g.dtype, g.shape, want[k].shape)
        if g.tobytes() != want[k].tobytes():
            bad = np.flatnonzero(g.reshape(-1) != want[k].reshape(-1))
            raise AssertionError("%s differs at %d places, first %d: got %s, want %s (shape %s)" % (
                k, bad.size, bad[0], g.reshape(-1)[bad[:8]].tolist(), want[k].reshape(-1)[bad[:8]].tolist(), g.shape))
    return want


@pytest.mark.parametrize("C", [1, 2, 63, 64])
@pytest.mark.parametrize("shape", SHAPES[:5], ids=["%dx%d" % s for s in SHAPES[:5]])
@gpu
def test_equals_the_restatement(shape, C):
    _gpu()
    H, W = shape
    d, m, ren = _case(H, W, C, 11 * H + C)
    want = _check(d, m, [0, C], ren, min_gain=1 if H * W < 200 else 3)
    if shape == (37, 53) and C >= 63:
        assert want["summary"][0, 2] >= 4 and (want["static"][:, 2] > 0).any(), "the case no longer takes several rounds"


@pytest.mark.parametrize("M", [1, 16, 64])
@gpu
def test_round_counts_at_37x53(M):
    """64 candidates with min_gain 1 and no violation weight: more eligible candidates than 1 and than 16 rounds."""
    _gpu()
    d, m, ren = _case(37, 53, 64, 5)
    want = _check(d, m, [0, 64], ren, min_gain=1, viol_weight=0, M=M)
    full = SC.explain_image(d, m, ren, TAU, 1, 0, 64)["summary"][2]
    assert full > 16 and want["summary"][0, 2] == min(M, full)


@pytest.fixture(scope="module")
def vga():
    return _case(480, 640, 64, 3)


@gpu
def test_equals_the_restatement_at_480x640(vga):
    _gpu()
    d, m, ren = vga
    want = _check(d, m, [0, 64], ren, min_gain=200)
    assert want["summary"][0, 2] >= 3
    _check(d, m, [0, 8], ren[:8], min_gain=200)


@gpu
def test_batch_alone_and_reversed():
    """Three images, the middle one without a candidate: each image's outputs are the same alone, in the batch and reversed."""
    _gpu()
    from cppf2_amd import scene
    cases = [_case(37, 53, 5, 21), _case(37, 53, 1, 22), _case(37, 53, 64, 23)]
    d = np.stack([c[0] for c in cases])
    m = np.stack([c[1] for c in cases])
    ren = np.concatenate([cases[0][2], cases[2][2]])
    want = _check(d, m, [0, 5, 5, 69], ren)
    assert want["chosen"][1].tolist() == [-1] * 16 and want["summary"][1, 0] > 0 and want["summary"][1, 1:].tolist() == [0, 0]
    assert (want["labels"][1] == 255).all() and want["summary"][0, 2] > 0 and want["summary"][2, 2] > 0
    rev = scene.explain(d[::-1].copy(), m[::-1].copy(), [0, 64, 64, 69], np.concatenate([cases[2][2], cases[0][2]]), TAU, 3, 1, 16)
    for k in ("chosen", "gain", "net", "labels", "summary"):
        assert rev[k].cpu().numpy()[::-1].tobytes() == want[k].tobytes(), k
    assert np.array_equal(rev["static"].cpu().numpy(), np.concatenate([want["static"][5:], want["static"][:5]]))
    for i, (lo, hi) in enumerate(((0, 5), (5, 5), (5, 69))):
        one = _check(d[i], m[i], [0, hi - lo], ren[lo:hi])
        for k in ("chosen", "gain", "net", "labels", "summary"):
            assert one[k][0].tobytes() == want[k][i].tobytes(), (i, k)
        assert np.array_equal(one["static"], want["static"][lo:hi])


@gpu
def test_more_than_128_images_in_one_call():
    """The offsets go by value 128 images at a time: 131 small images, some without a candidate."""
    _gpu()
    rng = np.random.default_rng(9)
    n = rng.integers(0, 4, 131)
    off = np.concatenate([[0], np.cumsum(n)])
    cases = [_case(5, 13, max(int(c), 1), 100 + i, bad=False) for i, c in enumerate(n)]
    ren = np.concatenate([c[2][:k] for c, k in zip(cases, n)])
    want = _check(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), off, ren, min_gain=1)
    assert (want["summary"][:, 2] > 0).sum() > 40


@gpu
def test_net_equal_to_min_gain_and_one_below():
    _gpu()
    d, m, ren = _case(37, 53, 6, 31)
    free = SC.explain_image(d, m, ren, TAU, 1, 1, 16)
    assert free["summary"][2] >= 3
    n1 = int(free["net"][1])
    at = _check(d, m, [0, 6], ren, min_gain=n1)              # net == min_gain: eligible
    assert at["chosen"][0, 1] == free["chosen"][1] and at["net"][0, 1] == n1
    below = _check(d, m, [0, 6], ren, min_gain=n1 + 1)       # net == min_gain - 1: not eligible
    assert below["chosen"][0, 1] == -1 and below["summary"][0, 2] <= 1


@gpu
def test_differences_of_exactly_tau():
    """|d_o - d_c| == (double)tau exactly and one float32 step to either side, inside and outside the region: fit and violation
    pixel by pixel as tests/test_scene.py states them, through the labels (fit) and against cppf_depth_fit_counts; alone, and
    as candidate 63 of 64 at the end of a 37 x 53 image."""
    _gpu()
    from cppf2_amd import verify
    from test_scene import EDGE_FIT, EDGE_VIOL
    d_o, m, d_c = SC.tau_edge_case(TAU)
    want = _check(d_o, m, [0, 1], d_c[0], min_gain=1, viol_weight=0, M=4)
    assert want["static"].tolist() == [[10, sum(EDGE_FIT), sum(EDGE_VIOL)]] == [[10, 5, 3]]
    assert want["labels"][0, 0].tolist() == [0 if f_ else 255 for f_ in EDGE_FIT] and want["summary"][0].tolist() == [8, 5, 1]
    # each pixel alone, so that a wrong comparison cannot hide in a sum: (drawn, fit, violations) per pixel
    one = np.zeros((10, 1, 10), F)
    one[np.arange(10), 0, np.arange(10)] = d_c[0, 0]
    per = _check(d_o, m, [0, 10], one, min_gain=1, viol_weight=0, M=16)
    assert per["static"].tolist() == [[1, int(f_), int(v_)] for f_, v_ in zip(EDGE_FIT, EDGE_VIOL)]
    fc = verify.fit_counts(d_o, m, [0, 10], one, (float(TAU),)).cpu().numpy()
    assert fc[:, [0, 4, 2]].tolist() == per["static"].tolist()
    big_o, big_m, ren = _case(37, 53, 64, 77, bad=False)
    big_o.reshape(-1)[-10:], big_m.reshape(-1)[-10:] = d_o[0], m[0]
    ren.reshape(64, -1)[:, -10:] = 0
    ren[63] = 0
    ren[63].reshape(-1)[-10:] = d_c[0, 0]
    big = _check(big_o, big_m, [0, 64], ren, min_gain=1, viol_weight=0, M=64)
    assert big["static"][63].tolist() == [10, 5, 3] and 63 in big["chosen"][0].tolist()
    k = big["chosen"][0].tolist().index(63)
    assert big["labels"][0].reshape(-1)[-10:].tolist() == [k if f_ else 255 for f_ in EDGE_FIT]


@gpu
def test_negative_net_top_bit_and_empty_region():
    _gpu()
    # a candidate with net < 0 between two good ones; candidate 63 wins the first round
    d_o, m, abc = SC.order_case(37, 53, 1000)
    ren = np.zeros((64, 37, 53), F)
    ren[63], ren[5], ren[20] = abc[0], abc[1], abc[2]
    ren[7] = abc[1]
    ren[7].reshape(-1)[200:300] = 0.5                        # 60 fit pixels, 100 violations
    ren[62] = abc[0]
    ren[62].reshape(-1)[1000] = 0                            # one pixel less than candidate 63
    want = _check(d_o, m, [0, 64], ren, min_gain=10, viol_weight=1)
    assert want["chosen"][0, :4].tolist() == [63, 20, 5, -1] and want["gain"][0, :3].tolist() == [100, 55, 10]
    assert want["static"][7].tolist() == [160, 60, 100] and 7 not in want["chosen"][0].tolist()
    # a region with no valid pixel: nothing to explain, though the renders are drawn
    none = _check(np.where(m > 0, F(0), d_o), m, [0, 64], ren, min_gain=1)
    assert none["summary"][0].tolist() == [0, 0, 0] and none["static"][63].tolist() == [100, 0, 0]
    none = _check(d_o, np.zeros_like(m), [0, 64], ren, min_gain=1)
    assert none["summary"][0].tolist() == [0, 0, 0] and none["static"][7].tolist() == [160, 0, 100]


@pytest.mark.parametrize("at", [0, 974, 1000, 1786])
@gpu
def test_order_matters_across_tiles(at):
    """The hand-drawn case of tests/test_scene.py on 37 x 53 at positions that straddle the 1024-pixel tile of a round launch and
    end on the image's last pixel: A, then C, then B's remainder of 10 pixels, refused at min_gain 11."""
    _gpu()
    d_o, m, ren = SC.order_case(37, 53, at)
    want = _check(d_o, m, [0, 3], ren, min_gain=11)
    assert want["chosen"][0, :3].tolist() == [0, 2, -1] and want["gain"][0, :2].tolist() == [100, 55]
    want = _check(d_o, m, [0, 3], ren, min_gain=10)
    assert want["chosen"][0, :4].tolist() == [0, 2, 1, -1] and want["gain"][0, :3].tolist() == [100, 55, 10]


@gpu
def test_static_counts_equal_depth_fit_counts(vga):
    """The columns drawn, fit and violations of cppf_depth_fit_counts on the same inputs: ties the new kernel to the existing one."""
    _gpu()
    from cppf2_amd import scene, verify
    for d, m, ren in (vga[:2] + (vga[2][:9],), _case(37, 53, 64, 41), _case(3, 1021, 63, 42)):
        C = ren.shape[0]
        got = scene.explain(d, m, [0, C], ren, TAU, 1, 1, 1)
        fc = verify.fit_counts(d, m, [0, C], ren, (float(TAU),)).cpu().numpy()
        assert np.array_equal(got["static"].cpu().numpy(), fc[:, [0, 4, 2]])
        assert int(got["summary"][0, 0]) == int(fc[0, 1])


# ---- end to end: two instances of one object and a cylinder on a generated table ---------------------------------------------------
import bop_data_ref as DR  # noqa: E402
import render_ref as RR  # noqa: E402
import segment_ref as SR  # noqa: E402

PHI = np.deg2rad(55.0)       # the scene of tests/test_segment_gpu.py: a table tilted towards the camera, a wall behind
TABLE_N = np.array([0.0, -np.cos(PHI), -np.sin(PHI)])
TABLE_C = np.array([0.0, 0.10, 0.85])
SCENE_SCALE = 10000.0        # depth units per metre of the scene's PNG
# By the restatement on the CPU renders (scene2 below), the share of each instance's visible pixels that the label image covers:
# 0.9904 and 0.9972.  What is missing is the contact line, which the proposals leave to the table.
SHARE = (0.990, 0.997)


def _rotx(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def _rotz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


@pytest.fixture(scope="module")
def scene2(tmp_path_factory):
    """Two instances of the fixture object well apart and the 15 mm cylinder standing on the table, every mesh rendered alone
    by the rasteriser's NumPy mirror (tests/render_ref.py); the depth is what the 16-bit PNG holds.  Candidates 0-3 belong to
    instance 0 and 4-7 to instance 1: the true pose, the object upside down (180 degrees about an axis in the table), the truth
    shifted by 3 cm along the table, and a near-duplicate of the truth (1 degree, 1 mm).  Everything here is CPU work."""
    from PIL import Image
    from cppf2_amd import render
    from cppf2_amd.pipeline import RESULT_DTYPE
    root = tmp_path_factory.mktemp("scene2")
    ex, ds = np.array([1.0, 0, 0]), np.array([0.0, -np.sin(PHI), np.cos(PHI)])
    Rt = _rotx(np.pi / 2 + PHI)
    fixture = render.load_mesh(DR.FIXTURE, 0.001)
    b = fixture.bounds
    fv = fixture.verts - (b[0] + b[1]) / 2                      # the record convention: centred on the bounding box
    cv, cf = DR.cylinder(r=15.0)
    cyl = render.Mesh(cv * 0.001, cf)
    table, wall = render.Mesh(*DR.box((0.6, 0.5, 0.01))), render.Mesh(*DR.box((1.5, 1.2, 0.01)))

    def centred(mesh):
        bb = mesh.bounds
        return mesh.verts - (bb[0] + bb[1]) / 2

    def stand(verts, R, u, v):
        low = (verts @ R.T @ TABLE_N).min()                     # the lowest vertex touches the table top
        return TABLE_C + u * ex + v * ds - low * TABLE_N
    Ra, Rb = Rt @ _rotz(0.7), Rt @ _rotz(2.3)
    truth = [(Ra, stand(fv, Ra, -0.20, 0.0)), (Rb, stand(fv, Rb, 0.10, -0.03))]
    parts = [(fv, fixture.faces) + truth[0], (fv, fixture.faces) + truth[1],
             (centred(cyl), cyl.faces, Rt, stand(centred(cyl), Rt, 0.31, -0.06)),
             (centred(table), table.faces, Rt, TABLE_C - 0.01 * TABLE_N), (centred(wall), wall.faces, np.eye(3), np.array([0.0, 0.0, 1.6]))]
    ren = np.stack([RR.render(v, f, RR.look_pose(R, t), DR.K, DR.H, DR.W)[0] for v, f, R, t in parts])
    owner = np.where(ren > 0, ren, np.inf).argmin(0)
    depth = np.where(ren > 0, ren, np.inf).min(0)
    assert np.isfinite(depth).all(), "the wall fills the image"
    dpath = str(root / "depth.png")
    Image.fromarray(np.round(depth * SCENE_SCALE).astype(np.uint16)).save(dpath)
    d = (np.array(Image.open(dpath)).astype(np.float64) / SCENE_SCALE).astype(F)
    cands = []
    for R, t in truth:
        cands += [(R, t), (R @ _rotx(np.pi), t), (R, t + 0.03 * ex), (R @ _rotz(np.deg2rad(1.0)), t + 0.001 * ds)]
    cren = np.stack([RR.render(fv, fixture.faces, RR.look_pose(R, t), DR.K, DR.H, DR.W)[0] for R, t in cands])
    recs = np.zeros(len(cands), dtype=RESULT_DTYPE)
    for r_, (R, t) in zip(recs, cands):
        r_["R"], r_["t"] = np.asarray(R, np.float64).reshape(r_["R"].shape), t
    ref = SR.propose(d, DR.K, 0)
    region = (ref["masks"] > 0).any(0)
    from cppf2_amd import scene
    want = SC.explain(d, region, [0, len(cands)], cren, scene.TAU, scene.MIN_GAIN, scene.VIOL_WEIGHT, scene.MAX_ROUNDS)
    return dict(d=d, owner=owner, depth_png=dpath, root=root, ref=ref, region=region, cren=cren, recs=recs, want=want, truth=truth,
                fixture=fixture)


def test_two_instances_by_the_restatement(scene2):
    """By the CPU renders and the restatement alone: exactly two instances, one per object instance, each the truth or its
    near-duplicate, and the labels cover the recorded share of each instance's visible pixels."""
    want, owner, ref = scene2["want"], scene2["owner"], scene2["ref"]
    vis = [owner == o for o in range(5)]
    print("owners", [int(v.sum()) for v in vis], "segments", ref["seg"][:, :2].tolist(), "static", want["static"].tolist(),
          "chosen", want["chosen"][0].tolist(), "gain", want["gain"][0].tolist(), "net", want["net"][0].tolist(),
          "summary", want["summary"][0].tolist())
    assert vis[0].sum() > 3000 and vis[1].sum() > 3000 and vis[2].sum() > 800
    assert len(ref["masks"]) == 3, "one proposal per object"
    n = int(want["summary"][0, 2])
    chosen = want["chosen"][0, :n].tolist()
    assert n == 2 and sorted(c // 4 for c in chosen) == [0, 1] and all(c % 4 in (0, 3) for c in chosen)
    for k, c in enumerate(chosen):
        o = c // 4
        share = float(((want["labels"][0] == k) & vis[o]).sum()) / float(vis[o].sum())
        print("instance", o, "candidate", c, "share", share)
        assert share >= SHARE[o]
        assert not ((want["labels"][0] == k) & ~vis[o]).any(), "an instance explains pixels of something else"
    assert (want["labels"][0][vis[2]] == 255).all(), "the cylinder is not explained by the mesh object"


@gpu
def test_the_gpu_equals_the_restatement_on_the_scene(scene2):
    """cppf_scene_explain on the CPU renders equals the restatement; explain_candidates, which renders the records on the GPU,
    chooses the same candidates with the same gains and labels."""
    _gpu()
    from cppf2_amd import scene
    s = scene2
    want = _check(s["d"], s["region"], [0, 8], s["cren"], scene.MIN_GAIN, scene.VIOL_WEIGHT, scene.MAX_ROUNDS, F(scene.TAU))
    assert want["chosen"].tobytes() == s["want"]["chosen"].tobytes()
    ex = scene.explain_candidates(s["fixture"], s["d"], s["region"], DR.K, s["recs"])
    n = int(want["summary"][0, 2])
    assert ex["chosen"].tolist() == want["chosen"][0, :n].tolist() and ex["gain"].tolist() == want["gain"][0, :n].tolist()
    assert ex["net"].tolist() == want["net"][0, :n].tolist() and np.array_equal(ex["static"], want["static"])
    assert ex["labels"].tobytes() == want["labels"][0].tobytes()
    assert (ex["region_pixels"], ex["explained_pixels"]) == tuple(want["summary"][0, :2].tolist())
    assert ex["records"].tobytes() == s["recs"][ex["chosen"]].tobytes()
    # a record that cannot be drawn (not finite; behind the camera) fits nothing and is never chosen
    recs = s["recs"][[0, 4, 0, 4]].copy()
    recs["t"][0, 2], recs["t"][1, 2] = np.nan, -1.0
    ex = scene.explain_candidates([s["fixture"]], s["d"], s["region"], DR.K, recs, [0, 0, 0, 0])
    assert ex["chosen"].tolist() in ([2, 3], [3, 2]) and ex["static"][:2].tolist() == [[0, 0, 0], [0, 0, 0]]


@gpu
def test_eval_explains_the_scene(scene2, tmp_path, monkeypatch):
    """eval.py --propose_masks --explain_scene with the object's pair table, 4 verified hypotheses and 10 ICP iterations: the two
    instances of the mesh object on the two proposals that overlap them, the cylinder's proposal rejected; the rest of the report
    is what the run without --explain_scene prints; the multi-object form with the one object id gives the same."""
    import json
    import shutil
    _gpu()
    from cppf2_amd import pair_table
    monkeypatch.chdir(ROOT)
    import eval as ev
    tables, models = tmp_path / "tables", tmp_path / "models"
    tables.mkdir()
    models.mkdir()
    pair_table.build(scene2["fixture"], views=32, seed=0, name="obj_000015.ply").save(str(tables / "obj_000015.npz"))
    shutil.copy(DR.FIXTURE, str(models / "obj_000015.ply"))
    kw = dict(data="depth", depth=scene2["depth_png"], depth_scale=SCENE_SCALE, intrinsics=DR.K.tolist(), num_pairs=20000, num_rots=36,
              opt=False, debug=True, hypotheses=4, icp_iters=10, seed=0, propose_masks=True)
    one = dict(mesh=DR.FIXTURE, mesh_scale=0.001, pair_table=str(tables / "obj_000015.npz"))
    plain = ev.main(**kw, **one)
    rep = ev.main(explain_scene=True, **kw, **one)
    sc = rep["scene"]
    print("best", rep["best"], "proposals", [(p["proposal"], p["pixels"], p.get("score")) for p in rep["proposals"]], "scene",
          [(i["proposal"], i["score"], i["gain"], i["net"]) for i in sc["instances"]], sc["explained_pixels"], sc["region_pixels"],
          sc["rejected"], sc["dropped"])
    assert "scene" not in plain and json.dumps({k: v for k, v in rep.items() if k != "scene"}) == json.dumps(plain)
    assert rep["best"] == plain["best"] and rep["proposals"] == plain["proposals"]
    # the proposals by size: instance 1, instance 0, the cylinder (test_two_instances_by_the_restatement)
    owner, masks = scene2["owner"], scene2["ref"]["masks"] > 0
    assert [int(np.bincount(owner[m], minlength=5).argmax()) for m in masks] == [1, 0, 2]
    assert sorted(i["proposal"] for i in sc["instances"]) == [0, 1] and len(sc["instances"]) == 2
    by_prop = {p["proposal"]: p for p in rep["proposals"]}
    for i in sc["instances"]:
        assert i["score"] >= 0.5 and i["gain"] >= i["net"] >= 200 and i["category"] == "custom"
        assert i["R"] == by_prop[i["proposal"]]["R"] and i["t"] == by_prop[i["proposal"]]["t"] and i["score"] == by_prop[i["proposal"]]["score"]
    assert [i["net"] for i in sc["instances"]] == sorted((i["net"] for i in sc["instances"]), reverse=True)
    assert sc["explained_pixels"] == sum(i["gain"] for i in sc["instances"]) <= sc["region_pixels"] == int(masks.any(0).sum())
    assert [(r["proposal"], r["reason"]) for r in sc["rejected"]] == [(2, "below_min_score")] and sc["dropped"] == 0
    # the multi-object form with the one object id
    multi = ev.main(explain_scene=True, models_dir=str(models), pair_tables=str(tables), obj_ids="15", **kw)

    def strip(x):
        return [{k: v for k, v in e.items() if k != "obj_id"} for e in x]
    assert all(e["obj_id"] == 15 for e in multi["proposals"] + multi["results"] + multi["scene"]["instances"] + multi["scene"]["rejected"])
    assert multi["best"] == dict(rep["best"], obj_id=15) and multi["obj_ids"] == [15]
    assert strip(multi["proposals"]) == rep["proposals"] and strip(multi["results"]) == rep["results"]
    assert strip(multi["scene"]["instances"]) == sc["instances"] and strip(multi["scene"]["rejected"]) == sc["rejected"]
    assert {k: v for k, v in multi["scene"].items() if k not in ("instances", "rejected")} == \
        {k: v for k, v in sc.items() if k not in ("instances", "rejected")}
