"""GPU checks of the model-to-depth ICP terms (cppf_icp_refine_depth, icp.refine(depth=...)): parity with the NumPy restatement
(tests/icp_depth_ref.py) iteration by iteration on the box views, on the fixture and at edge shapes, special pixels and index
cases; batch independence; the unchanged path without depth; the capability on cut masks; verify.select and eval.main end to end.
The tolerances are tests/test_icp_gpu.py's against icp_ref: inlier counts equal, RMS and pose within 1e-9 per iteration."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import icp_depth_ref as DR  # noqa: E402
import icp_ref as IR  # noqa: E402
import mask_ref as MR  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "example_data", "obj_000015.ply")
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example_data")
TOL = 1e-9                       # tests/test_icp_gpu.py::test_parity_iteration_by_iteration
FIXTURE_VIEWS = 40


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _records(poses):
    from cppf2_amd.pipeline import RESULT_DTYPE
    rec = np.zeros(len(poses), dtype=RESULT_DTYPE)
    for b, (R, t) in enumerate(poses):
        rec[b]["R"], rec[b]["t"] = R, t
    return rec


def _batch(pcs):
    return (np.concatenate(pcs) if len(pcs) else np.zeros((0, 3), np.float32)), np.cumsum([0] + [len(p) for p in pcs])


def _model(mp, mn):
    from cppf2_amd import icp
    return icp.ModelPoints(mp, mn, np.zeros(3))


def _check_steps(model, pcs, rec, depth, img_idx, K, dks, weight=1.0, expect_update=None):
    """iters = 1 calls along `dks`, each from the GPU's previous poses, against one restatement step from the same pose: both
    sides' inlier counts and the visible count equal, the other stats and the pose within TOL.  An instance whose img_idx is
    outside the batch is held to the one-way restatement (icp_ref.step)."""
    from cppf2_amd import icp
    pts, off = _batch(pcs)
    depth = np.asarray(depth, dtype=np.float32)
    depth = depth[None] if depth.ndim == 2 else depth
    for dk in dks:
        before = rec.copy()
        kw = dict(iters=1, max_dist=(float(dk), float(dk)), depth=depth, img_idx=img_idx, K=K, model_weight=weight)
        stats = icp.refine(model, pts if len(pts) else None, off if len(pts) else None, rec, **kw)
        assert stats.shape == (len(rec), 8) and stats.dtype == np.float32
        for b, pc in enumerate(pcs):
            if before[b]["flags"] & 1:
                assert rec[b].tobytes() == before[b].tobytes() and not stats[b].any()
                continue
            i = int(img_idx[b])
            if 0 <= i < len(depth):
                R, t, st = DR.step(pc, before[b]["R"], before[b]["t"], model.pts, model.nrm, dk, depth[i], K, weight)
            else:
                R, t, cnt, rms, upd = IR.step(pc, before[b]["R"], before[b]["t"], model.pts, model.nrm, dk)
                st = np.array([cnt, rms, cnt / len(pc), float(upd), 0, 0, 0, 0])
            assert rec[b]["flags"] == icp.REFINED
            for j in (0, 3, 4, 7):
                assert stats[b, j] == st[j], (b, j, stats[b], st)
            for j in (1, 2, 5, 6):
                assert abs(float(stats[b, j]) - float(np.float32(st[j]))) <= TOL, (b, j, stats[b], st)
            assert np.abs(rec[b]["R"] - R).max() <= TOL and np.abs(rec[b]["t"] - t).max() <= TOL, (b, dk)
            if expect_update is not None:
                assert st[3] == expect_update, (b, st)


@pytest.fixture(scope="module")
def box():
    _gpu()
    mp, mn = DR.box_model()
    return dict(model=_model(mp, mn), views=[DR.box_view(s) for s in range(DR.VIEWS)])


@pytest.fixture(scope="module")
def fixture_views():
    """FIXTURE_VIEWS rendered views of the fixture (uniform SO(3) poses) with their true poses.  The rasterizer samples the
    surface at (c + 0.5, r + 0.5); the views are drawn with the principal point moved by half a pixel, so that pixel (r, c) of
    the image shows the surface on the ray through (c, r) of K, the convention cppf_backproject and the kernel share."""
    dev = _gpu()
    import torch
    from cppf2_amd import icp, ops, render
    mesh = render.load_mesh(FIXTURE, 0.001)
    b = mesh.bounds
    K = np.array(render.INTRINSICS, dtype=np.float64)
    Kr = K.copy()
    Kr[0, 2] += 0.5
    Kr[1, 2] += 0.5
    poses = [render.camera_pose(*render.sample_pose(render.item_rng(3, i), True), 1.0, (b[0] + b[1]) / 2).astype(np.float64)
             .reshape(3, 4) for i in range(FIXTURE_VIEWS)]
    verts, tris = mesh.device(dev)
    T = tris.shape[0]
    depth = render.render_depth(verts, tris.repeat(FIXTURE_VIEWS, 1), ops._offsets([T] * FIXTURE_VIEWS, dev),
                                torch.from_numpy(np.stack(poses).astype(np.float32)).to(dev), Kr).cpu().numpy()
    return dict(mesh=mesh, model=icp.ModelPoints.from_mesh(mesh), K=K, depth=depth, gt=[(P[:, :3], P[:, 3]) for P in poses])


def _example():
    """The example pair's depth scale (it stores 1e-4 m) and intrinsics, as the golden summary records them."""
    import json
    return json.load(open(os.path.join(ROOT, "tests", "golden", "full_summary.json")))["example_backproject"]


def _sub(pc, n, seed):
    if len(pc) <= n:
        return pc
    return pc[np.sort(np.random.default_rng(seed).choice(len(pc), n, replace=False))]


@pytest.mark.parametrize("weight", [1.0, 0.37])
def test_parity_on_the_box_views(box, weight):
    """Three box views two-way (one-face mask), the same three without any observed point, one whose img_idx is out of range
    (it must equal one-way ICP) and one record flagged empty, in one batch: 12 iterations of the default schedule."""
    sel = [0, 3, 5]
    v = [box["views"][s] for s in sel]
    pcs = [x["one_face"] for x in v] + [np.zeros((0, 3), np.float32)] * 3 + [v[0]["one_face"][:700], v[1]["one_face"][:300]]
    rec = _records([(x["R0"], x["t0"]) for x in v] * 2 + [(v[0]["R0"], v[0]["t0"]), (v[1]["R0"], v[1]["t0"])])
    rec[7]["flags"] = 1
    img_idx = np.array([0, 1, 2, 0, 1, 2, 3, 1])
    _check_steps(box["model"], pcs, rec, np.stack([x["depth"] for x in v]), img_idx, DR.K_BOX,
                 IR.schedule(30, 0.05, 0.005)[:12], weight, expect_update=1.0)


def test_parity_without_a_mask_and_with_negative_img_idx(box):
    """max_n = 0 (pts = None): every instance runs on the model side alone; img_idx = -1 then leaves an instance nothing at all:
    no inliers, no update, the pose bytes as they were."""
    v = [box["views"][s] for s in (1, 6)]
    rec = _records([(x["R0"], x["t0"]) for x in v] + [(v[0]["R0"], v[0]["t0"])])
    start = rec.copy()
    from cppf2_amd import icp
    depth = np.stack([x["depth"] for x in v])
    for dk in IR.schedule(30, 0.05, 0.005)[:6]:
        before = rec.copy()
        stats = icp.refine(box["model"], None, None, rec, iters=1, max_dist=(float(dk),) * 2, depth=depth, img_idx=[0, 1, -1],
                           K=DR.K_BOX)
        for b in range(2):
            R, t, st = DR.step(None, before[b]["R"], before[b]["t"], box["model"].pts, box["model"].nrm, dk, depth[b], DR.K_BOX)
            assert stats[b, 0] == 0 and stats[b, 2] == 0 and stats[b, 3] == 1 and stats[b, 4] == st[4] and stats[b, 7] == st[7]
            assert abs(float(stats[b, 5]) - float(np.float32(st[5]))) <= TOL
            assert np.abs(rec[b]["R"] - R).max() <= TOL and np.abs(rec[b]["t"] - t).max() <= TOL
        assert not stats[2].any() and rec[2]["flags"] == icp.REFINED
    assert rec[2]["R"].tobytes() == start[2]["R"].tobytes() and rec[2]["t"].tobytes() == start[2]["t"].tobytes()


def test_parity_on_the_fixture(fixture_views):
    """Four rendered views of the fixture at seeded starts, 1 500 of each view's pixels as the observed points."""
    F = fixture_views
    rng = np.random.default_rng(21)
    sel = [0, 5, 17, 33]
    pcs = [_sub(DR.backproject(F["depth"][i], F["depth"][i] > 0, F["K"]), 1500, i) for i in sel]
    rec = _records([DR.perturb(*F["gt"][i], rng) for i in sel])
    _check_steps(F["model"], pcs, rec, F["depth"][sel], np.arange(4), F["K"], IR.schedule(30, 0.05, 0.005)[:8], expect_update=1.0)


@pytest.mark.parametrize("M,H,W", [(300, 37, 53), (5, 37, 53), (4096, 1, 1), (257, 480, 640)])
def test_parity_at_edge_shapes(M, H, W):
    """M not a multiple of 256, M < 6 (never 6 inliers on the model side alone), a 37 x 53 and a 1 x 1 image."""
    _gpu()
    mp, mn = DR.box_model(M, seed=M)
    rng = np.random.default_rng(M + H)
    if (H, W) == (1, 1):
        K = np.array([[600.0, 0, 0], [0, 600.0, 0], [0, 0, 1]])
    else:
        K = np.array([[W * 0.9, 0, W / 2 - 0.5], [0, W * 0.9, H / 2 - 0.5], [0, 0, 1]])
    R = IR.rodrigues(np.array([0.5, 0.6, 0.3]))
    t = np.array([0.0, 0.0, 0.7])
    depth, face = DR.render_box(R, t, K, H, W)
    full = DR.backproject(depth, face >= 0, K)
    pcs = [_sub(full, 400, 1), np.zeros((0, 3), np.float32)]
    rec = _records([DR.perturb(R, t, rng), DR.perturb(R, t, rng)])
    _check_steps(_model(mp, mn), pcs, rec, depth, np.array([0, 0]), K, IR.schedule(30, 0.05, 0.005)[:6])


def test_parity_on_special_pixels():
    """Samples whose pixel coordinate is exactly on the border or on a tie (col -0.5, W - 1.5, W - 1, W - 0.5, W; the same for
    rows), depths 0 / NaN / inf / negative under some of them, and a pair exactly d_k apart: the kernel and the restatement
    take the same samples (counts and visible counts equal) and the same step."""
    _gpu()
    from cppf2_amd import icp
    H, W = 16, 24
    K = np.array([[128.0, 0, 11.0], [0, 128.0, 7.0], [0, 0, 1]])
    R, t = np.eye(3), np.array([0.0, 0.0, 1.0])
    cols = [-1.0, -0.5, 0.0, 0.5, 1.5, 5.0, 9.0, 11.0, 13.0, W - 1.5, W - 1.0, W - 0.5, float(W)]
    rows = [-1.0, -0.5, 0.0, 2.5, 6.0, 7.0, 10.0, H - 1.5, H - 1.0, H - 0.5, float(H)]
    mp = np.array([[(c - 11.0) / 128.0, (r - 7.0) / 128.0, 0.0] for r in rows for c in cols], np.float32)    # exact in float32
    mn = np.tile(np.array([[0.0, 0.0, -1.0]], np.float32), (len(mp), 1))
    mn[4 * len(cols) + 5] = (0.0, 0.0, 1.0)                           # one back-facing sample inside the image
    depth = np.full((H, W), 1.0, np.float32)
    depth[0, 5], depth[6, 9], depth[6, 13], depth[10, 5], depth[7, 11] = 0.0, np.nan, np.inf, -1.0, 1.25      # (7, 11): straight ahead
    q, idx, vis = DR.project(R, t, mp, mn, depth, K, 0.25)
    pix = {(int(np.rint(r)), int(np.rint(c))) for r in rows for c in cols if 0 <= np.rint(c) < W and 0 <= np.rint(r) < H}
    assert vis == sum(1 for r in rows for c in cols if 0 <= np.rint(c) < W and 0 <= np.rint(r) < H) - 1 and len(pix) > 40
    assert 0 < len(idx) < vis
    hit = [i for i in idx if rows[i // len(cols)] == 7.0 and cols[i % len(cols)] == 11.0]
    assert len(hit) == 1                                              # the pair exactly d_k = 0.25 apart is an inlier ...
    assert hit[0] not in DR.project(R, t, mp, mn, depth, K, np.float32(0.2499))[1]          # ... and not a hair below
    for dk in (0.25, 0.2499, 0.05):
        rec = _records([(R, t)])
        _check_steps(_model(mp, mn), [np.zeros((0, 3), np.float32)], rec, depth, np.array([0]), K, [np.float32(dk)])


def test_independence_of_the_batch(box):
    """40 instances (the 8 views at different starts, mixed point counts, some without points, one flagged empty, 8 images
    addressed by img_idx): each record and its stats are byte-identical alone, in the batch and in the batch reversed."""
    import torch
    from cppf2_amd import icp
    _gpu()
    rng = np.random.default_rng(31)
    V = box["views"]
    depth = np.stack([x["depth"] for x in V])
    pcs, poses, img = [], [], []
    for j in range(40):
        s = j % DR.VIEWS
        pc = V[s]["one_face"]
        pcs.append(pc[:0] if j % 5 == 4 else pc[:int(rng.integers(1, len(pc) + 1))] if j % 3 else pc)
        poses.append(DR.perturb(V[s]["R"], V[s]["t"], rng))
        img.append(s)
    rec0 = _records(poses)
    rec0[11]["flags"] = 1
    kw = dict(K=DR.K_BOX, model_weight=0.5)

    def run(order):
        rec = rec0[order].copy()
        pts, off = _batch([pcs[j] for j in order])
        st = icp.refine(box["model"], pts, off, rec, depth=depth, img_idx=[img[j] for j in order], **kw)
        return rec, st
    order = np.arange(40)
    rec_a, st_a = run(order)
    rec_b, st_b = run(order)
    assert rec_a.tobytes() == rec_b.tobytes() and st_a.tobytes() == st_b.tobytes()
    rec_r, st_r = run(order[::-1])
    assert rec_r[::-1].tobytes() == rec_a.tobytes() and st_r[::-1].tobytes() == st_a.tobytes()
    assert rec_a[11].tobytes() == rec0[11].tobytes() and not st_a[11].any()
    for j in range(40):
        one = rec0[j:j + 1].copy()
        st = icp.refine(box["model"], pcs[j], [0, len(pcs[j])], one, depth=depth[img[j]], **kw)
        assert one.tobytes() == rec_a[j:j + 1].tobytes(), j
        assert st.tobytes() == st_a[j:j + 1].tobytes(), j
    assert (st_a[np.arange(40) != 11, 4] > 0).all()


def test_refine_without_depth_is_the_direct_call(box):
    """icp.refine without depth: the bytes of a direct cppf_icp_refine call on the same inputs, and [B,4] stats."""
    import torch
    from cppf2_amd import _lib, icp, ops
    dev = _gpu()
    V = box["views"]
    pcs = [V[s]["one_face"][:1000 + 100 * s] for s in range(4)]
    rec0 = _records([(V[s]["R0"], V[s]["t0"]) for s in range(4)])
    pts, off = _batch(pcs)
    rec = rec0.copy()
    stats = icp.refine(box["model"], pts, off, rec)
    assert stats.shape == (4, 4)
    L = _lib.load()
    B, max_n = 4, int(np.diff(off).max())
    pts_d = torch.from_numpy(pts).to(dev)
    off_d = torch.from_numpy(off.astype(np.int32)).to(dev)
    rec_d = torch.from_numpy(np.frombuffer(rec0.tobytes(), dtype=np.uint8).reshape(B, 160).copy()).to(dev)
    mp, mn = box["model"].device(dev)
    st_d = torch.empty((B, 4), dtype=torch.float32, device=dev)
    ws = torch.empty((L.cppf_icp_workspace_bytes(B, max_n),), dtype=torch.uint8, device=dev)
    _lib.check(L.cppf_icp_refine(B, ops._p(pts_d), ops._p(off_d), max_n, ops._p(mp), ops._p(mn), mp.shape[0], icp.ITERS,
                                 C.c_float(icp.MAX_DIST[0]), C.c_float(icp.MAX_DIST[1]), ops._p(rec_d), ops._p(st_d), ops._p(ws),
                                 ws.numel(), ops._stream()), "cppf_icp_refine")
    assert rec_d.cpu().numpy().tobytes() == rec.tobytes() and st_d.cpu().numpy().tobytes() == stats.tobytes()


def test_small_workspace_is_refused_with_the_needed_size(box):
    import torch
    from cppf2_amd import _lib, ops
    dev = _gpu()
    L = _lib.load()
    mp, mn = box["model"].device(dev)
    need = L.cppf_icp_depth_workspace_bytes(1, 0, mp.shape[0])
    assert need == 16 * 256 + 64
    x = torch.zeros((4096,), dtype=torch.uint8, device=dev)
    K = (C.c_double * 9)(*DR.K_BOX.reshape(-1))
    rc = L.cppf_icp_refine_depth(1, None, ops._p(x), 0, ops._p(mp), ops._p(mn), mp.shape[0], ops._p(x), 1, 4, 4, ops._p(x), C.addressof(K),
                                 C.c_float(1.0), 1, C.c_float(0.05), C.c_float(0.005), ops._p(x), ops._p(x), ops._p(x), need - 1, None)
    assert rc == -4 and str(need).encode() in L.cppf_last_error_string()


def test_capability_on_the_box_views(box):
    """The 8 views, 30 iterations from the start.  One-way ICP on the one-face mask stays more than FLOOR_MM off; with the
    model-to-depth terms the same mask, and no mask at all, come within CEIL_DEG / CEIL_MM (bounds from the restatement's own
    results, tests/icp_depth_ref.py and DESIGN.md section 19)."""
    from cppf2_amd import icp
    V = box["views"]
    depth = np.stack([x["depth"] for x in V])
    pts, off = _batch([x["one_face"] for x in V])
    start = _records([(x["R0"], x["t0"]) for x in V])
    one, two, free = start.copy(), start.copy(), start.copy()
    icp.refine(box["model"], pts, off, one)
    st2 = icp.refine(box["model"], pts, off, two, depth=depth, K=DR.K_BOX)
    st0 = icp.refine(box["model"], None, None, free, depth=depth, K=DR.K_BOX)
    for s, x in enumerate(V):
        e1, e2, e0 = (DR.pose_err(r[s]["R"], r[s]["t"], x["R"], x["t"]) for r in (one, two, free))
        print("view %d: one-way %.3f deg %.3f mm, two-way %.4f deg %.4f mm, mask-free %.4f deg %.4f mm" % ((s,) + e1 + e2 + e0))
        assert e1[1] > DR.FLOOR_MM, (s, e1)
        assert e2[0] < DR.CEIL_DEG and e2[1] < DR.CEIL_MM, (s, e2)
        assert e0[0] < DR.CEIL_DEG and e0[1] < DR.CEIL_MM, (s, e0)
    assert (st2[:, 3] == icp.ITERS).all() and (st0[:, 0] == 0).all() and (st0[:, 6] > 0.8).all()


def test_capability_on_cut_masks_of_the_fixture(fixture_views):
    """Masks cut by masks.clean at the default jump.  The views are picked on the CPU first (tests/mask_ref.py: the largest
    depth-connected component holds under 60 % of the visible pixels); on each, from the same start (5-10 degrees, 1-2 cm
    off), ICP on the kept part alone against ICP with the model-to-depth terms.  Compared on the translation error, the
    quantity the box scenes' floor is set on (the rotation errors are printed): two-way is no worse on every such view and
    better on the median."""
    from cppf2_amd import icp, masks
    F = fixture_views
    picked = []
    for i in range(FIXTURE_VIEWS):
        vis = F["depth"][i] > 0
        out, st = MR.components(vis, F["depth"][i], masks.JUMP, masks.MIN_PIXELS)
        if st[2] >= masks.MIN_PIXELS and st[2] < 0.6 * st[3]:
            picked.append((i, int(st[2]), int(st[3])))
    print("cut-mask views: %d of %d qualify: %s" % (len(picked), FIXTURE_VIEWS, picked))
    assert len(picked) >= 3, picked
    sel = [p[0] for p in picked]
    kept, stats = masks.clean(np.stack([F["depth"][i] > 0 for i in sel]), F["depth"][sel], np.arange(len(sel)))
    kept = kept.cpu().numpy() > 0
    assert [int(x) for x in stats.cpu().numpy()[:, 2]] == [p[1] for p in picked]
    rng = np.random.default_rng(41)
    pcs = [DR.backproject(F["depth"][i], kept[k], F["K"]) for k, i in enumerate(sel)]
    start = _records([DR.perturb(*F["gt"][i], rng) for i in sel])
    pts, off = _batch(pcs)
    one, two = start.copy(), start.copy()
    icp.refine(F["model"], pts, off, one)
    icp.refine(F["model"], pts, off, two, depth=F["depth"][sel], K=F["K"])
    e1 = np.array([DR.pose_err(one[k]["R"], one[k]["t"], *F["gt"][i]) for k, i in enumerate(sel)])
    e2 = np.array([DR.pose_err(two[k]["R"], two[k]["t"], *F["gt"][i]) for k, i in enumerate(sel)])
    for k, p in enumerate(picked):
        print("view %2d kept %d of %d px: one-way %.3f deg %.3f mm, two-way %.3f deg %.3f mm" % (p + tuple(e1[k]) + tuple(e2[k])))
    print("median translation error: one-way %.3f mm, two-way %.3f mm" % (np.median(e1[:, 1]), np.median(e2[:, 1])))
    assert (e2[:, 1] <= e1[:, 1]).all()
    assert np.median(e2[:, 1]) < np.median(e1[:, 1])


def test_verify_select_with_icp_depth():
    """verify.select(icp_depth=True) on the example pair: it runs, every hypothesis gets flags bit4 and eight stats, those of
    hypothesis h of the instance equal a direct icp.refine(depth=...) call on that record."""
    _gpu()
    from PIL import Image
    from cppf2_amd import icp, ops, render, verify
    e = _example()
    d = (np.array(Image.open(os.path.join(EXAMPLE, "depth.png"))).astype(np.float64) / float(e["depth_scale"])).astype(np.float32)
    m = np.array(Image.open(os.path.join(EXAMPLE, "mask.png")))
    m = (m[..., 0] if m.ndim == 3 else m) > 0
    K = np.array(e["K"], dtype=np.float64)
    mesh = render.load_mesh(FIXTURE, 0.001)
    model = icp.ModelPoints.from_mesh(mesh)
    pc = DR.backproject(d, m & (d > 0), K)[::4]
    c = pc.mean(0).astype(np.float64)
    rng = np.random.default_rng(51)
    recs = _records([(IR.rodrigues(rng.standard_normal(3)), c + 0.01 * rng.standard_normal(3)) for _ in range(4)]).reshape(1, 4)
    out = verify.select(mesh, d[None], m[None], K, recs, pts=pc, pt_off=[0, len(pc)], icp_model=model, icp_iters=10, icp_depth=True,
                        icp_model_weight=0.5)
    assert out["icp"].shape == (1, 4, 8) and (out["hypotheses"]["flags"] & icp.REFINED).all()
    assert out["records"][0]["flags"] & icp.REFINED and out["chosen"][0] >= 0
    direct = recs.reshape(4).copy()
    st = icp.refine(model, np.tile(pc, (4, 1)), np.arange(5) * len(pc), direct, iters=10, depth=d, K=K, model_weight=0.5)
    assert st.tobytes() == out["icp"].tobytes() and direct["R"].tobytes() == out["hypotheses"]["R"].tobytes()
    plain = verify.select(mesh, d[None], m[None], K, recs, pts=pc, pt_off=[0, len(pc)], icp_model=model, icp_iters=10)
    assert plain["icp"].shape == (1, 4, 4)


def test_eval_main_with_icp_depth(monkeypatch):
    """eval.main(data="depth", icp_iters=30, icp_depth=True) on the example pair, both routes: the report carries the eight
    stats and names the entry point, icp.refine / verify.select receive the depth image, and a run without the flag reports
    the four stats as before."""
    _gpu()
    from cppf2_amd import icp, verify
    monkeypatch.chdir(ROOT)
    sys.path.insert(0, ROOT)
    import eval as ev
    e = _example()
    kw = dict(data="depth", depth=os.path.join(EXAMPLE, "depth.png"), mask=os.path.join(EXAMPLE, "mask.png"),
              depth_scale=e["depth_scale"], intrinsics=e["K"], num_pairs=5000, num_rots=36, opt=False, debug=True, mesh=FIXTURE,
              mesh_scale=0.001, icp_iters=30)
    seen = []
    real = icp.refine

    def spy(model, pts, pt_off, results, **k):
        seen.append(k)
        return real(model, pts, pt_off, results, **k)
    monkeypatch.setattr(icp, "refine", spy)
    base = ev.main(**kw)
    rep = ev.main(icp_depth=True, icp_model_weight=2.0, **kw)
    assert set(seen[0]) == {"iters"} and set(seen[1]) == {"iters", "depth", "K", "model_weight"} and seen[1]["model_weight"] == 2.0
    assert seen[1]["depth"].dtype == np.float32 and seen[1]["depth"].shape == (480, 640)
    st = rep["results"][0]["icp"]
    assert set(base["results"][0]["icp"]) == {"inliers", "rms", "inlier_frac", "updates"}
    assert set(st) == {"inliers", "rms", "inlier_frac", "updates", "model_inliers", "model_rms", "model_inlier_frac", "model_visible"}
    assert rep["instances"] == 1 and st["model_visible"] > 0 and rep["icp"] == [st]
    assert "cppf_icp_refine_depth" in rep["icp_refinement"] and "cppf_icp_refine_depth" not in base["icp_refinement"]
    got = []
    real_sel = verify.select

    def spy_sel(*a, **k):
        res = real_sel(*a, **k)
        got.append((k, res))
        return res
    monkeypatch.setattr(verify, "select", spy_sel)
    rep8 = ev.main(icp_depth=True, hypotheses=4, **kw)
    k, res = got[0]
    assert k["icp_depth"] is True and k["icp_model_weight"] == 1.0 and res["icp"].shape == (1, 4, 8)
    assert res["records"][0]["flags"] & icp.REFINED
    assert "model_inliers" in rep8["results"][0]["icp"] and "verify" in rep8["results"][0]
