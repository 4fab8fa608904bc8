"""GPU checks of the proposal kernels: cppf_plane_fit, cppf_plane_foreground and cppf_mask_segments equal
to the restatement (tests/segment_ref.py) byte for byte on every shape, hypothesis count and depth content; an image's plane
alone, inside a batch and in reversed order; the ranking on ties, overflow and borders; and the layer end to end on a generated
tabletop scene (eval.py --data=depth --propose_masks) and on the real frame (python -m cppf2_amd.segment)."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import bop_data_ref as DR  # noqa: E402
import prep_ref as PR  # noqa: E402
import segment_ref as SR  # noqa: E402

F = np.float32
SHAPES = [(1, 1), (1, 64), (33, 4), (37, 53), (3, 1021), (480, 640)]
TAU, MIN_HEIGHT, JUMP = 0.005, 0.01, 0.01


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _np(t):
    return t.cpu().numpy()


def _camera(H, W):
    """A camera whose field of view does not depend on the image size: fx != fy, a principal point off the pixel grid."""
    f = 0.9 * max(H, W, 8)
    return [f, f * 1.01, (W - 1) / 2 + 0.25, (H - 1) / 2 - 0.125]


def _scene(H, W, seed, bad=True):
    """A tilted plane about 0.8 m away that covers the lower two thirds of the image, a far wall above it, two boxes standing
    5 cm and 12 cm in front of the plane, half a millimetre of noise, and (bad) pixels with depth 0, NaN, inf, -inf and a
    negative value."""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = 0.8 - 0.3 * (r - H / 2) / max(H, 8) + 0.05 * (c - W / 2) / max(W, 8)
    d = np.where(r < H // 3, 1.6, d)
    for (r0, r1, c0, c1, lift) in ((H // 2, H // 2 + H // 5, W // 6, W // 6 + W // 5, 0.05),
                                   (H // 2 + H // 8, H - H // 8, W // 2, W // 2 + W // 4, 0.12)):
        d[r0:r1, c0:c1] -= lift
    d = (d + rng.normal(0, 0.0005, (H, W))).astype(F)
    if bad and H * W >= 16:
        p = rng.choice(H * W, size=max(5, H * W // 50), replace=False)
        vals = np.array([0.0, np.nan, np.inf, -np.inf, -0.7], F)
        d.reshape(-1)[p] = vals[np.arange(p.size) % 5]
    return d


def _check_fit(d, K, seed, num_hyp, tau=TAU):
    """cppf_plane_fit and cppf_plane_foreground on one image against the restatement; returns the restatement's result."""
    from cppf2_amd import segment
    plane, stats, counts = SR.fit_plane(d, K, seed, num_hyp, tau)
    gp, gs = segment.fit_plane(d, K, [seed], num_hyp, tau)
    assert _np(gs)[0].tolist() == stats.tolist(), (d.shape, num_hyp, _np(gs)[0].tolist(), stats.tolist())
    assert _np(gp)[0].tobytes() == plane.tobytes(), (d.shape, num_hyp, _np(gp)[0].tolist(), plane.tolist())
    fg = SR.foreground(d, K, plane, MIN_HEIGHT)
    assert _np(segment.foreground(d, K, gp, MIN_HEIGHT))[0].tobytes() == fg.tobytes(), (d.shape, num_hyp)
    return plane, stats, counts, fg


@pytest.mark.parametrize("num_hyp", [1, 64, 65, 1024])
@pytest.mark.parametrize("shape", SHAPES[:5], ids=["%dx%d" % s for s in SHAPES[:5]])
def test_plane_fit_and_foreground_equal_the_restatement(shape, num_hyp):
    _gpu()
    H, W = shape
    d = _scene(H, W, 5 + H)
    if shape == (1, 64):
        d[:] = F(0.75)                                       # constant depth on one row: every triple is collinear
    plane, stats, counts, fg = _check_fit(d, _camera(H, W), 1234567 + num_hyp, num_hyp)
    if shape in ((1, 1), (1, 64)):
        assert stats[0] == -1 and stats[2] == 0 and not plane.any()
        assert np.array_equal(fg > 0, SR.valid_pixels(d)), "no plane: the foreground is the valid pixels"
    if shape == (37, 53) and num_hyp >= 64:
        assert stats[0] >= 0 and 0 < stats[2] < num_hyp and stats[1] > 0.3 * stats[3], "the case no longer has a plane to find"


@pytest.fixture(scope="module")
def vga():
    d = _scene(480, 640, 3)
    return d, _camera(480, 640)


@pytest.mark.parametrize("num_hyp", [1, 65, 256, 1024])
def test_plane_fit_at_480x640(vga, num_hyp):
    _gpu()
    d, K = vga
    plane, stats, counts, fg = _check_fit(d, K, 99, num_hyp)
    if num_hyp >= 256:
        assert stats[1] > 0.4 * stats[3] and 0 < (fg > 0).sum() < 0.5 * stats[3]


def test_images_without_a_valid_pixel_or_a_usable_hypothesis():
    """All pixels invalid: stats (-1, 0, 0, 0), plane zeros, no foreground.  One valid pixel in 37 x 53: no usable hypothesis,
    plane zeros, the pixel is foreground."""
    _gpu()
    K = _camera(37, 53)
    d = np.tile(np.array([0.0, np.nan, np.inf, -1.0], F), 37 * 53)[:37 * 53].reshape(37, 53)
    plane, stats, _, fg = _check_fit(d, K, 7, 64)
    assert stats.tolist() == [-1, 0, 0, 0] and not plane.any() and not fg.any()
    d[20, 30] = 0.9
    plane, stats, _, fg = _check_fit(d, K, 7, 64)
    assert stats.tolist() == [-1, 0, 0, 1] and fg.sum() == 255 and fg[20, 30] == 255


def test_an_exact_plane_ties_and_the_lowest_hypothesis_wins():
    """Constant depth seen by a pinhole camera is a plane in camera space on which every three-point cross product is exact
    (u.z = v.z = 0): every usable hypothesis is (0, 0, -1, z) and holds every valid pixel, so the key decides by index."""
    _gpu()
    d = np.full((37, 53), 0.5, F)
    d[0, 0], d[5, 7], d[36, 52] = 0.0, np.nan, -np.inf
    plane, stats, counts, fg = _check_fit(d, _camera(37, 53), 11, 1024, tau=1e-4)
    usable = np.flatnonzero(counts >= 0)
    assert len(usable) > 100 and (counts[usable] == 37 * 53 - 3).all(), "the hypotheses do not tie"
    assert usable[0] > 0 or counts[0] >= 0
    assert stats.tolist() == [usable[0], 37 * 53 - 3, len(usable), 37 * 53 - 3] and plane.tolist() == [0.0, 0.0, -1.0, 0.5]
    assert not fg.any()


def test_height_exactly_min_height_is_below_and_one_ulp_more_is_above():
    _gpu()
    from cppf2_amd import segment
    # the plane z = 0 with n = (0, 0, 1): the height of a pixel is its depth
    K = _camera(4, 8)
    lo = F(MIN_HEIGHT)
    d = np.full((4, 8), 0.5, F)
    d[1, 2], d[1, 3], d[1, 4] = lo, np.nextafter(lo, F(1)), np.nextafter(lo, F(0))
    plane = np.array([0, 0, 1, 0], F)
    want = SR.foreground(d, K, plane, MIN_HEIGHT)
    assert want[1, 2] == 0 and want[1, 3] == 255 and want[1, 4] == 0 and want.sum() == 255 * (32 - 2)
    assert _np(segment.foreground(d, K, plane, MIN_HEIGHT))[0].tobytes() == want.tobytes()
    # max_height: inclusive
    want = SR.foreground(d, K, plane, 0.0, max_height=lo)
    assert want[1, 2] == 255 and want[1, 3] == 0 and want[1, 4] == 255 and want.sum() == 255 * 2
    assert _np(segment.foreground(d, K, plane, 0.0, lo))[0].tobytes() == want.tobytes()
    # a fitted plane: the threshold moved onto one pixel's own height, and one ulp below it
    d = _scene(37, 53, 8)
    K = _camera(37, 53)
    plane, _, _ = SR.fit_plane(d, K, 5, 64, TAU)
    h = SR.heights(d, K, plane)
    r, c = np.unravel_index(np.nanargmax(np.where(SR.valid_pixels(d), h, -np.inf)), h.shape)
    assert h[r, c] > 0.03
    for thr, bit in ((h[r, c], 0), (np.nextafter(h[r, c], F(0)), 255)):
        want = SR.foreground(d, K, plane, thr)
        assert want[r, c] == bit
        assert _np(segment.foreground(d, K, plane, float(thr)))[0].tobytes() == want.tobytes()


def test_a_plane_does_not_depend_on_the_batch_or_the_order():
    _gpu()
    from cppf2_amd import segment
    H, W = 37, 53
    imgs = np.stack([_scene(H, W, s) for s in (21, 22, 23)])
    Ks = np.stack([np.array(_camera(H, W)) * (1 + 0.01 * i) for i in range(3)])
    seeds = [5, 2 ** 63 + 11, 7]                              # (a seed above 2^63: both key words are used)
    alone_p, alone_s = segment.fit_plane(imgs[2], Ks[2], [seeds[2]], 65, TAU)
    want = SR.fit_plane(imgs[2], Ks[2], seeds[2], 65, TAU)
    assert _np(alone_p)[0].tobytes() == want[0].tobytes() and _np(alone_s)[0].tolist() == want[1].tolist()
    p3, s3 = segment.fit_plane(imgs, Ks, seeds, 65, TAU)
    pr, sr = segment.fit_plane(imgs[::-1].copy(), Ks[::-1].copy(), seeds[::-1], 65, TAU)
    assert _np(p3)[2].tobytes() == _np(alone_p)[0].tobytes() == _np(pr)[0].tobytes()
    assert _np(s3)[2].tolist() == _np(alone_s)[0].tolist() == _np(sr)[0].tolist()
    assert _np(p3).tobytes() == _np(pr)[::-1].tobytes() and np.array_equal(_np(s3), _np(sr)[::-1])
    for i in range(3):
        w = SR.fit_plane(imgs[i], Ks[i], seeds[i], 65, TAU)
        assert _np(p3)[i].tobytes() == w[0].tobytes() and _np(s3)[i].tolist() == w[1].tolist()
    assert _np(s3)[1].tolist() != SR.fit_plane(imgs[1], Ks[1], 11, 65, TAU)[1].tolist(), "the high seed word is ignored"
    fg3 = _np(segment.foreground(imgs, Ks, p3, MIN_HEIGHT))
    for i in range(3):
        assert fg3[i].tobytes() == SR.foreground(imgs[i], Ks[i], _np(p3)[i], MIN_HEIGHT).tobytes()
    with pytest.raises(ValueError):
        segment.fit_plane(imgs[0], PR.INTRINSICS["skew"], [0])


# ---- cppf_mask_segments -----------------------------------------------------------------------------------------------------------
def _check_segments(mask, depth, jump, min_pixels, M):
    from cppf2_amd import segment
    rank, seg, stats = SR.segments(mask, depth, jump, min_pixels, M)
    gr, gs, gt = segment.segments(mask[None], depth, 0, jump, min_pixels, M)
    assert _np(gt)[0].tolist() == stats.tolist(), (mask.shape, M, _np(gt)[0].tolist(), stats.tolist())
    assert np.array_equal(_np(gs)[0], seg), (mask.shape, M, _np(gs)[0].tolist(), seg.tolist())
    assert _np(gr)[0].tobytes() == rank.tobytes(), (mask.shape, M)
    return rank, seg, stats


@pytest.mark.parametrize("shape", SHAPES[:5], ids=["%dx%d" % s for s in SHAPES[:5]])
def test_segments_equal_the_restatement(shape):
    _gpu()
    H, W = shape
    d = _scene(H, W, 40 + W)
    rng = np.random.default_rng(H * W)
    mask = (rng.random((H, W)) < 0.8).astype(np.uint8) * 255
    for min_pixels, M in ((0, 64), (1, 3), (2, 16), (5, 1)):
        _check_segments(mask, d, JUMP, min_pixels, M)


def test_segments_at_480x640(vga):
    _gpu()
    d, K = vga
    plane, _, _ = SR.fit_plane(d, K, 99, 256, TAU)
    fg = SR.foreground(d, K, plane, MIN_HEIGHT)
    rank, seg, stats = _check_segments(fg, d, JUMP, 200, 16)
    assert stats[1] >= 2, "the case no longer has two boxes on the plane"
    _check_segments(fg, d, JUMP, 0, 64)


def test_checkerboard_equal_sizes_overflow_and_borders():
    _gpu()
    from cppf2_amd import masks, segment
    # a checkerboard: every component has one pixel; none reaches min_pixels = 2, and at min_pixels = 1 the first M labels win
    cb = (np.add.outer(np.arange(33), np.arange(40)) % 2 == 0).astype(np.uint8)
    ones = np.ones((33, 40), F)
    rank, seg, stats = _check_segments(cb, ones, 1.0, 2, 8)
    assert stats.tolist() == [660, 0, 0, 660] and (rank == 255).all() and (seg == -1).all()
    rank, seg, stats = _check_segments(cb, ones, 1.0, 1, 64)
    assert stats.tolist() == [660, 64, 660, 660] and seg[:, 0].tolist() == [2 * k for k in range(20)] + [41 + 2 * k for k in range(20)] \
        + [80 + 2 * k for k in range(20)] + [121, 123, 125, 127]
    # equal-sized components (3 x 3 blocks on a grid, more of them than M): ties to the lowest label, exactly M kept
    m = np.zeros((37, 53), np.uint8)
    for r in range(0, 36, 4):
        for c in range(0, 52, 4):
            m[r:r + 3, c:c + 3] = 1
    m[8:11, 8:12] = 1                                        # one block of 12 joins its right neighbour: 3 x 7 = 21 pixels
    rank, seg, stats = _check_segments(m, np.ones((37, 53), F), 0.0, 9, 5)
    assert stats[1] == 5 and stats[0] == stats[2] == 9 * 13 - 1
    assert seg[:, :2].tolist() == [[8 * 53 + 8, 21], [0, 9], [4, 9], [8, 9], [12, 9]]
    assert seg[0].tolist() == [8 * 53 + 8, 21, 8, 8, 14, 10]
    # M = 1 is cppf_mask_components: the same mask bytes, label and pixel count
    d = _scene(37, 53, 77)
    mask = (np.random.default_rng(4).random((37, 53)) < 0.85).astype(np.uint8) * 255
    rank, seg, stats = _check_segments(mask, d, JUMP, 4, 1)
    kept, cstats = masks.clean(mask[None], d, 0, jump=JUMP, min_pixels=4)
    kept, cstats = _np(kept)[0], _np(cstats)[0]
    assert np.array_equal(kept > 0, rank == 0) and cstats[1] == seg[0, 0] >= 0 and cstats[2] == seg[0, 1]
    assert cstats[0] == stats[0] and cstats[3] == stats[3]
    # a frame that touches all four borders, a block inside it
    m = np.zeros((33, 40), np.uint8)
    m[0], m[-1], m[:, 0], m[:, -1] = 1, 1, 1, 1
    m[10:20, 10:20] = 1
    rank, seg, stats = _check_segments(m, np.ones((33, 40), F), 0.0, 1, 4)
    assert seg.tolist() == [[0, 2 * 40 + 2 * 31, 0, 0, 39, 32], [10 * 40 + 10, 100, 10, 10, 19, 19], [-1] * 6, [-1] * 6]


def test_a_serpentine_that_fills_the_image():
    """One one-pixel-wide path through every second row of 64 x 96, joined at alternating ends: one component, the longest
    union-find chains the merge can meet."""
    _gpu()
    H, W = 64, 96
    m = np.zeros((H, W), np.uint8)
    m[0::2] = 1
    for k, r in enumerate(range(1, H - 1, 2)):
        m[r, W - 1 if k % 2 == 0 else 0] = 1
    rank, seg, stats = _check_segments(m, np.ones((H, W), F), 0.0, 1, 2)
    assert stats.tolist() == [1, 1, 1, int(m.sum())] and seg[0].tolist() == [0, int(m.sum()), 0, 0, W - 1, H - 2]


def test_segments_do_not_depend_on_the_batch_or_the_order():
    _gpu()
    from cppf2_amd import segment
    H, W = 37, 53
    depth = np.stack([_scene(H, W, s) for s in (31, 32)])
    rng = np.random.default_rng(2)
    ms = (rng.random((3, H, W)) < 0.8).astype(np.uint8) * 255
    idx = [1, 0, 1]
    r3, s3, t3 = segment.segments(ms, depth, idx, JUMP, 3, 7)
    rr, sr, tr = segment.segments(ms[::-1].copy(), depth, idx[::-1], JUMP, 3, 7)
    r1, s1, t1 = segment.segments(ms[2:3], depth[1], 0, JUMP, 3, 7)
    assert _np(r3)[2].tobytes() == _np(r1)[0].tobytes() == _np(rr)[0].tobytes()
    assert np.array_equal(_np(s3)[2], _np(s1)[0]) and np.array_equal(_np(s3), _np(sr)[::-1])
    assert np.array_equal(_np(t3)[2], _np(t1)[0]) and np.array_equal(_np(t3), _np(tr)[::-1])
    for k in range(3):
        rank, seg, stats = SR.segments(ms[k], depth[idx[k]], JUMP, 3, 7)
        assert _np(r3)[k].tobytes() == rank.tobytes() and np.array_equal(_np(s3)[k], seg) and _np(t3)[k].tolist() == stats.tolist()
    # a mask whose image index is outside the batch has no valid pixel
    r0, s0, t0 = segment.segments(ms[:1], depth, 5, JUMP, 3, 7)
    assert (_np(r0) == 255).all() and (_np(s0) == -1).all() and _np(t0)[0].tolist() == [0, 0, 0, 0]


# ---- end to end: a generated tabletop scene ----------------------------------------------------------------------------------------
PHI = np.deg2rad(55.0)       # the table's normal is 55 degrees off the image plane: the whole wall lies below the table's plane
TABLE_N = np.array([0.0, -np.cos(PHI), -np.sin(PHI)])
TABLE_C = np.array([0.0, 0.10, 0.85])
SCENE_SCALE = 10000.0        # depth units per metre of the scene's PNG
# The cylinder has a radius of 15 mm, not bop_data_ref's 30: next to its silhouette the depth of a cylinder of radius r drops
# by up to sqrt(2 r p) from one pixel to the next (p = z / f, 1.4 mm here): 9 mm at r = 30 mm, more on the ellipse a tilted
# cylinder shows, so rim pixels would leave the component at jump = 1 cm (DESIGN.md section 18's grazing-angle limit); at
# r = 15 mm the step is 6.5 mm.


def _rotx(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def _rotz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


@pytest.fixture(scope="module")
def tabletop(tmp_path_factory):
    """The fixture and a cylinder standing on a rendered table (a thin box tilted towards the camera), a wall behind: the way
    tests/test_bop_detections_gpu.py builds its scenes, every mesh rendered alone for the pixel owners.  The depth is what the
    16-bit PNG holds."""
    from PIL import Image
    from cppf2_amd import bop_data, pair_table, render
    dev = _gpu()
    root = tmp_path_factory.mktemp("tabletop")
    ex, ds = np.array([1.0, 0, 0]), np.array([0.0, -np.sin(PHI), np.cos(PHI)])
    Rt = _rotx(np.pi / 2 + PHI)
    assert np.allclose(Rt @ [0, 0, 1], TABLE_N)
    fixture = render.load_mesh(DR.FIXTURE, 0.001)
    cv, cf = DR.cylinder(r=15.0)
    cyl = render.Mesh(cv * 0.001, cf)
    table, wall = render.Mesh(*DR.box((0.6, 0.5, 0.01))), render.Mesh(*DR.box((1.5, 1.2, 0.01)))

    def stand(mesh, R, u, v):
        b = mesh.bounds
        low = ((mesh.verts - (b[0] + b[1]) / 2) @ R.T @ TABLE_N).min()      # the lowest vertex touches the table top
        return TABLE_C + u * ex + v * ds - low * TABLE_N
    Rf = Rt @ _rotz(0.7)
    poses = [(Rf, stand(fixture, Rf, -0.13, 0.0)), (Rt, stand(cyl, Rt, 0.16, -0.06)), (Rt, TABLE_C - 0.01 * TABLE_N),
             (np.eye(3), np.array([0.0, 0.0, 1.6]))]
    ren = bop_data._render_alone([fixture, cyl, table, wall], [np.hstack([R, t[:, None]]) for R, t in poses], DR.K, DR.H, DR.W,
                                 dev).cpu().numpy()
    owner = np.where(ren > 0, ren, np.inf).argmin(0)
    owner[~(ren > 0).any(0)] = -1
    depth = np.where(ren > 0, ren, np.inf).min(0)
    assert np.isfinite(depth).all(), "the wall fills the image"
    dpath = str(root / "depth.png")
    Image.fromarray(np.round(depth * SCENE_SCALE).astype(np.uint16)).save(dpath)
    d = (np.array(Image.open(dpath)).astype(np.float64) / SCENE_SCALE).astype(F)
    tpath, ppath = str(root / "table.npz"), str(root / "pose.txt")
    pair_table.build(fixture, views=32, seed=0, name="obj_000015.ply").save(tpath)
    np.savetxt(ppath, np.hstack([poses[0][0], poses[0][1][:, None]]))
    return dict(d=d, owner=owner, depth_png=dpath, table=tpath, pose=ppath, root=root, ref=SR.propose(d, DR.K, 0))


def test_tabletop_proposals_are_the_objects(tabletop):
    """By the renders and the restatement alone: one proposal per object, none holds a table or wall pixel, each covers its
    object's visible pixels that the fitted plane puts more than min_height above the table.  Then the GPU equals the restatement."""
    from cppf2_amd import segment
    d, owner, ref = tabletop["d"], tabletop["owner"], tabletop["ref"]
    vis = [(owner == o) for o in range(4)]
    h = SR.heights(d, DR.K, ref["plane"])
    print("owners", [int(v.sum()) for v in vis], "plane", ref["plane"].tolist(), ref["pstats"].tolist(), "segments", ref["stats"].tolist(),
          ref["seg"].tolist(), "table heights", float(h[vis[2]].min()), float(h[vis[2]].max()))
    assert vis[0].sum() > 3000 and vis[1].sum() > 800 and vis[2].sum() > 100000 and vis[3].sum() > 20000
    assert len(ref["masks"]) == 2 and ref["stats"][1] == 2
    for p, o in zip(ref["masks"], (0, 1)):                    # the fixture is the larger
        p = p > 0
        assert not (p & (vis[2] | vis[3])).any(), "a proposal holds table or wall pixels"
        assert not (p & vis[1 - o]).any()
        assert not (vis[o] & (h > F(MIN_HEIGHT)) & ~p).any(), "a proposal misses part of its object"
        assert (p & vis[o]).sum() > 0.9 * vis[o].sum()
    m, props, plane = segment.propose(d, DR.K, seed=0)
    assert _np(m).tobytes() == ref["masks"].tobytes()
    assert [[q["label"], q["pixels"]] + q["bbox"] for q in props] == [
        [int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4] - r[2] + 1), int(r[5] - r[3] + 1)] for r in ref["seg"]]
    assert np.array(plane["n"] + [plane["d"]], F).tobytes() == ref["plane"].tobytes()
    assert [plane["hypothesis"], plane["inliers"], plane["usable_hypotheses"], plane["valid_pixels"]] == ref["pstats"].tolist()


def test_eval_with_proposed_masks(tabletop, tmp_path, monkeypatch):
    """eval.py --data=depth --propose_masks with the fixture's pair table, 4 verified hypotheses and 10 ICP iterations: `best` is
    the fixture's proposal, and each proposal's pose is bit-equal to a --mask run given that proposal's mask."""
    from PIL import Image
    monkeypatch.chdir(ROOT)
    import eval as ev
    kw = dict(data="depth", depth=tabletop["depth_png"], depth_scale=SCENE_SCALE, intrinsics=DR.K.tolist(), num_pairs=20000, num_rots=36,
              opt=False, debug=True, mesh=DR.FIXTURE, mesh_scale=0.001, pair_table=tabletop["table"], hypotheses=4, icp_iters=10, seed=0,
              gt_pose=tabletop["pose"])
    rep = ev.main(propose_masks=True, **kw)
    ref = tabletop["ref"]
    print("plane", rep["plane"], "best", rep.get("best"), "proposals", [(p["proposal"], p["pixels"], p.get("score")) for p in rep["proposals"]],
          "skipped", rep["skipped"], "bop", {k: rep["bop"][k] for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR") if k in rep.get("bop", {})})
    assert rep["plane"]["inliers"] == ref["pstats"][1] and rep["plane"]["usable_hypotheses"] == ref["pstats"][2]
    assert np.array(rep["plane"]["n"] + [rep["plane"]["d"]], F).tobytes() == ref["plane"].tobytes()
    assert rep["proposed"] == 2 and rep["skipped"] == dict(too_large=0, too_few_points=0)
    assert [(p["proposal"], p["pixels"]) for p in rep["proposals"]] == [(0, int(ref["seg"][0, 1])), (1, int(ref["seg"][1, 1]))]
    assert all("score" in p and p["R"] is not None for p in rep["proposals"])
    assert rep["best"]["proposal"] == 0, "the fixture's proposal does not have the highest verification score"
    assert rep["best"]["score"] == rep["proposals"][0]["score"] > rep["proposals"][1]["score"]
    assert "bop" in rep["results"][0] and "bop" not in rep["results"][1]
    for k in (0, 1):
        mpath = str(tmp_path / ("m%d.png" % k))
        Image.fromarray(ref["masks"][k]).save(mpath)
        one = ev.main(mask=mpath, **kw)
        a, b = one["results"][0], rep["results"][k]
        assert np.array(a["pred_RT"]).tobytes() == np.array(b["pred_RT"]).tobytes(), k
        assert np.array_equal(np.array(b["pred_RT"])[:3, 3], np.array(rep["proposals"][k]["t"]))
        assert a["verify"] == b["verify"] and a["table_hits"] == b["table_hits"] and a["icp"] == b["icp"]


# ---- end to end: the real frame ----------------------------------------------------------------------------------------------------
def test_real_frame_proposals_and_the_detections_file(tmp_path):
    """The GPU proposals on example_data/depth.png equal the restatement's, which tests/test_segment.py bounds; the detections
    file of `python -m cppf2_amd.segment` reads back to the same masks, once per object id."""
    _gpu()
    from cppf2_amd import bop_data, masks, segment
    d, _ = SR.example_frame()
    ref = SR.propose(d, PR.EXAMPLE_K, SR.REAL_SEED)
    m, props, plane = segment.propose(d, PR.EXAMPLE_K, seed=SR.REAL_SEED)
    assert _np(m).tobytes() == ref["masks"].tobytes() and len(props) == ref["stats"][1] >= 4
    assert [plane["hypothesis"], plane["inliers"], plane["usable_hypotheses"], plane["valid_pixels"]] == ref["pstats"].tolist()
    assert [plane["components"], len(props), plane["large_components"]] == ref["stats"][:3].tolist()
    out = str(tmp_path / "dets.json")
    k = PR.EXAMPLE_K
    assert segment.main(["--depth", os.path.join(ROOT, "tests", "golden", "example_data", "depth.png"), "--depth-scale", "10000",
                         "--intrinsics", "%r,%r,%r,%r" % (k[0][0], k[1][1], k[0][2], k[1][2]), "--obj-ids", "1,15", "--scene-id", "48",
                         "--image-id", "1", "--seed", str(SR.REAL_SEED), "--out", out]) == 0
    dets = bop_data.read_detections(out, image_size=d.shape)
    P = len(props)
    assert len(dets) == 2 * P and [e["category_id"] for e in dets] == [1] * P + [15] * P
    assert all(e["scene_id"] == 48 and e["image_id"] == 1 and e["score"] == 1.0 for e in dets)
    back = _np(masks.decode_batch([e["counts"] for e in dets], *d.shape))
    assert back[:P].tobytes() == ref["masks"].tobytes() == back[P:].tobytes()
    assert [e["bbox"] for e in dets[:P]] == [[float(v) for v in q["bbox"]] for q in props]
    json.load(open(out))
