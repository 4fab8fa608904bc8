"""GPU checks of cppf_concave_edges: keep and counts equal to the restatement (tests/concave_ref.py) byte
for byte on every shape, step, depth content and form of fg; an image alone, inside a batch and in reversed order; the output at
all four byte alignments between canaries; images crafted so that a comparison of the definition holds with equality; the
argument checks; segment.propose(concave=...) with and without the plane on the nine ray-cast scenes; and the layer end to end
on a generated tabletop scene (eval.py --data=depth --propose_masks --propose_concave --propose_no_plane)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import bop_data_ref as DR  # noqa: E402
import concave_ref as CR  # noqa: E402
import segment_ref as SR  # noqa: E402

F = np.float32
SHAPES = [(1, 1), (1, 64), (33, 4), (37, 53), (3, 1021), (240, 320)]
_EINVAL = -1


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
    """tests/test_segment_gpu.py's kind of scene: a tilted plane about 0.8 m away that covers the lower two thirds of the image,
    a far wall above it, two boxes standing 5 cm and 12 cm in front of the plane, half a millimetre of noise, and (bad) pixels
    with depth 0, NaN, inf, -inf and a negative value."""
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


def _raw(depth, kmat, fg, step, k2, floor2, reach, keep=None, offset=0):
    """cppf_concave_edges itself on host arrays depth [I,H,W], kmat [I,4], fg [I,H,W] or None, with the kernel's own parameters.
    keep: None, "fg" (the output is written over fg) or a uint8 device tensor the output goes into at byte `offset`.
    Returns (status, keep uint8 [I,H,W] on the host, counts [I,3])."""
    import torch
    from cppf2_amd import _lib, ops
    dev = _gpu()
    d = torch.from_numpy(np.ascontiguousarray(depth, dtype=F)).to(dev)
    I, H, W = d.shape
    km = torch.from_numpy(np.ascontiguousarray(kmat, dtype=F).reshape(I, 4)).to(dev)
    mk = None if fg is None else torch.from_numpy(np.ascontiguousarray(fg, dtype=np.uint8)).to(dev)
    counts = torch.full((I, 3), -7, dtype=torch.int32, device=dev)
    if keep is None:
        keep, offset = torch.full((I * H * W,), 0xAB, dtype=torch.uint8, device=dev), 0
    elif isinstance(keep, str):
        keep, offset = mk.reshape(-1), 0
    st = _lib.load().cppf_concave_edges(I, H, W, ops._p(d), ops._p(km), ops._p(mk), int(step), C.c_float(float(k2)),
                                        C.c_float(float(floor2)), C.c_float(float(reach)), C.c_void_p(keep.data_ptr() + offset),
                                        ops._p(counts), ops._stream())
    torch.cuda.synchronize()
    return st, _np(keep)[offset:offset + I * H * W].reshape(I, H, W), _np(counts)


def _want(depth, kmat, fg, step, k2, floor2, reach):
    """The restatement on the same arguments: (keep uint8 [I,H,W], counts [I,3])."""
    keeps, counts = [], []
    for i in range(depth.shape[0]):
        valid, edge = CR.edges(depth[i], np.asarray(kmat).reshape(-1, 4)[i], step, k2, floor2, reach)
        kept = valid & ~edge & (True if fg is None else fg[i] != 0)
        keeps.append(np.where(kept, 255, 0).astype(np.uint8))
        counts.append([valid.sum(), edge.sum(), kept.sum()])
    return np.stack(keeps), np.array(counts)


def _check_raw(depth, kmat, fg, step, k2, floor2, reach, **kw):
    st, keep, counts = _raw(depth, kmat, fg, step, k2, floor2, reach, **kw)
    wk, wc = _want(depth, kmat, fg, step, k2, floor2, reach)
    assert st == 0
    assert counts.tolist() == wc.tolist(), (depth.shape, step, counts.tolist(), wc.tolist())
    assert keep.tobytes() == wk.tobytes(), (depth.shape, step, int((keep != wk).sum()))
    return wk, wc


# ---- shapes, steps, depth content, fg ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 3, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_keep_and_counts_equal_the_restatement(shape, step):
    """Through segment.concave_edges: fg absent, then given.  1 x 1, 1 x 64 and 33 x 4 hold steps larger than the image: no
    profile along that direction gives a verdict.  Zeros, NaN, +-inf and negative readings are in every scene of 16 pixels or
    more."""
    _gpu()
    from cppf2_amd import segment
    H, W = shape
    d, K = _scene(H, W, 11 + H + step), _camera(H, W)
    if shape == (1, 64):
        d[0, 20:40] += F(0.004) * np.abs(np.arange(20) - 10).astype(F)       # a ridge and two valleys on the one row
    rng = np.random.default_rng(H * W + step)
    fg = (rng.random((H, W)) < 0.7).astype(np.uint8) * 255
    for mask in (None, fg):
        for angle, floor in ((15.0, 0.002), (5.0, 0.0)):
            want, wc = CR.concave_edges(d, K, mask, step, angle, floor)
            got, gc = segment.concave_edges(d, K, mask, step, angle, floor)
            assert gc.dtype == np.int64 and gc.shape == (1, 3) and gc[0].tolist() == wc.tolist(), (shape, step, gc.tolist(), wc.tolist())
            assert _np(got)[0].tobytes() == want.tobytes(), (shape, step, angle, floor)
    if min(shape) >= 33 and step <= 3:
        assert wc[1] > 0, "the case no longer has a concave pixel"


def test_keep_may_be_fg_itself():
    H, W = 37, 53
    d = np.stack([_scene(H, W, s) for s in (3, 4)])
    K = np.stack([_camera(H, W)] * 2)
    fg = (np.random.default_rng(9).random((2, H, W)) < 0.6).astype(np.uint8) * 3
    s, k2, f2, reach = CR.params(2, 5.0, 0.0)
    _check_raw(d, K, fg, s, k2, f2, reach)
    wk, wc = _check_raw(d, K, fg, s, k2, f2, reach, keep="fg")
    assert 0 < wc[:, 1].min() and wc[:, 2].max() < wc[:, 0].min()


def test_an_image_does_not_depend_on_the_batch_or_the_order():
    _gpu()
    from cppf2_amd import segment
    H, W = 37, 53
    imgs = np.stack([_scene(H, W, s) for s in (21, 22, 23)])
    Ks = np.stack([np.array(_camera(H, W)) * (1 + 0.01 * i) for i in range(3)])
    fg = (np.random.default_rng(5).random((3, H, W)) < 0.8).astype(np.uint8)
    alone, ac = segment.concave_edges(imgs[2], Ks[2], fg[2], 3, 10.0, 0.0)
    k3, c3 = segment.concave_edges(imgs, Ks, fg, 3, 10.0, 0.0)
    kr, cr = segment.concave_edges(imgs[::-1].copy(), Ks[::-1].copy(), fg[::-1].copy(), 3, 10.0, 0.0)
    assert _np(k3)[2].tobytes() == _np(alone)[0].tobytes() == _np(kr)[0].tobytes()
    assert c3[2].tolist() == ac[0].tolist() == cr[0].tolist()
    assert _np(k3).tobytes() == _np(kr)[::-1].tobytes() and np.array_equal(c3, cr[::-1])
    for i in range(3):
        want, wc = CR.concave_edges(imgs[i], Ks[i], fg[i], 3, 10.0, 0.0)
        assert _np(k3)[i].tobytes() == want.tobytes() and c3[i].tolist() == wc.tolist()
    assert c3[:, 1].min() > 0


@pytest.mark.parametrize("shape", [(37, 53), (3, 1021), (1, 5)], ids=["37x53", "3x1021", "1x5"])
def test_the_output_at_every_alignment_between_canaries(shape):
    """The output's first byte at addresses 0, 1, 2, 3 modulo 4 (two images: the second one's rows start at further phases);
    the bytes before and after it keep their value."""
    import torch
    dev = _gpu()
    H, W = shape
    d = np.stack([_scene(H, W, 31), _scene(H, W, 32)])
    K = np.stack([_camera(H, W)] * 2)
    s, k2, f2, reach = CR.params(1 if W < 8 else 3, 10.0, 0.0)
    wk, wc = _want(d, K, None, s, k2, f2, reach)
    n = 2 * H * W
    for off in (8, 9, 10, 11):
        buf = torch.full((n + 24,), 0xAB, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 4 == 0
        st, keep, counts = _raw(d, K, None, s, k2, f2, reach, keep=buf, offset=off)
        whole = _np(buf)
        assert st == 0 and counts.tolist() == wc.tolist()
        assert keep.tobytes() == wk.tobytes(), (shape, off, int((keep != wk).sum()))
        assert (whole[:off] == 0xAB).all() and (whole[off + n:] == 0xAB).all(), (shape, off)


# ---- crafted images: a comparison of the definition holds with equality ------------------------------------------------------------
def _spike(H, W, r0, c0, z):
    """Depth 1 everywhere but z at (r0, c0), and the camera fx = fy = 1 with the principal point on that pixel: the points are
    A = (-s, 0, 1), B = (0, 0, z), C = (s, 0, 1) along the row and the same along the column, and every product is exact."""
    d = np.ones((1, H, W), F)
    d[0, r0, c0] = z
    return d, np.array([[1.0, 1.0, float(c0), float(r0)]], F)


def test_a_reading_exactly_at_reach_counts_and_one_ulp_beyond_does_not():
    reach = F(0.03125)
    for z, edges in ((F(1.03125), 1), (np.nextafter(F(1.03125), F(2)), 0)):
        d, K = _spike(9, 12, 4, 5, z)
        wk, wc = _check_raw(d, K, None, 1, 0.0, 0.0, reach)
        assert wc[0].tolist() == [108, edges, 108 - edges] and (wk[0, 4, 5] == 0) == bool(edges)
    d, K = _spike(9, 12, 4, 5, F(1.03125))
    assert _check_raw(d, K, None, 1, 0.0, 0.0, np.nextafter(reach, F(0)))[1][0, 1] == 0


def test_the_angle_and_the_floor_are_strict():
    """s = 1, B = (0, 0, 1.125): u = (1, 0, 0.125), t = (2, 0, 0), tt = 4, ut = 2, o = (0, 0, 0.5), ob = 0.5625, oo = 0.25,
    t3 = 64.  4 * oo = 1 = k2 * t3 at k2 = 2^-6, and oo = 0.25 = floor2 * tt * tt at floor2 = 2^-6: equality is not concave,
    one ulp less is."""
    d, K = _spike(9, 12, 4, 5, F(1.125))
    e, below = F(2.0 ** -6), np.nextafter(F(2.0 ** -6), F(0))
    for k2, floor2, edges in ((e, 0.0, 0), (below, 0.0, 1), (0.0, e, 0), (0.0, below, 1), (below, below, 1), (e, below, 0), (below, e, 0)):
        wk, wc = _check_raw(d, K, None, 1, k2, floor2, 1.0)
        assert wc[0, 1] == edges, (k2, floor2, wc.tolist())


def test_profile_ends_on_the_images_border():
    """7 x 7 with s = 3: the centre pixel is the only one whose ends lie inside the image, and they lie on its border.
    u = (3, 0, 0.375), t = (6, 0, 0), tt = 36, o = (0, 0, 13.5), oo = 182.25, t3 = 46 656: 4 * oo = 729 = 2^-6 * t3."""
    d, K = _spike(7, 7, 3, 3, F(1.375))
    for k2, edges in ((F(2.0 ** -6), 0), (np.nextafter(F(2.0 ** -6), F(0)), 1)):
        wk, wc = _check_raw(d, K, None, 3, k2, 0.0, 1.0)
        assert wc[0].tolist() == [49, edges, 49 - edges]
    d[0, 3, 6] = 0.0                                          # the right end invalid: the row's profile is silent, the column's speaks
    assert _check_raw(d, K, None, 3, 0.0, 0.0, 1.0)[1][0].tolist() == [48, 1, 47]
    d[0, 0, 3] = np.nan
    assert _check_raw(d, K, None, 3, 0.0, 0.0, 1.0)[1][0].tolist() == [47, 0, 47]
    assert _check_raw(d[:, :, :6].copy(), K, None, 3, 0.0, 0.0, 1.0)[1][0, 1] == 0            # 7 x 6: no column has both ends


# ---- argument checks ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_nothing_is_written():
    import torch
    from cppf2_amd import _lib, ops
    dev = _gpu()
    H, W = 16, 16
    d = torch.ones((1, H, W), dtype=torch.float32, device=dev)
    km = torch.tensor([[20.0, 20.0, 8.0, 8.0]], dtype=torch.float32, device=dev)
    fg = torch.ones((1, H, W), dtype=torch.uint8, device=dev)
    keep = torch.full((H * W,), 0xAB, dtype=torch.uint8, device=dev)
    counts = torch.full((1, 3), -7, dtype=torch.int32, device=dev)
    L = _lib.load()
    inf, nan = float("inf"), float("nan")

    def call(I=1, H=H, W=W, depths=d.data_ptr(), Kmat=km.data_ptr(), fg=fg.data_ptr(), step=3, k2=0.0173, floor2=4e-6, reach=0.03,
             keep=keep.data_ptr(), counts=counts.data_ptr()):
        return L.cppf_concave_edges(I, H, W, C.c_void_p(depths), C.c_void_p(Kmat), C.c_void_p(fg), step, C.c_float(k2), C.c_float(floor2),
                                    C.c_float(reach), C.c_void_p(keep), C.c_void_p(counts), ops._stream())
    cases = [dict(I=-1), dict(H=0), dict(W=0), dict(H=8193), dict(W=8193), dict(step=0), dict(step=9), dict(k2=-1e-3), dict(k2=inf),
             dict(k2=nan), dict(floor2=-1e-9), dict(floor2=inf), dict(floor2=nan), dict(reach=-0.01), dict(reach=inf), dict(reach=nan),
             dict(depths=None), dict(Kmat=None), dict(keep=None), dict(counts=None), dict(keep=d.data_ptr()),
             dict(keep=d.data_ptr() + 4 * H * W - 1), dict(keep=d.data_ptr() - H * W + 1), dict(I=0, step=0)]
    for kw in cases:
        assert call(**kw) == _EINVAL, kw
        assert b"invalid argument" in L.cppf_last_error_string()
    torch.cuda.synchronize()
    assert (_np(keep) == 0xAB).all() and (_np(counts) == -7).all() and (_np(d) == 1).all()
    assert call(I=0) == 0 and call(I=0, depths=None, Kmat=None, fg=None, keep=None, counts=None) == 0
    torch.cuda.synchronize()
    assert (_np(keep) == 0xAB).all() and (_np(counts) == -7).all()
    assert call(fg=None) == 0 and call() == 0                 # the valid call, last
    torch.cuda.synchronize()
    assert _np(counts).tolist() == [[256, 0, 256]] and (_np(keep) == 255).all()


# ---- segment.propose on the nine scenes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,az", [(n, az) for n in CR.BOXES for az in CR.AZIMUTHS],
                         ids=["%s%+d" % (n, az) for n in CR.BOXES for az in CR.AZIMUTHS])
def test_propose_with_concave_edges_equals_the_restatement(name, az):
    _gpu()
    from cppf2_amd import segment
    d, owner = CR.scene(name, az)
    s = segment.concave_checked()
    for plane in (True, False):
        ref = CR.propose(d, CR.K4, 0, concave=s._asdict(), plane=plane)
        m, props, rep = segment.propose(d, CR.K4, seed=0, concave=s, plane=plane)
        assert _np(m).tobytes() == ref["masks"].tobytes(), (name, az, plane)
        assert [[q["label"], q["pixels"]] + q["bbox"] for q in props] == [
            [int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4] - r[2] + 1), int(r[5] - r[3] + 1)] for r in ref["seg"]]
        assert rep["concave"] == dict(s._asdict(), valid=int(ref["counts"][0]), edge=int(ref["counts"][1]), kept=int(ref["counts"][2]))
        assert np.array(rep["n"] + [rep["d"]], F).tobytes() == ref["plane"].tobytes()
        if plane:
            assert [rep["hypothesis"], rep["inliers"], rep["usable_hypotheses"], rep["valid_pixels"]] == ref["pstats"].tolist()
        else:
            assert [rep["hypothesis"], rep["inliers"], rep["usable_hypotheses"], rep["valid_pixels"]] == [-1, 0, 0, d.size]
            assert rep["n"] == [0.0, 0.0, 0.0] and rep["d"] == 0.0
        # every box is a proposal of its own, with or without the plane
        for b in range(1, int(owner.max()) + 1):
            vis = owner == b
            best = max(float(((p > 0) & vis).sum()) / float(((p > 0) | vis).sum()) for p in ref["masks"])
            assert best >= 0.8, (name, az, plane, b, best)
    # today's path keeps today's bytes
    old = SR.propose(d, CR.K4, 0)
    m, props, rep = segment.propose(d, CR.K4, seed=0)
    assert _np(m).tobytes() == old["masks"].tobytes() and "concave" not in rep


# ---- end to end: a generated tabletop scene ----------------------------------------------------------------------------------------
PHI = np.deg2rad(55.0)       # the table's normal is 55 degrees off the image plane
TABLE_N = np.array([0.0, -np.cos(PHI), -np.sin(PHI)])
TABLE_C = np.array([0.0, 0.10, 0.85])
SCENE_SCALE = 10000.0        # depth units per metre of the scene's PNG


def _rotx(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def _rotz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


@pytest.fixture(scope="module")
def tabletop(tmp_path_factory):
    """tests/test_segment_gpu.py's generated scene, rebuilt: the fixture and a cylinder of radius 15 mm standing on a rendered
    table (a thin box tilted towards the camera), a wall behind, every mesh rendered alone for the pixel owners.  The depth is
    what the 16-bit PNG holds."""
    from PIL import Image
    from cppf2_amd import bop_data, pair_table, render, segment
    dev = _gpu()
    root = tmp_path_factory.mktemp("tabletop_concave")
    ex, ds = np.array([1.0, 0, 0]), np.array([0.0, -np.sin(PHI), np.cos(PHI)])
    Rt = _rotx(np.pi / 2 + PHI)
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
    ref = CR.propose(d, DR.K, 0, concave=segment.concave_checked()._asdict(), plane=False)
    return dict(d=d, owner=owner, depth_png=dpath, table=tpath, pose=ppath, root=root, ref=ref)


def test_eval_with_concave_proposals_and_no_plane(tabletop, tmp_path, monkeypatch):
    """eval.py --data=depth --propose_masks --propose_concave --propose_no_plane with the fixture's pair table, 4 verified
    hypotheses and 10 ICP iterations: `best` is the fixture's proposal, and its pose is bit-equal to a --mask run given that
    proposal's mask (section 21's invariant).  Then a run without the new flags: the report section 21's test pins."""
    from PIL import Image
    from cppf2_amd import segment
    monkeypatch.chdir(ROOT)
    import eval as ev
    kw = dict(data="depth", depth=tabletop["depth_png"], depth_scale=SCENE_SCALE, intrinsics=DR.K.tolist(), num_pairs=20000, num_rots=36,
              opt=False, debug=True, mesh=DR.FIXTURE, mesh_scale=0.001, pair_table=tabletop["table"], hypotheses=4, icp_iters=10, seed=0,
              gt_pose=tabletop["pose"])
    ref, owner = tabletop["ref"], tabletop["owner"]
    vis = owner == 0
    overlap = [int(((p > 0) & vis).sum()) for p in ref["masks"]]
    k = int(np.argmax(overlap))
    print("proposals", ref["seg"].tolist(), "fixture pixels", int(vis.sum()), "overlaps", overlap, "counts", ref["counts"].tolist())
    # the fixture's proposal: made of the fixture's pixels, and the larger part of them (a concave object may lose parts)
    assert overlap[k] > 0.5 * vis.sum() and overlap[k] > 0.9 * (ref["masks"][k] > 0).sum(), "no proposal is the fixture"
    rep = ev.main(propose_masks=True, propose_concave=True, propose_no_plane=True, **kw)
    print("best", rep.get("best"), "proposals", [(p["proposal"], p["pixels"], p.get("score")) for p in rep["proposals"]],
          "skipped", rep["skipped"], "concave", rep["concave"])
    s = segment.concave_checked()
    assert rep["concave"] == dict(s._asdict(), valid=int(ref["counts"][0]), edge=int(ref["counts"][1]), kept=int(ref["counts"][2]))
    assert rep["mask_proposals"]["concave"] == dict(s._asdict()) and rep["mask_proposals"]["plane"] is False
    assert rep["plane"]["n"] == [0.0, 0.0, 0.0] and rep["plane"]["d"] == 0.0 and rep["plane"]["inliers"] == 0
    assert rep["proposed"] == len(ref["masks"])
    assert rep["proposals"] and all(p["pixels"] == int(ref["seg"][p["proposal"], 1]) for p in rep["proposals"])
    assert len(rep["proposals"]) + sum(rep["skipped"].values()) == rep["proposed"]
    assert rep["best"]["proposal"] == k, "the fixture's proposal does not have the highest verification score"
    mpath = str(tmp_path / "m.png")
    Image.fromarray(ref["masks"][k]).save(mpath)
    one = ev.main(mask=mpath, **kw)
    a = one["results"][0]
    b = [r for r in rep["results"] if r["proposal"] == k][0]
    assert np.array(a["pred_RT"]).tobytes() == np.array(b["pred_RT"]).tobytes()
    assert a["verify"] == b["verify"] and a["table_hits"] == b["table_hits"] and a["icp"] == b["icp"]
    # without the new flags: the plane path, its report's keys and numbers
    old = SR.propose(tabletop["d"], DR.K, 0)
    rep0 = ev.main(propose_masks=True, **kw)
    assert "concave" not in rep0 and sorted(rep0["mask_proposals"]) == sorted(
        ["num_hyp", "tau", "min_height", "jump", "min_pixels", "max_segments", "seed", "components", "large_components"])
    assert np.array(rep0["plane"]["n"] + [rep0["plane"]["d"]], F).tobytes() == old["plane"].tobytes()
    assert rep0["proposed"] == 2 and rep0["skipped"] == dict(too_large=0, too_few_points=0)
    assert [(p["proposal"], p["pixels"]) for p in rep0["proposals"]] == [(0, int(old["seg"][0, 1])), (1, int(old["seg"][1, 1]))]
    assert rep0["best"]["proposal"] == 0
