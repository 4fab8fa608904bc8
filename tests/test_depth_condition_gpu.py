"""GPU checks of depth conditioning: cppf_depth_condition byte-equal to the NumPy restatement
(tests/depth_condition_ref.py) at every shape, radius and threshold at which the kernel takes another path, its call hygiene,
the caps of the analytic scene through depthfilter.condition, normals before and after, eval.py --condition_depth on the scene
written as a PNG, and fusion with and without conditioning (measured, with a loose bound)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import depth_condition_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
TH, TW = R.TH, R.TW
JUMP = 2.0 ** -7
GUARD = 64                       # canary elements on either side of both outputs
CANARY_F, CANARY_I = -7.25, -77
RADII = [(0, 0), (1, 0), (0, 1), (1, 2), (2, 4), (4, 4)]
SIZES = [(1, 1), (1, 9), (9, 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 3, 2 * TW - 1)]


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def supports(r1):
    """The four min_support values: 0, the default (as far as r1 admits it), (2 r1 + 1)^2 - 1 and (2 r1 + 1)^2."""
    full = (2 * r1 + 1) ** 2
    return sorted({0, min(4, full), full - 1, full})


def dev_condition(img, r1=1, ms=4, r2=0, jump=JUMP, rel=0.0, calls=1):
    """cppf_depth_condition itself on a host array [I,H,W], both outputs between canaries that must survive: (out, counts) of
    each of `calls` calls on one input, which must keep its bytes."""
    import torch
    from cppf2_amd import _lib, ops
    dev, L = ops._dev(), _lib.load()
    img = np.ascontiguousarray(img, dtype=F)
    I, H, W = img.shape
    d = torch.from_numpy(img).to(dev)
    n = I * H * W
    res = []
    for _ in range(calls):
        out = torch.full((n + 2 * GUARD,), CANARY_F, dtype=torch.float32, device=dev)
        cnt = torch.full((3 * I + 2 * GUARD,), CANARY_I, dtype=torch.int32, device=dev)
        o, c = out[GUARD:GUARD + n], cnt[GUARD:GUARD + 3 * I]
        _lib.check(L.cppf_depth_condition(ops._p(d), I, H, W, r1, ms, r2, C.c_float(jump), C.c_float(rel), ops._p(o), ops._p(c),
                                          ops._stream()), "cppf_depth_condition")
        for b, v in ((out, CANARY_F), (cnt, CANARY_I)):
            assert bool((b[:GUARD] == v).all()) and bool((b[-GUARD:] == v).all()), "a canary was overwritten"
        res.append((o.cpu().numpy().reshape(I, H, W), c.cpu().numpy().reshape(I, 3)))
    assert same_bits(d.cpu().numpy(), img)
    return res[0] if calls == 1 else res


def assert_equal(img, **kw):
    want_out, want_counts, _ = R.condition(img, kw.get("r1", 1), kw.get("ms", 4), kw.get("r2", 0), kw.get("jump", JUMP), kw.get("rel", 0.0))
    out, counts = dev_condition(img, **kw)
    assert same_bits(out, want_out), (kw, int((out.view(np.uint32) != want_out.view(np.uint32)).sum()))
    assert counts.astype(np.int64).tolist() == want_counts.tolist(), kw
    return want_out, want_counts


# ----------------------------------------------------------------------------------------------
# byte equality
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SIZES)
def test_every_shape_radius_and_threshold_equals_the_restatement_byte_for_byte(H, W):
    seen = np.zeros(3, np.int64)
    for I in (1, 3):
        img = R.lattice_images(100 * H + W + I, I, H, W, dead=1 if I == 3 else None)
        for r1, r2 in RADII:
            for ms in supports(r1):
                for rel in (0.0, 2.0 ** -6):
                    _, counts = assert_equal(img, r1=r1, ms=ms, r2=r2, rel=rel)
                    seen += counts.sum(0)
                    assert I == 1 or counts[1].tolist() == [0, 0, 0]
    assert seen[0] > 0 and (H * W < 9 or (seen > 0).all()), seen


def test_more_images_than_the_grid_has_rows_for_and_many_tiles():
    """70 000 images of 3 x 5 pixels: the grid's second dimension holds 65 535, so the first 4 465 blocks take a second image;
    and one image of 50 x 200: 4 x 4 tiles, the last row and column partial."""
    img = R.lattice_images(7, 70000, 3, 5)
    want_out, want_counts, _ = R.condition(img, 1, 4, 1, JUMP, 0.0)
    out, counts = dev_condition(img, r2=1)
    assert same_bits(out, want_out) and counts.astype(np.int64).tolist() == want_counts.tolist()
    assert_equal(R.lattice_images(8, 1, 50, 200), r1=2, ms=12, r2=3)


def test_the_constructed_images_of_the_cpu_test():
    def up(x):
        return np.nextafter(F(x), F(np.inf), dtype=F)
    a = np.full((1, 3, 3), 0.5, F)
    a[0, 0, 2] = F(0.5 + JUMP)
    b = a.copy()
    b[0, 0, 2] = up(0.5 + JUMP)
    for img in (a, b):
        for ms in (7, 8):
            assert_equal(img, ms=ms)
    c = a.copy()
    c[0, 0, 2] = F(0.5 + 2.0 ** -6)
    e = a.copy()
    e[0, 0, 2] = up(0.5 + 2.0 ** -6)
    assert assert_equal(c, ms=8, rel=2.0 ** -6)[0][0, 1, 1] == F(0.5) and assert_equal(e, ms=8, rel=2.0 ** -6)[0][0, 1, 1] == 0
    row = np.array([[[0.5 + 2.0 ** -10, 0.5, 0.7]]], F)
    assert assert_equal(row, r1=0, ms=0, r2=1)[0][0, 0, 1] == F(0.5)
    row[0, 0, 2] = F(0.5 + 3 * 2.0 ** -10)
    assert assert_equal(row, r1=0, ms=0, r2=1)[1].tolist() == [[3, 0, 1]]
    one = np.array([[[0.625]]], F)
    for kw in (dict(), dict(ms=8), dict(ms=9), dict(r1=4, ms=80, r2=4), dict(r1=0, ms=0, r2=2)):
        assert_equal(one, **kw)
    corner = np.full((1, 2, 2), 0.5, F)
    corner[0, 1, 1] = 0.75
    assert assert_equal(corner, ms=6)[0].tolist() == [[[0.5, 0.5], [0.5, 0.0]]]
    special = np.array([[[np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e-40, 0.5]]], F)
    out, counts = assert_equal(special, r1=0, ms=0)
    assert counts.tolist() == [[2, 0, 0]] and out[0, 0, 6] == F(1e-40) > 0                # the denormal stays, bit for bit
    for ms in (6, 7, 8):
        assert_equal(special, ms=ms, r2=1)
    L, m, Rr = F(0.5), F(0.5 + 8 * 2.0 ** -10), F(0.5 + 20 * 2.0 ** -10)
    step = np.repeat(np.array([[L, L, L, m, Rr, Rr, Rr]], F), 5, 0)[None]
    assert assert_equal(step, ms=6, r2=1)[0][0, 2, 2] == L                               # stage 2 reads stage 1's output
    assert_equal(np.full((1, 5, 6), 0.75, F), ms=8)
    big = np.full((1, 2, 3), 3e38, F)                                                    # tol overflows to +inf: everything is near
    assert_equal(big, r1=1, ms=8, r2=1, rel=2.0)


# ----------------------------------------------------------------------------------------------
# call hygiene
# ----------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes_no_images_is_valid_and_refusals_write_nothing():
    import torch
    from cppf2_amd import _lib, ops
    img = R.lattice_images(3, 3, 2 * TH + 3, 2 * TW - 1, dead=2)
    first, second = dev_condition(img, r1=2, ms=10, r2=2, calls=2)
    assert same_bits(first[0], second[0]) and same_bits(first[1], second[1])
    dev, L = ops._dev(), _lib.load()
    d = torch.from_numpy(img).to(dev)
    out = torch.full(img.shape, CANARY_F, dtype=torch.float32, device=dev)
    cnt = torch.full((3, 3), CANARY_I, dtype=torch.int32, device=dev)

    def call(depth=d, I=3, H=img.shape[1], W=img.shape[2], r1=1, ms=4, r2=0, jump=JUMP, rel=0.0, o=out, c=cnt):
        return L.cppf_depth_condition(ops._p(depth), I, H, W, r1, ms, r2, C.c_float(jump), C.c_float(rel), ops._p(o), ops._p(c),
                                      ops._stream())
    assert call(I=0) == 0 and call(I=0, depth=None, o=None, c=None) == 0
    for kw in (dict(o=d), dict(o=d.view(-1)[4:]), dict(depth=None), dict(o=None), dict(c=None), dict(I=-1), dict(H=0), dict(W=16385),
               dict(r1=5), dict(r2=-1), dict(ms=10), dict(ms=-1), dict(r1=0, ms=2), dict(jump=-1.0), dict(jump=float("nan")),
               dict(rel=float("inf"))):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((out == CANARY_F).all()) and bool((cnt == CANARY_I).all()) and same_bits(d.cpu().numpy(), img)
    assert call() == 0
    want_out, want_counts, _ = R.condition(img, jump=JUMP)
    assert same_bits(out.cpu().numpy(), want_out) and cnt.cpu().numpy().tolist() == want_counts.tolist()


def test_the_wrapper():
    import torch
    from cppf2_amd import depthfilter as DF, masks, ops
    img = R.lattice_images(5, 2, 33, 70)
    out, counts = DF.condition(img)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == img.shape
    assert isinstance(counts, np.ndarray) and counts.dtype == np.int64 and counts.shape == (2, 3)
    want_out, want_counts, _ = R.condition(img, jump=masks.JUMP)
    assert same_bits(out.cpu().numpy(), want_out) and counts.tolist() == want_counts.tolist()
    dev_img = torch.from_numpy(img[0]).to(ops._dev())
    out, counts = DF.condition(dev_img, 2, 10, 2, JUMP, 2.0 ** -6)                         # [H,W], a device tensor
    want_out, want_counts, _ = R.condition(img[:1], 2, 10, 2, JUMP, 2.0 ** -6)
    assert same_bits(out.cpu().numpy(), want_out) and counts.tolist() == want_counts.tolist()
    assert same_bits(dev_img.cpu().numpy(), img[0])
    out, _ = DF.condition(img, flying_radius=0, smooth_radius=1)                           # stage 1 off: min_support is not used
    assert same_bits(out.cpu().numpy(), R.condition(img, 0, 0, 1, masks.JUMP)[0])
    s = DF.checked(2, 10, 2, JUMP, 2.0 ** -6)
    got, summary = DF.apply(img[:1], s)
    assert same_bits(got.cpu().numpy(), want_out) and summary == DF.summary(s, want_counts)
    with pytest.raises(DF.CppfError):
        DF.condition(torch.from_numpy(img))
    with pytest.raises(ValueError):
        DF.condition(np.zeros((0, 4, 4), F))


# ----------------------------------------------------------------------------------------------
# the scene
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conditioned_scene(sigma):
    """(the scene, the defaults' output, smooth_radius = 2's output) through depthfilter.condition."""
    from cppf2_amd import depthfilter as DF
    sc = R.scene(sigma)
    depth = sc["depth"].copy()                                 # (the scene's arrays are read-only)
    return sc, DF.condition(depth)[0][0].cpu().numpy(), DF.condition(depth, smooth_radius=2)[0][0].cpu().numpy()


@pytest.mark.parametrize("sigma", [0.001, 0.002])
def test_the_scene_on_the_device(sigma):
    sc, plain, smooth = conditioned_scene(sigma)
    assert same_bits(plain, R.condition(sc["depth"])[0][0]) and same_bits(smooth, R.condition(sc["depth"], r2=2)[0][0])
    fig = R.scene_figures(sc, plain, smooth)
    print("scene sigma=%g on the device: %s" % (sigma, fig))
    R.check_scene(fig)


K_SCENE = np.array([[R.F0, 0, R.W0 / 2 - 0.5], [0, R.F0, R.H0 / 2 - 0.5], [0, 0, 1]])
NORMAL_R = 0.02             # eval.py --data=depth: 10 * res of config/custom.yaml (ensemble.py: cfg.res * 10)


def normal_error(depth, mask):
    """Mean angle (degrees) between the library's normals of the masked cloud, as eval.py --data=depth builds it (2 mm voxels,
    radius 2 cm), and the sphere's analytic normals, whatever the sign; the points' count."""
    from cppf2_amd import shot
    from cppf2_amd.ensemble import instance_cloud
    pc = instance_cloud(depth.astype(np.float64), K_SCENE, mask, 2e-3, 0)
    n = shot.estimate_normal(pc, NORMAL_R).reshape(-1, 3).astype(np.float64)
    true = pc.astype(np.float64) - R.CENTRE
    true /= np.linalg.norm(true, axis=1, keepdims=True)
    ok = np.isfinite(n).all(1) & (np.linalg.norm(n, axis=1) > 0.5)
    cos = np.abs((n[ok] * true[ok]).sum(1)) / np.linalg.norm(n[ok], axis=1)
    return float(np.degrees(np.arccos(np.clip(cos, 0, 1))).mean()), int(ok.sum())


@pytest.mark.parametrize("sigma", [0.001, 0.002])
def test_normals_are_no_worse_after_conditioning(sigma):
    """Measured: see the section's table; the assertion is conditioned <= raw on the same noise draw."""
    sc, _, smooth = conditioned_scene(sigma)
    raw, n_raw = normal_error(sc["depth"], sc["mask"])
    after, n_after = normal_error(smooth, sc["mask"])
    print("normals sigma=%g radius %g: %.3f degrees raw (%d points), %.3f conditioned (%d points)" % (sigma, NORMAL_R, raw, n_raw, after, n_after))
    assert n_raw > 500 and n_after > 500
    assert after <= raw


def test_eval_depth_mode_conditions_the_image_once(monkeypatch, tmp_path):
    from PIL import Image
    monkeypatch.chdir(ROOT)
    import eval as ev
    sc = R.scene(0.001)
    dpath, mpath = str(tmp_path / "depth.png"), str(tmp_path / "mask.png")
    Image.fromarray(np.clip(np.rint(sc["depth"].astype(np.float64) * 10000.0), 0, 65535).astype(np.uint16)).save(dpath)
    Image.fromarray(sc["mask"].astype(np.uint8) * 255).save(mpath)
    clouds = []
    inner = ev.usable_cloud

    def recording(*a, **kw):
        out = inner(*a, **kw)
        clouds.append(out[0])
        return out
    monkeypatch.setattr(ev, "usable_cloud", recording)
    kw = dict(data="depth", depth=dpath, mask=mpath, depth_scale=10000.0, intrinsics=K_SCENE.tolist(), num_pairs=3000, num_rots=36,
              opt=False, debug=True)
    far = []
    for flags in (dict(), dict(condition_depth=True)):
        del clouds[:]
        rep = ev.main(**dict(kw, **flags))
        assert rep["instances"] == 1 and len(clouds) == 1
        pc = clouds[0].astype(np.float64)
        far.append(int((np.abs(np.linalg.norm(pc - R.CENTRE, axis=1) - R.RADIUS) > R.FAR).sum()))
        if not flags:
            assert "depth_condition" not in rep
            continue
        c = rep["depth_condition"]
        png = (np.array(Image.open(dpath)).astype(np.float64) / 10000.0).astype(F)
        want = R.condition(png, r2=flags.get("smooth_radius", 0))[1][0].tolist()
        assert [c["valid"], c["removed"], c["smoothed"]] == want and c["removed"] > 100
        assert c["flying_radius"] == 1 and c["min_support"] == 4 and c["smooth_radius"] == flags.get("smooth_radius", 0)
    print("eval.py --data=depth: points of the instance's cloud farther than 5 mm from the sphere: %s" % far)
    assert far[0] > 0 and far[1] == 0


# ----------------------------------------------------------------------------------------------
# fusion: measured, with a loose bound
# ----------------------------------------------------------------------------------------------
def icosphere(centre, radius, levels=4):
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v) * radius + centre, np.asarray(f, dtype=np.int64)


def test_fusion_with_and_without_conditioning():
    """The 18 table views of tests/test_close_gpu.py (the sphere on the table z = DOME_PZ), rendered at 4 x and block-averaged
    so that silhouette pixels are mixed; fused without and with conditioning at its defaults.  Recorded, and asserted only that
    the share of vertices farther than one voxel from the analytic surface does not grow by more than 0.01.  Measured (DESIGN.md
    section 33): 0.0000 raw (6 956 vertices), 0.0000 conditioned (7 041 vertices): the other views carve a view's mixed pixels away."""
    import torch
    import close_ref as cref
    import fuse_ref as ref
    from cppf2_amd import depthfilter as DF, fuse, ops, render
    dev = ops._dev()
    pz = ref.CENTRE[2] - 0.6 * ref.RADIUS
    poses = ref.look_at(cref.table_dirs())
    sv, sf = icosphere(ref.CENTRE, ref.RADIUS)
    s = 0.2                                   # every corner stays in front of every camera: the renderer does not clip
    tv = np.array([[-s, -s, pz], [s, -s, pz], [s, s, pz], [-s, s, pz]]) + np.array([ref.CENTRE[0], ref.CENTRE[1], 0.0])
    sphere = render.Mesh(sv, sf)
    both = render.Mesh(np.concatenate([sv, tv]), np.concatenate([sf, np.array([[0, 1, 2], [0, 2, 3]]) + len(sv)]))
    SS, H, W = 4, ref.H, ref.W
    fx, fy, cx, cy = ref.K4
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    K_fine = np.array([[SS * fx, 0, SS * cx], [0, SS * fy, SS * cy], [0, 0, 1]])
    V = len(poses)
    P = torch.from_numpy(np.asarray(poses, dtype=np.float32).reshape(V, 12)).to(dev)
    fine = []
    for mesh in (both, sphere):
        verts, tris = mesh.device(dev)
        fine.append(render.render_depth(verts, tris.repeat(V, 1), ops._offsets([tris.shape[0]] * V, dev), P, K_fine, SS * H, SS * W,
                                        cull=False).cpu().numpy().astype(np.float64))
    assert (fine[1] > 0).any() and (fine[0] > 0).sum() > (fine[1] > 0).sum()
    blocks = fine[0].reshape(V, H, SS, W, SS)
    depth = np.where((blocks > 0).all((2, 4)), blocks.mean((2, 4)), 0.0).astype(F)     # past the table's edge: no reading
    hit = ((fine[1] > 0) & (fine[1] == fine[0])).reshape(V, H, SS, W, SS).mean((2, 4))
    masks = (hit >= 0.5).astype(np.uint8)
    mixed = (hit > 0) & (hit < 1)
    assert mixed.sum() > 18 * 100
    origin, dims, trunc = ref.sphere_volume()
    share, verts = [], []
    for cond in (None, DF.checked()):
        vol = fuse.Volume(origin, ref.VOXEL, dims, trunc)
        mesh, report = fuse.fuse_views(depth, masks, poses, K, ref.VOXEL, volume=vol, pixel_offset=0.5, condition=cond)
        v = np.asarray(mesh.verts, dtype=np.float64)
        dist = np.minimum(ref.sphere_distance(v), np.abs(v[:, 2] - pz))
        share.append(float((dist > ref.VOXEL).mean()))
        verts.append(len(v))
        if cond is None:
            assert "condition" not in report
        else:
            c = report["condition"]
            assert c["valid"] == int(R.valid(depth).sum()) and c["removed"] > 0 and c["smoothed"] == 0
            assert c["removed"] == int(R.condition(depth)[1][:, 1].sum())
    print("fusion: share of vertices farther than one voxel from the surface %.5f raw (%d vertices), %.5f conditioned (%d vertices)"
          % (share[0], verts[0], share[1], verts[1]))
    assert verts[0] > 1000 and verts[1] > 1000
    assert share[1] <= share[0] + 0.01
