"""CPU checks of the weights by viewing angle on the NumPy restatement (tests/depth_weights_ref.py): the
definition on planes whose cosine is known in float64, the gate, the special readings, the counts, the settings record, every
refusal of both entry points (no device is touched), the weighted integrate against fuse_ref's unweighted one, and what the
feature has to achieve on fuse_ref's sphere against the unweighted fusion of the same images."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import depth_condition_ref as DR  # noqa: E402
import depth_weights_ref as R  # noqa: E402
import fuse_ref as FR  # noqa: E402

F = np.float32
K4 = R.PLANE_K4
H, W = 48, 64


def flat(h=H, w=W, z=0.6):
    return np.full((1, h, w), z, F)


def interior(a, s):
    return a[..., s:a.shape[-2] - s, s:a.shape[-1] - s]


@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_a_fronto_parallel_plane_gives_the_full_weight_but_for_a_border_of_step_pixels(s):
    """Within 14 degrees of the optical axis (here: 12.4 at the corners) the cosine between ray and normal rounds to L = 16."""
    w, counts = R.weights(flat(), K4, step=s)
    assert w.dtype == np.uint8 and w.shape == (1, H, W)
    assert (interior(w, s) == 16).all()
    border = np.ones((H, W), bool)
    border[s:H - s, s:W - s] = False
    assert (w[0][border] == 0).all()
    assert counts.tolist() == [[H * W, int(border.sum()), (H - 2 * s) * (W - 2 * s)]]
    w05, _ = R.weights(flat(), (K4[0], K4[1], K4[2] + 0.5, K4[3] + 0.5), pixel_offset=0.5, step=s)    # the same rays
    assert np.array_equal(w05, w)
    far = R.weights(flat(), K4, pixel_offset=20.0, step=s)[0]                                          # 22 to 24 degrees at the far corner
    assert far[0, H - s - 1, W - s - 1] == 15 and far[0, s, s] == 16


@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("degrees", [30, 60, 75, -60])
def test_a_tilted_plane_gives_the_level_of_the_cosine_between_ray_and_normal(degrees, axis):
    """The level floor(cos * L + 0.5) of the float64 cosine per pixel; a pixel whose cos * L + 0.5 lies within 1e-3 of an integer
    may take either neighbour.  jump = 10 opens the gate: at 75 degrees the plane's depth changes by 15 mm a pixel and more."""
    depth, cos = R.tilted_plane(H, W, degrees, axis)
    assert (depth > 0.05).all() and (depth < 10).all()
    for s, L in ((1, 16), (2, 16), (4, 255), (1, 1)):
        w, _ = R.weights(depth, K4, step=s, jump=10.0, levels=L, cos_min=0.0)
        lo, hi = R.expected_levels(cos, L)
        got = interior(w[0], s).astype(np.int64)
        ok = (got == interior(lo, s)) | (got == interior(hi, s))
        assert ok.all(), (s, L, int((~ok).sum()))
    assert len(np.unique(R.weights(depth, K4, jump=10.0, cos_min=0.0)[0])) >= 3        # graded, not one level


def test_cos_min_at_a_level_boundary():
    """cos_min = 8.5 / 16, exact in float32: c >= cos_min exactly when c * 16 + 0.5 >= 9, so every level up to 8 becomes 0 and
    every level from 9 stays."""
    depth, _ = R.tilted_plane(H, W, 60, "y")
    w0, _ = R.weights(depth, K4, jump=0.1, cos_min=0.0)
    assert (w0 <= 8).sum() > 50 and (w0 >= 9).sum() > 50 and (interior(w0, 1) >= 1).all()
    w1, counts = R.weights(depth, K4, jump=0.1, cos_min=8.5 / 16)
    assert np.array_equal(w1, np.where(w0 >= 9, w0, 0))
    assert counts[0, 1] == (w1 == 0).sum()
    below = np.nextafter(F(8.5 / 16), F(0))
    assert np.array_equal(R.weights(depth, K4, jump=0.1, cos_min=below)[0], w1)       # no float32 lies between


@pytest.mark.parametrize("s", [1, 2, 4])
def test_a_depth_step_larger_than_the_gate_gives_a_band_of_zeros_on_both_sides(s):
    d = flat()
    d[0, :, 32:] = F(0.6 + 0.0101)
    w, _ = R.weights(d, K4, step=s)
    inner = w[0, s:H - s]
    assert (inner[:, 32 - s:32 + s] == 0).all()
    assert (inner[:, s:32 - s] == 16).all() and (inner[:, 32 + s:W - s] == 16).all()
    d[0, :, 32:] = F(0.6 + 0.0099)                                                    # inside the gate: nothing is dropped
    assert (interior(R.weights(d, K4, step=s)[0], s) > 0).all()
    rows = flat()
    rows[0, 20:] = F(0.6 + 0.0101)                                                    # and along the other axis
    assert (R.weights(rows, K4, step=s)[0][0, 20 - s:20 + s, s:W - s] == 0).all()


def test_jump_rel_widens_the_gate_with_the_centres_reading():
    d = flat(z=1.0)
    d[0, :, 32:] = F(1.02)
    assert (R.weights(d, K4)[0][0, 1:-1, 31:33] == 0).all()
    w = R.weights(d, K4, jump_rel=0.0099)[0]                                          # tol is the CENTRE's: 0.0199 at 1.0, 0.020098 at 1.02
    assert (w[0, 1:-1, 31] == 0).all() and (w[0, 1:-1, 32] > 0).all()
    w = R.weights(d, K4, jump_rel=0.011)[0]                                           # 0.01 + 0.011 z > 0.02
    assert (interior(w, 1) > 0).all()
    d[0, :, 32:] = F(1.0201)                                                          # 0.020099 at 1.0201: outside on both sides
    w = R.weights(d, K4, jump_rel=0.0099)[0]
    assert (w[0, 1:-1, 31] == 0).all() and (w[0, 1:-1, 32] == 0).all()


@pytest.mark.parametrize("special", DR.SPECIALS)
def test_special_readings_as_pixels_and_as_neighbours(special):
    """NaN, the infinities, a negative, both zeros: no reading, weight 0, and 0 for the four pixels that need it.  The denormal
    is a valid reading (it counts) far from every neighbour: the same weights."""
    for s in (1, 3):
        d = flat()
        d[0, 20, 30] = special
        w, counts = R.weights(d, K4, step=s)
        zero = np.zeros((H, W), bool)
        zero[:s], zero[-s:], zero[:, :s], zero[:, -s:] = True, True, True, True
        for dy, dx in ((0, 0), (0, s), (0, -s), (s, 0), (-s, 0)):
            zero[20 + dy, 30 + dx] = True
        assert np.array_equal(w[0] == 0, zero) and (w[0][~zero] == 16).all()
        valid = H * W - (0 if special == F(1e-40) and special > 0 else 1)
        assert counts.tolist() == [[valid, int(zero.sum()) - (H * W - valid), int((~zero).sum())]]


def test_tiny_images_have_no_pixel_with_four_neighbours():
    for h, w in ((1, 1), (2, 2), (1, 200), (200, 1), (2, 9)):
        got, counts = R.weights(flat(h, w), K4)
        assert not got.any() and counts.tolist() == [[h * w, h * w, 0]]
    got, counts = R.weights(flat(3, 3), K4)
    assert got[0].tolist() == [[0, 0, 0], [0, 16, 0], [0, 0, 0]] and counts.tolist() == [[9, 8, 1]]
    assert not R.weights(flat(8, 8), K4, step=4)[0].any() and R.weights(flat(9, 9), K4, step=4)[0][0, 4, 4] == 16


def test_one_level_and_255_levels_and_the_counts_of_a_batch():
    depth, cos = R.tilted_plane(H, W, 60, "x")
    one, c1 = R.weights(depth, K4, jump=0.1, levels=1)
    assert set(np.unique(one)) == {0, 1} and c1[0, 2] == (one == 1).sum()
    many, c255 = R.weights(depth, K4, jump=0.1, levels=255)
    assert many.max() <= 255 and len(np.unique(many)) > 20
    assert np.array_equal(many == 0, one == 0)                                         # the levels do not decide who is dropped
    imgs = DR.lattice_images(11, 3, 33, 70, dead=1)
    w, counts = R.weights(imgs, K4)
    v = DR.valid(imgs)
    assert counts[:, 0].tolist() == v.sum((1, 2)).tolist() and counts[1].tolist() == [0, 0, 0]
    assert counts[:, 1].tolist() == (v & (w == 0)).sum((1, 2)).tolist() and counts[:, 2].tolist() == (w == 16).sum((1, 2)).tolist()
    assert not w[~v].any() and 0 < counts[0, 1] < counts[0, 0]
    for i in range(3):                                                                 # a batch is its images
        wi, ci = R.weights(imgs[i], K4)
        assert np.array_equal(wi[0], w[i]) and ci[0].tolist() == counts[i].tolist()


def test_the_settings_record_and_its_refusals():
    from cppf2_amd import depthweights as DW
    assert DW.checked() == DW.Settings(1, 0.01, 0.0, 16, 0.2, 1)
    assert DW.checked(step=4, levels=255, cos_min=0.0, carve_weight=0, jump=0, jump_rel=0.5) == DW.Settings(4, 0.0, 0.5, 255, 0.0, 0)
    for kw in (dict(step=0), dict(step=5), dict(step=1.5), dict(step="a"), dict(levels=0), dict(levels=256), dict(levels=None),
               dict(cos_min=1.0), dict(cos_min=-0.1), dict(cos_min=float("nan")), dict(jump=-1), dict(jump=float("inf")),
               dict(jump_rel=float("nan")), dict(jump_rel=-0.1), dict(carve_weight=-1), dict(carve_weight=256), dict(carve_weight=0.5)):
        with pytest.raises(ValueError):
            DW.checked(**kw)
    assert DW.from_flags(False, {}) is None and DW.from_flags(False, dict(weight_step=None)) is None
    assert DW.from_flags(True, {}) == DW.checked()
    assert DW.from_flags(True, dict(weight_step=2, weight_levels=8, weight_cos_min=0.3, weight_jump=0.02, weight_jump_rel=0.01,
                                    carve_weight=3)) == DW.Settings(2, 0.02, 0.01, 8, 0.3, 3)
    for flag in DW.FLAGS:
        with pytest.raises(ValueError, match="--" + flag.replace("_", "-") + " .* --weight-views"):
            DW.from_flags(False, {flag: 1})
    with pytest.raises(ValueError, match="levels"):
        DW.from_flags(True, dict(weight_levels=300))
    s = DW.summary(DW.checked(), np.array([[5, 2, 1], [7, 0, 3]]))
    assert (s["valid"], s["zero"], s["full"], s["levels"], s["carve_weight"]) == (12, 2, 4, 16, 1)
    assert DW.merged([s, s])["valid"] == 24 and s["valid"] == 12
    assert DW.apply(None, None, None) == (None, None)
    with pytest.raises(ValueError, match="Settings"):
        DW.apply(np.zeros((1, 2, 2), F), np.eye(3), (1, 0.01, 0.0, 16, 0.2, 1))


def test_fuse_main_refuses_a_sub_flag_without_the_switch(capsys):
    from cppf2_amd import fuse
    for extra in (["--weight-levels", "8"], ["--carve-weight", "2"], ["--weight-views", "--weight-step", "9"]):
        with pytest.raises(SystemExit):
            fuse.main(["--views", "nowhere", "--voxel", "0.004", "--out", "x.ply"] + extra)
        assert "weight" in capsys.readouterr().err


def test_every_refusal_of_cppf_depth_weights_before_any_pointer_is_followed():
    from cppf2_amd import _lib
    L = _lib.load()
    K = (C.c_double * 4)(150.0, 150.0, 8.0, 8.0)
    one = 1 << 20
    base = dict(depth=C.c_void_p(one), I=2, H=16, W=16, K=K, po=0.0, step=1, jump=0.01, rel=0.0, levels=16, cos_min=0.2,
                out=C.c_void_p(1 << 24), counts=C.c_void_p(1 << 28))

    def call(**kw):
        a = dict(base, **kw)
        return L.cppf_depth_weights(a["depth"], a["I"], a["H"], a["W"], a["K"], C.c_float(a["po"]), a["step"], C.c_float(a["jump"]),
                                    C.c_float(a["rel"]), a["levels"], C.c_float(a["cos_min"]), a["out"], a["counts"], None)
    nan, inf = float("nan"), float("inf")
    cases = [dict(I=-1), dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(step=0), dict(step=5), dict(step=-1), dict(levels=0),
             dict(levels=256), dict(cos_min=1.0), dict(cos_min=-0.5), dict(cos_min=nan), dict(jump=-1.0), dict(jump=nan), dict(jump=inf),
             dict(rel=-1.0), dict(rel=nan), dict(rel=inf), dict(po=nan), dict(po=inf), dict(K=None), dict(depth=None), dict(out=None),
             dict(counts=None), dict(out=C.c_void_p(one)), dict(out=C.c_void_p(one + 2 * 16 * 16 * 4 - 1)),
             dict(out=C.c_void_p(one - 2 * 16 * 16 + 1))]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert b"cppf_depth_weights" in L.cppf_last_error_string()
    assert call(I=0) == 0 and call(I=0, depth=None, out=None, counts=None) == 0
    assert call(I=0, step=0) == -1 and call(I=0, K=None) == -1


def test_every_refusal_of_cppf_tsdf_integrate_weighted_before_any_pointer_is_followed():
    from cppf2_amd import _lib
    L = _lib.load()
    K = (C.c_double * 4)(150.0, 150.0, 8.0, 8.0)
    origin = (C.c_double * 3)(0.0, 0.0, 0.0)
    p = [C.c_void_p(k << 20) for k in range(1, 7)]
    base = dict(V=2, depth=p[0], masks=p[1], poses=p[2], weights=p[3], carve=1, H=16, W=16, K=K, po=0.0, origin=origin, voxel=0.004,
                dims=(4, 4, 4), trunc=0.012, znear=0.05, acc=p[4], wsum=p[5])

    def call(**kw):
        a = dict(base, **kw)
        return L.cppf_tsdf_integrate_weighted(a["V"], a["depth"], a["masks"], a["poses"], a["weights"], a["carve"], a["H"], a["W"], a["K"],
                                              C.c_float(a["po"]), a["origin"], C.c_float(a["voxel"]), *a["dims"], C.c_float(a["trunc"]),
                                              C.c_float(a["znear"]), a["acc"], a["wsum"], None)
    nan = float("nan")
    cases = [dict(weights=None), dict(carve=-1), dict(carve=256), dict(V=-1), dict(V=65537), dict(depth=None), dict(poses=None),
             dict(acc=None), dict(wsum=None), dict(K=None), dict(origin=None), dict(H=0), dict(W=16385), dict(voxel=0.0), dict(voxel=nan),
             dict(trunc=-1.0), dict(znear=0.0), dict(po=nan), dict(dims=(0, 4, 4)), dict(dims=(1 << 14, 1 << 14, 1))]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert b"cppf_tsdf_integrate_weighted" in L.cppf_last_error_string()
    assert call(V=0) == 0 and call(V=0, depth=None, poses=None, weights=None, masks=None) == 0
    assert call(V=0, carve=256) == -1 and call(V=0, acc=None) == -1


# ----------------------------------------------------------------------------------------------
# the weighted integrate
# ----------------------------------------------------------------------------------------------
def small_views(n=4, h=24, w=32):
    """n views of fuse_ref's sphere at h x w (the camera scaled with the image), a wall behind it."""
    k = w / FR.W
    K4s = tuple(v * k for v in FR.K4)
    depth, masks, poses = FR.sphere_views(FR.fibonacci(n), wall=1.6, K4=K4s, H=h, W=w)
    return depth, masks, poses, K4s


def test_weights_of_one_give_the_unweighted_restatement_bit_for_bit():
    depth, masks, poses, K4s = small_views()
    origin, dims, trunc = FR.sphere_volume(voxel=0.008)
    rng = np.random.RandomState(0)
    acc0, wsum0 = rng.randn(*dims).astype(F), rng.randint(0, 5, dims).astype(np.int32)
    ones = np.ones(depth.shape, np.uint8)
    for m in (masks, None):
        for po in (0.0, 0.5):
            want = FR.integrate(acc0, wsum0, depth, m, poses, K4s, po, origin, 0.008, trunc, 0.05)
            got = R.integrate(acc0, wsum0, depth, m, poses, ones, 1, K4s, po, origin, 0.008, trunc, 0.05)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
            assert (want[1] > wsum0).any()


def test_the_weighted_restatement_weighs_skips_and_splits():
    depth, masks, poses, K4s = small_views()
    origin, dims, trunc = FR.sphere_volume(voxel=0.008)
    z, zi = np.zeros(dims, F), np.zeros(dims, np.int32)
    args = (K4s, 0.0, origin, 0.008, trunc, 0.05)
    w = np.random.RandomState(1).randint(0, 6, depth.shape).astype(np.uint8) * (np.random.RandomState(2).rand(*depth.shape) > 0.2)
    w = w.astype(np.uint8)
    whole = R.integrate(z, zi, depth, masks, poses, w, 7, *args)
    part = R.integrate(z, zi, depth[:1], masks[:1], poses[:1], w[:1], 7, *args)
    part = R.integrate(*part, depth[1:], masks[1:], poses[1:], w[1:], 7, *args)
    assert whole[0].tobytes() == part[0].tobytes() and whole[1].tobytes() == part[1].tobytes()
    unw = FR.integrate(z, zi, depth, masks, poses, *args)
    assert ((whole[1] == 0) | (unw[1] > 0)).all() and whole[1].max() > unw[1].max()
    nothing = R.integrate(z, zi, depth, masks, poses, np.zeros_like(w), 0, *args)
    assert not nothing[0].any() and not nothing[1].any()
    # carve_weight 0: only observations of the surface itself (q < 1 inside the mask) are left
    surf = R.integrate(z, zi, depth, masks, poses, np.full_like(w, 3), 0, *args)
    both = R.integrate(z, zi, depth, masks, poses, np.full_like(w, 3), 5, *args)
    assert (surf[1] % 3 == 0).all() and (surf[1] <= both[1]).all() and (both[1] > surf[1]).any()
    k = surf[1] > 0
    assert (surf[0][k] / surf[1][k] < 1).all()
    # twice the weights: twice the sums (exact: a power of two), the same mean
    dbl = R.integrate(z, zi, depth, masks, poses, (2 * np.minimum(w, 100)).astype(np.uint8), 14, *args)
    assert np.array_equal(dbl[1], 2 * whole[1]) and np.array_equal(dbl[0], 2 * whole[0])


# ----------------------------------------------------------------------------------------------
# what the feature has to achieve: against the unweighted fusion of the same images, on the same volume
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("kind", ["wall", "table"])
def test_the_weighted_mesh_lies_closer_to_the_sphere_than_the_unweighted_one(kind, noisy):
    """fuse_ref's sphere, 24 Fibonacci views of 160 x 120, voxel 4 mm, trunc 3 voxels; the defaults (step 1, 16 levels, cos_min
    0.2, carve_weight 1).  RMS distance of the mesh's vertices to the sphere at most 0.5 x the unweighted one with exact depth
    and 0.7 x with the axial noise of Nguyen et al. 2012 on the masked pixels; the largest distance no larger; at most 0.2 of
    the masked pixels dropped; closed where the unweighted mesh is; the triangle count within 5 per cent.  Measured on this
    restatement (RMS / max in mm, unweighted -> weighted): wall 0.699 / 2.295 -> 0.233 / 0.866 (ratio 0.334), wall noisy
    0.853 / 2.730 -> 0.393 / 1.372 (0.461), table 0.508 / 1.961 -> 0.190 / 0.758 (0.373), table noisy 0.675 / 2.648 ->
    0.363 / 1.248 (0.538); dropped 0.107, 0.146, 0.104, 0.144 of the masked pixels."""
    sc = R.sphere_scene(kind, noisy)
    origin, dims, trunc = FR.sphere_volume()
    w, _ = R.weights(sc["depth"], FR.K4)
    z, zi = np.zeros(dims, F), np.zeros(dims, np.int32)
    unweighted = FR.fuse(sc["depth"], sc["masks"], sc["poses"], origin, dims, FR.VOXEL, trunc)
    weighted = R.integrate(z, zi, sc["depth"], sc["masks"], sc["poses"], w, 1, FR.K4, 0.0, origin, FR.VOXEL, trunc, 0.05)
    R.check_scene(R.mesh_figures(*unweighted, origin), R.mesh_figures(*weighted, origin),
                  R.masked_zero_share(w, sc["masks"], sc["depth"]), noisy)
