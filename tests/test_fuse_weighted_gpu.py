"""GPU checks of the weighted fusion: cppf_tsdf_integrate_weighted byte-equal to the NumPy restatement
(tests/depth_weights_ref.py) on small, flat and several-block volumes, its call hygiene, weights of one against
cppf_tsdf_integrate's bytes; then end to end -- fuse.fuse_views(weighting=) and python -m cppf2_amd.fuse --weight-views on
fuse_ref's sphere, held to the bounds against the UNWEIGHTED fusion of the same images, and the tracked and joined paths
against the same loop on the restatement."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import depth_weights_ref as R  # noqa: E402
import fuse_ref as FR  # noqa: E402
import relocalise_ref as RR  # noqa: E402
import track_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
H, W = 24, 32
K4S = tuple(v * W / FR.W for v in FR.K4)
ZNEAR = 0.05
# (dims, origin, voxel): each straddles the sphere's surface (radius 50 mm about (3, -2, 4) mm); the last takes several blocks
VOLUMES = [((2, 2, 2), (0.046, -0.006, 0.0), 0.008), ((5, 1, 7), (0.03, 0.001, -0.02), 0.008),
           ((33, 17, 9), (-0.0637, -0.0337, -0.0137), 0.004)]


def views(n):
    depth, masks, poses = FR.sphere_views(FR.fibonacci(n), wall=1.6, K4=K4S, H=H, W=W)
    rng = np.random.RandomState(n)
    w = (rng.randint(1, 256, depth.shape) * (rng.rand(*depth.shape) > 0.25)).astype(np.uint8)
    w[rng.rand(*depth.shape) < 0.3] = 1
    return depth, masks, poses, w


def start(dims, seed=0):
    rng = np.random.RandomState(seed)
    return rng.randn(*dims).astype(F), rng.randint(0, 4, dims).astype(np.int32)


def dev_integrate(acc, wsum, depth, masks, poses, w, carve, po, origin, voxel, trunc, weighted=True, K4=K4S):
    """The entry point itself on host arrays: new (acc, wsum)."""
    import torch
    from cppf2_amd import _lib, ops
    dev, L = ops._dev(), _lib.load()

    def up(x, dt):
        return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    a, s = up(acc, F), up(wsum, np.int32)
    d, m, P, wt = up(depth, F), up(masks, np.uint8), up(np.asarray(poses).reshape(-1, 12), F), up(w, np.uint8)
    V = len(depth)
    grid = (H, W, (C.c_double * 4)(*K4), C.c_float(po), (C.c_double * 3)(*[float(v) for v in origin]), C.c_float(voxel), *acc.shape,
            C.c_float(trunc), C.c_float(ZNEAR), ops._p(a), ops._p(s), ops._stream())
    if weighted:
        _lib.check(L.cppf_tsdf_integrate_weighted(V, ops._p(d), ops._p(m), ops._p(P), ops._p(wt), carve, *grid), "cppf_tsdf_integrate_weighted")
    else:
        _lib.check(L.cppf_tsdf_integrate(V, ops._p(d), ops._p(m), ops._p(P), *grid), "cppf_tsdf_integrate")
    return a.cpu().numpy(), s.cpu().numpy()


def same(got, want):
    return got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("dims,origin,voxel", VOLUMES)
def test_acc_and_wsum_equal_the_restatement_byte_for_byte(dims, origin, voxel):
    trunc = float(F(3 * voxel))
    touched = 0
    for n in (3, 5):
        depth, masks, poses, w = views(n)
        acc0, wsum0 = start(dims, n)
        for m in (masks, None):
            for carve in (0, 1, 7):
                for po in (0.0, 0.5):
                    want = R.integrate(acc0, wsum0, depth, m, poses, w, carve, K4S, po, origin, voxel, trunc, ZNEAR)
                    got = dev_integrate(acc0, wsum0, depth, m, poses, w, carve, po, origin, voxel, trunc)
                    assert same(got, want), (n, m is None, carve, po, int((got[1] != want[1]).sum()))
                    touched += int((want[1] != wsum0).sum())
        # one call equals any split into consecutive calls
        part = dev_integrate(acc0, wsum0, depth[:1], masks[:1], poses[:1], w[:1], 7, 0.0, origin, voxel, trunc)
        part = dev_integrate(*part, depth[1:], masks[1:], poses[1:], w[1:], 7, 0.0, origin, voxel, trunc)
        assert same(part, R.integrate(acc0, wsum0, depth, masks, poses, w, 7, K4S, 0.0, origin, voxel, trunc, ZNEAR))
        # weights of one and carve_weight 1 are cppf_tsdf_integrate, byte for byte
        ones = np.ones_like(w)
        for m in (masks, None):
            plain = dev_integrate(acc0, wsum0, depth, m, poses, None, 0, 0.0, origin, voxel, trunc, weighted=False)
            assert same(plain, FR.integrate(acc0, wsum0, depth, m, poses, K4S, 0.0, origin, voxel, trunc, ZNEAR))
            assert same(dev_integrate(acc0, wsum0, depth, m, poses, ones, 1, 0.0, origin, voxel, trunc), plain)
    assert touched > 0


def test_no_views_is_valid_and_refusals_write_nothing():
    import torch
    from cppf2_amd import _lib, ops
    dev, L = ops._dev(), _lib.load()
    depth, masks, poses, w = views(3)
    dims, origin, voxel = VOLUMES[1]
    acc0, wsum0 = start(dims)
    a, s = torch.from_numpy(acc0).to(dev), torch.from_numpy(wsum0).to(dev)
    d, m, P, wt = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (depth, masks, poses.reshape(-1, 12), w))
    K, o = (C.c_double * 4)(*K4S), (C.c_double * 3)(*origin)
    nan = float("nan")

    def call(V=3, depth=d, masks=m, poses=P, weights=wt, carve=1, H=H, W=W, K=K, po=0.0, origin=o, voxel=voxel, dims=dims, trunc=0.024,
             znear=ZNEAR, acc=a, wsum=s):
        return L.cppf_tsdf_integrate_weighted(V, ops._p(depth), ops._p(masks), ops._p(poses), ops._p(weights), carve, H, W, K,
                                              C.c_float(po), origin, C.c_float(voxel), *dims, C.c_float(trunc), C.c_float(znear),
                                              ops._p(acc), ops._p(wsum), ops._stream())
    assert call(V=0) == 0 and call(V=0, depth=None, masks=None, poses=None, weights=None) == 0
    for kw in (dict(weights=None), dict(carve=-1), dict(carve=256), dict(V=-1), dict(V=65537), dict(depth=None), dict(poses=None),
               dict(acc=None), dict(wsum=None), dict(K=None), dict(origin=None), dict(H=0), dict(W=16385), dict(voxel=0.0),
               dict(voxel=nan), dict(trunc=0.0), dict(znear=-1.0), dict(po=nan), dict(dims=(0, 1, 7)), dict(dims=(5, 1, -1))):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == acc0.tobytes() and s.cpu().numpy().tobytes() == wsum0.tobytes()
    assert call() == 0
    want = R.integrate(acc0, wsum0, depth, masks, poses, w, 1, K4S, 0.0, origin, voxel, 0.024, ZNEAR)
    assert same((a.cpu().numpy(), s.cpu().numpy()), want)


def test_the_wrapper_takes_weights_and_refuses_a_wrong_shape():
    from cppf2_amd import fuse
    depth, masks, poses, w = views(4)
    dims, origin, voxel = VOLUMES[2]
    K = np.array([[K4S[0], 0, K4S[2]], [0, K4S[1], K4S[3]], [0, 0, 1.0]])
    z, zi = np.zeros(dims, F), np.zeros(dims, np.int32)
    vol = fuse.Volume(origin, voxel, dims)
    fuse.integrate(vol, depth[:2], poses[:2], K, masks[:2], weights=w[:2], carve_weight=7)
    fuse.integrate(vol, depth[2:], poses[2:], K, masks=None, pixel_offset=0.5, weights=w[2:], carve_weight=0)
    want = R.integrate(z, zi, depth[:2], masks[:2], poses[:2], w[:2], 7, K4S, 0.0, vol.origin, vol.voxel, vol.trunc, ZNEAR)
    want = R.integrate(*want, depth[2:], None, poses[2:], w[2:], 0, K4S, 0.5, vol.origin, vol.voxel, vol.trunc, ZNEAR)
    assert same((vol.acc.cpu().numpy(), vol.wsum.cpu().numpy()), want) and vol.views == 4
    plain, also = fuse.Volume(origin, voxel, dims), fuse.Volume(origin, voxel, dims)
    fuse.integrate(plain, depth, poses, K, masks)
    fuse.integrate(also, depth, poses, K, masks, weights=np.ones_like(w))
    assert same((plain.acc.cpu().numpy(), plain.wsum.cpu().numpy()), (also.acc.cpu().numpy(), also.wsum.cpu().numpy()))
    for bad in (dict(weights=w[:3]), dict(weights=w[:, :-1]), dict(weights=w, carve_weight=256), dict(weights=w, carve_weight=-1)):
        with pytest.raises(ValueError):
            fuse.integrate(vol, depth, poses, K, masks, **bad)


# ----------------------------------------------------------------------------------------------
# end to end: what the feature has to achieve, against the unweighted fusion of the same images on the same volume
# ----------------------------------------------------------------------------------------------
K3 = np.array([[FR.K4[0], 0.0, FR.K4[2]], [0.0, FR.K4[1], FR.K4[3]], [0.0, 0.0, 1.0]])


def mesh_figures(mesh):
    return R.figures_of(mesh.verts, mesh.faces, mesh.boundary_edges)


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("kind", ["wall", "table"])
def test_fuse_views_with_weighting_lies_closer_to_the_sphere_than_without(kind, noisy):
    """fuse_ref.sphere_views(fibonacci(24)) at 160 x 120, voxel 4 mm, through fuse.fuse_views with and without
    weighting=depthweights.checked() -- the same images, the same volume (fuse_ref.sphere_volume, the CPU test's; with the
    noise, Volume.around would follow the rim's outliers) --: the bounds of tests/test_depth_weights.py on the device's
    weights, volume and mesh.  The device's weights are the restatement's integers and its volume the restatement's bytes,
    so the figures are those of the CPU test."""
    from cppf2_amd import depthweights as DW, fuse
    sc = R.sphere_scene(kind, noisy)
    depth, masks, poses = sc["depth"].copy(), sc["masks"].copy(), sc["poses"].copy()
    origin, dims, trunc = FR.sphere_volume()
    s = DW.checked()
    plain, rep0 = fuse.fuse_views(depth, masks, poses, K3, FR.VOXEL, volume=fuse.Volume(origin, FR.VOXEL, dims, trunc))
    vol = fuse.Volume(origin, FR.VOXEL, dims, trunc)
    mesh, rep = fuse.fuse_views(depth, masks, poses, K3, FR.VOXEL, volume=vol, weighting=s)
    assert "weighting" not in rep0 and rep["dims"] == rep0["dims"] == list(dims) and rep["views"] == 24
    want_w, want_counts = R.weights(depth, FR.K4)
    assert rep["weighting"] == DW.summary(s, want_counts)
    w, _ = DW.weights(depth, K3)
    assert np.array_equal(w.cpu().numpy(), want_w)
    R.check_scene(mesh_figures(plain), mesh_figures(mesh), R.masked_zero_share(want_w, masks, depth), noisy)
    z = np.zeros(dims, F)
    want = R.integrate(z, z.astype(np.int32), depth, masks, poses, want_w, 1, FR.K4, 0.0, origin, FR.VOXEL, trunc, ZNEAR)
    assert same((vol.acc.cpu().numpy(), vol.wsum.cpu().numpy()), want)
    around, _ = fuse.fuse_views(depth, masks, poses, K3, FR.VOXEL, weighting=s)           # and on Volume.around: closed, as close
    fig = mesh_figures(around)
    print("Volume.around:", fig)
    assert fig["boundary_edges"] == 0 and fig["max"] <= 2 * FR.VOXEL


def write_scene(folder, depth, masks, poses, K4=FR.K4, scale=0.1):
    """A BOP-format scene folder of one object (id 1): depth in units of `scale` mm as 16-bit PNGs."""
    from PIL import Image
    os.makedirs(os.path.join(folder, "depth"))
    os.makedirs(os.path.join(folder, "mask_visib"))
    gt, cam = {}, {}
    Kl = [K4[0], 0.0, K4[2], 0.0, K4[1], K4[3], 0.0, 0.0, 1.0]
    for i, (d, m, P) in enumerate(zip(depth, masks, np.asarray(poses, dtype=np.float64).reshape(-1, 3, 4))):
        Image.fromarray(np.round(d.astype(np.float64) * 1000.0 / scale).astype(np.uint16)).save(os.path.join(folder, "depth", "%06d.png" % i))
        Image.fromarray((m != 0).astype(np.uint8) * 255).save(os.path.join(folder, "mask_visib", "%06d_%06d.png" % (i, 0)))
        gt[str(i)] = [dict(obj_id=1, cam_R_m2c=P[:, :3].reshape(-1).tolist(), cam_t_m2c=(P[:, 3] * 1000.0).tolist())]
        cam[str(i)] = dict(cam_K=Kl, depth_scale=scale)
    json.dump(gt, open(os.path.join(folder, "scene_gt.json"), "w"))
    json.dump(cam, open(os.path.join(folder, "scene_camera.json"), "w"))


def test_command_line_weights_the_views_of_a_written_scene_folder(tmp_path):
    """12 of the wall scene's views written as a scene folder (depth quantised to 0.1 mm) through python -m cppf2_amd.fuse with
    and without --weight-views: the report's `weighting` holds the settings and the restatement's counts of the images as read,
    the weighted mesh lies closer to the sphere, and the flags compose with --condition-depth, --close and --simplify-cell."""
    from cppf2_amd import depthweights as DW, fuse, render
    sc = R.sphere_scene("wall", False)
    folder = str(tmp_path / "000000")
    write_scene(folder, sc["depth"][::2], sc["masks"][::2], sc["poses"][::2])
    out, rep_path = str(tmp_path / "obj.ply"), str(tmp_path / "report.json")
    args = ["--views", folder, "--voxel", str(FR.VOXEL), "--out", out]
    plain = fuse.main(args)
    d0 = render.load_mesh(out, 0.001).verts
    report = fuse.main(args + ["--weight-views", "--weight-levels", "8", "--carve-weight", "2", "--report", rep_path])
    assert "weighting" not in plain and json.load(open(rep_path))["weighting"] == report["weighting"]
    read = fuse.read_views(folder)[0]
    s = DW.checked(levels=8, carve_weight=2)
    assert report["weighting"] == DW.summary(s, R.weights(read["depths"], FR.K4, levels=8)[1])
    d1 = render.load_mesh(out, 0.001).verts

    def rms(v):
        return float(np.sqrt(np.mean(FR.sphere_distance(v) ** 2)))
    print("command line, 12 views, 8 levels: RMS %.3f mm unweighted, %.3f mm weighted" % (1000 * rms(d0), 1000 * rms(d1)))
    assert rms(d1) < rms(d0) and report["triangles"] > 1000
    every = fuse.main(args + ["--weight-views", "--weight-step", "2", "--weight-cos-min", "0.3", "--weight-jump", "0.02",
                              "--weight-jump-rel", "0.01", "--condition-depth", "--close", "--simplify-cell", "0.008", "--min-weight", "8"])
    assert every["weighting"]["step"] == 2 and every["weighting"]["levels"] == 16 and "condition" in every and "close" in every
    assert "simplify" in every and every["weighting"]["valid"] <= report["weighting"]["valid"]
    with pytest.raises(SystemExit):
        fuse.main(args + ["--weight-levels", "8"])


# ----------------------------------------------------------------------------------------------
# the tracked and the joined path: the same loop on the restatement
# ----------------------------------------------------------------------------------------------
def test_onboard_with_weighting_equals_the_restatement_on_the_orbit():
    """tests/test_track_gpu.py's 36-frame orbit, first pose only, no sweep, weighting on: the device's poses within 1e-7 of the
    loop on the restatement (weights, weighted integrate and tracker restated), the same inliers and lost frames, the same
    counts; then one sweep, whose volume is integrated with the same weights."""
    from cppf2_amd import depthweights as DW, track
    depth, masks, poses = T.box_views(T.orbit_dirs(36))
    s = DW.checked()
    _, want, wrep = track.onboard(depth, masks, T.K3, poses[0], T.VOXEL, extent=0.13, sweeps=0, dev="cpu", track_fn=T.ref_track,
                                  integrate_fn=R.ref_integrate, weighting=s, weights_fn=R.ref_apply)
    vol, got, rep = track.onboard(depth, masks, T.K3, poses[0], T.VOXEL, extent=0.13, sweeps=0, weighting=s)
    print("weighted onboard: largest pose difference to the restatement %.3g; lost %d" % (np.abs(got - want).max(), rep["lost"]))
    assert np.abs(got - want).max() <= 1e-7
    assert [f["inliers"] for f in rep["frames"]] == [f["inliers"] for f in wrep["frames"]]
    assert [f["lost"] for f in rep["frames"]] == [f["lost"] for f in wrep["frames"]] and abs(rep["max_step"] - wrep["max_step"]) <= 1e-6
    assert rep["weighting"] == wrep["weighting"] and rep["weighting"]["levels"] == 16
    assert int(vol.wsum.max()) > 36                                                    # units of weight, not of views
    vol1, got1, rep1 = track.onboard(depth, masks, T.K3, poses[0], T.VOXEL, extent=0.13, sweeps=1, weighting=s)
    z = np.zeros(vol1.dims, F)
    w, _ = R.weights(depth, T.K4)
    want1 = R.integrate(z, z.astype(np.int32), depth, masks, got1, w, 1, T.K4, 0.0, vol1.origin, vol1.voxel, vol1.trunc, ZNEAR)
    assert same((vol1.acc.cpu().numpy(), vol1.wsum.cpu().numpy()), want1) and rep1["weighting"] == rep["weighting"]


def test_join_with_weighting_equals_the_frame_loop_on_the_restatement():
    """tests/test_relocalise_gpu.py's two sequences through track.join(weighting=), no sweep.  The exhaustive search is the
    device's (its restatement at this size takes minutes); from the pose it finds for frame 0 the frame loop runs again on the
    restatement -- the first sequence integrated with its restated weights, every later frame tracked and integrated with its
    own --, and the device's poses lie within 1e-7 of it; the report carries both sequences' counts."""
    import torch
    from cppf2_amd import depthweights as DW, fuse, track
    da, ma, pa = T.box_views(RR.dirs_a())
    db, mb, pb = T.box_views(RR.dirs_b())
    s = DW.checked()
    vol, poses, rep = track.join(dict(depths=da, masks=ma, K=T.K3, poses=pa), dict(depths=db, masks=mb, K=T.K3), T.VOXEL, reach=0.064,
                                 top=128, turned_over=True, weighting=s)
    wa, ca = R.weights(da, T.K4)
    wb, cb = R.weights(db, T.K4)
    assert rep["weighting"] == DW.summary(s, np.concatenate([ca, cb])) and vol.views == len(da) + len(db)
    host = fuse.Volume(vol.origin, vol.voxel, vol.dims, vol.trunc, "cpu")
    R.ref_integrate(host, da, pa, T.K3, ma, 0.0, ZNEAR, weights=wa, carve_weight=1)
    P = torch.zeros((len(db), 12), dtype=torch.float64)
    S = torch.zeros((len(db), 4), dtype=torch.float32)
    P[0] = torch.from_numpy(poses[0])
    kw = dict(iters=10, gate=None, stride=1, pixel_offset=0.0, min_weight=1)
    track._follow(host, torch.from_numpy(db), torch.from_numpy(mb), T.K3, P, S, kw, 0.0, ZNEAR, T.ref_track, R.ref_integrate, wb, s)
    diff = np.abs(P.numpy() - poses).max()
    rms = [T.surface_rms(db[i], mb[i], poses[i])[0] / T.VOXEL for i in range(len(db))]
    print("weighted join: largest pose difference to the restatement's frame loop %.3g; largest frame RMS %.3f voxel, lost %d"
          % (diff, max(rms), rep["lost"]))
    assert diff <= 1e-7
    assert [f["inliers"] for f in rep["frames"]][1:] == [int(x) for x in S.numpy()[1:, 0]]
