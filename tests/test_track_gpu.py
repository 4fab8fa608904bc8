"""GPU checks of depth-frame tracking: cppf_tsdf_track held to the NumPy restatement (tests/track_ref.py)
-- the inlier count exactly (the float32 part is stated bit for bit), the pose to 1e-9 after one iteration and 1e-7 after a
schedule, the stats to rtol 1e-6: tests/test_icp_gpu.py's tolerances for the same solve -- at every image size, stride, batch,
offset and mask form that takes another path, on constructed volumes whose cells sit at the definition's edges, through the
validation and workspace protocol, and then track.onboard and python -m cppf2_amd.fuse --track end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuse_ref as FR  # noqa: E402
import icp_depth_ref as DR  # noqa: E402
import track_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, "tests", "golden", "example_data", "obj_000015.ply")
VOXEL = T.VOXEL
CANARY = -7.25
EINVAL = -1


def _c(x, n):
    return (C.c_double * n)(*[float(v) for v in x])


def dev_track(depth, masks, K4, po, stride, poses, acc, wsum, origin, voxel, trunc, min_weight, dks):
    """cppf_tsdf_track itself on host arrays, the workspace exactly as large as asked for with canaries behind it and the stats
    filled with canaries: (poses float64 [B,12], stats float32 [B,4]) as the kernels left them."""
    import torch
    from cppf2_amd import _lib, ops
    dev, L = ops._dev(), _lib.load()
    d = torch.from_numpy(np.array(depth, dtype=np.float32)).to(dev)
    B, H, W = d.shape
    m = None if masks is None else torch.from_numpy(np.array(masks, dtype=np.uint8)).to(dev)
    a = torch.from_numpy(np.array(acc, dtype=np.float32)).to(dev)
    w = torch.from_numpy(np.array(wsum, dtype=np.int32)).to(dev)
    P = torch.from_numpy(np.array(poses, dtype=np.float64).reshape(-1, 12)).to(dev)
    st = torch.full((B, 4), CANARY, dtype=torch.float32, device=dev)
    need = L.cppf_tsdf_track_workspace_bytes(B, H, W, stride)
    assert need == B * ((H * W + 255) // 256) * 256
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=dev)
    dk = np.array(dks, dtype=np.float32)
    _lib.check(L.cppf_tsdf_track(B, ops._p(d), ops._p(m), H, W, _c(K4, 4), C.c_float(po), stride, ops._p(a), ops._p(w), _c(origin, 3),
                                 C.c_float(voxel), *a.shape, C.c_float(trunc), min_weight, len(dk), dk.ctypes.data_as(C.c_void_p),
                                 ops._p(P), ops._p(st), ops._p(ws), need, ops._stream()), "cppf_tsdf_track")
    assert bool((ws[need:] == 0x5A).all()), "the workspace's canaries"
    return P.cpu().numpy(), st.cpu().numpy()


def assert_tracks_equal(got, want, tol):
    (gp, gs), (wp, ws) = got, want
    assert gs[:, 0].tolist() == ws[:, 0].tolist(), "inliers"
    assert gs[:, 3].tolist() == ws[:, 3].tolist(), "iterations that moved the pose"
    np.testing.assert_allclose(gs, ws, rtol=1e-6, atol=0)
    assert np.abs(gp - wp).max() <= tol, np.abs(gp - wp).max()
    for b in range(len(wp)):
        if ws[b, 3] == 0:
            assert gp[b].tobytes() == wp[b].tobytes(), "a pose no iteration moved keeps its bytes"


@pytest.fixture(scope="module")
def box():
    """The box volume fused from 24 true poses by the restatement and five held-out frames 5 degrees and 10 mm off, the middle
    one emptied (all depth 0); the restatement's result of the 10-iteration schedule and of one iteration: computed once."""
    depth, masks, poses = T.box_views(FR.fibonacci(24))
    acc, wsum = FR.integrate(np.zeros(T.DIMS, np.float32), np.zeros(T.DIMS, np.int32), depth, masks, poses.astype(np.float32), T.K4, 0.0,
                             T.ORIGIN, VOXEL, T.TRUNC, T.ZNEAR)
    hd, hm, hp = T.box_views(FR.fibonacci(29)[[3, 9, 14, 20, 26]])
    hd[2] = 0
    start = np.stack([T.perturbed(hp[i], 5, 10, 40 + i) for i in range(5)])
    vol = (acc, wsum, T.ORIGIN, VOXEL, T.TRUNC, 1)
    dks = T.gates(10, T.TRUNC, VOXEL)
    return dict(vol=vol, depth=hd, masks=hm, start=start, dks=dks, ten=T.track_batch(hd, hm, T.K4, 0.0, 1, start, *vol, dks),
                one=T.track_batch(hd, hm, T.K4, 0.0, 1, start, *vol, dks[:1]))


def test_one_iteration_and_a_schedule_equal_the_restatement(box):
    """120 x 160 (75 blocks a frame), B = 5 with an empty frame in the middle: 1e-9 after one iteration, 1e-7 after ten; the
    empty frame keeps its pose's bytes and has stats 0."""
    one = dev_track(box["depth"], box["masks"], T.K4, 0.0, 1, box["start"], *box["vol"], box["dks"][:1])
    assert_tracks_equal(one, box["one"], 1e-9)
    ten = dev_track(box["depth"], box["masks"], T.K4, 0.0, 1, box["start"], *box["vol"], box["dks"])
    assert_tracks_equal(ten, box["ten"], 1e-7)
    assert box["ten"][1][[0, 1, 3, 4], 3].tolist() == [10.0] * 4 and box["ten"][1][[0, 1, 3, 4], 0].min() > 300
    for got in (one, ten):
        assert got[0][2].tobytes() == box["start"][2].tobytes() and not got[1][2].any()


@pytest.mark.parametrize("iters", [1, 10])
def test_batched_equals_separate_byte_for_byte(box, iters):
    dks = box["dks"][:iters]
    P, S = dev_track(box["depth"], box["masks"], T.K4, 0.0, 1, box["start"], *box["vol"], dks)
    for b in range(5):
        p, s = dev_track(box["depth"][b:b + 1], box["masks"][b:b + 1], T.K4, 0.0, 1, box["start"][b:b + 1], *box["vol"], dks)
        assert p.tobytes() == P[b:b + 1].tobytes() and s.tobytes() == S[b:b + 1].tobytes(), b
    p, s = dev_track(box["depth"][3:], box["masks"][3:], T.K4, 0.0, 1, box["start"][3:], *box["vol"], dks)          # B = 2
    assert p.tobytes() == P[3:].tobytes() and s.tobytes() == S[3:].tobytes()


def test_zero_iterations_and_zero_frames_launch_nothing(box):
    P, S = dev_track(box["depth"], box["masks"], T.K4, 0.0, 1, box["start"], *box["vol"], [])
    assert P.tobytes() == box["start"].tobytes() and bool((S == np.float32(CANARY)).all())
    from cppf2_amd import _lib
    acc, wsum = box["vol"][:2]
    assert _lib.load().cppf_tsdf_track_workspace_bytes(0, 120, 160, 1) == 0
    assert _lib.load().cppf_tsdf_track(0, None, None, 120, 160, _c(T.K4, 4), C.c_float(0), 1, 1, 1, _c(T.ORIGIN, 3), C.c_float(VOXEL),
                                       *acc.shape, C.c_float(T.TRUNC), 1, 0, None, None, None, None, 0, None) == 0


def small_views(H, W, po=0.0, n=2):
    """n views of the box in H x W images (the focal length shrunk with the image, the principal point at its centre), each
    started 2 degrees and 3 mm off.  Pixel (r, c) is rendered along the ray of (c + po, r + po): the convention po tracks by."""
    f = 2.0 * max(H, W)
    K4 = (f, f, (W - 1) / 2.0 + po, (H - 1) / 2.0 + po)
    K3 = np.array([[f, 0, K4[2] - po], [0, f, K4[3] - po], [0, 0, 1.0]])
    poses = FR.look_at(FR.fibonacci(29)[[3, 20][:n]], centre=np.zeros(3)).astype(np.float64)
    depth, masks = [], []
    for P in poses.reshape(-1, 3, 4):
        d, face = DR.render_box(P[:, :3], P[:, 3], K3, H, W)
        depth.append(d)
        masks.append(face >= 0)
    start = np.stack([T.perturbed(p, 2, 3, 7 + i) for i, p in enumerate(poses)])
    return np.asarray(depth, np.float32), np.asarray(masks).astype(np.uint8), start, K4


@pytest.mark.parametrize("H,W", [(16, 16), (17, 13), (1, 1), (23, 47)])
@pytest.mark.parametrize("stride,po,use_masks", [(1, 0.0, True), (2, 0.5, False), (3, 0.0, True), (1, 0.5, False)])
def test_image_sizes_strides_offsets_and_mask_forms(box, H, W, stride, po, use_masks):
    """One block (16 x 16), a ragged tail (17 x 13), one pixel, two blocks with a tail (23 x 47: 1 081 pixels); strides that do not
    divide the sizes; pixel_offset 0 and 0.5; masks given and NULL (the wall's pixels then pass the gate and fall outside the
    volume).  One iteration to 1e-9, three to 1e-7."""
    depth, masks, start, K4 = small_views(H, W, po)
    m = masks if use_masks else None
    dks = T.gates(3, T.TRUNC, VOXEL)
    want = T.track_batch(depth, m, K4, po, stride, start, *box["vol"], dks[:1])
    assert_tracks_equal(dev_track(depth, m, K4, po, stride, start, *box["vol"], dks[:1]), want, 1e-9)
    if H * W > 1 and stride == 1:
        assert want[1][:, 0].min() >= 6, "the case moves a pose"
    assert_tracks_equal(dev_track(depth, m, K4, po, stride, start, *box["vol"], dks),
                        T.track_batch(depth, m, K4, po, stride, start, *box["vol"], dks), 1e-7)


def test_depth_without_a_reading_is_skipped(box):
    """0, negative, NaN and infinite depth inside the mask are no reading: the gated count (stats [2]'s denominator) drops them."""
    depth, masks, start = box["depth"][:2].copy(), box["masks"][:2], box["start"][:2]
    r, c = np.nonzero(masks[0])
    for k, bad in enumerate((0.0, -0.4, np.nan, np.inf, -np.inf)):
        depth[0, r[k::5][:60], c[k::5][:60]] = bad
    want = T.track_batch(depth, masks, T.K4, 0.0, 1, start, *box["vol"], box["dks"][:1])
    clean = T.track_batch(box["depth"][:2], masks, T.K4, 0.0, 1, start, *box["vol"], box["dks"][:1])
    assert want[1][0, 0] < clean[1][0, 0] and want[1][1].tolist() == clean[1][1].tolist()
    assert_tracks_equal(dev_track(depth, masks, T.K4, 0.0, 1, start, *box["vol"], box["dks"][:1]), want, 1e-9)


# ---- constructed volumes: one point per frame, placed exactly ------------------------------------------------------------------
PV = 2.0 ** -8                 # the voxel: a power of two, so that origin + g * voxel is exact in float32 for g in sixteenths
PO = np.array([-4.0, -2.0, 3.0]) * PV


def point_frames(g):
    """B = len(g) frames of 1 x 1 pixels with K = (1, 1, 0, 0): pixel (0, 0) at depth 1 is the point (0, 0, 1), and with R = I
    and t = (0, 0, 1) - q the frame's only point is q = PO + g * PV exactly.  One point can never move a pose (6 unknowns), so
    stats [0] says whether it was an inlier and stats [1] is |trunc * phi| there."""
    q = PO + np.asarray(g, dtype=np.float64) * PV
    poses = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12), (len(q), 1))
    poses[:, [3, 7, 11]] = np.array([0.0, 0.0, 1.0]) - q
    return np.ones((len(q), 1, 1), np.float32), poses


def edge_points(dims):
    """g of points in the last cell of each axis, just outside each of the six sides, exactly on nodes, and inside."""
    n = np.array(dims, dtype=np.float64)
    mid = np.maximum(n - 1, 0) / 2 + 0.0625
    g = [mid, np.floor(mid), np.zeros(3), n - 1.0625, n - 2]
    for a in range(3):
        for v in (-0.0625, n[a] - 1, n[a] - 0.9375, n[a] - 1.5, n[a] - 2, 0.0):
            p = mid.copy()
            p[a] = v
            g.append(p)
    return np.array(g)


@pytest.mark.parametrize("dims", [(2, 2, 2), (5, 1, 7), (33, 17, 9)])
def test_points_at_the_edges_of_constructed_volumes(dims):
    """Random values and weights; the restatement decides which points count (inside iff 0 <= g < n - 1 on every axis: g = n - 1
    exactly is outside, the last cell [n - 2, n - 1) inside, an axis of one node has no cell at all) and the device agrees point
    by point, value by value."""
    rng = np.random.default_rng(sum(dims))
    wsum = rng.integers(1, 4, dims).astype(np.int32)
    acc = (rng.uniform(-1, 1, dims) * wsum).astype(np.float32)
    g = edge_points(dims)
    depth, poses = point_frames(g)
    vol = (acc, wsum, PO, PV, 3 * PV, 1)
    want = T.track_batch(depth, None, (1, 1, 0, 0), 0.0, 1, poses, *vol, [np.float32(4 * PV)])
    inside = ((g >= 0) & (g < np.array(dims) - 1)).all(1)
    assert want[1][:, 0].tolist() == inside.astype(np.float32).tolist()
    assert inside.sum() == (0 if min(dims) < 2 else 14), inside.sum()
    got = dev_track(depth, None, (1, 1, 0, 0), 0.0, 1, poses, *vol, [np.float32(4 * PV)])
    assert_tracks_equal(got, want, 0.0)
    assert got[0].tobytes() == poses.tobytes()


def test_unknown_corners_flat_cells_and_the_gate():
    """A node with wsum = min_weight - 1 silences the eight cells around it and no other; a cell of eight equal values has no
    gradient and is skipped; a point whose |trunc * phi| exceeds the gate is no inlier, one exactly at it is."""
    dims = (6, 5, 4)
    rng = np.random.default_rng(5)
    wsum = rng.integers(2, 5, dims).astype(np.int32)
    tsdf = rng.uniform(-1, 1, dims)
    tsdf[0:2, 0:2, 0:2] = 0.5                               # the flat cell (0,0,0)
    wsum[0:2, 0:2, 0:2] = 2
    wsum[3, 2, 2] = 1                                       # min_weight = 2: unknown
    acc = (tsdf * wsum).astype(np.float32)
    around = np.array([[3 + dx - 0.5, 2 + dy - 0.5, 2 + dz - 0.5] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)])
    others = np.array([[1.5, 2.5, 1.5], [4.25, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]])
    g = np.concatenate([around, [[0.5, 0.5, 0.5], [0.25, 0.75, 0.125]], others])
    depth, poses = point_frames(g)
    vol = (acc, wsum, PO, PV, 3 * PV, 2)
    wide = [np.float32(4 * PV)]
    want = T.track_batch(depth, None, (1, 1, 0, 0), 0.0, 1, poses, *vol, wide)
    assert want[1][:, 0].tolist() == [0.0] * 10 + [1.0] * 4
    assert_tracks_equal(dev_track(depth, None, (1, 1, 0, 0), 0.0, 1, poses, *vol, wide), want, 0.0)
    assert T.track_batch(depth, None, (1, 1, 0, 0), 0.0, 1, poses, acc, wsum, PO, PV, 3 * PV, 1, wide)[1][:8, 0].tolist() == [1.0] * 8
    e = want[1][10:, 1].astype(np.float32)                  # |trunc * phi| of the four inliers, float32
    order = np.argsort(e)
    gate = [e[order[1]]]                                    # exactly the second smallest: two inliers
    want = T.track_batch(depth, None, (1, 1, 0, 0), 0.0, 1, poses, *vol, gate)
    assert sorted(np.nonzero(want[1][:, 0])[0].tolist()) == sorted((10 + order[:2]).tolist())
    assert_tracks_equal(dev_track(depth, None, (1, 1, 0, 0), 0.0, 1, poses, *vol, gate), want, 0.0)


def test_validation_and_the_workspace_protocol(box):
    import torch
    from cppf2_amd import _lib, ops
    dev, L = ops._dev(), _lib.load()
    acc, wsum = (torch.from_numpy(x).to(dev) for x in box["vol"][:2])
    d = torch.from_numpy(box["depth"][:2]).to(dev)
    P = torch.from_numpy(box["start"][:2].copy()).to(dev)
    st = torch.full((2, 4), CANARY, dtype=torch.float32, device=dev)
    need = L.cppf_tsdf_track_workspace_bytes(2, 120, 160, 1)
    ws = torch.zeros((need,), dtype=torch.uint8, device=dev)
    dk = np.array(box["dks"], dtype=np.float32)
    base = dict(B=2, depth=ops._p(d), masks=None, H=120, W=160, K=_c(T.K4, 4), po=0.0, stride=1, acc=ops._p(acc), wsum=ops._p(wsum),
                origin=_c(T.ORIGIN, 3), voxel=VOXEL, dims=T.DIMS, trunc=T.TRUNC, min_weight=1, iters=10, dk=dk, poses=ops._p(P),
                stats=ops._p(st), ws=ops._p(ws), ws_bytes=need)

    def call(**kw):
        a = dict(base, **kw)
        dkp = None if a["dk"] is None else a["dk"].ctypes.data_as(C.c_void_p)
        return L.cppf_tsdf_track(a["B"], a["depth"], a["masks"], a["H"], a["W"], a["K"], C.c_float(a["po"]), a["stride"], a["acc"],
                                 a["wsum"], a["origin"], C.c_float(a["voxel"]), *a["dims"], C.c_float(a["trunc"]), a["min_weight"],
                                 a["iters"], dkp, a["poses"], a["stats"], a["ws"], a["ws_bytes"], ops._stream())
    bad_dk = [np.array([0.01, v], dtype=np.float32) for v in (0.0, -1.0, np.nan, np.inf)]
    cases = [dict(depth=None), dict(K=None), dict(acc=None), dict(wsum=None), dict(origin=None), dict(dk=None), dict(poses=None),
             dict(stats=None), dict(ws=None), dict(B=-1), dict(iters=-1), dict(stride=0), dict(stride=-2), dict(H=0), dict(W=0),
             dict(H=16385), dict(W=16385), dict(dims=(0, 30, 24)), dict(dims=(39, 30, -1)), dict(dims=(1 << 14, 1 << 14, 1)),
             dict(dims=(1024, 1024, 129)), dict(voxel=0.0), dict(voxel=float("nan")), dict(voxel=float("inf")),
             dict(origin=_c([0, float("nan"), 0], 3)), dict(trunc=0.0), dict(trunc=float("inf")), dict(min_weight=0),
             dict(po=float("nan")), dict(K=_c([0, 150, 80, 60], 4)), dict(ws_bytes=need - 1)]
    cases += [dict(iters=2, dk=b) for b in bad_dk]
    for kw in cases:
        assert call(**kw) == EINVAL, kw
        assert b"invalid argument" in L.cppf_last_error_string()
    torch.cuda.synchronize()
    assert P.cpu().numpy().tobytes() == box["start"][:2].tobytes() and bool((st == CANARY).all()), "a refused call wrote something"
    for args, want in (((2, 120, 160, 1), 2 * 75 * 256), ((1, 1, 1, 1), 256), ((5, 17, 13, 3), 5 * 256), ((0, 4, 4, 1), 0),
                       ((65535, 16384, 16384, 1), 65535 * (1 << 20) * 256), ((65536, 4, 4, 1), -1), ((-1, 4, 4, 1), -1),
                       ((1, 0, 4, 1), -1), ((1, 4, 16385, 1), -1), ((1, 4, 4, 0), -1)):
        assert L.cppf_tsdf_track_workspace_bytes(*args) == want, args
    assert call() == 0                                      # and the same arguments, untouched, are a valid call
    torch.cuda.synchronize()
    assert np.abs(P.cpu().numpy() - box["ten"][0][:2]).max() <= 1e-7


def test_wrapper_equals_the_entry_point(box):
    """track.track (hostargs, the cached scratch, the gate schedule on the host) gives the bytes of the direct call, leaves its
    argument alone, and takes [B,3,4] poses and a stride."""
    import torch
    from cppf2_amd import fuse, track
    acc, wsum = box["vol"][:2]
    vol = fuse.Volume(T.ORIGIN, VOXEL, T.DIMS)
    vol.acc.copy_(torch.from_numpy(acc))
    vol.wsum.copy_(torch.from_numpy(wsum))
    start = torch.from_numpy(box["start"].copy()).to(vol.device)
    for stride in (1, 2):
        P, S = track.track(vol, box["depth"], T.K3, start.reshape(5, 3, 4), box["masks"], stride=stride)
        want = dev_track(box["depth"], box["masks"], T.K4, 0.0, stride, box["start"], *box["vol"], box["dks"])
        assert P.cpu().numpy().tobytes() == want[0].tobytes() and S.cpu().numpy().tobytes() == want[1].tobytes()
    assert start.cpu().numpy().tobytes() == box["start"].tobytes()
    P, S = track.track(vol, box["depth"], T.K3, start, box["masks"], iters=0)
    assert P.cpu().numpy().tobytes() == box["start"].tobytes() and not S.any()


ORBIT_RMS = 1.64                        # tests/test_track.py's bound: twice the restatement's largest tracked RMS (0.820 voxel)


def test_onboard_equals_the_restatement_on_the_orbit():
    """track.onboard on the 36-frame orbit, first pose only, no sweep: the device's poses within 1e-7 of the restatement's (each
    frame's start and volume are the previous frames' results, so this holds the integration between the steps too), and
    its own mesh under (b)'s condition: closed, every vertex within 2 voxels of the box.  Then one sweep: the batched call
    against the finished volume, held to the restatement started from the device's own sweep-free poses."""
    import torch
    from cppf2_amd import fuse, track
    depth, masks, poses = T.box_views(T.orbit_dirs(36))
    _, want, wrep = track.onboard(depth, masks, T.K3, poses[0], VOXEL, extent=0.13, sweeps=0, dev="cpu", track_fn=T.ref_track,
                                  integrate_fn=T.ref_integrate)
    vol, got, rep = track.onboard(depth, masks, T.K3, poses[0], VOXEL, extent=0.13, sweeps=0)
    print("onboard: largest pose difference to the restatement %.3g" % np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-7
    assert [f["inliers"] for f in rep["frames"]] == [f["inliers"] for f in wrep["frames"]]
    assert [f["lost"] for f in rep["frames"]] == [f["lost"] for f in wrep["frames"]] and abs(rep["max_step"] - wrep["max_step"]) <= 1e-6
    mesh = fuse.extract(vol)
    far = T.box_distance(mesh.verts).max() / VOXEL
    after = max(T.surface_rms(depth[i], masks[i], got[i])[0] for i in range(36)) / VOXEL
    print("onboard: %d vertices, %d boundary edges, farthest %.3f voxel, largest frame RMS %.3f voxel" % (len(mesh.verts), mesh.boundary_edges, far, after))
    assert mesh.boundary_edges == 0 and far <= 2.0 and after <= ORBIT_RMS
    P, S = track.track(vol, depth[1:], T.K3, got[1:], masks[1:])
    acc, wsum = vol.acc.cpu().numpy(), vol.wsum.cpu().numpy()
    sweep = T.track_batch(depth[1:], masks[1:], T.K4, 0.0, 1, got[1:], acc, wsum, vol.origin, vol.voxel, vol.trunc, 1,
                          T.gates(10, vol.trunc, vol.voxel))
    assert_tracks_equal((P.cpu().numpy(), S.cpu().numpy()), sweep, 1e-7)
    vol1, got1, rep1 = track.onboard(depth, masks, T.K3, poses[0], VOXEL, extent=0.13, sweeps=1)
    assert got1[1:].tobytes() == P.cpu().numpy().tobytes() and got1[0].tobytes() == poses[0].tobytes() and vol1.views == 36
    mesh1 = fuse.extract(vol1)
    assert mesh1.boundary_edges == 0 and T.box_distance(mesh1.verts).max() / VOXEL <= 2.0


# Views of the orbit.  Checked on the CPU first (the restatement behind track.onboard, tests/render_ref.py's images): the fixture
# is 184 x 187 x 57 mm, so between two of 24 views its surface moves up to 44 mm, 4.9 trunc: 9 frames are lost; between two of 48,
# 22 mm: every frame finds its inliers (share >= 0.86) and still the sequence drifts 21 degrees and 26 mm, the mesh 19.6 voxel
# off; between two of 96, 11 mm (1.2 trunc): nothing lost, poses within 1.07 degrees and 2.9 mm of the rendered ones, every
# vertex within 1.41 voxel of the original.
CLI_VIEWS = 96


def test_command_line_onboards_rendered_views_from_the_first_pose_alone(tmp_path):
    """CLI_VIEWS rendered views of the fixture mesh on the orbit (160 x 120, depth quantised to 0.1 mm, pixel_offset 0.5, voxel
    3 mm) with every pose but the first image's REMOVED from scene_gt.json, through python -m cppf2_amd.fuse --track: every
    welded vertex lies within section 28's bound (trunc + sqrt(3) voxel + 0.1 mm) plus the tracked frames' largest reported RMS
    of the original surface.  Without --track the folder is refused (it has no poses to trust)."""
    import json
    from cppf2_amd import bop_data, fuse, render, symmetry
    mesh = render.load_mesh(FIXTURE, 0.001)
    K = render.INTRINSICS.copy()
    K[:2] *= 0.25
    dist = max(2.2 * float(np.linalg.norm(mesh.bounds[1] - mesh.bounds[0])), 0.3)
    P = FR.look_at(T.orbit_dirs(CLI_VIEWS), centre=np.zeros(3), dist=dist).astype(np.float64).reshape(-1, 3, 4)
    root = bop_data.write_dataset(str(tmp_path / "ds"), "train", {15: mesh}, [[[(15, p[:, :3], p[:, 3])] for p in P]], K=K, height=120,
                                  width=160, targets_file=None)
    scene = os.path.join(root, "train", "000000")
    out, rep = str(tmp_path / "obj_000015.ply"), str(tmp_path / "report.json")
    voxel = 0.003
    args = ["--views", scene, "--obj-id", "15", "--pixel-offset", "0.5", "--voxel", str(voxel), "--report", rep, "--out", out]
    with_poses = fuse.main(args + ["--track"])
    diffs = [f["recorded"] for f in with_poses["track"]["frames"]]
    assert len(diffs) == CLI_VIEWS and all(d is not None for d in diffs)
    assert diffs[0]["translation_m"] == 0.0 and diffs[0]["rotation_deg"] < 0.05          # float32 poses are orthonormal to 1e-7 only
    gt = json.load(open(os.path.join(scene, "scene_gt.json")))
    first = min(gt, key=int)
    for im, entries in gt.items():
        if im != first:
            for e in entries:
                del e["cam_R_m2c"], e["cam_t_m2c"]
    json.dump(gt, open(os.path.join(scene, "scene_gt.json"), "w"))
    with pytest.raises(KeyError):
        fuse.main(args)
    report = fuse.main(args + ["--track"])
    tr = report["track"]
    assert report["views"] == CLI_VIEWS and json.load(open(rep))["track"]["max_step"] == tr["max_step"]
    assert [f["recorded"] for f in tr["frames"][1:]] == [None] * (CLI_VIEWS - 1)
    assert [f["inliers"] for f in tr["frames"]] == [f["inliers"] for f in with_poses["track"]["frames"]]
    assert tr["lost"] == 0 and tr["sweeps"] == 1
    fused = render.load_mesh(out, 0.001)
    assert fused.faces.shape[0] == report["triangles"] > 1000
    tri = mesh.verts[mesh.faces].reshape(-1, 9)
    worst = float(symmetry.deviations(fused.verts, tri, np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(1, 12))[0])
    rms = max(f["rms"] for f in tr["frames"])
    bound = report["trunc"] + np.sqrt(3.0) * voxel + 1e-4 + rms
    print("fixture, first pose only: %d vertices, farthest vertex %.2f voxel (bound %.2f, of which RMS %.2f); max_step %.1f trunc; "
          "largest recorded difference %.2f degrees, %.2f mm"
          % (report["vertices"], worst / voxel, bound / voxel, rms / voxel, tr["max_step"] / tr["trunc"],
             max(d["rotation_deg"] for d in diffs), 1000 * max(d["translation_m"] for d in diffs)))
    assert worst <= bound
