"""GPU checks of the three scoring kernels at the shapes and values the other files do not reach: cppf_depth_fit_counts
(cppf_verify.hip), cppf_vsd_counts and cppf_mssd_mspd (cppf_bop.hip) against their NumPy restatements (tests/verify_ref.py,
tests/bop_ref.py) on synthetic arrays -- image sizes around one wavefront, one block and one grid pass, the launch split of the
fit counts, every count slot of a wavefront, decisions at exact equality, NaN / inf / negative / -0.0 depths, raw mask bytes,
and symmetry and vertex counts around the kernel's lane layout.  Counts are compared as integers, exactly; MSSD / MSPD at the
bars of tests/test_bop_gpu.py (1e-6 x diameter, 1e-3 px) and otherwise byte for byte."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bop_ref as BR  # noqa: E402
import verify_ref as VR  # noqa: E402

F = np.float32
UNIT_K = np.array([[2.0 ** 40, 0, 0], [0, 2.0 ** 40, 0], [0, 0, 1]])      # bop_ref.dist_factor = 1 exactly: D = d
TINY = float(np.finfo(np.float64).tiny)                                   # bop_ref's `near` at TINY counts exact ties only


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


# ----------------------------------------------------------------------------------------------
# cppf_depth_fit_counts
# ----------------------------------------------------------------------------------------------
FIT_TAUS = (0.002, 0.01, 0.05)
FIT_SIZES = [(1, 1), (3, 5), (1, 63), (1, 64), (1, 65),           # around one wavefront
             (23, 89), (32, 64), (1, 2049),                       # 2047, 2048, 2049: around one block (FIT_PIX)
             (45, 91), (17, 241)]                                 # 4095, 4097: around two blocks


def _fit_case(H, W, counts, seed):
    """(depth [I,H,W], mask uint8 [I,H,W], hyp_off [I+1], renders [P,H,W]): depths in [0.5, 1.5] with 20 % holes, a random mask,
    renders = the observed depth of their image +- 0.03 with 30 % of the pixels not drawn."""
    rng = np.random.default_rng(seed)
    I = len(counts)
    depth = rng.uniform(0.5, 1.5, (I, H, W))
    depth[rng.random((I, H, W)) < 0.2] = 0.0
    mask = (rng.random((I, H, W)) < 0.5).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    img = np.repeat(np.arange(I), counts)
    ren = depth[img] + rng.uniform(-0.03, 0.03, (len(img), H, W))
    ren[rng.random(ren.shape) < 0.3] = 0.0
    return depth.astype(F), mask, off, ren.astype(F)


@pytest.fixture(scope="module")
def fit_sizes():
    out = {}
    for k, (H, W) in enumerate(FIT_SIZES):
        d, m, off, r = _fit_case(H, W, [3, 2], 100 + k)
        out[(H, W)] = (d, m, off, r, VR.fit_counts(d, m, off, r, FIT_TAUS))
    return out


def _fit(d, m, off, r, taus):
    from cppf2_amd import verify
    _gpu()
    return verify.fit_counts(d, m, off, r, taus).cpu().numpy()


def test_fit_size_cases_reach_every_count(fit_sizes):
    """Each of the 7 columns is non-zero somewhere over the sizes: a kernel that wrote nothing cannot pass the test below."""
    total = sum(c[4] for c in fit_sizes.values()).sum(0)
    assert total.shape == (7,) and (total > 0).all(), total


@pytest.mark.parametrize("size", FIT_SIZES, ids=lambda s: "%dx%d" % s)
def test_fit_counts_image_sizes(fit_sizes, size):
    d, m, off, r, want = fit_sizes[size]
    got = _fit(d, m, off, r, FIT_TAUS)
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)


def _alone(d, m, off, r, taus, rows):
    """Hypothesis p submitted alone against its own image, for p in rows."""
    img = np.searchsorted(off, rows, side="right") - 1
    return np.concatenate([_fit(d[i], m[i], [0, 1], r[p:p + 1], taus) for p, i in zip(rows, img)])


def test_fit_counts_launch_split():
    """257 images = three launches of at most 128: ragged 0 .. 4 hypotheses on the first 128 images, none on images 128 .. 255
    (the second launch is skipped), 3 on image 256 (the third launch reads offset image, mask and global hypothesis rows)."""
    rng = np.random.default_rng(120)
    counts = np.concatenate([rng.integers(0, 5, 128), np.zeros(128, np.int64), [3]])
    counts[:6] = (0, 4, 0, 0, 1, 4)
    d, m, off, r = _fit_case(3, 5, counts, 121)
    assert off[128] == off[256] and off[257] - off[256] == 3
    want = VR.fit_counts(d, m, off, r, FIT_TAUS)
    got = _fit(d, m, off, r, FIT_TAUS)
    assert np.array_equal(got, want)
    assert (want.sum(0) > 0).all() and want[-3:].any(1).all() and len({w.tobytes() for w in want[-3:]}) == 3
    assert _alone(d, m, off, r, FIT_TAUS, np.arange(len(r))).tobytes() == got.tobytes()


def test_fit_counts_only_the_second_launch():
    """129 images, every hypothesis on image 128: the first launch is skipped, the second has one image."""
    counts = np.zeros(129, np.int64)
    counts[128] = 4
    d, m, off, r = _fit_case(3, 5, counts, 122)
    want = VR.fit_counts(d, m, off, r, FIT_TAUS)
    got = _fit(d, m, off, r, FIT_TAUS)
    assert np.array_equal(got, want) and want.any(1).all() and len({w.tobytes() for w in want}) == 4
    assert _alone(d, m, off, r, FIT_TAUS, np.arange(4)).tobytes() == got.tobytes()


@pytest.mark.parametrize("n", [1, 2, 67])
def test_fit_counts_hypothesis_parity(n):
    """1, 2 and 67 hypotheses on one image of 2047 pixels: the block alternates between two LDS buffers by hypothesis."""
    d, m, off, r = _fit_case(23, 89, [n], 130 + n)
    want = VR.fit_counts(d, m, off, r, FIT_TAUS)
    got = _fit(d, m, off, r, FIT_TAUS)
    assert np.array_equal(got, want)
    assert len({w.tobytes() for w in want}) == n


def _slot_taus(n, base):
    """n thresholds, unsorted, with duplicates and a 0."""
    return [base[k % len(base)] * (1 + 0.5 * (k // len(base))) for k in range(n)]


@pytest.mark.parametrize("n", [1, 28, 32])
def test_fit_counts_count_slots(n):
    """4 + n counts in the lanes of a wavefront: 5, 32 (half a wavefront) and 36 (the limit)."""
    taus = _slot_taus(n, (0.01, 0.002, 0.05, 0.0, 0.01, 0.03, 0.002, 0.02))
    d, m, off, r = _fit_case(23, 89, [3, 2], 140)
    want = VR.fit_counts(d, m, off, r, taus)
    got = _fit(d, m, off, r, taus)
    assert got.shape == (5, 4 + n) and np.array_equal(got, want)
    assert (want[:, 4] > 0).all() and (n < 4 or ((want[:, 7] == 0).all() and (want[:, 6] > want[:, 4]).all()))


def test_fit_counts_refuses_33_taus():
    from cppf2_amd import _lib
    d, m, off, r = _fit_case(3, 5, [1], 141)
    with pytest.raises(_lib.CppfError):
        _fit(d, m, off, r, [0.01] * 33)


def _fit_tie_arrays():
    """tests/test_verify.py::test_fit_counts_restatement_at_ties_and_special_values: (d_o, mask bytes, d_h, taus, row)."""
    t = F(2.0 ** -7)
    nan, inf = F(np.nan), F(np.inf)
    d_o = np.array([1, 1, 1, 1, nan, -1, inf, -0.0], F)
    m = np.array([1, 1, 2, 255, 1, 1, 1, 1], np.uint8)
    d_h = np.array([F(1) - t, np.nextafter(F(1) - t, F(0)), F(1) + t, np.nextafter(F(1) + t, F(2)), 1, 1, inf, nan], F)
    return d_o, m, d_h, np.array([t, 0.0], F), [7, 5, 1, 0, 2, 0]


def test_fit_counts_ties_special_values_and_raw_mask_bytes():
    """The hand-derived row, three times over in a 3 x 8 image (lanes 0 .. 23), through the C entry point itself so that the mask
    bytes 2 and 255 reach the kernel as they are."""
    import torch
    from cppf2_amd import _lib, ops
    dev = _gpu()
    d_o, m, d_h, taus, row = _fit_tie_arrays()
    depth, mask, ren = np.tile(d_o, (1, 3, 1)), np.tile(m, (1, 3, 1)), np.tile(d_h, (1, 3, 1))
    want = VR.fit_counts(depth, mask, [0, 1], ren, taus)
    assert want.tolist() == [[3 * c for c in row]]
    td, tm, tr, tt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (depth, mask, ren, taus))
    assert tm.dtype == torch.uint8 and sorted(set(tm.cpu().numpy().ravel().tolist())) == [1, 2, 255]
    counts = torch.full((1, 6), -1, dtype=torch.int64, device=dev)
    off = np.array([0, 1], np.int32)
    _lib.check(_lib.load().cppf_depth_fit_counts(1, 3, 8, ops._p(td), ops._p(tm), off.ctypes.data_as(C.c_void_p), 1, ops._p(tr),
                                                 ops._p(tt), 2, ops._p(counts), ops._stream()), "cppf_depth_fit_counts")
    assert np.array_equal(counts.cpu().numpy(), want)


# ----------------------------------------------------------------------------------------------
# cppf_vsd_counts
# ----------------------------------------------------------------------------------------------
VSD_SIZES = [(1, 1), (7, 37), (1, 255), (1, 256), (1, 257),       # around one block of 256
             (127, 129), (113, 145)]                              # 16 383, 16 385: around 64 blocks x 256 (the second grid pass)
VSD_TAUS = np.arange(1, 11) * 0.05
VSD_IDX = (1, 0, 1)


def _K(H, W):
    """An ordinary camera with its principal point inside the image, off the pixel grid."""
    return np.array([[572.4114, 0, 0.45 * W], [0, 573.57043, 0.55 * H], [0, 0, 1]])


def _vsd_case(H, W, seed, idx=VSD_IDX, I=2, grid=False):
    """(test [I,H,W], est [P,H,W], gt [P,H,W]): test depths in [0.5, 1.5] with 20 % holes, estimate and ground truth = their
    test image +- 0.03 with 30 % of the pixels not drawn; grid: every value a multiple of 2^-10."""
    rng = np.random.default_rng(seed)
    P = len(idx)
    if grid:
        test = rng.integers(512, 1537, (I, H, W)) / 1024.0
        pert = rng.integers(-31, 32, (2, P, H, W)) / 1024.0
    else:
        test = rng.uniform(0.5, 1.5, (I, H, W))
        pert = rng.uniform(-0.03, 0.03, (2, P, H, W))
    test[rng.random(test.shape) < 0.2] = 0.0
    src = test[np.clip(np.asarray(idx), 0, I - 1)]
    est, gt = src + pert[0], src + pert[1]
    est[rng.random(est.shape) < 0.3] = 0.0
    gt[rng.random(gt.shape) < 0.3] = 0.0
    return test.astype(F), est.astype(F), gt.astype(F)


def _vsd(test, idx, est, gt, K, diam, delta, taus):
    from cppf2_amd import bop
    _gpu()
    return bop.vsd_counts(test, np.asarray(idx, np.int32), est, gt, K, diam, delta, taus).cpu().numpy()


def _vsd_want(test, idx, est, gt, K, diam, delta, taus, near=0.0):
    """The restatement's rows (zero for a test index outside the batch) and the sum of its `near` counts."""
    diam = np.broadcast_to(np.asarray(diam, F), (len(idx),))
    rows, close = [], 0
    for p, i in enumerate(idx):
        if not 0 <= i < len(test):
            rows.append(np.zeros(2 + len(taus), np.int64))
            continue
        c, n = BR.vsd_counts(test[i], est[p], gt[p], K, delta, diam[p], taus, near=near)
        rows.append(c)
        close += n
    return np.stack(rows), close


@pytest.mark.parametrize("size", VSD_SIZES, ids=lambda s: "%dx%d" % s)
def test_vsd_counts_image_sizes(size):
    """Three pairs over two test images under an ordinary K.  No pixel of these seeds lies within 1e-12 of a threshold (asserted),
    so the comparison is exact and excuses nothing."""
    H, W = size
    test, est, gt = _vsd_case(H, W, 200 + VSD_SIZES.index(size))
    want, near = _vsd_want(test, VSD_IDX, est, gt, _K(H, W), 0.08, 0.015, VSD_TAUS, near=1e-12)
    assert near == 0
    got = _vsd(test, VSD_IDX, est, gt, _K(H, W), 0.08, 0.015, VSD_TAUS)
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)
    if H * W > 255:
        assert (want[:, 0] > want[:, 1]).all() and (want[:, 2] > want[:, -1]).all() and (want[:, -1] > 0).all()


def test_vsd_counts_unit_factor_exact_ties():
    """The same sizes with every D equal to its depth and every depth, delta and threshold a multiple of 2^-10: the float64
    arithmetic is exact, pixels sit exactly on delta and on every threshold (asserted over the set), equality is unconditional."""
    delta, diam, taus = 2.0 ** -6, 0.25, 2.0 ** -np.arange(7.0, 2.0, -1.0)        # thresholds 2, 4, 8, 16, 32 x 2^-10
    ties = np.zeros(1 + len(taus), np.int64)
    for k, (H, W) in enumerate(VSD_SIZES):
        test, est, gt = _vsd_case(H, W, 220 + k, grid=True)
        want, _ = _vsd_want(test, VSD_IDX, est, gt, UNIT_K, diam, delta, taus)
        got = _vsd(test, VSD_IDX, est, gt, UNIT_K, diam, delta, taus)
        assert np.array_equal(got, want), ((H, W), got, want)
        t = test[list(VSD_IDX)].astype(np.float64)
        ties[0] += np.count_nonzero((gt > 0) & (t != 0) & (gt.astype(np.float64) - t == delta))
        for j in range(len(taus)):
            ties[1 + j] += _vsd_want(test, VSD_IDX, est, gt, UNIT_K, diam, delta, taus[j:j + 1], near=TINY)[1]
    assert (ties > 0).all(), ties


@pytest.mark.parametrize("n", [1, 32])
def test_vsd_counts_test_index_diameters_and_count_slots(n):
    """Test indices -1 and I in the middle of a batch give zero rows and leave their neighbours alone; one diameter per pair;
    2 + n counts in the lanes of a wavefront: 3 and 34 (the limit)."""
    idx = (0, -1, 1, 2, 0)
    diam = np.array([0.1, 0.3, 0.05, 0.2, 0.15], F)
    taus = np.array(_slot_taus(n, (0.3, 0.05, 0.5, 0.0, 0.3, 0.1, 0.05, 0.2)), F)
    test, est, gt = _vsd_case(7, 37, 240, idx=idx)
    want, near = _vsd_want(test, idx, est, gt, _K(7, 37), diam, 0.015, taus, near=1e-12)
    assert near == 0
    got = _vsd(test, idx, est, gt, _K(7, 37), diam, 0.015, taus)
    assert got.shape == (5, 2 + n) and np.array_equal(got, want), (got, want)
    assert not got[1].any() and not got[3].any() and (got[[0, 2, 4], 1] > 0).all()
    assert len({w[:3].tobytes() for w in want[[0, 2, 4]]}) == 3
    assert n < 4 or ((want[[0, 2, 4], 5] == want[[0, 2, 4], 1]).all() and (want[[0, 2, 4], 4] < want[[0, 2, 4], 3]).all())


def test_vsd_counts_refuses_33_taus():
    from cppf2_amd import _lib
    test, est, gt = _vsd_case(3, 5, 241)
    with pytest.raises(_lib.CppfError):
        _vsd(test, VSD_IDX, est, gt, _K(3, 5), 0.1, 0.015, [0.1] * 33)


def _vsd_tie_arrays():
    """tests/test_bop.py::test_vsd_restatement_at_exact_ties and ..._at_special_values: [(d_test, d_est, d_gt, counts)]."""
    one = np.ones(8, F)
    dt, de = one.copy(), one.copy()
    dt[0] = F(1) - F(2.0 ** -6)
    dt[1] = np.nextafter(dt[0], F(0))
    de[2] = F(1) + F(2.0 ** -5)
    de[3] = np.nextafter(de[2], F(1))
    nan, inf = F(np.nan), F(np.inf)
    return [(dt, de, one, [7, 7, 1, 0]),
            (np.array([nan, -1, -0.0, inf, 0, 1, 1, 1], F), np.array([1, 1, 1, 1, nan, inf, -0.0, -2], F),
             np.array([1, 1, 1, 1, 1, 1, nan, inf], F), [4, 3, 1, 1])]


def test_vsd_counts_ties_and_special_values():
    """The two hand-derived rows, each three times over in a 3 x 8 image, as two pairs with their own test images."""
    rows = _vsd_tie_arrays()
    test, est, gt = (np.stack([np.tile(r[k], (3, 1)) for r in rows]) for k in range(3))
    want, _ = _vsd_want(test, (0, 1), est, gt, UNIT_K, 0.25, 2.0 ** -6, (0.125, 0.5))
    assert want.tolist() == [[3 * c for c in r[3]] for r in rows]
    got = _vsd(test, (0, 1), est, gt, UNIT_K, 0.25, 2.0 ** -6, (0.125, 0.5))
    assert np.array_equal(got, want), (got, want)


def test_vsd_counts_batch_and_grid_independence():
    """Each pair alone (a grid of 64 x 1 blocks instead of 64 x 3) gives the bytes of its row in the batch."""
    H, W = 113, 145
    test, est, gt = _vsd_case(H, W, 250)
    got = _vsd(test, VSD_IDX, est, gt, _K(H, W), 0.1, 0.015, VSD_TAUS)
    for p, i in enumerate(VSD_IDX):
        one = _vsd(test[i], (0,), est[p:p + 1], gt[p:p + 1], _K(H, W), 0.1, 0.015, VSD_TAUS)
        assert one.tobytes() == got[p:p + 1].tobytes(), p
    assert len({g.tobytes() for g in got}) == 3


# ----------------------------------------------------------------------------------------------
# cppf_mssd_mspd
# ----------------------------------------------------------------------------------------------
ALL_S = (1, 2, 3, 4, 5, 8, 63, 64, 65, 129)
ALL_V = (1, 2, 255, 1024, 1025, 2049)
MSSD_CASES = ([(S, 1025) for S in ALL_S] + [(S, V) for S in (3, 65) for V in ALL_V if V != 1025]
              + [(1, 1), (1, 2)])                                 # S = 1 with V = 1, 2: 254 of the 256 vertex groups idle
BOX = 0.1                                                         # metres: the vertices fill a 10 cm box
DIAMETER = BOX * np.sqrt(3.0)                                     # the box's diagonal, whatever number of vertices samples it
CAM_K = np.array([[572.4114, 0, 325.2611], [0, 573.57043, 242.04899], [0, 0, 1]])
IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])


def _rand_pose(rng, t):
    return np.hstack([BR.rotation(rng.standard_normal(3), rng.uniform(0, np.pi)), np.asarray(t, np.float64).reshape(3, 1)])


def _perturb(P, rng, deg=(1, 10), mm=(1, 20)):
    ax, d = rng.standard_normal(3), rng.standard_normal(3)
    Q = P.copy()
    Q[:, :3] = BR.rotation(ax, np.deg2rad(rng.uniform(*deg))) @ P[:, :3]
    Q[:, 3] = P[:, 3] + d / np.linalg.norm(d) * rng.uniform(*mm) * 1e-3
    return Q


def _syms(S, rng, identity_at=0):
    """The identity (at row identity_at) and S - 1 random proper rotations with translations of up to 1 cm."""
    out = []
    for _ in range(S):
        d = rng.standard_normal(3)
        out.append(_rand_pose(rng, d / np.linalg.norm(d) * rng.uniform(0, 0.01)))
    out[identity_at] = IDENTITY.copy()
    return np.stack(out)


def _verts(V, rng):
    return rng.uniform(-BOX / 2, BOX / 2, (V, 3)).astype(F)


def _pairs(rng, n=3):
    gt = np.stack([_rand_pose(rng, [rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), 0.8]) for _ in range(n)])
    return np.stack([_perturb(P, rng) for P in gt]), gt


def _mm(verts, syms, est, gt):
    from cppf2_amd import bop
    _gpu()
    return tuple(x.cpu().numpy() for x in bop.mssd_mspd(verts, syms, est, gt, CAM_K))


def _check_mm(verts, syms, est, gt):
    ms, mp = _mm(verts, syms, est, gt)
    assert ms.dtype == F and mp.dtype == F and ms.shape == mp.shape == (len(est),)
    for p in range(len(est)):
        wd, wp = BR.mssd_mspd(verts, syms, est[p], gt[p], CAM_K)
        assert abs(float(ms[p]) - wd) <= 1e-6 * DIAMETER, (p, ms[p], wd)
        assert (np.isinf(mp[p]) and np.isinf(wp)) or abs(float(mp[p]) - wp) <= 1e-3, (p, mp[p], wp)
    return ms, mp


@pytest.mark.parametrize("S,V", MSSD_CASES)
def test_mssd_mspd_symmetry_and_vertex_counts(S, V):
    """Every lane layout (SC = 1, 2, 4, 8, 64), sets that leave lanes invalid (3, 5, 63, 65, 129), a second block with one valid
    lane (65), fewer vertices than vertex groups, and whole and partial LDS tiles."""
    rng = np.random.default_rng(300 + 7 * S + V)
    est, gt = _pairs(rng)
    ms, mp = _check_mm(_verts(V, rng), _syms(S, rng), est, gt)
    assert (ms > 0).all() and (mp > 0).all() and np.isfinite(mp).all()


@pytest.mark.parametrize("S", ALL_S)
def test_mssd_mspd_estimate_equal_to_the_ground_truth_scores_zero(S):
    """est = gt and the identity in the set (in its last row: for S = 65 the one valid lane of the second block): exactly 0."""
    rng = np.random.default_rng(400 + S)
    _, gt = _pairs(rng)
    ms, mp = _mm(_verts(1025, rng), _syms(S, rng, identity_at=S - 1), gt, gt)
    assert ms.tobytes() == np.zeros(3, F).tobytes() and mp.tobytes() == np.zeros(3, F).tobytes(), (ms, mp)


@pytest.mark.parametrize("S,V", [(3, 1025), (5, 255), (65, 1025), (129, 2049)])
def test_mssd_mspd_order_and_batch_independence(S, V):
    """Maxima and minima of non-negative floats are exact: permuted symmetry rows, permuted vertex rows and each pair alone give
    the same bytes."""
    rng = np.random.default_rng(500 + S)
    est, gt = _pairs(rng)
    verts, syms = _verts(V, rng), _syms(S, rng)
    ms, mp = _check_mm(verts, syms, est, gt)
    for _ in range(2):
        a, b = _mm(verts, syms[rng.permutation(S)], est, gt)
        assert a.tobytes() == ms.tobytes() and b.tobytes() == mp.tobytes()
        a, b = _mm(verts[rng.permutation(V)], syms, est, gt)
        assert a.tobytes() == ms.tobytes() and b.tobytes() == mp.tobytes()
    for p in range(3):
        a, b = _mm(verts, syms, est[p:p + 1], gt[p:p + 1])
        assert a.tobytes() == ms[p:p + 1].tobytes() and b.tobytes() == mp[p:p + 1].tobytes(), p


@pytest.mark.parametrize("S", [3, 5, 63, 65, 129])
def test_mssd_mspd_rows_past_the_set_are_not_part_of_it(S):
    """The S rows are the head of a longer device array whose other rows hold the transform that maps the ground truth onto the
    estimate: a lane past S that took part would score about 0.  The result is that of the S rows alone, byte for byte."""
    import torch
    dev = _gpu()
    rng = np.random.default_rng(600 + S)
    T = _perturb(IDENTITY, rng, deg=(4, 6), mm=(4, 6))
    gt = _pairs(rng, 1)[1]
    est = np.hstack([gt[0][:, :3] @ T[:, :3], (gt[0][:, :3] @ T[:, 3] + gt[0][:, 3])[:, None]])[None]
    verts, syms = _verts(1025, rng), _syms(S, rng)
    assert max(BR.mssd_mspd(verts, T[None], est[0], gt[0], CAM_K)) < 1e-9
    ms, mp = _check_mm(verts, syms, est, gt)
    assert ms[0] > 1e-3 and mp[0] > 1.0
    long = torch.from_numpy(np.concatenate([syms, np.repeat(T[None], 192 - S, 0)]).reshape(-1, 12)).to(dev)
    a, b = _mm(verts, long[:S], est, gt)
    assert a.tobytes() == ms.tobytes() and b.tobytes() == mp.tobytes(), (a, ms, b, mp)


@pytest.mark.parametrize("at", [0, 4])
def test_mspd_ignores_a_symmetry_that_puts_a_vertex_behind_the_camera(at):
    """One symmetry of five moves exactly one vertex (5 mm) behind the camera plane: MSPD is that of the other four, MSSD too (the
    moved pose is 74 cm away).  When every symmetry does so, MSPD is +inf and MSSD finite."""
    rng = np.random.default_rng(700 + at)
    verts = _verts(255, rng)
    verts[0] = (0.0, 0.0, -0.06)                                  # 1 cm below the box: the only vertex with z < -0.05
    gt = np.hstack([np.eye(3), [[0.02], [-0.01], [0.8]]])[None]
    est = _perturb(gt[0], rng)[None]
    behind = np.hstack([np.eye(3), [[0.0], [0.0], [-0.745]]])
    z = verts[:, 2].astype(np.float64) - 0.745 + 0.8
    assert np.count_nonzero(z <= 0) == 1 and z[0] < -0.004 and np.delete(z, 0).min() > 0.004
    four = _syms(4, rng)
    five = np.insert(four, at, behind, axis=0)
    ms4, mp4 = _check_mm(verts, four, est, gt)
    ms5, mp5 = _check_mm(verts, five, est, gt)
    assert np.isfinite(mp5).all() and ms5.tobytes() == ms4.tobytes() and mp5.tobytes() == mp4.tobytes()
    far = behind.copy()
    far[2, 3] = -0.9
    ms, mp = _check_mm(verts, np.stack([behind, far]), est, gt)
    assert np.isfinite(ms).all() and ms[0] > 0.7 and np.isposinf(mp).all()
