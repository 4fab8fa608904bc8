"""GPU checks of the depth-to-cloud front end (cppf2_amd/csrc/cppf_prep.hip) against the plain restatements of tests/prep_ref.py,
which tests/test_prep.py pins on the CPU: cppf_backproject / cppf_backproject64 byte for byte on image sizes around the
1024-pixel scan pass, every mask kind, invalid depth and four cameras; cppf_voxel_downsample as an exact index set on lattice
clouds around the hash table's capacity steps; cppf_interpolate_features against a float64 restatement over channel counts,
grid sizes, keypoint counts and layouts."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prep_ref as PR  # noqa: E402


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


# ---------------------------------------------------------------------------------------------------------------
# back-projection
# ---------------------------------------------------------------------------------------------------------------
SENTINEL = -12345.5
GUARD = 8


def _raw_backproject(f64, depth, mask_u8, K, cap, rowcol=True):
    """The C entry point itself with `cap` rows of room and GUARD sentinel rows behind them:
    (count, out_pts [cap+GUARD,3], out_rowcol [cap+GUARD,2] or None)."""
    import torch
    from cppf2_amd import _lib, ops
    dev = _gpu()
    depth = np.ascontiguousarray(depth, dtype=np.float64 if f64 else np.float32)
    H, W = depth.shape
    d = torch.from_numpy(depth).to(dev)
    m = torch.from_numpy(np.ascontiguousarray(mask_u8, dtype=np.uint8)).to(dev)
    kinv = (ctypes.c_double * 9)(*np.linalg.inv(np.asarray(K, dtype=np.float64).reshape(3, 3)).reshape(9))
    pts = torch.full((cap + GUARD, 3), SENTINEL, dtype=d.dtype, device=dev)
    rc = torch.full((cap + GUARD, 2), -7, dtype=torch.int32, device=dev) if rowcol else None
    cnt = torch.full((1,), -1, dtype=torch.int32, device=dev)
    fn = ops._L.cppf_backproject64 if f64 else ops._L.cppf_backproject
    _lib.check(fn(ops._p(d), ops._p(m), H, W, kinv, cap, ops._p(pts), ops._p(rc), ops._p(cnt), ops._stream()), "backproject")
    return int(cnt.item()), pts.cpu().numpy(), None if rc is None else rc.cpu().numpy()


def _bp_case(shape):
    rng = np.random.default_rng(shape[0] * 10000 + shape[1])          # the inputs tests/test_prep.py pins on the CPU
    d32, d64, kind = PR.bp_depth(shape, rng)
    return d32, d64, kind, PR.bp_masks(shape, rng)


@pytest.mark.parametrize("shape", PR.BP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_backproject_equals_the_restatement_byte_for_byte(shape):
    """Both entry points on every mask kind and camera: points equal to prep_ref.backproject32 / backproject64 as bytes (the
    skewed K included: the restatement, not NumPy's matmul, is the contract), (rows, cols) equal to np.nonzero of the valid
    pixels, no pixel with depth 0, -1, NaN or -inf emitted, every masked subnormal emitted."""
    _gpu()
    from cppf2_amd import ops
    d32, d64, kind, masks = _bp_case(shape)
    assert set(masks) == {"empty", "full", "first", "last", "tail", "checker", "random", "values"}
    if shape[0] * shape[1] >= 16:
        assert set(np.unique(kind)) == {-1, 0, 1, 2, 3, 4}
    with np.errstate(invalid="ignore"):
        pos32, pos64 = d32 > 0, d64 > 0
    assert np.array_equal(pos32, pos64) and np.array_equal(pos32, (kind == -1) | (kind == 4))
    for kname, K in PR.INTRINSICS.items():
        for mname, m in masks.items():
            rows, cols = np.nonzero((m != 0) & pos32)
            tag = (shape, kname, mname)
            if mname == "tail":
                assert m.any() and np.flatnonzero(m.reshape(-1)).min() == PR.BP_BLOCK * ((m.size - 1) // PR.BP_BLOCK)
            want32, (wr, wc) = PR.backproject32(d32, K, m)
            got32, (r, c) = ops.backproject(d32, K, m)
            assert np.array_equal(wr, rows) and np.array_equal(wc, cols)
            assert np.array_equal(r, rows) and np.array_equal(c, cols), tag
            assert got32.dtype == np.float32 and got32.shape == want32.shape, tag
            assert got32.tobytes() == want32.tobytes(), tag
            want64, _ = PR.backproject64(d64, K, m)
            got64, (r, c) = ops.backproject_reference(d64, K, m)
            assert np.array_equal(r, rows) and np.array_equal(c, cols), tag
            assert got64.dtype == np.float64 and got64.shape == want64.shape, tag
            assert got64.tobytes() == want64.tobytes(), tag
            emitted = kind[r, c]
            assert np.isin(emitted, (-1, 4)).all() and (emitted == 4).sum() == ((kind == 4) & (m != 0)).sum(), tag
    # the kernel itself reads any nonzero byte as set: 1, 2 and 255 without the wrapper's `!= 0`
    m = masks["values"]
    if m.any():
        assert shape[0] * shape[1] < 16 or set(np.unique(m)) == {0, 1, 2, 255}
        for f64, d, ref in ((False, d32, PR.backproject32), (True, d64, PR.backproject64)):
            want, (wr, wc) = ref(d, PR.INTRINSICS["offcentre"], m)
            n, pts, rc = _raw_backproject(f64, d, m, PR.INTRINSICS["offcentre"], m.size)
            assert n == len(want) and pts[:n].tobytes() == want.tobytes()
            assert np.array_equal(rc[:n, 0], wr) and np.array_equal(rc[:n, 1], wc)


def test_backproject_keeps_infinite_depth_and_changes_no_other_row():
    """+inf passes depth > 0: the pixel is emitted with z = +inf (x and y infinite too), and every other row is what it was
    with a finite depth there."""
    _gpu()
    from cppf2_amd import ops
    shape = (37, 53)
    rr, cc = np.mgrid[0:shape[0], 0:shape[1]]
    base = (0.9 + 0.2 * np.sin(rr / 5.0) * np.cos(cc / 9.0)).astype(np.float32)
    m = np.ones(shape, np.uint8)
    at = 20 * shape[1] + 31
    inf = base.copy()
    inf.reshape(-1)[at] = np.inf
    for kname in ("example", "skew"):
        K = PR.INTRINSICS[kname]
        for f64 in (False, True):
            fn = ops.backproject_reference if f64 else ops.backproject
            ref = PR.backproject64 if f64 else PR.backproject32
            a, _ = fn(base.astype(np.float64) if f64 else base, K, m)
            b, (r, c) = fn(inf.astype(np.float64) if f64 else inf, K, m)
            assert len(a) == len(b) == m.size and (r[at], c[at]) == (20, 31)
            assert b[at, 2] == np.inf and np.isinf(b[at]).all()
            assert np.delete(a, at, 0).tobytes() == np.delete(b, at, 0).tobytes()
            assert b.tobytes() == ref(inf.astype(np.float64) if f64 else inf, K, m)[0].tobytes()


@pytest.mark.parametrize("shape", [(37, 53), (3, 1021)], ids=lambda s: "%dx%d" % s)
def test_backproject_cap_below_the_count_and_null_rowcol(shape):
    """include/cppf_hip.h: out_count is the number of valid pixels and "may exceed cap".  With cap = count - 1 and cap = 1 the
    count is still the full one, the first cap rows are the restatement's, and nothing is written behind row cap in out_pts or
    out_rowcol; out_rowcol = NULL gives the same points."""
    _gpu()
    d32, d64, kind, masks = _bp_case(shape)
    m = masks["random"]
    K = PR.INTRINSICS["skew"]
    for f64, d, ref in ((False, d32, PR.backproject32), (True, d64, PR.backproject64)):
        want, (wr, wc) = ref(d, K, m)
        count = len(want)
        assert count > 300
        wrc = np.stack([wr, wc], -1)
        for cap in (count - 1, 1, count):
            n, pts, rc = _raw_backproject(f64, d, m, K, cap)
            assert n == count, (f64, cap)
            k = min(cap, count)
            assert pts[:k].tobytes() == want[:k].tobytes(), (f64, cap)
            assert np.array_equal(rc[:k], wrc[:k]), (f64, cap)
            assert (pts[k:] == SENTINEL).all() and (rc[k:] == -7).all(), (f64, cap)
            n2, pts2, rc2 = _raw_backproject(f64, d, m, K, cap, rowcol=False)
            assert rc2 is None and n2 == count and pts2.tobytes() == pts.tobytes(), (f64, cap)


def test_backproject_device_and_tensor_inputs_give_the_same_bytes():
    """torch tensors (host or device, bool or uint8 mask) and return_device=True are plumbing only."""
    dev = _gpu()
    import torch
    from cppf2_amd import ops
    d32, d64, kind, masks = _bp_case((37, 53))
    K = PR.INTRINSICS["offcentre"]
    for mname in ("random", "values", "empty"):
        m = masks[mname]
        want, (wr, wc) = ops.backproject(d32, K, m)
        assert want.tobytes() == PR.backproject32(d32, K, m)[0].tobytes()
        for dt, mt in ((torch.from_numpy(d32), torch.from_numpy(m)), (torch.from_numpy(d32).to(dev), torch.from_numpy(m).to(dev)),
                       (torch.from_numpy(d32).to(dev), torch.from_numpy(m != 0).to(dev))):
            got, (r, c) = ops.backproject(dt, K, mt)
            assert got.tobytes() == want.tobytes() and np.array_equal(r, wr) and np.array_equal(c, wc)
            pts, (rd, cd) = ops.backproject(dt, torch.tensor(K, dtype=torch.float64), mt, return_device=True)
            assert pts.is_cuda and pts.dtype == torch.float32 and pts.cpu().numpy().tobytes() == want.tobytes()
            assert np.array_equal(rd.cpu().numpy(), wr) and np.array_equal(cd.cpu().numpy(), wc)
            g64, (r, c) = ops.backproject_reference(dt.double(), K, mt)
            assert g64.tobytes() == PR.backproject64(d32.astype(np.float64), K, m)[0].tobytes()


# ---------------------------------------------------------------------------------------------------------------
# voxel down-sample
# ---------------------------------------------------------------------------------------------------------------
def _ds_check(pc, res, seed, tag):
    from cppf2_amd import ops
    want = PR.downsample_exact(pc, res, seed)
    got = ops.downsample(pc, res, seed=seed)
    assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), \
        (tag, len(pc), len(want), len(got), int((got[:min(len(got), len(want))] != want[:min(len(got), len(want))]).sum()))
    return want


@pytest.mark.parametrize("n", PR.DS_COUNTS)
def test_downsample_is_the_exact_index_set_around_the_capacity_steps(n):
    """Point counts around the hash table's steps (1024 slots up to n = 512, doubling after), once with every point in a voxel
    of its own (the table at its fullest, every probe chain), once with about five points per voxel (every slot contended)."""
    _gpu()
    rng = np.random.default_rng(n)
    pc, res = PR.ds_own_voxel(n, rng)
    assert np.array_equal(_ds_check(pc, res, 11, "own"), np.arange(n))
    pc, res = PR.ds_five_per_voxel(n, rng)
    assert len(_ds_check(pc, res, 11, "five")) == max(1, n // 5)


def test_downsample_one_contended_slot_and_duplicate_points():
    """20 000 points in one voxel: one slot takes every atomicMin, and the survivor is the single smallest priority.  3000 points,
    each stored three times: duplicates share a voxel and only the priority (then the index) separates them."""
    _gpu()
    rng = np.random.default_rng(7)
    res = 2.0 ** -5
    one = PR.lattice_cloud(rng, np.zeros((20000, 3), np.int64), res, (0.5, -1.0, 0.75))
    for seed in (0, 9, 2 ** 40 + 1):
        assert len(_ds_check(one, res, seed, "one voxel")) == 1
    cells = PR.distinct_cells(rng, 200, 8)
    dup = PR.lattice_cloud(rng, cells[np.r_[np.arange(200), rng.integers(0, 200, 800)]], res, (0.5, -1.0, 0.75), multiplicity=3)
    assert dup.shape == (3000, 3) and len(np.unique(dup, axis=0)) == 1000
    assert len(_ds_check(dup, res, 9, "duplicates")) == 200


def test_downsample_geometry_one_axis_negative_far_and_the_21_bit_fields():
    """Clouds that vary along one axis only, lie in the negative octant, or sit at (1000, -2000, 500) with res 0.5; and six points
    whose voxel indices on one axis are 0, 1, 2^20, 2^21-3, 2^21-2, 2^21-1: the last indices a field of the packed key holds
    (res 2^-8, extent 8192), on x, y and z in turn, which must stay six voxels."""
    _gpu()
    for name, (pc, res) in PR.ds_geometry(np.random.default_rng(21)).items():
        for seed in (3, 2 ** 33 + 3):
            k = _ds_check(pc, res, seed, name)
            if name.startswith("field"):
                assert len(k) == 6


def test_downsample_uses_both_seed_words():
    """Seeds 0, 5, 2^32, 2^32 + 5 and 2^64 - 1 on one cloud: each equals its restatement, and 5 and 2^32 + 5 (equal low words)
    give different sets."""
    _gpu()
    pc, res = PR.ds_five_per_voxel(1025, np.random.default_rng(33))
    got = {seed: _ds_check(pc, res, seed, "seed %d" % seed) for seed in PR.DS_SEEDS}
    assert not np.array_equal(got[5], got[2 ** 32 + 5])
    assert not np.array_equal(got[0], got[2 ** 32])
    assert len({k.tobytes() for k in got.values()}) == len(PR.DS_SEEDS)


# ---------------------------------------------------------------------------------------------------------------
# feature interpolation
# ---------------------------------------------------------------------------------------------------------------
IF_TOL = max(2e-6, 2 * PR.ORACLE_VS_F64)


def _layouts(desc, dev):
    """The same [1,C,h,w] map three ways: NCHW contiguous, the patch-major [h,w,C] tokens permuted to NCHW, and a
    [:, :, 1:-1, 2:-1] slice of a larger NaN-filled tensor (storage offset, padded strides)."""
    import torch
    C, h, w = desc.shape
    nchw = torch.from_numpy(desc)[None].to(dev)
    patch = nchw[0].permute(1, 2, 0).contiguous().permute(2, 0, 1)[None]
    big = torch.full((1, C, h + 2, w + 3), float("nan"), dtype=torch.float32, device=dev)
    big[:, :, 1:-1, 2:-1] = nchw
    sl = big[:, :, 1:-1, 2:-1]
    assert nchw.is_contiguous() and (C == 1 or h * w == 1 or (patch.stride(1) == 1 and not patch.is_contiguous()))
    assert sl.storage_offset() == (w + 3) + 2 and sl.stride(1) == (h + 2) * (w + 3) and sl.stride(2) == w + 3
    assert torch.equal(patch, nchw) and torch.equal(sl, nchw)
    return nchw, patch, sl


@pytest.mark.parametrize("hw", PR.IF_GRIDS, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("C", PR.IF_CHANNELS)
def test_interpolate_features_equals_the_float64_restatement(C, hw):
    """float32 output against prep_ref.interpolate64 for n in {1, 3, 4, 5, 301} (prefixes of one keypoint list: token centres,
    half a token outside, corners, far outside, the in/out boundary, random), strides 4 and 14, raw and normalised.

    Tolerance IF_TOL = 2e-6 of the largest magnitude of the wanted output (1 for the unit rows of the normalised form): the larger
    of (a) the project's existing 2e-6 (tests/test_oracle_golden.py, tests/test_entry_points_gpu.py) and (b) twice the largest
    float32-oracle-vs-float64 difference over these same inputs, 2 x 1.826e-07 = 3.7e-07, measured on the CPU in
    tests/test_prep.py::test_interpolate64_is_the_oracle_on_the_gpu_inputs.  Neither figure comes from the kernel.

    Exact: far-outside rows are all zeros (never NaN); raw output at a keypoint whose float32 grid coordinates are whole numbers
    is the token itself, bit for bit.  (p = s (j + 0.5) - 0.5 does not always give a whole float32 coordinate: the reference's
    normalise / unnormalise round trip leaves up to 1e-6 of a token on 9 x 13; those centres are held to the restatement,
    which forms the same coordinates; every grid and stride has centres that are exact, 35 of 117 at the fewest on 9 x 13.)  The three
    layouts give identical bytes, and half=True is the float32 result rounded once."""
    dev = _gpu()
    import torch
    from cppf2_amd import ops
    h, w = hw
    desc = PR.if_desc(C, h, w)
    layouts = _layouts(desc, dev)
    for s in PR.IF_STRIDES:
        pts, kind = PR.if_keypoints(h, w, s)
        ix, iy = PR.grid_coords(pts, h, w, s)
        whole = (kind == "centre") & (ix == np.floor(ix)) & (iy == np.floor(iy))
        assert whole.any() and (kind == "centre").sum() == h * w
        assert ((ix[whole] >= 0) & (ix[whole] <= w - 1) & (iy[whole] >= 0) & (iy[whole] <= h - 1)).all()
        p = torch.from_numpy(pts).to(dev)
        for norm in (False, True):
            want = PR.interpolate64(desc, pts, s, norm)
            for n in PR.IF_COUNTS:
                got = ops.interpolate_features(layouts[0], p[None, :n], strides=s, normalize=norm)
                assert got.shape == (1, C, n) and got.dtype == torch.float32
                g = got[0].T.contiguous().cpu().numpy()
                tag = (C, hw, s, norm, n)
                assert np.isfinite(g).all(), tag
                scale = 1.0 if norm else float(np.abs(want[:n]).max())
                err = float(np.abs(g - want[:n]).max()) / scale
                assert err <= IF_TOL, (tag, err)
                assert not g[kind[:n] == "far"].any(), tag
                if not norm:
                    k = np.flatnonzero(whole[:n])
                    token = desc[:, iy[k].astype(np.int64), ix[k].astype(np.int64)].T
                    assert g[k].tobytes() == np.ascontiguousarray(token).tobytes(), tag
                for other in layouts[1:]:
                    o = ops.interpolate_features(other, p[None, :n], strides=s, normalize=norm)
                    assert o[0].T.contiguous().cpu().numpy().tobytes() == g.tobytes(), tag
                hf = ops.interpolate_features(layouts[n % 3], p[None, :n], strides=s, normalize=norm, half=True)
                assert hf.dtype == torch.float16 and hf.shape == (1, C, n)
                assert torch.equal(hf.view(torch.int16), got.half().view(torch.int16)), tag


def test_interpolate_features_zero_map_and_channel_limit():
    """An all-zero map normalises to zeros (0 / eps, not 0 / 0); C = 4096 is the LDS limit and C = 4097 is refused."""
    dev = _gpu()
    import torch
    from cppf2_amd import ops
    from cppf2_amd._lib import CppfError
    pts, kind = PR.if_keypoints(9, 13, 14)
    p = torch.from_numpy(pts).to(dev)
    for C in (1, 65, 4096):
        z = ops.interpolate_features(torch.zeros((1, C, 9, 13), device=dev), p[None], strides=14, normalize=True)
        assert z.shape == (1, C, PR.IF_NMAX) and not z.cpu().numpy().view(np.uint32).any()
    with pytest.raises(CppfError):
        ops.interpolate_features(torch.zeros((1, 4097, 9, 13), device=dev), p[None], strides=14)
