"""CPU tests that pin the restatements of tests/prep_ref.py (back-projection, voxel down-sample, feature interpolation) to the
oracle and the reference's golden vectors, before tests/test_prep_gpu.py holds the kernels of cppf_prep.hip to them."""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prep_ref as PR  # noqa: E402
from oracle import cppf_oracle as O  # noqa: E402


def _example(full_summary):
    from PIL import Image
    e = full_summary["example_backproject"]
    d = np.array(Image.open(os.path.join(GOLDEN, "example_data", "depth.png"))).astype(np.float64) / e["depth_scale"]
    m = np.array(Image.open(os.path.join(GOLDEN, "example_data", "mask.png")))
    return e, d, (m[..., 0] if m.ndim == 3 else m) > 0


def _bp_inputs():
    """(shape, mask name, mask, depth32, depth64) for every shape and mask of the GPU file."""
    for shape in PR.BP_SHAPES:
        rng = np.random.default_rng(shape[0] * 10000 + shape[1])
        d32, d64, _ = PR.bp_depth(shape, rng)
        for name, m in PR.bp_masks(shape, rng).items():
            yield shape, name, m, d32, d64


def test_backproject64_is_the_oracle_on_the_example_scene(full_summary):
    """The elementwise restatement equals the oracle's matmul form bit for bit on the reference's example scene, whose float64
    array is pinned to the reference's by SHA; backproject32 is that array on float32 depth, negated back and cast."""
    e, d, m = _example(full_summary)
    assert np.array_equal(np.array(e["K"]), np.array(PR.EXAMPLE_K))
    got, (r, c) = PR.backproject64(d, e["K"], m)
    want, (rows, cols) = O.backproject(d, np.array(e["K"]), m)
    assert got.shape == (e["n"], 3) and got.tobytes() == want.tobytes()
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == e["sha"]
    assert np.array_equal(r, rows) and np.array_equal(c, cols)
    d32 = d.astype(np.float32)
    w2, _ = O.backproject(d32.astype(np.float64), np.array(e["K"]), m)
    w2[:, :2] = -w2[:, :2]
    got32, (r, c) = PR.backproject32(d32, e["K"], m)
    assert got32.dtype == np.float32 and got32.tobytes() == w2.astype(np.float32).tobytes()
    assert np.array_equal(r, rows) and np.array_equal(c, cols)


@pytest.mark.parametrize("kname", PR.ZERO_SKEW)
def test_backproject64_is_the_oracle_for_intrinsics_without_skew(kname):
    """Without skew one product of each ray coordinate is by 0 and one by 1, so a matmul that fuses or reorders them rounds as
    the written order does: bit-identical on every shape, mask and depth of the GPU file (NaN, inf and subnormal depth never
    pass depth > 0 except the subnormal, whose products are exact or underflow alike)."""
    K = PR.INTRINSICS[kname]
    n = 0
    for shape, name, m, d32, d64 in _bp_inputs():
        got, (r, c) = PR.backproject64(d64, K, m)
        with np.errstate(all="ignore"):
            want, (rows, cols) = O.backproject(d64, np.array(K), m)
        assert got.tobytes() == want.tobytes(), (shape, name)
        assert np.array_equal(r, rows) and np.array_equal(c, cols)
        rr, cc = np.nonzero((m != 0) & np.nan_to_num(d64 > 0))
        assert np.array_equal(r, rr) and np.array_equal(c, cc)
        n += len(r)
    assert n > 20000


def test_backproject64_with_skew_is_reported_not_asserted():
    """With the skewed K (0.7) the written order (k0*u + k1*v) + k2 has two inexact products, and NumPy's matmul is free to fuse
    one of them.  Measured on the development CPU (x86-64, OpenBLAS): they do NOT agree.  Of the 23 112 points of the eight
    full masks, 1 differs from the oracle's matmul form, and of the 307 200 of a full 480 x 640 image, 160 do -- each by one unit
    in the last place of x (the row of inv(K) that holds the skew term); y and z never differ.  So cppf_backproject64's claim
    of NumPy's array bit for bit holds for intrinsics without skew only.  Nothing is asserted about
    the matmul here -- another BLAS may round differently; the figures are printed.  What is asserted: the two forms agree to
    4 ulp, i.e. the restatement is the same quantity."""
    K = PR.INTRINSICS["skew"]
    differing = total = 0
    worst = 0.0
    for shape, name, m, d32, d64 in _bp_inputs():
        if name != "full":
            continue
        got, _ = PR.backproject64(d64, K, m)
        with np.errstate(all="ignore"):
            want, _ = O.backproject(d64, np.array(K), m)
        ne = got != want
        differing += int(ne.any(1).sum())
        total += len(got)
        if ne.any():
            worst = max(worst, float((np.abs(got - want)[ne] / np.spacing(np.abs(want[ne]))).max()))
    print("skewed K: %d of %d points differ from the matmul form, worst %.1f ulp" % (differing, total, worst))
    assert total > 20000 and worst <= 4.0


def _rank_screen(pc, res, picks):
    """The uniformity screen of test_entry_points_gpu.py:520-536: u = (rank of the kept point in its voxel + 0.5) / voxel size over
    the voxels of four or more points; returns (number of such voxels, mean u, share of u < 0.25)."""
    key = np.floor((pc - pc.min(0)) / np.float32(res)).astype(np.int64)
    flat = (key[:, 0] << 42) | (key[:, 1] << 21) | key[:, 2]
    order = np.argsort(flat, kind="stable")
    sf = flat[order]
    starts = np.flatnonzero(np.r_[True, sf[1:] != sf[:-1]])
    cnt = np.diff(np.r_[starts, len(sf)])
    rank_of = np.empty(len(pc), np.int64)
    rank_of[order] = np.arange(len(pc)) - np.repeat(starts, cnt)
    cnt_of = np.empty(len(pc), np.int64)
    cnt_of[order] = np.repeat(cnt, cnt)
    u = []
    for k in picks:
        k = k[cnt_of[k] >= 4]
        u.append((rank_of[k] + 0.5) / cnt_of[k])
    u = np.concatenate(u)
    return int((cnt >= 4).sum()), float(u.mean()), float((u < 0.25).mean())


def test_downsample_exact_on_the_example_cloud(full_summary):
    """One index per voxel, as many voxels as the oracle's down-sample, reproducible, the high seed word matters, and the pick
    is uniform within the voxel (same screen and bounds as the kernel's test)."""
    e, d, m = _example(full_summary)
    pc, _ = PR.backproject32(d.astype(np.float32), e["K"], m)
    res = 0.004
    key = np.floor((pc - pc.min(0)) / np.float32(res)).astype(np.int64)
    a = PR.downsample_exact(pc, res, 5)
    assert a.dtype == np.int64 and np.all(np.diff(a) > 0)
    assert len(np.unique(key[a], axis=0)) == len(a) == len(np.unique(key, axis=0))            # exactly one per occupied voxel
    assert len(a) == len(O.downsample(pc, res, np.random.RandomState(0)))
    assert np.array_equal(a, PR.downsample_exact(pc, res, 5))
    b = PR.downsample_exact(pc, res, 2 ** 32 + 5)
    assert len(b) == len(a) and not np.array_equal(a, b)
    assert not np.array_equal(a, PR.downsample_exact(pc, res, 6))
    nbig, mean, low = _rank_screen(pc, res, [PR.downsample_exact(pc, res, 100 + s) for s in range(8)])
    print("uniformity: %d voxels of >= 4 points, mean %.4f, share below 0.25 %.4f" % (nbig, mean, low))
    assert nbig > 100 and abs(mean - 0.5) < 0.02 and abs(low - 0.25) < 0.03
    assert len(PR.downsample_exact(np.zeros((0, 3), np.float32), res, 0)) == 0


def test_downsample_exact_by_hand():
    """Four points, two voxels: the kept point of each voxel is the one with the smaller Philox word 0 (the index breaks ties),
    worked out here one point at a time."""
    pc = np.array([[0, 0, 0], [0.5, 0.5, 0.5], [1.5, 0, 0], [1.25, 0.5, 0.75]], np.float32)
    for seed in PR.DS_SEEDS:
        w = [int(O.philox4x32(i, 0, 0, 7, seed & 0xFFFFFFFF, seed >> 32)[0]) for i in range(4)]
        want = sorted([min((0, 1), key=lambda i: (w[i], i)), min((2, 3), key=lambda i: (w[i], i))])
        assert list(PR.downsample_exact(pc, 1.0, seed)) == want
    # the lattice clouds of the GPU file have the voxel structure their names promise
    rng = np.random.default_rng(1)
    for n in PR.DS_COUNTS:
        pc, res = PR.ds_own_voxel(n, rng)
        assert len(pc) == n and np.array_equal(PR.downsample_exact(pc, res, 3), np.arange(n))
        pc, res = PR.ds_five_per_voxel(n, rng)
        assert len(pc) == n and len(PR.downsample_exact(pc, res, 3)) == max(1, n // 5)
    for name, (pc, res) in PR.ds_geometry(rng).items():
        k = PR.downsample_exact(pc, res, 3)
        assert 0 < len(k) <= len(pc)
        if name.startswith("field"):
            assert len(k) == 6
            ax = "xyz".index(name[-1])
            idx = np.sort(np.floor((pc[:, ax] - pc[:, ax].min()) / np.float32(res)).astype(np.int64))
            assert list(idx) == [0, 1, 2 ** 20, 2 ** 21 - 3, 2 ** 21 - 2, 2 ** 21 - 1]


def test_interpolate64_matches_the_reference_golden():
    """dataset.py:40-59's own output (tests/golden/dino_interp.npz) within the project's 2e-6, raw and normalised."""
    g = np.load(os.path.join(GOLDEN, "dino_interp.npz"))
    for name, norm in (("normalized", True), ("raw", False)):
        got = PR.interpolate64(g["desc"], g["pts"], int(g["stride"]), norm)
        assert got.dtype == np.float64 and got.shape == g[name].shape
        assert np.abs(got - g[name]).max() < 2e-6, name


def test_interpolate64_is_the_oracle_on_the_gpu_inputs():
    """interpolate64 against the float32 oracle on every input of the GPU file (6 channel counts x 4 grids x 2 strides, 301
    keypoints, raw and normalised; the smaller keypoint counts are prefixes of the 301).  The difference, relative to the
    largest magnitude of the wanted output, is float32 rounding of four products, three sums and, normalised, a C-term sum of
    squares: measured on the development CPU it is 1.826e-07 (prep_ref.ORACLE_VS_F64, which the tolerance of
    tests/test_prep_gpu.py is derived from).  Asserted here: below 1e-6, so that twice the difference stays below the
    project's 2e-6 on any CPU and the choice between the two does not depend on the machine."""
    worst = 0.0
    for C in PR.IF_CHANNELS:
        for h, w in PR.IF_GRIDS:
            desc = PR.if_desc(C, h, w)
            for s in PR.IF_STRIDES:
                pts, kind = PR.if_keypoints(h, w, s)
                assert len(pts) == PR.IF_NMAX and list(kind[:5]) == ["centre", "half", "corner", "far", "random"]
                for norm in (False, True):
                    want = PR.interpolate64(desc, pts, s, norm)
                    got = O.interpolate_features(desc, pts, s, norm)
                    assert np.isfinite(want).all() and not want[kind == "far"].any()
                    worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print("largest float32-oracle-vs-float64 difference: %.3e" % worst)
    assert worst < 1e-6
