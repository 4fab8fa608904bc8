"""GPU checks of cppf_grid_peaks (cppf_vote_center.hip) against the NumPy restatement (tests/grid_peaks_ref.py): every output array is
compared for exact equality (NaN-aware for the world coordinates of empty slots) on real vote grids written by cppf_vote_center
and on constructed grids; a scene's peaks do not depend on the batch; K = 1 is cppf_vote_center's own first maximum."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grid_peaks_ref as GR  # noqa: E402


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _peaks(grids, grid, grid_off, cells_cap, res, K, sep):
    """cppf_grid_peaks through ctypes on host arrays: grids GRID_DTYPE [B], grid uint32 (flat), grid_off int64 [B] or None."""
    import torch
    from cppf2_amd import _lib, ops
    dev = _gpu()
    L = _lib.load()
    B = len(grids)
    gt = torch.from_numpy(np.frombuffer(np.ascontiguousarray(grids).tobytes(), np.uint8).copy()).to(dev)
    gr = grid if torch.is_tensor(grid) else torch.from_numpy(np.ascontiguousarray(grid).view(np.int32)).to(dev)
    go = None if grid_off is None else (grid_off if torch.is_tensor(grid_off) else torch.from_numpy(np.asarray(grid_off, np.int64)).to(dev))
    pi = torch.full((B, K), -7, dtype=torch.int64, device=dev)
    pv = torch.full((B, K), -7, dtype=torch.int32, device=dev)
    pw = torch.full((B, K, 3), -7.0, dtype=torch.float64, device=dev)
    n = torch.full((B,), -7, dtype=torch.int32, device=dev)
    need = max(L.cppf_grid_peaks_workspace_bytes(B, K), 256)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    _lib.check(L.cppf_grid_peaks(B, ops._p(gt), ops._p(gr), ops._p(go), int(cells_cap), C.c_double(res), K, sep, ops._p(pi), ops._p(pv),
                                 ops._p(pw), ops._p(n), ops._p(ws), need, ops._stream()), "cppf_grid_peaks")
    return pi.cpu().numpy(), pv.cpu().numpy().view(np.uint32), pw.cpu().numpy(), n.cpu().numpy()


def _same(got, want):
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert np.array_equal(got[2], want[2], equal_nan=True)
    assert np.array_equal(np.isnan(got[2]), np.isnan(want[2]))
    assert np.array_equal(got[3], want[3])


def _check(grids, grid, grid_off, cells_cap, res, K, sep):
    got = _peaks(grids, grid, grid_off, cells_cap, res, K, sep)
    want = GR.grid_peaks_batch(grid.cpu().numpy() if hasattr(grid, "cpu") else grid,
                               grid_off.cpu().numpy() if hasattr(grid_off, "cpu") else grid_off, grids, cells_cap, res, K, sep)
    _same(got, want)
    return got


def _pack(cubes, c0s=None, pad=0):
    """Scenes given as [gx,gy,gz] uint32 arrays -> (grids, flat grid, offsets); `pad` unused cells (poisoned) between scenes, so
    that offsets are not multiples of four cells."""
    B = len(cubes)
    grids = np.zeros(B, GR.GRID_DTYPE)
    off, parts, o = [], [], 0
    for b, c in enumerate(cubes):
        grids["g"][b], grids["ncell"][b] = c.shape, c.size
        grids["c0"][b] = (0.25 * b, -0.5, 1.0 + b) if c0s is None else c0s[b]
        off.append(o)
        parts += [c.reshape(-1).astype(np.uint32), np.full(pad, 0xFFFFFFF0, np.uint32)]
        o += c.size + pad
    return grids, np.concatenate(parts), np.array(off, np.int64)


def _vote_grids(dev, Ns, Ts, R, mode, weighted, seed, res=2e-3, scenes=None, cells_cap=1 << 21):
    """Real vote grids: synthetic scenes with the teacher's logits, as the parity tests build them."""
    import torch
    from cppf2_amd import ops, synth
    from cppf2_amd.pipeline import VotingPipeline
    B = len(Ns)
    scs = scenes or [synth.make_scene(seed, b, n) for b, n in enumerate(Ns)]
    pts = torch.from_numpy(np.concatenate([s["pc"] for s in scs])).to(dev)
    idx = torch.cat([ops.sample_tuples(n, t, 5, seed, (b,)) for b, (n, t) in enumerate(zip(Ns, Ts))])
    lg = torch.cat([torch.from_numpy(synth.teacher_logits(s["pc_canon"], idx[sum(Ts[:b]):sum(Ts[:b + 1])].cpu().numpy(), 32))
                    for b, s in enumerate(scs)]).to(dev)
    u = torch.cat([ops.philox_uniform(t, 6, seed, 1, (b,)) for b, t in enumerate(Ts)])
    pipe = VotingPipeline(Ns, Ts, num_rots=R, vote_mode=mode, res=res, cells_cap=cells_cap)
    pipe.decode(pts, idx, lg, u)
    wt = None
    if weighted:
        g = torch.Generator().manual_seed(seed)
        wt = (torch.rand(sum(Ts), generator=g) * 4.0).to(dev)
    grid = torch.zeros(B * pipe.cells_cap, dtype=torch.int32, device=dev)
    goff = torch.arange(B, dtype=torch.int64, device=dev) * pipe.cells_cap
    pipe.vote_center(pts, idx, grid=grid, grid_off=goff, vote_wt=wt)
    grids = np.frombuffer(pipe.grids.cpu().numpy().tobytes(), GR.GRID_DTYPE).copy()
    return pipe, grids, grid, goff


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("weighted", [False, True])
def test_real_vote_grids_ragged_batch(mode, weighted):
    """A ragged batch of synthetic scenes in the LDS-slab / persistent mode and in the global-atomic mode, unweighted and with
    weighted votes: peaks at several K and separations, and K = 1 against cppf_vote_center's own outputs bit for bit."""
    dev = _gpu()
    Ns, Ts = [900, 2048, 300, 1500, 4096, 700, 1200], [4000, 9000, 1500, 6000, 12000, 2500, 5000]
    pipe, grids, grid, goff = _vote_grids(dev, Ns, Ts, 90, mode, weighted, 9)
    assert grids["ncell"].min() > 1000
    for K, sep in ((4, 10), (16, 3), (8, 0), (3, 40)):
        got = _check(grids, grid, goff, pipe.cells_cap, pipe.res, K, sep)
        assert got[3].max() > 1
    one = _check(grids, grid, goff, pipe.cells_cap, pipe.res, 1, 10)
    assert np.array_equal(one[0][:, 0], pipe.argmax.cpu().numpy())
    assert np.array_equal(one[1][:, 0], pipe.peak.cpu().numpy().view(np.uint32))
    assert one[2][:, 0].tobytes() == pipe.world.cpu().numpy().tobytes()
    # the wrapper gives the same
    pi, pv, pw, n = pipe.grid_peaks(grid, goff, 4, 10)
    _same((pi.cpu().numpy(), pv.cpu().numpy().view(np.uint32), pw.cpu().numpy(), n.cpu().numpy()),
          GR.grid_peaks_batch(grid.cpu().numpy(), goff.cpu().numpy(), grids, pipe.cells_cap, pipe.res, 4, 10))


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("weighted", [False, True])
def test_full_size_grid(mode, weighted):
    """One grid of about 1e6 cells (a 4096-point scene at a finer resolution), unweighted and with weighted votes: K = 1, 4, 16."""
    dev = _gpu()
    from cppf2_amd import synth
    sc = synth.make_scene(0, 0, 4096)
    ext = (sc["pc"].max(0) - sc["pc"].min(0)).astype(np.float64)
    res = float((np.prod(ext) / 1.0e6) ** (1.0 / 3.0))
    pipe, grids, grid, goff = _vote_grids(dev, [4096], [20000], 180, mode, weighted, 0, res=res, scenes=[sc])
    assert 7e5 < grids["ncell"][0] <= pipe.cells_cap
    for K, sep in ((1, 10), (4, 10), (16, 6)):
        got = _check(grids, grid, goff, pipe.cells_cap, pipe.res, K, sep)
    assert got[3][0] == 16
    assert np.array_equal(got[0][:, 0], pipe.argmax.cpu().numpy()) and got[2][:, 0].tobytes() == pipe.world.cpu().numpy().tobytes()


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("weighted", [False, True])
def test_example_cloud(mode, weighted):
    """The vote grid of tests/golden/example_data's cloud (back-projected, 2 mm voxel down-sample), a PCA frame standing in for
    its unknown pose as in test_reference_size_gpu."""
    import torch
    from PIL import Image
    from cppf2_amd import ops
    dev = _gpu()
    e = json.load(open(os.path.join(GOLDEN, "full_summary.json")))["example_backproject"]
    d = np.array(Image.open(os.path.join(GOLDEN, "example_data", "depth.png"))).astype(np.float64) / float(e["depth_scale"])
    m = np.array(Image.open(os.path.join(GOLDEN, "example_data", "mask.png")))
    m = (m[..., 0] if m.ndim == 3 else m) > 0
    pc_full, _ = ops.backproject(d, np.array(e["K"], dtype=np.float64), m, return_device=True)
    pc = pc_full[ops.downsample(pc_full, 2e-3, 0, return_device=True)].cpu().numpy()
    c = pc.astype(np.float64).mean(0)
    _, _, Vt = np.linalg.svd(pc.astype(np.float64) - c, full_matrices=False)
    diag = float(np.linalg.norm(2 * np.abs((pc - c) @ Vt.T).max(0)))
    canon = ((pc.astype(np.float64) - c) @ Vt.T / diag).astype(np.float32)
    N = len(pc)
    pipe, grids, grid, goff = _vote_grids(dev, [N], [20000], 180, mode, weighted, 3, scenes=[dict(pc=pc, pc_canon=canon)])
    for K, sep in ((1, 10), (8, 10), (16, 2)):
        got = _check(grids, grid, goff, pipe.cells_cap, pipe.res, K, sep)
    assert got[3][0] > 1
    assert np.array_equal(got[0][:, 0], pipe.argmax.cpu().numpy())
    assert np.array_equal(got[1][:, 0], pipe.peak.cpu().numpy().view(np.uint32))


def test_constructed_grids():
    _gpu()
    rng = np.random.default_rng(2)
    res = 2e-3
    # all zero; one non-zero cell; two equal maxima; degenerate shapes
    z = np.zeros((5, 6, 7), np.uint32)
    one = z.copy()
    one[4, 5, 6] = 3
    two = z.copy()
    two[3, 1, 2] = two[1, 4, 4] = 11
    line_z = rng.integers(0, 5, (1, 1, 37)).astype(np.uint32)
    line_x = rng.integers(0, 5, (37, 1, 1)).astype(np.uint32)
    unit0, unit1 = np.zeros((1, 1, 1), np.uint32), np.full((1, 1, 1), 8, np.uint32)
    # a peak on every face and every corner of the grid
    faces = np.zeros((9, 10, 11), np.uint32)
    for ax in range(3):
        for side in (0, -1):
            p = [4, 5, 5]
            p[ax] = side
            faces[tuple(p)] = 20 + 2 * ax - side
    corners = np.zeros((9, 10, 11), np.uint32)
    for cx in (0, -1):
        for cy in (0, -1):
            for cz in (0, -1):
                corners[cx, cy, cz] = 6
    cubes = [z, one, two, line_z, line_x, unit0, unit1, faces, corners, rng.integers(0, 3, (13, 7, 5)).astype(np.uint32)]
    for pad in (0, 1, 3):                                      # scene ranges at every alignment within 16 bytes
        grids, grid, off = _pack(cubes, pad=pad)
        for K, sep in ((1, 0), (1, 5), (16, 0), (16, 1), (16, 4), (7, 2), (16, 100)):
            got = _check(grids, grid, off, 1 << 12, res, K, sep)
        assert got[3].tolist()[:3] == [1, 1, 1]                # (sep = 100 covers the whole grid)
    got = _check(*_pack(cubes), 1 << 12, res, 16, 0)
    assert got[3][0] == 1 and got[0][0, 0] == 0 and got[1][0, 0] == 0
    assert got[3][1] == 1 and got[0][1, 0] == one.size - 1
    assert got[0][2, :2].tolist() == [int(np.ravel_multi_index((1, 4, 4), z.shape)), int(np.ravel_multi_index((3, 1, 2), z.shape))]
    assert got[3][7] == 6 and got[3][8] == 8
    # equal maxima exactly sep apart (suppressed) and sep + 1 apart (the next peak), along each axis and a diagonal
    cubes, expect = [], []
    for sep in (1, 4, 7):
        for step in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            for extra in (0, 1):
                c = np.zeros((14, 14, 14), np.uint32)
                a = np.array((2, 2, 2))
                c[tuple(a)] = c[tuple(a + np.array(step) * (sep + extra))] = 5
                cubes.append((sep, c))
                expect.append(1 + extra)
    for sep, c in ((7, None), (6, None)):                       # (2, 3, 6): squared length 49
        c = np.zeros((14, 14, 14), np.uint32)
        c[1, 1, 1] = c[3, 4, 7] = 2
        cubes.append((sep, c))
        expect.append(1 if sep == 7 else 2)
    for sep in (1, 4, 6, 7):
        sel = [i for i, (s, _) in enumerate(cubes) if s == sep]
        grids, grid, off = _pack([cubes[i][1] for i in sel])
        got = _check(grids, grid, off, 1 << 12, res, 2, sep)
        assert got[3].tolist() == [expect[i] for i in sel]


def test_scene_above_cells_cap_and_mixed_sizes():
    """A batch with different grid sizes per scene, one of them larger than cells_cap (the sentinel: index 0, value 0xFFFFFFFF,
    one peak) and one empty scene (ncell = 0)."""
    _gpu()
    rng = np.random.default_rng(8)
    cubes = [rng.integers(0, 9, s).astype(np.uint32) for s in ((3, 3, 3), (20, 21, 22), (8, 1, 40), (30, 30, 30), (2, 2, 2))]
    grids, grid, off = _pack(cubes, pad=2)
    cap = 20 * 21 * 22
    assert grids["ncell"][3] > cap
    grids["ncell"][4], grids["flags"][4] = 0, 1                 # an empty scene: no cells are read
    for K, sep in ((1, 3), (5, 3), (16, 6)):
        got = _check(grids, grid, off, cap, 2e-3, K, sep)
        assert got[0][3, 0] == 0 and got[1][3, 0] == GR.SENTINEL and got[3][3] == 1 and np.all(got[0][3, 1:] == -1)
        assert got[3][4] == 1 and got[1][4, 0] == 0


def test_peaks_do_not_depend_on_the_batch():
    """The same scene alone, in a batch of 64 and with the batch reversed: byte-identical rows."""
    dev = _gpu()
    B = 64
    Ns, Ts = [600 + 37 * (b % 9) for b in range(B)], [3000 + 211 * (b % 7) for b in range(B)]
    pipe, grids, grid, goff = _vote_grids(dev, Ns, Ts, 36, 0, False, 21, cells_cap=1 << 19)
    K, sep = 8, 10
    full = _check(grids, grid, goff, pipe.cells_cap, pipe.res, K, sep)
    assert full[3].max() > 1
    order = np.arange(B)[::-1].copy()
    rev = _peaks(grids[order], grid, goff.cpu().numpy()[order], pipe.cells_cap, pipe.res, K, sep)
    for a, b_ in zip(full, rev):
        assert a[order].tobytes() == b_.tobytes()
    for b in (0, 17, 63):
        alone = _peaks(grids[b:b + 1], grid, goff.cpu().numpy()[b:b + 1], pipe.cells_cap, pipe.res, K, sep)
        for a, o in zip(full, alone):
            assert a[b:b + 1].tobytes() == o.tobytes()


def test_argument_checks():
    import torch
    from cppf2_amd import _lib
    from cppf2_amd.pipeline import VotingPipeline
    dev = _gpu()
    L = _lib.load()
    assert L.cppf_grid_peaks_workspace_bytes(1, 0) == 0 and L.cppf_grid_peaks_workspace_bytes(1, 17) == 0
    assert L.cppf_grid_peaks_workspace_bytes(0, 4) == 0 and L.cppf_grid_peaks_workspace_bytes(64, 16) >= 64 * 16 * 8
    grids, grid, off = _pack([np.ones((2, 2, 2), np.uint32)])
    for K, sep in ((0, 1), (17, 1), (2, -1)):
        with pytest.raises(_lib.CppfError):
            _peaks(grids, grid, off, 64, 2e-3, K, sep)
    pipe = VotingPipeline([10], [10], num_rots=8)
    g = torch.zeros(pipe.cells_cap, dtype=torch.int32, device=dev)
    for K, sep in ((0, 1), (17, 1), (2, -1)):
        with pytest.raises(_lib.CppfError):
            pipe.grid_peaks(g, None, K, sep)
