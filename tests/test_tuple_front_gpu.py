"""The tuple front end (cppf2_amd/csrc/cppf_core.hip up to encode_dino_kernel) against the plain host restatement of
tests/tuple_front_ref.py on ragged batches, bit for bit: every float output is compared through its uint32 / uint16 view.  The one
positions-only comparison is the NaN the normal cosine COMPUTES from a NaN normal (and the NaN a cast produces from a NaN).
tests/test_tuple_front_ref.py pins the restatement and checks on the CPU that these inputs tell a wrong kernel from a right one.

Which test launches which kernel:
  sample_tuples_kernel                      test_sampler_on_ragged_batches
  philox_uniform_kernel                     test_uniforms_on_ragged_batches
  nan_to_zero_kernel                        test_nan_to_zero_past_its_grid_cap
  cast_f16_kernel                           test_cast_f16_rounds_like_numpy
  scene_bounds_kernel                       test_scene_bounds_placements, test_scene_bounds_decisions
  encode_shot_kernel<5, 16>                 test_shot_rows_ragged[5-64], test_shot_rows_past_the_grid_cap
  encode_shot_kernel<0, 0>                  test_shot_rows_ragged (every other shape)
  encode_shot_f16_kernel                    test_shot_rows_from_a_half_table, test_half_rows_past_the_grid_cap
  encode_shot_heads_tile_kernel<5, false>   test_shot_heads_ragged[5], test_heads_into_wider_rows[5]
  encode_shot_heads_kernel<0>               test_shot_heads_ragged (k != 5), test_heads_into_wider_rows[3], test_heads_past_the_grid_cap
  encode_shot_heads_tile_kernel<5, true>    test_coord_heads_ragged[5], test_heads_into_wider_rows[5]
  encode_coord_heads_kernel                 test_coord_heads_ragged (k != 5), test_heads_into_wider_rows[3], test_heads_past_the_grid_cap
  encode_coord_kernel                       test_coord_rows_ragged, test_coord_rows_past_the_grid_cap
  encode_dino_kernel                        test_dino_rows_ragged, test_dino_rows_past_the_grid_cap
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tuple_front_ref as TR  # noqa: E402

SENT = -842150451            # 0xCDCDCDCD in every word of an output buffer before the call
GUARD = 8                    # sentinel rows before and after the rows an entry point may write
SEED = 0xFEDCBA9876543210    # both halves non-zero
SID_BASE, SID_STRIDE = 7, 3  # scene ids 7, 10, 13, ...


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_gpu())


def _words(rows, cols):
    """An int32 buffer of GUARD + rows + GUARD rows filled with the sentinel, and the pointer to row GUARD."""
    import torch
    buf = torch.full((rows + 2 * GUARD, cols), SENT, dtype=torch.int32, device=_gpu())
    return buf, C.c_void_p(buf.data_ptr() + 4 * GUARD * cols)


def _guards_untouched(buf):
    h = buf.cpu().numpy()
    assert np.all(h[:GUARD] == SENT) and np.all(h[-GUARD:] == SENT), "rows outside the output were written"
    return h[GUARD:-GUARD]


def _same(got, want, off=None, computed_nan=None):
    """Bit equality; `computed_nan`: columns in which a NaN of the restatement only has to be a NaN (any sign, any payload)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    gb, wb = TR.bits(got).copy(), TR.bits(want).copy()
    if computed_nan is not None:
        m = np.zeros(want.shape, bool)
        m[:, computed_nan] = np.isnan(want[:, computed_nan])
        assert m.any() and np.all(np.isnan(got[m])), "a computed NaN is missing"
        gb[m] = wb[m] = 0
    bad = np.argwhere(gb != wb)
    if bad.size:
        r, c = (int(bad[0][0]), int(bad[0][1])) if bad.shape[1] > 1 else (int(bad[0][0]), 0)
        scene = "" if off is None else " (scene %d)" % (np.searchsorted(np.asarray(off), r, side="right") - 1)
        raise AssertionError("%d values differ; first at row %d%s column %d: got %r (0x%x), want %r (0x%x)" % (
            len(bad), r, scene, c, got.reshape(got.shape[0], -1)[r, c], gb.reshape(got.shape[0], -1)[r, c],
            want.reshape(got.shape[0], -1)[r, c], wb.reshape(got.shape[0], -1)[r, c]))


_BATCH = {}


def _batch(k, F=None, D=None):
    """The ragged batch and its restatement, computed once per shape."""
    key = (k, F, D)
    if key not in _BATCH:
        d = TR.ragged_batch(k, F=F, D=D)
        if k >= 2:
            d["ref"] = TR.encode_batch(d["pts"], d["normals"], d["feat"], d["idx"], d["pt_off"], d["tup_off"], k)
        _BATCH[key] = d
    d = _BATCH[key]
    return d, _dev(d["pt_off"]), _dev(d["tup_off"])


def _one_scene(n, T, k, seed):
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, n, (T, k)).astype(np.int32)
    idx[0, 0], idx[-1, k - 1] = 0, n - 1
    return rng, rng.rand(n, 3).astype(np.float32), rng.randn(n, 3).astype(np.float32), idx, TR.offsets([n]), TR.offsets([T])


# ---------------------------------------------------------------------------------------------------------------
# the six encoders on the ragged batch
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,F", [(5, 64), (2, 4), (3, 8), (8, 16), (2, 352)])
def test_shot_rows_ragged(k, F):
    """(5, 64) is the compile-time instance, the others the run-time kernel; at k = 2 the head of a tuple is one float4, so the
    wavefront at the head / feature boundary runs both kinds of item (n_head = 3770, no multiple of 64)."""
    from cppf2_amd import ops
    d, pt_off, tup_off = _batch(k, F=F)
    got = ops.encode_tuples_shot(d["pts"], d["idx"], d["feat"], d["normals"], pt_off=pt_off, tup_off=tup_off).cpu().numpy()
    _same(got, d["ref"]["rows"], d["tup_off"], computed_nan=slice(TR.coord_cols(k), TR.head_cols(k)))


@pytest.mark.parametrize("F", [8, 64])
def test_shot_rows_from_a_half_table(F):
    """The float16 table form: rows equal to the float32 rows of the widened table, -0, subnormals, inf and NaN halves included."""
    import torch
    from cppf2_amd import ops
    k = 5
    d, pt_off, tup_off = _batch(k)
    table = TR.half_table(d["pts"].shape[0], F)
    want = TR.encode_batch(d["pts"], d["normals"], table.astype(np.float32), d["idx"], d["pt_off"], d["tup_off"], k)["rows"]
    got = ops.encode_tuples_shot(d["pts"], d["idx"], torch.from_numpy(table).to(_gpu()), d["normals"], pt_off=pt_off, tup_off=tup_off)
    _same(got.cpu().numpy(), want, d["tup_off"], computed_nan=slice(TR.coord_cols(k), TR.head_cols(k)))


@pytest.mark.parametrize("k", range(2, 9))
def test_shot_heads_ragged(k):
    from cppf2_amd import ops
    d, pt_off, tup_off = _batch(k)
    heads, gidx = ops.encode_tuples_shot_heads(d["pts"], d["idx"], d["normals"], pt_off=pt_off, tup_off=tup_off)
    _same(gidx.cpu().numpy(), d["ref"]["gidx"], d["tup_off"])
    _same(heads.cpu().numpy(), d["ref"]["heads"], d["tup_off"], computed_nan=slice(TR.coord_cols(k), TR.head_cols(k)))


@pytest.mark.parametrize("k", range(2, 9))
def test_coord_heads_ragged(k):
    from cppf2_amd import ops
    d, pt_off, tup_off = _batch(k)
    heads, gidx = ops.encode_tuples_coord_heads(d["pts"], d["idx"], pt_off=pt_off, tup_off=tup_off)
    _same(gidx.cpu().numpy(), d["ref"]["gidx"], d["tup_off"])
    _same(heads.cpu().numpy(), d["ref"]["cheads"], d["tup_off"])           # the zero padding included: +0 in every bit


@pytest.mark.parametrize("k", [3, 5])
def test_heads_into_wider_rows(k):
    """Both head entry points through the C ABI with ld_heads wider than the block: the columns past the block and the guard
    rows keep the sentinel."""
    from cppf2_amd import _lib, ops
    d, pt_off, tup_off = _batch(k)
    T, B = d["idx"].shape[0], len(d["pt_off"]) - 1
    pts, nrm, idx = _dev(d["pts"]), _dev(d["normals"]), _dev(d["idx"])
    for name, ncol in (("heads", TR.head_cols(k)), ("cheads", TR.coord_head_cols(k))):
        ld = ncol + 12
        hbuf, hp = _words(T, ld)
        gbuf, gp = _words(T, k)
        if name == "heads":
            st = ops._L.cppf_encode_tuples_shot_heads(B, ops._p(pts), ops._p(nrm), ops._p(idx), k, ops._p(pt_off), ops._p(tup_off), T, hp,
                                                      ld, gp, ops._stream())
        else:
            st = ops._L.cppf_encode_tuples_coord_heads(B, ops._p(pts), ops._p(idx), k, ops._p(pt_off), ops._p(tup_off), T, hp, ld, gp,
                                                       ops._stream())
        _lib.check(st, name)
        h, g = _guards_untouched(hbuf), _guards_untouched(gbuf)
        assert np.all(h[:, ncol:] == SENT), "columns past the head block were written"
        _same(g, d["ref"]["gidx"], d["tup_off"])
        _same(np.ascontiguousarray(h[:, :ncol]).view(np.float32), d["ref"][name], d["tup_off"],
              computed_nan=slice(TR.coord_cols(k), TR.head_cols(k)) if name == "heads" else None)


@pytest.mark.parametrize("k", [2, 5, 8])
def test_coord_rows_ragged(k):
    """encode_coord_kernel finds the scene of every flat row itself (find_scene over the empty scenes' duplicate offsets); written
    into the leading columns of a wider row."""
    import torch
    from cppf2_amd import ops
    d, pt_off, tup_off = _batch(k)
    T, ncol = d["idx"].shape[0], TR.coord_cols(k)
    out = torch.full((T, ncol + 7), SENT, dtype=torch.int32, device=_gpu())
    ops.encode_tuples_coord(d["pts"], d["idx"], out=out.view(torch.float32), pt_off=pt_off, tup_off=tup_off)
    o = out.cpu().numpy()
    assert np.all(o[:, ncol:] == SENT)
    _same(np.ascontiguousarray(o[:, :ncol]).view(np.float32), d["ref"]["coord"], d["tup_off"])
    got = ops.encode_tuples_coord(d["pts"], d["idx"], pt_off=pt_off, tup_off=tup_off).cpu().numpy()
    _same(got, d["ref"]["coord"], d["tup_off"])


@pytest.mark.parametrize("D", [4, 64, 256])
@pytest.mark.parametrize("k", [1, 5, 8])
def test_dino_rows_ragged(k, D):
    """An in-order float32 gather-add: equal to the host loop bit for bit, with and without a bias, at out_col 0 and 30."""
    import torch
    from cppf2_amd import ops
    d, pt_off, tup_off = _batch(k, D=D)
    T = d["idx"].shape[0]
    gidx = TR.global_indices(d["idx"], d["pt_off"], d["tup_off"]).astype(np.int64)
    tables = _dev(d["tables"])
    for bias in (d["bias"], None):
        want = TR.dino_rows(d["tables"], bias, gidx)
        for out_col in (0, 30):
            out = torch.full((T, out_col + D + 3), SENT, dtype=torch.int32, device=_gpu())
            ops.encode_tuples_dino(tables, bias, d["idx"], out.view(torch.float32), out_col, pt_off=pt_off, tup_off=tup_off)
            o = out.cpu().numpy()
            assert np.all(o[:, :out_col] == SENT) and np.all(o[:, out_col + D:] == SENT)
            _same(np.ascontiguousarray(o[:, out_col:out_col + D]).view(np.float32), want, d["tup_off"])


# ---------------------------------------------------------------------------------------------------------------
# past the grid caps: one scene each, a tuple count that is no multiple of 256
# ---------------------------------------------------------------------------------------------------------------
def test_shot_rows_past_the_grid_cap():
    """cppf_encode_tuples_shot launches min(ceil(items / 256), 4096) workgroups per scene, items = T (C(k,2) + k F / 4).  k = 5,
    F = 64: 90 items per tuple, 4096 * 256 / 90 = 11650.8, so from 11651 tuples on the grid-stride loop serves the rest; 13001
    tuples (50 * 256 + 201) = 1 170 090 items, 121 514 of them in the second pass.  Output 18.7 MB."""
    from cppf2_amd import ops
    k, F, T = 5, 64, 13001
    assert T * (10 + k * F // 4) > 4096 * 256 and T % 256
    rng, pts, nrm, idx, pt_off, tup_off = _one_scene(509, T, k, 1)
    feat = rng.randn(509, F).astype(np.float32)
    got = ops.encode_tuples_shot(pts, idx, feat, nrm, pt_off=_dev(pt_off), tup_off=_dev(tup_off)).cpu().numpy()
    _same(got, TR.encode_batch(pts, nrm, feat, idx, pt_off, tup_off, k)["rows"])


def test_half_rows_past_the_grid_cap():
    """The float16 kernel's items are 8 halves wide: 10 + 5 * 8 = 50 per tuple at k = 5, F = 64; 4096 * 256 / 50 = 20971.5, so the
    cap binds from 20972 tuples on; 23003 (89 * 256 + 219) = 1 150 150 items.  Output 33 MB."""
    import torch
    from cppf2_amd import ops
    k, F, T = 5, 64, 23003
    assert T * (10 + k * F // 8) > 4096 * 256 and T % 256
    rng, pts, nrm, idx, pt_off, tup_off = _one_scene(509, T, k, 2)
    table = TR.half_table(509, F, seed=1)
    got = ops.encode_tuples_shot(pts, idx, torch.from_numpy(table).to(_gpu()), nrm, pt_off=_dev(pt_off), tup_off=_dev(tup_off))
    _same(got.cpu().numpy(), TR.encode_batch(pts, nrm, table.astype(np.float32), idx, pt_off, tup_off, k)["rows"])


def test_heads_past_the_grid_cap():
    """The head kernels run one thread per tuple in min(ceil(T / 256), 4096) workgroups: the cap binds from 4096 * 256 + 1 tuples on.
    k = 2 keeps that affordable: T = 4096 * 256 + 257 rows of 4 (heads) / 8 (coordinate heads) floats, 16.8 / 33.6 MB.  (k = 5, the
    tile kernel, would need 168 MB of heads at its cap.)"""
    from cppf2_amd import ops
    k, T = 2, 4096 * 256 + 257
    assert (T + 255) // 256 > 4096 and T % 256
    rng, pts, nrm, idx, pt_off, tup_off = _one_scene(509, T, k, 3)
    ref = TR.encode_batch(pts, nrm, None, idx, pt_off, tup_off, k)
    po, to = _dev(pt_off), _dev(tup_off)
    heads, gidx = ops.encode_tuples_shot_heads(pts, idx, nrm, pt_off=po, tup_off=to)
    _same(gidx.cpu().numpy(), ref["gidx"])
    _same(heads.cpu().numpy(), ref["heads"])
    heads, gidx = ops.encode_tuples_coord_heads(pts, idx, pt_off=po, tup_off=to)
    _same(gidx.cpu().numpy(), ref["gidx"])
    _same(heads.cpu().numpy(), ref["cheads"])


def test_coord_rows_past_the_grid_cap():
    """cppf_encode_tuples_coord launches min(ceil(T * 3 C(k,2) / 256), 256 * 64) workgroups: 16384 * 256 = 4 194 304 items; k = 8 has
    84 per tuple, 4 194 304 / 84 = 49932.2, so the cap binds from 49933 tuples on; 50001 (195 * 256 + 81).  Output 16.8 MB."""
    from cppf2_amd import ops
    k, T = 8, 50001
    assert T * TR.coord_cols(k) > 16384 * 256 and T % 256
    rng, pts, nrm, idx, pt_off, tup_off = _one_scene(509, T, k, 4)
    got = ops.encode_tuples_coord(pts, idx, pt_off=_dev(pt_off), tup_off=_dev(tup_off)).cpu().numpy()
    _same(got, TR.encode_batch(pts, nrm, None, idx, pt_off, tup_off, k)["coord"])


def test_dino_rows_past_the_grid_cap():
    """cppf_encode_tuples_dino launches min(ceil(T * D / 4 / 256), 256 * 64) workgroups; D = 256 has 64 items per tuple, so the cap
    binds from 65537 tuples on; 66001 (257 * 256 + 209) tuples of k = 2.  Output 67.6 MB."""
    import torch
    from cppf2_amd import ops
    k, D, T, n = 2, 256, 66001, 67
    assert T * (D // 4) > 16384 * 256 and T % 256
    rng, pts, nrm, idx, pt_off, tup_off = _one_scene(n, T, k, 5)
    tables, bias = rng.randn(n, k, D).astype(np.float32), rng.randn(D).astype(np.float32)
    out = torch.empty((T, D), dtype=torch.float32, device=_gpu())
    ops.encode_tuples_dino(tables, bias, idx, out, 0, pt_off=_dev(pt_off), tup_off=_dev(tup_off))
    _same(out.cpu().numpy(), TR.dino_rows(tables, bias, idx.astype(np.int64)))


# ---------------------------------------------------------------------------------------------------------------
# sampler and uniforms through the ABI, ragged
# ---------------------------------------------------------------------------------------------------------------
# (point counts, tuple counts): the ragged batch with every tile shape of the 256-row LDS staging; its last scene holds the most
# points pt_off (int32) can still express there.  The second batch is the largest n of all, 2^31 - 1, which needs pt_off[b] = 0.
SAMPLER_BATCHES = [([1, 1, 2, 257, 50000, 2 ** 31 - 1 - 50261], [0, 1, 255, 256, 257, 1000]), ([2 ** 31 - 1], [1000])]
MAX_T = 300                  # smaller than the longest scene (1000): two workgroups per scene, the grid-stride loop serves the rest


@pytest.mark.parametrize("k", range(2, 9))
def test_sampler_on_ragged_batches(k):
    from cppf2_amd import _lib, ops
    for pt_counts, tup_counts in SAMPLER_BATCHES:
        pt_off, tup_off = TR.offsets(pt_counts), TR.offsets(tup_counts)
        T = int(tup_off[-1])
        buf, p = _words(T, k)
        d_pt, d_tup = _dev(pt_off), _dev(tup_off)                   # (named: they must outlive the launch)
        _lib.check(ops._L.cppf_sample_tuples(len(pt_counts), ops._p(d_pt), ops._p(d_tup), MAX_T, k, C.c_uint64(SEED), SID_BASE,
                                             SID_STRIDE, p, ops._stream()), "cppf_sample_tuples")
        got = _guards_untouched(buf)
        _same(got, TR.sample_batch(pt_counts, tup_counts, k, SEED, SID_BASE, SID_STRIDE), tup_off)
        for b, t0, t1 in TR.scene_slices(tup_off):
            assert got[t0:t1].min() >= 0 and got[t0:t1].max() < pt_counts[b]
        assert got[tup_off[-2]:].max() > 2 ** 30                    # the last scene really draws from the whole 31-bit range


@pytest.mark.parametrize("stream_id", [1, 0x12345678])
@pytest.mark.parametrize("m", range(1, 9))
def test_uniforms_on_ragged_batches(m, stream_id):
    from cppf2_amd import _lib, ops
    tup_counts = SAMPLER_BATCHES[0][1]
    tup_off = TR.offsets(tup_counts)
    T = int(tup_off[-1])
    buf, p = _words(T, m)
    d_tup = _dev(tup_off)
    _lib.check(ops._L.cppf_philox_uniform(len(tup_counts), ops._p(d_tup), MAX_T, m, C.c_uint64(SEED), SID_BASE, SID_STRIDE, stream_id,
                                          p, ops._stream()), "cppf_philox_uniform")
    got = _guards_untouched(buf).view(np.float32)
    _same(got, TR.uniform_batch(tup_counts, m, SEED, SID_BASE, SID_STRIDE, stream_id), tup_off)
    assert got.min() >= 0.0 and got.max() < 1.0


# ---------------------------------------------------------------------------------------------------------------
# cast_f16 and nan_to_zero
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 16384 * 256 + 257])
def test_cast_f16_rounds_like_numpy(n):
    """Round to nearest even at exact ties of both parities, just beside them, at the overflow tie 65520, in the subnormals and
    at +-0 / +-inf; the last size is 257 values past the 16384-workgroup cap, and its tail holds every special value."""
    import torch
    from cppf2_amd import _lib, ops
    x = TR.tiled(TR.cast_inputs(), n)
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    buf = torch.full((n + 2 * GUARD,), -12851, dtype=torch.int16, device=_gpu())           # 0xCDCD
    d_x = _dev(x)
    _lib.check(ops._L.cppf_cast_f16(ops._p(d_x), C.c_void_p(buf.data_ptr() + 2 * GUARD), n, ops._stream()), "cppf_cast_f16")
    h = buf.cpu().numpy()
    assert np.all(h[:GUARD] == -12851) and np.all(h[-GUARD:] == -12851)
    got = np.ascontiguousarray(h[GUARD:-GUARD]).view(np.float16)
    nan = np.isnan(x)
    assert np.array_equal(np.isnan(got), nan)                                               # a NaN the cast computes: positions only
    assert np.array_equal(TR.bits(got)[~nan], TR.bits(want)[~nan])


def test_nan_to_zero_past_its_grid_cap():
    """8192 * 256 + 257 values: 257 past the 8192-workgroup cap, NaNs of both signs in that tail; inf and -0.0 stay as they are."""
    import torch
    from cppf2_amd import _lib, ops
    n = 8192 * 256 + 257
    rng = np.random.RandomState(9)
    x = rng.randn(n).astype(np.float32)
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45], dtype=np.float32)
    x[rng.choice(n - 257, 4000, replace=False)] = np.resize(special, 4000)
    x[n - 257::8], x[n - 1], x[n - 2], x[n - 3] = np.nan, -np.nan, -0.0, np.inf
    xb = TR.bits(x)
    want = np.where(np.isnan(x), np.uint32(0), xb)
    assert (want != xb).sum() > 1000 and np.isnan(x[n - 257:]).sum() > 30
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device=_gpu())
    buf[GUARD:GUARD + n] = _dev(xb.view(np.int32))
    _lib.check(ops._L.cppf_nan_to_zero(C.c_void_p(buf.data_ptr() + 4 * GUARD), n, ops._stream()), "cppf_nan_to_zero")
    h = buf.cpu().numpy()
    assert np.all(h[:GUARD] == SENT) and np.all(h[-GUARD:] == SENT)
    assert np.array_equal(h[GUARD:-GUARD].view(np.uint32), want)


# ---------------------------------------------------------------------------------------------------------------
# cppf_scene_bounds alone
# ---------------------------------------------------------------------------------------------------------------
def _scene_bounds(pts, pt_off, res):
    """The C entry point with GUARD sentinel records before and after: structured array of the B records."""
    import torch
    from cppf2_amd import _lib, ops
    B = len(pt_off) - 1
    buf = torch.full((B + 2 * GUARD, 8), SENT, dtype=torch.int32, device=_gpu())
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    dpts = _dev(pts if pts.size else np.zeros((1, 3), np.float32))
    d_off = _dev(pt_off)
    _lib.check(ops._L.cppf_scene_bounds(B, ops._p(dpts), ops._p(d_off), C.c_float(res), C.c_void_p(buf.data_ptr() + 32 * GUARD),
                                        ops._stream()), "cppf_scene_bounds")
    return np.ascontiguousarray(_guards_untouched(buf)).view(TR.GRID_DTYPE).reshape(B)


def _same_grids(got, want, names):
    for i, s in enumerate(names):
        assert got[i].tobytes() == want[i].tobytes(), "scene %s: got %r, want %r" % (s, got[i], want[i])


@pytest.mark.parametrize("kind", ["min", "max"])
@pytest.mark.parametrize("place", ["first", "last", "p64"])
def test_scene_bounds_placements(place, kind):
    """Scenes of 0 .. 1025 points in one batch, negative coordinates; the extreme of every axis at the first point, the last point
    (the tail of the 256-strided loop) and point 64 (the wavefront edge)."""
    pts, pt_off = TR.bounds_batch(place, kind)
    got = _scene_bounds(pts, pt_off, TR.BOUNDS_RES)
    _same_grids(got, TR.scene_grids(pts, pt_off, TR.BOUNDS_RES), TR.BOUNDS_SIZES)
    assert np.all(got["ncell"][1:] > 0) and got["flags"][0] == 1 and not got["flags"][1:].any()


@pytest.mark.parametrize("name", ["exact", "wide"])
def test_scene_bounds_decisions(name):
    """Quotients that are exactly an integer and one ulp below; and the rule of include/cppf_hip.h for grids int32 cannot hold: a
    cell product above 2^31 - 1 keeps g and reports ncell = 0 with bit 1; a quotient of 2e9 or more, an infinite extent or an axis
    without a finite coordinate report bit 1, g = 0 and ncell = 0.  (tests/test_tuple_front_ref.py pins the expected records.)"""
    pts, pt_off, res, names = TR.bounds_special()[name]
    with np.errstate(all="ignore"):
        want = TR.scene_grids(pts, pt_off, res)
    got = _scene_bounds(pts, pt_off, res)
    _same_grids(got, want, names)
    if name == "wide":
        g = {s: got[i] for i, s in enumerate(names)}
        assert list(g["product"]["g"]) == [2001] * 3 and g["product"]["ncell"] == 0 and g["product"]["flags"] == 2
        for s in ("q_2e9", "q_3e38", "inf_point", "minus_inf_point", "all_inf_axis", "nan_axis", "all_nan"):
            assert list(g[s]["g"]) == [0, 0, 0] and g[s]["ncell"] == 0 and g[s]["flags"] == 2, s
        assert g["q_below_2e9"]["ncell"] == 2000000000 - 128 + 1 and g["q_below_2e9"]["flags"] == 0
