"""Plain host restatement of the tuple front end (cppf2_amd/csrc/cppf_core.hip up to encode_dino_kernel) for ragged batches.

NumPy only, one loop per scene, built on the oracle's single-scene functions (O.sample_tuples, O.philox_uniform,
O.tuple_coord_inputs, O.tuple_normal_inputs, O.prepare_tuple_inputs_shot, O.grid_geometry).  Every output is a chain of exact
IEEE operations or integer work, so tests/test_tuple_front_gpu.py compares the kernels with it bit for bit;
tests/test_tuple_front_ref.py pins it to the oracle and the reference's golden vectors on the CPU.

`variant` selects a deliberately WRONG restatement (the mistakes a kernel of this family can make without the single-scene
tests noticing); tests/test_tuple_front_ref.py checks that the inputs built here tell each of them from the right one.
"""
from itertools import combinations

import numpy as np

from oracle import cppf_oracle as O

F32 = np.float32
VARIANTS = ("neighbour_base", "pairs_ji", "feat_shift", "find_first")


# ---------------------------------------------------------------------------------------------------------------
# bit views and offsets
# ---------------------------------------------------------------------------------------------------------------
def bits(a):
    """The unsigned-integer view of a float array (uint32 / uint16), so that -0.0 and NaN payloads count; integers unchanged."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float16:
        return a.view(np.uint16)
    assert a.dtype.kind in "iu", a.dtype
    return a


def offsets(counts):
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(np.asarray(counts, dtype=np.int64), out=off[1:])
    assert off[-1] <= 2 ** 31 - 1
    return off.astype(np.int32)


def head_cols(k):
    return 4 * (k * (k - 1) // 2)


def coord_cols(k):
    return 3 * (k * (k - 1) // 2)


def coord_head_cols(k):
    return (coord_cols(k) + 7) // 8 * 8


# ---------------------------------------------------------------------------------------------------------------
# encoders
# ---------------------------------------------------------------------------------------------------------------
def _scene_of(b, tup_off, variant):
    """The scene whose point base serves the rows of scene b.  The kernels that search (find_scene) must return the LAST scene
    among equal offsets -- the empty scenes before b share tup_off[b]; "find_first" returns the first."""
    if variant != "find_first":
        return b
    return int(np.searchsorted(np.asarray(tup_off), tup_off[b], side="left"))


def _base(b, pt_off, variant):
    B = len(pt_off) - 1
    if variant == "neighbour_base":
        return int(pt_off[b + 1 if b + 1 < B else b - 1])
    return int(pt_off[b])


def _coord(points, idx, variant):
    if variant == "pairs_ji":
        k = idx.shape[1]
        return np.concatenate([points[idx[:, j]] - points[idx[:, i]] for (i, j) in combinations(range(k), 2)], -1)
    return O.tuple_coord_inputs(points, idx)


def global_indices(idx, pt_off, tup_off, variant=None):
    """pt_off[b] + idx for the rows of scene b: int32 [T, k] (any k >= 1)."""
    idx = np.asarray(idx)
    out = np.zeros(idx.shape, np.int32)
    for b in range(len(pt_off) - 1):
        t0, t1 = int(tup_off[b]), int(tup_off[b + 1])
        out[t0:t1] = _base(_scene_of(b, tup_off, variant), pt_off, variant) + idx[t0:t1]
    return out


def dino_rows(tables, bias, gidx):
    """bias + tables[g_0, 0] + ... + tables[g_{k-1}, k-1], added left to right in float32 (bias None: starts from +0)."""
    tables = np.asarray(tables, dtype=F32)
    _, k, D = tables.shape
    acc = np.zeros((gidx.shape[0], D), dtype=F32) if bias is None else np.broadcast_to(np.asarray(bias, F32), (gidx.shape[0], D)).copy()
    for i in range(k):
        acc = (acc + tables[gidx[:, i], i]).astype(F32)
    return acc


def encode_batch(pts, normals, feat, idx, pt_off, tup_off, k, tables=None, bias=None, variant=None):
    """Every encoder output for a ragged batch.  pts / normals float32 [N,3], feat float32 [N,F] (or None), idx [T,k] LOCAL
    indices, tables float32 [N,k,D] (or None).  Returns a dict:
      rows   float32 [T, 4 C(k,2) + k F]   cppf_encode_tuples_shot (if feat)
      heads  float32 [T, 4 C(k,2)]         cppf_encode_tuples_shot_heads
      cheads float32 [T, round8(3 C(k,2))] cppf_encode_tuples_coord_heads (zero padded)
      gidx   int32   [T, k]                pt_off[b] + idx
      coord  float32 [T, 3 C(k,2)]         cppf_encode_tuples_coord
      dino   float32 [T, D]                cppf_encode_tuples_dino (if tables)
    """
    assert variant is None or variant in VARIANTS
    pts = np.asarray(pts, dtype=F32)
    normals = np.asarray(normals, dtype=F32)
    idx = np.asarray(idx)
    N, T = pts.shape[0], idx.shape[0]
    assert idx.shape[1] == k and tup_off[-1] == T and pt_off[-1] == N
    F = 0 if feat is None else feat.shape[1]
    out = {"heads": np.zeros((T, head_cols(k)), F32), "cheads": np.zeros((T, coord_head_cols(k)), F32),
           "gidx": global_indices(idx, pt_off, tup_off, variant), "coord": np.zeros((T, coord_cols(k)), F32)}
    if feat is not None:
        feat = np.asarray(feat, dtype=F32)
        out["rows"] = np.zeros((T, head_cols(k) + k * F), F32)
    for b in range(len(pt_off) - 1):
        t0, t1 = int(tup_off[b]), int(tup_off[b + 1])
        if t1 == t0:
            continue
        n = int(pt_off[b + 1] - pt_off[b])
        li = idx[t0:t1].astype(np.int64)
        assert li.min() >= 0 and li.max() < n
        p0 = _base(_scene_of(b, tup_off, variant), pt_off, variant)
        sel = (p0 + np.arange(n)) % N                  # (only a wrong base can reach past the batch: wrapped, never an error)
        P, Nn = pts[sel], normals[sel]
        coord = _coord(P, li, variant)
        nrm = O.tuple_normal_inputs(Nn, li)
        out["coord"][t0:t1] = coord
        out["cheads"][t0:t1, :coord.shape[1]] = coord
        out["heads"][t0:t1] = np.concatenate([coord, nrm], -1)
        if feat is not None:
            if variant is None:
                rows = O.prepare_tuple_inputs_shot(P, li, feat[sel], Nn)
            else:
                block = np.concatenate([feat[sel][li[:, i]] for i in range(k)], -1)
                if variant == "feat_shift":
                    block = np.roll(block, 4, axis=1)
                rows = np.concatenate([coord, nrm, block], -1)
            out["rows"][t0:t1] = rows
    if tables is not None:
        out["dino"] = dino_rows(tables, bias, out["gidx"].astype(np.int64) % N)
    return out


# ---------------------------------------------------------------------------------------------------------------
# sampler and uniforms
# ---------------------------------------------------------------------------------------------------------------
def sample_batch(pt_counts, tup_counts, k, seed, sid_base, sid_stride):
    """cppf_sample_tuples on a ragged batch: scene b draws tup_counts[b] rows in [0, pt_counts[b]) with scene id base + b*stride."""
    parts = [O.sample_tuples(seed, sid_base + b * sid_stride, int(nt), k, int(n)) for b, (n, nt) in enumerate(zip(pt_counts, tup_counts))]
    return np.concatenate(parts, 0).astype(np.int32).reshape(-1, k)


def uniform_batch(tup_counts, m, seed, sid_base, sid_stride, stream_id):
    parts = [O.philox_uniform(seed, sid_base + b * sid_stride, stream_id, int(nt), m) for b, nt in enumerate(tup_counts)]
    return np.concatenate(parts, 0).astype(F32).reshape(-1, m)


# ---------------------------------------------------------------------------------------------------------------
# scene bounds: CppfSceneGrid as include/cppf_hip.h defines it
# ---------------------------------------------------------------------------------------------------------------
GRID_DTYPE = np.dtype([("c0", "<f4", (3,)), ("g", "<i4", (3,)), ("ncell", "<i4"), ("flags", "<i4")])
assert GRID_DTYPE.itemsize == 32
INT32_MAX = 2 ** 31 - 1


def scene_grids(pts, pt_off, res):
    pts = np.asarray(pts, dtype=F32)
    out = np.zeros(len(pt_off) - 1, dtype=GRID_DTYPE)
    for b in range(len(pt_off) - 1):
        pc = pts[int(pt_off[b]):int(pt_off[b + 1])]
        if pc.shape[0] == 0:
            out["c0"][b], out["flags"][b] = np.inf, 1
            continue
        lo = np.fmin.reduce(pc, axis=0, initial=F32(np.inf))        # NaN coordinates are skipped
        hi = np.fmax.reduce(pc, axis=0, initial=F32(-np.inf))
        out["c0"][b] = lo
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            q = (hi - lo) / F32(res)
        if not np.all((q >= 0) & (q < F32(2.0e9))):                  # unrepresentable: no axis count is reported
            out["flags"][b] = 2
            continue
        if not np.isnan(pc).any():
            c0, gr = O.grid_geometry(pc, float(F32(res)))
            assert np.array_equal(c0, lo)
        else:
            gr = q.astype(np.int64) + 1
        out["g"][b] = gr
        cells = int(gr[0]) * int(gr[1]) * int(gr[2])
        if cells > INT32_MAX:
            out["flags"][b] = 2
        else:
            out["ncell"][b] = cells
    return out


# ---------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests (built here so that the CPU file checks the very same arrays)
# ---------------------------------------------------------------------------------------------------------------
RAGGED_TUPLES = [0, 1, 255, 256, 257, 0, 3001, 0]
RAGGED_POINTS = [1, 1, 300, 77, 512, 5, 1024, 2]
ZERO_NORMAL = (2, 7)          # (scene, local point): the all-zero normal
NAN_NORMAL = (4, 11)          # the normal that carries a NaN: cosines computed from it are NaN


def ragged_batch(k, F=None, D=None, seed=0):
    """The ragged batch of the issue for one tuple size: dict(pts, normals, feat, tables, bias, idx, pt_off, tup_off).
    Scene b's points are shifted by b so that a wrong base changes values; every scene's idx reaches 0 and n_b - 1."""
    rng = np.random.RandomState(1000 + 17 * k + seed)
    pt_off, tup_off = offsets(RAGGED_POINTS), offsets(RAGGED_TUPLES)
    N, T = int(pt_off[-1]), int(tup_off[-1])
    pts = rng.rand(N, 3).astype(F32)
    normals = rng.randn(N, 3).astype(F32)
    idx = np.zeros((T, k), dtype=np.int32)
    for b, (n, nt) in enumerate(zip(RAGGED_POINTS, RAGGED_TUPLES)):
        pts[pt_off[b]:pt_off[b + 1]] += F32(b)
        if nt == 0:
            continue
        li = rng.randint(0, n, (nt, k)).astype(np.int32)
        li[0, 0], li[-1, k - 1] = 0, n - 1
        idx[tup_off[b]:tup_off[b + 1]] = li
    for (b, p), val in ((ZERO_NORMAL, [0, 0, 0]), (NAN_NORMAL, [0.5, np.nan, -0.25])):
        normals[pt_off[b] + p] = val
        idx[tup_off[b] + 3, 0] = p                       # drawn for certain (row 3 is neither the first nor the last row)
        idx[tup_off[b] + 5, k - 1] = p
    d = {"pts": pts, "normals": normals, "idx": idx, "pt_off": pt_off, "tup_off": tup_off, "k": k, "feat": None, "tables": None,
         "bias": None}
    if F is not None:
        d["feat"] = rng.randn(N, F).astype(F32)
    if D is not None:
        d["tables"] = rng.randn(N, k, D).astype(F32)
        d["bias"] = rng.randn(D).astype(F32)
    return d


def half_table(n, F, seed=0):
    """float16 [n, F]: random halves with -0, the largest / smallest normal halves, subnormals, inf and (quiet) NaN among them."""
    rng = np.random.RandomState(77 + seed)
    t = rng.randn(n, F).astype(np.float16)
    special = np.array([0x8000, 0x7BFF, 0xFBFF, 0x0400, 0x8400, 0x0001, 0x8001, 0x03FF, 0x7C00, 0xFC00, 0x7E00, 0x0000], dtype=np.uint16)
    flat = t.reshape(-1).view(np.uint16)
    pos = rng.choice(flat.size, size=min(flat.size, 16 * special.size), replace=False)
    flat[pos] = np.resize(special, pos.size)
    m = min(special.size, flat.size)
    flat[:m] = special[:m]                              # row 0, which every scene's idx reaches
    return t


def scene_slices(off):
    """[(b, start, stop)] of the scenes that hold rows."""
    return [(b, int(off[b]), int(off[b + 1])) for b in range(len(off) - 1) if off[b + 1] > off[b]]


def cast_inputs():
    """float32 values around every rounding decision of float32 -> float16 (round to nearest even)."""
    h = np.concatenate([np.arange(0x0000, 0x0012), np.arange(0x03F8, 0x0408), np.arange(0x3BFC, 0x3C08), np.arange(0x7BF0, 0x7BFF),
                        np.arange(0x0400, 0x7BFF, 0x0155)]).astype(np.uint16)      # even and odd mantissas, subnormals, 1.0, the top
    lo = h.view(np.float16).astype(np.float64)
    hi = (h + np.uint16(1)).view(np.float16).astype(np.float64)
    tie = ((lo + hi) / 2).astype(F32)                                               # exact in float32 (11 + 1 bits)
    assert np.array_equal(tie.astype(np.float64), (lo + hi) / 2)
    vals = [tie, np.nextafter(tie, F32(np.inf)), np.nextafter(tie, F32(-np.inf)), lo.astype(F32)]
    vals.append(np.array([65504.0, 65519.99, 65520.0, 65536.0, 2.0 ** -24, 2.0 ** -25, np.nextafter(F32(2.0 ** -25), F32(1)),
                          np.nextafter(F32(2.0 ** -25), F32(0)), 0.0, 1e-30, 3.4e38, np.inf], dtype=F32))
    v = np.concatenate(vals).astype(F32)
    return np.concatenate([v, -v, np.array([np.nan, -np.nan], dtype=F32)])


def tiled(values, n):
    """n values: `values` repeated, the last ones last (so that a tail beyond the grid still holds every special value)."""
    out = np.resize(values, n)
    m = min(n, values.size)
    out[n - m:] = values[values.size - m:]
    return out


BOUNDS_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025]      # around the wavefront (64) and the 256-thread strided loop
BOUNDS_RES = 0.25


def bounds_batch(place, kind):
    """(pts, pt_off) of the scene-bounds batch: negative coordinates in [-3, -1), and per scene the `kind` ("min" / "max") extreme of
    every axis at one point: the "first", the "last" or "p64" (point 64, the first lane of the second wavefront; the last
    point of a shorter scene)."""
    rng = np.random.RandomState(5 + len(place) + 3 * len(kind))
    pt_off = offsets(BOUNDS_SIZES)
    pts = (-3.0 + 2.0 * rng.rand(int(pt_off[-1]), 3)).astype(F32)
    for b, n in enumerate(BOUNDS_SIZES):
        if n == 0:
            continue
        pos = {"first": 0, "last": n - 1, "p64": min(64, n - 1)}[place]
        for c in range(3):
            pts[pt_off[b] + pos, c] = (-7.0 - c - 0.125 * b) if kind == "min" else (2.0 + c + 0.125 * b)
    return pts, pt_off


def bounds_special():
    """{name: (pts, pt_off, res, scene names)}: the extents at which cppf_scene_bounds decides something."""
    def batch(scenes, res):
        names = list(scenes)
        arrs = [np.asarray(scenes[s], dtype=F32).reshape(-1, 3) for s in names]
        return np.concatenate(arrs, 0), offsets([a.shape[0] for a in arrs]), res, names

    two, m2 = F32(2.0), F32(-2.0)
    inf, nan = np.inf, np.nan
    big = F32(2.0e9)
    exact = {
        "integer": [[0, 0, 0], [two, 1, 0.5]],                                           # q = (8, 4, 2) exactly
        "ulp_below": [[0, 0, 0], [np.nextafter(two, F32(0)), 1, 0.5]],                    # q_x = 8 - 2^-21
        "negative_integer": [[-4, -1, -1], [m2, -1, -1]],
        "negative_ulp_below": [[-4, -1, -1], [np.nextafter(m2, F32(-inf)), -1, -1]],
        "one_point": [[-1.5, 2.5, 0.0]],
    }
    wide = {
        "product": [[-1000, -1000, -1000], [1000, 1000, 1000]],                           # 2001^3 > 2^31 - 1, every axis fine
        "q_2e9": [[0, 0, 0], [big, 1, 1]],                                                # q_x = 2e9: not < 2e9
        "q_below_2e9": [[0, 0, 0], [np.nextafter(big, F32(0)), 0, 0]],                    # the largest axis count: 2e9 - 128 + 1
        "q_3e38": [[-3e38, 0, 0], [3e38, 1, 1]],                                          # hi - lo overflows to +inf
        "inf_point": [[0, 0, 0], [1, inf, 1], [2, 2, 2]],
        "minus_inf_point": [[0, 0, -inf], [1, 1, 1]],
        "all_inf_axis": [[inf, 0, 0], [inf, 1, 1]],                                       # inf - inf = NaN
        "nan_axis": [[0, nan, 0], [1, nan, 1], [2, nan, 2]],
        "all_nan": [[nan, nan, nan]],
        "partial_nan": [[0, nan, 0], [1, 3, nan], [nan, 1, 2], [4, 2, 5]],                # NaNs skipped: a grid of (5, 3, 6)
        "empty": np.zeros((0, 3)),
        "ordinary_after": [[0, 0, 0], [3, 2, 1]],
    }
    return {"exact": batch(exact, 0.25), "wide": batch(wide, 1.0)}
