"""CPU tests that pin the batch restatement of tests/tuple_front_ref.py to the oracle's single-scene functions and the reference's
golden vectors, and check that the inputs tests/test_tuple_front_gpu.py uses can tell a wrong kernel from a right one: every
deliberately wrong variant of the restatement differs from the right one on those very inputs."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tuple_front_ref as TR  # noqa: E402
from oracle import cppf_oracle as O  # noqa: E402

SHOT_SHAPES = [(5, 64), (2, 4), (3, 8), (8, 16)]


# ---------------------------------------------------------------------------------------------------------------
# the restatement against the reference's output and the oracle
# ---------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_rows(small):
    """small_encode_shot is the reference's own prepare_tuple_inputs output."""
    pc, idx = small["small_pc"], small["small_idx"]
    out = TR.encode_batch(pc, small["small_normal"], small["small_feat"], idx, TR.offsets([pc.shape[0]]), TR.offsets([idx.shape[0]]), 5)
    want = small["small_encode_shot"]
    assert np.array_equal(TR.bits(out["rows"]), TR.bits(want))
    assert np.array_equal(TR.bits(out["heads"]), TR.bits(want[:, :40]))
    assert np.array_equal(TR.bits(out["coord"]), TR.bits(want[:, :30]))
    assert np.array_equal(TR.bits(out["cheads"][:, :30]), TR.bits(want[:, :30])) and not out["cheads"][:, 30:].any()
    assert out["cheads"].shape[1] == 32 and np.array_equal(out["gidx"], idx.astype(np.int32))


@pytest.mark.parametrize("k", range(2, 9))
def test_restatement_is_the_oracle_on_one_scene(k):
    rng = np.random.RandomState(k)
    n, T, F, D = 97, 301, 8, 4
    pc, nrm, feat = rng.rand(n, 3).astype(np.float32), rng.randn(n, 3).astype(np.float32), rng.randn(n, F).astype(np.float32)
    idx = rng.randint(0, n, (T, k))
    tables = rng.randint(-50, 50, (n, k, D)).astype(np.float32)          # integers: the sum is exact in any order
    bias = rng.randint(-50, 50, D).astype(np.float32)
    out = TR.encode_batch(pc, nrm, feat, idx, TR.offsets([n]), TR.offsets([T]), k, tables=tables, bias=bias)
    assert np.array_equal(TR.bits(out["rows"]), TR.bits(O.prepare_tuple_inputs_shot(pc, idx, feat, nrm)))
    assert np.array_equal(TR.bits(out["coord"]), TR.bits(O.tuple_coord_inputs(pc, idx)))
    assert np.array_equal(TR.bits(out["heads"][:, TR.coord_cols(k):]), TR.bits(O.tuple_normal_inputs(nrm, idx)))
    assert out["cheads"].shape[1] % 8 == 0 and 0 <= out["cheads"].shape[1] - TR.coord_cols(k) < 8
    want = bias.astype(np.float64) + sum(tables[idx[:, i], i].astype(np.float64) for i in range(k))
    assert np.array_equal(out["dino"].astype(np.float64), want)


def test_dino_rows_add_left_to_right_in_float32():
    """Three terms whose float32 sum depends on the order: (1 + 2^-24) + 2^-24 = 1 left to right, 1 + 2^-23 the other way."""
    e = np.float32(2.0 ** -24)
    tables = np.array([[[1.0] * 4, [e] * 4, [e] * 4]], dtype=np.float32)
    got = TR.dino_rows(tables, None, np.zeros((1, 3), np.int64))
    assert np.all(got == np.float32(1.0))
    got = TR.dino_rows(tables[:, ::-1], None, np.zeros((1, 3), np.int64))
    assert np.all(got == np.float32(1.0 + 2.0 ** -23))
    # bias None starts from +0: a lone -0 comes out as +0, with a -0 bias it stays -0
    z = np.full((1, 1, 4), -0.0, np.float32)
    assert not TR.bits(TR.dino_rows(z, None, np.zeros((1, 1), np.int64))).any()
    assert np.all(TR.bits(TR.dino_rows(z, np.full(4, -0.0, np.float32), np.zeros((1, 1), np.int64))) == 0x80000000)


def test_ragged_sampler_tables_are_the_oracle_per_scene():
    seed = 0xFEDCBA9876543210
    pts, tup = [1, 1, 2, 257, 50000], [0, 1, 255, 256, 257]
    off = TR.offsets(tup)
    got = TR.sample_batch(pts, tup, 7, seed, 7, 3)
    u = TR.uniform_batch(tup, 5, seed, 7, 3, 9)
    assert got.shape == (769, 7) and u.shape == (769, 5)
    for b in range(5):
        assert np.array_equal(got[off[b]:off[b + 1]], O.sample_tuples(seed, 7 + 3 * b, tup[b], 7, pts[b]))
        assert np.array_equal(u[off[b]:off[b + 1]], O.philox_uniform(seed, 7 + 3 * b, 9, tup[b], 5))
    big = O.sample_tuples(seed, 7, 1000, 8, 2 ** 31 - 1)
    assert big.min() >= 0 and big.max() > 2 ** 30 and big.dtype == np.int32      # the 64-bit range map at the largest int32 n


# ---------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests tell the listed mistakes from the right kernel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, 9))
def test_ragged_batch_reaches_both_ends_of_every_scene(k):
    d = TR.ragged_batch(k, F=8, D=4)
    assert list(np.diff(d["tup_off"])) == TR.RAGGED_TUPLES and list(np.diff(d["pt_off"])) == TR.RAGGED_POINTS
    for b, t0, t1 in TR.scene_slices(d["tup_off"]):
        li = d["idx"][t0:t1]
        assert li.min() == 0 and li.max() == TR.RAGGED_POINTS[b] - 1
    for b, p in (TR.ZERO_NORMAL, TR.NAN_NORMAL):
        assert (d["idx"][d["tup_off"][b]:d["tup_off"][b + 1]] == p).any()
    assert not d["normals"][d["pt_off"][TR.ZERO_NORMAL[0]] + TR.ZERO_NORMAL[1]].any()
    assert np.isnan(d["normals"]).sum() == 1
    if k >= 2:
        heads = TR.encode_batch(d["pts"], d["normals"], None, d["idx"], d["pt_off"], d["tup_off"], k)["heads"]
        b = TR.NAN_NORMAL[0]
        assert np.isnan(heads[d["tup_off"][b]:d["tup_off"][b + 1], TR.coord_cols(k):]).any()     # the computed NaN is there
        assert not np.isnan(heads[:, :TR.coord_cols(k)]).any()


# what each mistake must change; a scene is exempt only where the mistake cannot change anything at all:
#  * scene 1 has ONE point: every coordinate difference is p0 - p0 = +0 and every pair is (0, 0), whichever base or pair order;
#  * "find_first" differs from the right lookup only where an empty scene shares the offset: scenes 1 and 6 (after 0 and 5);
#  * F = 4: a feature block of k equal rows (scene 1) shifted by one float4 is itself.
MUST_DIFFER = {"neighbour_base": ("rows", "heads", "gidx", "dino", "coord", "cheads"),
               "pairs_ji": ("rows", "heads", "coord", "cheads"),
               "feat_shift": ("rows",),
               "find_first": ("rows", "heads", "gidx", "dino", "coord", "cheads")}


def _blind(variant, name, b, F):
    if variant == "find_first" and b not in (1, 6):
        return True
    if b == 1:
        return variant == "pairs_ji" or (variant in ("neighbour_base", "find_first") and name in ("coord", "cheads")) or \
            (variant == "feat_shift" and F == 4)
    return False


@pytest.mark.parametrize("variant", TR.VARIANTS)
@pytest.mark.parametrize("k,F", SHOT_SHAPES)
def test_every_wrong_variant_differs_in_every_scene(k, F, variant):
    d = TR.ragged_batch(k, F=F, D=4)
    args = (d["pts"], d["normals"], d["feat"], d["idx"], d["pt_off"], d["tup_off"], k)
    right = TR.encode_batch(*args, tables=d["tables"], bias=d["bias"])
    wrong = TR.encode_batch(*args, tables=d["tables"], bias=d["bias"], variant=variant)
    scenes = TR.scene_slices(d["tup_off"])
    assert [b for b, _, _ in scenes] == [1, 2, 3, 4, 6]
    seen = 0
    for name in MUST_DIFFER[variant]:
        for b, t0, t1 in scenes:
            differs = not np.array_equal(TR.bits(right[name][t0:t1]), TR.bits(wrong[name][t0:t1]))
            if _blind(variant, name, b, F):
                assert not differs, "the exemption of (%s, %s, scene %d) is no longer needed" % (variant, name, b)
            else:
                assert differs, "%s is not told from the right kernel by %s of scene %d" % (variant, name, b)
                seen += 1
    assert seen >= 2


@pytest.mark.parametrize("k", [1, 5, 8])
def test_wrong_base_and_lookup_change_the_dino_rows(k):
    d = TR.ragged_batch(k, D=4)
    right = TR.dino_rows(d["tables"], d["bias"], TR.global_indices(d["idx"], d["pt_off"], d["tup_off"]))
    N = d["pts"].shape[0]
    for variant, scenes in (("neighbour_base", (1, 2, 3, 4, 6)), ("find_first", (1, 6))):
        wrong = TR.dino_rows(d["tables"], d["bias"], TR.global_indices(d["idx"], d["pt_off"], d["tup_off"], variant).astype(np.int64) % N)
        for b in scenes:
            t0, t1 = d["tup_off"][b], d["tup_off"][b + 1]
            assert not np.array_equal(TR.bits(right[t0:t1]), TR.bits(wrong[t0:t1]))


# ---------------------------------------------------------------------------------------------------------------
# scene bounds: the rule of include/cppf_hip.h
# ---------------------------------------------------------------------------------------------------------------
def _grids(name):
    pts, pt_off, res, names = TR.bounds_special()[name]
    with np.errstate(all="ignore"):
        g = TR.scene_grids(pts, pt_off, res)
    return {s: g[i] for i, s in enumerate(names)}


def test_scene_grids_truncate_the_float32_quotient():
    g = _grids("exact")
    assert list(g["integer"]["g"]) == [9, 5, 3] and g["integer"]["ncell"] == 135 and g["integer"]["flags"] == 0
    assert list(g["ulp_below"]["g"]) == [8, 5, 3] and g["ulp_below"]["ncell"] == 120
    assert list(g["negative_integer"]["g"]) == [9, 1, 1] and list(g["negative_integer"]["c0"]) == [-4, -1, -1]
    assert list(g["negative_ulp_below"]["g"]) == [8, 1, 1]
    assert list(g["one_point"]["g"]) == [1, 1, 1] and g["one_point"]["ncell"] == 1 and list(g["one_point"]["c0"]) == [-1.5, 2.5, 0.0]


def test_scene_grids_report_what_int32_cannot_hold_as_overflow():
    g = _grids("wide")
    assert list(g["product"]["g"]) == [2001] * 3 and g["product"]["ncell"] == 0 and g["product"]["flags"] == 2
    assert list(g["q_below_2e9"]["g"]) == [2000000000 - 128 + 1, 1, 1] and g["q_below_2e9"]["flags"] == 0
    assert g["q_below_2e9"]["ncell"] == 2000000000 - 128 + 1
    for s in ("q_2e9", "q_3e38", "inf_point", "minus_inf_point", "all_inf_axis", "nan_axis", "all_nan"):
        assert list(g[s]["g"]) == [0, 0, 0] and g[s]["ncell"] == 0 and g[s]["flags"] == 2, s
    assert g["nan_axis"]["c0"][1] == np.inf and list(g["nan_axis"]["c0"][[0, 2]]) == [0, 0]
    assert g["minus_inf_point"]["c0"][2] == -np.inf and g["all_inf_axis"]["c0"][0] == np.inf
    assert list(g["partial_nan"]["g"]) == [5, 3, 6] and g["partial_nan"]["ncell"] == 90 and g["partial_nan"]["flags"] == 0
    assert list(g["empty"]["g"]) == [0, 0, 0] and g["empty"]["ncell"] == 0 and g["empty"]["flags"] == 1
    assert np.all(g["empty"]["c0"] == np.inf)
    assert list(g["ordinary_after"]["g"]) == [4, 3, 2] and g["ordinary_after"]["ncell"] == 24


@pytest.mark.parametrize("kind", ["min", "max"])
@pytest.mark.parametrize("place", ["first", "last", "p64"])
def test_scene_grids_are_the_oracle_on_the_placement_batch(place, kind):
    pts, pt_off = TR.bounds_batch(place, kind)
    g = TR.scene_grids(pts, pt_off, TR.BOUNDS_RES)
    assert pts.max() < 0 or kind == "max"
    for b, n in enumerate(TR.BOUNDS_SIZES):
        if n == 0:
            assert g[b]["flags"] == 1
            continue
        pc = pts[pt_off[b]:pt_off[b + 1]]
        c0, gr = O.grid_geometry(pc, TR.BOUNDS_RES)
        assert np.array_equal(g[b]["c0"], c0) and np.array_equal(g[b]["g"], gr) and g[b]["ncell"] == int(np.prod(gr)) and g[b]["flags"] == 0
        pos = {"first": 0, "last": n - 1, "p64": min(64, n - 1)}[place]
        ext = pc.min(0) if kind == "min" else pc.max(0)
        assert np.array_equal(pc[pos], ext)                         # the extreme of every axis sits at that point
        if n > 1:
            assert not np.array_equal(np.delete(pc, pos, 0).min(0) if kind == "min" else np.delete(pc, pos, 0).max(0), ext)


# ---------------------------------------------------------------------------------------------------------------
# cast_f16 inputs
# ---------------------------------------------------------------------------------------------------------------
def test_cast_inputs_hold_the_ties_of_both_parities():
    v = TR.cast_inputs()
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)
    f = h.astype(np.float64)
    fin = np.isfinite(v) & np.isfinite(f)
    with np.errstate(over="ignore"):
        up = np.nextafter(h, np.float16(np.inf)).astype(np.float64)
        dn = np.nextafter(h, np.float16(-np.inf)).astype(np.float64)
    x = v.astype(np.float64)
    with np.errstate(invalid="ignore"):
        tie = fin & ((x - f == (up - f) / 2) | (x - f == (dn - f) / 2)) & (x != f)
    assert tie.sum() >= 100
    assert not (TR.bits(h[tie]) & 1).any()                          # every tie went to the even neighbour ...
    away = np.where(x[tie] > f[tie], up[tie], dn[tie])              # ... and the odd neighbour it left is as near
    assert np.array_equal(np.abs(away - x[tie]), np.abs(f[tie] - x[tie]))
    # ties whose lower neighbour is even and ties whose lower neighbour is odd (rounded down / rounded up in magnitude)
    assert (np.abs(f[tie]) < np.abs(x[tie])).sum() >= 30 and (np.abs(f[tie]) > np.abs(x[tie])).sum() >= 30
    for val, want in ((65504.0, 0x7BFF), (65519.99, 0x7BFF), (65520.0, 0x7C00), (2.0 ** -24, 0x0001), (2.0 ** -25, 0x0000),
                      (float(np.nextafter(np.float32(2.0 ** -25), np.float32(1))), 0x0001), (-0.0, 0x8000), (-np.inf, 0xFC00)):
        m = TR.bits(v) == TR.bits(np.array([val], np.float32))[0]
        assert m.any() and np.all(TR.bits(h[m]) == want), val
    assert np.isnan(v).sum() == 2 and np.isnan(h).sum() == 2
    for n in (1, 255, 257):
        t = TR.tiled(v, n)
        assert t.size == n and np.array_equal(TR.bits(t[-min(n, v.size):]), TR.bits(v[-min(n, v.size):]))


def test_half_table_holds_the_special_halves():
    t = TR.half_table(40, 8)
    u = set(TR.bits(t).reshape(-1).tolist())
    assert {0x8000, 0x7BFF, 0xFBFF, 0x0400, 0x8400, 0x0001, 0x8001, 0x03FF, 0x7C00, 0xFC00, 0x7E00} <= u
    nan = np.isnan(t)
    assert np.all(TR.bits(t)[nan] == 0x7E00)                        # quiet NaNs only: widening copies their payload
