"""CPU tests that pin the batch restatement of tests/tuple_back_ref.py to the oracle's single-scene functions and the reference's
golden vectors, show that its exact inputs are exact (integer CDFs; float64 sums inside the emulated fused norm that round
nowhere), and check that the inputs tests/test_tuple_back_gpu.py uses can tell a wrong kernel from a right one: every
deliberately wrong variant of the restatement differs from the right one on those very inputs."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tuple_back_ref as TB  # noqa: E402
import tuple_front_ref as TR  # noqa: E402
from oracle import cppf_oracle as O  # noqa: E402

UP, RIGHT, FRONT = [0, 1, 0], [1, 0, 0], [0, 0, 1]
GOLDEN_AXES = np.array([UP, FRONT, RIGHT], dtype=np.float64)       # the positional order of the reference's call site
SHAPES = [(5, 2), (5, 20), (5, 32), (5, 33), (5, 4096), (2, 32), (8, 32)]      # (k, nb) of the GPU tests' ragged batches
MARGIN_NB = (20, 32, 33)


# ---------------------------------------------------------------------------------------------------------------
# pinning: the restatement is the oracle on one scene, and the reference on the golden vectors
# ---------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_vectors(small):
    pc, idx, scaled = small["small_pc"], small["small_idx"], small["small_scaled"]
    T = idx.shape[0]
    off = TR.offsets([T])
    tr, rot = TB.target_pairs_batch(scaled, off, GOLDEN_AXES, None)
    assert np.array_equal(TR.bits(tr), TR.bits(small["small_tr0"])) and np.array_equal(rot, small["small_rot0"], equal_nan=True)
    tr, rot = TB.target_pairs_batch(scaled, off, GOLDEN_AXES, np.zeros((1, 3)))
    assert np.array_equal(TR.bits(tr), TR.bits(small["small_tr0"])) and np.array_equal(rot, small["small_rot0"], equal_nan=True)
    pairs = pc[idx[:, :2]]
    tr, rot = TB.target_pairs_batch(pairs, off, GOLDEN_AXES, small["small_centre"].reshape(1, 3))
    assert np.array_equal(tr, small["small_tr1"], equal_nan=True) and np.array_equal(rot, small["small_rot1"], equal_nan=True)
    assert not np.array_equal(small["small_tr0"], small["small_tr1"])


@pytest.mark.parametrize("nb", [2, 20, 32, 33, 64])
def test_restatement_is_the_oracle_on_one_scene(nb):
    rng = np.random.RandomState(nb)
    n, T, k = 97, 601, 5
    pc = rng.rand(n, 3).astype(np.float32)
    idx = rng.randint(0, n, (T, k))
    idx[7, 1] = idx[7, 0]
    logits = (rng.randn(T, 6, nb) * 3).astype(np.float32)
    u = rng.rand(T, 6).astype(np.float32)
    u[0], u[1] = 0.0, TB.ONE_BELOW
    bins, _, scale, scaled = O.decode_bins(logits, u, pc[idx[:, :2]])
    assert np.array_equal(TB.draw(logits, None, u), bins) and TB.draw(logits, None, u).dtype == np.int32
    prior = rng.randn(T, 6, nb).astype(np.float32)
    assert np.array_equal(TB.draw(logits, prior, u), O.decode_bins(logits + prior, u, pc[idx[:, :2]])[0])
    got = TB.decode_batch(bins, nb, pc, idx, TR.offsets([n]), TR.offsets([T]), GOLDEN_AXES)
    tr, rot = O.generate_target_pairs(scaled, UP, FRONT, RIGHT)
    for g, w in zip(got, (scaled.reshape(T, 6), scale, tr, rot)):
        assert g.dtype == np.float32 and np.array_equal(TR.bits(g), TR.bits(w))
    # the local lines of target_pair (the ones the unit_clamp_max variant edits) are the oracle's
    ctr = np.array([0.3, -0.1, 0.2])
    pairs = pc[idx[:, :2]]
    right = O.generate_target_pairs(pairs, *TB.AXES, center=ctr)
    assert not TB.rows_differ(right, TB._target_pairs(pairs, TB.AXES, ctr, "_local")).any()
    wrong = TB._target_pairs(pairs, TB.AXES, ctr, "unit_clamp_max")
    assert TB.rows_differ(right, wrong).mean() > 0.9 and not TB.rows_differ(right, wrong)[7]       # (row 7: a == b, both 1e-7)


def test_ulps_counts_float32_steps():
    one = np.float32(1)
    a = np.array([1.0, 0.0, -0.0, np.nan, 3.0, np.inf], np.float32)
    b = np.array([np.nextafter(one, np.float32(2)), -0.0, 1e-45, np.nan, 3.0, np.float32(3.4028235e38)], np.float32)
    assert TB.ulps(a, b).tolist() == [1, 0, 1, 0, 0, 1]
    assert TB.ulps(np.array([-1e-45], np.float32), np.array([1e-45], np.float32)).tolist() == [2]


# ---------------------------------------------------------------------------------------------------------------
# exactness of the exact inputs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", TB.EXACT_NB)
def test_exact_rows_have_integer_cdfs(nb):
    rows, u, S = TB.exact_rows(nb)
    assert rows.shape[0] >= (150 if nb >= 20 else 40) and S.min() >= 1 and S.max() == nb and (S == 1).any()
    e, cdf, acc = O.softmax_cdf(rows)
    unmasked = rows == rows.max(1, keepdims=True)
    assert np.array_equal(e, unmasked.astype(np.float32))                      # exp(0) = 1, exp(masked) = 0: nothing in between
    assert np.array_equal(cdf, np.rint(cdf)) and np.array_equal(acc, S.astype(np.float32))
    assert np.array_equal(cdf, np.cumsum(unmasked, 1).astype(np.float32))
    for low in TB.MASKED:                                                        # both sides' exp() of a masked logit is 0
        assert np.exp(np.float32(low)) == 0 and low < -104.0
    # the kinds of masking and every special uniform are there
    for lvl in TB.LEVELS:
        assert (rows.max(1) == np.float32(lvl)).any()
    assert np.isneginf(rows).any() and (np.isfinite(rows) & (rows < rows.max(1, keepdims=True))).any()
    for special in (0.0, TB.ONE_BELOW, 1.0):
        assert (u == np.float32(special)).sum() >= 3
    # ties: target == a CDF value, on the rows at j / S
    target = (u * acc).astype(np.float32)
    tie = (cdf == target[:, None]).any(1)
    assert tie.sum() >= rows.shape[0] // 5, tie.sum()
    # the clamp: only a uniform of exactly 1.0 counts every bin
    full = (cdf <= target[:, None]).sum(1) == nb
    assert np.array_equal(full, u == np.float32(1.0)) and full.any()
    # "draw_lt" gives another bin on exactly the ties, but for the ties at 1.0 whose last bin is unmasked (the clamp's bin)
    right, wrong = TB.draw(rows, None, u), TB.draw(rows, None, u, "draw_lt")
    differ = right != wrong
    assert not differ[~tie].any() and differ.sum() >= rows.shape[0] // 5
    assert np.all((u[tie & ~differ] == np.float32(1.0)) & unmasked[tie & ~differ, -1])
    assert right.min() == 0 and right.max() == nb - 1


@pytest.mark.parametrize("case", TB.PRIOR_CASES)
@pytest.mark.parametrize("nb", [2, 32, 33])
def test_prior_split_sums_to_the_exact_rows(nb, case):
    rows, u, S = TB.exact_rows(nb, flat=case == "flat_sum")
    logits, prior = TB.prior_split(rows, case)
    assert np.array_equal(TR.bits((logits + prior).astype(np.float32)), TR.bits(rows))
    masked = rows < rows.max(1, keepdims=True)
    if case == "flat_sum":
        assert not masked.any() and np.all(S == nb) and np.isfinite(logits).all() and np.isfinite(prior).all()
    else:
        side, other = (logits, prior) if case == "mask_in_logits" else (prior, logits)
        assert np.isfinite(other).all() and np.isneginf(side).any() and np.all(side[masked] <= -190) and np.all(np.abs(other) <= 4.5)
    assert np.ptp(logits, axis=1).min() > 0 and np.ptp(prior, axis=1).min() > 0      # neither side is flat by itself
    assert np.array_equal(TB.draw(logits, prior, u), TB.draw(rows, None, u))
    assert (TB.draw(logits, prior, u, "draw_lt") != TB.draw(logits, prior, u)).sum() >= max(3, rows.shape[0] // 10)


def _two_sum_is_exact(a, b):
    """The float64 sum a + b loses nothing (Knuth's error-free two-sum: the rounding error itself, computed exactly)."""
    s = a + b
    bb = s - a
    return ((a - (s - bb)) + (b - bb)) == 0.0


@pytest.mark.parametrize("nb", [2, 20, 32, 33, 64])
def test_the_emulated_fused_norm_is_exact_on_bin_differences(nb):
    """O._norm3 emulates fma(y, y, acc) as float32(float64(y) * float64(y) + float64(acc)): the product is exact, so the emulation
    is the fused operation wherever the float64 SUM is exact too.  Over every ordered triple of the magnitudes a difference of two
    bin coordinates can take, it is -- so pred_len of the restatement is the kernel's, bit for bit, for these bin counts."""
    pr = (np.arange(nb, dtype=np.float32) / np.float32(nb - 1) - np.float32(0.5)).astype(np.float32)
    d = np.unique(np.abs((pr[:, None] - pr[None, :]).astype(np.float32)))
    assert d.size ** 3 < 1.3e7, d.size
    y2 = (d.astype(np.float64) ** 2)[:, None]
    z2 = (d.astype(np.float64) ** 2)[None, :]
    fused_differs = 0
    for x in d:
        acc0 = np.float64(np.float32(x * x))
        assert np.all(_two_sum_is_exact(y2, acc0))
        acc1 = (y2 + acc0).astype(np.float32)                                     # [ny, 1]
        assert np.all(_two_sum_is_exact(z2, acc1.astype(np.float64)))
        fused = np.sqrt((z2 + acc1.astype(np.float64)).astype(np.float32))
        yy, zz = (d * d).astype(np.float32)[:, None], (d * d).astype(np.float32)[None, :]
        fused_differs += int((fused != np.sqrt((np.float32(x * x) + yy) + zz)).sum())
    assert (fused_differs == 0) == TB.dyadic(nb), (nb, fused_differs)              # where "pred_unfused" can show at all


# ---------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests tell the listed mistakes from the right kernel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,nb", SHAPES)
def test_ragged_batch_is_what_the_gpu_tests_need(k, nb):
    d = TB.ragged_batch(k, nb)
    tup, pt = d["tup_off"], d["pt_off"]
    assert list(np.diff(tup)) == TB.RAGGED_TUPLES and list(np.diff(pt)) == TB.RAGGED_POINTS
    T = int(tup[-1])
    assert T % 32 and T % 256 and all(int(t) % 32 for t in tup[1:-1] if 0 < t < T)
    assert TB.RAGGED_TUPLES[0] == 0 and TB.RAGGED_TUPLES[-1] == 0 and TB.RAGGED_TUPLES[3:5] == [0, 0]
    assert {1, 31, 33, 256, 257} <= set(TB.RAGGED_TUPLES) and max(TB.RAGGED_TUPLES) > 1000
    assert TB.RAGGED_POINTS[TB.ONE_POINT_SCENE] == 1 and pt[1] > 0
    for b, t0, t1 in TR.scene_slices(tup):
        li = d["idx"][t0:t1]
        assert li.min() == 0 and li.max() == TB.RAGGED_POINTS[b] - 1 and d["bins"][t0:t1].max() < nb
        if t1 - t0 >= 4:
            assert np.array_equal(d["bins"][t0 + 1, :3], d["bins"][t0 + 1, 3:])                    # pred_len = 0
            assert np.abs(d["bins"][t0 + 2, :3] - d["bins"][t0 + 2, 3:]).tolist() == [0, 1, 0]    # adjacent bins
    scaled, scale, tr, rot = TB.decode_batch(d["bins"], nb, d["pts"], d["idx"], pt, tup, TB.AXES)
    one = slice(tup[TB.ONE_POINT_SCENE], tup[TB.ONE_POINT_SCENE + 1])
    assert not scale[one].any() and not scaled[one].any()                                          # real_len = 0
    t6 = int(tup[6])
    assert scale[t6 + 1] > 1e5 and np.isfinite(scaled[t6 + 1]).all()                               # the 1e-7 clamp: a huge scale
    assert np.isfinite(scaled).all() and np.isfinite(tr).all() and np.isfinite(rot).all()
    c = d["centres"]
    assert len({tuple(row) for row in c}) == len(c) and not c[TB.ZERO_CENTRE].any()
    f32 = np.array([np.array_equal(row, row.astype(np.float32).astype(np.float64)) for row in c])
    assert f32[TB.F32_CENTRE] and not f32[[1, 2, 5, TB.FAR_CENTRE]].any()
    p = d["pairs"].reshape(T, 2, 3)
    assert np.isnan(p).any() and np.isposinf(p).any() and np.isneginf(p).any()
    fin = np.isfinite(p).all((1, 2))
    assert (fin & (p[:, 0] == p[:, 1]).all(1)).sum() >= 34
    tr, rot = TB.target_pairs_batch(d["pairs"], tup, TB.AXES, c)
    assert np.array_equal(np.isnan(tr).any(1), ~fin) and np.array_equal(np.isnan(rot).any(1), ~fin)
    assert tr[t6 + 3, 1] < 1e-5 and tr[int(tup[8]) + 3, 1] < 1e-3 and np.nanmin(tr[:, 1]) >= 0       # through the centre


# what each mistake must change, in every scene that holds tuples; a scene is exempt only where the mistake cannot show at all:
#  * "find_first" differs from the right lookup only where an empty scene shares the offset: scenes 1 and 5;
#  * scene 2 has ONE point: real_len = 0 there, so scaled = +-0, scale = 0 and the vote parameters are those of a == b whatever the
#    base, the norms and the clamps; only "den_nb" can still show, as the sign of a zero: for odd nb, where the middle bin's
#    coordinate is +0 under nb - 1 and negative under nb;
#  * "pred_unfused" shows nowhere when nb - 1 is a power of two (TB.dyadic: fused and unfused agree on every bin difference);
#  * "unit_clamp_max" shows in target_pairs wherever a != b: not in scene 2;
#  * "centre_f32" cannot show where the centre is a float32: the zero centre and the float32 one.
def _blind_decode(variant, b, nb):
    if variant == "find_first":
        return b not in TB.AFTER_EMPTY
    if variant == "pred_unfused" and TB.dyadic(nb):
        return True
    if b == TB.ONE_POINT_SCENE:
        return not (variant == "den_nb" and nb % 2 == 1)
    return False


def _blind_pairs(variant, b):
    if variant == "find_first":
        return b not in TB.AFTER_EMPTY
    if variant == "unit_clamp_max":
        return b == TB.ONE_POINT_SCENE
    if variant == "centre_f32":
        return b in (TB.ZERO_CENTRE, TB.F32_CENTRE)
    return False


@pytest.mark.parametrize("variant", TB.DECODE_VARIANTS)
@pytest.mark.parametrize("k,nb", SHAPES)
def test_every_wrong_decode_differs_in_every_scene(k, nb, variant):
    d = TB.ragged_batch(k, nb)
    args = (nb, d["pts"], d["idx"], d["pt_off"], d["tup_off"], TB.AXES)
    scenes = TR.scene_slices(d["tup_off"])
    assert [b for b, _, _ in scenes] == [1, 2, 5, 6, 7, 8]
    seen = 0
    for bins in (d["bins"], TB.exact_bins(nb, d["idx"].shape[0])):
        differ = TB.rows_differ(TB.decode_batch(bins, *args), TB.decode_batch(bins, *args, variant=variant))
        for b, t0, t1 in scenes:
            if bins is not d["bins"] and t1 - t0 < 256:
                continue                                   # (the crafted first tuple belongs to the batch's own bins)
            if _blind_decode(variant, b, nb):
                assert not differ[t0:t1].any(), "the exemption of (%s, scene %d) is no longer needed" % (variant, b)
            else:
                assert differ[t0:t1].any(), "%s is not told from the right kernel in scene %d" % (variant, b)
                seen += 1
            if variant in TB.PER_TUPLE and not _blind_decode(variant, b, nb) and bins is d["bins"] and b != TB.ONE_POINT_SCENE:
                assert differ[t0], "the crafted first tuple of scene %d does not show %s" % (b, variant)
    assert seen >= 2 or (variant == "pred_unfused" and TB.dyadic(nb))


@pytest.mark.parametrize("variant", TB.PAIR_VARIANTS)
@pytest.mark.parametrize("k", [2, 5, 8])
def test_every_wrong_target_pair_differs_in_every_scene(k, variant):
    d = TB.ragged_batch(k, 32)
    right = TB.target_pairs_batch(d["pairs"], d["tup_off"], TB.AXES, d["centres"])
    wrong = TB.target_pairs_batch(d["pairs"], d["tup_off"], TB.AXES, d["centres"], variant)
    differ = TB.rows_differ(right, wrong)
    seen = 0
    for b, t0, t1 in TR.scene_slices(d["tup_off"]):
        if _blind_pairs(variant, b):
            assert not differ[t0:t1].any(), "the exemption of (%s, scene %d) is no longer needed" % (variant, b)
        else:
            assert differ[t0:t1].any(), "%s is not told from the right kernel in scene %d" % (variant, b)
            seen += 1
    assert seen >= 2
    # without centres every scene's centre is zero: not the zero-centre scene's result alone
    none = TB.target_pairs_batch(d["pairs"], d["tup_off"], TB.AXES, None)
    for b, t0, t1 in TR.scene_slices(d["tup_off"]):
        assert TB.rows_differ(right, none)[t0:t1].any() == (b != TB.ZERO_CENTRE)


def test_the_cap_batch_lies_past_one_pass_of_the_grid():
    assert sum(TB.CAP_TUPLES) == TB.CAP_T == 65535 * 256 + 257 and TB.CAP_T % 256
    assert TB.CAP_TUPLES[1] > 65535 * 256 and TB.CAP_BLOCK % 2 == 1 and 3900 < TB.CAP_BLOCK < 4100
    p = TB.cap_block()
    off = TR.offsets([TB.CAP_BLOCK])
    a = TB.target_pairs_batch(p, off, TB.AXES, TB.CAP_CENTRES[1:2])
    b = TB.target_pairs_batch(p, off, TB.AXES, TB.CAP_CENTRES[3:4])
    fin = np.isfinite(p).all(1)
    assert (~fin).sum() == 3 and TB.rows_differ(a, b)[fin].all()                 # the two scenes' centres tell on every row


# ---------------------------------------------------------------------------------------------------------------
# the margin comparison's cap cannot hide a failure
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", MARGIN_NB)
def test_few_random_draws_lie_near_a_cdf_edge(nb):
    """tests/test_tuple_back_gpu.py lets a bin differ where the oracle's margin is below 1e-5 and asserts that fewer than 1e-3 of the
    draws differ: with fewer than 1e-3 of the draws that near an edge, the second bound never excuses what the first forbids."""
    d = TB.ragged_batch(5, nb)
    T = d["idx"].shape[0]
    pairs = np.zeros((T, 2, 3), np.float32)
    margin = np.stack([O.decode_bins(d["logits"], u, pairs, return_margin=True)[4] for u in d["uniforms"]])
    share = float((margin < 1e-5).mean())
    print("SHARE nb = %d: %d of %d draws within 1e-5 of a CDF edge (%.2e)" % (nb, (margin < 1e-5).sum(), margin.size, share))
    assert margin.shape == (TB.UNIFORM_SETS, T, 6) and share < 1e-3
