"""Plain host restatement of the tuple back end (cppf2_amd/csrc/cppf_core.hip from decode_bins_kernel on: the bin draw, the
vote-parameter decode and generate_target_pairs) for ragged batches.

NumPy only, one loop per scene, built on the oracle's single-scene functions (O.softmax_cdf, O._norm3, O.generate_target_pairs;
O.decode_bins is what tests/test_tuple_back_ref.py pins draw() + decode_batch() to).  Apart from the float64 acos behind `rot`
every output is a chain of exact IEEE operations, so tests/test_tuple_back_gpu.py compares the kernels with it bit for bit (`rot`:
one float32 ulp).

`variant` selects a deliberately WRONG restatement (the mistakes a kernel of this family can make without the single-scene
tests noticing); tests/test_tuple_back_ref.py checks that the inputs built here tell each of them from the right one.
"""
import numpy as np

import tuple_front_ref as TR
from oracle import cppf_oracle as O

F32, F64 = np.float32, np.float64
VARIANTS = ("find_first", "neighbour_base", "draw_lt", "den_nb", "real_fused", "pred_unfused", "pred_clamp_add", "unit_clamp_max",
            "centre_f32", "centre_scene0")
DECODE_VARIANTS = ("find_first", "neighbour_base", "den_nb", "real_fused", "pred_unfused", "pred_clamp_add", "unit_clamp_max")
PAIR_VARIANTS = ("find_first", "unit_clamp_max", "centre_f32", "centre_scene0")
PER_TUPLE = ("den_nb", "real_fused", "pred_unfused", "pred_clamp_add", "unit_clamp_max")      # can show in any tuple with two points

# general float64 axes (no component is a float32): the three dot products of target_pair all count
AXES = np.array([[0.1, 0.9, -0.3], [0.7, -0.2, 0.6], [-0.4, 0.3, 0.8]], dtype=F64)


# ---------------------------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------------------------
def draw(logits, prior, uniforms, variant=None):
    """Bins int32 [...] of the inverse-CDF draw: logits [..., nb] (+ prior, one float32 add), uniforms [...].  The first j with
    cdf[j] > target = #{j: cdf[j] <= target}, clamped to nb - 1; "draw_lt" counts cdf[j] < target."""
    assert variant in (None, "draw_lt")
    x = np.asarray(logits, dtype=F32)
    if prior is not None:
        x = (x + np.asarray(prior, dtype=F32)).astype(F32)
    nb = x.shape[-1]
    _, cdf, acc = O.softmax_cdf(x)
    target = (np.asarray(uniforms, dtype=F32).reshape(acc.shape) * acc).astype(F32)
    below = cdf < target[..., None] if variant == "draw_lt" else cdf <= target[..., None]
    return np.minimum(below.sum(-1), nb - 1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------
# vote parameters from bins, and from pairs
# ---------------------------------------------------------------------------------------------------------------
def _scene_of(b, tup_off, variant):
    """The scene a row of scene b is served from.  find_scene must return the LAST scene among equal offsets (the empty scenes
    before b share tup_off[b]); "find_first" returns the first."""
    if variant != "find_first":
        return b
    return int(np.searchsorted(np.asarray(tup_off), tup_off[b], side="left"))


def _base(b, pt_off, variant):
    B = len(pt_off) - 1
    if variant == "neighbour_base":
        return int(pt_off[b + 1 if b + 1 < B else b - 1])
    return int(pt_off[b])


def _norm3_unfused(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(F32)


def _target_pairs(pp, axes, centre, variant):
    """O.generate_target_pairs; "unit_clamp_max" restates it with max(n, 1e-7) under the unit vector ("_local": the same lines
    with the right n + 1e-7, which tests/test_tuple_back_ref.py holds to the oracle)."""
    if variant not in ("unit_clamp_max", "_local"):
        return O.generate_target_pairs(pp, axes[0], axes[1], axes[2], center=centre)
    pp = np.asarray(pp, dtype=F32)
    centre = np.zeros(3) if centre is None else np.asarray(centre, dtype=F64)
    a, b = pp[:, 0], pp[:, 1]
    d = a - b
    n = _norm3_unfused(d)
    den = np.maximum(n, F32(1e-7)) if variant == "unit_clamp_max" else (n + F32(1e-7)).astype(F32)
    u64 = (d / den[:, None]).astype(F32).astype(F64)
    ac = a.astype(F64) - centre
    p = ac * u64
    proj = (p[:, 0] + p[:, 1]) + p[:, 2]
    oc = ac - proj[:, None] * u64
    dist = np.sqrt((oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1]) + oc[:, 2] * oc[:, 2])
    rots = []
    for ax in axes:
        q = u64 * np.asarray(ax, dtype=F64)
        rots.append(np.arccos((q[:, 0] + q[:, 1]) + q[:, 2]))
    return np.stack([proj, dist], -1).astype(F32), np.stack(rots, -1).astype(F32)


def decode_scene(bins, nb, a, b, axes, variant=None):
    """eval.py:230-240 on the tuples of one scene: bins [T, 6], pair ends a, b float32 [T, 3].  Returns scaled [T, 6], scale [T],
    tr [T, 2], rot [T, 3]."""
    bins = np.asarray(bins)
    den = F32(nb if variant == "den_nb" else nb - 1)
    pred = (bins.astype(F32).reshape(-1, 2, 3) / den - F32(0.5)).astype(F32)                 # eval.py:230
    d = (b - a).astype(F32)
    real_len = O._norm3(d) if variant == "real_fused" else _norm3_unfused(d)                 # np.linalg.norm, eval.py:233
    pd = (pred[:, 1] - pred[:, 0]).astype(F32)
    pred_len = _norm3_unfused(pd) if variant == "pred_unfused" else O._norm3(pd)             # torch.norm, eval.py:234
    floor = (pred_len + F32(1e-7)).astype(F32) if variant == "pred_clamp_add" else np.maximum(pred_len, F32(1e-7))
    with np.errstate(all="ignore"):
        scale = (real_len / floor).astype(F32)
        scaled = (pred * scale[:, None, None]).astype(F32)                                   # eval.py:235
        tr, rot = _target_pairs(scaled, axes, None, variant)
    return scaled.reshape(-1, 6), scale, tr, rot


def decode_batch(bins, nb, pts, idx, pt_off, tup_off, axes, variant=None):
    """cppf_decode_from_bins (= the second phase of cppf_decode_bins) on a ragged batch: bins int32 [T, 6], pts float32 [N, 3],
    idx [T, k] LOCAL indices; the pair of tuple t of scene b is pts[pt_off[b] + idx[t, 0 / 1]].  Returns scaled float32 [T, 6],
    scale [T], tr [T, 2], rot [T, 3]."""
    assert variant is None or variant in DECODE_VARIANTS
    pts, idx, bins = np.asarray(pts, dtype=F32), np.asarray(idx), np.asarray(bins)
    N, T = pts.shape[0], idx.shape[0]
    assert bins.shape == (T, 6) and tup_off[-1] == T and pt_off[-1] == N and bins.min(initial=0) >= 0 and bins.max(initial=0) < nb
    scaled, scale, tr, rot = np.zeros((T, 6), F32), np.zeros(T, F32), np.zeros((T, 2), F32), np.zeros((T, 3), F32)
    for b in range(len(pt_off) - 1):
        t0, t1 = int(tup_off[b]), int(tup_off[b + 1])
        if t1 == t0:
            continue
        li = idx[t0:t1, :2].astype(np.int64)
        assert li.min() >= 0 and li.max() < int(pt_off[b + 1] - pt_off[b])
        p0 = _base(_scene_of(b, tup_off, variant), pt_off, variant)
        pa, pb = pts[(p0 + li[:, 0]) % N], pts[(p0 + li[:, 1]) % N]       # (only a wrong base can reach past the batch: wrapped)
        scaled[t0:t1], scale[t0:t1], tr[t0:t1], rot[t0:t1] = decode_scene(bins[t0:t1], nb, pa, pb, axes, variant)
    return scaled, scale, tr, rot


def target_pairs_batch(pairs, tup_off, axes, centres, variant=None):
    """cppf_generate_target_pairs on a ragged batch: pairs float32 [T, 6], centres float64 [B, 3] or None (every centre 0).
    Returns tr float32 [T, 2], rot [T, 3]."""
    assert variant is None or variant in PAIR_VARIANTS
    pairs = np.asarray(pairs, dtype=F32).reshape(-1, 2, 3)
    T = pairs.shape[0]
    assert tup_off[-1] == T
    tr, rot = np.zeros((T, 2), F32), np.zeros((T, 3), F32)
    for b in range(len(tup_off) - 1):
        t0, t1 = int(tup_off[b]), int(tup_off[b + 1])
        if t1 == t0:
            continue
        c = None
        if centres is not None:
            c = np.asarray(centres, dtype=F64)[0 if variant == "centre_scene0" else _scene_of(b, tup_off, variant)]
            if variant == "centre_f32":
                c = c.astype(F32).astype(F64)
        with np.errstate(all="ignore"):
            tr[t0:t1], rot[t0:t1] = _target_pairs(pairs[t0:t1], axes, c, variant)
    return tr, rot


# ---------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------
def ulps(got, want):
    """Distance in float32 steps between two float32 arrays (int64; NaN positions count 0: compare those with np.isnan)."""
    def ordered(a):
        i = np.ascontiguousarray(a, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(ordered(got) - ordered(want))
    d[np.isnan(got) | np.isnan(want)] = 0
    return d


def rows_differ(right, wrong):
    """bool [T]: the rows in which any output of two (scaled, scale, tr, rot) / (tr, rot) tuples differs in a bit."""
    out = np.zeros(right[0].shape[0], bool)
    for r, w in zip(right, wrong):
        out |= (TR.bits(r) != TR.bits(w)).reshape(r.shape[0], -1).any(1)
    return out


# ---------------------------------------------------------------------------------------------------------------
# rows whose CDF is exact: every unmasked logit equal, so softmax_exp(0) = 1 and the running sum counts 1 .. S
# ---------------------------------------------------------------------------------------------------------------
EXACT_NB = (2, 3, 20, 31, 32, 33, 64, 4096)
MASKED = (-np.inf, -200.0, -1000.0, -3.0e38)     # relative to the row's level: exp() of all of them is 0 in float32 on both sides
LEVELS = (0.0, 1.5, -3.0, 64.0)
ONE_BELOW = F32(1.0 - 2.0 ** -24)


def _masks(nb, rng):
    """Unmasked-bin patterns (at least one bin each): all, all but the first / last, the trailing / leading part, every other bin,
    one bin only, random halves."""
    m = [np.ones(nb, bool)]
    for lo, hi in ((1, nb), (0, nb - 1), (nb // 2, nb), (0, nb - nb // 3), (nb - 1, nb), (0, 1)):
        p = np.zeros(nb, bool)
        p[lo:hi] = True
        m.append(p)
    p = np.zeros(nb, bool)
    p[::2] = True
    m.append(p)
    for _ in range(2):
        p = rng.rand(nb) < 0.5
        p[rng.randint(nb)] = True
        m.append(p)
    return m


def exact_rows(nb, flat=False, seed=0):
    """(rows float32 [R, nb], u float32 [R], S int [R]): flat rows (every unmasked logit at the row's level, masked ones -inf or
    at least 200 below) with the uniforms j / S, the float32 below and the one above, and 0, 1 - 2^-24 and 1.0 on a few rows.
    No row is masked entirely.  flat: no masking at all (S = nb in every row)."""
    rng = np.random.RandomState(300 + nb + seed)
    rows, us = [], []
    for i, mask in enumerate([np.ones(nb, bool)] * 6 if flat else _masks(nb, rng)):
        S = int(mask.sum())
        level = F32(LEVELS[i % len(LEVELS)])
        row = np.full(nb, level, F32)
        low = np.array([MASKED[(i + (j if i % 5 == 4 else 0)) % len(MASKED)] for j in range(nb)], F32)    # one kind, or all mixed
        row[~mask] = (level + low)[~mask]
        near = {0, 1, 2, S // 3, S // 2, S // 2 + 1, 2 * S // 3, S - 2, S - 1}
        js = sorted(set(range(S)) if S <= 10 else near | set(rng.randint(0, S, 4 if flat else 1).tolist()))
        u = []
        for j in js:
            c = F32(F32(j) / F32(S))
            u += [c, np.nextafter(c, F32(2)), max(np.nextafter(c, F32(-1)), F32(0))]
        if i < 4:
            u += [F32(0), ONE_BELOW, F32(1)]
        rows += [row] * len(u)
        us += u
    rows, us = np.stack(rows), np.array(us, dtype=F32)
    S = (rows == rows.max(1, keepdims=True)).sum(1)
    assert np.all((us >= 0) & (us <= 1)) and np.isfinite(rows.max(1)).all()
    return rows, us, S


def exact_batch(nb, flat=False):
    """The exact rows as a decode batch: (logits float32 [T, 6, nb], uniforms [T, 6]), the tail padded with the first rows."""
    rows, us, _ = exact_rows(nb, flat)
    T = (rows.shape[0] + 5) // 6
    sel = np.arange(T * 6) % rows.shape[0]
    return rows[sel].reshape(T, 6, nb), us[sel].reshape(T, 6)


PRIOR_CASES = ("flat_sum", "mask_in_prior", "mask_in_logits")


def prior_split(rows, case, seed=0):
    """(logits, prior) whose float32 sum is `rows` bit for bit, neither of them flat: a varying finite part on one side and its
    complement on the other.  "flat_sum": for rows without masking; "mask_in_prior" / "mask_in_logits": the masking on that side
    only and the other side finite."""
    assert case in PRIOR_CASES
    rows = np.asarray(rows, dtype=F32)
    rng = np.random.RandomState(400 + len(case) + seed)
    assert case != "flat_sum" or np.all(rows == rows.max(-1, keepdims=True))
    part = (rng.randint(-16, 17, rows.shape) / 4.0).astype(F32)          # quarters: the complement and the sum are exact
    part[..., 0] = np.where(part[..., 0] == part[..., 1], part[..., 1] - F32(0.5), part[..., 0])     # never flat, even at nb = 2
    rest = (rows - part).astype(F32)                                      # (-inf and -3e38 absorb the part, both ways)
    logits, prior = (rest, part) if case == "mask_in_logits" else (part, rest)
    assert np.array_equal(TR.bits((logits + prior).astype(F32)), TR.bits(rows))
    assert np.isfinite(prior if case == "mask_in_logits" else logits).all()
    return logits, prior


# ---------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests (built here so that the CPU file checks the very same arrays)
# ---------------------------------------------------------------------------------------------------------------
# empty scenes first, twice in the middle and last; boundaries at 1, 34, 65, 322, 578 and 1581: inside 32-tuple and 256-thread
# blocks, the total a multiple of neither.  Scene 2 has ONE point: i0 == i1 and real_len = 0 in all its tuples.
RAGGED_TUPLES = [0, 1, 33, 0, 0, 31, 257, 256, 1003, 0]
RAGGED_POINTS = [3, 7, 1, 4, 0, 17, 300, 40, 64, 2]
ONE_POINT_SCENE = 2
AFTER_EMPTY = (1, 5)          # the scenes a "find_first" lookup serves from another scene
ZERO_CENTRE, F32_CENTRE, FAR_CENTRE = 6, 7, 8
UNIFORM_SETS = 4


def dyadic(nb):
    """nb - 1 a power of two: bin coordinates are short dyadic fractions and the fused and unfused pred_len agree everywhere."""
    return (nb - 1) & (nb - 2) == 0


def _offset_scale(b):
    return F32(1.0 + 0.75 * b), F32(0.05 * (1 + b % 3))


def _craft(rng, nb, b, axes, tries=4000):
    """A pair of points of scene b and the bins of one tuple on which every per-tuple mistake shows (fused and unfused norms differ
    on about a tenth of the inputs only, so the first tuple of every scene is chosen, not drawn)."""
    off, scl = _offset_scale(b)
    pa = (off + scl * rng.rand(tries, 3)).astype(F32)
    pb = (off + scl * rng.rand(tries, 3)).astype(F32)
    bins = rng.randint(0, nb, (tries, 6)).astype(np.int32)
    right = decode_scene(bins, nb, pa, pb, axes)
    ok = np.ones(tries, bool)
    for v in PER_TUPLE:
        if not (v == "pred_unfused" and dyadic(nb)):
            ok &= rows_differ(right, decode_scene(bins, nb, pa, pb, axes, v))
    i = int(np.argmax(ok))
    assert ok[i]
    return pa[i], pb[i], bins[i]


def ragged_batch(k, nb, seed=0):
    """The ragged batch of the back end for one tuple size and bin count: dict(pts, idx, pt_off, tup_off, bins, logits [T, 6, nb],
    uniforms [UNIFORM_SETS, T, 6], centres, pairs).  Scene b's points lie at their own offset and scale, so a wrong base changes the values; the first tuple of
    every scene with two points or more is (0, n - 1) with crafted ends and bins, the second has both ends in one bin (pred_len = 0:
    the 1e-7 clamp), the third in adjacent bins.  centres: float64 [B, 3], near the scene's points and no float32 (scenes 1, 2, 5),
    all zero (6), a float32 (7), far (8); the empty scenes' centres are different from all of them.  pairs: the real pairs of the
    batch, with a == b, a pair through the centre and NaN / inf coordinates among them."""
    rng = np.random.RandomState(2000 + 31 * k + nb + seed)
    pt_off, tup_off = TR.offsets(RAGGED_POINTS), TR.offsets(RAGGED_TUPLES)
    B, N, T = len(RAGGED_POINTS), int(pt_off[-1]), int(tup_off[-1])
    pts = rng.rand(N, 3).astype(F32)
    idx = np.zeros((T, k), dtype=np.int32)
    bins = rng.randint(0, nb, (T, 6)).astype(np.int32)
    centres = np.zeros((B, 3), dtype=F64)
    for b, (n, nt) in enumerate(zip(RAGGED_POINTS, RAGGED_TUPLES)):
        off, scl = _offset_scale(b)
        p0, t0 = int(pt_off[b]), int(tup_off[b])
        pts[p0:p0 + n] = off + scl * pts[p0:p0 + n]
        centres[b] = float(off) + float(scl) * np.array([0.37, 0.61, 0.43]) if nt else np.array([7.3, -3.1, 1.7]) * (b + 1)
        if nt == 0:
            continue
        li = rng.randint(0, n, (nt, k)).astype(np.int32)
        li[-1, k - 1] = n - 1
        li[0, 0], li[0, 1] = 0, n - 1
        idx[t0:t0 + nt] = li
        if n >= 2:
            pts[p0], pts[p0 + n - 1], bins[t0] = _craft(rng, nb, b, AXES)
        if nt >= 4:
            bins[t0 + 1, 3:] = bins[t0 + 1, :3]
            bins[t0 + 2, 3:] = bins[t0 + 2, :3]
            bins[t0 + 2, 4] += 1 if bins[t0 + 2, 4] + 1 < nb else -1
    centres[ZERO_CENTRE] = 0.0
    centres[F32_CENTRE] = centres[F32_CENTRE].astype(F32)
    centres[FAR_CENTRE] = [101.3, -707.1, 303.7]
    logits = (rng.randn(T, 6, nb) * 3).astype(F32) if nb <= 64 else None
    uniforms = rng.rand(UNIFORM_SETS, T, 6).astype(F32)       # several draws from the same logits: a steadier near-edge share
    uniforms[0, tup_off[5]], uniforms[0, tup_off[5] + 1] = 0.0, ONE_BELOW
    # the real pairs, and the special ones (never a scene's first row)
    pairs = np.zeros((T, 6), F32)
    for b in range(B):
        t0, t1, p0 = int(tup_off[b]), int(tup_off[b + 1]), int(pt_off[b])
        pairs[t0:t1] = pts[p0 + idx[t0:t1, :2]].reshape(-1, 6)
    t6, t8, t5 = int(tup_off[ZERO_CENTRE]), int(tup_off[FAR_CENTRE]), int(tup_off[5])
    pairs[t6 + 3, 3:] = -pairs[t6 + 3, :3]                                   # through the zero centre, exactly
    c8 = centres[FAR_CENTRE]
    pairs[t8 + 3] = np.concatenate([c8 + [0.5, 0.25, -0.125], c8 - [0.5, 0.25, -0.125]]).astype(F32)   # through the far one, nearly
    pairs[t8 + 4, 3:] = pairs[t8 + 4, :3]                                    # a == b
    pairs[t8 + 5, 1], pairs[t8 + 6, 3], pairs[t8 + 7, 2], pairs[t8 + 8, 4] = np.nan, np.inf, -np.inf, np.nan
    pairs[t8 + 9] = np.inf
    pairs[t5 + 3, 0], pairs[t5 + 4, 5] = np.nan, np.inf
    return {"k": k, "nb": nb, "pts": pts, "idx": idx, "pt_off": pt_off, "tup_off": tup_off, "bins": bins, "logits": logits,
            "uniforms": uniforms, "centres": centres, "pairs": pairs}


def exact_bins(nb, T):
    """The bins of the exact draw, repeated to [T, 6]."""
    logits, u = exact_batch(nb)
    return np.resize(draw(logits, None, u).reshape(-1), (T, 6)).astype(np.int32)


# past the grid cap of cppf_generate_target_pairs: 65535 workgroups of 256 threads
CAP_T = 65535 * 256 + 257
CAP_TUPLES = [0, 65535 * 256 + 40, 0, 217]       # the boundary 40 tuples past what one pass of the grid covers
CAP_BLOCK = 4001                                  # odd: coprime to 256, so every row of the block meets every thread slot
CAP_CENTRES = np.array([[3.3, 1.1, -2.7], [0.37, -0.61, 0.43], [-5.1, 4.7, 9.9], [-0.83, 0.29, 0.71]], dtype=F64)


def cap_block(seed=0):
    """float32 [CAP_BLOCK, 6]: random pairs with a == b, NaN and inf rows among them."""
    rng = np.random.RandomState(55 + seed)
    p = rng.randn(CAP_BLOCK, 6).astype(F32)
    p[7, 3:] = p[7, :3]
    p[11, 0], p[13, 4], p[17, 2] = np.nan, np.inf, -np.inf
    return p
