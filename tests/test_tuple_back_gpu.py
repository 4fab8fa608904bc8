"""The tuple back end (cppf2_amd/csrc/cppf_core.hip from decode_bins_kernel on: the bin draw, the vote-parameter decode and
generate_target_pairs) against the plain host restatement of tests/tuple_back_ref.py on ragged batches.  Bins, `scaled`, `scale` and
`tr` are compared bit for bit (through the uint32 view; a NaN `tr` that NaN / inf coordinates produce is compared by position);
`rot` is a float64 acos rounded to float32 and may differ by one float32 ulp.  Every output lies in a buffer filled with a sentinel,
with guard rows before and after.  tests/test_tuple_back_ref.py pins the restatement, shows that the exact inputs are exact and
checks on the CPU that these inputs tell a wrong kernel from a right one.

Which test launches which kernel:
  decode_bins_kernel<32>      test_exact_draw[32-*], test_decode_bins_second_phase[*-32], test_null_outputs_in_turn[32],
                              test_random_logits_on_the_ragged_batch[32]
  decode_bins_kernel<0>       test_exact_draw (every other nb), test_decode_bins_second_phase (nb != 32),
                              test_null_outputs_in_turn[20], test_random_logits_on_the_ragged_batch[20], [33]
  decode_targets_kernel       test_decode_from_bins_ragged, test_null_outputs_in_turn
  target_pairs_kernel         test_target_pairs_ragged, test_target_pairs_past_the_grid_cap (the grid-stride loop)
  the decode epilogue of cppf_reslayer_split_decode[_prior]   test_fused_draw_on_the_exact_rows
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tuple_back_ref as TB  # noqa: E402
import tuple_front_ref as TR  # noqa: E402
from oracle import cppf_oracle as O  # noqa: E402
from test_tuple_front_gpu import GUARD, SENT, _dev, _gpu, _guards_untouched, _words  # noqa: E402

COLS = {"bins": 6, "scaled": 6, "scale": 1, "tr": 2, "rot": 3}
FROM_BINS = ("scaled", "scale", "tr", "rot")
WORST_ROT = {"ulps": 0}          # the largest rot difference seen in this run (printed by the tests that compare rot)
NULL = C.c_void_p(0)


def _axes(axes=TB.AXES):
    return (C.c_double * 9)(*[float(v) for v in np.asarray(axes).reshape(9)])


def _outs(T, names, null=()):
    """{name: (guarded sentinel buffer | None, pointer)} -- the names in `null` get a null pointer."""
    return {n: ((None, NULL) if n in null else _words(T, COLS[n])) for n in names}


def _read(outs):
    """{name: array} of the outputs that were asked for; asserts the guards."""
    got = {}
    for n, (buf, _) in outs.items():
        if buf is not None:
            h = np.ascontiguousarray(_guards_untouched(buf))
            got[n] = h if n == "bins" else h.view(np.float32).reshape(-1) if n == "scale" else h.view(np.float32)
    return got


def _scene(off, r):
    return int(np.searchsorted(np.asarray(off), r, side="right") - 1)


def _same_bits(name, got, want, off=None, nan_by_position=False):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = TR.bits(got) != TR.bits(want)
    if nan_by_position:
        assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaNs at other positions" % name
        bad &= ~np.isnan(want)
    if bad.any():
        r = int(np.argwhere(bad.reshape(got.shape[0], -1))[0][0])
        raise AssertionError("%s: %d values differ; first in row %d%s: got %r, want %r" % (
            name, bad.sum(), r, "" if off is None else " (scene %d)" % _scene(off, r), got[r], want[r]))


def _rot_within_one_ulp(got, want, off=None):
    assert np.array_equal(np.isnan(got), np.isnan(want)), "rot: NaNs at other positions"
    d = TB.ulps(got, want)
    WORST_ROT["ulps"] = max(WORST_ROT["ulps"], int(d.max(initial=0)))
    if d.max(initial=0) > 1:
        r = int(np.argwhere(d.max(1) > 1)[0][0])
        raise AssertionError("rot: %d values differ by more than one ulp, at most %d; first in row %d%s: got %r, want %r" % (
            (d > 1).sum(), d.max(), r, "" if off is None else " (scene %d)" % _scene(off, r), got[r], want[r]))


def _held_to_restatement(got, want, off, rows=None):
    """The criteria of the decode: scaled, scale and tr bit for bit, rot to one ulp (rows: a boolean selection)."""
    sel = slice(None) if rows is None else rows
    for n, w in zip(FROM_BINS, want):
        if n not in got:
            continue
        if n == "rot":
            _rot_within_one_ulp(got[n][sel], w[sel], off if rows is None else None)
        else:
            _same_bits(n, got[n][sel], w[sel], off if rows is None else None)


_BATCH = {}


def _batch(k, nb):
    """The ragged batch on the host and on the device, and the restatement of its own bins, computed once per shape."""
    if (k, nb) not in _BATCH:
        d = TB.ragged_batch(k, nb)
        d["want"] = TB.decode_batch(d["bins"], nb, d["pts"], d["idx"], d["pt_off"], d["tup_off"], TB.AXES)
        d["dev"] = {n: _dev(d[n]) for n in ("pts", "idx", "pt_off", "tup_off")}
        _BATCH[(k, nb)] = d
    return _BATCH[(k, nb)]


def _decode_from_bins(d, bins, null=()):
    from cppf2_amd import _lib, ops
    g, T = d["dev"], d["idx"].shape[0]
    outs = _outs(T, FROM_BINS, null)
    d_bins = _dev(np.ascontiguousarray(bins, dtype=np.int32))
    _lib.check(ops._L.cppf_decode_from_bins(len(d["pt_off"]) - 1, ops._p(d_bins), d["nb"], ops._p(g["pts"]), ops._p(g["idx"]), d["k"],
                                            ops._p(g["pt_off"]), ops._p(g["tup_off"]), T, _axes(), outs["scaled"][1], outs["scale"][1],
                                            outs["tr"][1], outs["rot"][1], ops._stream()), "cppf_decode_from_bins")
    return _read(outs)


def _decode_bins(d, logits, uniforms, prior=None, null=(), B=None, names=("bins",) + FROM_BINS):
    """cppf_decode_bins (prior None) / cppf_decode_bins_prior on device tensors logits [T, 6, nb], uniforms [T, 6]."""
    from cppf2_amd import _lib, ops
    g, T = d["dev"], logits.shape[0]
    outs = _outs(T, ("bins",) + FROM_BINS, tuple(null) + tuple(n for n in COLS if n not in names))
    tail = (ops._p(g["pts"]), ops._p(g["idx"]), d["k"], ops._p(g["pt_off"]), ops._p(g["tup_off"]), T, _axes(), outs["bins"][1],
            outs["scaled"][1], outs["scale"][1], outs["tr"][1], outs["rot"][1], ops._stream())
    B = len(d["pt_off"]) - 1 if B is None else B
    if prior is None:
        _lib.check(ops._L.cppf_decode_bins(B, ops._p(logits), logits.shape[2], ops._p(uniforms), *tail), "cppf_decode_bins")
    else:
        _lib.check(ops._L.cppf_decode_bins_prior(B, ops._p(logits), ops._p(prior), logits.shape[2], ops._p(uniforms), *tail),
                   "cppf_decode_bins_prior")
    return _read(outs)


def _one_hot(bins, nb):
    """Logits that draw exactly `bins` at any uniform below 1: 0 at the bin, -inf elsewhere (S = 1)."""
    import torch
    b = _dev(np.ascontiguousarray(bins, dtype=np.int64))
    lg = torch.full(tuple(b.shape) + (nb,), float("-inf"), dtype=torch.float32, device=b.device)
    lg.scatter_(2, b[:, :, None], 0.0)
    return lg, torch.full(tuple(b.shape), 0.5, dtype=torch.float32, device=b.device)


# ---------------------------------------------------------------------------------------------------------------
# 3a. the draw on rows whose CDF is exact
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("no_prior",) + TB.PRIOR_CASES)
@pytest.mark.parametrize("nb", TB.EXACT_NB)
def test_exact_draw(nb, form):
    """Flat and masked rows: the CDF counts 1 .. S on both sides, the uniforms sit on the CDF's values (j / S: exact ties on a
    fifth of the rows at least), one float32 below and one above, at 0, at 1 - 2^-24 and at 1.0 (the clamp).  The rule is
    cdf[j] <= target: a kernel that draws with < differs on every tie.  With a prior the sum logits + prior is the same row, bit
    for bit, whichever side carries the masking.  nb = 32 is the template kernel, every other nb the generic one."""
    rows, u, _ = TB.exact_rows(nb, flat=form == "flat_sum")
    R = rows.shape[0]
    T = (R + 5) // 6
    sel = np.arange(T * 6) % R
    rows, u = rows[sel].reshape(T, 6, nb), u[sel].reshape(T, 6)
    logits, prior = (rows, None) if form == "no_prior" else TB.prior_split(rows, form)
    want = TB.draw(logits, prior, u)
    assert np.array_equal(want, TB.draw(rows, None, u))
    d = {"k": 2, "nb": nb, "pt_off": TR.offsets([2]),
         "dev": {"pts": _dev(np.array([[0, 0, 0], [1, 2, 3]], np.float32)), "idx": _dev(np.tile(np.array([[0, 1]], np.int32), (T, 1))),
                 "pt_off": _dev(TR.offsets([2])), "tup_off": _dev(TR.offsets([T]))}}
    got = _decode_bins(d, _dev(logits), _dev(u), None if prior is None else _dev(prior), names=("bins",))
    assert list(got) == ["bins"]
    _same_bits("bins", got["bins"], want)
    assert (got["bins"] != TB.draw(logits, prior, u, "draw_lt")).sum() >= max(3, R // 10)


# ---------------------------------------------------------------------------------------------------------------
# 3b. vote parameters from bins, on the ragged batch
# ---------------------------------------------------------------------------------------------------------------
BIN_SHAPES = [(k, nb) for nb in (2, 20, 32, 33, 4096) for k in (2, 5, 8)]


@pytest.mark.parametrize("k,nb", BIN_SHAPES)
def test_decode_from_bins_ragged(k, nb):
    """cppf_decode_from_bins on ten scenes of 0 .. 1003 tuples (empty ones first, twice in the middle and last; boundaries inside
    32-tuple and 256-thread blocks; a one-point scene; every scene's points at their own offset): the batch's own bins -- random,
    with a crafted first tuple per scene, both ends in one bin (the 1e-7 clamp, a huge scale) and adjacent bins -- and the bins of
    the exact draw."""
    d = _batch(k, nb)
    got = _decode_from_bins(d, d["bins"])
    assert list(got) == list(FROM_BINS)
    _held_to_restatement(got, d["want"], d["tup_off"])
    ex = TB.exact_bins(nb, d["idx"].shape[0])
    _held_to_restatement(_decode_from_bins(d, ex), TB.decode_batch(ex, nb, d["pts"], d["idx"], d["pt_off"], d["tup_off"], TB.AXES),
                         d["tup_off"])
    print("largest rot difference so far: %d ulp" % WORST_ROT["ulps"])


@pytest.mark.parametrize("k,nb", BIN_SHAPES)
def test_decode_bins_second_phase(k, nb):
    """The second phase of cppf_decode_bins on the same bins (drawn from one-hot logits): the bins come back, and every other
    output has the bits of cppf_decode_from_bins."""
    d = _batch(k, nb)
    two = _decode_from_bins(d, d["bins"])
    lg, u = _one_hot(d["bins"], nb)
    one = _decode_bins(d, lg, u)
    _same_bits("bins", one["bins"], d["bins"], d["tup_off"])
    for n in FROM_BINS:
        _same_bits(n, one[n], two[n], d["tup_off"])
    _held_to_restatement(one, d["want"], d["tup_off"])


@pytest.mark.parametrize("nb", [20, 32])
def test_null_outputs_in_turn(nb):
    """Each output of both entry points may be null: the others keep their bits."""
    d = _batch(5, nb)
    lg, u = _one_hot(d["bins"], nb)
    full = _decode_bins(d, lg, u)
    for n in ("bins",) + FROM_BINS:
        part = _decode_bins(d, lg, u, null=(n,))
        assert sorted(part) == sorted(set(full) - {n})
        for m in part:
            _same_bits(m, part[m], full[m], d["tup_off"])
    for n in FROM_BINS:
        part = _decode_from_bins(d, d["bins"], null=(n,))
        assert sorted(part) == sorted(set(FROM_BINS) - {n})
        for m in part:
            _same_bits(m, part[m], full[m], d["tup_off"])


# ---------------------------------------------------------------------------------------------------------------
# 3c. random logits on the ragged batch, against the oracle per scene
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [20, 32, 33])
def test_random_logits_on_the_ragged_batch(nb):
    """The criteria of test_gpu_parity.py::test_decode_bins_vs_oracle: a bin may differ only where the oracle's margin is below
    1e-5 (exp differs by ulps between the two sides), fewer than 1e-3 of the draws differ (tests/test_tuple_back_ref.py: fewer
    than 1e-3 of these draws lie that near an edge), and the tuples with equal bins are held to the restatement's criteria."""
    d = _batch(5, nb)
    lg = _dev(d["logits"])
    differ = near = draws = 0
    for u in d["uniforms"]:
        got = _decode_bins(d, lg, _dev(u))
        for b, t0, t1 in TR.scene_slices(d["tup_off"]):
            pairs = d["pts"][int(d["pt_off"][b]) + d["idx"][t0:t1, :2]]
            bins, _, scale, scaled, margin = O.decode_bins(d["logits"][t0:t1], u[t0:t1], pairs, return_margin=True)
            diff = got["bins"][t0:t1] != bins
            assert np.all(margin[diff] < 1e-5), "scene %d: a bin differs %g from the nearest CDF edge" % (b, margin[diff].max())
            differ, near, draws = differ + int(diff.sum()), near + int((margin < 1e-5).sum()), draws + diff.size
            tr, rot = O.generate_target_pairs(scaled, *TB.AXES)
            same = ~diff.any(1)
            _held_to_restatement({n: got[n][t0:t1] for n in FROM_BINS}, (scaled.reshape(-1, 6), scale, tr, rot), None, rows=same)
    print("nb = %d: %d of %d draws differ, %d within 1e-5 of a CDF edge (%.2e); largest rot difference so far: %d ulp" % (
        nb, differ, draws, near, near / draws, WORST_ROT["ulps"]))
    assert differ / draws < 1e-3


# ---------------------------------------------------------------------------------------------------------------
# 3d. generate_target_pairs with a centre per scene
# ---------------------------------------------------------------------------------------------------------------
def _target_pairs(pairs, tup_off, centres, T, null=()):
    """cppf_generate_target_pairs on device tensors (centres: float64 [B, 3] or None)."""
    from cppf2_amd import _lib, ops
    outs = _outs(T, ("tr", "rot"), null)
    _lib.check(ops._L.cppf_generate_target_pairs(tup_off.numel() - 1, ops._p(pairs), ops._p(tup_off), T, _axes(), ops._p(centres),
                                                 outs["tr"][1], outs["rot"][1], ops._stream()), "cppf_generate_target_pairs")
    return outs


@pytest.mark.parametrize("k", [2, 5, 8])
def test_target_pairs_ragged(k):
    """B = 10 with float64 centres near the points, far from them, all zero, a float32 and not: the centre of the scene a row lies
    in, found over the empty scenes' duplicate offsets, and used in float64.  Pairs with a == b, through the centre and with NaN
    and inf coordinates.  Then without centres, and with tr and rot null in turn."""
    d = _batch(k, 32)
    T = d["idx"].shape[0]
    pairs, tup_off, centres = _dev(d["pairs"]), d["dev"]["tup_off"], _dev(d["centres"])
    want_tr, want_rot = TB.target_pairs_batch(d["pairs"], d["tup_off"], TB.AXES, d["centres"])
    got = _read(_target_pairs(pairs, tup_off, centres, T))
    _same_bits("tr", got["tr"], want_tr, d["tup_off"], nan_by_position=True)
    _rot_within_one_ulp(got["rot"], want_rot, d["tup_off"])
    for null in ("tr", "rot"):
        part = _read(_target_pairs(pairs, tup_off, centres, T, null=(null,)))
        assert list(part) == [n for n in ("tr", "rot") if n != null]
        for n in part:
            _same_bits(n, part[n], got[n], d["tup_off"], nan_by_position=True)
    none = _read(_target_pairs(pairs, tup_off, None, T))
    want_tr, want_rot = TB.target_pairs_batch(d["pairs"], d["tup_off"], TB.AXES, None)
    _same_bits("tr", none["tr"], want_tr, d["tup_off"], nan_by_position=True)
    _rot_within_one_ulp(none["rot"], want_rot, d["tup_off"])
    print("largest rot difference so far: %d ulp" % WORST_ROT["ulps"])


def test_target_pairs_past_the_grid_cap():
    """cppf_generate_target_pairs launches min(ceil(T / 256), 65535) workgroups: T = 65535 * 256 + 257 tuples, the last 257 served
    by the grid-stride loop; four scenes (two empty) whose one boundary lies 40 tuples past the first pass, with different centres.
    The pairs tile a block of 4001 rows (coprime to 256), so the restatement is computed on the block, once per centre, and tiled
    on the device; the comparison runs there too.  402 MB of pairs, 134 MB of tr, 201 MB of rot (kept: not null)."""
    import torch
    T, L = TB.CAP_T, TB.CAP_BLOCK
    off = TR.offsets(TB.CAP_TUPLES)
    assert (T + 255) // 256 > 65535 and off[2] > 65535 * 256
    block = TB.cap_block()
    one = TR.offsets([L])
    refs = [TB.target_pairs_batch(block, one, TB.AXES, TB.CAP_CENTRES[b:b + 1]) for b in (1, 3)]
    r = torch.arange(T, device=_gpu()) % L
    late = (torch.arange(T, device=_gpu()) >= int(off[3]))[:, None]
    pairs = _dev(block)[r]
    outs = _target_pairs(pairs, _dev(off), _dev(TB.CAP_CENTRES), T)
    del pairs
    worst = 0
    for n in ("tr", "rot"):
        buf = outs[n][0]
        g = buf[GUARD:-GUARD]
        assert bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all()), "rows outside the output were written"
        w0, w1 = (_dev(TR.bits(ref[0 if n == "tr" else 1]).view(np.int32)) for ref in refs)
        w = torch.where(late, w1[r], w0[r])
        nan_g, nan_w = torch.isnan(g.view(torch.float32)), torch.isnan(w.view(torch.float32))
        assert torch.equal(nan_g, nan_w), "%s: NaNs at other positions" % n
        dist = (g.long() - w.long()).abs().masked_fill(nan_w, 0)            # rot is never negative: the ulp distance
        bad = dist > (0 if n == "tr" else 1)
        if n == "rot":
            worst = int(dist.max())
        if bool(bad.any()):
            row = int(torch.nonzero(bad.any(1))[0])
            raise AssertionError("%s: %d values differ; first in row %d (block row %d): got %r, want %r" % (
                n, int(bad.sum()), row, row % L, g[row].view(torch.float32).tolist(), w[row].view(torch.float32).tolist()))
        del g, w, w0, w1, dist, bad
    WORST_ROT["ulps"] = max(WORST_ROT["ulps"], worst)
    print("largest rot difference past the grid cap: %d ulp" % worst)


# ---------------------------------------------------------------------------------------------------------------
# 3e. the draw fused into the logit head's output layer
# ---------------------------------------------------------------------------------------------------------------
def test_fused_draw_on_the_exact_rows():
    """A logit encoder with every parameter zero has logits of exactly 0, so with the exact rows as its prior the epilogue of
    cppf_reslayer_split_decode_prior draws from those rows: the restatement's bins, bit for bit (without a prior: a flat row of 32)."""
    import torch
    from cppf2_amd import models
    from cppf2_amd.config import load_config
    rows, u = TB.exact_batch(32)
    T = rows.shape[0]
    want = TB.draw(rows, None, u)
    assert (want != TB.draw(rows, None, u, "draw_lt")).sum() >= T
    torch.manual_seed(3)
    net = models.BeyondCPPFShot(load_config("config", "config", ["category=bottle"])).to(_gpu()).eval()
    feat = torch.randn(T, 256, device=_gpu())
    prev = models.MLP_ARITH
    try:
        models.MLP_ARITH = "split"
        with torch.no_grad():
            for p in net.logit_encoder.parameters():
                p.zero_()
            assert models.decode_supported(net.logit_encoder, feat)
            buf, _ = _words(T, 6)
            bins = buf[GUARD:-GUARD]
            out = models.fused_stack(net.logit_encoder, feat, keep_input=True, decode=(_dev(u), _dev(rows), bins))
            assert out.data_ptr() == bins.data_ptr()
            _same_bits("bins", _guards_untouched(buf), want)
            flat = models.fused_stack(net.logit_encoder, feat, keep_input=True, decode=(_dev(u), None, None))
            _same_bits("bins", flat.cpu().numpy(), TB.draw(np.zeros((T, 6, 32), np.float32), None, u))
    finally:
        models.MLP_ARITH = prev
