"""The device-side ensemble score and selection (cppf_refine.hip: alignment_loss_kernel, ensemble_select_kernel) called directly.

* cppf_ensemble_select on 300 scenes (two blocks) whose losses run through every pair of {small, large, NaN, +inf, -0.0, 0.0}
  -- equal losses included -- under all four (enable0, enable1) settings, against the rule of eval.py:365-372 restated in plain
  Python: a NaN loss never wins, model 0 first on a tie, pick = -1 and best = inf when nothing is enabled or comparable, the
  scale always from slot 0.  Byte for byte.
* cppf_alignment_loss on a ragged batch of 0, 1, 127, 128, 129 and 5000 kept pairs (256 threads x 2 loss elements: 128 pairs
  fill the block exactly), y_only on and off, 32 and 20 bins, the scale read from the scored records or from another buffer, a
  scale of (0, 0, 0) whose norm counts as 1 -- against oracle.pipeline_oracle.alignment_loss and a math.fsum mean of the same
  clipped terms, to 1e-10.
Needs an MI355X: run with `pytest -m gpu`.
"""
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import pipeline_oracle as PO       # noqa: E402  (checker only)
from cppf2_amd import _lib, ops                # noqa: E402
from cppf2_amd.pipeline import RESULT_DTYPE    # noqa: E402

DEV = torch.device("cuda")
INF, NAN = float("inf"), float("nan")


def _d(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV, dtype)


def _records(a):
    return _d(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), 160), torch.uint8)


# ------------------------------------------------------------------------------------------ selection
def _select_rule(loss0, loss1, enable0, enable1):
    """eval.py:365-369 / PO.run_instance_ensemble: best = inf, strict '<', model 0 first, a disabled model is skipped."""
    best, pick = INF, -1
    for m, (loss, enabled) in enumerate(((loss0, enable0), (loss1, enable1))):
        if loss < best and enabled:
            best, pick = loss, m
    return pick, best


@pytest.mark.parametrize("enable0,enable1", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_ensemble_select_rules_on_every_pair_of_loss_kinds(enable0, enable1):
    L = _lib.load()
    B = 300
    kinds = [0.01, 0.09, NAN, INF, -0.0, 0.0]
    n = len(kinds)
    # scene b: the pair (b % 36) of kinds; every further round of 36 scales the finite losses, both by the same factor
    factor = 1.0 + (np.arange(B) // (n * n)) * 0.125
    loss0 = np.array([kinds[(b % (n * n)) // n] for b in range(B)]) * factor
    loss1 = np.array([kinds[b % n] for b in range(B)]) * factor
    rng = np.random.RandomState(11)
    raw = rng.randint(0, 256, (2, B, 160)).astype(np.uint8)      # distinct contents per slot and scene, every field
    rec = [np.frombuffer(raw[m].tobytes(), dtype=RESULT_DTYPE).copy() for m in (0, 1)]
    assert len({r.tobytes() for m in (0, 1) for r in rec[m]}) == 2 * B
    want_pick, want_best = map(np.array, zip(*[_select_rule(a, b, enable0, enable1) for a, b in zip(loss0, loss1)]))
    want = np.where(want_pick == 1, rec[1], rec[0])              # slot 0's record when nothing is picked
    want["scale"] = rec[0]["scale"]                              # the scale always from slot 0
    want["pad_"][:, 0] = want_pick
    if enable0 and enable1:                                      # the cases are really there
        eq = np.flatnonzero(loss0 == loss1)
        assert len(eq) and np.all(want_pick[eq][np.isfinite(loss0[eq])] == 0)                # model 0 first on a tie
        assert np.all(want_pick[np.isnan(loss0) & (loss1 < INF)] == 1) and np.all(want_pick[np.isnan(loss1) & (loss0 < INF)] == 0)
        assert np.all(want_pick[np.isnan(loss0) & np.isnan(loss1)] == -1) and np.all(want_pick[(loss0 == INF) & (loss1 == INF)] == -1)
        assert set(want_pick) == {-1, 0, 1} and np.signbit(want_best).any()                  # (-0.0 wins as itself)
    if not (enable0 or enable1):
        assert np.all(want_pick == -1) and np.all(want_best == INF)
    out = torch.full((B + 1, 160), 0xEE, dtype=torch.uint8, device=DEV)
    best = torch.full((B + 1,), -5.0, dtype=torch.float64, device=DEV)
    rec0_d, rec1_d, loss0_d, loss1_d = _records(rec[0]), _records(rec[1]), _d(loss0, torch.float64), _d(loss1, torch.float64)
    _lib.check(L.cppf_ensemble_select(B, ops._p(rec0_d), ops._p(rec1_d), ops._p(loss0_d), ops._p(loss1_d), enable0, enable1,
                                      ops._p(out), ops._p(best), ops._stream()), "cppf_ensemble_select")
    got = np.frombuffer(out.cpu().numpy().tobytes(), dtype=RESULT_DTYPE)
    got_best = best.cpu().numpy()
    assert np.array_equal(got["pad_"][:B, 0], want_pick)
    assert not np.isnan(got_best).any() and np.array_equal(got_best[:B], want_best, equal_nan=False)
    assert got_best[:B].tobytes() == want_best.astype(np.float64).tobytes()
    for b in range(B):
        assert got[b].tobytes() == want[b].tobytes(), (b, loss0[b], loss1[b], int(want_pick[b]))
    assert got[B].tobytes() == b"\xee" * 160 and got_best[B] == -5.0                         # nothing past scene B - 1


# ------------------------------------------------------------------------------------------ alignment loss
KEPT = [0, 1, 127, 128, 129, 5000]             # 256 threads x 2 loss elements: 128 pairs fill the block exactly
TUPLES = [4, 3, 200, 128, 300, 6000]
N_POINTS = 60
K = 5
_PROBLEM = {}


def _rotation(rng):
    q, r = np.linalg.qr(rng.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _scale_norm(s):
    """The kernel's documented norm: float32 sqrt((s0*s0 + s1*s1) + s2*s2), 1 where it is 0."""
    s = np.asarray(s, np.float32)
    n = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2], dtype=np.float32)
    return n if n > 0 else np.float32(1.0)


def _problem(nb):
    """One ragged batch: clouds in a 0.2 m box, random rotations, centres a few cm from the centroid, kept lists that are random
    subsets in random order; half the tuples' bins are the ones nearest the canonical coordinates (terms below the 0.1 clip),
    the others random (most terms above it).  Two sets of records: `recs` (scored; scene 4 has a zero scale) and `src` (another
    buffer with other scales; scene 3's is zero)."""
    if nb in _PROBLEM:
        return _PROBLEM[nb]
    rng = np.random.RandomState(100 + nb)
    B = len(KEPT)
    recs = np.frombuffer(rng.randint(0, 256, (B, 160)).astype(np.uint8).tobytes(), dtype=RESULT_DTYPE).copy()
    src = np.frombuffer(rng.randint(0, 256, (B, 160)).astype(np.uint8).tobytes(), dtype=RESULT_DTYPE).copy()
    pcs, idxs, binss, kepts = [], [], [], []
    for b, (kept, T) in enumerate(zip(KEPT, TUPLES)):
        pc = (rng.rand(N_POINTS, 3) * 0.2 + rng.randn(3)).astype(np.float32)
        recs["t"][b] = pc.astype(np.float64).mean(0) + rng.randn(3) * 0.02
        recs["R"][b] = _rotation(rng)
        recs["scale"][b] = (0.15 + 0.1 * rng.rand(3)).astype(np.float32)
        src["scale"][b] = (0.3 + 0.2 * rng.rand(3)).astype(np.float32)
        idx = rng.randint(0, N_POINTS, (T, K)).astype(np.int32)
        canon = (pc - recs["t"][b]) @ recs["R"][b] / _scale_norm(recs["scale"][b])
        near = np.clip(np.rint((canon[idx[:, :2]] + 0.5) * (nb - 1)), 0, nb - 1).astype(np.int32).reshape(T, 6)
        bins = np.where((rng.rand(T) < 0.5)[:, None], near, rng.randint(0, nb, (T, 6))).astype(np.int32)
        pcs.append(pc), idxs.append(idx), binss.append(bins), kepts.append(rng.permutation(T)[:kept].astype(np.int32))
    recs["scale"][4] = 0
    src["scale"][3] = 0
    off = lambda n: np.concatenate([[0], np.cumsum(n)]).astype(np.int32)      # noqa: E731
    tup_off = off(TUPLES)
    kept_tuple = np.full(tup_off[-1], -1, np.int32)               # past a scene's count: rows the kernel must not read
    for b, kt in enumerate(kepts):
        kept_tuple[tup_off[b]:tup_off[b] + len(kt)] = kt
    dev = dict(pts=_d(np.concatenate(pcs), torch.float32), pt_off=_d(off([N_POINTS] * B), torch.int32),
               idx=_d(np.concatenate(idxs), torch.int32), tup_off=_d(tup_off, torch.int32), bins=_d(np.concatenate(binss), torch.int32),
               kept_tuple=_d(kept_tuple, torch.int32), kept_count=_d(KEPT, torch.int32), recs=_records(recs), src=_records(src))
    _PROBLEM[nb] = dict(recs=recs, src=src, pcs=pcs, idxs=idxs, binss=binss, kepts=kepts, dev=dev)
    return _PROBLEM[nb]


def _loss_references(p, b, nb, y_only, scale_records):
    """(PO.alignment_loss, math.fsum mean of the same clipped terms, the unclipped terms) of scene b."""
    pc, idx, kt = p["pcs"][b], p["idxs"][b].astype(np.int64)[p["kepts"][b]], p["kepts"][b]
    pred = (p["binss"][b][kt].astype(np.float32) / np.float32(nb - 1) - np.float32(0.5)).reshape(-1, 2, 3)
    assert pred.dtype == np.float32
    t, R, nrm = p["recs"]["t"][b], p["recs"]["R"][b], _scale_norm(scale_records["scale"][b])
    want = PO.alignment_loss(pc, t, R, nrm, idx, pred, y_only)
    raw = np.abs(((pc - t) @ R / nrm)[idx[:, :2]] - pred)
    raw = raw[..., 1] if y_only else raw
    terms = np.clip(raw, 0, 0.1)
    return want, math.fsum(terms.ravel().tolist()) / terms.size, raw


@pytest.mark.parametrize("nb", [32, 20])
@pytest.mark.parametrize("y_only", [0, 1])
def test_alignment_loss_on_a_ragged_batch_to_1e_10(y_only, nb):
    """|loss - reference| <= 1e-10 against both references.  The bar follows from the arithmetic: every term is at most 0.1 in
    float64 and there are at most 30 000 of them, so summing in any order errs by less than n * 2^-53 * 0.1 ~ 3e-13, and a term
    computed in the kernel's written order differs from NumPy's matrix product by a few ulp of a number below 1."""
    L = _lib.load()
    p = _problem(nb)
    d, B = p["dev"], len(KEPT)
    assert 2 * KEPT[3] == 256 and KEPT[2] == KEPT[3] - 1 and KEPT[4] == KEPT[3] + 1
    worst = 0.0
    for which in ("same buffer", "other buffer"):
        scale_dev, scale_np = (d["recs"], p["recs"]) if which == "same buffer" else (d["src"], p["src"])
        assert (scale_dev.data_ptr() == d["recs"].data_ptr()) == (which == "same buffer")
        loss = torch.full((B + 1,), -5.0, dtype=torch.float64, device=DEV)
        _lib.check(L.cppf_alignment_loss(B, ops._p(d["pts"]), ops._p(d["pt_off"]), ops._p(d["idx"]), K, ops._p(d["tup_off"]),
                                         ops._p(d["bins"]), nb, ops._p(d["kept_tuple"]), ops._p(d["kept_count"]), y_only,
                                         ops._p(d["recs"]), ops._p(scale_dev), ops._p(loss), ops._stream()), "cppf_alignment_loss")
        got = loss.cpu().numpy()
        assert got[B] == -5.0
        assert np.isnan(got[0]) and KEPT[0] == 0                                             # nothing kept
        zero = 4 if which == "same buffer" else 3
        assert not scale_np["scale"][zero].any() and _scale_norm(scale_np["scale"][zero]) == 1.0
        for b in range(1, B):
            want, want_fsum, raw = _loss_references(p, b, nb, y_only, scale_np)
            if KEPT[b] >= 127:
                assert (raw > 0.1).any() and (raw < 0.1).any() and 0.0 < want < 0.1          # both sides of the clip
            diff = max(abs(got[b] - want), abs(got[b] - want_fsum))
            worst = max(worst, diff)
            print("alignment loss, y_only %d, nb %d, scale from the %s, kept %4d: got %.17g, oracle %.17g, fsum %.17g, diff %.3g"
                  % (y_only, nb, which, KEPT[b], got[b], want, want_fsum, diff))
            assert abs(got[b] - want) <= 1e-10, (which, b, got[b], want)
            assert abs(got[b] - want_fsum) <= 1e-10, (which, b, got[b], want_fsum)
        # the two launches score different scales: the norm really comes from scale_src
        if which == "other buffer":
            assert abs(_loss_references(p, 5, nb, y_only, p["recs"])[0] - _loss_references(p, 5, nb, y_only, p["src"])[0]) > 1e-4
    print("alignment loss, y_only %d, nb %d: largest |difference| %.3g" % (y_only, nb, worst))
