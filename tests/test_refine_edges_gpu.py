"""refine_pose_kernel alone, through cppf_refine_pose on hand-built input, against the independent float64 reference
(tests/refine_f64.py) at the kernel's structural boundaries: 1 pair (2 elements on 2 lanes), the wavefront (32 / 33 pairs),
the workgroup (128 / 129), the register cache (2047 / 2048 / 2049 pairs = 4094 / 4096 / 4098 loss elements), a
memory-resident tail that ends a full and a ragged round (2176 / 2177) and 4500 pairs, for 1 to 4 Adam steps -- few enough
that a residual's sign is a property of the input (the preconditions of refine_f64.step_case, asserted before the GPU is
touched, and again without one in tests/test_refine_f64.py) and not of the summation order.

The bar of a case is 4 x the float32 oracle's own distance to the reference, floored at 4 ulp (2.5e-7 in t, 5e-7 in R):
it is set by two faithful implementations, not by the kernel.

Measured (oracle / kernel distance to the reference, the largest over the cases of a row; xyz and y modes together):

    case                   steps      oracle t / R          kernel t / R          bars t / R
    1 pair                 1-2        2.4e-08 / 7.7e-08     2.4e-08 / 7.7e-08     1.0e-06 / 2.0e-06
    1 pair                 3-4        3.5e-08 / 7.7e-08     1.3e-07 / 2.6e-07     1.0e-06 / 2.0e-06
    2 pairs                1-2        3.1e-08 / 6.7e-08     3.1e-08 / 6.5e-08     1.0e-06 / 2.0e-06
    2 pairs                3-4        4.1e-08 / 6.4e-08     1.4e-07 / 2.5e-07     1.0e-06 / 2.0e-06
    32 pairs               1-2        3.8e-08 / 7.0e-08     3.8e-08 / 6.7e-08     1.0e-06 / 2.0e-06
    32 pairs               3-4        3.9e-08 / 8.2e-08     9.7e-08 / 2.6e-07     1.0e-06 / 2.0e-06
    33 pairs               1-2        1.3e-08 / 8.4e-08     1.3e-08 / 8.4e-08     1.0e-06 / 2.0e-06
    33 pairs               3-4        3.0e-08 / 1.1e-07     9.0e-08 / 2.8e-07     1.0e-06 / 2.0e-06
    128 pairs              1-2        3.8e-08 / 7.2e-08     3.8e-08 / 7.6e-08     1.0e-06 / 2.0e-06
    128 pairs              3-4        6.0e-08 / 6.0e-07     1.2e-07 / 5.8e-07     1.0e-06 / 2.4e-06
    129 pairs              1-2        3.0e-08 / 7.4e-08     6.1e-08 / 8.2e-08     1.0e-06 / 2.0e-06
    129 pairs              3-4        5.2e-08 / 1.1e-07     1.3e-07 / 3.0e-07     1.0e-06 / 2.0e-06
    2047 pairs             1-2        1.1e-07 / 1.0e-07     2.1e-08 / 8.0e-08     1.0e-06 / 2.0e-06
    2048 pairs             1-2        8.1e-08 / 8.7e-08     2.9e-08 / 8.9e-08     1.0e-06 / 2.0e-06
    2049 pairs             1-2        8.7e-08 / 2.6e-07     3.2e-08 / 1.1e-07     1.0e-06 / 2.0e-06
    2176 pairs             1-2        5.2e-08 / 7.7e-08     2.3e-08 / 8.7e-08     1.0e-06 / 2.0e-06
    2177 pairs             1-2        6.0e-08 / 7.7e-08     6.0e-08 / 7.8e-08     1.0e-06 / 2.0e-06
    4500 pairs             1-2        1.8e-07 / 6.8e-08     2.0e-08 / 7.4e-08     1.0e-06 / 2.0e-06
    129 pairs, lr 3e-3     2          2.2e-08 / 5.4e-08     2.2e-08 / 5.4e-08     1.0e-06 / 2.0e-06
    33 pairs, k = 2        2          1.3e-08 / 8.4e-08     1.3e-08 / 8.4e-08     1.0e-06 / 2.0e-06
    33 pairs, start + 1e-9 2          1.4e-08 / 8.4e-08     1.4e-08 / 8.4e-08     1.0e-06 / 2.0e-06
    one element decides    1          1.0e-09 / 2.9e-08     8.6e-10 / 2.9e-08     1.0e-06 / 2.0e-06
    scenes of the batch    2          8.7e-08 / 2.6e-07     3.2e-08 / 1.1e-07     1.0e-06 / 2.0e-06

Over all of them the kernel is within 1.4e-7 of the reference in t and 5.8e-7 in R, the oracle within 1.8e-7 and 6.0e-7.
Every test prints its own figures (run with -s).

The one-element scenes (one step; the reference without the element is more than 1e-2 away in R) and the six-scene batch
are held to the same bars; the batch's records are also byte-identical to every scene launched alone, to the batch in
reversed order and to a second launch."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refine_f64 as F  # noqa: E402
from oracle import cppf_oracle as O  # noqa: E402


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def _case(case, off_grid=False):
    return F.step_case(*case, O.refine_pose, start=F.off_grid_start() if off_grid else None)


# ---------------------------------------------------------------------------------------------------------------------------
# Input by hand


class Scene:
    """One scene's arrays: the kept pairs (idx2 [nk,2], tgt [nk,2,3]) scattered over Tf = nk + nk // 4 + 7 tuples in a
    seeded random order, kept_tuple[:nk] naming their rows (sparse, not ascending); the other tuples point at valid points and
    garbage targets, and the rest of kept_tuple names them, so that a kernel that read past kept_count would read in bounds
    and land far off.  idx's columns past the first two are random valid points."""

    def __init__(self, pc, idx2, tgt, R0, t0, seed=0, k=5, flags=0):
        nk = len(idx2)
        rng = np.random.RandomState([nk, seed, 77])
        self.pc = np.ascontiguousarray(pc, dtype=np.float32)
        self.nk, self.Tf, self.k = nk, nk + nk // 4 + 7, k
        rows = rng.permutation(self.Tf)
        self.idx = rng.randint(0, len(self.pc), (self.Tf, k)).astype(np.int32)
        self.scaled = rng.uniform(-9.0, 9.0, (self.Tf, 6)).astype(np.float32)
        self.idx[rows[:nk], :2] = idx2
        self.scaled[rows[:nk]] = np.asarray(tgt, dtype=np.float32).reshape(nk, 6)
        self.kept_tuple = rows.astype(np.int32)
        self.R0, self.t0, self.flags = np.asarray(R0, dtype=np.float64), np.asarray(t0, dtype=np.float64), flags

    def with_k(self, k):
        other = Scene.__new__(Scene)
        other.__dict__.update(self.__dict__)
        other.k, other.idx = k, np.ascontiguousarray(self.idx[:, :k])
        return other


def _scene_of(c, seed=0, **kw):
    return Scene(c["pc"], c["idx2"], c["tgt"], c["R0"], c["t0"], seed, **kw)


FLAGS_FILL = 0x5A5A5A50           # the pattern's flags word: bits 0 (empty scene) and 3 (refined) clear


def _records(scenes):
    """Records whose every byte is a non-zero pattern, then R, t and flags (the pattern's with bits 0 and 3 clear, or'ed with
    the scene's)."""
    from cppf2_amd.pipeline import RESULT_DTYPE
    raw = (np.arange(len(scenes) * 160, dtype=np.int64) % 251 + 1).astype(np.uint8)
    rec = raw.view(RESULT_DTYPE).copy()
    for b, s in enumerate(scenes):
        rec[b]["R"], rec[b]["t"], rec[b]["flags"] = s.R0, s.t0, FLAGS_FILL | s.flags
    return rec


def _raw(scenes, rec, y_only, steps, lr=1e-2, B=None, k=None, null=None):
    """cppf_refine_pose on the concatenated scenes; returns (status, the records afterwards).  null names an argument to pass
    as a null pointer."""
    import torch
    from cppf2_amd import _lib, ops
    from cppf2_amd.pipeline import record_bytes, records_of
    dev = _gpu()
    L = _lib.load()
    assert len({s.k for s in scenes}) == 1
    t = dict(pts=np.concatenate([s.pc for s in scenes]),
             pt_off=np.cumsum([0] + [len(s.pc) for s in scenes])[:-1].astype(np.int32),
             idx=np.concatenate([s.idx for s in scenes]),
             tup_off=np.cumsum([0] + [s.Tf for s in scenes])[:-1].astype(np.int32),
             scaled=np.concatenate([s.scaled for s in scenes]),
             kept_tuple=np.concatenate([s.kept_tuple for s in scenes]),
             kept_count=np.array([s.nk for s in scenes], dtype=np.int32))
    # what the kernel may touch is in bounds: every point index inside its scene's points, every kept row inside its tuples
    for s in scenes:
        assert 0 <= s.idx.min() and s.idx.max() < len(s.pc) and 0 <= s.kept_tuple.min() and s.kept_tuple.max() < s.Tf
        assert s.nk <= s.Tf and len(s.kept_tuple) == s.Tf
    d = {n: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for n, a in t.items()}
    d["results"] = record_bytes(rec, dev)
    p = {n: (C.c_void_p(0) if n == null else ops._p(v)) for n, v in d.items()}
    status = L.cppf_refine_pose(len(scenes) if B is None else B, p["pts"], p["pt_off"], p["idx"], scenes[0].k if k is None else k,
                                p["tup_off"], p["scaled"], p["kept_tuple"], p["kept_count"], int(y_only), steps,
                                C.c_float(lr), p["results"], ops._stream())
    torch.cuda.synchronize()
    return status, records_of(d["results"])


def _run(scenes, y_only, steps, lr=1e-2, rec=None):
    from cppf2_amd import _lib
    rec = _records(scenes) if rec is None else rec
    status, after = _raw(scenes, rec, y_only, steps, lr)
    _lib.check(status, "cppf_refine_pose")
    return rec, after


def _flags_off():
    from cppf2_amd.pipeline import RESULT_DTYPE
    return RESULT_DTYPE.fields["flags"][1]


def _only_pose_and_flags_changed(before, after):
    """Every byte outside t (8..32), R (32..104) and flags is as it was; flags gained bit 3 and nothing else."""
    a, b = after.view(np.uint8).reshape(-1, 160).copy(), before.view(np.uint8).reshape(-1, 160).copy()
    f = _flags_off()
    for x in (a, b):
        x[:, 8:104] = 0
        x[:, f:f + 4] = 0
    assert np.array_equal(a, b)
    assert np.array_equal(after["flags"], before["flags"] | 8)


def _distances(after, c):
    return float(np.abs(after["t"] - c["t"]).max()), float(np.abs(after["R"] - c["R"]).max())


def _held(after, c, what):
    d_t, d_R = _distances(after, c)
    print("%s: oracle %.2e / %.2e  kernel %.2e / %.2e  bars %.2e / %.2e" % (what, c["e_t"], c["e_R"], d_t, d_R, c["bar_t"], c["bar_R"]))
    assert d_t <= c["bar_t"] and d_R <= c["bar_R"], (what, d_t, c["bar_t"], d_R, c["bar_R"])


# ---------------------------------------------------------------------------------------------------------------------------
# Step cases


@pytest.mark.parametrize("case", F.STEP_CASES, ids=F.case_id)
def test_steps_against_the_float64_reference(case):
    kept, steps, y_only, seed, lr = case
    c = _case(case)                                                  # the three preconditions, asserted
    before, after = _run([_scene_of(c, seed)], y_only, steps, lr)
    _only_pose_and_flags_changed(before, after)
    _held(after[0], c, F.case_id(case))


@pytest.mark.parametrize("case", F.OFF_GRID_CASES, ids=F.case_id)
def test_k_of_two_and_a_start_that_is_no_float32(case):
    """k = 2 (idx has the pair's two columns and nothing else) gives the bytes of k = 5; a record whose doubles are the
    float32 start plus 1e-9 is read as the nearest float32, as the reference reads it."""
    kept, steps, y_only, seed, lr = case
    c = _case(case)
    five = _scene_of(c, seed)
    _, a5 = _run([five], y_only, steps, lr)
    _, a2 = _run([five.with_k(2)], y_only, steps, lr)
    _held(a2[0], c, "k=2 " + F.case_id(case))
    assert a2.tobytes() == a5.tobytes()
    g = _case(case, True)
    assert np.any(g["R0"] != g["R0"].astype(np.float32)) and np.any(g["t0"] != g["t0"].astype(np.float32))
    before, after = _run([_scene_of(g, seed)], y_only, steps, lr)
    _only_pose_and_flags_changed(before, after)
    _held(after[0], g, "off-grid " + F.case_id(case))
    assert after[0]["R"].tobytes() != a5[0]["R"].tobytes()          # the entries that round up are seen


# ---------------------------------------------------------------------------------------------------------------------------
# One element decides


@pytest.mark.parametrize("y_only", [False, True], ids=["xyz", "y"])
@pytest.mark.parametrize("e_star", F.DECISIVE_POSITIONS)
def test_one_element_decides(e_star, y_only):
    """Element e_star of 4354 (lane 0 / 1 / 63 of the first wavefront, the second wavefront's first, the workgroup's last and
    the second round's first, the register cache's last and the first re-read one, the last full round's ends and the ragged
    round's last) carries the rotation gradient's sign; a kernel that dropped it would land 2e-2 away in R."""
    pc, idx2, tgt, mask = F.decisive_scene(e_star)
    R0, t0 = np.eye(3), np.zeros(3)
    t_w, R_w = F.refine_f64(pc, idx2, tgt, t0, R0, y_only, 1)
    t_o, R_o = F.refine_f64(pc, idx2, tgt, t0, R0, y_only, 1, mask=mask)
    assert np.abs(R_w - R_o).max() > 1e-2
    t_f, R_f = O.refine_pose(pc, idx2, tgt, t0, R0, y_only, steps=1)
    bar_t, bar_R, e_t, e_R = F.bars(t_w, R_w, t_f, R_f)
    sc = Scene(pc, idx2, tgt, R0, t0, seed=e_star)
    before, after = _run([sc], y_only, 1)
    _only_pose_and_flags_changed(before, after)
    _held(after[0], dict(t=t_w, R=R_w, e_t=e_t, e_R=e_R, bar_t=bar_t, bar_R=bar_R), "element %d %s" % (e_star, y_only))


# ---------------------------------------------------------------------------------------------------------------------------
# Records and batches

BATCH = {False: [(1, 2, False, 1, 1e-2), (2048, 2, False, 2, 1e-2), (2049, 2, False, 2, 1e-2), (33, 2, False, 0, 1e-2)],
         True: [(1, 2, True, 8, 1e-2), (2048, 2, True, 2, 1e-2), (2049, 2, True, 1, 1e-2), (33, 2, True, 8, 1e-2)]}


def _batch(y_only):
    """Kept counts [0, 1, 2048, 300 with flags bit 0 set, 2049, 33]; returns (scenes, the step case of each or None)."""
    cs = [_case(c) for c in BATCH[y_only]]
    assert all(c in F.STEP_CASES for c in BATCH[y_only])
    pc, idx2, tgt, R0, t0 = F.banded_scene(300, 0)
    empty = Scene(pc[:100], idx2[:0], tgt[:0], R0, t0, seed=1)
    flagged = Scene(pc, idx2, tgt, R0, t0, seed=2, flags=1)
    scenes = [empty, _scene_of(cs[0], 3), _scene_of(cs[1], 4), flagged, _scene_of(cs[2], 5), _scene_of(cs[3], 6)]
    assert [s.nk for s in scenes] == [0, 1, 2048, 300, 2049, 33]
    return scenes, [None, cs[0], cs[1], None, cs[2], cs[3]]


@pytest.mark.parametrize("y_only", [False, True], ids=["xyz", "y"])
def test_a_batch_is_its_scenes_alone(y_only):
    scenes, cs = _batch(y_only)
    before, after = _run(scenes, y_only, 2)
    for s in scenes:                                                 # kept rows: sparse and not ascending
        assert s.nk < 2 or (np.any(np.diff(s.kept_tuple[:s.nk]) < 0) and s.kept_tuple[:s.nk].max() >= s.nk)
    skipped = [0, 3]
    for b in range(len(scenes)):
        if b in skipped:                                             # nothing kept / an empty scene: the record as it was
            assert after[b:b + 1].tobytes() == before[b:b + 1].tobytes() and not after[b]["flags"] & 8
        else:
            _only_pose_and_flags_changed(before[b:b + 1], after[b:b + 1])
            assert after[b]["flags"] & 8
            _held(after[b], cs[b], "batch scene %d" % b)
    _, again = _run(scenes, y_only, 2)
    assert again.tobytes() == after.tobytes()
    _, rev = _run(scenes[::-1], y_only, 2, rec=before[::-1].copy())
    assert rev[::-1].tobytes() == after.tobytes()
    for b in range(len(scenes)):
        _, alone = _run([scenes[b]], y_only, 2, rec=before[b:b + 1].copy())
        assert alone.tobytes() == after[b:b + 1].tobytes(), b
    _, still = _run(scenes, y_only, 0)                               # steps = 0: every byte alone
    assert still.tobytes() == before.tobytes()


def test_invalid_arguments_launch_nothing():
    from cppf2_amd import _lib
    scenes, _ = _batch(False)
    scenes = scenes[4:]
    rec = _records(scenes)
    bad = [dict(k=1), dict(k=0), dict(steps=-1), dict(lr=0.0), dict(lr=-1e-2), dict(B=0), dict(B=-1)]
    bad += [dict(null=n) for n in ("pts", "pt_off", "idx", "tup_off", "scaled", "kept_tuple", "kept_count", "results")]
    want = None
    for kw in bad:
        args = dict(y_only=False, steps=2)
        args.update(kw)
        status, after = _raw(scenes, rec, **args)
        assert status != 0 and after.tobytes() == rec.tobytes(), kw
        want = status if want is None else want
        assert status == want                                        # what CPPF_CHECK_ARG returns, every time
        with pytest.raises(_lib.CppfError, match="invalid argument"):
            _lib.check(status, "cppf_refine_pose")
    status, after = _raw(scenes, rec, False, 2)                      # and the same call with nothing wrong runs
    assert status == 0 and np.all(after["flags"] & 8)
