"""cppf_backvote_filter (backvote_errs_kernel + backvote_kernel, cppf_backvote.hip) called directly on the scenes of
tests/backvote_ref.py, against the oracle's np.percentile filter, bit for bit: ties at the order statistic (the v_hi = v_lo
branch), exact-zero errors (thr == 0, nothing kept), gamma == 0 and 0.5, scenes of 0, 1 and 2 tuples, tuple and kept counts on
both sides of BV_THREADS, thousands of hits on one point, degenerate pairs among the kept ones, both grid shapes of
backvote_errs_kernel.  Every buffer starts from a sentinel and carries guard entries past its end; every batch is launched twice
into the same buffers and workspace.  The resulting lists then go through cppf_kept_rows / cppf_kept_rows32.
tests/test_backvote_ref.py shows on the CPU that each scene reaches its edge.  Needs an MI355X: run with `pytest -m gpu`.
"""
import ctypes as C
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import backvote_ref as BR                      # noqa: E402  (checker only)
from cppf2_amd import _lib, ops                # noqa: E402

DEV = torch.device("cuda")
GUARD = 64                                     # entries past the end of every per-tuple output, which must keep the sentinel
SENT_I32, SENT_U8, SENT_F64 = -77, 0xAA, -12345.5
SENT_F32 = -54321.5
_RUNS = {}


def _d(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV, dtype)


def _launch(arrays, num_rots, axes, repeat=2):
    """`repeat` launches of cppf_backvote_filter on one batch into the same sentinel-filled buffers and workspace; the host
    copies of every output after each launch."""
    L = _lib.load()
    up, right, front = BR.AXES[axes]
    B, Ttot, Ntot = len(arrays["ratios"]), int(arrays["tup_off"][-1]), int(arrays["pt_off"][-1])
    kg = [ops.percentile_params(int(n), r) for n, r in zip(np.diff(arrays["tup_off"]), arrays["ratios"])]
    # the product's host half of the percentile is the arithmetic the reference's helper restates
    assert kg == [BR.percentile_params(int(n), r) for n, r in zip(np.diff(arrays["tup_off"]), arrays["ratios"])]
    kidx, gammas = _d([k for k, _ in kg], torch.int32), _d([g for _, g in kg], torch.float32)
    pts, pt_off, idx = _d(arrays["pts"], torch.float32), _d(arrays["pt_off"], torch.int32), _d(arrays["idx"], torch.int32)
    tup_off, tr, centres = _d(arrays["tup_off"], torch.int32), _d(arrays["tr"], torch.float32), _d(arrays["centres"], torch.float64)
    full = lambda n, v, dt: torch.full((n + GUARD,), v, dtype=dt, device=DEV)      # noqa: E731
    out = dict(mask=full(Ttot, SENT_U8, torch.uint8), kept_tuple=full(Ttot, SENT_I32, torch.int32),
               kept_count=full(B, SENT_I32, torch.int32), kept_wt=full(Ttot, SENT_F64, torch.float64),
               kept_row0=full(Ttot, SENT_I32, torch.int32), back_errs=full(Ttot, SENT_F32, torch.float32),
               thr=full(B, SENT_F32, torch.float32))
    ws_bytes = L.cppf_backvote_workspace_bytes(Ntot, B)
    assert ws_bytes >= 4 * Ntot
    ws = torch.full((ws_bytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)      # dirty: the entry point must clear it itself
    # positional (up, right, front) of generate_target_pairs <- (up, front, right): eval.py:252-256
    h_axes = ops._axes9(up, front, right)
    runs = []
    for _ in range(repeat):
        _lib.check(L.cppf_backvote_filter(B, ops._p(pts), ops._p(pt_off), ops._p(idx), BR.K, ops._p(tup_off), ops._p(tr),
                                          ops._p(centres), h_axes, ops._p(kidx), ops._p(gammas), C.c_double(BR.MARGIN),
                                          int(num_rots), ops._p(out["mask"]), ops._p(out["kept_tuple"]), ops._p(out["kept_count"]),
                                          ops._p(out["kept_wt"]), ops._p(out["kept_row0"]), ops._p(out["back_errs"]),
                                          ops._p(out["thr"]), ops._p(ws), ws_bytes, ops._stream()), "cppf_backvote_filter")
        torch.cuda.synchronize()
        runs.append({k: v.cpu().numpy() for k, v in out.items()})
        runs[-1]["ws_guard"] = ws[ws_bytes:].cpu().numpy()
    dev = dict(out, tup_off=tup_off, max_kept=max(k for k, _ in kg) + 1)
    return runs, dev


def _batch(name):
    if name not in _RUNS:
        cases, scenes, refs, num_rots, axes, arrays = BR.build_batch(name)
        runs, dev = _launch(arrays, num_rots, axes)
        _RUNS[name] = dict(cases=cases, scenes=scenes, refs=refs, arrays=arrays, runs=runs, dev=dev, num_rots=num_rots, axes=axes)
    return _RUNS[name]


def _bits(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("name", sorted(BR.BATCHES))
def test_filter_equals_the_percentile_reference_bit_for_bit(name):
    b = _batch(name)
    got, tup_off = b["runs"][0], b["arrays"]["tup_off"]
    Ttot, B = int(tup_off[-1]), len(b["cases"])
    report = []
    for s, (case, ref) in enumerate(zip(b["cases"], b["refs"])):
        t0, T, kept = int(tup_off[s]), ref["T"], ref["kept"]
        assert not BR.failed_edges(case, ref), (case.name, BR.failed_edges(case, ref))       # on the reference's numbers only
        report.append((case.name, T, ref["kq"], kept, int(got["kept_count"][s]), float(ref["thr"]), float(got["thr"][s])))
        assert np.array_equal(got["back_errs"][t0:t0 + T], ref["back_errs"]), case.name
        assert np.array_equal(_bits(got["back_errs"][t0:t0 + T]), _bits(ref["back_errs"])), case.name
        if T == 0:
            assert np.isnan(got["thr"][s]), case.name
        else:
            assert _bits(got["thr"][s])[0] == _bits(ref["thr"])[0], (case.name, got["thr"][s], ref["thr"])
        m = got["mask"][t0:t0 + T]
        assert np.all(m <= 1), case.name
        assert np.array_equal(m.astype(bool), ref["mask"]), (case.name, int(m.sum()), kept)
        assert got["kept_count"][s] == kept == int(ref["mask"].sum()), (case.name, got["kept_count"][s], kept)
        assert np.array_equal(got["kept_tuple"][t0:t0 + kept], np.flatnonzero(ref["mask"])), case.name
        assert got["kept_wt"][t0:t0 + kept].tobytes() == ref["kept_wt"].tobytes(), case.name
        assert np.array_equal(got["kept_row0"][t0:t0 + kept], ref["kept_row0"]), case.name
        # nothing past a scene's count, in its own list or a neighbour's
        assert np.all(got["kept_tuple"][t0 + kept:t0 + T] == SENT_I32), case.name
        assert np.all(got["kept_wt"][t0 + kept:t0 + T] == SENT_F64), case.name
        assert np.all(got["kept_row0"][t0 + kept:t0 + T] == SENT_I32), case.name
    print("\n".join("%-22s T %5d kq %5d kept want %5d got %5d thr want %.9g got %.9g" % r for r in report))
    # nothing past the end of any buffer, nor of the workspace
    for k, sent, n in (("mask", SENT_U8, Ttot), ("kept_tuple", SENT_I32, Ttot), ("kept_wt", SENT_F64, Ttot),
                       ("kept_row0", SENT_I32, Ttot), ("back_errs", SENT_F32, Ttot), ("kept_count", SENT_I32, B), ("thr", SENT_F32, B)):
        assert got[k].shape == (n + GUARD,) and np.all(got[k][n:] == sent), k
    assert np.all(got["ws_guard"] == 0x5A)


@pytest.mark.parametrize("name", sorted(BR.BATCHES))
def test_second_launch_into_the_same_buffers_and_workspace_is_identical(name):
    """The hit histogram lives in the workspace, which the first launch leaves full: the entry point's own clear is what makes the
    second launch's weights the first's."""
    first, second = _batch(name)["runs"]
    assert any(r["hits"].max() > 0 for r in _batch(name)["refs"])
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), k


@pytest.mark.parametrize("lone", BR.LONE)
def test_lone_launch_equals_the_scene_rows_of_the_batch(lone):
    """The heavy-tie scene and the thr == 0 scene as B = 1 launches: their outputs are their rows of the batch byte for byte, so
    neither the neighbours nor the shared hit workspace leak into a scene."""
    b = _batch("table")
    s = [c.name for c in b["cases"]].index(lone)
    assert 0 < s < len(b["cases"]) - 1
    runs, _ = _launch(BR.batch_arrays([b["scenes"][s]], [b["cases"][s].ratio]), b["num_rots"], b["axes"], repeat=1)
    t0, T = int(b["arrays"]["tup_off"][s]), b["refs"][s]["T"]
    for k in ("mask", "kept_tuple", "kept_wt", "kept_row0", "back_errs"):
        assert runs[0][k][:T].tobytes() == b["runs"][0][k][t0:t0 + T].tobytes(), (lone, k)
    for k in ("kept_count", "thr"):
        assert runs[0][k][:1].tobytes() == b["runs"][0][k][s:s + 1].tobytes(), (lone, k)


@pytest.mark.parametrize("name", sorted(BR.BATCHES))
def test_kept_rows_of_lists_that_came_from_ties_and_from_nothing_kept(name):
    """cppf_kept_rows / cppf_kept_rows32 on the filter's own device lists, max_kept = max(kidx) + 1: tup_off + flatnonzero(mask),
    padded with the scene's first row (row 0 for the empty scene)."""
    L = _lib.load()
    b = _batch(name)
    dev, B = b["dev"], len(b["cases"])
    max_kept = dev["max_kept"]
    assert max_kept >= max(r["kept"] for r in b["refs"]) and any(r["kept"] == 0 < r["T"] for r in b["refs"])
    want = BR.kept_rows(b["arrays"]["tup_off"], [np.flatnonzero(r["mask"]) for r in b["refs"]], max_kept)
    r64 = torch.full((B * max_kept + GUARD,), -7, dtype=torch.int64, device=DEV)
    r32 = torch.full((B * max_kept + GUARD,), -7, dtype=torch.int32, device=DEV)
    args = (B, ops._p(dev["tup_off"]), ops._p(dev["kept_tuple"]), ops._p(dev["kept_count"]), max_kept)
    _lib.check(L.cppf_kept_rows(*args, ops._p(r64), ops._stream()), "cppf_kept_rows")
    _lib.check(L.cppf_kept_rows32(*args, ops._p(r32), ops._stream()), "cppf_kept_rows32")
    exp = np.concatenate([want.reshape(-1), np.full(GUARD, -7, np.int64)])
    assert np.array_equal(r64.cpu().numpy(), exp)
    assert r32.cpu().numpy().dtype == np.int32 and np.array_equal(r32.cpu().numpy(), exp)
