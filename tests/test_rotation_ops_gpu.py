"""The stand-alone rotation operators -- ops.vote_rotation (cppf_vote_rotation: vr_scan_kernel + vr_emit_kernel) and
ops.sphere_counts / ops.get_topk_dir (cppf_sphere_counts: sphere_counts_kernel + the chunk fold) -- against the oracle at the
sizes where the kernels change path.  Needs an MI355X: run with `pytest -m gpu`.

Inputs and the reasoning behind them: tests/rotation_ops_ref.py (checked on the CPU by tests/test_rotation_ops_ref.py).

Bars: masks, shapes and unweighted / power-of-two-weighted counts are exact; candidate axes are unit vectors compared at 1e-6
(tanf differs from the host's tan by a few ulp -- the bar of the golden test in tests/test_gpu_parity.py, which also keeps the
pi/2 and pi quirks); arbitrary float64 weights get one float32 ulp per chunk fold (derived at the test).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():          # collected but skipped on CPU boxes (they run -m "not gpu" anyway)
    pytest.skip("no HIP device", allow_module_level=True)

import rotation_ops_ref as R                 # noqa: E402
from oracle import cppf_oracle as O          # noqa: E402  (checker only)
from cppf2_amd import _lib, ops              # noqa: E402

DEV = torch.device("cuda")
F32 = np.float32
UP_BAR = 1e-6


def _trig(num_rots):
    """The product's rotation table, as the input it is to both sides."""
    return tuple(t.cpu().numpy() for t in ops.rotation_table(num_rots, DEV))


def _oracle_counts(cand, sph, bmm, tol, wt=None):
    return O.get_topk_dir(cand, sph, bmm, tol, wt, return_counts=True, impl="numpy")[2]


# ------------------------------------------------------------------------------------------ vote_rotation
@pytest.mark.parametrize("case", R.VR_CASES, ids=R.vr_id)
def test_rotation_ops_vote_rotation_compacts_across_scan_blocks(case):
    """Degenerate pairs on both sides of every 1024-pair block edge, a block with no valid pair and one with 1024: the mask is the
    oracle's, the candidates of valid pair number r sit in row r (a wrong carry between blocks misplaces every later row by
    order 1), and with k = 5 the three filler columns are not read."""
    pc, idx, ang = R.vr_inputs(case)
    want, wmask = O.vote_rotation(pc, ang, idx, case.num_rots, trig=_trig(case.num_rots))
    up, mask = ops.vote_rotation(pc, ang, idx, case.num_rots)
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), wmask)
    assert up.dtype == torch.float32 and tuple(up.shape) == (int(wmask.sum()), case.num_rots, 3) == want.shape
    if want.size:
        err = np.abs(up.cpu().numpy() - want).reshape(want.shape[0], -1).max(1)
        print("max |up - want| %.3g (row %d of %d)" % (err.max(), err.argmax(), len(err)))
        assert err.max() <= UP_BAR


@pytest.mark.parametrize("k", [2, 5])
def test_rotation_ops_vote_rotation_without_pairs(k):
    """T = 0: an empty [0, R, 3] tensor and an empty mask, like the reference; nothing is launched over the one-element buffers."""
    up, mask = ops.vote_rotation(R.cloud(), np.zeros((0,), F32), np.zeros((0, k), np.int64), 36)
    torch.cuda.synchronize()
    assert tuple(up.shape) == (0, 36, 3) and up.dtype == torch.float32
    assert tuple(mask.shape) == (0,) and mask.dtype == torch.bool
    want, wmask = O.vote_rotation(R.cloud(), np.zeros((0,), F32), np.zeros((0, k), np.int64), 36)
    assert want.shape == (0, 36, 3) and wmask.shape == (0,)


def test_rotation_ops_vote_rotation_emit_grid_stride():
    """T * num_rots = 5 000 000 > 16384 * 256: vr_emit_kernel's capped grid goes round its loop a second time.  All rows at the
    bar, and the rows of the last 5 % of valid pairs -- all written by the second pass -- once more on their own."""
    case = R.VrCase(5000, 2, 1000, "edges")
    pc, idx, ang = R.vr_inputs(case)
    assert case.T * case.num_rots > R.EMIT_GRID
    trig = _trig(case.num_rots)
    want, wmask = O.vote_rotation(pc, ang, idx, case.num_rots, trig=trig)
    up, mask = ops.vote_rotation(pc, ang, idx, case.num_rots, trig=trig)
    assert np.array_equal(mask.cpu().numpy(), wmask) and tuple(up.shape) == want.shape
    got = up.cpu().numpy()
    assert np.abs(got - want).max() <= UP_BAR
    n = want.shape[0]
    tail = np.arange(n - n // 20, n)
    pairs = np.flatnonzero(wmask)[tail]                                   # the pair behind each tail row
    assert len(tail) >= 200 and pairs.min() * case.num_rots >= R.EMIT_GRID  # items past one pass of the grid
    for r in tail:
        assert np.abs(got[r] - want[r]).max() <= UP_BAR, r
    # a row of the tail is its own pair's: it is far from the rows of the pairs around it
    assert np.abs(want[tail[1:]] - want[tail[:-1]]).reshape(len(tail) - 1, -1).max(1).min() > 1e-3


def test_rotation_ops_vote_rotation_leaves_unwritten_rows_alone():
    """The raw entry point on a sentinel-filled `up` of T rows: rows [n_valid, T) keep the sentinel -- invalid pairs emit nothing
    -- and rows [0, n_valid) are what the wrapper returns."""
    case = R.VrCase(2049, 5, 36, "edges")
    pc, idx, ang = R.vr_inputs(case)
    T, k, num_rots, _ = case
    L = _lib.load()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)
    d_pts, d_idx, d_ang = t(pc, torch.float32), t(idx, torch.int32), t(ang, torch.float32)
    cs, sn = ops.rotation_table(num_rots, DEV)
    up = torch.full((T, num_rots, 3), -7.0, dtype=torch.float32, device=DEV)
    valid = torch.full((T,), 9, dtype=torch.uint8, device=DEV)
    nvalid = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty((T * 4,), dtype=torch.uint8, device=DEV)
    rc = L.cppf_vote_rotation(ops._p(d_pts), pc.shape[0], ops._p(d_idx), k, T, ops._p(d_ang), num_rots, ops._p(cs), ops._p(sn),
                              ops._p(up), ops._p(valid), ops._p(nvalid), ops._p(ws), ws.numel(), ops._stream())
    assert rc == 0
    wmask = O.vote_rotation(pc, ang, idx, 1)[1]
    n = int(nvalid.item())
    assert n == int(wmask.sum()) and 0 < n < T
    assert np.array_equal(valid.cpu().numpy(), wmask.astype(np.uint8))
    got = up.cpu().numpy()
    assert np.all(got[n:] == F32(-7.0))
    assert not np.any(got[:n] == F32(-7.0))
    assert np.array_equal(got[:n], ops.vote_rotation(pc, ang, idx, num_rots)[0].cpu().numpy())


# ------------------------------------------------------------------------------------------ sphere_counts
@pytest.mark.parametrize("case", R.SC_CASES, ids=R.sc_id)
def test_rotation_ops_sphere_counts_at_chunk_and_sub_block_edges(case):
    """M on the 512-row sub-block edges, on the chunk edges and 0; chunks shorter than a sub-block; bin counts around the
    256-thread loop; an all-zero and a NaN candidate.  Unweighted counts are integers below 2^24 and power-of-two float64
    weights make every float64 sum exact, so both equal the oracle's bit for bit whatever order the atomics arrive in."""
    M, bmm, S, tol = case
    sph = R.sphere(S)
    cand = R.candidates(M, sph, tol)
    want = _oracle_counts(cand, sph, bmm, tol)
    got = ops.sphere_counts(cand, sph, bmm, tol)
    assert got.dtype == torch.float32 and tuple(got.shape) == (S,)
    assert np.array_equal(got.cpu().numpy(), want)
    assert want.sum() > 0 or M < 100                    # not an all-zero agreement
    w = R.pow2_weights(M)
    want_w = _oracle_counts(cand, sph, bmm, tol, w)
    assert np.array_equal(ops.sphere_counts(cand, sph, bmm, tol, w).cpu().numpy(), want_w)
    assert M == 0 or not np.array_equal(want_w, want) or want.sum() == 0


def test_rotation_ops_sphere_counts_arbitrary_float64_weights():
    """Weights in imp_pair_wt's range [0.01, 2.01], C = 21 chunks.  A chunk's float64 sum of up to 100 quotients differs from the
    oracle's (another summation order) by about 1e-14 relative -- far less than half a float32 ulp (6e-8) -- so a fold
    `counts = float32(counts + sum)` rounds both the same way unless the exact value lies that close to a float32 tie, where
    the two may land one ulp apart.  Every later fold carries that ulp and may add one: at most C ulps of the final count (the
    counts only grow, so no partial count has a larger ulp)."""
    M, bmm, S, tol = 2049, 100, 720, 10.0
    C_ = R.n_chunks(M, bmm)
    sph = R.sphere(S)
    cand = R.candidates(M, sph, tol)
    w = np.random.RandomState(5).uniform(0.01, 2.01, (M, 1))
    want = _oracle_counts(cand, sph, bmm, tol, w)
    got = ops.sphere_counts(cand, sph, bmm, tol, w).cpu().numpy()
    ulps = np.abs(got.astype(np.float64) - want) / np.spacing(np.maximum(got, want))
    print("chunks %d, largest difference %.1f ulp, bins that differ %d of %d" % (C_, ulps.max(), (ulps > 0).sum(), S))
    assert C_ == 21 and want.min() > 0
    assert ulps.max() <= C_


@pytest.mark.parametrize("S,tol", [(64, 10.0), (720, 1.0)])
def test_rotation_ops_sphere_counts_dot_product_order_on_the_cone_edge(S, tol):
    """Candidates whose hit flips between fma(z,bz, fma(y,by, x*bx)) and the plain float32 sum (and, in the counts, the chain
    started from z): the kernel's counts equal the oracle's exactly, in one chunk and in chunks of 100."""
    cs = R.cone_edge_set(S, tol)
    assert len(cs.cand) >= 32
    want = _oracle_counts(cs.cand, cs.sphere, 100000, tol)
    assert not np.array_equal(want, R.counts_with(R.dot_plain, cs.cand, cs.sphere, tol))
    for bmm in (100000, 100):
        got = ops.sphere_counts(cs.cand, cs.sphere, bmm, tol).cpu().numpy()
        assert np.array_equal(got, want), bmm


def test_rotation_ops_sphere_counts_float32_weights_are_promoted():
    """The reference divides in the weights' own dtype; ops.sphere_counts promotes them to float64 (its docstring).  For
    power-of-two float32 weights both divisions are exact: counts equal the oracle's float32 division and the float64 run."""
    M, bmm, S, tol = 1025, 512, 257, 10.0
    sph = R.sphere(S)
    cand = R.candidates(M, sph, tol)
    w64 = R.pow2_weights(M)
    w32 = w64.astype(F32)
    want = _oracle_counts(cand, sph, bmm, tol, w32)
    assert want.sum() > 0
    for w in (w32, torch.from_numpy(w32), torch.from_numpy(w32).to(DEV), w32.astype(np.float16)):
        assert np.array_equal(ops.sphere_counts(cand, sph, bmm, tol, w).cpu().numpy(), want)
    assert np.array_equal(ops.sphere_counts(cand, sph, bmm, tol, w64).cpu().numpy(), want)


# ------------------------------------------------------------------------------------------ get_topk_dir
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("S,tol", [(64, 10.0), (720, 1.0)])
def test_rotation_ops_get_topk_dir_equals_oracle_where_the_top_is_distinct(S, tol, weighted):
    sph = R.sphere(S)
    cand = R.clustered_candidates(sph, tol)
    w = R.pow2_weights(len(cand)) if weighted else None
    allc = _oracle_counts(cand, sph, 100, tol, w)
    assert R.leading_counts_distinct(allc, 5)            # torch.topk and the reference leave the order of ties open
    for topk in (1, 5):
        wd, wc = O.get_topk_dir(cand, sph, 100, tol, w, topk=topk)
        gd, gc = ops.get_topk_dir(cand, sph, 100, tol, w, topk=topk)
        assert gd.shape == (topk, 3) and gc.shape == (topk,) and gd.dtype == np.float32 and gc.dtype == np.float32
        assert np.array_equal(gc, wc) and np.array_equal(gd, wd), topk


def test_rotation_ops_get_topk_dir_without_candidates():
    sph = R.sphere(64)
    none = np.zeros((0, 3), F32)
    assert np.array_equal(ops.sphere_counts(none, sph, 100, 1.0).cpu().numpy(), np.zeros(64, F32))
    dirs, cnts = ops.get_topk_dir(none, sph, 100, 1.0, topk=5)
    assert dirs.shape == (5, 3) and np.array_equal(cnts, np.zeros(5, F32))
    dirs, cnts = ops.get_topk_dir(torch.zeros((0, 3), device=DEV), sph, 100000, 10.0, np.zeros((0, 1)), topk=1)
    assert dirs.shape == (1, 3) and np.array_equal(cnts, np.zeros(1, F32))
    assert np.array_equal(O.get_topk_dir(none, sph, 100, 1.0, topk=5)[1], np.zeros(5, F32))
