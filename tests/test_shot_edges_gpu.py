"""SHOT normals / descriptors (cppf_shot.hip) against oracle/shot_oracle.c at the edges the kernels' own constants mark -- the
paths tests/test_shot.py (object-sized clouds, ~90..300 neighbours, equal radii) never reaches:

  CELL_CAP 16384      cells a scene's grid may have: shot_cells coarsens the cell edge by 1.26 until it fits (case 2);
  128 / 313 / 512 / 1024   list capacities: 64 * PCL_EMAX_SHORT and the histogram kernel's register arm, COV_LIST, NBR_CAP,
                      SH_LCAP (case 1: one scene on either side of each; case 3: both sides of NBR_CAP inside one scene);
  unequal radii       the max(rn, rs) list and its per-radius filters, the filtered copy and the rebuild of the histogram kernel
                      (case 3); tiny and empty scenes inside a batch (case 4); independence of batch neighbours (case 5); the
                      entry points no test held to a reference (case 6); the strict d2 < r2 rule hit exactly (case 7).

Every comparison goes through hold() (bars, exemption by the oracle's diagnostics, caps: the ones of tests/test_shot.py).  The
unmarked tests run on the CPU: they assert that each input reaches the path it is named for (neighbour counts, coarsening steps
recomputed with the kernel's formula, eigenvalue gaps) and that the oracle alone stays inside every cap, so an input that is
edited later stops the suite instead of falling back onto the common path.

PCL arithmetic and long lists: a query whose list over max(normal_r, shot_r) holds more than NBR_CAP entries keeps the float64
normal (SHOT section).  reference() builds exactly that: the oracle's normals of either arithmetic chosen per row
by that count, and the oracle's descriptors of those normals (S.describe)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import shot_oracle as S
from cppf2_amd import synth

CELL_CAP, PCL_SHORT, COV_LIST, NBR_CAP, SH_LCAP = 16384, 128, 313, 512, 1024     # cppf_shot.hip
ARITHS = ("f64", "pcl")
# tests/test_shot.py's bars: normals, frames, descriptors, and the margin below which the oracle calls a row undecided
BARS = {"f64": dict(n=2e-6, rf=2e-5, d=2e-5, margin=1e-6), "pcl": dict(n=2e-5, rf=2e-5, d=5e-5, margin=2e-5)}
RIM_MARGIN = 4e-7
OVER_BAR_CAP = 2e-2


# ------------------------------------------------------------------------------------------------------------------------
# the one comparison
# ------------------------------------------------------------------------------------------------------------------------
def exempt_rows(diag, arith):
    """Rows the ORACLE calls undecided: a neighbour within `margin` of a decision boundary of PCL's interpolation, or a point
    within 4e-7 (relative, squared) of the support's rim.  NaN diagnostics (rows without a descriptor) compare false."""
    with np.errstate(invalid="ignore"):
        return (diag[:, 5] < BARS[arith]["margin"]) | (diag[:, 8] < RIM_MARGIN)


def exempt_share(ref, arith):
    ok = ~np.isnan(ref["shot"]).any(1)
    return float(exempt_rows(ref["diag"], arith)[ok].mean()) if ok.any() else 0.0


def hold(got, ref, arith, cap, what=""):
    """got: dict(shot[, normal][, rf]) of the GPU; ref: the oracle's dict(shot, normal, rf, diag[, nbar]) for the same rows.
    NaN patterns equal; normals under their bar (ref["nbar"]: per row, where a run mixes the arithmetics); frames under 2e-5;
    every descriptor row the oracle does not exempt under the bar; the exempt share under `cap`, the share of rows at or
    above the bar under 2e-2; valid rows of unit norm.  Prints each figure before it asserts."""
    bars = BARS[arith]
    fig = {}
    if "normal" in got:
        assert np.array_equal(np.isnan(got["normal"]), np.isnan(ref["normal"])), what + ": NaN pattern of the normals"
        nerr = np.nan_to_num(np.abs(got["normal"] - ref["normal"]).max(1), nan=0.0)
        nbar = ref.get("nbar", np.full(len(nerr), bars["n"]))
        fig["normal_err/bar"] = float((nerr / nbar).max()) if len(nerr) else 0.0
    if got.get("rf") is not None:
        assert np.array_equal(np.isnan(got["rf"]), np.isnan(ref["rf"])), what + ": NaN pattern of the frames"
        fig["rf_err"] = float(np.nan_to_num(np.abs(got["rf"] - ref["rf"]), nan=0.0).max()) if got["rf"].size else 0.0
    assert np.array_equal(np.isnan(got["shot"]), np.isnan(ref["shot"])), what + ": NaN pattern of the descriptors"
    ok = ~np.isnan(ref["shot"]).any(1)
    err = np.abs(got["shot"][ok] - ref["shot"][ok]).max(1)
    ex = exempt_rows(ref["diag"], arith)[ok]
    fig["desc_err_not_exempt"] = float(err[~ex].max()) if (~ex).any() else 0.0
    fig["exempt_share"] = float(ex.mean()) if ok.any() else 0.0
    fig["over_bar_share"] = float((err >= bars["d"]).mean()) if ok.any() else 0.0
    norm = np.linalg.norm(got["shot"][ok].astype(np.float64), axis=1)
    fig["norm_err"] = float(np.abs(norm - 1.0).max()) if ok.any() else 0.0
    print("hold %s [%s]: %s" % (what, arith, fig))
    assert fig.get("normal_err/bar", 0.0) < 1.0, (what, fig)
    assert fig.get("rf_err", 0.0) < bars["rf"], (what, fig)
    assert fig["desc_err_not_exempt"] < bars["d"], (what, fig)
    assert fig["exempt_share"] < cap, (what, fig)
    assert fig["over_bar_share"] < OVER_BAR_CAP, (what, fig)
    assert fig["norm_err"] < 1e-5, (what, fig)
    return fig


# ------------------------------------------------------------------------------------------------------------------------
# inputs (by name, built once) and the oracle's answers (once per name, radii and arithmetic)
# ------------------------------------------------------------------------------------------------------------------------
def _patch(n, seed):
    """A small curved, anisotropic surface patch, 30 x 17.5 mm: z = 16 u^2 - 10 v^2 + 2.4 u v + noise of +-0.25 mm, tilted by 0.4
    rad about x, at (0.03, -0.02, 0.8).  Its diameter (35 mm) is below the 50 mm radius of case 1: every query sees all n."""
    rng = np.random.RandomState(seed)
    u = rng.uniform(-0.015, 0.015, n)
    v = rng.uniform(-0.00875, 0.00875, n)
    z = 16 * u * u - 10 * v * v + 2.4 * u * v + rng.uniform(-0.00025, 0.00025, n)
    c, s = np.cos(0.4), np.sin(0.4)
    R = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    return (np.stack([u, v, z], -1) @ R.T + np.array([0.03, -0.02, 0.8])).astype(np.float32)


CAP_SIZES = (128, 129, 313, 314, 512, 513, 1024, 1025)
TINY_SIZES = (0, 1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 0, 300, 0)
G = 2.0 ** -9                  # case 7's lattice; RIM_R = 8 steps: coordinates, differences and squared distances exact in float32
RIM_R = 2.0 ** -6
RIM_Q = np.array([0.0, 0.0, 0.75])
RIM_INSIDE = np.array([[3, 1, 0], [-2, 3, 1], [1, -3, 2], [-1, -2, -3], [2, 2, -2]]) * G
RIM_FAR = np.array([-20, -24, -28]) * G          # a point far outside: the scene's grid gets several cells in every direction


def rim_scene(kind, axis, inside):
    """query (row 0), points inside, one point at exactly 8 lattice steps along `axis` (last-but-one row; `inside`: moved one
    float32 step towards the query), one far point.  kind: 'normal' = 1 inside point, 'desc' = 4, 'value' = 5."""
    k = {"normal": 1, "desc": 4, "value": 5}[kind]
    rim = RIM_Q.astype(np.float32).copy()
    rim[axis] = np.float32(RIM_Q[axis] + RIM_R)
    if inside:
        rim[axis] = np.nextafter(rim[axis], np.float32(RIM_Q[axis]))
    pc = np.concatenate([RIM_Q[None], RIM_Q + RIM_INSIDE[:k], rim[None].astype(np.float64), (RIM_Q + RIM_FAR)[None]])
    out = pc.astype(np.float32)
    out[k + 1] = rim                              # (bit-exact: not through float64 and back)
    return out


def rim_dense_scene(n, inside):
    """query (row 0) with n - 1 random lattice points strictly inside the radius (none on the shell boundaries at 2, 4 and 6
    steps, where the histogram's own decisions sit), the six lattice points at exactly 8 steps (`inside`: each moved one float32
    step towards the query), one far point.  n > NBR_CAP: the histogram kernel rebuilds its list; n > SH_LCAP: it rescans."""
    k = np.arange(-8, 9)
    o = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    q2 = (o ** 2).sum(1)
    o = o[(q2 > 0) & (q2 < 64) & (q2 != 4) & (q2 != 16) & (q2 != 36) & (np.abs(o[:, 1]) <= 4) & (o[:, 2] >= -4)]      # (a lopsided ball)
    o = o[np.random.RandomState(n).permutation(len(o))[:n - 1]]
    rim = np.concatenate([8 * np.eye(3), -8 * np.eye(3)])
    out = (RIM_Q + np.concatenate([np.zeros((1, 3)), o, rim, RIM_FAR[None] / G]) * G).astype(np.float32)
    if inside:
        for i in range(6):
            a = i % 3
            out[n + i, a] = np.nextafter(out[n + i, a], out[0, a])
    return out


@functools.lru_cache(maxsize=None)
def cloud(name):
    if name.startswith("patch"):
        return _patch(int(name[5:]), int(name[5:]))
    if name.startswith("prefix"):
        return _patch(300, 300)[:int(name[6:])].copy()
    if name == "wide":                            # two objects 1.25 m apart in one scene, rows shuffled
        a, b = synth.make_scene(0, 0, 1500)["pc"], synth.make_scene(0, 1, 1500)["pc"]
        pc = np.concatenate([a, b + np.float32([0.9, 0.7, 0.5])]).astype(np.float32)
        return pc[np.random.RandomState(0).permutation(len(pc))].copy()
    if name == "plain777":
        return synth.make_scene(5, 1, 777)["pc"]
    if name == "plain65":
        return synth.make_scene(8, 0, 65)["pc"]
    if name == "obj1500":
        return synth.make_scene(0, 0, 1500)["pc"]
    if name == "voxel":
        return synth.make_scene_voxel2mm(0, 0, 4096)["pc"]
    if name.startswith("rimdense_"):
        _, n, where = name.split("_")
        return rim_dense_scene(int(n), where == "in")
    if name.startswith("rim_"):
        _, kind, axis, where = name.split("_")
        return rim_scene(kind, int(axis), where == "in")
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def counts(name, r):
    """Points with d2 < r^2 (self included) per query, in the kernels' float32 arithmetic ((dx dx + dy dy) + dz dz)."""
    pc = cloud(name)
    r2 = np.float32(r) * np.float32(r)
    out = np.zeros(len(pc), np.int64)
    for lo in range(0, len(pc), 512):
        d = pc[lo:lo + 512, None, :] - pc[None, :, :]
        out[lo:lo + 512] = (((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) < r2).sum(1)
    return out


@functools.lru_cache(maxsize=None)
def oracle(name, rn, rs, arith):
    s, n, rf, d = S.compute_ex(cloud(name), rn, rs, pcl_arithmetic=(arith == "pcl"))
    return dict(shot=s, normal=n, rf=rf, diag=d)


@functools.lru_cache(maxsize=None)
def reference(name, rn, rs, arith):
    """What the kernels are documented to compute, and the arithmetic whose bars hold it: (ref, bars' arithmetic).  "f64": the
    oracle.  "pcl": the oracle's PCL mode where no list over max(rn, rs) exceeds NBR_CAP; the float64 oracle where every list
    does; otherwise the normals of either mode chosen per row (nbar: that row's bar) and the oracle's descriptors of them."""
    if arith == "f64":
        return oracle(name, rn, rs, "f64"), "f64"
    big = counts(name, max(rn, rs)) > NBR_CAP
    if not big.any():
        return oracle(name, rn, rs, "pcl"), "pcl"
    if big.all():
        return oracle(name, rn, rs, "f64"), "f64"
    n = np.where(big[:, None], oracle(name, rn, rs, "f64")["normal"], oracle(name, rn, rs, "pcl")["normal"])
    s, rf, d = S.describe(cloud(name), n, rs, pcl_arithmetic=True)
    return dict(shot=s, normal=n, rf=rf, diag=d, nbar=np.where(big, BARS["f64"]["n"], BARS["pcl"]["n"]), big=big), "pcl"


def coarsening(pc, r):
    """shot_cells_kernel's loop in its float32 arithmetic: (steps, cell edge, cells)."""
    ext = (pc.max(0) - pc.min(0)).astype(np.float32)
    edge, steps = np.float32(r) * np.float32(1.0005), 0
    while True:
        dims = [int(np.float32(e / edge)) + 1 for e in ext]
        if dims[0] * dims[1] * dims[2] <= CELL_CAP:
            return steps, float(edge), dims[0] * dims[1] * dims[2]
        edge = np.float32(edge * np.float32(1.26))
        steps += 1


def lrf_gap(ref):
    """Smallest relative gap between neighbouring LRF eigenvalues over the rows that have a frame."""
    d = ref["diag"]
    ok = ~np.isnan(d[:, 0])
    return float(np.minimum((d[ok, 0] - d[ok, 1]) / d[ok, 0], (d[ok, 1] - d[ok, 2]) / d[ok, 0]).min())


# ------------------------------------------------------------------------------------------------------------------------
# GPU plumbing
# ------------------------------------------------------------------------------------------------------------------------
def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from cppf2_amd import ops, shot
    return torch, ops, shot


def _batch(names):
    torch, ops, _ = _gpu()
    pcs = [cloud(n) for n in names]
    sizes = [len(p) for p in pcs]
    pts = torch.as_tensor(np.concatenate(pcs).reshape(-1, 3)).cuda()
    return pts, ops._offsets(sizes, pts.device), np.concatenate([[0], np.cumsum(sizes)])


def _compute(names, rn, rs, arith):
    """compute_device(want_rf=True) on the batch: one dict(shot, normal, rf) per scene."""
    _, _, shot = _gpu()
    pts, off, o = _batch(names)
    s, n, rf = (t.cpu().numpy() for t in shot.compute_device(pts, off, rn, rs, want_rf=True, arithmetic=arith))
    return [dict(shot=s[o[i]:o[i + 1]], normal=n[o[i]:o[i + 1]], rf=rf[o[i]:o[i + 1]]) for i in range(len(names))]


# ------------------------------------------------------------------------------------------------------------------------
# 1. capacity steps: 128|129, 313|314, 512|513, 1024|1025 neighbours for every query of a scene
# ------------------------------------------------------------------------------------------------------------------------
CAP_NAMES = tuple("patch%d" % n for n in CAP_SIZES)
CAP_R = 0.05
CAP_EXEMPT = {"f64": 0.02, "pcl": 0.20}


def _cap_colours():
    rng = np.random.RandomState(11)
    cols = [rng.rand(n, 3).astype(np.float32) for n in CAP_SIZES]
    cols[3][:] = cols[3][0]                       # a patch of a single colour
    return cols


@functools.lru_cache(maxsize=None)
def _cap_colour_oracle(i):
    s, n, d = S.compute_color(cloud(CAP_NAMES[i]), _cap_colours()[i], CAP_R, CAP_R)
    return dict(shot=s, normal=n, diag=d)


def test_capacity_inputs_sit_on_the_capacities():
    assert sorted(CAP_SIZES) == sorted([PCL_SHORT, PCL_SHORT + 1, COV_LIST, COV_LIST + 1, NBR_CAP, NBR_CAP + 1, SH_LCAP, SH_LCAP + 1])
    for name, n in zip(CAP_NAMES, CAP_SIZES):
        pc = cloud(name)
        assert coarsening(pc, CAP_R)[2] == 1                             # one cell: every point is a candidate
        assert np.all(counts(name, CAP_R) == n)
        for arith in ARITHS:
            ref = oracle(name, CAP_R, CAP_R, arith)
            assert np.all(ref["diag"][:, 7] == n)
            assert not np.isnan(ref["shot"]).any() and not np.isnan(ref["normal"]).any()
            assert lrf_gap(ref) >= 0.02, (name, lrf_gap(ref))
            assert exempt_share(ref, arith) < CAP_EXEMPT[arith], (name, arith, exempt_share(ref, arith))
        # the bars tell the two arithmetics apart: a scene above NBR_CAP that is held to the float64 oracle (reference()) would
        # not pass against the PCL one, and the other way round
        dn = np.abs(oracle(name, CAP_R, CAP_R, "f64")["normal"] - oracle(name, CAP_R, CAP_R, "pcl")["normal"]).max()
        assert dn > 50 * BARS["pcl"]["n"], (name, float(dn))
        assert reference(name, CAP_R, CAP_R, "pcl")[1] == ("f64" if n > NBR_CAP else "pcl")
    for i in range(len(CAP_SIZES)):
        assert exempt_share(_cap_colour_oracle(i), "f64") < CAP_EXEMPT["f64"]
    one = _cap_colour_oracle(3)["shot"][:, 352:].reshape(-1, 32, 31)
    assert np.all(one[:, :, 1:] == 0) and one[:, :, 0].sum() > 0        # the single-colour patch fills colour slot 0 only


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ARITHS)
def test_capacity_steps_vs_oracle(arith):
    """Eight scenes whose every query has exactly 128, 129, 313, 314, 512, 513, 1024, 1025 neighbours, one ragged batch: the
    register arm and the list arm of shot_hist, shot_cov's ranked short list, LDS list and direct sums, shot_pcl_long's
    capacity, the rebuild above NBR_CAP and the rescan above SH_LCAP.  PCL arithmetic above 512: the float64 oracle."""
    got = _compute(CAP_NAMES, CAP_R, CAP_R, arith)
    for name, g in zip(CAP_NAMES, got):
        ref, bars = reference(name, CAP_R, CAP_R, arith)
        hold(g, ref, bars, CAP_EXEMPT[bars], name)


@pytest.mark.gpu
def test_capacity_steps_colour_vs_oracle():
    """shot_hist_kernel<true> (SHOT1344; no register arm) on the same eight scenes, float64 normals like the colour oracle."""
    torch, _, shot = _gpu()
    pts, off, o = _batch(CAP_NAMES)
    col = torch.as_tensor(np.concatenate(_cap_colours())).cuda()
    s, n = (t.cpu().numpy() for t in shot.compute_color_device(pts, col, off, CAP_R, CAP_R, arithmetic="f64"))
    for i, name in enumerate(CAP_NAMES):
        hold(dict(shot=s[o[i]:o[i + 1]], normal=n[o[i]:o[i + 1]]), _cap_colour_oracle(i), "f64", CAP_EXEMPT["f64"], name + " colour")


# ------------------------------------------------------------------------------------------------------------------------
# 2. a grid that must be coarsened
# ------------------------------------------------------------------------------------------------------------------------
WIDE = {0.02: dict(steps=2, edge=1.6, nan=(0.0, 0.01)), 0.01: dict(steps=5, edge=3.2, nan=(0.05, 0.2))}
WIDE_EXEMPT = 0.12


def test_wide_scene_is_coarsened():
    for r, w in WIDE.items():
        steps, edge, cells = coarsening(cloud("wide"), r)
        assert steps == w["steps"] and abs(edge / r - w["edge"]) < 0.1 and CELL_CAP / 2 < cells <= CELL_CAP, (r, steps, edge / r, cells)
        assert coarsening(cloud("plain777"), r)[0] == 0                  # the batch's other header is not coarsened
        for arith in ARITHS:
            ref = oracle("wide", r, r, arith)
            nan = np.isnan(ref["shot"]).any(1).mean()
            assert w["nan"][0] <= nan < w["nan"][1], (r, nan)
            assert exempt_share(ref, arith) < WIDE_EXEMPT, (r, arith, exempt_share(ref, arith))
            assert exempt_share(oracle("plain777", r, r, arith), arith) < WIDE_EXEMPT


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("r", sorted(WIDE))
def test_coarsened_grid_vs_oracle(r, arith):
    """Two objects 1.25 m apart in one scene: the grid at the radius has far more than CELL_CAP cells, shot_cells multiplies the
    edge by 1.26 twice (r = 2 cm, cells 1.6 r wide) or five times (r = 1 cm, 3.2 r; a tenth of the rows NaN for lack of
    neighbours).  An ordinary scene shares the batch."""
    names = ("wide", "plain777")
    for name, g in zip(names, _compute(names, r, r, arith)):
        ref, bars = reference(name, r, r, arith)
        hold(g, ref, bars, WIDE_EXEMPT, "%s r=%g" % (name, r))


# ------------------------------------------------------------------------------------------------------------------------
# 3. unequal radii, both ways
# ------------------------------------------------------------------------------------------------------------------------
PAIRS = ((0.01, 0.03), (0.03, 0.015))
PAIR_EXEMPT = 0.15


def test_unequal_radii_reach_both_sides_of_nbr_cap():
    big = counts("voxel", 0.03)
    assert 520 < big.mean() < 600 and big.max() > 650
    assert 0.6 < (big > NBR_CAP).mean() < 0.8 and (big > COV_LIST).mean() > 0.95 and (big <= NBR_CAP).sum() > 500
    assert np.array_equal(big, oracle("voxel", 0.01, 0.03, "pcl")["diag"][:, 7].astype(np.int64))
    assert counts("voxel", 0.01).max() < PCL_SHORT and counts("voxel", 0.015).max() < COV_LIST
    small = counts("obj1500", 0.03)
    assert small.max() <= PCL_SHORT and small.mean() > 40                # the short-list arm: pcl_list entries filtered by ed < rn2
    for name in ("voxel", "obj1500"):
        for rn, rs in PAIRS:
            for arith in ARITHS:
                ref, bars = reference(name, rn, rs, arith)
                assert np.isnan(ref["shot"]).any(1).mean() < 0.01
                assert exempt_share(ref, bars) < PAIR_EXEMPT, (name, rn, rs, arith, exempt_share(ref, bars))
            if name == "voxel":
                ref = reference(name, rn, rs, "pcl")[0]
                assert 0 < ref["big"].sum() < len(ref["big"])            # rows of both arithmetics in one run
                # ... and the bars tell which arithmetic a row got
                dn = np.abs(oracle(name, rn, rs, "f64")["normal"] - oracle(name, rn, rs, "pcl")["normal"]).max(1)
                assert np.median(dn[ref["big"]]) > 5 * BARS["pcl"]["n"] and np.median(dn[~ref["big"]]) > 5 * BARS["pcl"]["n"]


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("rn,rs", PAIRS)
@pytest.mark.parametrize("name", ["voxel", "obj1500"])
def test_unequal_radii_vs_oracle(name, rn, rs, arith):
    """normal_r != shot_r on a 2 mm voxel cloud (558 points on average inside 3 cm: both sides of NBR_CAP in one run) and on an
    object cloud (short lists).  (0.01, 0.03): shot_cov filters the shared list by rn for the normal sums.  (0.03, 0.015):
    shot_hist filters the shared list when it has at most NBR_CAP entries and rebuilds its own otherwise.  PCL arithmetic:
    normals per row by the documented rule (the list over the LARGER radius decides; reference()), descriptors against the
    oracle fed with exactly those normals -- neither of the issue's two fall-backs (grouping with exempt straddlers, float64
    descriptors only) is needed."""
    ref, bars = reference(name, rn, rs, arith)
    hold(_compute((name,), rn, rs, arith)[0], ref, bars, PAIR_EXEMPT, "%s (%g, %g)" % (name, rn, rs))


# ------------------------------------------------------------------------------------------------------------------------
# 4. tiny and empty scenes in one batch
# ------------------------------------------------------------------------------------------------------------------------
TINY_NAMES = tuple("prefix%d" % n for n in TINY_SIZES)
TINY_R = 0.02
TINY_EXEMPT = 0.15


def test_tiny_scenes_nan_policy_of_the_oracle():
    for name, n in zip(TINY_NAMES, TINY_SIZES):
        for arith in ARITHS:
            ref = oracle(name, TINY_R, TINY_R, arith)
            assert ref["shot"].shape == (n, 352)
            assert np.isnan(ref["normal"]).all() if n < 3 else not np.isnan(ref["normal"]).all()
            assert np.isnan(ref["shot"]).all() and np.isnan(ref["rf"]).all() if n < 6 else not np.isnan(ref["shot"]).all()
            assert np.array_equal(np.isnan(ref["shot"]).any(1), np.isnan(ref["rf"]).any(1))
            assert exempt_share(ref, arith) < TINY_EXEMPT, (name, arith, exempt_share(ref, arith))


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ARITHS)
def test_tiny_and_empty_scenes_in_one_batch(arith):
    """Scenes of 0 .. 7 and 63 / 64 / 65 points (prefixes of one patch) with empty scenes first, in the middle and last:
    normals NaN below 3 points, descriptors and frames NaN below 6, the rest held to the bars; out_rf is NaN exactly where the
    descriptor is."""
    for name, n, g in zip(TINY_NAMES, TINY_SIZES, _compute(TINY_NAMES, TINY_R, TINY_R, arith)):
        assert g["shot"].shape == (n, 352) and g["normal"].shape == (n, 3) and g["rf"].shape == (n, 9)
        if n < 3:
            assert np.isnan(g["normal"]).all()
        if n < 6:
            assert np.isnan(g["shot"]).all() and np.isnan(g["rf"]).all()
        assert np.array_equal(np.isnan(g["shot"]).all(1), np.isnan(g["rf"]).all(1))
        ref, bars = reference(name, TINY_R, TINY_R, arith)
        hold(g, ref, bars, TINY_EXEMPT, name)


@pytest.mark.gpu
def test_all_scenes_empty_is_ok_and_writes_nothing():
    torch, ops, shot = _gpu()
    from cppf2_amd import _lib
    L = _lib.load()
    dev = ops._dev()
    pts = torch.zeros((1, 3), dtype=torch.float32, device=dev)           # (a non-null pointer; total_points = 0)
    off = ops._offsets([0, 0, 0], dev)
    out = [torch.full(shape, 7.0, dtype=torch.float32, device=dev) for shape in ((1, 352), (1, 3), (1, 9), (1, 1344))]
    f = C.c_float(0.02)
    for flags in (0, 1):
        _lib.check(L.cppf_shot352(3, ops._p(pts), ops._p(off), 0, f, f, ops._p(out[0]), ops._p(out[1]), ops._p(out[2]), None, 0,
                                  flags, ops._stream()), "cppf_shot352")
        _lib.check(L.cppf_estimate_normals(3, ops._p(pts), ops._p(off), 0, f, ops._p(out[1]), None, 0, flags, ops._stream()),
                   "cppf_estimate_normals")
        _lib.check(L.cppf_shot1344(3, ops._p(pts), ops._p(pts), ops._p(off), 0, f, f, ops._p(out[3]), ops._p(out[1]), None, 0, flags,
                                   ops._stream()), "cppf_shot1344")
    _lib.check(L.cppf_shot352_from_normals(3, ops._p(pts), ops._p(off), 0, ops._p(pts), f, ops._p(out[0]), ops._p(out[2]), None, 0,
                                           ops._stream()), "cppf_shot352_from_normals")
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in out)
    assert L.cppf_shot352_workspace_bytes(3, 0) == 0


# ------------------------------------------------------------------------------------------------------------------------
# 5. batch independence
# ------------------------------------------------------------------------------------------------------------------------
INDEP_NAMES = ("plain65", "plain777", "patch513")
INDEP_R = 0.05


def test_independence_scenes_differ_in_kind():
    assert [len(cloud(n)) for n in INDEP_NAMES] == [65, 777, 513]
    assert np.all(counts("patch513", INDEP_R) == 513)                    # above NBR_CAP: rebuilt lists, float64 fallback
    c = counts("plain777", INDEP_R)
    assert PCL_SHORT < c.max() <= NBR_CAP and c.min() < PCL_SHORT        # shot_pcl_long and the short list in one scene
    assert not np.isnan(oracle("plain65", INDEP_R, INDEP_R, "f64")["shot"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ARITHS)
def test_rows_do_not_depend_on_batch_neighbours(arith):
    """Each scene alone, in a batch and in the reversed batch: byte-identical descriptors, normals and frames.  (The sums run
    in the scene's cell order; where points share a cell, their order inside it comes from LDS atomics of one workgroup per
    scene -- the same for the same scene wherever it sits in a batch, which is what this pins.)"""
    alone = [_compute((n,), INDEP_R, INDEP_R, arith)[0] for n in INDEP_NAMES]
    fwd = _compute(INDEP_NAMES, INDEP_R, INDEP_R, arith)
    rev = _compute(INDEP_NAMES[::-1], INDEP_R, INDEP_R, arith)[::-1]
    for name, a, f, r in zip(INDEP_NAMES, alone, fwd, rev):
        for key in ("shot", "normal", "rf"):
            assert a[key].tobytes() == f[key].tobytes(), (name, key, "alone vs batch")
            assert a[key].tobytes() == r[key].tobytes(), (name, key, "alone vs reversed batch")


# ------------------------------------------------------------------------------------------------------------------------
# 6. the entry points nothing held to a reference
# ------------------------------------------------------------------------------------------------------------------------
ENTRY_NAMES = TINY_NAMES + ("wide",)


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ARITHS)
def test_normals_and_from_normals_entries_vs_oracle(arith):
    """cppf_estimate_normals (normals_device) against S.normals / compute_ex's PCL normals on the ragged batch of case 4 and the
    coarsened scene of case 2; cppf_shot352_from_normals (descriptors_device) fed with those normals against the oracle of the
    same arithmetic, and byte-equal to cppf_shot352's descriptors (the same lists, frames and normals)."""
    _, _, shot = _gpu()
    pts, off, o = _batch(ENTRY_NAMES)
    nrm = shot.normals_device(pts, off, TINY_R, arithmetic=arith)
    desc = shot.descriptors_device(pts, off, nrm, TINY_R).cpu().numpy()
    whole, whole_n = (t.cpu().numpy() for t in shot.compute_device(pts, off, TINY_R, TINY_R, arithmetic=arith))
    nrm = nrm.cpu().numpy()
    assert nrm.tobytes() == whole_n.tobytes()
    assert desc.tobytes() == whole.tobytes()
    for i, name in enumerate(ENTRY_NAMES):
        ref, bars = reference(name, TINY_R, TINY_R, arith)
        assert bars == arith
        if arith == "f64":
            assert np.array_equal(ref["normal"], S.normals(cloud(name), TINY_R), equal_nan=True)
        hold(dict(shot=desc[o[i]:o[i + 1]], normal=nrm[o[i]:o[i + 1]]), ref, bars,
             WIDE_EXEMPT if name == "wide" else TINY_EXEMPT, name + " entries")


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ARITHS)
def test_prepare_describe_with_unequal_radii_above_nbr_cap(arith):
    """Two-call form == one-call form, byte for byte, where the lists over the larger radius overflow NBR_CAP for most queries;
    describe_device refuses a radius other than the prepared one."""
    _, _, shot = _gpu()
    from cppf2_amd import _lib
    pts, off, _ = _batch(("voxel",))
    for rn, rs in PAIRS:
        s1, n1 = shot.compute_device(pts, off, rn, rs, arithmetic=arith)
        n2 = shot.prepare_device(pts, off, rn, rs, arithmetic=arith)
        with pytest.raises(_lib.CppfError):
            shot.describe_device(pts, off, n2, rn)
        s2 = shot.describe_device(pts, off, n2, rs)
        assert n1.cpu().numpy().tobytes() == n2.cpu().numpy().tobytes()
        assert s1.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------------------------------
# 7. the rim: d2 == r2 exactly is outside
# ------------------------------------------------------------------------------------------------------------------------
RIM_NAMES = tuple("rim_%s_%d_%s" % (k, a, w) for a in range(3) for k in ("normal", "desc", "value") for w in ("on", "in"))
RIM_DENSE = ("rimdense_700_on", "rimdense_1300_on")             # rebuilt list | rescanned runs
RIM_BATCH = RIM_NAMES + RIM_DENSE + ("prefix300",)
# the second pair: shot_hist filters the list over 2 r by d2 < r2; the third: the normal's sums filter it by d2 < rn2 (shot_cov's
# float64 sums and its ranked short list; shot_pcl_long for the 206 entries of rimdense_200)
RIM_RADII = ((RIM_R, RIM_R), (2 * RIM_R, RIM_R), (RIM_R, 2 * RIM_R))
RIM_BATCHES = (RIM_BATCH, RIM_NAMES + ("prefix300",), RIM_NAMES + ("rimdense_200_on", "prefix300"))


def test_rim_inputs_are_exact_and_decide_the_outcome():
    for name in RIM_NAMES:
        _, kind, axis, where = name.split("_")
        pc = cloud(name)
        k = len(pc) - 3
        d = pc[k + 1].astype(np.float64) - pc[0].astype(np.float64)
        d2 = np.float32((d ** 2).sum())
        assert np.array_equal(pc[:k + 1].astype(np.float64) / G, np.round(pc[:k + 1].astype(np.float64) / G))       # on the lattice
        assert (d2 == np.float32(RIM_R * RIM_R)) if where == "on" else (d2 < np.float32(RIM_R * RIM_R) and d2 > np.float32(RIM_R * RIM_R) * 0.999)
        assert coarsening(pc, RIM_R)[2] >= 27                            # several cells
        assert counts(name, RIM_R)[0] == k + 1 + (where == "in")
        for arith in ARITHS:
            ref = oracle(name, RIM_R, RIM_R, arith)
            if kind == "normal":                                         # 2 strict neighbours | 3
                assert np.isnan(ref["normal"][0]).all() == (where == "on")
            if kind == "desc":                                           # 4 valid neighbours | 5
                assert np.isnan(ref["shot"][0]).all() == (where == "on") and not np.isnan(ref["normal"][0]).any()
            if kind == "value":                                          # a descriptor either way: without | with the rim point
                assert not np.isnan(ref["shot"][0]).any()
        if kind == "value" and where == "on":
            other = oracle(name[:-2] + "in", RIM_R, RIM_R, "f64")["shot"][0]
            assert np.abs(oracle(name, RIM_R, RIM_R, "f64")["shot"][0] - other).max() > 1e-2
        # under the wider normal radius the outcome of the frame and the descriptor stays the rim point's
        assert counts(name, 2 * RIM_R).max() == len(pc) - 1 <= PCL_SHORT
        ref = oracle(name, 2 * RIM_R, RIM_R, "f64")
        if kind == "desc":
            assert np.isnan(ref["shot"][0]).all() == (where == "on") and not np.isnan(ref["normal"][0]).any()
        for arith in ARITHS:
            ref = oracle(name, RIM_R, 2 * RIM_R, arith)
            if kind == "normal":
                assert np.isnan(ref["normal"][0]).all() == (where == "on")
    c = counts("rimdense_200_on", 2 * RIM_R)[0]
    assert counts("rimdense_200_on", RIM_R)[0] == 200 and PCL_SHORT < c == 206 <= COV_LIST
    dn = np.abs(oracle("rimdense_200_on", RIM_R, 2 * RIM_R, "pcl")["normal"][0] - oracle("rimdense_200_in", RIM_R, 2 * RIM_R, "pcl")["normal"][0])
    assert dn.max() > 10 * BARS["pcl"]["n"], float(dn.max())           # six more points in the normal's sums would show
    for name in RIM_DENSE:
        n = int(name.split("_")[1])
        pc = cloud(name)
        assert np.array_equal(pc[:n + 6].astype(np.float64) / G, np.round(pc[:n + 6].astype(np.float64) / G))
        d = pc[n:n + 6].astype(np.float64) - pc[0].astype(np.float64)
        assert np.all((d ** 2).sum(1).astype(np.float32) == np.float32(RIM_R * RIM_R))
        assert counts(name, RIM_R)[0] == n and counts(name[:-2] + "in", RIM_R)[0] == n + 6
        assert (NBR_CAP < n <= SH_LCAP) if n == 700 else n > SH_LCAP
        ref = oracle(name, RIM_R, RIM_R, "f64")
        d0 = ref["diag"][0]
        assert min(d0[0] - d0[1], d0[1] - d0[2]) / d0[0] > 0.01          # the query's frame is well defined
        other = oracle(name[:-2] + "in", RIM_R, RIM_R, "f64")["shot"][0]
        assert np.abs(ref["shot"][0] - other).max() > 1e-3               # six more neighbours would show


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ARITHS)
def test_rim_point_is_outside_in_every_pass(arith):
    """Points on the 2^-9 lattice around (0, 0, 0.75), r = 2^-6: a point at exactly 8 steps along x, y or z has d2 == r2 in
    float32 without rounding and is no neighbour -- not for the normal (NaN with 2 strict neighbours, finite once the point moves
    one float32 step inwards), not for the frame (NaN with 4 valid neighbours), not for the lists and the histogram (a query
    with 5 inside points and the rim point: the oracle's descriptor without it; this row is compared WITHOUT the oracle's rim
    exemption, whose reason -- a rounded d2 on either side -- does not exist on the lattice).  The same with 700 and 1300
    lattice points inside and six on the rim (the histogram kernel's rebuilt list and its rescan of the runs), and with a
    normal radius of 2 r (its filtered copy of the longer list), and with a descriptor radius of 2 r (the rim of the NORMAL's
    support inside a longer list: 2 strict neighbours again, and shot_pcl_long's 200 of 206).  A far point gives every scene a grid of several cells; an
    ordinary scene shares the batch."""
    for (rn, rs), names in zip(RIM_RADII, RIM_BATCHES):
        for name, g in zip(names, _compute(names, rn, rs, arith)):
            ref, held = reference(name, rn, rs, arith)
            for key in ("shot", "normal", "rf"):
                assert np.array_equal(np.isnan(g[key]), np.isnan(ref[key])), (name, rn, key)
            if "value" in name or "dense" in name:
                err = float(np.abs(g["shot"][0] - ref["shot"][0]).max())
                nerr = float(np.abs(g["normal"][0] - ref["normal"][0]).max())
                print("rim %s (%g, %g) [%s]: query row err %.3g, normal %.3g" % (name, rn, rs, arith, err, nerr))
                assert err < BARS[held]["d"], (name, rn, err)
                assert nerr < ref.get("nbar", np.full(len(g["normal"]), BARS[held]["n"]))[0], (name, rn, nerr)
                assert np.abs(g["rf"][0] - ref["rf"][0]).max() < BARS[held]["rf"]
