"""GPU checks of cppf_render_depth at its edges, on the inputs of tests/render_edge_cases.py (tests/test_render_edges.py checks
those inputs, their floors and their caps on the CPU): the device against the NumPy mirror bit for bit (depth, tri_id, both
status words) and against tests/render_exact.py, which shares no code with either (coverage and ids exactly, depth within 1e-6)
-- sample points on edges and vertices, lists longer than one 256-record LDS pass with ties across the passes, pixels cut by
the depth range, every reject path of the setup kernel, triangles that are silently not drawn, malformed and empty tri_off
ranges, 1x1 to 8192-long images, tri_id == NULL.  Every call goes through the C entry point (render.render_depth raises on a
rejection) with canary words behind depth, tri_id and status, and is issued twice: the bytes must not depend on the order in
which the scatter's atomics fill the tile lists."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_edge_cases as EC  # noqa: E402
import render_exact as RX  # noqa: E402

DEPTH_TOL = 1e-6
MARGIN = 64                       # canary words behind each output


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


def raw(c, dev, with_ids=True, capacity=None):
    """One cppf_render_depth call on case c: (depth float32 [B,H,W], tri_id int32 [B,H,W] or None, status int64 [2]) as NumPy.
    The list capacity defaults to exactly the need the exact reference computes."""
    import torch
    from cppf2_amd import _lib, ops
    L = _lib.load()
    B, T, n = len(c.tri_off) - 1, len(c.tris), (len(c.tri_off) - 1) * c.H * c.W
    cap = EC.exact(c.name).need if capacity is None else capacity
    verts = torch.as_tensor(c.verts).to(dev) if len(c.verts) else None
    tris = torch.as_tensor(c.tris).to(dev) if T else None
    tri_off = torch.as_tensor(c.tri_off).to(dev)
    poses = torch.as_tensor(np.tile(RX.POSE, (B, 1))).to(dev)
    nb = L.cppf_render_depth_workspace_bytes(B, T, c.H, c.W, cap)
    assert nb > 0
    ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
    depth = torch.full((n + MARGIN,), -7.5, dtype=torch.float32, device=dev)
    ids = torch.full((n + MARGIN,), 0x5a5a5a5a, dtype=torch.int32, device=dev) if with_ids else None
    st = torch.full((2 + MARGIN,), 0x1234567, dtype=torch.int64, device=dev)
    hK = (C.c_double * 4)(RX.FX, RX.FX, 0.0, 0.0)
    _lib.check(L.cppf_render_depth(B, ops._p(verts), len(c.verts), ops._p(tris), ops._p(tri_off), T, ops._p(poses), hK, c.H, c.W,
                                   C.c_float(c.znear), C.c_float(c.zfar), int(c.cull), ops._p(depth), ops._p(ids), ops._p(st),
                                   ops._p(ws), nb, cap, ops._stream()), "cppf_render_depth")
    d, s = depth.cpu().numpy(), st.cpu().numpy()
    assert (d[n:] == np.float32(-7.5)).all() and (s[2:] == 0x1234567).all(), "written past the end of an output"
    t = None
    if with_ids:
        t = ids.cpu().numpy()
        assert (t[n:] == 0x5a5a5a5a).all(), "written past the end of tri_id"
        t = t[:n].reshape(B, c.H, c.W)
    return d[:n].reshape(B, c.H, c.W), t, s[:2]


def _check(name, dev):
    """The device on one case, twice: against the mirror bit for bit, against the exact reference, status words exactly."""
    c, m, x = EC.case(name), EC.mirror(name), EC.exact(name)
    assert m.snapped
    d, t, st = raw(c, dev)
    d2, t2, st2 = raw(c, dev)
    assert np.array_equal(d.view(np.uint32), d2.view(np.uint32)) and np.array_equal(t, t2) and np.array_equal(st, st2)
    assert int(st[0]) == m.rejected == x.rejected
    assert int(st[1]) == m.need == x.need
    assert np.array_equal(d.view(np.uint32), m.depth.view(np.uint32)), int((d != m.depth).sum())
    assert np.array_equal(t, m.tri_id)
    assert np.array_equal(t, x.tri_id)
    err, near = EC.depth_error(d, name)
    print("%s: device against exact: worst relative depth error %.3g (%d pixels at a depth limit left out)" % (name, err, near))
    assert err <= DEPTH_TOL
    return c, d, t, st


# ---- a. lattice triangulations: the fill rule --------------------------------------------------------------------------
@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("zmode", ["flat", "mixed"])
@pytest.mark.parametrize("seed", range(4))
def test_lattice_is_covered_once(seed, zmode, cull):
    """60 lattice points (a third on pixel centres, a third on corners; 93-136 sample points per seed on an edge or a vertex),
    Delaunay-triangulated, as one view and as T views of one triangle in one call (T * 12 tiles > 1024: scan chunks of two).
    The sum of depth > 0 over the single-triangle views is the device's cover count: 1 strictly inside the hull, 0 outside,
    render_exact's everywhere; the one-view tri_id is the one covering triangle."""
    dev = _gpu()
    name = "lattice-s%d-%s-cull%d" % (seed, zmode, cull)
    c, d, t, _ = _check(name, dev)
    cs, ds, ts, _ = _check(name + "-split", dev)
    x = EC.exact(name)
    count = (ds > 0).sum(0)
    assert np.array_equal(count, x.count[0])
    inside, outside = EC.hull_sides(c.hull, c.H, c.W)
    assert (count[inside] == 1).all() and (count[outside] == 0).all()
    assert np.array_equal(t[0], np.where(count == 1, x.views[0]["cover"].argmax(0), -1))
    assert ((ts == 0) == (ds > 0)).all() and ((ts == -1) == (ds == 0)).all()          # a view's only triangle has id 0
    # the union of the single views is the one view, to the bit (no pixel has two candidates)
    assert np.array_equal(ds.max(0).view(np.uint32), d[0].view(np.uint32))
    on = EC.on_edge_pixels(c.su, c.sv, c.tris, c.H, c.W)
    assert on.sum() >= 60 and (count[on & inside] == 1).all()
    # tri_id == NULL: the same depth bytes
    d0, t0, _ = raw(c, dev, with_ids=False)
    assert t0 is None and np.array_equal(d0.view(np.uint32), d.view(np.uint32))


# ---- b. long lists and ties --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", EC.STACK_LENGTHS)
def test_long_lists_and_ties(T):
    """One tile, T coincident triangles (255 .. 600: one, two and three LDS passes, full and ragged): all at one depth -> id 0;
    the nearest last -> id T - 1; two coincident nearest ones at ids 300 (T - 1 in the short lists) and 10 -> id 10."""
    dev = _gpu()
    r, col = np.mgrid[0:16, 0:16]
    covered = r + col < 15
    for mode, want in (("same", 0), ("last", T - 1), ("pair", 10)):
        c, d, t, st = _check("stack-%d-%s" % (T, mode), dev)
        assert int(st[1]) == T
        assert (t[0][covered] == want).all() and (t[0][~covered] == -1).all()
        assert (d[0][covered] == 1.0).all() and not d[0][~covered].any()


# ---- c. depth range ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.RANGE)
def test_depth_range_cuts_pixels(name):
    """A tilted triangle over a flat one at z = 3 (render_edge_cases._range): pixels whose z lies past zfar show what is behind,
    or nothing where that is cut too.  Against the mirror nothing is left out; against render_exact the pixels within 1e-6 of a
    limit are (at most 2 % of the covered ones; none with these slopes)."""
    dev = _gpu()
    c, d, t, st = _check(name, dev)
    x = EC.exact(name)
    _, near = EC.depth_error(d, name)
    assert near <= EC.RANGE_CAP * (x.count[0] > 0).sum()
    if c.variant == "literal":
        assert int(st[0]) == 1 and not d.any()
        return
    tilted = x.views[0]["z"][0]
    cut = tilted > c.zfar
    assert cut.sum() >= 20
    assert (t[0][cut] == (1 if c.zfar > 3.0 else -1)).all() and (t[0][~cut & (tilted < 3.0)] == 0).all()


# ---- d. rejections, e. silent non-draws ------------------------------------------------------------------------------
def _assert_same_as_base(c, d, t, bd, bt):
    assert np.array_equal(d[:2].view(np.uint32), bd.view(np.uint32))
    assert np.array_equal(t[1], bt[1])
    assert np.array_equal(t[0], np.where(bt[0] >= 0, c.kept[np.maximum(bt[0], 0)], -1))


@pytest.mark.parametrize("name", EC.DISTURBED)
def test_rejected_and_silent_triangles_leave_the_rest_alone(name):
    """Vertex indices -1, INT_MIN, num_verts and INT_MAX; a vertex just below znear; NaN in x, y or z; a coordinate snapped to
    exactly +-2^22 px (the guard is strict); the largest float32 inside the guard (2^30 - 64: drawn, depth checked); and the
    triangles that are dropped without a word (zero area, an empty pixel box between sample points, off screen on each side,
    culled).  status[0] counts exactly the rejected ones, status[1] is the need of the others, and the other triangles of the
    batch render as in the batch without the extra ones."""
    dev = _gpu()
    c, d, t, st = _check(name, dev)
    _, bd, bt, bst = _check("base", dev)
    assert int(st[0]) == EC.REJECTS.get(name, 0)
    _assert_same_as_base(c, d, t, bd, bt)
    if name == "rej-inside-guard":
        assert (t[2] == 0).all() and int(st[1]) == int(bst[1]) + 12
    else:
        assert int(st[1]) == int(bst[1])
    if name == "silent":
        assert not d[2].any() and (t[2] == -1).all()


@pytest.mark.parametrize("name", EC.OFFSETS)
def test_tri_off_variants(name):
    """Empty first, middle and last views; B = 1 with no triangles at all; a decreasing tri_off and one that ends early, both
    within [0, total]: the triangles left without a view are counted as rejected and nothing else changes."""
    dev = _gpu()
    c, d, t, st = _check(name, dev)
    _, bd, bt, _ = _check("base", dev)
    assert int(st[0]) == c.want_rejected
    for b in range(len(c.tri_off) - 1):
        if c.shown.get(b, 0) is None:
            continue
        if b in c.shown:
            assert np.array_equal(d[b].view(np.uint32), bd[c.shown[b]].view(np.uint32)) and np.array_equal(t[b], bt[c.shown[b]])
        else:
            assert not d[b].any() and (t[b] == -1).all()


def test_list_overflow_on_a_ragged_batch_leaves_the_outputs_cleared():
    """One entry short of the need: both status words as before, depth 0 and tri_id -1 everywhere, the canaries untouched."""
    dev = _gpu()
    c, x = EC.case("rej-guard"), EC.exact("rej-guard")
    d, t, st = raw(c, dev, capacity=x.need - 1)
    assert int(st[0]) == x.rejected and int(st[1]) == x.need
    assert not d.any() and (t == -1).all()


# ---- f. shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.SHAPES) + list(EC.STRIPS))
def test_shapes(name):
    """1x1, one tile exactly, H below and W above a tile, and the two longest strips (tile index 511 in either half of the packed
    tile range; two triangles that cover all 8192 pixels)."""
    dev = _gpu()
    c, d, t, st = _check(name, dev)
    assert int(st[0]) == 0
    if name in EC.STRIPS:
        assert (d > 0).all() and d.size == 8192 and int(st[1]) == 1024
    d0, _, _ = raw(c, dev, with_ids=False)
    assert np.array_equal(d0.view(np.uint32), d.view(np.uint32))


# ---- a depth float32 cannot hold -----------------------------------------------------------------------------------------
def test_infinite_depth_is_not_drawn():
    """tests/test_render_edges.py::test_infinite_depth_is_not_drawn on the device: z = +inf under zfar = +inf stays empty."""
    dev = _gpu()
    c, m = EC.case("huge"), EC.mirror("huge")
    d, t, st = raw(c, dev, capacity=1)
    assert int(st[0]) == 0 and int(st[1]) == 1
    assert np.array_equal(d.view(np.uint32), m.depth.view(np.uint32)) and np.array_equal(t, m.tri_id)
    assert not d.any() and (t == -1).all()
