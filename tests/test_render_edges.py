"""CPU checks of the rasterizer's edge inputs (tests/render_edge_cases.py): the NumPy mirror of cppf_render_depth
(tests/render_ref.py) against the reference that shares none of its code (tests/render_exact.py), on every input that
tests/test_render_edges_gpu.py sends to the device -- counts, ids, rejections and the tile-list need exactly, depth within 1e-6
(all terms of the 1/z sum are positive, so nothing cancels: ten float32 roundings give 6e-7) -- and the floors and caps that make
those inputs worth sending: sample points on edges, lists longer than one LDS pass, scan chunks of two, pixels cut by zfar."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_edge_cases as EC  # noqa: E402

DEPTH_TOL = 1e-6


def _assert_mirror_is_exact(name):
    c, m, x = EC.case(name), EC.mirror(name), EC.exact(name)
    assert m.snapped, "render_ref.setup does not snap the constructed vertices to the constructed integers"
    assert np.array_equal(m.count, x.count)
    assert np.array_equal(m.tri_id, x.tri_id)
    assert m.rejected == x.rejected and m.need == x.need
    err, near = EC.depth_error(m.depth, name)
    print("%s: mirror against exact: worst relative depth error %.3g, %d pixels at a depth limit" % (name, err, near))
    assert err <= DEPTH_TOL
    return c, m, x, near


# ---- a. lattice triangulations -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.LATTICE)
def test_lattice_covers_each_pixel_of_the_hull_once(name):
    c, m, x, near = _assert_mirror_is_exact(name)
    assert near == 0 and x.rejected == 0
    T = len(c.tris)
    inside, outside = EC.hull_sides(c.hull, c.H, c.W)
    assert inside.sum() > 1500 and outside.sum() >= 10
    count = x.count.sum(0)                    # one view: itself; split: the sum over the single-triangle views
    assert (count[inside] == 1).all() and (count[outside] == 0).all() and count.max() <= 1
    if name.endswith("-split"):
        assert len(c.tri_off) == T + 1 and T * 12 > 1024          # every thread of the scan owns a chunk of two tiles
        assert np.array_equal((m.depth > 0).sum(0), count)
    else:
        assert np.array_equal(x.tri_id[0] >= 0, count == 1)
        cover = x.views[0]["cover"]
        assert np.array_equal(np.where(count == 1, cover.argmax(0), -1), x.tri_id[0])
        a, b, d = c.tris.T
        back = (c.su[b] - c.su[a]) * (c.sv[d] - c.sv[a]) - (c.sv[b] - c.sv[a]) * (c.su[d] - c.su[a]) > 0
        assert not back.any() if c.cull else 0.25 < back.mean() < 0.75          # half the windings flipped without culling


@pytest.mark.parametrize("seed", range(4))
def test_lattice_puts_sample_points_on_edges(seed):
    """Floor: at least 60 pixels per seed whose sample point lies on an edge or a vertex (measured: 110, 136, 117, 93), a third
    of the points on pixel centres and a third on pixel corners, coordinates reaching 2 px past every border."""
    su, sv, tris, _ = EC.lattice_mesh(seed, 40, 56, 60, 128)
    on = EC.on_edge_pixels(su, sv, tris, 40, 56)
    print("seed %d: %d points, %d triangles, %d pixels with their sample point on an edge or vertex" % (seed, len(su), len(tris), on.sum()))
    assert on.sum() >= 60
    assert ((su % 256 == 128) & (sv % 256 == 128)).sum() >= 15 and ((su % 256 == 0) & (sv % 256 == 0)).sum() >= 15
    assert su.min() == -512 and sv.min() == -512 and su.max() == 256 * 58 and sv.max() == 256 * 42
    # and those pixels are covered exactly once inside the hull, like all others
    x = EC.exact("lattice-s%d-flat-cull0" % seed)
    inside, _ = EC.hull_sides(EC.case("lattice-s%d-flat-cull0" % seed).hull, 40, 56)
    assert (on & inside).sum() >= 50 and (x.count[0][on & inside] == 1).all()


# ---- b. long lists and ties ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.STACK)
def test_stack_winner(name):
    c, m, x, near = _assert_mirror_is_exact(name)
    r, col = np.mgrid[0:16, 0:16]
    covered = r + col < 15                               # corners on pixel centres: the hypotenuse is a bottom-right edge
    assert covered.sum() == 120 and near == 0
    assert np.array_equal(x.count[0], covered * c.T) and x.need == c.T
    want = {"same": 0, "last": c.T - 1, "pair": min(EC.stack_pair(c.T))}[c.mode]
    assert (x.tri_id[0][covered] == want).all() and (x.tri_id[0][~covered] == -1).all()
    assert (x.depth[0][covered] == 1.0).all() and (m.depth[0][covered] == 1.0).all()
    if c.mode == "pair" and c.T > 256:
        a, b = EC.stack_pair(c.T)
        assert a >= 256 > b                              # whatever the list order, the two do not share every LDS pass


# ---- c. depth range ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.RANGE)
def test_depth_range_cuts_pixels(name):
    c, m, x, near = _assert_mirror_is_exact(name)
    covered = x.count[0] > 0
    assert covered.all() and near <= EC.RANGE_CAP * covered.sum()
    tilted, flat = x.views[0]["z"]
    if c.variant == "literal":
        assert x.rejected == 1 and (x.count[0] == 1).all() and not x.depth.any()
        return
    assert x.rejected == 0 and (x.count[0] == 2).all()
    cut = tilted > c.zfar
    assert cut.sum() >= 20 and (~cut).sum() >= 500 and (tilted[~cut] >= c.znear).all()
    assert np.allclose(flat, 3.0, rtol=1e-12)
    if c.zfar < 3.0:                                     # the flat triangle is cut everywhere: beyond the limit nothing is drawn
        assert np.array_equal(x.tri_id[0], np.where(cut, -1, 0))
    else:                                                # the flat one shows where the tilted one is behind it or cut
        assert np.array_equal(x.tri_id[0], np.where(tilted > 3.0, 1, 0)) and (x.tri_id[0][cut] == 1).all()


# ---- d, e. rejections, tri_off, silent non-draws ----------------------------------------------------------------------
def _assert_same_as_base(c, got_depth, got_id, base_depth, base_id):
    """Views 0 and 1 of a disturbed batch against the base batch: depth bytes equal, ids equal after renumbering view 0."""
    assert np.array_equal(got_depth[:2].view(np.uint32), base_depth.view(np.uint32))
    assert np.array_equal(got_id[1], base_id[1])
    assert np.array_equal(got_id[0], np.where(base_id[0] >= 0, c.kept[np.maximum(base_id[0], 0)], -1))


@pytest.mark.parametrize("name", EC.DISTURBED)
def test_rejected_and_silent_triangles_leave_the_rest_alone(name):
    c, m, x, near = _assert_mirror_is_exact(name)
    base, bx = EC.mirror("base"), EC.exact("base")
    assert x.rejected == EC.REJECTS.get(name, 0) and near == 0
    _assert_same_as_base(c, m.depth, m.tri_id, base.depth, base.tri_id)
    _assert_same_as_base(c, x.depth.astype(np.float32), x.tri_id, bx.depth.astype(np.float32), bx.tri_id)
    if name == "rej-inside-guard":                       # the triangle 1/4 px inside the guard band fills its own view
        assert (x.count[2] == 1).all() and x.need == bx.need + 12 and max(abs(c.su).max(), abs(c.sv).max()) == EC.BIG
        assert np.float32(EC.BIG) == EC.BIG and np.nextafter(np.float32(EC.BIG), np.float32(np.inf)) == 2.0 ** 30
    else:
        assert x.need == bx.need
    if name == "silent":
        assert c.added == 11 and not x.count[2].any() and not m.depth[2].any() and (m.tri_id[2] == -1).all()


def test_base_batch():
    c, m, x, near = _assert_mirror_is_exact("base")
    assert near == 0 and x.rejected == 0 and (x.depth > 0).sum() > 3000


@pytest.mark.parametrize("name", EC.OFFSETS)
def test_tri_off_variants(name):
    c, m, x, near = _assert_mirror_is_exact(name)
    bx = EC.exact("base")
    assert x.rejected == c.want_rejected
    for b in range(len(c.tri_off) - 1):
        if c.shown.get(b, 0) is None:                    # a view that lost some of its triangles: held to the exact render above
            assert (x.depth[b] > 0).sum() < (bx.depth[1] > 0).sum()
        elif b in c.shown:
            assert np.array_equal(x.depth[b], bx.depth[c.shown[b]]) and np.array_equal(x.tri_id[b], bx.tri_id[c.shown[b]])
        else:
            assert not x.depth[b].any() and (x.tri_id[b] == -1).all()
    if None not in c.shown.values():
        assert x.need == sum(bx.views[v]["need"] for v in c.shown.values())


# ---- f. shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.SHAPES) + list(EC.STRIPS))
def test_shapes(name):
    c, m, x, near = _assert_mirror_is_exact(name)
    assert near == 0 and x.rejected == 0
    if name in EC.STRIPS:
        assert (x.count == 1).all() and (x.depth > 0).all() and x.depth.size == 8192 and x.need == 2 * 512
        assert len(np.unique(x.tri_id)) == 2
    else:
        inside, outside = EC.hull_sides(c.hull, c.H, c.W)
        assert (x.count[0][inside] == 1).all() and (x.count[0][outside] == 0).all() and inside.sum() >= min(c.H * c.W, 100)


# ---- a depth float32 cannot hold -----------------------------------------------------------------------------------------
def test_infinite_depth_is_not_drawn():
    """Finite input that reaches z = +inf: a triangle at the largest float32 depth has a subnormal 1/z, and area / w rounds
    past the largest float on all of its 120 pixels.  zfar = +inf admits that z, but depth 0 / id -1 are the header's "nothing
    drawn" and +inf is no depth: the pixel stays empty (the kernel's running minimum starts at +inf, so it never did draw it;
    the mirror used to)."""
    c, m = EC.case("huge"), EC.mirror("huge")
    assert m.snapped and m.rejected == 0 and m.need == 1 and m.count.sum() == 120
    f32 = np.float32
    with np.errstate(over="ignore"):
        assert np.isinf(f32(3840 * 3840) / (f32(3840 * 3840) * (f32(1) / f32(c.z[0]))))        # the vertex pixel's z
    assert not m.depth.any() and (m.tri_id == -1).all()
    x = EC.exact("huge")                                                                                # float64 holds that depth
    assert np.array_equal(x.count, m.count) and np.allclose(x.depth[x.count > 0], c.z[0], rtol=1e-12)
