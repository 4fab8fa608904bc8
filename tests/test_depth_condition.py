"""CPU checks of depth conditioning: the NumPy restatement of cppf_depth_condition
(tests/depth_condition_ref.py) on constructed images that sit on the definition's edges, the entry point's refusals (which touch
no device), the settings record and eval.py's flag rules, and the caps of the analytic scene on the restatement."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import depth_condition_ref as R  # noqa: E402
from cppf2_amd import depthfilter as DF  # noqa: E402  (fails without the feature)

F = np.float32
Q = 2.0 ** -10                           # the lattice of the constructed readings
JUMP = 2.0 ** -7                         # 8 lattice steps


def up(x):
    return np.nextafter(F(x), F(np.inf), dtype=F)


def cond(img, **kw):
    kw.setdefault("jump", JUMP)
    out, counts, _ = R.condition(np.asarray(img, F), **kw)
    return out[0], counts[0].tolist()


def test_a_neighbour_exactly_tol_away_supports_and_one_float_farther_does_not():
    img = np.full((3, 3), 0.5, F)
    img[0, 2] = F(0.5 + JUMP)
    out, counts = cond(img, min_support=8)
    assert out[1, 1] == F(0.5) and counts == [9, 0, 0]
    img[0, 2] = up(0.5 + JUMP)
    out, counts = cond(img, min_support=8)
    assert out[1, 1] == 0 and counts[:2] == [9, 4]       # the centre and the far pixel's three other neighbours have 7 left
    assert cond(img, min_support=7)[0][1, 1] == F(0.5)
    # the gate is the CENTRE's: with jump_rel = 2^-6 the far pixel's own tol is wider than the centre's
    img[0, 2] = F(0.5 + 2.0 ** -6)
    out, _ = cond(img, min_support=8, jump_rel=2.0 ** -6)                 # tol(0.5) = 2^-7 + 2^-6 * 0.5 = 2^-6
    assert out[1, 1] == F(0.5)
    img[0, 2] = up(0.5 + 2.0 ** -6)
    out, _ = cond(img, min_support=8, jump_rel=2.0 ** -6)
    assert out[1, 1] == 0 and out[0, 2] == img[0, 2]                     # tol(0.515..) > 2^-6: the far pixel keeps its 8


def test_min_support_at_its_four_values():
    img = R.lattice_images(1, 1, 9, 11, holes=0.0)[0]
    valid = R.valid(img)
    for r1 in (1, 2):
        full = (2 * r1 + 1) ** 2
        kept = [cond(img, r1=r1, min_support=ms)[0] > 0 for ms in (0, 4, full - 1, full)]
        assert (kept[0] == valid).all()                                  # 0: stage 1 removes nothing
        assert not kept[3].any()                                         # (2 r1 + 1)^2: there are only that many minus one offsets
        assert (kept[1] >= kept[2]).all() and kept[1].sum() > kept[2].sum() > 0
    flat = np.full((5, 6), 0.75, F)
    assert (cond(flat, min_support=8)[0] == flat).all()                  # positions outside the image support the border
    assert not cond(flat, min_support=9)[0].any()
    assert not cond(flat, r1=0, min_support=1)[0].any() and (cond(flat, r1=0, min_support=0)[0] == flat).all()


def test_a_pair_of_which_one_partner_fails_adds_neither():
    row = np.array([[0.5 + Q, 0.5, 0.7]], F)
    out, counts = cond(row, r1=0, min_support=0, r2=1)
    assert out[0, 1] == F(0.5) and counts == [3, 0, 0]
    row[0, 2] = F(0.5 + 3 * Q)
    out, counts = cond(row, r1=0, min_support=0, r2=1)
    want = F(F(F(0.5) + F(0.5 + Q)) + F(0.5 + 3 * Q)) / F(3)             # s = (s + a) + b with a the LEFT neighbour
    assert out[0, 1] == want and counts == [3, 0, 1]
    assert out[0, 0] == row[0, 0] and out[0, 2] == row[0, 2]             # their partners lie outside the image
    row[0, 0] = 0
    assert cond(row, r1=0, min_support=0, r2=1)[0][0, 1] == F(0.5)       # an invalid partner


def test_a_corner_pixel_and_a_one_pixel_image():
    one = np.array([[0.625]], F)
    for kw in (dict(), dict(min_support=8), dict(r1=4, min_support=80, r2=4), dict(r1=0, min_support=0, r2=2)):
        out, counts = cond(one, **kw)
        assert out.tolist() == [[0.625]] and counts == [1, 0, 0], kw
    assert cond(one, min_support=9)[0][0, 0] == 0
    img = np.full((2, 2), 0.5, F)
    assert (cond(img, min_support=8)[0] == img).all()                    # 3 neighbours and 5 positions outside
    img[1, 1] = 0.75
    out, counts = cond(img, min_support=6)
    assert out.tolist() == [[0.5, 0.5], [0.5, 0.0]] and counts == [4, 1, 0]      # the corner has the 5 outside only
    out, _ = cond(np.full((2, 2), 0.5, F), r2=1)
    assert (out == F(0.5)).all()                                         # every partner of a corner's neighbour is outside


def test_special_values_leave_as_zero_and_a_denormal_is_valid():
    img = np.array([[np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e-40, 0.5]], F)
    out, counts = cond(img, r1=0, min_support=0)
    assert out.view(np.uint32).tolist() == [[0, 0, 0, 0, 0, 0, int(F(1e-40).view(np.uint32)), int(F(0.5).view(np.uint32))]]
    assert counts == [2, 0, 0]
    out, counts = cond(img, r1=1, min_support=8, r2=1)                   # the two are too far apart to support each other
    assert not out.any() and counts == [2, 2, 0]
    out, counts = cond(img, r1=1, min_support=7, r2=1)                   # the last pixel has 7 positions outside the image ...
    assert out[0, 7] == F(0.5) and not out[0, :7].any() and counts == [2, 1, 0]
    out, counts = cond(img, r1=1, min_support=6, r2=1)                   # ... the denormal has 6
    assert out[0, 7] == F(0.5) and out[0, 6] == F(1e-40) and counts == [2, 0, 0]
    # a special value is never a partner
    row = np.array([[0.5, 0.5, np.nan, 0.5, 0.5]], F)
    out, counts = cond(row, r1=0, min_support=0, r2=2)
    assert out.tolist() == [[0.5, 0.5, 0.0, 0.5, 0.5]] and counts == [4, 0, 0]


def test_the_counts_sum_as_defined():
    img = R.lattice_images(2, 3, 21, 34, dead=1)
    for kw in (dict(), dict(r1=2, min_support=12, r2=1), dict(r1=0, min_support=0, r2=3, jump_rel=2.0 ** -6)):
        out, counts, d1 = R.condition(img, jump=JUMP, **kw)
        valid = R.valid(img)
        assert counts[:, 0].tolist() == valid.sum((1, 2)).tolist() and counts[1].tolist() == [0, 0, 0]
        assert counts[:, 1].tolist() == (valid & (d1 == 0)).sum((1, 2)).tolist()
        assert ((out > 0) == (d1 > 0)).all() and (counts[:, 0] - counts[:, 1]).tolist() == (out > 0).sum((1, 2)).tolist()
        assert (counts[:, 2] <= counts[:, 0] - counts[:, 1]).all() and (kw.get("r2", 0) == 0) == (counts[:, 2].sum() == 0)
        assert (d1[d1 > 0] == img[d1 > 0]).all() and not out[~valid].any()


def test_stage_two_runs_on_stage_ones_output():
    """Columns 0-2 at L, column 3 a mixed reading m within the gate of L but not of R, columns 4-6 at R.  With min_support = 6
    stage 1 removes column 3 (5 neighbours within its gate); a pixel of column 2 keeps its reading, and its mean must not take
    the pair that holds m, which is within ITS gate."""
    L, m, Rr = F(0.5), F(0.5 + 8 * Q), F(0.5 + 20 * Q)
    img = np.repeat(np.array([[L, L, L, m, Rr, Rr, Rr]], F), 5, 0)
    assert abs(m - L) <= F(JUMP) < abs(Rr - m)
    out, counts, d1 = R.condition(img, r1=1, min_support=6, r2=1, jump=JUMP)
    assert not d1[0, 1:4, 3].any() and (d1[0, :, 2] == L).all()
    assert out[0, 2, 2] == L                                             # (L + L + L) / 3: the vertical pair only
    raw_mean, _, _ = R.condition(img, r1=0, min_support=0, r2=1, jump=JUMP)
    assert raw_mean[0, 2, 2] > L                                         # what smoothing the raw input would have given
    assert out[0, 2, 1] == L and counts[0, 2] > 0


def test_the_restatement_refuses_what_the_kernel_refuses():
    for kw in (dict(r1=5), dict(r2=5), dict(r1=-1), dict(min_support=10), dict(min_support=-1), dict(r1=0, min_support=2)):
        with pytest.raises(AssertionError):
            R.condition(np.ones((2, 2), F), **kw)


def test_the_entry_point_validates_before_any_device_work():
    from cppf2_amd import _lib
    L = _lib.load()
    one, two = C.c_void_p(1 << 20), C.c_void_p(1 << 24)                   # non-null pointers the refused calls never follow
    base = dict(depth=one, I=2, H=16, W=16, r1=1, ms=4, r2=0, jump=0.01, rel=0.0, out=two, counts=C.c_void_p(1 << 28))

    def call(**kw):
        a = dict(base, **kw)
        return L.cppf_depth_condition(a["depth"], a["I"], a["H"], a["W"], a["r1"], a["ms"], a["r2"], C.c_float(a["jump"]),
                                      C.c_float(a["rel"]), a["out"], a["counts"], None)
    nan, inf = float("nan"), float("inf")
    cases = [dict(depth=None), dict(out=None), dict(counts=None), dict(I=-1), dict(H=0), dict(W=0), dict(H=16385), dict(W=16385),
             dict(r1=-1), dict(r1=5), dict(r2=-1), dict(r2=5), dict(ms=-1), dict(ms=10), dict(r1=0, ms=2), dict(r1=2, ms=26),
             dict(jump=-0.001), dict(jump=nan), dict(jump=inf), dict(rel=-0.1), dict(rel=nan), dict(rel=inf),
             dict(out=one),                                               # in place: stage 1 reads neighbours
             dict(out=C.c_void_p((1 << 20) + 4)), dict(out=C.c_void_p((1 << 20) + 2 * 16 * 16 * 4 - 4)),
             dict(out=C.c_void_p((1 << 20) - 2 * 16 * 16 * 4 + 4))]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert b"cppf_depth_condition: invalid argument" in L.cppf_last_error_string()
    # no images: a valid call that does nothing and needs none of the arrays; the sizes are still checked
    assert call(I=0, depth=None, out=None, counts=None) == 0
    assert call(I=0, H=0) == -1 and call(I=0, r1=5) == -1
    # adjacent buffers do not overlap
    assert call(I=0, out=C.c_void_p((1 << 20) + 2 * 16 * 16 * 4)) == 0


def test_the_settings_record_is_built_in_one_place():
    assert DF.Settings._fields == ("flying_radius", "min_support", "smooth_radius", "jump", "jump_rel")
    from cppf2_amd import masks
    assert DF.checked() == DF.Settings(1, 4, 0, masks.JUMP, 0.0) == DF.from_flags(True, {})
    assert DF.from_flags(False, {}) is None and DF.from_flags(False, dict(flying_radius=None)) is None
    s = DF.from_flags(True, dict(flying_radius=2, flying_support="12", smooth_radius=2.0, depth_jump=0.006, depth_jump_rel="0.01"))
    assert s == DF.Settings(2, 12, 2, 0.006, 0.01) and [type(x) for x in s] == [int, int, int, float, float]
    assert DF.from_flags(True, dict(flying_radius=0)) == DF.Settings(0, 0, 0, masks.JUMP, 0.0)       # stage 1 off
    with pytest.raises(ValueError, match="--smooth_radius sets how the depth image is conditioned: it needs --condition_depth"):
        DF.from_flags(False, dict(smooth_radius=2))
    with pytest.raises(ValueError, match="--depth-jump .* it needs --condition-depth"):
        DF.from_flags(False, dict(depth_jump=0.0), lambda n: "--" + n.replace("_", "-"))
    for bad in (dict(flying_radius=5), dict(flying_radius=-1), dict(smooth_radius=5), dict(flying_radius=1.5), dict(flying_support=10),
                dict(flying_support=-1), dict(flying_radius=0, flying_support=2), dict(depth_jump=-1.0), dict(depth_jump=float("nan")),
                dict(depth_jump_rel=float("inf")), dict(smooth_radius="two")):
        with pytest.raises(ValueError):
            DF.from_flags(True, bad)
    assert DF.summary(s, [[5, 2, 1], [7, 0, 3]]) == dict(flying_radius=2, min_support=12, smooth_radius=2, jump=0.006, jump_rel=0.01,
                                                          valid=12, removed=2, smoothed=4)
    assert DF.merged([DF.summary(s, [[5, 2, 1]]), DF.summary(s, [[7, 0, 3]])]) == DF.summary(s, [[5, 2, 1], [7, 0, 3]])
    assert DF.apply("as it is", None) == ("as it is", None)
    with pytest.raises(ValueError, match="Settings"):
        DF.apply(np.ones((2, 2), F), (1, 4, 0, 0.01, 0.0))


def test_there_is_no_cpu_fallback():
    import torch
    with pytest.raises(DF.CppfError):
        DF.condition(torch.ones((4, 4)))
    with pytest.raises(ValueError):
        DF.condition(torch.ones((4, 4)), flying_radius=7)
    from cppf2_amd import fuse, track
    for fn in (fuse.fuse_views, fuse.fuse_scene, track.onboard, track.join, track.onboard_scene, track.join_scene):
        assert inspect.signature(fn).parameters["condition"].default is None, fn


def test_eval_flags(monkeypatch):
    monkeypatch.chdir(ROOT)
    import eval as ev
    base = {k: p.default for k, p in inspect.signature(ev.main).parameters.items()}
    assert ev._checked_flags(**base).condition is None
    depth = dict(base, data="depth", mask="m.png")
    assert ev._checked_flags(**depth).condition is None
    assert ev._checked_flags(**dict(depth, condition_depth=True)).condition == DF.checked()
    f = ev._checked_flags(**dict(base, data="bop", bop_root="x", out_csv="y.csv", condition_depth=True, flying_radius=2, flying_support=10,
                                 smooth_radius=1, depth_jump=0.006, depth_jump_rel=0.002))
    assert f.condition == DF.Settings(2, 10, 1, 0.006, 0.002)
    for flag in DF.FLAGS:
        with pytest.raises(ValueError, match="--%s sets how the depth image is conditioned: it needs --condition_depth" % flag):
            ev._checked_flags(**dict(depth, **{flag: 1}))
    for data in ("synthetic", "nocs"):
        with pytest.raises(ValueError, match="--condition_depth .* it needs --data=depth or --data=bop"):
            ev._checked_flags(**dict(base, data=data, condition_depth=True))
    with pytest.raises(ValueError):
        ev._checked_flags(**dict(depth, condition_depth=True, flying_radius=9))
    assert ev.DepthRun(*range(9)).conditioned is None


@pytest.mark.parametrize("extra", [["--flying-radius", "2"], ["--smooth-radius", "1"], ["--depth-jump", "0.01"],
                                   ["--condition-depth", "--flying-radius", "5"], ["--condition-depth", "--flying-support", "10"],
                                   ["--condition-depth", "--depth-jump", "-1"]])
def test_command_line_refuses_bad_conditioning_arguments(extra, tmp_path, capsys):
    from cppf2_amd import fuse
    with pytest.raises(SystemExit):
        fuse.main(["--views", str(tmp_path), "--voxel", "0.004", "--out", str(tmp_path / "o.ply")] + extra)
    assert "condition" in capsys.readouterr().err
    with pytest.raises(fuse.ViewsError):                    # and valid arguments reach the folder
        fuse.main(["--views", str(tmp_path), "--voxel", "0.004", "--out", str(tmp_path / "o.ply"), "--condition-depth", "--smooth-radius", "2"])


@pytest.mark.parametrize("sigma", [0.001, 0.002])
def test_the_scene_on_the_restatement(sigma):
    """The caps of DESIGN.md section 33 at 1 mm and at 2 mm of noise.  Measured with this restatement: flying removed 0.983 /
    0.983; clean removed 0.00003 / 0.0057; clean object pixels removed 0.0009 / 0.0040; masked points off the sphere 0.0153 /
    0.0158 raw and none after; RMS on the clean pixels kept 1.54 -> 0.33 mm / 2.98 -> 0.97 mm, on the object's 0.75 -> 0.43 mm /
    1.50 -> 0.53 mm."""
    sc = R.scene(sigma)
    assert sc["depth"].shape == (240, 320) and 150 < sc["flying"].sum() < 200 and 2000 < sc["mask"].sum() < 2600
    fig = R.scene_figures(sc, R.condition(sc["depth"])[0][0], R.condition(sc["depth"], r2=2)[0][0])
    print("scene sigma=%g: %s" % (sigma, fig))
    R.check_scene(fig)
