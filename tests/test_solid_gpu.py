"""cppf_support_counts and cppf_solid_overlap against their restatement (tests/solid_ref.py), byte for byte -- the outputs are
integer counts -- at the tile edges of the kernels, in batches, and at the exact boundaries of both thresholds; the two scenes of
tests/solid_scenes.py through explain_candidates, verify.select and eval.py."""
import os
import sys

import numpy as np
import pytest

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import render_ref as RR  # noqa: E402
import solid_ref as SO  # noqa: E402
from test_solid import facing_plane_case, overlap_tau_case  # noqa: E402

F = np.float32
SHAPES = [(1, 1), (1, 64), (33, 4), (37, 53), (3, 1021), (480, 640)]
TAU_S, TAU_X = F(0.01), F(0.02)


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _case(H, W, C, seed, bad=True):
    """C candidates of an H x W image: front faces about 0.9 m, back faces 0 .. 8 cm behind them, each candidate a run of pixels
    in row-major order (shorter when there are many, so that the pairs stay countable) plus a sprinkle; a tenth of the drawn
    pixels open to either side; (bad) 0, NaN, +-inf, a negative value and -0.0 in both renders.  The plane is tilted and passes
    through (0, 0, 1): back faces lie on both sides of it.  Returns (front, back [C,H,W], plane [4], kmat [4])."""
    rng = np.random.default_rng(seed)
    HW = H * W
    f = np.zeros((C, HW), F)
    b = np.zeros((C, HW), F)
    for c in range(C):
        n = int(rng.integers(1, max(2, HW // max(2, C // 2) + 1)))
        a = int(rng.integers(0, HW - n + 1))
        on = np.zeros(HW, bool)
        on[a:a + n] = True
        on |= rng.random(HW) < 0.02
        fz = (0.85 + 0.15 * rng.random(HW)).astype(F)
        bz = fz + (0.08 * rng.random(HW)).astype(F)
        kind = rng.choice(3, HW, p=[0.9, 0.05, 0.05])     # solid, front only, back only
        f[c] = np.where(on & (kind != 2), fz, 0)
        b[c] = np.where(on & (kind != 1), bz, 0)
    if bad and HW >= 16:
        vals = np.array([0.0, np.nan, np.inf, -np.inf, -0.7, -0.0], F)
        for c in range(C):
            for arr in (f, b):
                p = rng.choice(HW, size=max(6, HW // 40), replace=False)
                arr[c, p] = vals[(np.arange(p.size) + c) % 6]
    n = np.array([0.12, -0.55, -0.8])
    n /= np.linalg.norm(n)
    plane = np.concatenate([n, [-n[2]]]).astype(F)
    kmat = np.array([1.3 * W + 20, 1.2 * W + 20, W / 2 - 0.25, H / 2 + 0.125], F)
    return f.reshape(C, H, W), b.reshape(C, H, W), plane, kmat


def _same(got, want, what):
    g = got.cpu().numpy()
    assert g.dtype == want.dtype == np.int64 and g.shape == want.shape, (what, g.dtype, g.shape, want.shape)
    if g.tobytes() != want.tobytes():
        bad = np.flatnonzero(g.reshape(-1) != want.reshape(-1))
        raise AssertionError("%s differs at %d places, first %d: got %s, want %s (shape %s)" % (
            what, bad.size, bad[0], g.reshape(-1)[bad[:8]].tolist(), want.reshape(-1)[bad[:8]].tolist(), g.shape))


def _check(front, back, off, planes, kmat, tau_s=TAU_S, tau_x=TAU_X, overlap=True):
    """Both entry points against the restatement, byte for byte; returns the restatement's (counts, inter)."""
    from cppf2_amd import solid
    want_s = SO.support(front, back, off, planes, kmat, tau_s)
    _same(solid.support_counts(front, back, off, planes, kmat, tau_s), want_s, "counts")
    want_x = None
    if overlap:
        want_x = SO.overlap(front, back, off, tau_x)
        _same(solid.overlap_counts(front, back, off, tau_x), want_x, "inter")
        for i in range(len(off) - 1):                     # symmetric, the diagonal the solid count, nothing past C_i
            sq = want_x[off[i]:off[i + 1]]
            n = off[i + 1] - off[i]
            assert np.array_equal(sq[:, :n], sq[:, :n].T) and not sq[:, n:].any()
            assert np.array_equal(np.diagonal(sq[:, :n]), want_s[off[i]:off[i + 1], 2])
    return want_s, want_x


@pytest.mark.parametrize("C", [1, 2, 63, 64])
@pytest.mark.parametrize("shape", SHAPES[:5], ids=["%dx%d" % s for s in SHAPES[:5]])
@gpu
def test_equals_the_restatement(shape, C):
    _gpu()
    H, W = shape
    f, b, plane, kmat = _case(H, W, C, 13 * H + C)
    want_s, want_x = _check(f, b, [0, C], plane, kmat)
    if shape == (37, 53) and C >= 63:
        assert (want_s[:, 1] > 0).sum() > 20 and (want_s[:, 1] < want_s[:, 0]).sum() > 20, "no longer on both sides of the plane"
        off_diag = want_x[:, :C][~np.eye(C, dtype=bool)]
        assert (off_diag > 0).sum() > 200 and (want_s[:, 3] > 0).all(), "no longer overlapping, or no open pixels"


@pytest.fixture(scope="module")
def vga():
    return _case(480, 640, 64, 3)


@gpu
def test_equals_the_restatement_at_480x640(vga):
    _gpu()
    f, b, plane, kmat = vga
    want_s, want_x = _check(f, b, [0, 64], plane, kmat)
    assert (want_x[:, :64][~np.eye(64, dtype=bool)] > 0).sum() > 1000 and (want_s[:, 1] > 0).all()
    for C in (1, 2, 8, 63):
        _check(f[:C], b[:C], [0, C], plane, kmat)


@gpu
def test_65_candidates_are_refused_by_the_overlap_and_counted_by_the_support():
    _gpu()
    from cppf2_amd import _lib, solid
    import ctypes as C
    import torch
    f, b, plane, kmat = _case(37, 53, 65, 77)
    want = _check(f, b, [0, 65], plane, kmat, overlap=False)[0]
    assert (want[64] > 0).all()                           # the candidate past lane 63 has counts of every kind
    f200, b200 = np.concatenate([f, f, f, f[:5]]), np.concatenate([b, b, b, b[:5]])
    _check(f200, b200, [0, 200], plane, kmat, overlap=False)
    with pytest.raises(ValueError, match="at most 64"):
        solid.overlap_counts(f, b, [0, 65])
    ft = torch.from_numpy(f).cuda()
    out = torch.full((65, 64), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    off = (C.c_int32 * 2)(0, 65)
    rc = _lib.load().cppf_solid_overlap(1, 37, 53, ft.data_ptr(), ft.data_ptr(), off, 65, C.c_float(0.02), out.data_ptr(),
                                        ws.data_ptr(), ws.numel(), None)
    assert rc == -2 and (out.cpu().numpy() == -7).all()   # CPPF_EUNSUPPORTED before any device work


@gpu
def test_batch_alone_and_reversed():
    """Three images with planes and cameras of their own, the middle one without a candidate: each image's outputs are the same
    alone, in the batch and reversed."""
    _gpu()
    from cppf2_amd import solid
    cases = [_case(37, 53, 5, 21), _case(37, 53, 1, 22), _case(37, 53, 64, 23)]
    cases[1] = cases[1][:2] + (cases[1][2] * F(-1), cases[1][3] + F(3))
    cases[2] = cases[2][:2] + (cases[2][2], cases[2][3] * F(0.5))
    f, b = np.concatenate([cases[0][0], cases[2][0]]), np.concatenate([cases[0][1], cases[2][1]])
    planes, kmat = np.stack([c[2] for c in cases]), np.stack([c[3] for c in cases])
    want_s, want_x = _check(f, b, [0, 5, 5, 69], planes, kmat)
    fr, br = np.concatenate([cases[2][0], cases[0][0]]), np.concatenate([cases[2][1], cases[0][1]])
    rev_s = solid.support_counts(fr, br, [0, 64, 64, 69], planes[::-1].copy(), kmat[::-1].copy(), TAU_S).cpu().numpy()
    rev_x = solid.overlap_counts(fr, br, [0, 64, 64, 69], TAU_X).cpu().numpy()
    assert np.array_equal(rev_s, np.concatenate([want_s[5:], want_s[:5]]))
    assert np.array_equal(rev_x, np.concatenate([want_x[5:], want_x[:5]]))
    for i, (lo, hi) in enumerate(((0, 5), (5, 69))):
        k = (0, 2)[i]
        one_s, one_x = _check(f[lo:hi], b[lo:hi], [0, hi - lo], planes[k], kmat[k])
        assert np.array_equal(one_s, want_s[lo:hi]) and np.array_equal(one_x, want_x[lo:hi])


@gpu
def test_more_than_128_images_in_one_call():
    """The offsets go by value 128 images at a time: 131 small images, some without a candidate, a plane and a camera each."""
    _gpu()
    rng = np.random.default_rng(9)
    n = rng.integers(0, 4, 131)
    off = np.concatenate([[0], np.cumsum(n)])
    cases = [_case(5, 13, max(int(c), 1), 100 + i, bad=False) for i, c in enumerate(n)]
    f = np.concatenate([c[0][:k] for c, k in zip(cases, n)])
    b = np.concatenate([c[1][:k] for c, k in zip(cases, n)])
    planes = np.stack([c[2] * F(1 + 0.01 * i) for i, c in enumerate(cases)])
    kmat = np.stack([c[3] + F(0.01 * i) for i, c in enumerate(cases)])
    want_s, want_x = _check(f, b, off, planes, kmat)
    assert n[128:].sum() > 0 and (want_s[off[128]:, 0] > 0).all() and (want_s[:, 1] > 0).sum() > 40


@gpu
def test_the_exact_thresholds():
    """A back face exactly tau below the plane is not sunk, one float32 step farther is; a zero plane and a NaN plane sink
    nothing; an overlap of exactly tau does not count, one step more does."""
    _gpu()
    from test_solid import KMAT
    f, b, plane, tau = facing_plane_case()
    want = _check(f, b, [0, 1], plane, KMAT, tau_s=tau, overlap=False)[0]
    assert want.tolist() == [[4, 2, 3, 2]]
    b2 = b.copy()
    b2[0, 0, 5] = np.inf
    for pl in (np.zeros(4, F), np.full(4, np.nan, F), np.array([0, 0, -1, np.nan], F)):
        for t in (tau, F(0)):
            assert _check(f, b2, [0, 1], pl, KMAT, tau_s=t, overlap=False)[0].tolist() == [[5, 0, 3, 3]]
    fo, bo, t = overlap_tau_case()
    assert _check(fo, bo, [0, 2], np.zeros(4, F), KMAT, tau_x=t)[1][:, :2].tolist() == [[6, 2], [2, 5]]
    assert _check(fo, bo, [0, 2], np.zeros(4, F), KMAT, tau_x=F(0))[1][:, :2].tolist() == [[6, 4], [4, 5]]


@gpu
def test_values_that_are_no_depth_in_both_renders():
    _gpu()
    vals = np.array([0.0, np.nan, np.inf, -np.inf, -1.0, -0.0, 1.0], F)
    f, b = np.meshgrid(vals, vals, indexing="ij")
    f2 = np.stack([f, np.full_like(f, 0.5), f.T])
    b2 = np.stack([b, np.full_like(f, np.inf), b.T])
    plane = np.array([0.0, 0.0, -1.0, 0.5], F)
    want_s, want_x = _check(f2, b2, [0, 3], plane, np.array([8.0, 8.0, 100.0, 100.0], F))
    assert want_s[0].tolist()[0] == 14 and want_s[0, 2] == 4 and want_s[0, 3] == 20 and want_x[0, 1] == 1
    _check(f2, b2, [0, 3], plane, np.array([8.0, 8.0, 3.5, 3.5], F))        # the ray through a pixel's centre: 0 * inf


@gpu
def test_a_pair_across_a_tile_edge_that_ends_at_the_last_pixel():
    """3 x 1021 = 3063 pixels: two candidates both solid on pixels 2040 .. 3062 -- across the 2048-pixel tile, to the image's last
    pixel -- and a third on the last pixel alone."""
    _gpu()
    HW = 3 * 1021
    f, b = np.zeros((3, HW), F), np.zeros((3, HW), F)
    f[0, 2040:], b[0, 2040:] = 0.9, 1.0
    f[1, 2000:], b[1, 2000:] = 0.95, 1.1
    f[2, HW - 1], b[2, HW - 1] = 0.5, 2.0
    plane, kmat = np.array([0.0, 0.0, -1.0, 1.05], F), np.array([500.0, 500.0, 510.0, 1.5], F)
    want_s, want_x = _check(f.reshape(3, 3, 1021), b.reshape(3, 3, 1021), [0, 3], plane, kmat)
    assert want_x[:, :3].tolist() == [[1023, 1023, 1], [1023, 1063, 1], [1, 1, 1]]
    assert want_s.tolist() == [[1023, 0, 1023, 0], [1063, 1063, 1063, 0], [1, 1, 1, 0]]


@gpu
def test_the_reversed_winding_draws_the_mirrors_back_faces():
    """cppf_render_depth with cull = 1 on the reversed winding equals the NumPy rasteriser's render of the same triangles, and
    verify.render_records(back=True) is that call; on a closed mesh no pixel is open and the back face is never nearer."""
    _gpu()
    import torch
    from cppf2_amd import bop, render, verify
    H, W = 96, 128
    K = np.array([[150.0, 0, 64.0], [0, 150.0, 48.0], [0, 0, 1]])
    v, faces = RR.icosphere(2, 0.08)
    v = v * np.array([1.0, 0.6, 1.4])
    R = RR.random_rotation(np.random.default_rng(5))
    t = np.array([0.02, -0.01, 0.6])
    rev = SO.reversed_faces(faces)
    want_f = RR.render(v, faces, RR.look_pose(R, t), K, H, W)[0]
    want_b = RR.render(v, rev, RR.look_pose(R, t), K, H, W)[0]
    dev = torch.device("cuda")
    vt = torch.from_numpy(v.astype(F)).to(dev)
    pose = torch.from_numpy(RR.look_pose(R, t)[None]).to(dev)
    off = torch.tensor([0, len(faces)], dtype=torch.int32, device=dev)
    got_b = render.render_depth(vt, torch.from_numpy(rev).to(dev), off, pose, K, H, W, cull=True)[0].cpu().numpy()
    assert got_b.tobytes() == want_b.tobytes()
    obj = bop.ObjectInfo.from_mesh(render.Mesh(v, faces))
    c = (v.min(0) + v.max(0)) / 2
    Rs, ts = R[None], (R @ c + t)[None]
    rec_f = verify.render_records(obj, Rs, ts, np.array([True]), K, H, W, dev)[0].cpu().numpy()
    rec_b = verify.render_records(obj, Rs, ts, np.array([True]), K, H, W, dev, back=True)[0].cpu().numpy()
    assert obj.reversed_faces(dev) is obj.reversed_faces(dev) and np.array_equal(obj.reversed_faces(dev).cpu().numpy(), rev)
    back, solid, opn = SO.predicates(rec_f, rec_b)
    print("sphere pixels", int(solid.sum()), "open", int(opn.sum()))
    assert solid.sum() > 1000 and opn.sum() == 0 and (rec_b[solid] >= rec_f[solid]).all()
    # (the record convention centres the vertices: the same surface up to float32 rounding, the outline up to a few pixels)
    assert np.mean((rec_b > 0) != (want_b > 0)) < 0.002 and np.mean((rec_f > 0) != (want_f > 0)) < 0.002
    plane = np.array([0.0, 0.0, -1.0, 0.62], F)           # the sphere's far side lies past 0.62 m + 1 cm
    want = _check(rec_f[None], rec_b[None], [0, 1], plane, np.array([150.0, 150.0, 64.0, 48.0], F), overlap=False)[0]
    assert 0 < want[0, 1] < want[0, 0]


# ---- the two scenes of tests/solid_scenes.py on the GPU ---------------------------------------------------------------------------
import bop_data_ref as DR  # noqa: E402


@pytest.fixture(scope="module")
def s1():
    import solid_scenes
    return solid_scenes.scene1()


@pytest.fixture(scope="module")
def s2():
    import solid_scenes
    return solid_scenes.scene2()


def _explained(s, **kw):
    from cppf2_amd import scene
    return scene.explain_candidates(s["mesh"], s["d"], s["region"], DR.K, s["recs"], **kw)


def _agrees(ex, want):
    assert ex["chosen"].tolist() == want[0] and ex["gain"].tolist() == want[1] and ex["net"].tolist() == want[2]
    assert [tuple(p) for p in ex["refused_overlap"]] == want[3] and ex["passes"] == want[4]


@gpu
def test_s1_through_explain_candidates_and_select(s1):
    """The kernels on the mirror's renders, explain_candidates (which renders both windings on the GPU) and verify.select give
    the restatement's counts and decisions: without the plane A, with it A is refused and B is chosen."""
    _gpu()
    import solid_scenes as S
    from cppf2_amd import verify
    s = s1
    _check(s["f"], s["b"], [0, 2], S.PLANE, S.KMAT)
    plain = _explained(s)
    _agrees(plain, s["plain"])
    assert plain["refused_support"].size == 0 and "support" not in plain
    ex = _explained(s, plane=S.PLANE)
    _agrees(ex, s["supported"])
    assert np.array_equal(ex["support"], s["support"]) and ex["refused_support"].tolist() == [0]
    assert ex["static"][0].tolist() == [0, 0, 0] and np.array_equal(ex["static"][1], plain["static"][1])
    assert _explained(s, plane=np.zeros(4, F))["chosen"].tolist() == s["plain"][0]            # no plane was found: nothing sinks
    assert _explained(s, plane=S.PLANE, max_sunk=0.25)["chosen"].tolist() == s["plain"][0]    # 0.2366 of A is sunk
    # the plane refuses every candidate: nothing is left to explain with, and nothing is chosen
    from cppf2_amd import scene
    for kw in (dict(), dict(solid=True), dict(wide=True)):
        none = scene.explain_candidates(s["mesh"], s["d"], s["region"], DR.K, s["recs"][:1], plane=S.PLANE, **kw)
        assert none["chosen"].size == 0 and none["records"].size == 0 and none["refused_support"].tolist() == [0]
        assert none["passes"] == 1 and none["explained_pixels"] == 0 and none["region_pixels"] == int(s["region"].sum())
        assert (none["labels"] == 255).all() and none["static"].tolist() == [[0, 0, 0]] and np.array_equal(none["support"], s["support"][:1])
    both = _explained(s, plane=S.PLANE, solid=True)
    assert both["chosen"].tolist() == [1] and both["passes"] == 1 and both["refused_overlap"] == []
    # verify.select: one instance, the two candidates its hypotheses
    d, m = s["d"][None], s["region"][None]
    old = verify.select(s["mesh"], d, m, DR.K, s["recs"][None])
    new = verify.select(s["mesh"], d, m, DR.K, s["recs"][None], plane=S.PLANE)
    assert old["chosen"].tolist() == [0] and new["chosen"].tolist() == [1] and new["refused"].tolist() == [[True, False]]
    assert np.array_equal(new["support"][0], s["support"]) and new["scores"][0, 0] == 0.0 and new["scores"][0, 1] == old["scores"][0, 1]
    assert np.array_equal(new["counts"], old["counts"]) and set(new) - set(old) == {"support", "refused"}
    assert new["records"]["pad_"][0, 1] == 1 and new["records"]["flags"][0] & verify.CHOSEN


@gpu
def test_s2_through_explain_candidates_and_select(s2):
    """Today's greedy picks the pose inside the front cube as a third instance; with solid=True it is inside instance 0."""
    _gpu()
    import solid_scenes as S
    from cppf2_amd import solid, verify
    s = s2
    want_s, want_x = _check(s["f"], s["b"], [0, 3], S.PLANE, S.KMAT)
    assert np.array_equal(want_x, s["inter"])
    plain = _explained(s)
    _agrees(plain, s["plain"])
    ex = _explained(s, solid=True)
    _agrees(ex, s["solid"])
    assert ex["records"].tobytes() == s["recs"][[0, 2]].tobytes() and np.array_equal(ex["static"], plain["static"])
    assert ex["labels"].tobytes() != plain["labels"].tobytes() and ex["explained_pixels"] == sum(s["solid"][1])
    wide = _explained(s, solid=True, wide=True, plane=S.PLANE)
    _agrees(wide, s["solid"])
    assert np.array_equal(wide["support"], s["support"]) and wide["refused_support"].size == 0
    assert _explained(s, solid=True, max_overlap=0.5)["chosen"].tolist() == s["plain"][0]      # 0.42 of the phantom is inside
    assert _explained(s, solid=True, solid_tau=0.15)["chosen"].tolist() == s["plain"][0]       # longer than a cube's diagonal
    # verify.select with the plane: nothing stands under the table, and the result is the one without the plane
    d, m = np.repeat(s["d"][None], 2, 0), np.stack([s["ref"]["masks"][0] > 0, s["ref"]["masks"][1] > 0])
    recs = np.stack([s["recs"], s["recs"][[2, 1, 0]]])
    old = verify.select(s["mesh"], d, m, DR.K, recs)
    new = verify.select(s["mesh"], d, m, DR.K, recs, plane=np.stack([S.PLANE, S.PLANE]), support_tau=solid.SUPPORT_TAU)
    assert not new["refused"].any() and np.array_equal(new["support"][0], s["support"])
    assert np.array_equal(new["support"][1], s["support"][[2, 1, 0]])
    for k in old:
        if k != "icp":
            assert np.array_equal(np.asarray(old[k]), np.asarray(new[k]), equal_nan=(k == "scores")), k
    assert old["icp"] is None and new["icp"] is None and set(new) - set(old) == {"support", "refused"}


def _inject(monkeypatch, cands):
    """The vote's hypotheses replaced by the scene's candidates (the selected record with their R and t), so that eval.py's
    stages after the vote run on poses the restatement has decided."""
    from cppf2_amd import ensemble, verify

    def fake(selected, pick, hyps, enabled, H):
        recs = np.repeat(np.asarray(selected).reshape(1), H)
        recs["flags"] |= verify.EMPTY
        for h, c in enumerate(cands[:H]):
            recs[h]["R"], recs[h]["t"] = c["R"], c["t"]
            recs["flags"][h] &= ~verify.EMPTY
        return recs, np.where(np.arange(H) < len(cands), 0, -1).astype(np.int64)
    monkeypatch.setattr(ensemble, "_instance_hypotheses", fake)


def _equals_the_parents_report(rep, name):
    """The report of a run without the new flags against tests/golden/solid/<name>: that call's report as the parent commit printed it
    (recorded on an MI355X with the same candidates injected), as JSON text, byte for byte."""
    import json
    want = open(os.path.join(ROOT, "tests", "golden", "solid", name)).read()
    got = json.dumps(rep)
    assert json.dumps(json.loads(want)) == want, "the fixture is json.dumps' own text"
    if got != want:
        a, b = json.loads(got), json.loads(want)
        diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        raise AssertionError("the flag-less report differs from the parent's in %s" % diff)


def _without(rep, keys=("solid_checks",)):
    import copy
    rep = copy.deepcopy(rep)
    for k in keys:
        rep.pop(k, None)
    return rep


@gpu
def test_eval_refuses_the_pose_under_the_table(s1, tmp_path, monkeypatch):
    """eval.py --propose_masks --hypotheses=2 --explain_scene --explain_hypotheses on S1 with the two candidates as the
    hypotheses: without --support_check A is verified and explains the scene, with it A is refused in verify.select and is
    below_table in the explanation, and B is reported; without the new flags the report has none of the new entries."""
    import json
    from PIL import Image
    _gpu()
    import solid_scenes as S
    monkeypatch.chdir(ROOT)
    import eval as ev
    s = s1
    dpath = str(tmp_path / "depth.png")
    Image.fromarray(np.round(s["d"].astype(np.float64) * S.SCALE).astype(np.uint16)).save(dpath)
    _inject(monkeypatch, s["recs"])
    kw = dict(data="depth", depth=dpath, depth_scale=S.SCALE, intrinsics=DR.K.tolist(), num_pairs=5000, num_rots=36, opt=False,
              debug=True, hypotheses=2, seed=0, propose_masks=True, mesh=s["mesh_path"], mesh_scale=s["mesh_scale"],
              explain_scene=True, explain_hypotheses=True)
    plain = ev.main(**kw)
    _equals_the_parents_report(plain, "eval_s1.json")
    assert len(plain["proposals"]) == 1 and plain["results"][0]["verify"]["chosen"] == 0
    assert [i["hypothesis"] for i in plain["scene"]["instances"]] == [0] and "passes" not in plain["scene"]
    assert "solid_checks" not in plain and "support" not in plain["results"][0]["verify"]
    assert all("support_counts" not in e for e in plain["scene"]["instances"] + plain["scene"]["rejected"])
    assert plain["scene"]["instances"][0]["gain"] == s["plain"][1][0]
    rep = ev.main(support_check=True, **kw)
    v = rep["results"][0]["verify"]
    print("S1 eval", v, rep["scene"]["instances"], rep["scene"]["rejected"], rep["plane"])
    assert v["chosen"] == 1 and v["refused"] == [True, False] and v["score_first"] == 0.0
    # the plane is the fitted one, which the report carries exactly (floats of its float32 values): the restatement with that
    # plane on the mirror's renders gives the report's counts
    fitted = np.array(list(rep["plane"]["n"]) + [rep["plane"]["d"]], dtype=F)
    assert np.array_equal(fitted.astype(np.float64), np.array(list(rep["plane"]["n"]) + [rep["plane"]["d"]]))
    assert np.array_equal(fitted, s["ref"]["plane"].astype(F)), "the GPU's plane is the CPU segmentation's"
    want_sup = SO.support(s["f"], s["b"], [0, 2], fitted, S.KMAT, 0.01)
    sup = np.array(v["support"])
    assert sup.tolist() == want_sup.tolist() and want_sup[1, 1] == 0
    assert (SO.sunk_share(want_sup) > 0.1).tolist() == [True, False]
    sc = rep["scene"]
    assert [i["hypothesis"] for i in sc["instances"]] == [1] and sc["instances"][0]["gain"] == s["supported"][1][0]
    assert sc["instances"][0]["support_counts"] == sup[1].tolist() and sc["passes"] == 1
    assert [(r["hypothesis"], r["reason"], r["support_counts"]) for r in sc["rejected"]] == [(0, "below_table", sup[0].tolist())]
    assert rep["solid_checks"] == dict(support=dict(tau=0.01, max_share=0.1), overlap=None)
    assert rep["proposals"][0]["R"] == sc["instances"][0]["R"] and rep["proposals"][0]["t"] == sc["instances"][0]["t"]
    # a threshold that lets A through gives the plain run's decisions
    lax = ev.main(support_check=True, support_max_share=0.5, **kw)
    assert lax["results"][0]["verify"]["chosen"] == 0 and lax["results"][0]["verify"]["refused"] == [False, False]
    assert [i["hypothesis"] for i in lax["scene"]["instances"]] == [0]
    assert json.dumps(_without(lax)["proposals"]) == json.dumps(plain["proposals"])


@gpu
def test_eval_refuses_the_pose_inside_the_front_cube(s2, tmp_path, monkeypatch):
    """eval.py --explain_scene --explain_hypotheses on S2 with the three candidates as every proposal's hypotheses: the pose
    inside the front cube is a third instance today and is rejected as inside instance 0 with --explain_solid."""
    import json
    from PIL import Image
    _gpu()
    import solid_scenes as S
    monkeypatch.chdir(ROOT)
    import eval as ev
    s = s2
    dpath, mpath = str(tmp_path / "depth.png"), str(tmp_path / "cube.obj")
    Image.fromarray(np.round(s["d"].astype(np.float64) * S.SCALE).astype(np.uint16)).save(dpath)
    with open(mpath, "w") as fh:
        fh.write("".join("v %r %r %r\n" % tuple(float(x) for x in v) for v in s["cube"][0]))
        fh.write("".join("f %d %d %d\n" % tuple(int(x) + 1 for x in t) for t in s["cube"][1]))
    _inject(monkeypatch, s["recs"])
    kw = dict(data="depth", depth=dpath, depth_scale=S.SCALE, intrinsics=DR.K.tolist(), num_pairs=5000, num_rots=36, opt=False,
              debug=True, hypotheses=3, seed=0, propose_masks=True, mesh=mpath, mesh_scale=1.0, explain_scene=True,
              explain_hypotheses=True)
    plain = ev.main(**kw)
    _equals_the_parents_report(plain, "eval_s2.json")
    got = [(i["proposal"], i["hypothesis"], i["gain"]) for i in plain["scene"]["instances"]]
    print("S2 eval plain", got, plain["scene"]["rejected"])
    assert got == [(0, 0, s["plain"][1][0]), (1, 2, s["plain"][1][1]), (0, 1, s["plain"][1][2])]
    rep = ev.main(explain_solid=True, **kw)
    sc = rep["scene"]
    got = [(i["proposal"], i["hypothesis"], i["gain"]) for i in sc["instances"]]
    print("S2 eval solid", got, sc["rejected"], sc["passes"])
    assert got == [(0, 0, s["solid"][1][0]), (1, 2, s["solid"][1][1])] and sc["passes"] == 2
    inside = [r for r in sc["rejected"] if r["reason"] == "inside"]
    assert [(r["proposal"], r["hypothesis"], r["inside_of"]) for r in inside] == [(0, 1, 0)]
    assert all("support_counts" not in e for e in sc["instances"] + sc["rejected"])
    assert rep["solid_checks"] == dict(support=None, overlap=dict(tau=0.02, max_share=0.1))
    # everything outside the scene entry is the plain run's
    assert json.dumps({k: v for k, v in _without(rep).items() if k != "scene"}) == json.dumps({k: v for k, v in plain.items() if k != "scene"})
    allon = ev.main(explain_solid=True, support_check=True, **kw)
    assert [(i["proposal"], i["hypothesis"]) for i in allon["scene"]["instances"]] == [(0, 0), (1, 2)]
    assert all(r["reason"] != "below_table" for r in allon["scene"]["rejected"])
    assert not any(any(r_["verify"]["refused"]) for r_ in allon["results"])
    fitted = np.array(list(allon["plane"]["n"]) + [allon["plane"]["d"]], dtype=F)
    want_sup = SO.support(s["f"], s["b"], [0, 3], fitted, S.KMAT, 0.01).tolist()
    assert [r_["verify"]["support"] for r_ in allon["results"]] == [want_sup, want_sup]
