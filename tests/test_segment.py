"""CPU checks of the proposal layer (cppf2_amd/segment.py): the mechanism on the one real frame of this tree,
by the restatement alone (tests/segment_ref.py; tests/test_segment_gpu.py holds the kernels to it byte for byte); eval.py's
flag rules; the wrappers' argument errors; the return codes of the C entry points before any device work; the pinned workspace
sizes; the restatement's ranking on hand-drawn cases."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import prep_ref as PR  # noqa: E402
import segment_ref as SR  # noqa: E402


def test_real_frame_plane_and_proposals_by_the_restatement():
    """example_data/depth.png with EXAMPLE_K, Philox seed 0 (the first seed tried: it lies inside every bound) and the defaults:
    the winning plane holds at least 35 % of the valid pixels, exactly one proposal has an IoU above 0.5 with mask.png restricted
    to valid depth, and that IoU is at least 0.75."""
    from cppf2_amd import masks, segment
    d, mv = SR.example_frame()
    r = SR.propose(d, PR.EXAMPLE_K, SR.REAL_SEED, segment.NUM_HYP, segment.TAU, segment.MIN_HEIGHT, 0.0, masks.JUMP,
                   segment.MIN_SEGMENT_PIXELS, segment.MAX_SEGMENTS)
    valid = int(SR.valid_pixels(d).sum())
    ious = [float(np.count_nonzero((p > 0) & mv)) / float(np.count_nonzero((p > 0) | mv)) for p in r["masks"]]
    print("plane", r["plane"].tolist(), "stats", r["pstats"].tolist(), "of", valid, "valid; segments", r["stats"].tolist(),
          "IoU", [round(x, 3) for x in ious])
    assert r["pstats"][3] == valid == 224197
    assert r["pstats"][0] >= 0 and r["pstats"][1] >= 0.35 * valid
    assert abs(float(np.linalg.norm(r["plane"][:3].astype(np.float64))) - 1.0) < 1e-6 and r["plane"][3] > 0
    assert sum(i > 0.5 for i in ious) == 1
    assert max(ious) >= 0.75
    # the rows agree with the masks: pixels, inclusive boxes, labels = first pixels in row-major order
    for p, row in zip(r["masks"], r["seg"]):
        rr, cc = np.nonzero(p)
        assert row.tolist() == [int(rr[0] * p.shape[1] + cc[np.flatnonzero(rr == rr[0])[0]]), len(rr), cc.min(), rr.min(), cc.max(),
                                rr.max()]
    assert list(r["seg"][:, 1]) == sorted(r["seg"][:, 1], reverse=True) and (r["seg"][:, 1] >= segment.MIN_SEGMENT_PIXELS).all()


# ---- eval.py's flag rules ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,match", [
    (dict(data="depth", depth="d.png", propose_masks=True, mask="m.png"), "replaces --mask"),
    (dict(propose_masks=True), "data=depth"),
    (dict(data="bop", bop_root="r", out_csv="o.csv", propose_masks=True), "data=depth"),
    (dict(data="depth", depth="d.png", propose_masks=True, clean_mask=True), "clean_mask"),
    (dict(data="depth", depth="d.png", mask="m.png", plane_tau=0.01), "needs --propose_masks"),
    (dict(data="depth", depth="d.png", mask="m.png", plane_hypotheses=64), "needs --propose_masks"),
    (dict(data="depth", depth="d.png", mask="m.png", plane_min_height=0.02), "needs --propose_masks"),
    (dict(data="depth", depth="d.png", mask="m.png", min_segment_pixels=10), "needs --propose_masks"),
    (dict(data="depth", depth="d.png", mask="m.png", max_proposals=4), "needs --propose_masks"),
    (dict(data="depth", depth="d.png", propose_masks=True, plane_tau=0.0), "plane_tau"),
    (dict(data="depth", depth="d.png", propose_masks=True, plane_tau=float("nan")), "plane_tau"),
    (dict(data="depth", depth="d.png", propose_masks=True, plane_hypotheses=0), "plane_hypotheses"),
    (dict(data="depth", depth="d.png", propose_masks=True, plane_hypotheses=1025), "plane_hypotheses"),
    (dict(data="depth", depth="d.png", propose_masks=True, plane_min_height=float("inf")), "plane_min_height"),
    (dict(data="depth", depth="d.png", propose_masks=True, min_segment_pixels=-1), "min_segment_pixels"),
    (dict(data="depth", depth="d.png", propose_masks=True, max_proposals=0), "max_proposals"),
    (dict(data="depth", depth="d.png", propose_masks=True, max_proposals=65), "max_proposals"),
    (dict(data="depth", depth="d.png", propose_masks=True, mask_jump=-0.01), "mask_jump"),
    (dict(data="depth", depth="d.png", propose_masks=True, hypotheses=4), "needs --data=depth and --mesh"),
])
def test_eval_flag_rules(kw, match, monkeypatch):
    monkeypatch.chdir(ROOT)
    import eval as ev
    with pytest.raises(ValueError, match=match):
        ev.main(**kw)


def test_checked_flags_normalise_the_proposal_arguments(monkeypatch):
    import inspect
    monkeypatch.chdir(ROOT)
    import eval as ev
    from cppf2_amd import masks, segment
    base = {k: p.default for k, p in inspect.signature(ev.main).parameters.items()}
    assert ev._checked_flags(**dict(base, data="depth", mask="m.png")).propose is None
    assert ev._checked_flags(**base).propose is None
    f = ev._checked_flags(**dict(base, data="depth", propose_masks=True))
    assert f.propose == dict(num_hyp=segment.NUM_HYP, tau=segment.TAU, min_height=segment.MIN_HEIGHT, jump=masks.JUMP,
                             min_pixels=segment.MIN_SEGMENT_PIXELS, max_segments=segment.MAX_SEGMENTS)
    assert f.propose == dict(num_hyp=256, tau=0.005, min_height=0.01, jump=0.01, min_pixels=200, max_segments=16)
    f = ev._checked_flags(**dict(base, data="depth", propose_masks=True, plane_tau=0.002, plane_hypotheses=64, plane_min_height=0.02,
                                 mask_jump=0.005, min_segment_pixels=50, max_proposals=4))
    assert f.propose == dict(num_hyp=64, tau=0.002, min_height=0.02, jump=0.005, min_pixels=50, max_segments=4)


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_bad_arguments_before_any_launch():
    import torch
    from cppf2_amd import ops, segment
    d = np.ones((3, 4), np.float32)
    K = PR.EXAMPLE_K
    for kw in (dict(num_hyp=0), dict(num_hyp=1025), dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf"))):
        with pytest.raises(ValueError):
            segment.fit_plane(d, K, [0], **kw)
    with pytest.raises(ValueError):
        segment.fit_plane(d, K, ["x"])
    for kw in (dict(min_height=float("nan")), dict(max_height=float("nan"))):
        with pytest.raises(ValueError):
            segment.foreground(d, K, np.zeros(4, np.float32), **kw)
    for kw in (dict(jump=-0.01), dict(jump=float("nan")), dict(jump=float("inf")), dict(min_pixels=-1), dict(max_segments=0),
               dict(max_segments=65)):
        with pytest.raises(ValueError):
            segment.segments(np.ones((1, 3, 4), np.uint8), d, 0, **kw)
    with pytest.raises(ValueError):
        segment.propose(np.ones((2, 3, 4), np.float32), K)
    # the camera matrix: zero skew only
    assert segment.intrinsics4(K, 2).tolist() == [[np.float32(1066.778), np.float32(1067.487), np.float32(312.9869),
                                                   np.float32(241.3109)]] * 2
    assert segment.intrinsics4([500.0, 501.0, 3.0, 2.0], 1).tolist() == [[500.0, 501.0, 3.0, 2.0]]
    for bad in (PR.INTRINSICS["skew"], PR.INTRINSICS["w2"], np.eye(4), [1.0, 2.0, 3.0], [[0.0, 1.0, 2.0, 3.0]],
                [[float("nan"), 1.0, 2.0, 3.0]], np.ones((3, 4))):
        with pytest.raises(ValueError):
            segment.intrinsics4(bad, 2 if np.shape(bad) == (3, 4) else 1)
    if not torch.cuda.is_available():
        with pytest.raises(ops.CppfError):                  # no CPU fallback
            segment.fit_plane(d, K, [0])
        with pytest.raises(ops.CppfError):
            segment.foreground(d, K, np.zeros(4, np.float32))
        with pytest.raises(ops.CppfError):
            segment.segments(np.ones((1, 3, 4), np.uint8), d, 0)


def test_detections_list_every_proposal_once_per_object():
    from cppf2_amd import masks, segment
    m = np.zeros((2, 5, 6), np.uint8)
    m[0, 1:3, 2:5] = 255
    m[1, 4, 0] = 255
    dets = segment.detections(m, [1, 5], 7, 9)
    assert [(e["category_id"], e["bbox"]) for e in dets] == [(1, [2, 1, 3, 2]), (1, [0, 4, 1, 1]), (5, [2, 1, 3, 2]), (5, [0, 4, 1, 1])]
    assert all(e["scene_id"] == 7 and e["image_id"] == 9 and e["score"] == 1.0 and e["size"] == (5, 6) for e in dets)
    assert np.array_equal(masks.rle_decode(dets[2]["counts"], 5, 6), m[0])


# ---- the C entry points without a device ------------------------------------------------------------------------------------------
def _lib():
    from cppf2_amd import _lib
    lib = _lib.load()
    return lib._lib if isinstance(lib, _lib._Traced) else lib


# fake device addresses, 16-byte aligned and never dereferenced: validation comes before any device work
_A, _B, _C, _D, _E, _F, _G, _H = (0x100000 * (i + 1) for i in range(8))
_OK, _EINVAL = 0, -1


def test_workspace_bytes_are_pinned():
    lib = _lib()
    fit = lib.cppf_plane_fit_workspace_bytes
    assert fit(1, 1) == 512 and fit(1, 16) == 512 and fit(1, 17) == 768 and fit(1, 64) == 1280 and fit(1, 256) == 5120
    assert fit(1, 1024) == 20480 and fit(8, 1024) == 163840 and fit(3, 65) == 3328 + 1024 and fit(65535, 1024) == 65535 * 20480
    assert fit(0, 8) == fit(-1, 8) == fit(65536, 8) == fit(1, 0) == fit(1, 1025) == 0
    seg = lib.cppf_mask_segments_workspace_bytes
    assert seg(2, 3, 5, 1) == 256 + 2 * 15 * 8 == lib.cppf_mask_components_workspace_bytes(2, 3, 5)
    assert seg(2, 3, 5, 16) == 256 + 2 * 15 * 8 and seg(2, 3, 5, 17) == 512 + 2 * 15 * 8 and seg(1, 480, 640, 64) == 512 + 480 * 640 * 8
    assert seg(64, 480, 640, 16) == 8192 + 64 * 480 * 640 * 8
    assert seg(0, 3, 5, 4) == seg(-1, 3, 5, 4) == seg(2, 0, 5, 4) == seg(2, 3, 8193, 4) == seg(65536, 3, 5, 4) == 0
    assert seg(2, 3, 5, 0) == seg(2, 3, 5, 65) == 0


def test_validation_return_codes_without_a_device():
    lib = _lib()
    need_fit = lib.cppf_plane_fit_workspace_bytes

    def fit(I=2, H=3, W=5, depths=_A, K=_B, seeds=_C, num_hyp=8, tau=0.005, plane=_D, stats=_E, ws=_F, short=0):
        return lib.cppf_plane_fit(I, H, W, depths, K, seeds, num_hyp, C.c_float(tau), plane, stats, ws,
                                  need_fit(max(I, 1), min(max(num_hyp, 1), 1024)) - short, None)
    assert fit(I=0) == _OK and fit(I=0, depths=None, K=None, seeds=None, plane=None, stats=None, ws=None) == _OK
    for kw in [dict(I=-1), dict(I=65536), dict(H=0), dict(W=0), dict(H=8193), dict(W=8193), dict(num_hyp=0), dict(num_hyp=1025),
               dict(tau=0.0), dict(tau=-0.005), dict(tau=float("nan")), dict(tau=float("inf")), dict(depths=None), dict(K=None),
               dict(seeds=None), dict(plane=None), dict(stats=None), dict(ws=None), dict(ws=_F + 8), dict(short=1)]:
        assert fit(**kw) == _EINVAL, kw
        assert b"cppf_plane_fit: invalid argument" in lib.cppf_last_error_string()

    def fg(I=2, H=3, W=5, depths=_A, K=_B, plane=_D, lo=0.01, hi=0.0, out=_G):
        return lib.cppf_plane_foreground(I, H, W, depths, K, plane, C.c_float(lo), C.c_float(hi), out, None)
    assert fg(I=0) == _OK and fg(I=0, depths=None, K=None, plane=None, out=None) == _OK
    for kw in [dict(I=-1), dict(I=65536), dict(H=0), dict(W=8193), dict(depths=None), dict(K=None), dict(plane=None), dict(out=None),
               dict(lo=float("nan")), dict(hi=float("nan"))]:
        assert fg(**kw) == _EINVAL, kw
        assert b"cppf_plane_foreground: invalid argument" in lib.cppf_last_error_string()
    need = lib.cppf_mask_segments_workspace_bytes

    def seg(D=2, I=1, H=3, W=5, masks=_A, depths=_B, idx=_C, jump=0.01, min_pixels=1, M=4, rank=_D, rows=_E, stats=_G, ws=_F, short=0):
        return lib.cppf_mask_segments(D, I, H, W, masks, depths, idx, C.c_float(jump), min_pixels, M, rank, rows, stats, ws,
                                      need(max(D, 1), H, W, min(max(M, 1), 64)) - short, None)
    assert seg(D=0) == _OK
    assert seg(D=0, masks=None, depths=None, idx=None, rank=None, rows=None, stats=None, ws=None) == _OK
    for kw in [dict(D=-1), dict(D=65536), dict(I=0), dict(H=0), dict(W=8193), dict(M=0), dict(M=65), dict(masks=None), dict(depths=None),
               dict(idx=None), dict(rank=None), dict(rows=None), dict(stats=None), dict(ws=None), dict(ws=_F + 4), dict(short=1),
               dict(jump=-1e-6), dict(jump=float("nan")), dict(jump=float("inf")), dict(min_pixels=-1)]:
        assert seg(**kw) == _EINVAL, kw
        assert b"cppf_mask_segments: invalid argument" in lib.cppf_last_error_string()


# ---- the restatement on hand-drawn cases ------------------------------------------------------------------------------------------
def test_restatement_ranks_by_size_then_label_and_boxes_are_inclusive():
    mask = np.array([[1, 1, 0, 1, 1, 0, 1],
                     [0, 0, 0, 1, 0, 0, 1],
                     [1, 1, 0, 0, 0, 0, 1],
                     [0, 0, 0, 1, 1, 1, 0]], np.uint8)
    depth = np.ones((4, 7), np.float32)
    # components by label: 0 {0, 1}, 3 {3, 4, 10}, 6 {6, 13, 20}, 14 {14, 15}, 24 {24, 25, 26}
    rank, seg, stats = SR.segments(mask, depth, 0.0, 1, 4)
    assert stats.tolist() == [5, 4, 5, 13]
    assert seg.tolist() == [[3, 3, 3, 0, 4, 1], [6, 3, 6, 0, 6, 2], [24, 3, 3, 3, 5, 3], [0, 2, 0, 0, 1, 0]]
    assert rank[0].tolist() == [3, 3, 255, 0, 0, 255, 1] and rank[2].tolist() == [255, 255, 255, 255, 255, 255, 1]
    assert rank[3].tolist() == [255, 255, 255, 2, 2, 2, 255]
    # min_pixels 3 drops the pairs; two unused rows
    rank, seg, stats = SR.segments(mask, depth, 0.0, 3, 5)
    assert stats.tolist() == [5, 3, 3, 13] and seg[3:].tolist() == [[-1] * 6] * 2 and (rank == 3).sum() == 0
    # M = 1 is mask_ref.components
    import mask_ref as MR
    rank, seg, stats = SR.segments(mask, depth, 0.0, 1, 1)
    out, cstats = MR.components(mask, depth, 0.0, 1)
    assert np.array_equal(rank == 0, out > 0) and seg[0, :2].tolist() == [cstats[1], cstats[2]]


def test_restatement_plane_of_an_exact_ramp_and_the_height_threshold():
    """A plane z = const seen by a pinhole camera: every usable hypothesis is the plane itself up to rounding, so the lowest
    usable index wins with every valid pixel; the foreground keeps what is strictly higher than min_height."""
    d = np.full((12, 16), 0.5, np.float32)
    d[0, 0], d[3, 4], d[5, 5] = 0.0, np.nan, np.inf
    K = [50.0, 50.0, 8.0, 6.0]
    plane, stats, counts = SR.fit_plane(d, K, 3, 64, 1e-4)
    usable = np.flatnonzero(counts >= 0)
    assert stats[3] == 12 * 16 - 3 and stats[2] == len(usable) > 8 and stats[0] == usable[0] and stats[1] == stats[3]
    assert (counts[usable] == stats[3]).all()
    assert abs(abs(plane[2]) - 1) < 1e-6 and abs(plane[3] - 0.5) < 1e-6 and plane[2] < 0
    d[7, 7] = 0.25                                           # a quarter of a metre above the plane
    fg = SR.foreground(d, K, plane, 0.01)
    assert fg.sum() == 255 and fg[7, 7] == 255
    assert SR.foreground(d, K, np.zeros(4, np.float32), 0.01).sum() == 255 * (12 * 16 - 3)
    h = SR.heights(d, K, plane)[7, 7]
    assert SR.foreground(d, K, plane, h)[7, 7] == 0 and SR.foreground(d, K, plane, np.nextafter(h, np.float32(0)))[7, 7] == 255
    assert SR.foreground(d, K, plane, 0.01, max_height=0.2)[7, 7] == 0 and SR.foreground(d, K, plane, 0.01, max_height=h)[7, 7] == 255
