"""CPU checks of the mask layer: the host run-length codec (cppf2_amd/masks.py) on random and edge masks, COCO's compressed
string form on vectors worked by hand from its definition, the detections file (bop_data.read_detections / write_detections)
and each of its errors, the validation return codes of the three C entry points without a device, and the restatement
(tests/mask_ref.py) on hand-drawn cases whose answers are written here."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mask_ref as MR  # noqa: E402


def test_host_rle_round_trip_random_and_edge_masks():
    from cppf2_amd import masks
    rng = np.random.default_rng(3)
    cases = [rng.random(s) < p for s in ((37, 53), (1, 1), (3, 1021), (33, 4), (480, 640)) for p in (0.02, 0.5, 0.97)]
    cases += [np.zeros((5, 7), bool), np.ones((5, 7), bool), np.zeros((1, 1), bool), np.ones((1, 1), bool)]
    one_run = np.zeros((6, 4), bool)
    one_run[2:5, 1] = True                                  # a single run of ones inside one column
    first = np.zeros((4, 3), bool)
    first[0, 0] = True                                      # the first pixel set: a leading zero-length run
    cases += [one_run, first]
    for m in cases:
        c = masks.rle_encode(m)
        H, W = m.shape
        assert all(isinstance(x, int) and x >= 0 for x in c) and sum(c) == H * W
        assert all(x > 0 for x in c[1:]), "only the first run may be empty"
        got = masks.rle_decode(c, H, W)
        assert got.dtype == np.uint8 and np.array_equal(got, np.where(m, 255, 0)) and np.array_equal(got, MR.decode(c, H, W))
        assert masks.string_to_counts(masks.counts_to_string(c)) == c
    assert masks.rle_encode(np.zeros((5, 7), bool)) == [35] and masks.rle_encode(np.ones((5, 7), bool)) == [0, 35]
    assert masks.rle_encode(np.ones((1, 1), bool)) == [0, 1] and masks.rle_encode(np.zeros((1, 1), bool)) == [1]
    assert masks.rle_encode(one_run) == [8, 3, 13]          # column-major: column 0 (6) + rows 0-1 of column 1, the run, the rest
    assert masks.rle_encode(first) == [0, 1, 11]
    # column-major, not row-major: the two pixels of a row are H apart
    assert masks.rle_encode(np.array([[1, 1], [0, 0], [0, 0]])) == [0, 1, 2, 1, 2]
    for bad in ([36], [34], [10, -1, 26], [40, -5]):
        with pytest.raises(masks.RleError):
            masks.rle_decode(bad, 5, 7)


def test_compressed_string_vectors_worked_by_hand():
    """Each value v (a count, from index 3 on its difference to the count two before) as 5-bit groups, lowest first; a group g
    is followed by another unless the rest is 0 (g bit 0x10 clear) or -1 (g bit 0x10 set); character = chr(48 + g + 32 * more).
      0, 5, 3              -> '0' '5' '3'                                       (one group each)
      40 - 5 = 35          -> groups 3 (more), 1               -> chr(48+35) chr(48+1)          = 'S' '1'
      1000 - 3 = 997       -> 5 (more), 31 (bit 0x10 set, rest 0 is not -1: more), 0           = 'U' 'o' '0'
      2 - 40 = -38         -> -38 & 31 = 26 (rest -2: more), -2 & 31 = 30 (rest -1: last)      = 'j' 'N'
      100000               -> 0 (more), 21 (more), 1 (more), 3                                 = 'P' 'e' 'Q' '3'
      16                   -> 16 (bit 0x10 set, rest 0 is not -1: more), 0   -> chr(48+48) chr(48)      = '`' '0'
      [7, 7, 7, 7, 7]      -> 7, 7, 7, then 7 - 7 = 0 twice                                    = '77700'"""
    from cppf2_amd import masks
    vectors = [([0, 5, 3, 40, 1000, 2], "053S1Uo0jN"), ([100000], "PeQ3"), ([16], "`0"), ([7, 7, 7, 7, 7], "77700"),
               ([], ""), ([35], "S1"), ([0, 35], "0S1")]
    for counts, s in vectors:
        assert masks.counts_to_string(counts) == s, (counts, masks.counts_to_string(counts))
        assert masks.string_to_counts(s) == counts, (s, masks.string_to_counts(s))
        assert masks.string_to_counts(s.encode("ascii")) == counts
    for bad in ("P", "05o", "0 5", "05\x7f", "o" * 14 + "0"):             # cut off inside a value (twice), outside the code, too long
        with pytest.raises(masks.RleError):
            masks.string_to_counts(bad)


def _dets():
    from cppf2_amd import masks
    rng = np.random.default_rng(11)
    out = []
    for n in range(4):
        m = rng.random((12, 17)) < 0.4
        out.append(dict(scene_id=n // 2, image_id=n % 2, category_id=15 if n else 2, bbox=[float(x) for x in masks.bbox(m)],
                        score=1.0 / (n + 1), time=0.25 * n, size=(12, 17), counts=masks.rle_encode(m)))
    return out


@pytest.mark.parametrize("compress", [True, False])
def test_detections_file_round_trip(tmp_path, compress):
    from cppf2_amd import bop_data
    dets = _dets()
    p = str(tmp_path / "dets.json")
    bop_data.write_detections(p, dets, compress=compress)
    raw = json.load(open(p))
    assert isinstance(raw[0]["segmentation"]["counts"], str if compress else list) and raw[0]["segmentation"]["size"] == [12, 17]
    assert set(raw[0]) == {"scene_id", "image_id", "category_id", "bbox", "score", "time", "segmentation"}
    assert bop_data.read_detections(p) == dets
    assert bop_data.read_detections(p, image_size=(12, 17)) == dets
    assert bop_data.read_detections(p, image_size=lambda s, i: (12, 17)) == dets


def test_detections_file_errors(tmp_path):
    from cppf2_amd import bop_data

    def write(counts, size=(12, 17), **kw):
        e = dict(scene_id=0, image_id=0, category_id=15, bbox=[0, 0, 1, 1], score=0.5, time=0.0,
                 segmentation=dict(counts=counts, size=list(size)))
        e.update(kw)
        p = str(tmp_path / "bad.json")
        json.dump([e], open(p, "w"))
        return p
    good = [100, 4, 100]
    assert len(bop_data.read_detections(write(good))) == 1
    with pytest.raises(bop_data.BopDataError, match="differs"):                     # a size that differs from the image's
        bop_data.read_detections(write(good), image_size=(17, 12))
    with pytest.raises(bop_data.BopDataError, match="sum"):                         # runs that do not sum to H * W
        bop_data.read_detections(write([100, 4, 99]))
    with pytest.raises(bop_data.BopDataError, match="negative"):                    # a negative run
        bop_data.read_detections(write([110, -6, 100]))
    with pytest.raises(bop_data.BopDataError, match="ends inside"):                 # strings that do not parse
        bop_data.read_detections(write("05o"))
    with pytest.raises(bop_data.BopDataError, match="outside the code"):
        bop_data.read_detections(write("0 5"))
    with pytest.raises(bop_data.BopDataError, match="sum"):                         # a string that parses to the wrong total
        bop_data.read_detections(write("053"))
    with pytest.raises(bop_data.BopDataError):
        bop_data.read_detections(write([100.5, 3.5, 100]))
    with pytest.raises(bop_data.BopDataError, match="size"):
        bop_data.read_detections(write(good, size=(12, 17, 1)))
    with pytest.raises(bop_data.BopDataError, match="missing field"):
        bop_data.read_detections(write(good, segmentation=dict(counts=good)))
    p = str(tmp_path / "dict.json")
    json.dump({"a": 1}, open(p, "w"))
    with pytest.raises(bop_data.BopDataError):
        bop_data.read_detections(p)
    with pytest.raises(ValueError):
        bop_data.write_detections(p, [dict(_dets()[0], counts=[1, 2, 3])])


def _lib():
    from cppf2_amd import _lib
    lib = _lib.load()
    return lib._lib if isinstance(lib, _lib._Traced) else lib


# fake device addresses, 8-byte aligned and never dereferenced: validation comes before any device work
_A, _B, _C, _D, _E, _F = (0x100000 * (i + 1) for i in range(6))
_OK, _EINVAL = 0, -1


def test_validation_return_codes_without_a_device():
    import ctypes as C
    lib = _lib()
    dec = lib.cppf_rle_decode
    assert dec(0, 4, 4, None, 0, None, None, None) == _OK                          # no masks: nothing to do
    for args in [(-1, 4, 4, _A, 3, _B, _C), (1, 0, 4, _A, 3, _B, _C), (1, 4, 8193, _A, 3, _B, _C), (1, 4, 4, None, 3, _B, _C),
                 (1, 4, 4, _A, 3, None, _C), (1, 4, 4, _A, 3, _B, None), (1, 4, 4, _A, -1, _B, _C), (65536, 4, 4, _A, 3, _B, _C)]:
        assert dec(*args, None) == _EINVAL, args
        assert b"cppf_rle_decode: invalid argument" in lib.cppf_last_error_string()
    need = lib.cppf_mask_components_workspace_bytes
    assert need(2, 3, 5) == 256 + 2 * 15 * 8 and need(64, 480, 640) == 512 + 64 * 480 * 640 * 8
    assert need(0, 3, 5) == need(-1, 3, 5) == need(2, 0, 5) == need(2, 3, 8193) == need(65536, 3, 5) == 0
    cc = lib.cppf_mask_components

    def call(D=2, I=1, H=3, W=5, masks=_A, depths=_B, idx=_C, jump=0.01, min_pixels=1, out=_D, stats=_E, ws=_F, short=0):
        return cc(D, I, H, W, masks, depths, idx, C.c_float(jump), min_pixels, out, stats, ws, need(max(D, 1), H, W) - short, None)
    assert call(D=0) == _OK and call(D=0, masks=None, depths=None, idx=None, out=None, stats=None, ws=None) == _OK
    for kw in [dict(D=-1), dict(I=0), dict(H=0), dict(W=8193), dict(masks=None), dict(depths=None), dict(idx=None), dict(out=None),
               dict(stats=None), dict(ws=None), dict(ws=_F + 4), dict(short=1), dict(jump=-1e-6), dict(jump=float("nan")),
               dict(jump=float("inf")), dict(min_pixels=-1)]:
        assert call(**kw) == _EINVAL, kw
        assert b"cppf_mask_components: invalid argument" in lib.cppf_last_error_string()


def test_masks_clean_and_decode_refuse_bad_input_before_any_launch():
    import torch
    from cppf2_amd import masks, ops
    with pytest.raises(masks.RleError):
        masks.decode_batch([[12], [5, -1, 8]], 3, 4)
    with pytest.raises(masks.RleError):
        masks.decode_batch([[12], [11]], 3, 4)
    with pytest.raises(masks.RleError):
        masks.decode_batch(["<o"], 3, 4)
    for jump in (-0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            masks.clean(np.ones((1, 3, 4), np.uint8), np.ones((3, 4), np.float32), 0, jump=jump)
    if not torch.cuda.is_available():
        with pytest.raises(ops.CppfError):                  # no CPU fallback
            masks.decode_batch([[12]], 3, 4)


# ---- the restatement on hand-drawn cases --------------------------------------------------------------------------------------
JUMP = 0.0078125                                            # 2^-7: a float32 value; 1 + 2^-7 is one too
NEAR, FAR = np.float32(1.0), np.float32(1.0078125)


def _two_blobs(bridge):
    """3 x 5: blob A = columns 0-1 at 1.0, blob B = columns 3-4 at 1 + 2^-7, column 2 set only in row 1, at depth `bridge`."""
    mask = np.ones((3, 5), np.uint8)
    mask[0, 2] = mask[2, 2] = 0
    depth = np.empty((3, 5), np.float32)
    depth[:, :2], depth[:, 2], depth[:, 3:] = NEAR, bridge, FAR
    return mask, depth


def test_restatement_joins_at_exactly_jump_and_splits_one_ulp_above():
    assert np.float32(JUMP) == JUMP and FAR - NEAR == np.float32(JUMP)
    # the pair (1, 1) -- (1, 2) differs by exactly jump: one component of all 13 pixels, label 0
    mask, depth = _two_blobs(FAR)
    out, stats = MR.components(mask, depth, JUMP, 1)
    assert stats.tolist() == [1, 0, 13, 13] and np.array_equal(out, mask * 255)
    # one ulp more: the bridge pixel leaves A (6 pixels, label 0) and stays with B (2^-23 away): B has 7 pixels, label (0, 3) = 3
    up = np.nextafter(FAR, np.float32(2))
    assert up - NEAR > np.float32(JUMP) and np.float32(up - NEAR) == up - NEAR
    mask, depth = _two_blobs(up)
    out, stats = MR.components(mask, depth, JUMP, 1)
    want = np.zeros((3, 5), np.uint8)
    want[:, 3:] = 255
    want[1, 2] = 255
    assert stats.tolist() == [2, 3, 7, 13] and np.array_equal(out, want)
    lab, sizes = MR.labels(mask, depth, JUMP)
    assert sizes == {0: 6, 3: 7} and lab[1, 2] == 3 and lab[2, 1] == 0
    # min_pixels above both: nothing kept
    out, stats = MR.components(mask, depth, JUMP, 8)
    assert stats.tolist() == [2, -1, 0, 13] and not out.any()


def test_restatement_size_tie_goes_to_the_lowest_label_and_invalid_depth_is_no_pixel():
    mask = np.array([[0, 1, 1, 0, 1, 1],
                     [1, 0, 0, 0, 0, 0],
                     [1, 0, 1, 1, 1, 0]], np.uint8)
    depth = np.ones((3, 6), np.float32)
    # components: {1, 2}, {4, 5}, {6, 12}, {14, 15, 16}
    out, stats = MR.components(mask, depth, 0.0, 1)
    assert stats.tolist() == [4, 14, 3, 9] and out[2, 2:5].tolist() == [255] * 3 and out.sum() == 3 * 255
    depth[2, 3] = np.nan                                     # the triple falls apart: {14}, {16}; three pairs tie, label 1 wins
    out, stats = MR.components(mask, depth, 0.0, 1)
    assert stats.tolist() == [5, 1, 2, 8] and out[0, 1:3].tolist() == [255, 255] and out.sum() == 2 * 255
    for bad in (0.0, -1.0, np.inf, -np.inf):
        depth[0, 1] = bad                                    # {2} alone: the next pair by label is {4, 5}
        out, stats = MR.components(mask, depth, 0.0, 1)
        assert stats.tolist() == [5, 4, 2, 7], (bad, stats)
    # a checkerboard: every component one pixel, the lowest label wins
    cb = (np.add.outer(np.arange(4), np.arange(5)) % 2 == 1).astype(np.uint8)
    out, stats = MR.components(cb, np.ones((4, 5), np.float32), 1.0, 1)
    assert stats.tolist() == [10, 1, 1, 10] and out[0, 1] == 255 and out.sum() == 255
