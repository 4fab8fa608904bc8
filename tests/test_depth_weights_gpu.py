"""GPU checks of cppf_depth_weights: weights and counts equal to the integers of the NumPy restatement
(tests/depth_weights_ref.py) at every image size, step and batch at which the kernel takes another path -- one tile, partial
tiles, rows whose address is and is not a multiple of four (the packed store), ragged tails --, its call hygiene, and the
wrapper.  Readings lie in 0.05 .. 10 m, so that no product is denormal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import depth_condition_ref as DR  # noqa: E402
import depth_weights_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64                       # canary elements on either side of both outputs
CANARY_B, CANARY_I = 0xA5, -77
SIZES = [(1, 1), (1, 200), (200, 1), (16, 64), (17, 65), (33, 130), (48, 193)]
K4 = R.PLANE_K4


def lattice(seed, I, H, W, dead=None):
    """depth_condition_ref's lattice images (patches around 0.5 m, holes, dead rows) with the denormal reading replaced by
    0.05 m: valid, far from every neighbour, and no product of it is denormal."""
    d = DR.lattice_images(seed, I, H, W, dead=dead)
    d[(d > 0) & (d < F(1e-30))] = F(0.05)
    if H > 8:
        d[:, 5] = 0.0                                                                   # a dead row
    return d


def dev_weights(img, K4=K4, po=0.0, step=1, jump=0.01, rel=0.0, levels=16, cos_min=0.2, shift=0):
    """cppf_depth_weights itself on a host array [I,H,W], both outputs between canaries that must survive; `shift` moves the
    weights' first byte off the allocation's alignment.  The input must keep its bytes."""
    import torch
    from cppf2_amd import _lib, ops
    dev, L = ops._dev(), _lib.load()
    img = np.ascontiguousarray(img, dtype=F)
    I, H, W = img.shape
    d = torch.from_numpy(img).to(dev)
    n = I * H * W
    out = torch.full((n + 2 * GUARD + 8,), CANARY_B, dtype=torch.uint8, device=dev)
    cnt = torch.full((3 * I + 2 * GUARD,), CANARY_I, dtype=torch.int32, device=dev)
    a = GUARD + shift
    o, c = out[a:a + n], cnt[GUARD:GUARD + 3 * I]
    _lib.check(L.cppf_depth_weights(ops._p(d), I, H, W, (C.c_double * 4)(*K4), C.c_float(po), step, C.c_float(jump), C.c_float(rel),
                                    levels, C.c_float(cos_min), ops._p(o), ops._p(c), ops._stream()), "cppf_depth_weights")
    assert bool((out[:a] == CANARY_B).all()) and bool((out[a + n:] == CANARY_B).all()), "a canary byte was overwritten"
    assert bool((cnt[:GUARD] == CANARY_I).all()) and bool((cnt[-GUARD:] == CANARY_I).all()), "a canary count was overwritten"
    assert d.cpu().numpy().tobytes() == img.tobytes()
    return o.cpu().numpy().reshape(I, H, W), c.cpu().numpy().reshape(I, 3).astype(np.int64)


def assert_equal(img, **kw):
    ref = {dict(po="pixel_offset", rel="jump_rel").get(k, k): v for k, v in kw.items() if k != "shift"}
    want, want_counts = R.weights(img, ref.pop("K4", K4), **ref)
    got, counts = dev_weights(img, **kw)
    assert got.dtype == np.uint8 and np.array_equal(got, want), (kw, int((got != want).sum()))
    assert counts.tolist() == want_counts.tolist(), kw
    return want, want_counts


@pytest.mark.parametrize("H,W", SIZES)
def test_every_size_step_and_batch_equals_the_restatement(H, W):
    seen = np.zeros(3, np.int64)
    for I in (1, 2, 5):
        img = lattice(100 * H + W + I, I, H, W, dead=I // 2 if I > 1 else None)
        whole = None
        for s in (1, 2, 3, 4):
            want, counts = assert_equal(img, step=s, jump=2.0 ** -7, shift=(s + I) % 4)
            seen += counts.sum(0)
            assert I == 1 or counts[I // 2].tolist() == [0, 0, 0]                       # the all-invalid image in the middle
            whole = (want, counts) if s == 1 else whole
        if I == 5:                                                                      # a batch equals separate calls
            for i in range(I):
                got, c = dev_weights(img[i:i + 1], step=1, jump=2.0 ** -7)
                assert np.array_equal(got[0], whole[0][i]) and c[0].tolist() == whole[1][i].tolist()
    assert seen[0] > 0 and (min(H, W) < 3 or seen[2] + seen[1] > 0), seen


@pytest.mark.parametrize("degrees,axis", [(30, "x"), (60, "y"), (75, "x"), (-60, "y")])
def test_tilted_planes_levels_thresholds_and_offsets(degrees, axis):
    """The tilted planes of the CPU test, at 33 x 130 and 48 x 193 (four-pixel packing with a ragged tail), every alignment of
    the first byte, jump_rel, cos_min on and off a level boundary, 1, 16 and 255 levels, both pixel offsets."""
    for (H, W), s in (((33, 130), 1), ((48, 193), 2)):
        k = (600.0, 600.0, W / 2 - 0.5, H / 2 - 0.5)                                   # 9 degrees to either side: the plane stays in front
        depth, cos = R.tilted_plane(H, W, degrees, axis, K4=k)
        assert (depth > 0.05).all() and (depth < 10).all()
        for shift in range(4):
            want, counts = assert_equal(depth[None], K4=k, step=s, jump=10.0, cos_min=0.0, shift=shift)
        lo, hi = R.expected_levels(cos, 16)
        got = want[0][s:H - s, s:W - s].astype(np.int64)
        assert ((got == lo[s:H - s, s:W - s]) | (got == hi[s:H - s, s:W - s])).all()
        for kw in (dict(levels=1), dict(levels=255), dict(cos_min=8.5 / 16), dict(cos_min=0.5), dict(jump=0.01, rel=0.02), dict(po=0.5),
                   dict(jump=0.01)):
            assert_equal(depth[None], **dict(dict(K4=k, step=s, jump=10.0, cos_min=0.2), **kw))


def test_more_images_than_the_grid_has_rows_for():
    """70 000 images of 3 x 5 pixels: the grid's second dimension holds 65 535, so the first 4 465 blocks take a second image."""
    img = lattice(7, 70000, 3, 5)
    assert_equal(img, jump=2.0 ** -7)


def test_no_images_is_valid_and_refusals_write_nothing():
    import torch
    from cppf2_amd import _lib, ops
    img = lattice(3, 3, 35, 127, dead=2)
    dev, L = ops._dev(), _lib.load()
    d = torch.from_numpy(img).to(dev)
    out = torch.full(img.shape, CANARY_B, dtype=torch.uint8, device=dev)
    cnt = torch.full((3, 3), CANARY_I, dtype=torch.int32, device=dev)
    K = (C.c_double * 4)(*K4)
    nan, inf = float("nan"), float("inf")

    def call(depth=d, I=3, H=35, W=127, K=K, po=0.0, step=1, jump=0.01, rel=0.0, levels=16, cos_min=0.2, o=out, c=cnt):
        return L.cppf_depth_weights(ops._p(depth), I, H, W, K, C.c_float(po), step, C.c_float(jump), C.c_float(rel), levels,
                                    C.c_float(cos_min), ops._p(o), ops._p(c), ops._stream())
    assert call(I=0) == 0 and call(I=0, depth=None, o=None, c=None) == 0
    for kw in (dict(o=d.view(torch.uint8)), dict(o=d.view(torch.uint8).view(-1)[4 * img.size - 1:]), dict(depth=None), dict(o=None),
               dict(c=None), dict(K=None), dict(I=-1), dict(H=0), dict(W=16385), dict(H=16385), dict(step=0), dict(step=5),
               dict(levels=0), dict(levels=256), dict(cos_min=1.0), dict(cos_min=-0.1), dict(cos_min=nan), dict(jump=-1.0),
               dict(jump=nan), dict(jump=inf), dict(rel=-1.0), dict(rel=inf), dict(rel=nan), dict(po=nan), dict(po=inf)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((out == CANARY_B).all()) and bool((cnt == CANARY_I).all()) and d.cpu().numpy().tobytes() == img.tobytes()
    assert call() == 0 and call() == 0                                                  # two calls: the counts are cleared
    want, want_counts = R.weights(img, K4)
    assert np.array_equal(out.cpu().numpy(), want) and cnt.cpu().numpy().tolist() == want_counts.tolist()


def test_the_wrapper():
    import torch
    from cppf2_amd import depthweights as DW, ops
    img = lattice(5, 2, 33, 70)
    K = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]])
    w, counts = DW.weights(img, K)
    assert w.is_cuda and w.dtype == torch.uint8 and tuple(w.shape) == img.shape
    assert isinstance(counts, np.ndarray) and counts.dtype == np.int64 and counts.shape == (2, 3)
    want, want_counts = R.weights(img, K4)
    assert np.array_equal(w.cpu().numpy(), want) and counts.tolist() == want_counts.tolist()
    dev_img = torch.from_numpy(img[0]).to(ops._dev())
    w, counts = DW.weights(dev_img, K, 0.5, 2, 2.0 ** -7, 2.0 ** -6, 200, 0.4)           # [H,W], a device tensor
    want, want_counts = R.weights(img[:1], K4, 0.5, 2, 2.0 ** -7, 2.0 ** -6, 200, 0.4)
    assert np.array_equal(w.cpu().numpy(), want) and counts.tolist() == want_counts.tolist()
    assert dev_img.cpu().numpy().tobytes() == img[0].tobytes()
    s = DW.checked(2, 2.0 ** -7, 2.0 ** -6, 200, 0.4, 3)
    got, summary = DW.apply(img[:1], K, s, 0.5)
    assert np.array_equal(got.cpu().numpy(), want) and summary == DW.summary(s, want_counts) and summary["carve_weight"] == 3
    with pytest.raises(DW.CppfError):
        DW.weights(torch.from_numpy(img), K)
    with pytest.raises(ValueError):
        DW.weights(np.zeros((0, 4, 4), F), K)
    with pytest.raises(ValueError):
        DW.weights(img, K, step=5)
