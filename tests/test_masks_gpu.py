"""GPU checks of the mask kernels: cppf_rle_decode equal to the host decode byte for byte on every shape and on a mask whose
runs overflow one LDS pass; cppf_mask_components equal to the breadth-first restatement (tests/mask_ref.py) on mask bytes and
all four stats; both byte-identical alone, batched (D = 64) and in reversed order."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mask_ref as MR  # noqa: E402

SHAPES = [(480, 640), (37, 53), (1, 1), (3, 1021), (33, 4)]


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _blobs(rng, H, W, n=6):
    """A union of n random discs and boxes."""
    rr, cc = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for _ in range(n):
        r0, c0 = rng.integers(0, H), rng.integers(0, W)
        a, b = rng.integers(1, max(2, H // 4) + 1), rng.integers(1, max(2, W // 4) + 1)
        m |= (((rr - r0) / a) ** 2 + ((cc - c0) / b) ** 2 <= 1) if rng.random() < 0.5 else ((abs(rr - r0) <= a) & (abs(cc - c0) <= b))
    return m


def _decode_masks(rng, H, W):
    out = [_blobs(rng, H, W), rng.random((H, W)) < 0.5, np.zeros((H, W), bool), np.ones((H, W), bool)]
    first = np.zeros((H, W), bool)
    first[0, 0] = True
    last = np.zeros((H, W), bool)
    last[-1, -1] = True
    rows = (np.arange(H)[:, None] + np.zeros((1, W), int)) % 2 == 0          # one-pixel runs down every column
    return out + [first, last, rows]


@pytest.mark.parametrize("shape", SHAPES)
def test_decode_equals_the_host_decode(shape):
    _gpu()
    from cppf2_amd import masks
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    ms = _decode_masks(rng, H, W)
    counts = [masks.rle_encode(m) for m in ms]
    if H * W > 5000:
        assert max(len(c) for c in counts) > 3 * 2048, "no mask overflows one LDS pass of 2048 runs"
        assert len(masks.rle_encode(ms[-1])) > 100000                   # thousands of one-pixel runs
    got = masks.decode_batch(counts, H, W).cpu().numpy()
    for n, (m, c) in enumerate(zip(ms, counts)):
        want = masks.rle_decode(c, H, W)
        assert np.array_equal(want, np.where(m, 255, 0))
        print("decode", shape, "mask", n, "runs", len(c), "differing bytes", int((got[n] != want).sum()))
        assert got[n].tobytes() == want.tobytes(), (shape, n)
    # the compressed string goes the same way, and list and string forms mix in one call
    mixed = [masks.counts_to_string(c) if n % 2 else c for n, c in enumerate(counts)]
    assert masks.decode_batch(mixed, H, W).cpu().numpy().tobytes() == got.tobytes()
    assert masks.decode_batch([], H, W).shape == (0, H, W)


def test_decode_alone_batched_and_reversed_are_byte_identical():
    _gpu()
    from cppf2_amd import masks
    H, W = 120, 161                                                     # H * W odd: masks start at every byte alignment
    rng = np.random.default_rng(5)
    ms = [_blobs(rng, H, W, 1 + n % 5) if n % 8 else rng.random((H, W)) < 0.5 for n in range(64)]
    counts = [masks.rle_encode(m) for m in ms]
    assert max(len(c) for c in counts) > 2048
    batch = masks.decode_batch(counts, H, W).cpu().numpy()
    rev = masks.decode_batch(counts[::-1], H, W).cpu().numpy()
    for n in range(64):
        alone = masks.decode_batch([counts[n]], H, W).cpu().numpy()[0]
        assert alone.tobytes() == batch[n].tobytes() == rev[63 - n].tobytes() == np.where(ms[n], 255, 0).astype(np.uint8).tobytes(), n


# ---- components -----------------------------------------------------------------------------------------------------------------
def _stepped(rng, H, W, step=0.03):
    """Depth in plateaus with jumps of `step` between them and a gentle ramp inside each."""
    rr, cc = np.mgrid[0:H, 0:W]
    plate = (rr // max(H // 5, 1) + 2 * (cc // max(W // 4, 1))) % 4
    return (0.8 + step * plate + 1e-4 * (rr + cc) / max(H + W, 1) * 10 + 1e-5 * rng.random((H, W))).astype(np.float32)


def _serpentine(H, W):
    """A one-pixel-wide path that fills the image: every other row whole, joined at alternating ends."""
    m = np.zeros((H, W), bool)
    m[0::2] = True
    for k, r in enumerate(range(1, H, 2)):
        m[r, -1 if k % 2 == 0 else 0] = True
    return m


def _check(masks_np, depth, idx, jump, min_pixels, what):
    from cppf2_amd import masks
    out, stats = masks.clean(masks_np, depth, idx, jump=jump, min_pixels=min_pixels)
    out, stats = out.cpu().numpy(), stats.cpu().numpy()
    d3 = depth if depth.ndim == 3 else depth[None]
    idx = np.broadcast_to(np.asarray(idx), (len(masks_np),))
    for n, m in enumerate(masks_np):
        if 0 <= idx[n] < len(d3):
            want, wstats = MR.components(m, d3[idx[n]], jump, min_pixels)
        else:
            want, wstats = np.zeros(m.shape, np.uint8), np.array([0, -1, 0, 0], np.int32)
        print(what, "mask", n, "stats", stats[n].tolist(), "want", wstats.tolist(), "differing bytes", int((out[n] != want).sum()))
        assert stats[n].tolist() == wstats.tolist(), (what, n)
        assert out[n].tobytes() == want.tobytes(), (what, n)
    return out, stats


@pytest.mark.parametrize("shape", SHAPES)
def test_components_equal_the_restatement(shape):
    _gpu()
    H, W = shape
    rng = np.random.default_rng(7 * H + W)
    depth = _stepped(rng, H, W)
    ms = [_blobs(rng, H, W), _blobs(rng, H, W, 12), np.ones((H, W), bool), np.zeros((H, W), bool)]
    ms.append(_serpentine(H, W))
    ms.append(np.add.outer(np.arange(H), np.arange(W)) % 2 == 1)           # a checkerboard
    ms.append(rng.random((H, W)) < 0.6)
    ms = np.stack(ms)
    out, stats = _check(ms, depth, 0, 0.01, 1, "stepped %s" % (shape,))
    assert not out[3].any() and stats[3].tolist() == [0, -1, 0, 0]          # the empty mask
    if H * W > 1:
        n_cb = int(ms[5].sum())
        assert stats[5].tolist() == [n_cb, int(np.flatnonzero(ms[5].reshape(-1))[0]), 1, n_cb]
    # the serpentine on a flat depth: one component of every set pixel, whatever the path's length
    flat = np.full((H, W), 1.25, np.float32)
    out, stats = _check(ms[4:5], flat, 0, 0.01, 1, "serpentine %s" % (shape,))
    assert stats[0].tolist() == [1, 0, int(ms[4].sum()), int(ms[4].sum())] and np.array_equal(out[0] > 0, ms[4])
    # min_pixels above the largest component: nothing kept, the counts stay
    big = int(stats[0][2]) + 1
    out, stats2 = _check(ms[4:5], flat, 0, 0.01, big, "min_pixels %s" % (shape,))
    assert stats2[0].tolist() == [1, -1, 0, int(ms[4].sum())] and not out.any()


def test_components_with_invalid_depth_bad_indices_and_shared_images():
    _gpu()
    H, W = 96, 131
    rng = np.random.default_rng(21)
    depth = np.stack([_stepped(rng, H, W), _stepped(rng, H, W, 0.004), _stepped(rng, H, W)])
    holes = rng.random((H, W))
    depth[2][holes < 0.10] = 0.0
    depth[2][(holes >= 0.10) & (holes < 0.15)] = np.nan
    depth[2][(holes >= 0.15) & (holes < 0.20)] = np.inf
    depth[2][(holes >= 0.20) & (holes < 0.22)] = -1.0
    depth[2][(holes >= 0.22) & (holes < 0.24)] = -np.inf
    ms = np.stack([_blobs(rng, H, W, 8) for _ in range(9)])
    idx = np.array([2, 2, 0, 1, 1, 3, -1, 2, 0], dtype=np.int32)            # several masks per image; 3 and -1 lie outside [0, I)
    out, stats = _check(ms, depth, idx, 0.01, 4, "invalid depth")
    assert stats[5].tolist() == stats[6].tolist() == [0, -1, 0, 0] and not out[5].any() and not out[6].any()
    assert stats[0][3] < ms[0].sum()                                        # pixels without a usable depth are not valid
    # exactly jump apart joins, one ulp more does not (tests/test_masks.py draws the case)
    near, far = np.float32(1.0), np.float32(1.0078125)
    m = np.ones((1, 3, 5), np.uint8)
    m[0, 0, 2] = m[0, 2, 2] = 0
    d = np.empty((3, 5), np.float32)
    d[:, :2], d[:, 2], d[:, 3:] = near, far, far
    _, st = _check(m, d, 0, 0.0078125, 1, "exactly jump")
    assert st[0].tolist() == [1, 0, 13, 13]
    d[:, 2] = np.nextafter(far, np.float32(2))
    _, st = _check(m, d, 0, 0.0078125, 1, "one ulp above jump")
    assert st[0].tolist() == [2, 3, 7, 13]


def test_components_alone_batched_and_reversed_are_byte_identical():
    import torch
    _gpu()
    from cppf2_amd import masks
    H, W = 120, 161
    rng = np.random.default_rng(9)
    depth = np.stack([_stepped(rng, H, W), _stepped(rng, H, W, 0.008)])
    ms = np.stack([_blobs(rng, H, W, 2 + n % 7) if n % 9 else _serpentine(H, W) for n in range(64)])
    idx = (np.arange(64) % 2).astype(np.int32)
    out, stats = masks.clean(ms, depth, idx, jump=0.01, min_pixels=8)
    out2, stats2 = masks.clean(ms, depth, idx, jump=0.01, min_pixels=8)     # the same call again: no dependence on the schedule
    rout, rstats = masks.clean(ms[::-1].copy(), depth, idx[::-1].copy(), jump=0.01, min_pixels=8)
    out, stats, rout, rstats = out.cpu().numpy(), stats.cpu().numpy(), rout.cpu().numpy(), rstats.cpu().numpy()
    assert out2.cpu().numpy().tobytes() == out.tobytes() and stats2.cpu().numpy().tobytes() == stats.tobytes()
    for n in range(64):
        a, s = masks.clean(ms[n:n + 1], depth, idx[n:n + 1], jump=0.01, min_pixels=8)
        assert a.cpu().numpy()[0].tobytes() == out[n].tobytes() == rout[63 - n].tobytes(), n
        assert s.cpu().numpy()[0].tobytes() == stats[n].tobytes() == rstats[63 - n].tobytes(), n
    for n in (0, 1, 9, 10, 63):                                             # and the batch is the restatement's
        want, wstats = MR.components(ms[n], depth[idx[n]], 0.01, 8)
        assert out[n].tobytes() == want.tobytes() and stats[n].tolist() == wstats.tolist(), n
    # device tensors in, and the output may be fed back: cleaning a cleaned mask changes nothing
    again, st = masks.clean(torch.from_numpy(out).cuda(), torch.from_numpy(depth).cuda(), torch.from_numpy(idx).cuda(), 0.01, 8)
    assert again.cpu().numpy().tobytes() == out.tobytes()
    assert np.array_equal(st.cpu().numpy()[:, 2], stats[:, 2])
