"""GPU checks of the wrappers' shared argument helpers (cppf2_amd/hostargs.py): masks.clean,
segment.segments, verify.fit_counts and scene.explain give the same bytes whichever form the depth image and the mask come in,
and those bytes are the restatements' (tests/mask_ref.py, segment_ref.py, verify_ref.py, scene_ref.py); scratch by stream."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import mask_ref as MR  # noqa: E402
import scene_ref as SC  # noqa: E402
import segment_ref as SR  # noqa: E402
import verify_ref as VR  # noqa: E402

F = np.float32
# one 4 x 6 image: a near surface and one 5 cm behind it, one pixel without a reading
DEPTH = np.array([[1.00, 1.00, 1.00, 1.05, 1.05, 1.05],
                  [1.00, 1.00, 0.00, 1.05, 1.05, 1.05],
                  [1.00, 1.00, 1.00, 1.00, 1.05, 1.05],
                  [1.00, 1.00, 1.00, 1.00, 1.00, 1.00]], np.float64)
MASK = np.array([[1, 1, 0, 1, 1, 0],
                 [1, 1, 1, 1, 1, 0],
                 [0, 0, 1, 0, 1, 1],
                 [1, 0, 0, 0, 0, 1]], bool)
# two renders: the near surface's left part (one pixel 10 cm in front: a violation), and the far surface with a slight offset
RENDERS = np.zeros((2, 4, 6), F)
RENDERS[0, :, :3] = 1.0
RENDERS[0, 3, 0] = 0.9
RENDERS[1, :3, 3:] = 1.06
TAU = 0.02
JUMP = 0.01


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _forms(dev):
    """[(name, depth, mask)]: every depth form with every mask form."""
    import torch
    d32 = DEPTH.astype(F)
    depths = [("host float64", DEPTH), ("device float32", torch.from_numpy(d32).to(dev)),
              ("device transposed view", torch.from_numpy(np.ascontiguousarray(d32.T)).to(dev).T)]
    masks = [("host bool", MASK), ("device 0/255", torch.from_numpy(MASK.astype(np.uint8) * 255).to(dev)),
             ("device bool", torch.from_numpy(MASK).to(dev))]
    assert tuple(depths[2][1].shape) == (4, 6) and not depths[2][1].is_contiguous()
    return [(dn + ", " + mn, d, m) for dn, d in depths for mn, m in masks]


def _same(outs, want, what):
    """Every form's outputs (tuples of device tensors) equal `want` (host arrays), bytes and dtypes."""
    for name, got in outs:
        for k, (g, w) in enumerate(zip(got, want)):
            g = g.cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name, k, g.tolist(), w.tolist())


def test_clean_takes_every_form():
    from cppf2_amd import masks
    dev = _gpu()
    want_mask, want_stats = MR.components(MASK, DEPTH.astype(F), JUMP, 2)
    assert want_stats[0] >= 3 and 0 < want_stats[2] < want_stats[3]             # several components, one of them kept
    outs = [(name, masks.clean(m, d, 0, jump=JUMP, min_pixels=2)) for name, d, m in _forms(dev)]
    _same(outs, (want_mask[None], np.asarray(want_stats, np.int32)[None]), "masks.clean")


def test_segments_take_every_form():
    from cppf2_amd import segment
    dev = _gpu()
    rank, seg, stats = SR.segments(MASK, DEPTH.astype(F), JUMP, 2, 3)
    assert stats[1] >= 2 and stats[0] > stats[2]                                # two ranks at least, and components too small
    outs = [(name, segment.segments(m, d, 0, jump=JUMP, min_pixels=2, max_segments=3)) for name, d, m in _forms(dev)]
    _same(outs, (rank[None], seg[None], stats[None]), "segment.segments")


def test_fit_counts_take_every_form():
    import torch
    from cppf2_amd import verify
    dev = _gpu()
    want = VR.fit_counts(DEPTH.astype(F)[None], MASK[None], [0, 2], RENDERS, (TAU,))
    assert want[:, 2].sum() > 0 and want[:, 3].sum() > 0 and (want[:, 4] > 0).all()   # violations, unexplained pixels, fits
    ren = torch.from_numpy(RENDERS).to(dev)
    outs = [(name, (verify.fit_counts(d, m, [0, 2], ren, (TAU,)),)) for name, d, m in _forms(dev)]
    _same(outs, (want,), "verify.fit_counts")


def test_explain_takes_every_form():
    import torch
    from cppf2_amd import scene
    dev = _gpu()
    keys = ("chosen", "gain", "net", "static", "labels", "summary")
    ref = SC.explain(DEPTH.astype(F), MASK, [0, 2], RENDERS, F(TAU), 1, 1, 3)
    assert ref["summary"][0, 2] == 2 and ref["static"][:, 2].sum() > 0           # both candidates win a round; a violation counted
    ren = torch.from_numpy(RENDERS).to(dev)
    outs = []
    for name, d, m in _forms(dev):
        got = scene.explain(d, m, [0, 2], ren, TAU, 1, 1, 3)
        outs.append((name, tuple(got[k] for k in keys)))
    _same(outs, tuple(ref[k] for k in keys), "scene.explain")


def test_scratch_is_per_stream():
    import torch
    from cppf2_amd import hostargs
    dev = _gpu()
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    with torch.cuda.stream(s1):
        k1 = hostargs.stream_key(dev)
    with torch.cuda.stream(s2):
        k2 = hostargs.stream_key(dev)
        assert hostargs.stream_key("cuda") == k2                   # "cuda" and "cuda:<current>" are one device
    assert k1 != k2 and k1[0] == k2[0] == dev.index and hostargs.stream_key(dev) not in (k1, k2)
    cache = hostargs.ScratchCache("entry_workspace_bytes", RuntimeError)
    a, b = cache.get(k1, 4096, dev), cache.get(k2, 4096, dev)
    assert a.device == b.device == dev and a.numel() >= 4096 and b.numel() >= 4096
    assert a.data_ptr() + a.numel() <= b.data_ptr() or b.data_ptr() + b.numel() <= a.data_ptr()
    assert cache.get(k1, 100, dev) is a and cache.get(k2, 100, dev) is b
