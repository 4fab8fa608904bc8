"""CPU checks of the wrappers' shared argument and scratch helpers (cppf2_amd/hostargs.py) on
torch.device("cpu"): what they accept, what they return and what they refuse, with no library and no GPU; and the record
helpers next to RESULT_DTYPE (cppf2_amd/pipeline.py), which need the built library to import."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cppf2_amd import hostargs as HA  # noqa: E402

CPU = torch.device("cpu")


def test_the_module_needs_no_library():
    """A fresh interpreter that imports hostargs has loaded no other module of the package, and no shared library of it."""
    code = ("import sys, cppf2_amd.hostargs\n"
            "mods = sorted(m for m in sys.modules if m.startswith('cppf2_amd.') and m != 'cppf2_amd.hostargs')\n"
            "maps = [l for l in open('/proc/self/maps') if 'libcppf_hip' in l] if sys.platform == 'linux' else []\n"
            "assert not mods and not maps, (mods, maps)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- image batch ------------------------------------------------------------------------------------------------------------------
def test_image_batch_forms():
    a = np.arange(12, dtype=np.float64).reshape(3, 4) / 7.0
    t = HA.image_batch(a, CPU, "who")
    assert t.shape == (1, 3, 4) and t.dtype == torch.float32 and t.is_contiguous() and t.device == CPU
    assert np.array_equal(t.numpy()[0], a.astype(np.float32))
    b = torch.arange(24, dtype=torch.float32).reshape(4, 3, 2)
    v = b.permute(2, 1, 0)                                          # [2,3,4], not contiguous
    t = HA.image_batch(v, CPU, "who")
    assert not v.is_contiguous() and t.is_contiguous() and t.shape == (2, 3, 4) and torch.equal(t, v)
    v2 = torch.arange(24, dtype=torch.float32).reshape(6, 4).T      # the transpose of a [6,4] tensor
    t = HA.image_batch(v2, CPU, "who")
    assert t.is_contiguous() and t.shape == (1, 4, 6) and torch.equal(t[0], v2)
    c = torch.ones((2, 3, 4))
    assert HA.image_batch(c, CPU, "who").data_ptr() == c.data_ptr()  # what already is a batch is not copied
    assert HA.image_batch([[1, 2], [3, 4]], CPU, "who").tolist() == [[[1.0, 2.0], [3.0, 4.0]]]


@pytest.mark.parametrize("shape", [(8,), (2, 2, 3, 4), (0, 3, 4), (2, 0, 4), (2, 3, 0), (0, 4), (3, 0)])
def test_image_batch_refuses_ranks_and_empty_dimensions(shape):
    for x in (np.ones(shape, np.float32), torch.ones(shape)):
        with pytest.raises(ValueError, match="the_caller"):
            HA.image_batch(x, CPU, "the_caller")


def test_image_batch_limits():
    assert HA.image_batch(np.ones((5, 2, 3), np.float32), CPU, "who", max_images=5).shape == (5, 2, 3)
    with pytest.raises(ValueError, match="the_caller.*at most 5 images"):
        HA.image_batch(np.ones((6, 2, 3), np.float32), CPU, "the_caller", max_images=5)
    assert HA.image_batch(np.ones((7, 4), np.float32), CPU, "who", max_images=1, max_dim=7).shape == (1, 7, 4)
    assert HA.image_batch(np.ones((2, 4, 7), np.float32), CPU, "who", max_dim=7).shape == (2, 4, 7)
    for shape in ((8, 4), (4, 8), (2, 8, 4), (2, 4, 8)):
        with pytest.raises(ValueError, match="the_caller.*at most 7"):
            HA.image_batch(np.ones(shape, np.float32), CPU, "the_caller", max_dim=7)


# ---- mask batch -------------------------------------------------------------------------------------------------------------------
PATTERN = np.array([[[1, 0, 0, 1], [0, 0, 1, 1], [0, 1, 0, 0]], [[0, 0, 0, 0], [1, 1, 1, 1], [0, 0, 0, 1]]], dtype=bool)


def test_mask_batch_forms_agree():
    like = torch.zeros((2, 3, 4))
    forms = [PATTERN, PATTERN.astype(np.uint8), torch.from_numpy(PATTERN.astype(np.uint8) * 255), torch.from_numpy(PATTERN),
             PATTERN.astype(np.float32) * 0.5, torch.from_numpy(PATTERN.astype(np.int32) * 256)]
    for f in forms:
        for same in (False, True):
            m = HA.mask_batch(f, like, CPU, "who", same_shape=same)
            assert m.dtype == torch.uint8 and m.shape == (2, 3, 4) and m.is_contiguous() and m.device == CPU
            assert np.array_equal(m.numpy() != 0, PATTERN)
    u = torch.from_numpy(PATTERN.astype(np.uint8) * 255)
    assert HA.mask_batch(u, like, CPU, "who").data_ptr() == u.data_ptr()            # used as it is: no copy
    assert HA.mask_batch(u.reshape(6, 4), like, CPU, "who").data_ptr() == u.data_ptr()
    bt = torch.from_numpy(PATTERN)
    assert HA.mask_batch(bt, like, CPU, "who").data_ptr() == bt.data_ptr()          # a bool tensor's bytes are its mask
    nc = torch.from_numpy(np.ascontiguousarray(PATTERN.transpose(0, 2, 1)).astype(np.uint8)).permute(0, 2, 1)
    m = HA.mask_batch(nc, like, CPU, "who")
    assert not nc.is_contiguous() and m.is_contiguous() and np.array_equal(m.numpy() != 0, PATTERN)
    one = HA.mask_batch(PATTERN[0], torch.zeros((1, 3, 4)), CPU, "who", same_shape=True)     # [H,W] for a batch of one
    assert one.shape == (1, 3, 4) and np.array_equal(one.numpy()[0] != 0, PATTERN[0])
    assert HA.mask_batch(np.zeros((0, 3, 4), bool), like, CPU, "who").shape == (0, 3, 4)


class _Err(RuntimeError):
    pass


def test_mask_batch_refusals():
    like = torch.zeros((2, 3, 4))
    for bad in (np.ones((2, 3, 5), bool), torch.ones(13, dtype=torch.uint8), np.ones((3, 3), np.uint8)):
        with pytest.raises(ValueError, match="the_caller"):
            HA.mask_batch(bad, like, CPU, "the_caller")
    assert HA.mask_batch(np.ones((4, 3, 4), bool), like, CPU, "who").shape == (4, 3, 4)       # D need not be I ...
    for bad in (np.ones((4, 3, 4), bool), np.ones((1, 3, 4), bool), np.ones((3, 4), bool), torch.ones((2, 4, 3), dtype=torch.uint8),
                np.ones((2, 12), bool), np.ones((2, 3, 5), bool)):
        with pytest.raises(ValueError, match="the_caller"):                                     # ... unless the shapes must agree
            HA.mask_batch(bad, like, CPU, "the_caller", same_shape=True)
    with pytest.raises(_Err):
        HA.mask_batch(np.ones((4, 3, 4), bool), like, CPU, "who", same_shape=True, err=_Err)
    with pytest.raises(_Err):
        HA.mask_batch(np.ones(5, bool), like, CPU, "who", err=_Err)


# ---- per item ---------------------------------------------------------------------------------------------------------------------
def test_per_item():
    n = 4
    for x, want in ((3, [3] * 4), ([5, 6, 7, 8], [5, 6, 7, 8]), (torch.tensor([5, 6, 7, 8]), [5, 6, 7, 8]), (np.array([9]), [9] * 4),
                    (np.int64(2), [2] * 4), (torch.tensor([[5, 6], [7, 8]], dtype=torch.int16), [5, 6, 7, 8])):
        t = HA.per_item(x, n, torch.int32, CPU, "who")
        assert t.dtype == torch.int32 and t.shape == (n,) and t.is_contiguous() and t.tolist() == want
    f = HA.per_item(0.1, 3, torch.float32, CPU, "who")
    assert f.dtype == torch.float32 and f.numpy().tolist() == [np.float32(0.1)] * 3
    for bad in ([1, 2, 3], [1, 2, 3, 4, 5], np.arange(3), np.arange(5), []):
        with pytest.raises(ValueError, match="the_caller"):
            HA.per_item(bad, n, torch.int32, CPU, "the_caller")
    for bad in (torch.arange(3), torch.arange(5), torch.arange(1)):
        with pytest.raises(ValueError, match="the_caller"):
            HA.per_item(bad, n, torch.int32, CPU, "the_caller")
        with pytest.raises(_Err):                                   # a tensor's length is refused with the caller's error
            HA.per_item(bad, n, torch.int32, CPU, "who", err=_Err)
    with pytest.raises(ValueError):                                 # a host argument's always with ValueError
        HA.per_item([1, 2, 3], n, torch.int32, CPU, "who", err=_Err)
    for x in (7, [], np.zeros(0, np.int64), torch.zeros(0, dtype=torch.int32), [7]):
        assert HA.per_item(x, 0, torch.int32, CPU, "who").shape == (0,)
    with pytest.raises(ValueError):
        HA.per_item([1, 2], 0, torch.int32, CPU, "who")


def test_camera4():
    k = HA.camera4([[500.5, 0, 3.25], [0, 501.0, 2.0], [0, 0, 1]])
    assert list(k) == [500.5, 501.0, 3.25, 2.0] and len(bytes(k)) == 32
    assert list(HA.camera4(np.arange(9.0))) == [0.0, 4.0, 2.0, 5.0]
    with pytest.raises(ValueError):
        HA.camera4([1.0, 2.0, 3.0, 4.0])


# ---- records ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3,), (2, 2)])
def test_records_go_to_bytes_and_back(shape):
    from cppf2_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):                           # decided without loading anything: a library that is there
        pytest.skip("cppf2_amd.pipeline needs the built library, %s is absent" % _lib.LIB_PATH)     # but broken is a failure
    from cppf2_amd import pipeline
    n = int(np.prod(shape))
    raw = ((np.arange(n * 160) * 7 + 3) % 251).astype(np.uint8)     # distinct bytes within every record and field
    rec = raw.view(pipeline.RESULT_DTYPE).reshape(shape).copy()
    b = pipeline.record_bytes(rec, CPU)
    assert b.dtype == torch.uint8 and b.shape == (n, 160) and b.is_contiguous() and b.numpy().tobytes() == raw.tobytes()
    b.numpy()[0, 0] ^= 1                                            # a copy: the records do not change with it
    assert rec.tobytes() == raw.tobytes()
    b.numpy()[0, 0] ^= 1
    back = pipeline.records_of(b, shape)
    assert back.dtype == pipeline.RESULT_DTYPE and back.shape == shape
    for name in pipeline.RESULT_DTYPE.names:                        # bytes, not values: the random floats include NaNs
        assert np.ascontiguousarray(back[name]).tobytes() == np.ascontiguousarray(rec[name]).tobytes(), name
    assert pipeline.records_of(b).shape == (n,) and pipeline.records_of(b.reshape(shape + (160,))).tobytes() == raw.tobytes()
    part = pipeline.record_bytes(rec.reshape(-1)[::2], CPU)         # a strided view of records
    assert part.numpy().tobytes() == raw.reshape(n, 160)[::2].tobytes()
    assert pipeline.record_bytes(raw.reshape(n, 160), CPU).numpy().tobytes() == raw.tobytes()       # the records' bytes, as before


# ---- scratch ----------------------------------------------------------------------------------------------------------------------
def test_scratch_cache_reuses_grows_and_evicts():
    dropped = []
    c = HA.ScratchCache("entry_workspace_bytes", _Err, max_entries=3, on_drop=dropped.append)
    a = c.get((0, 1), 100, CPU)
    assert a.dtype == torch.uint8 and a.numel() >= 100 and a.device == CPU
    assert c.get((0, 1), 40, CPU) is a and c.get((0, 1), 100, CPU) is a and dropped == []
    big = c.get((0, 1), 101, CPU)
    assert big is not a and big.numel() >= 101 and dropped == [(0, 1)]
    assert c.get((0, 1), 0, CPU) is big and c[(0, 1)] is big
    with pytest.raises(_Err, match="entry_workspace_bytes"):        # a refused size: nothing is dropped or allocated
        c.get((0, 1), -1, CPU)
    assert c[(0, 1)] is big and dropped == [(0, 1)]
    c.get((0, 2), 8, CPU)
    c.get((0, 3), 8, CPU)
    assert c.get((0, 1), 8, CPU) is big                             # touched: now the newest
    c.get((0, 4), 8, CPU)                                           # a fourth key: the oldest, (0, 2), goes
    assert dropped == [(0, 1), (0, 2)] and list(c.buffers) == [(0, 3), (0, 1), (0, 4)]
    assert c.get((0, 1), 8, CPU) is big
    assert c.get((0, 5), 0, CPU).numel() == 0 and dropped == [(0, 1), (0, 2), (0, 3)]
    c.clear()
    assert not c.buffers and sorted(dropped[3:]) == [(0, 1), (0, 4), (0, 5)]
    quiet = HA.ScratchCache("entry", _Err)                                       # no callback; the default bound
    for k in range(HA.WS_CACHE_MAX + 1):
        quiet.get(k, 1, CPU)
    assert list(quiet.buffers) == list(range(1, HA.WS_CACHE_MAX + 1))


def test_one_shot_scratch():
    s = HA.scratch(24, CPU, "entry_workspace_bytes", _Err)
    assert s.dtype == torch.uint8 and s.numel() == 24 and s.device == CPU
    assert HA.scratch(0, CPU, "entry_workspace_bytes", _Err).numel() == 1
    assert HA.scratch(np.int64(5), CPU, "entry_workspace_bytes", _Err).numel() == 5
    with pytest.raises(_Err, match="entry_workspace_bytes"):
        HA.scratch(-1, CPU, "entry_workspace_bytes", _Err)
