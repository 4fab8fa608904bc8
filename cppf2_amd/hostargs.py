"""What the wrappers do between a caller's arguments and the C ABI: a depth image batch, a mask batch, a
value per item, the camera's four intrinsics, and scratch memory.  Every function takes its device, so all of it runs on
torch.device("cpu") as it does on the GPU; nothing here loads the library (the record helpers, which need RESULT_DTYPE, are
pipeline.record_bytes / pipeline.records_of).  New wrappers use these and write none of their own.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

WS_CACHE_MAX = 8        # keys whose scratch buffer a ScratchCache keeps alive; the least recently used one goes first


def tensor(x, dtype, dev):
    """Contiguous tensor of `dtype` on `dev` of a tensor, an array or a list (ops._t)."""
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dtype).contiguous()
    return torch.as_tensor(np.ascontiguousarray(x), device="cpu").to(device=dev, dtype=dtype).contiguous()


def image_batch(x, dev, who, max_images=None, max_dim=None):
    """Contiguous float32 [I,H,W] tensor on `dev` of an [H,W] or [I,H,W] image batch; ValueError for another rank, an empty
    dimension, more than max_images images or an H or W above max_dim.  The shape is checked before anything is copied."""
    shape = tuple(x.shape) if hasattr(x, "shape") else np.shape(x)
    full = (1,) + shape if len(shape) == 2 else shape
    if len(full) != 3 or min(full) < 1:
        raise ValueError("%s: depth is a non-empty [I,H,W] or [H,W] image batch, not %s" % (who, shape))
    if max_images is not None and full[0] > max_images:
        raise ValueError("%s: at most %d images per call, not %d" % (who, max_images, full[0]))
    if max_dim is not None and max(full[1:]) > max_dim:
        raise ValueError("%s: H and W are at most %d, not %s" % (who, max_dim, shape))
    return tensor(x, torch.float32, dev).reshape(full)


def mask_batch(x, like, dev, who, same_shape=False, err=ValueError):
    """Contiguous uint8 [D,H,W] tensor on `dev`, non-zero where x is, for the image batch `like` [I,H,W].  A uint8 tensor is
    taken as it is (every kernel tests != 0), a bool tensor is viewed as bytes, anything else becomes 1 / 0 in one comparison.
    `err` when x's size is no multiple of H * W or, with same_shape, when its shape ([H,W] counts as [1,H,W]) is not like's."""
    if torch.is_tensor(x):
        m = x.to(dev)
        m = m if m.dtype == torch.uint8 else (m if m.dtype == torch.bool else m != 0).view(torch.uint8)
    else:
        a = np.asarray(x)
        m = torch.from_numpy(np.ascontiguousarray(a if a.dtype == np.uint8 else (a != 0).view(np.uint8))).to(dev)
    _, H, W = like.shape
    if same_shape and ((1,) + tuple(m.shape) if m.dim() == 2 else tuple(m.shape)) != tuple(like.shape):
        raise err("%s: mask %s for depth %s" % (who, tuple(m.shape), tuple(like.shape)))
    if m.numel() % (H * W):
        raise err("%s: masks %s do not match the %d x %d depth image" % (who, tuple(m.shape), H, W))
    return m.reshape(-1, H, W).contiguous()


def per_item(x, n, dtype, dev, who, what="values", err=ValueError):
    """Contiguous tensor [n] of `dtype` on `dev`: a tensor of n entries, or a host value, array or list of one entry (for all
    items) or of n.  A host argument of another length is a ValueError, a tensor of another length is `err`."""
    if torch.is_tensor(x):
        if x.numel() != n:
            raise err("%s: %d %s for %d items" % (who, x.numel(), what, n))
        return x.to(device=dev, dtype=dtype).reshape(-1).contiguous()
    a = np.asarray(x).reshape(-1)
    if a.size != n and a.size != 1:
        raise ValueError("%s: %d %s for %d items" % (who, a.size, what, n))
    return torch.from_numpy(np.broadcast_to(a, (n,)).copy()).to(dtype).to(dev)          # converted on the host


def camera4(K):
    """(fx, fy, cx, cy) of a 3 x 3 camera matrix as the c_double[4] the ABI takes."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    return (C.c_double * 4)(K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def stream_key(dev):
    """(device index, current stream's handle) of a HIP device: the key of scratch that one stream's launches share."""
    dev = torch.device(dev)
    index = dev.index if dev.index is not None else torch.cuda.current_device()     # "cuda" and "cuda:0" are one device
    return (int(index), int(torch.cuda.current_stream(dev).cuda_stream))


def scratch(need, dev, entry, err):
    """One-shot scratch for the answer `need` of the ABI's *_workspace_bytes call `entry`: a uint8 tensor of max(need, 1)
    bytes (torch aligns device memory far beyond the ABI's 8 bytes); `err` naming the entry when the sizes were refused (< 0)."""
    if need < 0:
        raise err("%s: invalid sizes" % entry)
    return torch.empty((max(int(need), 1),), dtype=torch.uint8, device=dev)


class ScratchCache:
    """Scratch buffers by key (stream_key(dev): launches of one stream never overlap, those of different streams never share
    scratch), grown on demand.  At most max_entries are kept, the least recently used one goes first, so a process that keeps
    creating streams does not pin a buffer per stream.  on_drop(key) is told each key whose buffer was replaced or evicted:
    state that describes a buffer's contents must go with it, since a later buffer may be allocated at the same address.
    cache[key] is the key's buffer.  `entry` is the ABI's *_workspace_bytes call whose answers get() is given: a negative one
    (the sizes were refused) is `err` naming it."""

    def __init__(self, entry, err, max_entries=WS_CACHE_MAX, on_drop=lambda key: None):
        self.entry, self.err, self.max_entries, self.on_drop = entry, err, int(max_entries), on_drop
        self.buffers = {}                     # key -> uint8 tensor; dicts keep insertion order, the first key is the oldest

    def __getitem__(self, key):
        return self.buffers[key]

    def get(self, key, need, dev):
        """A uint8 tensor of at least `need` bytes on `dev`: the key's buffer if it is large enough, else a new one."""
        if need < 0:
            raise self.err("%s: invalid sizes" % self.entry)
        buf = self.buffers.pop(key, None)
        if buf is not None and buf.numel() < need:
            buf = None
            self.on_drop(key)
        if buf is None:
            buf = torch.empty((need,), dtype=torch.uint8, device=dev)
        self.buffers[key] = buf               # (re-)inserted last
        while len(self.buffers) > self.max_entries:
            old = next(iter(self.buffers))
            del self.buffers[old]
            self.on_drop(old)
        return buf

    def clear(self):
        for key in list(self.buffers):
            del self.buffers[key]
            self.on_drop(key)
