"""Detector masks: COCO's run-length encoding on the host (both directions, list and compressed-string form), decoding a batch
of them on the GPU (cppf_rle_decode) and cutting each mask down to its largest depth-connected component (cppf_mask_components).
The reference takes a mask as given (eval.py:173-201) and has neither step.

    counts = rle_encode(mask)                       # [int]: column-major runs, alternating 0s and 1s, starting with 0s
    s = counts_to_string(counts)                    # COCO's compressed form; string_to_counts(s) == counts
    m = decode_batch([counts, ...], H, W)           # uint8 [D,H,W] device tensor, 255 / 0
    kept, stats = clean(m, depth, 0, jump=0.01)     # 255 on the largest depth-connected component of each mask

The run rule (COCO's maskApi): the pixels of a mask in column-major order (position c * H + r) are cut into runs of equal
values; the lengths are listed starting with a run of 0s, so a mask whose first pixel is set starts with a length of 0.  The
string form: every count from index 3 on (the fourth) is replaced by its difference to the count two before it (maskApi.c
rleToString: `if (i > 2) x -= cnts[i - 2]`); each value is then written in 5-bit groups, lowest first, bit 0x20 of a group = more
groups follow, bit 0x10 of the last group = the sign (the value is sign-extended from there), each character = group + 48.
pycocotools was not available to compare against: the codec is pinned by vectors worked by hand from this definition
(tests/test_masks.py), parity with pycocotools is unpinned.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

JUMP = 0.01                 # metres: DESIGN.md section 18 derives it
MIN_PIXELS = 16             # a smaller component cannot carry a pose (a few 5-point tuples at most after down-sampling)
MAX_MASKS = 65535           # per call of either kernel


class RleError(ValueError):
    """Runs or a compressed string that are no run-length code of an H x W mask."""


# ----------------------------------------------------------------------------------------------
# host codec
# ----------------------------------------------------------------------------------------------
def rle_encode(mask):
    """[int]: COCO's run lengths of a 2-D mask (non-zero = set)."""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise RleError("rle_encode: a mask is 2-D, not %s" % (m.shape,))
    flat = (m != 0).T.reshape(-1)                                   # column-major
    if flat.size == 0:
        return []
    edges = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    counts = np.diff(np.concatenate([[0], edges, [flat.size]])).tolist()
    return ([0] + counts) if flat[0] else counts


def check_counts(counts, H, W):
    """int64 [n] of a mask's run lengths, or RleError: a negative run, or runs that do not sum to H * W."""
    try:
        c = np.asarray(counts, dtype=np.int64).reshape(-1)
    except (TypeError, ValueError, OverflowError):
        raise RleError("run lengths are integers, not %r" % (counts,)) from None
    if c.size and int(c.min()) < 0:
        raise RleError("negative run length %d" % int(c.min()))
    if int(c.sum()) != int(H) * int(W):
        raise RleError("runs sum to %d, the mask has %d x %d = %d pixels" % (int(c.sum()), H, W, int(H) * int(W)))
    return c


def rle_decode(counts, H, W):
    """uint8 [H,W] (255 / 0) of COCO run lengths; RleError as check_counts."""
    c = check_counts(counts, H, W)
    vals = np.zeros(c.size, dtype=np.uint8)
    vals[1::2] = 255
    return np.ascontiguousarray(np.repeat(vals, c).reshape(int(W), int(H)).T)


def counts_to_string(counts):
    """COCO's compressed string of run lengths."""
    c = [int(x) for x in counts]
    out = []
    for i, x in enumerate(c):
        if i > 2:
            x -= c[i - 2]
        more = True
        while more:
            g = x & 0x1f
            x >>= 5                                               # arithmetic shift: -1 stays -1
            more = (x != -1) if (g & 0x10) else (x != 0)
            out.append(chr((g | 0x20 if more else g) + 48))
    return "".join(out)


def string_to_counts(s):
    """[int]: the run lengths of COCO's compressed string; RleError for a character outside the code, a value cut off by the
    string's end, or a value longer than 13 groups (64 bits)."""
    if isinstance(s, bytes):
        s = s.decode("ascii", "replace")
    if not isinstance(s, str):
        raise RleError("a compressed run-length code is a string, not %r" % type(s).__name__)
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            if p >= len(s):
                raise RleError("compressed run-length string ends inside a value")
            g = ord(s[p]) - 48
            if g < 0 or g > 63:
                raise RleError("character %r at %d is outside the code (48 .. 111)" % (s[p], p))
            if k > 12:
                raise RleError("value at %d has more than 13 groups" % p)
            x |= (g & 0x1f) << (5 * k)
            more = bool(g & 0x20)
            p += 1
            k += 1
            if not more and (g & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def bbox(mask):
    """[x, y, w, h] of a mask's set pixels ([0, 0, 0, 0] when empty): the detections file's box."""
    m = np.asarray(mask) != 0
    if not m.any():
        return [0, 0, 0, 0]
    r, c = np.nonzero(m)
    return [int(c.min()), int(r.min()), int(c.max() - c.min() + 1), int(r.max() - r.min() + 1)]


# ----------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------
def decode_batch(counts_list, H, W):
    """uint8 [D,H,W] device tensor (255 / 0) of D masks' COCO run lengths (each a list or array of ints, or a compressed
    string), one image size: one cppf_rle_decode launch per MAX_MASKS masks.  Every mask is checked on the host first (RleError:
    a negative run, runs that do not sum to H * W, a string that does not parse); nothing is launched when one fails."""
    import torch
    from . import _lib, ops
    H, W = int(H), int(W)
    runs = [check_counts(string_to_counts(c) if isinstance(c, (str, bytes)) else c, H, W) for c in counts_list]
    dev = ops._dev()
    D = len(runs)
    out = torch.empty((D, H, W), dtype=torch.uint8, device=dev)
    L = _lib.load()
    for a in range(0, D, MAX_MASKS):
        part = runs[a:a + MAX_MASKS]
        off = np.cumsum([0] + [r.size for r in part])
        if off[-1] > 0x7fffffff:
            raise RleError("%d runs in one call" % off[-1])
        flat = ops._t(np.concatenate(part).astype(np.int32) if off[-1] else np.zeros(1, np.int32), torch.int32, dev)
        roff = ops._t(off.astype(np.int32), torch.int32, dev)
        _lib.check(L.cppf_rle_decode(len(part), H, W, ops._p(flat), int(off[-1]), ops._p(roff), ops._p(out[a:]), ops._stream()),
                   "cppf_rle_decode")
    return out


def clean(masks, depths, img_idx=0, jump=JUMP, min_pixels=MIN_PIXELS):
    """The largest depth-connected component of each mask (cppf_mask_components): masks uint8 or bool [D,H,W] (non-zero = set;
    host array or device tensor), depths float32 [I,H,W] or [H,W] (metres), img_idx int [D] (or one for all).  A pixel is valid
    when it is set and its depth is positive and finite; valid 4-neighbours whose depths differ by at most `jump` (float32) are
    connected.  Returns (uint8 [D,H,W] device tensor: 255 on the component with the most pixels -- ties to the one whose first
    pixel in row-major order comes first --, all 0 when it has fewer than min_pixels; int32 [D,4] device tensor: components,
    the kept one's lowest flat index or -1, its pixels, valid pixels).  No host synchronisation."""
    import torch
    from . import _lib, hostargs, ops
    jump = float(jump)
    if not (jump >= 0.0 and np.isfinite(jump)):
        raise ValueError("masks.clean: jump must be a finite distance >= 0, not %r" % jump)
    dev = ops._dev()
    dt = hostargs.image_batch(depths, dev, "masks.clean")
    I, H, W = (int(x) for x in dt.shape)
    mk = hostargs.mask_batch(masks, dt, dev, "masks.clean")
    D = int(mk.shape[0])
    ii = hostargs.per_item(img_idx, D, torch.int32, dev, "masks.clean", "image indices")
    out = torch.empty((D, H, W), dtype=torch.uint8, device=dev)
    stats = torch.empty((D, 4), dtype=torch.int32, device=dev)
    L = _lib.load()
    for a in range(0, D, MAX_MASKS):
        n = min(MAX_MASKS, D - a)
        need = int(L.cppf_mask_components_workspace_bytes(n, H, W))
        ws = hostargs.scratch(need, dev, "cppf_mask_components_workspace_bytes", _lib.CppfError)
        _lib.check(L.cppf_mask_components(n, I, H, W, ops._p(mk[a:]), ops._p(dt), ops._p(ii[a:]), C.c_float(jump), int(min_pixels),
                                          ops._p(out[a:]), ops._p(stats[a:]), ops._p(ws), need, ops._stream()),
                   "cppf_mask_components")
    return out, stats
