"""Solid-interval checks on candidate poses (the reference has no such step): verification and scene
explanation judge a pose by the surface it shows the camera, so a hypothesis may stand a third under the table, or have most
of its body inside an object chosen earlier, and still collect every pixel it fits.  Two renders of a closed mesh bound its
first solid interval along each pixel's ray: `front` with back faces culled, `back` with every triangle's winding reversed
(verify.render_records(back=True)).

    counts = support_counts(front, back, cand_off, planes, K)     # int64 [P,4] = (back, sunk, solid, open), device
    refused = sunk_share(counts) > MAX_SUNK                       # host
    inter = overlap_counts(front, back, cand_off)                 # int64 [P,64], device; at most 64 candidates per image
    clash = conflicts(inter[off[i]:off[i + 1]], MAX_OVERLAP)      # bool [C,C], host

The defaults are derived, none was swept: SUPPORT_TAU is the 1 cm band segment.MIN_HEIGHT already cuts around the plane,
OVERLAP_TAU verification's 2 cm (two poses that each verify within it may overlap by that much), and a tenth of a pose's far
side under the table, or of the smaller solid inside the other, is refused.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import segment as _segment

SUPPORT_TAU = _segment.MIN_HEIGHT
MAX_SUNK = 0.1
OVERLAP_TAU = 0.02                          # verify.TAU (not imported here: this module's checks need no library)
MAX_OVERLAP = 0.1
MAX_CANDIDATES = 64                         # per image, overlap_counts: one bit of a pixel's word each
MAX_DIM = 8192
MAX_RENDERS = 1 << 24


def checked_share(x, who, what):
    """A share in [0, 1] as a float; ValueError otherwise (NaN included)."""
    x = float(x)
    if not 0.0 <= x <= 1.0:
        raise ValueError("%s: %s is a share in 0 .. 1, not %r" % (who, what, x))
    return x


def checked_tau(x, who, what="tau"):
    """A finite distance in metres >= 0 as a float; ValueError otherwise."""
    x = float(x)
    if not (x >= 0.0 and np.isfinite(x)):
        raise ValueError("%s: %s is a finite distance in metres >= 0, not %r" % (who, what, x))
    return x


def checked_offsets(cand_off, who, limit=None, most=None):
    """Contiguous int32 [I+1] of a caller's candidate offsets (a host array, a list or a tensor): they start at 0 and never
    decrease, no image has more than `limit` candidates and there are at most `most` in all; ValueError otherwise.  The one
    check of scene.py's and this module's wrappers."""
    off = np.asarray(cand_off.cpu().numpy() if hasattr(cand_off, "cpu") else cand_off).reshape(-1)
    if off.size < 2 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError("%s: cand_off is int [I+1], I >= 1" % who)
    off = off.astype(np.int64)
    if off[0] != 0 or np.any(np.diff(off) < 0):
        raise ValueError("%s: cand_off must start at 0 and never decrease" % who)
    if most is not None and off[-1] > most:
        raise ValueError("%s: at most %d renders per call, not %d" % (who, most, int(off[-1])))
    if limit is not None and np.any(np.diff(off) > limit):
        raise ValueError("%s: at most %d candidates per image, not %d" % (who, limit, int(np.diff(off).max())))
    return np.ascontiguousarray(off, dtype=np.int32)


def _renders(front, back, off, dev, who):
    """(front, back float32 [P,H,W] on dev, P, H, W) of two render stacks of one shape [P,H,W], P = off[-1]."""
    import torch
    from . import hostargs
    sf = tuple(front.shape) if hasattr(front, "shape") else np.shape(front)
    sb = tuple(back.shape) if hasattr(back, "shape") else np.shape(back)
    if len(sf) != 3 or sf != sb or min(sf[1:]) < 1:
        raise ValueError("%s: front and back are renders [P,H,W] of one shape, not %s and %s" % (who, sf, sb))
    if max(sf[1:]) > MAX_DIM:
        raise ValueError("%s: H and W are at most %d, not %s" % (who, MAX_DIM, sf))
    if int(off[-1]) != sf[0]:
        raise ValueError("%s: cand_off ends at %d for %d renders" % (who, int(off[-1]), sf[0]))
    return hostargs.tensor(front, torch.float32, dev), hostargs.tensor(back, torch.float32, dev), sf[0], sf[1], sf[2]


def support_counts(front, back, cand_off, planes, K, tau=SUPPORT_TAU):
    """cppf_support_counts on the current stream: int64 [P,4] device tensor = (back, sunk, solid, open) per candidate.  front,
    back float32 [P,H,W] (0 = nothing drawn), cand_off int [I+1] (host: renders cand_off[i] .. cand_off[i+1]-1 belong to image
    i; any number each), planes float32 [I,4] or [4] = (n, d) as segment.fit_plane returns them (zeros or NaN: nothing sinks), K
    as segment.intrinsics4 takes it (or a float32 [I,4] device tensor).  No host synchronisation."""
    who = "solid.support_counts"
    tau = checked_tau(tau, who)
    off = checked_offsets(cand_off, who, most=MAX_RENDERS)
    import torch
    from . import _lib, hostargs, ops
    dev = ops._dev()
    f, b, P, H, W = _renders(front, back, off, dev, who)
    I = off.size - 1
    pl = hostargs.tensor(planes, torch.float32, dev).reshape(-1, 4)
    if pl.shape[0] != I:
        raise ValueError("%s: %d images, %d planes" % (who, I, pl.shape[0]))
    km = _segment._kmat(K, I, dev, who)
    counts = torch.empty((P, 4), dtype=torch.int64, device=dev)
    L = _lib.load()
    _lib.check(L.cppf_support_counts(I, H, W, ops._p(f), ops._p(b), off.ctypes.data_as(C.c_void_p), P, ops._p(pl), ops._p(km),
                                     C.c_float(tau), ops._p(counts), ops._stream()), "cppf_support_counts")
    return counts


def overlap_counts(front, back, cand_off, tau=OVERLAP_TAU):
    """cppf_solid_overlap on the current stream: int64 [P,64] device tensor; row cand_off[i] + a, column j < C_i = the pixels
    where candidates a and j of image i are both solid and their intervals share more than tau; symmetric, the diagonal = the
    solid pixels of a, columns from C_i on are 0.  At most 64 candidates per image.  No host synchronisation."""
    who = "solid.overlap_counts"
    tau = checked_tau(tau, who)
    off = checked_offsets(cand_off, who, MAX_CANDIDATES, MAX_RENDERS)
    import torch
    from . import _lib, hostargs, ops
    dev = ops._dev()
    f, b, P, H, W = _renders(front, back, off, dev, who)
    I = off.size - 1
    inter = torch.empty((P, MAX_CANDIDATES), dtype=torch.int64, device=dev)
    L = _lib.load()
    need = int(L.cppf_solid_overlap_workspace_bytes(I, H, W))
    ws = hostargs.scratch(need, dev, "cppf_solid_overlap_workspace_bytes", _lib.CppfError)
    _lib.check(L.cppf_solid_overlap(I, H, W, ops._p(f), ops._p(b), off.ctypes.data_as(C.c_void_p), P, C.c_float(tau), ops._p(inter),
                                    ops._p(ws), need, ops._stream()), "cppf_solid_overlap")
    return inter


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def sunk_share(counts):
    """float64 [P]: sunk / back of support_counts' rows, 0 where back == 0."""
    c = _host(counts).astype(np.int64).reshape(-1, 4)
    return np.where(c[:, 0] > 0, c[:, 1].astype(np.float64) / np.maximum(c[:, 0], 1).astype(np.float64), 0.0)


def conflicts(inter, max_overlap=MAX_OVERLAP):
    """bool [C,C] of ONE image's rows of overlap_counts (int64 [C,64]): a and c conflict iff inter[a, c] > max_overlap *
    min(solid_a, solid_c) in float64; no candidate conflicts with itself."""
    max_overlap = checked_share(max_overlap, "solid.conflicts", "max_overlap")
    m = _host(inter).astype(np.int64)
    if m.ndim != 2 or m.shape[1] != MAX_CANDIDATES or m.shape[0] > MAX_CANDIDATES:
        raise ValueError("solid.conflicts: one image's rows int64 [C,%d], C <= %d, not %s" % (MAX_CANDIDATES, MAX_CANDIDATES, m.shape))
    n = m.shape[0]
    sq = m[:, :n]
    solid = np.diagonal(sq).astype(np.float64)
    out = sq.astype(np.float64) > np.float64(max_overlap) * np.minimum(solid[:, None], solid[None, :])
    out[np.arange(n), np.arange(n)] = False
    return out
