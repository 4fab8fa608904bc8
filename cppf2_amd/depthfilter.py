"""Sensor depth conditioned before anything else reads it (cppf_depth_condition): mixed ("flying") pixels
along depth discontinuities are dropped, and what is left can be smoothed within its surface.  The reference takes a depth image
as it comes from the file and has no such step; nothing here runs unless a caller asks for it.

    out, counts = condition(depth)                          # the defaults: drop flying pixels, no smoothing
    out, counts = condition(depth, smooth_radius=2)         # and the paired mean within 1 cm of the centre
    s = from_flags(True, dict(smooth_radius=2))             # the settings record eval.py and python -m cppf2_amd.fuse share
    d, summary = apply(depths, s, "fuse.fuse_views")        # what their callers run on every depth batch

The definition (the kernel's file states it in the order of its float32 operations, tests/depth_condition_ref.py restates it):
a reading is valid if it is finite and > 0; tol(z) = jump + jump_rel * z; every comparison is |q - z| <= tol(z) with z the centre
pixel's reading.  Stage 1: a valid pixel keeps its reading iff at least min_support of the other (2 flying_radius + 1)^2 - 1
positions of its window lie outside the image or hold a valid reading within tol; every other pixel becomes 0.  Stage 2, on
stage 1's output: the mean of the pixel and of every PAIR of opposite neighbours within smooth_radius that are both kept and
both within tol -- opposite neighbours enter together or not at all, so the mean has no bias on a slanted surface however the
gate clips the window.  counts per image: (valid readings, valid readings stage 1 removed, pixels whose mean took a pair).
"""
from __future__ import annotations

import collections
import ctypes as C
import math

import numpy as np

from . import hostargs, masks
from ._lib import CppfError

MAX_RADIUS = 4              # flying_radius, smooth_radius
MAX_IMAGE = 16384           # H, W
FLYING_RADIUS = 1
MIN_SUPPORT = 4             # of the 8 neighbours: a pixel on a straight silhouette has 5 on its own side
SMOOTH_RADIUS = 0           # smoothing has to be asked for: it costs curvature bias

# The settings the callers pass on: what condition() takes after the image.
Settings = collections.namedtuple("Settings", "flying_radius min_support smooth_radius jump jump_rel")

# flag -> Settings field, in the spelling of eval.py (python -m cppf2_amd.fuse: the same words with hyphens)
FLAGS = dict(flying_radius="flying_radius", flying_support="min_support", smooth_radius="smooth_radius", depth_jump="jump",
             depth_jump_rel="jump_rel")


def checked(flying_radius=FLYING_RADIUS, min_support=None, smooth_radius=SMOOTH_RADIUS, jump=None, jump_rel=0.0,
            who="depthfilter.condition"):
    """The Settings of these values, or ValueError naming the first one outside the kernel's limits.  min_support None: the
    default MIN_SUPPORT, and 0 with flying_radius = 0 (no neighbour is looked at: stage 1 is off).  jump None: masks.JUMP."""
    def whole(x):
        v = float(x)
        if v != int(v):
            raise ValueError
        return int(v)
    try:
        r1, r2 = whole(flying_radius), whole(smooth_radius)
        support = (MIN_SUPPORT if r1 > 0 else 0) if min_support is None else whole(min_support)
        jump, jump_rel = float(masks.JUMP if jump is None else jump), float(jump_rel)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s: the radii and min_support are whole numbers, jump and jump_rel numbers" % who) from None
    if not (0 <= r1 <= MAX_RADIUS and 0 <= r2 <= MAX_RADIUS):
        raise ValueError("%s: flying_radius and smooth_radius are in 0 .. %d, not %d and %d" % (who, MAX_RADIUS, r1, r2))
    if not 0 <= support <= (2 * r1 + 1) ** 2:
        raise ValueError("%s: min_support is in 0 .. %d with flying_radius %d, not %d" % (who, (2 * r1 + 1) ** 2, r1, support))
    if not (jump >= 0 and math.isfinite(jump) and jump_rel >= 0 and math.isfinite(jump_rel)):
        raise ValueError("%s: jump (metres) and jump_rel are finite and >= 0, not %r and %r" % (who, jump, jump_rel))
    return Settings(r1, support, r2, jump, jump_rel)


def from_flags(switch, values, spell=lambda name: "--" + name, switch_name="condition_depth", who="eval.py"):
    """The one place the flags become Settings.  switch: whether conditioning was asked for; values: dict flag -> value or None
    over FLAGS' keys (a missing one counts as None).  None when the switch is off -- a sub-flag given without it is a ValueError
    in eval.py's wording --, else checked() of the given values over the defaults."""
    given = [k for k in FLAGS if values.get(k) is not None]
    if not switch:
        if given:
            raise ValueError("%s sets how the depth image is conditioned: it needs %s" % (spell(given[0]), spell(switch_name)))
        return None
    return checked(who=who, **{FLAGS[k]: values[k] for k in given})


def summary(settings, counts):
    """The reports' entry: the settings and the three counts summed over the images."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 3).sum(0)
    return dict(settings._asdict(), valid=int(c[0]), removed=int(c[1]), smoothed=int(c[2]))


def merged(summaries):
    """One summary of several batches' (same settings): the counts add up."""
    out = dict(summaries[0])
    for s in summaries[1:]:
        for k in ("valid", "removed", "smoothed"):
            out[k] += s[k]
    return out


def condition(depth, flying_radius=FLYING_RADIUS, min_support=MIN_SUPPORT, smooth_radius=SMOOTH_RADIUS, jump=masks.JUMP, jump_rel=0.0):
    """cppf_depth_condition: depth float32 [I,H,W] or [H,W] in metres (a device tensor, or a host array or list, which is
    uploaded) -> (out: device float32 [I,H,W], counts: int64 array [I,3] on the host = per image (valid readings, valid readings
    stage 1 removed, pixels whose mean took a pair)).  One launch for all images; the input is not written.  With flying_radius =
    0 stage 1 is off and min_support is not used.  CppfError for a tensor that is not on a HIP device, or without one: there is
    no CPU fallback."""
    import torch
    from . import _lib, ops
    s = checked(flying_radius, None if flying_radius == 0 else min_support, smooth_radius, jump, jump_rel)
    if torch.is_tensor(depth) and depth.device.type != "cuda":
        raise CppfError("depthfilter.condition: the depth tensor is on %s; cppf2_amd needs a HIP device, there is no CPU fallback"
                        % depth.device)
    dev = depth.device if torch.is_tensor(depth) else ops._dev()
    d = hostargs.image_batch(depth, dev, "depthfilter.condition", max_dim=MAX_IMAGE)
    I, H, W = (int(x) for x in d.shape)
    out = torch.empty_like(d)
    counts = torch.empty((I, 3), dtype=torch.int32, device=dev)
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.cppf_depth_condition(ops._p(d), I, H, W, s.flying_radius, s.min_support, s.smooth_radius, C.c_float(s.jump),
                                          C.c_float(s.jump_rel), ops._p(out), ops._p(counts), ops._stream()), "cppf_depth_condition")
    return out, counts.cpu().numpy().astype(np.int64)


def apply(depths, settings, who="depthfilter.apply"):
    """What a caller with `condition=settings` runs on a depth batch before anything else sees it: (the batch, None) as it is when
    settings is None, else (condition()'s out, summary)."""
    if settings is None:
        return depths, None
    if not isinstance(settings, Settings):
        raise ValueError("%s: condition is a depthfilter.Settings record (depthfilter.checked or from_flags), not %r" % (who, settings))
    out, counts = condition(depths, *settings)
    return out, summary(settings, counts)
