"""A weight per depth reading by its viewing angle (cppf_depth_weights): a reading taken face-on counts
`levels` times, one taken at a grazing angle once, and one whose neighbourhood does not give a normal (a silhouette, a hole's
rim, the image's border) not at all.  fuse.integrate(..., weights=) adds the views with these weights
(cppf_tsdf_integrate_weighted).  The reference has no such step; nothing here runs unless a caller asks for it.

    w, counts = weights(depths, K)                             # uint8 [I,H,W] on the device, the defaults: 16 levels
    fuse.integrate(vol, depths, poses, K, masks=masks, weights=w, carve_weight=1)
    s = from_flags(True, dict(weight_levels=8))                # the settings record python -m cppf2_amd.fuse builds
    mesh, report = fuse.fuse_views(depths, masks, poses, K, voxel=0.002, weighting=checked())
    w, summary = apply(depths, K, s, who="fuse.fuse_views")    # what the callers with `weighting=settings` run on every batch

The definition (the kernel's file states it in the order of its float32 operations, tests/depth_weights_ref.py restates it):
a reading is valid if it is finite and > 0; tol(z) = jump + jump_rel * z.  A valid pixel whose four neighbours at `step` pixels
to the left, right, up and down all lie inside the image and hold valid readings within tol of its own gets the normal n =
(P(right) - P(left)) x (P(down) - P(up)) of the back-projected points, and c = |n . p| / (|n| |p|), the cosine between its ray
and that normal.  Its weight is round(c * levels) clamped to 1 .. levels if c >= cos_min, and 0 otherwise; every other pixel
gets 0.  counts per image: (valid readings, valid readings with weight 0, readings with the full weight `levels`).

The volume stays what it is: acc becomes the sum of w * obs, wsum the sum of w, and min_weight of extract, track, close and
relocalise a threshold in units of weight -- with 16 levels one face-on view adds 16.
"""
from __future__ import annotations

import collections
import ctypes as C
import math

import numpy as np

from . import hostargs
from ._lib import CppfError

MAX_STEP = 4
MAX_LEVELS = 255
MAX_IMAGE = 16384           # H, W
STEP = 1                    # a wider difference smooths the normal and widens the silhouette's band of zeros
JUMP = 0.01                 # metres: masks.JUMP
LEVELS = 16
COS_MIN = 0.2               # 78.5 degrees: beyond it a reading's projective distance overstates the true one five times
CARVE_WEIGHT = 1            # the weight of "free space in front of this pixel": a silhouette pixel has no normal

# The settings the callers pass on: what weights() takes after the camera and the pixel offset, and integrate's carve_weight.
Settings = collections.namedtuple("Settings", "step jump jump_rel levels cos_min carve_weight")

# flag -> Settings field (python -m cppf2_amd.fuse: the same words with hyphens)
FLAGS = dict(weight_step="step", weight_jump="jump", weight_jump_rel="jump_rel", weight_levels="levels", weight_cos_min="cos_min",
             carve_weight="carve_weight")
COUNTS = ("valid", "zero", "full")


def checked(step=STEP, jump=JUMP, jump_rel=0.0, levels=LEVELS, cos_min=COS_MIN, carve_weight=CARVE_WEIGHT, who="depthweights.weights"):
    """The Settings of these values, or ValueError naming the first one outside the kernels' limits."""
    def whole(x):
        v = float(x)
        if v != int(v):
            raise ValueError
        return int(v)
    try:
        step, levels, carve_weight = whole(step), whole(levels), whole(carve_weight)
        jump, jump_rel, cos_min = float(jump), float(jump_rel), float(cos_min)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s: step, levels and carve_weight are whole numbers, jump, jump_rel and cos_min numbers" % who) from None
    if not 1 <= step <= MAX_STEP:
        raise ValueError("%s: step is in 1 .. %d pixels, not %d" % (who, MAX_STEP, step))
    if not (jump >= 0 and math.isfinite(jump) and jump_rel >= 0 and math.isfinite(jump_rel)):
        raise ValueError("%s: jump (metres) and jump_rel are finite and >= 0, not %r and %r" % (who, jump, jump_rel))
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError("%s: levels is in 1 .. %d, not %d" % (who, MAX_LEVELS, levels))
    if not 0 <= cos_min < 1:
        raise ValueError("%s: cos_min is a cosine in [0, 1), not %r" % (who, cos_min))
    if not 0 <= carve_weight <= 255:
        raise ValueError("%s: carve_weight is in 0 .. 255, not %d" % (who, carve_weight))
    return Settings(step, jump, jump_rel, levels, cos_min, carve_weight)


def from_flags(switch, values, spell=lambda name: "--" + name.replace("_", "-"), switch_name="weight_views", who="--weight-views"):
    """The one place the flags become Settings.  switch: whether weighting was asked for; values: dict flag -> value or None over
    FLAGS' keys (a missing one counts as None).  None when the switch is off -- a sub-flag given without it is a ValueError --,
    else checked() of the given values over the defaults."""
    given = [k for k in FLAGS if values.get(k) is not None]
    if not switch:
        if given:
            raise ValueError("%s sets how the views are weighted: it needs %s" % (spell(given[0]), spell(switch_name)))
        return None
    return checked(who=who, **{FLAGS[k]: values[k] for k in given})


def summary(settings, counts):
    """The reports' entry: the settings and the three counts summed over the images."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 3).sum(0)
    return dict(settings._asdict(), **{k: int(v) for k, v in zip(COUNTS, c)})


def merged(summaries):
    """One summary of several batches' (same settings): the counts add up."""
    out = dict(summaries[0])
    for s in summaries[1:]:
        for k in COUNTS:
            out[k] += s[k]
    return out


def weights(depths, K, pixel_offset=0.0, step=STEP, jump=JUMP, jump_rel=0.0, levels=LEVELS, cos_min=COS_MIN):
    """cppf_depth_weights: depths float32 [I,H,W] or [H,W] in metres (a device tensor, or a host array or list, which is
    uploaded) and the 3 x 3 camera matrix K -> (weights: device uint8 [I,H,W], counts: int64 array [I,3] on the host = per image
    (valid readings, valid readings with weight 0, readings with weight `levels`)).  pixel_offset as fuse.integrate's.  One launch
    for all images; the input is not written.  CppfError for a tensor that is not on a HIP device, or without one: there is no
    CPU fallback."""
    import torch
    from . import _lib, ops
    s = checked(step, jump, jump_rel, levels, cos_min)
    if not math.isfinite(float(pixel_offset)):
        raise ValueError("depthweights.weights: pixel_offset is a finite number, not %r" % (pixel_offset,))
    if torch.is_tensor(depths) and depths.device.type != "cuda":
        raise CppfError("depthweights.weights: the depth tensor is on %s; cppf2_amd needs a HIP device, there is no CPU fallback"
                        % depths.device)
    dev = depths.device if torch.is_tensor(depths) else ops._dev()
    d = hostargs.image_batch(depths, dev, "depthweights.weights", max_dim=MAX_IMAGE)
    I, H, W = (int(x) for x in d.shape)
    out = torch.empty((I, H, W), dtype=torch.uint8, device=dev)
    counts = torch.empty((I, 3), dtype=torch.int32, device=dev)
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.cppf_depth_weights(ops._p(d), I, H, W, hostargs.camera4(K), C.c_float(pixel_offset), s.step, C.c_float(s.jump),
                                        C.c_float(s.jump_rel), s.levels, C.c_float(s.cos_min), ops._p(out), ops._p(counts),
                                        ops._stream()), "cppf_depth_weights")
    return out, counts.cpu().numpy().astype(np.int64)


def apply(depths, K, settings, pixel_offset=0.0, who="depthweights.apply"):
    """What a caller with `weighting=settings` runs on a depth batch (after conditioning, when both are on): (None, None) when
    settings is None, else (weights()'s tensor, summary)."""
    if settings is None:
        return None, None
    if not isinstance(settings, Settings):
        raise ValueError("%s: weighting is a depthweights.Settings record (depthweights.checked or from_flags), not %r" % (who, settings))
    w, counts = weights(depths, K, pixel_offset, *settings[:5])
    return w, summary(settings, counts)
