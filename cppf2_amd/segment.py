"""Mask proposals from depth alone (the reference takes its masks from a detector): the support plane of
a tabletop depth image by sampled three-pixel hypotheses (cppf_plane_fit), the pixels that stand above it
(cppf_plane_foreground), and the depth-connected pieces of what is left, ranked by size (cppf_mask_segments).

    plane, pstats = fit_plane(depth, K, seeds)                # float32 [I,4] = (n, d); int32 [I,4]
    fg = foreground(depth, K, plane)                          # uint8 [I,H,W], 255 above the plane
    rank, seg, stats = segments(fg, depth, 0)                 # uint8 [D,H,W] rank or 255; int32 [D,M,6]; int32 [D,4]
    masks, props, report = propose(depth, K, seed=0)          # one image: uint8 [P,H,W] in rank order, [dict], dict
    keep, counts = concave_edges(depth, K, fg)                # uint8 [I,H,W]: fg without the concave pixels; int64 [I,3] (host)
    masks, props, report = propose(depth, K, concave=concave_checked(), plane=False)     # no support plane: a shelf, a bin

    python -m cppf2_amd.segment --depth d.png --depth-scale 1000 --intrinsics fx,fy,cx,cy --obj-ids 1,5 --scene-id 1 \
        --image-id 3 --out detections.json

The command writes every proposal once per object id, score 1.0, as a BOP detections file (bop_data.write_detections);
`eval.py --data=bop --detections=... --hypotheses=8` then chooses among them by verification score.  `--concave` removes the
locally concave pixels before the labelling, so that touching and stacked objects part and the contact line with the table is
cut where it is; `--concave --no-plane` proposes without a support plane.

The defaults are derived, none was swept: TAU = 5 mm, a depth camera's noise at a metre; MIN_HEIGHT =
1 cm, which cuts the contact line where an object and the table meet at equal depth (section 18); jump = masks.JUMP;
MIN_SEGMENT_PIXELS = 200, a 2.4 cm square at a metre; NUM_HYP = 256 hypotheses, of which about ten have all three pixels on a
table that covers a third of the image.  CONCAVE_STEP, CONCAVE_ANGLE and CONCAVE_FLOOR are the best row of section 35's table
over ray-cast scenes; none was swept beyond that table, none was tried on real sensor depth.
"""
from __future__ import annotations

import collections
import ctypes as C
import math

import numpy as np

from . import masks as _masks

NUM_HYP = 256
TAU = 0.005
MIN_HEIGHT = 0.01
MIN_SEGMENT_PIXELS = 200
MAX_SEGMENTS = 16
MAX_HYP = 1024               # cppf_plane_fit's LDS holds that many planes
SEGMENTS_LIMIT = 64          # cppf_mask_segments
MAX_IMAGES = 65535           # per call of either kernel
MAX_DIM = 8192               # H, W of the segment family
CONCAVE_MAX_STEP = 8         # cppf_concave_edges' LDS halo
CONCAVE_STEP = 3             # pixels between a profile's centre and its two ends; the removed band is 2 * step - 1 wide
CONCAVE_ANGLE = 15.0         # degrees: the turn between a profile's two sides above which it is a crease
CONCAVE_FLOOR = 0.002        # metres: the centre's offset from the chord below which an angle means nothing (sensor noise)

# cppf_concave_edges' settings: what concave_edges() takes after fg.  reach (metres): the depth difference up to which a
# profile's end belongs to the centre's neighbourhood; None in checked() means step * masks.JUMP.
ConcaveSettings = collections.namedtuple("ConcaveSettings", "step angle floor reach")

# flag -> ConcaveSettings field (python -m cppf2_amd.segment: the same words with hyphens)
CONCAVE_FLAGS = dict(concave_step="step", concave_angle="angle", concave_floor="floor", concave_reach="reach")
CONCAVE_COUNTS = ("valid", "edge", "kept")


def intrinsics4(K, I, who="segment"):
    """float32 [I,4] = (fx, fy, cx, cy) on the host of K: a 3 x 3 matrix or I of them (zero skew, last row 0 0 1; ValueError
    otherwise), or (fx, fy, cx, cy), one for all images or one each."""
    k = np.asarray(K, dtype=np.float64)
    if k.shape[-2:] == (3, 3) and k.ndim in (2, 3):
        k = k.reshape(-1, 3, 3)
        if np.any(k[:, 0, 1] != 0) or np.any(k[:, 1, 0] != 0) or np.any(k[:, 2, :] != np.array([0.0, 0.0, 1.0])):
            raise ValueError("%s: the camera matrix must have zero skew and the last row 0 0 1" % who)
        k = np.stack([k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2]], axis=1)
    elif k.shape[-1:] == (4,) and k.ndim in (1, 2):
        k = k.reshape(-1, 4)
    else:
        raise ValueError("%s: K is 3 x 3, [I,3,3], (fx, fy, cx, cy) or [I,4], not %s" % (who, k.shape))
    if k.shape[0] == 1:
        k = np.repeat(k, I, axis=0)
    if k.shape[0] != I:
        raise ValueError("%s: %d images, %d camera matrices" % (who, I, k.shape[0]))
    if not (np.isfinite(k).all() and (k[:, :2] > 0).all()):
        raise ValueError("%s: focal lengths must be finite and > 0, the principal point finite" % who)
    return np.ascontiguousarray(k.astype(np.float32))


def _kmat(K, I, dev, who):
    import torch
    from . import ops
    if torch.is_tensor(K):                       # a device tensor is taken as [I,4] (nothing is read back to check a matrix)
        if K.dim() != 2 or tuple(K.shape) != (I, 4):
            raise ValueError("%s: a tensor K is float32 [I,4] = (fx, fy, cx, cy), not %s" % (who, tuple(K.shape)))
        return ops._t(K, torch.float32, dev)
    return ops._t(intrinsics4(K, I, who), torch.float32, dev)


def fit_plane(depth, K, seeds, num_hyp=NUM_HYP, tau=TAU):
    """The plane with the most inliers among num_hyp three-pixel hypotheses per image (cppf_plane_fit).  depth float32 [I,H,W]
    or [H,W] (metres; host array or device tensor), K as intrinsics4 takes it (or a float32 [I,4] device tensor), seeds: one
    integer per image (or one for all): an image's plane depends on its own seed and pixels only, never on its place in the
    batch.  Returns (float32 [I,4] device tensor (n, d) with n . p + d = 0 and the camera on the positive side, zeros when no
    hypothesis was usable; int32 [I,4] device tensor: winning hypothesis or -1, its inliers, usable hypotheses, valid pixels).
    No host synchronisation."""
    import torch
    from . import _lib, hostargs, ops
    num_hyp, tau = int(num_hyp), float(tau)
    if not 1 <= num_hyp <= MAX_HYP:
        raise ValueError("segment.fit_plane: num_hyp must be in 1 .. %d, not %d" % (MAX_HYP, num_hyp))
    if not (tau > 0.0 and np.isfinite(tau)):
        raise ValueError("segment.fit_plane: tau must be a finite distance > 0, not %r" % tau)
    sd = None
    if not torch.is_tensor(seeds):
        try:                                     # through Python integers: a list that mixes small seeds and ones above 2^63 stays exact
            sd = np.array([int(s_) for s_ in (seeds if np.ndim(seeds) else [seeds])], dtype=np.uint64)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("segment.fit_plane: seeds are integers in [0, 2^64), not %r" % (seeds,)) from None
    dev = ops._dev()
    dt = hostargs.image_batch(depth, dev, "segment.fit_plane", max_images=MAX_IMAGES)
    I, H, W = (int(x) for x in dt.shape)
    if sd is None:
        st = seeds.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
    else:
        sd = np.repeat(sd, I) if sd.size == 1 else sd
        st = torch.from_numpy(sd.view(np.int64).copy()).to(dev)
    if st.numel() != I:
        raise ValueError("segment.fit_plane: %d images, %d seeds" % (I, st.numel()))
    km = _kmat(K, I, dev, "segment.fit_plane")
    plane = torch.empty((I, 4), dtype=torch.float32, device=dev)
    stats = torch.empty((I, 4), dtype=torch.int32, device=dev)
    L = _lib.load()
    need = int(L.cppf_plane_fit_workspace_bytes(I, num_hyp))
    ws = hostargs.scratch(need, dev, "cppf_plane_fit_workspace_bytes", _lib.CppfError)
    _lib.check(L.cppf_plane_fit(I, H, W, ops._p(dt), ops._p(km), ops._p(st), num_hyp, C.c_float(tau), ops._p(plane), ops._p(stats),
                                ops._p(ws), need, ops._stream()), "cppf_plane_fit")
    return plane, stats


def foreground(depth, K, plane, min_height=MIN_HEIGHT, max_height=0.0):
    """uint8 [I,H,W] device tensor: 255 where the depth is positive and finite and the pixel's height above `plane` (float32
    [I,4] or [4], fit_plane's) is > min_height and, when max_height > 0, <= max_height (cppf_plane_foreground).  An image whose
    plane is all zeros keeps every valid pixel.  No host synchronisation."""
    import torch
    from . import _lib, hostargs, ops
    min_height, max_height = float(min_height), float(max_height)
    if np.isnan(min_height) or np.isnan(max_height):
        raise ValueError("segment.foreground: min_height and max_height are distances, not NaN")
    dev = ops._dev()
    dt = hostargs.image_batch(depth, dev, "segment.foreground", max_images=MAX_IMAGES)
    I, H, W = (int(x) for x in dt.shape)
    pl = ops._t(plane, torch.float32, dev).reshape(-1, 4)
    if pl.shape[0] != I:
        raise ValueError("segment.foreground: %d images, %d planes" % (I, pl.shape[0]))
    km = _kmat(K, I, dev, "segment.foreground")
    fg = torch.empty((I, H, W), dtype=torch.uint8, device=dev)
    L = _lib.load()
    _lib.check(L.cppf_plane_foreground(I, H, W, ops._p(dt), ops._p(km), ops._p(pl), C.c_float(min_height), C.c_float(max_height),
                                       ops._p(fg), ops._stream()), "cppf_plane_foreground")
    return fg


def concave_checked(step=CONCAVE_STEP, angle=CONCAVE_ANGLE, floor=CONCAVE_FLOOR, reach=None, who="segment.concave_edges"):
    """The ConcaveSettings of these values (reach resolved), or ValueError naming the first one outside the kernel's limits."""
    try:
        if float(step) != int(float(step)):
            raise ValueError
        step, angle, floor = int(float(step)), float(angle), float(floor)
        reach = None if reach is None else float(reach)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s: step is a whole number, angle, floor and reach numbers" % who) from None
    if not 1 <= step <= CONCAVE_MAX_STEP:
        raise ValueError("%s: step is in 1 .. %d pixels, not %d" % (who, CONCAVE_MAX_STEP, step))
    if not 0.0 <= angle < 180.0:
        raise ValueError("%s: angle is a turn in [0, 180) degrees, not %r" % (who, angle))
    if not (floor >= 0.0 and math.isfinite(floor)):
        raise ValueError("%s: floor (metres) is finite and >= 0, not %r" % (who, floor))
    reach = step * _masks.JUMP if reach is None else reach
    if not (reach >= 0.0 and math.isfinite(reach)):
        raise ValueError("%s: reach (metres) is finite and >= 0, not %r" % (who, reach))
    return ConcaveSettings(step, angle, floor, reach)


def concave_from_flags(switch, values, spell=lambda name: "--" + name, switch_name="propose_concave", who="--propose_concave"):
    """The one place the flags become ConcaveSettings (depthweights.from_flags' shape).  switch: whether the concave cut was
    asked for; values: dict flag -> value or None over CONCAVE_FLAGS' keys.  None when the switch is off -- a sub-flag given
    without it is a ValueError --, else concave_checked() of the given values over the defaults."""
    given = [k for k in CONCAVE_FLAGS if values.get(k) is not None]
    if not switch:
        if given:
            raise ValueError("%s sets how concave edges are found: it needs %s" % (spell(given[0]), spell(switch_name)))
        return None
    return concave_checked(who=who, **{CONCAVE_FLAGS[k]: values[k] for k in given})


def concave_summary(settings, counts):
    """The reports' entry: the settings and the three counts summed over the images."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 3).sum(0)
    return dict(settings._asdict(), **{k: int(v) for k, v in zip(CONCAVE_COUNTS, c)})


def concave_edges(depth, K, fg=None, step=CONCAVE_STEP, angle=CONCAVE_ANGLE, floor=CONCAVE_FLOOR, reach=None):
    """fg without the locally concave pixels (cppf_concave_edges; the kernel's file states the definition, tests/concave_ref.py
    restates it).  depth float32 [I,H,W] or [H,W] (metres), K as fit_plane takes it, fg uint8 or bool of depth's shape or None
    (every valid pixel).  A valid pixel B is an edge when, along its row or its column, the pixels A and C at `step` pixels to
    either side are valid, lie within `reach` metres of B's depth (None: step * masks.JUMP), and B lies behind the chord AC by
    more than `floor` metres with a turn between BA and BC of more than `angle` degrees.  The profiles read the whole depth
    image, never only fg.  Returns (uint8 [I,H,W] device tensor: 255 where the pixel is valid, no edge and in fg; int64 [I,3]
    host array = (valid, edge, kept pixels) per image).  Reads the counts back."""
    import torch
    from . import _lib, hostargs, ops
    who = "segment.concave_edges"
    s = concave_checked(step, angle, floor, reach, who)
    dev = ops._dev()
    dt = hostargs.image_batch(depth, dev, who, max_dim=MAX_DIM)
    I, H, W = (int(x) for x in dt.shape)
    km = _kmat(K, I, dev, who)
    mk = None if fg is None else hostargs.mask_batch(fg, dt, dev, who, same_shape=True)
    keep = torch.empty((I, H, W), dtype=torch.uint8, device=dev)
    counts = torch.empty((I, 3), dtype=torch.int32, device=dev)
    k2 = math.tan(math.radians(s.angle) / 2.0) ** 2          # float64 here, float32 at the boundary
    L = _lib.load()
    _lib.check(L.cppf_concave_edges(I, H, W, ops._p(dt), ops._p(km), ops._p(mk), s.step, C.c_float(k2), C.c_float(s.floor ** 2),
                                    C.c_float(s.reach), ops._p(keep), ops._p(counts), ops._stream()), "cppf_concave_edges")
    return keep, counts.cpu().numpy().astype(np.int64)


def segments(fg, depth, img_idx=0, jump=_masks.JUMP, min_pixels=MIN_SEGMENT_PIXELS, max_segments=MAX_SEGMENTS):
    """The max_segments largest depth-connected components of each mask (cppf_mask_segments; masks.clean's pixel and
    neighbour rules): fg uint8 or bool [D,H,W] (non-zero = set), depth float32 [I,H,W] or [H,W], img_idx int [D] (or one for
    all).  Components of at least min_pixels pixels are ranked by size, descending, ties to the one whose first pixel in
    row-major order comes first.  Returns device tensors (uint8 [D,H,W]: the pixel's rank or 255; int32 [D,max_segments,6] =
    (label, pixels, x0, y0, x1, y1) per rank, the box inclusive, -1 in unused rows; int32 [D,4] = components, segments kept,
    components of at least min_pixels, valid pixels).  No host synchronisation."""
    import torch
    from . import _lib, hostargs, ops
    jump, min_pixels, M = float(jump), int(min_pixels), int(max_segments)
    if not (jump >= 0.0 and np.isfinite(jump)):
        raise ValueError("segment.segments: jump must be a finite distance >= 0, not %r" % jump)
    if min_pixels < 0:
        raise ValueError("segment.segments: min_pixels must be >= 0, not %d" % min_pixels)
    if not 1 <= M <= SEGMENTS_LIMIT:
        raise ValueError("segment.segments: max_segments must be in 1 .. %d, not %d" % (SEGMENTS_LIMIT, M))
    dev = ops._dev()
    dt = hostargs.image_batch(depth, dev, "segment.segments", max_images=MAX_IMAGES)
    I, H, W = (int(x) for x in dt.shape)
    mk = hostargs.mask_batch(fg, dt, dev, "segment.segments")
    D = int(mk.shape[0])
    if D > MAX_IMAGES:
        raise ValueError("segment.segments: at most %d masks per call, not %d" % (MAX_IMAGES, D))
    ii = hostargs.per_item(img_idx, D, torch.int32, dev, "segment.segments", "image indices")
    rank = torch.empty((D, H, W), dtype=torch.uint8, device=dev)
    seg = torch.empty((D, M, 6), dtype=torch.int32, device=dev)
    stats = torch.empty((D, 4), dtype=torch.int32, device=dev)
    if D == 0:
        return rank, seg, stats
    L = _lib.load()
    need = int(L.cppf_mask_segments_workspace_bytes(D, H, W, M))
    ws = hostargs.scratch(need, dev, "cppf_mask_segments_workspace_bytes", _lib.CppfError)
    _lib.check(L.cppf_mask_segments(D, I, H, W, ops._p(mk), ops._p(dt), ops._p(ii), C.c_float(jump), min_pixels, M, ops._p(rank),
                                    ops._p(seg), ops._p(stats), ops._p(ws), need, ops._stream()), "cppf_mask_segments")
    return rank, seg, stats


def propose(depth, K, seed=0, num_hyp=NUM_HYP, tau=TAU, min_height=MIN_HEIGHT, max_height=0.0, jump=_masks.JUMP,
            min_pixels=MIN_SEGMENT_PIXELS, max_segments=MAX_SEGMENTS, concave=None, plane=True):
    """Object masks of one depth image [H,W] (metres) that shows objects on a support plane: fit_plane with `seed`, foreground,
    segments.  concave: a ConcaveSettings record (concave_checked, concave_from_flags) or None; with it the foreground's locally
    concave pixels are removed before the labelling (concave_edges), which parts touching and stacked objects and cuts the
    contact line where it is.  plane=False (needs concave) fits no plane: every valid pixel is labelled, the table is itself a
    segment, and the report's plane is four zeros.  Returns (uint8 [P,H,W] device tensor: the proposals' masks, 255 / 0, in rank
    order (largest first); [dict(pixels, bbox [x, y, w, h], label)] per proposal; dict(n [3], d, inliers, usable_hypotheses,
    hypothesis, valid_pixels, components, large_components) of the plane and the labelling, with `concave` (the settings and the
    valid, edge and kept pixel counts) when concave is set).  Reads the results back once."""
    import torch
    from . import ops
    if len(tuple(depth.shape) if hasattr(depth, "shape") else np.shape(depth)) != 2:
        raise ValueError("segment.propose: one depth image [H,W], not %s" % (np.shape(depth),))
    if concave is not None and not isinstance(concave, ConcaveSettings):
        raise ValueError("segment.propose: concave is a segment.ConcaveSettings record (concave_checked or concave_from_flags), "
                         "not %r" % (concave,))
    if not plane and concave is None:
        raise ValueError("segment.propose: without a plane only concave edges part the objects from the table: "
                         "plane=False needs concave")
    d = ops._t(depth, torch.float32)                   # on the device once, for all stages
    fg = ccounts = None
    if plane:
        fitted, pstats = fit_plane(d, K, [int(seed)], num_hyp, tau)
        fg = foreground(d, K, fitted, min_height, max_height)
    if concave is not None:
        fg, ccounts = concave_edges(d, K, fg, *concave)
    rank, seg, stats = segments(fg, d, 0, jump, min_pixels, max_segments)
    sg, st = seg[0].cpu().numpy(), stats[0].cpu().numpy()
    if plane:
        pl, ps = fitted[0].cpu().numpy(), pstats[0].cpu().numpy()
    else:                                              # no plane, no hypothesis; the valid pixels are the concave cut's count
        pl, ps = np.zeros(4, np.float32), np.array([-1, 0, 0, ccounts[0, 0]], dtype=np.int64)
    P = int(st[1])
    ids = torch.arange(P, dtype=torch.uint8, device=rank.device).reshape(P, 1, 1)
    out = (rank[0][None] == ids).to(torch.uint8) * 255
    props = [dict(pixels=int(r[1]), bbox=[int(r[2]), int(r[3]), int(r[4] - r[2] + 1), int(r[5] - r[3] + 1)], label=int(r[0]))
             for r in sg[:P]]
    report = dict(n=[float(x) for x in pl[:3]], d=float(pl[3]), inliers=int(ps[1]), usable_hypotheses=int(ps[2]),
                  hypothesis=int(ps[0]), valid_pixels=int(ps[3]), components=int(st[0]), large_components=int(st[2]))
    if ccounts is not None:
        report["concave"] = concave_summary(concave, ccounts)
    return out, props, report


def detections(masks, obj_ids, scene_id, image_id):
    """The proposals' masks (bool or uint8 [P,H,W], host) once per object id, score 1.0, as bop_data.write_detections takes
    them: object-major, rank order within an object."""
    m = np.asarray(masks) != 0
    return [dict(scene_id=int(scene_id), image_id=int(image_id), category_id=int(o), bbox=_masks.bbox(p), score=1.0, time=-1.0,
                 size=(int(p.shape[0]), int(p.shape[1])), counts=_masks.rle_encode(p)) for o in obj_ids for p in m]


def main(argv=None):
    import argparse
    import json
    from PIL import Image
    from . import bop_data
    ap = argparse.ArgumentParser(prog="python -m cppf2_amd.segment", description="Mask proposals of one depth image as a BOP "
                                 "detections file: every proposal once per object id, score 1.0.")
    ap.add_argument("--depth", required=True, help="16-bit depth PNG")
    ap.add_argument("--depth-scale", type=float, default=1000.0, help="depth units per metre (default 1000)")
    ap.add_argument("--intrinsics", required=True, help="fx,fy,cx,cy or the nine entries of K, row-major")
    ap.add_argument("--obj-ids", required=True, help="comma-separated object ids the proposals may show")
    ap.add_argument("--scene-id", type=int, default=0)
    ap.add_argument("--image-id", type=int, default=0)
    ap.add_argument("--out", required=True, help="detections file to write")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--plane-hypotheses", type=int, default=NUM_HYP)
    ap.add_argument("--plane-tau", type=float, default=TAU)
    ap.add_argument("--plane-min-height", type=float, default=MIN_HEIGHT)
    ap.add_argument("--mask-jump", type=float, default=_masks.JUMP)
    ap.add_argument("--min-segment-pixels", type=int, default=MIN_SEGMENT_PIXELS)
    ap.add_argument("--max-proposals", type=int, default=MAX_SEGMENTS)
    ap.add_argument("--concave", action="store_true", help="remove the locally concave pixels before the labelling: touching and "
                    "stacked objects part (DESIGN.md section 35)")
    ap.add_argument("--concave-step", type=int, default=None, help="pixels between a profile's centre and its ends (default %d)"
                    % CONCAVE_STEP)
    ap.add_argument("--concave-angle", type=float, default=None, help="degrees (default %g)" % CONCAVE_ANGLE)
    ap.add_argument("--concave-floor", type=float, default=None, help="metres (default %g)" % CONCAVE_FLOOR)
    ap.add_argument("--concave-reach", type=float, default=None, help="metres (default: step x --mask-jump's default)")
    ap.add_argument("--no-plane", action="store_true", help="fit no support plane: a shelf, a bin, a tray (needs --concave)")
    a = ap.parse_args(argv)
    concave = concave_from_flags(a.concave, {k_: getattr(a, k_) for k_ in CONCAVE_FLAGS}, lambda name: "--" + name.replace("_", "-"),
                                 "concave", "--concave")
    if a.no_plane and concave is None:
        raise ValueError("--no-plane leaves the concave edges to part the objects from the table: it needs --concave")
    k = [float(x) for x in a.intrinsics.split(",")]
    if len(k) not in (4, 9):
        raise ValueError("--intrinsics is fx,fy,cx,cy or the nine entries of K, not %d numbers" % len(k))
    K = np.asarray(k).reshape(3, 3) if len(k) == 9 else np.asarray(k)
    obj_ids = [int(x) for x in a.obj_ids.split(",") if x.strip()]
    if not obj_ids:
        raise ValueError("--obj-ids names no object")
    d = np.array(Image.open(a.depth))
    d = (d[..., 0] if d.ndim == 3 else d).astype(np.float64) / float(a.depth_scale)
    m, props, report = propose(d.astype(np.float32), K, a.seed, a.plane_hypotheses, a.plane_tau, a.plane_min_height, 0.0,
                               a.mask_jump, a.min_segment_pixels, a.max_proposals, concave=concave, plane=not a.no_plane)
    bop_data.write_detections(a.out, detections(m.cpu().numpy(), obj_ids, a.scene_id, a.image_id))
    print(json.dumps(dict(out=a.out, proposals=props, plane=report, detections=len(props) * len(obj_ids))))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
