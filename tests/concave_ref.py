"""Plain restatement of cppf_concave_edges (cppf2_amd/csrc/cppf_segment.hip): the float32 arithmetic one
NumPy ufunc per operation (every operand float32, so every operation rounds to float32 where it is written), the host's
parameters as segment.concave_edges derives them, and the analytic scenes -- boxes on a table, ray-cast in float64 -- on which
the feature's claim is measured.  Test infrastructure only: product code does not import it."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import mask_ref as MR  # noqa: E402
import segment_ref as SR  # noqa: E402

F = np.float32
JUMP = 0.01                  # masks.JUMP
STEP, ANGLE, FLOOR = 3, 15.0, 0.002          # segment.CONCAVE_STEP, CONCAVE_ANGLE, CONCAVE_FLOOR (tests/test_concave.py compares)


def params(step=STEP, angle=ANGLE, floor=FLOOR, reach=None):
    """(step, k2, floor2, reach) as the entry point takes them: k2 = float32 of tan(angle / 2)^2 and floor2 = float32 of floor^2,
    both computed in float64; reach=None is step * JUMP."""
    step = int(step)
    reach = step * JUMP if reach is None else float(reach)
    return step, F(math.tan(math.radians(float(angle)) / 2.0) ** 2), F(float(floor) ** 2), F(reach)


def concave_profile(A, B, C, k2, floor2):
    """The verdict of profiles whose points A, B, C = (x, y, z) are float32 arrays (or scalars) of one shape:
    ob > 0 && 4 * oo > k2 * t3 && oo > floor2 * (tt * tt), in the kernel's order of operations."""
    A, B, C = ([np.asarray(v, dtype=F) for v in P] for P in (A, B, C))
    k2, floor2 = F(k2), F(floor2)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        u = [np.subtract(b, a) for a, b in zip(A, B)]
        t = [np.subtract(c, a) for a, c in zip(A, C)]
        tt = np.add(np.add(np.multiply(t[0], t[0]), np.multiply(t[1], t[1])), np.multiply(t[2], t[2]))
        ut = np.add(np.add(np.multiply(u[0], t[0]), np.multiply(u[1], t[1])), np.multiply(u[2], t[2]))
        o = [np.subtract(np.multiply(u[j], tt), np.multiply(t[j], ut)) for j in range(3)]
        ob = np.add(np.add(np.multiply(o[0], B[0]), np.multiply(o[1], B[1])), np.multiply(o[2], B[2]))
        oo = np.add(np.add(np.multiply(o[0], o[0]), np.multiply(o[1], o[1])), np.multiply(o[2], o[2]))
        t2 = np.multiply(tt, tt)
        t3 = np.multiply(t2, tt)
        assert all(v.dtype == F for v in (tt, ut, o[0], ob, oo, t3))
        return np.greater(ob, F(0)) & np.greater(np.multiply(F(4), oo), np.multiply(k2, t3)) & np.greater(oo, np.multiply(floor2, t2))


def edges(depth, K, step, k2, floor2, reach):
    """(valid bool [H,W], edge bool [H,W]) of one image: a pixel is an edge when it is valid and its profile along (0, 1) or
    along (1, 0) is concave; a profile gives a verdict only when A and C lie inside the image, all three pixels are valid and
    fabsf(zA - zB) <= reach, fabsf(zC - zB) <= reach."""
    x, y, z, valid = SR.points(depth, K)
    H, W = z.shape
    s, reach = int(step), F(reach)
    edge = np.zeros((H, W), dtype=bool)
    for dr, dc in ((0, 1), (1, 0)):
        if H - 2 * dr * s <= 0 or W - 2 * dc * s <= 0:
            continue                                           # no pixel has both neighbours inside the image

        def part(k):                                           # k = -1: A, 0: B, 1: C
            return slice(dr * s * (1 + k), H - dr * s * (1 - k)), slice(dc * s * (1 + k), W - dc * s * (1 - k))
        A, B, C = ([v[part(k)] for v in (x, y, z)] for k in (-1, 0, 1))
        with np.errstate(invalid="ignore", over="ignore"):
            near = (np.abs(np.subtract(A[2], B[2])) <= reach) & (np.abs(np.subtract(C[2], B[2])) <= reach)
        ok = valid[part(-1)] & valid[part(0)] & valid[part(1)] & near
        edge[part(0)] |= ok & concave_profile(A, B, C, k2, floor2)
    return valid, edge & valid


def concave_edges(depth, K, fg=None, step=STEP, angle=ANGLE, floor=FLOOR, reach=None):
    """(keep uint8 [H,W]: 255 where the pixel is valid, is no edge and (fg is None or fg != 0); counts int64 [3] = (valid, edge,
    kept pixels)) of one image, from the user's parameters."""
    valid, edge = edges(depth, K, *params(step, angle, floor, reach))
    kept = valid & ~edge
    if fg is not None:
        kept &= np.asarray(fg) != 0
    return np.where(kept, 255, 0).astype(np.uint8), np.array([valid.sum(), edge.sum(), kept.sum()], dtype=np.int64)


def propose(depth, K, seed, concave=None, plane=True, num_hyp=256, tau=0.005, min_height=0.01, jump=JUMP, min_pixels=200,
            max_segments=16):
    """segment.propose(..., concave=, plane=) restated: concave is None or dict(step, angle, floor, reach).  Returns
    segment_ref.propose's dict, with `keep` and `counts` when concave is set; the plane is four zeros when plane is False."""
    if plane:
        pl, pstats, _ = SR.fit_plane(depth, K, seed, num_hyp, tau)
        fg = SR.foreground(depth, K, pl, min_height)
    else:
        pl, pstats, fg = np.zeros(4, F), np.zeros(4, np.int32), None
    out = dict(plane=pl, pstats=pstats, fg=fg)
    mask = fg
    if concave is not None:
        mask, out["counts"] = concave_edges(depth, K, fg, **concave)
        out["keep"] = mask
    rank, seg, stats = SR.segments(mask, depth, jump, min_pixels, max_segments)
    P = int(stats[1])
    out.update(masks=np.stack([np.where(rank == k, 255, 0).astype(np.uint8) for k in range(P)]) if P
               else np.zeros((0,) + rank.shape, np.uint8), seg=seg[:P], stats=stats, rank=rank)
    return out


# ---- the scenes ---------------------------------------------------------------------------------------------------------------
H, W = 240, 320
K4 = (300.0, 300.0, 159.5, 119.5)
AZIMUTHS = (20.0, -50.0, 75.0)
ELEVATION, DISTANCE, TARGET = 35.0, 0.8, (0.0, 0.0, 0.04)
BOXES = dict(
    box=[((-.06, -.04, 0), (.06, .04, .08))],
    stacked=[((-.08, -.06, 0), (.08, .06, .06)), ((-.03, -.03, .06), (.03, .03, .12))],
    touching=[((-.10, -.04, 0), (0, .04, .08)), ((0, -.02, 0), (.08, .06, .05))],
)


def scene(name, az, sigma=0.0):
    """(depth float32 [240,320], owner int [240,320]: 0 the table, 1 + b box b) of BOXES[name] on the table z = 0, seen from
    0.8 m at 35 degrees of elevation and `az` degrees of azimuth, looking at (0, 0, 0.04): the camera-z of the nearest hit of
    each pixel's ray, float64 until the last cast.  sigma > 0: default_rng(0).normal(0, sigma) is added to the valid pixels."""
    el, a = math.radians(ELEVATION), math.radians(az)
    pos = DISTANCE * np.array([math.cos(el) * math.sin(a), -math.cos(el) * math.cos(a), math.sin(el)])
    f = np.asarray(TARGET) - pos
    f /= np.linalg.norm(f)
    right = np.cross(f, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    down = np.cross(f, right)
    fx, fy, cx, cy = K4
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    # a ray is pos + t * dir with dir's forward component 1: t is the hit's camera-z
    dirs = ((c - cx) / fx)[..., None] * right + ((r - cy) / fy)[..., None] * down + f
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dirs[..., 2] < 0, -pos[2] / dirs[..., 2], np.inf)
        depth, owner = t, np.where(np.isfinite(t), 0, -1)
        for b, (lo, hi) in enumerate(BOXES[name]):
            t0 = (np.asarray(lo, dtype=np.float64) - pos) / dirs                   # the slab method
            t1 = (np.asarray(hi, dtype=np.float64) - pos) / dirs
            near, far = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
            hit = (near <= far) & (near > 0) & (near < depth)
            depth, owner = np.where(hit, near, depth), np.where(hit, 1 + b, owner)
    depth = np.where(np.isfinite(depth), depth, 0.0)
    if sigma > 0:
        depth = np.where(depth > 0, depth + np.random.default_rng(0).normal(0.0, sigma, depth.shape), depth)
    return depth.astype(F), owner


def box_ious(mask, depth, owner, jump=JUMP, largest=12):
    """Per box of the scene: the best IoU of its visible pixels with one of the `largest` largest depth-connected components of
    `mask` (mask_ref.labels: masks.clean's pixel and neighbour rules)."""
    lab, sizes = MR.labels(mask, depth, jump)
    top = sorted(sizes, key=lambda l: (-sizes[l], l))[:largest]
    out = []
    for b in range(1, int(owner.max()) + 1):
        vis = owner == b
        best = 0.0
        for l in top:
            comp = lab == l
            best = max(best, float((comp & vis).sum()) / float((comp | vis).sum()))
        out.append(best)
    return out


def scene_ious(name, az, sigma=0.0, concave=True, step=STEP, angle=ANGLE, floor=FLOOR, reach=None, jump=JUMP):
    """(IoU per box, share of the valid pixels marked edge) of one scene; concave=False labels the valid pixels by depth jumps
    alone."""
    d, owner = scene(name, az, sigma)
    if not concave:
        return box_ious(SR.valid_pixels(d), d, owner, jump), 0.0
    keep, counts = concave_edges(d, K4, None, step, angle, floor, reach)
    return box_ious(keep, d, owner, jump), float(counts[1]) / float(counts[0])
