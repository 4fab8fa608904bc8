"""Plain restatements for the proposal layer (cppf2_amd/segment.py; cppf_plane_fit, cppf_plane_foreground, cppf_mask_segments):
the float32 arithmetic of cppf2_amd/csrc/cppf_segment.hip one NumPy ufunc per operation (every operand float32, so every
operation rounds to float32 where it is written), Philox from oracle/cppf_oracle.py, labels from tests/mask_ref.py, ranking
and boxes in plain Python.  Test infrastructure only: product code does not import it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import mask_ref as MR  # noqa: E402
from oracle import cppf_oracle as O  # noqa: E402

F = np.float32
MIN_LEN = F(1e-12)
EXAMPLE = os.path.join(ROOT, "tests", "golden", "example_data")
EXAMPLE_DEPTH_SCALE = 10000.0       # the YCB-V frame's depth unit: 0.1 mm
REAL_SEED = 0                       # the plane seed of the real-frame tests: the first one tried, inside every bound


def example_frame():
    """(example_data/depth.png as float32 [480,640] in metres, mask.png restricted to valid depth)."""
    from PIL import Image
    d = (np.array(Image.open(os.path.join(EXAMPLE, "depth.png"))).astype(np.float64) / EXAMPLE_DEPTH_SCALE).astype(F)
    m = np.array(Image.open(os.path.join(EXAMPLE, "mask.png")))
    m = (m[..., 0] if m.ndim == 3 else m) > 0
    return d, m & valid_pixels(d)


def k4(K):
    """(fx, fy, cx, cy) float32 of a 3 x 3 matrix or of the four numbers."""
    k = np.asarray(K, dtype=np.float64)
    k = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]]) if k.shape == (3, 3) else k.reshape(4)
    return k.astype(F)


def valid_pixels(depth):
    d = np.asarray(depth, dtype=F)
    with np.errstate(invalid="ignore"):
        return (d > 0) & (d < np.inf)


def points(depth, K):
    """(x, y, z float32 [H,W], valid bool [H,W]): z = depth, x = ((float)c - cx) * z / fx, y = ((float)r - cy) * z / fy."""
    d = np.asarray(depth, dtype=F)
    H, W = d.shape
    fx, fy, cx, cy = k4(K)
    r, c = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x = np.divide(np.multiply(np.subtract(c, cx), d), fx)
        y = np.divide(np.multiply(np.subtract(r, cy), d), fy)
    assert x.dtype == F and y.dtype == F
    return x, y, d, valid_pixels(d)


def hypotheses(depth, K, seed, num_hyp):
    """(planes float32 [num_hyp,4] = (n, d), NaN rows where unusable; usable bool [num_hyp]).  Hypothesis h: Philox counter
    (h, 0, 0, 0), key = the halves of the seed; pixels (uint64)word_j * (H * W) >> 32; cross = (u.y * v.z - u.z * v.y,
    u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x) with u = b - a, v = c - a."""
    x, y, z, valid = points(depth, K)
    HW = x.size
    x, y, z, valid = x.reshape(-1), y.reshape(-1), z.reshape(-1), valid.reshape(-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = O.philox4x32(np.arange(num_hyp, dtype=np.uint64), 0, 0, 0, seed & 0xFFFFFFFF, seed >> 32)
    p = [((w[j].astype(np.uint64) * np.uint64(HW)) >> np.uint64(32)).astype(np.int64) for j in range(3)]
    a, b, c = ((x[q], y[q], z[q]) for q in p)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ux, uy, uz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
        vx, vy, vz = c[0] - a[0], c[1] - a[1], c[2] - a[2]
        kx = uy * vz - uz * vy
        ky = uz * vx - ux * vz
        kz = ux * vy - uy * vx
        ln = np.sqrt((kx * kx + ky * ky) + kz * kz)
        usable = (p[0] != p[1]) & (p[0] != p[2]) & (p[1] != p[2]) & valid[p[0]] & valid[p[1]] & valid[p[2]] & (ln > MIN_LEN)
        nx, ny, nz = kx / ln, ky / ln, kz / ln
        d = -((nx * a[0] + ny * a[1]) + nz * a[2])
        flip = d < 0
        nx, ny, nz, d = (np.where(flip, -v, v) for v in (nx, ny, nz, d))
    planes = np.stack([nx, ny, nz, d], axis=1).astype(F)
    assert all(v.dtype == F for v in (kx, ln, nx, d))
    planes[~usable] = np.nan
    return planes, usable


def heights(depth, K, plane):
    """float32 [H,W]: ((n.x * x + n.y * y) + n.z * z) + d."""
    x, y, z, _ = points(depth, K)
    nx, ny, nz, d = (F(v) for v in plane)
    with np.errstate(invalid="ignore", over="ignore"):
        h = ((nx * x + ny * y) + nz * z) + d
    assert h.dtype == F
    return h


def fit_plane(depth, K, seed, num_hyp, tau):
    """(plane float32 [4], stats int32 [4] = (winning hypothesis or -1, its inliers, usable hypotheses, valid pixels), counts
    int64 [num_hyp] (-1 where unusable)).  The winner has the most inliers, ties to the lowest index."""
    planes, usable = hypotheses(depth, K, seed, num_hyp)
    x, y, z, valid = points(depth, K)
    x, y, z = x[valid], y[valid], z[valid]
    tau = F(tau)
    counts = np.full(num_hyp, -1, dtype=np.int64)
    for h in np.flatnonzero(usable):
        nx, ny, nz, d = planes[h]
        with np.errstate(invalid="ignore", over="ignore"):
            counts[h] = int(np.count_nonzero(np.abs(((nx * x + ny * y) + nz * z) + d) <= tau))
    win, best = -1, -1
    for h in range(num_hyp):
        if usable[h] and counts[h] > best:
            win, best = h, int(counts[h])
    plane = planes[win].copy() if win >= 0 else np.zeros(4, dtype=F)
    return plane, np.array([win, max(best, 0), int(usable.sum()), int(valid.sum())], dtype=np.int32), counts


def foreground(depth, K, plane, min_height, max_height=0.0):
    """uint8 [H,W]: 255 where valid and height > min_height (and <= max_height when max_height > 0); a plane of four zeros
    keeps every valid pixel."""
    valid = valid_pixels(depth)
    plane = np.asarray(plane, dtype=F)
    if (plane == 0).all():
        return np.where(valid, 255, 0).astype(np.uint8)
    h = heights(depth, K, plane)
    with np.errstate(invalid="ignore"):
        above = h > F(min_height)
        if F(max_height) > 0:
            above &= h <= F(max_height)
    return np.where(valid & above, 255, 0).astype(np.uint8)


def segments(mask, depth, jump, min_pixels, max_segments):
    """(rank uint8 [H,W]: the rank of the pixel's component or 255; seg int32 [max_segments,6] = (label, pixels, x0, y0, x1, y1),
    -1 in unused rows; stats int32 [4] = (components, segments kept, components of at least min_pixels, valid pixels)).
    Ranked by size, descending, ties to the lowest label."""
    lab, sizes = MR.labels(mask, depth, jump)
    H, W = lab.shape
    big = sorted((l for l in sizes if sizes[l] >= min_pixels), key=lambda l: (-sizes[l], l))
    kept = big[:max_segments]
    rank = np.full((H, W), 255, dtype=np.uint8)
    seg = np.full((max_segments, 6), -1, dtype=np.int32)
    lab_l = lab.tolist()
    boxes = {l: [W, H, -1, -1] for l in kept}
    for r in range(H):
        row = lab_l[r]
        for c in range(W):
            b = boxes.get(row[c])
            if b is not None:
                b[0] = min(b[0], c); b[1] = min(b[1], r); b[2] = max(b[2], c); b[3] = max(b[3], r)
    for k, l in enumerate(kept):
        rank[lab == l] = k
        seg[k] = [l, sizes[l]] + boxes[l]
    return rank, seg, np.array([len(sizes), len(kept), len(big), int((lab >= 0).sum())], dtype=np.int32)


def propose(depth, K, seed, num_hyp=256, tau=0.005, min_height=0.01, max_height=0.0, jump=0.01, min_pixels=200, max_segments=16):
    """(masks uint8 [P,H,W] in rank order, seg rows of the kept ranks, plane, plane stats, segment stats, fg, rank)."""
    plane, pstats, _ = fit_plane(depth, K, seed, num_hyp, tau)
    fg = foreground(depth, K, plane, min_height, max_height)
    rank, seg, stats = segments(fg, depth, jump, min_pixels, max_segments)
    P = int(stats[1])
    out = np.stack([np.where(rank == k, 255, 0).astype(np.uint8) for k in range(P)]) if P else np.zeros((0,) + rank.shape, np.uint8)
    return dict(masks=out, seg=seg[:P], plane=plane, pstats=pstats, stats=stats, fg=fg, rank=rank)
