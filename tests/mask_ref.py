"""Plain restatements for the mask layer (cppf2_amd/masks.py, cppf_rle_decode, cppf_mask_components): COCO's run-length decode
one run at a time, and the largest depth-connected component by breadth-first search in row-major order.  Test infrastructure
only: product code does not import it."""
from collections import deque

import numpy as np


def decode(counts, H, W):
    """uint8 [H,W] (255 / 0): the runs are column-major and alternate 0s and 1s, starting with 0s."""
    flat = np.zeros(H * W, dtype=np.uint8)
    p = 0
    for k, n in enumerate(counts):
        assert n >= 0 and p + n <= H * W
        if k & 1:
            flat[p:p + n] = 255
        p += n
    assert p == H * W
    out = np.zeros((H, W), dtype=np.uint8)
    for c in range(W):
        out[:, c] = flat[c * H:(c + 1) * H]
    return out


def valid_pixels(mask, depth):
    d = np.asarray(depth, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (np.asarray(mask) != 0) & (d > 0) & np.isfinite(d)


def labels(mask, depth, jump):
    """(label int64 [H,W]: the lowest flat index of the pixel's component, -1 where not valid; sizes {label: pixels}).  Valid:
    mask != 0 and depth > 0 and finite.  Valid 4-neighbours are connected when |d_a - d_b| <= jump, the difference one float32
    subtraction and jump rounded to float32."""
    d = np.asarray(depth, dtype=np.float32)
    H, W = d.shape
    v = valid_pixels(mask, d)
    j = np.float32(jump)
    with np.errstate(invalid="ignore", over="ignore"):
        right = v[:, :-1] & v[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= j)          # (r, c) -- (r, c + 1)
        down = v[:-1, :] & v[1:, :] & (np.abs(d[:-1, :] - d[1:, :]) <= j)           # (r, c) -- (r + 1, c)
    right, down, vl = right.tolist(), down.tolist(), v.tolist()
    lab = [[-1] * W for _ in range(H)]
    sizes = {}
    for r0 in range(H):
        for c0 in range(W):
            if not vl[r0][c0] or lab[r0][c0] >= 0:
                continue
            me = r0 * W + c0                                   # row-major scan: the first pixel met is the lowest index
            lab[r0][c0] = me
            n = 0
            todo = deque([(r0, c0)])
            while todo:
                r, c = todo.popleft()
                n += 1
                if c + 1 < W and right[r][c] and lab[r][c + 1] < 0:
                    lab[r][c + 1] = me; todo.append((r, c + 1))
                if c > 0 and right[r][c - 1] and lab[r][c - 1] < 0:
                    lab[r][c - 1] = me; todo.append((r, c - 1))
                if r + 1 < H and down[r][c] and lab[r + 1][c] < 0:
                    lab[r + 1][c] = me; todo.append((r + 1, c))
                if r > 0 and down[r - 1][c] and lab[r - 1][c] < 0:
                    lab[r - 1][c] = me; todo.append((r - 1, c))
            sizes[me] = n
    return np.asarray(lab, dtype=np.int64).reshape(H, W), sizes


def components(mask, depth, jump, min_pixels):
    """(out uint8 [H,W]: 255 on the kept component; stats int32 [4] = (components, kept label or -1, kept pixels, valid
    pixels)).  Kept: the component with the most pixels, ties to the lowest label, if it has at least min_pixels."""
    lab, sizes = labels(mask, depth, jump)
    kept, best = -1, 0
    for l in sorted(sizes):
        if sizes[l] > best and sizes[l] >= min_pixels:
            kept, best = l, sizes[l]
    out = np.where((lab == kept) & (kept >= 0), 255, 0).astype(np.uint8)
    return out, np.array([len(sizes), kept, best, int((lab >= 0).sum())], dtype=np.int32)
