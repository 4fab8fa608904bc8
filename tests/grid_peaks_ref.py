"""NumPy restatement of cppf_grid_peaks (include/cppf_hip.h): separated peaks of a centre-vote grid by greedy non-maximum
suppression.  Written from the definition, in integer arithmetic (float64 only for the world coordinates):

  peak 0 = the first maximum of the grid: the largest value, the lowest flat (C order) index on ties; index 0 for an all-zero
           grid; a scene whose ncell exceeds cells_cap received no votes: index 0, value 0xFFFFFFFF, one peak;
  peak k = the first maximum over the cells with a value > 0 that no earlier peak suppresses, where a cell (ix, iy, iz) is
           suppressed by a peak (px, py, pz) when (ix-px)^2 + (iy-py)^2 + (iz-pz)^2 <= sep_cells^2;
  no cell left: the remaining slots carry index -1, value 0 and NaN world coordinates;
  world = float64(c0) + float64(i) * res per axis.
"""
import numpy as np

GRID_DTYPE = np.dtype([("c0", "<f4", (3,)), ("g", "<i4", (3,)), ("ncell", "<i4"), ("flags", "<i4")])
SENTINEL = 0xFFFFFFFF


def world_of(c0, cell, res):
    return np.asarray(c0, dtype=np.float32).astype(np.float64) + np.asarray(cell, dtype=np.int64).astype(np.float64) * float(res)


def grid_peaks(values, g, c0, res, K, sep_cells, over=False):
    """One scene.  values: the grid's cells (any integer type, flat or [gx,gy,gz]); g = (gx, gy, gz); c0: the grid's corner
    (float32); over: the scene's ncell exceeds cells_cap (its cells are not read).  Returns (peak_idx int64 [K], peak_val uint32
    [K], peak_world float64 [K,3], n_peaks int)."""
    K, sep2 = int(K), int(sep_cells) ** 2
    g = tuple(int(x) for x in g)
    idx = np.full(K, -1, dtype=np.int64)
    val = np.zeros(K, dtype=np.uint32)
    world = np.full((K, 3), np.nan, dtype=np.float64)
    if over or g[0] * g[1] * g[2] <= 0:
        idx[0], val[0], world[0] = 0, (SENTINEL if over else 0), world_of(c0, (0, 0, 0), res)
        return idx, val, world, 1
    v = np.asarray(values).reshape(-1).astype(np.int64)
    assert v.size == g[0] * g[1] * g[2]
    ix, iy, iz = np.unravel_index(np.arange(v.size, dtype=np.int64), g)
    alive = v > 0
    n = 0
    for k in range(K):
        if k == 0:
            i = int(np.argmax(v))                              # the first maximum (index 0 when every cell is 0)
        else:
            if not alive.any():
                break
            i = int(np.argmax(np.where(alive, v, -1)))         # the first maximum over what is left
        p = (int(ix[i]), int(iy[i]), int(iz[i]))
        idx[k], val[k], world[k] = i, v[i], world_of(c0, p, res)
        n += 1
        alive &= (ix - p[0]) ** 2 + (iy - p[1]) ** 2 + (iz - p[2]) ** 2 > sep2
    return idx, val, world, max(n, 1)


def grid_peaks_batch(grid, grid_off, grids, cells_cap, res, K, sep_cells):
    """The batch as the entry point sees it.  grid: all scenes' cells (uint32 view of the buffer), grid_off int64 [B] (None:
    scene b at b * cells_cap), grids: GRID_DTYPE [B] (the CppfSceneGrid records).  Returns (peak_idx [B,K], peak_val [B,K],
    peak_world [B,K,3], n_peaks int32 [B])."""
    grids = np.asarray(grids)
    B = len(grids)
    out = (np.zeros((B, K), np.int64), np.zeros((B, K), np.uint32), np.zeros((B, K, 3), np.float64), np.zeros(B, np.int32))
    flat = np.asarray(grid).reshape(-1).view(np.uint32)
    for b in range(B):
        n = int(grids["ncell"][b])
        over = n > int(cells_cap)
        o = int(grid_off[b]) if grid_off is not None else b * int(cells_cap)
        cells = flat[o:o + n] if (not over and n > 0) else None
        g = grids["g"][b] if n > 0 else (0, 0, 0)
        out[0][b], out[1][b], out[2][b], out[3][b] = grid_peaks(cells, g, grids["c0"][b], res, K, sep_cells, over)
    return out
