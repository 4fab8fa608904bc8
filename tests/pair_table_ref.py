"""NumPy float32 / integer restatement of the pair-feature tables: key, payload, table assembly and draw,
written from the definitions, one float32 operation per line of the definition and in its order, so that the kernels' keys,
entries and bins can be compared bit for bit.  No transcendental except the host-side edges."""
import numpy as np

F32 = np.float32


def make_edges(na):
    """edges[j] = float32(cos(j pi / na)), j = 0 .. na."""
    return np.cos(np.arange(na + 1, dtype=np.float64) * np.pi / na).astype(F32)


def _dot(a, b):
    with np.errstate(all="ignore"):
        return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(F32) + a[:, 2] * b[:, 2]).astype(F32)


def angle_bin(c, na, edges):
    a = np.zeros(c.shape, dtype=np.int64)
    for j in range(1, na):
        a += c < edges[j]
    return a


def pair_keys(pts, normals, idx, pt_off, tup_off, nd, d_step, na, edges):
    """keys int32 [T] and the cell coordinates int64 [T,4] (bd, a1, a2, a3; meaningful where key >= 0)."""
    pts, normals = np.asarray(pts, dtype=F32), np.asarray(normals, dtype=F32)
    idx = np.asarray(idx).astype(np.int64)
    T = idx.shape[0]
    scene = np.searchsorted(np.asarray(tup_off), np.arange(T), side="right") - 1
    base = np.asarray(pt_off).astype(np.int64)[scene]
    i0, i1 = base + idx[:, 0], base + idx[:, 1]
    p0, p1, n0, n1 = pts[i0], pts[i1], normals[i0], normals[i1]
    d_step = F32(d_step)
    with np.errstate(all="ignore"):
        d = (p1 - p0).astype(F32)
        ln = np.sqrt(_dot(d, d)).astype(F32)
        c1 = (_dot(n0, d) / ln).astype(F32)
        c2 = (_dot(n1, d) / ln).astype(F32)
        c3 = _dot(n0, n1)
        finite = np.isfinite(np.concatenate([p0, p1, n0, n1], 1)).all(1)
        zero = (n0 == 0).all(1) | (n1 == 0).all(1)
        valid = finite & ~zero & (ln != 0) & (ln < F32(F32(nd) * d_step))
        bd = np.where(valid, ln / d_step, F32(0)).astype(F32).astype(np.int64)
    bd = np.minimum(bd, nd - 1)
    a1, a2, a3 = (angle_bin(c, na, edges) for c in (c1, c2, c3))
    key = ((bd * na + a1) * na + a2) * na + a3
    return np.where(valid, key, -1).astype(np.int32), np.stack([bd, a1, a2, a3], 1)


def canon_bins(x, nb):
    x = np.asarray(x, dtype=F32)
    c = np.fmin(np.fmax(x, F32(-0.5)), F32(0.5)).astype(F32)
    v = ((c + F32(0.5)).astype(F32) * F32(nb - 1)).astype(F32)
    return np.floor((v + F32(0.5)).astype(F32)).astype(np.int64)


def payload(canon, idx, pt_off, tup_off, nb):
    """uint8 [T,8]: the six bins of the canonical coordinates of the tuple's first two points, two zero bytes."""
    idx = np.asarray(idx).astype(np.int64)
    T = idx.shape[0]
    scene = np.searchsorted(np.asarray(tup_off), np.arange(T), side="right") - 1
    base = np.asarray(pt_off).astype(np.int64)[scene]
    canon = np.asarray(canon, dtype=F32)
    out = np.zeros((T, 8), dtype=np.uint8)
    out[:, 0:3] = canon_bins(canon[base + idx[:, 0]], nb)
    out[:, 3:6] = canon_bins(canon[base + idx[:, 1]], nb)
    return out


def assemble(keys, payloads, ncell):
    """(cell_off int32 [ncell+1], entries uint8 [E,8]): entries with key >= 0 in (key, entry id) order."""
    keys = np.asarray(keys)
    ids = np.nonzero(keys >= 0)[0]
    order = ids[np.argsort(keys[ids], kind="stable")]
    counts = np.bincount(keys[ids], minlength=ncell)
    cell_off = np.zeros(ncell + 1, dtype=np.int64)
    np.cumsum(counts, out=cell_off[1:])
    return cell_off.astype(np.int32), np.ascontiguousarray(np.asarray(payloads)[order]), order


def draw(keys, coords, tup_off, nd, na, cell_off, entries, u0):
    """bins int32 [T,6], hits int32 [B,3], source int [T] of every tuple from its key and cell coordinates."""
    keys = np.asarray(keys)
    T = keys.shape[0]
    E = entries.shape[0]
    cell_off = np.asarray(cell_off).astype(np.int64)
    strides = (na * na * na, na * na, na, 1)
    limits = (nd, na, na, na)
    start = np.zeros(T, dtype=np.int64)
    n = np.full(T, E, dtype=np.int64)
    source = np.full(T, 2, dtype=np.int64)
    for t in range(T):
        kk = int(keys[t])
        if kk < 0:
            continue
        if cell_off[kk + 1] > cell_off[kk]:
            start[t], n[t], source[t] = cell_off[kk], cell_off[kk + 1] - cell_off[kk], 0
            continue
        for c in range(4):
            for step in (-1, 1):
                v = int(coords[t, c]) + step
                if source[t] != 2 or v < 0 or v >= limits[c]:
                    continue
                nk = kk + step * strides[c]
                if cell_off[nk + 1] > cell_off[nk]:
                    start[t], n[t], source[t] = cell_off[nk], cell_off[nk + 1] - cell_off[nk], 1
    pick = (np.asarray(u0, dtype=F32) * n.astype(F32)).astype(F32).astype(np.int64)
    pick = np.maximum(np.minimum(pick, n - 1), 0)
    bins = entries[start + pick][:, :6].astype(np.int32)
    tup_off = np.asarray(tup_off)
    scene = np.searchsorted(tup_off, np.arange(T), side="right") - 1
    hits = np.zeros((len(tup_off) - 1, 3), dtype=np.int32)
    np.add.at(hits, (scene, source), 1)
    return bins, hits, source
