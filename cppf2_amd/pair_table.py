"""Pair-feature tables: vote from a mesh without trained weights.

For a known rigid object the six bins the tuple MLP predicts (the quantised canonical coordinates of a tuple's first two points)
are a lookup: key the pair by its point-pair feature (length and three angles from the points and the estimated normals), store
the canonical coordinates that model pairs with that key have, draw one such pair.  A PairTable is built from rendered views of
the mesh (render.make_items: the same normal estimator the scene will meet) with cppf_pair_keys; PairTable.draw fills a
VotingPipeline's bins with cppf_pair_table_draw, and every later stage consumes them unchanged.

    python -m cppf2_amd.pair_table --mesh obj.ply --mesh-scale 0.001 --out obj.npz
    python -m cppf2_amd.pair_table --bop-models <dataset>/models --out-dir tables      # obj_%06d.npz for every model

--sym-axis 0|1|2 canonicalises a continuous symmetry about that coordinate axis (render.make_items' sym_axis); --sym-axis auto
takes the axis from the mesh (cppf2_amd.symmetry.detect and coordinate_axis) or exits naming the axis it detected.
"""
from __future__ import annotations

import ctypes as C
import os
import time

import numpy as np

from . import _lib

# First guesses that nobody has measured against real data: the cell sizes (nd length bins over 1.02 diameters, na angle bins
# of 180 / na degrees) and the sampling of the model (views x tuples_per_view entries).  DESIGN.md section 20 records what the
# fixture mesh gives at these values; no sweep has been run.
ND, NA, NB = 32, 12, 256
VIEWS, TUPLES_PER_VIEW = 64, 20000
NB_MAX = 256
_ARRAYS = ("edges", "cell_off", "entries", "bound")
_SCALARS = (("nd", int), ("d_step", np.float32), ("na", int), ("nb", int), ("diameter", float))
_META = (("mesh", str), ("views", int), ("tuples_per_view", int), ("seed", int), ("res", float))


def make_edges(na):
    """float32 [na + 1]: edges[j] = float32(cos(j pi / na)), the angle-bin boundaries the kernels compare cosines with."""
    return np.cos(np.arange(int(na) + 1, dtype=np.float64) * np.pi / int(na)).astype(np.float32)


def check_geometry(nd, d_step, na, nb):
    nd, na, nb = int(nd), int(na), int(nb)
    if nd < 1:
        raise ValueError("pair table: nd must be >= 1, not %d" % nd)
    if not 2 <= na <= 1024:
        raise ValueError("pair table: na must be in [2, 1024], not %d" % na)
    if not 2 <= nb <= NB_MAX:
        raise ValueError("pair table: nb must be in [2, %d], not %d" % (NB_MAX, nb))
    if nd * na ** 3 >= 2 ** 31 - 1:
        raise ValueError("pair table: nd * na^3 = %d cells do not fit int32" % (nd * na ** 3))
    if not (np.isfinite(d_step) and float(d_step) > 0):
        raise ValueError("pair table: d_step must be finite and > 0, not %r" % (d_step,))
    return nd, na, nb


class PairTable:
    """nd, d_step, na, nb: the key's and the payload's geometry; edges float32 [na+1]; cell_off int32 [nd*na^3 + 1]; entries
    uint8 [E,8]; bound float32 [3] (the mesh's box extents in metres); diameter (the box diagonal, metres); meta: dict(mesh,
    views, tuples_per_view, seed, res).  Arrays are NumPy arrays or, after to(device), torch tensors."""

    def __init__(self, nd, d_step, na, nb, edges, cell_off, entries, bound, diameter, meta=None):
        self.nd, self.na, self.nb = check_geometry(nd, d_step, na, nb)
        self.d_step = np.float32(d_step)
        self.diameter = float(diameter)
        self.meta = dict(meta or {})
        self.edges, self.cell_off, self.entries, self.bound = edges, cell_off, entries, bound
        self._check_arrays()
        self._scales = None          # (Ttot, float32 [Ttot,3] on the device): bound broadcast to every pair, built by vote()
        self.last_hits = None        # draw()'s hit counts of the last vote() (device int32 [B,3])

    @property
    def ncell(self):
        return self.nd * self.na ** 3

    @property
    def E(self):
        return int(self.entries.shape[0])

    def _check_arrays(self):
        if tuple(self.edges.shape) != (self.na + 1,):
            raise ValueError("pair table: edges must have na + 1 = %d values, not %s" % (self.na + 1, tuple(self.edges.shape)))
        if tuple(self.cell_off.shape) != (self.ncell + 1,):
            raise ValueError("pair table: cell_off must have nd * na^3 + 1 = %d values, not %s" % (self.ncell + 1, tuple(self.cell_off.shape)))
        if self.entries.ndim != 2 or self.entries.shape[1] != 8:
            raise ValueError("pair table: entries must be [E, 8], not %s" % (tuple(self.entries.shape),))
        if tuple(self.bound.shape) != (3,):
            raise ValueError("pair table: bound must have 3 values")
        if isinstance(self.cell_off, np.ndarray):
            if self.edges.dtype != np.float32 or self.cell_off.dtype != np.int32 or self.entries.dtype != np.uint8 or self.bound.dtype != np.float32:
                raise ValueError("pair table: edges / bound float32, cell_off int32, entries uint8")
            off = self.cell_off.astype(np.int64)
            if off[0] != 0 or off[-1] != self.E or (np.diff(off) < 0).any():
                raise ValueError("pair table: cell_off must rise from 0 to the number of entries (%d)" % self.E)

    # -- files ----------------------------------------------------------------------------------
    def save(self, path):
        """One .npz of arrays and scalars (no pickled object)."""
        t = self.to(None)
        data = {k: getattr(t, k) for k in _ARRAYS}
        data.update({k: np.asarray(getattr(t, k), dtype=np.float32 if ty is np.float32 else (np.int64 if ty is int else np.float64))
                     for k, ty in _SCALARS})
        for k, ty in _META:
            v = t.meta.get(k, "" if ty is str else 0)
            data["meta_" + k] = np.asarray(v, dtype=np.str_ if ty is str else (np.int64 if ty is int else np.float64))
        with open(path, "wb") as f:
            np.savez(f, **data)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in _ARRAYS + tuple(k for k, _ in _SCALARS) if k not in z.files]
            if missing:
                raise ValueError("%s is not a pair table: no %s" % (path, ", ".join(missing)))
            meta = {k: ty(z["meta_" + k][()]) for k, ty in _META if "meta_" + k in z.files}
            return cls(int(z["nd"]), np.float32(z["d_step"]), int(z["na"]), int(z["nb"]), z["edges"], z["cell_off"], z["entries"],
                       z["bound"], float(z["diameter"]), meta)

    def to(self, device):
        """The table with its arrays on `device` (a torch device), or as NumPy arrays (device=None)."""
        import torch
        arrays = {}
        for k in _ARRAYS:
            a = getattr(self, k)
            if device is None:
                arrays[k] = a.cpu().numpy() if torch.is_tensor(a) else a
            else:
                arrays[k] = (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device).contiguous()
        return PairTable(self.nd, self.d_step, self.na, self.nb, arrays["edges"], arrays["cell_off"], arrays["entries"],
                         arrays["bound"], self.diameter, self.meta)

    # -- the draw -------------------------------------------------------------------------------
    def draw(self, pipe, pts, normals, idx, uniforms):
        """Fills pipe.bins (int32 [T,6]) from the table; returns hits int32 [B,3] (device): the tuples of each scene that took
        their own cell, a neighbouring cell, the whole table.  pts / normals float32 [Ntot,3], idx int32 [T,k], uniforms float32
        [T,6] (column 0 is read), all on pipe's device in pipe's batch layout; the table must be there too (to(device))."""
        import torch
        from . import ops
        if not torch.is_tensor(self.entries) or self.entries.device != pipe.bins.device:
            raise _lib.CppfError("PairTable.draw: move the table to the pipeline's device first (to(device))")
        if self.E == 0:
            raise _lib.CppfError("PairTable.draw: the table has no entries")
        for name, a, shape, dt in (("pts", pts, (pipe.Ntot, 3), torch.float32), ("normals", normals, (pipe.Ntot, 3), torch.float32),
                                   ("idx", idx, (pipe.Ttot, pipe.k), torch.int32), ("uniforms", uniforms, (pipe.Ttot, 6), torch.float32)):
            if tuple(a.shape) != shape or a.dtype != dt or not a.is_contiguous() or a.device != pipe.bins.device:
                raise _lib.CppfError("PairTable.draw: %s must be a contiguous %s %s tensor on the pipeline's device" % (name, dt, shape))
        L = _lib.load()
        hits = torch.zeros((pipe.B, 3), dtype=torch.int32, device=pipe.bins.device)
        _lib.check(L.cppf_pair_table_draw(pipe.B, ops._p(pts), ops._p(normals), ops._p(idx), pipe.k, ops._p(pipe.pt_off),
                                          ops._p(pipe.tup_off), pipe.Ttot, self.nd, C.c_float(self.d_step), self.na,
                                          ops._p(self.edges), ops._p(self.cell_off), ops._p(self.entries), self.E,
                                          ops._p(uniforms), ops._p(pipe.bins), ops._p(hits), ops._stream()), "cppf_pair_table_draw")
        return hits

    def vote(self, pipe, pts, normals, idx, uniforms, **kw):
        """draw(), then pipe.vote on the drawn bins with the mesh's box extents as every pair's scale.  Returns what
        pipe.vote returns (the device records); self.last_hits keeps draw()'s hit counts (device int32 [B,3])."""
        hits = self.draw(pipe, pts, normals, idx, uniforms)
        if self._scales is None or self._scales[0] != pipe.Ttot:
            self._scales = (pipe.Ttot, self.bound.to(pipe.bins.device).reshape(1, 3).expand(pipe.Ttot, 3).contiguous())
        self.last_hits = hits
        return pipe.vote(pts, idx, None, None, pred_scales=self._scales[1], nb=self.nb, **kw)


def pair_keys(pts, normals, idx, pt_off, tup_off, nd, d_step, na, edges, canon=None, nb=NB):
    """cppf_pair_keys on device tensors: keys int32 [T] (and payload uint8 [T,8] when canon, float32 [Ntot,3], is given)."""
    import torch
    from . import ops
    T, k = idx.shape
    keys = torch.empty((T,), dtype=torch.int32, device=pts.device)
    payload = torch.empty((T, 8), dtype=torch.uint8, device=pts.device) if canon is not None else None
    _lib.check(_lib.load().cppf_pair_keys(pt_off.numel() - 1, ops._p(pts), ops._p(normals), ops._p(canon), ops._p(idx), int(k),
                                          ops._p(pt_off), ops._p(tup_off), T, int(nd), C.c_float(d_step), int(na), ops._p(edges),
                                          int(nb), ops._p(keys), ops._p(payload), ops._stream()), "cppf_pair_keys")
    return (keys, payload) if canon is not None else keys


def assemble(keys, payload, ncell):
    """(cell_off int32 [ncell+1], entries uint8 [E,8]) from all keys / payloads in entry-id order (torch tensors): the entries
    with key >= 0 ordered by (key, entry id), cell_off the exclusive prefix of the entries per cell."""
    import torch
    ids = torch.nonzero(keys >= 0).reshape(-1)
    kv = keys[ids].long()
    order = torch.sort(kv, stable=True)[1]
    counts = torch.bincount(kv, minlength=int(ncell))
    cell_off = torch.zeros((int(ncell) + 1,), dtype=torch.int64, device=keys.device)
    cell_off[1:] = torch.cumsum(counts, 0)
    return cell_off.to(torch.int32), payload[ids[order]].contiguous()


def mesh_box(mesh):
    """(bound float32 [3], diameter): the mesh's box extents in metres and their diagonal -- no pair of the model is longer."""
    b = mesh.bounds
    bound = (np.asarray(b[1], dtype=np.float64) - np.asarray(b[0], dtype=np.float64))
    return bound.astype(np.float32), float(np.linalg.norm(bound))


def view_batch(mesh, view_ids, tuples_per_view, seed, full_rot, res, num_more, sym_axis, dev):
    """The device tensors of a batch of rendered views: dict(pts, normals, canon, idx, pt_off, tup_off, items).  View v's tuples
    are ops.sample_tuples' table of scene id v."""
    import torch
    from . import ops, render
    items = render.make_items(mesh, view_ids, seed=seed, full_rot=full_rot, res=res, num_more=num_more, sym_axis=sym_axis)
    counts = [it["pc"].shape[0] for it in items]
    cat = (lambda key: torch.from_numpy(np.concatenate([it[key] for it in items]).astype(np.float32)).to(dev).contiguous())
    idx = torch.cat([ops.sample_tuples(n, tuples_per_view, 2 + num_more, seed, (int(v),), dev) for v, n in zip(view_ids, counts)])
    return dict(pts=cat("pc"), normals=cat("normal"), canon=cat("pc_canon"), idx=idx, pt_off=ops._offsets(counts, dev),
                tup_off=ops._offsets([tuples_per_view] * len(items), dev), items=items)


def build(mesh, views=VIEWS, tuples_per_view=TUPLES_PER_VIEW, seed=0, full_rot=True, res=2e-3, num_more=3, sym_axis=None, nd=ND,
          na=NA, nb=NB, batch=64, name=""):
    """The table of a render.Mesh (in metres): `views` rendered views (ids 0 .. views-1 of render.make_items at `seed`),
    tuples_per_view tuples each; entry id = view * tuples_per_view + tuple.  Returns a PairTable on the host."""
    import torch
    from . import ops
    views, tuples_per_view = int(views), int(tuples_per_view)
    if views < 1 or tuples_per_view < 1:
        raise ValueError("pair table: views and tuples_per_view must be >= 1")
    bound, diameter = mesh_box(mesh)
    nd, na, nb = check_geometry(nd, 1.0, na, nb)
    d_step = np.float32(1.02 * diameter / nd)
    check_geometry(nd, d_step, na, nb)               # (a degenerate mesh: d_step 0)
    dev = ops._dev()
    edges_np = make_edges(na)
    edges = torch.from_numpy(edges_np).to(dev)
    t0 = time.perf_counter()
    keys, payloads = [], []
    for a in range(0, views, int(batch)):
        vb = view_batch(mesh, list(range(a, min(a + int(batch), views))), tuples_per_view, seed, full_rot, res, num_more, sym_axis, dev)
        k_, p_ = pair_keys(vb["pts"], vb["normals"], vb["idx"], vb["pt_off"], vb["tup_off"], nd, d_step, na, edges, vb["canon"], nb)
        keys.append(k_)
        payloads.append(p_)
    cell_off, entries = assemble(torch.cat(keys), torch.cat(payloads), nd * na ** 3)
    meta = dict(mesh=str(name), views=views, tuples_per_view=tuples_per_view, seed=int(seed), res=float(res))
    table = PairTable(nd, d_step, na, nb, edges_np, cell_off.cpu().numpy(), entries.cpu().numpy(), bound, diameter, meta)
    table.build_seconds = time.perf_counter() - t0
    return table


def main(argv=None):
    import argparse
    from . import render
    ap = argparse.ArgumentParser(description="Build pair-feature tables from meshes (DESIGN.md section 20)")
    ap.add_argument("--mesh")
    ap.add_argument("--mesh-scale", type=float, default=None, help="mesh units -> metres (default: 1 with --mesh, 0.001 with --bop-models)")
    ap.add_argument("--out")
    ap.add_argument("--bop-models", help="a BOP dataset's models directory (obj_%%06d.ply): one table per model")
    ap.add_argument("--out-dir")
    ap.add_argument("--views", type=int, default=VIEWS)
    ap.add_argument("--tuples", type=int, default=TUPLES_PER_VIEW)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sym-axis", default=None,
                    help="0, 1 or 2: the coordinate axis of a continuous symmetry (map_sym); auto: detected (cppf2_amd.symmetry)")
    a = ap.parse_args(argv)
    if a.sym_axis is not None and a.sym_axis != "auto":
        try:
            a.sym_axis = int(a.sym_axis)
        except ValueError:
            ap.error("--sym-axis is 0, 1, 2 or auto, not %r" % (a.sym_axis,))
    if bool(a.mesh) == bool(a.bop_models):
        ap.error("give --mesh with --out, or --bop-models with --out-dir")
    if a.mesh:
        if not a.out:
            ap.error("--mesh needs --out")
        jobs = [(a.mesh, a.out)]
    else:
        if not a.out_dir:
            ap.error("--bop-models needs --out-dir")
        os.makedirs(a.out_dir, exist_ok=True)
        names = sorted(n for n in os.listdir(a.bop_models) if n.startswith("obj_") and n.endswith(".ply"))
        if not names:
            ap.error("no obj_*.ply under %s" % a.bop_models)
        jobs = [(os.path.join(a.bop_models, n), os.path.join(a.out_dir, n[:-4] + ".npz")) for n in names]
    scale = a.mesh_scale if a.mesh_scale is not None else (1.0 if a.mesh else 0.001)
    for path, out in jobs:
        sym_axis = a.sym_axis
        if sym_axis == "auto":
            from . import symmetry
            try:
                sym_axis = symmetry.coordinate_axis(symmetry.detect(render.load_mesh(path, scale)))
            except ValueError as e:
                raise SystemExit("%s: %s" % (os.path.basename(path), e))
            print("%s: --sym-axis auto chose coordinate axis %d" % (os.path.basename(path), sym_axis))
        t = build(render.load_mesh(path, scale), a.views, a.tuples, a.seed, sym_axis=sym_axis, name=os.path.basename(path))
        t.save(out)
        print("%s: %d entries in %d of %d cells, %.1f s -> %s" % (os.path.basename(path), t.E, int((np.diff(t.cell_off) > 0).sum()),
                                                                 t.ncell, t.build_seconds, out))


if __name__ == "__main__":
    main()
