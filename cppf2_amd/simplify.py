"""A triangle mesh reduced on the GPU by vertex clustering with one quadric-optimal representative per cell (Lindstrom,
Out-of-core simplification of large polygonal models, SIGGRAPH 2000): the stage between a mesh with more
triangles than any image has pixels -- the marching-tetrahedra surface cppf2_amd.fuse extracts, a BOP `models` file -- and the
consumers that pay per triangle (the rasterizer, cppf_sym_deviation, the solid intervals).  The reference has no such step; BOP
ships a decimated `models_eval` beside `models` for the same reason.

    small, report = cluster(render.load_mesh("obj.ply", 0.001), cell=0.004)      # render.Mesh in, render.Mesh out
    a_to_b, b_to_a = deviation(mesh, small)                                      # sampled one-sided distances, metres
    python -m cppf2_amd.simplify --mesh obj.ply --mesh-scale 0.001 --cell 0.004 --out obj_small.ply [--report r.json]
    python -m cppf2_amd.simplify --bop-models <dataset>/models --cell 0.004 --out-dir <dataset>/models_eval

The kernels are cppf_cluster_keys and cppf_cluster_quadrics (include/cppf_hip_experimental.h; the definitions are stated in
cppf2_amd/csrc/cppf_simplify.hip and restated in tests/simplify_ref.py).  Opt-in everywhere: nothing uses a simplified mesh
unless it is handed one.  Not done: no edge collapse, no repair of non-manifold edges (they are counted), no target triangle
count (the caller gives the cell), no attributes.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

from . import _lib, hostargs, ops, render
from ._lib import CppfError

LAMBDA = 1e-3                    # the regulariser of the quadric's system, relative to the cluster's area (part of the definition)
KEY_BITS = 21                    # cells per axis: 2^21


def _host3(x):
    return (C.c_double * 3)(*[float(v) for v in np.asarray(x, dtype=np.float64).reshape(3)])


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize(dev)
    return time.perf_counter()


def _checked(cell, lam, origin):
    cell = float(np.float32(cell))
    if not (0 < cell < np.inf and 0 < float(lam) < np.inf):
        raise ValueError("simplify: cell and lam are positive and finite, not %r and %r" % (cell, lam))
    if origin is not None:
        origin = np.asarray(origin, dtype=np.float32).reshape(3)
        if not np.isfinite(origin).all():
            raise ValueError("simplify: the origin is finite, not %s" % (origin,))
    return cell, float(lam), origin


def cluster_keys(verts, origin, cell):
    """cppf_cluster_keys: int64 [N] device tensor, the cell i << 42 | j << 21 | k of each of the vertices float32 [N,3] on the
    lattice of `cell` at `origin` (rounded to float32), -1 for a vertex outside its 2^21 cells per axis or not finite."""
    dev = ops._dev()
    cell, _, origin = _checked(cell, LAMBDA, origin)
    v = hostargs.tensor(verts, torch.float32, dev).reshape(-1, 3)
    keys = torch.empty((v.shape[0],), dtype=torch.int64, device=dev)
    _lib.check(_lib.load().cppf_cluster_keys(ops._p(v), v.shape[0], _host3(origin), C.c_float(cell), ops._p(keys), ops._stream()),
               "cppf_cluster_keys")
    return keys


def cluster_quadrics(verts, faces, corners, seg_off, keys, origin, cell, lam=LAMBDA):
    """cppf_cluster_quadrics: float32 [C,3] device tensor, the representative of each cluster: verts float32 [N,3], faces int32
    [F,3], corners int32 [M] (3 f + j, sorted by cluster, ascending within one), seg_off int64 [C+1], keys int64 [C]."""
    dev = ops._dev()
    cell, lam, origin = _checked(cell, lam, origin)
    v = hostargs.tensor(verts, torch.float32, dev).reshape(-1, 3)
    f = hostargs.tensor(faces, torch.int32, dev).reshape(-1, 3)
    cn = hostargs.tensor(corners, torch.int32, dev).reshape(-1)
    so = hostargs.tensor(seg_off, torch.int64, dev).reshape(-1)
    k = hostargs.tensor(keys, torch.int64, dev).reshape(-1)
    if so.numel() != k.numel() + 1:
        raise ValueError("cluster_quadrics: %d segment offsets for %d clusters" % (so.numel(), k.numel()))
    pos = torch.empty((k.numel(), 3), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().cppf_cluster_quadrics(ops._p(v), v.shape[0], ops._p(f), f.shape[0], ops._p(cn), cn.numel(), ops._p(so),
                                                 ops._p(k), k.numel(), _host3(origin), C.c_float(cell), C.c_double(lam), ops._p(pos),
                                                 ops._stream()), "cppf_cluster_quadrics")
    return pos


def reduce_faces(cf):
    """The face rules on the clusters cf int64 [F,3] (a tensor on any device) of every corner: (kept int64 [F'] face indices,
    ascending, dict(collapsed, cancelled, multi)).
      - a face two of whose corners share a cluster is dropped (collapsed counts them);
      - the others are grouped by their sorted cluster triple; a group's net orientation is the number of even minus the number
        of odd permutations (of the sorted triple) among its faces;
      - a group of net 0 is removed entirely (cancelled counts its faces): it is a fin folded onto itself, and keeping one of its
        faces is what would open a closed surface;
      - otherwise the first face in input order with the majority orientation stays;
      - multi counts the groups with |net| > 1, the only place where a closed input can lose closedness."""
    cf = cf.reshape(-1, 3)
    a, b, c = cf[:, 0], cf[:, 1], cf[:, 2]
    degenerate = (a == b) | (b == c) | (c == a)
    idx = torch.nonzero(~degenerate).reshape(-1)
    counts = dict(collapsed=int(degenerate.sum()), cancelled=0, multi=0)
    if idx.numel() == 0:
        return idx, counts
    t = cf[idx]
    odd = ((t[:, 0] > t[:, 1]).to(torch.int64) + (t[:, 0] > t[:, 2]) + (t[:, 1] > t[:, 2])) & 1
    sign = 1 - 2 * odd
    _, group = torch.unique(torch.sort(t, 1).values, dim=0, return_inverse=True)
    group = group.reshape(-1)
    G = int(group.max()) + 1
    net = torch.zeros((G,), dtype=torch.int64, device=cf.device).index_add_(0, group, sign)
    majority = sign * net[group] > 0
    first = torch.full((G,), cf.shape[0], dtype=torch.int64, device=cf.device)
    first.scatter_reduce_(0, group[majority], idx[majority], reduce="amin")
    counts["cancelled"] = int((net[group] == 0).sum())
    counts["multi"] = int((net.abs() > 1).sum())
    return torch.sort(first[net != 0]).values, counts


def edge_counts(faces, n_verts):
    """(boundary edges, non-manifold edges) of faces int64 [F,3] (a tensor): undirected edges one face uses, more than two use."""
    if faces.numel() == 0:
        return 0, 0
    e = torch.sort(torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), 1).values
    _, n = torch.unique(e[:, 0] * max(int(n_verts), 1) + e[:, 1], return_counts=True)
    return int((n == 1).sum()), int((n > 2).sum())


def cluster(mesh, cell, origin=None, lam=LAMBDA):
    """(render.Mesh, report): `mesh` (a render.Mesh, metres) with the vertices of each cell of edge `cell` on the lattice at
    `origin` (default: the per-axis minimum, in float32, of the vertices the faces use) merged into one representative, the
    point that minimises the area-weighted squared distances to the planes of the cell's triangles, regularised by lam towards
    their area-weighted centroid and clamped into the cell (cppf_cluster_quadrics).  Vertices no face uses are dropped; a used
    vertex outside the lattice's 2^21 cells per axis (or not finite) is a ValueError that gives their number.  The faces follow
    reduce_faces' rules and keep their input order and winding; the output vertices are the clusters the surviving faces use,
    in key order.  Every point of the output lies within sqrt(3) cell of the input surface.  Deterministic.
    report: dict(vertices_in, vertices_out, triangles_in, triangles_out, collapsed, cancelled, multi, boundary_edges,
    nonmanifold_edges (edges more than two faces use: clustering can create them; counted, not repaired), cell, origin,
    seconds: dict(keys, sort, quadrics, faces))."""
    dev = ops._dev()
    cell, lam, origin = _checked(cell, lam, origin)
    t0 = _sync(dev)
    v, f = mesh.device(dev)
    v, f = v.contiguous(), f.to(torch.int32).contiguous()
    N, Fn = int(v.shape[0]), int(f.shape[0])
    fl = f.reshape(-1).to(torch.int64)
    used = torch.zeros((N,), dtype=torch.bool, device=dev)
    used[fl] = True
    if origin is None:
        origin = v[used].amin(0).cpu().numpy() if Fn else np.zeros(3, np.float32)
        if not np.isfinite(origin).all():
            raise ValueError("simplify.cluster: a vertex the faces use is not finite")
    keys = cluster_keys(v, origin, cell)
    used_keys = keys[used]
    bad = int((used_keys < 0).sum())
    if bad:
        raise ValueError("simplify.cluster: %d vertices that faces use lie outside the lattice of 2^%d cells of %g per axis at %s"
                         % (bad, KEY_BITS, cell, origin))
    t1 = _sync(dev)
    ukeys, inverse = torch.unique(used_keys, return_inverse=True)
    vc = torch.full((N,), -1, dtype=torch.int64, device=dev)
    vc[used] = inverse
    cf = vc[fl].reshape(-1, 3)
    Cn = int(ukeys.numel())
    corners = torch.sort(cf.reshape(-1), stable=True).indices.to(torch.int32)
    seg_off = torch.zeros((Cn + 1,), dtype=torch.int64, device=dev)
    if Cn:
        seg_off[1:] = torch.cumsum(torch.bincount(cf.reshape(-1), minlength=Cn), 0)
    t2 = _sync(dev)
    pos = cluster_quadrics(v, f, corners, seg_off, ukeys, origin, cell, lam)
    t3 = _sync(dev)
    kept, counts = reduce_faces(cf)
    used_c, new_f = torch.unique(cf[kept], return_inverse=True)
    out_v, out_f = pos[used_c], new_f.reshape(-1, 3)
    boundary, nonmanifold = edge_counts(out_f, out_v.shape[0])
    out = render.Mesh(out_v.cpu().numpy(), out_f.cpu().numpy(), mesh.scale)
    out.boundary_edges = boundary
    t4 = _sync(dev)
    report = dict(vertices_in=N, vertices_out=int(out.verts.shape[0]), triangles_in=Fn, triangles_out=int(out.faces.shape[0]),
                  boundary_edges=boundary, nonmanifold_edges=nonmanifold, cell=cell, origin=[float(x) for x in origin],
                  seconds=dict(keys=t1 - t0, sort=t2 - t1, quadrics=t3 - t2, faces=t4 - t3), **counts)
    return out, report


def deviation(a, b, count=1024, seed=0):
    """(a to b, b to a) in metres: the largest distance of `count` surface samples of one render.Mesh (symmetry.sample_surface,
    the seed used for both) to the triangles of the other, by cppf_sym_deviation with the identity map."""
    from . import symmetry
    ident = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(1, 12)

    def one_sided(p, q):
        _, _, _, tri, area = symmetry.surface_frame(p.verts, p.faces)
        queries = symmetry.sample_surface(tri, area, count, seed).astype(np.float32)
        tris = q.verts[q.faces].reshape(-1, 9).astype(np.float32)
        return float(symmetry.deviations(queries, tris, ident)[0])
    return one_sided(a, b), one_sided(b, a)


def write_mesh(path, mesh):
    """The mesh as a binary .ply in its file's units (vertices / mesh.scale): render.load_mesh(path, mesh.scale) gives the same
    float32 vertices and the same faces back."""
    from . import bop_data
    bop_data.write_ply(path, mesh.verts / mesh.scale, mesh.faces)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cppf2_amd.simplify", description=__doc__.split("\n\n")[0])
    ap.add_argument("--mesh", help="one .ply or .obj mesh")
    ap.add_argument("--mesh-scale", type=float, default=None, help="mesh units -> metres (default: 1 with --mesh, 0.001 with --bop-models)")
    ap.add_argument("--bop-models", help="a BOP dataset's models directory: every obj_%%06d.ply is simplified")
    ap.add_argument("--cell", type=float, required=True, help="the cell's edge in metres, e.g. 0.004")
    ap.add_argument("--lam", type=float, default=LAMBDA, help="the quadric's regulariser (default %g)" % LAMBDA)
    ap.add_argument("--out", help="with --mesh: the .ply to write, in the mesh's units")
    ap.add_argument("--out-dir", help="with --bop-models: the directory to write the obj_%%06d.ply into (a models_eval)")
    ap.add_argument("--report", default=None, help="write the report (with --bop-models: one per file name) as JSON here")
    a = ap.parse_args(argv)
    if bool(a.mesh) == bool(a.bop_models):
        ap.error("give --mesh or --bop-models")
    if not (a.cell > 0 and np.isfinite(a.cell)):
        ap.error("--cell is a positive length in metres")
    if not (a.lam > 0 and np.isfinite(a.lam)):
        ap.error("--lam is positive")
    scale = a.mesh_scale if a.mesh_scale is not None else (1.0 if a.mesh else 0.001)
    if not (scale > 0 and np.isfinite(scale)):
        ap.error("--mesh-scale is positive")
    if a.mesh:
        if not a.out or a.out_dir:
            ap.error("--mesh goes with --out")
        if not a.out.lower().endswith(".ply"):
            ap.error("--out is a .ply file")
        jobs = [(a.mesh, a.out)]
    else:
        if not a.out_dir or a.out:
            ap.error("--bop-models goes with --out-dir")
        if not os.path.isdir(a.bop_models):
            ap.error("%s: not a directory" % a.bop_models)
        names = sorted(n for n in os.listdir(a.bop_models) if n.startswith("obj_") and n.endswith(".ply"))
        if not names:
            ap.error("no obj_*.ply under %s" % a.bop_models)
        if os.path.abspath(a.out_dir) == os.path.abspath(a.bop_models):
            ap.error("--out-dir is another directory than --bop-models")
        jobs = [(os.path.join(a.bop_models, n), os.path.join(a.out_dir, n)) for n in names]
    for src, _ in jobs:
        if not os.path.exists(src):
            ap.error("%s: not found" % src)
    if a.out_dir:
        os.makedirs(a.out_dir, exist_ok=True)
    reports = {}
    for src, dst in jobs:
        small, rep = cluster(render.load_mesh(src, scale), a.cell, lam=a.lam)
        if not small.faces.shape[0]:
            raise CppfError("simplify: %s has no triangle left at --cell %g (every triangle lies within one cell)" % (src, a.cell))
        write_mesh(dst, small)
        reports[os.path.basename(src)] = rep
        print("%s: %d -> %d triangles, %d -> %d vertices, %d boundary edges, %d non-manifold edges -> %s"
              % (os.path.basename(src), rep["triangles_in"], rep["triangles_out"], rep["vertices_in"], rep["vertices_out"],
                 rep["boundary_edges"], rep["nonmanifold_edges"], dst), file=sys.stderr)
    out = reports[os.path.basename(a.mesh)] if a.mesh else reports
    if a.report:
        with open(a.report, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
