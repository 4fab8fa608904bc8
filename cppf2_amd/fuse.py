"""A mesh of an object without a CAD model, from posed depth views: the views (a turntable or hand-held
sequence with camera poses and masks, what BOP's model-free onboarding sequences provide) are fused into a truncated signed
distance volume, and the volume's zero surface is extracted by marching tetrahedra.  The reference has no such step: its
custom-object path starts from a mesh (train_custom.ipynb).

    vol = Volume.around(depths, masks, poses, K, voxel=0.002)
    integrate(vol, depths, poses, K, masks=masks)                   # any number of calls; images of one size and K per call
    mesh = extract(vol)                                             # render.Mesh, vertices welded; mesh.boundary_edges
    mesh, report = fuse_views(depths, masks, poses, K, voxel=0.002)
    python -m cppf2_amd.fuse --views <bop scene dir> --obj-id 15 --voxel 0.002 --out obj_000015.ply [--simplify-cell 0.006]
    python -m cppf2_amd.fuse --views <dir> --track --voxel 0.004 --out obj.ply          # only the first image's pose is used
    python -m cppf2_amd.fuse --views <dir> --join <dir of the object turned over> --voxel 0.004 --out obj.ply    # section 32
    closed, report = close(vol, plane=(a, b, c, d))                 # a new Volume: enclosed unseen space filled, cut at the plane
    mesh, report = fuse_views(depths, masks, poses, K, voxel=0.002, close=True, support_plane=(a, b, c, d))
    python -m cppf2_amd.fuse --views <dir> --voxel 0.002 --out obj.ply --close --support-plane auto [--support-lift 0.001]
    integrate(vol, depths, poses, K, masks=masks, weights=depthweights.weights(depths, K)[0])       # weighted by viewing angle
    mesh, report = fuse_views(depths, masks, poses, K, voxel=0.002, weighting=depthweights.checked())
    python -m cppf2_amd.fuse --views <dir> --voxel 0.002 --out obj.ply --weight-views [--weight-levels 16 --carve-weight 1]

The surface has one or two triangles per voxel it crosses; simplify_cell / --simplify-cell hands it to cppf2_amd.simplify
 before it is returned or written.

The kernels are cppf_tsdf_integrate and cppf_tsdf_extract (include/cppf_hip_experimental.h; the definitions are stated in
cppf2_amd/csrc/cppf_fuse.hip and restated in tests/fuse_ref.py).  Every observation counts once unless weighting / --weight-views
asks for weights by viewing angle (cppf2_amd/depthweights.py, cppf_tsdf_integrate_weighted).  Not done: no
weighting by distance, no colour.  What no view saw stays open (mesh.boundary_edges counts it) unless close / --close decides it (cppf_tsdf_close,
cppf2_amd/csrc/cppf_close.hip): unseen space that is enclosed becomes inside, the support plane cuts the
solid off where the object stands, and unseen space that reaches the volume's border stays open.  The poses are trusted as given; --track
(cppf2_amd/track.py) is for a sequence of which only the first pose is known: every later frame is aligned
to the volume built so far before it is integrated (cppf_tsdf_track).  No loop closure, no bundle adjustment.
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

TRUNC_VOXELS = 3.0               # the default truncation distance, in voxels
MAX_NODES = 1 << 27              # the entry points' limit on nx * ny * nz
MAX_VIEWS = 65536                # views per cppf_tsdf_integrate call
MAX_IMAGE = 16384                # H and W
INITIAL_CAPACITY = 1 << 16       # triangles of the first cppf_tsdf_extract call

_WS = hostargs.ScratchCache("cppf_tsdf_extract_workspace_bytes", CppfError)
_CLOSE_WS = hostargs.ScratchCache("cppf_tsdf_close_workspace_bytes", CppfError)


def _host3(x):
    return (C.c_double * 3)(*[float(v) for v in np.asarray(x, dtype=np.float64).reshape(3)])


class Volume:
    """The two device arrays of a signed distance volume: acc float32 [nx,ny,nz] (sum of the observations) and wsum int32
    [nx,ny,nz] (their number), z fastest; node (i,j,k) sits at origin + (i,j,k) * voxel in the object's frame, metres.  The sum
    and the count are kept, not the average, so that integrating views in one call or in several gives the same bytes.
    origin and voxel are rounded to float32 (what the kernels use); trunc defaults to 3 voxels; views counts what was integrated."""

    def __init__(self, origin, voxel, dims, trunc=None, dev=None):
        self.origin = np.asarray(origin, dtype=np.float32).astype(np.float64).reshape(3)
        self.voxel = float(np.float32(voxel))
        self.dims = tuple(int(d) for d in dims)
        self.trunc = float(np.float32(TRUNC_VOXELS * self.voxel if trunc is None else trunc))
        if len(self.dims) != 3 or min(self.dims) < 1:
            raise ValueError("Volume: dims are three positive node counts, not %s" % (dims,))
        if self.dims[0] * self.dims[1] * self.dims[2] > MAX_NODES:
            raise ValueError("Volume: %d x %d x %d nodes exceed the limit of %d" % (self.dims + (MAX_NODES,)))
        if not (np.isfinite(self.origin).all() and 0 < self.voxel < np.inf and 0 < self.trunc < np.inf):
            raise ValueError("Volume: origin is finite, voxel and trunc are positive and finite")
        dev = ops._dev() if dev is None else torch.device(dev)
        self.acc = torch.zeros(self.dims, dtype=torch.float32, device=dev)
        self.wsum = torch.zeros(self.dims, dtype=torch.int32, device=dev)
        self.views = 0

    @property
    def device(self):
        return self.acc.device

    @staticmethod
    def bounds(depths, masks, poses, K, pixel_offset=0.0, dev=None):
        """float64 [2,3]: the box, in the object's frame, of the masked pixels with a reading (every pixel with one when masks is
        None) back-projected through the ray of (c + pixel_offset, r + pixel_offset).  torch ops; not hot."""
        dev = ops._dev() if dev is None else torch.device(dev)
        d = hostargs.image_batch(depths, dev, "Volume.around")
        V, H, W = d.shape
        m = torch.ones_like(d, dtype=torch.bool) if masks is None else \
            hostargs.mask_batch(masks, d, dev, "Volume.around", same_shape=True) != 0
        P = hostargs.tensor(poses, torch.float64, dev).reshape(-1, 3, 4)
        if P.shape[0] != V:
            raise ValueError("Volume.around: %d poses for %d views" % (P.shape[0], V))
        fx, fy, cx, cy = hostargs.camera4(K)
        cols = torch.arange(W, dtype=torch.float64, device=dev) + float(pixel_offset)
        rows = torch.arange(H, dtype=torch.float64, device=dev) + float(pixel_offset)
        lo = torch.full((3,), float("inf"), dtype=torch.float64, device=dev)
        hi = -lo
        for v in range(V):
            z = d[v].to(torch.float64)
            ok = m[v] & (z > 0) & torch.isfinite(z)
            if not bool(ok.any()):
                continue
            r, c = torch.nonzero(ok, as_tuple=True)
            z = z[r, c]
            cam = torch.stack([(cols[c] - cx) * z / fx, (rows[r] - cy) * z / fy, z], 1)
            obj = (cam - P[v, :, 3]) @ P[v, :, :3]                    # R^T (x - t), written for row vectors
            lo, hi = torch.minimum(lo, obj.amin(0)), torch.maximum(hi, obj.amax(0))
        if not bool(torch.isfinite(lo).all()):
            raise ValueError("Volume.around: no masked pixel has a depth reading")
        return torch.stack([lo, hi]).cpu().numpy()

    @classmethod
    def around(cls, depths, masks, poses, K, voxel, margin=None, trunc=None, pixel_offset=0.0, dev=None):
        """The Volume of node spacing `voxel` around Volume.bounds(...), padded by `margin` (default trunc + voxel) on every side."""
        voxel = float(np.float32(voxel))
        trunc = float(np.float32(TRUNC_VOXELS * voxel if trunc is None else trunc))
        margin = trunc + voxel if margin is None else float(margin)
        b = cls.bounds(depths, masks, poses, K, pixel_offset, dev)
        lo, hi = b[0] - margin, b[1] + margin
        dims = np.ceil((hi - lo) / voxel).astype(np.int64) + 1
        return cls(lo, voxel, dims, trunc, dev)

    @property
    def unknown_share(self):
        """The share of nodes no view observed."""
        return float((self.wsum == 0).sum()) / float(self.wsum.numel())


def _device_of(volume):
    if volume.device.type != "cuda":
        raise CppfError("fuse: the volume lives on %s; the kernels need a HIP device and there is no CPU fallback" % volume.device)
    return volume.device


def integrate(volume, depths, poses, K, masks=None, pixel_offset=0.0, znear=render.ZNEAR, weights=None, carve_weight=1):
    """cppf_tsdf_integrate: adds the views depths [V,H,W] (metres; 0 = no reading) with poses [V,12] or [V,3,4] (model -> OpenCV
    camera), one camera matrix K and masks [V,H,W] (non-zero = the object; None: every pixel is) to the volume, in order.
    pixel_offset: 0 for sensor images (pixel (r,c) lies on the ray through (c,r), ops.backproject's convention), 0.5 for images
    from render.render_depth, which samples at pixel centres.  Images of another size or K go in another call.
    weights: uint8 [V,H,W] (depthweights.weights; None: cppf_tsdf_integrate, every observation counts once):
    cppf_tsdf_integrate_weighted adds an observation of the surface with its pixel's weight and the constant observation "free
    space" with carve_weight (0 .. 255), and skips a weight of 0.  The volume then holds the weighted sum and the sum of the
    weights, and every min_weight is a threshold in units of weight; wsum is int32 and the caller owns its total."""
    dev = _device_of(volume)
    d = hostargs.image_batch(depths, dev, "fuse.integrate", max_dim=MAX_IMAGE)
    V, H, W = d.shape
    m = None if masks is None else hostargs.mask_batch(masks, d, dev, "fuse.integrate", same_shape=True)
    P = hostargs.tensor(poses, torch.float32, dev).reshape(-1, 12)
    if P.shape[0] != V:
        raise ValueError("fuse.integrate: %d poses for %d views" % (P.shape[0], V))
    hK = hostargs.camera4(K)
    wt = None
    if weights is not None:
        wt = hostargs.tensor(weights, torch.uint8, dev)
        wt = wt.reshape((1,) + tuple(wt.shape)) if wt.dim() == 2 else wt
        if tuple(wt.shape) != (V, H, W):
            raise ValueError("fuse.integrate: weights %s for depths %s" % (tuple(wt.shape), (V, H, W)))
        if not 0 <= int(carve_weight) <= 255:
            raise ValueError("fuse.integrate: carve_weight is in 0 .. 255, not %r" % (carve_weight,))
    L = _lib.load()
    nx, ny, nz = volume.dims
    for a in range(0, V, MAX_VIEWS):
        n = min(MAX_VIEWS, V - a)
        grid = (H, W, hK, C.c_float(pixel_offset), _host3(volume.origin), C.c_float(volume.voxel), nx, ny, nz, C.c_float(volume.trunc),
                C.c_float(znear), ops._p(volume.acc), ops._p(volume.wsum), ops._stream())
        views = (n, ops._p(d[a:]), ops._p(m[a:] if m is not None else None), ops._p(P[a:]))
        if wt is None:
            _lib.check(L.cppf_tsdf_integrate(*views, *grid), "cppf_tsdf_integrate")
        else:
            _lib.check(L.cppf_tsdf_integrate_weighted(*views, ops._p(wt[a:]), int(carve_weight), *grid), "cppf_tsdf_integrate_weighted")
    volume.views += V
    return volume


def extract_triangles(volume, min_weight=1, capacity=None):
    """cppf_tsdf_extract: (tris float32 [T,9], keys int64 [T,3], status (triangles, cells that produced any), calls made) of the
    volume's zero surface, in the order cell, tetrahedron, triangle.  The buffers start at `capacity` triangles (default
    INITIAL_CAPACITY) and are grown to what status reports, once: at most two calls."""
    dev = _device_of(volume)
    nx, ny, nz = volume.dims
    L = _lib.load()
    ws = _WS.get(hostargs.stream_key(dev), int(L.cppf_tsdf_extract_workspace_bytes(nx, ny, nz)), dev)
    status = torch.zeros((2,), dtype=torch.int64, device=dev)
    cap = INITIAL_CAPACITY if capacity is None else int(capacity)
    for call in (1, 2):
        tris = torch.empty((cap, 9), dtype=torch.float32, device=dev)
        keys = torch.empty((cap, 3), dtype=torch.int64, device=dev)
        _lib.check(L.cppf_tsdf_extract(ops._p(volume.acc), ops._p(volume.wsum), _host3(volume.origin), C.c_float(volume.voxel), nx, ny,
                                       nz, int(min_weight), cap, ops._p(tris) if cap else None, ops._p(keys) if cap else None,
                                       ops._p(status), ops._p(ws), ws.numel(), ops._stream()), "cppf_tsdf_extract")
        needed, cells = (int(x) for x in status.cpu().tolist())
        if needed <= cap:
            return tris[:needed], keys[:needed], (needed, cells), call
        cap = needed
    raise CppfError("cppf_tsdf_extract: the triangle count changed between two calls on one volume")


def weld_by_key(tris, keys, drop_degenerate=True):
    """(verts float32 [N,3], faces int64 [F,3], boundary_edges) of triangles [T,9] and their vertex keys [T,3] (tensors on any
    device): one vertex per distinct key, in key order (equal keys carry equal bits, so the first occurrence stands for all);
    drop_degenerate drops the triangles two of whose vertices coincide (the same key, or a node of exactly 0, where several
    edges meet in one point); boundary_edges counts the undirected edges that one triangle only uses (0: a closed surface)."""
    keys = keys.reshape(-1)
    pos = tris.reshape(-1, 3)
    if keys.numel() == 0:
        return pos.new_zeros((0, 3)), keys.new_zeros((0, 3)), 0
    uniq, inverse = torch.unique(keys, return_inverse=True)
    first = torch.full((uniq.numel(),), keys.numel(), dtype=torch.int64, device=keys.device)
    first.scatter_reduce_(0, inverse, torch.arange(keys.numel(), device=keys.device), reduce="amin")
    verts = pos[first]
    faces = inverse.reshape(-1, 3)
    if drop_degenerate:
        p = verts[faces]
        same = (p[:, 0] == p[:, 1]).all(1) | (p[:, 1] == p[:, 2]).all(1) | (p[:, 2] == p[:, 0]).all(1)
        faces = faces[~same]
        used, faces = torch.unique(faces, return_inverse=True)         # vertices only dropped triangles used go too
        verts, faces = verts[used], faces.reshape(-1, 3)
    e = torch.cat([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e = torch.sort(e, 1).values
    _, counts = torch.unique(e[:, 0] * max(int(verts.shape[0]), 1) + e[:, 1], return_counts=True)
    return verts, faces, int((counts == 1).sum())


def extract(volume, min_weight=1, weld=True, drop_degenerate=True):
    """The volume's zero surface as a render.Mesh (vertices float64 of the kernel's float32, metres, object frame), wound
    counter-clockwise as seen from the outside.  weld=True merges the vertices by key and sets mesh.boundary_edges (edges used by
    one triangle only; 0 means closed) and drops triangles without area when drop_degenerate; weld=False returns three vertices per
    triangle, as emitted (boundary_edges None).  mesh.cells: the cells that produced triangles; mesh.extract_calls: 1 or 2."""
    tris, keys, (needed, cells), calls = extract_triangles(volume, min_weight)
    if weld:
        verts, faces, boundary = weld_by_key(tris, keys, drop_degenerate)
    else:
        verts, faces, boundary = tris.reshape(-1, 3), torch.arange(3 * needed, device=tris.device).reshape(-1, 3), None
    mesh = render.Mesh(verts.cpu().numpy(), faces.cpu().numpy())
    mesh.boundary_edges, mesh.cells, mesh.extract_calls = boundary, cells, calls
    return mesh


def unit_plane(plane, lift=0.0):
    """float64 [4]: the plane (a, b, c, d), a x + b y + c z + d = 0 with the object on the positive side, its normal scaled to
    unit length in float64 and the plane moved `lift` metres towards the object."""
    p = np.array(plane, dtype=np.float64).reshape(-1)
    lift = float(lift)
    if p.size != 4 or not np.isfinite(p).all():
        raise ValueError("fuse: a plane is four finite numbers a, b, c, d, not %r" % (plane,))
    n = float(np.linalg.norm(p[:3]))
    if not (n > 0 and np.isfinite(n)):
        raise ValueError("fuse: the plane's normal (a, b, c) is zero")
    if not (lift >= 0 and np.isfinite(lift)):
        raise ValueError("fuse: the lift is a length in metres >= 0, not %r" % lift)
    p = p / n
    p[3] -= lift
    return p


def plane_to_object(plane_cam, pose):
    """float64 [4]: a plane (n_c, d_c) of the camera frame in the object's frame of pose [12] or [3,4] (model -> camera):
    n_o = R^T n_c, d_o = n_c . t + d_c."""
    p = np.asarray(plane_cam, dtype=np.float64).reshape(4)
    P = np.asarray(pose, dtype=np.float64).reshape(3, 4)
    return np.concatenate([P[:, :3].T @ p[:3], [p[:3] @ P[:, 3] + p[3]]])


def close(volume, plane=None, min_weight=1):
    """cppf_tsdf_close: (closed Volume, report).  The new Volume has the geometry and `views` of `volume`,
    wsum 1 at every decided node (extract it with min_weight=1) and .state, a uint8 device tensor [nx,ny,nz]: 0 known, 1
    enclosed and never seen (filled as inside), 2 unseen and below the plane (outside), 3 unseen and connected to the volume's
    border (left unknown).  plane: (a, b, c, d) in the object's frame, metres, the object on the positive side (segment.fit_plane's
    orientation), normalised here in float64; None: no plane.  report: dict(known, filled, below, open, open_share, plane).
    `volume` is not written."""
    dev = _device_of(volume)
    if int(min_weight) < 1:
        raise ValueError("fuse.close: min_weight >= 1")
    p = None if plane is None else unit_plane(plane)
    out = Volume(volume.origin, volume.voxel, volume.dims, volume.trunc, dev)
    out.views = volume.views
    out.state = torch.empty(volume.dims, dtype=torch.uint8, device=dev)
    stats = torch.empty((4,), dtype=torch.int64, device=dev)
    nx, ny, nz = volume.dims
    L = _lib.load()
    ws = _CLOSE_WS.get(hostargs.stream_key(dev), int(L.cppf_tsdf_close_workspace_bytes(nx, ny, nz)), dev)
    _lib.check(L.cppf_tsdf_close(ops._p(volume.acc), ops._p(volume.wsum), _host3(volume.origin), C.c_float(volume.voxel), nx, ny, nz,
                                 C.c_float(volume.trunc), int(min_weight), None if p is None else (C.c_double * 4)(*p),
                                 ops._p(out.acc), ops._p(out.wsum), ops._p(out.state), ops._p(stats), ops._p(ws), ws.numel(),
                                 ops._stream()), "cppf_tsdf_close")
    known, filled, below, opened = (int(x) for x in stats.cpu().tolist())
    return out, dict(known=known, filled=filled, below=below, open=opened, open_share=opened / float(nx * ny * nz),
                     plane=None if p is None else [float(x) for x in p])


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize(dev)
    return time.perf_counter()


def _surface(volume, min_weight, close_it, support_plane, support_lift):
    """(mesh, close's report or None): the volume's surface; with close_it the surface of close(volume, the plane lifted by
    support_lift (default: half a voxel)) instead."""
    if not close_it:
        if support_plane is not None or support_lift is not None:
            raise ValueError("fuse: support_plane and support_lift belong to close=True")
        return extract(volume, min_weight), None
    lift = 0.5 * volume.voxel if support_lift is None else support_lift
    plane = None if support_plane is None else unit_plane(support_plane, lift)
    closed, report = close(volume, plane, min_weight)
    return extract(closed, 1), dict(report, lift=None if plane is None else float(lift))


def _report(volume, mesh, t_volume, t_integrate, t_extract):
    return dict(views=int(volume.views), dims=list(volume.dims), voxel=volume.voxel, trunc=volume.trunc,
                triangles=int(mesh.faces.shape[0]), vertices=int(mesh.verts.shape[0]), boundary_edges=int(mesh.boundary_edges),
                unknown_share=volume.unknown_share, seconds=dict(volume=t_volume, integrate=t_integrate, extract=t_extract))


def _finish(volume, mesh, seconds, simplify_cell, closed=None):
    """(mesh, report) of the mesh extracted from a volume.  With simplify_cell the mesh goes through simplify.cluster first, the
    cells on the voxel lattice (the origin is the volume's), and the report gains `simplify`, cluster's own report.  closed:
    _surface's report of the close stage, the report's `close` (None: no such stage, no such key)."""
    extra = {} if closed is None else dict(close=closed)
    if simplify_cell is None:
        return mesh, dict(_report(volume, mesh, *seconds), **extra)
    from . import simplify
    mesh, simplified = simplify.cluster(mesh, simplify_cell, origin=volume.origin)
    return mesh, dict(_report(volume, mesh, *seconds), simplify=simplified, **extra)


def _conditioned(result, conditioned):
    """(mesh, report) with the report's `condition` (depthfilter's summary; None: no such stage, no such key)."""
    mesh, report = result
    return mesh, report if conditioned is None else dict(report, condition=conditioned)


def _weighted(result, weighted):
    """(mesh, report) with the report's `weighting` (depthweights' summary; None: no such stage, no such key)."""
    mesh, report = result
    return mesh, report if weighted is None else dict(report, weighting=weighted)


def _weights_kw(w, weighting):
    """integrate's keyword arguments for a batch's weights (none when weighting is off: the call is what it always was)."""
    return {} if w is None else dict(weights=w, carve_weight=weighting.carve_weight)


def condition_batches(batches, condition):
    """read_views' batches with their depths conditioned (device tensors then), and the summary over all of them; (batches, None)
    as they are when condition is None."""
    if condition is None:
        return batches, None
    from . import depthfilter
    done = [depthfilter.apply(b["depths"], condition, "fuse") for b in batches]
    return [dict(b, depths=d) for b, (d, _) in zip(batches, done)], depthfilter.merged([c for _, c in done])


def fuse_views(depths, masks, poses, K, voxel, trunc=None, margin=None, min_weight=1, pixel_offset=0.0, znear=render.ZNEAR,
               volume=None, simplify_cell=None, close=False, support_plane=None, support_lift=None, condition=None, weighting=None):
    """Both stages on one batch of views: (mesh, report).  `volume`: an existing Volume to add to (else Volume.around the views).
    report: dict(views, dims, voxel, trunc, triangles, vertices, boundary_edges, unknown_share (nodes no view observed),
    seconds: dict(volume, integrate, extract)).  simplify_cell (metres; None: no such stage): the welded mesh goes through
    simplify.cluster with cells of that edge on the voxel lattice; triangles, vertices and boundary_edges then describe the
    simplified mesh and report["simplify"] is cluster's report (triangles_in: what was extracted).
    close=True: the volume goes through close() before it is extracted (the seconds count it under extract); support_plane (a, b,
    c, d) as close()'s plane (None: none), moved support_lift metres towards the object first (default: half a voxel; the mesh's
    bottom then lies that far above the plane).  report["close"] is close()'s report plus `lift`, and triangles, vertices and
    boundary_edges describe the closed mesh.
    condition: a depthfilter.Settings record (None: the readings as they are): the views are conditioned (depthfilter.condition,
    DESIGN.md section 33) before Volume.around and integrate see them, and report["condition"] holds the settings and the
    counts summed over the views.
    weighting: a depthweights.Settings record (None: every observation counts once): the views get weights by viewing angle
    (depthweights.weights, after conditioning when both are on) and are integrated with them;
    report["weighting"] holds the settings and the counts summed over the views, and min_weight is in units of weight (with 16
    levels one face-on view adds 16)."""
    from . import depthfilter, depthweights
    t0 = time.perf_counter()
    depths, conditioned = depthfilter.apply(depths, condition, "fuse.fuse_views")
    w, weighted = depthweights.apply(depths, K, weighting, pixel_offset, "fuse.fuse_views")
    if volume is None:
        volume = Volume.around(depths, masks, poses, K, voxel, margin, trunc, pixel_offset)
    t1 = _sync(volume.device)
    integrate(volume, depths, poses, K, masks, pixel_offset, znear, **_weights_kw(w, weighting))
    t2 = _sync(volume.device)
    mesh, closed = _surface(volume, min_weight, close, support_plane, support_lift)
    t3 = _sync(volume.device)
    return _weighted(_conditioned(_finish(volume, mesh, (t1 - t0, t2 - t1, t3 - t2), simplify_cell, closed), conditioned), weighted)


# ----------------------------------------------------------------------------------------------
# a BOP-format scene folder of views
# ----------------------------------------------------------------------------------------------
class ViewsError(ValueError):
    """A --views folder that cannot be read as one BOP-format scene."""


def read_views(views_dir, obj_id=None, mesh_scale=0.001, use_masks=True, first_pose_only=False, no_poses=False):
    """The views of one object in a BOP-format scene folder: scene_camera.json (cam_K, depth_scale), scene_gt.json (cam_R_m2c,
    cam_t_m2c in model units; read directly: no model file has to exist), depth/%06d.png and mask_visib/%06d_%06d.png.  obj_id:
    the object (None: the scene's only one).  Returns a list of batches dict(K, depths [V,H,W] float32 metres, masks [V,H,W]
    uint8 or None, poses [V,12] float32 model (metres) -> camera, im_ids), one per image size and K, in image order.
    first_pose_only (--track): an entry after the object's first may lack cam_R_m2c / cam_t_m2c; its pose is then NaN.
    no_poses (--join's folder): every entry may."""
    from PIL import Image
    gt_path, cam_path = os.path.join(views_dir, "scene_gt.json"), os.path.join(views_dir, "scene_camera.json")
    for p in (gt_path, cam_path):
        if not os.path.exists(p):
            raise ViewsError("%s: not found (a BOP-format scene folder has scene_gt.json and scene_camera.json)" % p)
    with open(gt_path) as f:
        gt = {int(k): v for k, v in json.load(f).items()}
    with open(cam_path) as f:
        cam = {int(k): v for k, v in json.load(f).items()}
    ids = sorted({int(g["obj_id"]) for lst in gt.values() for g in lst})
    if obj_id is None:
        if len(ids) != 1:
            raise ViewsError("%s: the scene shows objects %s; choose one with --obj-id" % (views_dir, ids))
        obj_id = ids[0]
    groups = {}
    for im in sorted(gt):
        for g_index, g in enumerate(gt[im]):
            if int(g["obj_id"]) != int(obj_id):
                continue
            if im not in cam:
                raise ViewsError("%s: image %d is in scene_gt.json but not in scene_camera.json" % (views_dir, im))
            dpath = os.path.join(views_dir, "depth", "%06d.png" % im)
            if not os.path.exists(dpath):
                raise ViewsError("%s: not found" % dpath)
            depth = (np.array(Image.open(dpath)).astype(np.float64) * float(cam[im].get("depth_scale", 1.0)) / 1000.0).astype(np.float32)
            mask = None
            if use_masks:
                mpath = os.path.join(views_dir, "mask_visib", "%06d_%06d.png" % (im, g_index))
                if not os.path.exists(mpath):
                    raise ViewsError("%s: not found (--no-masks fuses every pixel)" % mpath)
                mk = np.array(Image.open(mpath))
                mask = ((mk[..., 0] if mk.ndim == 3 else mk) > 0).astype(np.uint8)
                if mask.shape != depth.shape:
                    raise ViewsError("%s: mask %s for depth %s" % (mpath, mask.shape, depth.shape))
            K = np.asarray(cam[im]["cam_K"], dtype=np.float64).reshape(3, 3)
            if (no_poses or (first_pose_only and groups)) and not ("cam_R_m2c" in g and "cam_t_m2c" in g):
                R, t = np.full((3, 3), np.nan), np.full((3, 1), np.nan)
            else:
                R = np.asarray(g["cam_R_m2c"], dtype=np.float64).reshape(3, 3)
                t = np.asarray(g["cam_t_m2c"], dtype=np.float64).reshape(3, 1) * float(mesh_scale)
            b = groups.setdefault((K.tobytes(), depth.shape), dict(K=K, depths=[], masks=[], poses=[], im_ids=[]))
            b["depths"].append(depth)
            b["masks"].append(mask)
            b["poses"].append(np.hstack([R, t]).astype(np.float32).reshape(12))
            b["im_ids"].append(im)
    if not groups:
        raise ViewsError("%s: no image shows object %s (objects: %s)" % (views_dir, obj_id, ids))
    out = []
    for b in groups.values():
        out.append(dict(K=b["K"], depths=np.stack(b["depths"]), masks=np.stack(b["masks"]) if use_masks else None,
                        poses=np.stack(b["poses"]), im_ids=b["im_ids"]))
    return out


def auto_support_plane(batch, tau, pixel_offset=0.0, views_dir="the folder"):
    """The support plane of a read_views batch's first view in the object's frame (metres): segment.fit_plane (seed 0) on the
    whole depth image, taken over by that view's pose.  tau: the fit's inlier distance, the same statement of the table's noise
    as the lift.  pixel_offset as integrate's: the fit takes pixel (r, c) for the ray through (c, r), so the principal point
    moves by the offset.  ViewsError when the fit finds no plane."""
    from . import segment
    K = np.array(batch["K"], dtype=np.float64).reshape(3, 3)
    K[:2, 2] -= float(pixel_offset)
    plane, stats = segment.fit_plane(batch["depths"][:1], K, 0, tau=tau)
    plane, winner = plane.reshape(4).cpu().numpy().astype(np.float64), int(stats.reshape(4)[0])
    if winner < 0 or not np.isfinite(plane).all() or not np.linalg.norm(plane[:3]) > 0:
        raise ViewsError("%s: --support-plane auto found no plane in the first view's depth image (image %s); give the plane as "
                         "a,b,c,d" % (views_dir, batch["im_ids"][0]))
    return plane_to_object(plane, batch["poses"][0])


def _scene_plane(support_plane, support_lift, voxel, pixel_offset, batches, views_dir):
    """support_plane as given, or for "auto" the first view's fitted plane (inliers within the lift; half a voxel if that is
    None or 0)."""
    if not (isinstance(support_plane, str) and support_plane == "auto"):
        return support_plane
    tau = support_lift if support_lift else 0.5 * float(np.float32(voxel))
    return auto_support_plane(batches[0], tau, pixel_offset, views_dir)


def fuse_scene(views_dir, voxel, obj_id=None, trunc=None, min_weight=1, use_masks=True, pixel_offset=0.0, mesh_scale=0.001,
               simplify_cell=None, close=False, support_plane=None, support_lift=None, condition=None, weighting=None):
    """read_views fused into one volume (one integrate call per image size and K): (mesh in metres, report).  simplify_cell, close,
    support_plane and support_lift: as fuse_views'; support_plane "auto": auto_support_plane of the first view, found before
    anything is fused.  condition: as fuse_views'; every batch is conditioned right after it is read.  weighting: as
    fuse_views'; every batch gets its weights after that."""
    from . import depthweights
    batches, conditioned = condition_batches(read_views(views_dir, obj_id, mesh_scale, use_masks), condition)
    weighed = [depthweights.apply(b["depths"], b["K"], weighting, pixel_offset, "fuse.fuse_scene") for b in batches]
    weighted = None if weighting is None else depthweights.merged([c for _, c in weighed])
    support_plane = _scene_plane(support_plane, support_lift, voxel, pixel_offset, batches, views_dir)
    t0 = time.perf_counter()
    boxes = np.stack([Volume.bounds(b["depths"], b["masks"], b["poses"], b["K"], pixel_offset) for b in batches])
    voxel = float(np.float32(voxel))
    trunc = float(np.float32(TRUNC_VOXELS * voxel if trunc is None else trunc))
    lo, hi = boxes[:, 0].min(0) - (trunc + voxel), boxes[:, 1].max(0) + (trunc + voxel)
    volume = Volume(lo, voxel, np.ceil((hi - lo) / voxel).astype(np.int64) + 1, trunc)
    t1 = _sync(volume.device)
    for b, (w, _) in zip(batches, weighed):
        integrate(volume, b["depths"], b["poses"], b["K"], b["masks"], pixel_offset, **_weights_kw(w, weighting))
    t2 = _sync(volume.device)
    mesh, closed = _surface(volume, min_weight, close, support_plane, support_lift)
    t3 = _sync(volume.device)
    return _weighted(_conditioned(_finish(volume, mesh, (t1 - t0, t2 - t1, t3 - t2), simplify_cell, closed), conditioned), weighted)


def _plane_argument(text):
    """--support-plane: "auto" or the unit plane of "a,b,c,d"."""
    if text == "auto":
        return text
    try:
        return unit_plane([float(x) for x in text.split(",")])
    except ValueError as e:
        raise argparse.ArgumentTypeError("'auto' or four numbers a,b,c,d with a normal that is not zero (%s)" % e) from None


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cppf2_amd.fuse", description=__doc__.split("\n\n")[0])
    ap.add_argument("--views", required=True, help="one BOP-format scene folder: scene_camera.json, scene_gt.json, depth/, mask_visib/")
    ap.add_argument("--obj-id", type=int, default=None, help="the object to fuse (default: the scene's only one)")
    ap.add_argument("--voxel", type=float, required=True, help="node spacing in metres, e.g. 0.002")
    ap.add_argument("--trunc", type=float, default=None, help="truncation distance in metres (default: 3 voxels)")
    ap.add_argument("--min-weight", type=int, default=1,
                    help="observations a node needs to count as known; with --weight-views in units of weight: with 16 levels one "
                         "face-on view adds 16")
    ap.add_argument("--no-masks", action="store_true", help="fuse every pixel (no mask_visib/ is read)")
    ap.add_argument("--pixel-offset", type=float, default=0.0, help="0 for sensor images, 0.5 for images rendered at pixel centres")
    ap.add_argument("--mesh-scale", type=float, default=0.001, help="model units to metres (0.001: a model in mm, as BOP's)")
    ap.add_argument("--simplify-cell", type=float, default=None,
                    help="simplify the mesh by vertex clustering with cells of this edge in metres, e.g. 3 voxels (default: not at all)")
    ap.add_argument("--track", action="store_true",
                    help="use the first image's pose only: track every later image against the volume before integrating it")
    ap.add_argument("--track-iters", type=int, default=10, help="--track: iterations per frame")
    ap.add_argument("--track-stride", type=int, default=1, help="--track: use every n-th pixel row and column")
    ap.add_argument("--track-sweeps", type=int, default=1, help="--track: passes that re-track all frames against the finished volume")
    ap.add_argument("--track-extent", type=float, default=None,
                    help="--track: metres of volume beyond the first image's box (default: that box's longest side)")
    ap.add_argument("--join", default=None, metavar="VIEWS",
                    help="a second BOP-format scene folder of the same object, turned over, whose poses are not used: its first image "
                         "is found against the volume of --views by an exhaustive pose search, the rest are tracked, all are fused")
    ap.add_argument("--join-step-deg", type=float, default=15.0, help="--join: degrees between neighbours of the rotation grid")
    ap.add_argument("--join-top", type=int, default=32, help="--join: candidates that are refined")
    ap.add_argument("--join-coarse", type=int, default=2, help="--join: voxels of --voxel per node of the volume that is searched")
    ap.add_argument("--join-points", type=int, default=256, help="--join: points of the first image that score a candidate")
    ap.add_argument("--join-turned-over", action="store_true",
                    help="--join: among the refined candidates that the volume does not contradict, keep the one that shows the most "
                         "unseen space (for an object with symmetries, whose seen side the second folder fits as well as its own)")
    ap.add_argument("--close", action="store_true",
                    help="close the mesh: unseen space that is enclosed becomes inside; unseen space that reaches the volume's border stays open")
    ap.add_argument("--support-plane", type=_plane_argument, default=None,
                    help="--close: the plane the object stands on, a,b,c,d with a x + b y + c z + d = 0 in the object's frame, "
                         "lengths in metres, the object on the positive side; 'auto': fitted to the first image's whole depth "
                         "image (inliers within --support-lift) and taken into the object's frame by that image's pose")
    ap.add_argument("--support-lift", type=float, default=None,
                    help="--close: metres the plane is moved towards the object before the volume is cut, the statement of the "
                         "sensor's noise on the table (default: half a voxel); the mesh's bottom then lies this far above the table")
    ap.add_argument("--condition-depth", action="store_true",
                    help="condition every depth image before anything reads it: drop mixed pixels on silhouettes, and smooth within "
                         "a surface with --smooth-radius (default: the readings as they are)")
    ap.add_argument("--flying-radius", type=int, default=None, help="--condition-depth: half the window a reading's support is counted in (1; 0: off)")
    ap.add_argument("--flying-support", type=int, default=None, help="--condition-depth: neighbours within the gate that a reading needs to stay (4)")
    ap.add_argument("--smooth-radius", type=int, default=None, help="--condition-depth: half the window of the paired mean (0: no smoothing)")
    ap.add_argument("--depth-jump", type=float, default=None, help="--condition-depth: the gate in metres (0.01)")
    ap.add_argument("--depth-jump-rel", type=float, default=None, help="--condition-depth: the gate's share of the reading, added to --depth-jump (0)")
    ap.add_argument("--weight-views", action="store_true",
                    help="weight every reading by its viewing angle: face-on counts --weight-levels times, grazing once, a pixel "
                         "without a normal (silhouettes, rims of holes) not at all (default: every observation counts once)")
    ap.add_argument("--weight-step", type=int, default=None, help="--weight-views: pixels to the neighbours the normal is taken from (1; up to 4)")
    ap.add_argument("--weight-levels", type=int, default=None, help="--weight-views: the weight of a face-on reading (16; up to 255)")
    ap.add_argument("--weight-cos-min", type=float, default=None, help="--weight-views: readings whose ray meets the surface at a smaller cosine get weight 0 (0.2)")
    ap.add_argument("--weight-jump", type=float, default=None, help="--weight-views: the gate on a neighbour's reading in metres (0.01)")
    ap.add_argument("--weight-jump-rel", type=float, default=None, help="--weight-views: the gate's share of the reading, added to --weight-jump (0)")
    ap.add_argument("--carve-weight", type=int, default=None, help="--weight-views: the weight of 'the space in front of this pixel is empty' (1; 0 .. 255)")
    ap.add_argument("--report", default=None, help="write the report as JSON here")
    ap.add_argument("--out", required=True, help="the .ply to write, in model units")
    a = ap.parse_args(argv)
    if not (a.voxel > 0 and np.isfinite(a.voxel)):
        ap.error("--voxel is a positive length in metres")
    if a.trunc is not None and not (a.trunc > 0 and np.isfinite(a.trunc)):
        ap.error("--trunc is a positive length in metres")
    if a.min_weight < 1:
        ap.error("--min-weight is at least 1")
    if not (a.mesh_scale > 0 and np.isfinite(a.mesh_scale)):
        ap.error("--mesh-scale is positive")
    if not a.out.lower().endswith(".ply"):
        ap.error("--out is a .ply file")
    if a.simplify_cell is not None and not (a.simplify_cell > 0 and np.isfinite(a.simplify_cell)):
        ap.error("--simplify-cell is a positive length in metres")
    if a.track_iters < 1 or a.track_stride < 1 or a.track_sweeps < 0:
        ap.error("--track-iters and --track-stride are at least 1, --track-sweeps at least 0")
    if a.track_extent is not None and not (a.track_extent >= 0 and np.isfinite(a.track_extent)):
        ap.error("--track-extent is a length in metres")
    if a.join is not None and not (0 < a.join_step_deg <= 180 and a.join_top >= 1 and a.join_coarse >= 1 and 1 <= a.join_points <= 2048):
        ap.error("--join-step-deg is in (0, 180], --join-top and --join-coarse at least 1, --join-points 1 to 2048")
    if not a.close and (a.support_plane is not None or a.support_lift is not None):
        ap.error("--support-plane and --support-lift belong to --close")
    if a.support_lift is not None and not (a.support_lift >= 0 and np.isfinite(a.support_lift)):
        ap.error("--support-lift is a length in metres, 0 or more")
    if a.support_lift is not None and a.support_plane is None:
        ap.error("--support-lift moves the --support-plane; there is none")
    from . import depthfilter
    try:
        condition = depthfilter.from_flags(a.condition_depth, {k: getattr(a, k) for k in depthfilter.FLAGS},
                                           lambda name: "--" + name.replace("_", "-"), who="--condition-depth")
    except ValueError as e:
        ap.error(str(e))
    from . import depthweights
    try:
        weighting = depthweights.from_flags(a.weight_views, {k: getattr(a, k) for k in depthweights.FLAGS})
    except ValueError as e:
        ap.error(str(e))
    closing = dict(close=a.close, support_plane=a.support_plane, support_lift=a.support_lift, condition=condition, weighting=weighting)
    from . import bop_data
    if a.join is not None:
        from . import track
        mesh, report = track.join_scene(a.views, a.join, a.voxel, a.obj_id, a.trunc, a.min_weight, not a.no_masks, a.pixel_offset,
                                        a.mesh_scale, a.simplify_cell, a.track_iters, a.track_stride, a.track_sweeps if a.track else None,
                                        a.track_extent, np.deg2rad(a.join_step_deg), a.join_top, a.join_coarse, a.join_points,
                                        turned_over=a.join_turned_over, **closing)
    elif a.track:
        from . import track
        mesh, report = track.onboard_scene(a.views, a.voxel, a.obj_id, a.trunc, a.min_weight, not a.no_masks, a.pixel_offset,
                                           a.mesh_scale, a.simplify_cell, a.track_iters, a.track_stride, a.track_sweeps, a.track_extent,
                                           **closing)
    else:
        mesh, report = fuse_scene(a.views, a.voxel, a.obj_id, a.trunc, a.min_weight, not a.no_masks, a.pixel_offset, a.mesh_scale,
                                  a.simplify_cell, **closing)
    if not mesh.faces.shape[0]:
        raise CppfError("fuse: the volume has no surface (no node behind a reading); check the poses, --mesh-scale and --pixel-offset")
    bop_data.write_ply(a.out, mesh.verts / a.mesh_scale, mesh.faces)
    if a.report:
        with open(a.report, "w") as f:
            json.dump(report, f, indent=1)
    print("fused %d views into %d x %d x %d nodes: %d triangles, %d vertices, %d boundary edges -> %s"
          % (report["views"], *report["dims"], report["triangles"], report["vertices"], report["boundary_edges"], a.out), file=sys.stderr)
    return report


if __name__ == "__main__":
    main()
