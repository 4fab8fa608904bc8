"""Instance-level pose refinement against the object's mesh: point-to-plane ICP of the observed cloud against samples of the mesh
surface (cppf_icp_refine, include/cppf_hip.h), the usual last step of instance-level pose from depth.  The reference has no such
step; its only refinement is `opt` (eval.py:319-355), which aligns the cloud to the network's own predicted pair coordinates.

    model = ModelPoints.from_mesh(render.load_mesh("obj_000015.ply", 0.001))
    stats = refine(model, pts, pt_off, records, iters=30)          # records' R, t replaced in place

Frame: the model samples are centred on the mesh's bounding-box centre, the centring render.camera_pose applies, so a rendered
item's (rot, trans) -- pc = rot (v - centre) + trans at scale 1 -- is the record pose (R, t) under which the view and the samples
coincide.  The defaults are chosen in DESIGN.md section 13.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, hostargs, ops, pipeline
from ._lib import CppfError

_L = _lib.load()

COUNT = 4096
ITERS = 30
MAX_DIST = (0.05, 0.005)         # (d0, d1) metres: inlier distance of the first and of the last iteration
REFINED = 16                     # CppfSceneResult.flags bit4


class ModelPoints:
    """pts / nrm float32 [M,3] (model frame, centred on the bounding-box centre) and the centre itself (float64 [3]); device
    copies are made once per device and kept."""

    def __init__(self, pts, nrm, centre):
        self.pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
        self.nrm = np.ascontiguousarray(nrm, dtype=np.float32).reshape(-1, 3)
        if self.pts.shape != self.nrm.shape or not len(self.pts):
            raise ValueError("ModelPoints: pts and nrm must be non-empty [M,3] arrays of one shape")
        self.centre = np.asarray(centre, dtype=np.float64).reshape(3)
        self._dev = {}

    @classmethod
    def from_mesh(cls, mesh, count=COUNT, seed=0):
        """`count` points on the surface of a render.Mesh, area-weighted (numpy Generator(seed), float64), each with its
        triangle's unit normal."""
        v, f = mesh.verts, mesh.faces.astype(np.int64)
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        cr = np.cross(b - a, c - a)
        area2 = np.linalg.norm(cr, axis=1)
        if not area2.sum() > 0:
            raise ValueError("ModelPoints.from_mesh: the mesh has no triangle of non-zero area")
        rng = np.random.default_rng(seed)
        tri = rng.choice(len(f), size=int(count), p=area2 / area2.sum())
        r1, r2 = rng.random(int(count)), rng.random(int(count))
        s = np.sqrt(r1)
        p = (1.0 - s)[:, None] * a[tri] + (s * (1.0 - r2))[:, None] * b[tri] + (s * r2)[:, None] * c[tri]
        bnd = mesh.bounds
        centre = (bnd[0] + bnd[1]) / 2
        return cls(p - centre, cr[tri] / area2[tri][:, None], centre)

    def device(self, dev):
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.pts).to(dev), torch.from_numpy(self.nrm).to(dev))
        return self._dev[key]


_WS = hostargs.ScratchCache("cppf_icp_workspace_bytes", CppfError)                 # workspaces per (device index, stream)
_WS_DEPTH = hostargs.ScratchCache("cppf_icp_depth_workspace_bytes", CppfError)


def _depth_args(depth, img_idx, K, model_weight, B):
    """refine's depth arguments, checked before a device is asked for (a machine without one gets these errors): (depth as a
    contiguous float32 [I,H,W] batch where it already is, img_idx int32 [B] NumPy, K float64 [9], model_weight)."""
    if depth.dtype not in (torch.float32, np.dtype(np.float32)):
        raise ValueError("icp.refine: depth must be float32 metres, not %s" % (depth.dtype,))
    depth = hostargs.image_batch(depth, depth.device if torch.is_tensor(depth) else "cpu", "icp.refine")
    I = depth.shape[0]
    if K is None:
        raise ValueError("icp.refine: depth needs K, the camera's 3x3 intrinsics")
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError("icp.refine: K must be a 3x3 matrix, not %s" % (K.shape,))
    if not (np.isfinite(K[0, 0]) and np.isfinite(K[1, 1]) and K[0, 0] > 0 and K[1, 1] > 0):
        raise ValueError("icp.refine: K needs finite fx, fy > 0")
    w = float(model_weight)
    if not (w > 0 and np.isfinite(w)):
        raise ValueError("icp.refine: model_weight must be finite and > 0, not %r" % (model_weight,))
    if img_idx is None:
        if I == B:
            idx = np.arange(B, dtype=np.int32)
        elif I == 1:
            idx = np.zeros(B, dtype=np.int32)
        else:
            raise ValueError("icp.refine: %d depth images for %d instances need img_idx" % (I, B))
    else:
        idx = (img_idx.cpu().numpy() if torch.is_tensor(img_idx) else np.asarray(img_idx)).astype(np.int32).reshape(-1)
        if idx.size != B:
            raise ValueError("icp.refine: img_idx of %d entries for %d instances" % (idx.size, B))
    return depth, idx, np.ascontiguousarray(K.reshape(9)), w


def refine(model, pts, pt_off, results, iters=ITERS, max_dist=MAX_DIST, depth=None, img_idx=None, K=None, model_weight=1.0):
    """Refines the poses of `results` in place against `model` (cppf_icp_refine) and returns the stats float32 [B,4]: inliers
    of the last iteration, their RMS point-to-plane distance, inliers / n, iterations that changed the pose.

    pts: float32 [N,3] camera-frame points of the B instances, instance b = pts[pt_off[b]:pt_off[b+1]]; pt_off: int [B+1].
    results: the records, either a device uint8 [B,160] tensor (a VotingPipeline's results / selected; stats come back as a
    device tensor) or a pipeline.RESULT_DTYPE array (stats come back as a NumPy array).  Records flagged empty (flags bit0)
    are left as they are; every other one gets flags bit4.  B = 0 (pt_off of one entry) is an empty batch: nothing is launched
    and the stats are an empty [0,4] array (device tensor or NumPy, as above).

    depth (float32 metres, [H,W] or [I,H,W], NumPy or device tensor) adds the model-to-depth terms (cppf_icp_refine_depth,
    DESIGN.md section 19): every model sample facing the camera is associated with the surface seen at its pixel of image
    img_idx[b] (int [B]; default arange(B) when I == B, zeros when I == 1) through the intrinsics K (3x3), its terms weighted by
    model_weight.  The stats are then float32 [B,8]: the four above for the observed points, then the model-side inliers of the
    last iteration, their RMS distance, inliers / visible in-image samples, and the visible in-image samples.  With depth,
    pts = None and pt_off = None mean no observed points (no mask): B is then the number of records."""
    if depth is None:
        if img_idx is not None or K is not None or float(model_weight) != 1.0:
            raise ValueError("icp.refine: img_idx, K and model_weight belong to depth")
        if pts is None or pt_off is None:
            raise ValueError("icp.refine: without depth, pts and pt_off are required")
    elif (pts is None) != (pt_off is None):
        raise ValueError("icp.refine: pts and pt_off are given together or not at all")
    if depth is not None:
        nrec = len(results) if isinstance(results, np.ndarray) else results.shape[0]
        dargs = _depth_args(depth, img_idx, K, model_weight, nrec)
        if pt_off is None:
            pts, pt_off = np.zeros((0, 3), dtype=np.float32), np.zeros(nrec + 1, dtype=np.int64)
    ncol = 4 if depth is None else 8
    dev = ops._dev()
    host_records = isinstance(results, np.ndarray)
    if host_records:
        rec = pipeline.record_bytes(results, dev)
    else:
        rec = results
        if rec.dtype != torch.uint8 or rec.dim() != 2 or rec.shape[1] != 160 or not rec.is_contiguous() or rec.device != dev:
            raise CppfError("icp.refine: results must be a contiguous uint8 [B,160] tensor on %s" % dev)
    off_h = (pt_off.cpu().numpy() if torch.is_tensor(pt_off) else np.asarray(pt_off)).astype(np.int64).reshape(-1)
    B = off_h.size - 1
    if B != rec.shape[0]:
        raise CppfError("icp.refine: %d records for %d instances" % (rec.shape[0], B))
    if B == 0:
        return np.zeros((0, ncol), dtype=np.float32) if host_records else torch.zeros((0, ncol), dtype=torch.float32, device=dev)
    max_n = int(np.diff(off_h).max())
    if depth is None:
        max_n = max(max_n, 1)
    pts = ops._t(pts, torch.float32, dev).reshape(-1, 3).contiguous()
    if pts.shape[0] < off_h[-1]:
        raise CppfError("icp.refine: pt_off reaches %d points, pts holds %d" % (off_h[-1], pts.shape[0]))
    off = pt_off.to(device=dev, dtype=torch.int32).contiguous() if torch.is_tensor(pt_off) else \
        torch.from_numpy(off_h.astype(np.int32)).to(dev)
    mp, mn = model.device(dev)
    stats = torch.empty((B, ncol), dtype=torch.float32, device=dev)
    d0, d1 = (float(x) for x in max_dist)
    if depth is None:
        ws = _WS.get(hostargs.stream_key(dev), _L.cppf_icp_workspace_bytes(B, max_n), dev)
        _lib.check(_L.cppf_icp_refine(B, ops._p(pts), ops._p(off), max_n, ops._p(mp), ops._p(mn), mp.shape[0], int(iters),
                                      C.c_float(d0), C.c_float(d1), ops._p(rec), ops._p(stats), ops._p(ws), ws.numel(),
                                      ops._stream()), "cppf_icp_refine")
    else:
        dimg, idx, K9, w = dargs
        dimg = dimg.to(dev)
        I, H, W = dimg.shape
        idx_d = torch.from_numpy(idx).to(dev)
        ws = _WS_DEPTH.get(hostargs.stream_key(dev), _L.cppf_icp_depth_workspace_bytes(B, max_n, mp.shape[0]), dev)
        _lib.check(_L.cppf_icp_refine_depth(B, ops._p(pts) if max_n > 0 else None, ops._p(off), max_n, ops._p(mp), ops._p(mn),
                                            mp.shape[0], ops._p(dimg), I, H, W, ops._p(idx_d), K9.ctypes.data_as(C.c_void_p),
                                            C.c_float(w), int(iters), C.c_float(d0), C.c_float(d1), ops._p(rec), ops._p(stats),
                                            ops._p(ws), ws.numel(), ops._stream()), "cppf_icp_refine_depth")
    if host_records:
        results[...] = pipeline.records_of(rec, results.shape)
        return stats.cpu().numpy()
    return stats
