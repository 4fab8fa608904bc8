"""Instance-level pose errors on the GPU: the BOP metrics (Hodan et al., "On Evaluation of 6D Object Pose Estimation", ECCVW 2016;
the BOP'19 challenge's variants) -- VSD (Visible Surface Discrepancy, cppf_vsd_counts), MSSD and MSPD (Maximum Symmetry-aware
Surface / Projection Distance, cppf_mssd_mspd) -- and their average recall; and the visibility of ground-truth instances in their
test images (cppf_gt_visibility: BOP's scene_gt_info counts and boxes, mask_visib).  The reference has no such scorer.

    mesh = render.load_mesh("obj_000015.ply", 0.001)
    obj = ObjectInfo.from_mesh(mesh, models_info=info)              # info: the object's entry of a BOP models_info.json
    err = pose_errors(obj, depth, [0], R_est, t_est, R_gt, t_gt, K)  # vsd [P, n_taus], mssd [P], mspd [P]
    ar = average_recall(err, obj.diameter, width=640)

Frame: the record convention of eval.py and icp.py -- the model centred on its bounding-box centre (render.camera_pose's
centring), in metres, p = R m + t.  pose_from_bop converts BOP's scene_gt poses to it.  DESIGN.md section 14 states the arithmetic.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, hostargs, ops, render
from ._lib import CppfError

_L = _lib.load()

DELTA = 0.015                                                   # metres: VSD's visibility tolerance (BOP'19)
TAUS = tuple(round(0.05 * k, 2) for k in range(1, 11))          # VSD misalignment tolerances, fractions of the diameter
THETAS = TAUS                                                   # recall thresholds of VSD (errors) and MSSD (x diameter)
MSPD_PX = tuple(5.0 * k for k in range(1, 11))                  # recall thresholds of MSPD, pixels at an image width of 640
SYM_STEP = 0.01                                                 # max_sym_disc_step of BOP'19, radians
N_CONT = int(np.ceil(np.pi / SYM_STEP))                         # 315 rotations per continuous symmetry
RENDER_CHUNK = 32                                               # pairs rendered per call (64 views)
MAX_PAIRS = 65535                                               # pairs per kernel call
DIAM_CHUNK = 256


def _axis_rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64).reshape(3)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def _centred(R, t, centre):
    """x -> R x + t (metres, uncentred) as the map of the centred frame, m -> R m + (R c + t - c), float64 [3,4]."""
    return np.hstack([R, (R @ centre + t - centre)[:, None]])


def symmetry_transforms(models_info, scale, centre):
    """float64 [S,3,4]: the symmetry set of a BOP models_info entry in the centred metre frame.  The identity and each discrete
    transform D_j (its translation in model units times `scale`); with continuous symmetries, every C_i . D_j instead, C_i the
    rotation by 2 pi i / N_CONT about an axis through its offset, i = 0 .. N_CONT-1, the axes one after another (not composed
    with each other), in the order D_j (outer), axis, i.
    i = 0 is included on purpose, so that an estimate equal to the ground truth scores 0; bop_toolkit may leave that rotation
    out -- its expansion was not available to compare against."""
    c = np.asarray(centre, dtype=np.float64).reshape(3)
    s = float(scale)
    info = models_info or {}
    disc = [np.hstack([np.eye(3), np.zeros((3, 1))])]
    for d in info.get("symmetries_discrete", []):
        T = np.asarray(d, dtype=np.float64).reshape(4, 4)
        disc.append(_centred(T[:3, :3], T[:3, 3] * s, c))
    cont = []
    for sym in info.get("symmetries_continuous", []):
        o = np.asarray(sym.get("offset", (0.0, 0.0, 0.0)), dtype=np.float64).reshape(3) * s
        for i in range(N_CONT):
            R = _axis_rotation(sym["axis"], 2.0 * np.pi * i / N_CONT)
            cont.append(_centred(R, o - R @ o, c))
    if not cont:
        return np.stack(disc)
    return np.stack([np.hstack([Ck[:, :3] @ D[:, :3], (Ck[:, :3] @ D[:, 3] + Ck[:, 3])[:, None]]) for D in disc for Ck in cont])


def diameter(verts):
    """The largest distance between two vertices (float64 [V,3]): over the convex hull's vertices when scipy's ConvexHull
    takes the set, else over all of them, in chunks of DIAM_CHUNK rows."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    try:
        from scipy.spatial import ConvexHull
        v = v[ConvexHull(v).vertices]
    except Exception:                      # fewer than 4 points, flat or degenerate sets, no scipy: all vertices
        pass
    best = 0.0
    for a in range(0, len(v), DIAM_CHUNK):
        d = v[a:a + DIAM_CHUNK, None, :] - v[None, :, :]
        best = max(best, float(np.sqrt(np.max(np.sum(d * d, -1)))))
    return best


class ObjectInfo:
    """What the scorer needs of one object: verts float64 [V,3] and faces int32 [F,3] (centred on the bounding-box centre,
    metres), centre float64 [3] (in the mesh's frame), diameter (metres), syms float64 [S,3,4] (symmetry_transforms).  Device
    copies are made once per device and kept."""

    def __init__(self, verts, faces, centre, diameter, syms):
        self.verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        self.centre = np.asarray(centre, dtype=np.float64).reshape(3)
        self.diameter = float(diameter)
        self.syms = np.ascontiguousarray(syms, dtype=np.float64).reshape(-1, 3, 4)
        if not len(self.verts) or not len(self.syms):
            raise ValueError("ObjectInfo: no vertices or no symmetry transform")
        self._dev = {}

    @classmethod
    def from_mesh(cls, mesh, models_info=None, mesh_scale=None):
        """From a render.Mesh in metres.  models_info: one object's entry of a BOP models_info.json, in the model file's units
        (its `diameter` times the mesh scale replaces the computed one; its symmetries enter symmetry_transforms).  mesh_scale:
        file units -> metres, by default the scale load_mesh applied (mesh.scale)."""
        s = float(mesh.scale if mesh_scale is None else mesh_scale)
        b = mesh.bounds
        c = (b[0] + b[1]) / 2
        v = mesh.verts - c
        info = models_info or {}
        d = float(info["diameter"]) * s if "diameter" in info else diameter(v)
        return cls(v, mesh.faces, c, d, symmetry_transforms(info, s, c))

    def device(self, dev):
        """(verts float32 [V,3], faces int32 [F,3], syms float64 [S,12]) on `dev`."""
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.verts.astype(np.float32)).to(dev), torch.from_numpy(self.faces).to(dev),
                              torch.from_numpy(self.syms.reshape(-1, 12).copy()).to(dev))
        return self._dev[key]

    def reversed_faces(self, dev):
        """faces int32 [F,3] on `dev` with every triangle's second and third index swapped (the winding reversed: with back-face
        culling the renderer then draws the nearest back face), made once per device and kept beside the device copy."""
        key = str(dev) + ":reversed"
        if key not in self._dev:
            self._dev[key] = self.device(dev)[1][:, [0, 2, 1]].contiguous()
        return self._dev[key]


def pose_from_bop(R, t, mesh_scale, centre):
    """BOP scene_gt poses (x_cam = R x + t, x on the uncentred model and t in the model file's units) -> the record convention
    (centred model, metres): (R, R centre + t * mesh_scale).  R [3,3] or [N,3,3], t [3] ([3,1]) or [N,3]."""
    R = np.asarray(R, dtype=np.float64)
    single = R.ndim == 2
    R = R.reshape(-1, 3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    tp = np.einsum("pij,j->pi", R, np.asarray(centre, dtype=np.float64).reshape(3)) + t * float(mesh_scale)
    return (R[0], tp[0]) if single else (R, tp)


def pose_to_bop(R, t, mesh_scale, centre):
    """The inverse of pose_from_bop: record-convention poses (centred model, metres) -> BOP's (R, (t - R centre) / mesh_scale),
    x_cam = R x + t on the uncentred model in the model file's units.  R [3,3] or [N,3,3], t [3] or [N,3]."""
    R = np.asarray(R, dtype=np.float64)
    single = R.ndim == 2
    R = R.reshape(-1, 3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    tb = (t - np.einsum("pij,j->pi", R, np.asarray(centre, dtype=np.float64).reshape(3))) / float(mesh_scale)
    return (R[0], tb[0]) if single else (R, tb)


def load_pose(path):
    """(R [3,3], t [3]) from a .npy or whitespace text file holding a 3x4 or 4x4 model -> camera matrix."""
    M = np.load(path) if str(path).endswith(".npy") else np.loadtxt(path)
    M = np.asarray(M, dtype=np.float64)
    if M.shape not in ((3, 4), (4, 4)):
        raise ValueError("%s: a pose is a 3x4 or 4x4 matrix, not %s" % (path, M.shape))
    return M[:3, :3].copy(), M[:3, 3].copy()


def vsd_counts(depth_test, test_idx, depth_est, depth_gt, K, diam, delta=DELTA, taus=TAUS):
    """cppf_vsd_counts: int64 [P, 2 + n_taus] device tensor (union, intersection, cost_1 .. cost_n) of P pairs.  depth_test
    [I,H,W] or [H,W] (metres, 0 = no reading), test_idx int [P], depth_est / depth_gt [P,H,W] (renders, 0 = nothing drawn),
    diam: one diameter or one per pair (metres), taus: fractions of the diameter (at most 32)."""
    dev = ops._dev()
    dt = hostargs.image_batch(depth_test, dev, "bop.vsd_counts")
    I, H, W = dt.shape
    de = ops._t(depth_est, torch.float32, dev).reshape(-1, H, W)
    dg = ops._t(depth_gt, torch.float32, dev).reshape(-1, H, W)
    P = de.shape[0]
    if dg.shape[0] != P:
        raise CppfError("bop.vsd_counts: %d estimate renders, %d ground-truth renders" % (P, dg.shape[0]))
    ti = hostargs.per_item(test_idx, P, torch.int32, dev, "bop.vsd_counts", "test indices", CppfError)
    dm = hostargs.per_item(diam, P, torch.float32, dev, "bop.vsd_counts", "diameters", CppfError)
    tau = ops._t(np.asarray(taus, dtype=np.float32).reshape(-1), torch.float32, dev)
    counts = torch.empty((P, 2 + tau.numel()), dtype=torch.int64, device=dev)
    _lib.check(_L.cppf_vsd_counts(P, I, H, W, ops._p(dt), ops._p(ti), ops._p(de), ops._p(dg), hostargs.camera4(K),
                                  C.c_double(float(delta)), ops._p(dm), ops._p(tau), tau.numel(), ops._p(counts), ops._stream()),
               "cppf_vsd_counts")
    return counts


def vsd_errors(counts):
    """VSD errors float64 [P, n_taus] from the counts: (cost_k + union - inter) / union, 1 where union = 0."""
    c = (counts.cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)).astype(np.int64)
    c = c.reshape(len(c), -1)
    u, i = c[:, :1], c[:, 1:2]
    num = (c[:, 2:] + (u - i)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(u > 0, num / np.maximum(u, 1).astype(np.float64), 1.0)


def mssd_mspd(verts, syms, pose_est, pose_gt, K):
    """cppf_mssd_mspd: (mssd, mspd) float32 [P] device tensors.  verts float32 [V,3], syms float64 [S,12] or [S,3,4], pose_est /
    pose_gt float64 [P,12] or [P,3,4] (model -> OpenCV camera)."""
    dev = ops._dev()
    v = ops._t(verts, torch.float32, dev).reshape(-1, 3)
    S_ = ops._t(syms, torch.float64, dev).reshape(-1, 12)
    pe = ops._t(pose_est, torch.float64, dev).reshape(-1, 12)
    pg = ops._t(pose_gt, torch.float64, dev).reshape(-1, 12)
    P = pe.shape[0]
    if pg.shape[0] != P:
        raise CppfError("bop.mssd_mspd: %d estimates, %d ground truths" % (P, pg.shape[0]))
    mssd = torch.empty((P,), dtype=torch.float32, device=dev)
    mspd = torch.empty((P,), dtype=torch.float32, device=dev)
    for a in range(0, max(P, 1), MAX_PAIRS):
        n = min(MAX_PAIRS, P - a)
        _lib.check(_L.cppf_mssd_mspd(n, ops._p(v), v.shape[0], ops._p(S_), S_.shape[0], ops._p(pe[a:]), ops._p(pg[a:]),
                                     hostargs.camera4(K), ops._p(mssd[a:]), ops._p(mspd[a:]), ops._stream()), "cppf_mssd_mspd")
    return mssd, mspd


def gt_visibility_counts(depth_test, img_idx, renders, K, delta=DELTA, masks=False):
    """cppf_gt_visibility: (counts int64 [G,3] = (#all, #valid, #visib), bbox int32 [G,8] = (x, y, w, h) of all, then of visib,
    mask uint8 [G,H,W] (255 = visible) or None) device tensors.  depth_test [I,H,W] or [H,W] (metres, 0 = no reading), img_idx
    int [G] (or one for all), renders [G,H,W] (each instance rendered alone, 0 = nothing drawn)."""
    dev = ops._dev()
    dt = hostargs.image_batch(depth_test, dev, "bop.gt_visibility_counts")
    I, H, W = dt.shape
    rn = ops._t(renders, torch.float32, dev).reshape(-1, H, W)
    G = rn.shape[0]
    ii = hostargs.per_item(img_idx, G, torch.int32, dev, "bop.gt_visibility_counts", "image indices", CppfError)
    counts = torch.empty((G, 3), dtype=torch.int64, device=dev)
    bbox = torch.empty((G, 8), dtype=torch.int32, device=dev)
    mask = torch.empty((G, H, W), dtype=torch.uint8, device=dev) if masks else None
    for a in range(0, max(G, 1), MAX_PAIRS):
        n = min(MAX_PAIRS, G - a)
        _lib.check(_L.cppf_gt_visibility(n, I, H, W, ops._p(dt), ops._p(ii[a:]), ops._p(rn[a:]), hostargs.camera4(K),
                                         C.c_double(float(delta)), ops._p(counts[a:]), ops._p(bbox[a:]),
                                         ops._p(mask[a:]) if masks else None, ops._stream()), "cppf_gt_visibility")
    return counts, bbox, mask


def gt_visibility(obj_or_objs, depth_test, img_idx, R, t, K, delta=DELTA, masks=False, chunk=2 * RENDER_CHUNK):
    """What the test images show of G ground-truth instances (BOP's scene_gt_info entries and mask_visib): each instance is
    rendered alone (render.render_depth, back faces culled, `chunk` instances per call) and compared with its image by
    cppf_gt_visibility.  obj_or_objs: one ObjectInfo for all instances or one per instance; depth_test [I,H,W] or [H,W]
    (metres, 0 = no reading), img_idx int [G] (or one for all), R [G,3,3], t [G,3]: poses in the record convention (every
    instance beyond render.ZNEAR: the renderer does not clip).  Returns dict(px_count_all, px_count_valid, px_count_visib
    int64 [G], visib_fract float64 [G] (#visib / #all, 0 when nothing is drawn), bbox_obj, bbox_visib int32 [G,4] (x, y, w, h;
    -1 when empty; bbox_obj is the in-image part's box), mask_visib uint8 [G,H,W] host array (255 = visible) or None)."""
    dev = ops._dev()
    P = _poses(R, t)
    G = len(P)
    objs = list(obj_or_objs) if isinstance(obj_or_objs, (list, tuple)) else [obj_or_objs] * G
    if len(objs) != G:
        raise ValueError("bop.gt_visibility: %d objects for %d poses" % (len(objs), G))
    dt = hostargs.image_batch(depth_test, dev, "bop.gt_visibility")
    _, H, W = dt.shape
    ii = np.broadcast_to(np.asarray(img_idx, dtype=np.int32).reshape(-1), (G,))
    uniq, first = [], {}
    for o in objs:
        if id(o) not in first:
            first[id(o)] = len(uniq)
            uniq.append(o)
    counts = np.zeros((G, 3), dtype=np.int64)
    bbox = np.full((G, 8), -1, dtype=np.int32)
    mask = np.zeros((G, H, W), dtype=np.uint8) if masks else None
    if G:
        # several objects per call: their vertices one after another, each instance's triangles shifted to its object's
        vbase = np.cumsum([0] + [o.verts.shape[0] for o in uniq])
        verts = torch.cat([o.device(dev)[0] for o in uniq], 0)
    for a in range(0, G, int(chunk)):
        sel = range(a, min(G, a + int(chunk)))
        tris = torch.cat([objs[g].device(dev)[1] + int(vbase[first[id(objs[g])]]) for g in sel], 0)
        tri_off = ops._offsets([objs[g].faces.shape[0] for g in sel], dev)
        poses = torch.from_numpy(P[a:a + len(sel)].reshape(-1, 12).astype(np.float32)).to(dev)
        ren = render.render_depth(verts, tris, tri_off, poses, K, H, W, cull=True)
        c, b, m = gt_visibility_counts(dt, ii[a:a + len(sel)].copy(), ren, K, delta, masks)
        counts[a:a + len(sel)] = c.cpu().numpy()
        bbox[a:a + len(sel)] = b.cpu().numpy()
        if masks:
            mask[a:a + len(sel)] = m.cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore"):
        fract = np.where(counts[:, 0] > 0, counts[:, 2].astype(np.float64) / np.maximum(counts[:, 0], 1).astype(np.float64), 0.0)
    return dict(px_count_all=counts[:, 0].copy(), px_count_valid=counts[:, 1].copy(), px_count_visib=counts[:, 2].copy(),
                visib_fract=fract, bbox_obj=bbox[:, :4].copy(), bbox_visib=bbox[:, 4:].copy(), mask_visib=mask)


def _poses(R, t):
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
    if len(R) != len(t):
        raise ValueError("bop: %d rotations, %d translations" % (len(R), len(t)))
    return np.concatenate([R, t[:, :, None]], 2)


def pose_errors(obj, depth_test, test_idx, R_est, t_est, R_gt, t_gt, K, delta=DELTA, taus=TAUS, chunk=RENDER_CHUNK):
    """BOP errors of P (estimate, ground truth) pairs of the object `obj` (an ObjectInfo), poses in the record convention:
    dict(vsd float64 [P, n_taus], mssd float64 [P] (metres), mspd float64 [P] (pixels)).

    depth_test [I,H,W] or [H,W] (metres, 0 = no reading; host or device), test_idx int [P] (or one for all): the image of each
    pair.  All pairs share K and H x W (the renderer's restriction).  The est and gt poses are rendered with render.render_depth
    (back faces culled) `chunk` pairs at a time.  A missing estimate (a non-finite pose) gets +inf in every metric and no render.
    An estimate with a vertex nearer than render.ZNEAR cannot be rasterized (no clipping): its VSD is 1, its MSSD / MSPD are
    computed (MSPD is +inf when a vertex lies at or behind the camera plane).  A ground truth must be finite and in front of
    render.ZNEAR (ValueError)."""
    dev = ops._dev()
    pe, pg = _poses(R_est, t_est), _poses(R_gt, t_gt)
    P = len(pe)
    if len(pg) != P:
        raise ValueError("bop.pose_errors: %d estimates, %d ground truths" % (P, len(pg)))
    n_taus = len(np.asarray(taus).reshape(-1))
    out = dict(vsd=np.full((P, n_taus), np.inf), mssd=np.full(P, np.inf), mspd=np.full(P, np.inf))
    if P == 0:
        return out
    if not np.isfinite(pg).all():
        raise ValueError("bop.pose_errors: a ground-truth pose is not finite")
    v64 = obj.verts
    z_gt = np.einsum("pj,vj->pv", pg[:, 2, :3], v64).min(1) + pg[:, 2, 3]
    if not (z_gt >= render.ZNEAR).all():
        raise ValueError("bop.pose_errors: a ground-truth pose puts the model nearer than %g m" % render.ZNEAR)
    dt = hostargs.image_batch(depth_test, dev, "bop.pose_errors")
    I, H, W = dt.shape
    ti = np.broadcast_to(np.asarray(test_idx, dtype=np.int64).reshape(-1), (P,))
    if ti.min() < 0 or ti.max() >= I:
        raise ValueError("bop.pose_errors: test_idx outside [0, %d)" % I)
    ok = np.nonzero(np.isfinite(pe).all((1, 2)))[0]
    if not ok.size:
        return out
    verts, faces, syms = obj.device(dev)
    mssd, mspd = mssd_mspd(verts, syms, pe[ok].reshape(-1, 12), pg[ok].reshape(-1, 12), K)
    out["mssd"][ok] = mssd.cpu().numpy()
    out["mspd"][ok] = mspd.cpu().numpy()
    z_est = np.einsum("pj,vj->pv", pe[ok, 2, :3], v64).min(1) + pe[ok, 2, 3]
    out["vsd"][ok[~(z_est >= render.ZNEAR * (1 + 1e-5))]] = 1.0
    draw = ok[z_est >= render.ZNEAR * (1 + 1e-5)]
    F = faces.shape[0]
    for a in range(0, draw.size, int(chunk)):
        sel = draw[a:a + int(chunk)]
        n = sel.size
        poses = torch.from_numpy(np.concatenate([pe[sel], pg[sel]]).reshape(-1, 12).astype(np.float32)).to(dev)
        depth = render.render_depth(verts, faces.repeat(2 * n, 1), ops._offsets([F] * (2 * n), dev), poses, K, H, W, cull=True)
        counts = vsd_counts(dt, torch.from_numpy(ti[sel].astype(np.int32)), depth[:n], depth[n:], K, obj.diameter, delta, taus)
        out["vsd"][sel] = vsd_errors(counts)
    return out


def average_recall(errors, diameter, width, thetas=THETAS, mspd_px=MSPD_PX):
    """BOP'19 average recall of one estimate per ground-truth instance (strict e < threshold; +inf never counts):
    AR_VSD = the mean over the pairs, the VSD taus (the columns of errors["vsd"]) and thetas of [vsd < theta];
    AR_MSSD over thetas x diameter (one or one per pair); AR_MSPD over mspd_px x width / 640; AR = their mean."""
    vsd = np.asarray(errors["vsd"], dtype=np.float64)
    mssd = np.asarray(errors["mssd"], dtype=np.float64).reshape(-1)
    mspd = np.asarray(errors["mspd"], dtype=np.float64).reshape(-1)
    P = len(mssd)
    if P == 0:
        raise ValueError("bop.average_recall: no estimates")
    vsd = vsd.reshape(P, -1)
    th = np.asarray(thetas, dtype=np.float64)
    diam = np.broadcast_to(np.asarray(diameter, dtype=np.float64).reshape(-1), (P,))
    ar_vsd = float(np.mean(vsd[:, :, None] < th[None, None, :]))
    ar_mssd = float(np.mean(mssd[:, None] < th[None, :] * diam[:, None]))
    ar_mspd = float(np.mean(mspd[:, None] < np.asarray(mspd_px, dtype=np.float64)[None, :] * (float(width) / 640.0)))
    return dict(AR_VSD=ar_vsd, AR_MSSD=ar_mssd, AR_MSPD=ar_mspd, AR=(ar_vsd + ar_mssd + ar_mspd) / 3.0)
