"""Instance-level pose-hypothesis verification by render and compare: several well-separated peaks of each rotation-bin vote
become pose hypotheses (cppf_pose_hypotheses), each is refined against the object's mesh (cppf_icp_refine, optional), rendered
(cppf_render_depth) and counted against the observed depth (cppf_depth_fit_counts), and the hypothesis that explains the most of
the instance without hiding what the camera saw is kept.  The reference reports one rotation per pass, from the arg-max of each
vote; it has no such step.

    recs = hypotheses(pipe.counts[0], pipe.counts[1], pipe.sphere, pipe.results, H=8, up_axis=1, right_axis=0)
    out = select(obj, depth, mask, K, recs, pts=pts, pt_off=pt_off, icp_model=model, icp_iters=30)
    out["records"][b]                          # the chosen record of instance b: flags bit5, its hypothesis index in pad_[1]

Frame: the record convention of icp.py and bop.py -- the model centred on its bounding-box centre, metres, p = R m + t.
DESIGN.md section 15 states the arithmetic and how the defaults were chosen.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, bop, hostargs, icp, ops, render, solid
from ._lib import CppfError
from .pipeline import RESULT_DTYPE, record_bytes, records_of

_L = _lib.load()

PEAKS = 4                                   # peaks per vote
COS_SEP = float(np.cos(np.deg2rad(20.0)))   # a bin within 20 degrees of an earlier peak is no new peak
COS_PERP = float(np.cos(np.deg2rad(45.0)))  # (up, right) pairs more than 45 degrees from perpendicular are dropped
TAU = 0.02                                  # metres: a drawn pixel fits the observation within TAU
EMPTY = 1                                   # CppfSceneResult.flags bit0: no hypothesis in this slot
CHOSEN = 32                                 # CppfSceneResult.flags bit5: the record verification chose (index in pad_[1])
RENDER_CHUNK = 64                           # hypotheses rendered and counted per call
N_COUNTS = 4                                # drawn, observed, violations, unexplained; then fit_k per tau


def hypotheses(counts_up, counts_right, sphere, base, H, up_axis, right_axis, K=PEAKS, cos_sep=COS_SEP, cos_perp=COS_PERP,
               y_only=False, with_peaks=False):
    """cppf_pose_hypotheses on the current stream: device uint8 [B,H,160] records (slot 0 = the base record; empty slots carry
    flags bit0), and with with_peaks also (peak_idx int32 [B,2,K], peak_count float32 [B,2,K]).  counts_up / counts_right
    float32 [B,S] (a VotingPipeline's counts[0] / counts[1]), sphere float32 [S,3], base: device uint8 [B,160] records (a
    pipeline's results) or a RESULT_DTYPE array."""
    dev = ops._dev()
    cu = ops._t(counts_up, torch.float32, dev)
    cr = ops._t(counts_right, torch.float32, dev)
    sph = ops._t(sphere, torch.float32, dev).reshape(-1, 3)
    if isinstance(base, np.ndarray):
        base = record_bytes(base, dev)
    if base.dtype != torch.uint8 or base.dim() != 2 or base.shape[1] != 160 or not base.is_contiguous():
        raise CppfError("verify.hypotheses: base must be contiguous uint8 [B,160] records")
    B, S = base.shape[0], sph.shape[0]
    if cu.shape != (B, S) or cr.shape != (B, S):
        raise CppfError("verify.hypotheses: counts must be [%d,%d], not %s and %s" % (B, S, tuple(cu.shape), tuple(cr.shape)))
    out = torch.empty((B, int(H), 160), dtype=torch.uint8, device=dev)
    pi = torch.empty((B, 2, int(K)), dtype=torch.int32, device=dev) if with_peaks else None
    pc = torch.empty((B, 2, int(K)), dtype=torch.float32, device=dev) if with_peaks else None
    _lib.check(_L.cppf_pose_hypotheses(B, S, ops._p(cu), ops._p(cr), ops._p(sph), int(K), C.c_float(cos_sep),
                                       C.c_float(cos_perp), int(up_axis), int(right_axis), int(bool(y_only)), ops._p(base),
                                       int(H), ops._p(out), ops._p(pi), ops._p(pc), ops._stream()), "cppf_pose_hypotheses")
    return (out, pi, pc) if with_peaks else out


def fit_counts(depth, mask, hyp_off, renders, taus=(TAU,)):
    """cppf_depth_fit_counts: int64 [P, 4 + n_taus] device tensor (drawn, observed, violations, unexplained, fit_1 .. fit_n).
    depth float32 [I,H,W] or [H,W] (metres, 0 = no reading), mask [I,H,W] or [H,W] (non-zero: the instance), hyp_off int
    [I+1] (host: renders hyp_off[i] .. hyp_off[i+1]-1 are hypotheses of image i), renders float32 [P,H,W] (0 = nothing
    drawn), taus: metres, at most 32 (taus[0] is also the violation margin)."""
    dev = ops._dev()
    d = hostargs.image_batch(depth, dev, "verify.fit_counts")
    I, H, W = d.shape
    m = hostargs.mask_batch(mask, d, dev, "verify.fit_counts", same_shape=True, err=CppfError)
    off = np.ascontiguousarray((hyp_off.cpu().numpy() if torch.is_tensor(hyp_off) else np.asarray(hyp_off)).reshape(-1),
                               dtype=np.int32)
    if off.size != I + 1:
        raise CppfError("verify.fit_counts: hyp_off of %d entries for %d images" % (off.size, I))
    r = ops._t(renders, torch.float32, dev).reshape(-1, H, W)
    P = r.shape[0]
    tau = ops._t(np.asarray(taus, dtype=np.float32).reshape(-1), torch.float32, dev)
    counts = torch.zeros((P, N_COUNTS + tau.numel()), dtype=torch.int64, device=dev)
    _lib.check(_L.cppf_depth_fit_counts(I, H, W, ops._p(d), ops._p(m), off.ctypes.data_as(C.c_void_p), P, ops._p(r), ops._p(tau),
                                        tau.numel(), ops._p(counts), ops._stream()), "cppf_depth_fit_counts")
    return counts


def score(counts):
    """float64 [P]: fit_0 / (observed + violations) -- the share of the observed instance the render explains within taus[0],
    with every pixel the render would hide counted against it; 0 where the denominator is 0."""
    c = (counts.cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)).astype(np.int64)
    c = c.reshape(len(c), -1)
    den = c[:, 1] + c[:, 2]
    return np.where(den > 0, c[:, N_COUNTS].astype(np.float64) / np.maximum(den, 1).astype(np.float64), 0.0)


def choose(scores, empty=None):
    """int64 [B]: per row of scores [B,H] the index of the highest score, the lower index on ties (hypothesis 0 wins unless
    something beats it); entries flagged in empty [B,H] never win (-1 when every entry of a row is)."""
    s = np.asarray(scores, dtype=np.float64)
    s = s.reshape(len(s), -1).copy()
    if empty is not None:
        s[np.asarray(empty, dtype=bool).reshape(s.shape)] = -np.inf
    s[np.isnan(s)] = -np.inf
    pick = np.argmax(s, axis=1).astype(np.int64)           # the first maximum
    pick[~np.isfinite(s.max(axis=1, initial=-np.inf))] = -1
    return pick


def _as_records(records):
    """(RESULT_DTYPE [B,H] host copy, device uint8 [B*H,160])."""
    dev = ops._dev()
    if torch.is_tensor(records):
        host = records_of(records, (records.shape[0], -1))
    else:
        host = np.ascontiguousarray(records, dtype=RESULT_DTYPE)
        host = host.reshape(len(host), -1).copy()
    return host, record_bytes(host, dev)


def drawable(obj, R, t, ok):
    """bool [P]: the poses (R float64 [P,3,3], t [P,3]) of obj (a bop.ObjectInfo) among `ok` that can be rendered: finite, and
    no vertex nearer than render.ZNEAR (the renderer does not clip)."""
    ok = np.asarray(ok, dtype=bool) & np.isfinite(R).all((1, 2)) & np.isfinite(t).all(1)
    z = np.full(len(R), -np.inf)
    if ok.any():
        z[ok] = np.einsum("pj,vj->pv", R[ok, 2, :], obj.verts).min(1) + t[ok, 2]
    return ok & (z >= render.ZNEAR * (1 + 1e-5))


def render_records(obj, R, t, draw, K, Hi, Wi, dev, back=False):
    """float32 [P,Hi,Wi] device tensor: obj at each pose with draw[p] set, back faces culled, in one cppf_render_depth call;
    zeros (nothing drawn) for the others.  back=True draws the reversed winding instead: the nearest BACK face of a closed mesh,
    the far end of its first solid interval along the pixel's ray (solid.py)."""
    dr = np.flatnonzero(draw)
    ren = torch.zeros((len(R), Hi, Wi), dtype=torch.float32, device=dev)
    if dr.size:
        verts, faces, _ = obj.device(dev)
        if back:
            faces = obj.reversed_faces(dev)
        F = faces.shape[0]
        poses = torch.from_numpy(np.concatenate([R[dr], t[dr, :, None]], 2).reshape(-1, 12).astype(np.float32)).to(dev)
        ren[torch.from_numpy(dr).to(dev)] = render.render_depth(verts, faces.repeat(dr.size, 1), ops._offsets([F] * dr.size, dev),
                                                                poses, K, Hi, Wi, cull=True)
    return ren


def select(obj_or_mesh, depth, mask, K, records, pts=None, pt_off=None, icp_model=None, icp_iters=0, tau=TAU,
           chunk=RENDER_CHUNK, icp_depth=False, icp_model_weight=1.0, plane=None, support_tau=solid.SUPPORT_TAU,
           max_sunk=solid.MAX_SUNK):
    """Verifies H pose hypotheses of each of B instances and keeps one per instance.

    obj_or_mesh: a bop.ObjectInfo or a render.Mesh (metres); depth [B,H_img,W_img] or [H_img,W_img] (metres, 0 = no reading) and
    mask (non-zero: the instance) of the same shape: instance b is seen in image b; K: the camera's 3x3 intrinsics; records
    [B,H] (RESULT_DTYPE, or a device uint8 [B,H,160] tensor such as hypotheses() returns).  With icp_iters > 0, every
    non-empty hypothesis is first refined by icp.refine against icp_model (an icp.ModelPoints) from the instance's points pts
    float32 [N,3] (camera frame), pt_off int [B+1]; with icp_depth that refinement also uses the instance's depth image (the
    model-to-depth terms of icp.refine(depth=...), weighted by icp_model_weight) and icp is float32 [B,H,8].  Each hypothesis is then rendered (back faces culled); one that is not
    finite, or puts a vertex nearer than render.ZNEAR (the renderer does not clip), is not drawn and scores 0.  score() of its
    fit_counts at (tau,) ranks it, and choose() picks.  With plane (float32 [4] or [B,4] = (n, d) of the support plane, as
    segment.fit_plane returns it) each hypothesis is also rendered with the winding reversed, and one whose nearest back faces lie
    more than support_tau below the plane on more than max_sunk of their pixels (solid.support_counts) is refused: it scores 0
    like one that cannot be drawn; the dict then also has support int64 [B,H,4] = (back, sunk, solid, open) and refused bool
    [B,H].  plane=None changes nothing.

    Returns dict(records RESULT_DTYPE [B] (the chosen records, flags bit5, the hypothesis index in pad_[1]; an instance whose
    hypotheses are all empty keeps records[b, 0] unmarked), chosen int64 [B] (-1: none), scores float64 [B,H] (NaN for empty
    slots), counts int64 [B,H,5], hypotheses RESULT_DTYPE [B,H] (after ICP), icp float32 [B,H,4] ([B,H,8] with icp_depth) or None)."""
    if plane is not None:
        support_tau = solid.checked_tau(support_tau, "verify.select", "support_tau")
        max_sunk = solid.checked_share(max_sunk, "verify.select", "max_sunk")
    obj = obj_or_mesh if isinstance(obj_or_mesh, bop.ObjectInfo) else bop.ObjectInfo.from_mesh(obj_or_mesh)
    dev = ops._dev()
    host, rec = _as_records(records)
    B, Hh = host.shape
    d = hostargs.image_batch(depth, dev, "verify.select")
    if d.shape[0] != B:
        raise CppfError("verify.select: %d instances, depth %s" % (B, tuple(d.shape)))
    m = hostargs.mask_batch(mask, d, dev, "verify.select", same_shape=True, err=CppfError)
    _, Hi, Wi = d.shape
    empty = (host["flags"] & EMPTY) != 0
    stats = None
    if int(icp_iters) > 0 and B:
        if icp_model is None or pts is None or pt_off is None:
            raise ValueError("verify.select: icp_iters > 0 needs icp_model, pts and pt_off")
        off = (pt_off.cpu().numpy() if torch.is_tensor(pt_off) else np.asarray(pt_off)).astype(np.int64).reshape(-1)
        if off.size != B + 1:
            raise CppfError("verify.select: pt_off of %d entries for %d instances" % (off.size, B))
        p = ops._t(pts, torch.float32, dev).reshape(-1, 3)
        # each instance's points once per hypothesis: the B*H records refine in one batch
        sel = torch.from_numpy(np.concatenate([np.arange(off[b], off[b + 1]) for b in range(B) for _ in range(Hh)])).to(dev)
        rep_off = np.concatenate([[0], np.cumsum(np.repeat(np.diff(off), Hh))])
        if icp_depth:                              # hypothesis h of instance b is record b * H + h: it reads image b
            stats = icp.refine(icp_model, p[sel].contiguous(), rep_off, rec, iters=int(icp_iters), depth=d,
                               img_idx=np.repeat(np.arange(B), Hh), K=K, model_weight=icp_model_weight)
        else:
            stats = icp.refine(icp_model, p[sel].contiguous(), rep_off, rec, iters=int(icp_iters))
        stats = stats.cpu().numpy().reshape(B, Hh, -1)
        host = records_of(rec, (B, Hh))
    # poses of the records (float64), drawable ones
    R = host["R"].reshape(-1, 3, 3)
    t = host["t"].reshape(-1, 3)
    P = B * Hh
    draw = drawable(obj, R, t, ~empty.reshape(-1))
    counts = np.zeros((P, N_COUNTS + 1), dtype=np.int64)
    support = np.zeros((P, 4), dtype=np.int64)
    if plane is not None:
        pl = ops._t(plane, torch.float32, dev).reshape(-1, 4)
        pl = pl.expand(B, 4).contiguous() if pl.shape[0] == 1 else pl
        if pl.shape[0] != B:
            raise CppfError("verify.select: %d instances, %d planes" % (B, pl.shape[0]))
    img_of = np.repeat(np.arange(B), Hh)
    for a in range(0, P, int(chunk)):
        idx = np.arange(a, min(P, a + int(chunk)))
        ren = render_records(obj, R[idx], t[idx], draw[idx], K, Hi, Wi, dev)
        # the chunk's hypotheses lie on consecutive images: offsets over all B images, zero-length outside the chunk
        hyp_off = np.searchsorted(img_of[idx], np.arange(B + 1), side="left").astype(np.int32)
        counts[idx] = fit_counts(d, m, hyp_off, ren, (tau,)).cpu().numpy()
        if plane is not None and B:
            far = render_records(obj, R[idx], t[idx], draw[idx], K, Hi, Wi, dev, back=True)
            support[idx] = solid.support_counts(ren, far, hyp_off, pl, K, support_tau).cpu().numpy()
    sc = score(counts)
    sc[~draw] = 0.0
    refused = (solid.sunk_share(support) > max_sunk) if plane is not None else np.zeros(P, dtype=bool)
    sc[refused] = 0.0
    sc = sc.reshape(B, Hh)
    pick = choose(sc, empty)
    sc[empty] = np.nan
    out = host[np.arange(B), np.maximum(pick, 0)].copy()
    hit = pick >= 0
    out["flags"][hit] |= CHOSEN
    out["pad_"][hit, 1] = pick[hit]
    res = dict(records=out, chosen=pick, scores=sc, counts=counts.reshape(B, Hh, -1), hypotheses=host, icp=stats)
    if plane is not None:
        res.update(support=support.reshape(B, Hh, 4), refused=refused.reshape(B, Hh))
    return res
