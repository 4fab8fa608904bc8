"""Scene explanation (the reference has no such step): of all verified candidate poses of a depth image,
the subset that together explains the observed depth, every observed pixel counted once (cppf_scene_explain).  verify.select
decides per mask and in isolation; this decides per image: which candidates are instances and which are clutter.

    out = explain(depth, region, cand_off, renders)           # device tensors: chosen, gain, net, static, labels, summary
    out = explain_wide(depth, region, cand_off, renders)      # the same with up to 512 candidates per image (section 24)
    out = explain_candidates(objs, depth, region, K, records, obj_of)         # wide=True: up to 512 records
    out["records"]                                            # the chosen records, in the order they were chosen

Greedy rounds: a candidate's gain is the number of region pixels it fits within tau that no earlier winner explained, its net
the gain minus viol_weight times its violations (pixels where it would hide a surface the camera saw); the largest net of at
least min_gain wins, ties to the lower index, and its fit pixels are explained.  The defaults are derived, none was swept: TAU
is verification's 2 cm, MIN_GAIN the smallest segment that can carry a pose (segment.MIN_SEGMENT_PIXELS), VIOL_WEIGHT = 1 lets
one hidden observed pixel cancel one explained pixel, the trade verify.score makes in its denominator.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import segment as _segment
from . import solid as _solid

TAU = 0.02                                  # verify.TAU (not imported here: this module's checks need no library)
MIN_GAIN = _segment.MIN_SEGMENT_PIXELS
VIOL_WEIGHT = 1
MAX_ROUNDS = 16
MAX_CANDIDATES = 64                         # per image: one bit of a pixel's word each
MAX_CANDIDATES_WIDE = 512                   # explain_wide: up to 8 words per pixel
ROUNDS_LIMIT = 64
MAX_DIM = 8192


def _checked(cand_off, tau, min_gain, viol_weight, max_rounds, who, limit=MAX_CANDIDATES):
    """The host-side arguments, checked before a device is touched: (int32 offsets, tau, min_gain, viol_weight, max_rounds)."""
    tau, min_gain, viol_weight, max_rounds = float(tau), int(min_gain), int(viol_weight), int(max_rounds)
    if not tau >= 0.0:
        raise ValueError("%s: tau is a distance in metres >= 0, not %r" % (who, tau))
    if not 1 <= min_gain < 2 ** 31:
        raise ValueError("%s: min_gain must be >= 1, not %d" % (who, min_gain))
    if not 0 <= viol_weight < 2 ** 31:
        raise ValueError("%s: viol_weight must be >= 0, not %d" % (who, viol_weight))
    if not 1 <= max_rounds <= ROUNDS_LIMIT:
        raise ValueError("%s: max_rounds must be in 1 .. %d, not %d" % (who, ROUNDS_LIMIT, max_rounds))
    return _solid.checked_offsets(cand_off, who, limit), tau, min_gain, viol_weight, max_rounds


def explain(depth, region, cand_off, renders, tau=TAU, min_gain=MIN_GAIN, viol_weight=VIOL_WEIGHT, max_rounds=MAX_ROUNDS):
    """cppf_scene_explain on the current stream.  depth float32 [I,H,W] or [H,W] (metres, 0 = no reading), region [I,H,W] or
    [H,W] (non-zero: a pixel to explain), cand_off int [I+1] (host: renders cand_off[i] .. cand_off[i+1]-1 are the candidates of
    image i, at most 64 each), renders float32 [P,H,W] (0 = nothing drawn).  Returns a dict of device tensors: chosen int32
    [I,M] (the winner's index within its image per round, -1 past the end), gain and net int64 [I,M], static int64 [P,3]
    (drawn, fit, violations: columns 0, 4 and 2 of verify.fit_counts), labels uint8 [I,H,W] (the round that explained the pixel,
    255: none), summary int64 [I,3] (region pixels with a reading, explained pixels, rounds used).  No host synchronisation."""
    return _explain(depth, region, cand_off, renders, tau, min_gain, viol_weight, max_rounds, "scene.explain", False)


def explain_wide(depth, region, cand_off, renders, tau=TAU, min_gain=MIN_GAIN, viol_weight=VIOL_WEIGHT, max_rounds=MAX_ROUNDS):
    """cppf_scene_explain_wide on the current stream: explain() with at most 512 candidates per image -- the same arguments,
    checks and dict of device tensors, every output the same byte for byte where explain() takes the input (chosen holds
    indices up to 511).  The call's largest image fixes the planes of 64 candidates the workspace holds.  No host
    synchronisation."""
    return _explain(depth, region, cand_off, renders, tau, min_gain, viol_weight, max_rounds, "scene.explain_wide", True)


def _explain(depth, region, cand_off, renders, tau, min_gain, viol_weight, max_rounds, who, wide):
    off, tau, min_gain, viol_weight, M = _checked(cand_off, tau, min_gain, viol_weight, max_rounds, who,
                                                  MAX_CANDIDATES_WIDE if wide else MAX_CANDIDATES)
    import torch
    from . import _lib, hostargs, ops
    dev = ops._dev()
    d = hostargs.image_batch(depth, dev, who, max_dim=MAX_DIM)
    I, H, W = (int(x) for x in d.shape)
    m = hostargs.mask_batch(region, d, dev, who, same_shape=True)
    if off.size != I + 1:
        raise ValueError("%s: cand_off of %d entries for %d images" % (who, off.size, I))
    r = ops._t(renders, torch.float32, dev)
    if r.numel() % (H * W):
        raise ValueError("%s: renders %s do not match the %d x %d depth image" % (who, tuple(r.shape), H, W))
    P = r.numel() // (H * W)
    r = r.reshape(P, H, W)
    if int(off[-1]) != P:
        raise ValueError("%s: cand_off ends at %d for %d renders" % (who, int(off[-1]), P))
    out = dict(chosen=torch.empty((I, M), dtype=torch.int32, device=dev), gain=torch.empty((I, M), dtype=torch.int64, device=dev),
               net=torch.empty((I, M), dtype=torch.int64, device=dev), static=torch.empty((P, 3), dtype=torch.int64, device=dev),
               labels=torch.empty((I, H, W), dtype=torch.uint8, device=dev),
               summary=torch.empty((I, 3), dtype=torch.int64, device=dev))
    L = _lib.load()
    name = "cppf_scene_explain_wide" if wide else "cppf_scene_explain"
    most = (max(int(np.diff(off).max()), 1),) if wide else ()      # the wide form's max_candidates
    need = int(getattr(L, name + "_workspace_bytes")(I, H, W, M, *most))
    ws = hostargs.scratch(need, dev, name + "_workspace_bytes", _lib.CppfError)
    _lib.check(getattr(L, name)(I, H, W, ops._p(d), ops._p(m), off.ctypes.data_as(C.c_void_p), P, ops._p(r), C.c_float(tau), min_gain,
                                viol_weight, M, *most, ops._p(out["chosen"]), ops._p(out["gain"]), ops._p(out["net"]),
                                ops._p(out["static"]), ops._p(out["labels"]), ops._p(out["summary"]), ops._p(ws), need, ops._stream()),
               name)
    return out


def explain_candidates(objs, depth, region, K, records, obj_of=None, tau=TAU, min_gain=MIN_GAIN, viol_weight=VIOL_WEIGHT,
                       max_rounds=MAX_ROUNDS, chunk=None, wide=False, plane=None, support_tau=_solid.SUPPORT_TAU,
                       max_sunk=_solid.MAX_SUNK, solid=False, solid_tau=_solid.OVERLAP_TAU, max_overlap=_solid.MAX_OVERLAP):
    """Explains one depth image [H,W] (metres) by candidate poses: records (RESULT_DTYPE [C], C <= 64, with wide C <= 512 through
    explain_wide; R, t in the record convention of verify.py) of the objects objs (one bop.ObjectInfo or render.Mesh, or a list of them) with obj_of int [C] (the
    index into objs of each record; None: all are objs[0]).  The candidates are rendered as verify.select renders its
    hypotheses -- back faces culled; a record flagged empty, one that is not finite, or one that puts a vertex nearer than
    render.ZNEAR is not drawn, fits nothing and is never chosen -- and given to explain() with the region [H,W].

    With plane (float32 [4] = (n, d) of the image's support plane, segment.fit_plane's) a candidate whose nearest back faces lie
    more than support_tau below the plane on more than max_sunk of their pixels (solid.support_counts on the reversed-winding
    render) is removed before the explanation.  With solid=True a candidate is ineligible once more than max_overlap of the
    smaller solid of it and an earlier winner lies inside the other by more than solid_tau (solid.overlap_counts, DESIGN.md
    section 25): the explanation is run, the first chosen candidate that conflicts with an earlier one is dropped, and it is run
    again until no chosen pair conflicts -- dropping a non-winner changes no earlier round, so this is the greedy selection
    with that one more rule, in at most C passes.

    Returns dict(records RESULT_DTYPE [n] (the chosen records, in the order they were chosen), chosen int64 [n] (their indices
    in `records`), gain, net int64 [n], static int64 [C,3] (zeros for a candidate refused below the plane), labels uint8 [H,W]
    (host), region_pixels, explained_pixels, passes (explanations run), refused_support int64 [k] (indices in `records`),
    refused_overlap [(candidate, the earlier winner it conflicts with)], and with plane support int64 [C,4] = (back, sunk,
    solid, open))."""
    who = "scene.explain_candidates"
    off_check = _checked([0, len(records)], tau, min_gain, viol_weight, max_rounds, who,
                         MAX_CANDIDATES_WIDE if wide else MAX_CANDIDATES)
    if plane is not None:
        support_tau, max_sunk = _solid.checked_tau(support_tau, who, "support_tau"), _solid.checked_share(max_sunk, who, "max_sunk")
    if solid:
        solid_tau, max_overlap = _solid.checked_tau(solid_tau, who, "solid_tau"), _solid.checked_share(max_overlap, who, "max_overlap")
    import torch
    from . import bop, hostargs, ops, verify
    from .pipeline import RESULT_DTYPE
    objs = list(objs) if isinstance(objs, (list, tuple)) else [objs]
    objs = [o if isinstance(o, bop.ObjectInfo) else bop.ObjectInfo.from_mesh(o) for o in objs]
    host = np.ascontiguousarray(records, dtype=RESULT_DTYPE).reshape(-1).copy()
    Cn = host.size
    of = np.zeros(Cn, dtype=np.int64) if obj_of is None else np.asarray(obj_of, dtype=np.int64).reshape(-1)
    if of.size != Cn or (Cn and (of.min() < 0 or of.max() >= len(objs))):
        raise ValueError("scene.explain_candidates: obj_of names an object of objs for each of the %d records" % Cn)
    dev = ops._dev()
    if len(np.shape(depth)) != 2:
        raise ValueError("scene.explain_candidates: one depth image [H,W], not %s" % (np.shape(depth),))
    d = hostargs.image_batch(depth, dev, "scene.explain_candidates", max_dim=MAX_DIM)
    _, Hi, Wi = (int(x) for x in d.shape)
    ren = torch.zeros((Cn, Hi, Wi), dtype=torch.float32, device=dev)
    far = torch.zeros((Cn, Hi, Wi), dtype=torch.float32, device=dev) if plane is not None or solid else None
    empty = (host["flags"] & verify.EMPTY) != 0
    R, t = host["R"].reshape(-1, 3, 3), host["t"].reshape(-1, 3)
    for o, obj in enumerate(objs):
        idx = np.flatnonzero(of == o)
        draw = verify.drawable(obj, R[idx], t[idx], ~empty[idx])
        for a in range(0, idx.size, int(chunk or verify.RENDER_CHUNK)):
            part = slice(a, a + int(chunk or verify.RENDER_CHUNK))
            where = torch.from_numpy(idx[part]).to(dev)
            ren[where] = verify.render_records(obj, R[idx[part]], t[idx[part]], draw[part], K, Hi, Wi, dev)
            if far is not None:
                far[where] = verify.render_records(obj, R[idx[part]], t[idx[part]], draw[part], K, Hi, Wi, dev, back=True)
    alive = np.arange(Cn, dtype=np.int64)
    extra = dict(refused_support=np.zeros(0, np.int64))
    if plane is not None:
        sup = _solid.support_counts(ren, far, [0, Cn], plane, K, support_tau).cpu().numpy() if Cn else np.zeros((0, 4), np.int64)
        sunk = _solid.sunk_share(sup) > max_sunk
        extra = dict(support=sup, refused_support=alive[sunk])
        alive = alive[~sunk]
    static = np.zeros((Cn, 3), dtype=np.int64)
    refused_overlap, passes = [], 0
    while True:
        passes += 1
        sub = ren if alive.size == Cn else ren[torch.from_numpy(alive).to(dev)]
        out = (explain_wide if wide else explain)(d, region, [0, alive.size], sub, tau, min_gain, viol_weight, max_rounds)
        summary = out["summary"][0].cpu().numpy()
        n = int(summary[2])
        pick = alive[out["chosen"][0, :n].cpu().numpy().astype(np.int64)]
        if passes == 1:
            static[alive] = out["static"].cpu().numpy()
        clash = None
        if solid and n >= 2:                               # the chosen ones: at most ROUNDS_LIMIT = 64 of them
            at = torch.from_numpy(pick).to(dev)
            hit = _solid.conflicts(_solid.overlap_counts(ren[at], far[at], [0, n], solid_tau), max_overlap)
            clash = next(((k, e) for k in range(n) for e in range(k) if hit[k, e]), None)
        if clash is None:
            break
        refused_overlap.append((int(pick[clash[0]]), int(pick[clash[1]])))
        alive = alive[alive != pick[clash[0]]]
    return dict(records=host[pick].copy(), chosen=pick, gain=out["gain"][0, :n].cpu().numpy(), net=out["net"][0, :n].cpu().numpy(),
                static=static, labels=out["labels"][0].cpu().numpy(), region_pixels=int(summary[0]),
                explained_pixels=int(summary[1]), passes=passes, refused_overlap=refused_overlap, **extra)
