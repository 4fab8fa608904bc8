"""3-D IoU of oriented boxes on the GPU: what the NOCS scorer's IoU AP is built on
(metrics.degree_cm_mAP(iou="device")).  The reference computes it on the host, one box pair at a time (utils/util.py:475-547 ->
utils/iou.py, utils/box.py).

    iou = box_iou(R1, t1, s1, R2, t2, s2, turns)                    # float64 [P] device tensor
    iou = iou_3d_batch(RT_1, RT_2, scales_1, scales_2, symmetric)   # metrics.iou_3d for many pairs in one call

The kernel is cppf_box_iou (include/cppf_hip_experimental.h): held to 1e-9 also where planes of the two boxes coincide or nearly
do (identical boxes, shared faces, boxes that touch), where the host's convex hull is arbitrary.
"""
from __future__ import annotations

import numpy as np

from . import _lib

MAX_PAIRS = 1 << 20              # pairs per kernel call
MAX_TURNS = 64                   # the entry point's cap on turns
SYM_TURNS = 36                   # the toolkit's rule: 10-degree steps about y (utils/util.py:516-536)


def turn_table(max_turns):
    """float64 [max_turns (max_turns + 1) / 2, 2]: (cos, sin)(2 pi i / n) at row n (n - 1) / 2 + i for n = 1 .. max_turns, i < n;
    the angle as metrics.iou_3d forms it."""
    rows = []
    for n in range(1, int(max_turns) + 1):
        a = 2 * np.pi * np.arange(n) / float(n)
        rows.append(np.stack([np.cos(a), np.sin(a)], 1))
    return np.concatenate(rows)


def box_iou(R1, t1, s1, R2, t2, s2, turns):
    """cppf_box_iou: float64 [P] device tensor, the largest IoU of box 1 (R1 float64 [P,3,3] orthonormal, centre t1 [P,3], full
    edge lengths s1 [P,3]) turned by 2 pi i / turns[p], i < turns[p], about its own y axis with box 2.  turns: int [P] or one int,
    1 .. 64.  Device or host arrays."""
    import torch
    from . import hostargs, ops
    dev = ops._dev()
    a = [hostargs.tensor(x, torch.float64, dev).reshape(-1, w) for x, w in ((R1, 9), (t1, 3), (s1, 3), (R2, 9), (t2, 3), (s2, 3))]
    P = a[0].shape[0]
    if np.ndim(turns) == 0 and not isinstance(turns, torch.Tensor):
        turns = np.full(P, int(turns), np.int32)
    tn = hostargs.tensor(turns, torch.int32, dev).reshape(-1)
    if any(x.shape[0] != P for x in a) or tn.shape[0] != P:
        raise ValueError("box_iou: the arguments describe %s pairs" % sorted({int(x.shape[0]) for x in a + [tn]}))
    out = torch.empty((P,), dtype=torch.float64, device=dev)
    if P == 0:
        return out
    lo, hi = (int(x) for x in torch.stack(torch.aminmax(tn)).cpu())          # one copy
    if lo < 1 or hi > MAX_TURNS:
        raise ValueError("box_iou: turns are 1 .. %d, not %d .. %d" % (MAX_TURNS, lo, hi))
    cs = hostargs.tensor(turn_table(hi), torch.float64, dev)
    L = _lib.load()
    for b in range(0, P, MAX_PAIRS):
        n = min(MAX_PAIRS, P - b)
        _lib.check(L.cppf_box_iou(*(ops._p(x[b:]) for x in a), ops._p(tn[b:]), ops._p(cs), hi, n, ops._p(out[b:]), ops._stream()),
                   "cppf_box_iou")
    return out


def unit_boxes(RTs, scales):
    """(R float64 [P,3,3], t [P,3], s [P,3]) of poses [P,4,4] and edge lengths [P,3] with metrics.iou_3d's normalisation: the
    cube root of the determinant divided out of the rotation block, the scales as they are."""
    RTs = np.asarray(RTs, dtype=np.float64).reshape(-1, 4, 4)
    R = RTs[:, :3, :3]
    R = R / np.cbrt(np.linalg.det(R))[:, None, None] if len(R) else R
    return R, RTs[:, :3, 3], np.asarray(scales, dtype=np.float64).reshape(-1, 3)


def iou_3d_batch(RT_1, RT_2, scales_1, scales_2, symmetric):
    """metrics.iou_3d for P pairs: poses [P,4,4], edge lengths [P,3], symmetric bool [P] (the class is symmetric about y: box 1
    is tried in 36 turns).  float64 [P] device tensor."""
    R1, t1, s1 = unit_boxes(RT_1, scales_1)
    R2, t2, s2 = unit_boxes(RT_2, scales_2)
    turns = np.where(np.asarray(symmetric, dtype=bool).reshape(-1), SYM_TURNS, 1).astype(np.int32)
    return box_iou(R1, t1, s1, R2, t2, s2, turns)
