"""NumPy statement of cppf_box_iou (cppf2_amd/csrc/cppf_box_iou.hip) for the tests, and the generators the tests share.

box_iou: the kernel's float64 algorithm, one array element per kernel lane (pair, turn, face) -- the same plane distances, the
same partner rule for nearly coinciding planes, the same clip order and the same face sum, so that it differs from the device
only by the rounding of single operations (the reduction order over the twelve faces, the device's divide and square root).
Nothing of cppf2_amd is imported.  Being the same algorithm, it cannot vouch for it: the tests hold it and the device to the
toolkit's stored values, to closed forms and to the host's convex hull (metrics.box_iou_3d) as well.

analytic_tie_cases: box pairs whose planes coincide exactly before a seeded random rotation is applied, with the IoU known in
closed form.  near_tie_cases: the same pairs with box 2 turned and shifted by 1e-15 .. 1e-4.  synthetic_results: per-image records
like tests/golden/make_golden_map.py's, for the scorer's timing.  write_nocs_fixture: a two-image REAL275-layout folder.
"""
import numpy as np

MAX_VERTS = 10           # a rectangle clipped by six half-planes
EPS_REL = 1e-12           # a touching face pair: every corner within EPS_REL x the pair's size of the other plane -> V = 0
TILT = 1e-5               # planes whose normals are within this sine of parallel ...
SEP_REL = 1e-5            # ... and within SEP_REL x the pair's size of each other are scored together by box 1's lane


def turn_table(max_turns):
    """float64 [max_turns (max_turns + 1) / 2, 2]: (cos, sin)(2 pi i / n) at row n (n - 1) / 2 + i, i < n, n = 1 .. max_turns
    (the angle exactly as metrics.iou_3d forms it)."""
    rows = []
    for n in range(1, int(max_turns) + 1):
        a = 2 * np.pi * np.arange(n) / float(n)
        rows.append(np.stack([np.cos(a), np.sin(a)], 1))
    return np.concatenate(rows)


def _sel(k, a0, a1, a2):
    return np.where(k == 0, a0, np.where(k == 1, a1, a2))


def _clip(src, n, a, b, c):
    """One Sutherland-Hodgman pass of every lane's polygon src [L, MAX_VERTS, 2] (n [L] vertices) against a + b p + c q <= 0;
    a crossing is emitted between distances of strictly opposite signs."""
    L = len(n)
    dst = np.zeros_like(src)
    m = np.zeros(L, dtype=np.int64)
    lanes = np.arange(L)
    last = np.maximum(n - 1, 0)
    p0, q0 = src[lanes, last, 0], src[lanes, last, 1]
    d0 = (a + b * p0) + c * q0
    for i in range(MAX_VERTS):
        live = i < n
        if not live.any():
            break
        p1, q1 = src[:, i, 0], src[:, i, 1]
        d1 = (a + b * p1) + c * q1
        cross = live & (((d0 < 0) & (d1 > 0)) | ((d0 > 0) & (d1 < 0)))
        with np.errstate(all="ignore"):
            t = np.where(cross, d0 / (d0 - d1), 0.0)
        e = np.nonzero(cross & (m < MAX_VERTS))[0]
        dst[e, m[e], 0] = (p0 + t * (p1 - p0))[e]
        dst[e, m[e], 1] = (q0 + t * (q1 - q0))[e]
        m[e] += 1
        e = np.nonzero(live & (d1 <= 0) & (m < MAX_VERTS))[0]
        dst[e, m[e], 0] = p1[e]
        dst[e, m[e], 1] = q1[e]
        m[e] += 1
        p0, q0, d0 = np.where(live, p1, p0), np.where(live, q1, q0), np.where(live, d1, d0)
    return dst, m


def _area(poly, n):
    """The triangle-fan area of every lane's polygon."""
    p0, q0 = poly[:, 0, 0], poly[:, 0, 1]
    fan = np.zeros(len(n))
    for i in range(1, MAX_VERTS - 1):
        tri = (poly[:, i, 0] - p0) * (poly[:, i + 1, 1] - q0) - (poly[:, i + 1, 0] - p0) * (poly[:, i, 1] - q0)
        fan = fan + np.where(i + 1 < n, tri, 0.0)
    return 0.5 * np.abs(fan)


def box_iou(R1, t1, s1, R2, t2, s2, turns, return_max_verts=False):
    """float64 [P]: max over i < turns[p] of the IoU of box 1 turned by 2 pi i / turns[p] about its own y axis with box 2.
    R float64 [P,3,3] orthonormal, t [P,3] centres, s [P,3] full edge lengths, turns int [P] >= 1."""
    R1, R2 = np.asarray(R1, np.float64).reshape(-1, 3, 3), np.asarray(R2, np.float64).reshape(-1, 3, 3)
    t1, t2 = np.asarray(t1, np.float64).reshape(-1, 3), np.asarray(t2, np.float64).reshape(-1, 3)
    s1, s2 = np.asarray(s1, np.float64).reshape(-1, 3), np.asarray(s2, np.float64).reshape(-1, 3)
    turns = np.asarray(turns, np.int64).reshape(-1)
    P = len(turns)
    out = np.zeros(P)
    if P == 0:
        return (out, 0) if return_max_verts else out
    table = turn_table(turns.max())
    # one row per (pair, turn)
    pair = np.repeat(np.arange(P), turns)
    turn = np.concatenate([np.arange(n) for n in turns])
    cs = table[turns[pair] * (turns[pair] - 1) // 2 + turn]
    c, s = cs[:, 0, None], cs[:, 1, None]
    A = R1[pair]
    A = np.stack([c * A[:, :, 0] - s * A[:, :, 2], A[:, :, 1], s * A[:, :, 0] + c * A[:, :, 2]], 2)      # R1 . Ry
    B = R2[pair]
    dt = t1[pair] - t2[pair]
    ca = 0.5 * dt
    ha, hb = 0.5 * s1[pair], 0.5 * s2[pair]
    size = (np.sqrt((s1[pair] ** 2).sum(1)) + np.sqrt((s2[pair] ** 2).sum(1))) + np.sqrt((dt ** 2).sum(1))
    # one lane per (row, face): faces 0..5 are box 1's (clipped by box 2), 6..11 box 2's; face = 2 * axis + (sign > 0)
    rows = len(pair)
    row = np.repeat(np.arange(rows), 12)
    face = np.tile(np.arange(12), rows)
    second = face >= 6
    k = (face % 6) // 2
    sg = np.where(face % 2 == 1, 1.0, -1.0)
    sec3, sec33 = second[:, None], second[:, None, None]
    O, Y = np.where(sec33, B[row], A[row]), np.where(sec33, A[row], B[row])
    oc, yc = np.where(sec3, -ca[row], ca[row]), np.where(sec3, ca[row], -ca[row])
    oh, yh = np.where(sec3, hb[row], ha[row]), np.where(sec3, ha[row], hb[row])
    size = size[row]
    eps, sep = EPS_REL * size, SEP_REL * size
    k1, k2 = (k + 1) % 3, (k + 2) % 3
    nrm = np.stack([_sel(k, O[:, r, 0], O[:, r, 1], O[:, r, 2]) for r in range(3)], 1)
    e1 = np.stack([_sel(k1, O[:, r, 0], O[:, r, 1], O[:, r, 2]) for r in range(3)], 1)
    e2 = np.stack([_sel(k2, O[:, r, 0], O[:, r, 1], O[:, r, 2]) for r in range(3)], 1)
    hk, h1, h2 = (_sel(kk, oh[:, 0], oh[:, 1], oh[:, 2]) for kk in (k, k1, k2))
    dot = lambda u, v: (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]
    fc = oc + (sg * hk)[:, None] * nrm
    d_f = sg * dot(nrm, oc) + hk
    L = len(face)
    poly = np.zeros((L, MAX_VERTS, 2))
    poly[:, 0], poly[:, 1] = np.stack([-h1, -h2], 1), np.stack([h1, -h2], 1)
    poly[:, 2], poly[:, 3] = np.stack([h1, h2], 1), np.stack([-h1, h2], 1)
    n = np.full(L, 4, dtype=np.int64)
    # box 1's lanes look for the plane of box 2 that nearly coincides with their face; the pair is then scored by that lane alone
    paired, flat = np.zeros(L, bool), np.zeros(L, bool)
    opposite = np.zeros(L, bool)
    pa, pb, pc, d_o = np.zeros(L), np.zeros(L), np.zeros(L), np.zeros(L)
    partner = np.full(L, -1)
    most = 4
    rel = fc - yc
    for j in range(3):
        v = Y[:, :, j]
        a0, b, c_ = dot(v, rel), dot(v, e1), dot(v, e2)
        nv = sg * dot(nrm, v)
        vy = dot(v, yc)
        for ti, tau in enumerate((-1.0, 1.0)):
            a = tau * a0 - yh[:, j]
            near = ~second & ~paired & (np.abs(b) <= TILT) & (np.abs(c_) <= TILT) & (np.abs(a) <= sep)
            flat |= near & (tau * nv < 0) & ((np.abs(a) + np.abs(b) * h1) + np.abs(c_) * h2 <= eps)
            opposite = np.where(near, tau * nv < 0, opposite)
            pa, pb, pc = np.where(near, a, pa), np.where(near, tau * b, pb), np.where(near, tau * c_, pc)
            d_o = np.where(near, tau * vy + yh[:, j], d_o)
            partner = np.where(near, 6 + 2 * j + ti, partner)
            paired |= near
            # (the nearly coinciding plane is left for last: everything counts as inside it here)
            poly, n = _clip(poly, n, np.where(near, -1.0, a), np.where(near, 0.0, tau * b), np.where(near, 0.0, tau * c_))
            most = max(most, int(n.max()))
    area = _area(poly, n)
    inner, n_in = _clip(poly, n, np.where(paired, pa, -1.0), np.where(paired, pb, 0.0), np.where(paired, pc, 0.0))
    most = max(most, int(n_in.max()))
    area_in = _area(inner, n_in)
    term = np.where(paired, np.where(opposite, (d_f + d_o) * area_in, d_f * area_in + d_o * (area - area_in)), d_f * area)
    # box 2's faces that a lane of box 1 took over contribute nothing
    taken = np.zeros((rows, 12), bool)
    lanes_p = np.nonzero(paired)[0]
    taken[row[lanes_p], partner[lanes_p]] = True
    term = np.where(taken.reshape(-1), 0.0, term)
    V = term.reshape(rows, 12).sum(1) / 3.0
    V = np.where(flat.reshape(rows, 12).any(1), 0.0, V)
    V = np.where(V < 0, 0.0, V)
    v1, v2 = s1[pair].prod(1), s2[pair].prod(1)
    iou = V / (v1 + v2 - V)
    np.maximum.at(out, pair, iou)
    return (out, most) if return_max_verts else out


def normalised(RT_1, RT_2, scales_1, scales_2):
    """metrics.iou_3d's normalisation in float64: (R1, t1, s1, R2, t2, s2) with det(R)^(1/3) divided out of the rotations."""
    out = []
    for RT, s in ((RT_1, scales_1), (RT_2, scales_2)):
        RT = np.asarray(RT, np.float64)
        out += [RT[:3, :3] / np.cbrt(np.linalg.det(RT[:3, :3])), RT[:3, 3].copy(), np.asarray(s, np.float64).reshape(3)]
    return out


def is_symmetric(cls, hv):
    return cls in ("bottle", "bowl", "can") or (cls == "mug" and hv == 0)


def golden_pairs(pairs):
    """The golden's iou_pairs as the kernel's arguments: (R1, t1, s1, R2, t2, s2, turns, expected)."""
    cols = [[] for _ in range(6)]
    for p in pairs:
        for col, x in zip(cols, normalised(p["RT1"], p["RT2"], p["s1"], p["s2"])):
            col.append(x)
    turns = np.array([36 if is_symmetric(p["cls"], p["hv"]) else 1 for p in pairs], np.int32)
    return tuple(np.array(c) for c in cols) + (turns, np.array([p["iou"] for p in pairs]))


def rand_rot(rng):
    q, _ = np.linalg.qr(rng.randn(3, 3))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def analytic_tie_cases(seed=3, per_kind=10, along_y=False):
    """(R1, t1, s1, R2, t2, s2, expected, kind): box pairs built axis-aligned with exactly coinciding planes, then taken through
    one seeded random rotation and a translation; expected is the closed-form IoU at turns = 1.  along_y: every shift and
    contact along box 1's y axis, so that the value also holds for turns = 36 (a turn of box 1 about y then keeps a contact a
    contact and can only shrink the common cross-section; a contained box's IoU f = V2 / V1 is the largest possible anyway)."""
    rng = np.random.RandomState(seed)
    rows = []
    for i in range(per_kind):
        s = rng.uniform(0.2, 1.0, 3)
        axis = 1 if along_y else i % 3
        f = rng.uniform(0.2, 0.9)
        e = np.eye(3)[axis]
        sq = s.copy()
        sq[2] = sq[0]                                     # square section about y
        quarter = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])
        for kind, R2l, t2l, sa, sb, want in (
                ("identical", np.eye(3), np.zeros(3), s, s, 1.0),
                # box 2 shrunk by f along `axis`, pushed against box 1's face: it shares five planes with box 1
                ("shrunk", np.eye(3), e * s[axis] * (1 - f) / 2, s, np.where(e > 0, s * f, s), f),
                ("touching", np.eye(3), e * s[axis], s, s, 0.0),
                ("half_shift", np.eye(3), e * s[axis] / 2, s, s, 1.0 / 3.0),
                ("quarter_turn", quarter, np.zeros(3), sq, sq, 1.0)):
            Q, t = rand_rot(rng), rng.randn(3) * 0.3
            rows.append((Q, t, np.array(sa), Q @ R2l, t + Q @ t2l, np.array(sb), want, kind))
    cols = list(zip(*rows))
    return tuple(np.array(c) for c in cols[:7]) + (list(cols[7]),)


NEAR_TIE_MAGNITUDES = (1e-15, 1e-14, 1e-13, 3e-13, 1e-12, 3e-12, 1e-11, 1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 3e-6, 1e-5, 3e-5, 1e-4)
CLOSED_FORM_UP_TO = 1e-11        # a perturbation m moves the true IoU by at most ~15 m here: 1.5e-10 of the 1e-9 allowed


def _rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def near_tie_cases(seed=5, per_kind=2):
    """(R1, t1, s1, R2, t2, s2, closed, m, kind): every pair of analytic_tie_cases(seed, per_kind) with box 2 turned by a random
    rotation vector of length m, shifted by a random vector of length m, or both, for m in NEAR_TIE_MAGNITUDES.  closed: the
    unperturbed pair's closed-form IoU, which the perturbed pair's IoU is within ~15 m of."""
    rng = np.random.RandomState(seed + 1)
    R1, t1, s1, R2, t2, s2, want, kind = analytic_tie_cases(seed=seed, per_kind=per_kind)
    rows = []
    for m in NEAR_TIE_MAGNITUDES:
        for i in range(len(want)):
            for mode in ("rot", "rot+shift", "shift"):
                w, d = rng.randn(3), rng.randn(3)
                w, d = w * (m / np.linalg.norm(w)), d * (m / np.linalg.norm(d))
                rows.append((R1[i], t1[i], s1[i], _rodrigues(w) @ R2[i] if "rot" in mode else R2[i],
                             t2[i] + d if "shift" in mode else t2[i], s2[i], want[i], m, kind[i] + ":" + mode))
    cols = list(zip(*rows))
    return tuple(np.array(c) for c in cols[:8]) + (list(cols[8]),)


def near_tie_reference(cases, hull_iou):
    """What a near-tie case is held to: the closed form up to m = CLOSED_FORM_UP_TO (the hull is arbitrary on exact ties and is
    not trusted that close to one), above it hull_iou(R1, t1, s1, R2, t2, s2) = the host's convex hull, reliable away from ties."""
    R1, t1, s1, R2, t2, s2, closed, m, _ = cases
    return np.array([closed[i] if m[i] <= CLOSED_FORM_UP_TO else hull_iou(R1[i], t1[i], s1[i], R2[i], t2[i], s2[i])
                     for i in range(len(m))])


def random_pairs(P, seed, mixed=True):
    """(R1, t1, s1, R2, t2, s2, turns): seeded random overlapping box pairs, turns mixed 1 and 36."""
    rng = np.random.RandomState(seed)
    R1 = np.array([rand_rot(rng) for _ in range(P)]).reshape(P, 3, 3)
    R2 = np.array([rand_rot(rng) for _ in range(P)]).reshape(P, 3, 3)
    near = rng.rand(P) < 0.5                              # half of the pairs: box 2 a small turn away from box 1
    for i in np.nonzero(near)[0]:
        w = rng.randn(3) * 0.1
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        q, _ = np.linalg.qr(np.eye(3) + K)
        R2[i] = (q * np.sign(np.diag(q.T @ np.eye(3)))) @ R1[i]
        if np.linalg.det(R2[i]) < 0:
            R2[i] = rand_rot(rng)
    t1 = rng.randn(P, 3) * 0.3
    t2 = t1 + rng.randn(P, 3) * rng.choice([0.0, 0.02, 0.1, 0.5], (P, 1))
    s1 = rng.uniform(0.2, 1.0, (P, 3))
    s2 = s1 * rng.uniform(0.7, 1.3, (P, 3))
    turns = np.where(rng.rand(P) < 0.5, 36, 1).astype(np.int32) if mixed else np.ones(P, np.int32)
    return R1, t1, s1, R2, t2, s2, turns


def synthetic_results(images, seed=11, max_gt=7):
    """Per-image result records like tests/golden/make_golden_map.py's make_results (perturbed copies of the ground truth, now
    and then one dropped, false positives), with up to max_gt - 1 objects per image."""
    rng = np.random.RandomState(seed)

    def small_rot(deg):
        ax = rng.randn(3)
        ax /= np.linalg.norm(ax)
        a = np.radians(deg)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K

    out = []
    for _ in range(images):
        n_gt = rng.randint(1, max_gt)
        gt_cls = rng.randint(1, 7, n_gt)
        gt_RTs, gt_scales = [], []
        for _ in range(n_gt):
            RT = np.eye(4)
            RT[:3, :3] = rand_rot(rng) * rng.uniform(0.1, 0.4)
            RT[:3, 3] = rng.randn(3) * 0.3 + np.array([0, 0, 1.0])
            gt_RTs.append(RT)
            gt_scales.append(rng.uniform(0.3, 1.0, 3))
        p_cls, p_RTs, p_scales, p_scores = [], [], [], []
        for j in range(n_gt):
            if rng.rand() < 0.15:
                continue
            RT = gt_RTs[j].copy()
            RT[:3, :3] = small_rot(rng.choice([1.0, 4.0, 8.0, 14.0, 40.0])) @ RT[:3, :3] * rng.uniform(0.9, 1.1)
            RT[:3, 3] += rng.randn(3) * rng.choice([0.005, 0.03, 0.08])
            p_cls.append(gt_cls[j]); p_RTs.append(RT); p_scales.append(gt_scales[j] * rng.uniform(0.9, 1.1, 3))
            p_scores.append(rng.uniform(0.3, 1.0))
        for _ in range(rng.randint(0, 3)):
            RT = np.eye(4)
            RT[:3, :3] = rand_rot(rng) * 0.2
            RT[:3, 3] = rng.randn(3)
            p_cls.append(rng.randint(1, 7)); p_RTs.append(RT); p_scales.append(rng.uniform(0.3, 1.0, 3))
            p_scores.append(rng.uniform(0.0, 0.6))
        out.append(dict(gt_class_ids=gt_cls.astype(np.int32), gt_RTs=np.array(gt_RTs), gt_scales=np.array(gt_scales),
                        gt_handle_visibility=rng.randint(0, 2, n_gt).astype(np.int32),
                        pred_class_ids=np.array(p_cls, dtype=np.int32), pred_RTs=np.array(p_RTs).reshape(-1, 4, 4),
                        pred_scales=np.array(p_scales).reshape(-1, 3), pred_scores=np.array(p_scores, dtype=np.float64)))
    return out


def write_nocs_fixture(root, golden_dir):
    """Two images in the reference's REAL275 layout, built from the example frame under golden_dir/example_data (data, not code):
    <root>/real_test/scene_1/000{0,1}_depth.png (millimetres) and <root>/log/results_*.pkl with the keys eval.py:103-151 reads; one
    bottle and one can detection on the example object's mask."""
    import os
    import pickle
    from PIL import Image
    d = np.array(Image.open(os.path.join(golden_dir, "example_data", "depth.png")))
    m = np.array(Image.open(os.path.join(golden_dir, "example_data", "mask.png")))
    m = (m[..., 0] if m.ndim == 3 else m) > 0
    depth_mm = (d.astype(np.float64) / 10.0).round().astype(np.uint16)           # the example stores 1e-4 m, NOCS 1e-3 m
    os.makedirs(os.path.join(root, "real_test", "scene_1"))
    os.makedirs(os.path.join(root, "log"))
    rr, cc = np.nonzero(m)
    bbox = np.array([rr.min(), cc.min(), rr.max(), cc.max()])
    gt = np.eye(4)
    gt[:3, :3] *= 0.25
    gt[:3, 3] = [0.0, 0.0, 1.0]
    for frame, cls in enumerate((1, 4)):
        Image.fromarray(depth_mm).save(os.path.join(root, "real_test", "scene_1", "%04d_depth.png" % frame))
        rec = dict(image_path="data/real/test/scene_1/%04d" % frame, pred_bboxes=bbox[None], pred_masks=m[:, :, None],
                   pred_class_ids=np.array([cls]), pred_scores=np.array([0.9]), gt_class_ids=np.array([cls]), gt_RTs=gt[None],
                   gt_scales=np.ones((1, 3)) * 0.5, gt_bboxes=bbox[None], gt_handle_visibility=np.array([1]))
        with open(os.path.join(root, "log", "results_real_test_scene_1_%04d.pkl" % frame), "wb") as f:
            pickle.dump(rec, f)
