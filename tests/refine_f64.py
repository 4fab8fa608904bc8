"""Independent float64 reference of the online alignment refinement (eval.py:321-350; what refine_pose_kernel computes, not
how), and the banded input family the kernel-level GPU tests run it on.  The gradients come from torch.autograd in float64
(the loss of (I + hat(xi)) M R0 at xi = 0, and of t), so the reference shares neither the oracle's nor the kernel's hand
derivation; this module does not import the oracle.  Test infrastructure only."""
import numpy as np
import torch

F64 = torch.float64


def _hat(v):
    z = v[0] * 0
    return torch.stack([torch.stack([z, -v[2], v[1]]), torch.stack([v[2], z, -v[0]]), torch.stack([-v[1], v[0], z])])


def so3_matrix_f64(q):
    """lietorch's SO3(q).matrix() for q = (x, y, z, w), not normalised: I + 2 w hat(v) + 2 hat(v)^2."""
    q = torch.as_tensor(q, dtype=F64)
    h = _hat(q[:3])
    return torch.eye(3, dtype=F64) + 2 * q[3] * h + 2 * h @ h


def refine_f64(pc, idx2, tgt, t0, R0, y_only, steps, lr=1e-2, return_margins=False, return_components=False, mask=None):
    """`steps` Adam updates (torch defaults, eps outside the root) of the translation and of the quaternion (0, 0, 0, 1) on
    mean |((P - t) @ (M(q) R0)) - tgt| over all coordinates, or over y when y_only.  pc [N,3]; idx2 int [Tf,2]; tgt [Tf,2,3];
    t0 [3] and R0 [3,3] are rounded to float32 first (the kernel reads the record's doubles as floats), everything after that
    is float64.  The quaternion's xyz gradient is the left-tangent gradient times pi / 180, its w gradient 0.  Returns
    (t [3], R [3,3]) as float64 arrays; with return_margins also (the smallest |residual| of an element in the loss, the
    smallest |g_c| of the six gradient components Adam sees for t and the tangent), both minima over all steps (inf for
    steps = 0); with return_components the second is the six per-component minima instead.  mask (bool [Tf,2], all true when
    None) leaves single end points out of the loss and of its mean."""
    P = torch.as_tensor(np.asarray(pc, dtype=np.float64)[np.asarray(idx2, dtype=np.int64)])        # [Tf,2,3]
    tgt = torch.as_tensor(np.asarray(tgt, dtype=np.float64).reshape(-1, 2, 3))
    t = torch.as_tensor(np.asarray(t0, dtype=np.float64).reshape(3).astype(np.float32).astype(np.float64))
    R0 = torch.as_tensor(np.asarray(R0, dtype=np.float64).reshape(3, 3).astype(np.float32).astype(np.float64))
    q = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=F64)
    x = torch.cat([t, q])                                           # the 7 parameters
    m, v = torch.zeros(7, dtype=F64), torch.zeros(7, dtype=F64)
    b1, b2, eps = 0.9, 0.999, 1e-8
    min_res, min_g = np.inf, np.full(6, np.inf)
    on = torch.ones(tgt.shape[:2], dtype=torch.bool) if mask is None else torch.as_tensor(np.asarray(mask, dtype=bool))
    for step in range(1, steps + 1):
        tt = x[:3].clone().requires_grad_(True)
        xi = torch.zeros(3, dtype=F64, requires_grad=True)
        rot = (torch.eye(3, dtype=F64) + _hat(xi)) @ so3_matrix_f64(x[3:]) @ R0
        r = ((P - tt) @ rot - tgt)[on]                              # [elements in the loss, 3]
        if y_only:
            r = r[:, 1]
        r.abs().mean().backward()
        g = torch.cat([tt.grad, xi.grad * (np.pi / 180.0), torch.zeros(1, dtype=F64)])
        min_res = min(min_res, float(r.detach().abs().min()))
        min_g = np.minimum(min_g, g[:6].abs().numpy())
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        denom = v.sqrt() / np.sqrt(1 - b2 ** step) + eps
        x = x - (lr / (1 - b1 ** step)) * m / denom
    R = (so3_matrix_f64(x[3:]) @ R0).numpy()
    if return_components:
        return x[:3].numpy().copy(), R, min_res, min_g
    if return_margins:
        return x[:3].numpy().copy(), R, min_res, float(min_g.min())
    return x[:3].numpy().copy(), R


# ---------------------------------------------------------------------------------------------------------------------------
# The banded input family: every residual starts 4.5-5.5 mm or 60-80 mm from zero.  One Adam step moves every coordinate by
# about 1 cm, so the near band changes sign between step 1 and step 2 by a wide margin and the far band never does; the
# gradient of step 2 differs from that of step 1 by a known, robust amount, and the pose after two steps depends smoothly on
# their ratio -- which Adam's first step (+-lr whatever the gradient's size) hides.

N_POINTS = 3000


def start_pose():
    """(R0, t0): 2 degrees about a generic axis (no gradient component is structurally zero), as float32-valued doubles."""
    ax = np.array([0.48, -0.62, 0.62])
    ax /= np.linalg.norm(ax)
    a = np.radians(2.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R0 = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    t0 = np.array([0.054, -0.034, 0.904])
    return R0.astype(np.float32).astype(np.float64), t0.astype(np.float32).astype(np.float64)


def banded_scene(kept, seed):
    """(pc f32 [3000,3], idx2 int64 [kept,2], tgt f32 [kept,2,3], R0, t0) of the family, seeded by (kept, seed)."""
    rng = np.random.RandomState([kept, seed])
    R0, t0 = start_pose()
    canon = (rng.rand(N_POINTS, 3) - 0.5) * np.array([0.08, 0.2, 0.08])
    pc = (canon @ R0.T + t0).astype(np.float32)
    idx2 = rng.randint(0, N_POINTS, (kept, 2)).astype(np.int64)
    c_start = (pc.astype(np.float64)[idx2] - t0) @ R0
    s = np.where(rng.rand(kept, 2, 3) < 0.6, 1.0, -1.0)
    near = rng.rand(kept, 2, 3) < 0.5
    mag = np.where(near, rng.uniform(4.5e-3, 5.5e-3, (kept, 2, 3)), rng.uniform(60e-3, 80e-3, (kept, 2, 3)))
    tgt = (c_start - s * mag).astype(np.float32)
    return pc, idx2, tgt, R0, t0


# ---------------------------------------------------------------------------------------------------------------------------
# The step cases and their preconditions, shared by the CPU and the GPU tests.

RES_FLOOR = 1e-4            # smallest |residual|: 1000 x the float32 error of a canonicalised coordinate
G_FLOOR = 1e-6              # smallest |g_c|: 100 x Adam's eps
G_FLOOR_SPIN = 1e-7         # see gradient_floors
T_FLOOR, R_FLOOR = 2.5e-7, 5e-7      # 4 ulp of a float32 at 0.9 (m) and at 1.0
SEES_A_PAIR = 10.0          # the reference without the last kept pair is this many bars away
BIG = 2047                  # the kept counts from here on run 1 and 2 steps, the smaller ones 1 to 4


def gradient_floors(kept, y_only):
    """The floor of each of the six gradient components.  G_FLOOR everywhere but for one component of the large y_only
    cases: a y-only loss does not change under a rotation about the object's y axis a = rot e_y, so the tangent gradient is
    orthogonal to a; with R0 two degrees from the identity a is within 0.035 of e_y and the gradient's y component is about
    0.03 of its x and z components, which are zero-mean sums over the elements (the signs do not depend on the lever arms)
    and shrink as 1 / sqrt(kept).  From 2047 pairs on no seed of 300 reaches 1e-6 there (the largest 5e-7, the median 1e-7),
    so that component's floor is 10 x eps.  What the floor is for still holds: Adam's update is lr m^ / (sqrt(v^) + eps), its
    first step's slope in g is lr eps / (|g| + eps)^2 <= 8.3e3 at |g| = 1e-7, and the float32 error of that component, a sum
    of 2 * kept terms of at most 0.12 / (2 * kept) with rounding errors that add as a random walk, is about
    sqrt(2 * kept) * 2^-24 * 3e-5 * pi / 180 ~ 2e-12 at 2047 pairs: 2e-8 in the update, a fiftieth of the smallest bar."""
    f = np.full(6, G_FLOOR)
    if y_only and kept >= BIG:
        f[4] = G_FLOOR_SPIN
    return f


def bars(t_ref, R_ref, t_orc, R_orc):
    """(bar_t, bar_R, e_t, e_R): 4 x the float32 oracle's distance to the float64 reference, floored at 4 ulp."""
    e_t, e_R = float(np.abs(t_orc - t_ref).max()), float(np.abs(R_orc - R_ref).max())
    return 4 * max(e_t, T_FLOOR), 4 * max(e_R, R_FLOOR), e_t, e_R


def evaluate_case(kept, steps, y_only, seed, lr, oracle_refine, start=None):
    """Runs the reference (with and without the last kept pair) and `oracle_refine` (the float32 restatement's refine_pose,
    handed in: this module does not import it) on a scene of the family.  Returns a dict: the scene, the reference's t and R,
    the bars, and the figures of the three preconditions.  start = (R0, t0) replaces the starting pose the record holds (the
    targets stay those of the family's own start)."""
    pc, idx2, tgt, R0, t0 = banded_scene(kept, seed)
    if start is not None:
        R0, t0 = start
    t, R, min_res, g = refine_f64(pc, idx2, tgt, t0, R0, y_only, steps, lr, return_components=True)
    t_o, R_o = oracle_refine(pc, idx2, tgt, t0, R0, y_only, steps=steps, lr=lr)
    bar_t, bar_R, e_t, e_R = bars(t, R, t_o, R_o)
    if kept > 1:
        t_d, R_d = refine_f64(pc, idx2[:-1], tgt[:-1], t0, R0, y_only, steps, lr)
    else:                                                           # nothing kept: the kernel leaves the record as it was
        t_d, R_d = t0, R0
    sees = max(np.abs(t_d - t).max() / bar_t, np.abs(R_d - R).max() / bar_R)
    return dict(pc=pc, idx2=idx2, tgt=tgt, R0=R0, t0=t0, t=t, R=R, bar_t=bar_t, bar_R=bar_R, e_t=e_t, e_R=e_R,
                min_res=min_res, g=g, g_ok=bool(np.all(g >= gradient_floors(kept, y_only))), sees=float(sees))


def step_case(kept, steps, y_only, seed, lr, oracle_refine, start=None):
    """evaluate_case with the preconditions asserted.  The third one, that the comparison can see one missing pair, is
    asserted from two steps on (and for a single pair, whose absence leaves the start pose): after one step every parameter
    has moved by lr (1 - eps / |g|) against its gradient's sign whatever the gradient's size, so no bar can see a pair that
    does not turn a sign, and at one step the comparison checks the six signs, the update's arithmetic and the composed
    rotation; the one-element scenes of the GPU tests are what sees a dropped element there."""
    c = evaluate_case(kept, steps, y_only, seed, lr, oracle_refine, start)
    assert c["min_res"] >= RES_FLOOR, (kept, steps, y_only, seed, c["min_res"])
    assert c["g_ok"], (kept, steps, y_only, seed, c["g"])
    if steps >= 2 or kept == 1:
        assert c["sees"] >= SEES_A_PAIR, (kept, steps, y_only, seed, c["sees"])
    return c


# (kept pairs, steps, y_only, seed, lr): for each case the first seed of 0 .. 399 at which the three preconditions hold.
# Kept counts: the smallest (1 pair = 2 elements on 2 lanes), the wavefront boundary (32 / 33 pairs = 64 / 66 elements), the
# workgroup boundary (128 / 129), the register-cache boundary (2047 / 2048 / 2049 pairs = 4094 / 4096 / 4098 elements), a
# memory-resident tail that ends a full round (2176) and a ragged one (2177), and 4500.  The last two rows: lr = 3e-3.
STEP_CASES = [
    (1, 1, False, 0, 1e-2), (1, 1, True, 3, 1e-2), (1, 2, False, 1, 1e-2), (1, 2, True, 8, 1e-2),
    (1, 3, False, 1, 1e-2), (1, 3, True, 8, 1e-2), (1, 4, False, 2, 1e-2), (1, 4, True, 8, 1e-2),
    (2, 1, False, 0, 1e-2), (2, 1, True, 0, 1e-2), (2, 2, False, 0, 1e-2), (2, 2, True, 0, 1e-2),
    (2, 3, False, 0, 1e-2), (2, 3, True, 0, 1e-2), (2, 4, False, 1, 1e-2), (2, 4, True, 1, 1e-2),
    (32, 1, False, 1, 1e-2), (32, 1, True, 0, 1e-2), (32, 2, False, 1, 1e-2), (32, 2, True, 0, 1e-2),
    (32, 3, False, 2, 1e-2), (32, 3, True, 0, 1e-2), (32, 4, False, 6, 1e-2), (32, 4, True, 6, 1e-2),
    (33, 1, False, 0, 1e-2), (33, 1, True, 5, 1e-2), (33, 2, False, 0, 1e-2), (33, 2, True, 8, 1e-2),
    (33, 3, False, 1, 1e-2), (33, 3, True, 8, 1e-2), (33, 4, False, 1, 1e-2), (33, 4, True, 8, 1e-2),
    (128, 1, False, 0, 1e-2), (128, 1, True, 9, 1e-2), (128, 2, False, 0, 1e-2), (128, 2, True, 9, 1e-2),
    (128, 3, False, 42, 1e-2), (128, 3, True, 9, 1e-2), (128, 4, False, 147, 1e-2), (128, 4, True, 12, 1e-2),
    (129, 1, False, 0, 1e-2), (129, 1, True, 2, 1e-2), (129, 2, False, 0, 1e-2), (129, 2, True, 2, 1e-2),
    (129, 3, False, 149, 1e-2), (129, 3, True, 75, 1e-2), (129, 4, False, 329, 1e-2), (129, 4, True, 75, 1e-2),
    (2047, 1, False, 0, 1e-2), (2047, 1, True, 0, 1e-2), (2047, 2, False, 0, 1e-2), (2047, 2, True, 1, 1e-2),
    (2048, 1, False, 0, 1e-2), (2048, 1, True, 2, 1e-2), (2048, 2, False, 2, 1e-2), (2048, 2, True, 2, 1e-2),
    (2049, 1, False, 2, 1e-2), (2049, 1, True, 1, 1e-2), (2049, 2, False, 2, 1e-2), (2049, 2, True, 1, 1e-2),
    (2176, 1, False, 1, 1e-2), (2176, 1, True, 3, 1e-2), (2176, 2, False, 2, 1e-2), (2176, 2, True, 3, 1e-2),
    (2177, 1, False, 0, 1e-2), (2177, 1, True, 1, 1e-2), (2177, 2, False, 0, 1e-2), (2177, 2, True, 1, 1e-2),
    (4500, 1, False, 0, 1e-2), (4500, 1, True, 2, 1e-2), (4500, 2, False, 0, 1e-2), (4500, 2, True, 3, 1e-2),
    (129, 2, False, 2, 3e-3), (129, 2, True, 3, 3e-3),
]


# The same scenes started from a record whose doubles are not float32 values (the float32 start plus 1e-9, which moves the
# entries of R below 2^-5 to the next float32 and leaves the others where they were).
OFF_GRID_CASES = [(33, 2, False, 0, 1e-2), (33, 2, True, 8, 1e-2)]


def off_grid_start():
    R0, t0 = start_pose()
    return R0 + 1e-9, t0 + 1e-9


def case_id(case):
    kept, steps, y_only, seed, lr = case
    return "%d-%dstep-%s%s" % (kept, steps, "y" if y_only else "xyz", "" if lr == 1e-2 else "-lr%g" % lr)


# ---------------------------------------------------------------------------------------------------------------------------
# One element decides: a scene of DECISIVE_NE loss elements, one step from R0 = I, t0 = 0, in which the sign of the rotation
# gradient's z component hangs on the single element e_star.  All other elements sit within 0.1 m of the origin with residuals
# of +1 to +3 cm in every coordinate; element e_star is a dedicated point 50 m off along x whose y residual is negative.  The
# others' x and y coordinates are offset by +-4 mm, so their z torque sum (dx - dy) / n (sum dx / n when y_only) is about
# +35 / n (+17 / n) with a spread of 3 / n, clearly positive; e_star adds -50 / n and turns it.  The first Adam step is
# -lr sign(g), so the quaternion's z lands at +lr with the element and at -lr without it.

DECISIVE_NE = 4354
DECISIVE_POSITIONS = (0, 1, 63, 64, 255, 256, 4095, 4096, 4351, 4352, DECISIVE_NE - 1)


def decisive_scene(e_star):
    """(pc f32 [3001,3], idx2 int64 [2177,2], tgt f32 [2177,2,3], mask bool [2177,2] that is false at e_star only)."""
    rng = np.random.RandomState([DECISIVE_NE, e_star])
    kept = DECISIVE_NE // 2
    pc = ((rng.rand(N_POINTS + 1, 3) - 0.5) * 0.1 + np.array([0.004, -0.004, 0.012])).astype(np.float32)
    pc[N_POINTS] = (50.0, 0.013, -0.021)
    idx2 = rng.randint(0, N_POINTS, (kept, 2)).astype(np.int64)
    idx2[e_star // 2, e_star % 2] = N_POINTS
    res = rng.uniform(0.01, 0.03, (kept, 2, 3))
    res[e_star // 2, e_star % 2, 1] *= -1
    tgt = (pc.astype(np.float64)[idx2] - res).astype(np.float32)
    mask = np.ones((kept, 2), dtype=bool)
    mask[e_star // 2, e_star % 2] = False
    return pc, idx2, tgt, mask
