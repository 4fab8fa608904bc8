"""NumPy restatement of cppf_depth_condition (cppf2_amd/csrc/cppf_depthfilter.hip): every float32
operation in the kernel's order, so that the bytes match; and the analytic test scene with mixed pixels and range-dependent
noise that the CPU and the GPU tests share.  Nothing here needs the library or a GPU."""
import functools

import numpy as np

F = np.float32
JUMP = 0.01                 # masks.JUMP
TH, TW = 16, 64             # the kernel's tile (DF_TH, DF_TW)


def valid(d):
    """Finite and > 0, on the bits (a denormal is valid)."""
    b = np.ascontiguousarray(d, dtype=F).view(np.int32)
    return (b > 0) & (b < 0x7f800000)


def _shift(a, dy, dx, r, fill):
    """a[..., y + dy, x + dx] with `fill` outside the image (|dy|, |dx| <= r)."""
    H, W = a.shape[-2:]
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(r, r), (r, r)], constant_values=fill)
    return p[..., r + dy:r + dy + H, r + dx:r + dx + W]


def condition(depth, r1=1, min_support=4, r2=0, jump=JUMP, jump_rel=0.0):
    """(out float32 [I,H,W], counts int64 [I,3], d1 float32 [I,H,W]) of depth [I,H,W] or [H,W]."""
    d = np.ascontiguousarray(depth, dtype=F)
    d = d.reshape((1,) + d.shape) if d.ndim == 2 else d
    assert d.ndim == 3 and 0 <= r1 <= 4 and 0 <= r2 <= 4 and 0 <= min_support <= (2 * r1 + 1) ** 2
    jump, jump_rel = F(jump), F(jump_rel)
    v = valid(d)
    with np.errstate(all="ignore"):
        z = np.where(v, d, F(0))
        tol = (jump + (jump_rel * z).astype(F)).astype(F)
        support = np.zeros(d.shape, np.int32)
        inside = np.ones(d.shape, bool)
        for dy in range(-r1, r1 + 1):
            for dx in range(-r1, r1 + 1):
                if dy == 0 and dx == 0:
                    continue
                q, qv, qin = _shift(z, dy, dx, r1, F(0)), _shift(v, dy, dx, r1, False), _shift(inside, dy, dx, r1, False)
                support += ~qin | (qv & (np.abs((q - z).astype(F)) <= tol))
        d1 = np.where(v & (support >= min_support), z, F(0)).astype(F)
        k = d1 > 0
        tol = (jump + (jump_rel * d1).astype(F)).astype(F)
        s, n = d1.copy(), np.ones(d.shape, np.int32)
        first_half = [(dy, dx) for dy in range(-r2, 0) for dx in range(-r2, r2 + 1)] + [(0, dx) for dx in range(-r2, 0)]
        for dy, dx in first_half:
            a, b = _shift(d1, dy, dx, r2, F(0)), _shift(d1, -dy, -dx, r2, F(0))            # 0 outside the image: never a partner
            take = k & (a > 0) & (b > 0) & (np.abs((a - d1).astype(F)) <= tol) & (np.abs((b - d1).astype(F)) <= tol)
            s = np.where(take, ((s + a).astype(F) + b).astype(F), s)
            n = n + 2 * take
        out = np.where(k, (s / n.astype(F)).astype(F), F(0)).astype(F)
    ax = (1, 2)
    counts = np.stack([v.sum(ax), (v & ~k).sum(ax), (n > 1).sum(ax)], 1).astype(np.int64)
    return out, counts, d1


# ----------------------------------------------------------------------------------------------
# the scene: a 5 cm sphere at 0.55 m in front of a tilted plane
# ----------------------------------------------------------------------------------------------
H0, W0, F0, SS = 240, 320, 300.0, 4
PLANE_N, PLANE_D = np.array([0.0, -0.5, -0.866]), -0.62
CENTRE, RADIUS = np.array([0.0, 0.0, 0.55]), 0.05
FAR = 0.005                 # metres: "off the object", "off both surfaces of a mixed pixel"


def rays(H, W, f):
    """float64 [H,W,3]: pixel (v, u) looks along ((u + 0.5 - W/2) / f, (v + 0.5 - H/2) / f, 1)."""
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    return np.stack([(u + 0.5 - W / 2) / f, (v + 0.5 - H / 2) / f, np.ones((H, W))], -1)


def trace(H, W, f):
    """(depth float64 [H,W], hit bool [H,W]): the nearer intersection along each ray; hit = it is the sphere's."""
    d = rays(H, W, f)
    plane = PLANE_D / (d @ PLANE_N)
    a, b = (d * d).sum(-1), d @ CENTRE
    disc = b * b - a * (CENTRE @ CENTRE - RADIUS ** 2)
    sphere = np.where(disc >= 0, (b - np.sqrt(np.maximum(disc, 0))) / a, np.inf)
    hit = sphere < plane
    return np.where(hit, sphere, plane), hit


@functools.lru_cache(maxsize=None)
def scene(sigma, H=H0, W=W0, f=F0):
    """The scene at `sigma` metres of noise (at 0.6 m): a dict of read-only arrays [H,W] --
    depth float32: 4 x 4 block means of the 4H x 4W trace plus RandomState(0).randn(H,W) * sigma * (z / 0.6)^2, added in float64
    exact float32: the block means without noise;  coverage: the share of a block's rays that hit the sphere
    flying: 0 < coverage < 1 and the reading more than 5 mm from both the block's smallest and largest depth
    clean: coverage is 0 or 1;  mask: coverage >= 0.5;  rays float64 [H,W,3]."""
    fine, hit = trace(SS * H, SS * W, SS * f)
    blocks = fine.reshape(H, SS, W, SS)
    mean, lo, hi = blocks.mean((1, 3)), blocks.min((1, 3)), blocks.max((1, 3))
    coverage = hit.reshape(H, SS, W, SS).mean((1, 3))
    depth = (mean + np.random.RandomState(0).randn(H, W) * sigma * (mean / 0.6) ** 2).astype(F)
    mixed = (coverage > 0) & (coverage < 1)
    out = dict(depth=depth, exact=mean.astype(F), coverage=coverage, clean=~mixed, mask=coverage >= 0.5,
               flying=mixed & (np.abs(depth - lo) > FAR) & (np.abs(depth - hi) > FAR), rays=rays(H, W, f))
    for a in out.values():
        a.setflags(write=False)
    return out


def off_sphere(sc, z):
    """Distance (metres, float64) of each masked, kept (z > 0) pixel's back-projected point from the sphere's surface."""
    m = sc["mask"] & (z > 0)
    p = sc["rays"][m] * z[m].astype(np.float64)[:, None]
    return np.abs(np.linalg.norm(p - CENTRE, axis=1) - RADIUS)


def rms(a, b, m):
    return float(np.sqrt(np.mean((a[m].astype(np.float64) - b[m].astype(np.float64)) ** 2)))


def scene_figures(sc, out_default, out_smooth):
    """The figures the scene checks compare with their caps, of the defaults' output and of
    smooth_radius = 2's."""
    raw, exact = sc["depth"], sc["exact"]
    obj = sc["coverage"] == 1
    gone, gone_s = out_default == 0, out_smooth == 0
    kept, kept_obj = sc["clean"] & ~gone_s, obj & ~gone_s
    return dict(flying_removed=float(gone[sc["flying"]].mean()), clean_removed=float(gone[sc["clean"]].mean()),
                object_removed=float(gone[obj].mean()),
                far_raw=float((off_sphere(sc, raw) > FAR).mean()), far_after=int((off_sphere(sc, out_default) > FAR).sum()),
                rms_raw=rms(raw, exact, kept), rms_smooth=rms(out_smooth, exact, kept),
                rms_obj_raw=rms(raw, exact, kept_obj), rms_obj_smooth=rms(out_smooth, exact, kept_obj))


def check_scene(fig):
    """The caps that DESIGN.md section 33 states."""
    assert fig["flying_removed"] >= 0.95, fig
    assert fig["clean_removed"] <= 0.01 and fig["object_removed"] <= 0.01, fig
    assert fig["far_raw"] > 0 and fig["far_after"] == 0, fig
    assert fig["rms_smooth"] <= 0.5 * fig["rms_raw"], fig
    assert fig["rms_obj_smooth"] <= 0.75 * fig["rms_obj_raw"], fig


# ----------------------------------------------------------------------------------------------
# constructed images: readings on a 2^-10 lattice, jump = 2^-7
# ----------------------------------------------------------------------------------------------
LJ = F(2.0 ** -7)
SPECIALS = [np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e-40]          # the last is a denormal: valid


def lattice_images(seed, I, H, W, holes=0.2, dead=None):
    """float32 [I,H,W]: readings k * 2^-10 around 0.5 m in patches (steps between patches on either side of the gate), about
    `holes` of them replaced by SPECIALS; image `dead` entirely invalid."""
    rng = np.random.RandomState(seed)
    base = 512 + 24 * rng.randint(0, 3, (I, (H + 3) // 4, (W + 3) // 4)).repeat(4, 1).repeat(4, 2)[:, :H, :W]
    d = ((base + rng.randint(-5, 6, (I, H, W))) * 2.0 ** -10).astype(F)
    hole = rng.rand(I, H, W) < holes
    d[hole] = np.array(SPECIALS, F)[rng.randint(0, len(SPECIALS), int(hole.sum()))]
    if dead is not None:
        d[dead] = np.array(SPECIALS[:6], F)[rng.randint(0, 6, (H, W))]
    return d
