"""Restatement of cppf_scene_explain (cppf2_amd/csrc/cppf_scene.hip) in NumPy, one operation per step: the
per-pixel predicates of cppf_depth_fit_counts at one tau, the static counts per candidate, and the greedy rounds.  Everything
is an integer count or an integer maximum, so the GPU outputs must equal these byte for byte."""
import numpy as np

NONE = 255


def predicates(d_o, m, d_c, tau):
    """(drawn, fit, viol) bool [C,H,W] of the renders d_c float32 [C,H,W] against d_o float32 [H,W] and region m [H,W].
    Comparisons with 0 in float32, the difference in float64, NaN compares false."""
    d_o = np.asarray(d_o, dtype=np.float32)
    d_c = np.asarray(d_c, dtype=np.float32).reshape((-1,) + d_o.shape)
    tau_d = np.float64(np.float32(tau))
    with np.errstate(invalid="ignore"):
        seen = d_o > np.float32(0)
        obs = seen & (np.asarray(m) != 0)
        drawn = d_c > np.float32(0)
        diff = d_o.astype(np.float64)[None] - d_c.astype(np.float64)
        fit = obs[None] & drawn & (np.abs(diff) <= tau_d)
        viol = drawn & seen[None] & (diff > tau_d)
    return drawn, fit, viol


def explain_image(d_o, m, d_c, tau, min_gain, viol_weight, max_rounds):
    """One image: dict(chosen int32 [M], gain int64 [M], net int64 [M], static int64 [C,3], labels uint8 [H,W], summary int64 [3])."""
    d_o = np.asarray(d_o, dtype=np.float32)
    M = int(max_rounds)
    drawn, fit, viol = predicates(d_o, m, d_c, tau)
    C = fit.shape[0]
    npx = d_o.size
    static = np.stack([drawn.reshape(C, npx).sum(1), fit.reshape(C, npx).sum(1), viol.reshape(C, npx).sum(1)], 1).astype(np.int64)
    with np.errstate(invalid="ignore"):
        region_pixels = int(((d_o > np.float32(0)) & (np.asarray(m) != 0)).sum())
    unexplained = np.ones(d_o.shape, dtype=bool)
    labels = np.full(d_o.shape, NONE, dtype=np.uint8)
    chosen = np.full(M, -1, dtype=np.int32)
    gain = np.zeros(M, dtype=np.int64)
    net = np.zeros(M, dtype=np.int64)
    taken = np.zeros(C, dtype=bool)
    rounds = 0
    for k in range(M):
        g = (fit & unexplained[None]).reshape(C, npx).sum(1).astype(np.int64)
        n = g - np.int64(viol_weight) * static[:, 2]
        eligible = ~taken & (n >= np.int64(min_gain))
        if not eligible.any():
            break
        # (uint64)net << 32 | (0xFFFFFFFF - c): only an eligible, hence positive, net is converted
        keys = [(int(n[c]) << 32) | (0xFFFFFFFF - c) for c in range(C) if eligible[c]]
        assert all(0 < key < 1 << 63 for key in keys)
        w = 0xFFFFFFFF - (max(keys) & 0xFFFFFFFF)
        chosen[k], gain[k], net[k] = w, g[w], n[w]
        labels[fit[w] & unexplained] = k
        unexplained &= ~fit[w]
        taken[w] = True
        rounds = k + 1
    summary = np.array([region_pixels, int((labels != NONE).sum()), rounds], dtype=np.int64)
    return dict(chosen=chosen, gain=gain, net=net, static=static, labels=labels, summary=summary)


def explain(depth, region, cand_off, renders, tau, min_gain, viol_weight, max_rounds):
    """The batch: image i with the renders cand_off[i] .. cand_off[i+1]-1; the outputs of scene.explain as host arrays."""
    depth = np.asarray(depth, dtype=np.float32)
    depth = depth[None] if depth.ndim == 2 else depth
    region = np.asarray(region).reshape(depth.shape)
    renders = np.asarray(renders, dtype=np.float32).reshape((-1,) + depth.shape[1:])
    per = [explain_image(depth[i], region[i], renders[cand_off[i]:cand_off[i + 1]], tau, min_gain, viol_weight, max_rounds)
           for i in range(depth.shape[0])]
    out = {k: np.stack([p[k] for p in per]) for k in ("chosen", "gain", "net", "labels", "summary")}
    out["static"] = np.concatenate([p["static"] for p in per]).reshape(-1, 3)
    return out


def order_case(H=12, W=20, at=0):
    """Observed depth 1 m everywhere, the whole image the region.  A fits 100 pixels; B fits 60, 50 of them inside A; C fits 55
    pixels apart from both.  The pixels are taken from position `at` of the row-major order onward.  Returns (d_o, m, renders
    [3,H,W] = A, B, C)."""
    d_o = np.full((H, W), 1.0, np.float32)
    m = np.ones((H, W), np.uint8)
    ren = np.zeros((3, H * W), np.float32)
    ren[0, at:at + 100] = 1.0
    ren[1, at + 50:at + 110] = 1.0
    ren[2, at + 120:at + 175] = 1.0
    return d_o, m, ren.reshape(3, H, W)


def tau_edge_case(tau=0.02):
    """One row of ten pixels whose float64 difference d_o - d_c is exactly +-float32(tau) or one float32 step of d_c to either
    side of it (2 * tau and the neighbours of tau and 2 * tau are float32 numbers, and their differences are exact in float64).
    Pixel: 0 diff == tau; 1 one step above tau; 2 one step below; 3 diff == -tau; 4 one step beyond -tau; 5 one step inside;
    6 and 7: pixels 0 and 1 outside the region; 8 d_o one step above 2 * tau against tau; 9 d_o one step below.
    Returns (d_o [1,10], m [1,10], d_c [1,1,10])."""
    f = np.float32
    t = f(tau)
    t2 = f(2) * t
    dn, up = (lambda x: np.nextafter(x, f(0))), (lambda x: np.nextafter(x, f(1)))
    d_o = np.array([[t2, t2, t2, t, t, t, t2, t2, up(t2), dn(t2)]], f)
    d_c = np.array([[[t, dn(t), up(t), t2, up(t2), dn(t2), t, dn(t), t, t]]], f)
    m = np.array([[1, 1, 1, 1, 1, 1, 0, 0, 1, 1]], np.uint8)
    assert np.float64(d_o[0, 0]) - np.float64(d_c[0, 0, 0]) == np.float64(t) == np.float64(d_c[0, 0, 3]) - np.float64(d_o[0, 3])
    return d_o, m, d_c

