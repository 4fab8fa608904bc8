"""Golden outputs of the split-arithmetic ResLayer kernels (cppf_mlp_split.hip) at the kernels' edges, for
tests/test_mlp_split_lean_gpu.py: byte equality of a later build with the build this file was run on.

    python tests/golden/mlp_split/make_golden_mlp_split.py     (on the GPU, at the commit whose outputs are the reference)

writes, beside itself (a directory of its own: tests/test_golden_regen.py keeps the table of the CPU generators and fixtures that
lie directly in tests/golden), mlp_split_lean.npz (the arrays of the cases of at most ARRAY_ROWS rows) and mlp_split_lean_sha256.json (the SHA-256 of every
output's bytes).  Inputs and weights come from numpy's RandomState (a frozen stream) and are placed, not computed, so the same call
yields the same bytes everywhere; only public cppf2_amd.ops entry points (and models.pack_split for the weight stream) are used.

Forms (k_in -> n_out, chained identity layers):
  plain    128 -> 128 identity skip, chain 1                        proj     352 -> 128 projection, chain 4 (point-encoder shape)
  encode   40 pair features + 5 x 64 gathered = 360 -> 128, chain 4, two ragged scenes: the one launch with a ragged K step
  gather   the same rows through the two-kernel form (head array + gathering launch)
  tap      128 -> 256 projection, chain 2: `out` and the tapped first-layer output
  decode   256 -> 192 with the bin draw; decode_prior: with the generated prior
Special rows (plain / proj): *_nan = one input row holds a NaN; *_negzero = row 7 of the first fc1 (and row 9 of the first chained
fc1) is all zero with bias -0.0, so those hidden pre-activations are zeros whose sign only the ReLU's form decides; zero_layer = a
projection layer whose EVERY term is a signed zero (W1 = W0 = +0, b1 = b0 = -0.0, every piece of every W2 entry and of every x
entry negative on half of the rows): the one construction in which the sign of a hidden zero can reach a stored output.
Rows 901 = 128 * 7 + 5 run on a forced grid of 2 workgroups (several row blocks each, the dynamic claim path)."""
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ARRAYS = os.path.join(HERE, "mlp_split_lean.npz")
DIGESTS = os.path.join(HERE, "mlp_split_lean_sha256.json")
ARRAY_ROWS = 33
ROWS = [1, 31, 32, 33, 255, 256, 257, 128 * 7 + 5]
FORCED_GRID_ROWS = 128 * 7 + 5
FORMS = ["plain", "proj", "encode", "gather", "tap", "decode", "decode_prior"]
SPECIAL = [(f, r) for f in ("plain_nan", "proj_nan", "plain_negzero", "proj_negzero") for r in (33, 257)] + [("zero_layer", 33), ("zero_layer", 257)]
CASES = [(f, r) for f in FORMS for r in ROWS] + SPECIAL + [("encode", 353)]          # 353 = 150 + 203 tuples
NAN_ROW = 5
NEG = -(1.0 + 2.0 ** -9 + 2.0 ** -18)        # bf16 pieces (-1, -2^-9, -2^-18): all three negative


def _rs(*key):
    return np.random.RandomState(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (1 << 31))


def _randn(rs, *shape, scale=1.0):
    return (rs.standard_normal(shape) * scale).astype(np.float32)


def _layer(rs, k, n, proj, chain):
    w1 = _randn(rs, n, k, scale=k ** -0.5)
    w2 = _randn(rs, n, n, scale=n ** -0.5)
    w0 = _randn(rs, n, k, scale=k ** -0.5) if proj else None
    rest = [(_randn(rs, n, n, scale=n ** -0.5), _randn(rs, n, n, scale=n ** -0.5)) for _ in range(chain)]
    b1 = _randn(rs, (1 + chain) * n, scale=0.1)
    b0 = _randn(rs, n, scale=0.1) if proj else None
    return w1, w0, w2, rest, b1, b0


def scene_split(rows):
    """(points per scene, tuples per scene) of the gathering forms: two ragged scenes (one for a single row)."""
    if rows == 1:
        return [40], [1]
    a = 150 if rows == 353 else max(1, rows * 3 // 7)
    return [40, 57], [a, rows - a]


def run_case(form, rows):
    """{output name: numpy array} of one case, computed on cuda:0 by the library that is loaded."""
    import torch
    from cppf2_amd import _lib, models, ops
    dev = torch.device("cuda:0")
    L = _lib.load()

    def t(a, dtype=None):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)

    def stream(w1, w0, w2, k, rest):
        return models.pack_split(t(w1), t(w0), t(w2), k, chain=[(t(a), t(b)) for a, b in rest])

    base = form.split("_")[0] if form not in ("decode_prior", "zero_layer") else form
    out = {}
    forced = rows == FORCED_GRID_ROWS
    if forced:
        _lib.check(L.cppf_reslayer_split_debug_grid(2), "grid")
    try:
        if base in ("plain", "proj"):
            k, n, proj, chain = (128, 128, False, 1) if base == "plain" else (352, 128, True, 4)
            w1, w0, w2, rest, b1, b0 = _layer(_rs(1, k), k, n, proj, chain)
            x = _randn(_rs(2, k, rows), rows, k)
            if form.endswith("_nan"):
                x[min(NAN_ROW, rows - 1), 17] = np.nan
            if form.endswith("_negzero"):
                w1[7, :] = 0.0
                b1[7] = -0.0
                rest[0][0][9, :] = 0.0
                b1[n + 9] = -0.0
            out["out"] = ops.reslayer_split(t(x), stream(w1, w0, w2, k, rest), t(b1), t(b0), n, out=None if proj else torch.empty(rows, n, device=dev),
                                            chain=chain)
        elif form == "zero_layer":
            k, n = 352, 128
            x = np.full((rows, k), NEG, np.float32)
            x[1::2] = -NEG
            w1 = np.zeros((n, k), np.float32)
            w2 = np.full((n, n), NEG, np.float32)
            b = np.full(n, -0.0, np.float32)
            out["out"] = ops.reslayer_split(t(x), stream(w1, w1.copy(), w2, k, []), t(b), t(b.copy()), n)
        elif base in ("encode", "gather"):
            Ns, Ts = scene_split(rows)
            rs = _rs(3, rows)
            pts, nrm, feat = _randn(rs, sum(Ns), 3), _randn(rs, sum(Ns), 3), _randn(rs, sum(Ns), 64)
            idx = np.concatenate([rs.randint(0, n_, (t_, 5)) for n_, t_ in zip(Ns, Ts)]).astype(np.int32)
            w1, w0, w2, rest, b1, b0 = _layer(_rs(1, 360), 360, 128, True, 4)
            wq = stream(w1, w0, w2, 360, rest)
            pt_off, tup_off = ops._offsets(Ns, dev), ops._offsets(Ts, dev)
            if base == "encode":
                src = ops.TupleSource(t(pts), t(idx), t(nrm), pt_off, tup_off)
                out["out"] = ops.reslayer_split_encode(src, t(feat), wq, t(b1), t(b0), 128, chain=4)
            else:
                heads, gidx = ops.encode_tuples_shot_heads(t(pts), t(idx), t(nrm), pt_off, tup_off)
                out["out"] = ops.reslayer_split_gather(heads, gidx, t(feat), wq, t(b1), t(b0), 128, chain=4)
        elif base == "tap":
            w1, w0, w2, rest, b1, b0 = _layer(_rs(1, 128, 256), 128, 256, True, 2)
            x = _randn(_rs(2, 128, rows), rows, 128)
            tap = torch.empty(rows, 256, device=dev)
            out["out"] = ops.reslayer_split(t(x), stream(w1, w0, w2, 128, rest), t(b1), t(b0), 256, chain=2, tap=tap)
            out["tap"] = tap
        else:
            w1, w0, w2, rest, b1, b0 = _layer(_rs(1, 256, 192), 256, 192, True, 0)
            rs = _rs(4, rows)
            x = _randn(rs, rows, 256)
            u = rs.random_sample((rows, 6)).astype(np.float32)
            prior = None
            if form == "decode_prior":
                prior = ops.BinPrior(t((rs.random_sample((rows, 6)) * 31.0).astype(np.float32)), 0.5)
            out["bins"] = ops.reslayer_split_decode(t(x), stream(w1, w0, w2, 256, rest), t(b1), t(b0), t(u), prior=prior)
        torch.cuda.synchronize()
        out = {k_: v.cpu().numpy() for k_, v in out.items()}
        out["sched"] = np.stack([b.cpu().numpy() for b in ops._SCHED.values()]) if ops._SCHED else np.zeros((1, 2), np.int32)
    finally:
        if forced:
            L.cppf_reslayer_split_debug_grid(0)
    return out


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def key(form, rows, name):
    return "%s/%d/%s" % (form, rows, name)


def main():
    arrays, digests = {}, {}
    for form, rows in CASES:
        for name, a in run_case(form, rows).items():
            if name == "sched":
                assert not a.any(), (form, rows, a)
                continue
            digests[key(form, rows, name)] = digest(a)
            if rows <= ARRAY_ROWS:
                arrays[key(form, rows, name)] = a
    np.savez_compressed(ARRAYS, **arrays)
    with open(DIGESTS, "w") as f:
        json.dump(digests, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %d arrays, %d digests" % (len(arrays), len(digests)))


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))
    if len(sys.argv) > 2 and sys.argv[1] == "--out":          # somewhere else than beside this file
        ARRAYS = os.path.join(sys.argv[2], os.path.basename(ARRAYS))
        DIGESTS = os.path.join(sys.argv[2], os.path.basename(DIGESTS))
    main()
