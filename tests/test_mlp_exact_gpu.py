"""The split-arithmetic MLP kernels (cppf_mlp_split.hip) against answers that are exact float32 numbers whatever the order of the
sums, and against themselves under power-of-two scaling.  tests/mlp_exact_ref.py builds the cases and holds the int64 / float64
references; tests/test_mlp_exact.py proves on the host that each case is what it claims to be.  What the tolerance tests of
tests/test_mlp_split.py cannot see -- a wrong low-order piece in one feature position, an operand that loses a piece, a split that
is right only near |v| ~ 1 -- changes a bit here."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_exact_ref as R  # noqa: E402


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def run_case(c, arith, dev, e=0):
    """(out, tap or None, tables or None) of case c through the library: ops.reslayer_split / _gather / _sumgather / linear_split
    (arith "bf16x3") or their f16x2 forms, weights packed by models.pack_split / pack_linear.  e: x, the gathered tables, the table
    launch's points and the biases are multiplied by 2^e first -- on the host, by np.ldexp: torch.ldexp multiplies by pow(2, e), which the
    device evaluates one unit in the last place off for some e (32 and 80 among them)."""
    from cppf2_amd import models, ops
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    up = lambda a: None if a is None else t(np.ldexp(a, e))
    f16 = arith == "f16x2"
    n, chain = c.n, len(c.chain)
    x, b1, b0 = up(c.x), up(c.b1), up(c.b0)
    if c.form == "linear":
        if f16:
            sc = models.f16_scale(t(c.w1))
            return ops.linear_split(x, models.pack_linear(t(c.w1), x.shape[1], arith="f16x2", scale=sc), b1 * sc, n, scale=sc), None, None
        return ops.linear_split(x, models.pack_linear(t(c.w1), x.shape[1]), b1, n), None, None
    k = c.first_input().shape[1]
    pairs = [(t(a), t(b)) for a, b in c.chain]
    sc = models.f16_scale(t(c.w1), t(c.w0), t(c.w2), *[w for p in pairs for w in p]) if f16 else None
    wq = models.pack_split(t(c.w1), t(c.w0), t(c.w2), k, chain=pairs, **(dict(arith="f16x2", scale=sc) if f16 else {}))
    if f16:
        b1, b0 = b1 * sc, None if b0 is None else b0 * sc
    tap = torch.full((c.rows, n), float("nan"), device=dev) if c.tap else None
    if c.form == "gather":
        gidx, table = t(c.gidx), up(c.table)
        if f16:
            return ops.reslayer_split16(x, wq, b1, b0, n, sc, chain=chain, gather=(gidx, table)), None, None
        return ops.reslayer_split_gather(x, gidx, table, wq, b1, b0, n, chain=chain), None, None
    if c.form == "sumgather":
        slots = c.gidx.shape[1]
        if f16:
            sct = models.f16_scale(t(c.wtab))
            tables = ops.linear_split(up(c.points), models.pack_linear(t(c.wtab), c.points.shape[1], arith="f16x2", scale=sct), None,
                                      slots * 256, scale=sct)
        else:
            tables = ops.linear_split(up(c.points), models.pack_linear(t(c.wtab), c.points.shape[1]), None, slots * 256)
        return ops.reslayer_split_sumgather(x, t(c.gidx), tables, wq, b1, b0, n, chain=chain, scale=sc), None, tables
    if f16:
        return ops.reslayer_split16(x.clone(), wq, b1, b0, n, sc, chain=chain, tap=tap), tap, None
    return ops.reslayer_split(x.clone(), wq, b1, b0, n, chain=chain, tap=tap), tap, None


def _mismatch(got, want):
    bad = (got != want).nonzero()
    return "%d of %d elements differ, first at %s: got %r, want %r" % (
        bad.shape[0], want.numel(), bad[0].tolist(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item())


@pytest.mark.parametrize("arith", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("name", [s[0] for s in R.LATTICE])
def test_integer_lattice_is_bit_exact_against_int64(name, arith):
    """1. Integer inputs, dense W1 / W0 in {-1, 0, 1}, sparse signed-one W2 and chained matrices, integer biases: every partial sum
    of every piece product is an integer below 2^24 (test_mlp_exact.py), so the kernel must return the int64 result itself, at 1,
    33 and 257 rows, in both arithmetics -- identity, projection, chains of 1, 4 and 15, the tap's two outputs, the gathered rows,
    the table-fed first layer with tables the library wrote, and the plain Linear."""
    dev = _dev()
    full = R.lattice_case(name, arith)
    want, want_tap = (torch.from_numpy(a.astype(np.float32)).to(dev) if a is not None else None for a in R.reference(full, np.int64))
    for rows in R.LATTICE_ROWS:
        c = full.head_rows(rows)
        got, tap, tables = run_case(c, arith, dev)
        assert got.shape == (rows, want.shape[1])
        assert torch.equal(got, want[:rows]), (c.name, arith, _mismatch(got, want[:rows]))
        if c.tap:
            assert torch.equal(tap, want_tap[:rows]), (c.name, arith, "tap", _mismatch(tap, want_tap[:rows]))
        if tables is not None:
            wt = torch.from_numpy(c.tables(np.int64).astype(np.float32)).to(dev).reshape(tables.shape)
            assert torch.equal(tables, wt), (c.name, arith, "tables", _mismatch(tables, wt))


@pytest.mark.parametrize("variant", R.UNIT_VARIANTS)
@pytest.mark.parametrize("dense", R.UNIT_DENSE)
@pytest.mark.parametrize("k,n", R.UNIT_SHAPES)
def test_unit_rows_return_the_weights_own_pieces(k, n, dense, variant):
    """2. Row r = s_r e_r against ONE dense random float32 matrix of the launch (W1, W0, W2, a chained W1, a chained W2), the others
    monomial or zero: each output is one entry of that matrix times a power of two, through ReLU -- exact whichever of its (at most
    six) piece products the kernel adds first (every order is evaluated in test_mlp_exact.py).  "mid": s_r = (1 + 2^-9) 2^a and
    12-bit weights, where the value needs the mid x mid product."""
    dev = _dev()
    c = R.unit_case(k, n, dense, variant)
    want = torch.from_numpy(R.reference(c, np.float64)[0].astype(np.float32)).to(dev)
    got, _, _ = run_case(c, "bf16x3", dev)
    assert torch.equal(got, want), (c.name, _mismatch(got, want))


@pytest.mark.parametrize("k,n", R.UNIT_SHAPES)
def test_unit_rows_return_the_activations_own_pieces(k, n):
    """2, the other operand: x[r] = s_r e_r with s_r a full 24-bit float32 against monomial power-of-two matrices -- all three pieces
    of every input column in the first product, through W0 and through W1, ReLU and W2."""
    dev = _dev()
    c = R.unit_x_case(k, n)
    want = torch.from_numpy(R.reference(c, np.float64)[0].astype(np.float32)).to(dev)
    got, _, _ = run_case(c, "bf16x3", dev)
    assert torch.equal(got, want), (c.name, _mismatch(got, want))


@pytest.mark.parametrize("name", [s[0] for s in R.HOMOGENEITY])
def test_scaling_the_input_by_a_power_of_two_scales_the_output(name):
    """3. out(2^e x; W, 2^e b1, 2^e b0) == 2^e out(x; W, b1, b0) bit for bit (bf16 triples).  Why: rounding to bfloat16, the exact
    float32 remainders of the split, the exact piece products, the float32 accumulation, max(h, 0) and the residual addition all
    commute with a power-of-two factor as long as nothing leaves the normal range -- and the weights are not scaled, so every term
    of the scaled launch is 2^e times the unscaled launch's.  Inputs, weights and biases are multiples of 2^-12; the emulation in
    mlp_exact_ref gives the unscaled launch's smallest piece product (2^-24 for the Linear, 2^-36 .. 2^-41 behind a second and a
    tenth product) and largest value (below 2^5); of e = -64, -32, -8, 8, 32, 64 those are kept that leave both inside
    [2^-100, 2^100] (test_mlp_exact.py asserts the list).  A split that is inexact in some exponent range, an absolute threshold or a
    flush inside the range breaks the equality; no reference is involved."""
    dev = _dev()
    c = R.homogeneity_case(name)
    es = R.homogeneity_exponents(*R.homogeneity_range(name))
    assert len(es) >= 5
    base, base_tap, base_tab = run_case(c, "bf16x3", dev)
    assert torch.isfinite(base).all() and float(base.abs().max()) > 0.5
    scaled = lambda a, e: torch.from_numpy(np.ldexp(a.cpu().numpy(), e)).to(dev)
    for e in es:
        got, tap, tab = run_case(c, "bf16x3", dev, e=e)
        assert torch.equal(got, scaled(base, e)), (name, e, _mismatch(got, scaled(base, e)))
        if c.tap:
            assert torch.equal(tap, scaled(base_tap, e)), (name, e, "tap")
        if tab is not None:
            assert torch.equal(tab, scaled(base_tab, e)), (name, e, "tables")


@pytest.mark.parametrize("name", ["chain4", "plain", "gather"])
def test_infinite_inputs_turn_their_rows_into_nan_and_no_other(name):
    """4. The header's non-finite rules (bf16 triples): +Inf, -Inf and 3.4e38 -- above the largest bfloat16, it rounds to Inf -- in
    one row each: an infinite operand splits into Inf + NaN, so those rows come out all NaN (dense weights); every other row keeps
    the clean run's bits."""
    dev = _dev()
    c = R.homogeneity_case(name)
    clean, _, _ = run_case(c, "bf16x3", dev)
    x = c.x.copy()
    hit = {3: np.inf, 40: -np.inf, 100: 3.4e38}
    for r, v in hit.items():
        x[r, (7 * r) % x.shape[1]] = v
    x[200, x.shape[1] - 1] = np.inf                        # the last column of the last ragged K step
    d = c.head_rows(c.rows)
    d.x = x
    got, _, _ = run_case(d, "bf16x3", dev)
    rows = sorted(list(hit) + [200])
    others = [r for r in range(c.rows) if r not in rows]
    assert torch.isnan(got[rows]).all()
    assert torch.equal(got[others], clean[others])


def f16x2_scale_sweep(dev, shape):
    """{e: (e16, e_library)}: max error against float64 over the largest |output|, for x = 2^e randn [257, k] through the f16x2
    kernel and through the library's float32 GEMMs, weights and biases as in test_reslayer_split16_matches_float64_like_a_float32_gemm."""
    from cppf2_amd import models, ops
    k, n, proj, chain = shape
    w1, b1, w0, b0, w2 = (None if a is None else a.to(dev) for a in R.gaussian_layer(torch, k, n, proj, seed=k * 7 + n))
    rest = [[None if a is None else a.to(dev) for a in R.gaussian_layer(torch, n, n, False, seed=20 + l)] for l in range(chain)]
    pairs = [(r[0], r[4]) for r in rest]
    sc = models.f16_scale(w1, w0, w2, *[w for p in pairs for w in p])
    wq = models.pack_split(w1, w0, w2, k, chain=pairs, arith="f16x2", scale=sc)
    bias = torch.cat([b1] + [r[1] for r in rest])
    x0 = torch.randn(R.SWEEP_ROWS, k, generator=torch.Generator().manual_seed(R.SWEEP_ROWS))

    def layer64(x, w1, b1, w0, b0, w2):
        h = torch.relu(x @ w1.double().t() + b1.double())
        return (x if w0 is None else x @ w0.double().t() + b0.double()) + h @ w2.double().t()
    res = {}
    for e in R.SWEEP_E:
        x = torch.from_numpy(np.ldexp(x0.numpy(), e)).to(dev)
        want = layer64(x.double(), w1, b1, w0, b0, w2)
        nat = torch.addmm(x if w0 is None else torch.addmm(b0, x, w0.t()), torch._addmm_activation(b1, x, w1.t()), w2.t())
        for r in rest:
            want = layer64(want, r[0], r[1], None, None, r[4])
            nat = torch.addmm(nat, torch._addmm_activation(r[1], nat, r[0].t()), r[4].t())
        got = ops.reslayer_split16(x.clone(), wq, bias * sc, None if b0 is None else b0 * sc, n, sc, chain=chain)
        scale = want.abs().max().item()
        res[e] = ((got.double() - want).abs().max().item() / scale, (nat.double() - want).abs().max().item() / scale,
                  bool(torch.isfinite(got).all()))
    return res


# the smallest e of the sweep at which BOTH shapes met the bound in the recorded run (docs/measurements.md 13.1)
SWEEP_E_MIN = -16


def test_f16x2_holds_its_bound_down_to_the_measured_input_scale():
    """5. The lower edge of the f16x2 activation range: x = 2^e randn, e = 4, 2, ..., -16, on (360 -> 128 projection, chain 4) and
    (256 identity, chain 1) at 257 rows.  The error table of the recorded run is in docs/measurements.md 13.1; the bound of
    tests/test_mlp_split.py (e16 < 3e-6 and e16 < 3 e_library + 2e-7) is asserted for e >= e_min + 2, two steps (a factor of 4 in
    the regime where the error grows as 2^-e) above the smallest e at which both shapes met it there; below that only that the
    result is finite."""
    dev = _dev()
    for shape in R.SWEEP_SHAPES:
        res = f16x2_scale_sweep(dev, shape)
        print("f16x2 scale sweep", shape)
        for e in R.SWEEP_E:
            e16, e_lib, finite = res[e]
            print("  e = %3d   e16 = %.3e   e_library = %.3e   bound %s" % (e, e16, e_lib, "met" if e16 < 3e-6 and e16 < 3.0 * e_lib + 2e-7 else "MISSED"))
        for e in R.SWEEP_E:
            e16, e_lib, finite = res[e]
            assert finite, (shape, e)
            if e >= SWEEP_E_MIN + 2:
                assert e16 < 3e-6 and e16 < 3.0 * e_lib + 2e-7, (shape, e, e16, e_lib)
