"""Host-side proofs for tests/test_mlp_exact_gpu.py: every case the GPU file runs through the split-arithmetic MLP kernels is shown
here, without a GPU, to have ONE right float32 answer whatever the order of the kernel's sums (tests/mlp_exact_ref.py), or -- the
power-of-two sweep -- to stay inside the exponent range in which scaling by 2^e commutes with every operation."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_exact_ref as R  # noqa: E402

ARITHS = ("bf16x3", "f16x2")


def test_pieces_are_the_librarys_splits():
    """mlp_exact_ref.pieces (numpy) == models.split_bf16 / split_f16 bit for bit, over 80 binades and on integers; a float32 number
    is the exact sum of its three bfloat16 pieces anywhere in [2^-100, 2^100]."""
    from cppf2_amd import models
    rng = np.random.default_rng(0)
    v = (rng.standard_normal((64, 160)) * 2.0 ** rng.integers(-100, 100, size=(64, 160))).astype(np.float32)
    v[:, :8] = rng.integers(-70000, 70000, size=(64, 8))
    want = models.split_bf16(torch.from_numpy(v)).float().numpy()
    got = R.pieces(v, "bf16x3")
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert np.array_equal(got[0].astype(np.float64) + got[1] + got[2], v.astype(np.float64))
    small = (v * np.float32(2.0 ** -8)).astype(np.float32)
    small = small[np.abs(small) < 60000]
    want = models.split_f16(torch.from_numpy(small)).float().numpy()
    got = R.pieces(small, "f16x2")
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", [s[0] for s in R.LATTICE])
def test_lattice_case_is_exact_in_any_order(name, arith):
    """The abs-sum bound (integer pieces, exact splits, every partial sum below 2^24, nothing in the dropped products; f16x2: |x| <= 8
    and every B operand below 65504) on all 257 rows, and the float32 emulation of the kernel's product order against int64."""
    c = R.lattice_case(name, arith)
    assert c.rows == max(R.LATTICE_ROWS)
    assert float(np.abs(c.first_input()).max()) <= (8.0 if arith == "f16x2" else 1024.0)
    assert set(np.unique(c.w1)) <= {-1.0, 0.0, 1.0}
    if c.form != "linear":
        per_row = 1 if len(c.chain) >= 15 else 4
        for w in [c.w2] + [m for p in c.chain for m in p]:
            assert set(np.unique(w)) <= {-1.0, 0.0, 1.0} and int((w != 0).sum(1).max()) <= per_row
    bound = R.prove_lattice(c, arith)
    assert bound < R.EXACT
    out, _ = R.reference(c, np.int64)
    assert np.abs(out).max() > 0 and len(np.unique(out)) > 16             # not a degenerate case


@pytest.mark.parametrize("variant", R.UNIT_VARIANTS)
@pytest.mark.parametrize("dense", R.UNIT_DENSE)
@pytest.mark.parametrize("k,n", R.UNIT_SHAPES)
def test_unit_row_case_is_exact_in_every_order_of_its_piece_products(k, n, dense, variant):
    c = R.unit_case(k, n, dense, variant)
    ok, out, _ = R.prove_unit(c)
    assert ok.all()
    want, _ = R.reference(c, np.float64)
    assert np.array_equal(out.astype(np.float64), want)                      # the float64 value IS a float32 number
    src = {"w1": c.w1, "w0": c.w0, "w2": c.w2}.get(dense)
    if src is None:
        src = c.chain[-1][0 if dense == "chain_w1" else 1]
    # the dense matrix carries what the variant says: 24 significant bits in most entries, or 12 in all
    frac = np.frexp(src[src != 0].astype(np.float64))[0] * 2.0 ** 24
    if variant == "full":
        assert (frac % 2 == 1).mean() > 0.4 and (frac % 256 != 0).mean() > 0.98
    else:
        assert (frac % 2 ** 12 == 0).all() and (frac % 2 ** 13 != 0).mean() > 0.4
    assert (want != 0).mean() > 0.4
    if variant == "mid":
        # ... and the result depends on the mid x mid product: without it a representable bit changes
        kept = R.KEPT["bf16x3"]
        try:
            R.KEPT["bf16x3"] = [p for p in kept if p != (1, 1)]
            ok2, _, _ = R.prove_unit(c)
        finally:
            R.KEPT["bf16x3"] = kept
        assert (~ok2).mean() > 0.2


@pytest.mark.parametrize("k,n", R.UNIT_SHAPES)
def test_unit_row_case_with_full_precision_activations_is_exact_in_every_order(k, n):
    """The activations' three pieces in the first product (the lattice's |x| <= 2^10 and the other unit rows need at most two)."""
    c = R.unit_x_case(k, n)
    ok, out, _ = R.prove_unit(c)
    assert ok.all()
    want, _ = R.reference(c, np.float64)
    assert np.array_equal(out.astype(np.float64), want)
    s = np.diag(c.x)
    assert all((p != 0).mean() >= 0.75 for p in R.pieces(s, "bf16x3"))                # three live pieces in (nearly) every row
    assert ((want != 0).sum(1) == 2).all()


@pytest.mark.parametrize("name", [s[0] for s in R.HOMOGENEITY])
def test_homogeneity_sweep_stays_inside_the_safe_exponent_range(name):
    """Inputs, weights and biases are multiples of 2^-12 with no nonzero magnitude below it; the emulation gives the smallest and
    the largest term of the unscaled launch, and the sweep keeps the e of (-64, -32, -8, 8, 32, 64) at which 2^e times both stays
    inside [2^-100, 2^100] -- 26 binades from the float32 normal range at either end."""
    c = R.homogeneity_case(name)
    for a in [c.x, c.w1, c.b1, c.w0, c.b0, c.w2, c.table, c.points, c.wtab] + [m for p in c.chain for m in p]:
        if a is not None:
            q = a.astype(np.float64) * 4096.0
            assert np.array_equal(q, np.rint(q)) and np.abs(q).min() >= 1.0
    lo, hi = R.homogeneity_range(name)
    es = R.homogeneity_exponents(lo, hi)
    assert 2.0 ** -60 < lo and hi < 2.0 ** 8, (lo, hi)
    assert len(es) >= 5 and -32 in es and 64 in es, es
    for e in es:
        assert lo * 2.0 ** e >= 2.0 ** -100 and hi * 2.0 ** e <= 2.0 ** 100
