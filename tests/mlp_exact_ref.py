"""Cases for the split-arithmetic MLP kernels (cppf_mlp_split.hip) whose right answer is an exact float32 number that does not depend
on the order of the sums, with their references and the host-side proofs that they are what they claim to be.

Nothing here restates the kernel.  The references are plain int64 / float64 evaluations of
    y = skip(x) + relu(x W1^T + b1) W2^T,  skip = x or x W0^T + b0,  then  y <- y + relu(y W1_l^T + b1_l) W2_l^T  per chained layer
and of y = x W^T + b (linear).  The proofs are about the operand pieces (hi, mid, lo as models.split_bf16 / split_f16 define them):
  * prove_lattice: the abs-sum bound (every partial sum of every piece product, in any order, is an integer below 2^24) and an
    emulation, term by term in float32, of the product order the kernel documents (a.l b.h, a.h b.l, a.m b.m, a.m b.h, a.h b.m,
    a.h b.h per K step of 16; the f16x2 arithmetic: a.l b.h, a.h b.l, a.h b.h);
  * prove_unit: every accumulator element of a unit-row case receives at most one nonzero contraction term; every order of its
    (at most six) piece products is summed in float32 and must give the float64 value;
  * term_range: the emulation's smallest and largest piece product and accumulator, for the power-of-two scale sweep.
Families: lattice_cases (1), unit_cases (2), homogeneity_cases (3), and the f16x2 scale sweep's layers (5)."""
import functools
import itertools

import numpy as np

F32 = np.float32
EXACT = float(2 ** 24)               # integers below it are float32 numbers, and so is every sum of them that stays below it


# ---------------------------------------------------------------------------------------------------------------------------
# operand pieces (numpy; tests/test_mlp_exact.py checks them against models.split_bf16 / split_f16 bit for bit)
def bf16_round(v):
    """float32 -> the nearest bfloat16 (ties to even), as float32.  Finite input."""
    u = np.ascontiguousarray(v, dtype=F32).view(np.uint32)
    r = (u + (((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    return r.view(F32)


def pieces(v, arith):
    """The operand pieces of float32 v: [hi, mid, lo] bfloat16 (arith "bf16x3") or [hi, lo] float16 ("f16x2"), as float32 arrays."""
    v = np.ascontiguousarray(v, dtype=F32)
    if arith == "f16x2":
        with np.errstate(over="ignore"):
            hi = v.astype(np.float16).astype(F32)
            lo = (v - hi).astype(np.float16).astype(F32)
        return [hi, lo]
    hi = bf16_round(v)
    r = v - hi
    mid = bf16_round(r)
    return [hi, mid, bf16_round(r - mid)]


# (a piece, b piece) of the products the kernel keeps, in the order rs_mma issues them; DROPPED: the ones it leaves out
KEPT = {"bf16x3": [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)], "f16x2": [(1, 0), (0, 1), (0, 0)]}
DROPPED = {"bf16x3": [(1, 2), (2, 1), (2, 2)], "f16x2": [(1, 1)]}


def h_order(n):
    """The K order of a product whose B operand is accumulator tiles (second products, chained layers): step (t, s') contracts over
    features 32 t + 16 s' + 4 g + (j & 3) + 8 (j >> 2), g = 0, 1, j = 0 .. 7 (models.pack_split)."""
    out = []
    for t in range(n // 32):
        for sp in range(2):
            for g in range(2):
                for j in range(8):
                    out.append(32 * t + 16 * sp + 4 * g + (j & 3) + 8 * (j >> 2))
    return np.array(out)


# ---------------------------------------------------------------------------------------------------------------------------
class Case:
    """One launch: form "plain" | "gather" | "sumgather" | "linear"; float32 numpy arrays as nn.Linear stores them.
    plain: x [rows, k].  gather: x = heads [rows, head], gidx [rows, slots], table [points, fdim] (k = head + slots fdim).
    sumgather: x = heads [rows, k], gidx, points [npts, dp], wtab [slots * 256, dp] (the tables are points wtab^T, written by
    linear_split).  linear: out = x w1^T + b1, n a multiple of 256."""

    def __init__(self, name, form, x, w1, b1, w0=None, b0=None, w2=None, chain=(), tap=False, gidx=None, table=None, points=None,
                 wtab=None):
        self.name, self.form, self.tap = name, form, tap
        f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=F32)
        self.x, self.w1, self.b1, self.w0, self.b0, self.w2 = f(x), f(w1), f(b1), f(w0), f(b0), f(w2)
        self.chain = [(f(a), f(b)) for a, b in chain]
        self.gidx = None if gidx is None else np.ascontiguousarray(gidx, dtype=np.int32)
        self.table, self.points, self.wtab = f(table), f(points), f(wtab)
        self.n = self.w1.shape[0]
        self.rows = self.x.shape[0]

    def head_rows(self, rows):
        """The same case on its first `rows` rows (rows are independent)."""
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.x, c.rows = self.x[:rows], rows
        c.gidx = None if self.gidx is None else self.gidx[:rows]
        c.name = "%s rows%d" % (self.name, rows)
        return c

    def first_input(self):
        """The rows the first product contracts over: x, or (gather) [heads | table[gidx[:, 0]] | ...]."""
        if self.form != "gather":
            return self.x
        return np.concatenate([self.x] + [self.table[self.gidx[:, i]] for i in range(self.gidx.shape[1])], axis=1)

    def tables(self, dtype):
        """sumgather: the per-point slot tables [points, slots, 256] = points wtab^T in `dtype`."""
        t = self.points.astype(dtype) @ self.wtab.astype(dtype).T
        return t.reshape(self.points.shape[0], -1, 256)


def reference(case, dtype):
    """(out, tap or None) of the launch in `dtype` (np.int64 for integer cases, np.float64): the formula, nothing else."""
    x = case.first_input().astype(dtype)
    w1, b1 = case.w1.astype(dtype), case.b1.astype(dtype)
    n = case.n
    if case.form == "linear":
        return x @ w1.T + b1, None
    pre = x @ w1.T + b1[:n]
    skip = x if case.w0 is None else x @ case.w0.astype(dtype).T + case.b0.astype(dtype)
    if case.form == "sumgather":
        t = case.tables(dtype)
        for i in range(case.gidx.shape[1]):
            pre = pre + t[case.gidx[:, i], i, :n]
            skip = skip + t[case.gidx[:, i], i, n:]
    y = skip + np.maximum(pre, 0) @ case.w2.astype(dtype).T
    tap = y.copy() if case.tap else None
    for l, (a, b) in enumerate(case.chain):
        y = y + np.maximum(y @ a.astype(dtype).T + b1[(1 + l) * n:(2 + l) * n], 0) @ b.astype(dtype).T
    return y, tap


# ---------------------------------------------------------------------------------------------------------------------------
# the products of a launch, one after the other: what the bound, the emulation and the order check all walk
def _walk(case, product, sc=F32(1), bs=F32(1)):
    """Evaluates the launch through `product(acc0, A, B, korder) -> acc` (A [n, K] weights, B [rows, K] activations, float32; acc0
    the initial accumulators [rows, n]; korder the order the K steps take the features in).  sc, bs: the f16x2 kernels' power-of-two
    weight scale and its inverse -- biases, table sums and the residual enter the accumulators times sc, the B operands of the
    later products and the outputs leave them times bs (both 1 for the bf16 triples).  Returns (out, tap)."""
    x = case.first_input()
    rows, k = x.shape
    n = case.n
    nat = np.arange(k)
    relu = lambda v: np.maximum(v, F32(0))
    bc = lambda b, w: np.broadcast_to(b.astype(F32) * sc, (rows, w)).copy()
    if case.form == "linear":
        return product(bc(case.b1, n), case.w1, x, nat) * bs, None
    init = bc(case.b1[:n], n) if case.w0 is None else np.concatenate([bc(case.b1[:n], n), bc(case.b0, n)], axis=1)
    if case.form == "sumgather":                 # + the slot tables, in slot order (float32 additions)
        t = case.tables(np.float64).astype(F32)
        for i in range(case.gidx.shape[1]):
            init = init + t[case.gidx[:, i], i, :] * sc
    a0 = case.w1 if case.w0 is None else np.concatenate([case.w1, case.w0])
    first = product(init, a0, x, nat)
    h = relu(first[:, :n])
    skip = x.astype(F32) * sc if case.w0 is None else first[:, n:]
    ho = h_order(n)
    y = product(skip, case.w2, h * bs, ho)
    tap = y * bs if case.tap else None
    for l, (a, b) in enumerate(case.chain):
        h = relu(product(bc(case.b1[(1 + l) * n:(2 + l) * n], n), a, y * bs, ho))
        y = product(y, b, h * bs, ho)
    return y * bs, tap


class Stats:
    """Magnitudes met while a launch is evaluated piece by piece."""

    def __init__(self):
        self.bound = 0.0                 # largest abs-sum bound of an accumulator element
        self.integers = True             # every operand piece and initial accumulator is an integer
        self.exact_split = True          # every operand is the exact sum of its pieces
        self.dropped = 0.0               # largest abs-sum of the products the kernel leaves out
        self.min_term = np.inf           # emulation: smallest nonzero |piece product|, largest, largest |accumulator|
        self.max_term = 0.0
        self.max_acc = 0.0
        self.max_b = 0.0                 # largest |B operand| (activations; f16x2: must stay below 65504)


def abs_sum_bound(case, arith, dtype=np.int64):
    """Stats of the launch with every intermediate taken from the exact reference in `dtype`: for each product, max over the
    accumulator elements of  |initial accumulator| + sum_k (sum |pieces of a|)(sum |pieces of b|)  -- an upper bound of every partial
    sum of the kept products in ANY order --, whether all pieces are integers, whether the splits are exact, and the abs-sum of
    the dropped products.  (f16x2: the kernel's accumulators carry the weights' power-of-two scale, which changes none of this.)"""
    st = Stats()
    is_int = lambda v: bool(np.all(v == np.rint(v)))

    def product(acc0, a, b, korder):
        ap, bp = pieces(a, arith), pieces(b, arith)
        for p, v in ((ap, a), (bp, b)):
            s = p[0].astype(np.float64)
            for q in p[1:]:
                s = s + q
            st.exact_split &= bool(np.array_equal(s, v.astype(np.float64)))
            st.integers &= all(is_int(q) for q in p)
        st.integers &= is_int(acc0)
        sa = sum(np.abs(q).astype(np.float64) for q in ap)
        sb = sum(np.abs(q).astype(np.float64) for q in bp)
        st.bound = max(st.bound, float((np.abs(acc0).astype(np.float64) + sb @ sa.T).max()))
        st.max_b = max(st.max_b, float(np.abs(b).max()))
        for i, j in DROPPED[arith]:
            st.dropped = max(st.dropped, float((np.abs(bp[j]).astype(np.float64) @ np.abs(ap[i]).astype(np.float64).T).max()))
        exact = acc0.astype(np.float64) + b.astype(np.float64) @ a.astype(np.float64).T
        if dtype == np.int64:                    # the next operand is the exact value: it must be a float32 number
            st.exact_split &= bool(np.abs(exact).max() < EXACT)
        return exact.astype(F32)

    if case.form == "sumgather":                 # the table launch (linear_split) and the slot sums
        lin = Case(case.name + " tables", "linear", case.points, case.wtab, np.zeros(case.wtab.shape[0], F32))
        s2 = abs_sum_bound(lin, arith, dtype)
        st.bound, st.integers, st.exact_split, st.dropped = s2.bound, s2.integers, s2.exact_split, s2.dropped
        t = np.abs(case.tables(np.float64))
        tot = sum(t[case.gidx[:, i], i, :] for i in range(case.gidx.shape[1]))
        st.bound = max(st.bound, float(tot.max() + max(np.abs(case.b1).max(), np.abs(case.b0).max())))
    _walk(case, product)
    return st


def emulate(case, arith, scale=1.0):
    """The launch evaluated term by term in float32 in the order the kernel documents: per K step of 16 features the kept products
    one after the other, each contracting its 16 terms in sequence into the float32 accumulator.  (The matrix core's own order
    inside one instruction is not documented; the cases that use this are proved order-free by abs_sum_bound, and the emulation
    shows the kept products suffice and gives the magnitudes.)  f16x2: `scale` = the weights' power of two; the accumulators carry it
    and the B operands / outputs are multiplied by 1 / scale, as in the kernel.  Returns (out, tap, Stats)."""
    st = Stats()
    sc, bs = F32(scale), F32(1.0 / scale)

    def product(acc0, a, b, korder):
        ap, bp = pieces(a * sc, arith), pieces(b, arith)
        acc = acc0.astype(F32).copy()
        kk = a.shape[1]
        for s in range(0, kk, 16):
            ks = korder[s:s + 16]
            for i, j in KEPT[arith]:
                for k in ks:
                    av, bv = ap[i][:, k], bp[j][:, k]
                    na, nb = np.abs(av[av != 0]), np.abs(bv[bv != 0])
                    if na.size == 0 or nb.size == 0:
                        continue
                    st.min_term = min(st.min_term, float(na.min()) * float(nb.min()))
                    st.max_term = max(st.max_term, float(na.max()) * float(nb.max()))
                    acc += bv[:, None] * av[None, :]
            st.max_acc = max(st.max_acc, float(np.abs(acc).max()))
        return acc

    out, tap = _walk(case, product, sc, bs)
    return out, tap, st


def prove_lattice(case, arith, emulate_rows=None):
    """Asserts that `case` has one right answer in float32 whatever the order of the sums: integer pieces, exact splits, abs-sum
    bound below 2^24, nothing in the dropped products, B operands inside fp16's range (f16x2) -- and that the emulation of the
    kernel's product order reproduces the int64 result.  Returns the bound."""
    st = abs_sum_bound(case, arith)
    assert st.integers and st.exact_split, case.name
    assert st.bound < EXACT, (case.name, st.bound)
    assert st.dropped == 0.0, (case.name, st.dropped)
    if arith == "f16x2":
        assert st.max_b < 65504.0 and float(np.abs(case.first_input()).max()) <= 8.0, (case.name, st.max_b)
    sub = case if emulate_rows is None else case.head_rows(min(emulate_rows, case.rows))
    want, want_tap = reference(sub, np.int64)
    got, got_tap, _ = emulate(sub, arith, scale=f16_scale_of(sub) if arith == "f16x2" else 1.0)
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(F32)), case.name
    if sub.tap:
        assert np.array_equal(got_tap, want_tap.astype(F32)), case.name
    return st.bound


def f16_scale_of(case):
    """models.f16_scale of the launch's weights (the largest |w| lands in [2^12, 2^13))."""
    import math
    ws = [case.w1, case.w0, case.w2] + [w for p in case.chain for w in p]
    m = max(float(np.abs(w).max()) for w in ws if w is not None)
    return 2.0 ** (13 - math.ceil(math.log2(m))) if m > 0 else 1.0


# ---------------------------------------------------------------------------------------------------------------------------
# 1. integer lattice
def _signed_sparse(rng, n_out, n_in, per_row):
    w = np.zeros((n_out, n_in), F32)
    for r in range(n_out):
        cols = rng.choice(n_in, size=per_row, replace=False)
        w[r, cols] = rng.choice([-1.0, 1.0], size=per_row)
    return w


def _lattice_build(name, form, k, n, proj, chain, xmax, density, seed, per_row, tap=False, rows=257):
    rng = np.random.default_rng(seed)
    tri = lambda *s: rng.integers(-1, 2, size=s).astype(F32)
    ints = lambda hi, *s: (rng.integers(-hi, hi + 1, size=s) * (rng.random(s) < density)).astype(F32)
    if form == "linear":
        return Case(name, form, ints(xmax, rows, k), tri(n, k), ints(64, n))
    w1, w0 = tri(n, k), (tri(n, k) if proj else None)
    w2 = _signed_sparse(rng, n, n, per_row)
    rest = [(_signed_sparse(rng, n, n, per_row), _signed_sparse(rng, n, n, per_row)) for _ in range(chain)]
    b1 = ints(16, (1 + chain) * n)
    b0 = ints(16, n) if proj else None
    kw = dict(w0=w0, b0=b0, w2=w2, chain=rest, tap=tap)
    if form == "gather":                         # 40 head columns + 5 descriptors of a 64-wide table (the SHOT tuple encoder's row)
        npts = 97
        return Case(name, form, ints(xmax, rows, 40), w1, b1, gidx=rng.integers(0, npts, size=(rows, 5)), table=ints(xmax, npts, 64), **kw)
    if form == "sumgather":                      # k head columns; 5 slots of tables = points wtab^T, points [npts, 24] integers
        npts = 61
        return Case(name, form, ints(xmax, rows, k), w1, b1, gidx=rng.integers(0, npts, size=(rows, 5)),
                    points=ints(xmax, npts, 24), wtab=tri(5 * 256, 24), **kw)
    return Case(name, form, ints(xmax, rows, k), w1, b1, **kw)


# (name, form, k, n, projection, chain, tap): every width, every first-product width, every form the issue lists.  Chains of 15
# (the documented limit) take ONE signed one per row of the sparse matrices (values at most double per layer), the others four.
LATTICE = [
    ("identity64", "plain", 64, 64, False, 0, False),
    ("identity128", "plain", 128, 128, False, 0, False),
    ("identity192", "plain", 192, 192, False, 0, False),
    ("identity256", "plain", 256, 256, False, 0, False),
    ("proj8to256", "plain", 8, 256, True, 0, False),
    ("proj72to192", "plain", 72, 192, True, 0, False),
    ("proj360to128", "plain", 360, 128, True, 0, False),
    ("proj1032to64", "plain", 1032, 64, True, 0, False),
    ("identity64chain1", "plain", 64, 64, False, 1, False),
    ("proj360to128chain4", "plain", 360, 128, True, 4, False),
    ("identity256chain4", "plain", 256, 256, False, 4, False),
    ("proj72to64chain15", "plain", 72, 64, True, 15, False),
    ("identity192chain15", "plain", 192, 192, False, 15, False),
    ("tap360to128chain4", "plain", 360, 128, True, 4, True),
    ("tap72to256chain1", "plain", 72, 256, True, 1, True),
    ("gather360to128chain4", "gather", 360, 128, True, 4, False),
    ("sumgather32to128chain1", "sumgather", 32, 128, True, 1, False),
    ("linear8to256", "linear", 8, 256, False, 0, False),
    ("linear360to512", "linear", 360, 512, False, 0, False),
    ("linear1032to256", "linear", 1032, 256, False, 0, False),
]
LATTICE_ROWS = (1, 33, 257)


@functools.lru_cache(maxsize=None)
def lattice_case(name, arith):
    """The case `name` of LATTICE for `arith` at 257 rows: |x| <= 2^10 (f16x2: 8), shrunk -- magnitude first, then the share of
    nonzero entries -- until the abs-sum bound is below 2^24 and (f16x2) every B operand below 65504."""
    spec = next(s for s in LATTICE if s[0] == name)
    _, form, k, n, proj, chain, tap = spec
    per_row = 1 if chain >= 15 else 4
    seed = 1000 + [s[0] for s in LATTICE].index(name)
    ladder = [(m, 1.0) for m in (1024, 256, 64, 16, 8, 4, 2, 1) if arith != "f16x2" or m <= 8] + [(1, 0.25), (1, 1.0 / 16), (1, 1.0 / 64)]
    for xmax, density in ladder:
        c = _lattice_build(name, form, k, n, proj, chain, xmax, density, seed, per_row, tap)
        st = abs_sum_bound(c, arith)
        if st.bound < EXACT and st.exact_split and (arith != "f16x2" or st.max_b < 65504.0):
            c.xmax, c.density = xmax, density
            return c
    raise AssertionError("no lattice case for %s / %s" % (name, arith))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. unit rows
UNIT_SHAPES = [(72, 64), (360, 128), (360, 192), (1032, 256), (8, 256)]
UNIT_DENSE = ("w1", "w0", "w2", "chain_w1", "chain_w2")
UNIT_VARIANTS = ("full", "mid")


def _round_bits(v, bits):
    """float32 rounded to `bits` significant bits (ties to even)."""
    u = np.ascontiguousarray(v, dtype=F32).view(np.uint32)
    sh = np.uint32(24 - bits)
    half = (np.uint32(1) << sh) - np.uint32(1)
    r = (u + (((u >> sh) & np.uint32(1)) + (half >> np.uint32(1)))) >> sh << sh
    return r.view(F32)


def _mono(rng, n_out, n_in, shift, positive=False):
    """Signed power-of-two monomial matrix: column c has its one nonzero, +-2^p with |p| <= 3, in row (c + shift) % n_out."""
    m = np.zeros((n_out, n_in), F32)
    c = np.arange(n_in)
    sign = np.ones(n_in) if positive else rng.choice([-1.0, 1.0], size=n_in)
    m[(c + shift) % n_out, c] = sign * 2.0 ** rng.integers(-3, 4, size=n_in)
    return m


def _unit_build(k, n, dense, variant, d):
    """The unit-row launch around the dense matrix d (see unit_case)."""
    rng = np.random.default_rng(7 * k + n)
    r = np.arange(k)
    a = (5 * r) % 17 - 8                                             # row scales 2^-8 .. 2^8
    sgn = np.where(((r % n) // 3) % 2 == 0, 1.0, -1.0)                # the sign depends on the row's hidden position only
    s = sgn * 2.0 ** a * ((1.0 + 2.0 ** -9) if variant == "mid" else 1.0)
    x = np.zeros((k, k), F32)
    x[r, r] = s
    zero = lambda *sh: np.zeros(sh, F32)
    shut = -np.ones(n, F32)                                         # a bias that keeps a ReLU closed over zero weights
    if dense == "w1":          # out[r, (j + 1) % n] = P relu(s_r d[j, r])
        return Case("", "plain", x, d, zero(n), w0=zero(n, k), b0=zero(n), w2=_mono(rng, n, n, 1))
    if dense == "w0":          # out[r, i] = s_r d[i, r]
        return Case("", "plain", x, zero(n, k), shut, w0=d, b0=zero(n), w2=_mono(rng, n, n, 1))
    if dense == "w2":          # h = |s_r| 2^p e_j, j = r % n;  out[r, i] = d[i, j] h_j
        w1 = _mono(rng, n, k, 0, positive=True) * sgn[None, :]
        return Case("", "plain", x, w1, zero(n), w0=zero(n, k), b0=zero(n), w2=d)
    # chained: the first layer hands t e_j (j = r % n) to a closed identity layer and then to the layer that holds d
    first = dict(w0=_mono(rng, n, k, 0, positive=True), b0=zero(n), w2=zero(n, n))
    closed = (zero(n, n), _mono(rng, n, n, 1))
    b1 = np.concatenate([shut, shut, zero(n)])
    if dense == "chain_w1":    # out[r] = t e_j + P relu(t d[:, j]);  d[(j - 1) % n, j] = 0 keeps element j to the residual alone
        return Case("", "plain", x, zero(n, k), b1, chain=[closed, (d, _mono(rng, n, n, 1))], **first)
    # chain_w2: h = |t| 2^p e_(j+1);  out[r] = t e_j + d[:, j + 1] h;  d[j, (j + 1) % n] = 0
    jj = np.arange(n)
    w1 = _mono(rng, n, n, 1, positive=True) * np.where((jj // 3) % 2 == 0, 1.0, -1.0)[None, :].astype(F32)
    return Case("", "plain", x, zero(n, k), b1, chain=[closed, (w1, d)], **first)


def _unit_source(k, n, dense):
    """(row, column) of the dense matrix that output element [r, i] of the case comes from."""
    r, i = np.meshgrid(np.arange(k), np.arange(n), indexing="ij")
    if dense == "w1":
        return (i - 1) % n, r
    if dense == "w0":
        return i, r
    if dense == "w2":
        return i, r % n
    if dense == "chain_w1":
        return (i - 1) % n, r % n
    return i, (r + 1) % n


def prove_unit(case, arith="bf16x3"):
    """The order check of a unit-row case.  For every product of the launch: each accumulator element has at most one nonzero
    contraction term a b (so the order of the K steps and inside a K step cannot matter); its kept piece products are summed onto
    the initial accumulator in float32 in EVERY order; each order must give the float64 value of acc0 + a b, all nine products
    included.  Returns (ok [rows, n] bool: every product feeding the element passed, out, tap)."""
    rows, n = case.rows, case.n

    def product(acc0, ok_acc, a, b, ok_b):
        nz = (b != 0).astype(np.float64) @ (a != 0).astype(np.float64).T
        assert nz.max() <= 1.0, "more than one contraction term"
        ap, bp = pieces(a, arith), pieces(b, arith)
        want = acc0.astype(np.float64) + b.astype(np.float64) @ a.astype(np.float64).T       # one term: exact in float64
        terms = []
        for i, j in KEPT[arith]:
            t = bp[j].astype(np.float64) @ ap[i].astype(np.float64).T
            if t.any():
                assert np.array_equal(t.astype(F32).astype(np.float64), t)
                terms.append(t.astype(F32))
        ok = ok_acc.copy()
        for order in itertools.permutations(range(len(terms))):
            acc = acc0.astype(F32).copy()
            for q in order:
                acc = acc + terms[q]
            ok &= acc.astype(np.float64) == want
        # ... and the element's one live term must come from a B operand element that was itself exact
        ok &= (((b != 0) & ~ok_b).astype(np.float64) @ (a != 0).astype(np.float64).T) == 0
        return want.astype(F32), ok

    x = case.first_input()
    yes = lambda w: np.ones((rows, w), bool)
    relu = lambda v: np.maximum(v, F32(0))
    bc = lambda v, w: np.broadcast_to(v.astype(F32), (rows, w)).copy()
    init = bc(case.b1[:n], n) if case.w0 is None else np.concatenate([bc(case.b1[:n], n), bc(case.b0, n)], axis=1)
    a0 = case.w1 if case.w0 is None else np.concatenate([case.w1, case.w0])
    first, ok_first = product(init, yes(init.shape[1]), a0, x, yes(x.shape[1]))
    skip, ok_skip = (x, yes(n)) if case.w0 is None else (first[:, n:], ok_first[:, n:])
    y, ok = product(skip, ok_skip, case.w2, relu(first[:, :n]), ok_first[:, :n])
    tap = y.copy() if case.tap else None
    for l, (a, b) in enumerate(case.chain):
        h, ok_h = product(bc(case.b1[(1 + l) * n:(2 + l) * n], n), yes(n), a, y, ok)
        y, ok = product(y, ok, b, relu(h), ok_h)
    return ok, y, tap


@functools.lru_cache(maxsize=None)
def unit_case(k, n, dense, variant):
    """Rows = k unit rows x[r] = s_r e_r, s_r = +-2^a ("mid": (1 + 2^-9) 2^a, two operand pieces); ONE matrix of the launch --
    `dense`: w1, w0, w2, or W1 / W2 of the last of two chained layers -- is dense random float32 with full 24-bit significands
    ("mid": rounded to 12 bits, so that w s needs the mid x mid product and is still a float32 number); the others are signed
    power-of-two monomial matrices or zero, the biases zero or -1 where a ReLU must stay closed: every output element is one column
    entry of the dense matrix times a power of two, through ReLU, or the residual's one entry.  Entries for which some order of
    the piece products is inexact in float32 (a carry past 24 bits) are drawn again until prove_unit passes everywhere."""
    rng = np.random.default_rng(100 * k + n + 17 * UNIT_DENSE.index(dense) + (5 if variant == "mid" else 0))
    cols = k if dense in ("w1", "w0") else n

    def draw(*shape):
        d = (rng.standard_normal(shape) / np.sqrt(cols)).astype(F32)
        d[d == 0] = F32(0.5)
        return _round_bits(d, 12) if variant == "mid" else d

    def masked(d):
        j = np.arange(n)
        if dense == "chain_w1":
            d[(j - 1) % n, j] = 0
        if dense == "chain_w2":
            d[j, (j + 1) % n] = 0
        return d
    d = masked(draw(n, cols))
    si, sj = _unit_source(k, n, dense)
    for _ in range(40):
        c = _unit_build(k, n, dense, variant, d)
        c.name = "unit %dto%d %s %s" % (k, n, dense, variant)
        ok, _, _ = prove_unit(c)
        if ok.all():
            return c
        bad = ~ok
        d[si[bad], sj[bad]] = draw(int(bad.sum()))
        d = masked(d)
    raise AssertionError("unit case %d %d %s %s did not settle" % (k, n, dense, variant))


@functools.lru_cache(maxsize=None)
def unit_x_case(k, n):
    """The activations' own pieces in the first product: x[r] = s_r e_r with s_r a random float32 of full 24-bit significand (three
    operand pieces) against monomial power-of-two W1 (sign-matched, so the ReLU is open), W0 and W2: out[r] holds s_r 2^p' through
    W0 at position (r + 2) % n and s_r 2^p 2^p'' through W1, ReLU and W2 at (r % n + 1) % n.  Rows whose s_r fails prove_unit in
    some order are drawn again."""
    rng = np.random.default_rng(9000 + 10 * k + n)
    r = np.arange(k)
    s = (rng.standard_normal(k) * 2.0 ** ((5 * r) % 17 - 8)).astype(F32)
    w0, w2 = _mono(rng, n, k, 2), _mono(rng, n, n, 1)
    w1p = _mono(rng, n, k, 0, positive=True)
    for _ in range(40):
        x = np.zeros((k, k), F32)
        x[r, r] = s
        c = Case("unit %dto%d x full" % (k, n), "plain", x, w1p * np.sign(s)[None, :], np.zeros(n, F32), w0=w0, b0=np.zeros(n, F32), w2=w2)
        ok, _, _ = prove_unit(c)
        bad = ~ok.all(axis=1)
        if not bad.any():
            return c
        s[bad] = (rng.standard_normal(int(bad.sum())) * 2.0 ** ((5 * r[bad]) % 17 - 8)).astype(F32)
    raise AssertionError("unit x case %d %d did not settle" % (k, n))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. power-of-two homogeneity
HOMOGENEITY = [
    ("plain", "plain", 256, 256, False, 0, False),
    ("projection", "plain", 72, 192, True, 0, False),
    ("chain4", "plain", 360, 128, True, 4, False),
    ("tap", "plain", 72, 64, True, 1, True),
    ("gather", "gather", 360, 128, True, 4, False),
    ("linear", "linear", 1032, 256, False, 0, False),
    ("sumgather", "sumgather", 32, 128, True, 1, False),
]
HOMOGENEITY_START = (-64, -32, -8, 8, 32, 64)
TERM_LO, TERM_HI = 2.0 ** -100, 2.0 ** 100


def _snap(v):
    """Multiples of 2^-12, no nonzero magnitude below 2^-12 (what rounds to zero is moved to +-2^-12)."""
    q = np.rint(np.asarray(v, np.float64) * 4096.0)
    q[q == 0] = 1.0
    return (q / 4096.0).astype(F32)


@functools.lru_cache(maxsize=None)
def homogeneity_case(name, rows=257):
    """Dense Gaussian weights (1 / sqrt(fan-in)), inputs and biases, all snapped to multiples of 2^-12."""
    spec = next(s for s in HOMOGENEITY if s[0] == name)
    _, form, k, n, proj, chain, tap = spec
    rng = np.random.default_rng(500 + [s[0] for s in HOMOGENEITY].index(name))
    w = lambda o, i: _snap(rng.standard_normal((o, i)) / np.sqrt(i))
    v = lambda *s: _snap(rng.standard_normal(s))
    if form == "linear":
        return Case(name, form, v(rows, k), w(n, k), _snap(rng.standard_normal(n) * 0.125))
    kw = dict(w0=w(n, k) if proj else None, b0=_snap(rng.standard_normal(n) * 0.125) if proj else None, w2=w(n, n),
              chain=[(w(n, n), w(n, n)) for _ in range(chain)], tap=tap)
    b1 = _snap(rng.standard_normal((1 + chain) * n) * 0.125)
    if form == "gather":
        return Case(name, form, v(rows, 40), w(n, k), b1, gidx=rng.integers(0, 97, size=(rows, 5)), table=v(97, 64), **kw)
    if form == "sumgather":
        return Case(name, form, v(rows, k), w(n, k), b1, gidx=rng.integers(0, 61, size=(rows, 5)), points=v(61, 24),
                    wtab=w(5 * 256, 24), **kw)
    return Case(name, form, v(rows, k), w(n, k), b1, **kw)


def term_range(case, arith="bf16x3", rows=None):
    """(smallest nonzero |piece product|, largest |piece product| or |accumulator|) of the emulated launch, table launch included."""
    sub = case if rows is None else case.head_rows(min(rows, case.rows))
    _, _, st = emulate(sub, arith)
    lo, hi = st.min_term, max(st.max_term, st.max_acc)
    if case.form == "sumgather":
        lin = Case(case.name + " tables", "linear", case.points, case.wtab, np.zeros(case.wtab.shape[0], F32))
        _, _, s2 = emulate(lin, arith)
        lo, hi = min(lo, s2.min_term), max(hi, s2.max_term, s2.max_acc)
    return lo, hi


def homogeneity_exponents(lo, hi):
    """The e of HOMOGENEITY_START at which every term of the launch on 2^e x stays inside [2^-100, 2^100]: every term of that launch
    is 2^e times the unscaled launch's (weights are not scaled; x, the biases and hence every activation are)."""
    return tuple(e for e in HOMOGENEITY_START if lo * 2.0 ** e >= TERM_LO and hi * 2.0 ** e <= TERM_HI)


@functools.lru_cache(maxsize=None)
def homogeneity_range(name):
    """term_range of the homogeneity case `name` (under a second per form: both test files evaluate it)."""
    return term_range(homogeneity_case(name))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the f16x2 scale sweep: the layers of test_reslayer_split16_matches_float64_like_a_float32_gemm (tests/test_mlp_split.py: _layer)
SWEEP_SHAPES = [(360, 128, True, 4), (256, 256, False, 1)]
SWEEP_E = tuple(range(4, -17, -2))
SWEEP_ROWS = 257


def gaussian_layer(torch, k, n, proj, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    w1 = torch.randn(n, k, generator=g) / k ** 0.5
    w2 = torch.randn(n, n, generator=g) / n ** 0.5
    w0 = torch.randn(n, k, generator=g) / k ** 0.5 if proj else None
    b1 = torch.randn(n, generator=g) * 0.1
    b0 = torch.randn(n, generator=g) * 0.1 if proj else None
    return w1, b1, w0, b0, w2
