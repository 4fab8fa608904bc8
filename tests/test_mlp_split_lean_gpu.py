"""The split-arithmetic ResLayer kernels (cppf_mlp_split.hip) against the outputs of the build before their vector work was trimmed
(one-instruction ReLU, scalar weight-piece addresses; docs/measurements.md 13): BYTE equality with the fixture that
tests/golden/mlp_split/make_golden_mlp_split.py wrote on that earlier build -- arrays for the cases of at most 33 rows, SHA-256 digests for
all.  The cases sit at the kernels' edges (rows 1, 31, 32, 33, 255, 256, 257 and 901 on a forced grid of two workgroups, where the
dynamic row-block counters are used and must read zero afterwards) and cover every launch form; see the generator's docstring.

The -0.0 cases decide the one-instruction ReLU: `*_negzero` (a hidden pre-activation that is an exact zero: an all-zero fc1 row with bias -0.0) and
`zero_layer` (every term of every sum a signed zero -- the only way the sign of a hidden zero can reach a stored value)."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_split")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_mlp_split", os.path.join(GOLDEN, "make_golden_mlp_split.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(G.DIGESTS) as f:
        digests = json.load(f)
    with np.load(G.ARRAYS) as z:
        arrays = {k: z[k] for k in z.files}
    return digests, arrays


@functools.lru_cache(maxsize=None)
def _run(form, rows):
    return G.run_case(form, rows)


def test_fixture_covers_every_case():
    digests, arrays = _fixture()
    assert len(digests) == len(G.CASES) + sum(1 for f, _ in G.CASES if f == "tap")          # tap: two outputs
    assert {k.split("/")[0] for k in digests} == set(G.FORMS) | {f for f, _ in G.SPECIAL}
    for k, a in arrays.items():
        assert int(k.split("/")[1]) <= G.ARRAY_ROWS and G.digest(a) == digests[k]


@pytest.mark.parametrize("form,rows", G.CASES, ids=["%s-%d" % c for c in G.CASES])
def test_bytes_equal_the_earlier_build(form, rows):
    digests, arrays = _fixture()
    got = _run(form, rows)
    assert not got["sched"].any(), "the row-block counters are left zero"
    names = [n for n in got if n != "sched"]
    assert names
    for name in names:
        k = G.key(form, rows, name)
        a = got[name]
        assert a.shape[0] == rows
        if k in arrays:
            want = arrays[k]
            assert a.dtype == want.dtype and a.shape == want.shape
            diff = np.flatnonzero(a.view(np.uint32).ravel() != want.view(np.uint32).ravel())
            assert diff.size == 0, "%s: %d words differ, first at %d: %r != %r" % (k, diff.size, diff[0], a.ravel()[diff[0]], want.ravel()[diff[0]])
        assert G.digest(a) == digests[k], k


@pytest.mark.parametrize("form", ["plain", "proj"])
@pytest.mark.parametrize("rows", [33, 257])
def test_a_nan_in_one_row_stays_in_that_row(form, rows):
    clean, dirty = _run(form, rows)["out"], _run(form + "_nan", rows)["out"]
    assert np.isnan(dirty[G.NAN_ROW]).all()
    others = np.arange(rows) != G.NAN_ROW
    assert np.array_equal(dirty[others].view(np.uint32), clean[others].view(np.uint32))


def test_the_zero_rows_of_the_negzero_layers_change_nothing_else():
    """the all-zero fc1 rows with bias -0.0 contribute nothing: the outputs are finite and differ from the unmodified layer's (whose
    rows 7 / 9 do contribute), i.e. the case is not vacuous"""
    for form in ("plain", "proj"):
        a, b = _run(form, 33)["out"], _run(form + "_negzero", 33)["out"]
        assert np.isfinite(b).all() and not np.array_equal(a, b)
