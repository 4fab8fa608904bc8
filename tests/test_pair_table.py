"""Pair-feature tables without a GPU: the invariants of the NumPy restatement (tests/pair_table_ref.py),
the .npz round trip of cppf2_amd.pair_table.PairTable, parameter validation on the host and in the library, and eval.py's
flag conflicts."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pair_table_ref as R      # noqa: E402

F32 = np.float32


def _batch(seed=0, counts_p=(30, 50), counts_t=(400, 700), k=5):
    rng = np.random.default_rng(seed)
    n = sum(counts_p)
    pts = (rng.integers(0, 40, (n, 3)) * 2.0 ** -9).astype(F32)
    nrm = rng.standard_normal((n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    nrm[3] = 0
    canon = rng.uniform(-0.6, 0.6, (n, 3)).astype(F32)
    idx = np.concatenate([rng.integers(0, c, (t, k)) for c, t in zip(counts_p, counts_t)]).astype(np.int32)
    off = (lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.int32))
    return pts, nrm, canon, idx, off(counts_p), off(counts_t)


def _table(seed=0, nd=5, na=4, nb=256):
    from cppf2_amd import pair_table
    pts, nrm, canon, idx, pt_off, tup_off = _batch(seed)
    d_step = F32(2.0 ** -5)
    edges = R.make_edges(na)
    keys, coords = R.pair_keys(pts, nrm, idx, pt_off, tup_off, nd, d_step, na, edges)
    pay = R.payload(canon, idx, pt_off, tup_off, nb)
    cell_off, entries, order = R.assemble(keys, pay, nd * na ** 3)
    t = pair_table.PairTable(nd, d_step, na, nb, edges, cell_off, entries, np.array([0.1, 0.2, 0.3], F32), 0.374,
                             dict(mesh="m.ply", views=2, tuples_per_view=400, seed=seed, res=2e-3))
    return t, keys, coords, pay, order, tup_off


def test_reference_table_invariants():
    t, keys, coords, pay, order, tup_off = _table()
    off = t.cell_off.astype(np.int64)
    assert off[0] == 0 and off[-1] == t.E == int((keys >= 0).sum()) and (np.diff(off) >= 0).all()
    assert 0 < t.E < len(keys)                                        # some tuples are invalid (the zero normal, long pairs)
    for c in np.nonzero(np.diff(off))[0]:
        ids = order[off[c]:off[c + 1]]
        assert (keys[ids] == c).all() and (np.diff(ids) > 0).all()    # a cell's entries: its key, in entry-id order
    assert np.array_equal(t.entries, pay[order]) and not t.entries[:, 6:].any()
    k4 = ((coords[:, 0] * t.na + coords[:, 1]) * t.na + coords[:, 2]) * t.na + coords[:, 3]
    assert np.array_equal(k4[keys >= 0], keys[keys >= 0])
    assert (coords[keys >= 0] >= 0).all() and (coords[keys >= 0, 0] < t.nd).all() and (coords[keys >= 0, 1:] < t.na).all()
    # the draw takes every tuple from exactly one source, and an own-cell draw returns an entry of that cell
    u0 = np.random.default_rng(1).random(len(keys)).astype(F32)
    bins, hits, source = R.draw(keys, coords, tup_off, t.nd, t.na, t.cell_off, t.entries, u0)
    assert hits.sum() == len(keys) and np.array_equal(hits.sum(1), np.diff(tup_off))
    assert (source[keys < 0] == 2).all() and (source[keys >= 0] == 0).all()
    for tt in np.nonzero(source == 0)[0][:50]:
        cell = t.entries[off[keys[tt]]:off[keys[tt] + 1], :6]
        assert (cell == bins[tt]).all(1).any()
    assert bins.dtype == np.int32 and bins.min() >= 0 and bins.max() <= 255


def test_reference_payload_rounding():
    x = np.array([-0.6, -0.5, 0.0, 0.5, 0.7, np.nan], F32)
    assert R.canon_bins(x, 256).tolist() == [0, 0, 128, 255, 255, 0]
    assert R.canon_bins(x, 2).tolist() == [0, 0, 1, 1, 1, 0]
    assert R.make_edges(12)[0] == 1 and R.make_edges(12)[12] == -1 and (np.diff(R.make_edges(12)) < 0).all()


def test_npz_round_trip_is_bit_equal(tmp_path):
    from cppf2_amd import pair_table
    t = _table(2)[0]
    path = str(tmp_path / "t.npz")
    t.save(path)
    with np.load(path, allow_pickle=False) as z:                      # arrays and scalars only: loads without pickle
        assert all(z[k].dtype != object for k in z.files)
    b = pair_table.PairTable.load(path)
    for k in ("edges", "cell_off", "entries", "bound"):
        assert getattr(b, k).dtype == getattr(t, k).dtype and getattr(b, k).tobytes() == getattr(t, k).tobytes(), k
    assert (b.nd, b.na, b.nb, b.diameter) == (t.nd, t.na, t.nb, t.diameter)
    assert b.d_step.dtype == np.float32 and b.d_step.tobytes() == t.d_step.tobytes()
    assert b.meta == t.meta == dict(mesh="m.ply", views=2, tuples_per_view=400, seed=2, res=2e-3)
    path2 = str(tmp_path / "t2.npz")
    b.save(path2)
    with np.load(path) as z1, np.load(path2) as z2:
        assert sorted(z1.files) == sorted(z2.files) and all(z1[k].tobytes() == z2[k].tobytes() for k in z1.files)


def test_parameter_validation(tmp_path):
    from cppf2_amd import pair_table
    t = _table()[0]
    args = dict(nd=t.nd, d_step=t.d_step, na=t.na, nb=t.nb, edges=t.edges, cell_off=t.cell_off, entries=t.entries, bound=t.bound,
                diameter=t.diameter)
    pair_table.PairTable(**args)
    bad_off = t.cell_off.copy()
    bad_off[-1] += 1
    for kw in (dict(nd=0), dict(na=1), dict(nb=1), dict(nb=257), dict(nd=1 << 20, na=64), dict(d_step=0.0), dict(d_step=np.nan),
               dict(edges=t.edges[:-1]), dict(cell_off=t.cell_off[:-1]), dict(cell_off=bad_off), dict(cell_off=t.cell_off[::-1].copy()),
               dict(entries=t.entries[:, :6]), dict(entries=t.entries.astype(np.int32)), dict(bound=t.bound[:2])):
        with pytest.raises(ValueError):
            pair_table.PairTable(**dict(args, **kw))
    box = type("M", (), dict(bounds=(np.zeros(3), np.array([0.1, 0.2, 0.3]))))()
    for kw in (dict(nd=0), dict(na=1), dict(nb=300), dict(views=0), dict(tuples_per_view=0)):
        with pytest.raises(ValueError):                               # before any device work
            pair_table.build(box, **kw)
    with pytest.raises(ValueError):
        pair_table.build(type("M", (), dict(bounds=(np.zeros(3), np.zeros(3))))())
    np.savez(str(tmp_path / "x.npz"), edges=t.edges)
    with pytest.raises(ValueError, match="not a pair table"):
        pair_table.PairTable.load(str(tmp_path / "x.npz"))
    with pytest.raises(SystemExit):
        pair_table.main(["--mesh", "a.ply"])                          # --out missing
    with pytest.raises(SystemExit):
        pair_table.main(["--mesh", "a.ply", "--bop-models", "m", "--out", "t.npz"])


_A = [0x100000 * (i + 1) for i in range(12)]       # fake device addresses, never dereferenced: validation comes first


def _keys(lib, **kw):
    a = dict(B=2, pts=_A[0], normals=_A[1], canon=_A[2], idx=_A[3], k=5, pt_off=_A[4], tup_off=_A[5], total=0, nd=32,
             d_step=0.01, na=12, edges=_A[6], nb=256, keys=_A[7], payload=_A[8])
    a.update(kw)
    return lib.cppf_pair_keys(a["B"], a["pts"], a["normals"], a["canon"], a["idx"], a["k"], a["pt_off"], a["tup_off"], a["total"],
                              a["nd"], ctypes.c_float(a["d_step"]), a["na"], a["edges"], a["nb"], a["keys"], a["payload"], None)


def _draw(lib, **kw):
    a = dict(B=2, pts=_A[0], normals=_A[1], idx=_A[3], k=5, pt_off=_A[4], tup_off=_A[5], total=0, nd=32, d_step=0.01, na=12,
             edges=_A[6], cell_off=_A[7], entries=_A[8], E=100, uniforms=_A[9], bins=_A[10], hits=_A[11])
    a.update(kw)
    return lib.cppf_pair_table_draw(a["B"], a["pts"], a["normals"], a["idx"], a["k"], a["pt_off"], a["tup_off"], a["total"], a["nd"],
                                    ctypes.c_float(a["d_step"]), a["na"], a["edges"], a["cell_off"], a["entries"], a["E"],
                                    a["uniforms"], a["bins"], a["hits"], None)


@pytest.mark.parametrize("fn,kw,want", [
    ("keys", {}, 0), ("keys", dict(canon=None, payload=None, nb=0), 0), ("keys", dict(na=2, nb=2), 0),
    ("keys", dict(nb=1), -1), ("keys", dict(nb=257), -1), ("keys", dict(canon=None), -1), ("keys", dict(payload=None), -1),
    ("keys", dict(payload=_A[8] + 4), -1), ("keys", dict(k=1), -1), ("keys", dict(k=9), -1), ("keys", dict(nd=0), -1),
    ("keys", dict(na=1), -1), ("keys", dict(nd=1 << 20, na=64), -1), ("keys", dict(d_step=0.0), -1),
    ("keys", dict(d_step=float("nan")), -1), ("keys", dict(edges=None), -1), ("keys", dict(keys=None), -1), ("keys", dict(B=0), -1),
    ("draw", {}, 0), ("draw", dict(E=0, total=10), -1), ("draw", dict(E=1 << 31), -1), ("draw", dict(nd=1 << 20, na=64), -1),
    ("draw", dict(na=1), -1), ("draw", dict(k=9), -1), ("draw", dict(entries=_A[8] + 4), -1), ("draw", dict(hits=None), -1),
    ("draw", dict(cell_off=None), -1), ("draw", dict(uniforms=None), -1), ("draw", dict(d_step=-1.0), -1),
])
def test_library_argument_validation(fn, kw, want):
    """Both entry points refuse a bad size, pointer or alignment with CPPF_EINVAL before any device work (no GPU needed), and a
    valid call without tuples returns 0."""
    from cppf2_amd import _lib
    lib = _lib.load()
    lib = lib._lib if isinstance(lib, _lib._Traced) else lib
    got = (_keys if fn == "keys" else _draw)(lib, **kw)
    assert got == want, (fn, kw, got, lib.cppf_last_error_string())
    if want:
        assert b"invalid argument" in lib.cppf_last_error_string()


@pytest.mark.parametrize("kw,match", [
    (dict(data="depth", pair_table="t.npz", teacher_prior=True), "teacher_prior"),
    (dict(data="depth", pair_table="t.npz", ckpt_shot="a.pth"), "ckpt"),
    (dict(data="depth", pair_table="t.npz", ckpt_dino="a.pth"), "ckpt"),
    (dict(data="depth", pair_table="t.npz", ckpt_dir="ckpts"), "ckpt"),
    (dict(data="synthetic", pair_table="t.npz"), "data=depth"),
    (dict(pair_table="t.npz"), "data=depth"),
    (dict(data="nocs", pair_table="t.npz", log_dir="x"), "data=depth"),
    (dict(data="bop", pair_table="t.npz", bop_root="r", out_csv="o.csv"), "data=depth"),
    (dict(data="depth", pair_tables="tables"), "data=bop"),
    (dict(data="bop", pair_tables="tables", bop_root="r", out_csv="o.csv", teacher_prior=True), "teacher_prior"),
    (dict(data="bop", pair_tables="tables", bop_root="r", out_csv="o.csv", ckpt_shot="a.pth"), "ckpt"),
])
def test_eval_flag_conflicts(kw, match, monkeypatch):
    monkeypatch.chdir(ROOT)
    import eval as ev
    with pytest.raises(ValueError, match=match):
        ev.main(**kw)


def test_a_missing_table_is_named(monkeypatch, tmp_path):
    monkeypatch.chdir(ROOT)
    import eval as ev
    with pytest.raises(FileNotFoundError, match="obj_000007.npz"):
        ev.load_pair_table(str(tmp_path / "obj_000007.npz"), "cpu")
