"""CPU checks of the boundary: the C-ABI library loads without a GPU and exports every symbol that
include/cppf_hip.h declares; struct layouts match; argument validation fails loudly (no compute calls)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols(name="cppf_hip.h"):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(cppf_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    """ABI 11: include/cppf_hip.h (stable) <-> _lib.STABLE and include/cppf_hip_experimental.h <-> _lib.EXPERIMENTAL, symbol by
    symbol; the library exports all of them and nothing else under the cppf_ prefix."""
    import subprocess
    from cppf2_amd import _lib
    lib = _lib.load()
    stable, exper = _header_symbols(), _header_symbols("cppf_hip_experimental.h")
    assert len(stable) >= 40 and len(exper) >= 10 and not set(stable) & set(exper)
    for s in stable + exper:
        assert hasattr(lib, s), "missing export " + s
    assert sorted(_lib.STABLE) == stable, "ctypes signatures out of sync with the stable header"
    assert sorted(_lib.EXPERIMENTAL) == exper, "ctypes signatures out of sync with the experimental header"
    assert lib.cppf_version() == _lib.ABI_VERSION == 11
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = sorted(set(re.findall(r"\sT\s+(cppf_[a-z0-9_]+)$", nm, flags=re.M)))
    assert exported == sorted(stable + exper), "the library exports a cppf_ symbol no header declares (or the reverse)"


def test_stable_header_is_free_of_the_bench_only_prior_and_of_superseded_forms():
    """What moved out of the stable interface in round 6 stays out: the reference has no logit prior (eval.py:225-235), the f16x2
    arithmetic, the two-kernel encode forms and the test hook are experimental."""
    src = open(os.path.join(ROOT, "include", "cppf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for word in ("logit_prior", "prior_pos", "prior_inv_sigma", "Split16", "debug_grid", "_heads", "reslayer128", "sumgather"):
        assert word not in code, word
    assert "#define CPPF_ABI_VERSION 11" in src


def test_documents_state_the_interface_they_describe():
    """DESIGN.md / INTEGRATION.md / README.md name the ABI version and the sizes of the two interface parts the headers really have."""
    from cppf2_amd import _lib
    n_stable, n_exp = len(_lib.STABLE), len(_lib.EXPERIMENTAL)
    for doc in ("DESIGN.md", "INTEGRATION.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "ABI %d" % _lib.ABI_VERSION in text, doc
        assert "%d entry points" % n_stable in text or "%d stable entry points" % n_stable in text, (doc, n_stable)
        assert str(n_exp) in text, (doc, n_exp)
    assert "cppf_hip_experimental.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_struct_layouts():
    from cppf2_amd import _lib
    from cppf2_amd.pipeline import RESULT_DTYPE
    assert C.sizeof(_lib.SceneGrid) == 32 and C.sizeof(_lib.SceneResult) == 160
    for name in RESULT_DTYPE.names:
        if name == "R":
            assert RESULT_DTYPE.fields[name][1] == _lib.SceneResult.R.offset
        else:
            assert RESULT_DTYPE.fields[name][1] == getattr(_lib.SceneResult, name).offset, name


def test_argument_validation_is_loud():
    from cppf2_amd import _lib
    lib = _lib.load()
    # null pointers / bad sizes are rejected before anything touches a device
    st = lib.cppf_sample_tuples(0, None, None, 10, 5, 1, 0, 1, None, None)
    assert st == -1
    assert b"invalid argument" in lib.cppf_last_error_string()
    with pytest.raises(_lib.CppfError):
        _lib.check(st, "cppf_sample_tuples")
    assert lib.cppf_vote_center_workspace_bytes(4, 1 << 20, 1000) > 4 * (1 << 20) * 4 + 1000 * 44
    assert lib.cppf_rot_bins_workspace_bytes(2, 720, 2000, 180, 100000) >= 2 * 5 * 720 * 8


def test_ops_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from cppf2_amd import ops
    with pytest.raises(ops.CppfError):
        ops.sample_tuples(100, 10, 5, 0)


def test_missing_library_is_loud(monkeypatch, tmp_path):
    from cppf2_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.CppfError):
        _lib.load()


def test_percentile_params_match_numpy():
    import numpy as np
    from cppf2_amd.ops import percentile_params
    rng = np.random.RandomState(0)
    for n in (1, 2, 7, 512, 1111, 20000, 65536):
        for ratio in (0.1, 0.25, 0.5, 0.05):
            x = np.sort(rng.rand(n).astype(np.float32))
            k, g = percentile_params(n, ratio)
            g = np.float32(g)
            lo = x[k]
            hi = x[min(k + 1, n - 1)]
            d = hi - lo
            want = np.percentile(x, ratio * 100)
            got = lo + d * g if g < 0.5 else hi - d * (np.float32(1) - g)
            assert np.float32(got) == np.float32(want), (n, ratio)


def test_no_packed_float32_instruction_of_the_erratum_forms_in_the_library(tmp_path):
    """gfx950 erratum measured in round 3 (scratch/rs/pk_victim4.hip, profiles/r3_pk_op_sel_erratum.md): v_pk_{mul,add,fma}_f32
    whose low lane takes the HIGH half of source 1 (op_sel:[x,1,...]) occasionally computes that lane with source 1 = 0 while a
    wavefront of the wide MLP kernels (another workgroup, another stream) runs on the same SIMD.  The library is built so that the compiler does not emit them
    (cppf2_amd/build.py); this disassembles every gfx950 code object in the built .so and fails on any such instruction."""
    import shutil
    import subprocess
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not found")
    from cppf2_amd import _lib
    so = shutil.copy(_lib.LIB_PATH, tmp_path / "libcppf_hip.so")
    subprocess.run([objdump, "--offloading", str(so)], check=True, cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    objs = sorted(p for p in os.listdir(tmp_path) if p.endswith("gfx950"))
    assert len(objs) >= 7, objs                    # one code object per .hip source
    pat = re.compile(r"v_pk_(mul|add|fma)_f32\b.*\bop_sel:\[[01],1")
    total = packed = 0
    for o in objs:
        dis = subprocess.run([objdump, "-d", str(tmp_path / o)], check=True, stdout=subprocess.PIPE, text=True).stdout
        for line in dis.splitlines():
            if "\tv_" in line or "\ts_" in line:
                total += 1
            if "v_pk_" in line and "_f32" in line:
                packed += 1
                assert not pat.search(line), "packed float32 instruction of an erratum form in %s: %s" % (o, line.strip())
    assert total > 100000          # the disassembly really covered the kernels


def test_no_kernel_of_the_library_uses_scratch_memory(tmp_path):
    """Every kernel keeps its state in registers and LDS: private_segment_fixed_size == 0 and no vector-register spills in the metadata
    of every gfx950 code object of the built library (a register array indexed by a loop-varying value silently becomes a
    scratch allocation; the matrix-core kernels sit at 416-500 of 512 registers).  Scalar registers spilled to VGPR lanes
    (v_writelane, no memory: the rarely taken overflow paths of shot_hist have hundreds) are not counted."""
    import shutil
    import subprocess
    tools = "/opt/rocm/lib/llvm/bin/"
    if not os.path.exists(tools + "llvm-readelf"):
        pytest.skip("llvm-readelf not found")
    from cppf2_amd import _lib
    so = shutil.copy(_lib.LIB_PATH, tmp_path / "libcppf_hip.so")
    subprocess.run([tools + "llvm-objdump", "--offloading", str(so)], check=True, cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    kernels = 0
    for o in sorted(p for p in os.listdir(tmp_path) if p.endswith("gfx950")):
        notes = subprocess.run([tools + "llvm-readelf", "--notes", str(tmp_path / o)], check=True, stdout=subprocess.PIPE, text=True).stdout
        name = None
        for line in notes.splitlines():
            m = re.match(r"\s*\.(name|private_segment_fixed_size|vgpr_spill_count):\s*(\S+)", line)
            if not m:
                continue
            if m.group(1) == "name":
                name = m.group(2)
                kernels += 1
            elif name is not None:
                assert int(m.group(2)) == 0, "%s: %s = %s" % (name, m.group(1), m.group(2))
    assert kernels >= 60


def _untraced_lib():
    """The CDLL itself: calls through it are not recorded in _lib.CALLED (tests/test_zz_stable_abi_coverage_gpu.py counts what
    the GPU tests really ran)."""
    from cppf2_amd import _lib
    lib = _lib.load()
    return lib._lib if isinstance(lib, _lib._Traced) else lib


# fake device addresses, 16-byte aligned and never dereferenced: validation and the rows == 0 return come before any device work
_X, _OUT, _WQ, _B1, _B0, _TAB, _IDX, _AUX, _AUX2, _TAP = (0x100000 * (i + 1) for i in range(10))
_OK, _EINVAL, _EUNSUPPORTED = 0, -1, -2


def _sb(k_in, n_out, proj, chain, pc=3):
    lib = _untraced_lib()
    fn = lib.cppf_reslayer_split_stream_bytes if pc == 3 else lib.cppf_reslayer_split16_stream_bytes
    return fn(k_in, n_out, proj, chain)


def _call_plain(lib, x=_X, ldx=64, k_in=64, out=_OUT, ldo=128, n_out=128, rows=0, wq=_WQ, wq_bytes=None, b1=_B1, b0=_B0, chain=0):
    if wq_bytes is None:
        wq_bytes = _sb(k_in, n_out, b0 is not None, chain)
    return lib.cppf_reslayer_split(x, ldx, k_in, out, ldo, n_out, rows, wq, wq_bytes, b1, b0, chain, None, None)


def _call_tap(lib, first=_TAP, ld_first=128, x=_X, out=_OUT, n_out=128, rows=0):
    wq_bytes = _sb(64, n_out, 1, 1)
    return lib.cppf_reslayer_split_tap(x, 64, 64, first, ld_first, out, 128, n_out, rows, _WQ, wq_bytes, _B1, _B0, 1, None, None)


def _call_gather(lib, head_cols=40, ld_heads=40, slots=5, fdim=32, table=_TAB, ldo=128, n_out=128, rows=0, b0=_B0, wq_bytes=None,
                 chain=0):
    if wq_bytes is None:
        wq_bytes = _sb(head_cols + slots * fdim, n_out, 1, chain)
    return lib.cppf_reslayer_split_gather(_X, ld_heads, head_cols, _IDX, slots, table, fdim, _OUT, ldo, n_out, rows, _WQ, wq_bytes,
                                          _B1, b0, chain, None, None)


def _call_encode(lib, B=2, pts=_AUX, normals=_AUX2, idx=_IDX, k=5, pt_off=_AUX, tup_off=_AUX2, fdim=32, out=_OUT, ldo=128, n_out=128,
                 rows=0, wq_bytes=None):
    if wq_bytes is None:
        wq_bytes = _sb(40 + 5 * fdim, 128, 1, 0)
    return lib.cppf_reslayer_split_encode(B, pts, normals, idx, k, pt_off, tup_off, _TAB, fdim, out, ldo, n_out, rows, _WQ, wq_bytes,
                                          _B1, _B0, 0, None, None)


def _call_decode_prior(lib, x=_X, ldx=128, k_in=128, rows=0, b0=_B0, prior=None, prior_pos=None, sigma=0.0, uniforms=_AUX,
                       bins=_IDX, wq_bytes=None):
    if wq_bytes is None:
        wq_bytes = _sb(k_in, 192, 1, 0)
    return lib.cppf_reslayer_split_decode_prior(x, ldx, k_in, rows, _WQ, wq_bytes, _B1, b0, prior, prior_pos, sigma, uniforms, bins,
                                                None, None)


def _call_decode(lib, k_in=128, rows=0, wq_bytes=None, bins=_IDX):
    if wq_bytes is None:
        wq_bytes = _sb(k_in, 192, 1, 0)
    return lib.cppf_reslayer_split_decode(_X, 128, k_in, rows, _WQ, wq_bytes, _B1, _B0, _AUX, bins, None, None)


def _call_linear(lib, x=_X, ldx=64, k_in=64, ldo=256, n_out=256, rows=0, bias=None, wq_bytes=None):
    if wq_bytes is None:
        wq_bytes = _untraced_lib().cppf_linear_split_stream_bytes(k_in, n_out)
    return lib.cppf_linear_split(x, ldx, k_in, _OUT, ldo, n_out, rows, _WQ, wq_bytes, bias, None)


def _call_sumgather(lib, head_cols=32, ld_heads=32, slots=5, ld_tables=1280, tables=_TAB, n_out=128, rows=0, wq_bytes=None, chain=0):
    if wq_bytes is None:
        wq_bytes = _sb(head_cols, n_out, 1, chain)
    return lib.cppf_reslayer_split_sumgather(_X, ld_heads, head_cols, _IDX, slots, tables, ld_tables, _OUT, 128, n_out, rows, _WQ,
                                             wq_bytes, _B1, _B0, chain, None, None)


def _call_sumencode(lib, B=2, k=5, ld_tables=1280, tables=_TAB, n_out=128, rows=0, wq_bytes=None):
    if wq_bytes is None:
        wq_bytes = _sb(32, n_out, 1, 0)
    return lib.cppf_reslayer_split_sumencode(B, _AUX, _IDX, k, _AUX, _AUX2, tables, ld_tables, _OUT, 128, n_out, rows, _WQ, wq_bytes,
                                             _B1, _B0, 0, None, None)


def _call_reslayer128(lib, x=_X, rows=0, w1=_WQ):
    return lib.cppf_reslayer128(x, rows, w1, _B1, _AUX, None)


def _call_tail(lib, x=_X, ldx=64, k_in=64, n_out=3, rows=0, w0=_AUX, b0=_B0, scatter=None, valid=None, per_group=0, ldo=3):
    return lib.cppf_reslayer_tail(x, ldx, k_in, n_out, rows, _WQ, _B1, w0, b0, _AUX2, scatter, valid, per_group, _OUT, ldo, None)


def _call_split16(lib, **kw):
    """cppf_reslayer_split16 on a plain projection layer (k_in 64 -> 128, one chained layer) unless kw says otherwise; the stream
    size follows the form (gather: head + slot columns; decode: 192 outputs; mode 1: the Linear formula) unless given."""
    from cppf2_amd._lib import ReslayerSplit16Args
    a = dict(x=_X, ldx=64, k_in=64, out=_OUT, ldo=128, n_out=128, rows=0, wq=_WQ, b1=_B1, b0=_B0, chain=1, weight_scale=256.0)
    a.update(kw)
    if "wq_bytes" not in a:
        if a.get("mode") == 1:
            a["wq_bytes"] = _untraced_lib().cppf_linear_split_stream_bytes(a["k_in"], a["n_out"]) // 3 * 2
        elif a.get("uniforms"):
            a["wq_bytes"] = _sb(a["k_in"], 192, 1, 0, pc=2)
        else:
            k = a["k_in"] + (a.get("slots", 0) * a.get("fdim", 0) if a.get("gidx") and a.get("mode") != 2 else 0)
            a["wq_bytes"] = _sb(k, a["n_out"], a["b0"] is not None, a["chain"], pc=2)
    args = ReslayerSplit16Args(**a)
    return lib.cppf_reslayer_split16(C.byref(args))


_GATHER16 = dict(gidx=_IDX, slots=5, table=_TAB, fdim=32, k_in=40, ldx=40)
_DECODE16 = dict(uniforms=_AUX, bins=_AUX2, out=None, ldo=0, chain=0, ldx=128, k_in=128)
_LINEAR16 = dict(mode=1, b0=None, n_out=256, ldo=256, chain=0)
_SUMGATHER16 = dict(mode=2, gidx=_IDX, slots=5, table=_TAB, ld_table=1280, k_in=32, ldx=32)

_VALIDATION_CASES = [
    # (entry, keyword arguments, expected return code)
    ("plain", {}, _OK),
    ("plain", dict(b0=None, k_in=128, ldx=128), _OK),
    ("plain", dict(n_out=256, ldo=256, chain=3), _OK),
    ("plain", dict(x=None), _EINVAL),
    ("plain", dict(out=None), _EINVAL),
    ("plain", dict(b1=None), _EINVAL),
    ("plain", dict(rows=-1), _EINVAL),
    ("plain", dict(k_in=60, ldx=64), _EINVAL),
    ("plain", dict(ldx=66), _EINVAL),
    ("plain", dict(ldx=56), _EINVAL),
    ("plain", dict(ldo=130), _EINVAL),
    ("plain", dict(ldo=64), _EINVAL),
    ("plain", dict(n_out=96, ldo=96, wq_bytes=-1), _EINVAL),
    ("plain", dict(chain=16), _EINVAL),
    ("plain", dict(b0=None), _EINVAL),
    ("plain", dict(x=_X + 4), _EINVAL),
    ("plain", dict(wq=_WQ + 8), _EINVAL),
    ("plain", dict(wq_bytes=1024), _EINVAL),
    ("tap", {}, _OK),
    ("tap", dict(first=None), _EINVAL),
    ("tap", dict(first=_OUT), _EINVAL),
    ("tap", dict(first=_X), _EINVAL),
    ("tap", dict(ld_first=130), _EINVAL),
    ("tap", dict(ld_first=64), _EINVAL),
    ("tap", dict(first=_TAP + 4), _EINVAL),
    ("gather", {}, _OK),
    ("gather", dict(head_cols=0, ld_heads=0), _OK),
    ("gather", dict(head_cols=36, ld_heads=40), _EINVAL),
    ("gather", dict(ld_heads=42), _EINVAL),
    ("gather", dict(slots=0), _EINVAL),
    ("gather", dict(slots=9), _EINVAL),
    ("gather", dict(fdim=24), _EINVAL),
    ("gather", dict(fdim=4), _EINVAL),
    ("gather", dict(table=_TAB + 4), _EINVAL),
    ("gather", dict(b0=None), _EINVAL),
    ("gather", dict(ldo=126), _EINVAL),
    ("gather", dict(chain=16), _EINVAL),
    ("gather", dict(wq_bytes=1024), _EINVAL),
    ("gather", dict(n_out=64, ldo=64), _EUNSUPPORTED),
    ("gather", dict(n_out=64, ldo=64, wq_bytes=1024), _EINVAL),
    ("encode", {}, _OK),
    ("encode", dict(B=0), _EINVAL),
    ("encode", dict(normals=None), _EINVAL),
    ("encode", dict(pts=None), _EINVAL),
    ("encode", dict(idx=None), _EINVAL),
    ("encode", dict(pt_off=None), _EINVAL),
    ("encode", dict(tup_off=None), _EINVAL),
    ("encode", dict(fdim=24), _EINVAL),
    ("encode", dict(out=_OUT + 4), _EINVAL),
    ("encode", dict(ldo=126), _EINVAL),
    ("encode", dict(wq_bytes=1024), _EINVAL),
    ("encode", dict(k=4), _EUNSUPPORTED),
    ("encode", dict(k=4, wq_bytes=1024), _EUNSUPPORTED),
    ("encode", dict(n_out=64, ldo=64), _EUNSUPPORTED),
    ("decode_prior", {}, _OK),
    ("decode_prior", dict(prior=_TAB), _OK),
    ("decode_prior", dict(prior_pos=_TAB, sigma=2.0), _OK),
    ("decode_prior", dict(x=None), _EINVAL),
    ("decode_prior", dict(prior=_TAB, prior_pos=_TAB, sigma=2.0), _EINVAL),
    ("decode_prior", dict(prior_pos=_TAB, sigma=0.0), _EINVAL),
    ("decode_prior", dict(prior_pos=_TAB, sigma=float("inf")), _EINVAL),
    ("decode_prior", dict(prior=_TAB + 4), _EINVAL),
    ("decode_prior", dict(uniforms=None), _EINVAL),
    ("decode_prior", dict(bins=None), _EINVAL),
    ("decode_prior", dict(b0=None), _EINVAL),
    ("decode_prior", dict(k_in=124, ldx=128), _EINVAL),
    ("decode_prior", dict(ldx=130), _EINVAL),
    ("decode_prior", dict(wq_bytes=1024), _EINVAL),
    ("decode", {}, _OK),
    ("decode", dict(bins=None), _EINVAL),
    ("decode", dict(wq_bytes=1024), _EINVAL),
    ("linear", {}, _OK),
    ("linear", dict(bias=_B1, n_out=512, ldo=512), _OK),
    ("linear", dict(x=None), _EINVAL),
    ("linear", dict(n_out=128, ldo=128, wq_bytes=-1), _EINVAL),
    ("linear", dict(k_in=12, ldx=64), _EINVAL),
    ("linear", dict(ldo=258, n_out=256), _EINVAL),
    ("linear", dict(ldo=252, n_out=256), _EINVAL),
    ("linear", dict(ldx=60), _EINVAL),
    ("linear", dict(x=_X + 4), _EINVAL),
    ("linear", dict(wq_bytes=1024), _EINVAL),
    ("sumgather", {}, _OK),
    ("sumgather", dict(head_cols=0, ld_heads=0), _EINVAL),
    ("sumgather", dict(slots=9, ld_tables=9 * 256), _EINVAL),
    ("sumgather", dict(ld_tables=1276), _EINVAL),
    ("sumgather", dict(ld_tables=1282), _EINVAL),
    ("sumgather", dict(tables=_TAB + 4), _EINVAL),
    ("sumgather", dict(chain=16), _EINVAL),
    ("sumgather", dict(wq_bytes=1024), _EINVAL),
    ("sumgather", dict(n_out=64), _EUNSUPPORTED),
    ("sumgather", dict(n_out=64, wq_bytes=1024), _EINVAL),
    ("sumencode", {}, _OK),
    ("sumencode", dict(B=0), _EINVAL),
    ("sumencode", dict(ld_tables=1276), _EINVAL),
    ("sumencode", dict(tables=_TAB + 4), _EINVAL),
    ("sumencode", dict(wq_bytes=1024), _EINVAL),
    ("sumencode", dict(k=4), _EUNSUPPORTED),
    ("sumencode", dict(n_out=64), _EUNSUPPORTED),
    ("reslayer128", {}, _OK),
    ("reslayer128", dict(x=None), _EINVAL),
    ("reslayer128", dict(w1=None), _EINVAL),
    ("reslayer128", dict(rows=-1), _EINVAL),
    ("tail", {}, _OK),
    ("tail", dict(w0=None, b0=None, k_in=4, ldx=4, n_out=4, ldo=4), _OK),
    ("tail", dict(scatter=_IDX, valid=_AUX2, per_group=4), _OK),
    ("tail", dict(n_out=9, ldo=9), _EINVAL),
    ("tail", dict(k_in=62), _EINVAL),
    ("tail", dict(x=_X + 4), _EINVAL),
    ("tail", dict(b0=None), _EINVAL),
    ("tail", dict(valid=_AUX2, per_group=4), _EINVAL),
    ("tail", dict(scatter=_IDX, valid=_AUX2, per_group=0), _EINVAL),
    # f16x2: one struct for every form (plain, tap, gather, decode; mode 1 = Linear, mode 2 = sumgather)
    ("split16", {}, _OK),
    ("split16", dict(b0=None, k_in=128, ldx=128), _OK),
    ("split16", dict(first_out=_TAP, ld_first=128), _OK),
    ("split16", _GATHER16, _OK),
    ("split16", _DECODE16, _OK),
    ("split16", dict(_DECODE16, prior_pos=_TAB, prior_inv_sigma=2.0), _OK),
    ("split16", _LINEAR16, _OK),
    ("split16", _SUMGATHER16, _OK),
    ("split16", dict(x=None), _EINVAL),
    ("split16", dict(wq=None), _EINVAL),
    ("split16", dict(b1=None), _EINVAL),
    ("split16", dict(rows=-1), _EINVAL),
    ("split16", dict(chain=16), _EINVAL),
    ("split16", dict(weight_scale=3.0), _EINVAL),
    ("split16", dict(weight_scale=0.0), _EINVAL),
    ("split16", dict(x=_X + 4), _EINVAL),
    ("split16", dict(ldo=130), _EINVAL),
    ("split16", dict(first_out=_TAP + 4, ld_first=128), _EINVAL),
    ("split16", dict(_GATHER16, uniforms=_AUX, bins=_AUX2), _EINVAL),
    ("split16", dict(_GATHER16, first_out=_TAP, ld_first=128), _EINVAL),
    ("split16", dict(_LINEAR16, b0=_B0), _EINVAL),
    ("split16", dict(mode=2), _EINVAL),
    ("split16", dict(mode=3), _EINVAL),
    # f16x2 rules of the form itself: checked before the rows == 0 return, like the bf16 forms
    ("split16", dict(k_in=60), _EINVAL),
    ("split16", dict(ldx=56), _EINVAL),
    ("split16", dict(n_out=96, ldo=96, wq_bytes=-1), _EINVAL),
    ("split16", dict(ldo=64), _EINVAL),
    ("split16", dict(b0=None), _EINVAL),
    ("split16", dict(wq_bytes=1024), _EINVAL),
    ("split16", dict(out=None), _EINVAL),
    ("split16", dict(first_out=_OUT, ld_first=128), _EINVAL),
    ("split16", dict(first_out=_TAP, ld_first=64), _EINVAL),
    ("split16", dict(_GATHER16, fdim=24), _EINVAL),
    ("split16", dict(_GATHER16, slots=9), _EINVAL),
    ("split16", dict(_GATHER16, table=None), _EINVAL),
    ("split16", dict(_GATHER16, b0=None), _EINVAL),
    ("split16", dict(_GATHER16, n_out=64, ldo=64), _EUNSUPPORTED),
    ("split16", dict(_GATHER16, k_in=0, ldx=-4), _EINVAL),
    ("split16", dict(_DECODE16, bins=None), _EINVAL),
    ("split16", dict(_DECODE16, b0=None), _EINVAL),
    ("split16", dict(_DECODE16, logit_prior=_TAB, prior_pos=_TAB, prior_inv_sigma=2.0), _EINVAL),
    ("split16", dict(_DECODE16, wq_bytes=1024), _EINVAL),
    ("split16", dict(_LINEAR16, n_out=128, ldo=128, wq_bytes=-1), _EINVAL),
    ("split16", dict(_LINEAR16, wq_bytes=1024), _EINVAL),
    ("split16", dict(_SUMGATHER16, ld_table=1276), _EINVAL),
    ("split16", dict(_SUMGATHER16, table=None), _EINVAL),
    ("split16", dict(_SUMGATHER16, n_out=64, ldo=64), _EUNSUPPORTED),
]


@pytest.mark.parametrize("entry,kw,expected", _VALIDATION_CASES,
                         ids=["%s-%d" % (c[0], i) for i, c in enumerate(_VALIDATION_CASES)])
def test_mlp_launch_validation_return_codes(entry, kw, expected):
    """Every ResLayer launch entry point: a valid call with rows = 0 returns 0 (no device work), and a call that breaks one shape,
    stride, alignment, pointer or stream-size rule returns its exact code, without a GPU."""
    lib = _untraced_lib()
    got = globals()["_call_" + entry](lib, **kw)
    assert got == expected, (entry, kw, got, lib.cppf_last_error_string())


# Workspace sizes of the multi-kernel stages, as the layouts gave them before they were written once per stage:
# (B, total_points) -> (cppf_shot352_workspace_bytes, cppf_shot1344_workspace_bytes)
_SHOT_WORKSPACE_BYTES = {
    (1, 0): (0, 0), (4, 0): (0, 0), (0, 100): (0, 0), (-1, 100): (0, 0), (4, -5): (0, 0),
    (1, 1): (70144, 70656), (1, 7): (83712, 84224), (1, 255): (653056, 661248), (1, 257): (658944, 667648),
    (1, 10000): (23067136, 23387136), (1, 123457): (284018944, 287970048),
    (4, 1): (266752, 267264), (4, 257): (855552, 864256), (4, 1000): (2563584, 2595840), (4, 10000): (23263744, 23583744),
    (64, 1): (4200704, 4201216), (64, 7): (4214272, 4214784), (64, 255): (4783616, 4791808), (64, 1000): (6497536, 6529792),
    (64, 10000): (27197696, 27517696), (64, 123457): (288149504, 292100608),
}
# (B, cells_cap, total_tuples) -> cppf_vote_center_workspace_bytes
_VC_WORKSPACE_BYTES = {
    (0, 100, 10): 0, (4, 0, 10): 0, (4, 100, -1): 0,
    (1, 1, 0): 1536, (1, 1, 999): 49664, (1, 1000, 1): 5632, (1, 36864, 0): 148736, (1, 36865, 999): 197120,
    (1, 1048576, 1280000): 65635584, (1, 1179649, 1): 4720640,
    (4, 1, 1): 3840, (4, 1000, 999): 67584, (4, 36864, 1280000): 62033152, (4, 36865, 0): 593408, (4, 1048576, 1): 16780800,
    (4, 1179649, 999): 18926848,
    (64, 1, 0): 49664, (64, 1000, 1): 305664, (64, 36864, 999): 9534720, (64, 36865, 1280000): 70926848,
    (64, 1048576, 0): 268484864, (64, 1048576, 1280000): 329924864, (64, 1179649, 999): 302089216,
}


def test_stage_workspace_bytes_are_pinned():
    lib = _untraced_lib()
    for (B, n), (b352, b1344) in _SHOT_WORKSPACE_BYTES.items():
        assert lib.cppf_shot352_workspace_bytes(B, n) == b352, (B, n)
        assert lib.cppf_shot1344_workspace_bytes(B, n) == b1344, (B, n)
    for (B, cells, T), want in _VC_WORKSPACE_BYTES.items():
        assert lib.cppf_vote_center_workspace_bytes(B, cells, T) == want, (B, cells, T)


# Workspace sizes of the post-vote stages, recorded from the library as it was built while they shared one source file with the
# centre vote (cppf_vote_center's are above).
# (B, S, max_kept, num_rots, bmm_size) -> cppf_rot_bins_workspace_bytes.  The lookup-table path's partials are never smaller than
# the dense path's sums (2 * nchunks * sub >= nchunks + 1 slots per scene): "dense wins" is at most a tie, one chunk and one sub-block.
_RB_WORKSPACE_BYTES = {
    (0, 720, 100, 180, 100000): 0, (2, 0, 100, 180, 100000): 0, (2, 720, -1, 180, 100000): 0, (2, 720, 100, 0, 100000): 0,
    (2, 720, 100, 180, 0): 0,                                                              # each rejected argument
    (2, 720, 0, 180, 100000): 414720, (64, 720, 0, 180, 100000): 2949120,                  # nothing kept
    (15, 720, 2000, 180, 100000): 12441600, (16, 720, 2000, 180, 100000): 2949120,         # 32- and 160-pair row blocks
    (2, 720, 2000, 180, 5760): 1451520, (2, 720, 2000, 180, 5761): 2903040,                # block target >= and < bmm_size
    (16, 64, 50, 8, 1280): 16384, (16, 64, 50, 8, 1281): 32768,
    (2, 64, 9, 8, 8): 18432, (2, 64, 9, 8, 4): 36864,                                      # num_rots == bmm_size, and above it
    (2, 720, 10, 180, 2000): 23040,                                                        # the tie: dense == lookup-table
    (2, 720, 100, 180, 100000): 414720,                                                    # the lookup-table size wins
    (64, 720, 20000, 180, 100000): 106168320,                                              # the benchmark's own
    (2, 64, 0, 8, 32): 2048, (2, 64, 1, 8, 32): 2048, (2, 64, 9, 8, 32): 6144,
    (1, 1, 1, 1, 1): 256, (1, 32767, 100000, 1024, 1048576): 1644116992, (3, 721, 50000, 180, 100000): 56065024,
}
# (total_points, B) -> cppf_backvote_workspace_bytes
_BV_WORKSPACE_BYTES = {(0, 1): 0, (1, 1): 256, (63, 4): 256, (64, 4): 256, (65, 4): 512, (100000, 64): 400128, (1 << 31, 1): 8589934592}
# (B, K) -> cppf_grid_peaks_workspace_bytes
_GP_WORKSPACE_BYTES = {(0, 4): 0, (-1, 4): 0, (4, 0): 0, (4, 17): 0, (1, 1): 256, (1, 16): 256, (4, 5): 256, (32, 1): 256, (33, 1): 512,
                       (64, 16): 8192, (65535, 16): 8388608}


def test_post_vote_workspace_bytes_are_pinned():
    lib = _untraced_lib()
    for args, want in _RB_WORKSPACE_BYTES.items():
        assert lib.cppf_rot_bins_workspace_bytes(*args) == want, args
    for args, want in _BV_WORKSPACE_BYTES.items():
        assert lib.cppf_backvote_workspace_bytes(*args) == want, args
    for args, want in _GP_WORKSPACE_BYTES.items():
        assert lib.cppf_grid_peaks_workspace_bytes(*args) == want, args


def test_rot_bins_refuses_chunks_shorter_than_one_pair_before_any_device_work():
    """Validation order of cppf_rot_bins / cppf_rot_bins2: arguments, then the workspace size, then num_rots > bmm_size."""
    lib = _untraced_lib()

    def call(nax, bmm_size, short=0, num_rots=8, sphere=_AUX):
        need = lib.cppf_rot_bins_workspace_bytes(2, 64, 9, num_rots, bmm_size) - short
        cols = (0, 2) if nax == 2 else (0,)
        return (lib.cppf_rot_bins2 if nax == 2 else lib.cppf_rot_bins)(
            2, _X, _AUX, _IDX, 5, _AUX2, _B1, *cols, _IDX, _AUX, _B0, _AUX2, 9, num_rots, _TAB, _TAP, sphere, 64, 0.9, bmm_size, None,
            0, 0, _OUT, None, None, _WQ, need, None)

    for nax in (1, 2):
        assert call(nax, 4) == _EUNSUPPORTED
        assert lib.cppf_last_error_string() == b"cppf_rot_bins: bmm_size 4 < num_rots 8 unsupported"
        assert call(nax, 4, short=1) == _EINVAL
        assert call(nax, 4, sphere=None) == _EINVAL
        assert call(nax, 32, num_rots=1025) == _EINVAL


_SHOT_PARAMS = {
    "cppf_estimate_normals": ("B", "pts", "pt_off", "n", "normal_r", "out_normal", "ws", "ws_bytes", "flags", "stream"),
    "cppf_shot352": ("B", "pts", "pt_off", "n", "normal_r", "shot_r", "out_shot", "out_normal", "out_rf", "ws", "ws_bytes", "flags",
                     "stream"),
    "cppf_shot352_from_normals": ("B", "pts", "pt_off", "n", "normals", "shot_r", "out_shot", "out_rf", "ws", "ws_bytes", "stream"),
    "cppf_shot_prepare": ("B", "pts", "pt_off", "n", "normal_r", "shot_r", "out_normal", "ws", "ws_bytes", "flags", "stream"),
    "cppf_shot_describe": ("B", "pts", "pt_off", "n", "normals", "shot_r", "nan_to_zero", "out_shot", "out_rf", "ws", "ws_bytes",
                           "stream"),
    "cppf_shot1344": ("B", "pts", "colors", "pt_off", "n", "normal_r", "shot_r", "out_shot", "out_normal", "ws", "ws_bytes", "flags",
                      "stream"),
}


def _call_shot(lib, entry, short=0, **kw):
    """`entry` with valid fake arguments for 1000 points, but for `kw`; the workspace is `short` bytes smaller than it needs."""
    a = dict(B=2, pts=_X, colors=_AUX2, pt_off=_AUX, n=1000, normal_r=0.02, shot_r=0.03, normals=_IDX, out_shot=_OUT,
             out_normal=_TAB, out_rf=_B0, nan_to_zero=0, ws=_WQ, flags=0, stream=None)
    a.update(kw)
    need = lib.cppf_shot1344_workspace_bytes if entry == "cppf_shot1344" else lib.cppf_shot352_workspace_bytes
    a["ws_bytes"] = need(a["B"], max(a["n"], 1)) - short
    return getattr(lib, entry)(*(a[p] for p in _SHOT_PARAMS[entry]))


def _call_vc(lib, short=0, **kw):
    """cppf_vote_center with valid fake arguments (4 scenes, 1000 pairs, mode 1), but for `kw`."""
    a = dict(B=4, pts=_X, pt_off=_AUX, idx=_IDX, k=5, tup_off=_AUX2, max_t=300, T=1000, tr=_B1, vote_wt=None, res=0.01, num_rots=90,
             cos_tab=_TAB, sin_tab=_TAP, grids=_B0, grid=None, grid_off=None, cells_cap=200000, mode=1, ws=_WQ, out_argmax=_OUT,
             out_peak=None, out_world=None)
    a.update(kw)
    ws_bytes = lib.cppf_vote_center_workspace_bytes(a["B"], a["cells_cap"], a["T"]) - short
    return lib.cppf_vote_center(a["B"], a["pts"], a["pt_off"], a["idx"], a["k"], a["tup_off"], a["max_t"], a["T"], a["tr"],
                                a["vote_wt"], a["res"], a["num_rots"], a["cos_tab"], a["sin_tab"], a["grids"], a["grid"],
                                a["grid_off"], a["cells_cap"], a["mode"], a["ws"], ws_bytes, a["out_argmax"], a["out_peak"],
                                a["out_world"], None)


_REQUIRED = {
    "cppf_estimate_normals": ("pts", "pt_off", "out_normal"),
    "cppf_shot352": ("pts", "pt_off", "out_shot", "out_normal"),
    "cppf_shot352_from_normals": ("pts", "pt_off", "normals", "out_shot"),
    "cppf_shot_prepare": ("pts", "pt_off", "out_normal"),
    "cppf_shot_describe": ("pts", "pt_off", "normals", "out_shot"),
    "cppf_shot1344": ("pts", "colors", "pt_off", "out_shot", "out_normal"),
}
_STAGE_CASES = []
for _e, _req in _REQUIRED.items():
    _radii = [r for r in ("normal_r", "shot_r") if r in _SHOT_PARAMS[_e]]
    _STAGE_CASES += [("shot", _e, {p: None}, _EINVAL) for p in _req]
    _STAGE_CASES += [("shot", _e, {r: v}, _EINVAL) for r in _radii for v in (0.0, -0.01)]
    _STAGE_CASES += [
        ("shot", _e, dict(B=0), _EINVAL),
        ("shot", _e, dict(n=-1), _EINVAL),
        ("shot", _e, dict(n=0), _OK),
        ("shot", _e, dict(n=0, ws=None), _OK),
        ("shot", _e, dict(short=1), _EINVAL),
        ("shot", _e, dict(ws=None), _EINVAL),
    ]
_STAGE_CASES += [
    ("vc", None, dict(out_argmax=None), _EINVAL),
    ("vc", None, dict(grids=None), _EINVAL),
    ("vc", None, dict(k=1), _EINVAL),
    ("vc", None, dict(num_rots=0), _EINVAL),
    ("vc", None, dict(cells_cap=0), _EINVAL),
    ("vc", None, dict(max_t=1001), _EINVAL),
    ("vc", None, dict(grid=_AUX2), _EINVAL),
    ("vc", None, dict(short=1), _EINVAL),
    ("vc", None, dict(short=1, mode=2), _EINVAL),
    ("vc", None, dict(ws=None), _EINVAL),
    ("vc", None, dict(mode=4), _EINVAL),
    ("vc", None, dict(mode=4 | 0x800), _EINVAL),
    ("vc", None, dict(mode=0xff), _EINVAL),
]


@pytest.mark.parametrize("kind,entry,kw,expected", _STAGE_CASES,
                         ids=["%s-%d" % (c[1] or "cppf_vote_center", i) for i, c in enumerate(_STAGE_CASES)])
def test_shot_and_vote_center_validation_return_codes(kind, entry, kw, expected):
    """The six SHOT entry points and cppf_vote_center: a null required pointer, a non-positive radius or size, a workspace one
    byte short and an unknown mode are refused, and no points is a valid call, all before any device work."""
    lib = _untraced_lib()
    got = _call_shot(lib, entry, **kw) if kind == "shot" else _call_vc(lib, **kw)
    assert got == expected, (entry, kw, got, lib.cppf_last_error_string())
