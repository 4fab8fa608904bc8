"""What the tuple MLPs launch: for each call form of the models, the ordered list of MLP launches -- (ops function, first layer,
chain length, n_out, produces the tapped activation, writes in place) -- in each arithmetic.  GPU part: the real ops functions are
wrapped at attribute level (as benchlib.evidence.mlp_launch_loops does) and the launches of real calls are recorded; the library-GEMM
layers of the native arithmetic are recorded through torch._addmm_activation (their order and widths only).  CPU part: the same table
from models.plan_launches alone.  Plus: an in-place weight update re-packs the streams a plan reads."""
import pytest

torch = pytest.importorskip("torch")

ARITHS = ("split", "split16", "native")
RECORDED = ("reslayer_split_encode", "reslayer_split_sumencode", "reslayer_split_gather", "reslayer_split_sumgather",
            "reslayer_split", "reslayer_split_decode", "reslayer_split16", "reslayer_tail", "reslayer128_")

# rows: (op, first layer, chain, n_out, tapped, in place); layers of a two-stack call are counted over both stacks
_TUPLE_MLP = [("reslayer_split", 5, 2, 256, True, False), ("reslayer_split", 8, 0, 192, False, False)]
_TUPLE_MLP_NATIVE = ([("gemm", 0, 0, 128, False, False)] + [("reslayer128_", i, 0, 128, False, True) for i in range(1, 5)]
                     + [("gemm", 5, 0, 256, True, False), ("gemm", 6, 0, 256, False, False), ("gemm", 7, 0, 256, False, True),
                        ("gemm", 8, 0, 192, False, False)])
_SCALE = [("reslayer_split", 0, 0, 128, False, False), ("reslayer_split", 1, 0, 64, False, False), ("reslayer_tail", 2, 0, 3, False, False)]
_SCALE_NATIVE = [("gemm", 0, 0, 128, False, False), ("gemm", 1, 0, 64, False, False), ("gemm", 2, 0, 3, False, False)]
_DECODE = [("reslayer_split_decode", 8, 0, 192, False, False)]

EXPECTED = {
    # the headline SHOT pass: pair features built by the first launch, the tap inside the second, the bins drawn by the third
    "shot_tuples_decode": {"split": [("reslayer_split_encode", 0, 4, 128, False, False)] + _TUPLE_MLP[:1] + _DECODE,
                           "native": _TUPLE_MLP_NATIVE},
    "shot_tuples": {"split": [("reslayer_split_encode", 0, 4, 128, False, False)] + _TUPLE_MLP, "native": _TUPLE_MLP_NATIVE},
    "shot_tuples_scale": {"split": [("reslayer_split_encode", 0, 4, 128, False, False)] + _TUPLE_MLP + _SCALE,
                          "native": _TUPLE_MLP_NATIVE + _SCALE_NATIVE},
    "shot_sum_tables": {"split": [("reslayer_split_sumgather", 0, 4, 128, False, False)] + _TUPLE_MLP, "native": _TUPLE_MLP_NATIVE},
    "shot_separate_encode": {"split": [("reslayer_split_gather", 0, 4, 128, False, False)] + _TUPLE_MLP, "native": _TUPLE_MLP_NATIVE},
    "shot_heads_rows": {"split": [("reslayer_split", 0, 4, 128, False, False)] + _TUPLE_MLP + _SCALE,
                        "native": _TUPLE_MLP_NATIVE + _SCALE_NATIVE},
    "dino_tuples_decode": {"split": [("reslayer_split_sumencode", 0, 4, 128, False, False)] + _TUPLE_MLP[:1] + _DECODE,
                           "native": _TUPLE_MLP_NATIVE},
    "scale_rows_tail": {"split": [("reslayer_split_gather", 0, 0, 128, False, False)] + _SCALE[1:2]
                        + [("reslayer_tail", 2, 0, 3, False, False)], "native": _SCALE_NATIVE},
    "logit_keep_input": {"split": [("reslayer_split", 0, 1, 256, False, False), ("reslayer_split", 2, 0, 192, False, False)],
                         "native": [("gemm", 0, 0, 256, False, False), ("gemm", 1, 0, 256, False, True), ("gemm", 2, 0, 192, False, False)]},
    # an input the split kernels cannot read (not 16-byte aligned): the library GEMMs until a launch has written a fresh buffer
    "misaligned_input": {"split": [("gemm", 0, 0, 128, False, False)] + _SCALE[1:]
                         + [("gemm", 0, 0, 256, False, True), ("gemm", 1, 0, 256, False, True), ("gemm", 2, 0, 192, False, False)],
                         "native": _SCALE_NATIVE + [("gemm", 0, 0, 256, False, True), ("gemm", 1, 0, 256, False, True),
                                                    ("gemm", 2, 0, 192, False, False)]},
}
# f16x2 arithmetic: the same launches through cppf_reslayer_split16, except the table-fed first layer (its own entry point) and the
# pair features, which only the split-arithmetic first launch builds itself (the f16x2 forms read them from an array)
_F16 = {"reslayer_split": "reslayer_split16", "reslayer_split_gather": "reslayer_split16", "reslayer_split_encode": "reslayer_split16",
        "reslayer_split_decode": "reslayer_split16", "reslayer_split_sumencode": "reslayer_split_sumgather"}
for _rows in EXPECTED.values():
    _rows["split16"] = [(_F16.get(r[0], r[0]),) + r[1:] for r in _rows["split"]]


# ------------------------------------------------------------------------------------------------------------------------------
# the cases, on the GPU
# ------------------------------------------------------------------------------------------------------------------------------
def scenario(dev, B=2, N=1024, T=2000, seed=0):
    """The models (default init, k = 5, F = 64) and the inputs of a B-scene batch of T tuples per scene."""
    from cppf2_amd import models, ops
    from cppf2_amd.config import load_config
    cfg = load_config("config", "config", ["category=bottle"])
    torch.manual_seed(seed)
    env = {"shot": models.BeyondCPPFShot(cfg).to(dev).eval(), "dino": models.BeyondCPPFDino(cfg).to(dev).eval()}
    g = torch.Generator(device="cpu").manual_seed(seed)
    env.update(pts=torch.randn(B * N, 3, generator=g).to(dev),
               nrm=torch.nn.functional.normalize(torch.randn(B * N, 3, generator=g), dim=-1).to(dev),
               feat=torch.randn(B * N, 64, generator=g).to(dev), desc=torch.randn(B * N, 1024, generator=g).to(dev),
               idx=torch.randint(0, N, (B * T, 5), generator=g).to(dev, torch.int32), u=torch.rand(B * T, 6, generator=g).to(dev),
               feat256=torch.randn(B * T, 256, generator=g).to(dev), pt_off=ops._offsets([N] * B, dev), tup_off=ops._offsets([T] * B, dev),
               rows=torch.randint(0, B * T, (B * 64,), generator=g).to(dev, torch.int32),
               counts=torch.randint(1, 65, (B,), generator=g).to(dev, torch.int32))
    return env


def _misaligned(x):
    """A copy of x whose data pointer is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    y = buf[1:].view(x.shape)
    y.copy_(x)
    return y


def run_case(name, env):
    """Runs case `name` in the current models.MLP_ARITH; returns its outputs."""
    from cppf2_amd import models, ops
    shot, dino = env["shot"], env["dino"]
    pts, nrm, feat, idx, pt_off, tup_off = (env[k] for k in ("pts", "nrm", "feat", "idx", "pt_off", "tup_off"))
    bins = torch.zeros((idx.shape[0], 6), dtype=torch.int32, device=pts.device)
    if name in ("shot_tuples_decode", "shot_tuples", "shot_tuples_scale", "shot_sum_tables"):
        cls, second = shot.heads_from_tuples(pts, idx, feat, nrm, pt_off, tup_off, lazy_scale=name != "shot_tuples_scale",
                                             decode=(env["u"], None, bins) if name == "shot_tuples_decode" else None,
                                             sum_tables=name == "shot_sum_tables")
        return (bins if cls is None else cls, second)
    if name == "shot_separate_encode":          # bench.py --separate-encode: the pair features from their own kernel
        if shot.gather_supported(64, 5):
            heads, gidx = ops.encode_tuples_shot_heads(pts, idx, nrm, pt_off, tup_off)
            return models.fused_stack((shot.tuple_encoder, shot.logit_encoder), None, gather=(heads, gidx, feat))
        return shot.heads(ops.encode_tuples_shot(pts, idx, feat, nrm, pt_off, tup_off), lazy_scale=True)
    if name == "shot_heads_rows":
        return shot.heads(ops.encode_tuples_shot(pts, idx, feat, nrm, pt_off, tup_off))
    if name == "dino_tuples_decode":
        cls, second = dino.heads_from_tuples(pts, env["desc"], idx, pt_off, tup_off, lazy_scale=True, decode=(env["u"], None, bins))
        return (bins if cls is None else cls, second)
    if name == "scale_rows_tail":
        out = torch.zeros((idx.shape[0], 3), dtype=torch.float32, device=pts.device)
        return (shot.scale_head_rows(env["feat256"], env["rows"], scatter=(env["counts"], 64, out)),)
    if name == "logit_keep_input":
        x = env["feat256"].clone()
        y = models.fused_stack(shot.logit_encoder, x, keep_input=True)
        assert torch.equal(x, env["feat256"])
        return (y,)
    if name == "misaligned_input":
        x = _misaligned(env["feat256"])
        assert x.data_ptr() % 16 != 0
        return (models.fused_stack(shot.scale_encoder, x), models.fused_stack(shot.logit_encoder, _misaligned(env["feat256"])))
    raise KeyError(name)


class _Recorder:
    """Records the MLP launches of fused_stack calls: the ops functions of RECORDED and torch._addmm_activation (one per GEMM layer),
    wrapped at attribute level; holds every output so that no buffer is reused while a call is recorded."""

    def __init__(self, monkeypatch):
        from cppf2_amd import models, ops
        self.launches, self.cur = [], None
        for n in RECORDED:
            monkeypatch.setattr(ops, n, self._op(n, getattr(ops, n)))
        monkeypatch.setattr(torch, "_addmm_activation", self._op("gemm", torch._addmm_activation))
        monkeypatch.setattr(models, "fused_stack", self._stack(models.fused_stack))

    def _op(self, name, fn):
        def f(*args, **kw):
            ret = fn(*args, **kw)
            if self.cur is not None:
                self.cur.append((name, args, kw, ret))
            return ret
        return f

    def _stack(self, fn):
        def f(seq, *args, **kw):
            self.cur = []
            ret = fn(seq, *args, **kw)
            tapped = ret[1] if isinstance(seq, (tuple, list)) else None
            rows, first, tap_row = [], 0, None
            for name, a, k, out in self.cur:
                x = a[1] if name == "gemm" else a[0]
                if name == "gemm":
                    n_out, in_place, writes = out.shape[1], None, []
                else:
                    drawn = name == "reslayer_split_decode" or k.get("decode") is not None
                    n_out = 192 if drawn else out.shape[1]
                    in_place = isinstance(x, torch.Tensor) and x.data_ptr() == out.data_ptr()
                    writes = [t for t in (out, k.get("tap")) if t is not None]
                if tapped is not None and any(t.data_ptr() == tapped.data_ptr() for t in writes):
                    tap_row = len(rows)
                rows.append([name, first, k.get("chain", 0) or 0, n_out, False, in_place])
                first += 1 + rows[-1][2]
            if tap_row is not None:
                rows[tap_row][4] = True
            self.launches += [tuple(r) for r in rows]
            self.cur = None
            return ret
        return f


def _same(got, want):
    """Recorded launches against the table: GEMM layers by (op, first layer, chain, n_out) only."""
    if len(got) != len(want):
        return False
    return all(g[:4] == w[:4] if g[0] == "gemm" else g == w for g, w in zip(got, want))


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return scenario(torch.device("cuda:0"))


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_launch_sequence(case, arith, env, monkeypatch):
    from cppf2_amd import models
    monkeypatch.setattr(models, "MLP_ARITH", arith)
    rec = _Recorder(monkeypatch)
    with torch.no_grad():
        run_case(case, env)
    assert _same(rec.launches, EXPECTED[case][arith]), rec.launches


def _launch_args(monkeypatch, op):
    """Arguments of every call of ops.<op> from now on."""
    from cppf2_amd import ops
    seen, fn = [], getattr(ops, op)

    def f(*a, **kw):
        seen.append(a)
        return fn(*a, **kw)
    monkeypatch.setattr(ops, op, f)
    return seen


@pytest.mark.gpu
def test_in_place_weight_updates_re_pack_the_cross_stack_and_folded_launches(env, monkeypatch):
    """A logit-head weight updated in place: the tapped launch (tuple encoder into logit head) runs a re-packed stream and its
    output changes.  A parameter of the DINO fold updated in place (desc_pair_transform's bias): the table-fed first launch runs
    re-folded biases and its output changes."""
    from cppf2_amd import models
    monkeypatch.setattr(models, "MLP_ARITH", "split")
    shot, dino = env["shot"], env["dino"]
    pts, nrm, feat, idx, pt_off, tup_off = (env[k] for k in ("pts", "nrm", "feat", "idx", "pt_off", "tup_off"))
    taps = _launch_args(monkeypatch, "reslayer_split")
    firsts = _launch_args(monkeypatch, "reslayer_split_sumencode")
    saved = {k: v.clone() for k, v in list(shot.state_dict().items()) + [("dp." + k, v) for k, v in dino.desc_pair_transform.state_dict().items()]}
    try:
        with torch.no_grad():
            cls0, _ = shot.heads_from_tuples(pts, idx, feat, nrm, pt_off, tup_off, lazy_scale=True)
            wq0 = taps[0][1].clone()
            shot.logit_encoder[0].fc1.weight.mul_(1.5)
            cls1, _ = shot.heads_from_tuples(pts, idx, feat, nrm, pt_off, tup_off, lazy_scale=True)
            assert not torch.equal(taps[-2][1], wq0) and not torch.equal(cls0, cls1)
            d0, _ = dino.heads_from_tuples(pts, env["desc"], idx, pt_off, tup_off, lazy_scale=True)
            b0 = firsts[0][3].clone()
            dino.desc_pair_transform.bias.add_(0.5)          # folded into the first launch's biases (its stream holds the head columns)
            d1, _ = dino.heads_from_tuples(pts, env["desc"], idx, pt_off, tup_off, lazy_scale=True)
            assert not torch.equal(firsts[-1][3], b0) and not torch.equal(d0, d1)
    finally:
        with torch.no_grad():
            shot.load_state_dict({k: v for k, v in saved.items() if not k.startswith("dp.")})
            dino.desc_pair_transform.load_state_dict({k[3:]: v for k, v in saved.items() if k.startswith("dp.")})


# ------------------------------------------------------------------------------------------------------------------------------
# the same table from the planner alone, on the CPU
# ------------------------------------------------------------------------------------------------------------------------------
def _planned_calls(case, arith, shot, dino):
    """The fused_stack calls of run_case(case) as (stacks, MlpCall, fold), in order."""
    from cppf2_amd import models
    Call = models.MlpCall
    mlp, dmlp = (shot.tuple_encoder, shot.logit_encoder), (dino.tuple_encoder, dino.logit_encoder)
    kernel = arith != "native"
    rows = (mlp, Call(width=360), None)
    if case in ("shot_tuples_decode", "shot_tuples", "shot_tuples_scale"):
        calls = [(mlp, Call(gather="encode", heads=40, slots=5, table=64, decode=case == "shot_tuples_decode"), None) if kernel else rows]
        return calls + ([(shot.scale_encoder, Call(width=256), None)] if case == "shot_tuples_scale" else [])
    if case == "shot_sum_tables":
        return [(mlp, Call(gather="sumgather", heads=40, slots=5, table=5 * 256), shot.first_layer_fold(64, 5)) if kernel else rows]
    if case == "shot_separate_encode":
        return [(mlp, Call(gather="gather", heads=40, slots=5, table=64), None) if kernel else rows]
    if case == "shot_heads_rows":
        return [rows, (shot.scale_encoder, Call(width=256), None)]
    if case == "dino_tuples_decode":
        if not kernel:
            return [(dmlp, Call(width=288), None)]
        return [(dmlp, Call(gather="sumencode", heads=32, slots=5, table=5 * 256, decode=True), dino.first_layer_fold(5))]
    if case == "scale_rows_tail":
        return [(shot.scale_encoder, Call(gather="gather", heads=0, slots=1, table=256, tail=True) if kernel else Call(width=256), None)]
    if case == "logit_keep_input":
        return [(shot.logit_encoder, Call(width=256, keep_input=True), None)]
    if case == "misaligned_input":
        return [(shot.scale_encoder, Call(width=256, aligned=False), None), (shot.logit_encoder, Call(width=256, aligned=False), None)]
    raise KeyError(case)


@pytest.mark.parametrize("arith", ARITHS)
def test_planner_gives_the_launch_table(arith):
    from cppf2_amd import models
    from cppf2_amd.config import load_config
    cfg = load_config("config", "config", ["category=bottle"])
    torch.manual_seed(0)
    shot, dino = models.BeyondCPPFShot(cfg), models.BeyondCPPFDino(cfg)
    with torch.no_grad():
        for case in sorted(EXPECTED):
            got = []
            for stacks, call, fold in _planned_calls(case, arith, shot, dino):
                got += [(e.op, e.first, e.chain, e.n_out, e.tapped, e.out == "inplace")
                        for e in models.plan_launches(stacks, call, arith, fold).launches]
            assert got == EXPECTED[case][arith], (case, got)


def test_plans_follow_the_weights():
    """fused_stack's plan cache: one entry per call description and arithmetic, rebuilt when any parameter it reads changes in place
    -- either stack of a cross-stack call, or the fold of a table-fed first layer."""
    from cppf2_amd import models
    from cppf2_amd.config import load_config
    cfg = load_config("config", "config", ["category=bottle"])
    torch.manual_seed(0)
    dino = models.BeyondCPPFDino(cfg)
    call = models.MlpCall(gather="sumgather", heads=32, slots=5, table=5 * 256)
    stacks = (dino.tuple_encoder, dino.logit_encoder)
    with torch.no_grad():
        fold = dino.first_layer_fold(5)
        p0 = models.plan_launches(stacks, call, "split", fold)
        assert dino.first_layer_fold(5) is fold                                      # cached while nothing changes
        dino.desc_pair_transform.bias.add_(1.0)
        fold1 = dino.first_layer_fold(5)
        assert fold1 is not fold and fold1.stamp != fold.stamp
        p1 = models.plan_launches(stacks, call, "split", fold1)
        assert not torch.equal(p0.launches[0].weights[1], p1.launches[0].weights[1])     # the folded bias moved
        dino.logit_encoder[0].fc1.weight.mul_(2.0)
        p2 = models.plan_launches(stacks, call, "split", fold1)
        assert not torch.equal(p1.launches[1].weights[0], p2.launches[1].weights[0])     # the tapped launch runs into the logit head
        assert torch.equal(p1.launches[0].weights[0], p2.launches[0].weights[0])
