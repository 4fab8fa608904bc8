"""The tuple MLPs of CPPF++: plain torch modules (training, checkpoints, the reference's state-dict layout) whose inference
runs through the library's matrix-core kernels (fused_stack), with the tuple encode (prepare_tuple_inputs) and the bin draw
feeding / draining them in-kernel.

State-dict key layout is the reference's (train_shot.py:19-73, train_dino.py:21-89:
`shot_encoder.N.fc1.weight`, `tuple_encoder.N.fc0.bias`, `logit_encoder...`, `scale_encoder...`,
`desc_transform.*`, `desc_pair_transform.*`), so a Lightning checkpoint's `state_dict` loads with
load_reference_checkpoint().
"""
from __future__ import annotations

import os
from itertools import combinations
from typing import NamedTuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


class ResLayer(nn.Module):
    """Residual 2-layer block, no norm, no dropout (train_shot.py:19-45 with bn=False, dropout=False)."""

    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.fc1 = nn.Linear(dim_in, dim_out)
        self.fc2 = nn.Linear(dim_out, dim_out)
        self.fc0 = nn.Linear(dim_in, dim_out) if dim_in != dim_out else None

    def forward(self, x):
        skip = x if self.fc0 is None else self.fc0(x)
        return self.fc2(F.relu(self.fc1(x))) + skip


def _stack(dims):
    return nn.Sequential(*[ResLayer(dims[i], dims[i + 1]) for i in range(len(dims) - 1)])


# Arithmetic of the inference MLPs on the GPU: "split" = every ResLayer as one kernel on the bf16 matrix cores with each
# float32 operand split exactly into three bf16 values (cppf_reslayer_split: error vs float64 within 3 x a float32 GEMM's, 2-3x the rate of
# the f32-input matrix instruction); "native" = f32-input matrix cores (library GEMMs + cppf_reslayer128).
# "split16" = the same kernels in f16x2 arithmetic (fp16 operand pairs, three products: half the matrix-core work, float32-GEMM
# level error against float64, fp16's operand range; ops.reslayer_split16) -- an option, not the default.
MLP_ARITH = os.environ.get("CPPF_MLP_ARITH", "split")


def _kernel_arith():
    """True when the ResLayers run as the library's matrix-core kernels (either operand split)."""
    return MLP_ARITH in ("split", "split16")


def split_bf16(w):
    """float32 tensor -> bfloat16 [3, ...]: w == hi + mid + lo exactly (round-to-nearest-even each, exact remainders)."""
    w = w.detach().float()
    hi = w.to(torch.bfloat16)
    r1 = w - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    return torch.stack([hi, mid, lo])


def split_f16(w):
    """float32 tensor -> float16 [2, ...]: hi = RNE(w), lo = RNE(w - hi): w to 22-23 significant bits (f16x2 arithmetic)."""
    w = w.detach().float()
    hi = w.to(torch.float16)
    lo = (w - hi.float()).to(torch.float16)
    return torch.stack([hi, lo])


def f16_scale(*weights):
    """The power of two the weights of one f16x2 launch are multiplied by: the largest |w| lands in [2^12, 2^13)."""
    import math
    m = max(float(w.detach().abs().max()) for w in weights if w is not None)
    return 2.0 ** (13 - math.ceil(math.log2(m))) if m > 0 and math.isfinite(m) else 1.0


def pack_split(w1, w0, w2, k_in, chain=(), arith="bf16x3", scale=1.0):
    """The weight stream cppf_reslayer_split consumes for one ResLayer (w1 [N, K], w0 [N, K] or None, w2 [N, N] as
    nn.Linear stores them; k_in >= K = the columns of x the kernel reads, the extra ones get zero weights), optionally
    followed by the identity layers `chain` = [(w1_l [N, N], w2_l [N, N]), ...] of the same width.
    One operand fragment = 64 lanes x 8 bf16; lane = 32 g + i multiplies output feature 32 u + i of tile u; a tile is its
    (hi, mid, lo) fragments; a K step (16 input features) of a product is its tiles one after the other:
      first product, step s: lane half g holds input features 16 s + 8 g + j, j < 8; tiles = the N/32 tiles of W1 and, for
        a projection layer, the N/32 tiles of W0 behind them (one pass over x computes both);
      second product (W2), step (t, s') over the hidden features in the accumulator order of the first product:
        lane half g holds hidden features 32 t + 16 s' + 4 g + (j & 3) + 8 (j >> 2);
      then per chained layer W1_l and W2_l, both in that accumulator feature order (their input is the previous layer's
      output tiles in registers).
    arith="f16x2" (cppf_reslayer_split16): the same order with (hi, lo) fp16 fragments of scale x the weights."""
    n = w1.shape[0]
    nt = n // 32
    ks1 = (k_in + 15) // 16
    dev = w1.device
    if arith == "f16x2":
        pc, split = 2, (lambda w: split_f16(w * scale))
    else:
        pc, split = 3, split_bf16

    def pack_x(w, tiles):
        s = split(F.pad(w.detach().float(), (0, ks1 * 16 - w.shape[1])))
        return s.reshape(pc, tiles, 32, ks1, 2, 8).permute(3, 1, 0, 4, 2, 5).reshape(-1)      # [s, u, slice, g, i, j]

    def pack_h(w):
        t = torch.arange(nt, device=dev).view(nt, 1, 1, 1)
        sp = torch.arange(2, device=dev).view(1, 2, 1, 1)
        g = torch.arange(2, device=dev).view(1, 1, 2, 1)
        j = torch.arange(8, device=dev).view(1, 1, 1, 8)
        col = (32 * t + 16 * sp + 4 * g + (j & 3) + 8 * (j >> 2)).reshape(-1)
        s = split(w)[:, :, col]
        return s.reshape(pc, nt, 32, nt, 2, 2, 8).permute(3, 4, 1, 0, 5, 2, 6).reshape(-1)    # [t, s', u, slice, g, i, j]

    parts = [pack_x(w1, nt) if w0 is None else pack_x(torch.cat([w1, w0]), 2 * nt), pack_h(w2)]
    for w1_l, w2_l in chain:
        assert w1_l.shape == (n, n) and w2_l.shape == (n, n)
        parts += [pack_h(w1_l), pack_h(w2_l)]
    return torch.cat(parts).contiguous()


def pack_linear(w, k_in, arith="bf16x3", scale=1.0):
    """The weight stream cppf_linear_split consumes for out = x W^T (w [n_out, K] as nn.Linear stores it, n_out a multiple of
    256, k_in >= K the columns of x the kernel reads): per column group of 256 outputs the first-product segment of pack_split
    (K steps of 8 tiles, operand pieces per tile), the groups one after the other."""
    n, k = w.shape
    assert n % 256 == 0 and k_in >= k
    ks1 = (k_in + 15) // 16
    pc, split = (2, (lambda t: split_f16(t * scale))) if arith == "f16x2" else (3, split_bf16)
    s = split(F.pad(w.detach().float(), (0, ks1 * 16 - k)))                         # [pc, n, ks1 * 16]
    return s.reshape(pc, n // 256, 8, 32, ks1, 2, 8).permute(1, 4, 2, 0, 5, 3, 6).reshape(-1).contiguous()   # [grp, s, u, slice, g, i, j]


def _stamp(params):
    """Weight versions of `params`: changes when any of them is updated in place (version counter) or moved (data pointer)."""
    return tuple((p.data_ptr(), p._version) for p in params)


def _cached(owner, key, stamp, build):
    """build(), cached on `owner` under `key` and rebuilt when `stamp` (the _stamp of every parameter build() reads) changes: the one
    weight-version cache of this module (folded biases, launch plans with their packed streams, folds, Linear streams)."""
    cache = owner.__dict__.setdefault("_weight_cache", {})
    hit = cache.get(key)
    if hit is None or hit[0] != stamp:
        hit = cache[key] = (stamp, build())
    return hit[1]


def _linear_stream(w, k_in, arith):
    """(cppf_linear_split stream of w, weight scale or None) in `arith`."""
    if arith == "split16":
        sc = f16_scale(w)
        return pack_linear(w, k_in, arith="f16x2", scale=sc), sc
    return pack_linear(w, k_in), None


class _FoldedFirstLayer:
    """A tuple encoder's first ResLayer (a projection layer) on rows [heads | s] with s linear in per-point vectors p of the tuple's
    points, s = s0 + sum_i E_i p[idx_i]: the per-point parts of x W1^T and x W0^T are moved into per-point slot tables
        tables[n, i] = [A_i p_n | C_i p_n],   A_i = W1[:, s-columns] E_i,   C_i = W0[:, s-columns] E_i      (128 + 128 floats)
    (ops.linear_split with `wq_tab`), the constant parts into the biases, and the layer's own products shrink to the head columns
    (w1_heads / w0_heads).  Algebraically the same layer; the products are folded in float64 and rounded to float32 once.
    stamp: the weight versions it was folded from (part of the stamp of every launch plan it feeds)."""

    def __init__(self, stamp, a_list, c_list, w1_heads, w0_heads, b1_add=None, b0_add=None):
        self.stamp = stamp
        self.slots = len(a_list)
        self.dp = a_list[0].shape[1]
        self.tab_w = torch.cat([torch.cat([a, c]) for a, c in zip(a_list, c_list)]).float().contiguous()     # [slots * 256, dp]
        self.w1_heads, self.w0_heads = w1_heads.float().contiguous(), w0_heads.float().contiguous()       # [128, head columns]
        self.b1_add, self.b0_add = b1_add, b0_add

    def table_stream(self):
        """(packed stream of the table weights, weight scale or None) in the current arithmetic."""
        return _cached(self, ("table_stream", MLP_ARITH), self.stamp, lambda: _linear_stream(self.tab_w, self.dp, MLP_ARITH))

    def tables(self, p):
        """[points, slots * 256] from the per-point vectors p [points, dp] (float32, device)."""
        wq, sc = self.table_stream()
        return ops.linear_split(p, wq, None, self.slots * 256, scale=sc)


def _fused_plan(seq):
    """(layers, c): per layer (W1^T, b1', W0^T | None, b0', W2^T) with the pending-offset algebra of fused_stack applied once, and
    the offset c still pending behind the last layer (None when it is a projection layer); rebuilt when a parameter changes."""
    def build():
        layers, c = [], None
        with torch.no_grad():
            for layer in seq:
                w1, b1, w2, b2 = layer.fc1.weight, layer.fc1.bias, layer.fc2.weight, layer.fc2.bias
                if c is not None:
                    b1 = torch.addmv(b1, w1, c)
                if layer.fc0 is not None:
                    b0 = layer.fc0.bias + b2
                    if c is not None:
                        b0 = torch.addmv(b0, layer.fc0.weight, c)
                    layers.append((w1.t(), b1.clone(), layer.fc0.weight.t(), b0, w2.t()))
                    c = None
                else:
                    layers.append((w1.t(), b1.clone(), None, None, w2.t()))
                    c = b2.clone() if c is None else c + b2
        return layers, c
    return _cached(seq, "fused_plan", _stamp(seq.parameters()), build)


def _decode_fits(layers, c):
    """The fused bin draw's condition on a stack: a 192-wide projection layer (6 x 32 bins) with a multiple of 8 inputs last,
    nothing pending behind it."""
    w1t, _, w0t, _, _ = layers[-1]
    return w0t is not None and w1t.shape[1] == 192 and w1t.shape[0] % 8 == 0 and c is None


def _tail_fits(k_in, n_out, proj):
    """A layer cppf_reslayer_tail evaluates: at most 8 outputs, a multiple of 4 inputs, a projection or an equal-width skip."""
    return n_out <= 8 and k_in % 4 == 0 and (proj or k_in == n_out)


class MlpCall(NamedTuple):
    """What the launches of fused_stack depend on besides the weights and the arithmetic (the key of its plan cache)."""
    width: int = 0              # columns of x (0: gathered first layer)
    aligned: bool = True        # x float32, unit column stride, row stride a multiple of 4, 16-byte aligned: the split kernels read it
    contiguous: bool = True     # x float32 and contiguous: cppf_reslayer128 reads it
    gather: str | None = None   # first layer's input: "gather" | "encode" | "sumgather" | "sumencode" (ops.reslayer_split_<form>)
    heads: int = 0              # head columns of the gathered rows
    slots: int = 0              # gathered points per row
    table: int = 0              # columns of the gathered table
    decode: bool = False
    tail: bool = False
    keep_input: bool = False


class Launch(NamedTuple):
    """One launch of a plan."""
    op: str           # the ops function it calls; "gemm": the library-GEMM triple of a native layer
    first: int        # its first layer, counted over both stacks
    chain: int        # identity layers chained behind it in the same launch
    n_out: int
    weights: tuple    # split launches: (stream, first biases of its layers, skip bias, weight scale | None);
                      # reslayer128_: (W1, b1, W2); reslayer_tail: (W1, b1, W0 | None, b0, W2); gemm: (W1^T, b1, W0^T | None, b0, W2^T)
    out: str          # "inplace" | "new" (buffer) | "tap" (new buffer + the first layer's own) | "caller" (decode's bins, tail's out)
    tapped: bool      # it produces the tapped activation (its tap buffer when out == "tap", else its output)


class LaunchPlan(NamedTuple):
    launches: tuple
    offset: torch.Tensor | None     # pending bias offset added to the result at the end
    tap: int | None                 # tapped layer (the first stack's last one)


_ENCODE_OPS = ("reslayer_split_encode", "reslayer_split_sumencode")


def _chain_length(layers, li, tap, k_in=None, proj=False):
    """Identity layers of layer li's width that one launch chains behind it: at most 15, each accepted by
    ops.reslayer_split_supported(k_in, width, proj, chain) (k_in None: not asked), cut at the tapped layer unless it starts there."""
    n = layers[li][0].shape[1]
    chain = 0
    while (li + 1 + chain < len(layers) and chain < 15 and layers[li + 1 + chain][2] is None
           and layers[li + 1 + chain][0].shape == (n, n)
           and (k_in is None or ops.reslayer_split_supported(k_in, n, proj, chain + 1))):
        chain += 1
    if tap is not None and li < tap <= li + chain:
        return tap - li
    return chain


def plan_launches(seq, call, arith, fold=None):
    """The ordered launches of fused_stack(seq, ...) for the call `call` (MlpCall) in arithmetic `arith` -- every launch decision
    of the executor, with the packed weight streams.  seq: a stack or (stack_a, stack_b) (tapped at stack_a's last layer); fold:
    the _FoldedFirstLayer of a table-fed first layer.  Pure: reads the weights and the library's kernel coverage only."""
    kernel = arith in ("split", "split16")
    if isinstance(seq, (tuple, list)):
        layers_a, c_a = _fused_plan(seq[0])
        assert c_a is None, "the first stack must end in a projection layer"
        layers_b, c = _fused_plan(seq[1])
        layers, tap = layers_a + layers_b, len(layers_a) - 1
    else:
        (layers, c), tap = _fused_plan(seq), None
    last = len(layers) - 1

    def split(op, li, chain, k_in, n_out, out, first=None, add=(None, None)):
        """A split-arithmetic launch of layers li .. li + chain reading k_in columns (first / add: a folded first layer)."""
        w1t, b1, w0t, b0, w2t = layers[li] if first is None else first
        b1 = b1 if add[0] is None else b1 + add[0]
        b0 = b0 if add[1] is None else b0 + add[1]
        rest = layers[li + 1:li + 1 + chain]
        pairs = [(e[0].t(), e[4].t()) for e in rest]
        biases = torch.cat([b1] + [e[1] for e in rest])
        if arith == "split16":
            sc = f16_scale(w1t, w0t, w2t, *[w for pair in pairs for w in pair])
            wq = pack_split(w1t.t(), None if w0t is None else w0t.t(), w2t.t(), k_in, chain=pairs, arith="f16x2", scale=sc)
            weights = (wq, (biases * sc).contiguous(), None if b0 is None else (b0 * sc).contiguous(), sc)
        else:
            weights = (pack_split(w1t.t(), None if w0t is None else w0t.t(), w2t.t(), k_in, chain=pairs), biases.contiguous(), b0, None)
        return Launch(op, li, chain, n_out, weights, out, tap is not None and li <= tap <= li + chain)

    launches = []
    li, width, aligned, contiguous = 0, call.width, call.aligned, call.contiguous
    if call.gather is not None:
        # the first layer reads its rows itself: [heads | table[gidx_0] | ...] or, table-fed, heads plus the slot tables' rows
        form = call.gather
        if form in ("encode", "sumencode") and not (arith == "split" and ops.reslayer_split_encode_supported(call.slots, 128)):
            form = form.replace("encode", "gather")            # the head columns come from an array (TupleSource.heads)
        w1t, b1, w0t, b0, w2t = layers[0]
        first, add = None, (None, None)
        if fold is not None:
            k_in = call.heads
            assert kernel and w0t is not None and w1t.shape[1] == 128 and k_in % 8 == 0, "table-fed first layer: see sum_supported"
            first, add = (fold.w1_heads.t(), b1, fold.w0_heads.t(), b0, w2t), (fold.b1_add, fold.b0_add)
        else:
            k_in = call.heads + call.slots * call.table
            assert kernel and w0t is not None and w1t.shape == (k_in, 128), "gathered first layer: see gather_supported"
        op = "reslayer_split16" if (form == "gather" and arith == "split16") else "reslayer_split_" + form
        chain = 0 if tap == 0 else _chain_length(layers, 0, tap)          # (the gathering launch has no second output)
        launches.append(split(op, 0, chain, k_in, 128, "new", first, add))
        li, width, aligned, contiguous = 1 + chain, 128, True, True
    while li < len(layers):
        w1t, b1, w0t, b0, w2t = layers[li]
        n_out, proj = w1t.shape[1], w0t is not None
        prev = launches[-1] if launches else None
        # an identity layer must not overwrite the caller's x (keep_input) or the tapped activation
        keep = (li == 0 and call.keep_input) or (prev is not None and prev.tapped and prev.out != "tap")
        if call.decode and li == last:
            assert kernel and _decode_fits(layers, c), "fused bin draw: see decode_supported"
            launches.append(split("reslayer_split16" if arith == "split16" else "reslayer_split_decode", li, 0, width, n_out, "caller"))
            return LaunchPlan(tuple(launches), None, tap)
        if kernel and aligned and width >= w1t.shape[0] and ops.reslayer_split_supported(width, n_out, proj):
            # the layer and the identity layers of its width behind it, while they fit one kernel: the activation stays in registers
            chain = _chain_length(layers, li, tap, width, proj)
            out = "tap" if (tap == li and chain > 0) else "inplace" if not (proj or keep) else "new"
            launch = split("reslayer_split16" if arith == "split16" else "reslayer_split", li, chain, width, n_out, out)
        elif (kernel and aligned and width >= w1t.shape[0] and _tail_fits(w1t.shape[0], n_out, proj)
              and (call.tail or c is None or li < last)):
            # a layer too narrow for a matrix-core tile (the scale head's 64 -> 3): cppf_reslayer_tail, which also scatters its rows
            scatter = call.tail and li == last
            assert not scatter or c is None
            launch = Launch("reslayer_tail", li, 0, n_out, (w1t.t(), b1, None if w0t is None else w0t.t(), b0, w2t.t()),
                            "caller" if scatter else "new", tap == li)
        elif not proj and w1t.shape == (128, 128) and width == 128 and contiguous and not (li == 0 and call.keep_input):
            # 128-wide identity layer: both products, the bias, the ReLU and the residual add in one kernel (cppf_reslayer128)
            launch = Launch("reslayer128_", li, 0, n_out, (w1t.t(), b1, w2t.t()), "new" if keep else "inplace", tap == li)
        else:
            launch = Launch("gemm", li, 0, n_out, (w1t, b1, w0t, b0, w2t), "inplace" if not (proj or keep) else "new", tap == li)
        launches.append(launch)
        if launch.out != "inplace":
            aligned = contiguous = True
        elif width > w1t.shape[0]:
            contiguous = False                       # (a column slice of the input, updated in place)
        li, width = li + 1 + launch.chain, n_out
    return LaunchPlan(tuple(launches), c, tap)


def _describe(x, gather, decode, tail, keep_input):
    """The MlpCall of a fused_stack call."""
    flags = dict(decode=decode is not None, tail=tail is not None, keep_input=bool(keep_input))
    if gather is None:
        f32 = x.dtype == torch.float32
        return MlpCall(width=x.shape[1], aligned=f32 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0,
                       contiguous=f32 and x.is_contiguous(), **flags)
    heads, gidx, table = gather[:3]
    source = isinstance(heads, ops.TupleSource)
    # the head columns are built inside the first launch where that kernel exists (cppf_reslayer_split_encode: the SHOT model's pair
    # features; cppf_reslayer_split_sumencode: the DINO model's coordinate block in front of its slot tables)
    if len(gather) > 3:
        form = "sumencode" if source and heads.nrm is None else "sumgather"
    else:
        form = "encode" if source and heads.nrm is not None else "gather"
    return MlpCall(gather=form, heads=heads.shape[1], slots=heads.k if source else gidx.shape[1], table=table.shape[1], **flags)


def fused_stack(seq, x, keep_input=False, gather=None, decode=None, tail=None):
    """Inference-only execution of a stack of ResLayers (train_shot.py:19-45) on the matrix cores.
    MLP_ARITH == "split" (default): every layer whose shape the kernel covers -- widths 64 / 128 / 192 / 256, input columns
    a multiple of 8 -- runs as ONE cppf_reslayer_split launch together with the identity layers of the same width behind it
    (the activation stays in registers across the chain); split-bf16 arithmetic on exact float32 operands.
    MLP_ARITH == "native", and layers outside that coverage (the scale head's 64 -> 3 output layer): library GEMMs with the
    elementwise work folded into their epilogues --
      h   = relu(x W1^T + b1)            one GEMM, bias+ReLU epilogue (torch._addmm_activation)
      out = x W0^T + (b0 + b2)           one GEMM, bias epilogue          (layers with a projection skip)
      out += h W2^T                      one GEMM, beta = 1, in place
    -- and 128-wide identity layers as cppf_reslayer128 (f32-input matrix cores, h never leaves the registers).
    In both modes an identity layer's output bias b2 is not added to the activation but carried as a pending per-channel
    offset c (true activation = x + c) and folded into the biases of the next layer (b1 + W1 c, b0 + W0 c), which is
    algebraically the same network; every stack of the reference's models ends in a projection layer, which absorbs the
    pending offset.  An identity first layer overwrites `x` unless keep_input is set.
    Plan and executor: plan_launches decides every launch of a call -- which ops function, which layers it chains, where the
    tap lands, which buffer it writes -- with the packed weight streams; the plan is cached per call description (MlpCall) and
    arithmetic on the first stack under one weight stamp of every parameter it reads (both stacks, the fold's weights), so any
    in-place update or move of a weight re-plans.  This function looks the plan up and runs it.
    gather = (heads [T, H], gidx int32 [T, k], table [points, F]) instead of x: the rows [heads | table[gidx[:, 0]] | ...] are
    read by the first layer's kernel itself (ops.reslayer_split_gather; split arithmetic, 128-wide projection first layer);
    heads may be an ops.TupleSource (the head columns built by the first launch, ops.reslayer_split_encode).  gather = (heads,
    gidx, tables, fold): the per-point parts of the first products come from slot tables (fold: _FoldedFirstLayer).
    decode = (uniforms [T, 6], prior [T, 6, 32] | None, bins int32 [T, 6] | None): the stack's last layer (the logit head's
    192-wide projection layer) draws the bins in its epilogue instead of writing its logits (ops.reslayer_split_decode); the
    return value is then the bins.  Use decode_supported(seq, x) first.
    seq = (stack_a, stack_b): the two stacks run as one, returning (output of stack_b, output of stack_a): stack_a's last layer
    (a projection layer) and the identity layers that open stack_b share one kernel whose first layer's result is written to a
    buffer of its own (ops.reslayer_split(tap=...)) -- the tuple encoder into the logit head, whose input also feeds the scale
    head (train_shot.py:112-114): the 256-wide features are written once and not read back by the logit head.
    tail = (rows int32 [n], counts int32 [n / per_group], per_group, out [T, n_out]): the stack's last layer, when it is a narrow
    one (n_out <= 8: ops.reslayer_tail), writes row i of its result to out[rows[i]], skipping the padded entries of each
    group (VotingPipeline.kept_rows32 / kept_count / max_kept); returns `out`.  Use tail_supported(seq) first."""
    fold = gather[3] if gather is not None and len(gather) > 3 else None
    call = _describe(x, gather, decode, tail, keep_input)
    stacks = tuple(seq) if isinstance(seq, (tuple, list)) else (seq,)
    stamp = (_stamp(p for s in stacks for p in s.parameters()), None if fold is None else fold.stamp)
    plan = _cached(stacks[0], ("launch_plan", len(stacks), call, MLP_ARITH), stamp, lambda: plan_launches(seq, call, MLP_ARITH, fold))
    if gather is not None:
        heads, gidx, table = gather[:3]
        if isinstance(heads, ops.TupleSource) and plan.launches[0].op not in _ENCODE_OPS:
            heads, gidx = heads.heads()                 # this launch form reads the head columns from an array
    tapped = None
    for e in plan.launches:
        fn = getattr(ops, e.op, None)                   # (looked up per call: bench evidence swaps the ops functions for recorders)
        w = e.weights
        tap = None
        if e.first == 0 and gather is not None:
            if e.op in _ENCODE_OPS:
                x = fn(heads, table, *w[:3], 128, chain=e.chain)
            elif e.op == "reslayer_split16":
                x = fn(heads, *w[:3], 128, w[3], chain=e.chain, gather=(gidx, table))
            elif e.op == "reslayer_split_sumgather":
                x = fn(heads, gidx, table, *w[:3], 128, chain=e.chain, scale=w[3])
            else:
                x = fn(heads, gidx, table, *w[:3], 128, chain=e.chain)
        elif e.op == "reslayer_split_decode":
            x = fn(x, *w[:3], decode[0], prior=decode[1], bins=decode[2])
        elif e.out == "caller" and e.op == "reslayer_split16":
            x = fn(x, *w[:3], 192, w[3], decode=decode)
        elif e.op in ("reslayer_split", "reslayer_split16"):
            out = None if e.out == "inplace" else torch.empty((x.shape[0], e.n_out), dtype=torch.float32, device=x.device)
            if e.out == "tap":
                tap = torch.empty((x.shape[0], e.n_out), dtype=torch.float32, device=x.device)
            if e.op == "reslayer_split16":
                x = fn(x, *w[:3], e.n_out, w[3], out=out, chain=e.chain, tap=tap)
            else:
                x = fn(x, *w[:3], e.n_out, out=out, chain=e.chain, tap=tap)
        elif e.op == "reslayer_tail":
            t = tail if e.out == "caller" else None
            x = fn(x, *w, out=None if t is None else t[3], scatter_rows=None if t is None else t[0],
                   valid_count=None if t is None else t[1], per_group=0 if t is None else t[2])
        elif e.op == "reslayer128_":
            x = fn(x.clone() if e.out == "new" else x, *w)
        else:                                           # gemm
            w1t, b1, w0t, b0, w2t = w
            if x.shape[1] > w1t.shape[0]:               # zero-padded input columns (see BeyondCPPFDino.prepare_tuple_inputs)
                x = x[:, :w1t.shape[0]]
            h = torch._addmm_activation(b1, x, w1t)
            if w0t is not None:
                x = torch.addmm(b0, x, w0t).addmm_(h, w2t)
            elif e.out == "new":
                x = torch.addmm(x, h, w2t)              # same GEMM, written to a new tensor: the input survives
            else:
                x = x.addmm_(h, w2t)
        if e.tapped:
            tapped = tap if tap is not None else x
    if plan.offset is not None:
        x = x.add_(plan.offset)
    return x if plan.tap is None else (x, tapped)


def tail_supported(seq):
    """True when fused_stack(seq, ..., tail=...) can scatter the last layer's rows itself: split arithmetic, inference, a
    projection layer with at most 8 outputs and a multiple of 4 inputs last."""
    last = seq[len(seq) - 1]
    return (_kernel_arith() and not torch.is_grad_enabled() and last.fc0 is not None
            and _tail_fits(last.fc1.in_features, last.fc1.out_features, True))


def decode_supported(seq, x):
    """True when fused_stack(seq, x, decode=...) can draw the bins inside the stack's last layer: split arithmetic, inference,
    a 192-wide projection layer (6 x 32 bins) last, preceded by a projection or nothing pending (no carried bias offset)."""
    return _kernel_arith() and not torch.is_grad_enabled() and x.is_cuda and _decode_fits(*_fused_plan(seq))


class _EncodeShot(torch.autograd.Function):
    """HIP tuple encode with a backward for the per-point feature table (the only differentiable input:
    points and normals are data).  d feat[n] = sum over (tuple, slot) with idx == n of d out[:, slot block]."""

    @staticmethod
    def forward(ctx, points, idx, feat, normal):
        out = ops.encode_tuples_shot(points, idx, feat.detach(), normal)
        ctx.save_for_backward(idx)
        ctx.feat_shape = feat.shape
        return out

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        n, f = ctx.feat_shape
        k = idx.shape[1]
        head = k * (k - 1) // 2 * 4
        gf = torch.zeros((n, f), dtype=g.dtype, device=g.device)
        for s in range(k):
            gf.index_add_(0, idx[:, s].long(), g[:, head + s * f: head + (s + 1) * f])
        return None, None, gf, None


class _TupleHeads(nn.Module):
    """The heads both models put behind their tuple encoder (tuple_encoder -> logit_encoder / scale_encoder, train_shot.py:112-114,
    train_dino.py:130-132) and their inference on the library's kernels."""

    def heads(self, inputs, decode=None, lazy_scale=False):
        """(preds_cls [T,6,32], preds_scale [T,3]) from the tuple inputs; inference on the GPU runs the tuple encoder and the logit
        head as one chain of launches (fused_stack) with the tuple features tapped for the scale head.  decode: see
        BeyondCPPFShot.heads_from_tuples (None is returned in place of the logits when the bins were drawn).  lazy_scale=True
        (inference) returns (preds_cls, feat) instead: the scale head's output is only ever read for the pairs that survive the
        back-vote filter (eval.py:272, ~10 % of the tuples), so a caller can run scale_head() on just those rows of `feat` later --
        same rows through the same layers."""
        if not torch.is_grad_enabled() and inputs.is_cuda:
            return self._tuple_mlp(inputs, None, decode, lazy_scale)
        feat = self.tuple_encoder(inputs)
        preds_scale = self.scale_encoder(feat)
        preds_cls = self.logit_encoder(feat).reshape(feat.shape[0], 6, -1)
        return preds_cls, preds_scale

    def _tuple_mlp(self, x, gather, decode, lazy_scale):
        """fused_stack((tuple_encoder, logit_encoder), x, gather=gather) with the bins drawn by the last launch when
        decode_supported, then the scale head on the tapped tuple features unless lazy_scale: (logits | None, scales | features)."""
        probe = x if gather is None else gather[2]
        draw = decode if (decode is not None and decode_supported(self.logit_encoder, probe)) else None
        preds_cls, feat = fused_stack((self.tuple_encoder, self.logit_encoder), x, gather=gather, decode=draw)
        second = feat if lazy_scale else fused_stack(self.scale_encoder, feat)      # first layer projects: feat is left intact
        if draw is not None:
            return None, second
        return preds_cls.reshape(feat.shape[0], 6, -1), second

    def scale_head(self, feat_rows):
        """scale_encoder on a subset of tuple features (rows of the `feat` heads(lazy_scale=True) returned)."""
        if not torch.is_grad_enabled() and feat_rows.is_cuda:
            return fused_stack(self.scale_encoder, feat_rows)
        return self.scale_encoder(feat_rows)

    def scale_head_rows(self, feat, rows, scatter=None):
        """scale_head(feat[rows]) on the kept pairs only (eval.py:272 reads nothing else; it is the DINO model's scale that the
        reference keeps, eval.py:308-310), without materialising feat[rows]: the scale head's first layer (a 128-wide projection
        layer) reads the selected rows of `feat` through the gathering x-tile fetch of cppf_reslayer_split_gather (a table gather
        with no pair-feature block).  rows: int32 (or int64) [n] tuple rows.
        scatter = (counts int32 [n / per_group], per_group, out [T, 3]): the result rows are written to out[rows[i]] (padded entries
        of each group skipped) and `out` is returned -- by the head's last kernel where tail_supported: no index_put, no torch kernel."""
        first = self.scale_encoder[0]
        f = feat.shape[1]
        if (_kernel_arith() and not torch.is_grad_enabled() and feat.is_cuda and feat.is_contiguous()
                and first.fc0 is not None and first.fc1.out_features == 128 and first.fc1.in_features == f
                and f >= 8 and f & (f - 1) == 0 and feat.shape[0] < 2 ** 31):
            gidx = (rows if rows.dtype == torch.int32 else rows.to(torch.int32)).reshape(-1, 1)
            tail = None
            if scatter is not None and tail_supported(self.scale_encoder):
                tail = (gidx.reshape(-1), scatter[0], scatter[1], scatter[2])
            vals = fused_stack(self.scale_encoder, None, gather=(feat[:, :0], gidx, feat), tail=tail)
            if tail is not None:
                return vals
        else:
            vals = self.scale_head(feat[rows.long()])
        if scatter is None:
            return vals
        counts, per_group, out = scatter
        keep = (torch.arange(rows.numel(), device=rows.device) % per_group) < counts.repeat_interleave(per_group)
        out[rows.long()[keep]] = vals[keep]
        return out


class BeyondCPPFShot(_TupleHeads):
    """train_shot.py:48-122.  forward(points, point_idxs_all, shot_feat, normal) -> (preds_cls [T,6,32], preds_scale [T,3])."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        k = cfg.num_more + 2
        self.shot_encoder = _stack([352] + [128] * 5 + [64])
        input_dim = len(list(combinations(range(k), 2))) * 4 + k * 64
        self.tuple_encoder = _stack([input_dim] + [128] * 5 + [256])
        self.logit_encoder = _stack([256, 256, 256, 64 * 3])
        self.scale_encoder = _stack([256, 128, 64, 3])

    def prepare_tuple_inputs(self, points, point_idxs_all, shot_feat, normal):
        idx = point_idxs_all.to(torch.int32)
        if shot_feat.requires_grad:
            return _EncodeShot.apply(points, idx, shot_feat, normal)
        return ops.encode_tuples_shot(points, idx, shot_feat, normal)

    def gather_supported(self, feat_dim, k):
        """True when heads_from_tuples can feed the tuple encoder without materialising its input rows."""
        first = self.tuple_encoder[0]
        return (_kernel_arith() and not torch.is_grad_enabled() and first.fc0 is not None and first.fc1.out_features == 128
                and feat_dim >= 8 and feat_dim & (feat_dim - 1) == 0 and (k * (k - 1) // 2 * 4) % 8 == 0 and k <= 8
                and first.fc1.in_features == k * (k - 1) // 2 * 4 + k * feat_dim)

    def sum_supported(self, feat_dim, k):
        """True when heads_from_tuples(sum_tables=True) can feed the tuple encoder from per-point slot tables."""
        first = self.tuple_encoder[0]
        head = k * (k - 1) // 2 * 4
        return (_kernel_arith() and not torch.is_grad_enabled() and first.fc0 is not None and first.fc1.out_features == 128
                and feat_dim % 8 == 0 and head % 8 == 0 and k <= 8 and first.fc1.in_features == head + k * feat_dim)

    def first_layer_fold(self, feat_dim, k):
        """_FoldedFirstLayer of tuple_encoder[0] for rows [pair features | feat[idx_0] | ... | feat[idx_{k-1}]]
        (train_shot.py:75-83): slot i's table weights are the columns of fc1 / fc0 that multiply feat[idx_i] (no product to
        fold: the same multiplications as the row form, summed per slot first)."""
        first = self.tuple_encoder[0]
        stamp = _stamp(first.parameters())

        def build():
            head = k * (k - 1) // 2 * 4
            w1, w0 = first.fc1.weight.detach(), first.fc0.weight.detach()
            return _FoldedFirstLayer(stamp, [w1[:, head + i * feat_dim: head + (i + 1) * feat_dim] for i in range(k)],
                                     [w0[:, head + i * feat_dim: head + (i + 1) * feat_dim] for i in range(k)],
                                     w1[:, :head], w0[:, :head])
        return _cached(self, ("first_layer_fold", feat_dim, k), stamp, build)

    def heads_from_tuples(self, points, point_idxs_all, feat, normal, pt_off=None, tup_off=None, lazy_scale=False, decode=None,
                          sum_tables=False):
        """heads(prepare_tuple_inputs(...)) with the [T, 360] tuple rows never written: the first ResLayer's kernel computes the
        pair features (40 columns) of its rows from points / normals / the sampler's indices and reads the per-point descriptors
        `feat` itself (cppf_reslayer_split_encode; same values, same arithmetic, bit-identical logits).  Falls back to the materialised rows when the first layer has
        no gathering kernel (other widths, training, native arithmetic).
        sum_tables=True: the descriptor columns' products with the first layer's weights are evaluated once per point and slot
        (first_layer_fold) and summed into the kernel's accumulators: the same multiplications in another order (float32-level
        differences against the row form), 20 of the first product's 23 K steps fewer per tuple.
        decode = (uniforms [T, 6], prior [T, 6, 32] | None, bins int32 [T, 6]): the bins of eval.py:225-229 are drawn by the
        logit head's output layer into `bins` (e.g. VotingPipeline.bins) and None is returned in place of the logits -- only when
        decode_supported(); otherwise the logits are returned as usual and the caller decodes them."""
        idx = point_idxs_all.to(torch.int32)
        if not (points.is_cuda and self.gather_supported(feat.shape[1], idx.shape[1])):
            return self.heads(ops.encode_tuples_shot(points, idx, feat, normal, pt_off, tup_off), lazy_scale=lazy_scale)
        tuples = ops.TupleSource(points, idx, normal, pt_off, tup_off)
        if sum_tables and self.sum_supported(feat.shape[1], idx.shape[1]):
            # the descriptor columns' share of the first products, once per point and slot instead of once per tuple
            fold = self.first_layer_fold(feat.shape[1], idx.shape[1])
            heads, gidx = tuples.heads()
            src = (heads, gidx, fold.tables(feat.contiguous()), fold)
        else:
            # (round 5: the pair features are built by the first launch itself -- no per-tuple array between sampler and encoder)
            src = (tuples, None, feat.contiguous())
        return self._tuple_mlp(None, src, decode, lazy_scale)

    def encode_points(self, shot_feat):
        """shot_encoder over the per-point descriptors (train_shot.py:118)."""
        if not torch.is_grad_enabled() and shot_feat.is_cuda:
            return fused_stack(self.shot_encoder, shot_feat)
        return self.shot_encoder(shot_feat)

    def forward(self, points, point_idxs_all, shot_feat, normal):
        inputs = self.prepare_tuple_inputs(points, point_idxs_all, self.encode_points(shot_feat), normal)
        return self.heads(inputs)


class BeyondCPPFDino(_TupleHeads):
    """train_dino.py:58-133.  forward(points, point_descs, point_idxs_all).
    desc_transform is applied per point BEFORE the gather: same Linear on the same rows,
    1/5 of the FLOPs at T >> N and no [T,5,1024] temporary."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        k = cfg.num_more + 2
        d = 256
        self.ncoord = len(list(combinations(range(k), 2))) * 3
        self.tuple_encoder = _stack([self.ncoord + d] + [128] * 5 + [256])
        self.logit_encoder = _stack([256, 256, 256, 64 * 3])
        self.scale_encoder = _stack([256, 128, 64, 3])
        self.desc_transform = nn.Linear(1024, d)
        self.desc_pair_transform = nn.Linear(d * k, d)

    def prepare_tuple_inputs(self, points, point_descs, point_idxs_all):
        idx = point_idxs_all.to(torch.int32)
        T, k = idx.shape
        per_point = self.desc_transform(point_descs)                                   # [N,256]
        d = per_point.shape[1]
        if not torch.is_grad_enabled() and per_point.is_cuda:
            # Linear over the concatenation = sum of k per-point products: k GEMMs over N rows + a gather-add kernel
            # instead of a [T, k*256] gather and a K = k*256 GEMM over T rows (T/N = 5x the FLOPs, 6.5 GB at bench size)
            w = self.desc_pair_transform.weight                                        # [256, k*256]
            tables = torch.stack([per_point @ w[:, i * d:(i + 1) * d].t() for i in range(k)], 1).contiguous()
            # rows padded with zero columns to a multiple of 8 floats (286 -> 288): 16-byte aligned rows for the MLP kernels,
            # which give the extra columns zero weights (fused_stack)
            width = (self.ncoord + d + 7) // 8 * 8
            out = torch.empty((T, width), dtype=torch.float32, device=per_point.device)
            if width > self.ncoord + d:
                out[:, self.ncoord + d:] = 0
            ops.encode_tuples_coord(points, idx, out=out)
            ops.encode_tuples_dino(tables, self.desc_pair_transform.bias, idx, out, self.ncoord)
            return out
        gathered = per_point[idx.long().reshape(-1)].reshape(T, k * d)                 # cat_i desc_transform(desc[idx_i])
        desc_part = self.desc_pair_transform(gathered)
        coord = ops.encode_tuples_coord(points, idx)
        return torch.cat([coord, desc_part], -1)

    def sum_supported(self, k):
        """True when heads_from_tuples can run: every Linear of prepare_tuple_inputs on the library's matrix-core kernels and the
        tuple rows never formed (split arithmetic, inference, the reference's layer widths)."""
        first = self.tuple_encoder[0]
        d = self.desc_transform.out_features
        return (_kernel_arith() and not torch.is_grad_enabled() and first.fc0 is not None and first.fc1.out_features == 128
                and d == 256 and self.desc_transform.in_features % 8 == 0 and k <= 8
                and self.desc_pair_transform.in_features == k * d and self.desc_pair_transform.out_features == d
                and first.fc1.in_features == k * (k - 1) // 2 * 3 + d)

    def first_layer_fold(self, k):
        """_FoldedFirstLayer of tuple_encoder[0] for rows [coords | desc_pair_transform(cat_i q[idx_i])], q = desc_transform(desc)
        (train_dino.py:91-97): the Linear over the concatenation is a sum of k per-point products W_i q[idx_i] (W = [W_0 | ... ]),
        and the first ResLayer's fc1 / fc0 are linear too, so slot i's table weights are fc1[:, desc columns] W_i and
        fc0[:, desc columns] W_i (folded in float64, rounded to float32 once), desc_pair_transform's bias goes through the same
        columns into the layer's biases, and the layer's own products keep the 30 coordinate columns only."""
        first = self.tuple_encoder[0]
        stamp = _stamp(list(first.parameters()) + list(self.desc_pair_transform.parameters()))

        def build():
            nc, d = self.ncoord, self.desc_transform.out_features
            w1, w0 = first.fc1.weight.detach().double(), first.fc0.weight.detach().double()
            wp, bp = self.desc_pair_transform.weight.detach().double(), self.desc_pair_transform.bias.detach().double()
            return _FoldedFirstLayer(stamp, [w1[:, nc:] @ wp[:, i * d:(i + 1) * d] for i in range(k)],
                                     [w0[:, nc:] @ wp[:, i * d:(i + 1) * d] for i in range(k)], w1[:, :nc], w0[:, :nc],
                                     b1_add=(w1[:, nc:] @ bp).float(), b0_add=(w0[:, nc:] @ bp).float())
        return _cached(self, ("first_layer_fold", k), stamp, build)

    def transform_points(self, point_descs):
        """desc_transform over the per-point descriptors (train_dino.py:95; applied per point, before the gather) on the library's
        matrix-core Linear kernel: [N, 1024] -> [N, 256]."""
        lin = self.desc_transform

        def build():
            wq, sc = _linear_stream(lin.weight, lin.in_features, MLP_ARITH)
            return wq, (lin.bias.detach() if sc is None else lin.bias.detach() * sc).contiguous(), sc
        wq, bias, sc = _cached(self, ("transform_points", MLP_ARITH), _stamp(lin.parameters()), build)
        return ops.linear_split(point_descs, wq, bias, lin.out_features, scale=sc)

    def point_tables(self, point_descs, k):
        """Per-point slot tables [N, k * 256] of the folded first layer from the raw descriptors [N, 1024]: two library launches
        per batch (desc_transform, then the k folded slot products), no BLAS call, no [N, k, 256] stack copy."""
        return self.first_layer_fold(k).tables(self.transform_points(point_descs.contiguous()))

    def heads_from_tuples(self, points, point_descs, point_idxs_all, pt_off=None, tup_off=None, lazy_scale=False, decode=None,
                          tables=None):
        """heads(prepare_tuple_inputs(...)) with the [T, 286] tuple rows never written and every layer a kernel of the library:
        coordinate columns + global point indices (ops.encode_tuples_coord_heads), per-point slot tables (point_tables; pass
        `tables` to reuse them), and the first ResLayer summing its tuple's table rows into its accumulators
        (ops.reslayer_split_sumgather).  point_idxs_all are scene-local with pt_off / tup_off given (batches), global otherwise.
        lazy_scale / decode as BeyondCPPFShot.heads_from_tuples.  Falls back to heads(prepare_tuple_inputs(...)) when the
        kernels do not cover the configuration (training, native arithmetic, other widths)."""
        idx = point_idxs_all.to(torch.int32)
        k = idx.shape[1]
        if not (points.is_cuda and self.sum_supported(k)):
            if pt_off is not None:
                base = torch.repeat_interleave(pt_off[:-1], (tup_off[1:] - tup_off[:-1]).long()).to(torch.int32)
                idx = idx + base[:, None]
            return self.heads(self.prepare_tuple_inputs(points, point_descs, idx), decode=decode, lazy_scale=lazy_scale)
        fold = self.first_layer_fold(k)
        if tables is None:
            tables = fold.tables(self.transform_points(point_descs.contiguous()))
        # (round 5: the coordinate columns are built by the first launch itself -- no per-tuple array between sampler and encoder)
        tuples = ops.TupleSource(points, idx, None, pt_off, tup_off)
        return self._tuple_mlp(None, (tuples, None, tables, fold), decode, lazy_scale)

    def forward(self, points, point_descs, point_idxs_all):
        return self.heads(self.prepare_tuple_inputs(points, point_descs, point_idxs_all))


def load_reference_checkpoint(model, path):
    """Loads a Lightning checkpoint written by the reference's trainer (train_shot.py:139): weights live under
    ckpt['state_dict'] with the same key names as this module."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    sd = ckpt.get("state_dict", ckpt)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    if missing or unexpected:
        raise RuntimeError("checkpoint key mismatch: missing=%s unexpected=%s" % (missing, unexpected))
    return model
