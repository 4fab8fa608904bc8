"""The per-batch library behind eval.py's drivers (eval.py imports every name back): the vote of one batch of instances through
both models (run_ensemble) or through an object's pair-feature table (run_table), the pipeline cache they share, and the stages
every data mode repeats -- an instance's cloud from its mask, the stand-in descriptors, hypothesis verification and ICP after
the vote, and the report items they leave."""
import collections
import os

import numpy as np
import torch

from cppf2_amd import ops, shot
from cppf2_amd.pipeline import VotingPipeline


def needed_cells(pc, res):
    """Cells of the vote grid of one instance (train_dino.py:173-175: int32 truncation of the float32 extent / res, + 1)."""
    ext = (pc.max(0) - pc.min(0)).astype(np.float32) / np.float32(res)
    return int(np.prod(ext.astype(np.int64) + 1))


def too_wide(pc, res):
    """An instance wider than 1000 cells along an axis: the reference skips it (eval.py:199-200)."""
    return ((pc.max(0) - pc.min(0)).max() / res) > 1000


def instance_cloud(depth_m, K, mask, res, seed, pixels=False):
    """The cloud of one instance: the depth image (metres) back-projected through its mask (eval.py:185-189), one point per
    `res` voxel (eval.py:191-193), at most 50 000 points (eval.py:194-197); float32 [n,3] on the host, an empty mask giving an
    empty cloud.  seed: the down-sampling draw's and the cap's.  pixels: also the kept points' pixels, int64 [n,2] (row, col)."""
    pc, (rr, cc) = ops.backproject(depth_m, K, mask, return_device=True)
    if pc.shape[0]:
        keep = ops.downsample(pc, res, seed, return_device=True)
        pc = pc[keep]
        if pixels:
            rr, cc = rr[keep], cc[keep]
    pc = pc.cpu().numpy()
    idxs = np.stack([rr.cpu().numpy(), cc.cpu().numpy()], -1).astype(np.int64) if pixels else None
    if pc.shape[0] > 50000:
        sub = np.random.RandomState(seed).randint(pc.shape[0], size=50000)
        pc, idxs = pc[sub], idxs[sub] if pixels else None
    return (pc, idxs) if pixels else pc


def usable_cloud(depth_m, K, mask, cfg, seed, min_points=True):
    """instance_cloud at cfg.res as (cloud, None), or (None, why it cannot be voted on): `too_few_points` for fewer than a tuple
    takes (min_points=False: not checked, as the reference's own route), `too_large` for one that is too_wide (eval.py:200)."""
    pc = instance_cloud(depth_m, K, mask, cfg.res, seed)
    if min_points and pc.shape[0] < cfg.num_more + 2:
        return None, "too_few_points"
    if too_wide(pc, cfg.res):
        return None, "too_large"
    return pc, None


def stand_in_descriptors(n, gen):
    """DINOv2 features are inputs to the path (weights absent): float32 [n,1024] seeded unit vectors stand in for them, from a
    CPU generator -- the same numbers on every device.  gen: a torch.Generator to draw on from, or the seed of a fresh one."""
    if not isinstance(gen, torch.Generator):
        gen = torch.Generator(device="cpu").manual_seed(gen)
    return torch.nn.functional.normalize(torch.randn((n, 1024), generator=gen), dim=-1)


_SIDE_STREAMS = {}


def _side_streams(dev):
    """The two HIP streams the model passes of run_ensemble run on (one pair per device for the life of the process: scratch
    buffers keyed by stream are reused from call to call)."""
    key = str(torch.device(dev))
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
    return _SIDE_STREAMS[key]


_PIPES = {}                # batch geometry -> (pipe, twin | None, [scales_buf, scales_buf], workspace bytes); least recently used first
PIPE_CACHE_MAX = 4
PIPE_CACHE_BYTES = 16 << 30        # bound on the cached pipelines' vote workspaces (B x cells_cap x 4 bytes each, twice with a twin)


def _pipelines(dev, Ns, num_pairs, k, cfg, num_rots, angle_tol, backproj_ratio, imp_wt_margin, cap, two):
    """The VotingPipeline (+ its twin for the two-stream mode, + the [T, 3] scale buffers of the two passes) of one batch geometry,
    kept from call to call: a streaming evaluation calls run_ensemble once per batch and category, and building a pipeline means
    ~25 device allocations, the workspace, and host-to-device copies of the offsets, sphere bins, bin lookup table and rotation
    table -- per call, before.  Keyed by everything the buffers' sizes and tables depend on; at most PIPE_CACHE_MAX geometries are
    kept, and at most PIPE_CACHE_BYTES of vote workspace (real batches are ragged: a batch with new point counts -- the usual case
    on REAL275 chunks -- builds its own; the oldest entries are dropped BEFORE the new one is built, so the peak is the bound, not
    the bound plus one).  The cache pays for repeated geometries: the synthetic mode, the benchmarks, fixed-size crops.  The
    buffers of a cached pipeline are overwritten by the next call with the same geometry: a caller that keeps run_ensemble's
    `pipe` reads it before."""
    key = (str(torch.device(dev)), tuple(Ns), int(num_pairs), int(k), float(cfg.res), int(num_rots), float(angle_tol),
           float(backproj_ratio), float(imp_wt_margin), tuple(cfg.up), tuple(cfg.right), tuple(cfg.front), int(cap), bool(two))
    hit = _PIPES.pop(key, None)
    if hit is None:
        cost = len(Ns) * int(cap) * 4 * (2 if two else 1)
        while _PIPES and (len(_PIPES) >= PIPE_CACHE_MAX or sum(v[3] for v in _PIPES.values()) + cost > PIPE_CACHE_BYTES):
            del _PIPES[next(iter(_PIPES))]           # evict first: the new pipeline never coexists with more than the bound
        pipe = VotingPipeline(Ns, [num_pairs] * len(Ns), k=k, res=cfg.res, num_rots=num_rots, angle_tol=angle_tol,
                              backproj_ratio=backproj_ratio, imp_wt_margin=imp_wt_margin, cfg_up=cfg.up,
                              cfg_right=cfg.right, cfg_front=cfg.front, cells_cap=cap)
        bufs = [torch.zeros((pipe.Ttot, 3), dtype=torch.float32, device=dev) for _ in range(2)]
        hit = (pipe, pipe.twin() if two else None, bufs, cost)
    _PIPES[key] = hit
    return hit[:3]


def _vote_cap(pcs, cfg):
    """cells_cap of a batch's vote grids (a power of two >= 2^18); refuses an instance the reference skips (eval.py:200) and a
    batch whose grids do not fit."""
    for p in pcs:                                                                          # eval.py:200
        if too_wide(p, cfg.res):
            raise ValueError("instance larger than 1000 cells: the reference skips it (eval.py:200); drop it from the batch")
    cap = max(1 << 18, max(needed_cells(p, cfg.res) for p in pcs))
    cap = 1 << int(np.ceil(np.log2(cap)))
    if cap * len(pcs) > (1 << 33):
        raise ValueError("vote grids of %d cells x %d instances do not fit one batch; evaluate fewer instances per call" % (cap, len(pcs)))
    return cap


def _hypothesis_args(hypotheses, centre_peaks):
    """(hypotheses: None or int >= 1, centre_peaks: int >= 1) of run_ensemble / run_table, checked."""
    if hypotheses is not None:
        hypotheses = int(hypotheses)
        if hypotheses < 1:
            raise ValueError("hypotheses must be >= 1, not %d" % hypotheses)
    centre_peaks = int(centre_peaks)
    if centre_peaks < 1:
        raise ValueError("centre_peaks must be >= 1, not %d" % centre_peaks)
    if centre_peaks > 1 and hypotheses is None:
        raise ValueError("centre_peaks > 1 forms hypotheses per centre-vote peak: it needs hypotheses")
    return hypotheses, centre_peaks


def _pass_hypotheses(pp, hypotheses, centre_peaks, up_sym):
    """(H hypotheses of a pass from the peaks of its two votes, slot 0 = its assembled record; with centre_peaks > 1 also the
    list per centre-vote peak, peak 0's being the former, else None), right after the pass' vote: device tensors."""
    from cppf2_amd import verify
    hyps = verify.hypotheses(pp.counts[0], pp.counts[1], pp.sphere, pp.results, hypotheses, pp.up_axis, pp.right_axis,
                             y_only=up_sym)
    if centre_peaks <= 1:
        return hyps, None
    # the further peaks' hypotheses from their own counts and records (peak 0's are the ones above)
    return hyps, [hyps] + [verify.hypotheses(pp.centre_counts[c, 0], pp.centre_counts[c, 1], pp.sphere, pp.centre_results[c],
                                             hypotheses, pp.up_axis, pp.right_axis, y_only=up_sym) for c in range(1, centre_peaks)]


def _pass_output(pipe, records, idx, pts, hypotheses, hyps, centre_hyps, centre_n):
    """The dict run_ensemble / run_table return, from the two passes' records (host), after pipe.select(): refuses records that
    were not voted; hyps / centre_hyps / centre_n: per pass, device tensors or None."""
    B = pipe.B
    for rec in records:
        bad = np.nonzero(rec["flags"] & 6)[0]
        if bad.size:
            raise RuntimeError("instances %s were not voted (flags %s: grid above cells_cap / int32)" %
                               (bad.tolist(), rec["flags"][bad].tolist()))
    chosen = pipe.results_to_numpy(pipe.selected)
    losses = pipe.losses.cpu().numpy()                                                     # [2,B] float64
    pick = chosen["pad_"][:, 0].astype(np.int64)
    best = pipe.best.cpu().numpy()
    scale = records[0]["scale"].copy()                                                     # eval.py:308-310: float32 [B,3]
    scale_norm = np.array([np.linalg.norm(s_) for s_ in scale], dtype=np.float32)          # np.linalg.norm per instance
    out = dict(records=records, selected=chosen, losses=losses, pick=pick, best=best, scale=scale.astype(np.float64),
               scale_norm=scale_norm.astype(np.float64), idx=idx, pipe=pipe, pts=pts)
    if hypotheses is not None:
        out["hypotheses"] = [pipe.results_to_numpy(h_.reshape(-1, 160)).reshape(B, hypotheses) for h_ in hyps]
    if centre_hyps[0] is not None:
        out["centre_hypotheses"] = [np.stack([pipe.results_to_numpy(h_.reshape(-1, 160)).reshape(B, hypotheses) for h_ in ch])
                                    for ch in centre_hyps]
        out["centre_n"] = [n_.cpu().numpy() for n_ in centre_n]
    return out


@torch.no_grad()
def run_ensemble(cfg, dino_model, shot_model, pcs, descs, seed, scene_ids, num_pairs, num_rots, angle_tol=1.,
                 imp_wt_margin=0.01, backproj_ratio=.1, opt=False, geo_branch=True, visual_branch=True, up_sym=False,
                 priors=None, keep=False, scale_priors=None, two_streams=True, hypotheses=None, centre_peaks=1):
    """eval.py:207-372 for a batch of instances of one category.  pcs: list of float32 [N_b,3]; descs: list of float32
    [N_b,1024] arrays or (device) tensors (DINOv2 features at the points: inputs to the path); priors: optional callable(idx_global, base) -> logit
    prior [T,6,nb] added to both models' logits; scale_priors: optional float32 [B,3] teacher box extents that stand in for
    the scale head of random-init weights (the head's output stays in the sum at 1e-3).  Returns dict(records=[2 x
    structured array], losses float64 [2,B], pick int [B], scale, scale_norm, idx, pipe, ...).
    two_streams (default): the DINO pass and the SHOT pass (descriptors included) run on two HIP streams at once, each with
    working buffers of its own (VotingPipeline.twin) -- one pass' voting and descriptor kernels beside the other's wide
    matrix-core kernels; the only cross-stream dependency is the DINO pass' scale, which scores the SHOT pass too
    (eval.py:308-310).  Same records as the one-stream order (keep=True, which hands out intermediates, uses that order).
    hypotheses: None (default) or H >= 1: each pass also forms H pose hypotheses from the peaks of its two votes
    (verify.hypotheses, right after its vote and before `opt`; slot 0 is the pass' assembled record), returned as
    out["hypotheses"] = [2 x RESULT_DTYPE [B,H]] (model 0, model 1).
    centre_peaks: C >= 1 (needs hypotheses): each pass votes with VotingPipeline.vote(centre_peaks=C) and forms H hypotheses per
    centre-vote peak from that peak's counts and record; out["centre_hypotheses"] = [2 x RESULT_DTYPE [C,B,H]], whose [m][0] is
    out["hypotheses"][m] (the first maximum: what C = 1 gives), and out["centre_n"] = [2 x int32 [B]] the peaks each scene had.
    Records, losses and the selection are those of C = 1."""
    dev = ops._dev()
    B = len(pcs)
    Ns = [int(p.shape[0]) for p in pcs]
    k = cfg.num_more + 2
    cap = _vote_cap(pcs, cfg)
    pts = torch.from_numpy(np.concatenate(pcs)).to(dev)
    two = bool(two_streams) and not keep
    pipe, twin, scale_bufs = _pipelines(dev, Ns, num_pairs, k, cfg, num_rots, angle_tol, backproj_ratio, imp_wt_margin, cap, two)
    # eval.py:207 -- one tuple table per instance, shared by both models
    idx = torch.cat([ops.sample_tuples(n, num_pairs, k, seed, (s,), dev) for s, n in zip(scene_ids, Ns)])
    # descriptors: device tensors stay where they are (main_nocs samples them on the GPU), host arrays are uploaded one by one --
    # the batch is assembled on the device, not by a host-side copy of its largest input (16.8 MB per 4096 points)
    desc = torch.cat([d.to(dev) if torch.is_tensor(d) else torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).to(dev)
                      for d in descs])
    base = torch.cat([torch.full((num_pairs,), o, dtype=torch.int64) for o in np.cumsum([0] + Ns[:-1])]).to(dev)
    prior = priors(idx, base) if priors is not None else None      # a [T, 6, nb] array or an ops.BinPrior
    prior_arr = (lambda: prior.dense() if isinstance(prior, ops.BinPrior) else prior)
    scale_prior = None
    if scale_priors is not None:
        scale_prior = torch.from_numpy(np.asarray(scale_priors, dtype=np.float32)).to(dev).repeat_interleave(num_pairs, 0)
    main = torch.cuda.current_stream(dev)
    streams = _side_streams(dev) if two else [main, main]
    pipes = [pipe, twin if two else pipe]
    for st_ in streams:
        st_.wait_stream(main)
    kept = []
    extra = {}
    hyps = [None, None]
    hypotheses, centre_peaks = _hypothesis_args(hypotheses, centre_peaks)
    centre_hyps, centre_n = [None, None], [None, None]
    dino_scored = torch.cuda.Event() if two else None

    def one_pass(model_idx):
        model = (dino_model, shot_model)[model_idx]
        pp = pipes[model_idx]
        pp.use_slot(model_idx)                       # each pass writes its own records; nothing is read back before the end
        scales_buf = scale_bufs[model_idx]           # (rows of pairs that are not kept are never read: assemble() walks the kept list)
        u = torch.cat([ops.philox_uniform(num_pairs, 6, seed, 1 + model_idx, (s,), dev) for s in scene_ids])
        # eval.py:225-229 (the bin draw) runs as the epilogue of the logit head's output layer when the kernels allow it (split
        # arithmetic, no intermediates requested): the heads then return None in place of the logits.  The scale head is
        # evaluated after the back-vote filter, on the kept pairs' rows only (eval.py:272 reads nothing else).
        draw = None if keep else (u, None if prior is None else (prior if isinstance(prior, ops.BinPrior) else prior.contiguous()), pp.bins)
        if model_idx == 0:
            # train_dino.py:91-97, 128-133 without its rows: per-point slot tables + coordinate columns, summed by the first
            # ResLayer's kernel; every layer is a kernel of the library
            pred_cls, second = dino_model.heads_from_tuples(pts, desc, idx, pp.pt_off, pp.tup_off, lazy_scale=not keep, decode=draw)
        else:
            # eval.py:210-216, then train_shot.py:75-83 + :100-111; the tuple rows are gathered inside the first ResLayer's kernel
            shot_feat, normal = shot.compute_device(pts, pp.pt_off, cfg.res * 10, cfg.res * 10)
            shot_feat = ops.nan_to_zero_(shot_feat)
            normal = ops.nan_to_zero_(normal)
            extra["shot_feat"], extra["normal"] = shot_feat, normal
            feat_shot = shot_model.encode_points(shot_feat)
            pred_cls, second = shot_model.heads_from_tuples(pts, idx, feat_shot, normal, pp.pt_off, pp.tup_off,
                                                            lazy_scale=not keep, decode=draw)
        raw_cls = pred_cls
        if prior is not None and pred_cls is not None:
            pred_cls = pred_cls + prior_arr()

        def scales():
            s_ = second if keep else model.scale_head_rows(second, pp.kept_rows32(),
                                                           scatter=(pp.kept_count, pp.max_kept, scales_buf))
            return (scale_prior + 1e-3 * s_).contiguous() if scale_prior is not None else s_.contiguous()
        pred_scales = scales() if keep else scales
        if centre_peaks > 1:
            pp.vote(pts, idx, None if pred_cls is None else pred_cls.contiguous(), u, pred_scales, centre_peaks=centre_peaks)
        else:
            pp.vote(pts, idx, None if pred_cls is None else pred_cls.contiguous(), u, pred_scales)
        if hypotheses is not None:
            # here, on this pass' stream: the one-stream order reuses pp.counts for the next pass, and `opt` rewrites the records
            hyps[model_idx], centre_hyps[model_idx] = _pass_hypotheses(pp, hypotheses, centre_peaks, up_sym)
            if centre_peaks > 1:
                centre_n[model_idx] = pp.centre_n
        if opt:
            pp.refine(pts, idx, up_sym)                                                    # eval.py:319-355
        if two and model_idx == 0:
            dino_scored.record()                     # the DINO pass' records (scale) are final
        if two and model_idx == 1:
            torch.cuda.current_stream(dev).wait_event(dino_scored)
        pp.alignment_loss(pts, idx, up_sym)                    # eval.py:358-363; the DINO pass' scale scores both passes
        if keep:
            kept.append(dict(bins=pp.bins.cpu().numpy(), mask=pp.mask.cpu().numpy().astype(bool),
                             pred_cls=pred_cls.cpu().numpy(), raw_cls=raw_cls.cpu().numpy(), pred_scales=pred_scales.cpu().numpy(), u=u.cpu().numpy(),
                             counts=pp.counts.cpu().numpy()))

    # (two streams: the persistent MLP launches leave one CU per shader engine to the other pass' kernels, cppf_mlp_reserve_cus)
    prev_reserved = ops.mlp_reserve_cus(ops.batch_mode_reserved_cus(dev) if two else 0)
    try:
        for model_idx in (0, 1):                                                           # eval.py:219
            with torch.cuda.stream(streams[model_idx]):
                one_pass(model_idx)
    finally:
        ops.mlp_reserve_cus(prev_reserved)        # an enclosing BatchMode / mlp_cus_reserved block keeps its reservation
    for st_ in streams:
        main.wait_stream(st_)
    # ---- ensemble selection (eval.py:217,365-372): strict '<' against inf, model 0 first -- on the device ---------
    pipe.select(geo_branch, visual_branch)
    records = [pipe.results_to_numpy(pipe.result_slots[m]) for m in (0, 1)]                # the 160-byte records: the first read
    out = _pass_output(pipe, records, idx, pts, hypotheses, hyps, centre_hyps, centre_n)
    if keep:
        out["kept"] = kept
        out["shot_feat"], out["normal"] = extra["shot_feat"].cpu().numpy(), extra["normal"].cpu().numpy()
    return out


_TABLES = {}               # (path, device) -> pair_table.PairTable on the device


def load_pair_table(path, dev):
    """The pair-feature table of `path` on `dev`, loaded once per process; a missing file is an error that names it."""
    from cppf2_amd import pair_table
    key = (os.path.abspath(str(path)), str(torch.device(dev)))
    if key not in _TABLES:
        if not os.path.isfile(key[0]):
            raise FileNotFoundError("pair table %s not found (build it with `python -m cppf2_amd.pair_table`)" % path)
        _TABLES[key] = pair_table.PairTable.load(key[0]).to(dev)
    return _TABLES[key]


@torch.no_grad()
def run_table(cfg, table, pcs, seed, scene_ids, num_pairs, num_rots, angle_tol=1., imp_wt_margin=0.01, backproj_ratio=.1,
              opt=False, up_sym=False, hypotheses=None, centre_peaks=1):
    """run_ensemble's place for a known object: ONE pass whose bins come from the object's pair-feature table
    (pair_table.PairTable.vote) instead of the two model passes.  Normals:
    shot.normals_device(pts, pt_off, res * 10), NaN -> 0; no descriptor is computed.  The pass writes record slot 0 and the
    selection is select(True, False).  Returns run_ensemble's dict (records = the pass' twice, losses row 1 = inf, pick 0 or -1,
    hypotheses / centre_hypotheses with the pass' list in both places: callers enable pass 0 only) plus table_hits int [B,3]."""
    dev = ops._dev()
    Ns = [int(p.shape[0]) for p in pcs]
    k = cfg.num_more + 2
    res_built = table.meta.get("res")
    if res_built and abs(float(res_built) - float(cfg.res)) > 1e-9:
        # the table's normals were estimated on clouds down-sampled at its res with radius 10 res: the scene's must be too
        raise ValueError("the pair table was built at res = %g, the configuration has res = %g" % (res_built, cfg.res))
    cap = _vote_cap(pcs, cfg)
    hypotheses, centre_peaks = _hypothesis_args(hypotheses, centre_peaks)
    pts = torch.from_numpy(np.concatenate(pcs)).to(dev)
    pipe, _, _ = _pipelines(dev, Ns, num_pairs, k, cfg, num_rots, angle_tol, backproj_ratio, imp_wt_margin, cap, False)
    idx = torch.cat([ops.sample_tuples(n, num_pairs, k, seed, (s,), dev) for s, n in zip(scene_ids, Ns)])
    u = torch.cat([ops.philox_uniform(num_pairs, 6, seed, 1, (s,), dev) for s in scene_ids])
    normal = ops.nan_to_zero_(shot.normals_device(pts, pipe.pt_off, cfg.res * 10))
    pipe.use_slot(0)
    table.vote(pipe, pts, normal, idx, u, **(dict(centre_peaks=centre_peaks) if centre_peaks > 1 else {}))
    hits = table.last_hits
    hyps = centre_hyps = None
    if hypotheses is not None:
        hyps, centre_hyps = _pass_hypotheses(pipe, hypotheses, centre_peaks, up_sym)
    if opt:
        pipe.refine(pts, idx, up_sym)
    pipe.alignment_loss(pts, idx, up_sym)
    pipe.select(True, False)
    rec = pipe.results_to_numpy(pipe.result_slots[0])
    out = _pass_output(pipe, [rec, rec], idx, pts, hypotheses, [hyps, hyps], [centre_hyps, centre_hyps],
                       [pipe.centre_n] * 2 if centre_hyps is not None else [None, None])
    out["losses"] = out["losses"].copy()
    out["losses"][1] = np.inf                       # there is no second pass
    out["table_hits"] = hits.cpu().numpy().astype(np.int64)
    return out


def _teacher_prior(canon, dev):
    canon = torch.from_numpy(canon).to(dev)
    kb = torch.arange(32, device=dev, dtype=torch.float32)

    def prior(idx, base):
        coords = canon[(idx[:, :2].long() + base[:, None]).reshape(-1)].reshape(-1, 6)
        pos = (coords.clamp(-0.5, 0.5) + 0.5) * 31.0
        return ops.BinPrior(pos.contiguous(), 1.0 / 0.6)          # generated inside the fused bin draw; .dense() where an array is needed
    return prior


def _instance_hypotheses(selected, pick, hyps, enabled, H):
    """The hypothesis list of one instance (pure host code).  selected: its selected record (after `opt`: what H = 1 reports);
    pick: the picked pass (-1: none); hyps[m][c]: pass m's hypothesis records of centre-vote peak c (RESULT_DTYPE [H'], slot 0 =
    the pass' record for that centre; hyps[m] may be None for a pass that formed none); enabled[m]: pass m takes part.
    Order.  Centre peak 0 (the first maximum of the vote grid), exactly the list without further centre peaks: the selected
    record, the other peak combinations of the picked pass, then those of the other pass if it is enabled; empty records
    (flags bit0) dropped.  Then the further centre peaks, round-robin: the first hypothesis of peak 1, of peak 2, ..., then
    their second ones, and so on, each peak's own list being the picked pass' combinations followed by the other enabled pass'.
    When H cuts the list, peak 0's part is cut first to min(its length, H - the number of further peaks that have a hypothesis)
    (at least 1), so that a small H still sees every centre once; with one centre peak that is the plain cut at H.
    Returns (records RESULT_DTYPE [H], centre int64 [H]): slots past the end of the list carry the selected record with flags
    bit0 and centre -1."""
    from cppf2_amd import verify
    from cppf2_amd.pipeline import RESULT_DTYPE
    recs = np.zeros((H,), dtype=RESULT_DTYPE)
    centre = np.full((H,), -1, dtype=np.int64)
    lst = []
    p_ = int(pick)
    if p_ >= 0:
        order = [p_] + ([1 - p_] if enabled[1 - p_] and hyps[1 - p_] is not None else [])
        n_c = len(hyps[p_])

        def of_peak(c):
            out = []
            for m in order:
                out += list(hyps[m][c][1:] if (m == p_ and c == 0) else hyps[m][c])
            return [h_ for h_ in out if not h_["flags"] & verify.EMPTY]
        first = [selected] + of_peak(0)
        first = [h_ for h_ in first if not h_["flags"] & verify.EMPTY]
        others = [of_peak(c) for c in range(1, n_c)]
        live = sum(1 for o_ in others if o_)
        lst = [(h_, 0) for h_ in first[:max(1, H - live)]]
        for j in range(max([len(o_) for o_ in others], default=0)):
            lst += [(o_[j], c + 1) for c, o_ in enumerate(others) if j < len(o_)]
        lst = lst[:H]
    for h in range(H):
        if h < len(lst):
            recs[h], centre[h] = lst[h]
        else:
            recs[h] = selected
            recs["flags"][h] |= verify.EMPTY
    return recs, centre


# the settings of the stages after the vote, resolved once from the flags (eval._checked_flags)
Stages = collections.namedtuple("Stages", "icp_iters icp_depth icp_model_weight hypotheses verify_tau centre_peaks")


def _icp_item(st):
    """The ICP stats of one instance as the report carries them; the model-side figures when cppf_icp_refine_depth ran."""
    item = dict(inliers=int(st[0]), rms=float(st[1]), inlier_frac=float(st[2]), updates=int(st[3]))
    if len(st) == 8:
        item.update(model_inliers=int(st[4]), model_rms=float(st[5]), model_inlier_frac=float(st[6]), model_visible=int(st[7]))
    return item


def _verify_instances(r, enabled, obj, depth, mask, K, pt_off, icp_model, stages, support=None):
    """The hypotheses of each instance in _instance_hypotheses' order, cut at stages.hypotheses (empty slots past the end; an
    instance without a pick gets only empty slots), then verify.select (ICP first when stages.icp_iters > 0) on the instance's
    image; support: verify.select's plane, support_tau and max_sunk (the support check of solid.py) or None.  The result also
    carries centre int64 [B,H] (the centre-vote peak of each hypothesis, -1 for empty slots) and centre_peak int64 [B] (that of
    the chosen one)."""
    from cppf2_amd import verify
    from cppf2_amd.pipeline import RESULT_DTYPE
    B, H = len(r["pick"]), stages.hypotheses
    recs = np.zeros((B, H), dtype=RESULT_DTYPE)
    centre = np.full((B, H), -1, dtype=np.int64)
    per_pass = r.get("centre_hypotheses") or [h_[None] for h_ in r["hypotheses"]]
    for b in range(B):
        recs[b], centre[b] = _instance_hypotheses(r["selected"][b], r["pick"][b], [pp_[:, b] for pp_ in per_pass], enabled, H)
    img, msk = np.asarray(depth, dtype=np.float32), np.asarray(mask, dtype=bool)
    if img.ndim == 2:                              # one image for the whole batch (the depth mode)
        img = np.broadcast_to(img, (B,) + img.shape)
    if msk.ndim == 2:
        msk = np.broadcast_to(msk, (B,) + msk.shape)
    extra = dict(icp_depth=True, icp_model_weight=stages.icp_model_weight) if stages.icp_depth else {}
    extra.update(support or {})
    out = verify.select(obj, img, msk, K, recs, pts=r["pts"], pt_off=pt_off, icp_model=icp_model, icp_iters=stages.icp_iters,
                        tau=stages.verify_tau, **extra)
    out["centre"] = centre
    out["centre_peak"] = centre[np.arange(B), np.maximum(out["chosen"], 0)]
    return out


def refine_and_verify(r, enabled, obj, depth, mask, K, pt_off, icp_model, stages, support=None):
    """What follows the vote r of a batch whose instances have a mesh; stages: the Stages settings.  hypotheses > 1: that many
    hypotheses per instance verified against depth / mask ([H_img,W_img] for the whole batch or [B,H_img,W_img]), each refined
    by icp_iters first (_verify_instances); else, with icp_iters > 0, the selected records refined against icp_model (after the
    ensemble selection and `opt`).  support: the support check's arguments for verify.select (hypotheses > 1 only) or None.
    Returns (the B records to report: the verified ones, else the refined selected ones, else each instance's picked pass';
    icp_stats float32 [B,4 or 8] of the reported records or None; verify.select's dict or None)."""
    from cppf2_amd import icp
    B = len(r["pick"])
    if stages.hypotheses > 1:
        ver = _verify_instances(r, enabled, obj, depth, mask, K, pt_off, icp_model, stages, support)
        icp_stats = ver["icp"][np.arange(B), np.maximum(ver["chosen"], 0)] if stages.icp_iters > 0 else None
        return ver["records"], icp_stats, ver
    if stages.icp_iters > 0:
        extra = dict(depth=np.asarray(depth).astype(np.float32), K=K, model_weight=stages.icp_model_weight) if stages.icp_depth else {}
        icp_stats = icp.refine(icp_model, r["pts"], pt_off, r["selected"], iters=stages.icp_iters, **extra)
        return r["selected"], icp_stats, None
    return [r["records"][r["pick"][b]][b] for b in range(B)], None, None


def instance_items(r, b, icp_stats, ver, stages):
    """The report items these stages leave for instance b: `verify` and `icp` where it has a pose, `table_hits` after run_table."""
    from cppf2_amd import verify
    items = {}
    if r["pick"][b] >= 0 and ver is not None:
        k_ = int(ver["chosen"][b])
        items["verify"] = dict(hypotheses=int(np.count_nonzero((ver["hypotheses"][b]["flags"] & verify.EMPTY) == 0)),
                               chosen=k_, score=float(ver["scores"][b, k_]), score_first=float(ver["scores"][b, 0]))
        if stages.centre_peaks > 1:
            items["verify"]["centre_peak"] = int(ver["centre_peak"][b])
        if "support" in ver:                       # the support check ran: (back, sunk, solid, open) per hypothesis
            items["verify"].update(support=ver["support"][b].tolist(), refused=[bool(x_) for x_ in ver["refused"][b]])
    if r["pick"][b] >= 0 and icp_stats is not None:
        items["icp"] = _icp_item(icp_stats[b])
    if "table_hits" in r:
        items["table_hits"] = [int(x) for x in r["table_hits"][b]]
    return items


_ICP_DEPTH_NOTE = ("%d point-to-plane ICP iterations against %s, observed points to model and model samples to the depth image, "
                   "model weight %g (cppf_icp_refine_depth)")
_CENTRE_NOTE = "; translation hypotheses from %d separated peaks of each centre vote (cppf_grid_peaks)"


def stage_notes(against, stages, mask_cleaning=None):
    """The report's `mask_cleaning` / `icp_refinement` / `verification` entries.  against: what the ICP refined against, in
    words; mask_cleaning: the entry itself (the modes word it differently), None: masks were not cleaned."""
    from cppf2_amd import verify
    notes = {}
    if mask_cleaning is not None:
        notes["mask_cleaning"] = mask_cleaning
    if stages.icp_iters > 0:
        notes["icp_refinement"] = "%d point-to-plane ICP iterations against %s (cppf_icp_refine)" % (stages.icp_iters, against)
        if stages.icp_depth:
            notes["icp_refinement"] = _ICP_DEPTH_NOTE % (stages.icp_iters, against, stages.icp_model_weight)
    if stages.hypotheses > 1:
        notes["verification"] = ("%d pose hypotheses per instance from %d peaks per vote, rendered and compared with the depth "
                                 "at tau = %g m (cppf_pose_hypotheses, cppf_depth_fit_counts)"
                                 % (stages.hypotheses, verify.PEAKS, stages.verify_tau))
        if stages.centre_peaks > 1:
            notes["verification"] += _CENTRE_NOTE % stages.centre_peaks
    return notes
