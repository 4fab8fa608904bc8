#!/usr/bin/env python
"""Entry point with the reference's eval.py flag surface (eval.py:54-65):

    python eval.py --angle_tol=1. --imp_wt_margin=0.01 --backproj_ratio=.1 --num_pairs=50000 --num_rots=180 \
                   --opt=False --geo_branch=True --visual_branch=True \
                   [--data=synthetic --num_scenes=16 --categories=bottle,mug | --category=bottle] [--ckpt_dir=ckpts]

Like the reference (eval.py:84-101) it sets up one DINO model + one SHOT model + one cfg per category of the whitelist
(all six by default) and evaluates every object instance with both models, keeping the pose with the smaller
alignment loss (eval.py:219-372).  The per-instance loop of the reference (tuple sampling -> SHOT -> two models ->
decode -> centre vote -> back-vote filter -> rotation votes -> pose -> ensemble selection) runs here batched over all
instances of a category on the GPU through cppf2_amd, with no host round trip before the final 160-byte records.
What the image cannot provide is stated, not faked:
  * NOCS REAL275 images / SAR-Net masks / last.ckpt / DINOv2 weights are absent -> `--data=synthetic` (default)
    evaluates seeded synthetic instances (cppf2_amd.synth) with random-init weights (or the checkpoints found under
    `--ckpt_dir`, laid out like the reference's: <ckpt_dir>/{dino,shot}/<cat>-num_more-3/{.hydra/config.yaml,
    lightning_logs/version_0/checkpoints/last.ckpt}, eval.py:91-99) plus a teacher prior; `--data=depth` evaluates
    one depth+mask PNG pair (example_data layout) through backproject/downsample.
  * the Adam/lietorch refinement (eval.py:319-355, `opt`) runs as one HIP kernel per batch
    (cppf_refine_pose); lietorch is absent, so its semantics are restated from the published algorithm and pinned
    only by the oracle (parity unpinned).
  * `--data=depth --mesh=<ply|obj> [--mesh_scale=1.0] --icp_iters=N` (N > 0) refines the selected pose of the instance by N
    point-to-plane ICP iterations against samples of the object's mesh (cppf2_amd.icp, cppf_icp_refine; not in the
    reference), after the ensemble selection and `opt`; the report gains the ICP stats.  --icp_iters=0 (default): off.
  * `--icp_iters=N --icp_depth [--icp_model_weight=1.0]` (--data=depth and --data=bop) adds the model-to-depth terms to that ICP
    (cppf_icp_refine_depth): every model sample facing the camera is associated with the surface the depth
    image shows at its pixel, inside the mask or not, its terms weighted by --icp_model_weight; on both routes, the direct
    refinement and the per-hypothesis one of --hypotheses > 1.  The ICP stats gain the model-side figures.  Off by default.
  * `--data=depth --mesh=<ply|obj> --gt_pose=<.npy|.txt> [--models_info=<json>]` scores the reported pose against the true one
    (a 3x4 or 4x4 model -> OpenCV camera matrix in the record convention, metres) with the BOP metrics VSD, MSSD and MSPD
    (cppf2_amd.bop; --models_info: the object's BOP models_info entry, for its symmetries and diameter): each result gains
    `bop` (and `bop_before_icp` with --icp_iters > 0), the report their average recall.
  * `--data=depth --mesh=<ply|obj> --hypotheses=H [--verify_tau=0.01]` (H > 1) verifies H pose hypotheses of the instance
    against the depth image (cppf2_amd.verify, cppf_pose_hypotheses + cppf_depth_fit_counts; not in the reference): the
    selected pose first, then the other peak combinations of both votes of the picked pass and of the other enabled pass;
    each is refined by --icp_iters, rendered, and the one whose render explains the most of the observed instance is
    reported.  Each result gains `verify`, and with --gt_pose `bop_first` (the errors of the selected pose: what H = 1
    reports).  --hypotheses=1 (default): off.
  * `--hypotheses=H --centre_peaks=C` (C > 1; --data=depth and --data=bop) also verifies translation hypotheses: each pass takes C
    peaks of its centre-vote grid at least 2 cm apart (cppf_grid_peaks) and runs the back-vote filter, both rotation votes and the
    pose assembly again for every peak (VotingPipeline.vote(centre_peaks=C)); the hypotheses of the further peaks follow those of
    the first maximum in the list (_instance_hypotheses), and `verify` gains `centre_peak`, the peak the chosen hypothesis came
    from.  --centre_peaks=1 (default): off.
  * `--data=bop --bop_root=<dir> --split=<name> [--targets=<json>] --out_csv=<file> [--model_scale=0.001]` runs the instance-level
    path over a BOP-format dataset (cppf2_amd.bop_data; not in the reference): per target the instances' masks come from
    mask_visib/ (computed by cppf_gt_visibility when the folder is missing: the "ground-truth masks" protocol), each is
    back-projected and down-sampled as in the depth mode, instances of one object are batched across images through
    run_ensemble (config/custom.yaml, --ckpt_shot / --ckpt_dino), --icp_iters / --hypotheses / --verify_tau apply per
    instance against the object's model, and the reported poses go to a BOP results CSV (score: the verification score, else
    the negated alignment loss; time: the image's share of its batches' wall time), which bop_data.score then scores.
    `--teacher_prior` (this mode only) builds the logit prior and the scale from each instance's ground-truth pose, the same
    stand-in the synthetic mode uses: trained checkpoints are absent from this tree, and without it untrained weights vote noise.
  * `--data=bop --detections=<json> [--det_score_min=0.0]` starts from a detections file instead (bop_data.read_detections:
    COCO-style JSON, one entry per detection with a score and a run-length encoded mask): every detection of a target's object
    in its image with score >= det_score_min is decoded on the GPU (cppf2_amd.masks, cppf_rle_decode) and gives one CSV row
    (score: the detection's, times the verification score with --hypotheses > 1); bop_data.score keeps the best inst_count per
    target.  With `--teacher_prior` a detection takes the prior of the valid ground-truth instance whose visible mask overlaps
    it most; one that overlaps none is dropped (skipped.no_gt_for_prior).
  * `--clean_masks [--mask_jump=0.01]` (--data=bop, with or without detections; `--clean_mask` with --data=depth) cuts every
    mask down to its largest depth-connected component (cppf_mask_components: valid 4-neighbours within mask_jump metres)
    before back-projection and verification: depth-separated bleed of a detector's mask onto the background or onto a
    neighbour goes, a table the object stands on stays.  Off by default.
  * `--pair_table=<npz>` (--data=depth) / `--pair_tables=<dir>` (--data=bop: one obj_%06d.npz per object; a missing one is an
    error that names the file) vote from the object's pair-feature table (python -m cppf2_amd.pair_table)
    instead of the two models: one pass (run_table) whose bins are looked up from each tuple's point-pair feature, no prior, no
    checkpoint; --hypotheses, --centre_peaks, --icp_iters, --icp_depth, --opt, --gt_pose, --out_csv, --detections and
    --clean_masks work as before, and the report gains `table_hits` (per instance: tuples that took their own cell, a
    neighbouring cell, the whole table).  Not with --teacher_prior, --ckpt_* or the synthetic / NOCS modes.
Swapped flag names are kept: geo_branch gates model 0 (DINO), visual_branch gates model 1 (SHOT) (eval.py:367).
"""
import json
import os
import sys

import numpy as np
import torch

from cppf2_amd import geometry, ops, shot, synth
from cppf2_amd.config import load_checkpoint_config, load_config
from cppf2_amd.models import BeyondCPPFDino, BeyondCPPFShot, load_reference_checkpoint
from cppf2_amd.ops import get_topk_dir  # noqa: F401  (the reference defines it in this file, eval.py:37-51; demo.py and the notebook import it from here)
from cppf2_amd.pipeline import VotingPipeline

id2category = {1: "bottle", 2: "bowl", 3: "camera", 4: "can", 5: "laptop", 6: "mug"}     # dataset.py:29-37
category2id = {v: k for k, v in id2category.items()}
WHITELIST = ["can", "bowl", "laptop", "bottle", "camera", "mug"]                          # eval.py:78
UP_SYM = ("can", "bottle", "bowl")                                                        # eval.py:333,362


def _flag(v):
    if isinstance(v, str):
        if v.lower() in ("true", "false"):
            return v.lower() == "true"
        try:
            return float(v) if any(c in v for c in ".e") else int(v)
        except ValueError:
            return v
    return v


def load_custom(ckpt_shot=None, ckpt_dino=None, config_dir="config", device=None, models=True):
    """The instance-level setup of the reference's demo (config/custom.yaml: no category group): (cfg, dino, shot).
    models=False: (cfg, None, None) -- a pair-feature table stands where the models stood (run_table)."""
    dev = device or ops._dev()
    cfg = load_config(config_dir, "custom", [])
    if not models:
        return cfg, None, None
    dino_model = BeyondCPPFDino(cfg).to(dev).eval()
    shot_model = BeyondCPPFShot(cfg).to(dev).eval()
    if ckpt_dino:
        load_reference_checkpoint(dino_model, ckpt_dino)
    if ckpt_shot:
        load_reference_checkpoint(shot_model, ckpt_shot)
    return cfg, dino_model, shot_model


def load_category(cat_name, ckpt_dir=None, ckpt_shot=None, ckpt_dino=None, config_dir="config", device=None):
    """eval.py:87-101 for one category: (cfg, dino_model, shot_model).  With a checkpoint directory each model is built
    from the cfg saved next to its weights (`.hydra/config.yaml`) and the loop keeps the SHOT run's cfg (the last
    assignment, eval.py:101); otherwise config/ + category group and random-init weights."""
    dev = device or ops._dev()
    cfg = load_config(config_dir, "config", ["category=%s" % cat_name])
    cfgs = {"dino": cfg, "shot": cfg}
    weights = {"dino": ckpt_dino, "shot": ckpt_shot}
    if ckpt_dir:
        for name in ("dino", "shot"):
            root = os.path.join(ckpt_dir, name, "%s-num_more-3" % cat_name)               # eval.py:91,96
            hy = os.path.join(root, ".hydra", "config.yaml")
            if os.path.exists(hy):
                cfgs[name] = load_checkpoint_config(hy)                                    # eval.py:92,97
            ck = os.path.join(root, "lightning_logs", "version_0", "checkpoints", "last.ckpt")
            if weights[name] is None and os.path.exists(ck):
                weights[name] = ck
    dino_model = BeyondCPPFDino(cfgs["dino"]).to(dev).eval()
    shot_model = BeyondCPPFShot(cfgs["shot"]).to(dev).eval()
    if weights["dino"]:
        load_reference_checkpoint(dino_model, weights["dino"])
    if weights["shot"]:
        load_reference_checkpoint(shot_model, weights["shot"])
    return cfgs["shot"], dino_model, shot_model


def needed_cells(pc, res):
    """Cells of the vote grid of one instance (train_dino.py:173-175: int32 truncation of the float32 extent / res, + 1)."""
    ext = (pc.max(0) - pc.min(0)).astype(np.float32) / np.float32(res)
    return int(np.prod(ext.astype(np.int64) + 1))


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
        if ((p.max(0) - p.min(0)).max() / cfg.res) > 1000:
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


# ---------------------------------------------------------------------------------------------------------------------
# The REAL275 instance loop of the reference (eval.py:103-201, 364-412): detection results -> per-instance clouds -> poses ->
# one result record per image -> mAP.
# ---------------------------------------------------------------------------------------------------------------------
REAL_INTRINSICS = [[591.0125, 0, 322.525], [0, 590.16775, 244.11084], [0, 0, 1]]           # eval.py:82


def load_result_list(log_dir):
    """eval.py:103-127: every results_*.pkl under log_dir (SAR-Net / Mask-RCNN detections: image_path, pred_bboxes,
    pred_masks [H,W,n], pred_class_ids, pred_scores, gt_*), a dict or a list of dicts each, flattened in file order."""
    import glob
    import pickle
    paths = sorted(glob.glob(os.path.join(log_dir, "results_*.pkl")))
    assert len(paths), "no results_*.pkl under %r" % log_dir
    final_results = []
    for path in paths:
        with open(path, "rb") as f:
            result = pickle.load(f)
        items = result if isinstance(result, list) else [result]
        assert all(isinstance(r, dict) for r in items)
        for r in items:
            if "gt_handle_visibility" not in r:
                r["gt_handle_visibility"] = np.ones_like(r["gt_class_ids"])
            else:
                assert len(r["gt_handle_visibility"]) == len(r["gt_class_ids"])
        final_results += items
    return final_results


def crop_transform(bbox, padding=0.0, out_size=256):
    """The 3x3 crop-frame -> image-frame transform of resize_crop (dataset.py:322-337) for a PIL bbox (left, upper, right,
    lower): key points of the crop are `inv(transform) @ (x, y, 1)` (eval.py:203)."""
    width, height = bbox[2] - bbox[0], bbox[3] - bbox[1]
    size = max(height, width) * (1 + padding)
    cx, cy = (bbox[2] + bbox[0]) / 2, (bbox[3] + bbox[1]) / 2
    return (np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.]])
            @ np.array([[size / out_size, 0, 0], [0, size / out_size, 0], [0, 0, 1]])
            @ np.array([[1, 0, -out_size / 2], [0, 1, -out_size / 2], [0, 0, 1.]]))


def _read_depth(path):
    from PIL import Image
    return np.array(Image.open(path)).astype(np.float64)             # cv2.imread(path, -1) of a 16-bit PNG (eval.py:139)


def image_instances(res, data_root, cfgs, seed, image_index, intrinsics=REAL_INTRINSICS, token_maps=None):
    """eval.py:133-203 for one image: yields one dict per detection that reaches the voting path -- instance index i, category,
    cloud pc float32 [n,3] (back-projected through the mask, flipped, voxel down-sampled at cfg.res, capped at 50 000 points)
    and desc float32 [n,1024] or None.  Detections of other classes and clouds wider than 1000 cells are skipped like the
    reference does (their pred_RTs stay the identity)."""
    from PIL import Image
    image_path = res["image_path"].replace("data/real/test", data_root)                    # eval.py:133
    depth = _read_depth(image_path + "_depth.png")
    masks = np.asarray(res["pred_masks"])
    rgb = None
    if os.path.exists(image_path + "_color.png"):
        rgb = np.array(Image.open(image_path + "_color.png").convert("RGB"))
    K = np.asarray(intrinsics, dtype=np.float64).reshape(3, 3)
    for i in range(len(res["pred_bboxes"])):
        cls_id = int(res["pred_class_ids"][i])
        cat = id2category.get(cls_id)
        if cat not in cfgs:                                                                # eval.py:163-165 (whitelist)
            continue
        cfg = cfgs[cat]
        mask = masks[:, :, i] != 0
        pc, (rr, cc) = ops.backproject(depth / 1000., K, mask, return_device=True)         # eval.py:185-189
        if pc.shape[0] == 0:
            continue
        inst_seed = (seed * 1000003 + image_index * 131 + i) & 0x7FFFFFFF
        keep = ops.downsample(pc, cfg.res, inst_seed, return_device=True)                   # eval.py:191-193
        pc, rr, cc = pc[keep], rr[keep.long()], cc[keep.long()]
        pc = pc.cpu().numpy()
        idxs = np.stack([rr.cpu().numpy(), cc.cpu().numpy()], -1).astype(np.int64)         # K x 2 (row, col)
        if pc.shape[0] > 50000:                                                            # eval.py:194-197
            sub = np.random.RandomState(inst_seed).randint(pc.shape[0], size=(50000,))
            pc, idxs = pc[sub], idxs[sub]
        if ((pc.max(0) - pc.min(0)).max() / cfg.res) > 1000:                               # eval.py:199-200
            continue
        desc = None
        tok = None if token_maps is None else token_maps.get("%d_%d" % (image_index, i))
        if tok is not None:
            # eval.py:177-183,202-205: crop frame of the masked RGB (its non-zero bounding box; the mask's when the colour
            # image is absent), key points = pixel (col, row) mapped into the 256 x 256 crop, descriptors = the ViT patch
            # tokens of the crop (an INPUT of the path: DINOv2 weights are not part of it) sampled there, stride 4 (dataset.py:63)
            if rgb is not None:
                masked = np.zeros_like(rgb)
                masked[mask] = rgb[mask]
                bbox = Image.fromarray(masked).getbbox()
            else:
                bbox = Image.fromarray(mask.astype(np.uint8) * 255).getbbox()
            transform = crop_transform(bbox, padding=0, out_size=256)
            kp = np.flip(idxs, -1).astype(np.float64)
            kp_local = (np.linalg.inv(transform) @ np.concatenate([kp, np.ones((kp.shape[0], 1))], -1).T).T[:, :2]
            tok = np.asarray(tok, dtype=np.float32)
            desc = ops.interpolate_features(torch.from_numpy(tok)[None], kp_local.astype(np.float32)[None], strides=4)[0].T
            desc = desc.contiguous()               # stays on the device until its batch is evaluated (run_ensemble)
        yield dict(i=i, cat=cat, pc=pc, desc=desc, pixels=idxs)


def main_nocs(setups, log_dir, data_root="NOCS/real_test", out_dir=None, desc_npz=None, angle_tol=1., imp_wt_margin=0.01,
              backproj_ratio=.1, num_pairs=50000, num_rots=180, opt=True, geo_branch=True, visual_branch=True, seed=0,
              batch_instances=16, intrinsics=None, max_images=None, debug=False, out=None):
    """eval.py:103-412 on a directory in the reference's layout: `log_dir`/results_*.pkl (detections + ground truth per image)
    and `data_root`/<scene>/<frame>_{depth,color}.png.  Instances are collected image by image exactly as the reference
    filters them, evaluated in batches per category on the GPU (run_ensemble), and written back into their image's record
    (pred_RTs, pred_scales: eval.py:143-147, 370-372); every record is pickled under out_dir with the reference's file name
    (eval.py:134, 399) and the list is scored with degree_cm_mAP (eval.py:400-412).
    desc_npz: optional .npz of DINOv2 patch-token maps float32 [1024, 64, 64] keyed "<image index>_<instance index>" (the
    crop of eval.py:177-183 at stride 4); without it seeded unit vectors stand in (the DINO branch then votes on noise)."""
    import pickle
    from cppf2_amd import metrics
    dev = ops._dev()
    final_results = load_result_list(log_dir)
    if max_images:
        final_results = final_results[:int(max_images)]
    token_maps = np.load(desc_npz) if desc_npz else None
    cfgs = {c: s[0] for c, s in setups.items()}
    K = REAL_INTRINSICS if intrinsics is None else intrinsics
    # Instances are evaluated as they come: every category keeps at most `batch_instances` pending instances (point cloud +
    # descriptors, the latter on the device) and is flushed through run_ensemble when the batch is full -- the same batches, in
    # the same order per category, as collecting the whole list first, with memory bounded by the batch (a full REAL275 run has
    # ~12 000 instances x up to 200 MB of descriptors).
    pending = {c: [] for c in setups}               # category -> [(image index, instance index, global instance id, pc, desc)]
    seen = {c: 0 for c in setups}
    evaluated = 0
    picks = {"dino": 0, "shot": 0, "none": 0}

    def flush(cat):
        nonlocal evaluated
        chunk, pending[cat] = pending[cat], []
        if not chunk:
            return
        cfg, dino_model, shot_model = setups[cat]
        descs = []
        for (_, _, g_, pc, desc) in chunk:
            if desc is None:
                # no token maps: seeded unit vectors from a CPU generator, one stream per instance -- the same numbers on every
                # device and in every round (round 4 drew them with a device generator, whose stream is not the CPU's: seeded
                # `--data=nocs` stand-in runs were not comparable with earlier ones)
                gen = torch.Generator(device="cpu").manual_seed(seed * 7919 + g_ + 1)
                desc = torch.nn.functional.normalize(torch.randn((pc.shape[0], 1024), generator=gen), dim=-1).to(dev)
            descs.append(desc)
        r = run_ensemble(cfg, dino_model, shot_model, [c_[3] for c_ in chunk], descs, seed, [c_[2] for c_ in chunk],
                         num_pairs, num_rots, angle_tol, imp_wt_margin, backproj_ratio, bool(opt), geo_branch,
                         visual_branch, cat in UP_SYM)
        for b, (n_img, i, _, _, _) in enumerate(chunk):
            evaluated += 1
            if r["pick"][b] < 0:
                picks["none"] += 1
                continue
            picks[["dino", "shot"][r["pick"][b]]] += 1
            rec = r["records"][r["pick"][b]][b]
            res = final_results[n_img]
            res["pred_RTs"][i][:3, :3] = rec["R"] * r["scale_norm"][b]                 # eval.py:370
            res["pred_RTs"][i][:3, -1] = rec["t"]                                      # eval.py:371
            if r["scale_norm"][b] > 0:
                res["pred_scales"][i] = r["scale"][b] / r["scale_norm"][b]              # eval.py:372

    gid = 0
    for n_img, res in enumerate(final_results):
        nb = len(res["pred_bboxes"])
        res["pred_RTs"] = np.stack([np.eye(4) for _ in range(nb)]) if nb else np.zeros((0, 4, 4))      # eval.py:143
        res["pred_scales"] = np.stack([np.ones((3,)) for _ in range(nb)]) if nb else np.zeros((0, 3))  # eval.py:144
        for inst in image_instances(res, data_root, cfgs, seed, n_img, K, token_maps):
            cat = inst["cat"]
            pending[cat].append((n_img, inst["i"], gid + inst["i"], inst["pc"], inst["desc"]))
            seen[cat] += 1
            if len(pending[cat]) >= int(batch_instances):
                flush(cat)
        gid += nb
    for cat in setups:
        flush(cat)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        for res in final_results:
            image_path = res["image_path"].replace("data/real/test", data_root)
            with open(os.path.join(out_dir, "_".join(image_path.split("/")[1:]) + ".pkl"), "wb") as f:     # eval.py:134,399
                pickle.dump(res, f)
    total = sum(len(r_["pred_bboxes"]) for r_ in final_results)
    iou_aps, aps = metrics.degree_cm_mAP(final_results, metrics.SYNSET_NAMES, (5, 10, 15), (5, 10, 15),
                                         np.linspace(0, 1, 101), 0.1, True)                # eval.py:400-411
    cats = [c for c in setups if seen[c]]

    def mean_over(fn):
        v = [fn(category2id[c]) for c in cats]
        v = [x for x in v if np.isfinite(x)]
        return float(np.mean(v)) if v else None
    report = dict(data="nocs", images=len(final_results), detections=total, evaluated=evaluated, skipped=total - evaluated,
                  picked=picks, categories=cats, descriptors="token maps from %s" % desc_npz if desc_npz else "seeded unit vectors (no DINOv2 tokens given)",
                  pose_AP={"%ddeg_%dcm" % (d_, s_): mean_over(lambda c, i_=i_, j_=j_: aps[c, i_, j_])
                           for i_, d_ in enumerate((5, 10, 15)) for j_, s_ in enumerate((5, 10, 15))},
                  iou_AP={"IoU%d" % t_: mean_over(lambda c, t_=t_: iou_aps[c, t_]) for t_ in (25, 50, 75)})
    print(json.dumps(report))
    if out:
        with open(out, "w") as f:
            json.dump(report, f)
    report["final_results"] = final_results
    return report



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


def _icp_item(st):
    """The ICP stats of one instance as the report carries them; the model-side figures when cppf_icp_refine_depth ran."""
    item = dict(inliers=int(st[0]), rms=float(st[1]), inlier_frac=float(st[2]), updates=int(st[3]))
    if len(st) == 8:
        item.update(model_inliers=int(st[4]), model_rms=float(st[5]), model_inlier_frac=float(st[6]), model_visible=int(st[7]))
    return item


def _icp_depth_flag(icp_depth, icp_model_weight, icp_iters):
    if icp_depth and int(icp_iters) <= 0:
        raise ValueError("--icp_depth adds the model-to-depth terms to the ICP refinement: it needs --icp_iters > 0")
    w = float(icp_model_weight)
    if not (w > 0 and np.isfinite(w)):
        raise ValueError("--icp_model_weight must be finite and > 0, not %r" % (icp_model_weight,))
    if w != 1.0 and not icp_depth:
        raise ValueError("--icp_model_weight weighs the model-to-depth terms: it needs --icp_depth")
    return bool(icp_depth), w


def _verify_instances(r, B, H, enabled, obj, depth, mask, K, pt_off, icp_model, icp_iters, tau, icp_depth=False,
                      icp_model_weight=1.0):
    """The hypotheses of each instance in _instance_hypotheses' order, cut at H (empty slots past the end; an instance without a
    pick gets only empty slots), then verify.select (ICP first when icp_iters > 0) on the instance's image.  The result also
    carries centre int64 [B,H] (the centre-vote peak of each hypothesis, -1 for empty slots) and centre_peak int64 [B] (that of
    the chosen one)."""
    from cppf2_amd import verify
    from cppf2_amd.pipeline import RESULT_DTYPE
    recs = np.zeros((B, H), dtype=RESULT_DTYPE)
    centre = np.full((B, H), -1, dtype=np.int64)
    per_pass = r.get("centre_hypotheses") or [h_[None] for h_ in r["hypotheses"]]
    for b in range(B):
        recs[b], centre[b] = _instance_hypotheses(r["selected"][b], r["pick"][b], [pp_[:, b] for pp_ in per_pass], enabled, H)
    if np.ndim(depth) == 3:                        # one image and mask per instance (main_bop)
        img, msk = np.asarray(depth, dtype=np.float32), np.asarray(mask, dtype=bool)
    else:
        img = np.broadcast_to(np.asarray(depth, dtype=np.float32), (B,) + np.shape(depth))
        msk = np.broadcast_to(np.asarray(mask, dtype=bool), (B,) + np.shape(mask))
    extra = dict(icp_depth=True, icp_model_weight=icp_model_weight) if icp_depth else {}
    out = verify.select(obj, img, msk, K, recs, pts=r["pts"], pt_off=pt_off, icp_model=icp_model, icp_iters=icp_iters, tau=tau,
                        **extra)
    out["centre"] = centre
    out["centre_peak"] = centre[np.arange(B), np.maximum(out["chosen"], 0)]
    return out


def main_bop(setup, bop_root, split, out_csv, targets=None, mesh_scale=0.001, angle_tol=1., imp_wt_margin=0.01, backproj_ratio=.1,
             num_pairs=50000, num_rots=180, opt=True, geo_branch=True, visual_branch=True, seed=0, batch_instances=16,
             icp_iters=0, hypotheses=1, verify_tau=None, teacher_prior=False, visib_gt_min=None, debug=False, out=None,
             centre_peaks=1, detections=None, det_score_min=0.0, clean_masks=False, mask_jump=None, icp_depth=False,
             icp_model_weight=1.0, pair_tables=None):
    """The instance-level path over one split of a BOP-format dataset (cppf2_amd.bop_data.Dataset): one estimate per valid
    ground-truth instance of every target, from its visible mask; poses written to `out_csv` in BOP's frame and scored with
    bop_data.score.  Instances of one object (and one K and image size) are evaluated in batches of `batch_instances` across
    images.  detections: a detections file (bop_data.read_detections); every detection of a target's object in its image with
    score >= det_score_min then stands where the ground-truth instances stood, its mask decoded on the GPU (masks.decode_batch,
    one call per target), and gives one CSV row (score: the detection's, times the verification score with hypotheses > 1).
    pair_tables: a folder of obj_%06d.npz pair-feature tables (python -m cppf2_amd.pair_table): each object's instances are then
    voted from its table (run_table) instead of the two model passes; no prior.
    clean_masks: every mask is cut down to its largest depth-connected component (masks.clean, mask_jump metres) before
    back-projection and verification.  Returns the report (report["bop"] = bop_data.score's)."""
    import time
    from cppf2_amd import bop, bop_data, icp, masks, verify
    dev = ops._dev()
    cfg, dino_model, shot_model = setup
    if pair_tables and teacher_prior:
        raise ValueError("--pair_tables votes from the tables: it cannot be combined with --teacher_prior")
    up_sym = bool(cfg.get("up_sym", False))
    vmin = bop_data.VISIB_GT_MIN if visib_gt_min is None else float(visib_gt_min)
    ds = bop_data.Dataset(bop_root, split, mesh_scale)
    tlist = ds.targets(targets, vmin)
    verify_tau = verify.TAU if verify_tau is None else float(verify_tau)
    icp_models, pending, rows, summary = {}, {}, [], []
    im_time = {}
    skipped = dict(too_few_points=0, too_large=0, no_pick=0)
    mask_jump = masks.JUMP if mask_jump is None else float(mask_jump)
    if clean_masks:
        skipped["empty_after_clean"] = 0
    dets = None
    if detections is not None:
        # every detection's runs are checked here; its size against its image's when the image is read
        n_detections = 0
        dets = {}
        wanted = {(s_, i_, o_) for s_, i_, o_, _ in tlist}
        skipped.update(below_score=0, no_target=0)
        if "empty_after_clean" not in skipped:
            skipped["empty_after_clean"] = 0
        if teacher_prior:
            skipped["no_gt_for_prior"] = 0
        for n_, det in enumerate(bop_data.read_detections(detections)):
            n_detections += 1
            key = (det["scene_id"], det["image_id"], det["category_id"])
            if key not in wanted:
                skipped["no_target"] += 1
            elif det["score"] < float(det_score_min):
                skipped["below_score"] += 1
            else:
                dets.setdefault(key, []).append(dict(det, index=n_))
    gid = [0]
    enabled = (True, False) if pair_tables else (geo_branch, visual_branch)

    def flush(key):
        chunk, pending[key] = pending.get(key, []), []
        if not chunk:
            return
        t0 = time.perf_counter()
        o = key[0]
        obj = ds.object(o)
        B = len(chunk)
        descs = []
        for c_ in ([] if pair_tables else chunk):   # DINOv2 features are inputs to the path (weights absent): seeded unit vectors
            gen = torch.Generator(device="cpu").manual_seed(seed * 7919 + c_["gid"] + 1)
            descs.append(torch.nn.functional.normalize(torch.randn((c_["pc"].shape[0], 1024), generator=gen), dim=-1).numpy())
        priors = scale_priors = None
        if teacher_prior:
            # the synthetic mode's stand-in (synth.make_scene): canonical coordinates (pc - t) @ R / diag from the true pose
            ext = obj.verts.max(0) - obj.verts.min(0)
            diag = float(np.linalg.norm(ext))
            canon = [((c_["pc"].astype(np.float64) - c_["gt"]["t"]) @ c_["gt"]["R"] / diag).astype(np.float32) for c_ in chunk]
            priors = _teacher_prior(np.concatenate(canon), dev)
            scale_priors = np.stack([ext] * B)
        if pair_tables:
            r = run_table(cfg, load_pair_table(os.path.join(str(pair_tables), "obj_%06d.npz" % o), dev), [c_["pc"] for c_ in chunk],
                          seed, [c_["gid"] for c_ in chunk], num_pairs, num_rots, angle_tol, imp_wt_margin, backproj_ratio, bool(opt),
                          up_sym, hypotheses if hypotheses > 1 else None, centre_peaks)
        else:
            r = run_ensemble(cfg, dino_model, shot_model, [c_["pc"] for c_ in chunk], descs, seed, [c_["gid"] for c_ in chunk],
                             num_pairs, num_rots, angle_tol, imp_wt_margin, backproj_ratio, bool(opt), geo_branch, visual_branch,
                             up_sym, priors, scale_priors=scale_priors, hypotheses=hypotheses if hypotheses > 1 else None,
                             centre_peaks=centre_peaks)
        pt_off = np.cumsum([0] + [c_["pc"].shape[0] for c_ in chunk])
        ver = icp_stats = None
        if icp_iters > 0 and o not in icp_models:
            icp_models[o] = icp.ModelPoints.from_mesh(ds.mesh(o))
        if hypotheses > 1:
            ver = _verify_instances(r, B, hypotheses, enabled, obj, np.stack([c_["depth"] for c_ in chunk]),
                                    np.stack([c_["mask"] for c_ in chunk]), chunk[0]["K"], pt_off, icp_models.get(o), icp_iters,
                                    verify_tau, icp_depth, icp_model_weight)
            if icp_iters > 0:
                icp_stats = ver["icp"][np.arange(B), np.maximum(ver["chosen"], 0)]
        elif icp_iters > 0:
            extra = {}
            if icp_depth:
                extra = dict(depth=np.stack([c_["depth"] for c_ in chunk]).astype(np.float32), K=chunk[0]["K"],
                             model_weight=icp_model_weight)
            icp_stats = icp.refine(icp_models[o], r["pts"], pt_off, r["selected"], iters=icp_iters, **extra)
        dt = (time.perf_counter() - t0) / B
        for b, c_ in enumerate(chunk):
            im_time[(c_["scene_id"], c_["im_id"])] = im_time.get((c_["scene_id"], c_["im_id"]), 0.0) + dt + c_["prep_s"]
            item = dict(scene_id=c_["scene_id"], im_id=c_["im_id"], obj_id=o, gt_index=c_["gt_index"], points=int(c_["pc"].shape[0]),
                        model=None)
            if dets is not None:
                item.update(detection=c_["det"]["index"], det_score=c_["det"]["score"])
            summary.append(item)
            if r["pick"][b] < 0:
                skipped["no_pick"] += 1
                continue
            rec = r["records"][r["pick"][b]][b] if icp_stats is None else r["selected"][b]
            score = -float(r["best"][b])
            if ver is not None:
                rec = ver["records"][b]
                k_ = int(ver["chosen"][b])
                score = float(ver["scores"][b, k_]) if k_ >= 0 else 0.0
                item["verify"] = dict(hypotheses=int(np.count_nonzero((ver["hypotheses"][b]["flags"] & verify.EMPTY) == 0)),
                                      chosen=k_, score=score, score_first=float(ver["scores"][b, 0]))
                if centre_peaks > 1:
                    item["verify"]["centre_peak"] = int(ver["centre_peak"][b])
            if icp_stats is not None:
                item["icp"] = _icp_item(icp_stats[b])
            Rb, tb = bop.pose_to_bop(np.asarray(rec["R"], dtype=np.float64).reshape(3, 3), np.asarray(rec["t"], dtype=np.float64), mesh_scale,
                                     obj.centre)
            if dets is not None:
                score = c_["det"]["score"] * score if ver is not None else c_["det"]["score"]
            item.update(model="table" if pair_tables else ["dino", "shot"][r["pick"][b]], loss=float(r["best"][b]), score=score)
            if pair_tables:
                item["table_hits"] = [int(x) for x in r["table_hits"][b]]
            rows.append(dict(scene_id=c_["scene_id"], im_id=c_["im_id"], obj_id=o, score=score, R=Rb, t=tb))

    def candidates(s_id, im, o, info, gts, depth):
        """The masks that stand for the instances of one target: [dict(mask bool [H,W], gt, gt_index, det)].  Ground-truth mode:
        the visible mask of every valid instance.  Detections: every kept detection's decoded mask, one decode call; with the
        teacher prior each takes the valid ground-truth instance of its object whose visible mask overlaps it most (IoU; the
        lower instance index on ties) and is dropped when none overlaps."""
        valid = [g for g, gt in enumerate(gts) if gt["obj_id"] == o and info[g]["visib_fract"] >= vmin]
        if dets is None:
            return [dict(mask=ds.mask_visib(s_id, im, g), gt=gts[g], gt_index=g, det=None) for g in valid]
        lst = dets.get((s_id, im, o), [])
        if not lst:
            return []
        for det in lst:
            bop_data.check_detection_size(det, depth.shape, "%s entry %d" % (detections, det["index"]))
        decoded = masks.decode_batch([det["counts"] for det in lst], depth.shape[0], depth.shape[1]).cpu().numpy() > 0
        out = []
        gt_masks = [ds.mask_visib(s_id, im, g) for g in valid] if teacher_prior else []
        for det, m in zip(lst, decoded):
            g = None
            if teacher_prior:
                inter = [int(np.count_nonzero(m & gm)) for gm in gt_masks]
                iou = [i_ / max(int(np.count_nonzero(m | gm)), 1) for i_, gm in zip(inter, gt_masks)]
                if not inter or max(inter) == 0:
                    skipped["no_gt_for_prior"] += 1
                    continue
                g = valid[int(np.argmax(iou))]
            out.append(dict(mask=m, gt=None if g is None else gts[g], gt_index=g, det=det))
        return out

    depth_of = {}
    for s_id, im, o, _ in tlist:
        sc = ds.scene(s_id)
        info = ds.gt_info(s_id)[im]
        K = sc["camera"][im]["K"]
        t0 = time.perf_counter()
        if (s_id, im) not in depth_of:
            depth_of = {(s_id, im): ds.depth(s_id, im)}                                    # (the last image's is kept)
        depth = depth_of[(s_id, im)]
        cands = candidates(s_id, im, o, info, sc["gt"].get(im, []), depth)
        if clean_masks and cands:
            kept, stats = masks.clean(np.stack([c_["mask"] for c_ in cands]), depth, 0, mask_jump)
            kept, stats = kept.cpu().numpy() > 0, stats.cpu().numpy()
            for c_, m_, st_ in zip(cands, kept, stats):
                c_.update(mask=m_, clean=dict(components=int(st_[0]), kept_pixels=int(st_[2]), valid_pixels=int(st_[3])))
        shared = (time.perf_counter() - t0) / max(len(cands), 1)
        for c_ in cands:
            t0 = time.perf_counter()
            m = c_["mask"]
            gid[0] += 1
            if clean_masks and not m.any():
                skipped["empty_after_clean"] += 1
                continue
            pc, _ = ops.backproject(depth.astype(np.float64), K, m, return_device=True)    # as the depth mode does
            inst_seed = (seed * 1000003 + gid[0] - 1) & 0x7FFFFFFF
            if pc.shape[0]:
                pc = pc[ops.downsample(pc, cfg.res, inst_seed, return_device=True)]
            pc = pc.cpu().numpy()
            if pc.shape[0] > 50000:
                pc = pc[np.random.RandomState(inst_seed).randint(pc.shape[0], size=50000)]
            if pc.shape[0] < cfg.num_more + 2:
                skipped["too_few_points"] += 1
                continue
            if ((pc.max(0) - pc.min(0)).max() / cfg.res) > 1000:                           # eval.py:200
                skipped["too_large"] += 1
                continue
            key = (o, K.tobytes(), depth.shape)
            pending.setdefault(key, []).append(dict(scene_id=s_id, im_id=im, gt_index=c_["gt_index"], gid=gid[0] - 1, pc=pc,
                                                    gt=c_["gt"], depth=depth, mask=m, K=K, det=c_["det"],
                                                    prep_s=shared + time.perf_counter() - t0))
            if len(pending[key]) >= int(batch_instances):
                flush(key)
    for key in list(pending):
        flush(key)
    res = bop_data.make_results([r_["scene_id"] for r_ in rows], [r_["im_id"] for r_ in rows], [r_["obj_id"] for r_ in rows],
                                [r_["score"] for r_ in rows], np.asarray([r_["R"] for r_ in rows]).reshape(-1, 3, 3),
                                np.asarray([r_["t"] for r_ in rows]).reshape(-1, 3),
                                [im_time[(r_["scene_id"], r_["im_id"])] for r_ in rows])
    bop_data.write_results(out_csv, res)
    scored = bop_data.score(ds, bop_data.read_results(out_csv), tlist, vmin)              # the file, as a reader of it scores it
    report = dict(data="bop", bop_root=str(bop_root), split=str(split), targets=len(tlist), instances=len(summary), rows=len(rows),
                  skipped=skipped, out_csv=str(out_csv), teacher_prior=bool(teacher_prior),
                  opt_refinement="100 Adam steps (cppf_refine_pose)" if opt else "off", bop=scored, results=summary)
    if pair_tables:
        report.update(pair_tables=str(pair_tables), table_hits=[s_.get("table_hits") for s_ in summary])
    if dets is not None:
        report.update(detections=n_detections, detections_file=str(detections), det_score_min=float(det_score_min))
    if clean_masks:
        report["mask_cleaning"] = ("largest depth-connected component of each mask, neighbours within %g m "
                                   "(cppf_mask_components)" % mask_jump)
    if icp_iters > 0:
        report["icp_refinement"] = "%d point-to-plane ICP iterations against each object's model (cppf_icp_refine)" % icp_iters
        if icp_depth:
            report["icp_refinement"] = _ICP_DEPTH_NOTE % (icp_iters, "each object's model", icp_model_weight)
    if hypotheses > 1:
        report["verification"] = ("%d pose hypotheses per instance from %d peaks per vote, rendered and compared with the depth "
                                  "at tau = %g m (cppf_pose_hypotheses, cppf_depth_fit_counts)" % (hypotheses, verify.PEAKS, verify_tau))
        if centre_peaks > 1:
            report["verification"] += _CENTRE_NOTE % centre_peaks
    print(json.dumps(report if debug else {k_: v for k_, v in report.items() if k_ != "results"}))
    if out:
        with open(out, "w") as f:
            json.dump(report, f)
    return report


_ICP_DEPTH_NOTE = ("%d point-to-plane ICP iterations against %s, observed points to model and model samples to the depth image, "
                   "model weight %g (cppf_icp_refine_depth)")
_CENTRE_NOTE = "; translation hypotheses from %d separated peaks of each centre vote (cppf_grid_peaks)"


def _centre_peaks_flag(centre_peaks, hypotheses):
    centre_peaks = int(centre_peaks)
    if centre_peaks < 1:
        raise ValueError("--centre_peaks must be >= 1, not %d" % centre_peaks)
    if centre_peaks > 1 and int(hypotheses) <= 1:
        raise ValueError("--centre_peaks > 1 verifies translation hypotheses among the pose hypotheses: it needs --hypotheses > 1")
    return centre_peaks


def _teacher_prior(canon, dev):
    canon = torch.from_numpy(canon).to(dev)
    kb = torch.arange(32, device=dev, dtype=torch.float32)

    def prior(idx, base):
        coords = canon[(idx[:, :2].long() + base[:, None]).reshape(-1)].reshape(-1, 6)
        pos = (coords.clamp(-0.5, 0.5) + 0.5) * 31.0
        return ops.BinPrior(pos.contiguous(), 1.0 / 0.6)          # generated inside the fused bin draw; .dense() where an array is needed
    return prior


def main(angle_tol=1., imp_wt_margin=0.01, backproj_ratio=.1, num_pairs=50000, num_rots=180, opt=True, debug=False,
         use_grounded_sam=False, geo_branch=True, visual_branch=True, data="synthetic", num_scenes=8, num_points=4096,
         category=None, categories=None, seed=0, ckpt_dir=None, ckpt_shot=None, ckpt_dino=None, depth=None, mask=None,
         intrinsics=None, depth_scale=1000.0, out=None, out_pkl=None, log_dir=None, data_root="NOCS/real_test", out_dir=None,
         desc_npz=None, batch_instances=16, max_images=None, mesh=None, mesh_scale=1.0, icp_iters=0, gt_pose=None,
         models_info=None, hypotheses=1, verify_tau=None, bop_root=None, split="test", targets=None, out_csv=None,
         teacher_prior=False, model_scale=0.001, centre_peaks=1, detections=None, det_score_min=0.0, clean_masks=False,
         clean_mask=False, mask_jump=None, icp_depth=False, icp_model_weight=1.0, pair_table=None, pair_tables=None):
    custom = False
    if pair_table or pair_tables:
        # a known object's pair-feature table stands where the two models stood (run_table): no prior, no checkpoints
        flag = "--pair_table" if pair_table else "--pair_tables"
        if pair_table and data != "depth":
            raise ValueError("--pair_table is the table of the one object of --data=depth (--data=bop: --pair_tables=<dir>); "
                             "the synthetic and NOCS modes have no table")
        if pair_tables and data != "bop":
            raise ValueError("--pair_tables is a folder of obj_%06d.npz tables for --data=bop (--data=depth: --pair_table=<npz>)")
        if teacher_prior:
            raise ValueError("%s votes from the table: it cannot be combined with --teacher_prior" % flag)
        if ckpt_dir or ckpt_shot or ckpt_dino:
            raise ValueError("%s votes from the table: it cannot be combined with --ckpt_*" % flag)
    if data in ("depth", "bop"):
        icp_depth, icp_model_weight = _icp_depth_flag(icp_depth, icp_model_weight, icp_iters)
    elif icp_depth:
        raise ValueError("--icp_depth refines against the depth image: it needs --data=depth or --data=bop")
    clean_masks = bool(clean_masks) or bool(clean_mask)
    if mask_jump is not None and not (float(mask_jump) >= 0.0 and np.isfinite(float(mask_jump))):
        raise ValueError("--mask_jump is a distance in metres >= 0, not %r" % (mask_jump,))
    if data == "bop":
        # the BOP-dataset mode: its models come from the dataset, every other mode below runs as before
        if not bop_root or not out_csv:
            raise ValueError("--data=bop needs --bop_root (the dataset folder) and --out_csv (the results file to write)")
        if int(hypotheses) < 1:
            raise ValueError("--hypotheses must be >= 1, not %d" % int(hypotheses))
        centre_peaks = _centre_peaks_flag(centre_peaks, hypotheses)
        if gt_pose is not None or mesh:
            raise ValueError("--data=bop takes the models and the true poses from the dataset: --mesh and --gt_pose belong to --data=depth")
        dev = ops._dev()
        torch.manual_seed(seed)
        return main_bop(load_custom(ckpt_shot, ckpt_dino, device=dev, models=not pair_tables), bop_root, split, out_csv, targets,
                        float(model_scale), angle_tol, imp_wt_margin, backproj_ratio,
                        num_pairs, num_rots, opt, geo_branch, visual_branch, seed, batch_instances, int(icp_iters), int(hypotheses),
                        verify_tau, bool(teacher_prior), None, debug, out, centre_peaks, detections, float(det_score_min), clean_masks,
                        mask_jump, icp_depth, icp_model_weight, pair_tables)
    if detections is not None:
        raise ValueError("--detections is a BOP detections file: it needs --data=bop")
    if clean_masks and data != "depth":
        raise ValueError("--clean_masks cleans instance masks against the depth image: it needs --data=bop or --data=depth")
    if teacher_prior:
        raise ValueError("--teacher_prior builds the prior from a BOP dataset's ground-truth poses: it needs --data=bop")
    icp_iters = int(icp_iters)
    hypotheses = int(hypotheses)
    if hypotheses < 1:
        raise ValueError("--hypotheses must be >= 1, not %d" % hypotheses)
    if hypotheses > 1 and (data != "depth" or not mesh):
        raise ValueError("--hypotheses > 1 verifies poses against the object's mesh: it needs --data=depth and --mesh")
    centre_peaks = _centre_peaks_flag(centre_peaks, hypotheses)
    if icp_iters > 0 and (data != "depth" or not mesh):
        raise ValueError("--icp_iters > 0 refines against the object's mesh: it needs --data=depth and --mesh")
    if gt_pose is not None and (data != "depth" or not mesh):
        raise ValueError("--gt_pose scores the pose against the object's mesh (BOP metrics): it needs --data=depth and --mesh")
    icp_model = None
    if icp_iters > 0:
        from cppf2_amd import icp, render
        icp_model = icp.ModelPoints.from_mesh(render.load_mesh(mesh, mesh_scale))
    bop_obj = None
    if gt_pose is not None:
        from cppf2_amd import bop, render
        info = None
        if models_info:
            with open(models_info) as f:
                info = json.load(f)
        bop_obj = bop.ObjectInfo.from_mesh(render.load_mesh(mesh, mesh_scale), models_info=info, mesh_scale=mesh_scale)
        gt_R, gt_t = bop.load_pose(gt_pose)
        bop_reported, bop_width = [], None
    verify_obj = None
    if hypotheses > 1:
        from cppf2_amd import bop, render, verify
        verify_tau = verify.TAU if verify_tau is None else float(verify_tau)
        verify_obj = bop_obj if bop_obj is not None else bop.ObjectInfo.from_mesh(render.load_mesh(mesh, mesh_scale))
    if categories is None:
        if category:
            categories = [category]
        elif data == "depth":
            # a single depth + mask pair is one instance; without --category it is an instance-level object like the
            # reference's example (a YCB object: config/custom.yaml, no category group, full rotation)
            categories, custom = ["custom"], True
        else:
            categories = [id2category[i] for i in range(1, 7)]                             # eval.py:87-90
    elif isinstance(categories, str):
        categories = [c for c in categories.replace(" ", "").split(",") if c]
    categories = [c for c in categories if c in WHITELIST or custom]
    dev = ops._dev()
    torch.manual_seed(seed)
    # eval.py:84-101: models and cfgs of every category up front
    if custom:
        setups = {"custom": load_custom(ckpt_shot, ckpt_dino, device=dev, models=not pair_table)}
    else:
        setups = {c: load_category(c, ckpt_dir, ckpt_shot, ckpt_dino, device=dev) for c in categories}
    if data == "nocs":
        assert log_dir, "--data=nocs needs --log_dir (the directory of results_*.pkl, eval.py:72-76)"
        return main_nocs(setups, log_dir, data_root, out_dir, desc_npz, angle_tol, imp_wt_margin, backproj_ratio, num_pairs,
                         num_rots, opt, geo_branch, visual_branch, seed, batch_instances, intrinsics, max_images, debug, out)

    from cppf2_amd import metrics
    summary, all_cls, all_RT, all_scale, all_gt, all_gt_scale = [], [], [], [], [], []
    inst = 0
    for ci, cat in enumerate(categories):
        cfg, dino_model, shot_model = setups[cat]
        up_sym = cat in UP_SYM or bool(cfg.get("up_sym", False))
        # ---- instances ---------------------------------------------------------------------------
        if data == "depth":
            from PIL import Image
            d = np.array(Image.open(depth)).astype(np.float64) / float(depth_scale)
            m = np.array(Image.open(mask))
            m = (m[..., 0] if m.ndim == 3 else m) > 0
            if clean_masks:
                # the largest depth-connected component of the mask (cppf_mask_components): what is back-projected and verified
                from cppf2_amd import masks
                kept, stats = masks.clean(m[None], d.astype(np.float32), 0, masks.JUMP if mask_jump is None else float(mask_jump))
                m = kept[0].cpu().numpy() > 0
                mask_stats = [int(x) for x in stats[0].cpu().numpy()]
                if not m.any():
                    raise ValueError("--clean_mask: no depth-connected component of the mask has %d pixels" % masks.MIN_PIXELS)
            K = np.array(intrinsics if intrinsics is not None else
                         [[591.0125, 0, 322.525], [0, 590.16775, 244.11084], [0, 0, 1]], dtype=np.float64).reshape(3, 3)
            pc, _ = ops.backproject(d, K, m, return_device=True)               # eval.py:185-189 (flip + f32 cast folded in)
            pc = pc[ops.downsample(pc, cfg.res, seed, return_device=True)].cpu().numpy()   # eval.py:192
            if pc.shape[0] > 50000:
                pc = pc[np.random.RandomState(seed).randint(pc.shape[0], size=50000)]
            scenes = [dict(pc=pc, pc_canon=None, R=None, t=None)]
        else:
            scenes = [synth.make_scene(seed, inst + s, num_points) for s in range(num_scenes)]
        made = len(scenes)
        keep_ids = [inst + j for j, s in enumerate(scenes) if ((s["pc"].max(0) - s["pc"].min(0)).max() / cfg.res) <= 1000]
        scenes = [s for s in scenes if ((s["pc"].max(0) - s["pc"].min(0)).max() / cfg.res) <= 1000]     # eval.py:200
        B = len(scenes)
        if B == 0:
            inst += made
            continue
        scene_ids = keep_ids          # a dropped instance does not shift the others' seeds (tuple / uniform streams = scene seed)
        # DINOv2 features are inputs to the path (weights absent): seeded unit vectors stand in for them
        g = torch.Generator(device="cpu").manual_seed(seed + 1 + ci)
        descs = [torch.nn.functional.normalize(torch.randn((s["pc"].shape[0], 1024), generator=g), dim=-1).numpy()
                 for s in ([] if pair_table else scenes)]          # (a table pass reads no descriptor)
        priors = scale_priors = None
        if scenes[0]["pc_canon"] is not None:
            priors = _teacher_prior(np.concatenate([s["pc_canon"] for s in scenes]), dev)
            scale_priors = np.stack([s["extent"] for s in scenes])
        if pair_table:
            r = run_table(cfg, load_pair_table(pair_table, dev), [s["pc"] for s in scenes], seed, scene_ids, num_pairs, num_rots,
                          angle_tol, imp_wt_margin, backproj_ratio, bool(opt), up_sym,
                          hypotheses if verify_obj is not None else None, centre_peaks)
        else:
            r = run_ensemble(cfg, dino_model, shot_model, [s["pc"] for s in scenes], descs, seed, scene_ids, num_pairs,
                             num_rots, angle_tol, imp_wt_margin, backproj_ratio, bool(opt), geo_branch, visual_branch,
                             up_sym, priors, scale_priors=scale_priors, hypotheses=hypotheses if verify_obj is not None else None,
                             centre_peaks=centre_peaks)
        cls_id = category2id.get(cat, 0)
        icp_stats = None
        ver = None
        if verify_obj is not None:
            ver = _verify_instances(r, B, hypotheses, (True, False) if pair_table else (geo_branch, visual_branch), verify_obj, d, m, K,
                                    np.cumsum([0] + [s["pc"].shape[0] for s in scenes]), icp_model, icp_iters, verify_tau,
                                    icp_depth, icp_model_weight)
            if icp_model is not None:
                icp_stats = ver["icp"][np.arange(B), np.maximum(ver["chosen"], 0)]
        elif icp_model is not None:
            # after the ensemble selection (and `opt`): the selected record of each instance against the mesh
            extra = dict(depth=d.astype(np.float32), K=K, model_weight=icp_model_weight) if icp_depth else {}
            icp_stats = icp.refine(icp_model, r["pts"], np.cumsum([0] + [s["pc"].shape[0] for s in scenes]), r["selected"],
                                   iters=icp_iters, **extra)
        for b in range(B):
            RT, sc = np.eye(4), np.ones(3)                                      # eval.py:143-144 defaults
            item = dict(scene=scene_ids[b], category=cat, model=None)
            if r["pick"][b] >= 0:                                               # eval.py:367-372
                rec = r["records"][r["pick"][b]][b] if icp_stats is None else r["selected"][b]
                if ver is not None:
                    rec = ver["records"][b]
                RT[:3, :3] = rec["R"] * r["scale_norm"][b]
                RT[:3, 3] = rec["t"]
                if r["scale_norm"][b] > 0:
                    sc = r["scale"][b] / r["scale_norm"][b]
                item.update(model="table" if pair_table else ["dino", "shot"][r["pick"][b]], loss=float(r["best"][b]),
                            losses=[float(r["losses"][0][b]), float(r["losses"][1][b])], pred_RT=RT.tolist(),
                            pred_scale=sc.tolist())
                if icp_stats is not None:
                    item["icp"] = _icp_item(icp_stats[b])
                if ver is not None:
                    c_ = int(ver["chosen"][b])
                    item["verify"] = dict(hypotheses=int(np.count_nonzero((ver["hypotheses"][b]["flags"] & verify.EMPTY) == 0)),
                                          chosen=c_, score=float(ver["scores"][b, c_]), score_first=float(ver["scores"][b, 0]))
                    if centre_peaks > 1:
                        item["verify"]["centre_peak"] = int(ver["centre_peak"][b])
                if scenes[b]["R"] is not None:
                    item["tr_err_cm"] = float(np.linalg.norm(rec["t"] - scenes[b]["t"]) * 100)
                    item["rot_err_deg"] = geometry.rot_err_deg(rec["R"], scenes[b]["R"], up_sym)
            if pair_table:
                item["table_hits"] = [int(x) for x in r["table_hits"][b]]
            summary.append(item)
            all_cls.append(cls_id); all_RT.append(RT); all_scale.append(sc)
            if scenes[b]["R"] is not None:
                # synthetic instances carry their pose and box: NOCS convention, rotation scaled by the box diagonal and
                # the extents normalised by it (what eval.py:370-372 builds from the prediction)
                gt = np.eye(4)
                gt[:3, :3], gt[:3, 3] = scenes[b]["R"] * scenes[b]["diag"], scenes[b]["t"]
                all_gt.append(gt)
                all_gt_scale.append(scenes[b]["extent"] / scenes[b]["diag"])
        if bop_obj is not None:
            # the BOP errors of each instance's reported pose (and of its pose before ICP) against --gt_pose, on the depth
            # image and K loaded above; an instance without an estimate scores +inf
            nan = (np.full((3, 3), np.nan), np.full(3, np.nan))
            reported = [(r["records"][r["pick"][b]][b] if icp_stats is None else r["selected"][b]) if r["pick"][b] >= 0 else None
                        for b in range(B)]
            if ver is not None:
                first = [ver["hypotheses"][b, 0] if r["pick"][b] >= 0 else None for b in range(B)]
                reported = [ver["records"][b] if r["pick"][b] >= 0 else None for b in range(B)]
            poses = [(p_["R"], p_["t"]) if p_ is not None else nan for p_ in reported]
            if ver is not None:
                poses += [(p_["R"], p_["t"]) if p_ is not None else nan for p_ in first]
            if icp_stats is not None:
                poses += [(r["records"][r["pick"][b]][b]["R"], r["records"][r["pick"][b]][b]["t"]) if r["pick"][b] >= 0 else nan
                          for b in range(B)]
            err = bop.pose_errors(bop_obj, d, np.zeros(len(poses), dtype=np.int64), [p_[0] for p_ in poses],
                                  [p_[1] for p_ in poses], [gt_R] * len(poses), [gt_t] * len(poses), K)

            def block(j):
                return dict(vsd=[float(x) for x in err["vsd"][j]], mssd=float(err["mssd"][j]), mspd=float(err["mspd"][j]))
            nv = B if ver is not None else 0
            for b, item in enumerate(summary[len(summary) - B:]):
                item["bop"] = block(b)
                if ver is not None:
                    item["bop_first"] = block(B + b)
                if icp_stats is not None:
                    item["bop_before_icp"] = block(B + nv + b)
            bop_reported.append({k_: v_[:B] for k_, v_ in err.items()})
            bop_width = d.shape[1]
        inst += made

    report = dict(categories=categories, instances=len(summary),
                  opt_refinement="100 Adam steps (cppf_refine_pose)" if opt else "off", results=summary)
    if pair_table:
        report.update(pair_table=str(pair_table), table_hits=[s_["table_hits"] for s_ in summary])
    if clean_masks:
        report["mask_cleaning"] = dict(components=mask_stats[0], kept_pixels=mask_stats[2], valid_pixels=mask_stats[3])
    if icp_model is not None:
        report["icp_refinement"] = "%d point-to-plane ICP iterations against %s (cppf_icp_refine)" % (icp_iters, os.path.basename(mesh))
        if icp_depth:
            report["icp_refinement"] = _ICP_DEPTH_NOTE % (icp_iters, os.path.basename(mesh), icp_model_weight)
        report["icp"] = [s_["icp"] for s_ in summary if "icp" in s_]
    if verify_obj is not None:
        report["verification"] = ("%d pose hypotheses per instance from %d peaks per vote, rendered and compared with the depth "
                                  "at tau = %g m (cppf_pose_hypotheses, cppf_depth_fit_counts)" % (hypotheses, verify.PEAKS, verify_tau))
        if centre_peaks > 1:
            report["verification"] += _CENTRE_NOTE % centre_peaks
    if bop_obj is not None and bop_reported:
        errs = {k_: np.concatenate([e_[k_] for e_ in bop_reported]) for k_ in ("vsd", "mssd", "mspd")}
        report["bop"] = dict(bop.average_recall(errs, bop_obj.diameter, bop_width), delta=bop.DELTA, taus=list(bop.TAUS))
    if len(categories) == 1:
        report["category"] = categories[0]
    scored = [s for s in summary if "rot_err_deg" in s]
    if scored:
        report["acc_5deg_5cm"] = float(np.mean([s["rot_err_deg"] < 5 and s["tr_err_cm"] < 5 for s in scored]))
        report["acc_5deg_5cm_per_category"] = {
            c: float(np.mean([s["rot_err_deg"] < 5 and s["tr_err_cm"] < 5 for s in scored if s["category"] == c]))
            for c in categories if any(s["category"] == c for s in scored)}
    # the reference's per-image result record (eval.py:143-147, 370-372, 399): pred_RTs [n,4,4] (rotation scaled by the
    # scale norm), pred_scales [n,3] (normalised); all instances of the run form one record, like those of one image
    n = len(summary)
    gt = {}
    if n and len(all_gt) == n:
        gt = dict(gt_class_ids=np.array(all_cls), gt_RTs=np.stack(all_gt), gt_scales=np.stack(all_gt_scale))
    record = metrics.make_result_record(np.array(all_cls, dtype=np.int64), np.stack(all_RT) if n else np.zeros((0, 4, 4)),
                                        np.stack(all_scale) if n else np.zeros((0, 3)), None, **gt)
    if gt:
        # eval.py:400-411: degree / cm AP over the instances matched at 3-D IoU > 0.1, and the 3-D IoU AP itself
        thr = np.linspace(0, 1, 101)
        iou_aps, aps = metrics.degree_cm_mAP([record], metrics.SYNSET_NAMES, (5, 10, 15), (5, 10, 15), thr, 0.1, True)
        scored_cats = sorted({s_["category"] for s_ in summary if s_["category"] in category2id})

        def _mean(vals):                      # categories without a scored instance have NaN APs: they do not enter the mean
            vals = [v for v in vals if np.isfinite(v)]
            return float(np.mean(vals)) if vals else None
        report["pose_AP"] = {"%ddeg_%dcm" % (d_, s_): _mean([aps[category2id[c], i_, j_] for c in scored_cats])
                             for i_, d_ in enumerate((5, 10, 15)) for j_, s_ in enumerate((5, 10, 15))}
        report["pose_AP_per_category"] = {c: {"%ddeg_%dcm" % (d_, s_): float(aps[category2id[c], i_, j_])
                                              for i_, d_ in enumerate((5, 10, 15)) for j_, s_ in enumerate((5, 10, 15))}
                                          for c in scored_cats}
        report["iou_AP"] = {"IoU%d" % t_: _mean([iou_aps[category2id[c], t_] for c in scored_cats]) for t_ in (25, 50, 75)}
    if out_pkl:
        import pickle
        with open(out_pkl, "wb") as f:
            pickle.dump(record, f)
    print(json.dumps(report if debug else {k_: v for k_, v in report.items() if k_ != "results"}))
    if out:
        with open(out, "w") as f:
            json.dump(report, f)
    return report


if __name__ == "__main__":
    kwargs = {}
    for a in sys.argv[1:]:
        if a.startswith("--") and "=" in a:
            k_, v_ = a[2:].split("=", 1)
            kwargs[k_] = _flag(v_)
        elif a.startswith("--"):
            kwargs[a[2:]] = True
    main(**kwargs)
