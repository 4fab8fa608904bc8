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
  * `--data=depth --mesh=<ply|obj> --detect_symmetries [--sym_tol=0.01]` finds the mesh's rotational symmetries on the GPU
    (cppf2_amd.symmetry, cppf_sym_deviation) where --models_info would supply them: the object scored by
    --gt_pose is built from the detected entry, and the report gains `symmetries` (counts, continuous axes, the largest accepted
    and the smallest refused deviation over the diameter).  --sym_tol: a symmetry deviates by at most that share of the
    diameter.  Off by default.
  * `--data=nocs --iou_device` scores the 3-D box overlaps of the NOCS scorer on the GPU (cppf2_amd.box_iou, cppf_box_iou, DESIGN.md
    section 27): metrics.degree_cm_mAP(iou="device"), every same-class (prediction, ground truth) pair of the run in one batched
    call instead of one convex hull per pair and turn on the host; the report gains `scorer_seconds`.  Off by default.
    `python -m cppf2_amd.metrics --results <out_dir> [--iou host|device]` scores the records --out_dir saved without voting again.
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
  * `--data=depth --propose_masks [--plane_hypotheses=256 --plane_tau=0.005 --plane_min_height=0.01 --mask_jump=0.01
    --min_segment_pixels=200 --max_proposals=16]` stands where --mask stood: the support plane of the depth image is fitted and
    dropped and what is left is cut into depth-connected segments (cppf2_amd.segment; the plane's
    hypotheses are drawn from --seed).  Every proposal is one instance of the batch, with the tuple streams a --mask run of its
    mask would have; proposals wider than 1000 cells or with too few points are skipped and counted.  The report gains `plane`,
    `proposals` (pixels, bbox, pose; the verification score with --hypotheses > 1) and, with --hypotheses > 1, `best`: the
    proposal with the highest score, ties to the larger one.  --gt_pose scores `best` when it exists, else every proposal.
    `--propose_concave [--concave_step=3 --concave_angle=15 --concave_floor=0.002 --concave_reach=<step x 0.01>]` removes the
    locally concave pixels from what is labelled (cppf_concave_edges): touching and stacked objects
    part, and the contact line with the table is cut where it is.  `--propose_no_plane` (needs --propose_concave) fits no
    support plane -- a shelf, a bin, a tray: every valid pixel is labelled, the table is a proposal of its own, which goes
    through the same too-wide and too-few-points skips and otherwise scores low in the verification, and the report's plane
    is four zeros; --support_check and the --plane_* flags need the plane and are refused beside it.  The report gains `concave` (the settings; valid, edge and kept pixels).
  * `--data=depth --propose_masks --explain_scene [--explain_min_score=0.5 --explain_min_gain=200 --explain_viol_weight=1
    --explain_max=16]` (with --hypotheses > 1 and a mesh) decides per image, not per mask (cppf2_amd.scene, cppf_scene_explain,
    DESIGN.md section 22; not in the reference): the verified pose of every proposal with a verification score of at least
    --explain_min_score is a candidate (the 64 best when there are more), the region is the union of the proposed masks, and
    the candidates that together explain it, each pixel counted once, are chosen greedily.  The report gains `scene`:
    `instances` in chosen order (proposal, object, R, t, score, gain, net), `explained_pixels`, `region_pixels`, `rejected`
    (reason `below_min_score` or `no_gain`) and `dropped`; everything else in the report stays what it is without the flag.
    `--models_dir=<BOP models dir> --pair_tables=<dir> [--obj_ids=1,5 --model_scale=0.001]` stands in for --mesh and
    --pair_table: obj_%06d.ply (+ models_info.json) and obj_%06d.npz per object; the proposal path runs once per object id,
    the candidates of all objects are pooled into one explanation, and every result, proposal and instance carries `obj_id`.
    `--explain_hypotheses [--explain_min_support=0.5]` makes every verified hypothesis of every proposal a candidate, not only
    the one the verification kept, so that two objects that touch -- one depth segment, one proposal -- can both be found
    (cppf_scene_explain_wide).  The gate is the hypothesis' support, fit / drawn: the share of what the
    pose shows the camera that the depth confirms (the per-mask score divides by the whole mask, which two objects share; 0.5
    is "at least half", not swept), so --explain_min_score is refused beside it.  The 512 best supported are kept when there
    are more (`dropped`); instances and rejected entries gain `hypothesis` and `support`, the reasons are `below_min_support`
    and `no_gain`, and `parameters` gains `min_support` and `hypotheses`.
    `--support_check [--support_tau=0.01 --support_max_share=0.1]` (needs --hypotheses > 1 and a mesh)
    refuses a hypothesis whose nearest back faces lie more than support_tau under the plane the proposals were cut with on
    more than that share of their pixels (cppf_support_counts): it scores 0 in the verification and is `below_table` in the
    explanation.  `--explain_solid [--solid_tau=0.02 --solid_max_share=0.1]` (needs --explain_scene) makes a candidate
    ineligible once more than that share of the smaller solid of it and an earlier instance lies inside the other by more
    than solid_tau (cppf_solid_overlap): reason `inside`, `inside_of` the instance's index.  The report gains `support` and
    `refused` per hypothesis under `verify`, `support_counts` per candidate of the scene, `scene.passes` and `solid_checks`.
  * `--condition_depth [--flying_radius=1 --flying_support=4 --smooth_radius=0 --depth_jump=0.01 --depth_jump_rel=0]`
    (--data=depth and --data=bop; cppf2_amd.depthfilter, cppf_depth_condition; not in the reference)
    conditions every depth image once, right after it is read and scaled: a reading with fewer than --flying_support of its
    (2 flying_radius + 1)^2 - 1 neighbours within depth_jump + depth_jump_rel * z of it -- a mixed pixel on a silhouette --
    becomes 0, and with --smooth_radius > 0 every kept reading becomes the mean of itself and the pairs of opposite neighbours
    within that gate.  Mask cleaning, proposals, back-projection, verification, --icp_depth and the scene explanation then all
    read the conditioned image.  The report gains `depth_condition` (the settings; valid, removed and smoothed pixels).  Off
    by default, and without it nothing changes.
Swapped flag names are kept: geo_branch gates model 0 (DINO), visual_branch gates model 1 (SHOT) (eval.py:367).
"""
import collections
import json
import os
import sys
import time
import types

import numpy as np
import torch

from cppf2_amd import geometry, ops, synth
from cppf2_amd.config import load_checkpoint_config, load_config
from cppf2_amd.ensemble import (PIPE_CACHE_BYTES, PIPE_CACHE_MAX, _PIPES, _TABLES, Stages, _hypothesis_args, _icp_item,  # noqa: F401
                                _instance_hypotheses, _pass_hypotheses, _pass_output, _pipelines, _side_streams, _teacher_prior,
                                _verify_instances, _vote_cap, instance_cloud, instance_items, load_pair_table, needed_cells,
                                refine_and_verify, run_ensemble, run_table, stage_notes, stand_in_descriptors, too_wide,
                                usable_cloud)
from cppf2_amd.models import BeyondCPPFDino, BeyondCPPFShot, load_reference_checkpoint
from cppf2_amd.ops import get_topk_dir  # noqa: F401  (the reference defines it in this file, eval.py:37-51; demo.py and the notebook import it from here)

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
        inst_seed = (seed * 1000003 + image_index * 131 + i) & 0x7FFFFFFF
        pc, idxs = instance_cloud(depth / 1000., K, mask, cfg.res, inst_seed, pixels=True)  # eval.py:185-197; idxs: K x 2 (row, col)
        if pc.shape[0] == 0 or too_wide(pc, cfg.res):                                      # eval.py:199-200
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


# the nine voting parameters that travel from the flags to run_ensemble / run_table unchanged
Vote = collections.namedtuple("Vote", "angle_tol imp_wt_margin backproj_ratio num_pairs num_rots opt geo_branch visual_branch seed")


def vote_batch(setup, pcs, descs, scene_ids, v, up_sym, priors=None, scale_priors=None, stages=None, table=None):
    """One batch of instances through both models of setup = (cfg, dino_model, shot_model) (run_ensemble: this module's, looked
    up when called), or through the object's pair-feature table when there is one (run_table); v: the Vote parameters; stages:
    the Stages settings, whose hypotheses and centre_peaks the vote keeps records for (None: the vote alone).
    Returns (their dict, the (model 0, model 1) pair of passes that took part)."""
    cfg, dino_model, shot_model = setup
    H = stages.hypotheses if stages is not None and stages.hypotheses > 1 else None
    centre_peaks = 1 if stages is None else stages.centre_peaks
    if table is not None:
        return run_table(cfg, table, pcs, v.seed, scene_ids, v.num_pairs, v.num_rots, v.angle_tol, v.imp_wt_margin, v.backproj_ratio,
                         bool(v.opt), up_sym, H, centre_peaks), (True, False)
    return run_ensemble(cfg, dino_model, shot_model, pcs, descs, v.seed, scene_ids, v.num_pairs, v.num_rots, v.angle_tol,
                        v.imp_wt_margin, v.backproj_ratio, bool(v.opt), v.geo_branch, v.visual_branch, up_sym, priors,
                        scale_priors=scale_priors, hypotheses=H, centre_peaks=centre_peaks), (v.geo_branch, v.visual_branch)


def _opt_note(vote):
    return "100 Adam steps (cppf_refine_pose)" if vote.opt else "off"


def _emit(report, debug, out):
    """The report printed as one JSON line, without its per-instance `results` unless debug, and written whole to `out`."""
    print(json.dumps(report if debug else {k_: v for k_, v in report.items() if k_ != "results"}))
    if out:
        with open(out, "w") as f:
            json.dump(report, f)
    return report


def main_nocs(setups, vote, log_dir, data_root="NOCS/real_test", out_dir=None, desc_npz=None, batch_instances=16, intrinsics=None,
              max_images=None, debug=False, out=None, iou_device=False):
    """eval.py:103-412 on a directory in the reference's layout: `log_dir`/results_*.pkl (detections + ground truth per image)
    and `data_root`/<scene>/<frame>_{depth,color}.png.  Instances are collected image by image exactly as the reference
    filters them, evaluated in batches per category on the GPU (run_ensemble), and written back into their image's record
    (pred_RTs, pred_scales: eval.py:143-147, 370-372); every record is pickled under out_dir with the reference's file name
    (eval.py:134, 399) and the list is scored with degree_cm_mAP (eval.py:400-412); iou_device: with its box overlaps from the
    GPU (degree_cm_mAP(iou="device")), and the report gains `scorer_seconds`.
    desc_npz: optional .npz of DINOv2 patch-token maps float32 [1024, 64, 64] keyed "<image index>_<instance index>" (the
    crop of eval.py:177-183 at stride 4); without it seeded unit vectors stand in (the DINO branch then votes on noise)."""
    import pickle
    from cppf2_amd import metrics
    dev = ops._dev()
    seed = vote.seed
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
        # no token maps: the stand-in, one stream per instance -- the same numbers on every device and in every round (round 4
        # drew them with a device generator, whose stream is not the CPU's: seeded `--data=nocs` stand-in runs were not
        # comparable with earlier ones)
        descs = [stand_in_descriptors(pc.shape[0], seed * 7919 + g_ + 1).to(dev) if desc is None else desc
                 for (_, _, g_, pc, desc) in chunk]
        r, _ = vote_batch(setups[cat], [c_[3] for c_ in chunk], descs, [c_[2] for c_ in chunk], vote, cat in UP_SYM)
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
    t_scorer = time.perf_counter()
    iou_aps, aps = metrics.degree_cm_mAP(final_results, metrics.SYNSET_NAMES, (5, 10, 15), (5, 10, 15),
                                         np.linspace(0, 1, 101), 0.1, True,                # eval.py:400-411
                                         iou="device" if iou_device else "host")
    t_scorer = time.perf_counter() - t_scorer
    cats = [c for c in setups if seen[c]]
    report = dict(data="nocs", images=len(final_results), detections=total, evaluated=evaluated, skipped=total - evaluated,
                  picked=picks, categories=cats, descriptors="token maps from %s" % desc_npz if desc_npz else "seeded unit vectors (no DINOv2 tokens given)",
                  **metrics.nocs_summary(iou_aps, aps, [category2id[c] for c in cats]))
    if iou_device:
        report["scorer_seconds"] = t_scorer
    _emit(report, debug, out)                       # (it has no `results`: the whole report either way)
    report["final_results"] = final_results
    return report


def _icp_depth_flag(icp_depth, icp_model_weight, icp_iters):
    if icp_depth and int(icp_iters) <= 0:
        raise ValueError("--icp_depth adds the model-to-depth terms to the ICP refinement: it needs --icp_iters > 0")
    w = float(icp_model_weight)
    if not (w > 0 and np.isfinite(w)):
        raise ValueError("--icp_model_weight must be finite and > 0, not %r" % (icp_model_weight,))
    if w != 1.0 and not icp_depth:
        raise ValueError("--icp_model_weight weighs the model-to-depth terms: it needs --icp_depth")
    return bool(icp_depth), w


def main_bop(setup, vote, stages, bop_root, split, out_csv, targets=None, mesh_scale=0.001, batch_instances=16, teacher_prior=False,
             visib_gt_min=None, debug=False, out=None, detections=None, det_score_min=0.0, clean_masks=False, mask_jump=None,
             pair_tables=None, condition=None):
    """The instance-level path over one split of a BOP-format dataset (cppf2_amd.bop_data.Dataset): one estimate per valid
    ground-truth instance of every target, from its visible mask; poses written to `out_csv` in BOP's frame and scored with
    bop_data.score.  Instances of one object (and one K and image size) are evaluated in batches of `batch_instances` across
    images.  detections: a detections file (bop_data.read_detections); every detection of a target's object in its image with
    score >= det_score_min then stands where the ground-truth instances stood, its mask decoded on the GPU (masks.decode_batch,
    one call per target), and gives one CSV row (score: the detection's, times the verification score with hypotheses > 1).
    pair_tables: a folder of obj_%06d.npz pair-feature tables (python -m cppf2_amd.pair_table): each object's instances are then
    voted from its table (run_table) instead of the two model passes; no prior.
    clean_masks: every mask is cut down to its largest depth-connected component (masks.clean, mask_jump metres) before
    back-projection and verification.  condition: a depthfilter.Settings record or None; every depth image is then conditioned
    once, right after it is read, and every step reads the conditioned image (the report's `depth_condition`: the counts summed
    over the images).  Returns the report (report["bop"] = bop_data.score's)."""
    import time
    from cppf2_amd import bop, bop_data, depthfilter, icp, masks
    dev = ops._dev()
    cfg, seed = setup[0], vote.seed
    conditioned = []
    if pair_tables and teacher_prior:             # main() has checked this; kept for callers of this function, which is public
        raise ValueError("--pair_tables votes from the tables: it cannot be combined with --teacher_prior")
    up_sym = bool(cfg.get("up_sym", False))
    vmin = bop_data.VISIB_GT_MIN if visib_gt_min is None else float(visib_gt_min)
    ds = bop_data.Dataset(bop_root, split, mesh_scale)
    tlist = ds.targets(targets, vmin)
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

    def flush(key):
        chunk, pending[key] = pending.get(key, []), []
        if not chunk:
            return
        t0 = time.perf_counter()
        o = key[0]
        obj = ds.object(o)
        B = len(chunk)
        descs = [] if pair_tables else [stand_in_descriptors(c_["pc"].shape[0], seed * 7919 + c_["gid"] + 1).numpy() for c_ in chunk]
        priors = scale_priors = None
        if teacher_prior:
            # the synthetic mode's stand-in (synth.make_scene): canonical coordinates (pc - t) @ R / diag from the true pose
            ext = obj.verts.max(0) - obj.verts.min(0)
            diag = float(np.linalg.norm(ext))
            canon = [((c_["pc"].astype(np.float64) - c_["gt"]["t"]) @ c_["gt"]["R"] / diag).astype(np.float32) for c_ in chunk]
            priors = _teacher_prior(np.concatenate(canon), dev)
            scale_priors = np.stack([ext] * B)
        table = load_pair_table(os.path.join(str(pair_tables), "obj_%06d.npz" % o), dev) if pair_tables else None
        r, enabled = vote_batch(setup, [c_["pc"] for c_ in chunk], descs, [c_["gid"] for c_ in chunk], vote, up_sym, priors,
                                scale_priors, stages, table)
        if stages.icp_iters > 0 and o not in icp_models:
            icp_models[o] = icp.ModelPoints.from_mesh(ds.mesh(o))
        images = stages.hypotheses > 1 or stages.icp_depth       # (the stages that read the instances' images)
        reported, icp_stats, ver = refine_and_verify(
            r, enabled, obj, np.stack([c_["depth"] for c_ in chunk]) if images else None,
            np.stack([c_["mask"] for c_ in chunk]) if images else None, chunk[0]["K"],
            np.cumsum([0] + [c_["pc"].shape[0] for c_ in chunk]), icp_models.get(o), stages)
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
            rec = reported[b]
            item.update(instance_items(r, b, icp_stats, ver, stages))
            score = -float(r["best"][b])
            if ver is not None:
                if ver["chosen"][b] < 0:           # every hypothesis empty: the CSV's score stays a number
                    item["verify"]["score"] = 0.0
                score = item["verify"]["score"]
            Rb, tb = bop.pose_to_bop(np.asarray(rec["R"], dtype=np.float64).reshape(3, 3), np.asarray(rec["t"], dtype=np.float64), mesh_scale,
                                     obj.centre)
            if dets is not None:
                score = c_["det"]["score"] * score if ver is not None else c_["det"]["score"]
            item.update(model="table" if pair_tables else ["dino", "shot"][r["pick"][b]], loss=float(r["best"][b]), score=score)
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
            if condition is not None:
                raw = depth_of[(s_id, im)]
                dc, counted = depthfilter.apply(raw.astype(np.float32), condition, "eval.py")
                depth_of[(s_id, im)] = dc[0].cpu().numpy().astype(raw.dtype)
                conditioned.append(counted)
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
            pc, why = usable_cloud(depth.astype(np.float64), K, m, cfg, (seed * 1000003 + gid[0] - 1) & 0x7FFFFFFF)   # as the depth mode does
            if pc is None:
                skipped[why] += 1
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
                  opt_refinement=_opt_note(vote), bop=scored, results=summary)
    if pair_tables:
        report.update(pair_tables=str(pair_tables), table_hits=[s_.get("table_hits") for s_ in summary])
    if dets is not None:
        report.update(detections=n_detections, detections_file=str(detections), det_score_min=float(det_score_min))
    cleaning = ("largest depth-connected component of each mask, neighbours within %g m (cppf_mask_components)" % mask_jump
                if clean_masks else None)
    report.update(stage_notes("each object's model", stages, cleaning))
    if condition is not None:
        report["depth_condition"] = (depthfilter.merged(conditioned) if conditioned
                                     else depthfilter.summary(condition, np.zeros((0, 3), np.int64)))
    return _emit(report, debug, out)


def _symmetry_flags(f):
    """The tolerance of --detect_symmetries (a share of the diameter), or None when it is off."""
    if not f.detect_symmetries:
        if f.sym_tol is not None:
            raise ValueError("--sym_tol sets the tolerance of --detect_symmetries: it needs that flag")
        return None
    if f.models_info:
        raise ValueError("--detect_symmetries finds the symmetries --models_info would supply: give one of them")
    if f.data != "depth" or not f.mesh:
        raise ValueError("--detect_symmetries finds the symmetries of the one object of --mesh: it needs --data=depth and --mesh")
    from cppf2_amd import symmetry
    tol = symmetry.TOL if f.sym_tol is None else float(f.sym_tol)
    if not (tol > 0.0 and np.isfinite(tol)):
        raise ValueError("--sym_tol is a share of the diameter > 0, not %r" % (f.sym_tol,))
    return tol


def _centre_peaks_flag(centre_peaks, hypotheses):
    centre_peaks = int(centre_peaks)
    if centre_peaks < 1:
        raise ValueError("--centre_peaks must be >= 1, not %d" % centre_peaks)
    if centre_peaks > 1 and int(hypotheses) <= 1:
        raise ValueError("--centre_peaks > 1 verifies translation hypotheses among the pose hypotheses: it needs --hypotheses > 1")
    return centre_peaks


_PROPOSE_FLAGS = ("plane_tau", "plane_hypotheses", "plane_min_height", "min_segment_pixels", "max_proposals")


def _propose_flags(f):
    """segment.propose's keyword arguments from the --propose_masks flags, or None when it is off."""
    from cppf2_amd import segment
    given = [k_ for k_ in _PROPOSE_FLAGS if getattr(f, k_) is not None]
    concave = segment.concave_from_flags(bool(f.propose_concave), {k_: getattr(f, k_) for k_ in segment.CONCAVE_FLAGS})
    if f.propose_no_plane and concave is None:
        raise ValueError("--propose_no_plane leaves the concave edges to part the objects from the table: it needs --propose_concave")
    if not f.propose_masks:
        if given:
            raise ValueError("--%s sets how masks are proposed: it needs --propose_masks" % given[0])
        if concave is not None:
            raise ValueError("--propose_concave sets how masks are proposed: it needs --propose_masks")
        return None
    if f.data != "depth":
        raise ValueError("--propose_masks proposes the masks of one depth image: it needs --data=depth "
                         "(--data=bop: python -m cppf2_amd.segment writes a detections file)")
    if f.mask:
        raise ValueError("--propose_masks replaces --mask: give one of them")
    if bool(f.clean_masks) or bool(f.clean_mask):
        raise ValueError("--clean_mask cleans a given mask: proposals are depth-connected already")
    if f.propose_no_plane:
        planar = [k_ for k_ in _PROPOSE_FLAGS if k_.startswith("plane_") and getattr(f, k_) is not None]
        if planar:
            raise ValueError("--%s sets how the support plane is fitted and dropped: not with --propose_no_plane" % planar[0])
        if f.support_check:
            raise ValueError("--support_check tests poses against the plane the proposals were cut with: not with --propose_no_plane")
    from cppf2_amd import masks
    p = dict(num_hyp=segment.NUM_HYP if f.plane_hypotheses is None else int(f.plane_hypotheses),
             tau=segment.TAU if f.plane_tau is None else float(f.plane_tau),
             min_height=segment.MIN_HEIGHT if f.plane_min_height is None else float(f.plane_min_height),
             jump=masks.JUMP if f.mask_jump is None else float(f.mask_jump),
             min_pixels=segment.MIN_SEGMENT_PIXELS if f.min_segment_pixels is None else int(f.min_segment_pixels),
             max_segments=segment.MAX_SEGMENTS if f.max_proposals is None else int(f.max_proposals))
    if not 1 <= p["num_hyp"] <= segment.MAX_HYP:
        raise ValueError("--plane_hypotheses must be in 1 .. %d, not %d" % (segment.MAX_HYP, p["num_hyp"]))
    if not (p["tau"] > 0 and np.isfinite(p["tau"])):
        raise ValueError("--plane_tau is a distance in metres > 0, not %r" % (f.plane_tau,))
    if not np.isfinite(p["min_height"]):
        raise ValueError("--plane_min_height is a distance in metres, not %r" % (f.plane_min_height,))
    if p["min_pixels"] < 0:
        raise ValueError("--min_segment_pixels must be >= 0, not %d" % p["min_pixels"])
    if not 1 <= p["max_segments"] <= segment.SEGMENTS_LIMIT:
        raise ValueError("--max_proposals must be in 1 .. %d, not %d" % (segment.SEGMENTS_LIMIT, p["max_segments"]))
    if concave is not None:                        # without the flag the dict, and with it the report, keeps its keys
        p.update(concave=concave, plane=not f.propose_no_plane)
    return p


_EXPLAIN_FLAGS = ("explain_min_score", "explain_min_gain", "explain_viol_weight", "explain_max")


def _explain_flags(f):
    """scene.explain's parameters (and min_score) from the --explain_scene flags, or None when it is off; f.obj_ids becomes a
    list of ints or None."""
    given = [k_ for k_ in _EXPLAIN_FLAGS if getattr(f, k_) is not None]
    if f.obj_ids is not None and not f.models_dir:
        raise ValueError("--obj_ids names objects of a models folder: it needs --models_dir")
    if f.explain_min_support is not None and not f.explain_hypotheses:
        raise ValueError("--explain_min_support gates the hypotheses of --explain_hypotheses: it needs that flag")
    if not f.explain_scene:
        if given:
            raise ValueError("--%s sets how the scene is explained: it needs --explain_scene" % given[0])
        if f.explain_hypotheses:
            raise ValueError("--explain_hypotheses makes every verified hypothesis a candidate of the scene: it needs --explain_scene")
        if f.models_dir:
            raise ValueError("--models_dir pools the candidates of several objects into one explanation: it needs --explain_scene")
        return None
    if f.propose is None:
        raise ValueError("--explain_scene explains an image by the verified poses of its proposals: it needs --propose_masks")
    if int(f.hypotheses) <= 1:
        raise ValueError("--explain_scene takes verified poses: it needs --hypotheses > 1")
    if f.models_dir:
        if f.mesh or f.pair_table:
            raise ValueError("--models_dir and --pair_tables stand in for --mesh and --pair_table: give the one object or the folders")
        if not f.pair_tables:
            raise ValueError("--models_dir votes from each object's table: it needs --pair_tables=<dir> (obj_%06d.npz per object)")
        if f.gt_pose is not None:
            raise ValueError("--gt_pose is the pose of the one object of --mesh: not with --models_dir")
        if f.obj_ids is not None:
            try:
                ids = f.obj_ids if isinstance(f.obj_ids, (list, tuple)) else str(f.obj_ids).split(",")
                f.obj_ids = [int(str(x_).strip()) for x_ in ids if str(x_).strip()]
            except ValueError:
                raise ValueError("--obj_ids is a comma-separated list of object ids, not %r" % (f.obj_ids,)) from None
            if not f.obj_ids or len(set(f.obj_ids)) != len(f.obj_ids):
                raise ValueError("--obj_ids names each object once, not %r" % (f.obj_ids,))
    from cppf2_amd import scene
    e = dict(min_score=0.5 if f.explain_min_score is None else float(f.explain_min_score),
             min_gain=scene.MIN_GAIN if f.explain_min_gain is None else int(f.explain_min_gain),
             viol_weight=scene.VIOL_WEIGHT if f.explain_viol_weight is None else int(f.explain_viol_weight),
             max_rounds=scene.MAX_ROUNDS if f.explain_max is None else int(f.explain_max))
    if not 0.0 <= e["min_score"] <= 1.0:
        raise ValueError("--explain_min_score is a verification score in [0, 1], not %r" % (f.explain_min_score,))
    if e["min_gain"] < 1:
        raise ValueError("--explain_min_gain must be >= 1, not %d" % e["min_gain"])
    if e["viol_weight"] < 0:
        raise ValueError("--explain_viol_weight must be >= 0, not %d" % e["viol_weight"])
    if not 1 <= e["max_rounds"] <= scene.ROUNDS_LIMIT:
        raise ValueError("--explain_max must be in 1 .. %d, not %d" % (scene.ROUNDS_LIMIT, e["max_rounds"]))
    if f.explain_hypotheses:
        if f.explain_min_score is not None:
            raise ValueError("--explain_min_score gates one pose per proposal; with --explain_hypotheses the gate is "
                             "--explain_min_support: give one of them")
        e.update(min_support=0.5 if f.explain_min_support is None else float(f.explain_min_support), hypotheses=True)
        if not 0.0 <= e["min_support"] <= 1.0:
            raise ValueError("--explain_min_support is a share of the drawn pixels in [0, 1], not %r" % (f.explain_min_support,))
    return e


_SOLID_FLAGS = (("support_check", ("support_tau", "support_max_share")), ("explain_solid", ("solid_tau", "solid_max_share")))


def _solid_flags(f):
    """The solid-interval checks' parameters (cppf2_amd/solid.py) from --support_check and --explain_solid: dict(support=dict(tau,
    max_share) or None, overlap=dict(tau, max_share) or None), or None when both are off.  Read after f.propose, f.explain and
    f.hypotheses."""
    for switch, values in _SOLID_FLAGS:
        given = [k_ for k_ in values if getattr(f, k_) is not None]
        if given and not getattr(f, switch):
            raise ValueError("--%s sets a threshold of --%s: it needs that flag" % (given[0], switch))
    if not f.support_check and not f.explain_solid:
        return None
    from cppf2_amd import solid

    def pair(tau_flag, share_flag, tau0, share0):
        tau, share = getattr(f, tau_flag), getattr(f, share_flag)
        return dict(tau=solid.checked_tau(tau0 if tau is None else tau, "eval.py", "--" + tau_flag),
                    max_share=solid.checked_share(share0 if share is None else share, "eval.py", "--" + share_flag))
    out = dict(support=None, overlap=None)
    if f.support_check:
        if f.propose is None:
            raise ValueError("--support_check tests poses against the plane the proposals were cut with: it needs --propose_masks")
        if f.hypotheses <= 1:
            raise ValueError("--support_check refuses verified hypotheses: it needs --hypotheses > 1")
        out["support"] = pair("support_tau", "support_max_share", solid.SUPPORT_TAU, solid.MAX_SUNK)
    if f.explain_solid:
        if f.explain is None:
            raise ValueError("--explain_solid constrains the scene explanation: it needs --explain_scene")
        out["overlap"] = pair("solid_tau", "solid_max_share", solid.OVERLAP_TAU, solid.MAX_OVERLAP)
    return out


def _checked_flags(**kw):
    """main()'s keyword arguments as a namespace, after every rule that ties one flag to another: the first broken rule raises
    its ValueError, before a device, a model or a file is touched.  Normalised on the way: icp_iters, hypotheses, centre_peaks
    ints; icp_depth, icp_model_weight; clean_masks true under either spelling.  f.stages: those six settings as the Stages
    record the drivers pass on, verify_tau resolved to its default here and nowhere else."""
    f = types.SimpleNamespace(**kw)
    bop_mode = f.data == "bop"
    on_mesh = f.data == "depth" and (f.mesh or f.models_dir)
    if f.pair_table or f.pair_tables:
        # a known object's pair-feature table stands where the two models stood (run_table): no prior, no checkpoints
        flag = "--pair_table" if f.pair_table else "--pair_tables"
        if f.pair_table and f.data != "depth":
            raise ValueError("--pair_table is the table of the one object of --data=depth (--data=bop: --pair_tables=<dir>); "
                             "the synthetic and NOCS modes have no table")
        if f.pair_tables and not bop_mode and not f.models_dir:
            raise ValueError("--pair_tables is a folder of obj_%06d.npz tables for --data=bop (--data=depth: --pair_table=<npz>)")
        if f.teacher_prior:
            raise ValueError("%s votes from the table: it cannot be combined with --teacher_prior" % flag)
        if f.ckpt_dir or f.ckpt_shot or f.ckpt_dino:
            raise ValueError("%s votes from the table: it cannot be combined with --ckpt_*" % flag)
    if f.data in ("depth", "bop"):
        f.icp_depth, f.icp_model_weight = _icp_depth_flag(f.icp_depth, f.icp_model_weight, f.icp_iters)
    elif f.icp_depth:
        raise ValueError("--icp_depth refines against the depth image: it needs --data=depth or --data=bop")
    f.clean_masks = bool(f.clean_masks) or bool(f.clean_mask)
    if f.mask_jump is not None and not (float(f.mask_jump) >= 0.0 and np.isfinite(float(f.mask_jump))):
        raise ValueError("--mask_jump is a distance in metres >= 0, not %r" % (f.mask_jump,))
    f.propose = _propose_flags(f)
    f.explain = _explain_flags(f)
    if bop_mode and not (f.bop_root and f.out_csv):
        raise ValueError("--data=bop needs --bop_root (the dataset folder) and --out_csv (the results file to write)")
    if not bop_mode and f.detections is not None:
        raise ValueError("--detections is a BOP detections file: it needs --data=bop")
    if not bop_mode and f.clean_masks and f.data != "depth":
        raise ValueError("--clean_masks cleans instance masks against the depth image: it needs --data=bop or --data=depth")
    if not bop_mode and f.teacher_prior:
        raise ValueError("--teacher_prior builds the prior from a BOP dataset's ground-truth poses: it needs --data=bop")
    f.icp_iters, f.hypotheses = int(f.icp_iters), int(f.hypotheses)
    if f.hypotheses < 1:
        raise ValueError("--hypotheses must be >= 1, not %d" % f.hypotheses)
    if not bop_mode and f.hypotheses > 1 and not on_mesh:
        raise ValueError("--hypotheses > 1 verifies poses against the object's mesh: it needs --data=depth and --mesh")
    f.centre_peaks = _centre_peaks_flag(f.centre_peaks, f.hypotheses)
    if bop_mode and (f.gt_pose is not None or f.mesh):
        raise ValueError("--data=bop takes the models and the true poses from the dataset: --mesh and --gt_pose belong to --data=depth")
    if not bop_mode and f.icp_iters > 0 and not on_mesh:
        raise ValueError("--icp_iters > 0 refines against the object's mesh: it needs --data=depth and --mesh")
    if not bop_mode and f.gt_pose is not None and not on_mesh:
        raise ValueError("--gt_pose scores the pose against the object's mesh (BOP metrics): it needs --data=depth and --mesh")
    f.sym_tol = _symmetry_flags(f)
    if f.iou_device and f.data != "nocs":
        raise ValueError("--iou_device scores the NOCS scorer's box overlaps on the GPU: it needs --data=nocs")
    f.solid = _solid_flags(f)
    from cppf2_amd import depthfilter
    f.condition = depthfilter.from_flags(bool(f.condition_depth), {k_: getattr(f, k_) for k_ in depthfilter.FLAGS})
    if f.condition is not None and f.data not in ("depth", "bop"):
        raise ValueError("--condition_depth conditions the depth image before anything reads it: it needs --data=depth or --data=bop")
    from cppf2_amd import verify
    f.stages = Stages(f.icp_iters, f.icp_depth, f.icp_model_weight, f.hypotheses,
                      verify.TAU if f.verify_tau is None else float(f.verify_tau), f.centre_peaks)
    return f


# what the synthetic and the depth mode collect per instance: the report's items and the arrays of the result record
Results = collections.namedtuple("Results", "summary cls RT scale gt gt_scale")


def _add_results(acc, cat, scene_ids, r, reported, up_sym, truth=None):
    """One item per instance of the voted batch r into acc, from its reported record; truth: the synthetic scenes, which carry
    their pose and box."""
    for b, rec in enumerate(reported):
        RT, sc = np.eye(4), np.ones(3)                                      # eval.py:143-144 defaults
        item = dict(scene=scene_ids[b], category=cat, model=None)
        if r["pick"][b] >= 0:                                               # eval.py:367-372
            RT[:3, :3] = rec["R"] * r["scale_norm"][b]
            RT[:3, 3] = rec["t"]
            if r["scale_norm"][b] > 0:
                sc = r["scale"][b] / r["scale_norm"][b]
            item.update(model="table" if "table_hits" in r else ["dino", "shot"][r["pick"][b]], loss=float(r["best"][b]),
                        losses=[float(r["losses"][0][b]), float(r["losses"][1][b])], pred_RT=RT.tolist(),
                        pred_scale=sc.tolist())
            if truth is not None:
                item["tr_err_cm"] = float(np.linalg.norm(rec["t"] - truth[b]["t"]) * 100)
                item["rot_err_deg"] = geometry.rot_err_deg(rec["R"], truth[b]["R"], up_sym)
        acc.summary.append(item)
        acc.cls.append(category2id.get(cat, 0)); acc.RT.append(RT); acc.scale.append(sc)
        if truth is not None:
            # synthetic instances carry their pose and box: NOCS convention, rotation scaled by the box diagonal and
            # the extents normalised by it (what eval.py:370-372 builds from the prediction)
            gt = np.eye(4)
            gt[:3, :3], gt[:3, 3] = truth[b]["R"] * truth[b]["diag"], truth[b]["t"]
            acc.gt.append(gt)
            acc.gt_scale.append(truth[b]["extent"] / truth[b]["diag"])


def _finish(report, acc, categories, debug, out, out_pkl):
    """The tail the synthetic and the depth mode share: accuracy and mAP of the scored instances into the report, the result
    record to out_pkl, the report printed and written to `out`."""
    from cppf2_amd import metrics
    summary = acc.summary
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
    if n and len(acc.gt) == n:
        gt = dict(gt_class_ids=np.array(acc.cls), gt_RTs=np.stack(acc.gt), gt_scales=np.stack(acc.gt_scale))
    record = metrics.make_result_record(np.array(acc.cls, dtype=np.int64), np.stack(acc.RT) if n else np.zeros((0, 4, 4)),
                                        np.stack(acc.scale) if n else np.zeros((0, 3)), None, **gt)
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
    return _emit(report, debug, out)


def main_synthetic(setups, categories, vote, num_scenes=8, num_points=4096, debug=False, out=None, out_pkl=None):
    """`num_scenes` seeded synthetic instances (cppf2_amd.synth) per category, voted with a teacher prior and scored against
    the poses they were made with."""
    dev = ops._dev()
    acc = Results([], [], [], [], [], [])
    for ci, cat in enumerate(categories):
        cfg = setups[cat][0]
        up_sym = cat in UP_SYM or bool(cfg.get("up_sym", False))
        scenes = [synth.make_scene(vote.seed, ci * num_scenes + s, num_points) for s in range(num_scenes)]
        # a dropped instance does not shift the others' seeds (tuple / uniform streams = scene seed)
        scene_ids = [ci * num_scenes + j for j, s in enumerate(scenes) if not too_wide(s["pc"], cfg.res)]
        scenes = [s for s in scenes if not too_wide(s["pc"], cfg.res)]                     # eval.py:200
        if not scenes:
            continue
        g = torch.Generator(device="cpu").manual_seed(vote.seed + 1 + ci)                  # one stream, drawn scene after scene
        descs = [stand_in_descriptors(s["pc"].shape[0], g).numpy() for s in scenes]
        priors = _teacher_prior(np.concatenate([s["pc_canon"] for s in scenes]), dev)
        r, _ = vote_batch(setups[cat], [s["pc"] for s in scenes], descs, scene_ids, vote, up_sym, priors,
                          np.stack([s["extent"] for s in scenes]))
        _add_results(acc, cat, scene_ids, r, [r["records"][r["pick"][b]][b] for b in range(len(scenes))], up_sym, scenes)
    report = dict(categories=categories, instances=len(acc.summary), opt_refinement=_opt_note(vote), results=acc.summary)
    return _finish(report, acc, categories, debug, out, out_pkl)


def _score_against_gt(item, gt, d, K, r, b, reported, ver, icp_stats):
    """The BOP errors of instance b's reported pose (of its first hypothesis; of its pose before ICP) against --gt_pose, gt =
    (the object's bop.ObjectInfo, R, t), on the depth image d and K, into item[`bop`] ([`bop_first`], [`bop_before_icp`]); an
    instance without an estimate scores +inf.  Returns the reported pose's errors, for the run's average recall."""
    from cppf2_amd import bop
    bop_obj, gt_R, gt_t = gt
    poses = [reported[b]] + ([ver["hypotheses"][b, 0]] if ver is not None else [])
    poses += [r["records"][r["pick"][b]][b]] if icp_stats is not None else []
    nan = (np.full((3, 3), np.nan), np.full(3, np.nan))
    poses = [(p_["R"], p_["t"]) if r["pick"][b] >= 0 else nan for p_ in poses]
    err = bop.pose_errors(bop_obj, d, np.zeros(len(poses), dtype=np.int64), [p_[0] for p_ in poses],
                          [p_[1] for p_ in poses], [gt_R] * len(poses), [gt_t] * len(poses), K)
    keys = ["bop"] + (["bop_first"] if ver is not None else []) + (["bop_before_icp"] if icp_stats is not None else [])
    for j, k_ in enumerate(keys):
        item[k_] = dict(vsd=[float(x) for x in err["vsd"][j]], mssd=float(err["mssd"][j]), mspd=float(err["mspd"][j]))
    return {k_: v_[:1] for k_, v_ in err.items()}


def _scene_objects(models_dir, pair_tables, obj_ids, model_scale, stages):
    """The objects of the multi-object form, read through bop_data.Models as a BOP dataset's are: obj_%06d.ply of models_dir
    (all of them without obj_ids) with their models_info.json entries, and obj_%06d.npz of pair_tables.  A list of dicts (obj_id,
    obj: bop.ObjectInfo, icp_model, pair_table: the file's path; a missing table is an error when it is loaded)."""
    from cppf2_amd import bop_data, icp
    models = bop_data.Models(models_dir, model_scale)
    if obj_ids is None:
        obj_ids = models.ids()
        if not obj_ids:
            raise FileNotFoundError("--models_dir=%s holds no obj_%%06d.ply" % models_dir)
    return [dict(obj_id=int(o), obj=models.object(o), icp_model=icp.ModelPoints.from_mesh(models.mesh(o)) if stages.icp_iters > 0 else None,
                 pair_table=os.path.join(str(pair_tables), "obj_%06d.npz" % int(o))) for o in obj_ids]


def _hypothesis_candidates(ver, b, tag):
    """--explain_hypotheses: every hypothesis of instance b that refine_and_verify's `ver` holds and that is not an empty slot,
    as a candidate of _explain_scene: the pose after ICP, its per-mask score, and its support fit / drawn in float64 (the share
    of what the pose shows the camera that the depth confirms inside the mask; 0 where nothing is drawn)."""
    from cppf2_amd import verify
    out = []
    for h, rec in enumerate(ver["hypotheses"][b]):
        if rec["flags"] & verify.EMPTY:
            continue
        drawn, fit = int(ver["counts"][b, h, 0]), int(ver["counts"][b, h, verify.N_COUNTS])
        out.append(dict(tag, hypothesis=h, score=float(ver["scores"][b, h]), record=rec.copy(),
                        support=float(np.float64(fit) / np.float64(drawn)) if drawn else 0.0))
    return out


def _explain_scene(cands, objs, d, region, K, tau, explain, solid=None):
    """The report's `scene` entry: the candidates (dicts with proposal, category, score, record, obj: index into objs, and
    obj_id in the multi-object form) with a score of at least min_score, the 64 best of them when there are more (ties to the
    lower index), explained over `region` by scene.explain_candidates.  With explain["hypotheses"] (--explain_hypotheses) the
    candidates are hypotheses (they also carry hypothesis and support), the gate is a support of at least min_support, and the
    512 best supported go through the wide form.  solid: explain_candidates' keyword arguments of the support and overlap checks
     or nothing: with them a candidate may be rejected as below_table, or as inside the instance whose
    index `inside_of` gives, every entry of a run with a plane carries its support_counts, and the entry gains `passes`."""
    from cppf2_amd import scene
    from cppf2_amd.pipeline import RESULT_DTYPE
    wide = bool(explain.get("hypotheses"))
    gate, floor, limit = ("support", explain["min_support"], scene.MAX_CANDIDATES_WIDE) if wide else \
        ("score", explain["min_score"], scene.MAX_CANDIDATES)

    def entry(c_, **more):
        e = {k_: c_[k_] for k_ in ("proposal", "category", "obj_id", "hypothesis") if k_ in c_}
        e.update(score=c_["score"], **more)
        if wide:
            e["support"] = c_["support"]
        return e
    rejected = [entry(c_, reason="below_min_" + gate) for c_ in cands if not c_[gate] >= floor]
    kept = [c_ for c_ in cands if c_[gate] >= floor]
    order = sorted(range(len(kept)), key=lambda j: (-kept[j][gate], j))[:limit]
    dropped = len(kept) - len(order)
    kept = [kept[j] for j in sorted(order)]
    recs = np.array([c_["record"] for c_ in kept], dtype=RESULT_DTYPE).reshape(-1)
    ex = scene.explain_candidates(objs, d.astype(np.float32), region, K, recs, [c_["obj"] for c_ in kept], tau=tau,
                                  min_gain=explain["min_gain"], viol_weight=explain["viol_weight"], max_rounds=explain["max_rounds"],
                                  wide=wide, **(solid or {}))

    def counts(j):
        return dict(support_counts=[int(x_) for x_ in ex["support"][j]]) if "support" in ex else {}
    instances = []
    for j, g, n in zip(ex["chosen"], ex["gain"], ex["net"]):
        rec = kept[int(j)]["record"]
        instances.append(entry(kept[int(j)], R=np.asarray(rec["R"], dtype=np.float64).reshape(3, 3).tolist(),
                               t=np.asarray(rec["t"], dtype=np.float64).tolist(), gain=int(g), net=int(n), **counts(int(j))))
    taken = {int(j) for j in ex["chosen"]}
    sunk = {int(j) for j in ex["refused_support"]}
    inside = {int(j): [int(x_) for x_ in ex["chosen"]].index(int(w_)) for j, w_ in ex["refused_overlap"]}
    for j, c_ in enumerate(kept):
        if j in sunk:
            rejected.append(entry(c_, reason="below_table", **counts(j)))
        elif j in inside:
            rejected.append(entry(c_, reason="inside", inside_of=inside[j], **counts(j)))
        elif j not in taken:
            rejected.append(entry(c_, reason="no_gain", **counts(j)))
    out = dict(instances=instances, explained_pixels=ex["explained_pixels"], region_pixels=ex["region_pixels"], rejected=rejected,
               dropped=dropped, candidates=len(kept),
               parameters=dict(explain, tau=float(tau)))
    if solid:
        out["passes"] = ex["passes"]
    return out


# what the instance loop of one depth image reads besides its masks and objects: the depth in metres and K, the categories'
# setups, the Vote and Stages settings, what the ICP refined against (the report's words), and where the report goes
DepthRun = collections.namedtuple("DepthRun", "d K setups vote stages against debug out out_pkl conditioned", defaults=(None,))


def _depth_instances(ctx, masks, objects, categories, proposed=None, gt=None, explain=None, cleaning=None, pair_tables=None,
                     solid=None, symmetries=None):
    """The depth mode over the masks (bool [M,H,W]) of the image of ctx, a DepthRun: per object and category one batch whose
    instances are the masks that give a usable cloud, each with the cloud, scene index and tuple streams a --mask run of its mask
    has; voted, refined and verified as ctx.stages says, then reported (_finish).
    objects: dicts of obj (bop.ObjectInfo or None), icp_model and pair_table (a path or None), one per run over the masks; those
    of the multi-object form (_scene_objects) also hold obj_id, which every item then carries, and pair_tables names their folder.
    proposed: None for the one given mask, the reference's route: no guard on too few points (eval.py:185-197), a too-wide cloud
    dropped silently (eval.py:200), `cleaning` as the report's mask_cleaning.  Else (props, plane, propose), what segment.propose
    returned and its keyword arguments: unusable clouds are counted, items carry their proposal, and the report gains plane,
    proposals, proposed, skipped, mask_proposals and best.
    gt: (the object's bop.ObjectInfo, R, t) of --gt_pose or None: every instance of the given mask is scored; of proposals the best
    one when the verification chose one, else every one.  explain: _explain_flags' dict: the verified poses become the candidates
    of _explain_scene.  solid: _solid_flags' dict or None; its `support` entry makes verify.select and the explanation refuse
    poses that sink into the proposals' plane, its `overlap` entry makes the explanation refuse a pose inside an earlier instance.
    symmetries: symmetry.summary of --detect_symmetries' entry or None: the report's `symmetries`."""
    from cppf2_amd import bop
    dev = ops._dev()
    d, K, vote, stages = ctx.d, ctx.K, ctx.vote, ctx.stages
    props, plane, propose = proposed or (None, None, None)
    support = None
    if solid is not None and solid["support"] is not None:
        support = dict(plane=np.array(list(plane["n"]) + [plane["d"]], dtype=np.float32), support_tau=solid["support"]["tau"],
                       max_sunk=solid["support"]["max_share"])
    multi = "obj_id" in objects[0]
    acc = Results([], [], [], [], [], [])
    skipped = dict(too_large=0, too_few_points=0)
    proposals, best, bop_reported, cands = [], None, [], []
    for oi, ob in enumerate(objects):
        tag = dict(obj_id=ob["obj_id"]) if multi else {}
        for ci, cat in enumerate(categories):       # an instance is scene `ci` of the run: its tuple / uniform streams' seed
            cfg = ctx.setups[cat][0]
            up_sym = cat in UP_SYM or bool(cfg.get("up_sym", False))
            ranks, pcs = [], []
            for p_, m in enumerate(masks):
                pc, why = usable_cloud(d, K, m, cfg, vote.seed, min_points=props is not None)
                if pc is None:
                    skipped[why] += 1
                else:
                    ranks.append(p_)
                    pcs.append(pc)
            B = len(pcs)
            if not B:
                continue
            # (a table pass reads no descriptor)
            descs = [] if ob["pair_table"] else [stand_in_descriptors(pc.shape[0], vote.seed + 1 + ci).numpy() for pc in pcs]
            r, enabled = vote_batch(ctx.setups[cat], pcs, descs, [ci] * B, vote, up_sym, stages=stages,
                                    table=load_pair_table(ob["pair_table"], dev) if ob["pair_table"] else None)
            reported, icp_stats, ver = refine_and_verify(r, enabled, ob["obj"], d, masks[ranks], K,
                                                         np.cumsum([0] + [pc.shape[0] for pc in pcs]), ob["icp_model"], stages,
                                                         **(dict(support=support) if support else {}))
            _add_results(acc, cat, [ci] * B, r, reported, up_sym)
            items = acc.summary[-B:]
            top = None
            for b, item in enumerate(items):
                item.update(instance_items(r, b, icp_stats, ver, stages))
                if props is None:
                    continue
                prop = props[ranks[b]]
                item.update(proposal=ranks[b], pixels=prop["pixels"], bbox=prop["bbox"], points=int(pcs[b].shape[0]), **tag)
                entry = dict(proposal=ranks[b], category=cat, pixels=item["pixels"], bbox=item["bbox"], R=None, t=None, **tag)
                if r["pick"][b] >= 0:
                    entry.update(R=np.asarray(reported[b]["R"], dtype=np.float64).reshape(3, 3).tolist(),
                                 t=np.asarray(reported[b]["t"], dtype=np.float64).tolist())
                    if ver is not None:
                        entry["score"] = item["verify"]["score"]
                        if top is None or entry["score"] > items[top]["verify"]["score"]:      # ties: the lower rank stays
                            top = b
                        if explain is None or not explain.get("hypotheses"):
                            cands.append(dict(proposal=ranks[b], category=cat, score=entry["score"], record=reported[b].copy(),
                                              obj=oi, **tag))
                        else:
                            cands += _hypothesis_candidates(ver, b, dict(proposal=ranks[b], category=cat, obj=oi, **tag))
                proposals.append(entry)
            if top is not None and (best is None or items[top]["verify"]["score"] > best["score"]):
                best = dict(proposal=ranks[top], category=cat, score=items[top]["verify"]["score"], **tag)
            if gt is not None:
                scored = range(B) if props is None or ver is None else [b for b in (top,) if b is not None]
                bop_reported += [_score_against_gt(items[b], gt, d, K, r, b, reported, ver, icp_stats) for b in scored]
    report = dict(categories=categories, instances=len(acc.summary), opt_refinement=_opt_note(vote), results=acc.summary)
    if props is not None:
        report.update(plane=dict(n=plane["n"], d=plane["d"], inliers=plane["inliers"], usable_hypotheses=plane["usable_hypotheses"],
                                 valid_pixels=plane["valid_pixels"]),
                      proposals=proposals, proposed=len(props), skipped=skipped,
                      mask_proposals=dict(propose, seed=int(vote.seed), components=plane["components"],
                                          large_components=plane["large_components"]))
        if "concave" in plane:                         # --propose_concave: the settings and the valid, edge and kept pixels
            report["concave"] = plane["concave"]
            report["mask_proposals"]["concave"] = dict(propose["concave"]._asdict())
        if best is not None:
            report["best"] = best
    if multi:
        report.update(obj_ids=[ob["obj_id"] for ob in objects], pair_tables=str(pair_tables),
                      table_hits=[s_["table_hits"] for s_ in acc.summary])
    elif objects[0]["pair_table"]:
        report.update(pair_table=str(objects[0]["pair_table"]), table_hits=[s_["table_hits"] for s_ in acc.summary])
    report.update(stage_notes(ctx.against, stages, cleaning))
    if stages.icp_iters > 0:
        report["icp"] = [s_["icp"] for s_ in acc.summary if "icp" in s_]
    if bop_reported:
        errs = {k_: np.concatenate([e_[k_] for e_ in bop_reported]) for k_ in ("vsd", "mssd", "mspd")}
        report["bop"] = dict(bop.average_recall(errs, gt[0].diameter, d.shape[1]), delta=bop.DELTA, taus=list(bop.TAUS))
    if explain is not None:
        more = dict(support or {})
        if solid is not None and solid["overlap"] is not None:
            more.update(solid=True, solid_tau=solid["overlap"]["tau"], max_overlap=solid["overlap"]["max_share"])
        report["scene"] = _explain_scene(cands, [ob["obj"] for ob in objects], d, masks.any(0), K, stages.verify_tau, explain, more)
    if solid is not None:
        report["solid_checks"] = solid
    if symmetries is not None:
        report["symmetries"] = symmetries
    if ctx.conditioned is not None:
        report["depth_condition"] = ctx.conditioned
    return _finish(report, acc, categories, ctx.debug, ctx.out, ctx.out_pkl)


def main_depth(setups, categories, vote, stages, depth, mask=None, intrinsics=None, depth_scale=1000.0, mesh=None, mesh_scale=1.0,
               gt_pose=None, models_info=None, clean_mask=False, mask_jump=None, pair_table=None, debug=False, out=None, out_pkl=None,
               propose=None, explain=None, models_dir=None, pair_tables=None, obj_ids=None, model_scale=0.001, solid=None,
               sym_tol=None, condition=None):
    """One depth + mask PNG pair (example_data layout): one instance, evaluated once per category of `categories`; with `mesh`
    its pose is refined (stages.icp_iters), verified (stages.hypotheses) and scored against gt_pose (BOP errors), see the module
    docstring.  propose: segment.propose's keyword arguments; the proposed masks then stand where the one of `mask` stood, one
    instance each in one batch per category.  explain: _explain_flags' dict (the report's `scene`); models_dir, pair_tables,
    obj_ids, model_scale: the objects of the multi-object form, which stand where mesh and pair_table stood.  solid:
    _solid_flags' dict (the support and overlap checks of cppf2_amd/solid.py).  sym_tol: --detect_symmetries' tolerance or None;
    the detected entry then stands where the one of models_info stood.  condition: a depthfilter.Settings record or None; the
    depth image is then conditioned once, right after it is read and scaled, and every later step reads the conditioned image
    (the report's `depth_condition`).  This reads the inputs; _depth_instances runs them."""
    from PIL import Image
    from cppf2_amd import bop, icp, masks, render, segment
    gt = symmetries = None
    if models_dir:
        objects, against = _scene_objects(models_dir, pair_tables, obj_ids, model_scale, stages), "each object's model"
    else:
        icp_model = icp.ModelPoints.from_mesh(render.load_mesh(mesh, mesh_scale)) if stages.icp_iters > 0 else None
        obj = info = None
        if sym_tol is not None:
            from cppf2_amd import symmetry
            info = symmetry.detect(render.load_mesh(mesh, mesh_scale), tol=sym_tol)
            symmetries = symmetry.summary(info)
        if gt_pose is not None:
            if models_info:
                with open(models_info) as f:
                    info = json.load(f)
            obj = bop.ObjectInfo.from_mesh(render.load_mesh(mesh, mesh_scale), models_info=info, mesh_scale=mesh_scale)
            gt = (obj,) + tuple(bop.load_pose(gt_pose))
        elif stages.hypotheses > 1:
            obj = bop.ObjectInfo.from_mesh(render.load_mesh(mesh, mesh_scale))
        objects, against = [dict(obj=obj, icp_model=icp_model, pair_table=pair_table)], os.path.basename(mesh or "")
    d = np.array(Image.open(depth)).astype(np.float64) / float(depth_scale)
    conditioned = None
    if condition is not None:
        from cppf2_amd import depthfilter
        dc, conditioned = depthfilter.apply(d.astype(np.float32), condition, "eval.py")
        d = dc[0].cpu().numpy().astype(np.float64)
    K = np.array(intrinsics if intrinsics is not None else REAL_INTRINSICS, dtype=np.float64).reshape(3, 3)
    ctx = DepthRun(d, K, setups, vote, stages, against, debug, out, out_pkl, conditioned)
    if propose is not None:
        pm, props, plane = segment.propose(d.astype(np.float32), K, vote.seed, **propose)
        return _depth_instances(ctx, pm.cpu().numpy() > 0, objects, categories, (props, plane, propose), gt, explain,
                                pair_tables=pair_tables, solid=solid, symmetries=symmetries)
    m = np.array(Image.open(mask))
    m = (m[..., 0] if m.ndim == 3 else m) > 0
    cleaning = None
    if clean_mask:
        # the largest depth-connected component of the mask (cppf_mask_components): what is back-projected and verified
        kept, stats = masks.clean(m[None], d.astype(np.float32), 0, masks.JUMP if mask_jump is None else float(mask_jump))
        m = kept[0].cpu().numpy() > 0
        stats = [int(x) for x in stats[0].cpu().numpy()]
        cleaning = dict(components=stats[0], kept_pixels=stats[2], valid_pixels=stats[3])
        if not m.any():
            raise ValueError("--clean_mask: no depth-connected component of the mask has %d pixels" % masks.MIN_PIXELS)
    return _depth_instances(ctx, m[None], objects, categories, gt=gt, cleaning=cleaning, symmetries=symmetries)


def main(angle_tol=1., imp_wt_margin=0.01, backproj_ratio=.1, num_pairs=50000, num_rots=180, opt=True, debug=False,
         use_grounded_sam=False, geo_branch=True, visual_branch=True, data="synthetic", num_scenes=8, num_points=4096,
         category=None, categories=None, seed=0, ckpt_dir=None, ckpt_shot=None, ckpt_dino=None, depth=None, mask=None,
         intrinsics=None, depth_scale=1000.0, out=None, out_pkl=None, log_dir=None, data_root="NOCS/real_test", out_dir=None,
         desc_npz=None, batch_instances=16, max_images=None, mesh=None, mesh_scale=1.0, icp_iters=0, gt_pose=None,
         models_info=None, hypotheses=1, verify_tau=None, bop_root=None, split="test", targets=None, out_csv=None,
         teacher_prior=False, model_scale=0.001, centre_peaks=1, detections=None, det_score_min=0.0, clean_masks=False,
         clean_mask=False, mask_jump=None, icp_depth=False, icp_model_weight=1.0, pair_table=None, pair_tables=None,
         propose_masks=False, plane_tau=None, plane_hypotheses=None, plane_min_height=None, min_segment_pixels=None,
         max_proposals=None, explain_scene=False, explain_min_score=None, explain_min_gain=None, explain_viol_weight=None,
         explain_max=None, models_dir=None, obj_ids=None, explain_hypotheses=False, explain_min_support=None,
         support_check=False, support_tau=None, support_max_share=None, explain_solid=False, solid_tau=None, solid_max_share=None,
         detect_symmetries=False, sym_tol=None, iou_device=False, condition_depth=False, flying_radius=None, flying_support=None,
         smooth_radius=None, depth_jump=None, depth_jump_rel=None, propose_concave=False, concave_step=None, concave_angle=None,
         concave_floor=None, concave_reach=None, propose_no_plane=False):
    f = _checked_flags(**locals())
    vote = Vote(*(getattr(f, k_) for k_ in Vote._fields))
    dev = ops._dev()
    torch.manual_seed(seed)
    if data == "bop":                               # its models come from the dataset
        return main_bop(load_custom(ckpt_shot, ckpt_dino, device=dev, models=not pair_tables), vote, f.stages, bop_root, split, out_csv,
                        targets=targets, mesh_scale=float(model_scale), batch_instances=batch_instances,
                        teacher_prior=bool(teacher_prior), debug=debug, out=out, detections=detections,
                        det_score_min=float(det_score_min), clean_masks=f.clean_masks, mask_jump=mask_jump, pair_tables=pair_tables,
                        condition=f.condition)
    custom = False
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
    # eval.py:84-101: models and cfgs of every category up front
    if custom:
        setups = {"custom": load_custom(ckpt_shot, ckpt_dino, device=dev, models=not (pair_table or models_dir))}
    else:
        setups = {c: load_category(c, ckpt_dir, ckpt_shot, ckpt_dino, device=dev) for c in categories}
    if data == "nocs":
        assert log_dir, "--data=nocs needs --log_dir (the directory of results_*.pkl, eval.py:72-76)"
        return main_nocs(setups, vote, log_dir, data_root=data_root, out_dir=out_dir, desc_npz=desc_npz,
                         batch_instances=batch_instances, intrinsics=intrinsics, max_images=max_images, debug=debug, out=out,
                         iou_device=bool(iou_device))
    if data == "depth":
        return main_depth(setups, categories, vote, f.stages, depth, mask, intrinsics=intrinsics, depth_scale=depth_scale, mesh=mesh,
                          mesh_scale=mesh_scale, gt_pose=gt_pose, models_info=models_info, clean_mask=f.clean_masks,
                          mask_jump=mask_jump, pair_table=pair_table, debug=debug, out=out, out_pkl=out_pkl, propose=f.propose,
                          explain=f.explain, models_dir=models_dir, pair_tables=pair_tables, obj_ids=f.obj_ids,
                          model_scale=float(model_scale), solid=f.solid, sym_tol=f.sym_tol, condition=f.condition)
    return main_synthetic(setups, categories, vote, num_scenes=num_scenes, num_points=num_points, debug=debug, out=out,
                          out_pkl=out_pkl)


if __name__ == "__main__":
    kwargs = {}
    for a in sys.argv[1:]:
        if a.startswith("--") and "=" in a:
            k_, v_ = a[2:].split("=", 1)
            kwargs[k_] = _flag(v_)
        elif a.startswith("--"):
            kwargs[a[2:]] = True
    main(**kwargs)
