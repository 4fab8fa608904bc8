"""The post-vote kernels at the reference's default size (eval.py: num_pairs=50000, num_rots=180; ~5 000 kept pairs), where
their long-list paths run, against the oracle or an exact host computation.

* cppf_assemble_pose: the scale head's lower median over the kept pairs is selected from LDS for kept <= ASM_STAGE (4096) and
  straight from global memory above it -- both sides, bit for bit;
* cppf_refine_pose: the first 4096 loss elements (2 per kept pair) sit in registers, the rest are re-read on every Adam step --
  both sides, and the early return of scenes without kept pairs or without a grid;
* the post-MLP path at 50 000 x 180 on a ragged batch (one scene with exactly 4096 kept pairs), the bench's whole Step at
  50 000 tuples, and the reference's example cloud through eval.run_ensemble at the reference's defaults.
Needs an MI355X: run with `pytest -m gpu`.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

from oracle import cppf_oracle as O            # noqa: E402  (checker only)
from oracle import pipeline_oracle as PO       # noqa: E402  (checker only)
from cppf2_amd import _lib, ops                # noqa: E402
from cppf2_amd.pipeline import RESULT_DTYPE, VotingPipeline   # noqa: E402
from test_refine import RF_CACHED_PAIRS, _kept_problem   # noqa: E402

ASM_STAGE = 4096            # cppf_backvote.hip: kept pairs whose scale-head rows are staged in LDS for the median
UP, RIGHT, FRONT = [0, 1, 0], [1, 0, 0], [0, 0, 1]
DEV = torch.device("cuda")


def _d(x, dtype):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV, dtype)


def _total_order_key(x):
    """float32 -> uint32 in IEEE totalOrder (-0.0 below +0.0): the order the kernel's radix select ranks keys in."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _rotation_counts_with_device_tanf(pc, idx, want, trig):
    """The oracle's up / right sphere counts (eval.py:277-293) recomputed with tan of its angles evaluated by the device's tanf
    (torch.tan on the GPU) instead of NumPy's: the kernels' only libm call in this stage.  At ~5 000 kept pairs x 180 rotations
    two float32 tans an ulp apart flip cone tests in more bins than the 20 000-tuple tests' <= 4 (NumPy's float32 tan against
    the correctly rounded one already does, up to 7); with the device's tanf on both sides that bar holds again."""
    mask = want["pairs_mask"]
    filt = np.asarray(idx)[mask]
    sph = O.sphere_bins(1.0)
    out = {}
    for col, name in ((0, "up"), (2, "right")):
        ang = want["targets_rot"][mask][:, col]
        tn = torch.tan(_d(ang, torch.float32)).cpu().numpy()
        cand, vm = O.vote_rotation(pc, ang, filt[:, :2], len(trig[0]), trig, tan=tn)
        wt = np.broadcast_to(want["imp_pair_wt"][vm, None], (int(vm.sum()), len(trig[0]))).reshape(-1, 1)
        out[name] = O.get_topk_dir(cand.reshape(-1, 3), sph, 100000, 1.0, wt, topk=1, return_counts=True, impl="c")[2]
    return out


def _check_rotation_counts(got_counts, pc, idx, want, trig):
    """got_counts [2, S] (up, right) against the oracle: per bin within 2 votes of the largest weight of the NumPy-tan oracle,
    and within the tanf-flip bound of test_gpu_parity (<= 4 bins off by <= 2 votes) of the oracle run on the device's tanf."""
    bound = 2.0 / want["imp_pair_wt"].min()
    same_tan = _rotation_counts_with_device_tanf(pc, idx, want, trig)
    for a, name in ((0, "up"), (1, "right")):
        assert np.abs(got_counts[a] - want[name + "_counts"]).max() <= bound
        d = np.abs(got_counts[a] - same_tan[name])
        assert (d > 0).sum() <= 4 and d.max() <= bound, (name, int((d > 0).sum()), float(d.max()))


# ------------------------------------------------------------------------------------------ scale median
def _scale_columns(rng, T):
    """[T, 3] float32: mixed signs; heavy exact ties; +-0.0 and subnormals of both signs around the middle."""
    x = np.empty((T, 3), np.float32)
    x[:, 0] = rng.randn(T) * 0.3 - 0.05
    x[:, 1] = rng.randint(-3, 4, T).astype(np.float32) * np.float32(0.25)
    kind = rng.choice(6, T, p=rng.dirichlet(np.ones(6) * 4))
    sub = (rng.randint(1, 1 << 23, T).astype(np.uint32)).view(np.float32)          # subnormal magnitudes
    c = np.where(kind == 0, -np.abs(rng.randn(T)).astype(np.float32),
        np.where(kind == 1, -sub,
        np.where(kind == 2, np.float32(-0.0),
        np.where(kind == 3, np.float32(0.0),
        np.where(kind == 4, sub, np.abs(rng.randn(T)).astype(np.float32))))))
    x[:, 2] = c
    return x


def test_scale_median_kernel_on_both_sides_of_the_lds_stage():
    """cppf_assemble_pose's lower median (torch.median, eval.py:309) per column over a ragged batch whose kept lists are random
    permutations of random subsets of each scene's tuples: 1, 2, 4095, 4096 (staged in LDS), 4097, 5000, 50 000 = T (selected
    from global memory) kept pairs, and a scene with none (NaN).  Bit equality per column."""
    L = _lib.load()
    rng = np.random.RandomState(21)
    kept_counts = [1, 2, 4095, ASM_STAGE, ASM_STAGE + 1, 5000, 50000, 0]
    Ts = [3, 2, 4100, 9000, 4097, 12345, 50000, 100]             # (kept == T for 2, 4097 and 50 000)
    B = len(Ts)
    tup_off = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int32)
    kept_tuple = np.zeros(tup_off[-1], np.int32)                 # past a scene's count: valid rows the kernel must not read
    scales = np.concatenate([_scale_columns(rng, T) for T in Ts])   # mixes differ per scene
    for b, (T, k) in enumerate(zip(Ts, kept_counts)):
        kept_tuple[tup_off[b]:tup_off[b] + k] = rng.permutation(T)[:k]
    S = 4
    sphere = np.eye(S, 3, dtype=np.float32)
    res = torch.zeros((B, 160), dtype=torch.uint8, device=DEV)
    zi, zf = torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.float32, device=DEV)
    ri = torch.ones(B, dtype=torch.int32, device=DEV)
    argmax = torch.zeros(B, dtype=torch.int64, device=DEV)
    world = torch.zeros((B, 3), dtype=torch.float64, device=DEV)
    args = [_d(sphere, torch.float32), zi, zf, ri, zf, 1, 0, argmax, None, world, None, _d(scales, torch.float32),
            _d(tup_off, torch.int32), _d(kept_tuple, torch.int32), _d(kept_counts, torch.int32), res]
    _lib.check(L.cppf_assemble_pose(B, *[a if isinstance(a, int) else ops._p(a) for a in args], ops._stream()),
               "cppf_assemble_pose")
    rec = np.frombuffer(res.cpu().numpy().tobytes(), dtype=RESULT_DTYPE)
    assert {ASM_STAGE, ASM_STAGE + 1} <= set(kept_counts) and max(kept_counts) > ASM_STAGE
    for b, (T, k) in enumerate(zip(Ts, kept_counts)):
        got = rec["scale"][b]
        assert rec["kept"][b] == k
        if k == 0:
            assert np.all(np.isnan(got))
            continue
        x = scales[tup_off[b] + kept_tuple[tup_off[b]:tup_off[b] + k]]
        want = np.sort(x, axis=0)[(k - 1) // 2]
        # np.sort ranks -0.0 and +0.0 as equal; the kernel ranks -0.0 first (totalOrder): the bits come from that order
        want_bits = np.array([np.sort(_total_order_key(x[:, c]))[(k - 1) // 2] for c in range(3)], np.uint32)
        want_bits = np.where(want_bits & np.uint32(0x80000000), want_bits & np.uint32(0x7fffffff), ~want_bits)
        assert np.array_equal(got.view(np.uint32), want_bits), (b, k, got, want)
        assert np.array_equal(got, want)                         # (the columns without -0.0 are bit-equal to np.sort's too)
    # the +-0 / subnormal column really puts its median among them in some scenes
    assert any(rec["scale"][b][2] == 0 or abs(rec["scale"][b][2]) < np.finfo(np.float32).tiny
               for b in range(B) if kept_counts[b] > 4000)


# ------------------------------------------------------------------------------------------ refinement, kernel level
def _refine_batch(kept_counts, y_only, steps=100, lr=1e-2):
    """One cppf_refine_pose launch over test_refine._kept_problem scenes of the given kept counts, plus a scene with
    kept_count == 0 and one whose record has flags & 1.  Each scene's tuple rows are in random order; the kept list names the
    kept pairs in problem order, so its positions past RF_CACHED_PAIRS are the pairs with shifted targets.  Returns (records before, records after, per scene (pc, idx2, tgt) of the kept pairs in list
    order)."""
    import ctypes
    L = _lib.load()
    rng = np.random.RandomState(7)
    probs = []
    for k in kept_counts:
        pc, idx, tgt, R0, t0 = _kept_problem(k)
        perm = rng.permutation(len(idx))                         # pair j sits in tuple row perm[j]
        idx_rows, tgt_rows = np.empty_like(idx), np.empty_like(tgt)
        idx_rows[perm], tgt_rows[perm] = idx, tgt
        probs.append(dict(pc=pc, idx=idx_rows, tgt=tgt_rows, kept=perm[:k], pose=(R0, t0)))
    probs.append(dict(probs[0], kept=probs[0]["kept"][:0]))     # nothing kept
    probs.append(dict(probs[1]))                                  # flags & 1 (set below)
    B = len(probs)
    counts = [len(p["kept"]) for p in probs]
    pt_off = np.concatenate([[0], np.cumsum([p["pc"].shape[0] for p in probs])])
    tup_off = np.concatenate([[0], np.cumsum([p["idx"].shape[0] for p in probs])])
    kept_tuple = np.zeros(tup_off[-1], np.int32)
    for b, p in enumerate(probs):
        kept_tuple[tup_off[b]:tup_off[b] + counts[b]] = p["kept"]
    before = np.zeros(B, RESULT_DTYPE)
    for b, p in enumerate(probs):
        before["R"][b], before["t"][b] = p["pose"]
        before["kept"][b], before["argmax"][b], before["scale"][b] = counts[b], 1000 + b, (0.1, 0.2, 0.3)
    before["flags"][B - 1] = 1
    recs = _d(before.view(np.uint8).reshape(B, 160), torch.uint8)
    bufs = [_d(np.concatenate([p["pc"] for p in probs]), torch.float32), _d(pt_off, torch.int32),
            _d(np.concatenate([p["idx"] for p in probs]), torch.int32), _d(tup_off, torch.int32),
            _d(np.concatenate([p["tgt"] for p in probs]), torch.float32), _d(kept_tuple, torch.int32), _d(counts, torch.int32)]
    pts, pt_off_d, idx_d, tup_off_d, scaled, kept_d, count_d = bufs
    _lib.check(L.cppf_refine_pose(B, ops._p(pts), ops._p(pt_off_d), ops._p(idx_d), 2, ops._p(tup_off_d), ops._p(scaled),
                                  ops._p(kept_d), ops._p(count_d), int(bool(y_only)), int(steps), ctypes.c_float(lr),
                                  ops._p(recs), ops._stream()), "cppf_refine_pose")
    after = np.frombuffer(recs.cpu().numpy().tobytes(), dtype=RESULT_DTYPE)
    kept_pairs = [(p["pc"], p["idx"][p["kept"]], p["tgt"][p["kept"]]) for p in probs]
    return before, after, kept_pairs


def _check_refined(before, after, kept_pairs, n_refined, y_only, steps=100, lr=1e-2):
    for b in range(n_refined):
        pc, idx2, tgt = kept_pairs[b]
        want_t, want_R = O.refine_pose(pc, idx2, tgt, before["t"][b], before["R"][b], y_only, steps=steps, lr=lr)
        assert after["flags"][b] & 8, b
        # the oracle's bars (test_refine.test_hip_refinement_matches_the_oracle): 0.2 mm, 2e-3
        assert np.abs(after["t"][b] - want_t).max() < 2e-4, (b, len(idx2), after["t"][b], want_t)
        assert np.abs(after["R"][b] - want_R).max() < 2e-3, (b, len(idx2))
        assert np.abs(after["t"][b] - before["t"][b]).max() > 1e-5
    # kept_count == 0, and flags & 1 (no grid): the records come back byte for byte, bit 3 clear
    for b in (n_refined, n_refined + 1):
        assert after[b].tobytes() == before[b].tobytes() and not after["flags"][b] & 8


@pytest.mark.parametrize("y_only", [False, True])
def test_refine_kernel_on_both_sides_of_the_register_cache(y_only):
    """cppf_refine_pose directly, kept counts 2047 / 2048 / 2049 (4094 / 4096 / 4098 loss elements: all in registers, exactly
    filled, one pair re-read), 5 000 and 20 000, against O.refine_pose on the same kept pairs in the same order."""
    kept_counts = [RF_CACHED_PAIRS - 1, RF_CACHED_PAIRS, RF_CACHED_PAIRS + 1, 5000, 20000]
    elems = 2 * np.array(kept_counts)
    assert (elems < 4096).any() and (elems == 4096).any() and (elems > 4096).any()
    before, after, kept_pairs = _refine_batch(kept_counts, y_only)
    _check_refined(before, after, kept_pairs, len(kept_counts), y_only)


def test_refine_kernel_with_other_steps_and_learning_rate():
    kept_counts = [RF_CACHED_PAIRS + 1, 5000]
    before, after, kept_pairs = _refine_batch(kept_counts, False, steps=37, lr=3e-3)
    _check_refined(before, after, kept_pairs, len(kept_counts), False, steps=37, lr=3e-3)


# ------------------------------------------------------------------------------------------ post-MLP path, 50 000 x 180
def test_post_mlp_path_at_the_reference_default_size():
    """test_gpu_parity.test_pipeline_vs_oracle_ragged_batch at eval.py's defaults: 50 000 tuples x 180 rotations (9 bmm_size
    chunks in get_topk_dir, ~5 000 kept pairs: the scale median selects from global memory) and a ragged scene of 40 955 tuples,
    whose percentile index leaves exactly ASM_STAGE = 4096 kept pairs (found with the oracle: 0.1 x 40 954 = 4095.4, so 4096
    errors lie below the interpolated threshold) -- the largest list the median still stages in LDS.  The oracle decodes the
    device's bins (C get_topk_dir); 6 s on the GPU host."""
    from test_gpu_parity import _scene_inputs
    Ns, Ts, R = [4096, 2500, 3000], [50000, 50000, 40955], 180
    scenes = [_scene_inputs(12, s, Ns[s], Ts[s], np.random.RandomState(40 + s)) for s in range(3)]
    pipe = VotingPipeline(Ns, Ts, k=5, res=2e-3, num_rots=R, cells_cap=1 << 21)
    pts = _d(np.concatenate([s[0]["pc"] for s in scenes]), torch.float32)
    idx, logits, u, sc = (_d(np.concatenate([s[i] for s in scenes]), dt)
                          for i, dt in ((1, torch.int32), (2, torch.float32), (3, torch.float32), (4, torch.float32)))
    res =pipe.results_to_numpy(pipe.vote(pts, idx, logits, u, sc))
    trig = (pipe.cs.cpu().numpy(), pipe.sn.cpu().numpy())
    bins_all, mask_all, errs_all = pipe.bins.cpu().numpy(), pipe.mask.cpu().numpy(), pipe.errs.cpu().numpy()
    thr_all, wt_all, counts_all = pipe.thr.cpu().numpy(), pipe.kept_wt.cpu().numpy(), pipe.counts.cpu().numpy()
    rot_all = pipe.rot.cpu().numpy()
    assert res["kept"][2] == ASM_STAGE and res["kept"].max() > ASM_STAGE
    t0 = 0
    for s, (scene, idx_s, lg, us, scl) in enumerate(scenes):
        T = Ts[s]
        ob = O.decode_bins(lg, us, scene["pc"][idx_s[:, :2]], return_margin=True)
        flips = (ob[0] != bins_all[t0:t0 + T])
        assert np.all(ob[4][flips] < 1e-5)
        onehot = np.full((T, 6, 32), -1e4, np.float32)
        np.put_along_axis(onehot, bins_all[t0:t0 + T, :, None].astype(np.int64), 0.0, -1)
        want = O.run_scene(scene["pc"], idx_s, onehot, scl, us, UP, RIGHT, FRONT, 2e-3, num_rots=R, trig=trig, topk_impl="c")
        r = res[s]
        assert r["argmax"] == want["argmax"] and r["peak"] == want["grid_obj"].max()
        assert np.array_equal(r["t"], want["T_est"])
        assert r["kept"] == int(want["pairs_mask"].sum())
        assert np.array_equal(mask_all[t0:t0 + T].astype(bool), want["pairs_mask"])
        assert np.array_equal(errs_all[t0:t0 + T], want["back_errs"])
        assert np.float32(thr_all[s]) == np.float32(want["thr"])
        kept = r["kept"]
        assert np.array_equal(wt_all[t0:t0 + kept], want["imp_pair_wt"])
        assert np.array_equal(rot_all[t0:t0 + T], want["targets_rot"])
        _check_rotation_counts(counts_all[:, s], scene["pc"], idx_s, want, trig)
        for name in ("up", "right"):
            assert int(r[name + "_idx"]) == want[name + "_idx"]
        assert np.allclose(r["R"], want["R_est"], atol=1e-6)
        assert np.array_equal(r["scale"], want["pred_scale"])
        assert np.array_equal(r["scale"].view(np.uint32), want["pred_scale"].view(np.uint32))
        assert np.linalg.norm(r["t"] - scene["t"]) < 5e-3
        cosang = abs(float(r["R"][:, 1] @ scene["R"][:, 1]))
        assert np.degrees(np.arccos(min(cosang, 1.0))) < 5.0
        t0 += T


# ------------------------------------------------------------------------------------------ whole step, 50 000 tuples
@pytest.mark.parametrize("cloud", ["synthetic", "voxel2mm"])
def test_whole_step_at_the_reference_default_tuples(cloud):
    """test_end_to_end_gpu's Step-vs-whole-scene-oracle comparison (same bars) at 4096 points x 50 000 tuples x 180 rotations,
    and the record's scale = the exact lower median of the device's own scale-head rows over the kept pairs.  The oracle's
    scene (C SHOT on all cores, NumPy MLP, C get_topk_dir): 2-3 s per cloud on the GPU host."""
    from cppf2_amd.benchlib import workloads as W
    from test_end_to_end_gpu import _args, check_step_against_the_oracle
    st = W.Step(_args(1, tuples=50000), 0, 1, DEV, cloud=cloud)
    st.run()
    torch.cuda.synchronize()
    rec, outs = check_step_against_the_oracle(st, 1, shot_threads=0)
    kept = int(rec["kept"][0])
    assert kept > ASM_STAGE
    rows = st.pipe.kept_tuple[:kept].long().cpu().numpy()
    x = st.scales_buf.cpu().numpy()[rows]
    assert np.array_equal(rec["scale"][0], np.sort(x, axis=0)[(kept - 1) // 2])


# ------------------------------------------------------------------------------------------ the reference's example cloud
def _pca_frame(pc):
    """A canonical frame for a cloud without ground truth: centroid, PCA axes (largest variance first; the first two signed so
    that the third moment along them is positive, the third their cross product), and the diagonal of the centroid-centred box
    that holds the cloud, so that (pc - c) @ R / diag lies in [-0.5, 0.5]^3."""
    p = pc.astype(np.float64)
    c = p.mean(0)
    _, vec = np.linalg.eigh(np.cov((p - c).T))
    R = vec[:, ::-1].copy()
    for j in range(2):
        if (((p - c) @ R[:, j]) ** 3).sum() < 0:
            R[:, j] = -R[:, j]
    R[:, 2] = np.cross(R[:, 0], R[:, 1])
    diag = float(np.linalg.norm(2 * np.abs((p - c) @ R).max(0)))
    return c, R, diag


def test_example_cloud_through_run_ensemble_at_the_reference_defaults(monkeypatch):
    """tests/golden/example_data (the reference's demo depth + mask) through the product's preprocessing (GPU back-projection,
    2 mm voxel down-sample of the `custom` config) and eval.run_ensemble at num_pairs=50000, num_rots=180, against
    oracle.pipeline_oracle.run_instance_ensemble as test_config3_gpu.test_ensemble_full_size_vs_oracle compares synthetic
    scenes.  The cloud has no ground truth: a PCA frame stands in for one, so the teacher prior makes it solvable and the votes
    are not ties.  4.5 s on the GPU host (C get_topk_dir)."""
    import json
    from PIL import Image
    monkeypatch.chdir(ROOT)
    import eval as ev
    e = json.load(open(os.path.join(GOLDEN, "full_summary.json")))["example_backproject"]
    d = np.array(Image.open(os.path.join(GOLDEN, "example_data", "depth.png"))).astype(np.float64) / float(e["depth_scale"])
    m = np.array(Image.open(os.path.join(GOLDEN, "example_data", "mask.png")))
    m = (m[..., 0] if m.ndim == 3 else m) > 0
    cfg, dino_model, shot_model = ev.load_custom(device=DEV)
    T, R, seed = 50000, 180, 0
    # eval.main's preprocessing (data="depth"), pinned
    pc_full, _ = ops.backproject(d, np.array(e["K"], dtype=np.float64), m, return_device=True)
    assert pc_full.shape[0] == e["n"]
    keep = ops.downsample(pc_full, cfg.res, seed, return_device=True)
    assert len(keep) == len(O.downsample(pc_full.cpu().numpy(), cfg.res, np.random.RandomState(0)))
    pc = pc_full[keep].cpu().numpy()
    N = pc.shape[0]
    assert N <= 50000 and ((pc.max(0) - pc.min(0)).max() / cfg.res) <= 1000
    c, Rc, diag = _pca_frame(pc)
    pc_canon = ((pc.astype(np.float64) - c) @ Rc / diag).astype(np.float32)
    assert np.abs(pc_canon).max() <= 0.5
    priors = ev._teacher_prior(pc_canon, DEV)
    g = torch.Generator(device="cpu").manual_seed(5)
    descs = [torch.nn.functional.normalize(torch.randn((N, 1024), generator=g), dim=-1).numpy()]
    r = ev.run_ensemble(cfg, dino_model, shot_model, [pc], descs, seed, [0], T, R, opt=False, up_sym=False, priors=priors,
                        keep=True)
    pipe = r["pipe"]
    assert int(r["records"][0]["ncell"][0]) == int(r["records"][1]["ncell"][0]) == ev.needed_cells(pc, cfg.res)
    trig = (pipe.cs.cpu().numpy(), pipe.sn.cpu().numpy())
    idx = r["idx"].cpu().numpy().astype(np.int64)
    assert np.array_equal(idx, O.sample_tuples(seed, 0, T, 5, N))
    w_dino = {k: v.detach().cpu().numpy() for k, v in dino_model.state_dict().items()}
    w_shot = {k: v.detach().cpu().numpy() for k, v in shot_model.state_dict().items()}
    # (1) the networks on a slice of the tuples (as test_ensemble_full_size_vs_oracle)
    sub = slice(0, 2000)
    lg_d, sc_d = PO.mlp_dino(w_dino, pc, descs[0], idx[sub])
    assert np.abs(lg_d - r["kept"][0]["raw_cls"][sub]).max() < 2e-4
    assert np.abs(sc_d - r["kept"][0]["pred_scales"][sub]).max() < 2e-4
    lg_s, sc_s = PO.mlp_shot(w_shot, pc, idx[sub], r["shot_feat"], r["normal"])
    assert np.abs(lg_s - r["kept"][1]["raw_cls"][sub]).max() < 2e-4
    assert np.abs(sc_s - r["kept"][1]["pred_scales"][sub]).max() < 2e-4
    # (2) both voting passes and the selection, the oracle decoding the device's bins
    per_model = []
    for mi in (0, 1):
        k = r["kept"][mi]
        ob = O.decode_bins(k["pred_cls"], k["u"], pc[idx[:, :2]], return_margin=True)
        flips = ob[0] != k["bins"]
        assert np.all(ob[4][flips] < 1e-5) and flips.mean() < 1e-3
        onehot = np.full((T, 6, 32), -1e4, np.float32)
        np.put_along_axis(onehot, k["bins"][:, :, None].astype(np.int64), 0.0, -1)
        per_model.append((onehot, k["pred_scales"], k["u"]))
    want = PO.run_instance_ensemble(pc, idx, per_model, cfg.up, cfg.right, cfg.front, cfg.res, num_rots=R, y_only=False,
                                    trig=trig, topk_impl="c")
    for mi in (0, 1):
        rec, o = r["records"][mi][0], want["models"][mi]
        assert rec["argmax"] == o["argmax"] and rec["peak"] == o["grid_obj"].max()
        assert np.array_equal(rec["t"], o["T_est"])
        assert np.array_equal(r["kept"][mi]["mask"], o["pairs_mask"])
        assert rec["kept"] > ASM_STAGE
        _check_rotation_counts(r["kept"][mi]["counts"][:, 0], pc, idx, o, trig)
        for name in ("up", "right"):
            assert int(rec[name + "_idx"]) == o[name + "_idx"]
        assert np.allclose(rec["R"], o["R_est"], atol=1e-6)
        assert np.array_equal(rec["scale"], o["pred_scale"])
        assert abs(r["losses"][mi][0] - o["loss"]) < 1e-7
    assert int(r["pick"][0]) == want["pick"]
    assert abs(r["best"][0] - want["loss"]) < 1e-7
    assert abs(want["models"][0]["loss"] - want["models"][1]["loss"]) > 1e-5          # the selection is not a coin flip
    assert np.float32(r["scale_norm"][0]) == np.float32(want["scale_norm"])
    rec = r["records"][r["pick"][0]][0]
    RT = np.eye(4)
    RT[:3, :3], RT[:3, 3] = rec["R"] * r["scale_norm"][0], rec["t"]
    assert np.allclose(RT, want["pred_RT"], atol=1e-6)
    assert np.allclose(r["scale"][0] / r["scale_norm"][0], want["pred_scale"], atol=1e-6)
    # the stand-in ground truth was found: centre within 5 mm of the centroid, first PCA axis within 5 degrees
    assert np.linalg.norm(rec["t"] - c) < 5e-3
    assert np.degrees(np.arccos(min(1.0, abs(float(rec["R"][:, 0] @ Rc[:, 0]))))) < 5.0
