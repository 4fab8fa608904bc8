/*
 * cppf_hip_experimental.h -- the EXPERIMENTAL part of libcppf_hip.so's C ABI (see cppf_hip.h for the stable part and the
 * conventions, which hold here too).  Nothing in this file is bound by the reference-facing modules' default paths; entries
 * may change or disappear without an ABI bump.  What is here and why it is kept:
 *   - launch forms superseded on the default paths but kept for A/B measurements (bench.py --separate-encode,
 *     --materialize-tuples, --mlp-arith native|split16) and as the two-kernel references the fused forms are tested against;
 *   - helpers of BASELINE configs[4]'s extensions (float16 feature table) that the reference does not have;
 *   - the logit prior of the synthetic benchmarks: THE REFERENCE HAS NO PRIOR (eval.py:225-235 draws from the network's own
 *     logits).  It exists because the reference's checkpoints are not available: random-init weights need a teacher for votes to
 *     cluster.  bench.py reports value_no_prior beside the headline;
 *   - a test hook;
 *   - the solid-interval checks on candidate poses (cppf2_amd/solid.py): opt-in and new;
 *   - the deviation statistic of the symmetry detection (cppf2_amd/symmetry.py): opt-in and new;
 *   - the oriented-box IoU of the NOCS scorer (cppf2_amd/box_iou.py): opt-in and new;
 *   - depth-view fusion into a signed distance volume and its surface mesh (cppf2_amd/fuse.py): new;
 *   - mesh simplification by vertex clustering with quadric representatives (cppf2_amd/simplify.py):
 *     opt-in and new;
 *   - depth frames tracked against the fused volume, for sequences with one known pose (cppf2_amd/track.py, DESIGN.md
 *     section 30): opt-in and new;
 *   - a depth frame's pose searched against the fused volume with no starting pose, which joins a second sequence of the object
 *     turned over (cppf2_amd/relocalise.py): opt-in and new;
 *   - mask proposals cut at concave edges, with or without a support plane (cppf2_amd/segment.py): opt-in
 *     and new.
 */
#ifndef CPPF_HIP_EXPERIMENTAL_H_
#define CPPF_HIP_EXPERIMENTAL_H_

#include "cppf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the synthetic benchmarks' logit prior ------------------------------------------------------------------------------
 * cppf_decode_bins with logit_prior float32 [T, 6, nb] (same shape as logits; NULL = cppf_decode_bins) added to the logits before
 * the softmax with one float32 add each. */
int cppf_decode_bins_prior(int B, const float* logits, const float* logit_prior, int nb, const float* uniforms,
                           const float* pts, const int32_t* idx, int k, const int32_t* pt_off, const int32_t* tup_off,
                           int64_t total_tuples, const double* h_axes, int32_t* bins, float* scaled, float* scale,
                           float* tr, float* rot, void* stream);
/* cppf_reslayer_split_decode with a prior: logit_prior float32 [rows, 192] or NULL; or prior_pos float32 [rows, 6] /
 * prior_inv_sigma (instead of logit_prior, never both): the prior GENERATED in the epilogue -- prior[t, c, k] =
 * -0.5 ((k - prior_pos[t, c]) * prior_inv_sigma)^2, float32, these three operations in this order -- a Gaussian bump in logit
 * space around a per-coordinate bin position: 24 bytes per row read instead of 768 (the array form costs the launch 0.34 ms per
 * 1.28 M rows, all of it its 983 MB of reads).  Bit-identical to passing the array built with the same three operations. */
int cppf_reslayer_split_decode_prior(const float* x, int64_t ldx, int32_t k_in, int64_t rows, const void* wq, int64_t wq_bytes,
                                     const float* b1, const float* b0, const float* logit_prior, const float* prior_pos,
                                     float prior_inv_sigma, const float* uniforms, int32_t* bins, int32_t* sched, void* stream);

/* ---- a2 / a3 variants -------------------------------------------------------------------------------------------------- */
/* The descriptor half alone, on normals the caller already has (e.g. from cppf_estimate_normals). */
int cppf_shot352_from_normals(int B, const float* pts, const int32_t* pt_off, int64_t total_points,
                              const float* normals, float shot_r, float* out_shot, float* out_rf,
                              void* workspace, int64_t workspace_bytes, void* stream);

/* out_half[i] = (float16) x[i], n elements (round to nearest even): the float16 feature table of BASELINE config 5 from the
 * point encoder's float32 output (cppf_encode_tuples_shot_f16 gathers it). */
int cppf_cast_f16(const float* x, void* out_half, int64_t n, void* stream);

/* Same row layout from a half-precision feature table (float16 [n, feat_dim], feat_dim % 8 == 0), float32 output
 * (BASELINE config 5, "fp16 features"; not in the reference -- equals the float32 entry on half-rounded features). */
int cppf_encode_tuples_shot_f16(int B, const float* pts, const float* normals, const void* feat_half, int feat_dim,
                                const int32_t* idx, int k, const int32_t* pt_off, const int32_t* tup_off,
                                int64_t total_tuples, float* out, void* stream);

/* a3' descriptor part (DINO model): replaces desc_pair_transform(cat_i desc_transform(desc[idx_i])) (train_dino.py:95-96)
 * by a gather-add of per-point products: tables float32[total_points, k, D] with tables[n][i] = W_i . d[n] (W_i = the i-th
 * column block of desc_pair_transform.weight, d = desc_transform(desc)), bias float32[D] or NULL;
 * out[t, out_col + c] = bias[c] + sum_i tables[pt_off[b] + idx[t,i]][i][c].  D % 4 == 0; out row stride in floats. */
int cppf_encode_tuples_dino(int B, const float* tables, int k, int D, const float* bias, const int32_t* idx,
                            const int32_t* pt_off, const int32_t* tup_off, int64_t total_tuples, float* out,
                            int out_stride, int out_col, void* stream);

/* cppf_kept_rows32 as int64[B, max_kept] (device): row = tup_off[b] + kept_tuple[tup_off[b] + j] for
 * j < kept_count[b], the scene's first tuple row otherwise -- the fixed-shape index a caller gathers per-pair tensors with
 * (e.g. the tuple features the scale head runs on, eval.py:272) without reading kept_count on the host. */
int cppf_kept_rows(int B, const int32_t* tup_off, const int32_t* kept_tuple, const int32_t* kept_count, int max_kept,
                   int64_t* rows, void* stream);

/* ---- superseded launch forms of the MLP ------------------------------------------------------------------------------- */
/* ---- 128-wide residual layer of the tuple / point encoders (train_shot.py:19-45 ResLayer with dim_in == dim_out == 128,
 * bn = dropout = False; five of the six layers of `tuple_encoder` and `shot_encoder`):
 *     x <- x + relu(x W1^T + b1) W2^T        in place on x float32[rows,128] (device, contiguous)
 * w1, w2: float32[128,128] row-major [out,in] (the nn.Linear weights), b1 float32[128]; fc2's bias is left to the caller
 * (it commutes with the residual stream).  One kernel on the f32 matrix cores: both products of a 32-row tile stay in
 * registers.  float32 in, float32 accumulate: results differ from a library GEMM's only by summation order. */
int cppf_reslayer128(float* x, int64_t rows, const float* w1, const float* b1, const float* w2, void* stream);

/* ---- the tuple encode feeding the tuple MLP without materialising its rows (train_shot.py:75-83 -> :100-111): the pair
 * features alone and the tuples' global point indices ...
 *   heads float32 [T, ld_heads >= 4 C(k,2)]: the first 4 C(k,2) columns of cppf_encode_tuples_shot's rows, bit for bit;
 *   gidx  int32 [T, k] = scene point base + idx
 * ... and the first ResLayer of the tuple encoder (a 128-wide projection layer, `chain` identity layers behind it) reading
 * row t = [heads[t, 0:head_cols] | table[gidx[t, 0]] | ... | table[gidx[t, slots-1]]] through its x-tile fetches: table
 * float32 [points, fdim] (the point encoder's output), fdim a power of two >= 8, head_cols % 8 == 0, slots <= 8; wq / b1 /
 * b0 / chain as cppf_reslayer_split for k_in = head_cols + slots * fdim.  Bit-identical to cppf_reslayer_split on the
 * materialised rows; saves writing and re-reading them (1.8 GB per 64 scenes). */
int cppf_encode_tuples_shot_heads(int B, const float* pts, const float* normals, const int32_t* idx, int k,
                                  const int32_t* pt_off, const int32_t* tup_off, int64_t total_tuples, float* heads,
                                  int32_t ld_heads, int32_t* gidx, void* stream);
int cppf_reslayer_split_gather(const float* heads, int64_t ld_heads, int32_t head_cols, const int32_t* gidx, int32_t slots,
                               const float* table, int32_t fdim, float* out, int64_t ldo, int32_t n_out, int64_t rows,
                               const void* wq, int64_t wq_bytes, const float* b1, const float* b0, int32_t chain,
                               int32_t* sched, void* stream);

/* The DINO model's two-kernel form of cppf_reslayer_split_sumencode:
 * cppf_encode_tuples_coord_heads: heads float32 [T, ld_heads >= round8(3 C(k,2))] = the coordinate columns of
 *   cppf_encode_tuples_coord's rows (train_dino.py:92), bit for bit, zero-padded to a multiple of 8 columns; gidx int32 [T, k] =
 *   scene point base + idx.
 * cppf_reslayer_split_sumgather: the first ResLayer on rows [heads | s(t)] with the per-point parts of its first products summed
 *   from tables float32 [points, slots, 256] (see cppf_reslayer_split_sumencode); also usable for the SHOT model (s(t) = the
 *   concatenated point features, train_shot.py:82: a re-slicing, no fold -- measured slower than the x-tile gather there).
 *   wq = cppf_reslayer_split_stream_bytes(head_cols, 128, 1, chain) bytes. */
int cppf_encode_tuples_coord_heads(int B, const float* pts, const int32_t* idx, int k, const int32_t* pt_off,
                                   const int32_t* tup_off, int64_t total_tuples, float* heads, int32_t ld_heads, int32_t* gidx,
                                   void* stream);
int cppf_reslayer_split_sumgather(const float* heads, int64_t ld_heads, int32_t head_cols, const int32_t* gidx, int32_t slots,
                                  const float* tables, int64_t ld_tables, float* out, int64_t ldo, int32_t n_out, int64_t rows,
                                  const void* wq, int64_t wq_bytes, const float* b1, const float* b0, int32_t chain,
                                  int32_t* sched, void* stream);

/* ---- the same ResLayer launches in f16x2 arithmetic (cppf2_amd.models.MLP_ARITH = "split16"; not the default): every
 * float32 operand as an fp16 pair hi + lo (RNE; 22-23 significant bits), the three products hi hi + hi lo + lo hi on the fp16
 * matrix cores, float32 accumulate -- half the matrix-core work of the exact bf16-triple form, error against float64 at the
 * level of a float32 GEMM's accumulation error (tests/test_mlp_split.py, bench.py mlp_error_vs_f64), but NOT exact products, and
 * fp16's range: activations must stay below 65504 in magnitude (larger ones become Inf -> NaN rows); activations whose lo piece
 * is subnormal keep an absolute resolution of 2^-25.  wq = fp16 (hi, lo) fragment pairs of weight_scale x the weights in the
 * fragment order of cppf_reslayer_split (cppf_reslayer_split16_stream_bytes bytes), b1 / b0 = weight_scale x the biases,
 * weight_scale a power of two chosen so that the largest |weight| x weight_scale is ~2^13.  One struct for all launch forms:
 * plain (x, out[, first_out = tap]); gather (gidx != NULL: x = heads with k_in head columns, table, slots, fdim; n_out = 128);
 * decode (uniforms != NULL: n_out = 192, chain = 0, bins out, logit_prior optional).  Unused members must be zero. */
typedef struct CppfReslayerSplit16Args {
  const float* x; int64_t ldx; int32_t k_in;
  float* out; int64_t ldo; int32_t n_out; int64_t rows;
  const void* wq; int64_t wq_bytes; const float* b1; const float* b0; int32_t chain;
  float weight_scale;
  float* first_out; int64_t ld_first;
  const int32_t* gidx; int32_t slots; const float* table; int32_t fdim;
  const float* logit_prior; const float* uniforms; int32_t* bins;
  void* stream;
  int32_t mode;            /* 0: the forms above; 1: plain Linear (cppf_linear_split: n_out % 256 == 0, b1 = bias or NULL, b0 NULL);
                              2: gather with per-point slot tables summed into the accumulators (cppf_reslayer_split_sumgather:
                              table = [points, slots, 256], ld_table its point pitch, fdim unused) */
  int64_t ld_table;
  int32_t* sched;          /* NULL or the block-scheduling counters (see cppf_reslayer_split; not used by mode 1) */
  const float* prior_pos;  /* decode: the generated prior of cppf_reslayer_split_decode (instead of logit_prior) or NULL */
  float prior_inv_sigma;
} CppfReslayerSplit16Args;
int64_t cppf_reslayer_split16_stream_bytes(int32_t k_in, int32_t n_out, int32_t proj, int32_t chain);
int cppf_reslayer_split16(const CppfReslayerSplit16Args* args);

/* Test hook: workgroups > 0 forces the number of persistent workgroups of every later cppf_reslayer_split* launch of this
 * process (the kernels' results do not depend on it; tests/test_mlp_split.py runs the counted-wait protocol at 1, 7 and all
 * CUs beside a saturating copy stream); 0 restores one workgroup per CU. */
int cppf_reslayer_split_debug_grid(int32_t workgroups);

/* ---- solid-interval checks on candidate poses: below the support plane, inside one another (not in the reference;
 * cppf2_amd/solid.py) ----
 * Per candidate two renders of one closed mesh at one pose, float32[P,H,W] each, 0 = nothing drawn: front (back faces culled: the
 * nearest front face) and back (the same call with every triangle's winding reversed: the nearest back face); [front, back] is
 * the first solid interval along the pixel's ray.  h_cand_off int32[I+1] on the HOST as cppf_scene_explain's (0 = h_cand_off[0]
 * <= ... <= h_cand_off[I] = P <= 2^24), I >= 1, H, W <= 8192, tau >= 0 (metres).  Per pixel: back_c = b > 0, solid_c = f > 0 &&
 * b > 0, open_c = (f > 0) != (b > 0) (float32 comparisons: NaN and -0.0 are not > 0).  The exact order of the float32
 * operations is stated in cppf2_amd/csrc/cppf_solid.hip.  Integer counts only: an image's outputs do not depend on the batch or
 * the order.  Experimental while the checks are opt-in and young: the signatures may still change without an ABI bump.
 *
 * cppf_support_counts: planes float32[I,4] = (n, d) as cppf_plane_fit writes them, Kmat float32[I,4] = (fx, fy, cx, cy).  Pixel
 * (r, c), z = b: x = ((((float)c + 0.5f) - cx) * z) / fx, y = ((((float)r + 0.5f) - cy) * z) / fy, h = ((n.x*x + n.y*y) + n.z*z)
 * + d; sunk_c = back_c && h < -tau.  A plane of zeros or of NaN sinks nothing.  counts int64[P,4] = (back, sunk, solid, open)
 * per candidate, any number of candidates per image.  One launch per 128 images behind one clear, no workspace.
 *
 * cppf_solid_overlap: at most 64 candidates per image.  inter int64[P,64]: row cand_off[i] + a, column j < C_i = the pixels
 * where a and j are both solid and (double)fminf(b_a, b_j) - (double)fmaxf(f_a, f_j) > (double)tau; symmetric, the diagonal = the
 * solid pixels of a, columns C_i .. 63 are 0.  workspace: cppf_solid_overlap_workspace_bytes(I, H, W) bytes (8 per pixel; 0 for
 * sizes the call refuses), 8-byte aligned.  Two launches per 128 images behind one clear, no host synchronisation.
 *
 * Both return CPPF_EINVAL for a negative or NaN tau, bad offsets, H or W above 8192, P above 2^24 and null pointers;
 * cppf_solid_overlap returns CPPF_EUNSUPPORTED for more than 64 candidates on an image and CPPF_ECAPACITY for a workspace that
 * is too small; all before any device work. */
int cppf_support_counts(int I, int H, int W, const float* front, const float* back, const int32_t* h_cand_off, int P,
                        const float* planes, const float* Kmat, float tau, int64_t* counts, void* stream);
int64_t cppf_solid_overlap_workspace_bytes(int I, int H, int W);
int cppf_solid_overlap(int I, int H, int W, const float* front, const float* back, const int32_t* h_cand_off, int P, float tau,
                       int64_t* inter, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- a mesh's symmetries: deviation of a sampled surface from the mesh under candidate maps (the reference has no such step) ----
 * cppf_sym_deviation: queries float32[nq,3] (points of the surface), tris float32[nf,9] (three vertices per row; triangles
 * without area contribute nothing), maps float64[nc,12] (row-major 3x4 maps x -> R x + t, cppf_mssd_mspd's syms layout), all in
 * one frame.  Out, float32[nc]: max_d2[c] = max over the queries of min over the triangles of the SQUARED distance between the
 * mapped query and the triangle (the closest point by the vertex / edge / face regions): the one-sided Hausdorff deviation of
 * the mapped samples from the mesh, squared.  Each map is rounded to float32 once, everything after it is float32; a NaN
 * distance is ignored, so a non-finite query (every map) or a non-finite map (that map) gives +inf.  nq >= 1, nf >= 1,
 * 0 <= nc <= 65535; nc = 0 launches nothing.  No workspace; one launch after the output is cleared on the stream.  An integer
 * atomic maximum only: the output does not depend on the batch or the order.  The exact order of the operations is stated in
 * cppf2_amd/csrc/cppf_symmetry.hip.  Experimental while the detection is opt-in and young: the stable
 * interface keeps its 74 entry points. */
int cppf_sym_deviation(const float* queries, int nq, const float* tris, int nf, const double* maps, int nc, float* max_d2,
                       void* stream);

/* ---- 3-D IoU of oriented boxes, batched (the reference computes it on the host: utils/util.py:475-547, utils/iou.py) ----
 * cppf_box_iou: P box pairs, everything float64 on the device.  Box 1 = R1[P,9] (row-major, orthonormal: an isotropic scale is
 * divided out by the caller), t1[P,3] (centre), s1[P,3] (full edge lengths); box 2 = R2, t2, s2 alike.  turns int32[P]:
 * iou[p] = max over i < turns[p] of the IoU of box 1 turned by 2 pi i / turns[p] about its own y axis (R1 . Ry) with box 2;
 * turns = 1 is the plain IoU, 36 the toolkit's rule for the classes that are symmetric about y.  turn_cs float64
 * [max_turns (max_turns + 1) / 2, 2]: (cos, sin)(2 pi i / n) at row n (n - 1) / 2 + i for every n = 1 .. max_turns, i < n,
 * filled by the host, so that the device's sincos plays no part in the result.  0 <= P <= 2^20 (1 048 576; callers chunk),
 * 1 <= max_turns <= 64; P = 0 launches nothing.  A pair whose turns is outside 1 .. max_turns gets NaN.
 * The volume of the intersection is summed over its (at most twelve) faces, each a box face clipped by the other box's six
 * closed half-spaces.  Where a plane of box 2 nearly coincides with a face of box 1 (normals within 1e-5 of parallel, the plane
 * within 1e-5 (|s1| + |s2| + |t1 - t2|) of the face's centre) that face's lane scores both faces, so that one decision says which
 * plane bounds the intersection where; what this neglects is of second order, about 1e-10 relative, and planes tilted by more
 * are met by plain clipping, whose error there is of the same size.  Checked to 1e-9: exact ties (identical boxes 1, boxes
 * sharing faces their ratio, boxes touching in a face exactly 0.0), the same pairs turned and shifted by 1e-15 .. 1e-4, generic
 * pairs.  Boxes thinner than 1e-5 of the pair's size are outside what was checked.  No workspace; one launch after the output is cleared on the stream.  A 64-bit integer atomic maximum
 * only: the output does not depend on the batch or the order.  The exact order of the operations is stated in
 * cppf2_amd/csrc/cppf_box_iou.hip.  Experimental while the device scorer is opt-in and young: the stable
 * interface keeps its 74 entry points. */
int cppf_box_iou(const double* R1, const double* t1, const double* s1, const double* R2, const double* t2, const double* s2,
                 const int32_t* turns, const double* turn_cs, int max_turns, int P, double* iou, void* stream);

/* ---- a mesh from posed depth views: truncated signed distance volume, marching tetrahedra (the reference has no such step) ----
 * The volume is two device arrays, z fastest: acc float32 [nx,ny,nz] (the sum of the observations) and wsum int32 [nx,ny,nz]
 * (their number); node (i,j,k) sits at h_origin + (i,j,k) * voxel in the object's frame, metres.  h_origin: double[3] on the
 * HOST, rounded to float32 once; h_K: double[4] = (fx, fy, cx, cy) on the HOST, rounded alike.  nx, ny, nz >= 1 and
 * nx ny nz <= 2^27 (134 217 728 nodes, 512^3: 1 GiB of volume); voxel, trunc, znear > 0 and finite.  The exact order of the
 * float32 operations is stated in cppf2_amd/csrc/cppf_fuse.hip and restated in tests/fuse_ref.py.
 *
 * cppf_tsdf_integrate: adds V views (0 <= V <= 65536; 0 launches nothing) to the caller's acc / wsum (zeroed by the caller
 * before the first call) in one launch: depth float32 [V,H,W] (metres; 0, negative, NaN and infinite = no reading), masks uint8
 * [V,H,W] or NULL (non-zero = the object), poses float32 [V,12] (row-major 3x4, model -> OpenCV camera), 1 <= H, W <= 16384.
 * pixel_offset: 0 for images whose pixel (r, c) lies on the ray through (c, r) (cppf_backproject's convention), 0.5 for images
 * sampled at pixel centres (cppf_render_depth).  A node at camera depth zc >= znear that projects into the image at a pixel
 * with a reading d observes min((d - zc) / trunc, 1) when the pixel is inside the mask (or no masks are given) and
 * d - zc >= -trunc; outside the mask it observes 1 when d - zc > 0 (free space) and nothing otherwise, so that background
 * never becomes surface and still carves.  The views are summed in order inside the kernel: views 0..V-1 in one call give the
 * bytes of any split into consecutive calls.
 *
 * cppf_tsdf_extract: the surface tsdf = acc / wsum = 0 by marching tetrahedra (six per cell around the body diagonal).  A node
 * is known iff wsum >= min_weight (>= 1) and inside iff tsdf < 0; a cell is processed iff its 8 corners are known.  Out:
 * tris float32 [capacity,9] (three vertices per row, counter-clockwise seen from the outside), keys int64 [capacity,3] (per
 * vertex 8 * lo + (dx | dy << 1 | dz << 2) of the grid edge it lies on, lo = the smaller linear node index (i ny + j) nz + k of
 * the edge's ends, (dx,dy,dz) the step to the other end: equal keys have equal bits, so welding by key is exact), status int64
 * [2] = (triangles needed, cells that produced any).  Order: cell, tetrahedron, triangle.  If more triangles are needed than
 * `capacity` only status is written: grow the buffers and call again (capacity 0 with tris = keys = NULL just counts).
 * Triangles without area (a node exactly 0) are emitted like any other.  workspace: cppf_tsdf_extract_workspace_bytes(nx, ny,
 * nz) bytes (-1 for sizes the call refuses), 8-byte aligned.  Three launches, no host synchronisation.
 *
 * All return CPPF_EINVAL for null pointers, dims < 1 or above the size limit, non-positive or non-finite voxel / trunc / znear,
 * min_weight < 1, a negative capacity and a workspace that is too small; all before any device work. */
int cppf_tsdf_integrate(int V, const float* depth, const uint8_t* masks, const float* poses, int H, int W, const double* h_K,
                        float pixel_offset, const double* h_origin, float voxel, int nx, int ny, int nz, float trunc, float znear,
                        float* acc, int32_t* wsum, void* stream);
int64_t cppf_tsdf_extract_workspace_bytes(int nx, int ny, int nz);
int cppf_tsdf_extract(const float* acc, const int32_t* wsum, const double* h_origin, float voxel, int nx, int ny, int nz,
                      int min_weight, int64_t capacity, float* tris, int64_t* keys, int64_t* status, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* ---- a mesh simplified by vertex clustering with quadric representatives (the reference has no such step) ----
 * The lattice: cell (i,j,k), 0 <= i,j,k < 2^21, is [o + i cell, o + (i+1) cell) per axis, o = h_origin (double[3] on the HOST)
 * rounded to float32 once, cell > 0 and finite, metres.  The exact order of the operations is stated in
 * cppf2_amd/csrc/cppf_simplify.hip and restated in tests/simplify_ref.py.
 *
 * cppf_cluster_keys: keys int64 [n] of verts float32 [n,3]: i << 42 | j << 21 | k of the vertex' cell, float32 arithmetic
 * (t = (x - o) / cell per axis, inside iff 0 <= t < 2^21 on every axis, decided in float32 before any cast), -1 for a vertex
 * outside the lattice or not finite.  A coordinate exactly on a boundary belongs to the upper cell.
 *
 * cppf_cluster_quadrics: pos float32 [nc,3], one representative per cluster.  verts float32 [n,3], faces int32 [nf,3]
 * (nf <= 715 827 882), corners int32 [m] (entry 3 f + j = corner j of face f; 0 <= m <= 3 nf) sorted by cluster, seg_off int64
 * [nc+1] (cluster c owns corners[seg_off[c] .. seg_off[c+1])), keys int64 [nc] (each cluster's cell).  Float64, one lane per
 * cluster, the corners summed sequentially in list order (the order is part of the definition; no atomics).  The
 * representative minimises sum over the cluster's corners' triangles of area (u . x - d)^2 + lam area |x - centroid|^2 (u, d
 * the triangle's plane; x relative to the cell's centre), i.e. solves (A + lam w I) x = b + lam m, symmetric positive definite
 * with condition number at most (1 + lam) / lam, by LDL^T without pivoting; a cluster of triangles without area gets the mean
 * of its corners; the result is clamped into the cell and rounded to float32 once.  lam > 0 and finite.  A corner or vertex
 * index outside its array skips that corner; a negative key gives NaN.
 *
 * Both: n, nf, nc = 0 are valid calls that launch nothing; no workspace; one launch each.  CPPF_EINVAL for null required
 * pointers, negative counts, m outside [0, 3 nf], a non-finite origin and cell or lam not positive and finite; all before any
 * device work.  Experimental while the stage is opt-in and young: the stable interface keeps its 74
 * entry points. */
int cppf_cluster_keys(const float* verts, int n, const double* h_origin, float cell, int64_t* keys, void* stream);
int cppf_cluster_quadrics(const float* verts, int n, const int32_t* faces, int nf, const int32_t* corners, int64_t m,
                          const int64_t* seg_off, const int64_t* keys, int nc, const double* h_origin, float cell, double lam,
                          float* pos, void* stream);

/* ---- depth frames tracked against the signed distance volume (the reference has no such step) ----
 * cppf_tsdf_track: B frames (0 <= B <= 65535; 0 launches nothing) aligned to the volume acc / wsum of cppf_tsdf_integrate
 * (described above; h_origin, voxel, nx, ny, nz, trunc and h_K = (fx, fy, cx, cy) as there, fx, fy > 0) by point-to-plane
 * steps on the volume's trilinear value and gradient (Bylow et al., RSS 2013): no mesh, no raycast, no search.  depth float32
 * [B,H,W] (metres; 0, negative, NaN and infinite = no reading), masks uint8 [B,H,W] or NULL (non-zero = use the pixel),
 * 1 <= H, W <= 16384; the pixels (r, c) with r and c multiples of stride (>= 1) take part; pixel (r, c) lies on the ray
 * through (c + pixel_offset, r + pixel_offset), the convention cppf_tsdf_integrate inverts.  poses: float64 [B,12] on the
 * DEVICE (row-major 3x4, model -> OpenCV camera), each frame's start, updated in place.  iters (>= 0; 0 launches nothing)
 * iterations of two launches each, no host synchronisation; h_dk: float32 [iters] on the HOST, iteration k's inlier gate in
 * metres on |trunc * phi|, each positive and finite.  A pixel takes part when its point falls in a cell whose eight nodes
 * have wsum >= min_weight (>= 1) and the gradient there is not zero.  The step is cppf_icp_refine's minimum-norm Gauss-Newton
 * step (unobserved directions do not move); fewer than 6 inliers, rank 0 or a zero or non-finite step leave the pose's bytes
 * as they are.  stats float32 [B,4]: inliers of the last iteration, sqrt(sum e^2 / inliers), inliers / gated pixels (pixels
 * inside the mask with a reading), iterations that moved the pose; written only when iters > 0.  Deterministic: no atomics,
 * every sum in a fixed order, so B frames in one call give the bytes of B calls of one frame.  The exact order of the
 * operations is stated in cppf2_amd/csrc/cppf_track.hip and restated in tests/track_ref.py.
 * workspace: cppf_tsdf_track_workspace_bytes(B, H, W, stride) bytes (-1 for sizes the call refuses), 8-byte aligned.
 * CPPF_EINVAL, before any device work, for: h_K, h_origin, acc or wsum NULL; depth, poses, stats or workspace NULL when B > 0;
 * h_dk NULL when iters > 0; B or iters < 0; stride < 1; H or W outside 1..16384; the volume checks of cppf_tsdf_extract;
 * min_weight < 1; trunc, fx or fy not positive and finite; a gate that is not positive and finite; a workspace that is too
 * small.  An axis of one node is valid: no cells, no inliers, the poses keep their bytes. */
int64_t cppf_tsdf_track_workspace_bytes(int B, int H, int W, int stride);
int cppf_tsdf_track(int B, const float* depth, const uint8_t* masks, int H, int W, const double* h_K, float pixel_offset,
                    int stride, const float* acc, const int32_t* wsum, const double* h_origin, float voxel, int nx, int ny, int nz,
                    float trunc, int min_weight, int iters, const float* h_dk, double* poses, float* stats, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* ---- a fused volume closed where no view saw it: support-plane bottom, enclosed unseen space (the reference has no such step) ----
 * cppf_tsdf_close: reads the volume acc / wsum of cppf_tsdf_integrate (described above; h_origin, voxel, nx, ny, nz, trunc as
 * there) and writes a NEW volume acc_out float32 / wsum_out int32 [nx,ny,nz], state uint8 [nx,ny,nz] and stats int64 [4] (the
 * nodes per state), all on the device.  h_plane: double[4] = (a, b, c, d) on the HOST or NULL: the support plane a x + b y +
 * c z + d = 0 in the object's frame, metres, unit normal (|a^2 + b^2 + c^2 - 1| <= 1e-3), the object on the positive side;
 * rounded to float32 once.  Per node, float32: known = wsum >= min_weight (>= 1), t = acc / (float)wsum for a known node and -1
 * otherwise; with a plane h = ((a x + b y) + c z) + d at the node, b = (-h) / trunc clamped to [-1, 1], below = h <= 0 (without:
 * b = -1, below = false).  The nodes that are neither known nor below are joined by 6-connectivity; such a component is open
 * iff it holds a node on a face of the volume.  An open node: acc_out = 0, wsum_out = 0, state 3 (still unknown to
 * cppf_tsdf_extract).  Every other node: acc_out = (b > t) ? b : t, wsum_out = 1, state 0 (known), 1 (enclosed and never seen:
 * inside, sharpened to the plane within trunc of it) or 2 (unseen and below the plane: outside) -- the solid (observed, or
 * enclosed and never seen) intersected with the half-space above the plane.  cppf_tsdf_extract(acc_out, wsum_out,
 * min_weight = 1) then sees acc_out bit for bit.  The outputs depend on component membership only: two calls give the same
 * bytes.  The stats are cleared, then four launches; no host synchronisation.  The exact order of the operations is stated in
 * cppf2_amd/csrc/cppf_close.hip and restated in tests/close_ref.py.
 * workspace: cppf_tsdf_close_workspace_bytes(nx, ny, nz) bytes (-1 for sizes the call refuses), 8-byte aligned.
 * CPPF_EINVAL, before any device work, for: the volume checks of cppf_tsdf_extract; a NULL pointer other than h_plane; an
 * output (the workspace included) that overlaps acc, wsum or another output; a plane that is not finite or whose normal is not
 * a unit vector; trunc not positive and finite; min_weight < 1; a workspace that is too small. */
int64_t cppf_tsdf_close_workspace_bytes(int nx, int ny, int nz);
int cppf_tsdf_close(const float* acc, const int32_t* wsum, const double* h_origin, float voxel, int nx, int ny, int nz, float trunc,
                    int min_weight, const double* h_plane, float* acc_out, int32_t* wsum_out, uint8_t* state, int64_t* stats,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the pose of a depth frame against a fused volume with no starting pose: exhaustive search (the reference has no such step) ----
 * cppf_tsdf_pose_scores: scores int32 [NR,NT,4] on the device = (inliers, misses, unknown, outside) of candidate (r, j), summing
 * to P.  The volume acc / wsum, h_origin, voxel, nx, ny, nz, trunc and min_weight as cppf_tsdf_track takes them.  points float32
 * [P,3], camera frame, 1 <= P <= 2048; rotations float64 [NR,9], row-major, model -> camera, cast to float32 entry by entry;
 * offsets int32 [NT,3], whole nodes of the model frame (all three on the device); h_pivot_cam c and h_pivot_model m0: float[3]
 * on the HOST; tau float32: the inlier distance on the volume's value, metres.  Per point p and rotation R, float32 in this
 * order: d = p - c; x = R^T d in cppf_tsdf_track's expression; q = x + m0; g = (q - o) / voxel per axis.  A point with a g that
 * is not finite or has |g| >= 2^20 on any axis is outside for every offset.  Otherwise fl = floorf(g), f = g - fl, and for offset
 * j the cell is i = (int)fl + off_j: outside unless 0 <= i <= n - 2 on every axis; unknown if any of the cell's 8 corners has
 * wsum < min_weight; otherwise phi is cppf_tsdf_track's trilinear value of acc / (float)wsum at fractions f, and the point is an
 * inlier iff fabsf(trunc * phi) <= tau, else a miss.  The pose of candidate (r, j) is R_r, t = c - R_r (m0 + off_j voxel).  One
 * launch, no atomics, no workspace, no host synchronisation; the exact order of the operations is stated in
 * cppf2_amd/csrc/cppf_relocalise.hip and restated in tests/relocalise_ref.py.  NR = 0 or NT = 0: valid, nothing is written.
 * CPPF_EINVAL, before any device work, for: a NULL acc, wsum, h_origin, points or pivot (rotations, offsets and scores too
 * unless NR = 0 or NT = 0); P outside 1..2048; NR or NT < 0 or NR * NT > 2^29; the volume checks of cppf_tsdf_extract; voxel,
 * trunc or tau not positive and finite; a pivot that is not finite; min_weight < 1. */
int cppf_tsdf_pose_scores(const float* acc, const int32_t* wsum, const double* h_origin, float voxel, int nx, int ny, int nz,
                          float trunc, int min_weight, const float* points, int P, const double* rotations, int NR,
                          const float* h_pivot_cam, const float* h_pivot_model, const int32_t* offsets, int NT, float tau,
                          int32_t* scores, void* stream);

/* ---- sensor depth conditioned before anything reads it: mixed pixels dropped, smoothing within a surface (the reference has no such step) ----
 * cppf_depth_condition: depth float32 [I,H,W] (metres) -> out float32 [I,H,W] and counts int32 [I,3], all on the device.  A
 * reading is valid if it is finite and > 0 (a denormal is).  tol(z) = jump + (jump_rel * z), float32, product and sum rounded
 * each; every comparison is fabsf(q - z) <= tol(z) with z the CENTRE pixel's reading.  Stage 1 (flying pixels): for a valid
 * pixel, support = the number of offsets (dy, dx) != (0, 0) in [-r1, r1]^2 whose position lies outside the image or holds a
 * valid reading within tol; d1 = z if support >= min_support, else 0; an invalid pixel gives 0 (NaN, infinities and negatives
 * leave as 0).  It reads the input only and is not iterated; with r1 = 0 there is no offset, and min_support = 0 keeps every
 * valid pixel.  Stage 2 (smoothing, r2 = 0 switches it off) runs on d1: for a pixel with d1 > 0, s = z, n = 1, then over the
 * first half of the window in row-major order (dy = -r2 .. -1 with every dx, then dy = 0 with dx = -r2 .. -1) the pair
 * a = d1(p + o), b = d1(p - o) enters -- s = (s + a) + b, n += 2 -- iff both positions are inside the image, both values are
 * > 0 and both are within tol(z); out = s / (float)n, correctly rounded; 0 where d1 = 0.  counts[i] = (valid readings of image
 * i, valid readings that stage 1 removed, pixels with n > 1).  The counts are cleared, then one launch for all I images; no
 * atomics but the integer counts, no workspace, no host synchronisation: two calls give the same bytes.  The exact order of the
 * operations is stated in cppf2_amd/csrc/cppf_depthfilter.hip and restated in tests/depth_condition_ref.py.  I = 0: valid,
 * nothing is written.
 * CPPF_EINVAL, before any device work (out and counts keep their bytes), for: I < 0; H or W outside 1..16384; r1 or r2 outside
 * 0..4; min_support outside 0..(2 r1 + 1)^2; jump or jump_rel negative or not finite; and, when I > 0, a NULL depth, out or
 * counts, or an out that overlaps depth (stage 1 reads neighbours: the operation cannot run in place). */
int cppf_depth_condition(const float* depth, int I, int H, int W, int r1, int min_support, int r2, float jump, float jump_rel,
                         float* out, int32_t* counts, void* stream);

/* ---- depth views fused with weights by viewing angle: small integer weights per pixel (the reference has no such step) ----
 * cppf_depth_weights: depth float32 [I,H,W] (metres) -> weights uint8 [I,H,W] and counts int32 [I,3], all on the device.  h_K =
 * (fx, fy, cx, cy): double[4] on the HOST, cast to float32 like cppf_tsdf_integrate's; pixel (r, c) lies on the ray through
 * (c + pixel_offset, r + pixel_offset).  valid(q), tol(z) = jump + (jump_rel * z) and near(q, z) are cppf_depth_condition's, z
 * the centre's reading.  P(c, r, d) = ((((float)c + pixel_offset) - cx) / fx * d, (((float)r + pixel_offset) - cy) / fy * d, d).
 * A valid pixel p = P(c, r, z) gets weight 0 unless the four positions (c -+ step, r), (c, r -+ step) lie inside the image and
 * hold valid readings near z.  Otherwise tx = P(right) - P(left), ty = P(down) - P(up), n = tx x ty (each component a*b - c*d),
 * a = (n.x*p.x + n.y*p.y) + n.z*p.z, nn = n.n and pp = p.p summed the same way, den = nn * pp; weight 0 unless 0 < den < inf;
 * c = sqrtf((a * a) / den), the cosine between the pixel's ray and the surface normal; weight 0 unless c >= cos_min; otherwise
 * t = floorf(c * (float)levels + 0.5f) clamped to [1, levels].  An invalid pixel gets 0.  counts[i] = (valid readings of image
 * i, valid readings with weight 0, readings with weight `levels`).  Every float32 operation is rounded where it is written
 * (no fused multiply-add), divide and square root correctly rounded; the exact order is stated in
 * cppf2_amd/csrc/cppf_depthweights.hip and restated in tests/depth_weights_ref.py.  The counts are cleared, then one launch for
 * all I images; no workspace, no host synchronisation, no atomics but the integer counts.  I = 0: valid, nothing is written.
 * CPPF_EINVAL, before any device work, for: I < 0; H or W outside 1..16384; step outside 1..4; levels outside 1..255; cos_min
 * outside [0, 1) or NaN; jump or jump_rel negative or not finite; a pixel_offset that is not finite; h_K NULL; and, when I > 0,
 * a NULL depth, weights or counts, or an output that overlaps depth.
 *
 * cppf_tsdf_integrate_weighted: cppf_tsdf_integrate (above) with a weight per observation.  weights uint8 [V,H,W] on the device
 * (required when V > 0), carve_weight in 0..255.  Per node and view everything up to the observation is cppf_tsdf_integrate's;
 * then an observation q = sdf / trunc < 1 inside the mask (or without masks) has w = weights[v,row,col], and the constant
 * observation 1 (q not < 1 inside the mask; free space outside the mask) has w = carve_weight: a silhouette pixel has no normal
 * but still says that the space in front of it is empty.  w = 0 skips; otherwise acc = acc + (float)w * obs, wsum += w.  The
 * volume keeps its layout: acc is the weighted sum, wsum the sum of the weights, acc / (float)wsum the weighted mean, and
 * min_weight of cppf_tsdf_extract, cppf_tsdf_track, cppf_tsdf_close and cppf_tsdf_pose_scores is then a threshold in units of
 * weight.  The views are summed in order inside the kernel: one call gives the bytes of any split into consecutive calls; all
 * weights 1 and carve_weight 1 give cppf_tsdf_integrate's bytes.  wsum is int32 and one call adds at most 65 536 x 255 to a
 * node: the caller owns the total over its calls.  CPPF_EINVAL as cppf_tsdf_integrate, and for carve_weight outside 0..255 and,
 * when V > 0, a NULL weights. */
int cppf_depth_weights(const float* depth, int I, int H, int W, const double* h_K, float pixel_offset, int step, float jump,
                       float jump_rel, int levels, float cos_min, uint8_t* weights, int32_t* counts, void* stream);
int cppf_tsdf_integrate_weighted(int V, const float* depth, const uint8_t* masks, const float* poses, const uint8_t* weights,
                                 int carve_weight, int H, int W, const double* h_K, float pixel_offset, const double* h_origin,
                                 float voxel, int nx, int ny, int nz, float trunc, float znear, float* acc, int32_t* wsum,
                                 void* stream);

/* ---- mask proposals without a support plane: segments cut at concave edges (the reference has no such step) ----
 * cppf_concave_edges: depths float32 [I,H,W] (metres), Kmat float32 [I,4] = (fx, fy, cx, cy), fg uint8 [I,H,W] or NULL -> keep
 * uint8 [I,H,W] and counts int32 [I,3], all on the device.  valid and the point of a pixel are cppf_plane_fit's: depth > 0 &&
 * depth < +inf; z = depth, x = ((float)c - cx) * z / fx, y = ((float)r - cy) * z / fy.  The profile of a pixel B = (r, c) along
 * e = (0, 1) or (1, 0) uses A = the pixel at -step e and C = the pixel at +step e and gives a verdict only when both lie inside
 * the image, all three are valid, fabsf(zA - zB) <= reach and fabsf(zC - zB) <= reach.  With u = B - A, t = C - A,
 * tt = (t.x*t.x + t.y*t.y) + t.z*t.z, ut = (u.x*t.x + u.y*t.y) + u.z*t.z, o = u * tt - t * ut (per component: two rounded
 * products, one difference; tt times B's offset from the chord AC), ob = (o.x*B.x + o.y*B.y) + o.z*B.z, oo = o.o summed the same
 * way and t3 = (tt * tt) * tt, the profile is concave iff ob > 0 (B lies behind the chord) && 4.0f * oo > k2 * t3 (the turn
 * between the two sides exceeds the angle of k2 = (float)tan(angle / 2)^2) && oo > floor2 * (tt * tt) (the offset exceeds the
 * distance of floor2 = (float)floor^2).  A pixel is an edge when it is valid and either profile is concave; keep = 255 where
 * the pixel is valid, is no edge and (fg == NULL or fg != 0), else 0; counts[i] = (valid pixels, edge pixels, kept pixels) of
 * image i.  The profiles read the whole depth image, never only fg.  Every float32 operation is rounded where it is written (no
 * fused multiply-add), the divide correctly rounded; tests/concave_ref.py restates the order.  The counts are cleared, then one
 * launch for all I images; no workspace, no host synchronisation, no atomics but the integer counts; an image's outputs do not
 * depend on its place in the batch.  keep may be fg itself.  I = 0: valid, nothing is written.
 * CPPF_EINVAL, before any device work, for: I < 0; H or W outside 1..8192; step outside 1..8; k2, floor2 or reach negative or
 * not finite; and, when I > 0, a NULL depths, Kmat, keep or counts, or a keep that overlaps depths. */
int cppf_concave_edges(int I, int H, int W, const float* depths, const float* Kmat, const uint8_t* fg, int step, float k2,
                       float floor2, float reach, uint8_t* keep, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CPPF_HIP_EXPERIMENTAL_H_ */
