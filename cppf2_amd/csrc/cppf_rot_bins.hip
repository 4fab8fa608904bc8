// cppf_rot_bins.hip -- rotation vote fused with the sphere-bin counts (dense and lookup-table paths), and the stand-alone
// halves cppf_vote_rotation / cppf_sphere_counts.  gfx950 only.  See include/cppf_hip.h for the contract of each entry point.
#include "cppf_common.h"

// =============================================================================================
// a8 + a9. vote_rotation (train_dino.py:218-239) fused with get_topk_dir (eval.py:37-51).
//
// Dense kernel: a workgroup takes pairs_per_block kept pairs of one (scene, axis), generates their
// pairs_per_block*num_rots candidate axes once into LDS (one thread per candidate), then every thread owns every
// RB_THREADS-th sphere bin and walks the candidate list (LDS broadcast reads), accumulating
// 1/weight in float64 for candidates inside the cone.  Per-chunk (bmm_size rows) float64 sums are merged
// with float64 atomics and folded into float32 counts chunk by chunk, exactly like the reference's
// `counts += torch.sum(... / wt, 0)`.
// =============================================================================================
#define RB_THREADS 256
#define RB_MAX_CAND 1024

struct RotCand {
  float x, y, z;
  int slot;      // chunk id of the row this candidate occupies (absolute); -1 = skip
  double inv_wt;
};

// one candidate axis (train_dino.py:233-237)
__device__ __forceinline__ void rot_candidate(const PairFrame& f, float tn, float cs, float sn, float& ox, float& oy,
                                              float& oz) {
  // x = co / clamp_min(|co|, 1e-7); y = cross(x, u)
  const float den = fmaxf(f.nco, 1e-7f);
  const float xx = f.cox / den, xy = f.coy / den, xz = f.coz / den;
  const float yx = cross_term(xy, f.uz, xz, f.uy);
  const float yy = cross_term(xz, f.ux, xx, f.uz);
  const float yz = cross_term(xx, f.uy, xy, f.ux);
  const float offx = cs * xx + sn * yx, offy = cs * xy + sn * yy, offz = cs * xz + sn * yz;
  const float sg = (tn > 0.0f) ? 1.0f : -1.0f;
  const float ux = tn * offx + sg * f.ux, uy = tn * offy + sg * f.uy, uz = tn * offz + sg * f.uz;
  const float n = fmaxf(norm3_fused(ux, uy, uz), 1e-7f);
  ox = ux / n; oy = uy / n; oz = uz / n;
}

__global__ __launch_bounds__(RB_THREADS) void rot_bins_dense_kernel(
    const float* __restrict__ pts, const int32_t* __restrict__ pt_off, const int32_t* __restrict__ idx, int k,
    const int32_t* __restrict__ tup_off, const float* __restrict__ rot, int rot_col,
    const int32_t* __restrict__ kept_tuple, const int32_t* __restrict__ kept_count,
    const double* __restrict__ kept_wt, const int32_t* __restrict__ kept_row0, int pairs_per_block, int num_rots,
    const float* __restrict__ cos_tab, const float* __restrict__ sin_tab, const float* __restrict__ sphere, int S,
    float cos_thr, int bmm_size, int max_chunks, double* __restrict__ sums /* [B][max_chunks][S] */) {
  __shared__ RotCand s_c[RB_MAX_CAND];
  __shared__ int s_cb;
  const int b = blockIdx.y;
  const int kept = kept_count[b];
  const int j0 = blockIdx.x * pairs_per_block;
  if (j0 >= kept) return;
  const int npairs = min(pairs_per_block, kept - j0);
  const int ncand = npairs * num_rots;
  const int t0 = tup_off[b];
  const float* p = pts + 3 * (int64_t)pt_off[b];
  if (threadIdx.x == 0) s_cb = 0x7fffffff;
  __syncthreads();
  for (int c = threadIdx.x; c < ncand; c += RB_THREADS) {
    const int pj = c / num_rots, r = c - pj * num_rots;
    const int j = j0 + pj;
    const int row0 = kept_row0[t0 + j];
    RotCand rc;
    rc.slot = -1; rc.x = rc.y = rc.z = 0.0f; rc.inv_wt = 0.0;
    if (row0 >= 0) {
      const int64_t row = (int64_t)(t0 + kept_tuple[t0 + j]);
      const PairFrame f = pair_frame(p, idx[row * k], idx[row * k + 1]);
      const float tn = tanf(rot[row * 3 + rot_col]);
      rot_candidate(f, tn, cos_tab[r], sin_tab[r], rc.x, rc.y, rc.z);
      rc.slot = (row0 + r) / bmm_size;
      rc.inv_wt = 1.0 / kept_wt[t0 + j];
      atomicMin(&s_cb, rc.slot);
    }
    s_c[c] = rc;
  }
  __syncthreads();
  const int cb = s_cb;
  if (cb == 0x7fffffff) return;
  double* out = sums + ((int64_t)b * max_chunks) * S;
  for (int s = threadIdx.x; s < S; s += RB_THREADS) {
    const float bx = sphere[3 * s], by = sphere[3 * s + 1], bz = sphere[3 * s + 2];
    double acc0 = 0.0, acc1 = 0.0;
    for (int c = 0; c < ncand; ++c) {
      const RotCand rc = s_c[c];
      if (rc.slot < 0) continue;
      const float d = fmaf(rc.z, bz, fmaf(rc.y, by, rc.x * bx));     // mm, K = 3: fused like sgemm
      const double w = (d > cos_thr) ? rc.inv_wt : 0.0;
      if (rc.slot == cb) acc0 += w; else acc1 += w;
    }
    if (acc0 != 0.0) atomicAdd(&out[(int64_t)cb * S + s], acc0);
    if (acc1 != 0.0) atomicAdd(&out[(int64_t)(cb + 1) * S + s], acc1);
  }
}

// Lookup-table kernel.  The caller tabulates, for every cell of an (equal-area rows in y) x (azimuth) partition of
// the sphere, the bins whose cone can contain a direction of that cell (cppf2_amd.ops.build_bin_lut: bins within
// cone + cell circumradius of the cell centre; <= RL_K per cell, 0.46 on average for the 720 fibonacci bins).
// One thread per candidate axis: cell of the candidate -> one 16-byte table row -> exact cosine test of those few
// bins only.  Works for any bin set; counts are identical to the dense kernel's (tests compare them).
//
// Work decomposition follows the reference's float32 accumulation chunks (eval.py:41-45: rows [c*bmm, (c+1)*bmm) of the
// candidate list are summed in float64, then added to the float32 counts): a workgroup owns `rows_per_block`
// consecutive candidate rows that never straddle a chunk boundary (`sub_blocks` workgroups per chunk), so it has ONE
// float64 accumulator set per voted axis in LDS, and it votes BOTH axes (eval.py:277-293: the up and the right vote
// share the pair frames and differ only in the angle column) from the same per-pair frames.  The accumulators
// leave with plain coalesced stores and rot_bins_fold_kernel adds the sub-block sums of a chunk in a fixed order:
// no global atomics.  Within a workgroup the votes arrive in thread-scheduling order, so the LDS accumulators are 64-bit
// FIXED-POINT sums (integer adds commute: run-to-run identical bits, which a float64 atomic sum is not): the scale is the
// largest power of two that keeps rows_per_block x (largest 1 / weight of the block's pairs) below 2^62, i.e. a resolution of
// ~2^-62 of the largest possible sum -- at least as fine as the float64 rounding of the sums it replaces.
#define RW_THREADS 256
#define RL_K 8             // table slots per cell (int16 bin ids, -1 = empty)
struct RwFrame {
  float xx, xy, xz, yx, yy, yz, ux, uy, uz;   // in-plane axes, pair direction
  float tn[2];                                // tan of the predicted angle to each voted axis
  int row0;                                   // first row of the pair in vote_rotation's compacted candidate list
  double inv_wt;                              // 1 / pair weight; phase 1b overwrites it with its fixed-point image (uint64 bits)
};

template <int NAX>
__global__ __launch_bounds__(RW_THREADS) void rot_bins_lut_kernel(
    const float* __restrict__ pts, const int32_t* __restrict__ pt_off, const int32_t* __restrict__ idx, int k,
    const int32_t* __restrict__ tup_off, const float* __restrict__ rot, int rot_col0, int rot_col1,
    const int32_t* __restrict__ kept_tuple, const int32_t* __restrict__ kept_count,
    const double* __restrict__ kept_wt, const int32_t* __restrict__ kept_row0, int rows_per_block, int sub_blocks,
    int max_pairs, int num_rots, const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
    const float* __restrict__ sphere, int S, float cos_thr, const int4* __restrict__ lut, int lut_rows, int lut_cols,
    int bmm_size, double* __restrict__ partial /* [B][gridDim.x][NAX][S] */) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* s_sph = (float4*)smem;                                     // [S] (x, y, z, -)
  unsigned long long* s_acc = (unsigned long long*)(smem + (size_t)S * 16);   // [NAX][S] fixed-point sums
  float2* s_trig = (float2*)(s_acc + (size_t)NAX * S);               // [num_rots] (cos, sin)
  RwFrame* s_fr = (RwFrame*)(s_trig + num_rots);                     // [max_pairs]
  int* s_list = (int*)(s_fr + max_pairs);                            // [max_pairs] kept-list positions of the block's pairs
  __shared__ int s_n;
  __shared__ unsigned long long s_maxw;      // bits of the largest 1 / weight of the block's pairs (positive doubles order like integers)
  const int b = blockIdx.y;
  const int chunk = blockIdx.x / sub_blocks, sub = blockIdx.x - chunk * sub_blocks;
  const int64_t lo64 = (int64_t)chunk * bmm_size + (int64_t)sub * rows_per_block;
  const int64_t hi64 = min(lo64 + rows_per_block, (int64_t)(chunk + 1) * bmm_size);
  const int kept = kept_count[b];
  const int t0 = tup_off[b];
  double* out = partial + ((int64_t)b * gridDim.x + blockIdx.x) * NAX * S;
  if (threadIdx.x == 0) {
    s_n = 0;
    s_maxw = 0;
  }
  __syncthreads();
  // pairs with a candidate row in [lo, hi): row0 is increasing over the valid kept pairs, -1 for degenerate ones
  if (lo64 < (int64_t)kept * num_rots) {
    const int lo = (int)lo64, hi = (int)min(hi64, (int64_t)kept * num_rots);
    for (int j = threadIdx.x; j < kept; j += RW_THREADS) {
      const int row0 = kept_row0[t0 + j];
      if (row0 >= 0 && row0 < hi && row0 + num_rots > lo) {
        const int pos = atomicAdd(&s_n, 1);
        if (pos < max_pairs) s_list[pos] = j;
      }
    }
  }
  __syncthreads();
  const int npairs = min(s_n, max_pairs);
  if (npairs == 0) {                                                  // chunk beyond this scene's rows
    for (int i = threadIdx.x; i < NAX * S; i += RW_THREADS) out[i] = 0.0;
    return;
  }
  const int lo = (int)lo64, hi = (int)hi64;
  const float* p = pts + 3 * (int64_t)pt_off[b];
  for (int i = threadIdx.x; i < S; i += RW_THREADS)
    s_sph[i] = make_float4(sphere[3 * i], sphere[3 * i + 1], sphere[3 * i + 2], 0.0f);
  for (int i = threadIdx.x; i < NAX * S; i += RW_THREADS) s_acc[i] = 0ull;
  for (int i = threadIdx.x; i < num_rots; i += RW_THREADS) s_trig[i] = make_float2(cos_tab[i], sin_tab[i]);
  // phase 1: one thread per pair -- frame of the pair (train_dino.py:219-232), tan of its angles, weight
  for (int i = threadIdx.x; i < npairs; i += RW_THREADS) {
    const int j = s_list[i];
    const int64_t row = (int64_t)(t0 + kept_tuple[t0 + j]);
    const PairFrame f = pair_frame(p, idx[row * k], idx[row * k + 1]);
    RwFrame fr;
    const float den = fmaxf(f.nco, 1e-7f);
    fr.xx = f.cox / den; fr.xy = f.coy / den; fr.xz = f.coz / den;
    fr.yx = cross_term(fr.xy, f.uz, fr.xz, f.uy);
    fr.yy = cross_term(fr.xz, f.ux, fr.xx, f.uz);
    fr.yz = cross_term(fr.xx, f.uy, fr.xy, f.ux);
    fr.ux = f.ux; fr.uy = f.uy; fr.uz = f.uz;
    fr.tn[0] = tanf(rot[row * 3 + rot_col0]);
    fr.tn[1] = (NAX > 1) ? tanf(rot[row * 3 + rot_col1]) : 0.0f;
    fr.row0 = kept_row0[t0 + j];
    fr.inv_wt = 1.0 / kept_wt[t0 + j];
    s_fr[i] = fr;
    if (fr.inv_wt > 0.0 && fr.inv_wt < 1e300) atomicMax(&s_maxw, (unsigned long long)__double_as_longlong(fr.inv_wt));
  }
  __syncthreads();
  // phase 1b: the block's fixed-point scale 2^e with rows_per_block * max(1 / weight) * 2^e < 2^62, and every pair's addend
  // round(inv_wt * 2^e) (a non-positive / non-finite weight, which the reference would turn into inf / NaN counts, adds 0)
  int fx_e;
  {
    const double bound = (double)rows_per_block * fmax(__longlong_as_double((long long)s_maxw), 1e-300);
    int eb;
    frexp(bound, &eb);                        // bound < 2^eb
    fx_e = 62 - eb;
  }
  for (int i = threadIdx.x; i < npairs; i += RW_THREADS) {
    const double w = s_fr[i].inv_wt;
    const unsigned long long q = (w > 0.0 && w < 1e300) ? (unsigned long long)__double2ll_rn(ldexp(w, fx_e)) : 0ull;
    s_fr[i].inv_wt = __longlong_as_double((long long)q);
  }
  __syncthreads();
  const float row_scale = 0.5f * (float)lut_rows, col_scale = (float)lut_cols * 0.15915494309189535f;
  // phase 2: one thread per candidate offset (pair, rotation); each voted axis' candidate (train_dino.py:233-237)
  const int ncand = npairs * num_rots;
  const int dq = RW_THREADS / num_rots, dr = RW_THREADS - dq * num_rots;
  int pj = (int)threadIdx.x / num_rots, r = (int)threadIdx.x - pj * num_rots;
  for (int c = threadIdx.x; c < ncand; c += RW_THREADS) {
    const RwFrame fr = s_fr[pj];
    const int row = fr.row0 + r;
    const float2 t = s_trig[r];
    pj += dq; r += dr;
    if (r >= num_rots) { r -= num_rots; ++pj; }
    if (row < lo || row >= hi) continue;
    const float cs = t.x, sn = t.y;
    const float offx = cs * fr.xx + sn * fr.yx, offy = cs * fr.xy + sn * fr.yy, offz = cs * fr.xz + sn * fr.yz;
#pragma unroll
    for (int a = 0; a < NAX; ++a) {
      const float tn = fr.tn[a];
      const float sg = (tn > 0.0f) ? 1.0f : -1.0f;
      const float ux = tn * offx + sg * fr.ux, uy = tn * offy + sg * fr.uy, uz = tn * offz + sg * fr.uz;
      const float nn = fmaxf(norm3_fused(ux, uy, uz), 1e-7f);
      const float x = ux / nn, y = uy / nn, z = uz / nn;
      if (!(y == y) || !(x == x) || !(z == z)) continue;               // NaN candidate never passes the test
      // the angle only selects the lookup cell, whose bin list carries 2e-3 rad of slack (ops.build_bin_lut): the
      // polynomial atan2 (1.3e-7 rad) is as good as libm's here at a third of the instructions
      float phi = atan2_poly(z, x);
      phi += (phi < 0.0f) ? 6.2831853071795865f : 0.0f;
      int ci = (int)((1.0f - y) * row_scale), cj = (int)(phi * col_scale);
      ci = min(max(ci, 0), lut_rows - 1);
      cj = min(max(cj, 0), lut_cols - 1);
      const int4 e = lut[ci * lut_cols + cj];
      const int ids[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
      for (int h = 0; h < 4; ++h) {
#pragma unroll
        for (int lo16 = 0; lo16 < 2; ++lo16) {
          const int s = lo16 ? (ids[h] >> 16) : (int)(short)(ids[h] & 0xffff);
          if (s >= 0) {
            const float4 q = s_sph[s];
            const float d = fmaf(z, q.z, fmaf(y, q.y, x * q.x));
            if (d > cos_thr) atomicAdd(&s_acc[a * S + s], (unsigned long long)__double_as_longlong(fr.inv_wt));
          }
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NAX * S; i += RW_THREADS) out[i] = ldexp((double)s_acc[i], -fx_e);
}

// float32 counts of one (scene, axis): per chunk, the float64 sum of its sub-block partials in sub-block order, one
// float32 rounding per chunk (eval.py:45), then first maximum
__global__ __launch_bounds__(1024) void rot_bins_fold_kernel(const double* __restrict__ partial, int nblk,
                                                            int sub_blocks, int nax, int S, int B,
                                                            float* __restrict__ counts, int32_t* __restrict__ top_idx,
                                                            float* __restrict__ top_count) {
  const int b = blockIdx.x, a = blockIdx.y;
  const double* part = partial + ((int64_t)b * nblk * nax + a) * S;
  const int64_t bstride = (int64_t)nax * S;
  float best = -INFINITY;
  int besti = 0x7fffffff;
  for (int s = threadIdx.x; s < S; s += blockDim.x) {
    float c = 0.0f;
    for (int i0 = 0; i0 < nblk; i0 += sub_blocks) {
      double acc = 0.0;
      for (int k0 = 0; k0 < sub_blocks; k0 += 8) {
        // 8 independent loads in flight, then their sum in sub-block order (absent ones add an exact 0.0)
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (k0 + k < sub_blocks) ? part[(i0 + k0 + k) * bstride + s] : 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += v[k];
      }
      c = (float)((double)c + acc);
    }
    counts[((int64_t)a * B + b) * S + s] = c;
    if (c > best || (c == best && s < besti)) { best = c; besti = s; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(besti, off);
    if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
  }
  __shared__ float s_b[16];
  __shared__ int s_i[16];
  if (wave_lane() == 0) { s_b[threadIdx.x >> 6] = best; s_i[threadIdx.x >> 6] = besti; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
      if (s_b[w] > best || (s_b[w] == best && s_i[w] < besti)) { best = s_b[w]; besti = s_i[w]; }
    if (besti == 0x7fffffff) besti = 0;
    if (top_idx) top_idx[(int64_t)a * B + b] = besti;
    if (top_count) top_count[(int64_t)a * B + b] = best;
  }
}

// counts (float32) = fold of the per-chunk float64 sums, then first maximum
__global__ __launch_bounds__(256) void rot_bins_final_kernel(const double* __restrict__ sums, int S, int max_chunks,
                                                             float* __restrict__ counts, int32_t* __restrict__ top_idx,
                                                             float* __restrict__ top_count) {
  const int b = blockIdx.x;
  const double* in = sums + ((int64_t)b * max_chunks) * S;
  float best = -INFINITY;
  int besti = 0x7fffffff;
  for (int s = threadIdx.x; s < S; s += blockDim.x) {
    float c = 0.0f;
    for (int ch = 0; ch < max_chunks; ++ch) c = (float)((double)c + in[(int64_t)ch * S + s]);
    counts[(int64_t)b * S + s] = c;
    if (c > best || (c == best && s < besti)) { best = c; besti = s; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(besti, off);
    if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
  }
  __shared__ float s_b[4];
  __shared__ int s_i[4];
  if (wave_lane() == 0) { s_b[threadIdx.x >> 6] = best; s_i[threadIdx.x >> 6] = besti; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      if (s_b[w] > best || (s_b[w] == best && s_i[w] < besti)) { best = s_b[w]; besti = s_i[w]; }
    if (besti == 0x7fffffff) besti = 0;
    if (top_idx) top_idx[b] = besti;
    if (top_count) top_count[b] = best;
  }
}

// Byte sizes of the workspace, one path at a time (a call uses one).  sums: the dense path's float64 sums [B][max_chunks][S],
// which it clears; dense: the same, padded.  lut: the lookup-table path's partials [B][nblk][2][S] -- two axes' worth whichever
// entry point asks, so that one workspace serves cppf_rot_bins and cppf_rot_bins2.
struct RbLayout {
  int64_t sums, dense, lut, bytes;
};

// Every launch decision of one call, taken before any launch.  lut: the lookup-table path (the caller gave a table, the kernel's
// LDS fits and there are rows to vote), else the dense one.  Lookup-table path: chunks of bmm_size rows, each cut into `sub`
// workgroups of `rpb` rows (about 160 pairs' worth for throughput-sized batches, 32 for small ones so that a single scene still
// fills the chip), nblk workgroups per scene with max_pairs frames and lut_lds bytes of dynamic LDS each; fold_threads: one bin
// per thread when they fit.  Dense path: max_chunks slots of sums per scene, ppb pairs per workgroup (a block's rows span at most
// two chunks), dense_blocks workgroups per scene -- none without kept pairs, or where num_rots > bmm_size (ppb = 0), which
// rot_bins_impl rejects.
struct RbPlan {
  bool lut;
  int nchunks, sub, rpb, nblk, max_pairs, fold_threads;
  int max_chunks, ppb, dense_blocks;
  size_t lut_lds;
  RbLayout L;
};

static RbPlan rb_plan(int nax, int B, int S, int max_kept, int num_rots, int bmm_size, bool have_lut) {
  RbPlan p;
  // lookup-table path
  const int64_t rows = (int64_t)(max_kept > 0 ? max_kept : 1) * num_rots;
  p.nchunks = (int)((rows + bmm_size - 1) / bmm_size);
  const int64_t target = (int64_t)(B >= 16 ? 160 : 32) * num_rots;
  p.sub = (target >= bmm_size) ? 1 : (int)((bmm_size + target - 1) / target);
  p.rpb = (bmm_size + p.sub - 1) / p.sub;
  p.nblk = p.nchunks * p.sub;
  p.max_pairs = p.rpb / num_rots + 2;
  p.fold_threads = S >= 1024 ? 1024 : ((S + 63) / 64) * 64;
  // the kernel's sphere, accumulators, rotation table and frames; within the default 64 KiB dynamic-LDS limit, so nothing is
  // declared to the runtime (no minimum is requested either: cppf2_amd/build.py, the packed-float32 erratum)
  p.lut_lds = (size_t)S * 16 + (size_t)nax * S * 8 + (size_t)num_rots * 8 + (size_t)p.max_pairs * (sizeof(RwFrame) + 4);
  p.lut = have_lut && p.lut_lds <= 64000 && max_kept > 0;
  // dense path
  p.max_chunks = (int)(((int64_t)max_kept * num_rots + bmm_size - 1) / bmm_size) + 1;
  p.ppb = std::max(std::min(RB_MAX_CAND / num_rots, 4), 1);
  if ((int64_t)p.ppb * num_rots > bmm_size) p.ppb = bmm_size / num_rots;
  p.dense_blocks = (max_kept > 0 && p.ppb > 0) ? (max_kept + p.ppb - 1) / p.ppb : 0;
  p.L.sums = (int64_t)B * p.max_chunks * S * 8;
  p.L.dense = align_up(p.L.sums, 256);
  p.L.lut = align_up((int64_t)B * p.nblk * 2 * S * 8, 256);
  p.L.bytes = std::max(p.L.dense, p.L.lut);
  return p;
}

extern "C" int64_t cppf_rot_bins_workspace_bytes(int B, int S, int max_kept, int num_rots, int bmm_size) {
  if (B <= 0 || S <= 0 || max_kept < 0 || num_rots <= 0 || bmm_size <= 0) return 0;
  return rb_plan(2, B, S, max_kept, num_rots, bmm_size, true).L.bytes;
}

// nax = 1: counts [B,S], top_* [B];  nax = 2: counts [2,B,S], top_* [2,B] (axis-major)
static int rot_bins_impl(int nax, int B, const float* pts, const int32_t* pt_off, const int32_t* idx, int k,
                         const int32_t* tup_off, const float* rot, int rot_col0, int rot_col1,
                         const int32_t* kept_tuple, const int32_t* kept_count, const double* kept_wt,
                         const int32_t* kept_row0, int max_kept, int num_rots, const float* cos_tab,
                         const float* sin_tab, const float* sphere, int S, float cos_thr, int bmm_size,
                         const int16_t* bin_lut, int lut_rows, int lut_cols, float* counts, int32_t* top_idx,
                         float* top_count, void* workspace, int64_t workspace_bytes, void* stream) {
  CPPF_CHECK_ARG(B > 0 && pts && pt_off && idx && tup_off && rot && kept_tuple && kept_count && kept_wt && kept_row0);
  CPPF_CHECK_ARG(cos_tab && sin_tab && sphere && counts);
  CPPF_CHECK_ARG(rot_col0 >= 0 && rot_col0 < 3 && rot_col1 >= 0 && rot_col1 < 3);
  CPPF_CHECK_ARG(S > 0 && num_rots > 0 && num_rots <= RB_MAX_CAND && bmm_size > 0);
  CPPF_CHECK_ARG(bin_lut == nullptr || (lut_rows > 0 && lut_cols > 0 && S <= 32767));
  CPPF_CHECK_ARG((int64_t)max_kept * num_rots < 0x7fffffffLL);
  CPPF_CHECK_ARG(workspace && workspace_bytes >= cppf_rot_bins_workspace_bytes(B, S, max_kept, num_rots, bmm_size));
  if (num_rots > bmm_size) {
    snprintf(g_cppf_err, sizeof(g_cppf_err), "cppf_rot_bins: bmm_size %d < num_rots %d unsupported", bmm_size, num_rots);
    return CPPF_EUNSUPPORTED;
  }
  const RbPlan p = rb_plan(nax, B, S, max_kept, num_rots, bmm_size, bin_lut != nullptr);
  hipStream_t st = (hipStream_t)stream;
  double* ws = (double*)workspace;
  if (p.lut) {
    const auto lut_kernel = nax == 2 ? rot_bins_lut_kernel<2> : rot_bins_lut_kernel<1>;
    hipLaunchKernelGGL(lut_kernel, dim3(p.nblk, B), dim3(RW_THREADS), p.lut_lds, st, pts, pt_off, idx, k, tup_off, rot, rot_col0,
                       rot_col1, kept_tuple, kept_count, kept_wt, kept_row0, p.rpb, p.sub, p.max_pairs, num_rots, cos_tab, sin_tab,
                       sphere, S, cos_thr, (const int4*)bin_lut, lut_rows, lut_cols, bmm_size, ws);
    CPPF_LAUNCH_CHECK();
    hipLaunchKernelGGL(rot_bins_fold_kernel, dim3(B, nax), dim3(p.fold_threads), 0, st, ws, p.nblk, p.sub, nax, S, B, counts,
                       top_idx, top_count);
    CPPF_LAUNCH_CHECK();
    return CPPF_OK;
  }
  // dense path: one axis at a time through the same sums
  for (int a = 0; a < nax; ++a) {
    CPPF_HIP(hipMemsetAsync(ws, 0, (size_t)p.L.sums, st));
    if (p.dense_blocks > 0) {
      hipLaunchKernelGGL(rot_bins_dense_kernel, dim3(p.dense_blocks, B), dim3(RB_THREADS), 0, st, pts, pt_off, idx, k, tup_off, rot,
                         a ? rot_col1 : rot_col0, kept_tuple, kept_count, kept_wt, kept_row0, p.ppb, num_rots, cos_tab, sin_tab,
                         sphere, S, cos_thr, bmm_size, p.max_chunks, ws);
      CPPF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(rot_bins_final_kernel, dim3(B), dim3(256), 0, st, ws, S, p.max_chunks, counts + (int64_t)a * B * S,
                       top_idx ? top_idx + (int64_t)a * B : nullptr, top_count ? top_count + (int64_t)a * B : nullptr);
    CPPF_LAUNCH_CHECK();
  }
  return CPPF_OK;
}

extern "C" int cppf_rot_bins(int B, const float* pts, const int32_t* pt_off, const int32_t* idx, int k,
                             const int32_t* tup_off, const float* rot, int rot_col, const int32_t* kept_tuple,
                             const int32_t* kept_count, const double* kept_wt, const int32_t* kept_row0, int max_kept,
                             int num_rots, const float* cos_tab, const float* sin_tab, const float* sphere, int S,
                             float cos_thr, int bmm_size, const int16_t* bin_lut, int lut_rows, int lut_cols,
                             float* counts, int32_t* top_idx, float* top_count, void* workspace,
                             int64_t workspace_bytes, void* stream) {
  return rot_bins_impl(1, B, pts, pt_off, idx, k, tup_off, rot, rot_col, rot_col, kept_tuple, kept_count, kept_wt,
                       kept_row0, max_kept, num_rots, cos_tab, sin_tab, sphere, S, cos_thr, bmm_size, bin_lut, lut_rows,
                       lut_cols, counts, top_idx, top_count, workspace, workspace_bytes, stream);
}

extern "C" int cppf_rot_bins2(int B, const float* pts, const int32_t* pt_off, const int32_t* idx, int k,
                              const int32_t* tup_off, const float* rot, int rot_col0, int rot_col1,
                              const int32_t* kept_tuple, const int32_t* kept_count, const double* kept_wt,
                              const int32_t* kept_row0, int max_kept, int num_rots, const float* cos_tab,
                              const float* sin_tab, const float* sphere, int S, float cos_thr, int bmm_size,
                              const int16_t* bin_lut, int lut_rows, int lut_cols, float* counts, int32_t* top_idx,
                              float* top_count, void* workspace, int64_t workspace_bytes, void* stream) {
  return rot_bins_impl(2, B, pts, pt_off, idx, k, tup_off, rot, rot_col0, rot_col1, kept_tuple, kept_count, kept_wt,
                       kept_row0, max_kept, num_rots, cos_tab, sin_tab, sphere, S, cos_thr, bmm_size, bin_lut, lut_rows,
                       lut_cols, counts, top_idx, top_count, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------------------------
// Stand-alone halves with the reference's signatures
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void vr_scan_kernel(const float* __restrict__ pts, const int32_t* __restrict__ idx,
                                                       int k, int T, uint8_t* __restrict__ valid,
                                                       int32_t* __restrict__ rank, int32_t* __restrict__ n_valid) {
  __shared__ int s_wave[BV_THREADS / 64];
  int base_rank = 0;
  for (int base = 0; base < T; base += BV_THREADS) {
    const int t = base + threadIdx.x;
    bool v = false;
    if (t < T) {
      const int i0 = idx[(int64_t)t * k], i1 = idx[(int64_t)t * k + 1];
      v = norm3_fused(pts[3 * i0] - pts[3 * i1], pts[3 * i0 + 1] - pts[3 * i1 + 1],
                      pts[3 * i0 + 2] - pts[3 * i1 + 2]) > 1e-7f;
      valid[t] = v ? 1 : 0;
    }
    int tot;
    const int pos = block_scan_flag(v, s_wave, &tot);
    if (t < T) rank[t] = v ? base_rank + pos : -1;
    base_rank += tot;
  }
  if (threadIdx.x == 0) *n_valid = base_rank;
}

__global__ __launch_bounds__(256) void vr_emit_kernel(const float* __restrict__ pts, const int32_t* __restrict__ idx,
                                                      int k, int T, const float* __restrict__ angle, int num_rots,
                                                      const float* __restrict__ cos_tab,
                                                      const float* __restrict__ sin_tab,
                                                      const int32_t* __restrict__ rank, float* __restrict__ up) {
  const int64_t total = (int64_t)T * num_rots;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(c / num_rots), r = (int)(c - (int64_t)t * num_rots);
    const int rk = rank[t];
    if (rk < 0) continue;
    const PairFrame f = pair_frame(pts, idx[(int64_t)t * k], idx[(int64_t)t * k + 1]);
    float x, y, z;
    rot_candidate(f, tanf(angle[t]), cos_tab[r], sin_tab[r], x, y, z);
    float* o = up + ((int64_t)rk * num_rots + r) * 3;
    o[0] = x; o[1] = y; o[2] = z;
  }
}

extern "C" int cppf_vote_rotation(const float* pts, int n_points, const int32_t* idx, int k, int T,
                                  const float* rot_angle, int num_rots, const float* cos_tab, const float* sin_tab,
                                  float* up, uint8_t* valid, int32_t* n_valid, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  CPPF_CHECK_ARG(pts && cos_tab && sin_tab && up && valid && n_valid && workspace);
  CPPF_CHECK_ARG(n_points > 0 && k >= 2 && T >= 0 && num_rots > 0 && workspace_bytes >= (int64_t)T * 4);
  CPPF_CHECK_ARG(T == 0 || (idx && rot_angle));      // empty inputs have no address (an empty torch tensor's is NULL)
  hipStream_t st = (hipStream_t)stream;
  int32_t* rank = (int32_t*)workspace;
  hipLaunchKernelGGL(vr_scan_kernel, dim3(1), dim3(BV_THREADS), 0, st, pts, idx, k, T, valid, rank, n_valid);
  CPPF_LAUNCH_CHECK();
  if (T > 0) {
    const int64_t blocks = ((int64_t)T * num_rots + 255) / 256;
    hipLaunchKernelGGL(vr_emit_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, st, pts, idx, k,
                       T, rot_angle, num_rots, cos_tab, sin_tab, rank, up);
    CPPF_LAUNCH_CHECK();
  }
  return CPPF_OK;
}

// get_topk_dir on explicit candidates: thread = sphere bin, rows of a chunk split over SC_SPLIT workgroups
#define SC_ROWS 512
__global__ __launch_bounds__(256) void sphere_counts_kernel(const float* __restrict__ cand, int64_t M,
                                                            const double* __restrict__ wt,
                                                            const float* __restrict__ sphere, int S, float cos_thr,
                                                            int bmm_size, int blocks_per_chunk,
                                                            double* __restrict__ sums) {
  __shared__ float s_x[SC_ROWS], s_y[SC_ROWS], s_z[SC_ROWS];
  __shared__ double s_w[SC_ROWS];
  const int chunk = blockIdx.x / blocks_per_chunk, sub = blockIdx.x - chunk * blocks_per_chunk;
  const int64_t c_lo = (int64_t)chunk * bmm_size;
  const int64_t c_hi = (c_lo + bmm_size < M) ? c_lo + bmm_size : M;
  const int64_t lo = c_lo + (int64_t)sub * SC_ROWS;
  if (lo >= c_hi) return;
  const int n = (int)((c_hi - lo < SC_ROWS) ? c_hi - lo : SC_ROWS);
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    s_x[i] = cand[(lo + i) * 3]; s_y[i] = cand[(lo + i) * 3 + 1]; s_z[i] = cand[(lo + i) * 3 + 2];
    s_w[i] = wt ? 1.0 / wt[lo + i] : 1.0;
  }
  __syncthreads();
  for (int s = threadIdx.x; s < S; s += blockDim.x) {
    const float bx = sphere[3 * s], by = sphere[3 * s + 1], bz = sphere[3 * s + 2];
    double acc = 0.0;
    for (int i = 0; i < n; ++i) {
      const float d = fmaf(s_z[i], bz, fmaf(s_y[i], by, s_x[i] * bx));
      acc += (d > cos_thr) ? s_w[i] : 0.0;
    }
    if (acc != 0.0) atomicAdd(&sums[(int64_t)chunk * S + s], acc);
  }
}

extern "C" int cppf_sphere_counts(const float* cand, int64_t M, const double* wt, const float* sphere, int S,
                                  float cos_thr, int bmm_size, float* counts, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  CPPF_CHECK_ARG(sphere && counts && workspace && S > 0 && bmm_size > 0 && M >= 0);
  CPPF_CHECK_ARG(M == 0 || cand);                    // no candidates: zero counts
  const int nchunks = (int)((M + bmm_size - 1) / bmm_size);
  const int mc = nchunks > 0 ? nchunks : 1;
  CPPF_CHECK_ARG(workspace_bytes >= (int64_t)mc * S * 8);
  hipStream_t st = (hipStream_t)stream;
  double* sums = (double*)workspace;
  CPPF_HIP(hipMemsetAsync(sums, 0, (size_t)mc * S * 8, st));
  if (M > 0) {
    const int bpc = (bmm_size + SC_ROWS - 1) / SC_ROWS;
    hipLaunchKernelGGL(sphere_counts_kernel, dim3(nchunks * bpc), dim3(256), 0, st, cand, M, wt, sphere, S, cos_thr,
                       bmm_size, bpc, sums);
    CPPF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(rot_bins_final_kernel, dim3(1), dim3(256), 0, st, sums, S, mc, counts, (int32_t*)nullptr,
                     (float*)nullptr);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
