// Pose-hypothesis verification (render and compare; not in the reference): several well-separated peaks of each rotation-bin
// vote become pose hypotheses, and each hypothesis' render is counted against the observed depth.  cppf2_amd/verify.py drives
// both entry points; tests/verify_ref.py restates them.  gfx950 only.
//
// cppf_pose_hypotheses: one launch, grid B, 256 threads; workgroup b reads its two count rows once per peak.
//   Peaks of one row (float32 counts[S]), k = 0 .. K-1:
//     peak 0 = the first maximum: larger count first, lower index on ties, index 0 when no count compares (rot_bins_final_kernel's
//       rule, so peak 0 is the pass' top_idx and its count the pass' top count);
//     peak k = the first maximum, by the same rule, over the bins s with count > 0 that are no earlier peak q and that no earlier
//       peak suppresses: ((x_s*x_q + y_s*y_q) + z_s*z_q) >= cos_sep in float32 (the sphere's unit vectors).  No such bin: the row
//       has k peaks.  Antipodal bins are never suppressed by each other (cos_sep > -1).  y_only: the right row keeps peak 0 only.
//   Combinations c = i * n_right + j of up peak i and right peak j: (0, 0) always, every other one with
//     |(u_x*r_x + u_y*r_y) + u_z*r_z| <= cos_perp (float32).  Key = (double)up_count[i] * (double)right_count[j] (exact; NaN
//     counts as -inf); (0, 0) goes to slot 0 (its key is the largest), the others follow in descending key, ties by ascending c;
//     the first H are kept.  Slot record = the base record (t, scale, argmax, peak, kept, ncell, flags, pad_) with up_idx,
//     right_idx, up_count, right_count of the combination and R = pose_from_bins (cppf_common.h, the Gram-Schmidt of
//     assemble_pose_kernel): slot 0 is the base record, byte for byte, when the base is cppf_assemble_pose's.  Slots past the
//     kept combinations: the base record with flags |= 1 (empty), up_idx = right_idx = -1, up_count = right_count = 0.
//
// cppf_depth_fit_counts: one launch per FIT_IMGS images after a clear of the output, grid (ceil(H*W / FIT_PIX), images),
//   256 threads; block (x, i) loads its FIT_PIX pixels of observed image i (depth and mask) into registers once and then walks
//   the hypotheses hyp_off[i] .. hyp_off[i+1]-1 of that image, reading each render's pixels once.  Each wavefront counts with
//   ballots (lane k keeps count k), the 4 wavefronts meet in LDS, and each block adds its non-zero sums with 64-bit integer
//   atomics: integer sums, so the counts do not depend on the grid, the batch or the order.  Per pixel, d_o the observed depth,
//   m its mask byte != 0, d_h the render (0 = nothing drawn), diff = (double)d_o - (double)d_h, tau_k = (double)taus[k]:
//     drawn       = d_h > 0
//     observed    = m && d_o > 0
//     violations  = d_h > 0 && d_o > 0 && diff > tau_0                 (any pixel, masked or not)
//     unexplained = m && d_o > 0 && d_h == 0
//     fit_k       = m && d_o > 0 && d_h > 0 && |diff| <= tau_k
//   (comparisons with 0 in float32; the build's -ffp-contract=off keeps every operation where it is written.)
#include "cppf_common.h"

#define HYP_THREADS 256
#define HYP_MAX_K 32
#define HYP_MAX_H (HYP_MAX_K * HYP_MAX_K)
#define HYP_EMPTY 1              // CppfSceneResult.flags bit0: no hypothesis in this slot

#define FIT_THREADS 256
#define FIT_PPT 8                // pixels per thread
#define FIT_PIX (FIT_THREADS * FIT_PPT)
#define FIT_MAX_TAUS 32
#define FIT_IMGS 128             // images per launch (their hypothesis offsets go by value)
#define FIT_MAX_DIM 8192         // H, W (the renderer's limit): H * W fits int32
#define FIT_MAX_P (1 << 24)

__device__ __forceinline__ bool hyp_better(float c, int s, float best, int besti) {
  return c > best || (c == best && s < besti);
}

// The first maximum of the block's candidates (best, besti) -> thread 0 (rot_bins_final_kernel's reduction)
__device__ __forceinline__ void hyp_block_argmax(float& best, int& besti, float* s_b, int* s_i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off);
    const int oi = __shfl_xor(besti, off);
    if (hyp_better(ob, oi, best, besti)) { best = ob; besti = oi; }
  }
  if (wave_lane() == 0) { s_b[threadIdx.x >> 6] = best; s_i[threadIdx.x >> 6] = besti; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < HYP_THREADS / CPPF_WAVE; ++w)
      if (hyp_better(s_b[w], s_i[w], best, besti)) { best = s_b[w]; besti = s_i[w]; }
}

__global__ __launch_bounds__(HYP_THREADS) void pose_hypotheses_kernel(int S, const float* __restrict__ counts_up,
                                                                      const float* __restrict__ counts_right,
                                                                      const float* __restrict__ sphere, int K, float cos_sep,
                                                                      float cos_perp, int up_axis, int right_axis, int y_only,
                                                                      const CppfSceneResult* __restrict__ base, int H,
                                                                      CppfSceneResult* __restrict__ out,
                                                                      int32_t* __restrict__ peak_idx,
                                                                      float* __restrict__ peak_count) {
  __shared__ int s_pi[2][HYP_MAX_K];
  __shared__ float s_pc[2][HYP_MAX_K];
  __shared__ float s_pv[2][HYP_MAX_K][3];
  __shared__ int s_np[2];
  __shared__ float s_b[HYP_THREADS / CPPF_WAVE];
  __shared__ int s_i[HYP_THREADS / CPPF_WAVE];
  __shared__ double s_key[HYP_MAX_H];
  __shared__ int s_code[HYP_MAX_H];
  __shared__ int s_nvalid;
  const int b = blockIdx.x;
  for (int ax = 0; ax < 2; ++ax) {
    const float* row = (ax == 0 ? counts_up : counts_right) + (int64_t)b * S;
    const int kmax = (ax == 1 && y_only) ? 1 : K;
    int k = 0;
    for (; k < kmax; ++k) {
      float best = -INFINITY;
      int besti = 0x7fffffff;
      for (int s = threadIdx.x; s < S; s += HYP_THREADS) {
        const float c = row[s];
        bool ok = true;
        if (k > 0) {
          ok = c > 0.0f;
          const float x = sphere[3 * s], y = sphere[3 * s + 1], z = sphere[3 * s + 2];
          for (int q = 0; q < k && ok; ++q) {
            const float d = (x * s_pv[ax][q][0] + y * s_pv[ax][q][1]) + z * s_pv[ax][q][2];
            ok = s != s_pi[ax][q] && !(d >= cos_sep);
          }
        }
        if (ok && hyp_better(c, s, best, besti)) { best = c; besti = s; }
      }
      hyp_block_argmax(best, besti, s_b, s_i);
      if (threadIdx.x == 0) {
        const bool found = k == 0 || besti != 0x7fffffff;
        if (k == 0 && besti == 0x7fffffff) besti = 0;
        if (found) {
          s_pi[ax][k] = besti;
          s_pc[ax][k] = best;
          s_pv[ax][k][0] = sphere[3 * besti]; s_pv[ax][k][1] = sphere[3 * besti + 1]; s_pv[ax][k][2] = sphere[3 * besti + 2];
        }
        s_np[ax] = found ? k + 1 : k;
      }
      __syncthreads();
      if (s_np[ax] == k) break;                   // no further peak (the same value for every thread)
    }
    if (peak_idx || peak_count) {
      const int n = s_np[ax];
      for (int q = threadIdx.x; q < K; q += HYP_THREADS) {
        const int64_t o = ((int64_t)b * 2 + ax) * K + q;
        if (peak_idx) peak_idx[o] = q < n ? s_pi[ax][q] : -1;
        if (peak_count) peak_count[o] = q < n ? s_pc[ax][q] : 0.0f;
      }
    }
  }
  // combinations: validity and key, then each valid one's rank by counting the valid ones before it
  const int nu = s_np[0], nr = s_np[1], nc = nu * nr;
  if (threadIdx.x == 0) s_nvalid = 0;
  __syncthreads();
  for (int c = threadIdx.x; c < nc; c += HYP_THREADS) {
    const int i = c / nr, j = c - i * nr;
    const float d = (s_pv[0][i][0] * s_pv[1][j][0] + s_pv[0][i][1] * s_pv[1][j][1]) + s_pv[0][i][2] * s_pv[1][j][2];
    const bool valid = c == 0 || fabsf(d) <= cos_perp;
    double key = (double)s_pc[0][i] * (double)s_pc[1][j];
    key = key == key ? key : -INFINITY;
    s_key[c] = valid ? key : NAN;                  // NaN marks a dropped combination
    if (valid) atomicAdd(&s_nvalid, 1);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nc; c += HYP_THREADS) {
    const double key = s_key[c];
    if (key != key) continue;
    int rank = 0;
    if (c != 0) {
      rank = 1;
      for (int c2 = 1; c2 < nc; ++c2) {
        const double k2 = s_key[c2];
        rank += (k2 > key || (k2 == key && c2 < c)) ? 1 : 0;      // NaN (dropped) compares false
      }
    }
    if (rank < H) s_code[rank] = c;
  }
  __syncthreads();
  const int nvalid = s_nvalid < H ? s_nvalid : H;
  const CppfSceneResult* bs = base + b;
  for (int h = threadIdx.x; h < H; h += HYP_THREADS) {
    CppfSceneResult r = *bs;
    if (h < nvalid) {
      const int c = s_code[h], i = c / nr, j = c - i * nr;
      r.up_idx = s_pi[0][i]; r.right_idx = s_pi[1][j];
      r.up_count = s_pc[0][i]; r.right_count = s_pc[1][j];
      pose_from_bins(sphere, r.up_idx, r.right_idx, up_axis, right_axis, r.R);
    } else {
      r.flags |= HYP_EMPTY;
      r.up_idx = r.right_idx = -1;
      r.up_count = r.right_count = 0.0f;
    }
    out[(int64_t)b * H + h] = r;
  }
}

struct FitImages {
  int32_t off[FIT_IMGS + 1];     // global hypothesis offsets of the launch's images
};

__global__ __launch_bounds__(FIT_THREADS) void depth_fit_counts_kernel(const float* __restrict__ depth,
                                                                       const uint8_t* __restrict__ mask, FitImages img, int HW,
                                                                       const float* __restrict__ renders,
                                                                       const float* __restrict__ taus, int n_taus,
                                                                       unsigned long long* __restrict__ counts) {
  __shared__ double s_tau[FIT_MAX_TAUS];
  __shared__ uint32_t s_c[2][FIT_THREADS / CPPF_WAVE][FIT_MAX_TAUS + 4];
  const int i = blockIdx.y;
  const int p0 = img.off[i], p1 = img.off[i + 1];
  if (p0 == p1) return;                                 // the same for the whole block
  if (threadIdx.x < n_taus) s_tau[threadIdx.x] = (double)taus[threadIdx.x];
  const int px0 = blockIdx.x * FIT_PIX + threadIdx.x;
  float dob[FIT_PPT];
  uint32_t seen = 0, obs = 0;                           // bit j: pixel j of this thread has d_o > 0 / and its mask set
#pragma unroll
  for (int j = 0; j < FIT_PPT; ++j) {
    const int px = px0 + j * FIT_THREADS;
    dob[j] = 0.0f;
    if (px < HW) {
      const float d = depth[(int64_t)i * HW + px];
      const bool m = mask[(int64_t)i * HW + px] != 0;
      dob[j] = d;
      seen |= (d > 0.0f ? 1u : 0u) << j;
      obs |= (d > 0.0f && m ? 1u : 0u) << j;
    }
  }
  __syncthreads();
  const int nc = 4 + n_taus;
  const int lane = wave_lane(), w = threadIdx.x / CPPF_WAVE;
  for (int p = p0; p < p1; ++p) {
    const int par = (p - p0) & 1;
    const float* dh = renders + (int64_t)p * HW;
    uint32_t mine = 0;                                  // lane k: count k of this wavefront
#pragma unroll
    for (int j = 0; j < FIT_PPT; ++j) {
      const int px = px0 + j * FIT_THREADS;
      const float h = px < HW ? dh[px] : 0.0f;
      const bool sn = (seen >> j) & 1u, ob = (obs >> j) & 1u;
      const double diff = (double)dob[j] - (double)h;
      const bool drawn = h > 0.0f;
      const uint32_t n_drawn = (uint32_t)__popcll(wave_ballot(drawn));
      const uint32_t n_obs = (uint32_t)__popcll(wave_ballot(ob));
      const uint32_t n_viol = (uint32_t)__popcll(wave_ballot(drawn && sn && diff > s_tau[0]));
      const uint32_t n_unex = (uint32_t)__popcll(wave_ballot(ob && h == 0.0f));
      mine += lane == 0 ? n_drawn : (lane == 1 ? n_obs : (lane == 2 ? n_viol : (lane == 3 ? n_unex : 0u)));
      const bool both = ob && drawn;
      const double ad = fabs(diff);
      for (int k = 0; k < n_taus; ++k) {
        const uint32_t nk = (uint32_t)__popcll(wave_ballot(both && ad <= s_tau[k]));
        mine += lane == 4 + k ? nk : 0u;
      }
    }
    if (lane < nc) s_c[par][w][lane] = mine;
    __syncthreads();                                    // (the buffer written next is the other one)
    if (threadIdx.x < nc) {
      unsigned long long s = 0;
#pragma unroll
      for (int k = 0; k < FIT_THREADS / CPPF_WAVE; ++k) s += s_c[par][k][threadIdx.x];
      if (s) atomicAdd(&counts[(int64_t)p * nc + threadIdx.x], s);
    }
  }
}

extern "C" int cppf_pose_hypotheses(int B, int S, const float* counts_up, const float* counts_right, const float* sphere, int K,
                                    float cos_sep, float cos_perp, int up_axis, int right_axis, int y_only,
                                    const CppfSceneResult* base, int H, CppfSceneResult* out, int32_t* peak_idx,
                                    float* peak_count, void* stream) {
  CPPF_CHECK_ARG(B >= 0 && S >= 1);
  CPPF_CHECK_ARG(K >= 1 && K <= HYP_MAX_K && H >= 1 && H <= HYP_MAX_H);
  CPPF_CHECK_ARG(cos_sep >= -1.0f && cos_sep <= 1.0f && cos_perp >= 0.0f && cos_perp <= 1.0f);
  CPPF_CHECK_ARG(up_axis >= 0 && up_axis < 3 && right_axis >= 0 && right_axis < 3 && up_axis != right_axis);
  if (B == 0) return CPPF_OK;
  CPPF_CHECK_ARG(counts_up && counts_right && sphere && base && out);
  hipLaunchKernelGGL(pose_hypotheses_kernel, dim3(B), dim3(HYP_THREADS), 0, (hipStream_t)stream, S, counts_up, counts_right,
                     sphere, K, cos_sep, cos_perp, up_axis, right_axis, y_only ? 1 : 0, base, H, out, peak_idx, peak_count);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}

extern "C" int cppf_depth_fit_counts(int I, int H, int W, const float* depth, const uint8_t* mask, const int32_t* h_hyp_off,
                                     int P, const float* renders, const float* taus, int n_taus, int64_t* counts,
                                     void* stream) {
  CPPF_CHECK_ARG(I >= 1 && H >= 1 && W >= 1 && H <= FIT_MAX_DIM && W <= FIT_MAX_DIM);
  CPPF_CHECK_ARG(n_taus >= 1 && n_taus <= FIT_MAX_TAUS);
  CPPF_CHECK_ARG(P >= 0 && P <= FIT_MAX_P && h_hyp_off);
  CPPF_CHECK_ARG(h_hyp_off[0] == 0 && h_hyp_off[I] == P);
  for (int i = 0; i < I; ++i) CPPF_CHECK_ARG(h_hyp_off[i] <= h_hyp_off[i + 1]);
  if (P == 0) return CPPF_OK;
  CPPF_CHECK_ARG(depth && mask && renders && taus && counts);
  hipStream_t st = (hipStream_t)stream;
  CPPF_HIP(hipMemsetAsync(counts, 0, (size_t)P * (4 + n_taus) * sizeof(int64_t), st));
  const int HW = H * W;
  const int nbx = (HW + FIT_PIX - 1) / FIT_PIX;
  for (int i0 = 0; i0 < I; i0 += FIT_IMGS) {
    const int n = I - i0 < FIT_IMGS ? I - i0 : FIT_IMGS;
    if (h_hyp_off[i0] == h_hyp_off[i0 + n]) continue;  // no hypothesis on these images
    FitImages img;
    for (int i = 0; i <= n; ++i) img.off[i] = h_hyp_off[i0 + i];
    hipLaunchKernelGGL(depth_fit_counts_kernel, dim3(nbx, n), dim3(FIT_THREADS), 0, st, depth + (int64_t)i0 * HW,
                       mask + (int64_t)i0 * HW, img, HW, renders, taus, n_taus, (unsigned long long*)counts);
    CPPF_LAUNCH_CHECK();
  }
  return CPPF_OK;
}
