// Scene explanation (global hypothesis verification; not in the reference): of all verified candidate poses of a depth image,
// the subset that together explains the observed depth, every observed pixel counted once, chosen greedily.
// cppf2_amd/scene.py drives the entry point; tests/scene_ref.py restates it.  Integer counts and integer maxima only, so an
// image's outputs do not depend on the grid, the batch or the order.  gfx950 only.
//
// Per pixel, cppf_depth_fit_counts' predicates (cppf_verify.hip) with one tau: d_o the observed depth, m its region byte != 0,
// d_c candidate c's render (0 = nothing drawn), diff = (double)d_o - (double)d_c, tau_d = (double)tau:
//     drawn_c = d_c > 0
//     fit_c   = m && d_o > 0 && d_c > 0 && |diff| <= tau_d
//     viol_c  = d_c > 0 && d_o > 0 && diff > tau_d                            (any pixel, in the region or not)
//   (comparisons with 0 in float32; NaN compares false everywhere, -0.0 is not > 0, +inf is.)
//   stat[p] = (drawn, fit, violations) of render p = cand_off[i] + c: the columns 0, 4 and 2 of cppf_depth_fit_counts.
// Greedy rounds k = 0 .. M-1 of image i, every pixel unexplained at first:
//     gain_c = unexplained pixels with fit_c;  net_c = (int64)gain_c - viol_weight * violations_c
//     eligible: net_c >= min_gain (>= 1), so only a positive net ever reaches the key below, and net_c <= H * W < 2^31
//     winner = the maximum of (uint64)net_c << 32 | (0xFFFFFFFF - c): the largest net, ties to the lowest candidate
//              (cppf_grid_peaks' and cppf_plane_fit's key); its fit pixels become explained and get label k
//     no eligible candidate: the rounds end.  A chosen candidate has no unexplained fit pixel left: its gain is 0, its net
//     <= 0 < min_gain, and it is never eligible again without being marked.
//
// cppf_scene_explain: per chunk of SCN_IMGS images (their candidate offsets go by value), behind the clears of the outputs:
//   bits    grid (ceil(H*W / SCN_PIX), images), 256 threads: block (x, i) holds its SCN_PIX pixels of image i (depth, region) in
//           registers, reads each render's pixels once and keeps one 64-bit word per pixel, bit c = fit_c.  The wavefront's
//           ballot counts of candidate c stay with lane c (three integers per lane); at the end the four wavefronts meet in LDS
//           and the block adds its non-zero sums with one 64-bit integer atomic per count.  summary[i][0] likewise.
//   round k grid (ceil(H*W / RND_PIX), images), k = 0 .. M: every wavefront first closes round k-1 (k >= 1): the maximum key
//           over gains[i][k-1] -- 64 candidates, one per lane -- is the winner w; block 0 writes the round's row; every word
//           with bit w becomes 0 and its pixel's label k-1.  Then (k < M) round k is counted: the population count of the ballot
//           on bit c is kept by lane c, so that 64 candidates cost one integer add per lane, the wavefronts meet in LDS, and one
//           32-bit integer atomic per candidate and block goes to gains[i][k].  A launch whose round k-2 chose nothing (or whose
//           round k-1 does not) returns at once.  No host synchronisation anywhere.
//   workspace: the words (8 bytes per pixel), then gains uint32 [I][M][64].
#include "cppf_common.h"

#define SCN_THREADS 256
#define SCN_PPT 8                  // pixels per thread of the bits launch
#define SCN_PIX (SCN_THREADS * SCN_PPT)
#define RND_PPT 4                  // words per thread of a round launch
#define RND_PIX (SCN_THREADS * RND_PPT)
#define SCN_MAX_C 64               // candidates per image: one bit each
#define SCN_MAX_M 64               // rounds
#define SCN_IMGS 128               // images per launch (their candidate offsets go by value)
#define SCN_MAX_DIM 8192           // H, W (the renderer's limit): H * W <= 2^26
#define SCN_MAX_P (1 << 24)

struct SceneImages {
  int32_t off[SCN_IMGS + 1];       // global candidate offsets of the launch's images
};

static int64_t scene_words_bytes(int I, int HW) { return align_up((int64_t)I * HW * 8, 256); }

__global__ __launch_bounds__(SCN_THREADS) void scene_bits_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ region,
                                                                 SceneImages img, int HW, const float* __restrict__ renders,
                                                                 float tau, unsigned long long* __restrict__ words,
                                                                 unsigned long long* __restrict__ stat,
                                                                 unsigned long long* __restrict__ summary) {
  __shared__ uint32_t s_c[SCN_THREADS / CPPF_WAVE][3][SCN_MAX_C];
  __shared__ uint32_t s_obs[SCN_THREADS / CPPF_WAVE];
  const int i = blockIdx.y;
  const int p0 = img.off[i], p1 = img.off[i + 1];        // the same for the whole block
  const int px0 = blockIdx.x * SCN_PIX + threadIdx.x;
  const int lane = wave_lane(), w = threadIdx.x / CPPF_WAVE;
  const double tau_d = (double)tau;
  // dob: the observed depth, NaN where it is not > 0 (no comparison on the difference then holds); tfit: tau inside the
  // region, -1 outside it (no |difference| is <= -1): the predicates below need no mask per pixel in scalar registers
  float dob[SCN_PPT], tfit[SCN_PPT];
  uint32_t n_obs = 0;
#pragma unroll
  for (int j = 0; j < SCN_PPT; ++j) {
    const int px = px0 + j * SCN_THREADS;
    dob[j] = __builtin_nanf("");
    tfit[j] = -1.0f;
    bool ob = false;
    if (px < HW) {
      const float d = depth[(int64_t)i * HW + px];
      const bool m = region[(int64_t)i * HW + px] != 0;
      ob = d > 0.0f && m;
      dob[j] = d > 0.0f ? d : dob[j];
      tfit[j] = ob ? tau : tfit[j];
    }
    n_obs += (uint32_t)__popcll(wave_ballot(ob));
  }
  if (lane == 0) s_obs[w] = n_obs;
  unsigned long long bits[SCN_PPT];
#pragma unroll
  for (int j = 0; j < SCN_PPT; ++j) bits[j] = 0;
  uint32_t a_drawn = 0, a_fit = 0, a_viol = 0;            // lane c: the wavefront's counts of candidate c
  for (int p = p0; p < p1; ++p) {
    const int c = p - p0;
    const unsigned long long bit = 1ull << c;
    const float* dc = renders + (int64_t)p * HW;
    uint32_t n_drawn = 0, n_fit = 0, n_viol = 0;
#pragma unroll
    for (int j = 0; j < SCN_PPT; ++j) {
      const int px = px0 + j * SCN_THREADS;
      const float h = px < HW ? dc[px] : 0.0f;
      const double diff = (double)dob[j] - (double)h;
      const bool drawn = h > 0.0f;
      const bool fit = drawn && fabs(diff) <= (double)tfit[j];
      n_drawn += (uint32_t)__popcll(wave_ballot(drawn));
      n_viol += (uint32_t)__popcll(wave_ballot(drawn && diff > tau_d));
      n_fit += (uint32_t)__popcll(wave_ballot(fit));
      bits[j] |= fit ? bit : 0ull;
    }
    a_drawn = lane == c ? n_drawn : a_drawn;
    a_fit = lane == c ? n_fit : a_fit;
    a_viol = lane == c ? n_viol : a_viol;
  }
  s_c[w][0][lane] = a_drawn;
  s_c[w][1][lane] = a_fit;
  s_c[w][2][lane] = a_viol;
  if (p1 > p0) {
#pragma unroll
    for (int j = 0; j < SCN_PPT; ++j) {
      const int px = px0 + j * SCN_THREADS;
      if (px < HW) words[(int64_t)i * HW + px] = bits[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 * SCN_MAX_C) {                      // thread t: count t / 64 of candidate t % 64
    const int q = threadIdx.x / SCN_MAX_C, c = threadIdx.x % SCN_MAX_C;
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < SCN_THREADS / CPPF_WAVE; ++k) s += s_c[k][q][c];
    if (c < p1 - p0 && s) atomicAdd(&stat[(int64_t)(p0 + c) * 3 + q], s);
  } else if (threadIdx.x == 3 * SCN_MAX_C) {
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < SCN_THREADS / CPPF_WAVE; ++k) s += s_obs[k];
    if (s) atomicAdd(&summary[3 * i], s);
  }
}

__global__ __launch_bounds__(SCN_THREADS) void scene_round_kernel(int k, int M, SceneImages img, int HW, long long min_gain,
                                                                  long long viol_weight, const long long* __restrict__ stat,
                                                                  unsigned long long* __restrict__ words,
                                                                  uint32_t* __restrict__ gains, int32_t* __restrict__ chosen,
                                                                  long long* __restrict__ gain, long long* __restrict__ net,
                                                                  uint8_t* __restrict__ labels, long long* __restrict__ summary) {
  __shared__ uint32_t s_cnt[SCN_MAX_C];
  const int i = blockIdx.y;
  const int p0 = img.off[i];
  const int C = img.off[i + 1] - p0;                      // the same for the whole block, like every return below
  if (C == 0) return;
  if (k >= 2 && chosen[(int64_t)i * M + k - 2] < 0) return;                // round k-2 chose nothing: the rounds are over
  const int lane = wave_lane();
  uint32_t* G = gains + (int64_t)i * M * SCN_MAX_C;
  int win = -1;
  if (k >= 1) {
    // round k-1's winner, by every wavefront for itself: candidate `lane`
    unsigned long long key = 0;
    if (lane < C) {
      const long long g = (long long)G[(k - 1) * SCN_MAX_C + lane];
      const long long n = g - viol_weight * stat[(int64_t)(p0 + lane) * 3 + 2];
      if (n >= min_gain) key = ((unsigned long long)n << 32) | (0xFFFFFFFFu - (uint32_t)lane);    // n >= 1: never a negative net
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(key, off);
      key = o > key ? o : key;
    }
    if (key == 0) return;                                 // no eligible candidate (chosen[i][k-1] stays -1)
    win = (int)(0xFFFFFFFFu - (uint32_t)key);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      const long long g = (long long)G[(k - 1) * SCN_MAX_C + win];
      chosen[(int64_t)i * M + k - 1] = win;
      gain[(int64_t)i * M + k - 1] = g;
      net[(int64_t)i * M + k - 1] = (long long)(key >> 32);
      summary[3 * i + 1] += g;                            // one thread per image and launch
      summary[3 * i + 2] = k;
    }
  }
  if (threadIdx.x < SCN_MAX_C) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long wbit = win >= 0 ? 1ull << win : 0ull;
  unsigned long long wd[RND_PPT];
  bool any = false;
#pragma unroll
  for (int j = 0; j < RND_PPT; ++j) {
    const int px = blockIdx.x * RND_PIX + j * SCN_THREADS + threadIdx.x;
    wd[j] = 0;
    if (px < HW) {
      unsigned long long v = words[(int64_t)i * HW + px];
      if (v & wbit) {                                     // the winner explains this pixel
        v = 0;
        words[(int64_t)i * HW + px] = 0;
        labels[(int64_t)i * HW + px] = (uint8_t)(k - 1);
      }
      wd[j] = v;
    }
    any = any || wd[j] != 0;
  }
  if (k < M && wave_ballot(any) != 0) {
    uint32_t acc = 0;
    for (int c = 0; c < C; ++c) {
      const unsigned long long bit = 1ull << c;
      uint32_t n = 0;
#pragma unroll
      for (int j = 0; j < RND_PPT; ++j) n += (uint32_t)__popcll(wave_ballot((wd[j] & bit) != 0));
      acc = lane == c ? n : acc;
    }
    if (acc) atomicAdd(&s_cnt[lane], acc);
  }
  __syncthreads();
  if (k < M && threadIdx.x < C) {
    const uint32_t n = s_cnt[threadIdx.x];
    if (n) atomicAdd(&G[k * SCN_MAX_C + threadIdx.x], n);
  }
}

extern "C" int64_t cppf_scene_explain_workspace_bytes(int I, int H, int W, int max_rounds) {
  if (I < 1 || H < 1 || W < 1 || H > SCN_MAX_DIM || W > SCN_MAX_DIM || max_rounds < 1 || max_rounds > SCN_MAX_M) return 0;
  return scene_words_bytes(I, H * W) + (int64_t)I * max_rounds * SCN_MAX_C * (int64_t)sizeof(uint32_t);
}

extern "C" int cppf_scene_explain(int I, int H, int W, const float* depth, const uint8_t* region, const int32_t* h_cand_off, int P,
                                  const float* renders, float tau, int min_gain, int viol_weight, int max_rounds, int32_t* chosen,
                                  int64_t* gain, int64_t* net, int64_t* stat, uint8_t* labels, int64_t* summary, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  CPPF_CHECK_ARG(I >= 1 && H >= 1 && W >= 1 && H <= SCN_MAX_DIM && W <= SCN_MAX_DIM);    // H * W <= 2^26: a net fits 31 bits
  CPPF_CHECK_ARG(max_rounds >= 1 && max_rounds <= SCN_MAX_M);
  CPPF_CHECK_ARG(min_gain >= 1);
  CPPF_CHECK_ARG(viol_weight >= 0);
  CPPF_CHECK_ARG(tau >= 0.0f);
  CPPF_CHECK_ARG(P >= 0 && P <= SCN_MAX_P && h_cand_off);
  CPPF_CHECK_ARG(h_cand_off[0] == 0 && h_cand_off[I] == P);
  for (int i = 0; i < I; ++i) CPPF_CHECK_ARG(h_cand_off[i] <= h_cand_off[i + 1]);
  for (int i = 0; i < I; ++i) {
    if (h_cand_off[i + 1] - h_cand_off[i] > SCN_MAX_C) {
      snprintf(g_cppf_err, sizeof(g_cppf_err), "cppf_scene_explain: %d candidates on image %d, more than %d unsupported",
               h_cand_off[i + 1] - h_cand_off[i], i, SCN_MAX_C);
      return CPPF_EUNSUPPORTED;
    }
  }
  CPPF_CHECK_ARG(depth && region && chosen && gain && net && labels && summary && (P == 0 || (renders && stat)));
  CPPF_CHECK_ARG(workspace && (uintptr_t)workspace % 8 == 0);
  if (workspace_bytes < cppf_scene_explain_workspace_bytes(I, H, W, max_rounds)) {
    snprintf(g_cppf_err, sizeof(g_cppf_err), "cppf_scene_explain: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)cppf_scene_explain_workspace_bytes(I, H, W, max_rounds));
    return CPPF_ECAPACITY;
  }
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W, M = max_rounds;
  unsigned long long* words = (unsigned long long*)workspace;
  uint32_t* gains = (uint32_t*)((char*)workspace + scene_words_bytes(I, HW));
  CPPF_HIP(hipMemsetAsync(gains, 0, (size_t)I * M * SCN_MAX_C * sizeof(uint32_t), st));
  CPPF_HIP(hipMemsetAsync(chosen, 0xff, (size_t)I * M * sizeof(int32_t), st));
  CPPF_HIP(hipMemsetAsync(gain, 0, (size_t)I * M * sizeof(int64_t), st));
  CPPF_HIP(hipMemsetAsync(net, 0, (size_t)I * M * sizeof(int64_t), st));
  CPPF_HIP(hipMemsetAsync(labels, 0xff, (size_t)I * HW, st));
  CPPF_HIP(hipMemsetAsync(summary, 0, (size_t)I * 3 * sizeof(int64_t), st));
  if (P) CPPF_HIP(hipMemsetAsync(stat, 0, (size_t)P * 3 * sizeof(int64_t), st));
  const int nbx = (HW + SCN_PIX - 1) / SCN_PIX, nrx = (HW + RND_PIX - 1) / RND_PIX;
  for (int i0 = 0; i0 < I; i0 += SCN_IMGS) {
    const int n = I - i0 < SCN_IMGS ? I - i0 : SCN_IMGS;
    SceneImages img;
    for (int i = 0; i <= n; ++i) img.off[i] = h_cand_off[i0 + i];
    hipLaunchKernelGGL(scene_bits_kernel, dim3(nbx, n), dim3(SCN_THREADS), 0, st, depth + (int64_t)i0 * HW,
                       region + (int64_t)i0 * HW, img, HW, renders, tau, words + (int64_t)i0 * HW, (unsigned long long*)stat,
                       (unsigned long long*)summary + (int64_t)i0 * 3);
    if (img.off[0] == img.off[n]) continue;               // no candidate on these images
    for (int k = 0; k <= M; ++k)
      hipLaunchKernelGGL(scene_round_kernel, dim3(nrx, n), dim3(SCN_THREADS), 0, st, k, M, img, HW, (long long)min_gain,
                         (long long)viol_weight, (const long long*)stat, words + (int64_t)i0 * HW,
                         gains + (int64_t)i0 * M * SCN_MAX_C, chosen + (int64_t)i0 * M, (long long*)gain + (int64_t)i0 * M,
                         (long long*)net + (int64_t)i0 * M, labels + (int64_t)i0 * HW, (long long*)summary + (int64_t)i0 * 3);
    CPPF_LAUNCH_CHECK();
  }
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
