// Scene explanation over up to 512 candidates per image: cppf_scene_explain's definition -- the head
// comment of cppf_scene.hip, word for word: predicates, stat, gain, net, eligibility, key, labels, summary, end of the rounds --
// with the candidate index c up to 511.  cppf2_amd/scene.py (explain_wide) drives the entry point; tests/scene_ref.py restates
// it for any C.  Integer counts and integer maxima only: every output equals the restatement's, and for images of at most 64
// candidates cppf_scene_explain's, byte for byte.  cppf_scene.hip is not touched by this file: the 64-candidate kernels and
// their launches stay what they were.  gfx950 only.
//
// G = ceil(max_candidates / 64) word planes: plane g, image i, pixel px is one 64-bit word, bit b = fit_c for c = 64 g + b.
// cppf_scene_explain_wide: per chunk of WSC_IMGS images, behind the clears of the outputs:
//   bits    grid (ceil(H*W / WSC_PIX), images, G), 256 threads: scene_bits_kernel's body on the candidates 64 z .. 64 z + 63 of
//           its image (a block whose image has none of them returns); only the blocks z = 0 add summary[i][0].
//   round k grid (ceil(H*W / WRN_PIX), images), k = 0 .. M: ONE block owns its pixel tile in EVERY plane.  Closing round k-1
//           clears a pixel in all planes when the winner's bit is set in plane win / 64; were the planes spread over blocks, one
//           block would read the winner's plane while its owner clears it, in the same launch.  So a thread first reads its
//           pixels' words of the winner's plane and keeps one bit per pixel (explained or not), then walks g = 0 .. G_i - 1:
//           load, clear and label where the winner explains the pixel, count the rest -- the words of one plane in registers at
//           a time.  Every wavefront computes the winner for itself: lane l folds the keys of the candidates l, l + 64, ..,
//           then the 6-step maximum.  The transposed ballot count runs per plane into 64 G counters in LDS; a wavefront whose
//           words of a plane are all zero skips that plane.  The early returns are cppf_scene_explain's, so the M + 2 launches
//           per 128 images are planned without asking the host.
//   workspace: G planes of words (each 8 bytes per pixel, rounded up to 256), then gains uint32 [I][M][64 G].
#include "cppf_common.h"

#define WSC_THREADS 256
#define WSC_PPT 8                  // pixels per thread of the bits launch
#define WSC_PIX (WSC_THREADS * WSC_PPT)
#define WRN_PPT 4                  // pixels per thread of a round launch
#define WRN_PIX (WSC_THREADS * WRN_PPT)
#define WSC_PLANE 64               // candidates per word plane: one bit each
#define WSC_MAX_C 512              // candidates per image
#define WSC_MAX_G (WSC_MAX_C / WSC_PLANE)
#define WSC_MAX_M 64               // rounds
#define WSC_IMGS 128               // images per launch (their candidate offsets go by value)
#define WSC_MAX_DIM 8192           // H, W (the renderer's limit): H * W <= 2^26
#define WSC_MAX_P (1 << 24)

struct WideImages {
  int32_t off[WSC_IMGS + 1];       // global candidate offsets of the launch's images
};

static int64_t wide_plane_bytes(int I, int HW) { return align_up((int64_t)I * HW * 8, 256); }

// plane: 64-bit words from one plane to the next (the whole call's images)
__global__ __launch_bounds__(WSC_THREADS) void scene_bits_wide_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ region,
                                                                      WideImages img, int HW, const float* __restrict__ renders,
                                                                      float tau, unsigned long long* __restrict__ words,
                                                                      long long plane, unsigned long long* __restrict__ stat,
                                                                      unsigned long long* __restrict__ summary) {
  __shared__ uint32_t s_c[WSC_THREADS / CPPF_WAVE][3][WSC_PLANE];
  __shared__ uint32_t s_obs[WSC_THREADS / CPPF_WAVE];
  const int i = blockIdx.y, g = blockIdx.z;
  const int p0 = img.off[i] + g * WSC_PLANE;              // the same for the whole block, like the return below
  const int p1 = img.off[i + 1] < p0 + WSC_PLANE ? img.off[i + 1] : p0 + WSC_PLANE;
  if (g > 0 && p1 <= p0) return;                          // the image has no candidate of this plane
  const int px0 = blockIdx.x * WSC_PIX + threadIdx.x;
  const int lane = wave_lane(), w = threadIdx.x / CPPF_WAVE;
  const double tau_d = (double)tau;
  // dob: the observed depth, NaN where it is not > 0 (no comparison on the difference then holds); tfit: tau inside the
  // region, -1 outside it (no |difference| is <= -1)
  float dob[WSC_PPT], tfit[WSC_PPT];
  uint32_t n_obs = 0;
#pragma unroll
  for (int j = 0; j < WSC_PPT; ++j) {
    const int px = px0 + j * WSC_THREADS;
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
  unsigned long long bits[WSC_PPT];
#pragma unroll
  for (int j = 0; j < WSC_PPT; ++j) bits[j] = 0;
  uint32_t a_drawn = 0, a_fit = 0, a_viol = 0;            // lane b: the wavefront's counts of candidate 64 g + b
  for (int p = p0; p < p1; ++p) {
    const int b = p - p0;
    const unsigned long long bit = 1ull << b;
    const float* dc = renders + (int64_t)p * HW;
    uint32_t n_drawn = 0, n_fit = 0, n_viol = 0;
#pragma unroll
    for (int j = 0; j < WSC_PPT; ++j) {
      const int px = px0 + j * WSC_THREADS;
      const float h = px < HW ? dc[px] : 0.0f;
      const double diff = (double)dob[j] - (double)h;
      const bool drawn = h > 0.0f;
      const bool fit = drawn && fabs(diff) <= (double)tfit[j];
      n_drawn += (uint32_t)__popcll(wave_ballot(drawn));
      n_viol += (uint32_t)__popcll(wave_ballot(drawn && diff > tau_d));
      n_fit += (uint32_t)__popcll(wave_ballot(fit));
      bits[j] |= fit ? bit : 0ull;
    }
    a_drawn = lane == b ? n_drawn : a_drawn;
    a_fit = lane == b ? n_fit : a_fit;
    a_viol = lane == b ? n_viol : a_viol;
  }
  s_c[w][0][lane] = a_drawn;
  s_c[w][1][lane] = a_fit;
  s_c[w][2][lane] = a_viol;
  if (p1 > p0) {
    unsigned long long* wp = words + (int64_t)g * plane + (int64_t)i * HW;
#pragma unroll
    for (int j = 0; j < WSC_PPT; ++j) {
      const int px = px0 + j * WSC_THREADS;
      if (px < HW) wp[px] = bits[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 * WSC_PLANE) {                      // thread t: count t / 64 of candidate 64 g + t % 64
    const int q = threadIdx.x / WSC_PLANE, b = threadIdx.x % WSC_PLANE;
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < WSC_THREADS / CPPF_WAVE; ++k) s += s_c[k][q][b];
    if (b < p1 - p0 && s) atomicAdd(&stat[(int64_t)(p0 + b) * 3 + q], s);
  } else if (threadIdx.x == 3 * WSC_PLANE && g == 0) {
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < WSC_THREADS / CPPF_WAVE; ++k) s += s_obs[k];
    if (s) atomicAdd(&summary[3 * i], s);
  }
}

// CS: the gains of one round, 64 G entries (G the call's plane count); an image of C candidates uses its planes 0 .. ceil(C / 64) - 1
__global__ __launch_bounds__(WSC_THREADS) void scene_round_wide_kernel(int k, int M, WideImages img, int HW, int CS, long long min_gain,
                                                                       long long viol_weight, const long long* __restrict__ stat,
                                                                       unsigned long long* __restrict__ words, long long plane,
                                                                       uint32_t* __restrict__ gains, int32_t* __restrict__ chosen,
                                                                       long long* __restrict__ gain, long long* __restrict__ net,
                                                                       uint8_t* __restrict__ labels, long long* __restrict__ summary) {
  __shared__ uint32_t s_cnt[WSC_MAX_C];
  const int i = blockIdx.y;
  const int p0 = img.off[i];
  const int C = img.off[i + 1] - p0;                      // the same for the whole block, like every return below
  if (C == 0) return;
  if (k >= 2 && chosen[(int64_t)i * M + k - 2] < 0) return;                // round k-2 chose nothing: the rounds are over
  const int lane = wave_lane();
  const int Gi = (C + WSC_PLANE - 1) / WSC_PLANE;         // <= CS / 64
  uint32_t* G = gains + (int64_t)i * M * CS;
  int win = -1;
  if (k >= 1) {
    // round k-1's winner, by every wavefront for itself: lane l folds the candidates l, l + 64, ..
    unsigned long long key = 0;
    for (int c = lane; c < C; c += WSC_PLANE) {
      const long long g = (long long)G[(k - 1) * CS + c];
      const long long n = g - viol_weight * stat[(int64_t)(p0 + c) * 3 + 2];
      if (n >= min_gain) {                                // n >= 1: never a negative net
        const unsigned long long kc = ((unsigned long long)n << 32) | (0xFFFFFFFFu - (uint32_t)c);
        key = kc > key ? kc : key;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(key, off);
      key = o > key ? o : key;
    }
    if (key == 0) return;                                 // no eligible candidate (chosen[i][k-1] stays -1)
    win = (int)(0xFFFFFFFFu - (uint32_t)key);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      const long long g = (long long)G[(k - 1) * CS + win];
      chosen[(int64_t)i * M + k - 1] = win;
      gain[(int64_t)i * M + k - 1] = g;
      net[(int64_t)i * M + k - 1] = (long long)(key >> 32);
      summary[3 * i + 1] += g;                            // one thread per image and launch
      summary[3 * i + 2] = k;
    }
  }
  for (int t = threadIdx.x; t < Gi * WSC_PLANE; t += WSC_THREADS) s_cnt[t] = 0;
  __syncthreads();
  unsigned long long* wi = words + (int64_t)i * HW;       // plane 0 of image i
  const int px0 = blockIdx.x * WRN_PIX + threadIdx.x;
  // the winner's plane first: whether it explains each of this thread's pixels, before any plane of them is cleared
  bool hit[WRN_PPT];
#pragma unroll
  for (int j = 0; j < WRN_PPT; ++j) hit[j] = false;
  if (win >= 0) {
    const unsigned long long wbit = 1ull << (win % WSC_PLANE);
    const unsigned long long* ww = wi + (int64_t)(win / WSC_PLANE) * plane;
#pragma unroll
    for (int j = 0; j < WRN_PPT; ++j) {
      const int px = px0 + j * WSC_THREADS;
      if (px < HW) hit[j] = (ww[px] & wbit) != 0;
    }
#pragma unroll
    for (int j = 0; j < WRN_PPT; ++j) {
      const int px = px0 + j * WSC_THREADS;
      if (hit[j]) labels[(int64_t)i * HW + px] = (uint8_t)(k - 1);
    }
  }
  for (int g = 0; g < Gi; ++g) {
    unsigned long long* wp = wi + (int64_t)g * plane;
    unsigned long long wd[WRN_PPT];
    bool any = false;
#pragma unroll
    for (int j = 0; j < WRN_PPT; ++j) {
      const int px = px0 + j * WSC_THREADS;
      wd[j] = 0;
      if (px < HW) {
        unsigned long long v = wp[px];
        if (hit[j]) {                                     // the winner explains this pixel: no candidate gains it again
          if (v) wp[px] = 0;
          v = 0;
        }
        wd[j] = v;
      }
      any = any || wd[j] != 0;
    }
    if (k < M && wave_ballot(any) != 0) {
      const int cn = C - g * WSC_PLANE < WSC_PLANE ? C - g * WSC_PLANE : WSC_PLANE;
      uint32_t acc = 0;
      for (int b = 0; b < cn; ++b) {
        const unsigned long long bit = 1ull << b;
        uint32_t n = 0;
#pragma unroll
        for (int j = 0; j < WRN_PPT; ++j) n += (uint32_t)__popcll(wave_ballot((wd[j] & bit) != 0));
        acc = lane == b ? n : acc;
      }
      if (acc) atomicAdd(&s_cnt[g * WSC_PLANE + lane], acc);
    }
  }
  __syncthreads();
  if (k < M) {
    for (int t = threadIdx.x; t < C; t += WSC_THREADS) {
      const uint32_t n = s_cnt[t];
      if (n) atomicAdd(&G[k * CS + t], n);
    }
  }
}

static bool wide_sizes_ok(int I, int H, int W, int max_rounds, int max_candidates) {
  return I >= 1 && H >= 1 && W >= 1 && H <= WSC_MAX_DIM && W <= WSC_MAX_DIM && max_rounds >= 1 && max_rounds <= WSC_MAX_M &&
         max_candidates >= 1 && max_candidates <= WSC_MAX_C;
}

extern "C" int64_t cppf_scene_explain_wide_workspace_bytes(int I, int H, int W, int max_rounds, int max_candidates) {
  if (!wide_sizes_ok(I, H, W, max_rounds, max_candidates)) return 0;
  const int64_t G = (max_candidates + WSC_PLANE - 1) / WSC_PLANE;
  return G * wide_plane_bytes(I, H * W) + (int64_t)I * max_rounds * G * WSC_PLANE * (int64_t)sizeof(uint32_t);
}

extern "C" int cppf_scene_explain_wide(int I, int H, int W, const float* depth, const uint8_t* region, const int32_t* h_cand_off, int P,
                                       const float* renders, float tau, int min_gain, int viol_weight, int max_rounds,
                                       int max_candidates, int32_t* chosen, int64_t* gain, int64_t* net, int64_t* stat,
                                       uint8_t* labels, int64_t* summary, void* workspace, int64_t workspace_bytes, void* stream) {
  CPPF_CHECK_ARG(I >= 1 && H >= 1 && W >= 1 && H <= WSC_MAX_DIM && W <= WSC_MAX_DIM);    // H * W <= 2^26: a net fits 31 bits
  CPPF_CHECK_ARG(max_rounds >= 1 && max_rounds <= WSC_MAX_M);
  CPPF_CHECK_ARG(min_gain >= 1);
  CPPF_CHECK_ARG(viol_weight >= 0);
  CPPF_CHECK_ARG(tau >= 0.0f);
  CPPF_CHECK_ARG(P >= 0 && P <= WSC_MAX_P && h_cand_off);
  CPPF_CHECK_ARG(h_cand_off[0] == 0 && h_cand_off[I] == P);
  for (int i = 0; i < I; ++i) CPPF_CHECK_ARG(h_cand_off[i] <= h_cand_off[i + 1]);
  if (max_candidates < 1 || max_candidates > WSC_MAX_C) {
    snprintf(g_cppf_err, sizeof(g_cppf_err), "cppf_scene_explain_wide: max_candidates = %d: fewer than 1 or more than %d unsupported",
             max_candidates, WSC_MAX_C);
    return CPPF_EUNSUPPORTED;
  }
  for (int i = 0; i < I; ++i) {
    if (h_cand_off[i + 1] - h_cand_off[i] > max_candidates) {
      snprintf(g_cppf_err, sizeof(g_cppf_err), "cppf_scene_explain_wide: invalid argument: %d candidates on image %d, max_candidates = %d",
               h_cand_off[i + 1] - h_cand_off[i], i, max_candidates);
      return CPPF_EINVAL;
    }
  }
  CPPF_CHECK_ARG(depth && region && chosen && gain && net && labels && summary && (P == 0 || (renders && stat)));
  CPPF_CHECK_ARG(workspace && (uintptr_t)workspace % 8 == 0);
  const int64_t need = cppf_scene_explain_wide_workspace_bytes(I, H, W, max_rounds, max_candidates);
  if (workspace_bytes < need) {
    snprintf(g_cppf_err, sizeof(g_cppf_err), "cppf_scene_explain_wide: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)need);
    return CPPF_ECAPACITY;
  }
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W, M = max_rounds;
  const int G = (max_candidates + WSC_PLANE - 1) / WSC_PLANE, CS = G * WSC_PLANE;
  const long long plane = (long long)(wide_plane_bytes(I, HW) / 8);
  unsigned long long* words = (unsigned long long*)workspace;
  uint32_t* gains = (uint32_t*)((char*)workspace + (int64_t)G * wide_plane_bytes(I, HW));
  CPPF_HIP(hipMemsetAsync(gains, 0, (size_t)I * M * CS * sizeof(uint32_t), st));
  CPPF_HIP(hipMemsetAsync(chosen, 0xff, (size_t)I * M * sizeof(int32_t), st));
  CPPF_HIP(hipMemsetAsync(gain, 0, (size_t)I * M * sizeof(int64_t), st));
  CPPF_HIP(hipMemsetAsync(net, 0, (size_t)I * M * sizeof(int64_t), st));
  CPPF_HIP(hipMemsetAsync(labels, 0xff, (size_t)I * HW, st));
  CPPF_HIP(hipMemsetAsync(summary, 0, (size_t)I * 3 * sizeof(int64_t), st));
  if (P) CPPF_HIP(hipMemsetAsync(stat, 0, (size_t)P * 3 * sizeof(int64_t), st));
  const int nbx = (HW + WSC_PIX - 1) / WSC_PIX, nrx = (HW + WRN_PIX - 1) / WRN_PIX;
  for (int i0 = 0; i0 < I; i0 += WSC_IMGS) {
    const int n = I - i0 < WSC_IMGS ? I - i0 : WSC_IMGS;
    WideImages img;
    int most = 0;                                         // the chunk's largest image: the planes its bits launch needs
    for (int i = 0; i <= n; ++i) img.off[i] = h_cand_off[i0 + i];
    for (int i = 0; i < n; ++i) most = img.off[i + 1] - img.off[i] > most ? img.off[i + 1] - img.off[i] : most;
    const int gz = most > WSC_PLANE ? (most + WSC_PLANE - 1) / WSC_PLANE : 1;
    hipLaunchKernelGGL(scene_bits_wide_kernel, dim3(nbx, n, gz), dim3(WSC_THREADS), 0, st, depth + (int64_t)i0 * HW,
                       region + (int64_t)i0 * HW, img, HW, renders, tau, words + (int64_t)i0 * HW, plane, (unsigned long long*)stat,
                       (unsigned long long*)summary + (int64_t)i0 * 3);
    if (img.off[0] == img.off[n]) continue;               // no candidate on these images
    for (int k = 0; k <= M; ++k)
      hipLaunchKernelGGL(scene_round_wide_kernel, dim3(nrx, n), dim3(WSC_THREADS), 0, st, k, M, img, HW, CS, (long long)min_gain,
                         (long long)viol_weight, (const long long*)stat, words + (int64_t)i0 * HW, plane,
                         gains + (int64_t)i0 * M * CS, chosen + (int64_t)i0 * M, (long long*)gain + (int64_t)i0 * M,
                         (long long*)net + (int64_t)i0 * M, labels + (int64_t)i0 * HW, (long long*)summary + (int64_t)i0 * 3);
    CPPF_LAUNCH_CHECK();
  }
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
