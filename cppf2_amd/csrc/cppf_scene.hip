// Scene explanation (global hypothesis verification; not in the reference): of all verified candidate poses of a depth image,
// the subset that together explains the observed depth, every observed pixel counted once, chosen greedily.
// cppf2_amd/scene.py (explain, explain_wide) drives the two entry points; tests/scene_ref.py restates the definition for any C.
// Integer counts and integer maxima only, so an image's outputs do not depend on the grid, the batch or the order: every output
// equals the restatement's, and for images of at most 64 candidates cppf_scene_explain_wide's equals cppf_scene_explain's, byte
// for byte.  gfx950 only.
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
// The candidate index c goes up to 511 (DESIGN.md sections 22 and 24).  G = ceil(max_candidates / 64) word planes: plane g,
// image i, pixel px is one 64-bit word, bit b = fit_c for c = 64 g + b.  cppf_scene_explain_wide runs the general case below.
// cppf_scene_explain has G = 1: its bits kernel is the same template, instantiated with the plane index a constant 0 (the
// `ONE` branches; instruction for instruction a kernel written for one plane), and its round kernel is the one-plane form
// beside the general one -- a template folded that pair too, with equal registers and LDS, but its one-plane instantiation
// missed the timing condition of DESIGN.md section 24 in three of four comparisons (up to 1.5 % behind), so the pair stays.
// Either entry point, per chunk of SCN_IMGS images (their candidate offsets go by value), behind the clears of the outputs:
//   bits    grid (ceil(H*W / SCN_PIX), images, planes of the chunk's largest image), 256 threads: block (x, i, z) holds its
//           SCN_PIX pixels of image i (depth, region) in registers, reads each render's pixels of the candidates 64 z .. 64 z + 63
//           once (a block whose image has none of them returns) and keeps one 64-bit word per pixel, bit b = fit_c.  The
//           wavefront's ballot counts of candidate 64 z + b stay with lane b (three integers per lane); at the end the four
//           wavefronts meet in LDS and the block adds its non-zero sums with one 64-bit integer atomic per count.  summary[i][0]
//           likewise, by the blocks z = 0 only.
//   round k grid (ceil(H*W / RND_PIX), images), k = 0 .. M: ONE block owns its pixel tile in EVERY plane.  Closing round k-1
//           clears a pixel in all planes when the winner's bit is set in plane win / 64; were the planes spread over blocks, one
//           block would read the winner's plane while its owner clears it, in the same launch.  Every wavefront first closes
//           round k-1 (k >= 1) for itself: lane l folds the keys of the candidates l, l + 64, .. of gains[i][k-1], then the
//           6-step maximum is the winner w; block 0 writes the round's row.  A thread then reads its pixels' words of the
//           winner's plane and keeps one bit per pixel (explained or not), their labels become k-1, and it walks g = 0 .. G_i - 1:
//           load, clear where the winner explains the pixel, count the rest -- the words of one plane in registers at a time.
//           (scene_round_kernel, one plane: one key per lane, no plane loop, and the word just loaded decides -- it is
//           cleared and labelled in the same place; gains uint32 [I][M][64].)  Then (k < M) round k is
//           counted: the population count of the ballot on bit b is kept by lane b, so that 64 candidates cost one integer add
//           per lane, per plane into 64 G counters in LDS where the wavefronts meet; a wavefront whose words of a plane are all
//           zero skips that plane.  One 32-bit integer atomic per candidate and block goes to gains[i][k].  A launch whose round
//           k-2 chose nothing (or whose round k-1 does not) returns at once, so the M + 2 launches per 128 images are planned
//           without asking the host.  No host synchronisation anywhere.
//   workspace: G planes of words (each 8 bytes per pixel, rounded up to 256), then gains uint32 [I][M][64 G].
#include <string.h>
#include "cppf_common.h"

#define SCN_THREADS 256
#define SCN_PPT 8                  // pixels per thread of the bits launch
#define SCN_PIX (SCN_THREADS * SCN_PPT)
#define RND_PPT 4                  // words per thread and plane of a round launch
#define RND_PIX (SCN_THREADS * RND_PPT)
#define SCN_PLANE 64               // candidates per word plane: one bit each
#define SCN_MAX_C 512              // candidates per image
#define SCN_MAX_M 64               // rounds
#define SCN_IMGS 128               // images per launch (their candidate offsets go by value)
#define SCN_MAX_DIM 8192           // H, W (the renderer's limit): H * W <= 2^26
#define SCN_MAX_P (1 << 24)

struct SceneImages {
  int32_t off[SCN_IMGS + 1];       // global candidate offsets of the launch's images
};

static int64_t scene_words_bytes(int I, int HW) { return align_up((int64_t)I * HW * 8, 256); }

// plane: 64-bit words from one plane to the next (the whole call's images)
template <int MAXC>
__global__ __launch_bounds__(SCN_THREADS) void scene_bits_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ region,
                                                                 SceneImages img, int HW, const float* __restrict__ renders,
                                                                 float tau, unsigned long long* __restrict__ words, long long plane,
                                                                 unsigned long long* __restrict__ stat,
                                                                 unsigned long long* __restrict__ summary) {
  constexpr bool ONE = MAXC <= SCN_PLANE;
  __shared__ uint32_t s_c[SCN_THREADS / CPPF_WAVE][3][SCN_PLANE];
  __shared__ uint32_t s_obs[SCN_THREADS / CPPF_WAVE];
  const int i = blockIdx.y, g = ONE ? 0 : blockIdx.z;
  const int p0 = img.off[i] + g * SCN_PLANE;              // the same for the whole block, like the return below
  const int p1 = ONE || img.off[i + 1] < p0 + SCN_PLANE ? img.off[i + 1] : p0 + SCN_PLANE;
  if (g > 0 && p1 <= p0) return;                          // the image has no candidate of this plane
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
  uint32_t a_drawn = 0, a_fit = 0, a_viol = 0;            // lane b: the wavefront's counts of candidate 64 g + b
  for (int p = p0; p < p1; ++p) {
    const int b = p - p0;
    const unsigned long long bit = 1ull << b;
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
    for (int j = 0; j < SCN_PPT; ++j) {
      const int px = px0 + j * SCN_THREADS;
      if (px < HW) wp[px] = bits[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 * SCN_PLANE) {                      // thread t: count t / 64 of candidate 64 g + t % 64
    const int q = threadIdx.x / SCN_PLANE, b = threadIdx.x % SCN_PLANE;
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < SCN_THREADS / CPPF_WAVE; ++k) s += s_c[k][q][b];
    if (b < p1 - p0 && s) atomicAdd(&stat[(int64_t)(p0 + b) * 3 + q], s);
  } else if (threadIdx.x == 3 * SCN_PLANE && g == 0) {
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < SCN_THREADS / CPPF_WAVE; ++k) s += s_obs[k];
    if (s) atomicAdd(&summary[3 * i], s);
  }
}

// The rounds of one plane (cppf_scene_explain): scene_round_wide_kernel below with G = 1 written out.
__global__ __launch_bounds__(SCN_THREADS) void scene_round_kernel(int k, int M, SceneImages img, int HW, long long min_gain,
                                                                  long long viol_weight, const long long* __restrict__ stat,
                                                                  unsigned long long* __restrict__ words,
                                                                  uint32_t* __restrict__ gains, int32_t* __restrict__ chosen,
                                                                  long long* __restrict__ gain, long long* __restrict__ net,
                                                                  uint8_t* __restrict__ labels, long long* __restrict__ summary) {
  __shared__ uint32_t s_cnt[SCN_PLANE];
  const int i = blockIdx.y;
  const int p0 = img.off[i];
  const int C = img.off[i + 1] - p0;                      // the same for the whole block, like every return below
  if (C == 0) return;
  if (k >= 2 && chosen[(int64_t)i * M + k - 2] < 0) return;                // round k-2 chose nothing: the rounds are over
  const int lane = wave_lane();
  uint32_t* G = gains + (int64_t)i * M * SCN_PLANE;
  int win = -1;
  if (k >= 1) {
    // round k-1's winner, by every wavefront for itself: candidate `lane`
    unsigned long long key = 0;
    if (lane < C) {
      const long long g = (long long)G[(k - 1) * SCN_PLANE + lane];
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
      const long long g = (long long)G[(k - 1) * SCN_PLANE + win];
      chosen[(int64_t)i * M + k - 1] = win;
      gain[(int64_t)i * M + k - 1] = g;
      net[(int64_t)i * M + k - 1] = (long long)(key >> 32);
      summary[3 * i + 1] += g;                            // one thread per image and launch
      summary[3 * i + 2] = k;
    }
  }
  if (threadIdx.x < SCN_PLANE) s_cnt[threadIdx.x] = 0;
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
    if (n) atomicAdd(&G[k * SCN_PLANE + threadIdx.x], n);
  }
}

// CS: the gains of one round, 64 G entries (G the call's plane count); an image of C candidates uses its planes 0 .. ceil(C / 64) - 1
__global__ __launch_bounds__(SCN_THREADS) void scene_round_wide_kernel(int k, int M, SceneImages img, int HW, int CS, long long min_gain,
                                                                       long long viol_weight, const long long* __restrict__ stat,
                                                                       unsigned long long* __restrict__ words, long long plane,
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
  const int Gi = (C + SCN_PLANE - 1) / SCN_PLANE;         // <= CS / 64
  uint32_t* G = gains + (int64_t)i * M * CS;
  int win = -1;
  if (k >= 1) {
    // round k-1's winner, by every wavefront for itself: lane l folds the candidates l, l + 64, ..
    unsigned long long key = 0;
    for (int c = lane; c < C; c += SCN_PLANE) {
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
  for (int t = threadIdx.x; t < Gi * SCN_PLANE; t += SCN_THREADS) s_cnt[t] = 0;
  __syncthreads();
  unsigned long long* wi = words + (int64_t)i * HW;       // plane 0 of image i
  const int px0 = blockIdx.x * RND_PIX + threadIdx.x;
  // the winner's plane first: whether it explains each of this thread's pixels, before any plane of them is cleared
  bool hit[RND_PPT];
#pragma unroll
  for (int j = 0; j < RND_PPT; ++j) hit[j] = false;
  if (win >= 0) {
    const unsigned long long wbit = 1ull << (win % SCN_PLANE);
    const unsigned long long* ww = wi + (int64_t)(win / SCN_PLANE) * plane;
#pragma unroll
    for (int j = 0; j < RND_PPT; ++j) {
      const int px = px0 + j * SCN_THREADS;
      if (px < HW) hit[j] = (ww[px] & wbit) != 0;
    }
#pragma unroll
    for (int j = 0; j < RND_PPT; ++j) {
      const int px = px0 + j * SCN_THREADS;
      if (hit[j]) labels[(int64_t)i * HW + px] = (uint8_t)(k - 1);
    }
  }
  for (int g = 0; g < Gi; ++g) {
    unsigned long long* wp = wi + (int64_t)g * plane;
    unsigned long long wd[RND_PPT];
    bool any = false;
#pragma unroll
    for (int j = 0; j < RND_PPT; ++j) {
      const int px = px0 + j * SCN_THREADS;
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
      const int cn = C - g * SCN_PLANE < SCN_PLANE ? C - g * SCN_PLANE : SCN_PLANE;
      uint32_t acc = 0;
      for (int b = 0; b < cn; ++b) {
        const unsigned long long bit = 1ull << b;
        uint32_t n = 0;
#pragma unroll
        for (int j = 0; j < RND_PPT; ++j) n += (uint32_t)__popcll(wave_ballot((wd[j] & bit) != 0));
        acc = lane == b ? n : acc;
      }
      if (acc) atomicAdd(&s_cnt[g * SCN_PLANE + lane], acc);
    }
  }
  __syncthreads();
  if (k < M) {
    for (int t = threadIdx.x; t < C; t += SCN_THREADS) {
      const uint32_t n = s_cnt[t];
      if (n) atomicAdd(&G[k * CS + t], n);
    }
  }
}

extern "C" int64_t cppf_scene_explain_wide_workspace_bytes(int I, int H, int W, int max_rounds, int max_candidates) {
  if (I < 1 || H < 1 || W < 1 || H > SCN_MAX_DIM || W > SCN_MAX_DIM || max_rounds < 1 || max_rounds > SCN_MAX_M ||
      max_candidates < 1 || max_candidates > SCN_MAX_C)
    return 0;
  const int64_t G = (max_candidates + SCN_PLANE - 1) / SCN_PLANE;
  return G * scene_words_bytes(I, H * W) + (int64_t)I * max_rounds * G * SCN_PLANE * (int64_t)sizeof(uint32_t);
}

extern "C" int64_t cppf_scene_explain_workspace_bytes(int I, int H, int W, int max_rounds) {
  return cppf_scene_explain_wide_workspace_bytes(I, H, W, max_rounds, SCN_PLANE);
}

// CPPF_CHECK_ARG under the entry point's name.  cppf_scene_explain_wide's messages spell the limits WSC_MAX_.., as they did
// while it had constants of its own: the texts are part of what the entry points answer (tests/test_scene_wide.py).
static int scene_invalid(const char* fn, bool wide, const char* cond) {
  snprintf(g_cppf_err, sizeof(g_cppf_err), "%s: invalid argument: %s", fn, cond);
  for (char* s = g_cppf_err; wide && (s = strstr(s, "SCN_MAX_")) != nullptr;) memcpy(s, "WSC", 3);
  return CPPF_EINVAL;
}
#define SCENE_CHECK_ARG(cond)                                            \
  do {                                                                   \
    if (!(cond)) return scene_invalid(fn, MAXC > SCN_PLANE, #cond);      \
  } while (0)
#undef CPPF_FN
#define CPPF_FN fn                 // CPPF_HIP and CPPF_LAUNCH_CHECK below: under the entry point's name too

// Both entry points: fn the entry's name, MAXC the most candidates of an image it takes and the kernels it launches.
template <int MAXC>
static int scene_explain(const char* fn, int I, int H, int W, const float* depth, const uint8_t* region, const int32_t* h_cand_off,
                         int P, const float* renders, float tau, int min_gain, int viol_weight, int max_rounds, int max_candidates,
                         int32_t* chosen, int64_t* gain, int64_t* net, int64_t* stat, uint8_t* labels, int64_t* summary,
                         void* workspace, int64_t workspace_bytes, void* stream) {
  constexpr bool WIDE = MAXC > SCN_PLANE;
  SCENE_CHECK_ARG(I >= 1 && H >= 1 && W >= 1 && H <= SCN_MAX_DIM && W <= SCN_MAX_DIM);   // H * W <= 2^26: a net fits 31 bits
  SCENE_CHECK_ARG(max_rounds >= 1 && max_rounds <= SCN_MAX_M);
  SCENE_CHECK_ARG(min_gain >= 1);
  SCENE_CHECK_ARG(viol_weight >= 0);
  SCENE_CHECK_ARG(tau >= 0.0f);
  SCENE_CHECK_ARG(P >= 0 && P <= SCN_MAX_P && h_cand_off);
  SCENE_CHECK_ARG(h_cand_off[0] == 0 && h_cand_off[I] == P);
  for (int i = 0; i < I; ++i) SCENE_CHECK_ARG(h_cand_off[i] <= h_cand_off[i + 1]);
  if (max_candidates < 1 || max_candidates > MAXC) {      // the wide entry's argument; cppf_scene_explain passes 64
    snprintf(g_cppf_err, sizeof(g_cppf_err), "%s: max_candidates = %d: fewer than 1 or more than %d unsupported", fn, max_candidates,
             MAXC);
    return CPPF_EUNSUPPORTED;
  }
  for (int i = 0; i < I; ++i) {
    const int C = h_cand_off[i + 1] - h_cand_off[i];
    if (C <= max_candidates) continue;
    if (WIDE) snprintf(g_cppf_err, sizeof(g_cppf_err), "%s: invalid argument: %d candidates on image %d, max_candidates = %d", fn, C, i, max_candidates);
    else snprintf(g_cppf_err, sizeof(g_cppf_err), "%s: %d candidates on image %d, more than %d unsupported", fn, C, i, MAXC);
    return WIDE ? CPPF_EINVAL : CPPF_EUNSUPPORTED;
  }
  SCENE_CHECK_ARG(depth && region && chosen && gain && net && labels && summary && (P == 0 || (renders && stat)));
  SCENE_CHECK_ARG(workspace && (uintptr_t)workspace % 8 == 0);
  const int64_t need = cppf_scene_explain_wide_workspace_bytes(I, H, W, max_rounds, max_candidates);
  if (workspace_bytes < need) {
    snprintf(g_cppf_err, sizeof(g_cppf_err), "%s: workspace of %lld bytes, %lld needed", fn, (long long)workspace_bytes, (long long)need);
    return CPPF_ECAPACITY;
  }
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W, M = max_rounds;
  const int G = (max_candidates + SCN_PLANE - 1) / SCN_PLANE, CS = G * SCN_PLANE;
  const long long plane = (long long)(scene_words_bytes(I, HW) / 8);
  unsigned long long* words = (unsigned long long*)workspace;
  uint32_t* gains = (uint32_t*)((char*)workspace + (int64_t)G * scene_words_bytes(I, HW));
  CPPF_HIP(hipMemsetAsync(gains, 0, (size_t)I * M * CS * sizeof(uint32_t), st));
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
    int most = 0;                                         // the chunk's largest image: the planes its bits launch needs
    for (int i = 0; i <= n; ++i) img.off[i] = h_cand_off[i0 + i];
    for (int i = 0; i < n; ++i) most = img.off[i + 1] - img.off[i] > most ? img.off[i + 1] - img.off[i] : most;
    const int gz = most > SCN_PLANE ? (most + SCN_PLANE - 1) / SCN_PLANE : 1;      // 1 with MAXC = 64
    hipLaunchKernelGGL(scene_bits_kernel<MAXC>, dim3(nbx, n, gz), dim3(SCN_THREADS), 0, st, depth + (int64_t)i0 * HW,
                       region + (int64_t)i0 * HW, img, HW, renders, tau, words + (int64_t)i0 * HW, plane, (unsigned long long*)stat,
                       (unsigned long long*)summary + (int64_t)i0 * 3);
    if (img.off[0] == img.off[n]) continue;               // no candidate on these images
    for (int k = 0; k <= M; ++k) {
      if (WIDE)
        hipLaunchKernelGGL(scene_round_wide_kernel, dim3(nrx, n), dim3(SCN_THREADS), 0, st, k, M, img, HW, CS, (long long)min_gain,
                           (long long)viol_weight, (const long long*)stat, words + (int64_t)i0 * HW, plane,
                           gains + (int64_t)i0 * M * CS, chosen + (int64_t)i0 * M, (long long*)gain + (int64_t)i0 * M,
                           (long long*)net + (int64_t)i0 * M, labels + (int64_t)i0 * HW, (long long*)summary + (int64_t)i0 * 3);
      else
        hipLaunchKernelGGL(scene_round_kernel, dim3(nrx, n), dim3(SCN_THREADS), 0, st, k, M, img, HW, (long long)min_gain,
                           (long long)viol_weight, (const long long*)stat, words + (int64_t)i0 * HW,
                           gains + (int64_t)i0 * M * SCN_PLANE, chosen + (int64_t)i0 * M, (long long*)gain + (int64_t)i0 * M,
                           (long long*)net + (int64_t)i0 * M, labels + (int64_t)i0 * HW, (long long*)summary + (int64_t)i0 * 3);
    }
    CPPF_LAUNCH_CHECK();
  }
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}

extern "C" int cppf_scene_explain(int I, int H, int W, const float* depth, const uint8_t* region, const int32_t* h_cand_off, int P,
                                  const float* renders, float tau, int min_gain, int viol_weight, int max_rounds, int32_t* chosen,
                                  int64_t* gain, int64_t* net, int64_t* stat, uint8_t* labels, int64_t* summary, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  return scene_explain<SCN_PLANE>("cppf_scene_explain", I, H, W, depth, region, h_cand_off, P, renders, tau, min_gain, viol_weight,
                                  max_rounds, SCN_PLANE, chosen, gain, net, stat, labels, summary, workspace, workspace_bytes, stream);
}

extern "C" int cppf_scene_explain_wide(int I, int H, int W, const float* depth, const uint8_t* region, const int32_t* h_cand_off, int P,
                                       const float* renders, float tau, int min_gain, int viol_weight, int max_rounds,
                                       int max_candidates, int32_t* chosen, int64_t* gain, int64_t* net, int64_t* stat,
                                       uint8_t* labels, int64_t* summary, void* workspace, int64_t workspace_bytes, void* stream) {
  return scene_explain<SCN_MAX_C>("cppf_scene_explain_wide", I, H, W, depth, region, h_cand_off, P, renders, tau, min_gain,
                                  viol_weight, max_rounds, max_candidates, chosen, gain, net, stat, labels, summary, workspace,
                                  workspace_bytes, stream);
}
