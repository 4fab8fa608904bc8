// Solid-interval checks on candidate poses (not in the reference): how much of a pose's far side lies below
// the support plane, and how much of the solid of one pose lies inside the solid of another.  cppf2_amd/solid.py drives the
// entry points; tests/solid_ref.py restates them.  Integer counts only, so an image's outputs do not depend on the grid, the
// batch or the order.  gfx950 only.
//
// Per candidate c two renders of one closed mesh at one pose: f_c with back faces culled (the nearest front face) and b_c with
// the winding reversed (the nearest back face); the first solid interval along a pixel's ray is [f_c, b_c].  0 = nothing drawn.
//     back_c  = b_c > 0
//     solid_c = f_c > 0 && b_c > 0
//     open_c  = (f_c > 0) != (b_c > 0)                       (the mesh is not closed there: counted, never used)
//   (comparisons with 0 in float32; NaN compares false, -0.0 is not > 0, +inf is.)
// Support: plane (n, d) and Kmat (fx, fy, cx, cy) of the image, pixel (r, c) at the renderer's centre, z = b_c, float32, every
// operation rounded where it is written:
//     x = ((((float)c + 0.5f) - cx) * z) / fx,  y = ((((float)r + 0.5f) - cy) * z) / fy,  h = ((n.x*x + n.y*y) + n.z*z) + d
//     sunk_c = back_c && h < -tau                            (a plane of zeros gives h = 0 or NaN, a NaN plane NaN: neither sinks)
//   counts[p] = (back, sunk, solid, open) of render pair p = cand_off[i] + c.
// Overlap, for the C_i <= 64 candidates of image i, on pixels where a and c are both solid:
//     lo = fmaxf(f_a, f_c), hi = fminf(b_a, b_c); the pixel counts iff (double)hi - (double)lo > (double)tau
//   inter[cand_off[i] + a][j] = that count for (a, j), j < C_i; inter[..][a] = the solid pixels of a; columns C_i .. 63 are 0.
//
// cppf_support_counts: grid (ceil(H*W / SLD_PIX), images) per chunk of SLD_IMGS images (their candidate offsets go by value),
//   256 threads: a lane keeps the ray factors of its SLD_PPT pixels in registers and reads each pair of renders once.  Four
//   ballots per candidate and pixel row; the wavefront's counts of candidate c stay with lane c mod 64; after every 64
//   candidates the four wavefronts meet in LDS and the block adds its non-zero sums with one 64-bit integer atomic per count.
// cppf_solid_overlap: solid_bits_kernel (the same grid) writes one 64-bit word per pixel, bit j = solid_j, and the diagonal;
//   solid_pairs_kernel (the same grid) reads the words: a block without a word of two bits returns; a wavefront with one takes
//   the union of such words and walks that union's bits pairwise -- a's renders in registers, c's read once per pair -- the
//   ballot's population count goes to a 64 x 64 table in LDS, and the block issues one integer atomic per non-zero pair and side.
//   workspace: the words, 8 bytes per pixel.
#include "cppf_common.h"

#define SLD_THREADS 256
#define SLD_PPT 8                  // pixels per thread
#define SLD_PIX (SLD_THREADS * SLD_PPT)
#define SLD_WAVES (SLD_THREADS / CPPF_WAVE)
#define SLD_MAX_C 64               // candidates per image of the overlap test: one bit each
#define SLD_IMGS 128               // images per launch (their candidate offsets go by value)
#define SLD_MAX_DIM 8192           // H, W (the renderer's limit): H * W <= 2^26
#define SLD_MAX_P (1 << 24)

struct SolidImages {
  int32_t off[SLD_IMGS + 1];       // global candidate offsets of the launch's images
};

static int64_t solid_words_bytes(int I, int HW) { return align_up((int64_t)I * HW * 8, 256); }

__global__ __launch_bounds__(SLD_THREADS) void support_counts_kernel(SolidImages img, int HW, int W, const float* __restrict__ front,
                                                                     const float* __restrict__ back,
                                                                     const float* __restrict__ planes, const float* __restrict__ Kmat,
                                                                     float tau, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t s_c[SLD_WAVES][4][CPPF_WAVE];
  const int i = blockIdx.y;
  const int p0 = img.off[i], p1 = img.off[i + 1];        // the same for the whole block
  if (p0 == p1) return;
  const int px0 = blockIdx.x * SLD_PIX + threadIdx.x;
  const int lane = wave_lane(), w = threadIdx.x / CPPF_WAVE;
  const float nx = planes[4 * i], ny = planes[4 * i + 1], nz = planes[4 * i + 2], d = planes[4 * i + 3];
  const float fx = Kmat[4 * i], fy = Kmat[4 * i + 1], cx = Kmat[4 * i + 2], cy = Kmat[4 * i + 3];
  const float neg_tau = -tau;
  float rx[SLD_PPT], ry[SLD_PPT];                         // the pixel's ray factors, once per lane
#pragma unroll
  for (int j = 0; j < SLD_PPT; ++j) {
    const int px = px0 + j * SLD_THREADS;
    const int r = px / W, c = px - r * W;
    rx[j] = ((float)c + 0.5f) - cx;
    ry[j] = ((float)r + 0.5f) - cy;
  }
  for (int g0 = p0; g0 < p1; g0 += CPPF_WAVE) {           // 64 candidates at a time: candidate c's counts with lane c mod 64
    const int g1 = g0 + CPPF_WAVE < p1 ? g0 + CPPF_WAVE : p1;
    uint32_t a_back = 0, a_sunk = 0, a_solid = 0, a_open = 0;
    for (int p = g0; p < g1; ++p) {
      const float* fc = front + (int64_t)p * HW;
      const float* bc = back + (int64_t)p * HW;
      uint32_t n_back = 0, n_sunk = 0, n_solid = 0, n_open = 0;
#pragma unroll
      for (int j = 0; j < SLD_PPT; ++j) {
        const int px = px0 + j * SLD_THREADS;
        const float f = px < HW ? fc[px] : 0.0f;
        const float z = px < HW ? bc[px] : 0.0f;
        const float x = (rx[j] * z) / fx;
        const float y = (ry[j] * z) / fy;
        const float h = ((nx * x + ny * y) + nz * z) + d;
        const bool isf = f > 0.0f, isb = z > 0.0f;
        n_back += (uint32_t)__popcll(wave_ballot(isb));
        n_sunk += (uint32_t)__popcll(wave_ballot(isb && h < neg_tau));
        n_solid += (uint32_t)__popcll(wave_ballot(isf && isb));
        n_open += (uint32_t)__popcll(wave_ballot(isf != isb));
      }
      const bool mine = lane == p - g0;
      a_back = mine ? n_back : a_back;
      a_sunk = mine ? n_sunk : a_sunk;
      a_solid = mine ? n_solid : a_solid;
      a_open = mine ? n_open : a_open;
    }
    s_c[w][0][lane] = a_back;
    s_c[w][1][lane] = a_sunk;
    s_c[w][2][lane] = a_solid;
    s_c[w][3][lane] = a_open;
    __syncthreads();
    {                                                     // thread t: count t / 64 of candidate g0 + t % 64
      const int q = threadIdx.x / CPPF_WAVE, c = threadIdx.x % CPPF_WAVE;
      unsigned long long s = 0;
#pragma unroll
      for (int k = 0; k < SLD_WAVES; ++k) s += s_c[k][q][c];
      if (g0 + c < g1 && s) atomicAdd(&counts[(int64_t)(g0 + c) * 4 + q], s);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(SLD_THREADS) void solid_bits_kernel(SolidImages img, int HW, const float* __restrict__ front,
                                                                 const float* __restrict__ back,
                                                                 unsigned long long* __restrict__ words,
                                                                 unsigned long long* __restrict__ inter) {
  __shared__ uint32_t s_c[SLD_WAVES][SLD_MAX_C];
  const int i = blockIdx.y;
  const int p0 = img.off[i], p1 = img.off[i + 1];        // the same for the whole block; p1 - p0 <= 64
  if (p0 == p1) return;
  const int px0 = blockIdx.x * SLD_PIX + threadIdx.x;
  const int lane = wave_lane(), w = threadIdx.x / CPPF_WAVE;
  unsigned long long bits[SLD_PPT];
#pragma unroll
  for (int j = 0; j < SLD_PPT; ++j) bits[j] = 0;
  uint32_t a_solid = 0;                                   // lane c: the wavefront's solid pixels of candidate c
  for (int p = p0; p < p1; ++p) {
    const unsigned long long bit = 1ull << (p - p0);
    const float* fc = front + (int64_t)p * HW;
    const float* bc = back + (int64_t)p * HW;
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < SLD_PPT; ++j) {
      const int px = px0 + j * SLD_THREADS;
      const float f = px < HW ? fc[px] : 0.0f;
      const float b = px < HW ? bc[px] : 0.0f;
      const bool solid = f > 0.0f && b > 0.0f;
      n += (uint32_t)__popcll(wave_ballot(solid));
      bits[j] |= solid ? bit : 0ull;
    }
    a_solid = lane == p - p0 ? n : a_solid;
  }
  s_c[w][lane] = a_solid;
#pragma unroll
  for (int j = 0; j < SLD_PPT; ++j) {
    const int px = px0 + j * SLD_THREADS;
    if (px < HW) words[(int64_t)i * HW + px] = bits[j];
  }
  __syncthreads();
  if (threadIdx.x < p1 - p0) {
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < SLD_WAVES; ++k) s += s_c[k][threadIdx.x];
    if (s) atomicAdd(&inter[(int64_t)(p0 + threadIdx.x) * SLD_MAX_C + threadIdx.x], s);
  }
}

__global__ __launch_bounds__(SLD_THREADS) void solid_pairs_kernel(SolidImages img, int HW, const float* __restrict__ front,
                                                                  const float* __restrict__ back, float tau,
                                                                  const unsigned long long* __restrict__ words,
                                                                  unsigned long long* __restrict__ inter) {
  __shared__ uint32_t s_pair[SLD_MAX_C * SLD_MAX_C];      // [a][c], a < c
  __shared__ unsigned long long s_union[SLD_WAVES];
  const int i = blockIdx.y;
  const int p0 = img.off[i];
  const int C = img.off[i + 1] - p0;                      // the same for the whole block, like the return below
  if (C < 2) return;
  const int px0 = blockIdx.x * SLD_PIX + threadIdx.x;
  const int lane = wave_lane(), w = threadIdx.x / CPPF_WAVE;
  const double tau_d = (double)tau;
  unsigned long long wd[SLD_PPT];
  unsigned long long mine = 0;                            // the union of this lane's words of two bits or more
#pragma unroll
  for (int j = 0; j < SLD_PPT; ++j) {
    const int px = px0 + j * SLD_THREADS;
    unsigned long long v = px < HW ? words[(int64_t)i * HW + px] : 0ull;
    v = (v & (v - 1)) ? v : 0ull;                         // a word of fewer than two bits has no pair
    wd[j] = v;
    mine |= v;
  }
  if (!__syncthreads_or(mine != 0)) return;               // most of an image: no two solids meet in this block
  for (int t = threadIdx.x; t < SLD_MAX_C * SLD_MAX_C; t += SLD_THREADS) s_pair[t] = 0;
  if (lane == 0) s_union[w] = 0;
  __syncthreads();
  if (mine) atomicOr(&s_union[w], mine);
  __syncthreads();
  const unsigned long long u_all = s_union[w];            // the same in every lane of the wavefront
  const unsigned long long un = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u_all >> 32)) << 32) |
                                (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u_all);
  for (unsigned long long ma = un; ma & (ma - 1); ma &= ma - 1) {
    const int a = __builtin_ctzll(ma);
    const float* fa_p = front + (int64_t)(p0 + a) * HW;
    const float* ba_p = back + (int64_t)(p0 + a) * HW;
    float fa[SLD_PPT], ba[SLD_PPT];
#pragma unroll
    for (int j = 0; j < SLD_PPT; ++j) {
      const int px = px0 + j * SLD_THREADS;
      const bool has = (wd[j] >> a) & 1ull;               // only then px < HW
      fa[j] = has ? fa_p[px] : 0.0f;
      ba[j] = has ? ba_p[px] : 0.0f;
    }
    for (unsigned long long mc = ma & (ma - 1); mc; mc &= mc - 1) {
      const int c = __builtin_ctzll(mc);
      const float* fc_p = front + (int64_t)(p0 + c) * HW;
      const float* bc_p = back + (int64_t)(p0 + c) * HW;
      uint32_t n = 0;
#pragma unroll
      for (int j = 0; j < SLD_PPT; ++j) {
        const int px = px0 + j * SLD_THREADS;
        const bool both = ((wd[j] >> a) & (wd[j] >> c) & 1ull) != 0;
        bool in = false;
        if (both) {
          const float lo = fmaxf(fa[j], fc_p[px]);
          const float hi = fminf(ba[j], bc_p[px]);
          in = (double)hi - (double)lo > tau_d;
        }
        n += (uint32_t)__popcll(wave_ballot(in));
      }
      if (n && lane == 0) atomicAdd(&s_pair[a * SLD_MAX_C + c], n);
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < SLD_MAX_C * SLD_MAX_C; t += SLD_THREADS) {
    const uint32_t n = s_pair[t];
    if (n) {                                              // only a < c < C was ever added to
      const int a = t / SLD_MAX_C, c = t % SLD_MAX_C;
      atomicAdd(&inter[(int64_t)(p0 + a) * SLD_MAX_C + c], (unsigned long long)n);
      atomicAdd(&inter[(int64_t)(p0 + c) * SLD_MAX_C + a], (unsigned long long)n);
    }
  }
}

// the checks both entry points share: sizes, offsets, P
#define SLD_CHECK_COMMON()                                                                              \
  CPPF_CHECK_ARG(I >= 1 && H >= 1 && W >= 1 && H <= SLD_MAX_DIM && W <= SLD_MAX_DIM);                    \
  CPPF_CHECK_ARG(tau >= 0.0f);                                                                          \
  CPPF_CHECK_ARG(P >= 0 && P <= SLD_MAX_P && h_cand_off);                                               \
  CPPF_CHECK_ARG(h_cand_off[0] == 0 && h_cand_off[I] == P);                                             \
  for (int i = 0; i < I; ++i) CPPF_CHECK_ARG(h_cand_off[i] <= h_cand_off[i + 1])

extern "C" int cppf_support_counts(int I, int H, int W, const float* front, const float* back, const int32_t* h_cand_off, int P,
                                   const float* planes, const float* Kmat, float tau, int64_t* counts, void* stream) {
  SLD_CHECK_COMMON();
  CPPF_CHECK_ARG(planes && Kmat && (P == 0 || (front && back && counts)));
  if (P == 0) return CPPF_OK;
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W;
  CPPF_HIP(hipMemsetAsync(counts, 0, (size_t)P * 4 * sizeof(int64_t), st));
  const int nbx = (HW + SLD_PIX - 1) / SLD_PIX;
  for (int i0 = 0; i0 < I; i0 += SLD_IMGS) {
    const int n = I - i0 < SLD_IMGS ? I - i0 : SLD_IMGS;
    SolidImages img;
    for (int i = 0; i <= n; ++i) img.off[i] = h_cand_off[i0 + i];
    if (img.off[0] == img.off[n]) continue;               // no candidate on these images
    hipLaunchKernelGGL(support_counts_kernel, dim3(nbx, n), dim3(SLD_THREADS), 0, st, img, HW, W, front, back,
                       planes + (int64_t)i0 * 4, Kmat + (int64_t)i0 * 4, tau, (unsigned long long*)counts);
    CPPF_LAUNCH_CHECK();
  }
  return CPPF_OK;
}

extern "C" int64_t cppf_solid_overlap_workspace_bytes(int I, int H, int W) {
  if (I < 1 || H < 1 || W < 1 || H > SLD_MAX_DIM || W > SLD_MAX_DIM) return 0;
  return solid_words_bytes(I, H * W);
}

extern "C" int cppf_solid_overlap(int I, int H, int W, const float* front, const float* back, const int32_t* h_cand_off, int P,
                                  float tau, int64_t* inter, void* workspace, int64_t workspace_bytes, void* stream) {
  SLD_CHECK_COMMON();
  for (int i = 0; i < I; ++i) {
    if (h_cand_off[i + 1] - h_cand_off[i] > SLD_MAX_C) {
      snprintf(g_cppf_err, sizeof(g_cppf_err), "cppf_solid_overlap: %d candidates on image %d, more than %d unsupported",
               h_cand_off[i + 1] - h_cand_off[i], i, SLD_MAX_C);
      return CPPF_EUNSUPPORTED;
    }
  }
  CPPF_CHECK_ARG(P == 0 || (front && back && inter));
  CPPF_CHECK_ARG(workspace && (uintptr_t)workspace % 8 == 0);
  if (workspace_bytes < cppf_solid_overlap_workspace_bytes(I, H, W)) {
    snprintf(g_cppf_err, sizeof(g_cppf_err), "cppf_solid_overlap: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
             (long long)cppf_solid_overlap_workspace_bytes(I, H, W));
    return CPPF_ECAPACITY;
  }
  if (P == 0) return CPPF_OK;
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W;
  unsigned long long* words = (unsigned long long*)workspace;
  CPPF_HIP(hipMemsetAsync(inter, 0, (size_t)P * SLD_MAX_C * sizeof(int64_t), st));
  const int nbx = (HW + SLD_PIX - 1) / SLD_PIX;
  for (int i0 = 0; i0 < I; i0 += SLD_IMGS) {
    const int n = I - i0 < SLD_IMGS ? I - i0 : SLD_IMGS;
    SolidImages img;
    for (int i = 0; i <= n; ++i) img.off[i] = h_cand_off[i0 + i];
    if (img.off[0] == img.off[n]) continue;               // no candidate on these images
    hipLaunchKernelGGL(solid_bits_kernel, dim3(nbx, n), dim3(SLD_THREADS), 0, st, img, HW, front, back,
                       words + (int64_t)i0 * HW, (unsigned long long*)inter);
    CPPF_LAUNCH_CHECK();
    hipLaunchKernelGGL(solid_pairs_kernel, dim3(nbx, n), dim3(SLD_THREADS), 0, st, img, HW, front, back, tau,
                       (const unsigned long long*)(words + (int64_t)i0 * HW), (unsigned long long*)inter);
    CPPF_LAUNCH_CHECK();
  }
  return CPPF_OK;
}
