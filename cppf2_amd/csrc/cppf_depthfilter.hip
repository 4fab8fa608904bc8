// Conditioning of sensor depth before anything else reads it: mixed ("flying") pixels along depth discontinuities are dropped,
// and what is left can be smoothed within its surface (cppf2_amd/depthfilter.py).  The reference takes
// a depth image as it comes from the file and has no such step.  gfx950 only.  tests/depth_condition_ref.py restates every
// definition below in NumPy; the build's -ffp-contract=off keeps every operation where it is written (no fused multiply-add
// anywhere in this file) and the float32 divide is correctly rounded.
//
// cppf_depth_condition: depth float32 [I,H,W] (metres) -> out float32 [I,H,W], counts int32 [I,3].  Parameters r1, min_support,
// r2, jump, jump_rel.  In the order of the float32 operations:
//   valid(q)    q is finite and > 0, decided on the bits: 0 < bits(q) < 0x7f800000 as int32 (a denormal is valid; NaN, the
//               infinities, negatives and both zeros are not)
//   tol(z)      jump + (jump_rel * z): the product is rounded, then the sum
//   near(q, z)  fabsf(q - z) <= tol(z), z always the CENTRE pixel's reading
//   stage 1     (flying pixels) for a valid pixel p with reading z: support = the number of offsets (dy, dx) != (0, 0) of
//               [-r1, r1]^2 whose position lies outside the image, or whose reading q is valid and near(q, z);
//               d1(p) = support >= min_support ? z : 0.  An invalid p gives 0.  Stage 1 reads the input only and is not iterated.
//               With r1 = 0 there is no offset: support = 0, and min_support = 0 keeps every valid pixel.
//   stage 2     (smoothing within a surface) on d1, never on the input.  For p with d1(p) > 0 and z = d1(p): s = z, n = 1; then
//               the offsets o of the first half of the window in row-major order -- dy = -r2 .. -1 with dx = -r2 .. r2, then
//               dy = 0 with dx = -r2 .. -1 --: a = d1(p + o), b = d1(p - o); if both positions lie inside the image, a > 0,
//               b > 0, near(a, z) and near(b, z): s = (s + a) + b, n += 2.  out(p) = s / (float)n; 0 where d1(p) = 0.
//               Opposite neighbours enter together or not at all: the mean has no bias on a slanted surface however the gate
//               clips the window.  r2 = 0: out = d1.
//   counts[i]   (valid readings of image i, valid readings with d1 = 0, pixels with n > 1)
//
// One launch for all I images after the counts are cleared: grid (tiles of an image, min(I, 65535)), 256 threads; block
// (t, j) serves tile t of the images j, j + gridDim.y, ...  A tile is DF_TH x DF_TW = 16 x 64 pixels.
//   stage   the tile's readings plus a halo of r1 + r2 go to s_raw, normalised: a valid reading as it is, an invalid one 0, a
//           position outside the image -1 (a sign test tells it from both).  One global read per pixel plus the halo.
//   d1      every position of the tile plus a halo of r2 gets its stage-1 value in s_d1 (0 outside the image, so that stage 2's
//           "inside the image" is d1 > 0).  The threads walk the positions in linear order; s_d1's pitch is the region's width
//           dw and s_raw's pitch is dw + 32, so the 32 lanes of a half-wavefront always touch 32 consecutive banks, row
//           wraps included: ds_read_b32 / ds_write_b32 bank = (address / 4) mod 32 per half-wavefront.
//   smooth  wavefront w takes the tile's rows w, w + 4, w + 8, w + 12, its lanes the 64 columns: every window read is 64
//           consecutive floats of a row of s_d1, free of bank conflicts.  One global write per pixel.
//   counts  three ballots per row, popcounts; the four wavefronts' sums meet in LDS and thread 0 adds each to the image's
//           integer with one vector atomic add.  Integer sums do not depend on the order.
// LDS: 32 x 104 + 24 x 72 floats = 20 KiB at the largest radii.  No scratch memory, no workspace, no host synchronisation.
#include "cppf_common.h"

#define DF_THREADS 256
#define DF_TW 64                          // tile width: one wavefront per row
#define DF_TH 16                          // tile height: four rows per wavefront
#define DF_MAX_R 4                        // r1, r2
#define DF_MAX_DIM 16384                  // H, W
#define DF_MAX_GRID_Y 65535
#define DF_D1_W (DF_TW + 2 * DF_MAX_R)
#define DF_D1_H (DF_TH + 2 * DF_MAX_R)
#define DF_RAW_P (DF_D1_W + 32)           // pitch of s_raw at the largest r2
#define DF_RAW_H (DF_TH + 4 * DF_MAX_R)

__device__ __forceinline__ bool df_valid_bits(int32_t b) { return b > 0 && b < 0x7f800000; }

__global__ __launch_bounds__(DF_THREADS) void depth_condition_kernel(const float* __restrict__ depth, int I, int H, int W,
                                                                     int tiles_x, int r1, int min_support, int r2, float jump,
                                                                     float jump_rel, float* __restrict__ out,
                                                                     int* __restrict__ counts) {
  __shared__ float s_raw[DF_RAW_H * DF_RAW_P];
  __shared__ float s_d1[DF_D1_H * DF_D1_W];
  __shared__ uint32_t s_cnt[3][DF_THREADS / CPPF_WAVE];
  const int R = r1 + r2;
  const int rh = DF_TH + 2 * R, rw = DF_TW + 2 * R;           // the staged readings
  const int dh = DF_TH + 2 * r2, dw = DF_TW + 2 * r2;         // the stage-1 values
  const int rp = dw + 32;                                     // s_raw's pitch: >= rw, and = dw modulo the 32 banks
  const int tile_y = blockIdx.x / tiles_x;
  const int y0 = tile_y * DF_TH, x0 = (blockIdx.x - tile_y * tiles_x) * DF_TW;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / CPPF_WAVE), lane = wave_lane();
  const int64_t HW = (int64_t)H * W;
  for (int i = blockIdx.y; i < I; i += gridDim.y) {
    const int32_t* src = reinterpret_cast<const int32_t*>(depth) + i * HW;
    float* dst = out + i * HW;
    for (int k = threadIdx.x; k < rh * rw; k += DF_THREADS) {
      const int row = k / rw, col = k - row * rw;
      const int y = y0 - R + row, x = x0 - R + col;
      float v = -1.0f;
      if (y >= 0 && y < H && x >= 0 && x < W) {
        const int32_t b = src[(int64_t)y * W + x];
        v = df_valid_bits(b) ? __int_as_float(b) : 0.0f;
      }
      s_raw[row * rp + col] = v;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < dh * dw; k += DF_THREADS) {
      const int row = k / dw, col = k - row * dw;
      const float* c = s_raw + (row + r1) * rp + (col + r1);
      const float z = *c;
      float d = 0.0f;
      if (__float_as_int(z) > 0) {
        const float tol = jump + (jump_rel * z);
        int support = 0;
        for (int dy = -r1; dy <= r1; ++dy)
          for (int dx = -r1; dx <= r1; ++dx) {
            const float q = c[dy * rp + dx];
            const int32_t qb = __float_as_int(q);
            const bool sup = qb < 0 || (qb > 0 && fabsf(q - z) <= tol);
            support += (sup && (dy | dx) != 0) ? 1 : 0;
          }
        d = support >= min_support ? z : 0.0f;
      }
      s_d1[k] = d;
    }
    __syncthreads();
    uint32_t n_valid = 0, n_removed = 0, n_smoothed = 0;
#pragma unroll
    for (int k = 0; k < DF_TH / (DF_THREADS / CPPF_WAVE); ++k) {
      const int ly = wave + k * (DF_THREADS / CPPF_WAVE);
      const int y = y0 + ly, x = x0 + lane;
      const bool was_valid = __float_as_int(s_raw[(ly + R) * rp + (lane + R)]) > 0;      // -1 outside the image
      const float* c = s_d1 + (ly + r2) * dw + (lane + r2);
      const float z = *c;
      const bool kept = __float_as_int(z) > 0;
      float o = 0.0f;
      int n = 1;
      if (kept) {
        const float tol = jump + (jump_rel * z);
        float s = z;
        for (int dy = -r2; dy <= 0; ++dy) {
          const int last = dy < 0 ? r2 : -1;
          for (int dx = -r2; dx <= last; ++dx) {
            const int off = dy * dw + dx;
            const float a = c[off], b = c[-off];
            if (__float_as_int(a) > 0 && __float_as_int(b) > 0 && fabsf(a - z) <= tol && fabsf(b - z) <= tol) {
              s = (s + a) + b;
              n += 2;
            }
          }
        }
        o = s / (float)n;
      }
      if (y < H && x < W) dst[(int64_t)y * W + x] = o;
      n_valid += (uint32_t)__popcll(wave_ballot(was_valid));
      n_removed += (uint32_t)__popcll(wave_ballot(was_valid && !kept));
      n_smoothed += (uint32_t)__popcll(wave_ballot(n > 1));
    }
    if (lane == 0) {
      s_cnt[0][wave] = n_valid;
      s_cnt[1][wave] = n_removed;
      s_cnt[2][wave] = n_smoothed;
    }
    __syncthreads();                                          // also: every read of s_raw and s_d1 is done before the next image
    if (threadIdx.x == 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < DF_THREADS / CPPF_WAVE; ++w) s += s_cnt[j][w];
        if (s) atomicAdd(&counts[3 * (int64_t)i + j], (int)s);
      }
    }
    __syncthreads();                                          // s_cnt is read before the next image's sums are written
  }
}

extern "C" int cppf_depth_condition(const float* depth, int I, int H, int W, int r1, int min_support, int r2, float jump,
                                    float jump_rel, float* out, int32_t* counts, void* stream) {
  CPPF_CHECK_ARG(I >= 0 && H >= 1 && W >= 1 && H <= DF_MAX_DIM && W <= DF_MAX_DIM);
  CPPF_CHECK_ARG(r1 >= 0 && r1 <= DF_MAX_R && r2 >= 0 && r2 <= DF_MAX_R);
  CPPF_CHECK_ARG(min_support >= 0 && min_support <= (2 * r1 + 1) * (2 * r1 + 1));
  CPPF_CHECK_ARG(jump >= 0.0f && jump < __builtin_inff() && jump_rel >= 0.0f && jump_rel < __builtin_inff());
  if (I == 0) return CPPF_OK;
  CPPF_CHECK_ARG(depth && out && counts);
  const uintptr_t bytes = (uintptr_t)I * H * W * sizeof(float);
  // stage 1 reads neighbours: the operation cannot run in place (out == depth), nor on any other overlap
  CPPF_CHECK_ARG((uintptr_t)out + bytes <= (uintptr_t)depth || (uintptr_t)depth + bytes <= (uintptr_t)out);
  hipStream_t st = (hipStream_t)stream;
  CPPF_HIP(hipMemsetAsync(counts, 0, (size_t)I * 3 * sizeof(int32_t), st));
  const int tiles_x = (W + DF_TW - 1) / DF_TW, tiles_y = (H + DF_TH - 1) / DF_TH;      // <= 256 * 1024 tiles
  hipLaunchKernelGGL(depth_condition_kernel, dim3(tiles_x * tiles_y, I < DF_MAX_GRID_Y ? I : DF_MAX_GRID_Y), dim3(DF_THREADS), 0,
                     st, depth, I, H, W, tiles_x, r1, min_support, r2, jump, jump_rel, out, (int*)counts);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
