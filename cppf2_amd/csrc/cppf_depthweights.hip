// A weight per depth reading by its viewing angle, as a small integer: what lets the fusion count a reading taken face-on more
// than one taken at a grazing angle without changing the volume's layout (cppf2_amd/depthweights.py, cppf_tsdf_integrate_weighted
// in cppf_fuse.hip).  The reference has no such step.  gfx950 only.  tests/depth_weights_ref.py restates
// every definition below in NumPy; the build's -ffp-contract=off keeps every operation where it is written (no fused
// multiply-add anywhere in this file) and the float32 divide and square root are correctly rounded.
//
// cppf_depth_weights: depth float32 [I,H,W] (metres), camera (fx, fy, cx, cy) and pixel_offset po as float32 -> weights uint8
// [I,H,W], counts int32 [I,3].  Parameters step s (1..4), jump, jump_rel, levels L (1..255), cos_min.  In the order of the
// float32 operations:
//   valid(q)    q is finite and > 0, decided on the bits: 0 < bits(q) < 0x7f800000 as int32 (cppf_depth_condition's)
//   tol(z)      jump + (jump_rel * z): the product is rounded, then the sum
//   near(q, z)  fabsf(q - z) <= tol(z), z always the CENTRE pixel's reading
//   ux(c)       (((float)c + po) - cx) / fx;   uy(r) = (((float)r + po) - cy) / fy
//   P(c, r, d)  (ux(c) * d, uy(r) * d, d)
//   a valid pixel (c, r) with reading z gets weight 0 unless (c - s, r), (c + s, r), (c, r - s), (c, r + s) all lie inside the
//   image and hold valid readings near z.  Otherwise, with p = P(c, r, z):
//     tx = P(c + s, r, right) - P(c - s, r, left),  ty = P(c, r + s, down) - P(c, r - s, up)        component by component
//     n  = (tx.y*ty.z - tx.z*ty.y,  tx.z*ty.x - tx.x*ty.z,  tx.x*ty.y - tx.y*ty.x)                 two products, one difference
//     a  = (n.x*p.x + n.y*p.y) + n.z*p.z;   nn = (n.x*n.x + n.y*n.y) + n.z*n.z;   pp = (p.x*p.x + p.y*p.y) + p.z*p.z
//     den = nn * pp;                        weight 0 unless den > 0 and den < +inf
//     c  = sqrtf((a * a) / den)             the cosine between the pixel's ray and the surface normal
//                                           weight 0 unless c >= cos_min
//     t  = floorf(c * (float)L + 0.5f);     weight = L if t >= (float)L, else (int)t if t >= 1, else 1
//   an invalid pixel gets 0.
//   counts[i]   (valid readings of image i, valid readings with weight 0, readings with weight L)
//
// One launch for all I images after the counts are cleared: grid (tiles of an image, min(I, 65535)), 256 threads; block (t, j)
// serves tile t of the images j, j + gridDim.y, ...  A tile is DW_TH x DW_TW = 16 x 64 pixels.
//   stage   the tile's readings plus a halo of s go to s_raw, normalised: a valid reading as it is, an invalid one 0, a position
//           outside the image -1 (a sign test tells it from both).  The threads walk the region in linear order and its pitch is
//           its width, so a half-wavefront's 32 ds_write_b32 touch 32 consecutive banks.  One global read per pixel plus the halo.
//   weigh   wavefront w takes the tile's rows w, w + 4, w + 8, w + 12, its lanes the 64 columns: each of the five reads is 64
//           consecutive floats of a row of s_raw, free of bank conflicts.  ux of a lane's three columns is computed once per
//           block; uy of the wavefront's four rows and their neighbours, twelve values that every lane shares, in one
//           division spread over twelve lanes and read back with v_readlane.
//   store   one byte per pixel would be 64 single-byte stores per row.  A lane whose byte address is a multiple of 4 fetches
//           the weights of the three lanes after it (three shifts across the wavefront) and writes all four with ONE 32-bit
//           store, if the four columns lie inside the image; the lanes it covers write nothing.  What is left -- up to three
//           pixels before the row's first aligned address, the ragged tail of a row, and the last lanes of the tile's 64 when
//           the alignment splits a group across two tiles -- goes out as single bytes.  Which lanes lead is the same for the
//           whole wavefront's row: it depends on the row's address modulo 4 only.
//   counts  three ballots per row, popcounts; the four wavefronts' sums meet in LDS and thread 0 adds each to the image's
//           integer with one vector atomic add.  Integer sums do not depend on the order.
// LDS: 24 x 72 floats = 6.75 KiB at the largest step.  No scratch memory, no workspace, no host synchronisation.
#include "cppf_common.h"

#define DW_THREADS 256
#define DW_TW 64                          // tile width: one wavefront per row
#define DW_TH 16                          // tile height: four rows per wavefront
#define DW_MAX_STEP 4
#define DW_MAX_LEVELS 255
#define DW_MAX_DIM 16384                  // H, W
#define DW_MAX_GRID_Y 65535
#define DW_RAW_W (DW_TW + 2 * DW_MAX_STEP)
#define DW_RAW_H (DW_TH + 2 * DW_MAX_STEP)

__global__ __launch_bounds__(DW_THREADS) void depth_weights_kernel(const float* __restrict__ depth, int I, int H, int W, int tiles_x,
                                                                   float fx, float fy, float cx, float cy, float po, int s,
                                                                   float jump, float jump_rel, int L, float cos_min,
                                                                   uint8_t* __restrict__ weights, int* __restrict__ counts) {
  __shared__ float s_raw[DW_RAW_H * DW_RAW_W];
  __shared__ uint32_t s_cnt[3][DW_THREADS / CPPF_WAVE];
  const int rh = DW_TH + 2 * s, rw = DW_TW + 2 * s;           // the staged readings; rw is s_raw's pitch
  const int tile_y = blockIdx.x / tiles_x;
  const int y0 = tile_y * DW_TH, x0 = (blockIdx.x - tile_y * tiles_x) * DW_TW;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / CPPF_WAVE), lane = wave_lane();
  const int64_t HW = (int64_t)H * W;
  const int x = x0 + lane;
  const float fL = (float)L;
  const float ux_l = (((float)(x - s) + po) - cx) / fx, ux_c = (((float)x + po) - cx) / fx, ux_r = (((float)(x + s) + po) - cx) / fx;
  // uy of the wavefront's four rows and their neighbours above and below: twelve values, the same for every lane, so lane
  // 3 k + j computes row k's (j = 0: up, 1: centre, 2: down) in ONE division and the rows read them back lane by lane
  const int uy_k = lane / 3, uy_j = lane - 3 * uy_k;
  const float uy_all = (((float)(y0 + wave + uy_k * (DW_THREADS / CPPF_WAVE) + (uy_j - 1) * s) + po) - cy) / fy;
  for (int i = blockIdx.y; i < I; i += gridDim.y) {
    const int32_t* src = reinterpret_cast<const int32_t*>(depth) + i * HW;
    uint8_t* dst = weights + i * HW;
    for (int k = threadIdx.x; k < rh * rw; k += DW_THREADS) {
      const int row = k / rw, col = k - row * rw;
      const int yy = y0 - s + row, xx = x0 - s + col;
      float v = -1.0f;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
        const int32_t b = src[(int64_t)yy * W + xx];
        v = (b > 0 && b < 0x7f800000) ? __int_as_float(b) : 0.0f;
      }
      s_raw[k] = v;
    }
    __syncthreads();
    uint32_t n_valid = 0, n_zero = 0, n_full = 0;
#pragma unroll
    for (int k = 0; k < DW_TH / (DW_THREADS / CPPF_WAVE); ++k) {
      const int ly = wave + k * (DW_THREADS / CPPF_WAVE);
      const int y = y0 + ly;
      const float* c = s_raw + (ly + s) * rw + (lane + s);
      const float z = *c;
      const bool valid = __float_as_int(z) > 0;               // -1 outside the image
      const float uy_u = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(uy_all), 3 * k)),
                  uy_c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(uy_all), 3 * k + 1)),
                  uy_d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(uy_all), 3 * k + 2));
      int w = 0;
      if (valid) {
        const float tol = jump + (jump_rel * z);
        const float ql = c[-s], qr = c[s], qu = c[-s * rw], qd = c[s * rw];
        const bool all_near = __float_as_int(ql) > 0 && __float_as_int(qr) > 0 && __float_as_int(qu) > 0 && __float_as_int(qd) > 0 &&
                              fabsf(ql - z) <= tol && fabsf(qr - z) <= tol && fabsf(qu - z) <= tol && fabsf(qd - z) <= tol;
        if (all_near) {
          const float px = ux_c * z, py = uy_c * z, pz = z;
          const float txx = ux_r * qr - ux_l * ql, txy = uy_c * qr - uy_c * ql, txz = qr - ql;
          const float tyx = ux_c * qd - ux_c * qu, tyy = uy_d * qd - uy_u * qu, tyz = qd - qu;
          const float nx = txy * tyz - txz * tyy, ny = txz * tyx - txx * tyz, nz = txx * tyy - txy * tyx;
          const float a = (nx * px + ny * py) + nz * pz;
          const float nn = (nx * nx + ny * ny) + nz * nz;
          const float pp = (px * px + py * py) + pz * pz;
          const float den = nn * pp;
          if (den > 0.0f && den < __builtin_inff()) {
            const float cosv = sqrtf((a * a) / den);
            if (cosv >= cos_min) {
              const float t = floorf(cosv * fL + 0.5f);
              w = t >= fL ? L : (t >= 1.0f ? (int)t : 1);
            }
          }
        }
      }
      // four pixels per store where the address allows it; dst + y * W + x0 is the row's first byte in this tile
      const bool in_image = y < H && x < W;
      const int lead_phase = (int)((0u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) + (uint64_t)y * W + x0)) & 3u);
      const int w1 = __shfl_down(w, 1), w2 = __shfl_down(w, 2), w3 = __shfl_down(w, 3);
      const bool lead = ((lane - lead_phase) & 3) == 0 && lane >= lead_phase && lane + 3 < CPPF_WAVE && y < H && x + 3 < W;
      const unsigned long long leads = wave_ballot(lead);
      const bool covered = (((leads | leads << 1 | leads << 2 | leads << 3) >> lane) & 1ull) != 0;
      if (lead)
        *reinterpret_cast<uint32_t*>(dst + (int64_t)y * W + x) = (uint32_t)w | (uint32_t)w1 << 8 | (uint32_t)w2 << 16 | (uint32_t)w3 << 24;
      else if (in_image && !covered)
        dst[(int64_t)y * W + x] = (uint8_t)w;
      n_valid += (uint32_t)__popcll(wave_ballot(valid));
      n_zero += (uint32_t)__popcll(wave_ballot(valid && w == 0));
      n_full += (uint32_t)__popcll(wave_ballot(w == L));
    }
    if (lane == 0) {
      s_cnt[0][wave] = n_valid;
      s_cnt[1][wave] = n_zero;
      s_cnt[2][wave] = n_full;
    }
    __syncthreads();                                          // also: every read of s_raw is done before the next image
    if (threadIdx.x == 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        uint32_t sum = 0;
#pragma unroll
        for (int q = 0; q < DW_THREADS / CPPF_WAVE; ++q) sum += s_cnt[j][q];
        if (sum) atomicAdd(&counts[3 * (int64_t)i + j], (int)sum);
      }
    }
    __syncthreads();                                          // s_cnt is read before the next image's sums are written
  }
}

extern "C" int cppf_depth_weights(const float* depth, int I, int H, int W, const double* h_K, float pixel_offset, int step, float jump,
                                  float jump_rel, int levels, float cos_min, uint8_t* weights, int32_t* counts, void* stream) {
  CPPF_CHECK_ARG(I >= 0 && H >= 1 && W >= 1 && H <= DW_MAX_DIM && W <= DW_MAX_DIM);
  CPPF_CHECK_ARG(step >= 1 && step <= DW_MAX_STEP && levels >= 1 && levels <= DW_MAX_LEVELS);
  CPPF_CHECK_ARG(jump >= 0.0f && jump < __builtin_inff() && jump_rel >= 0.0f && jump_rel < __builtin_inff());
  CPPF_CHECK_ARG(cos_min >= 0.0f && cos_min < 1.0f);
  CPPF_CHECK_ARG(h_K && __builtin_isfinite(pixel_offset));
  if (I == 0) return CPPF_OK;
  CPPF_CHECK_ARG(depth && weights && counts);
  const uintptr_t in_bytes = (uintptr_t)I * H * W * sizeof(float), out_bytes = (uintptr_t)I * H * W;
  // a block reads its neighbours' pixels: the weights cannot be written over the readings
  CPPF_CHECK_ARG((uintptr_t)weights + out_bytes <= (uintptr_t)depth || (uintptr_t)depth + in_bytes <= (uintptr_t)weights);
  hipStream_t st = (hipStream_t)stream;
  CPPF_HIP(hipMemsetAsync(counts, 0, (size_t)I * 3 * sizeof(int32_t), st));
  const int tiles_x = (W + DW_TW - 1) / DW_TW, tiles_y = (H + DW_TH - 1) / DW_TH;      // <= 256 * 1024 tiles
  hipLaunchKernelGGL(depth_weights_kernel, dim3(tiles_x * tiles_y, I < DW_MAX_GRID_Y ? I : DW_MAX_GRID_Y), dim3(DW_THREADS), 0, st,
                     depth, I, H, W, tiles_x, (float)h_K[0], (float)h_K[1], (float)h_K[2], (float)h_K[3], pixel_offset, step, jump,
                     jump_rel, levels, cos_min, weights, (int*)counts);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
