// Mask proposals from depth alone, first half: the support plane of a tabletop depth image by sampled three-point hypotheses
// and inlier counting, and the pixels that stand above it (cppf2_amd/segment.py drives both; cppf_mask_segments in
// cppf_mask.hip cuts what is left into depth-connected pieces).  The reference has no such step.  Counts are integers and
// the winner is an integer maximum, so an image's outputs do not depend on the grid, the batch or the order.  gfx950 only.
//
// Every float operation below is float32 and rounds where it is written (-ffp-contract=off, correctly rounded division and
// square root).
//   valid(r, c)   = depth > 0 && depth < +inf                                  (NaN fails depth > 0)
//   point(r, c)   : z = depth, x = ((float)c - cx) * z / fx, y = ((float)r - cy) * z / fy      (x right, y down, z forward:
//                   cppf_gt_visibility's camera frame); (fx, fy, cx, cy) = Kmat[i]
//   hypothesis h of image i: w = philox4x32_10(counter (h, 0, 0, 0), key (seeds[i] low word, seeds[i] high word));
//                   pixel j = (uint64)w[j] * (H * W) >> 32 for j = 0, 1, 2 -> points a, b, c
//                   u = b - a, v = c - a                                       (component by component)
//                   cross = (u.y * v.z - u.z * v.y,  u.z * v.x - u.x * v.z,  u.x * v.y - u.y * v.x)
//                           (each product rounded, then one subtraction)
//                   len = sqrtf((cross.x * cross.x + cross.y * cross.y) + cross.z * cross.z)
//                   unusable when two pixel indices coincide, a pixel is not valid, or !(len > 1e-12f)
//                   n = cross / len (three divisions), d = -((n.x * a.x + n.y * a.y) + n.z * a.z);
//                   if d < 0: n = -n, d = -d                                   (the camera is on the positive side)
//   inlier        = valid && fabsf(((n.x * x + n.y * y) + n.z * z) + d) <= tau
//   winner        = the 64-bit maximum over the usable hypotheses of count << 32 | (0xFFFFFFFF - h): the most inliers, ties
//                   to the lowest index -- cppf_grid_peaks' and cc_select_kernel's key
//
// cppf_plane_fit: three launches behind one clear (stats) on the stream.
//   1 hypotheses  grid (ceil(num_hyp / 256), I): planes[i][h] = (n, d) or four NaNs, counts[i][h] = 0 or -1 (unusable)
//   2 count       grid (ceil(H * W / 1024), I), 256 threads: each lane keeps 4 back-projected pixels in registers (an invalid
//                 pixel carries NaNs: its comparison fails), the block holds the image's planes in LDS (16 KiB at 1024
//                 hypotheses, every read a broadcast) and walks them 64 at a time: the four ballots' population counts of
//                 hypothesis h0 + j are kept by lane j, so that 64 hypotheses cost the wavefront one LDS integer add per
//                 lane; at the end one global integer atomic per hypothesis and block.  An unusable hypothesis has no
//                 inlier, so its count stays -1.  stats[i][3] += valid pixels the same way.
//   3 select      grid (1, I): the maximum key and the number of usable hypotheses; plane[i] = the winner's (n, d) or zeros,
//                 stats[i] = (winner or -1, its inliers, usable hypotheses, valid pixels)
//
// cppf_plane_foreground: one launch, grid (ceil(groups / 256), I); each lane owns 4 consecutive pixels and stores their bytes
//   as one aligned 32-bit word (cc_write_kernel's layout: the first and the last group of an image may be partial).
//   height = ((n.x * x + n.y * y) + n.z * z) + d;  fg = valid && height > min_height && (max_height <= 0 || height <= max_height)
//   ? 255 : 0; an image whose plane is four zeros: fg = valid ? 255 : 0.
#include "cppf_common.h"

#define SEG_THREADS 256
#define SEG_PX 4                   // pixels per lane
#define SEG_TILE (SEG_THREADS * SEG_PX)
#define SEG_MAX_HYP 1024
#define SEG_MAX_DIM 8192           // H, W: H * W <= 2^26
#define SEG_MIN_LEN 1e-12f

struct SegPoint {
  float x, y, z;
  bool valid;
};

__device__ __forceinline__ SegPoint seg_point(const float* __restrict__ dp, int i, int W, float fx, float fy, float cx, float cy) {
  SegPoint p;
  const int r = i / W, c = i - r * W;
  const float z = dp[i];
  p.valid = z > 0.0f && z < __builtin_inff();
  p.z = z;
  p.x = ((float)c - cx) * z / fx;
  p.y = ((float)r - cy) * z / fy;
  return p;
}

static int64_t plane_planes_bytes(int I, int num_hyp) { return align_up((int64_t)I * num_hyp * 16, 256); }

__global__ __launch_bounds__(SEG_THREADS) void plane_hyp_kernel(const float* __restrict__ depths, const float* __restrict__ Kmat,
                                                                const uint64_t* __restrict__ seeds, int H, int W, int num_hyp,
                                                                float4* __restrict__ planes, int* __restrict__ counts) {
  const int i = blockIdx.y;
  const int h = blockIdx.x * SEG_THREADS + threadIdx.x;
  if (h >= num_hyp) return;
  const int HW = H * W;
  const float* dp = depths + (int64_t)i * HW;
  const float fx = Kmat[4 * i], fy = Kmat[4 * i + 1], cx = Kmat[4 * i + 2], cy = Kmat[4 * i + 3];
  const uint64_t seed = seeds[i];
  const Philox4 w = philox4x32_10((uint32_t)h, 0u, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  const int pa = (int)(((uint64_t)w.v[0] * (uint64_t)HW) >> 32);
  const int pb = (int)(((uint64_t)w.v[1] * (uint64_t)HW) >> 32);
  const int pc = (int)(((uint64_t)w.v[2] * (uint64_t)HW) >> 32);
  const SegPoint a = seg_point(dp, pa, W, fx, fy, cx, cy);
  const SegPoint b = seg_point(dp, pb, W, fx, fy, cx, cy);
  const SegPoint c = seg_point(dp, pc, W, fx, fy, cx, cy);
  const float ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
  const float vx = c.x - a.x, vy = c.y - a.y, vz = c.z - a.z;
  const float kx = uy * vz - uz * vy;
  const float ky = uz * vx - ux * vz;
  const float kz = ux * vy - uy * vx;
  const float len = sqrtf((kx * kx + ky * ky) + kz * kz);
  const bool usable = pa != pb && pa != pc && pb != pc && a.valid && b.valid && c.valid && len > SEG_MIN_LEN;
  const float nan = __builtin_nanf("");
  float4 pl = make_float4(nan, nan, nan, nan);
  if (usable) {
    float nx = kx / len, ny = ky / len, nz = kz / len;
    float d = -((nx * a.x + ny * a.y) + nz * a.z);
    if (d < 0.0f) { nx = -nx; ny = -ny; nz = -nz; d = -d; }
    pl = make_float4(nx, ny, nz, d);
  }
  planes[(int64_t)i * num_hyp + h] = pl;
  counts[(int64_t)i * num_hyp + h] = usable ? 0 : -1;
}

__global__ __launch_bounds__(SEG_THREADS) void plane_count_kernel(const float* __restrict__ depths, const float* __restrict__ Kmat,
                                                                  int H, int W, int num_hyp, float tau,
                                                                  const float4* __restrict__ planes, int* __restrict__ counts,
                                                                  int* __restrict__ stats) {
  __shared__ float4 s_pl[SEG_MAX_HYP];
  __shared__ int s_cnt[SEG_MAX_HYP];
  __shared__ int s_valid;
  const int i = blockIdx.y;
  const int HW = H * W;
  const float* dp = depths + (int64_t)i * HW;
  const float fx = Kmat[4 * i], fy = Kmat[4 * i + 1], cx = Kmat[4 * i + 2], cy = Kmat[4 * i + 3];
  for (int h = threadIdx.x; h < num_hyp; h += SEG_THREADS) {
    s_pl[h] = planes[(int64_t)i * num_hyp + h];
    s_cnt[h] = 0;
  }
  if (threadIdx.x == 0) s_valid = 0;
  const float nan = __builtin_nanf("");
  float x[SEG_PX], y[SEG_PX], z[SEG_PX];
  int nvalid = 0;
#pragma unroll
  for (int j = 0; j < SEG_PX; ++j) {
    // pixel j of the lane: consecutive lanes read consecutive floats
    const int p = blockIdx.x * SEG_TILE + j * SEG_THREADS + threadIdx.x;
    x[j] = y[j] = z[j] = nan;
    bool valid = false;
    if (p < HW) {
      const SegPoint q = seg_point(dp, p, W, fx, fy, cx, cy);
      valid = q.valid;
      if (valid) { x[j] = q.x; y[j] = q.y; z[j] = q.z; }
    }
    nvalid += (int)__popcll(wave_ballot(valid));
  }
  __syncthreads();
  const int lane = wave_lane();
  if (lane == 0 && nvalid) atomicAdd(&s_valid, nvalid);
  for (int h0 = 0; h0 < num_hyp; h0 += CPPF_WAVE) {
    const int cnt = num_hyp - h0 < CPPF_WAVE ? num_hyp - h0 : CPPF_WAVE;       // uniform
    int acc = 0;
    for (int k = 0; k < cnt; ++k) {
      const float4 pl = s_pl[h0 + k];                                           // one address for the wavefront: a broadcast
      int n = 0;
#pragma unroll
      for (int j = 0; j < SEG_PX; ++j) {
        const float dist = ((pl.x * x[j] + pl.y * y[j]) + pl.z * z[j]) + pl.w;
        n += (int)__popcll(wave_ballot(fabsf(dist) <= tau));
      }
      acc = lane == k ? n : acc;
    }
    if (lane < cnt && acc) atomicAdd(&s_cnt[h0 + lane], acc);
  }
  __syncthreads();
  for (int h = threadIdx.x; h < num_hyp; h += SEG_THREADS) {
    const int n = s_cnt[h];
    if (n) atomicAdd(&counts[(int64_t)i * num_hyp + h], n);
  }
  if (threadIdx.x == 0 && s_valid) atomicAdd(&stats[4 * i + 3], s_valid);
}

__global__ __launch_bounds__(SEG_THREADS) void plane_select_kernel(int num_hyp, const float4* __restrict__ planes,
                                                                   const int* __restrict__ counts, float* __restrict__ plane,
                                                                   int* __restrict__ stats) {
  __shared__ unsigned long long s_best;
  __shared__ int s_usable;
  const int i = blockIdx.x;
  if (threadIdx.x == 0) { s_best = 0; s_usable = 0; }
  __syncthreads();
  unsigned long long key = 0;
  int usable = 0;
  for (int h0 = 0; h0 < num_hyp; h0 += SEG_THREADS) {
    const int h = h0 + threadIdx.x;
    const int n = h < num_hyp ? counts[(int64_t)i * num_hyp + h] : -1;
    if (n >= 0) {
      const unsigned long long k = ((unsigned long long)(uint32_t)n << 32) | (0xFFFFFFFFu - (uint32_t)h);
      key = k > key ? k : key;
    }
    usable += (int)__popcll(wave_ballot(n >= 0));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off);
    key = o > key ? o : key;
  }
  if (wave_lane() == 0) {
    if (key) atomicMax(&s_best, key);
    if (usable) atomicAdd(&s_usable, usable);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long best = s_best;                // != 0 whenever a hypothesis is usable: 0xFFFFFFFF - h > 0
    const int win = best ? (int)(0xFFFFFFFFu - (uint32_t)best) : -1;
    float4 pl = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (win >= 0) pl = planes[(int64_t)i * num_hyp + win];
    plane[4 * i] = pl.x; plane[4 * i + 1] = pl.y; plane[4 * i + 2] = pl.z; plane[4 * i + 3] = pl.w;
    stats[4 * i] = win;
    stats[4 * i + 1] = (int)(best >> 32);
    stats[4 * i + 2] = s_usable;                           // stats[4 * i + 3]: the count launch's sum
  }
}

__global__ __launch_bounds__(SEG_THREADS) void plane_foreground_kernel(const float* __restrict__ depths, const float* __restrict__ Kmat,
                                                                       const float* __restrict__ plane, int H, int W,
                                                                       float min_height, float max_height, uint8_t* __restrict__ fg) {
  const int i = blockIdx.y;
  const int HW = H * W;
  const float* dp = depths + (int64_t)i * HW;
  const float fx = Kmat[4 * i], fy = Kmat[4 * i + 1], cx = Kmat[4 * i + 2], cy = Kmat[4 * i + 3];
  const float nx = plane[4 * i], ny = plane[4 * i + 1], nz = plane[4 * i + 2], d = plane[4 * i + 3];
  const bool none = nx == 0.0f && ny == 0.0f && nz == 0.0f && d == 0.0f;
  uint8_t* out = fg + (int64_t)i * HW;
  const int m = (int)((uintptr_t)out & 3);                // groups as in rle_decode_kernel: out + 4q - m is 4-byte aligned
  const int nq = (HW + m + SEG_PX - 1) / SEG_PX;
  const int q = blockIdx.x * SEG_THREADS + threadIdx.x;
  if (q >= nq) return;
  const int i0 = SEG_PX * q - m;
  uint32_t bytes = 0;
#pragma unroll
  for (int j = 0; j < SEG_PX; ++j) {
    const int p = i0 + j;
    if (p < 0 || p >= HW) continue;
    const SegPoint pt = seg_point(dp, p, W, fx, fy, cx, cy);
    const float height = ((nx * pt.x + ny * pt.y) + nz * pt.z) + d;
    const bool above = none || (height > min_height && (!(max_height > 0.0f) || height <= max_height));
    if (pt.valid && above) bytes |= 0xffu << (8 * j);
  }
  if (i0 >= 0 && i0 + SEG_PX - 1 < HW) {
    *reinterpret_cast<uint32_t*>(out + i0) = bytes;
  } else {
#pragma unroll
    for (int j = 0; j < SEG_PX; ++j)
      if (i0 + j >= 0 && i0 + j < HW) out[i0 + j] = (uint8_t)(bytes >> (8 * j));
  }
}

extern "C" int64_t cppf_plane_fit_workspace_bytes(int I, int num_hyp) {
  if (I <= 0 || I > 65535 || num_hyp < 1 || num_hyp > SEG_MAX_HYP) return 0;
  return plane_planes_bytes(I, num_hyp) + align_up((int64_t)I * num_hyp * (int64_t)sizeof(int32_t), 256);
}

extern "C" int cppf_plane_fit(int I, int H, int W, const float* depths, const float* Kmat, const uint64_t* seeds, int num_hyp,
                              float tau, float* plane, int32_t* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  CPPF_CHECK_ARG(I >= 0 && I <= 65535);
  CPPF_CHECK_ARG(H >= 1 && W >= 1 && H <= SEG_MAX_DIM && W <= SEG_MAX_DIM);
  CPPF_CHECK_ARG(num_hyp >= 1 && num_hyp <= SEG_MAX_HYP);
  CPPF_CHECK_ARG(tau > 0.0f && tau < __builtin_inff());
  if (I == 0) return CPPF_OK;
  CPPF_CHECK_ARG(depths && Kmat && seeds && plane && stats);
  CPPF_CHECK_ARG(workspace && (uintptr_t)workspace % 16 == 0);
  CPPF_CHECK_ARG(workspace_bytes >= cppf_plane_fit_workspace_bytes(I, num_hyp));
  hipStream_t st = (hipStream_t)stream;
  float4* planes = (float4*)workspace;
  int* counts = (int*)((char*)workspace + plane_planes_bytes(I, num_hyp));
  const int HW = H * W;
  CPPF_HIP(hipMemsetAsync(stats, 0, (size_t)I * 4 * sizeof(int32_t), st));
  hipLaunchKernelGGL(plane_hyp_kernel, dim3((num_hyp + SEG_THREADS - 1) / SEG_THREADS, I), dim3(SEG_THREADS), 0, st, depths, Kmat,
                     seeds, H, W, num_hyp, planes, counts);
  hipLaunchKernelGGL(plane_count_kernel, dim3((HW + SEG_TILE - 1) / SEG_TILE, I), dim3(SEG_THREADS), 0, st, depths, Kmat, H, W,
                     num_hyp, tau, (const float4*)planes, counts, (int*)stats);
  hipLaunchKernelGGL(plane_select_kernel, dim3(I), dim3(SEG_THREADS), 0, st, num_hyp, (const float4*)planes, (const int*)counts,
                     plane, (int*)stats);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}

extern "C" int cppf_plane_foreground(int I, int H, int W, const float* depths, const float* Kmat, const float* plane,
                                     float min_height, float max_height, uint8_t* fg, void* stream) {
  CPPF_CHECK_ARG(I >= 0 && I <= 65535);
  CPPF_CHECK_ARG(H >= 1 && W >= 1 && H <= SEG_MAX_DIM && W <= SEG_MAX_DIM);
  CPPF_CHECK_ARG(min_height == min_height && max_height == max_height);
  if (I == 0) return CPPF_OK;
  CPPF_CHECK_ARG(depths && Kmat && plane && fg);
  const int nq = H * W / SEG_PX + 2;                      // groups of an image, misaligned start and partial end included
  hipLaunchKernelGGL(plane_foreground_kernel, dim3((nq + SEG_THREADS - 1) / SEG_THREADS, I), dim3(SEG_THREADS), 0,
                     (hipStream_t)stream, depths, Kmat, plane, H, W, min_height, max_height, fg);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
