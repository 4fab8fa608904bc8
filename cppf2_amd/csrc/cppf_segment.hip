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
//
// cppf_concave_edges (experimental; DESIGN.md section 35, tests/concave_ref.py restates it one NumPy ufunc per operation): the
// pixels at which the depth image is locally concave -- where an object meets the table or another object -- leave the mask, so
// that cppf_mask_segments cuts there.  Inputs: depth, Kmat, fg uint8 [I,H,W] or NULL, step s in 1..8, k2 = (float)tan(angle / 2)^2
// (the host computes it in float64), floor2 = (float)floor^2, reach.  valid and point as above.
//   profile of B = (r, c) along e in {(0, 1), (1, 0)}: A = the pixel at -s e, C = the pixel at +s e.  It gives a verdict only
//   when A and C lie inside the image, all three are valid, fabsf(zA - zB) <= reach and fabsf(zC - zB) <= reach.  Then
//     u = B - A, t = C - A                                              (component by component)
//     tt = (t.x * t.x + t.y * t.y) + t.z * t.z;   ut = (u.x * t.x + u.y * t.y) + u.z * t.z
//     o  = (u.x * tt - t.x * ut,  u.y * tt - t.y * ut,  u.z * tt - t.z * ut)    two rounded products, one difference: tt times
//                                                                       B's offset from the chord AC, so nothing is divided
//     ob = (o.x * B.x + o.y * B.y) + o.z * B.z;   oo = (o.x * o.x + o.y * o.y) + o.z * o.z;   t3 = (tt * tt) * tt
//     concave = ob > 0                      B lies behind the chord
//            && 4.0f * oo > k2 * t3         offset / half chord = tan(turn / 2) of a symmetric crease: the turn exceeds `angle`
//            && oo > floor2 * (tt * tt)     the offset itself exceeds `floor`
//   (strict comparisons: collinear points, oo == 0, are never concave; a NaN or an overflow fails them)
//   edge  = valid && (the profile along (0, 1) is concave || the profile along (1, 0) is concave)
//   keep  = valid && !edge && (fg == NULL || fg != 0) ? 255 : 0;   counts[i] = (valid pixels, edge pixels, kept pixels)
// The profiles read the whole depth image, never only fg: the table beside an object is what makes the contact concave.
// One launch for all I images after the counts are cleared, in depth_weights_kernel's shape (cppf_depthweights.hip): grid (tiles
// of an image, min(I, 65535)), 256 threads; block (t, j) serves tile t of the images j, j + gridDim.y, ...; a tile is 16 x 64
// pixels.
//   stage   the tile's readings plus a halo of s go to LDS, normalised: a valid reading as it is, an invalid one 0, a position
//           outside the image -1 (a sign test on the bits tells a valid reading from both).  The region's pitch is its width and
//           the threads walk it in linear order: 32 consecutive banks per half-wavefront.
//   decide  wavefront w takes the tile's rows w, w + 4, w + 8, w + 12, its lanes the 64 columns: each of the five reads is 64
//           consecutive floats of a row of the region, free of bank conflicts.  The five points are back-projected from the staged
//           readings (their divisions are the only ones), the vertical profile only where the horizontal one is not concave.
//   store   a lane whose byte address is a multiple of 4 takes the bytes of the three lanes after it and writes one 32-bit word;
//           what is left (before a row's first aligned address, a row's ragged tail, a group split across two tiles) goes out as
//           single bytes.  A lane reads its own fg byte before any lane of its wavefront stores, and no other wavefront touches
//           the row's 64 bytes: keep may be fg itself.
//   counts  three ballots per row; the four wavefronts' sums meet in LDS, thread 0 adds each with one vector atomic add.
// LDS: 32 x 80 floats = 10 KiB at s = 8.  No scratch memory, no workspace, no host synchronisation.
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

#define CE_TW 64                          // tile width: one wavefront per row
#define CE_TH 16                          // tile height: four rows per wavefront
#define CE_MAX_STEP 8
#define CE_MAX_GRID_Y 65535
#define CE_RAW_W (CE_TW + 2 * CE_MAX_STEP)
#define CE_RAW_H (CE_TH + 2 * CE_MAX_STEP)

// the verdict of one profile whose three points are valid and within reach
__device__ __forceinline__ bool concave_profile(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy,
                                                float cz, float k2, float floor2) {
  const float ux = bx - ax, uy = by - ay, uz = bz - az;
  const float tx = cx - ax, ty = cy - ay, tz = cz - az;
  const float tt = (tx * tx + ty * ty) + tz * tz;
  const float ut = (ux * tx + uy * ty) + uz * tz;
  const float ox = ux * tt - tx * ut, oy = uy * tt - ty * ut, oz = uz * tt - tz * ut;
  const float ob = (ox * bx + oy * by) + oz * bz;
  const float oo = (ox * ox + oy * oy) + oz * oz;
  const float t2 = tt * tt;
  const float t3 = t2 * tt;
  return ob > 0.0f && 4.0f * oo > k2 * t3 && oo > floor2 * t2;
}

__global__ __launch_bounds__(SEG_THREADS) void concave_edges_kernel(const float* __restrict__ depths, const float* __restrict__ Kmat,
                                                                    const uint8_t* fg, int I, int H, int W, int tiles_x, int s,
                                                                    float k2, float floor2, float reach, uint8_t* keep,
                                                                    int* __restrict__ counts) {
  __shared__ float s_raw[CE_RAW_H * CE_RAW_W];
  __shared__ uint32_t s_cnt[3][SEG_THREADS / CPPF_WAVE];
  const int rh = CE_TH + 2 * s, rw = CE_TW + 2 * s;           // the staged readings; rw is s_raw's pitch
  const int tile_y = blockIdx.x / tiles_x;
  const int y0 = tile_y * CE_TH, x0 = (blockIdx.x - tile_y * tiles_x) * CE_TW;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / CPPF_WAVE), lane = wave_lane();
  const int64_t HW = (int64_t)H * W;
  const int x = x0 + lane;
  const float col_l = (float)(x - s), col_c = (float)x, col_r = (float)(x + s);
  for (int i = blockIdx.y; i < I; i += gridDim.y) {
    const int32_t* src = reinterpret_cast<const int32_t*>(depths) + i * HW;
    const uint8_t* own = fg ? fg + i * HW : nullptr;
    uint8_t* dst = keep + i * HW;
    const float fx = Kmat[4 * (int64_t)i], fy = Kmat[4 * (int64_t)i + 1], cx = Kmat[4 * (int64_t)i + 2], cy = Kmat[4 * (int64_t)i + 3];
    for (int k = threadIdx.x; k < rh * rw; k += SEG_THREADS) {
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
    uint32_t n_valid = 0, n_edge = 0, n_kept = 0;
#pragma unroll
    for (int k = 0; k < CE_TH / (SEG_THREADS / CPPF_WAVE); ++k) {
      const int ly = wave + k * (SEG_THREADS / CPPF_WAVE);
      const int y = y0 + ly;
      const float* c = s_raw + (ly + s) * rw + (lane + s);
      const float zb = *c;
      const bool valid = __float_as_int(zb) > 0;              // 0 invalid, -1 outside the image
      bool edge = false;
      int w = 0;
      if (valid) {
        const float bx = (col_c - cx) * zb / fx, by = ((float)y - cy) * zb / fy;
        const float zl = c[-s], zr = c[s];
        if (__float_as_int(zl) > 0 && __float_as_int(zr) > 0 && fabsf(zl - zb) <= reach && fabsf(zr - zb) <= reach) {
          const float ry = (float)y - cy;
          edge = concave_profile((col_l - cx) * zl / fx, ry * zl / fy, zl, bx, by, zb, (col_r - cx) * zr / fx, ry * zr / fy, zr, k2,
                                 floor2);
        }
        if (!edge) {
          const float zu = c[-s * rw], zd = c[s * rw];
          if (__float_as_int(zu) > 0 && __float_as_int(zd) > 0 && fabsf(zu - zb) <= reach && fabsf(zd - zb) <= reach) {
            const float rx = col_c - cx;
            edge = concave_profile(rx * zu / fx, ((float)(y - s) - cy) * zu / fy, zu, bx, by, zb, rx * zd / fx,
                                   ((float)(y + s) - cy) * zd / fy, zd, k2, floor2);
          }
        }
        if (!edge && (own == nullptr || own[(int64_t)y * W + x] != 0)) w = 255;      // a valid pixel lies inside the image
      }
      // four pixels per store where the address allows it (depth_weights_kernel's); dst + y * W + x0 is the row's first byte here
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
      n_edge += (uint32_t)__popcll(wave_ballot(edge));
      n_kept += (uint32_t)__popcll(wave_ballot(w != 0));
    }
    if (lane == 0) {
      s_cnt[0][wave] = n_valid;
      s_cnt[1][wave] = n_edge;
      s_cnt[2][wave] = n_kept;
    }
    __syncthreads();                                          // also: every read of s_raw is done before the next image
    if (threadIdx.x == 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        uint32_t sum = 0;
#pragma unroll
        for (int q = 0; q < SEG_THREADS / CPPF_WAVE; ++q) sum += s_cnt[j][q];
        if (sum) atomicAdd(&counts[3 * (int64_t)i + j], (int)sum);
      }
    }
    __syncthreads();                                          // s_cnt is read before the next image's sums are written
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

extern "C" int cppf_concave_edges(int I, int H, int W, const float* depths, const float* Kmat, const uint8_t* fg, int step, float k2,
                                  float floor2, float reach, uint8_t* keep, int32_t* counts, void* stream) {
  CPPF_CHECK_ARG(I >= 0 && H >= 1 && W >= 1 && H <= SEG_MAX_DIM && W <= SEG_MAX_DIM);
  CPPF_CHECK_ARG(step >= 1 && step <= CE_MAX_STEP);
  CPPF_CHECK_ARG(k2 >= 0.0f && k2 < __builtin_inff() && floor2 >= 0.0f && floor2 < __builtin_inff());
  CPPF_CHECK_ARG(reach >= 0.0f && reach < __builtin_inff());
  if (I == 0) return CPPF_OK;
  CPPF_CHECK_ARG(depths && Kmat && keep && counts);
  const uintptr_t in_bytes = (uintptr_t)I * H * W * sizeof(float), out_bytes = (uintptr_t)I * H * W;
  // a block reads its neighbours' pixels: the mask cannot be written over the readings (it may be written over fg)
  CPPF_CHECK_ARG((uintptr_t)keep + out_bytes <= (uintptr_t)depths || (uintptr_t)depths + in_bytes <= (uintptr_t)keep);
  hipStream_t st = (hipStream_t)stream;
  CPPF_HIP(hipMemsetAsync(counts, 0, (size_t)I * 3 * sizeof(int32_t), st));
  const int tiles_x = (W + CE_TW - 1) / CE_TW, tiles_y = (H + CE_TH - 1) / CE_TH;      // <= 128 * 512 tiles
  hipLaunchKernelGGL(concave_edges_kernel, dim3(tiles_x * tiles_y, I < CE_MAX_GRID_Y ? I : CE_MAX_GRID_Y), dim3(SEG_THREADS), 0, st,
                     depths, Kmat, fg, I, H, W, tiles_x, step, k2, floor2, reach, keep, (int*)counts);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
