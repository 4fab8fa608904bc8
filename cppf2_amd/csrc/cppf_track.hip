// B depth frames aligned to one signed distance volume (Bylow et al., "Real-Time Camera Tracking and 3D Reconstruction Using
// Signed Distance Functions", RSS 2013): point-to-plane ICP with "the nearest model sample and its normal" replaced by "the
// volume's value and gradient at the point" -- no mesh, no raycast, no nearest-neighbour search.  How a sequence with one known
// pose gets the poses cppf_tsdf_integrate needs (cppf2_amd/track.py).  The reference has no such step.
// gfx950 only.  tests/track_ref.py restates every definition below in NumPy; the build's -ffp-contract=off keeps every operation
// where it is written and the float32 divide and square root are correctly rounded.
//
// One cppf_tsdf_track call enqueues, for k = 0 .. iters-1, two launches on the caller's stream (no host synchronisation):
//   track_accum  grid (ceil(H W / 256), B), 256 threads, thread x of block y owns pixel pix = 256 y + x, r = pix / W, c = pix % W,
//                and handles it iff pix < H W, r % stride == 0 and c % stride == 0.  The frame's pose (float64 [12], row-major
//                3x4, model -> OpenCV camera) is cast to float32 once.  Per handled pixel, float32, left to right:
//     gate      mask[b,r,c] != 0 (no masks: every pixel) and d = depth[b,r,c] with d > 0 and d < +inf; a gated pixel counts 1
//               into entry 30 of the block's slot
//     p         p.x = ((((float)c + po) - cx) * d) / fx,  p.y = ((((float)r + po) - cy) * d) / fy,  p.z = d    (po = pixel_offset)
//     q         dd = p - tf;  q.x = (Rf00*dd.x + Rf10*dd.y) + Rf20*dd.z,  q.y = (Rf01*dd.x + Rf11*dd.y) + Rf21*dd.z,
//               q.z = (Rf02*dd.x + Rf12*dd.y) + Rf22*dd.z                                  (cppf_icp.hip's expression)
//     cell      g.a = (q.a - o.a) / voxel per axis a;  inside iff 0 <= g.a < (float)(n.a - 1) on every axis (a NaN fails);
//               fl = floorf(g.a), i.a = (int)fl, f.a = g.a - fl;  node lin = (i.x * ny + i.y) * nz + i.z, corner
//               t[dx | dy << 1 | dz << 2] = acc / (float)wsum at lin + dx ny nz + dy nz + dz (cppf_tsdf_extract's tsdf);
//               the pixel is skipped unless all eight wsum >= min_weight
//     lerp      L(a, b, w) = a + (b - a) * w
//     phi       L(L(L(t0,t1,f.x), L(t2,t3,f.x), f.y), L(L(t4,t5,f.x), L(t6,t7,f.x), f.y), f.z)
//     grad      G.x = L(L(t1-t0, t3-t2, f.y), L(t5-t4, t7-t6, f.y), f.z)
//               G.y = L(L(t2-t0, t3-t1, f.x), L(t6-t4, t7-t5, f.x), f.z)
//               G.z = L(L(t4-t0, t5-t1, f.x), L(t6-t2, t7-t3, f.x), f.y)             (units of 1 / voxel, divided by nothing)
//               g2 = (G.x*G.x + G.y*G.y) + G.z*G.z; skipped unless g2 > 0 and g2 < +inf;  s = sqrtf(g2),  n = G / s per component
//     e         e = trunc * phi;  inlier iff |e| <= dk  (a NaN fails)
//   float64 (q, n, e widened from float32):  J = [q x n, n], (q x n) = (q.y*n.z - q.z*n.y, q.z*n.x - q.x*n.z, q.x*n.y - q.y*n.x);
//               the 30 terms of cppf_icp.hip's icp_match: entries [0,21) J_a * J_c (a <= c, row-major), [21,27) J_a * e, [27] 1,
//               [28] e * e, [29] (q.x*q.x + q.y*q.y) + q.z*q.z;  [30] the gated pixels, [31] 0.
//               Reduction: wave_sum (a fixed xor butterfly) per wavefront (a wavefront without a gated pixel writes the +0.0 the
//               butterfly would give without running it), the 4 wavefronts added in order 0, 1, 2, 3, every block writes all 32
//               entries of its own workspace slot, zeros included.  No atomics: nothing depends on scheduling.
//   track_solve  one wavefront per frame: lane j < 32 sums entry j over the frame's slots in block order from 0.0 (the slots staged
//                through LDS 64 at a time, which changes no addition); lane 0 then does
//                cppf_icp.hip's solve on the 30 terms (stated there under "solve" and "Rodrigues", restated in tests/icp_ref.py's
//                _min_norm_solve and rodrigues; ICP_TAU, ICP_JEPS and ICP_SWEEPS: the device functions of cppf_icp_solve.h, which
//                both files include) and the update R <- R dR^T, t <- t - R v with the new R.
//                Fewer than 6 inliers, rank 0 or a zero or non-finite step: the pose is not written, it keeps its bytes.
// Stats per frame (float32 [4], written every iteration): [0] inliers of the last iteration, [1] sqrt(sum e^2 / inliers) (0
// without inliers), [2] inliers / gated pixels (0 without gated pixels), [3] the iterations that moved the pose.
#include "cppf_common.h"
#include "cppf_icp_solve.h"

#include <math.h>

#define TRK_THREADS 256
#define TRK_SLOT 32            // doubles per block slot: the 30 terms, the gated pixels, 0
#define TRK_CHUNK 64           // slots track_solve stages in LDS at a time (16 KiB)
#define TRK_MAX_NODES (1LL << 27)        // cppf_fuse.hip's TSDF_MAX_NODES
#define TRK_MAX_IMAGE 16384              // H and W, as cppf_tsdf_integrate's
#define TRK_MAX_FRAMES 65535             // the grid's y extent

struct TrackGrid {
  float ox, oy, oz, voxel;
  int nx, ny, nz;
};

struct TrackCamera {
  float fx, fy, cx, cy, po;
};

__device__ __forceinline__ float trk_lerp(float a, float b, float w) { return a + (b - a) * w; }

__global__ __launch_bounds__(TRK_THREADS) void track_accum_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ masks,
                                                                  int H, int W, int stride, TrackCamera cam,
                                                                  const float* __restrict__ acc, const int32_t* __restrict__ wsum,
                                                                  TrackGrid g, float trunc, int min_weight, float dk,
                                                                  const double* __restrict__ poses, int nblk,
                                                                  double* __restrict__ part) {
  __shared__ double s_w[TRK_THREADS / CPPF_WAVE][TRK_SLOT];
  const int b = blockIdx.y;
  const double* P = poses + 12 * (int64_t)b;
  const int pix = blockIdx.x * TRK_THREADS + threadIdx.x;            // H W <= 2^28
  const int r = pix / W, c = pix - r * W;
  double v[TRK_SLOT];
#pragma unroll
  for (int a = 0; a < TRK_SLOT; ++a) v[a] = 0.0;
  if (pix < H * W && r % stride == 0 && c % stride == 0) {
    const int64_t at = ((int64_t)b * H + r) * W + c;
    const float d = depth[at];
    if ((masks == nullptr || masks[at] != 0) && d > 0.0f && d < __builtin_inff()) {
      v[30] = 1.0;
      const float Rf0 = (float)P[0], Rf1 = (float)P[1], Rf2 = (float)P[2], tf0 = (float)P[3];
      const float Rf3 = (float)P[4], Rf4 = (float)P[5], Rf5 = (float)P[6], tf1 = (float)P[7];
      const float Rf6 = (float)P[8], Rf7 = (float)P[9], Rf8 = (float)P[10], tf2 = (float)P[11];
      const float px = ((((float)c + cam.po) - cam.cx) * d) / cam.fx;
      const float py = ((((float)r + cam.po) - cam.cy) * d) / cam.fy;
      const float dx = px - tf0, dy = py - tf1, dz = d - tf2;
      const float qx = (Rf0 * dx + Rf3 * dy) + Rf6 * dz;
      const float qy = (Rf1 * dx + Rf4 * dy) + Rf7 * dz;
      const float qz = (Rf2 * dx + Rf5 * dy) + Rf8 * dz;
      const float gx = (qx - g.ox) / g.voxel, gy = (qy - g.oy) / g.voxel, gz = (qz - g.oz) / g.voxel;
      // compared in float32 first: a huge or NaN coordinate never reaches the cast, and i + 1 <= n - 1 on every axis
      if (gx >= 0.0f && gx < (float)(g.nx - 1) && gy >= 0.0f && gy < (float)(g.ny - 1) && gz >= 0.0f && gz < (float)(g.nz - 1)) {
        const float flx = floorf(gx), fly = floorf(gy), flz = floorf(gz);
        const float fx = gx - flx, fy = gy - fly, fz = gz - flz;
        const int64_t lin = ((int64_t)(int)flx * g.ny + (int)fly) * g.nz + (int)flz;
        float t[8];                      // compile-time indices only (the loop is unrolled): registers, no scratch memory
        bool known = true;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int64_t n = lin + (int64_t)(k & 1) * g.ny * g.nz + (int64_t)((k >> 1) & 1) * g.nz + ((k >> 2) & 1);
          const int32_t w = wsum[n];
          t[k] = acc[n] / (float)w;
          known = known && w >= min_weight;
        }
        if (known) {
          const float phi = trk_lerp(trk_lerp(trk_lerp(t[0], t[1], fx), trk_lerp(t[2], t[3], fx), fy),
                                     trk_lerp(trk_lerp(t[4], t[5], fx), trk_lerp(t[6], t[7], fx), fy), fz);
          const float Gx = trk_lerp(trk_lerp(t[1] - t[0], t[3] - t[2], fy), trk_lerp(t[5] - t[4], t[7] - t[6], fy), fz);
          const float Gy = trk_lerp(trk_lerp(t[2] - t[0], t[3] - t[1], fx), trk_lerp(t[6] - t[4], t[7] - t[5], fx), fz);
          const float Gz = trk_lerp(trk_lerp(t[4] - t[0], t[5] - t[1], fx), trk_lerp(t[6] - t[2], t[7] - t[3], fx), fy);
          const float g2 = (Gx * Gx + Gy * Gy) + Gz * Gz;
          const float ef = trunc * phi;
          if (g2 > 0.0f && g2 < __builtin_inff() && fabsf(ef) <= dk) {
            const float s = __builtin_sqrtf(g2);
            const double nx = (double)(Gx / s), ny = (double)(Gy / s), nz = (double)(Gz / s);
            const double Qx = qx, Qy = qy, Qz = qz, e = ef;
            const double J[6] = {Qy * nz - Qz * ny, Qz * nx - Qx * nz, Qx * ny - Qy * nx, nx, ny, nz};
            int o = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
              for (int k = a; k < 6; ++k) v[o++] = J[a] * J[k];
#pragma unroll
            for (int a = 0; a < 6; ++a) v[21 + a] = J[a] * e;
            v[27] = 1.0;
            v[28] = e * e;
            v[29] = (Qx * Qx + Qy * Qy) + Qz * Qz;
          }
        }
      }
    }
  }
  const int w = threadIdx.x / CPPF_WAVE;
  if (wave_ballot(v[30] != 0.0) == 0) {            // a wavefront without a gated pixel (most of a masked image): every sum is +0.0,
    if (wave_lane() < TRK_SLOT) s_w[w][wave_lane()] = 0.0;          // the bits the butterfly would give
  } else {
#pragma unroll
    for (int a = 0; a < TRK_SLOT; ++a) {
      const double s = wave_sum(v[a]);
      if (wave_lane() == 0) s_w[w][a] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x < TRK_SLOT) {
    double s = s_w[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < TRK_THREADS / CPPF_WAVE; ++k) s += s_w[k][threadIdx.x];
    part[((int64_t)b * nblk + blockIdx.x) * TRK_SLOT + threadIdx.x] = s;
  }
}

// One wavefront per frame; lane 0 does the 6x6 solve and the pose update in LDS (cppf_icp_solve.h, shared with cppf_icp.hip).
__global__ __launch_bounds__(CPPF_WAVE) void track_solve_kernel(int nblk, const double* __restrict__ part, int k,
                                                                double* __restrict__ poses, float* __restrict__ stats) {
  __shared__ double s_t[TRK_SLOT];
  __shared__ double s_c[TRK_CHUNK * TRK_SLOT];
  __shared__ IcpSolveLds L;
  const int b = blockIdx.x;
  double* P = poses + 12 * (int64_t)b;
  float* st = stats + 4 * (int64_t)b;
  // The frame's slots in block order.  A 640 x 480 frame has 1 200 of them: read one after the other by 32 lanes that is 1 200
  // dependent trips to memory (measured 328 us, against 11 us for the frame's track_accum), so the wavefront copies
  // TRK_CHUNK slots at a time into LDS with all 64 lanes (independent loads, 512 contiguous bytes each), and lane j adds entry j of
  // the copies in slot order: the same additions in the same order.
  double sum = 0.0;
  const double* row = part + (int64_t)b * nblk * TRK_SLOT;
  for (int blk0 = 0; blk0 < nblk; blk0 += TRK_CHUNK) {
    const int cnt = min(TRK_CHUNK, nblk - blk0);
    const double* src = row + (int64_t)blk0 * TRK_SLOT;
    if (cnt == TRK_CHUNK) {
#pragma unroll
      for (int i = 0; i < TRK_CHUNK * TRK_SLOT / CPPF_WAVE; ++i) s_c[i * CPPF_WAVE + threadIdx.x] = src[i * CPPF_WAVE + threadIdx.x];
    } else {
      for (int i = threadIdx.x; i < cnt * TRK_SLOT; i += CPPF_WAVE) s_c[i] = src[i];
    }
    __syncthreads();
    if (threadIdx.x < TRK_SLOT) {
#pragma unroll 8
      for (int q = 0; q < cnt; ++q) sum += s_c[q * TRK_SLOT + threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x < TRK_SLOT) s_t[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double cnt = s_t[27];
  const bool ok = cnt >= 6.0 && icp_min_norm_step(s_t, cnt, L);
  if (ok) {
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) L.R[r * 3 + q] = P[r * 4 + q];
    icp_rotation_update(L);
    for (int r = 0; r < 3; ++r) {
      P[r * 4 + 3] = P[r * 4 + 3] - ((L.Rn[r * 3] * L.x[3] + L.Rn[r * 3 + 1] * L.x[4]) + L.Rn[r * 3 + 2] * L.x[5]);
      for (int q = 0; q < 3; ++q) P[r * 4 + q] = L.Rn[r * 3 + q];
    }
  }
  const double gated = s_t[30];
  st[0] = (float)cnt;
  st[1] = cnt > 0.0 ? (float)sqrt(s_t[28] / cnt) : 0.0f;
  st[2] = gated > 0.0 ? (float)(cnt / gated) : 0.0f;
  st[3] = (k == 0 ? 0.0f : st[3]) + (ok ? 1.0f : 0.0f);
}

static bool trk_positive(float x) { return x > 0.0f && x < INFINITY; }

static bool trk_blocks(int B, int H, int W, int stride, int64_t* nblk) {
  if (B < 0 || B > TRK_MAX_FRAMES || H < 1 || H > TRK_MAX_IMAGE || W < 1 || W > TRK_MAX_IMAGE || stride < 1) return false;
  *nblk = ((int64_t)H * W + TRK_THREADS - 1) / TRK_THREADS;
  return true;
}

extern "C" int64_t cppf_tsdf_track_workspace_bytes(int B, int H, int W, int stride) {
  int64_t nblk;
  if (!trk_blocks(B, H, W, stride, &nblk)) return -1;
  return (int64_t)B * nblk * TRK_SLOT * (int64_t)sizeof(double);
}

extern "C" int cppf_tsdf_track(int B, const float* depth, const uint8_t* masks, int H, int W, const double* h_K, float pixel_offset,
                               int stride, const float* acc, const int32_t* wsum, const double* h_origin, float voxel, int nx, int ny,
                               int nz, float trunc, int min_weight, int iters, const float* h_dk, double* poses, float* stats,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  int64_t nblk;
  CPPF_CHECK_ARG(trk_blocks(B, H, W, stride, &nblk));
  CPPF_CHECK_ARG(iters >= 0);
  CPPF_CHECK_ARG(h_K && h_origin && acc && wsum);
  CPPF_CHECK_ARG(nx >= 1 && ny >= 1 && nz >= 1 && trk_positive(voxel));
  CPPF_CHECK_ARG((int64_t)nx * ny <= TRK_MAX_NODES && (int64_t)nx * ny * nz <= TRK_MAX_NODES);
  TrackGrid g;
  g.ox = (float)h_origin[0]; g.oy = (float)h_origin[1]; g.oz = (float)h_origin[2];
  g.voxel = voxel; g.nx = nx; g.ny = ny; g.nz = nz;
  CPPF_CHECK_ARG(__builtin_isfinite(g.ox) && __builtin_isfinite(g.oy) && __builtin_isfinite(g.oz));
  CPPF_CHECK_ARG(trk_positive(trunc) && __builtin_isfinite(pixel_offset) && min_weight >= 1);
  TrackCamera cam;
  cam.fx = (float)h_K[0]; cam.fy = (float)h_K[1]; cam.cx = (float)h_K[2]; cam.cy = (float)h_K[3]; cam.po = pixel_offset;
  CPPF_CHECK_ARG(trk_positive(cam.fx) && trk_positive(cam.fy) && __builtin_isfinite(cam.cx) && __builtin_isfinite(cam.cy));
  CPPF_CHECK_ARG(iters == 0 || h_dk);
  for (int k = 0; k < iters; ++k) CPPF_CHECK_ARG(trk_positive(h_dk[k]));
  if (B == 0) return CPPF_OK;
  CPPF_CHECK_ARG(depth && poses && stats && workspace);
  CPPF_CHECK_ARG(workspace_bytes >= cppf_tsdf_track_workspace_bytes(B, H, W, stride));
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  for (int k = 0; k < iters; ++k) {
    hipLaunchKernelGGL(track_accum_kernel, dim3((unsigned)nblk, B), dim3(TRK_THREADS), 0, st, depth, masks, H, W, stride, cam, acc,
                       wsum, g, trunc, min_weight, h_dk[k], (const double*)poses, (int)nblk, part);
    CPPF_LAUNCH_CHECK();
    hipLaunchKernelGGL(track_solve_kernel, dim3(B), dim3(CPPF_WAVE), 0, st, (int)nblk, (const double*)part, k, poses, stats);
    CPPF_LAUNCH_CHECK();
  }
  return CPPF_OK;
}
