// The pose of a depth frame against a signed distance volume with no starting pose: an exhaustive search over NR rotations times
// NT whole-node translations, each candidate scored by counting where P points of the frame fall in the volume (cppf2_amd/
// relocalise.py).  What lets a second sequence of an object that was turned over join the volume of the
// first, and what finds a frame again that cppf_tsdf_track lost.  The reference has no such step.  gfx950 only.
// tests/relocalise_ref.py restates every definition below in NumPy; the build's -ffp-contract=off keeps every operation where it
// is written and the float32 divide is correctly rounded.
//
// One cppf_tsdf_pose_scores call is one launch on the caller's stream:
//   pose_scores  grid NR * ceil(NT / 256) blocks of 256 threads; block b serves rotation r = b / chunks and the offsets
//                [256 (b % chunks), min(NT, 256 (b % chunks + 1))).  The rotation (float64 [9], row-major, model -> camera) is cast
//                to float32 entry by entry.
//     stage      per point p (float32 [3], camera frame), float32, left to right, once per block:
//                d = p - c;  x.x = (R0*d.x + R3*d.y) + R6*d.z,  x.y = (R1*d.x + R4*d.y) + R7*d.z,  x.z = (R2*d.x + R5*d.y) + R8*d.z
//                (cppf_track.hip's expression for R^T d);  q = x + m0;  g.a = (q.a - o.a) / voxel per axis a.
//                The point is OUTSIDE FOR EVERY OFFSET unless |g.a| < 2^20 on every axis (a NaN or an infinity fails; compared in
//                float32 before any cast).  Otherwise fl = floorf(g.a), cell.a = (int)fl, f.a = g.a - fl.  (cell, f) of the block's
//                points live in LDS, 24 bytes a point: the fractions do not depend on the offset, which is the point of stating
//                translations as whole nodes of the model frame.
//     count      one wavefront takes one offset (ox, oy, oz) at a time, its lanes the points 64 at a time: i.a = cell.a + off.a
//                (exact: evaluated modulo 2^32 and compared unsigned, which no sum of |cell| <= 2^20 and an int32 can fool);
//                outside  unless 0 <= i.a <= n.a - 2 on every axis
//                unknown  if any of the 8 corners has wsum < min_weight
//                phi      cppf_track.hip's: t[dx | dy << 1 | dz << 2] = acc / (float)wsum at node (i.x + dx, i.y + dy, i.z + dz),
//                         L(a, b, w) = a + (b - a) * w,
//                         phi = L(L(L(t0,t1,f.x), L(t2,t3,f.x), f.y), L(L(t4,t5,f.x), L(t6,t7,f.x), f.y), f.z)
//                inlier   iff fabsf(trunc * phi) <= tau (a NaN fails), else miss: free space the volume saw, or its deep inside
//                The counts are popcounts of the three ballots; outside = P - (inliers + misses + unknown).  Lane 0 writes the
//                four integers of (r, j).  No atomics, no scratch memory: nothing depends on scheduling.
#include "cppf_common.h"

#include <math.h>

#define RLC_THREADS 256
#define RLC_CHUNK 256                    // offsets per block
#define RLC_MAX_POINTS 2048              // 48 KiB of LDS
#define RLC_MAX_NODES (1LL << 27)        // cppf_fuse.hip's TSDF_MAX_NODES
#define RLC_MAX_CANDIDATES (1LL << 29)   // NR * NT: the output's 4 int32 each stay below 2^31 entries
#define RLC_OUTSIDE INT32_MIN            // cell.x of a point that is outside for every offset (a cell is within +-2^20)

struct RelocGrid {
  float ox, oy, oz, voxel;
  int nx, ny, nz;
};

struct RelocPivot {
  float cx, cy, cz, mx, my, mz;
};

__device__ __forceinline__ float rlc_lerp(float a, float b, float w) { return a + (b - a) * w; }

__global__ __launch_bounds__(RLC_THREADS) void pose_scores_kernel(const float* __restrict__ points, int P,
                                                                  const double* __restrict__ rotations, RelocPivot pv,
                                                                  const int32_t* __restrict__ offsets, int NT, int chunks,
                                                                  const float* __restrict__ acc, const int32_t* __restrict__ wsum,
                                                                  RelocGrid g, float trunc, int min_weight, float tau,
                                                                  int32_t* __restrict__ out) {
  extern __shared__ int32_t s_mem[];                 // [3][P] cells, then [3][P] fractions
  int32_t* s_cell = s_mem;
  float* s_frac = (float*)(s_mem + 3 * P);
  const int r = blockIdx.x / chunks, chunk = blockIdx.x - r * chunks;
  const double* R = rotations + 9 * (int64_t)r;
  const float R0 = (float)R[0], R1 = (float)R[1], R2 = (float)R[2], R3 = (float)R[3], R4 = (float)R[4], R5 = (float)R[5];
  const float R6 = (float)R[6], R7 = (float)R[7], R8 = (float)R[8];
  for (int p = threadIdx.x; p < P; p += RLC_THREADS) {
    const float dx = points[3 * p] - pv.cx, dy = points[3 * p + 1] - pv.cy, dz = points[3 * p + 2] - pv.cz;
    const float xx = (R0 * dx + R3 * dy) + R6 * dz;
    const float xy = (R1 * dx + R4 * dy) + R7 * dz;
    const float xz = (R2 * dx + R5 * dy) + R8 * dz;
    const float qx = xx + pv.mx, qy = xy + pv.my, qz = xz + pv.mz;
    const float gx = (qx - g.ox) / g.voxel, gy = (qy - g.oy) / g.voxel, gz = (qz - g.oz) / g.voxel;
    // compared in float32 first: a huge or NaN coordinate never reaches the cast
    const bool near = fabsf(gx) < 1048576.0f && fabsf(gy) < 1048576.0f && fabsf(gz) < 1048576.0f;
    const float flx = floorf(gx), fly = floorf(gy), flz = floorf(gz);
    s_cell[p] = near ? (int)flx : RLC_OUTSIDE;
    s_cell[P + p] = near ? (int)fly : 0;
    s_cell[2 * P + p] = near ? (int)flz : 0;
    s_frac[p] = gx - flx;
    s_frac[P + p] = gy - fly;
    s_frac[2 * P + p] = gz - flz;
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / CPPF_WAVE), lane = wave_lane();
  const int j0 = chunk * RLC_CHUNK, j1 = min(NT, j0 + RLC_CHUNK);
  const int nyz = g.ny * g.nz;
  const uint32_t mx = (uint32_t)(g.nx - 2), my = (uint32_t)(g.ny - 2), mz = (uint32_t)(g.nz - 2);
  const bool cells = g.nx >= 2 && g.ny >= 2 && g.nz >= 2;          // an axis of one node has no cell at all
  for (int j = j0 + wave; j < j1; j += RLC_THREADS / CPPF_WAVE) {
    const uint32_t ox = (uint32_t)offsets[3 * (int64_t)j], oy = (uint32_t)offsets[3 * (int64_t)j + 1];
    const uint32_t oz = (uint32_t)offsets[3 * (int64_t)j + 2];
    int inliers = 0, misses = 0, unknown = 0;
    for (int p0 = 0; p0 < P; p0 += CPPF_WAVE) {                     // whole wavefronts reach the ballots
      const int p = p0 + lane;
      int state = 0;                                                // 0 outside (or no point), 1 inlier, 2 miss, 3 unknown
      if (p < P && cells) {
        const int32_t cx = s_cell[p];
        const uint32_t ix = (uint32_t)cx + ox, iy = (uint32_t)s_cell[P + p] + oy, iz = (uint32_t)s_cell[2 * P + p] + oz;
        if (cx != RLC_OUTSIDE && ix <= mx && iy <= my && iz <= mz) {
          const float fx = s_frac[p], fy = s_frac[P + p], fz = s_frac[2 * P + p];
          const int lin = ((int)ix * g.ny + (int)iy) * g.nz + (int)iz;          // < 2^27
          float t[8];                    // compile-time indices only (the loop is unrolled): registers, no scratch memory
          bool known = true;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int n = lin + (k & 1) * nyz + ((k >> 1) & 1) * g.nz + ((k >> 2) & 1);
            const int32_t w = wsum[n];
            t[k] = acc[n] / (float)w;
            known = known && w >= min_weight;
          }
          const float phi = rlc_lerp(rlc_lerp(rlc_lerp(t[0], t[1], fx), rlc_lerp(t[2], t[3], fx), fy),
                                     rlc_lerp(rlc_lerp(t[4], t[5], fx), rlc_lerp(t[6], t[7], fx), fy), fz);
          state = !known ? 3 : (fabsf(trunc * phi) <= tau ? 1 : 2);
        }
      }
      inliers += __popcll(wave_ballot(state == 1));
      misses += __popcll(wave_ballot(state == 2));
      unknown += __popcll(wave_ballot(state == 3));
    }
    if (lane == 0) {
      int32_t* o = out + 4 * ((int64_t)r * NT + j);
      o[0] = inliers; o[1] = misses; o[2] = unknown; o[3] = P - ((inliers + misses) + unknown);
    }
  }
}

static bool rlc_positive(float x) { return x > 0.0f && x < INFINITY; }

extern "C" int cppf_tsdf_pose_scores(const float* acc, const int32_t* wsum, const double* h_origin, float voxel, int nx, int ny,
                                     int nz, float trunc, int min_weight, const float* points, int P, const double* rotations,
                                     int NR, const float* h_pivot_cam, const float* h_pivot_model, const int32_t* offsets, int NT,
                                     float tau, int32_t* scores, void* stream) {
  CPPF_CHECK_ARG(P >= 1 && P <= RLC_MAX_POINTS);
  CPPF_CHECK_ARG(NR >= 0 && NT >= 0 && (int64_t)NR * NT <= RLC_MAX_CANDIDATES);
  CPPF_CHECK_ARG(h_origin && h_pivot_cam && h_pivot_model && acc && wsum && points);
  CPPF_CHECK_ARG(nx >= 1 && ny >= 1 && nz >= 1 && rlc_positive(voxel));
  CPPF_CHECK_ARG((int64_t)nx * ny <= RLC_MAX_NODES && (int64_t)nx * ny * nz <= RLC_MAX_NODES);
  RelocGrid g;
  g.ox = (float)h_origin[0]; g.oy = (float)h_origin[1]; g.oz = (float)h_origin[2];
  g.voxel = voxel; g.nx = nx; g.ny = ny; g.nz = nz;
  CPPF_CHECK_ARG(__builtin_isfinite(g.ox) && __builtin_isfinite(g.oy) && __builtin_isfinite(g.oz));
  CPPF_CHECK_ARG(rlc_positive(trunc) && rlc_positive(tau) && min_weight >= 1);
  RelocPivot pv;
  pv.cx = h_pivot_cam[0]; pv.cy = h_pivot_cam[1]; pv.cz = h_pivot_cam[2];
  pv.mx = h_pivot_model[0]; pv.my = h_pivot_model[1]; pv.mz = h_pivot_model[2];
  CPPF_CHECK_ARG(__builtin_isfinite(pv.cx) && __builtin_isfinite(pv.cy) && __builtin_isfinite(pv.cz));
  CPPF_CHECK_ARG(__builtin_isfinite(pv.mx) && __builtin_isfinite(pv.my) && __builtin_isfinite(pv.mz));
  if (NR == 0 || NT == 0) return CPPF_OK;
  CPPF_CHECK_ARG(rotations && offsets && scores);
  const int chunks = (NT + RLC_CHUNK - 1) / RLC_CHUNK;               // NR * chunks <= NR * NT <= 2^29 blocks
  const size_t lds = (size_t)P * 6 * sizeof(int32_t);
  hipLaunchKernelGGL(pose_scores_kernel, dim3((unsigned)((int64_t)NR * chunks)), dim3(RLC_THREADS), lds, (hipStream_t)stream, points, P,
                     rotations, pv, offsets, NT, chunks, acc, wsum, g, trunc, min_weight, tau, scores);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
