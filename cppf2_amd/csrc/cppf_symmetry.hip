// One-sided Hausdorff deviation of a sampled surface to a triangle mesh under many candidate rigid maps: the statistic
// cppf2_amd/symmetry.py searches a mesh's rotational symmetries with.  The reference has no such step.
// gfx950 only.
//
// cppf_sym_deviation: one launch after a clear of the output, grid (ceil(nq / 256), nc), 256 threads, one query per thread.
//   The triangles go through LDS in tiles of SYM_TILE (thread j of the block stages triangle j of the tile: its three vertices
//   and its two edge vectors, 4 float4); in the loop every lane reads the same triangle, so each LDS read is a broadcast.  Each
//   thread keeps the smallest squared distance of its mapped query to a triangle; the block's largest one is found by a
//   wavefront butterfly and 4 LDS words and raised into max_d2[c] with an integer atomic maximum on the bits of the
//   non-negative float.  A maximum of non-negative floats is exact, so the result does not depend on the grid, the batch or
//   the order.  No float atomics, no float64 in the loop.
// Arithmetic (tests/symmetry_ref.py restates it in NumPy; the build's -ffp-contract=off keeps every operation where it is
// written, and the divide is correctly rounded).  All float32; dot(u, w) = (u.x*w.x + u.y*w.y) + u.z*w.z:
//   M = (float)maps[c] (12 entries, rounded once),  q = the query,
//   m.x = ((M0*q.x + M1*q.y) + M2*q.z) + M3,  m.y and m.z with rows 1 and 2
//   per triangle (a, b, c):  ab = b - a, ac = c - a (at staging);  ap = m - a, bp = m - b, cp = m - c,
//     d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp),
//     vc = d1*d4 - d3*d2,  vb = d5*d2 - d1*d6,  va = d3*d6 - d5*d4,  e43 = d4 - d3,  e56 = d5 - d6
//   the region, the first rule that holds (Ericson, "Real-Time Collision Detection", 5.1.5), as (nv, nw, den):
//     A:    d1 <= 0 && d2 <= 0                  (0, 0, 1)
//     B:    d3 >= 0 && d4 <= d3                 (1, 0, 1)
//     AB:   vc <= 0 && d1 >= 0 && d3 <= 0       (d1, 0, d1 - d3)
//     C:    d6 >= 0 && d5 <= d6                 (0, 1, 1)
//     AC:   vb <= 0 && d2 >= 0 && d6 <= 0       (0, d2, d2 - d6)
//     BC:   va <= 0 && e43 >= 0 && e56 >= 0     (-, e43, e43 + e56)
//     face: otherwise                           (vb, vc, (va + vb) + vc)
//   r = 1 / den,  w = nw * r,  v = nv * r  (BC: v = 1 - w);  the closest point is a + v ab + w ac, and
//   e.x = (ap.x - ab.x*v) - ac.x*w  (e.y, e.z alike),  d2 = (e.x*e.x + e.y*e.y) + e.z*e.z
//   best starts at +inf and is lowered only by d2 < best, so a NaN d2 (a non-finite query or map; a triangle without area,
//   whose den is 0) is ignored; a query none of whose distances is a number keeps +inf.  max_d2[c] = max over the queries of best.
#include "cppf_common.h"

#define SYM_THREADS 256
#define SYM_TILE 256             // triangles per LDS tile (16 KiB of 4 float4 each): one per thread at staging
#define SYM_MAX_MAPS 65535       // grid.y

__device__ __forceinline__ float sym_dot(float ux, float uy, float uz, float wx, float wy, float wz) {
  return (ux * wx + uy * wy) + uz * wz;
}

__global__ __launch_bounds__(SYM_THREADS) void sym_deviation_kernel(const float* __restrict__ queries, int nq,
                                                                    const float* __restrict__ tris, int nf,
                                                                    const double* __restrict__ maps,
                                                                    unsigned int* __restrict__ max_d2) {
  __shared__ float4 s_t[SYM_TILE][4];      // (a, ab.x), (b, ab.y), (c, ab.z), (ac, 0)
  __shared__ unsigned int s_w[SYM_THREADS / CPPF_WAVE];
  const int c = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * SYM_THREADS + threadIdx.x;
  const bool valid = i < nq;
  const double* Mp = maps + 12 * (int64_t)c;
  float M[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) M[k] = (float)Mp[k];
  float mx = 0.0f, my = 0.0f, mz = 0.0f;
  if (valid) {
    const float* q = queries + 3 * i;
    const float x = q[0], y = q[1], z = q[2];
    mx = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
    my = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
    mz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
  }
  float best = __builtin_inff();
  for (int j0 = 0; j0 < nf; j0 += SYM_TILE) {
    const int cnt = min(SYM_TILE, nf - j0);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
      const float* t = tris + 9 * (int64_t)(j0 + (int)threadIdx.x);
      const float ax = t[0], ay = t[1], az = t[2], bx = t[3], by = t[4], bz = t[5], cx = t[6], cy = t[7], cz = t[8];
      s_t[threadIdx.x][0] = make_float4(ax, ay, az, bx - ax);
      s_t[threadIdx.x][1] = make_float4(bx, by, bz, by - ay);
      s_t[threadIdx.x][2] = make_float4(cx, cy, cz, bz - az);
      s_t[threadIdx.x][3] = make_float4(cx - ax, cy - ay, cz - az, 0.0f);
    }
    __syncthreads();
    if (valid) {
#pragma unroll 2
      for (int j = 0; j < cnt; ++j) {
        const float4 A = s_t[j][0], B = s_t[j][1], Cc = s_t[j][2], E = s_t[j][3];
        const float abx = A.w, aby = B.w, abz = Cc.w, acx = E.x, acy = E.y, acz = E.z;
        const float apx = mx - A.x, apy = my - A.y, apz = mz - A.z;
        const float bpx = mx - B.x, bpy = my - B.y, bpz = mz - B.z;
        const float cpx = mx - Cc.x, cpy = my - Cc.y, cpz = mz - Cc.z;
        const float d1 = sym_dot(abx, aby, abz, apx, apy, apz), d2 = sym_dot(acx, acy, acz, apx, apy, apz);
        const float d3 = sym_dot(abx, aby, abz, bpx, bpy, bpz), d4 = sym_dot(acx, acy, acz, bpx, bpy, bpz);
        const float d5 = sym_dot(abx, aby, abz, cpx, cpy, cpz), d6 = sym_dot(acx, acy, acz, cpx, cpy, cpz);
        const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
        const float e43 = d4 - d3, e56 = d5 - d6;
        const bool rA = d1 <= 0.0f && d2 <= 0.0f;
        const bool rB = d3 >= 0.0f && d4 <= d3;
        const bool rAB = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
        const bool rC = d6 >= 0.0f && d5 <= d6;
        const bool rAC = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
        const bool rBC = va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f;
        // the rules from the last to the first: an earlier one overrides
        float nv = vb, nw = vc, den = (va + vb) + vc;
        bool onBC = rBC;
        if (rBC) { nw = e43; den = e43 + e56; }
        if (rAC) { nv = 0.0f; nw = d2; den = d2 - d6; onBC = false; }
        if (rC) { nv = 0.0f; nw = 1.0f; den = 1.0f; onBC = false; }
        if (rAB) { nv = d1; nw = 0.0f; den = d1 - d3; onBC = false; }
        if (rB) { nv = 1.0f; nw = 0.0f; den = 1.0f; onBC = false; }
        if (rA) { nv = 0.0f; nw = 0.0f; den = 1.0f; onBC = false; }
        const float r = 1.0f / den;
        const float w = nw * r;
        const float v = onBC ? 1.0f - w : nv * r;
        const float ex = (apx - abx * v) - acx * w, ey = (apy - aby * v) - acy * w, ez = (apz - abz * v) - acz * w;
        const float dd = (ex * ex + ey * ey) + ez * ez;
        if (dd < best) best = dd;
      }
    }
  }
  unsigned int u = valid ? __float_as_uint(best) : 0u;      // best >= +0 or +inf: the bits order as the values do
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) u = max(u, (unsigned int)__shfl_xor((int)u, off));
  if (wave_lane() == 0) s_w[threadIdx.x / CPPF_WAVE] = u;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < SYM_THREADS / CPPF_WAVE; ++k) u = max(u, s_w[k]);
    atomicMax(&max_d2[c], u);
  }
}

extern "C" int cppf_sym_deviation(const float* queries, int nq, const float* tris, int nf, const double* maps, int nc,
                                  float* max_d2, void* stream) {
  CPPF_CHECK_ARG(nq >= 1);
  CPPF_CHECK_ARG(nf >= 1);
  CPPF_CHECK_ARG(nc >= 0 && nc <= SYM_MAX_MAPS);
  if (nc == 0) return CPPF_OK;
  CPPF_CHECK_ARG(queries && tris && maps && max_d2);
  hipStream_t st = (hipStream_t)stream;
  CPPF_HIP(hipMemsetAsync(max_d2, 0, (size_t)nc * sizeof(float), st));
  const unsigned int nbx = (unsigned int)(((int64_t)nq + SYM_THREADS - 1) / SYM_THREADS);
  hipLaunchKernelGGL(sym_deviation_kernel, dim3(nbx, nc), dim3(SYM_THREADS), 0, st, queries, nq, tris, nf, maps,
                     (unsigned int*)max_d2);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
