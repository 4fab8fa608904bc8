// BOP pose-error metrics (Hodan et al., "On Evaluation of 6D Object Pose Estimation", ECCVW 2016; the BOP'19 variants): VSD as
// integer pixel counts, MSSD and MSPD as a maximum over the model's vertices and a minimum over its symmetry transforms.  The
// reference has no such scorer; cppf2_amd/bop.py drives both entry points.  gfx950 only.
//
// cppf_vsd_counts: one launch after a clear of the output, grid (nbx, P), 256 threads; the nbx blocks of pair p stride over its
//   pixels.  Each wavefront counts its pixels with ballots (lane k of the wavefront keeps count k), the 4 wavefronts' counts are
//   added in LDS and each block adds its non-zero sums to counts[p] with 64-bit integer atomics: integer sums, so the counts do
//   not depend on the grid, the batch or the order.  A pair whose test_idx lies outside [0, I) is not counted (its row stays 0).
//   Arithmetic per pixel (r, c) of pair p (tests/bop_ref.py restates it; the build's -ffp-contract=off keeps every operation
//   where it is written):
//     float64:  x = ((double)c - cx) / fx,  y = ((double)r - cy) / fy,  f = sqrt((x*x + y*y) + 1),
//               D_t = (double)d_test * f,  D_e = (double)d_est * f,  D_g = (double)d_gt * f,
//               thr_k = (double)taus[k] * (double)diameter[p]
//     vis_gt  = d_gt > 0 && (D_g - D_t <= delta || d_test == 0)
//     vis_est = (d_est > 0 && (D_e - D_t <= delta || d_test == 0)) || (vis_gt && d_est > 0)
//     counts[p] = (union: vis_gt || vis_est, inter: vis_gt && vis_est, cost_k: inter && |D_g - D_e| >= thr_k)
//   (d > 0 and d == 0 compared in float32; fx, fy, cx, cy and delta are the caller's doubles.)
//
// cppf_mssd_mspd: one launch after the outputs are set to +inf, grid (ceil(S / SC), P), 256 threads = SC symmetry lanes x
//   (256 / SC) vertex groups, SC the smallest power of two >= min(S, 64).  Thread (s, g) forms the maps of pair p and symmetry s
//   in float64 and rounds them to float32 once:  [G | h] = [R_g | t_g] [R_s | t_s] (the gt pose after the symmetry; each entry
//   (g0*s0 + g1*s1) + g2*s2, then + t_g), E = [R_e | t_e], A = E - [G | h]; then it streams the vertices through LDS (tiles of
//   BOP_TILE float4) and keeps, over its vertices v = g, g + 256/SC, ...:
//     float32:  d = A v (each row ((a0*x + a1*y) + a2*z) + a3),  m1 = max (d.x*d.x + d.y*d.y) + d.z*d.z
//               e = E v, q = [G | h] v (same row order),  +inf if !(e.z > 0) || !(q.z > 0), else
//               u = fx * (e.x * (1/e.z) - q.x * (1/q.z)),  w = fy * (e.y * (1/e.z) - q.y * (1/q.z)),  m2 = max u*u + w*w
//   (a NaN square counts as +inf; fx, fy rounded to float32).  The groups' maxima meet in LDS; each symmetry lane takes sqrt of
//   its maxima and lowers mssd[p] / mspd[p] with an integer atomic minimum on the float bits.  Max and min of non-negative floats
//   are exact, so the result does not depend on the grid, the batch or the order.
//
// cppf_gt_visibility: which part of a ground-truth instance the test image shows (BOP's scene_gt_info and mask_visib).  One launch
//   after the counts are cleared and the box slots set to INT_MAX, grid (nbx, G), 256 threads; the nbx blocks of instance g stride
//   over its pixels in groups of 4 consecutive ones per lane, the groups laid so that a whole group's 4 mask bytes are one aligned
//   32-bit vector store (the first and last group of an instance may be partial and are stored byte by byte).  Per pixel (r, c),
//   with exactly the conversion and the vis_gt rule above (d_gt = the instance's render alone):
//     all = d_gt > 0,  valid = all && d_test > 0,  visib = all && (D_g - D_t <= delta || d_test == 0)
//   (a pixel with d_gt == 0 is none of the three, so its float64 part is skipped).  Each wavefront counts with ballots, the 4
//   wavefronts meet in LDS, and each block adds its sums with one 64-bit integer atomic per count; the box corners (min column,
//   min row, -(max column), -(max row) of `all`, then of `visib`) are lowered with integer atomic minima.  The add to counts[g][0]
//   carries a ticket in bits 40 and up (H * W <= 2^26, nbx <= 64): the block that draws the last ticket of its instance -- after
//   every other block's atomics, fenced -- removes the ticket bits and turns the corners into (x, y, w, h), (-1, -1, -1, -1) for
//   an empty set, all with atomics, so no workspace and no second launch is needed.  Integer sums and minima: the outputs do not
//   depend on the grid, the batch or the order.  An instance whose img_idx lies outside [0, I) reads nothing: counts 0, boxes -1,
//   mask 0.  bbox_obj here is the box of the in-image part; bop_toolkit renders on an enlarged canvas and reports the box of
//   the whole projection, so the two differ for an instance cut by the image border.
#include "cppf_common.h"
#include <limits.h>

#define BOP_THREADS 256
#define BOP_TILE 1024            // vertices per LDS tile (16 KiB of float4)
#define VSD_MAX_TAUS 32
#define VSD_MAX_BLOCKS 64        // blocks per pair at most (each strides over the pair's pixels)
#define BOP_MAX_DIM 8192         // H, W (the renderer's limit): H * W fits int32
#define BOP_MAX_SYMS (1 << 24)
#define BOP_SC_LOG2_MAX 6        // at most 64 symmetry lanes per block
#define GTV_PX 4                 // consecutive pixels per lane and step: one 32-bit store of mask bytes
#define GTV_TICKET_SHIFT 40      // counts[g][0] carries the blocks' tickets above the pixel count (H * W <= 2^26)

__global__ __launch_bounds__(BOP_THREADS) void vsd_counts_kernel(const float* __restrict__ depth_test, int I,
                                                                 const int32_t* __restrict__ test_idx,
                                                                 const float* __restrict__ depth_est,
                                                                 const float* __restrict__ depth_gt, int H, int W, double fx,
                                                                 double fy, double cx, double cy, double delta,
                                                                 const float* __restrict__ diameter, const float* __restrict__ taus,
                                                                 int n_taus, unsigned long long* __restrict__ counts) {
  __shared__ double s_thr[VSD_MAX_TAUS];
  __shared__ uint32_t s_c[BOP_THREADS / CPPF_WAVE][VSD_MAX_TAUS + 2];
  const int p = blockIdx.y;
  const int ti = test_idx[p];
  if (ti < 0 || ti >= I) return;                       // the same for the whole block
  if (threadIdx.x < n_taus) s_thr[threadIdx.x] = (double)taus[threadIdx.x] * (double)diameter[p];
  __syncthreads();
  const int HW = H * W;
  const float* dt = depth_test + (int64_t)ti * HW;
  const float* de = depth_est + (int64_t)p * HW;
  const float* dg = depth_gt + (int64_t)p * HW;
  const int lane = wave_lane(), w = threadIdx.x / CPPF_WAVE;
  uint32_t mine = 0;                                   // lane k: count k of this wavefront (k < 2 + n_taus)
  for (int i0 = blockIdx.x * BOP_THREADS; i0 < HW; i0 += gridDim.x * BOP_THREADS) {
    const int i = i0 + threadIdx.x;
    bool vg = false, ve = false;
    double diff = 0.0;
    if (i < HW) {
      const int r = i / W, c = i - r * W;
      const float t = dt[i], e = de[i], g = dg[i];
      const double x = ((double)c - cx) / fx, y = ((double)r - cy) / fy;
      const double f = sqrt((x * x + y * y) + 1.0);
      const double Dt = (double)t * f, De = (double)e * f, Dg = (double)g * f;
      vg = g > 0.0f && (Dg - Dt <= delta || t == 0.0f);
      ve = (e > 0.0f && (De - Dt <= delta || t == 0.0f)) || (vg && e > 0.0f);
      diff = fabs(Dg - De);
    }
    const bool in = vg && ve;
    const uint32_t nu = (uint32_t)__popcll(wave_ballot(vg || ve)), ni = (uint32_t)__popcll(wave_ballot(in));
    mine += lane == 0 ? nu : (lane == 1 ? ni : 0u);
    for (int k = 0; k < n_taus; ++k) {
      const uint32_t nk = (uint32_t)__popcll(wave_ballot(in && diff >= s_thr[k]));
      mine += lane == 2 + k ? nk : 0u;
    }
  }
  if (lane < 2 + n_taus) s_c[w][lane] = mine;
  __syncthreads();
  if (threadIdx.x < 2 + n_taus) {
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < BOP_THREADS / CPPF_WAVE; ++k) s += s_c[k][threadIdx.x];
    if (s) atomicAdd(&counts[(int64_t)p * (2 + n_taus) + threadIdx.x], s);
  }
}

__device__ __forceinline__ float bop_row(const float* m, float x, float y, float z) {
  return ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
}

__global__ __launch_bounds__(BOP_THREADS) void mssd_mspd_kernel(const float* __restrict__ verts, int V,
                                                                const double* __restrict__ pose_est,
                                                                const double* __restrict__ pose_gt,
                                                                const double* __restrict__ syms, int S, int sc_log2, float fx,
                                                                float fy, unsigned int* __restrict__ mssd,
                                                                unsigned int* __restrict__ mspd) {
  __shared__ float4 s_v[BOP_TILE];
  __shared__ float s_m[2][BOP_THREADS];
  const int p = blockIdx.y;
  const int SC = 1 << sc_log2, G = BOP_THREADS >> sc_log2;
  const int sl = threadIdx.x & (SC - 1), g = threadIdx.x >> sc_log2;
  const int s = blockIdx.x * SC + sl;
  const bool valid = s < S;
  const double* Pe = pose_est + 12 * (int64_t)p;
  const double* Pg = pose_gt + 12 * (int64_t)p;
  const double* Ps = syms + 12 * (int64_t)(valid ? s : 0);
  float me[12], mg[12], ma[12];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double v = (Pg[4 * r] * Ps[c] + Pg[4 * r + 1] * Ps[4 + c]) + Pg[4 * r + 2] * Ps[8 + c];
      if (c == 3) v = v + Pg[4 * r + 3];
      me[4 * r + c] = (float)Pe[4 * r + c];
      mg[4 * r + c] = (float)v;
      ma[4 * r + c] = (float)(Pe[4 * r + c] - v);
    }
  }
  float m1 = 0.0f, m2 = 0.0f;
  for (int j0 = 0; j0 < V; j0 += BOP_TILE) {
    const int cnt = min(BOP_TILE, V - j0);
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += BOP_THREADS) {
      const float* v = verts + 3 * (int64_t)(j0 + j);
      s_v[j] = make_float4(v[0], v[1], v[2], 0.0f);
    }
    __syncthreads();
    if (valid) {
      for (int j = g; j < cnt; j += G) {
        const float4 v = s_v[j];
        const float dx = bop_row(ma, v.x, v.y, v.z), dy = bop_row(ma + 4, v.x, v.y, v.z), dz = bop_row(ma + 8, v.x, v.y, v.z);
        float d2 = (dx * dx + dy * dy) + dz * dz;
        d2 = d2 == d2 ? d2 : __builtin_inff();
        m1 = fmaxf(m1, d2);
        const float ez = bop_row(me + 8, v.x, v.y, v.z), qz = bop_row(mg + 8, v.x, v.y, v.z);
        float e2 = __builtin_inff();
        if (ez > 0.0f && qz > 0.0f) {
          const float ie = 1.0f / ez, iq = 1.0f / qz;
          const float u = fx * (bop_row(me, v.x, v.y, v.z) * ie - bop_row(mg, v.x, v.y, v.z) * iq);
          const float w = fy * (bop_row(me + 4, v.x, v.y, v.z) * ie - bop_row(mg + 4, v.x, v.y, v.z) * iq);
          e2 = u * u + w * w;
          e2 = e2 == e2 ? e2 : __builtin_inff();
        }
        m2 = fmaxf(m2, e2);
      }
    }
  }
  s_m[0][threadIdx.x] = m1;
  s_m[1][threadIdx.x] = m2;
  __syncthreads();
  if (g == 0 && valid) {
    for (int k = 1; k < G; ++k) {
      m1 = fmaxf(m1, s_m[0][k * SC + sl]);
      m2 = fmaxf(m2, s_m[1][k * SC + sl]);
    }
    atomicMin(&mssd[p], __float_as_uint(sqrtf(m1)));
    atomicMin(&mspd[p], __float_as_uint(sqrtf(m2)));
  }
}

__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(BOP_THREADS) void gt_visibility_kernel(const float* __restrict__ depth_test, int I,
                                                                    const int32_t* __restrict__ img_idx,
                                                                    const float* __restrict__ renders, int H, int W, double fx,
                                                                    double fy, double cx, double cy, double delta,
                                                                    unsigned long long* __restrict__ counts, int* __restrict__ bbox,
                                                                    uint8_t* __restrict__ mask_visib) {
  __shared__ uint32_t s_c[BOP_THREADS / CPPF_WAVE][3];
  __shared__ int s_b[8];
  __shared__ int s_last;
  const int g = blockIdx.y;
  const int ti = img_idx[g];
  const bool ok = ti >= 0 && ti < I;                   // the same for the whole block
  const int HW = H * W;
  const float* dt = depth_test + (int64_t)(ok ? ti : 0) * HW;
  const float* dg = renders + (int64_t)g * HW;
  uint8_t* mk = mask_visib ? mask_visib + (int64_t)g * HW : nullptr;
  // group q holds pixels 4q - m .. 4q - m + 3: m = the mask row's misalignment, so that mk + 4q - m is 4-byte aligned
  const int m = (VEC || !mk) ? 0 : (int)((uintptr_t)mk & 3);
  const int nq = (HW + m + GTV_PX - 1) / GTV_PX;
  const int lane = wave_lane(), w = threadIdx.x / CPPF_WAVE;
  if (threadIdx.x < 8) s_b[threadIdx.x] = INT_MAX;
  uint32_t mine = 0;                                   // lane k < 3: count k of this wavefront
  int b[8];                                            // this lane's corners: (min c, min r, -max c, -max r) of all, of visib
#pragma unroll
  for (int k = 0; k < 8; ++k) b[k] = INT_MAX;
  for (int q0 = blockIdx.x * BOP_THREADS; q0 < nq; q0 += gridDim.x * BOP_THREADS) {
    const int q = q0 + threadIdx.x;
    const int i0 = GTV_PX * q - m;
    const bool have = q < nq;
    const bool whole = have && i0 >= 0 && i0 + GTV_PX - 1 < HW;
    float t[GTV_PX], d[GTV_PX];
    if (VEC) {                                         // HW % 4 == 0 and 16-byte aligned rows: every group is whole
      float4 t4 = make_float4(0.f, 0.f, 0.f, 0.f), d4 = t4;
      if (have && ok) {
        t4 = *reinterpret_cast<const float4*>(dt + i0);
        d4 = *reinterpret_cast<const float4*>(dg + i0);
      }
      t[0] = t4.x; t[1] = t4.y; t[2] = t4.z; t[3] = t4.w;
      d[0] = d4.x; d[1] = d4.y; d[2] = d4.z; d[3] = d4.w;
    } else {
#pragma unroll
      for (int j = 0; j < GTV_PX; ++j) {
        const int i = i0 + j;
        const bool in = have && ok && i >= 0 && i < HW;
        t[j] = in ? dt[i] : 0.0f;
        d[j] = in ? dg[i] : 0.0f;
      }
    }
    uint32_t bytes = 0;
#pragma unroll
    for (int j = 0; j < GTV_PX; ++j) {
      const bool all = d[j] > 0.0f;                    // (pixels outside the instance were read as 0)
      const bool valid = all && t[j] > 0.0f;
      bool visib = false;
      if (all) {
        const int i = i0 + j;
        const int r = i / W, c = i - r * W;
        const double x = ((double)c - cx) / fx, y = ((double)r - cy) / fy;
        const double f = sqrt((x * x + y * y) + 1.0);
        const double Dt = (double)t[j] * f, Dg = (double)d[j] * f;
        visib = Dg - Dt <= delta || t[j] == 0.0f;
        b[0] = min(b[0], c); b[1] = min(b[1], r); b[2] = min(b[2], -c); b[3] = min(b[3], -r);
        if (visib) { b[4] = min(b[4], c); b[5] = min(b[5], r); b[6] = min(b[6], -c); b[7] = min(b[7], -r); }
      }
      const uint32_t na = (uint32_t)__popcll(wave_ballot(all)), nv = (uint32_t)__popcll(wave_ballot(valid)),
                     ns = (uint32_t)__popcll(wave_ballot(visib));
      mine += lane == 0 ? na : (lane == 1 ? nv : (lane == 2 ? ns : 0u));
      bytes |= visib ? 0xffu << (8 * j) : 0u;
    }
    if (mk) {
      if (whole) {
        *reinterpret_cast<uint32_t*>(mk + i0) = bytes;
      } else if (have) {
#pragma unroll
        for (int j = 0; j < GTV_PX; ++j)
          if (i0 + j >= 0 && i0 + j < HW) mk[i0 + j] = (uint8_t)(bytes >> (8 * j));
      }
    }
  }
  if (lane < 3) s_c[w][lane] = mine;
  __syncthreads();                                     // s_b is set, s_c is written
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int v = wave_min_i32(b[k]);
    if (lane == 0 && v != INT_MAX) atomicMin(&s_b[k], v);
  }
  __syncthreads();
  unsigned long long sum = 0;
  if (threadIdx.x < 3) {
#pragma unroll
    for (int k = 0; k < BOP_THREADS / CPPF_WAVE; ++k) sum += s_c[k][threadIdx.x];
    if (threadIdx.x > 0 && sum) atomicAdd(&counts[(int64_t)g * 3 + threadIdx.x], sum);
  }
  if (threadIdx.x < 8 && s_b[threadIdx.x] != INT_MAX) atomicMin(&bbox[(int64_t)g * 8 + threadIdx.x], s_b[threadIdx.x]);
  __threadfence();                                     // this block's atomics before its ticket
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long old = atomicAdd(&counts[(int64_t)g * 3], sum + (1ull << GTV_TICKET_SHIFT));
    s_last = (int)(old >> GTV_TICKET_SHIFT) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();                                     // the last ticket: every block's atomics are done
  if (threadIdx.x < 2) {                               // one lane per box; reads and writes are atomics (they bypass this XCD's L2 lines)
    int* bb = bbox + (int64_t)g * 8 + 4 * threadIdx.x;
    const int c0 = atomicMin(&bb[0], INT_MAX), r0 = atomicMin(&bb[1], INT_MAX);
    const int c1 = atomicMin(&bb[2], INT_MAX), r1 = atomicMin(&bb[3], INT_MAX);
    const bool empty = c0 == INT_MAX;
    atomicExch(&bb[0], empty ? -1 : c0);
    atomicExch(&bb[1], empty ? -1 : r0);
    atomicExch(&bb[2], empty ? -1 : -c1 - c0 + 1);
    atomicExch(&bb[3], empty ? -1 : -r1 - r0 + 1);
  } else if (threadIdx.x == 2) {
    atomicAnd(&counts[(int64_t)g * 3], (1ull << GTV_TICKET_SHIFT) - 1);
  }
}

static bool bop_k_ok(const double* h_K) {
  if (!h_K) return false;
  for (int i = 0; i < 4; ++i)
    if (!(fabs(h_K[i]) < 1e30)) return false;
  return h_K[0] > 0.0 && h_K[1] > 0.0;
}

extern "C" int cppf_vsd_counts(int P, int I, int H, int W, const float* depth_test, const int32_t* test_idx, const float* depth_est,
                               const float* depth_gt, const double* h_K, double delta, const float* diameter, const float* taus,
                               int n_taus, int64_t* counts, void* stream) {
  CPPF_CHECK_ARG(P >= 0 && P <= 65535);
  CPPF_CHECK_ARG(I >= 1 && H >= 1 && W >= 1 && H <= BOP_MAX_DIM && W <= BOP_MAX_DIM);
  CPPF_CHECK_ARG(n_taus >= 1 && n_taus <= VSD_MAX_TAUS);
  CPPF_CHECK_ARG(bop_k_ok(h_K));
  CPPF_CHECK_ARG(fabs(delta) < 1e30);
  if (P == 0) return CPPF_OK;
  CPPF_CHECK_ARG(depth_test && test_idx && depth_est && depth_gt && diameter && taus && counts);
  hipStream_t st = (hipStream_t)stream;
  CPPF_HIP(hipMemsetAsync(counts, 0, (size_t)P * (2 + n_taus) * sizeof(int64_t), st));
  const int blocks = (H * W + BOP_THREADS - 1) / BOP_THREADS;
  const int nbx = blocks < VSD_MAX_BLOCKS ? blocks : VSD_MAX_BLOCKS;
  hipLaunchKernelGGL(vsd_counts_kernel, dim3(nbx, P), dim3(BOP_THREADS), 0, st, depth_test, I, test_idx, depth_est, depth_gt, H, W,
                     h_K[0], h_K[1], h_K[2], h_K[3], delta, diameter, taus, n_taus, (unsigned long long*)counts);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}

extern "C" int cppf_mssd_mspd(int P, const float* verts, int V, const double* syms, int S, const double* pose_est,
                              const double* pose_gt, const double* h_K, float* mssd, float* mspd, void* stream) {
  CPPF_CHECK_ARG(P >= 0 && P <= 65535);
  CPPF_CHECK_ARG(V >= 1 && S >= 1 && S <= BOP_MAX_SYMS);
  CPPF_CHECK_ARG(bop_k_ok(h_K));
  if (P == 0) return CPPF_OK;
  CPPF_CHECK_ARG(verts && syms && pose_est && pose_gt && mssd && mspd);
  hipStream_t st = (hipStream_t)stream;
  CPPF_HIP(hipMemsetD32Async((hipDeviceptr_t)mssd, 0x7f800000, (size_t)P, st));        // +inf
  CPPF_HIP(hipMemsetD32Async((hipDeviceptr_t)mspd, 0x7f800000, (size_t)P, st));
  int sc_log2 = 0;
  while ((1 << sc_log2) < S && sc_log2 < BOP_SC_LOG2_MAX) ++sc_log2;
  const int chunks = (S + (1 << sc_log2) - 1) >> sc_log2;
  hipLaunchKernelGGL(mssd_mspd_kernel, dim3(chunks, P), dim3(BOP_THREADS), 0, st, verts, V, pose_est, pose_gt, syms, S, sc_log2,
                     (float)h_K[0], (float)h_K[1], (unsigned int*)mssd, (unsigned int*)mspd);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}

extern "C" int cppf_gt_visibility(int G, int I, int H, int W, const float* depth_test, const int32_t* img_idx, const float* renders,
                                  const double* h_K, double delta, int64_t* counts, int32_t* bbox, uint8_t* mask_visib,
                                  void* stream) {
  CPPF_CHECK_ARG(G >= 0 && G <= 65535);
  CPPF_CHECK_ARG(I >= 1 && H >= 1 && W >= 1 && H <= BOP_MAX_DIM && W <= BOP_MAX_DIM);
  CPPF_CHECK_ARG(bop_k_ok(h_K));
  CPPF_CHECK_ARG(fabs(delta) < 1e30);
  if (G == 0) return CPPF_OK;
  CPPF_CHECK_ARG(depth_test && img_idx && renders && counts && bbox);
  hipStream_t st = (hipStream_t)stream;
  CPPF_HIP(hipMemsetAsync(counts, 0, (size_t)G * 3 * sizeof(int64_t), st));
  CPPF_HIP(hipMemsetD32Async((hipDeviceptr_t)bbox, INT_MAX, (size_t)G * 8, st));
  const int HW = H * W;
  const int blocks = (HW / GTV_PX + 1 + BOP_THREADS - 1) / BOP_THREADS;
  const int nbx = blocks < VSD_MAX_BLOCKS ? blocks : VSD_MAX_BLOCKS;
  // whole groups everywhere and float4 loads: every row of every array starts on a 16-byte (mask: 4-byte) boundary
  const bool vec = HW % GTV_PX == 0 && ((uintptr_t)depth_test | (uintptr_t)renders) % 16 == 0 && (uintptr_t)mask_visib % 4 == 0;
  auto kernel = vec ? gt_visibility_kernel<true> : gt_visibility_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(nbx, G), dim3(BOP_THREADS), 0, st, depth_test, I, img_idx, renders, H, W, h_K[0], h_K[1], h_K[2],
                     h_K[3], delta, (unsigned long long*)counts, (int*)bbox, mask_visib);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
