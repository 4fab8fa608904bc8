// Point-to-plane ICP of B observed clouds against one model (instance-level pose refinement against the object's mesh; a step
// the reference does not have -- its only refinement is eval.py:319-355, cppf_refine.hip).  gfx950 only.
//
// One cppf_icp_refine call enqueues, for k = 0 .. iters-1, two launches on the caller's stream (no host synchronisation):
//   icp_match  grid (ceil(max_n / 256), B), 256 threads, one observed point per thread.  The pose of the instance (float64 in its
//              CppfSceneResult) is cast to float32 once; the point goes into the model frame, the nearest model sample is found
//              by brute force over the M samples (positions streamed through LDS in tiles of ICP_TILE; the winner's normal is
//              read from global memory after the search, it is the only one needed), and an inlier adds its point-to-plane
//              terms (float64) to 30 block sums: the 21 upper-triangle terms of J^T J (row-major), the 6 of J^T e, the inlier
//              count, sum e^2 and sum |q|^2.  Wavefront sums on the DPP path (a fixed butterfly), then the 4 wavefronts' sums added in
//              wavefront order; each block writes its own workspace slot -- no atomics, so nothing depends on scheduling.
//   icp_solve  one wavefront per instance: the block slots summed in block order, then the minimum-norm Gauss-Newton step of
//              A x = -b (float64, lane 0, matrices in LDS): the unknowns scaled to one unit, S = diag(1/L, 1/L, 1/L, 1, 1, 1) with
//              L^2 = sum |q|^2 / inliers (a rotation times the RMS lever arm is a length), the eigen-decomposition of S A S by
//              cyclic Jacobi, and the pseudo-inverse over the eigenvalues above ICP_TAU * lambda_max; x = S y.  Then the pose is
//              updated in place:  dR = Rodrigues(w), R <- R dR^T, t <- t - R v  (x = [w, v], the new R in the second).
//              Fewer than 6 inliers, no eigenvalue kept (rank 0) or a zero or non-finite step: the pose does not change.
//
// ICP_TAU = 1e-9.  Measured spectra of S A S (eigenvalue / lambda_max, float64): directions that only
// rounding constrains -- a plate's in-plane translation and spin, a smooth cylinder's spin and slide, a smooth sphere's
// rotation -- sit at <= 1.2e-13 (exactly 0 where the normals are exactly axis-aligned); the weakest genuine constraints are a
// faceted sphere cap's rotation (1.1e-6 to 4.7e-5 over poses, 192 segments), a 128-facet cylinder's spin (1.8e-4) and the
// fixture's views (>= 0.12): tau is three orders below the weakest and four above the rounding level.
// A rank-deficient system therefore corrects what it observes and leaves the other directions exactly where they were (the
// step has no component along them), instead of dividing by a rounding-level pivot.
// Arithmetic (tests/icp_ref.py restates it in NumPy; the build's -ffp-contract=off keeps every operation where it is written):
//   float32:  Rf = (float)R, tf = (float)t, d = p - tf,
//             q.x = (Rf00*d.x + Rf10*d.y) + Rf20*d.z,  q.y = (Rf01*d.x + Rf11*d.y) + Rf21*d.z,  q.z = (Rf02*d.x + Rf12*d.y) + Rf22*d.z
//             d2(j) = ((q.x - m.x)^2 + (q.y - m.y)^2) + (q.z - m.z)^2;  nearest = the lowest j of the smallest d2 (strict '<' in
//             index order; a NaN d2 never wins); inlier <=> d2 <= dk * dk  (dk = (float)d_k, the product in float32)
//   float64:  r = q - m,  e = (n.x*r.x + n.y*r.y) + n.z*r.z,  J = [q x n, n],  (q x n) = (q.y*n.z - q.z*n.y, q.z*n.x - q.x*n.z,
//             q.x*n.y - q.y*n.x), |q|^2 = (q.x*q.x + q.y*q.y) + q.z*q.z -- q, m, n widened from float32
//   schedule: d_k = d0 * (d1 / d0)^(k / (iters - 1)) in float64 on the host (d_k = d0 when iters = 1)
//   Rodrigues: th2 = (w0^2 + w1^2) + w2^2; a = sin(th)/th, c = (1 - cos(th))/th2 (a = 1 - th2/6, c = 0.5 - th2/24 when th2 < 1e-8);
//             dR_ij = (delta_ij * (1 - c*th2) + a*K_ij) + (c*w_i)*w_j,  K = [w]x
//   solve:    L2 = sum|q|^2 / cnt, r = L2 > 0 ? 1 / sqrt(L2) : 0, s = (r, r, r, 1, 1, 1), As_ij = (s_i * A_ij) * s_j, V = I;
//             sweeps (at most ICP_SWEEPS, until one rotates nothing) over (p, q) = (0,1), (0,2), .. (4,5): skip when a_pq == 0
//             or |a_pq| <= ICP_JEPS * (|a_pp| + |a_qq|) (a_pq, a_qp set to 0); else th = (a_qq - a_pp) / (2 a_pq),
//             t = sgn(th) / (|th| + sqrt(th*th + 1)) (sgn(0) = 1), c = 1 / sqrt(t*t + 1), s = t * c, a_pp -= t a_pq, a_qq += t a_pq,
//             a_pq = a_qp = 0, for k != p, q: a_kp = a_pk = c a_kp - s a_kq, a_kq = a_qk = s a_kp + c a_kq (old values), and for
//             every k: V_kp = c V_kp - s V_kq, V_kq = s V_kp + c V_kq.  lmax = the largest a_ii; i in ascending order with
//             a_ii > ICP_TAU * lmax: g = sum_j V_ji (s_j b_j) (j ascending, from 0), y_j += (-g / a_ii) V_ji; x_j = s_j y_j.
// Stats per instance (float32, written every iteration, final after the last): [0] inliers of the last match, [1] sqrt(sum e^2 /
// inliers) of that match (0 without inliers), [2] inliers / n, [3] iterations with a non-zero step (those that moved the pose).
//
// cppf_icp_refine_depth adds the other direction, model to depth image: three launches per iteration,
//   icp_match    as above (skipped when max_n == 0), writing slots [0, nblk) of the instance's row of nblk + mblk slots,
//   icp_project  grid (ceil(M / 256), B), 256 threads, one model sample per thread, writing slots [nblk, nblk + mblk): the sample
//                goes into the camera frame, a front-facing one in front of the camera is projected to its pixel, the depth read
//                there is back-projected, and when that observed point lies within d_k of the sample it adds the same
//                point-to-plane terms, times model_weight, by the same reduction.  No z-buffer: a sample hidden by another part
//                of the object meets the nearer surface at its pixel, and the distance gate drops it.
//   icp_solve    the same solve over the row's observed slots and then its model slots, in slot order.
// Arithmetic of icp_project (tests/icp_depth_ref.py restates it):
//   float32:  Rf, tf as above; fx, fy, cx, cy = (float)K once on the host;  m, n the sample and its normal,
//             p.x = ((Rf00*m.x + Rf01*m.y) + Rf02*m.z) + tf.x, p.y, p.z with rows 1, 2;  nc the same with n and without tf
//             visible <=> p.z > 0 and (nc.x*p.x + nc.y*p.y) + nc.z*p.z < 0
//             col = rintf(fx * p.x / p.z + cx), row = rintf(fy * p.y / p.z + cy)  (the product, the quotient, the sum; ties to
//             even); in the image <=> 0 <= col < W and 0 <= row < H  (pixel (r, c) back-projects through (c, r), the
//             reference's convention);  d = depth[img][row][col], used when finite and > 0
//             o = ((col - cx) * d / fx, (row - cy) * d / fy, d);  inlier <=> ((o.x-p.x)^2 + (o.y-p.y)^2) + (o.z-p.z)^2 <= dk * dk
//             q = Rf^T (o - tf) by the match kernel's expression
//   float64:  e, J, |q|^2 as above with this q and the sample's own m, n.  Slot entries [0, 30): the match kernel's 30 terms, each
//             sample's term times (double)model_weight (the count entry: 1.0 * weight); [30] the plain count; [31] the plain e^2.
//   An instance whose img_idx is outside [0, I) gets zero model slots.  The visible in-image samples of each block are counted
//   into an int32 [B, mblk] table behind the slot rows.
//   solve:    entries [0, 30) summed over the observed slots, then on over the model slots; cnt (the >= 6 test, L2) and the
//             normal equations are those combined weighted sums.
// Stats of cppf_icp_refine_depth (float32 [B,8]): [0..2] as above from the observed slots alone, [3] iterations with a non-zero
// step of the combined system, [4] model-side inliers of the last iteration, [5] sqrt(sum e^2 / inliers) of those (plain sums),
// [6] inliers / visible in-image samples, [7] the visible in-image samples.
#include "cppf_common.h"
#include "cppf_icp_solve.h"

#define ICP_THREADS 256
#define ICP_TILE 1024          // model samples per LDS tile (16 KiB of float4)
#define ICP_SLOT 32            // doubles per block slot
#define ICP_REFINED 16         // CppfSceneResult.flags bit4: pose refined by ICP

__global__ __launch_bounds__(ICP_THREADS) void icp_match_kernel(const float* __restrict__ pts, const int32_t* __restrict__ pt_off,
                                                                int max_n, int nblk, const float* __restrict__ model_pts,
                                                                const float* __restrict__ model_nrm, int M, float thr2,
                                                                const CppfSceneResult* __restrict__ results,
                                                                double* __restrict__ part) {
  __shared__ float4 s_m[ICP_TILE];
  __shared__ double s_w[ICP_THREADS / CPPF_WAVE][ICP_TERMS];
  const int b = blockIdx.y;
  const CppfSceneResult& rec = results[b];
  if (rec.flags & 1) return;
  int n = pt_off[b + 1] - pt_off[b];
  n = n < 0 ? 0 : (n > max_n ? max_n : n);
  const int i0 = blockIdx.x * ICP_THREADS;
  if (i0 >= n) return;
  const int i = i0 + threadIdx.x;
  const bool valid = i < n;
  float Rf[9], tf[3];
#pragma unroll
  for (int c = 0; c < 9; ++c) Rf[c] = (float)rec.R[c];
#pragma unroll
  for (int c = 0; c < 3; ++c) tf[c] = (float)rec.t[c];
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  if (valid) {
    const float* p = pts + 3 * ((int64_t)pt_off[b] + i);
    const float dx = p[0] - tf[0], dy = p[1] - tf[1], dz = p[2] - tf[2];
    qx = (Rf[0] * dx + Rf[3] * dy) + Rf[6] * dz;
    qy = (Rf[1] * dx + Rf[4] * dy) + Rf[7] * dz;
    qz = (Rf[2] * dx + Rf[5] * dy) + Rf[8] * dz;
  }
  float best = __builtin_inff();
  int bi = -1;
  for (int j0 = 0; j0 < M; j0 += ICP_TILE) {
    const int cnt = min(ICP_TILE, M - j0);
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += ICP_THREADS) {
      const float* m = model_pts + 3 * (int64_t)(j0 + j);
      s_m[j] = make_float4(m[0], m[1], m[2], 0.0f);
    }
    __syncthreads();
    if (valid) {
#pragma unroll 4
      for (int j = 0; j < cnt; ++j) {
        const float4 m = s_m[j];
        const float ex = qx - m.x, ey = qy - m.y, ez = qz - m.z;
        const float d2 = (ex * ex + ey * ey) + ez * ez;
        if (d2 < best) {
          best = d2;
          bi = j0 + j;
        }
      }
    }
  }
  double v[ICP_TERMS];
#pragma unroll
  for (int c = 0; c < ICP_TERMS; ++c) v[c] = 0.0;
  if (valid && bi >= 0 && best <= thr2) {
    const double Qx = qx, Qy = qy, Qz = qz;
    const float* mp = model_pts + 3 * (int64_t)bi;
    const float* mn = model_nrm + 3 * (int64_t)bi;
    const double nx = mn[0], ny = mn[1], nz = mn[2];
    const double rx = Qx - (double)mp[0], ry = Qy - (double)mp[1], rz = Qz - (double)mp[2];
    const double e = (nx * rx + ny * ry) + nz * rz;
    const double J[6] = {Qy * nz - Qz * ny, Qz * nx - Qx * nz, Qx * ny - Qy * nx, nx, ny, nz};
    int o = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int c = a; c < 6; ++c) v[o++] = J[a] * J[c];
#pragma unroll
    for (int a = 0; a < 6; ++a) v[21 + a] = J[a] * e;
    v[27] = 1.0;
    v[28] = e * e;
    v[29] = (Qx * Qx + Qy * Qy) + Qz * Qz;
  }
  const int w = threadIdx.x / CPPF_WAVE;
#pragma unroll
  for (int c = 0; c < ICP_TERMS; ++c) {
    const double s = wave_sum(v[c]);
    if (wave_lane() == 0) s_w[w][c] = s;
  }
  __syncthreads();
  if (threadIdx.x < ICP_TERMS) {
    double s = s_w[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < ICP_THREADS / CPPF_WAVE; ++k) s += s_w[k][threadIdx.x];
    part[((int64_t)b * nblk + blockIdx.x) * ICP_SLOT + threadIdx.x] = s;
  }
}

// One model sample per thread against the depth image of the instance (arithmetic in the header).  Every block of a non-empty
// record writes its slot and its visible count, zeros included, so the solve reads nothing unwritten.
__global__ __launch_bounds__(ICP_THREADS) void icp_project_kernel(const float* __restrict__ model_pts,
                                                                  const float* __restrict__ model_nrm, int M,
                                                                  const float* __restrict__ depth, int I, int H, int W,
                                                                  const int32_t* __restrict__ img_idx, float fx, float fy, float cx,
                                                                  float cy, double weight, float thr2, int slots, int nblk,
                                                                  const CppfSceneResult* __restrict__ results,
                                                                  double* __restrict__ part, int32_t* __restrict__ vis) {
  __shared__ double s_w[ICP_THREADS / CPPF_WAVE][ICP_SLOT];
  __shared__ int s_v[ICP_THREADS / CPPF_WAVE];
  const int b = blockIdx.y;
  const CppfSceneResult& rec = results[b];
  if (rec.flags & 1) return;
  const int img = img_idx[b];
  const int i = blockIdx.x * ICP_THREADS + threadIdx.x;
  float Rf[9], tf[3];
#pragma unroll
  for (int c = 0; c < 9; ++c) Rf[c] = (float)rec.R[c];
#pragma unroll
  for (int c = 0; c < 3; ++c) tf[c] = (float)rec.t[c];
  double v[ICP_SLOT];
#pragma unroll
  for (int c = 0; c < ICP_SLOT; ++c) v[c] = 0.0;
  bool seen = false;
  if (i < M && img >= 0 && img < I) {
    const float* mp = model_pts + 3 * (int64_t)i;
    const float* mn = model_nrm + 3 * (int64_t)i;
    const float mx = mp[0], my = mp[1], mz = mp[2], ax = mn[0], ay = mn[1], az = mn[2];
    const float px = ((Rf[0] * mx + Rf[1] * my) + Rf[2] * mz) + tf[0];
    const float py = ((Rf[3] * mx + Rf[4] * my) + Rf[5] * mz) + tf[1];
    const float pz = ((Rf[6] * mx + Rf[7] * my) + Rf[8] * mz) + tf[2];
    const float ncx = (Rf[0] * ax + Rf[1] * ay) + Rf[2] * az;
    const float ncy = (Rf[3] * ax + Rf[4] * ay) + Rf[5] * az;
    const float ncz = (Rf[6] * ax + Rf[7] * ay) + Rf[8] * az;
    if (pz > 0.0f && (ncx * px + ncy * py) + ncz * pz < 0.0f) {
      const float colf = rintf(fx * px / pz + cx), rowf = rintf(fy * py / pz + cy);
      if (colf >= 0.0f && colf < (float)W && rowf >= 0.0f && rowf < (float)H) {       // a NaN fails every comparison
        seen = true;
        const float d = depth[((int64_t)img * H + (int)rowf) * W + (int)colf];
        if (d > 0.0f && d < __builtin_inff()) {
          const float ox = (colf - cx) * d / fx, oy = (rowf - cy) * d / fy;
          const float gx = ox - px, gy = oy - py, gz = d - pz;
          if ((gx * gx + gy * gy) + gz * gz <= thr2) {
            const float dx = ox - tf[0], dy = oy - tf[1], dz = d - tf[2];
            const double Qx = (Rf[0] * dx + Rf[3] * dy) + Rf[6] * dz;
            const double Qy = (Rf[1] * dx + Rf[4] * dy) + Rf[7] * dz;
            const double Qz = (Rf[2] * dx + Rf[5] * dy) + Rf[8] * dz;
            const double nx = ax, ny = ay, nz = az;
            const double rx = Qx - (double)mx, ry = Qy - (double)my, rz = Qz - (double)mz;
            const double e = (nx * rx + ny * ry) + nz * rz;
            const double J[6] = {Qy * nz - Qz * ny, Qz * nx - Qx * nz, Qx * ny - Qy * nx, nx, ny, nz};
            int o = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
              for (int c = a; c < 6; ++c) v[o++] = (J[a] * J[c]) * weight;
#pragma unroll
            for (int a = 0; a < 6; ++a) v[21 + a] = (J[a] * e) * weight;
            v[27] = weight;
            v[28] = (e * e) * weight;
            v[29] = ((Qx * Qx + Qy * Qy) + Qz * Qz) * weight;
            v[30] = 1.0;
            v[31] = e * e;
          }
        }
      }
    }
  }
  const int w = threadIdx.x / CPPF_WAVE;
  const int nseen = __popcll(wave_ballot(seen));
  if (wave_lane() == 0) s_v[w] = nseen;
#pragma unroll
  for (int c = 0; c < ICP_SLOT; ++c) {
    const double s = wave_sum(v[c]);
    if (wave_lane() == 0) s_w[w][c] = s;
  }
  __syncthreads();
  if (threadIdx.x < ICP_SLOT) {
    double s = s_w[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < ICP_THREADS / CPPF_WAVE; ++k) s += s_w[k][threadIdx.x];
    part[((int64_t)b * slots + nblk + blockIdx.x) * ICP_SLOT + threadIdx.x] = s;
  }
  if (threadIdx.x == 0) vis[(int64_t)b * (slots - nblk) + blockIdx.x] = (s_v[0] + s_v[1]) + (s_v[2] + s_v[3]);
}

// One wavefront per instance; lane 0 does the 6x6 solve and the pose update in LDS (cppf_icp_solve.h, shared with
// cppf_track.hip).  DEPTH = false is cppf_icp_refine's solve: rows of nblk observed slots, 4 stats.
// DEPTH = true is cppf_icp_refine_depth's: nblk is the whole row (ceil(max_n / 256) observed slots, then the model slots, then
// behind all rows the visible counts), the sums run on from the observed slots over the model slots, 8 stats.
template <bool DEPTH>
__global__ __launch_bounds__(CPPF_WAVE) void icp_solve_kernel(const int32_t* __restrict__ pt_off, int max_n, int nblk,
                                                              const double* __restrict__ part, int k, int iters,
                                                              CppfSceneResult* __restrict__ results, float* __restrict__ stats) {
  __shared__ double s_t[ICP_SLOT];
  __shared__ double s_o[DEPTH ? ICP_SLOT : 1];
  __shared__ IcpSolveLds L;
  const int b = blockIdx.x;
  CppfSceneResult& rec = results[b];
  float* st = stats + (DEPTH ? 8 : 4) * (int64_t)b;
  if (rec.flags & 1) {
    if (threadIdx.x < (DEPTH ? 8 : 4)) st[threadIdx.x] = 0.0f;
    return;
  }
  int n = pt_off[b + 1] - pt_off[b];
  n = n < 0 ? 0 : (n > max_n ? max_n : n);
  const int nb = (n + ICP_THREADS - 1) / ICP_THREADS;
  const int oblk = DEPTH ? (max_n + ICP_THREADS - 1) / ICP_THREADS : nblk;       // observed slots of a row; the rest: model slots
  if (DEPTH) {
    if (threadIdx.x < ICP_SLOT) {                  // entries 30, 31 exist in the model slots only
      double s = 0.0;
      if (threadIdx.x < ICP_TERMS)
        for (int blk = 0; blk < nb; ++blk) s += part[((int64_t)b * nblk + blk) * ICP_SLOT + threadIdx.x];
      s_o[threadIdx.x] = s;
      for (int blk = oblk; blk < nblk; ++blk) s += part[((int64_t)b * nblk + blk) * ICP_SLOT + threadIdx.x];
      s_t[threadIdx.x] = s;
    }
  } else if (threadIdx.x < ICP_TERMS) {
    double s = 0.0;
    for (int blk = 0; blk < nb; ++blk) s += part[((int64_t)b * nblk + blk) * ICP_SLOT + threadIdx.x];
    s_t[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double cnt = s_t[27];
  const bool ok = cnt >= 6.0 && icp_min_norm_step(s_t, cnt, L);
  if (ok) {
    for (int j = 0; j < 9; ++j) L.R[j] = rec.R[j];
    icp_rotation_update(L);
    for (int r = 0; r < 3; ++r) {
      rec.t[r] = rec.t[r] - ((L.Rn[r * 3] * L.x[3] + L.Rn[r * 3 + 1] * L.x[4]) + L.Rn[r * 3 + 2] * L.x[5]);
      for (int q = 0; q < 3; ++q) rec.R[r * 3 + q] = L.Rn[r * 3 + q];
    }
  }
  const double ocnt = DEPTH ? s_o[27] : cnt, sse = DEPTH ? s_o[28] : s_t[28];
  st[0] = (float)ocnt;
  st[1] = ocnt > 0.0 ? (float)sqrt(sse / ocnt) : 0.0f;
  st[2] = n > 0 ? (float)(ocnt / (double)n) : 0.0f;
  st[3] = (k == 0 ? 0.0f : st[3]) + (ok ? 1.0f : 0.0f);
  if (DEPTH) {
    const int32_t* vis = (const int32_t*)(part + (int64_t)gridDim.x * nblk * ICP_SLOT) + (int64_t)b * (nblk - oblk);
    int seen = 0;
    for (int blk = 0; blk < nblk - oblk; ++blk) seen += vis[blk];
    const double mcnt = s_t[30];
    st[4] = (float)mcnt;
    st[5] = mcnt > 0.0 ? (float)sqrt(s_t[31] / mcnt) : 0.0f;
    st[6] = seen > 0 ? (float)(mcnt / (double)seen) : 0.0f;
    st[7] = (float)seen;
  }
  if (k == iters - 1) rec.flags |= ICP_REFINED;
}

static bool icp_blocks(int B, int max_n, int64_t* nblk) {
  if (B < 1 || B > 65535 || max_n < 1) return false;
  *nblk = ((int64_t)max_n + ICP_THREADS - 1) / ICP_THREADS;
  return true;
}

extern "C" int64_t cppf_icp_workspace_bytes(int B, int max_n) {
  int64_t nblk;
  if (!icp_blocks(B, max_n, &nblk)) return CPPF_EINVAL;
  return (int64_t)B * nblk * ICP_SLOT * (int64_t)sizeof(double);
}

extern "C" int cppf_icp_refine(int B, const float* pts, const int32_t* pt_off, int max_n, const float* model_pts,
                               const float* model_nrm, int M, int iters, float d0, float d1, CppfSceneResult* results,
                               float* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  int64_t nblk;
  CPPF_CHECK_ARG(icp_blocks(B, max_n, &nblk));
  CPPF_CHECK_ARG(pts && pt_off && model_pts && model_nrm && results && stats && workspace);
  CPPF_CHECK_ARG(M > 0 && iters > 0);
  CPPF_CHECK_ARG(d1 > 0.0f && d0 >= d1 && d0 < __builtin_inff());
  const int64_t need = cppf_icp_workspace_bytes(B, max_n);
  if (workspace_bytes < need) {
    snprintf(g_cppf_err, sizeof(g_cppf_err), "%s: workspace of %lld bytes, %lld needed", __func__, (long long)workspace_bytes,
             (long long)need);
    return CPPF_ECAPACITY;
  }
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  for (int k = 0; k < iters; ++k) {
    const double dk = iters == 1 ? (double)d0 : (double)d0 * pow((double)d1 / (double)d0, (double)k / (double)(iters - 1));
    const float dkf = (float)dk;
    const float thr2 = dkf * dkf;
    hipLaunchKernelGGL(icp_match_kernel, dim3((unsigned)nblk, B), dim3(ICP_THREADS), 0, st, pts, pt_off, max_n, (int)nblk, model_pts,
                       model_nrm, M, thr2, results, part);
    CPPF_LAUNCH_CHECK();
    hipLaunchKernelGGL((icp_solve_kernel<false>), dim3(B), dim3(CPPF_WAVE), 0, st, pt_off, max_n, (int)nblk, part, k, iters, results,
                       stats);
    CPPF_LAUNCH_CHECK();
  }
  return CPPF_OK;
}

static bool icp_depth_blocks(int B, int max_n, int M, int64_t* nblk, int64_t* mblk) {
  if (B < 1 || B > 65535 || max_n < 0 || M < 1) return false;
  *nblk = ((int64_t)max_n + ICP_THREADS - 1) / ICP_THREADS;
  *mblk = ((int64_t)M + ICP_THREADS - 1) / ICP_THREADS;
  return *nblk + *mblk <= 0x7fffffff / ICP_SLOT;
}

// B rows of nblk + mblk slots, then the int32 [B, mblk] visible counts (rounded up to whole doubles).
extern "C" int64_t cppf_icp_depth_workspace_bytes(int B, int max_n, int M) {
  int64_t nblk, mblk;
  if (!icp_depth_blocks(B, max_n, M, &nblk, &mblk)) return CPPF_EINVAL;
  return (int64_t)B * (nblk + mblk) * ICP_SLOT * (int64_t)sizeof(double) + ((int64_t)B * mblk * 4 + 7) / 8 * 8;
}

extern "C" int cppf_icp_refine_depth(int B, const float* pts, const int32_t* pt_off, int max_n, const float* model_pts,
                                     const float* model_nrm, int M, const float* depth, int I, int H, int W, const int32_t* img_idx,
                                     const double* K, float model_weight, int iters, float d0, float d1, CppfSceneResult* results,
                                     float* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  int64_t nblk, mblk;
  CPPF_CHECK_ARG(icp_depth_blocks(B, max_n, M, &nblk, &mblk));
  CPPF_CHECK_ARG((pts || max_n == 0) && pt_off && model_pts && model_nrm && results && stats && workspace);
  CPPF_CHECK_ARG(depth && img_idx && K);
  CPPF_CHECK_ARG(I >= 1 && H >= 1 && W >= 1 && (int64_t)I * H * W <= 0x7fffffffffffLL);
  CPPF_CHECK_ARG(iters > 0);
  CPPF_CHECK_ARG(d1 > 0.0f && d0 >= d1 && d0 < __builtin_inff());
  CPPF_CHECK_ARG(K[0] > 0.0 && K[0] < __builtin_inf() && K[4] > 0.0 && K[4] < __builtin_inf());
  CPPF_CHECK_ARG(model_weight > 0.0f && model_weight < __builtin_inff());
  const int64_t need = cppf_icp_depth_workspace_bytes(B, max_n, M);
  if (workspace_bytes < need) {
    snprintf(g_cppf_err, sizeof(g_cppf_err), "%s: workspace of %lld bytes, %lld needed", __func__, (long long)workspace_bytes,
             (long long)need);
    return CPPF_ECAPACITY;
  }
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  const int slots = (int)(nblk + mblk);
  int32_t* vis = (int32_t*)(part + (int64_t)B * slots * ICP_SLOT);
  const float fx = (float)K[0], fy = (float)K[4], cx = (float)K[2], cy = (float)K[5];
  for (int k = 0; k < iters; ++k) {
    const double dk = iters == 1 ? (double)d0 : (double)d0 * pow((double)d1 / (double)d0, (double)k / (double)(iters - 1));
    const float dkf = (float)dk;
    const float thr2 = dkf * dkf;
    if (max_n > 0) {         // the match kernel's nblk is its row length
      hipLaunchKernelGGL(icp_match_kernel, dim3((unsigned)nblk, B), dim3(ICP_THREADS), 0, st, pts, pt_off, max_n, slots, model_pts,
                         model_nrm, M, thr2, results, part);
      CPPF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(icp_project_kernel, dim3((unsigned)mblk, B), dim3(ICP_THREADS), 0, st, model_pts, model_nrm, M, depth, I, H, W,
                       img_idx, fx, fy, cx, cy, (double)model_weight, thr2, slots, (int)nblk, results, part, vis);
    CPPF_LAUNCH_CHECK();
    hipLaunchKernelGGL((icp_solve_kernel<true>), dim3(B), dim3(CPPF_WAVE), 0, st, pt_off, max_n, slots, part, k, iters, results,
                       stats);
    CPPF_LAUNCH_CHECK();
  }
  return CPPF_OK;
}
