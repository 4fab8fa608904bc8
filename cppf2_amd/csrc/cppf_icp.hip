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
#include "cppf_common.h"

#define ICP_THREADS 256
#define ICP_TILE 1024          // model samples per LDS tile (16 KiB of float4)
#define ICP_TERMS 30           // 21 (J^T J upper) + 6 (J^T e) + count + sum e^2 + sum |q|^2
#define ICP_SLOT 32            // doubles per block slot
#define ICP_REFINED 16         // CppfSceneResult.flags bit4: pose refined by ICP
#define ICP_TAU 1e-9           // eigenvalues of S A S at or below ICP_TAU * lambda_max are dropped (unobservable directions)
#define ICP_JEPS 1e-17         // Jacobi: an off-diagonal entry this small next to its two diagonal entries counts as 0
#define ICP_SWEEPS 16          // Jacobi sweeps at most (measured: 3-8, the last of them rotating nothing)

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

// One wavefront per instance; lane 0 does the 6x6 solve and the pose update in LDS (no register array with a loop-varying
// index, so nothing goes to scratch memory).
__global__ __launch_bounds__(CPPF_WAVE) void icp_solve_kernel(const int32_t* __restrict__ pt_off, int max_n, int nblk,
                                                              const double* __restrict__ part, int k, int iters,
                                                              CppfSceneResult* __restrict__ results, float* __restrict__ stats) {
  __shared__ double s_t[ICP_SLOT];
  __shared__ double s_A[36], s_V[36], s_s[6], s_y[6], s_x[6], s_K[9], s_R[9], s_dR[9], s_Rn[9];
  const int b = blockIdx.x;
  CppfSceneResult& rec = results[b];
  float* st = stats + 4 * (int64_t)b;
  if (rec.flags & 1) {
    if (threadIdx.x < 4) st[threadIdx.x] = 0.0f;
    return;
  }
  int n = pt_off[b + 1] - pt_off[b];
  n = n < 0 ? 0 : (n > max_n ? max_n : n);
  const int nb = (n + ICP_THREADS - 1) / ICP_THREADS;
  if (threadIdx.x < ICP_TERMS) {
    double s = 0.0;
    for (int blk = 0; blk < nb; ++blk) s += part[((int64_t)b * nblk + blk) * ICP_SLOT + threadIdx.x];
    s_t[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double cnt = s_t[27], sse = s_t[28];
  bool ok = cnt >= 6.0;
  if (ok) {
    const double L2 = s_t[29] / cnt;
    const double r = L2 > 0.0 ? 1.0 / sqrt(L2) : 0.0;
    for (int j = 0; j < 6; ++j) s_s[j] = j < 3 ? r : 1.0;
    int o = 0;
    for (int a = 0; a < 6; ++a)
      for (int c = a; c < 6; ++c) {
        const double v = (s_s[a] * s_t[o]) * s_s[c];
        s_A[a * 6 + c] = v;
        s_A[c * 6 + a] = v;
        s_V[a * 6 + c] = a == c ? 1.0 : 0.0;
        s_V[c * 6 + a] = a == c ? 1.0 : 0.0;
        ++o;
      }
    for (int sweep = 0; sweep < ICP_SWEEPS; ++sweep) {       // cyclic Jacobi: S A S = V diag(a_ii) V^T
      bool rotated = false;
      for (int p = 0; p < 5; ++p)
        for (int q = p + 1; q < 6; ++q) {
          const double apq = s_A[p * 6 + q], app = s_A[p * 7], aqq = s_A[q * 7];
          if (apq == 0.0) continue;
          if (fabs(apq) <= ICP_JEPS * (fabs(app) + fabs(aqq))) {
            s_A[p * 6 + q] = 0.0;
            s_A[q * 6 + p] = 0.0;
            continue;
          }
          const double th = (aqq - app) / (2.0 * apq);
          const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
          s_A[p * 7] = app - t * apq;
          s_A[q * 7] = aqq + t * apq;
          s_A[p * 6 + q] = 0.0;
          s_A[q * 6 + p] = 0.0;
          for (int k = 0; k < 6; ++k) {
            if (k != p && k != q) {
              const double akp = s_A[k * 6 + p], akq = s_A[k * 6 + q];
              const double np_ = c * akp - sn * akq, nq = sn * akp + c * akq;
              s_A[k * 6 + p] = np_;
              s_A[p * 6 + k] = np_;
              s_A[k * 6 + q] = nq;
              s_A[q * 6 + k] = nq;
            }
            const double vkp = s_V[k * 6 + p], vkq = s_V[k * 6 + q];
            s_V[k * 6 + p] = c * vkp - sn * vkq;
            s_V[k * 6 + q] = sn * vkp + c * vkq;
          }
          rotated = true;
        }
      if (!rotated) break;
    }
    double lmax = 0.0;
    for (int i = 0; i < 6; ++i)
      if (s_A[i * 7] > lmax) lmax = s_A[i * 7];
    for (int j = 0; j < 6; ++j) s_y[j] = 0.0;
    int rank = 0;
    for (int i = 0; i < 6; ++i) {                            // y = -sum_kept V_i (V_i . S b) / lambda_i
      const double lam = s_A[i * 7];
      if (!(lam > ICP_TAU * lmax)) continue;
      double g = 0.0;
      for (int j = 0; j < 6; ++j) g += s_V[j * 6 + i] * (s_s[j] * s_t[21 + j]);
      const double f = -g / lam;
      for (int j = 0; j < 6; ++j) s_y[j] += f * s_V[j * 6 + i];
      ++rank;
    }
    bool nonzero = false, finite = true;
    for (int j = 0; j < 6; ++j) {
      s_x[j] = s_s[j] * s_y[j];
      nonzero = nonzero || s_x[j] != 0.0;
      finite = finite && fabs(s_x[j]) < __builtin_inf();
    }
    ok = rank > 0 && nonzero && finite;
  }
  if (ok) {
    const double w0 = s_x[0], w1 = s_x[1], w2 = s_x[2];
    const double th2 = (w0 * w0 + w1 * w1) + w2 * w2;
    double a, c;
    if (th2 < 1e-8) {
      a = 1.0 - th2 / 6.0;
      c = 0.5 - th2 / 24.0;
    } else {
      const double th = sqrt(th2);
      a = sin(th) / th;
      c = (1.0 - cos(th)) / th2;
    }
    s_K[0] = 0.0; s_K[1] = -w2; s_K[2] = w1;
    s_K[3] = w2; s_K[4] = 0.0; s_K[5] = -w0;
    s_K[6] = -w1; s_K[7] = w0; s_K[8] = 0.0;
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) s_dR[r * 3 + q] = ((r == q ? 1.0 - c * th2 : 0.0) + a * s_K[r * 3 + q]) + (c * s_x[r]) * s_x[q];
    for (int j = 0; j < 9; ++j) s_R[j] = rec.R[j];
    for (int r = 0; r < 3; ++r)                      // R dR^T
      for (int q = 0; q < 3; ++q)
        s_Rn[r * 3 + q] = (s_R[r * 3] * s_dR[q * 3] + s_R[r * 3 + 1] * s_dR[q * 3 + 1]) + s_R[r * 3 + 2] * s_dR[q * 3 + 2];
    for (int r = 0; r < 3; ++r) {
      rec.t[r] = rec.t[r] - ((s_Rn[r * 3] * s_x[3] + s_Rn[r * 3 + 1] * s_x[4]) + s_Rn[r * 3 + 2] * s_x[5]);
      for (int q = 0; q < 3; ++q) rec.R[r * 3 + q] = s_Rn[r * 3 + q];
    }
  }
  st[0] = (float)cnt;
  st[1] = cnt > 0.0 ? (float)sqrt(sse / cnt) : 0.0f;
  st[2] = n > 0 ? (float)(cnt / (double)n) : 0.0f;
  st[3] = (k == 0 ? 0.0f : st[3]) + (ok ? 1.0f : 0.0f);
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
    hipLaunchKernelGGL(icp_solve_kernel, dim3(B), dim3(CPPF_WAVE), 0, st, pt_off, max_n, (int)nblk, part, k, iters, results, stats);
    CPPF_LAUNCH_CHECK();
  }
  return CPPF_OK;
}
