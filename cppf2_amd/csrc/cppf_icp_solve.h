// The 6x6 solve and pose update that cppf_icp.hip's icp_solve_kernel and cppf_track.hip's track_solve_kernel share: one lane, the
// matrices in LDS (no register array with a loop-varying index, so nothing goes to scratch memory).  The arithmetic is stated in
// cppf_icp.hip's header under "solve" and "Rodrigues" and restated in tests/icp_ref.py (_min_norm_solve, rodrigues).
#pragma once
#include "cppf_common.h"

#define ICP_TERMS 30           // 21 (J^T J upper) + 6 (J^T e) + count + sum e^2 + sum |q|^2
#define ICP_TAU 1e-9           // eigenvalues of S A S at or below ICP_TAU * lambda_max are dropped (unobservable directions)
#define ICP_JEPS 1e-17         // Jacobi: an off-diagonal entry this small next to its two diagonal entries counts as 0
#define ICP_SWEEPS 16          // Jacobi sweeps at most (measured: 3-8, the last of them rotating nothing)

struct IcpSolveLds {
  double A[36], V[36], s[6], y[6], x[6], K[9], R[9], dR[9], Rn[9];
};

// The minimum-norm Gauss-Newton step of A x = -b from the ICP_TERMS sums s_t (cnt = s_t[27] >= 6 is the caller's test): L.x.
// Returns whether the step moves the pose: rank > 0 and a non-zero, finite x.
__device__ __forceinline__ bool icp_min_norm_step(const double* s_t, double cnt, IcpSolveLds& L) {
  const double L2 = s_t[29] / cnt;
  const double r = L2 > 0.0 ? 1.0 / sqrt(L2) : 0.0;
  for (int j = 0; j < 6; ++j) L.s[j] = j < 3 ? r : 1.0;
  int o = 0;
  for (int a = 0; a < 6; ++a)
    for (int c = a; c < 6; ++c) {
      const double v = (L.s[a] * s_t[o]) * L.s[c];
      L.A[a * 6 + c] = v;
      L.A[c * 6 + a] = v;
      L.V[a * 6 + c] = a == c ? 1.0 : 0.0;
      L.V[c * 6 + a] = a == c ? 1.0 : 0.0;
      ++o;
    }
  for (int sweep = 0; sweep < ICP_SWEEPS; ++sweep) {       // cyclic Jacobi: S A S = V diag(a_ii) V^T
    bool rotated = false;
    for (int p = 0; p < 5; ++p)
      for (int q = p + 1; q < 6; ++q) {
        const double apq = L.A[p * 6 + q], app = L.A[p * 7], aqq = L.A[q * 7];
        if (apq == 0.0) continue;
        if (fabs(apq) <= ICP_JEPS * (fabs(app) + fabs(aqq))) {
          L.A[p * 6 + q] = 0.0;
          L.A[q * 6 + p] = 0.0;
          continue;
        }
        const double th = (aqq - app) / (2.0 * apq);
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        L.A[p * 7] = app - t * apq;
        L.A[q * 7] = aqq + t * apq;
        L.A[p * 6 + q] = 0.0;
        L.A[q * 6 + p] = 0.0;
        for (int k = 0; k < 6; ++k) {
          if (k != p && k != q) {
            const double akp = L.A[k * 6 + p], akq = L.A[k * 6 + q];
            const double np_ = c * akp - sn * akq, nq = sn * akp + c * akq;
            L.A[k * 6 + p] = np_;
            L.A[p * 6 + k] = np_;
            L.A[k * 6 + q] = nq;
            L.A[q * 6 + k] = nq;
          }
          const double vkp = L.V[k * 6 + p], vkq = L.V[k * 6 + q];
          L.V[k * 6 + p] = c * vkp - sn * vkq;
          L.V[k * 6 + q] = sn * vkp + c * vkq;
        }
        rotated = true;
      }
    if (!rotated) break;
  }
  double lmax = 0.0;
  for (int i = 0; i < 6; ++i)
    if (L.A[i * 7] > lmax) lmax = L.A[i * 7];
  for (int j = 0; j < 6; ++j) L.y[j] = 0.0;
  int rank = 0;
  for (int i = 0; i < 6; ++i) {                            // y = -sum_kept V_i (V_i . S b) / lambda_i
    const double lam = L.A[i * 7];
    if (!(lam > ICP_TAU * lmax)) continue;
    double g = 0.0;
    for (int j = 0; j < 6; ++j) g += L.V[j * 6 + i] * (L.s[j] * s_t[21 + j]);
    const double f = -g / lam;
    for (int j = 0; j < 6; ++j) L.y[j] += f * L.V[j * 6 + i];
    ++rank;
  }
  bool nonzero = false, finite = true;
  for (int j = 0; j < 6; ++j) {
    L.x[j] = L.s[j] * L.y[j];
    nonzero = nonzero || L.x[j] != 0.0;
    finite = finite && fabs(L.x[j]) < __builtin_inf();
  }
  return rank > 0 && nonzero && finite;
}

// dR = Rodrigues(L.x[0..3)) and L.Rn = L.R dR^T (the caller fills L.R with the pose's rotation first and then writes
// R <- L.Rn, t <- t - L.Rn v, v = L.x[3..6)).
__device__ __forceinline__ void icp_rotation_update(IcpSolveLds& L) {
  const double w0 = L.x[0], w1 = L.x[1], w2 = L.x[2];
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
  L.K[0] = 0.0; L.K[1] = -w2; L.K[2] = w1;
  L.K[3] = w2; L.K[4] = 0.0; L.K[5] = -w0;
  L.K[6] = -w1; L.K[7] = w0; L.K[8] = 0.0;
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) L.dR[r * 3 + q] = ((r == q ? 1.0 - c * th2 : 0.0) + a * L.K[r * 3 + q]) + (c * L.x[r]) * L.x[q];
  for (int r = 0; r < 3; ++r)                      // R dR^T
    for (int q = 0; q < 3; ++q)
      L.Rn[r * 3 + q] = (L.R[r * 3] * L.dR[q * 3] + L.R[r * 3 + 1] * L.dR[q * 3 + 1]) + L.R[r * 3 + 2] * L.dR[q * 3 + 2];
}
