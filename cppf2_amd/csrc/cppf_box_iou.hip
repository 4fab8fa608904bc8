// IoU of oriented boxes from their clipped faces, batched: the overlap the NOCS scorer's 3-D IoU AP is built on (cppf2_amd/box_iou.py,
// metrics.degree_cm_mAP(iou="device")).  The reference computes it on the host (utils/iou.py, utils/box.py).
// gfx950 only.  All float64.
//
// cppf_box_iou: one launch after a clear of the output, BOX_THREADS = 128 threads = 8 rows of 16 lanes, one row per (pair,
//   turn), row r = pair * max_turns + turn (rows with turn >= turns[pair] do nothing), twelve of a row's lanes one face each:
//   lanes 0..5 the faces of box 1 (turned), 6..11 those of box 2; face = 2 * axis + (1 if the +axis side).  A lane clips its
//   face's rectangle by the six half-spaces of the other box (Sutherland-Hodgman) in 2-D in-plane coordinates; the polygon lives
//   in LDS as two buffers [vertex][coordinate][thread] (320 bytes per lane, 40 KiB per block; consecutive lanes 8 bytes apart),
//   never in a runtime-indexed register array.  The volume of the intersection is a sum over its faces,
//   V = 1/3 sum_f d_f Area_f, the row's twelve terms added on the DPP path; lane 0 of the row raises iou[pair] with a 64-bit
//   integer atomic maximum on the bits of the non-negative double.  A maximum is exact: the result does not depend on the grid,
//   the batch or the order.
// Arithmetic (tests/box_iou_ref.py restates it in NumPy); dot(u, w) = (u.x*w.x + u.y*w.y) + u.z*w.z:
//   (c, s) = turn_cs[n (n - 1) / 2 + turn], n = turns[pair];  A = R1 . Ry: column 0 = c col0 - s col2, column 1 = col1,
//   column 2 = s col0 + c col2;  B = R2.  Origin midway between the centres: ca = 0.5 (t1 - t2), cb = -ca; halves h = 0.5 s;
//   size = (|s1| + |s2|) + |t1 - t2|.
//   A face (axis k, sign sg) of its own box (axes O, centre oc, halves oh): n = O[:, k], e1 = O[:, k+1], e2 = O[:, k+2] (mod 3),
//   centre fc = oc + (sg h_k) n, offset d_f = sg dot(n, oc) + h_k, rectangle (-h1,-h2), (h1,-h2), (h1,h2), (-h1,h2) in (e1, e2).
//   The other box (axes Y, centre yc, halves yh), for j = 0, 1, 2 and tau = -1, +1 in this order: v = Y[:, j],
//   a0 = dot(v, fc - yc), b = dot(v, e1), c = dot(v, e2); a point (p, q) of the face is at dist = ((tau a0 - yh_j) + (tau b) p) +
//   (tau c) q, inside when dist <= 0; no distance is snapped.  Walking the edges prev -> cur from the last vertex: a crossing
//   (dist strictly of opposite signs) emits prev + t (cur - prev), t = d_prev / (d_prev - d_cur); then cur is emitted when inside.
//   Area = 0.5 |sum_{i=1}^{m-2} (p_i - p_0)(q_{i+1} - q_0) - (p_{i+1} - p_0)(q_i - q_0)|.
//   Nearly coinciding planes.  A vertex within rounding of a plane has an arbitrary side; that is harmless unless a whole face
//   lies that close to a plane of the other box, where the two faces' lanes would each decide alone which parts of them bound the
//   intersection (identical boxes, shared faces, boxes that touch -- exactly or almost: the line in which two planes tilted by
//   theta meet is known to u / theta only, u the rounding).  So one lane decides for both: a lane of box 1 takes the first plane
//   (j, tau) of box 2 with |b| <= 1e-5, |c| <= 1e-5 and |tau a0 - yh_j| <= 1e-5 size as its face's partner.  It clips by the other
//   five planes only (the partner counts as inside everywhere): area C; then by the partner: area C_in; with the partner's offset
//   d_o = tau dot(v, yc) + yh_j its term is
//     same way (sg tau dot(n, v) > 0):  d_f C_in + d_o (C - C_in)      -- each plane where it is the inner one
//     facing each other:               (d_f + d_o) C_in               -- the slab between them where it has thickness
//   and the partner face's own lane contributes nothing (the row ORs the taken faces' bits over the DPP path).  What is neglected
//   is of second order, theta^2 + theta sep <= 2e-10 relative; pairs tilted by more are clipped face by face, u / theta <= 1e-10.
//   A partner that faces the lane's face with all four corners within 1e-12 size, (|tau a0 - yh_j| + |b| h1) + |c| h2, means the
//   boxes only touch: V = 0 exactly.
//   Otherwise the term is d_f C.  V = (sum of the terms) / 3, a negative V is 0; iou = V / (s1x s1y s1z + s2x s2y s2z - V).
//   A pair whose turns is outside 1 .. max_turns gets NaN.
#include "cppf_common.h"

#define BOX_THREADS 128
#define BOX_ROWS (BOX_THREADS / 16)
#define BOX_MAX_VERTS 10          // a rectangle clipped by six half-planes (the partner's clip replaces the one left out)
#define BOX_TILT 1e-5             // sine of the tilt up to which two planes count as nearly parallel
#define BOX_SEP 1e-5              // x size: how far from the face's centre such a plane may pass
#define BOX_TOUCH 1e-12           // x size: a facing partner this close in all four corners -> V = 0
#define BOX_MAX_TURNS 64
#define BOX_MAX_PAIRS (1 << 20)

__device__ __forceinline__ double box_dot(double ux, double uy, double uz, double wx, double wy, double wz) {
  return (ux * wx + uy * wy) + uz * wz;
}

__device__ __forceinline__ double box_sel(int k, double a0, double a1, double a2) { return k == 0 ? a0 : (k == 1 ? a1 : a2); }

// this lane's polygon: vertex v, coordinate c at [(2 v + c) * BOX_THREADS]
// (m < BOX_MAX_VERTS never fails for a convex polygon -- a half-plane adds at most one vertex, 4 + 6 = 10 -- it only keeps a
// polygon that rounding made non-convex inside its LDS column)
__device__ __forceinline__ int box_clip(const double* __restrict__ src, double* __restrict__ dst, int n, double a, double b,
                                        double c) {
  if (n == 0) return 0;
  int m = 0;
  double p0 = src[(2 * (n - 1)) * BOX_THREADS], q0 = src[(2 * (n - 1) + 1) * BOX_THREADS];
  double d0 = (a + b * p0) + c * q0;
  for (int i = 0; i < n; ++i) {
    const double p1 = src[(2 * i) * BOX_THREADS], q1 = src[(2 * i + 1) * BOX_THREADS];
    const double d1 = (a + b * p1) + c * q1;
    if (((d0 < 0.0 && d1 > 0.0) || (d0 > 0.0 && d1 < 0.0)) && m < BOX_MAX_VERTS) {
      const double t = d0 / (d0 - d1);
      dst[(2 * m) * BOX_THREADS] = p0 + t * (p1 - p0);
      dst[(2 * m + 1) * BOX_THREADS] = q0 + t * (q1 - q0);
      ++m;
    }
    if (d1 <= 0.0 && m < BOX_MAX_VERTS) {
      dst[(2 * m) * BOX_THREADS] = p1;
      dst[(2 * m + 1) * BOX_THREADS] = q1;
      ++m;
    }
    p0 = p1; q0 = q1; d0 = d1;
  }
  return m;
}

__device__ __forceinline__ double box_area(const double* __restrict__ buf, int n) {
  double fan = 0.0;
  if (n >= 3) {
    const double p0 = buf[0], q0 = buf[BOX_THREADS];
    double pa = buf[2 * BOX_THREADS] - p0, qa = buf[3 * BOX_THREADS] - q0;
    for (int i = 2; i < n; ++i) {
      const double pb = buf[(2 * i) * BOX_THREADS] - p0, qb = buf[(2 * i + 1) * BOX_THREADS] - q0;
      fan = fan + (pa * qb - pb * qa);
      pa = pb; qa = qb;
    }
  }
  return 0.5 * fabs(fan);
}

// the sum over a row of 16 lanes, in every lane of the row (the first four exchanges of wave_sum)
__device__ __forceinline__ double box_row_sum(double v) {
  v += dpp_f64<0xB1>(v);                 // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);                 // quad_perm [2,3,0,1]
  v += dpp_f64<0x141>(v);                // row_half_mirror
  v += dpp_f64<0x140>(v);                // row_mirror
  return v;
}
__device__ __forceinline__ unsigned int box_row_or(unsigned int v) {
  v |= (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);
  v |= (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);
  v |= (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true);
  v |= (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, true);
  return v;
}

__global__ __launch_bounds__(BOX_THREADS) void box_iou_kernel(const double* __restrict__ R1, const double* __restrict__ t1,
                                                              const double* __restrict__ s1, const double* __restrict__ R2,
                                                              const double* __restrict__ t2, const double* __restrict__ s2,
                                                              const int32_t* __restrict__ turns,
                                                              const double* __restrict__ turn_cs, int max_turns, int P,
                                                              unsigned long long* __restrict__ iou) {
  __shared__ double s_poly[2][2 * BOX_MAX_VERTS][BOX_THREADS];
  const int64_t row = (int64_t)blockIdx.x * BOX_ROWS + (threadIdx.x >> 4);
  const int face = threadIdx.x & 15;
  const int64_t pair = row / max_turns;
  const int turn = (int)(row - pair * max_turns);
  int n_turns = 0;
  if (pair < P) n_turns = turns[pair];
  const bool bad = pair < P && (n_turns < 1 || n_turns > max_turns);
  const bool row_live = pair < P && !bad && turn < n_turns;
  double term = 0.0, vol12 = 1.0;
  bool flat = false;
  unsigned int taken = 0u;              // bit f: face 6 + f of box 2 is scored by a lane of box 1
  if (row_live && face < 12) {
    const double* cs = turn_cs + 2 * ((int64_t)n_turns * (n_turns - 1) / 2 + turn);
    const double co = cs[0], si = cs[1];
    const double *r1 = R1 + 9 * pair, *r2 = R2 + 9 * pair;
    const double s1x = s1[3 * pair], s1y = s1[3 * pair + 1], s1z = s1[3 * pair + 2];
    const double s2x = s2[3 * pair], s2y = s2[3 * pair + 1], s2z = s2[3 * pair + 2];
    const double dx = t1[3 * pair] - t2[3 * pair], dy = t1[3 * pair + 1] - t2[3 * pair + 1],
                 dz = t1[3 * pair + 2] - t2[3 * pair + 2];
    const double size = (sqrt((s1x * s1x + s1y * s1y) + s1z * s1z) + sqrt((s2x * s2x + s2y * s2y) + s2z * s2z)) +
                        sqrt((dx * dx + dy * dy) + dz * dz);
    const double eps = BOX_TOUCH * size, sep = BOX_SEP * size;
    vol12 = (s1x * s1y) * s1z + (s2x * s2y) * s2z;
    const bool second = face >= 6;
    const int f6 = second ? face - 6 : face;
    const int k = f6 >> 1, k1 = k == 2 ? 0 : k + 1, k2 = k == 0 ? 2 : k - 1;
    const double sg = (f6 & 1) ? 1.0 : -1.0;
    // own box O (the face's), other box Y (the clipper); entry [i][j] = component i of axis j
    double O[9], Y[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double a0 = r1[3 * i], a1 = r1[3 * i + 1], a2 = r1[3 * i + 2];
      const double A0 = co * a0 - si * a2, A1 = a1, A2 = si * a0 + co * a2;
      const double B0 = r2[3 * i], B1 = r2[3 * i + 1], B2 = r2[3 * i + 2];
      O[3 * i] = second ? B0 : A0; O[3 * i + 1] = second ? B1 : A1; O[3 * i + 2] = second ? B2 : A2;
      Y[3 * i] = second ? A0 : B0; Y[3 * i + 1] = second ? A1 : B1; Y[3 * i + 2] = second ? A2 : B2;
    }
    const double cax = 0.5 * dx, cay = 0.5 * dy, caz = 0.5 * dz;
    const double ocx = second ? -cax : cax, ocy = second ? -cay : cay, ocz = second ? -caz : caz;      // yc = -oc
    const double ohx = 0.5 * (second ? s2x : s1x), ohy = 0.5 * (second ? s2y : s1y), ohz = 0.5 * (second ? s2z : s1z);
    const double yh[3] = {0.5 * (second ? s1x : s2x), 0.5 * (second ? s1y : s2y), 0.5 * (second ? s1z : s2z)};
    const double nx = box_sel(k, O[0], O[1], O[2]), ny = box_sel(k, O[3], O[4], O[5]), nz = box_sel(k, O[6], O[7], O[8]);
    const double e1x = box_sel(k1, O[0], O[1], O[2]), e1y = box_sel(k1, O[3], O[4], O[5]), e1z = box_sel(k1, O[6], O[7], O[8]);
    const double e2x = box_sel(k2, O[0], O[1], O[2]), e2y = box_sel(k2, O[3], O[4], O[5]), e2z = box_sel(k2, O[6], O[7], O[8]);
    const double hk = box_sel(k, ohx, ohy, ohz), h1 = box_sel(k1, ohx, ohy, ohz), h2 = box_sel(k2, ohx, ohy, ohz);
    const double sh = sg * hk;
    const double fcx = ocx + sh * nx, fcy = ocy + sh * ny, fcz = ocz + sh * nz;
    const double d_f = sg * box_dot(nx, ny, nz, ocx, ocy, ocz) + hk;
    const double relx = fcx - (-ocx), rely = fcy - (-ocy), relz = fcz - (-ocz);
    double* buf0 = &s_poly[0][0][threadIdx.x];
    double* buf1 = &s_poly[1][0][threadIdx.x];
    buf0[0 * BOX_THREADS] = -h1; buf0[1 * BOX_THREADS] = -h2;
    buf0[2 * BOX_THREADS] = h1;  buf0[3 * BOX_THREADS] = -h2;
    buf0[4 * BOX_THREADS] = h1;  buf0[5 * BOX_THREADS] = h2;
    buf0[6 * BOX_THREADS] = -h1; buf0[7 * BOX_THREADS] = h2;
    int n = 4;
    bool paired = false, opposite = false;
    double pa = -1.0, pb = 0.0, pc = 0.0, d_o = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double vx = Y[j], vy = Y[3 + j], vz = Y[6 + j];
      const double a0 = box_dot(vx, vy, vz, relx, rely, relz);
      const double b = box_dot(vx, vy, vz, e1x, e1y, e1z), c = box_dot(vx, vy, vz, e2x, e2y, e2z);
      const double nv = sg * box_dot(nx, ny, nz, vx, vy, vz);
      const double vyc = box_dot(vx, vy, vz, -ocx, -ocy, -ocz);
      const bool parallel = !second && fabs(b) <= BOX_TILT && fabs(c) <= BOX_TILT;
      const double bh = fabs(b) * h1, ch = fabs(c) * h2;
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) {                       // tau = -1: buf0 -> buf1, tau = +1: buf1 -> buf0
        const double tau = ti ? 1.0 : -1.0;
        const double a = tau * a0 - yh[j];
        const bool near = parallel && !paired && fabs(a) <= sep;
        if (near) {
          paired = true;
          opposite = tau * nv < 0.0;
          flat = opposite && (fabs(a) + bh) + ch <= eps;
          pa = a; pb = tau * b; pc = tau * c;
          d_o = tau * vyc + yh[j];
          taken = 1u << (2 * j + ti);
        }
        // (the partner is left for last: everything counts as inside it here)
        n = box_clip(ti ? buf1 : buf0, ti ? buf0 : buf1, n, near ? -1.0 : a, near ? 0.0 : tau * b, near ? 0.0 : tau * c);
      }
    }
    const double area = box_area(buf0, n);
    term = d_f * area;
    if (paired) {
      const double area_in = box_area(buf1, box_clip(buf0, buf1, n, pa, pb, pc));
      term = opposite ? (d_f + d_o) * area_in : d_f * area_in + d_o * (area - area_in);
    }
  }
  // every lane of the wavefront takes part in the exchanges; lanes without a face carry 0
  taken = box_row_or(taken);
  if (face >= 6 && face < 12 && ((taken >> (face - 6)) & 1u)) term = 0.0;
  const double sum = box_row_sum(term);
  const unsigned int flat_row = (unsigned int)(wave_ballot(flat) >> (wave_lane() & 48)) & 0xffffu;
  if (face == 0 && (row_live || (bad && turn == 0))) {
    double V = sum / 3.0;
    V = flat_row ? 0.0 : V;
    V = V < 0.0 ? 0.0 : V;
    const double r = bad ? __builtin_nan("") : V / (vol12 - V);
    atomicMax(&iou[pair], (unsigned long long)__double_as_longlong(r));
  }
}

extern "C" int cppf_box_iou(const double* R1, const double* t1, const double* s1, const double* R2, const double* t2,
                            const double* s2, const int32_t* turns, const double* turn_cs, int max_turns, int P, double* iou,
                            void* stream) {
  CPPF_CHECK_ARG(P >= 0 && P <= BOX_MAX_PAIRS);
  CPPF_CHECK_ARG(max_turns >= 1 && max_turns <= BOX_MAX_TURNS);
  if (P == 0) return CPPF_OK;
  CPPF_CHECK_ARG(R1 && t1 && s1 && R2 && t2 && s2 && turns && turn_cs && iou);
  hipStream_t st = (hipStream_t)stream;
  CPPF_HIP(hipMemsetAsync(iou, 0, (size_t)P * sizeof(double), st));
  const int64_t rows = (int64_t)P * max_turns;
  const unsigned int blocks = (unsigned int)((rows + BOX_ROWS - 1) / BOX_ROWS);
  hipLaunchKernelGGL(box_iou_kernel, dim3(blocks), dim3(BOX_THREADS), 0, st, R1, t1, s1, R2, t2, s2, turns, turn_cs,
                     max_turns, P, (unsigned long long*)iou);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
