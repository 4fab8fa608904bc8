// A triangle mesh reduced by vertex clustering with one quadric-optimal representative per cell (Lindstrom, Out-of-core
// simplification of large polygonal models, SIGGRAPH 2000): the stage between a mesh with more triangles than pixels (a fused
// volume's surface, a BOP `models` file) and the consumers that pay per triangle (cppf2_amd/simplify.py).
// The reference has no such step.  gfx950 only.  tests/simplify_ref.py restates every definition below in NumPy; the build's
// -ffp-contract=off keeps every operation where it is written (no fused multiply-add), and the float32 divide is correctly
// rounded.
//
// The lattice: cell (i,j,k), 0 <= i,j,k < 2^21, is [o + i cell, o + (i+1) cell) per axis; o = h_origin rounded to float32.
//
// cppf_cluster_keys: 256 threads, one lane per vertex, float32.  Per axis t = (x - o) / cell (one subtraction, one division).
//   The vertex is inside iff 0 <= t < 2097152.0f on all three axes, compared in float32 before any cast (a NaN, an infinity or
//   a huge value never reaches the cast; -0.0f is inside, cell 0).  Inside: i = (int64)floorf(t) per axis,
//   key = i << 42 | j << 21 | k.  Outside: key = -1.  A coordinate exactly on a cell boundary belongs to the upper cell.
//
// cppf_cluster_quadrics: 256 threads, one lane per cluster, float64, no atomics.  Cluster c owns the corners
//   corners[seg_off[c] .. seg_off[c+1]) (entry 3 f + j = corner j of face f), visited sequentially in list order: the order of
//   the sums is part of the definition.  (i,j,k) are the three 21-bit fields of keys[c]; a negative key gives NaN.
//     ctr = (double)o + ((double)i + 0.5) * (double)cell                      per axis
//   per corner j of face (v0, v1, v2), with p_k = (double)verts[v_k] - ctr:
//     count += 1;  vsum += p_j
//     e1 = p1 - p0, e2 = p2 - p0;  n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x);  l2 = (nx nx + ny ny) + nz nz
//     the rest of the corner is skipped unless l2 > 0 and l2 < +inf
//     l = sqrt(l2);  area = l / 2;  u = n / l (three divisions);  d = (ux p0x + uy p0y) + uz p0z
//     au = area * u (three products);  A00 += aux ux, A01 += aux uy, A02 += aux uz, A11 += auy uy, A12 += auy uz, A22 += auz uz
//     ad = area * d;  b += ad * u;  w += area;  m += area * (((p0 + p1) + p2) / 3)
//   after the last corner, if w > 0:  (A + lam w I) x = b + lam m  by an LDL^T factorisation without pivoting:
//     kk = lam * w;  a00 = A00 + kk, a11 = A11 + kk, a22 = A22 + kk;  r = b + lam * m
//     l10 = A01 / a00, l20 = A02 / a00;  d1 = a11 - l10 * A01;  t21 = A12 - l20 * A01;  l21 = t21 / d1
//     d2 = (a22 - l20 * A02) - l21 * t21
//     y0 = r0, y1 = r1 - l10 * y0, y2 = (r2 - l20 * y0) - l21 * y1
//     x2 = y2 / d2;  x1 = y1 / d1 - l21 * x2;  x0 = (y0 / a00 - l10 * x1) - l20 * x2
//   (trace A = w, so the matrix is symmetric positive definite with condition number at most (1 + lam) / lam: no rank
//   decision, and the regulariser pulls towards the area-weighted mean m / w exactly where the quadric is flat);
//   else (only triangles without area) x = vsum / (double)count, and 0 for a cluster without corners.
//     x = x < -h ? -h : (x > h ? h : x),  h = (double)cell / 2               per axis: the representative stays in its cell
//     pos = (float)(ctr + x)
//   A corner index outside [0, 3 nf) or a vertex index outside [0, n) skips the corner entirely (the wrapper refuses such a
//   mesh before the call); segment bounds are clipped to [0, m].  The gathers are uncoalesced and the loop is serial per lane:
//   clusters hold tens of corners, and a wave-wide reduction would change the order of the sums, which is the definition.
#include "cppf_common.h"

#include <math.h>

#define SIMPLIFY_THREADS 256
#define SIMPLIFY_KEY_RANGE 2097152.0f      // 2^21 cells per axis
#define SIMPLIFY_MAX_FACES 715827882       // 3 nf fits int32

__global__ __launch_bounds__(SIMPLIFY_THREADS) void cluster_keys_kernel(const float* __restrict__ verts, int n, float ox, float oy,
                                                                        float oz, float cell, int64_t* __restrict__ keys) {
  const int64_t v = (int64_t)blockIdx.x * SIMPLIFY_THREADS + threadIdx.x;
  if (v >= n) return;
  const float tx = (verts[3 * v] - ox) / cell, ty = (verts[3 * v + 1] - oy) / cell, tz = (verts[3 * v + 2] - oz) / cell;
  const bool inside = tx >= 0.0f && tx < SIMPLIFY_KEY_RANGE && ty >= 0.0f && ty < SIMPLIFY_KEY_RANGE && tz >= 0.0f &&
                      tz < SIMPLIFY_KEY_RANGE;
  int64_t key = -1;
  if (inside) key = (int64_t)floorf(tx) << 42 | (int64_t)floorf(ty) << 21 | (int64_t)floorf(tz);
  keys[v] = key;
}

__global__ __launch_bounds__(SIMPLIFY_THREADS) void cluster_quadrics_kernel(
    const float* __restrict__ verts, int n, const int32_t* __restrict__ faces, int nf, const int32_t* __restrict__ corners, int64_t m,
    const int64_t* __restrict__ seg_off, const int64_t* __restrict__ keys, int nc, float ox, float oy, float oz, float cell, double lam,
    float* __restrict__ pos) {
  const int64_t c = (int64_t)blockIdx.x * SIMPLIFY_THREADS + threadIdx.x;
  if (c >= nc) return;
  const int64_t key = keys[c];
  if (key < 0) {
    const float q = __builtin_nanf("");
    pos[3 * c] = q; pos[3 * c + 1] = q; pos[3 * c + 2] = q;
    return;
  }
  const double dcell = (double)cell;
  const double cx = (double)ox + ((double)((key >> 42) & 0x1fffff) + 0.5) * dcell;
  const double cy = (double)oy + ((double)((key >> 21) & 0x1fffff) + 0.5) * dcell;
  const double cz = (double)oz + ((double)(key & 0x1fffff) + 0.5) * dcell;
  int64_t s0 = seg_off[c], s1 = seg_off[c + 1];
  s0 = s0 < 0 ? 0 : s0;
  s1 = s1 > m ? m : s1;
  double count = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
  double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0;
  double bx = 0.0, by = 0.0, bz = 0.0, w = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
  const int64_t m3 = 3 * (int64_t)nf;
  for (int64_t s = s0; s < s1; ++s) {
    const int32_t corner = corners[s];
    if (corner < 0 || corner >= m3) continue;
    const int32_t f = corner / 3, j = corner - 3 * f;
    const int32_t v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
    if (v0 < 0 || v0 >= n || v1 < 0 || v1 >= n || v2 < 0 || v2 >= n) continue;
    const double p0x = (double)verts[3 * (int64_t)v0] - cx, p0y = (double)verts[3 * (int64_t)v0 + 1] - cy,
                 p0z = (double)verts[3 * (int64_t)v0 + 2] - cz;
    const double p1x = (double)verts[3 * (int64_t)v1] - cx, p1y = (double)verts[3 * (int64_t)v1 + 1] - cy,
                 p1z = (double)verts[3 * (int64_t)v1 + 2] - cz;
    const double p2x = (double)verts[3 * (int64_t)v2] - cx, p2y = (double)verts[3 * (int64_t)v2 + 1] - cy,
                 p2z = (double)verts[3 * (int64_t)v2 + 2] - cz;
    count += 1.0;
    sx += j == 0 ? p0x : (j == 1 ? p1x : p2x);
    sy += j == 0 ? p0y : (j == 1 ? p1y : p2y);
    sz += j == 0 ? p0z : (j == 1 ? p1z : p2z);
    const double e1x = p1x - p0x, e1y = p1y - p0y, e1z = p1z - p0z;
    const double e2x = p2x - p0x, e2y = p2y - p0y, e2z = p2z - p0z;
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double l2 = (nx * nx + ny * ny) + nz * nz;
    if (!(l2 > 0.0 && l2 < (double)__builtin_inff())) continue;
    const double l = sqrt(l2);
    const double area = l / 2.0;
    const double ux = nx / l, uy = ny / l, uz = nz / l;
    const double d = (ux * p0x + uy * p0y) + uz * p0z;
    const double aux = area * ux, auy = area * uy, auz = area * uz;
    A00 += aux * ux; A01 += aux * uy; A02 += aux * uz;
    A11 += auy * uy; A12 += auy * uz; A22 += auz * uz;
    const double ad = area * d;
    bx += ad * ux; by += ad * uy; bz += ad * uz;
    w += area;
    mx += area * (((p0x + p1x) + p2x) / 3.0);
    my += area * (((p0y + p1y) + p2y) / 3.0);
    mz += area * (((p0z + p1z) + p2z) / 3.0);
  }
  double x0, x1, x2;
  if (w > 0.0) {
    const double kk = lam * w;
    const double a00 = A00 + kk, a11 = A11 + kk, a22 = A22 + kk;
    const double r0 = bx + lam * mx, r1 = by + lam * my, r2 = bz + lam * mz;
    const double l10 = A01 / a00, l20 = A02 / a00;
    const double d1 = a11 - l10 * A01;
    const double t21 = A12 - l20 * A01;
    const double l21 = t21 / d1;
    const double d2 = (a22 - l20 * A02) - l21 * t21;
    const double y1 = r1 - l10 * r0;
    const double y2 = (r2 - l20 * r0) - l21 * y1;
    x2 = y2 / d2;
    x1 = y1 / d1 - l21 * x2;
    x0 = (r0 / a00 - l10 * x1) - l20 * x2;
  } else if (count > 0.0) {
    x0 = sx / count; x1 = sy / count; x2 = sz / count;
  } else {
    x0 = 0.0; x1 = 0.0; x2 = 0.0;
  }
  const double h = dcell / 2.0;
  x0 = x0 < -h ? -h : (x0 > h ? h : x0);
  x1 = x1 < -h ? -h : (x1 > h ? h : x1);
  x2 = x2 < -h ? -h : (x2 > h ? h : x2);
  pos[3 * c] = (float)(cx + x0);
  pos[3 * c + 1] = (float)(cy + x1);
  pos[3 * c + 2] = (float)(cz + x2);
}

static bool simplify_positive(double x) { return x > 0.0 && x < (double)INFINITY; }

static bool simplify_origin(const double* h_origin, float* o) {
  if (!h_origin) return false;
  o[0] = (float)h_origin[0]; o[1] = (float)h_origin[1]; o[2] = (float)h_origin[2];
  return __builtin_isfinite(o[0]) && __builtin_isfinite(o[1]) && __builtin_isfinite(o[2]);
}

extern "C" int cppf_cluster_keys(const float* verts, int n, const double* h_origin, float cell, int64_t* keys, void* stream) {
  float o[3];
  CPPF_CHECK_ARG(simplify_origin(h_origin, o));
  CPPF_CHECK_ARG(n >= 0);
  CPPF_CHECK_ARG(simplify_positive((double)cell));
  if (n == 0) return CPPF_OK;
  CPPF_CHECK_ARG(verts && keys);
  const unsigned int nb = (unsigned int)(((int64_t)n + SIMPLIFY_THREADS - 1) / SIMPLIFY_THREADS);
  hipLaunchKernelGGL(cluster_keys_kernel, dim3(nb), dim3(SIMPLIFY_THREADS), 0, (hipStream_t)stream, verts, n, o[0], o[1], o[2], cell,
                     keys);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}

extern "C" int cppf_cluster_quadrics(const float* verts, int n, const int32_t* faces, int nf, const int32_t* corners, int64_t m,
                                     const int64_t* seg_off, const int64_t* keys, int nc, const double* h_origin, float cell,
                                     double lam, float* pos, void* stream) {
  float o[3];
  CPPF_CHECK_ARG(simplify_origin(h_origin, o));
  CPPF_CHECK_ARG(n >= 0 && nf >= 0 && nf <= SIMPLIFY_MAX_FACES && nc >= 0);
  CPPF_CHECK_ARG(m >= 0 && m <= 3 * (int64_t)nf);
  CPPF_CHECK_ARG(simplify_positive((double)cell) && simplify_positive(lam));
  if (nc == 0) return CPPF_OK;
  CPPF_CHECK_ARG(seg_off && keys && pos);
  CPPF_CHECK_ARG(m == 0 || (verts && faces && corners));
  const unsigned int nb = (unsigned int)(((int64_t)nc + SIMPLIFY_THREADS - 1) / SIMPLIFY_THREADS);
  hipLaunchKernelGGL(cluster_quadrics_kernel, dim3(nb), dim3(SIMPLIFY_THREADS), 0, (hipStream_t)stream, verts, n, faces, nf, corners,
                     m, seg_off, keys, nc, o[0], o[1], o[2], cell, lam, pos);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
