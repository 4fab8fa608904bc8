// Posed depth views fused into a truncated signed distance volume, and the volume's zero surface as triangles: how an object
// without a CAD model gets the mesh every mesh consumer of the library takes (cppf2_amd/fuse.py).  The
// reference has no such step.  gfx950 only.  tests/fuse_ref.py restates every definition below in NumPy; the build's
// -ffp-contract=off keeps every float32 operation where it is written and the divide is correctly rounded.
//
// The volume: acc float32 [nx,ny,nz] (sum of the observations) and wsum int32 [nx,ny,nz] (their number), z fastest; node
// (i,j,k) sits at (ox + (float)i * voxel, oy + (float)j * voxel, oz + (float)k * voxel) in the object's frame, metres.  The
// linear node index is lin = (i * ny + j) * nz + k.
//
// cppf_tsdf_integrate: ONE launch for all V views, 256 threads, one lane per node in linear order (lanes run along z: acc and
//   wsum are read once and written once per call as coalesced rows), the views looped inside in order -- that order is the
//   summation order, so views 0..V-1 in one call are byte-identical to any split into consecutive calls.  A view's 12 pose
//   entries are the same for every lane (scalar loads); the only scattered traffic is the depth gather, and neighbouring nodes
//   hit neighbouring pixels.  Per node (x, y, z) and view, float32, left to right:
//     xc = ((P0*x + P1*y) + P2*z) + P3,  yc with row 1, zc with row 2;            skip unless zc >= znear
//     uf = (((fx*xc) / zc + cx) - pixel_offset) + 0.5f,  vf with fy, yc, cy;      skip unless 0 <= uf < (float)W, 0 <= vf < (float)H
//     col = (int)floorf(uf), row = (int)floorf(vf)        (compared in float32 first: a huge or NaN uf never reaches the cast)
//     d = depth[v,row,col];                                                       skip unless d > 0 and d < +inf
//     sdf = d - zc
//     inside the mask (or no masks):  skip if sdf < -trunc;  obs = sdf / trunc, 1 if that is not < 1
//     outside the mask:               obs = 1 if sdf > 0 (free space in front of whatever the pixel shows), else skip
//     acc += obs;  wsum += 1
//
// cppf_tsdf_integrate_weighted: the same kernel template with WEIGHTED set; weights uint8 [V,H,W], one per
//   reading (cppf_depth_weights), and carve_weight in 0..255.  Everything up to obs is as above; then
//     inside the mask (or no masks) and sdf / trunc < 1:  w = weights[v,row,col]
//     obs is the constant 1 (inside the mask with sdf / trunc not < 1; free space outside the mask):  w = carve_weight
//     skip if w == 0;  acc = acc + (float)w * obs;  wsum += w
//   acc is then the weighted sum and wsum the sum of the weights: acc / (float)wsum, what every reader of the volume forms, is
//   the weighted mean, and their min_weight a threshold in units of weight.  (float)w * 1.0f and (float)1 * obs are exact, so
//   weights of 1 and carve_weight 1 give the unweighted bytes.  wsum is int32: one call adds at most 65 536 x 255 per node, the
//   caller owns the total.
//
// cppf_tsdf_extract: marching tetrahedra over the cells (i,j,k), i < nx-1, j < ny-1, k < nz-1, in the linear cell order
//   ((i * (ny-1) + j) * (nz-1) + k).  tsdf = acc / (float)wsum; a node is known iff wsum >= min_weight and inside iff tsdf < 0
//   (exactly 0, and -0, are outside); a cell is processed iff its 8 corners are known.  The six tetrahedra of a cell follow the
//   axis permutations (a,b,c) in lexicographic order, corners p0 = n, p1 = n + e_a, p2 = n + e_a + e_b, p3 = n + (1,1,1): all six
//   share the body diagonal, which makes the split consistent across cell faces (no cracks, no ambiguous cases).  A vertex
//   lies on a tetrahedron edge whose ends differ in side, always computed from the end with the smaller linear index lo (inside
//   a tetrahedron that is the corner with the smaller number) to the other, hi:
//     s = t_lo / (t_lo - t_hi);  per axis  pos = o + ((float)n_lo + (d ? s : 0.0f)) * voxel,  d = n_hi - n_lo in {0,1}
//     key = 8 * lin_lo + (dx | dy << 1 | dz << 2)
//   so every cell and tetrahedron sharing the edge produces the same key and the same bits.  TET_CASES below lists, per inside
//   mask, the edges of the polygon counter-clockwise as seen from the outside for a tetrahedron of positive orientation (an
//   even permutation); 3 vertices = triangle (q0,q1,q2), 4 = triangles (q0,q1,q2), (q0,q2,q3); an odd permutation swaps the
//   last two vertices of every triangle.  Output order: cell, tetrahedron, triangle.
//   Three launches, no host synchronisation: count (per cell, reduced per block), one workgroup that scans the block sums
//   (TSDF_SCAN_THREADS per pass, carried over as many passes as there are), emit (recomputes its cells; writes nothing when the
//   total exceeds the capacity: the caller reads status, grows its buffers and calls again).
#include "cppf_common.h"

#include <math.h>

#define TSDF_THREADS 256
#define TSDF_SCAN_THREADS 1024            // block sums per pass of the scan: one pass covers 1024 * 256 = 262 144 cells
#define TSDF_MAX_NODES (1LL << 27)        // 134 217 728 nodes (512^3): 1 GiB of volume; at most 12 triangles per cell fit int32
#define TSDF_MAX_IMAGE 16384              // H and W
#define TSDF_MAX_VIEWS 65536

struct TsdfGrid {
  float ox, oy, oz, voxel;
  int nx, ny, nz;
};

template <bool WEIGHTED>
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_integrate_kernel(int V, const float* __restrict__ depth,
                                                                      const uint8_t* __restrict__ masks,
                                                                      const float* __restrict__ poses,
                                                                      const uint8_t* __restrict__ weights, int carve_weight,
                                                                      int H, int W, float fx,
                                                                      float fy, float cx, float cy, float pixel_offset, TsdfGrid g,
                                                                      float trunc, float znear, int64_t nodes,
                                                                      float* __restrict__ acc, int32_t* __restrict__ wsum) {
  const int64_t lin = (int64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
  if (lin >= nodes) return;
  const int k = (int)(lin % g.nz);
  const int64_t ij = lin / g.nz;
  const int j = (int)(ij % g.ny), i = (int)(ij / g.ny);
  const float x = g.ox + (float)i * g.voxel, y = g.oy + (float)j * g.voxel, z = g.oz + (float)k * g.voxel;
  const float fW = (float)W, fH = (float)H;
  float a = acc[lin];
  int32_t w = wsum[lin];
  for (int v = 0; v < V; ++v) {
    const float* P = poses + 12 * (int64_t)v;
    const float zc = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
    if (!(zc >= znear)) continue;
    const float xc = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
    const float yc = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
    const float uf = (((fx * xc) / zc + cx) - pixel_offset) + 0.5f;
    const float vf = (((fy * yc) / zc + cy) - pixel_offset) + 0.5f;
    if (!(uf >= 0.0f && uf < fW && vf >= 0.0f && vf < fH)) continue;
    const int col = (int)floorf(uf), row = (int)floorf(vf);          // 0 .. W-1, 0 .. H-1 by the comparison above
    const int64_t px = ((int64_t)v * H + row) * W + col;
    const float d = depth[px];
    if (!(d > 0.0f && d < __builtin_inff())) continue;
    const float sdf = d - zc;
    const bool in_mask = masks == nullptr || masks[px] != 0;
    float obs;
    bool carves = true;                                              // obs is the constant 1
    if (in_mask) {
      if (sdf < -trunc) continue;
      const float q = sdf / trunc;
      carves = !(q < 1.0f);
      obs = carves ? 1.0f : q;
    } else {
      if (!(sdf > 0.0f)) continue;
      obs = 1.0f;
    }
    if constexpr (WEIGHTED) {
      const int wv = carves ? carve_weight : (int)weights[px];
      if (wv == 0) continue;
      a = a + (float)wv * obs;
      w += wv;
    } else {
      a = a + obs;
      w += 1;
    }
  }
  acc[lin] = a;
  wsum[lin] = w;
}

// Per inside mask (bit p = corner p of the tetrahedron is inside), four edges of 4 bits each (lo | hi << 2, lo < hi), the
// first edge in the low bits; entries of three edges repeat the first one, masks 0 and 15 are never read.
//   one corner q inside:   (q,a), (q,b), (q,c)   with (q,a,b,c) the even permutation of least a
//   one corner q outside:  (q,a), (q,c), (q,b)   the same triangle seen from the other side
//   A < B inside:          (A,C), (A,D), (B,D), (B,C)   with (A,B,C,D) even
__constant__ uint16_t TET_CASES[16] = {
    0x4444,
    0x4c84,      //  1: p0            01 02 03
    0x49d4,      //  2: p1            01 13 12
    0x9dc8,      //  3: p0 p1         02 03 13 12
    0x8e98,      //  4: p2            02 12 23
    0xe94c,      //  5: p0 p2         03 01 12 23
    0x8ed4,      //  6: p1 p2         01 13 23 02
    0xcedc,      //  7: p0 p1 p2      03 13 23
    0xcdec,      //  8: p3            03 23 13
    0xde84,      //  9: p0 p3         01 02 23 13
    0xec49,      // 10: p1 p3         12 01 03 23
    0x89e8,      // 11: p0 p1 p3      02 23 12
    0xcd98,      // 12: p2 p3         02 12 13 03
    0x4d94,      // 13: p0 p2 p3      01 12 13
    0x48c4,      // 14: p1 p2 p3      01 03 02
    0x4444};

__device__ __forceinline__ int tet_triangles(int m) {
  const int pc = __popc((unsigned)m);
  return pc == 2 ? 2 : ((pc == 1 || pc == 3) ? 1 : 0);
}

// The 8 corner values of cell (i,j,k) in t[dx | dy << 1 | dz << 2]; returns the inside mask, or -1 for a cell with an unknown
// corner.  t is indexed with compile-time constants only (the loops are unrolled), so it stays in registers.
__device__ __forceinline__ int cell_corners(const float* __restrict__ acc, const int32_t* __restrict__ wsum, int64_t lin, int ny,
                                            int nz, int min_weight, float* t) {
  bool known = true;
  int inside = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int64_t at = lin + (int64_t)(c & 1) * ny * nz + (int64_t)((c >> 1) & 1) * nz + ((c >> 2) & 1);
    const int32_t w = wsum[at];
    const float v = acc[at] / (float)w;
    t[c] = v;
    known = known && w >= min_weight;
    inside |= (v < 0.0f ? 1 : 0) << c;
  }
  return known ? inside : -1;
}

// The inside mask of the tetrahedron with corners 0, V1, V2, 7 of the cell.
template <int V1, int V2>
__device__ __forceinline__ int tet_mask(int inside) {
  return (inside & 1) | (((inside >> V1) & 1) << 1) | (((inside >> V2) & 1) << 2) | (((inside >> 7) & 1) << 3);
}

__device__ __forceinline__ int cell_triangles(int inside) {
  return tet_triangles(tet_mask<1, 3>(inside)) + tet_triangles(tet_mask<1, 5>(inside)) + tet_triangles(tet_mask<2, 3>(inside)) +
         tet_triangles(tet_mask<2, 6>(inside)) + tet_triangles(tet_mask<4, 5>(inside)) + tet_triangles(tet_mask<4, 6>(inside));
}

// Cell c of the linear cell order -> (i,j,k) and its first node's linear index.
__device__ __forceinline__ int64_t cell_node(int64_t c, const TsdfGrid& g, int* i, int* j, int* k) {
  const int cz = g.nz - 1, cy = g.ny - 1;
  *k = (int)(c % cz);
  const int64_t ij = c / cz;
  *j = (int)(ij % cy);
  *i = (int)(ij / cy);
  return ((int64_t)*i * g.ny + *j) * g.nz + *k;
}

// ws: uint32 [nb] block triangle counts (exclusive offsets after the scan), uint32 [nb] block cell counts, uint32 [2] totals.
__global__ __launch_bounds__(TSDF_THREADS) void tsdf_count_kernel(const float* __restrict__ acc, const int32_t* __restrict__ wsum,
                                                                  TsdfGrid g, int min_weight, int64_t cells, uint32_t nb,
                                                                  uint32_t* __restrict__ ws) {
  __shared__ uint32_t s_t[TSDF_THREADS / CPPF_WAVE], s_c[TSDF_THREADS / CPPF_WAVE];
  const int64_t c = (int64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
  uint32_t n = 0;
  if (c < cells) {
    int i, j, k;
    const int64_t lin = cell_node(c, g, &i, &j, &k);
    float t[8];
    const int inside = cell_corners(acc, wsum, lin, g.ny, g.nz, min_weight, t);
    n = inside > 0 && inside < 255 ? (uint32_t)cell_triangles(inside) : 0u;
  }
  const uint32_t any = (uint32_t)__popcll(wave_ballot(n != 0));
  const uint32_t sum = wave_inclusive_scan_u32(n);
  if (wave_lane() == CPPF_WAVE - 1) {
    s_t[threadIdx.x / CPPF_WAVE] = sum;
    s_c[threadIdx.x / CPPF_WAVE] = any;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t st = 0, sc = 0;
#pragma unroll
    for (int w = 0; w < TSDF_THREADS / CPPF_WAVE; ++w) { st += s_t[w]; sc += s_c[w]; }
    ws[blockIdx.x] = st;
    ws[nb + blockIdx.x] = sc;
  }
}

__global__ __launch_bounds__(TSDF_SCAN_THREADS) void tsdf_scan_kernel(uint32_t nb, uint32_t* __restrict__ ws,
                                                                      int64_t* __restrict__ status) {
  __shared__ uint32_t s_t[TSDF_SCAN_THREADS / CPPF_WAVE], s_c[TSDF_SCAN_THREADS / CPPF_WAVE];
  uint32_t carry_t = 0, carry_c = 0;
  const int wv = threadIdx.x / CPPF_WAVE;
  for (uint32_t b0 = 0; b0 < nb; b0 += TSDF_SCAN_THREADS) {
    const uint32_t b = b0 + threadIdx.x;
    const uint32_t nt = b < nb ? ws[b] : 0u, nc = b < nb ? ws[nb + b] : 0u;
    const uint32_t it = wave_inclusive_scan_u32(nt), ic = wave_inclusive_scan_u32(nc);
    if (wave_lane() == CPPF_WAVE - 1) { s_t[wv] = it; s_c[wv] = ic; }
    __syncthreads();
    uint32_t base = 0, tot_t = 0, tot_c = 0;
#pragma unroll
    for (int w = 0; w < TSDF_SCAN_THREADS / CPPF_WAVE; ++w) {
      const uint32_t x = s_t[w];
      base += w < wv ? x : 0u;
      tot_t += x;
      tot_c += s_c[w];
    }
    if (b < nb) ws[b] = carry_t + base + (it - nt);
    carry_t += tot_t;
    carry_c += tot_c;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ws[2 * (int64_t)nb] = carry_t;
    ws[2 * (int64_t)nb + 1] = carry_c;
    status[0] = (int64_t)carry_t;
    status[1] = (int64_t)carry_c;
  }
}

// One tetrahedron's triangles written at tri / key row `at`; returns the rows written.
template <int V1, int V2, bool ODD>
__device__ __forceinline__ uint32_t tet_emit(const float* t, int inside, int i, int j, int k, int64_t lin, const TsdfGrid& g,
                                             float* __restrict__ tris, int64_t* __restrict__ keys, int64_t at) {
  const int m = tet_mask<V1, V2>(inside);
  const int ntri = tet_triangles(m);
  if (ntri == 0) return 0;
  const float t0 = t[0], t1 = t[V1], t2 = t[V2], t3 = t[7];
  const uint32_t edges = TET_CASES[m];
  float px[4], py[4], pz[4];
  int64_t key[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int lo = (edges >> (4 * q)) & 3, hi = (edges >> (4 * q + 2)) & 3;
    const int clo = lo == 0 ? 0 : (lo == 1 ? V1 : (lo == 2 ? V2 : 7)), chi = hi == 1 ? V1 : (hi == 2 ? V2 : 7);
    const float tl = lo == 0 ? t0 : (lo == 1 ? t1 : (lo == 2 ? t2 : t3)), th = hi == 1 ? t1 : (hi == 2 ? t2 : t3);
    const int d = chi ^ clo;                     // the corners of a tetrahedron are nested: hi's offsets contain lo's
    const float s = tl / (tl - th);
    const int li = i + (clo & 1), lj = j + ((clo >> 1) & 1), lk = k + ((clo >> 2) & 1);
    px[q] = g.ox + ((float)li + ((d & 1) ? s : 0.0f)) * g.voxel;
    py[q] = g.oy + ((float)lj + ((d & 2) ? s : 0.0f)) * g.voxel;
    pz[q] = g.oz + ((float)lk + ((d & 4) ? s : 0.0f)) * g.voxel;
    const int64_t llin = lin + (int64_t)(clo & 1) * g.ny * g.nz + (int64_t)((clo >> 1) & 1) * g.nz + ((clo >> 2) & 1);
    key[q] = 8 * llin + d;
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (r < ntri) {
      const int b = ODD ? r + 2 : r + 1, c = ODD ? r + 1 : r + 2;          // compile-time after unrolling
      float* o = tris + 9 * (at + r);
      o[0] = px[0]; o[1] = py[0]; o[2] = pz[0];
      o[3] = px[b]; o[4] = py[b]; o[5] = pz[b];
      o[6] = px[c]; o[7] = py[c]; o[8] = pz[c];
      int64_t* ko = keys + 3 * (at + r);
      ko[0] = key[0]; ko[1] = key[b]; ko[2] = key[c];
    }
  }
  return (uint32_t)ntri;
}

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_emit_kernel(const float* __restrict__ acc, const int32_t* __restrict__ wsum,
                                                                 TsdfGrid g, int min_weight, int64_t cells, uint32_t nb,
                                                                 const uint32_t* __restrict__ ws, int64_t capacity,
                                                                 float* __restrict__ tris, int64_t* __restrict__ keys) {
  __shared__ uint32_t s_t[TSDF_THREADS / CPPF_WAVE];
  if ((int64_t)ws[2 * (int64_t)nb] > capacity) return;                       // the same for every thread of the grid
  const int64_t c = (int64_t)blockIdx.x * TSDF_THREADS + threadIdx.x;
  uint32_t n = 0;
  int i = 0, j = 0, k = 0, inside = 0;
  int64_t lin = 0;
  float t[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) t[q] = 0.0f;
  if (c < cells) {
    lin = cell_node(c, g, &i, &j, &k);
    inside = cell_corners(acc, wsum, lin, g.ny, g.nz, min_weight, t);
    n = inside > 0 && inside < 255 ? (uint32_t)cell_triangles(inside) : 0u;
  }
  const uint32_t incl = wave_inclusive_scan_u32(n);
  if (wave_lane() == CPPF_WAVE - 1) s_t[threadIdx.x / CPPF_WAVE] = incl;
  __syncthreads();
  uint32_t base = ws[blockIdx.x];
#pragma unroll
  for (int w = 0; w < TSDF_THREADS / CPPF_WAVE; ++w) base += w < (int)(threadIdx.x / CPPF_WAVE) ? s_t[w] : 0u;
  if (n == 0) return;
  int64_t at = (int64_t)base + (incl - n);
  at += tet_emit<1, 3, false>(t, inside, i, j, k, lin, g, tris, keys, at);      // (x,y,z)
  at += tet_emit<1, 5, true>(t, inside, i, j, k, lin, g, tris, keys, at);       // (x,z,y)
  at += tet_emit<2, 3, true>(t, inside, i, j, k, lin, g, tris, keys, at);       // (y,x,z)
  at += tet_emit<2, 6, false>(t, inside, i, j, k, lin, g, tris, keys, at);      // (y,z,x)
  at += tet_emit<4, 5, false>(t, inside, i, j, k, lin, g, tris, keys, at);      // (z,x,y)
  at += tet_emit<4, 6, true>(t, inside, i, j, k, lin, g, tris, keys, at);       // (z,y,x)
}

static bool tsdf_positive(float x) { return x > 0.0f && x < INFINITY; }

static bool tsdf_grid(const double* h_origin, float voxel, int nx, int ny, int nz, TsdfGrid* g) {
  if (!h_origin || nx < 1 || ny < 1 || nz < 1 || !tsdf_positive(voxel)) return false;
  if ((int64_t)nx * ny > TSDF_MAX_NODES || (int64_t)nx * ny * nz > TSDF_MAX_NODES) return false;
  g->ox = (float)h_origin[0]; g->oy = (float)h_origin[1]; g->oz = (float)h_origin[2];
  g->voxel = voxel; g->nx = nx; g->ny = ny; g->nz = nz;
  return __builtin_isfinite(g->ox) && __builtin_isfinite(g->oy) && __builtin_isfinite(g->oz);
}

static int64_t tsdf_cells(int nx, int ny, int nz) { return (int64_t)(nx - 1) * (ny - 1) * (nz - 1); }

#undef CPPF_FN
#define CPPF_FN fn                       // the shared host function reports under its entry point's name
template <bool WEIGHTED>
static int tsdf_integrate(int V, const float* depth, const uint8_t* masks, const float* poses, const uint8_t* weights,
                          int carve_weight, int H, int W, const double* h_K, float pixel_offset, const double* h_origin, float voxel,
                          int nx, int ny, int nz, float trunc, float znear, float* acc, int32_t* wsum, void* stream) {
  const char* fn = WEIGHTED ? "cppf_tsdf_integrate_weighted" : "cppf_tsdf_integrate";
  TsdfGrid g;
  CPPF_CHECK_ARG(tsdf_grid(h_origin, voxel, nx, ny, nz, &g));
  CPPF_CHECK_ARG(V >= 0 && V <= TSDF_MAX_VIEWS);
  CPPF_CHECK_ARG(H >= 1 && H <= TSDF_MAX_IMAGE && W >= 1 && W <= TSDF_MAX_IMAGE);
  CPPF_CHECK_ARG(tsdf_positive(trunc) && tsdf_positive(znear) && __builtin_isfinite(pixel_offset));
  CPPF_CHECK_ARG(h_K && acc && wsum);
  CPPF_CHECK_ARG(!WEIGHTED || (carve_weight >= 0 && carve_weight <= 255));
  if (V == 0) return CPPF_OK;
  CPPF_CHECK_ARG(depth && poses);
  CPPF_CHECK_ARG(!WEIGHTED || weights);
  const int64_t nodes = (int64_t)nx * ny * nz;
  const unsigned int nb = (unsigned int)((nodes + TSDF_THREADS - 1) / TSDF_THREADS);
  hipLaunchKernelGGL(tsdf_integrate_kernel<WEIGHTED>, dim3(nb), dim3(TSDF_THREADS), 0, (hipStream_t)stream, V, depth, masks, poses,
                     weights, carve_weight, H, W, (float)h_K[0], (float)h_K[1], (float)h_K[2], (float)h_K[3], pixel_offset, g, trunc,
                     znear, nodes, acc, wsum);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
#undef CPPF_FN
#define CPPF_FN __func__

extern "C" int cppf_tsdf_integrate(int V, const float* depth, const uint8_t* masks, const float* poses, int H, int W,
                                   const double* h_K, float pixel_offset, const double* h_origin, float voxel, int nx, int ny,
                                   int nz, float trunc, float znear, float* acc, int32_t* wsum, void* stream) {
  return tsdf_integrate<false>(V, depth, masks, poses, nullptr, 0, H, W, h_K, pixel_offset, h_origin, voxel, nx, ny, nz, trunc, znear,
                               acc, wsum, stream);
}

extern "C" int cppf_tsdf_integrate_weighted(int V, const float* depth, const uint8_t* masks, const float* poses,
                                            const uint8_t* weights, int carve_weight, int H, int W, const double* h_K,
                                            float pixel_offset, const double* h_origin, float voxel, int nx, int ny, int nz,
                                            float trunc, float znear, float* acc, int32_t* wsum, void* stream) {
  return tsdf_integrate<true>(V, depth, masks, poses, weights, carve_weight, H, W, h_K, pixel_offset, h_origin, voxel, nx, ny, nz,
                              trunc, znear, acc, wsum, stream);
}

extern "C" int64_t cppf_tsdf_extract_workspace_bytes(int nx, int ny, int nz) {
  if (nx < 1 || ny < 1 || nz < 1 || (int64_t)nx * ny > TSDF_MAX_NODES || (int64_t)nx * ny * nz > TSDF_MAX_NODES) return -1;
  const int64_t nb = (tsdf_cells(nx, ny, nz) + TSDF_THREADS - 1) / TSDF_THREADS;
  return (2 * nb + 2) * (int64_t)sizeof(uint32_t);
}

extern "C" int cppf_tsdf_extract(const float* acc, const int32_t* wsum, const double* h_origin, float voxel, int nx, int ny, int nz,
                                 int min_weight, int64_t capacity, float* tris, int64_t* keys, int64_t* status, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
  TsdfGrid g;
  CPPF_CHECK_ARG(tsdf_grid(h_origin, voxel, nx, ny, nz, &g));
  CPPF_CHECK_ARG(min_weight >= 1);
  CPPF_CHECK_ARG(capacity >= 0);
  CPPF_CHECK_ARG(acc && wsum && status && workspace);
  CPPF_CHECK_ARG(capacity == 0 || (tris && keys));
  CPPF_CHECK_ARG(workspace_bytes >= cppf_tsdf_extract_workspace_bytes(nx, ny, nz));
  hipStream_t st = (hipStream_t)stream;
  const int64_t cells = tsdf_cells(nx, ny, nz);
  if (cells == 0) {
    CPPF_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int64_t), st));
    return CPPF_OK;
  }
  const unsigned int nb = (unsigned int)((cells + TSDF_THREADS - 1) / TSDF_THREADS);
  uint32_t* ws = (uint32_t*)workspace;
  hipLaunchKernelGGL(tsdf_count_kernel, dim3(nb), dim3(TSDF_THREADS), 0, st, acc, wsum, g, min_weight, cells, nb, ws);
  CPPF_LAUNCH_CHECK();
  hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), dim3(TSDF_SCAN_THREADS), 0, st, nb, ws, status);
  CPPF_LAUNCH_CHECK();
  if (capacity > 0) {
    hipLaunchKernelGGL(tsdf_emit_kernel, dim3(nb), dim3(TSDF_THREADS), 0, st, acc, wsum, g, min_weight, cells, nb,
                       (const uint32_t*)ws, capacity, tris, keys);
    CPPF_LAUNCH_CHECK();
  }
  return CPPF_OK;
}
