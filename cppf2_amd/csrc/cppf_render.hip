// Batched depth-only triangle rasterizer (the render step of the reference's data generation: dataset.py:177-319
// ShapeNetDirectDataset, dataset.py:371-413 dump_data, train_custom.ipynb cell 4 -- pyrender over OpenGL there).
//
// Four launches on the caller's stream after the clears (depth = 0, tri_id = -1, status = 0, tile counters = 0):
//   1. render_setup   one thread per (view, triangle): model -> OpenCV camera transform, projection, snap to 1/256 px,
//                     rejection / culling, canonical winding, one 48-byte record, +1 on each 16x16 tile its pixel bbox touches;
//   2. render_scan    one workgroup: exclusive scan of the per-(view, tile) counts -> list offsets; status[1] = total;
//   3. render_scatter one thread per triangle: its global id into the list of every tile it touches (skipped when the
//                     lists need more than list_capacity entries);
//   4. render_raster  one 256-thread workgroup per (view, tile), one pixel per thread: the tile's records stream through LDS
//                     in chunks of 256; each thread keeps its (z, local id) minimum in registers -- no atomics, so the
//                     result does not depend on the order of the list (which the scatter's atomics make arbitrary).
//
// Arithmetic (tests/render_ref.py mirrors it in NumPy float32 / int64; the build's -ffp-contract=off and correctly rounded
// division keep every float op below rounding where it is written):
//   xc = ((p0*x + p1*y) + p2*z) + p3   (same for yc, zc)
//   su = rint((fx*(xc/zc) + cx) * 256)   sv = rint((fy*(yc/zc) + cy) * 256)   (integers, 1/256 px)
//   pixel (r, c) samples (256c + 128, 256r + 128); edge functions in int64; top-left fill rule (image y down)
//   depth = area / ((f(e0)*iz0 + f(e1)*iz1) + f(e2)*iz2), iz = 1/zc, f = int64 -> float32 (round to nearest even)
#include "cppf_common.h"

#define RENDER_TILE 16
#define RENDER_THREADS 256
#define RENDER_SCAN_THREADS 1024
#define RENDER_GUARD 1073741824.0f      // 2^22 px in 1/256 px units: snapped coordinates must lie strictly inside
#define RENDER_MAX_DIM 8192             // H, W: keeps 256*(W-1)+128 - x inside int32 for every |x| < 2^30

// One triangle after setup, canonical winding (positive area with image y down), coordinates in 1/256 px.
struct RenderRec {
  int32_t x0, y0, x1, y1, x2, y2;
  float iz0, iz1, iz2;    // 1 / camera z of each vertex
  float area;             // (float) twice the signed area (> 0)
  int32_t id;             // triangle index within its view's range (tri_off[b] .. tri_off[b+1])
  int32_t tl;             // bit k: edge k is a top or left edge (edge 0 = v1->v2, 1 = v2->v0, 2 = v0->v1)
};
static_assert(sizeof(RenderRec) == 48, "RenderRec is read as three 16-byte words");

// Tile range of one record: view (-1 = draws nothing), tiles [c0, c1] x [r0, r1] packed as 16-bit pairs.
struct RenderBin {
  int32_t b, lo, hi, pad;
};

__device__ __forceinline__ int64_t render_edge(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t px, int32_t py) {
  // (b - a) x (p - a); every operand fits int32 (|coordinate| < 2^30), the products are exact in int64
  return (int64_t)(bx - ax) * (int64_t)(py - ay) - (int64_t)(by - ay) * (int64_t)(px - ax);
}

__device__ __forceinline__ bool render_top_left(int32_t ax, int32_t ay, int32_t bx, int32_t by) {
  const int32_t dy = by - ay;
  return dy < 0 || (dy == 0 && bx > ax);
}

__global__ __launch_bounds__(RENDER_THREADS) void render_setup_kernel(
    const float* __restrict__ verts, int64_t num_verts, const int32_t* __restrict__ tris, const int32_t* __restrict__ tri_off,
    int B, int64_t total, const float* __restrict__ poses, float fx, float fy, float cx, float cy, int H, int W, int tiles_x,
    int tiles_y, float znear, int cull, RenderRec* __restrict__ rec, RenderBin* __restrict__ bin, int32_t* __restrict__ tile_count,
    unsigned long long* __restrict__ status) {
  const int64_t g = (int64_t)blockIdx.x * RENDER_THREADS + threadIdx.x;
  if (g >= total) return;
  RenderBin bn;
  bn.b = -1; bn.lo = 0; bn.hi = 0; bn.pad = 0;
  // the view: the largest b with tri_off[b] <= g (a malformed tri_off leaves g without a view: rejected, never out of bounds)
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int64_t)tri_off[mid] <= g) lo = mid; else hi = mid - 1;
  }
  const int b = lo;
  const int64_t t0 = tri_off[b], t1 = tri_off[b + 1];
  bool reject = !(t0 <= g && g < t1);
  int32_t vi[3] = {0, 0, 0};
  if (!reject) {
    vi[0] = tris[3 * g]; vi[1] = tris[3 * g + 1]; vi[2] = tris[3 * g + 2];
    reject = vi[0] < 0 || vi[1] < 0 || vi[2] < 0 || vi[0] >= num_verts || vi[1] >= num_verts || vi[2] >= num_verts;
  }
  int32_t sx[3], sy[3];
  float iz[3];
  if (!reject) {
    const float* P = poses + 12 * (int64_t)b;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float x = verts[3 * (int64_t)vi[k]], y = verts[3 * (int64_t)vi[k] + 1], z = verts[3 * (int64_t)vi[k] + 2];
      const float xc = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
      const float yc = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
      const float zc = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
      const float u = rintf((fx * (xc / zc) + cx) * 256.0f);
      const float v = rintf((fy * (yc / zc) + cy) * 256.0f);
      // NaN fails every comparison: rejected too
      if (!(zc >= znear) || !(fabsf(u) < RENDER_GUARD) || !(fabsf(v) < RENDER_GUARD)) reject = true;
      sx[k] = reject ? 0 : (int32_t)u;
      sy[k] = reject ? 0 : (int32_t)v;
      iz[k] = 1.0f / zc;
    }
  }
  if (reject) {
    atomicAdd(&status[0], 1ull);
    bin[g] = bn;
    return;
  }
  int64_t area = (int64_t)(sx[1] - sx[0]) * (int64_t)(sy[2] - sy[0]) - (int64_t)(sy[1] - sy[0]) * (int64_t)(sx[2] - sx[0]);
  // area < 0: (v1-v0)x(v2-v0) points toward the camera (front face); area > 0: back face
  bool draw = area != 0 && !(cull && area > 0);
  RenderRec r;
  r.x0 = sx[0]; r.y0 = sy[0];
  if (area < 0) {         // canonical winding: swap v1 and v2
    r.x1 = sx[2]; r.y1 = sy[2]; r.x2 = sx[1]; r.y2 = sy[1];
    r.iz0 = iz[0]; r.iz1 = iz[2]; r.iz2 = iz[1];
    area = -area;
  } else {
    r.x1 = sx[1]; r.y1 = sy[1]; r.x2 = sx[2]; r.y2 = sy[2];
    r.iz0 = iz[0]; r.iz1 = iz[1]; r.iz2 = iz[2];
  }
  r.area = (float)area;
  r.id = (int32_t)(g - t0);
  r.tl = (render_top_left(r.x1, r.y1, r.x2, r.y2) ? 1 : 0) | (render_top_left(r.x2, r.y2, r.x0, r.y0) ? 2 : 0) |
         (render_top_left(r.x0, r.y0, r.x1, r.y1) ? 4 : 0);
  // pixels whose sample point (256c + 128) lies in [min, max]; >> floors for negative values
  const int32_t mnx = min(r.x0, min(r.x1, r.x2)), mxx = max(r.x0, max(r.x1, r.x2));
  const int32_t mny = min(r.y0, min(r.y1, r.y2)), mxy = max(r.y0, max(r.y1, r.y2));
  const int32_t c0 = max((mnx + 127) >> 8, 0), c1 = min((mxx - 128) >> 8, W - 1);
  const int32_t r0 = max((mny + 127) >> 8, 0), r1 = min((mxy - 128) >> 8, H - 1);
  draw = draw && c0 <= c1 && r0 <= r1;
  if (draw) {
    const int tc0 = c0 / RENDER_TILE, tc1 = c1 / RENDER_TILE, tr0 = r0 / RENDER_TILE, tr1 = r1 / RENDER_TILE;
    bn.b = b;
    bn.lo = tc0 | (tr0 << 16);
    bn.hi = tc1 | (tr1 << 16);
    int32_t* cnt = tile_count + (int64_t)b * tiles_x * tiles_y;
    for (int ty = tr0; ty <= tr1; ++ty)
      for (int tx = tc0; tx <= tc1; ++tx) atomicAdd(&cnt[ty * tiles_x + tx], 1);
    rec[g] = r;
  }
  bin[g] = bn;
}

// Exclusive scan of n tile counts (one workgroup; each thread owns one contiguous chunk) -> start[0..n]; status[1] = start[n].
__global__ __launch_bounds__(RENDER_SCAN_THREADS) void render_scan_kernel(const int32_t* __restrict__ count, int64_t n,
                                                                          int64_t* __restrict__ start,
                                                                          unsigned long long* __restrict__ status) {
  __shared__ int64_t s_part[RENDER_SCAN_THREADS];
  const int t = threadIdx.x;
  const int64_t chunk = (n + RENDER_SCAN_THREADS - 1) / RENDER_SCAN_THREADS;
  const int64_t a = min((int64_t)t * chunk, n), e = min(a + chunk, n);
  int64_t sum = 0;
  for (int64_t i = a; i < e; ++i) sum += count[i];
  s_part[t] = sum;
  __syncthreads();
  for (int off = 1; off < RENDER_SCAN_THREADS; off <<= 1) {       // Hillis-Steele inclusive scan of the chunk sums
    const int64_t add = t >= off ? s_part[t - off] : 0;
    __syncthreads();
    s_part[t] += add;
    __syncthreads();
  }
  int64_t run = s_part[t] - sum;
  for (int64_t i = a; i < e; ++i) {
    start[i] = run;
    run += count[i];
  }
  if (t == RENDER_SCAN_THREADS - 1) {
    start[n] = s_part[t];
    status[1] = (unsigned long long)s_part[t];
  }
}

__global__ __launch_bounds__(RENDER_THREADS) void render_scatter_kernel(const RenderBin* __restrict__ bin, int64_t total, int tiles_x,
                                                                        int tiles_y, int32_t* __restrict__ tile_count,
                                                                        const int64_t* __restrict__ start, int32_t* __restrict__ list,
                                                                        int64_t capacity, const unsigned long long* __restrict__ status) {
  const int64_t g = (int64_t)blockIdx.x * RENDER_THREADS + threadIdx.x;
  if (g >= total || (int64_t)status[1] > capacity) return;
  const RenderBin bn = bin[g];
  if (bn.b < 0) return;
  const int64_t base = (int64_t)bn.b * tiles_x * tiles_y;
  const int tc0 = bn.lo & 0xffff, tr0 = bn.lo >> 16, tc1 = bn.hi & 0xffff, tr1 = bn.hi >> 16;
  for (int ty = tr0; ty <= tr1; ++ty)
    for (int tx = tc0; tx <= tc1; ++tx) {
      const int64_t tile = base + ty * tiles_x + tx;
      // the count runs down from the tile's total: slots start[tile] .. start[tile + 1] - 1, each taken once
      const int32_t pos = atomicSub(&tile_count[tile], 1) - 1;
      list[start[tile] + pos] = (int32_t)g;
    }
}

__global__ __launch_bounds__(RENDER_THREADS) void render_raster_kernel(const RenderRec* __restrict__ rec, const int64_t* __restrict__ start,
                                                                       const int32_t* __restrict__ list, int64_t capacity,
                                                                       const unsigned long long* __restrict__ status, int H, int W,
                                                                       int tiles_x, float znear, float zfar, float* __restrict__ depth,
                                                                       int32_t* __restrict__ tri_id) {
  __shared__ RenderRec s_rec[RENDER_THREADS];
  if ((int64_t)status[1] > capacity) return;          // lists were not written: the output stays cleared (marked invalid)
  const int b = blockIdx.y;
  const int64_t tile = (int64_t)b * gridDim.x + blockIdx.x;
  const int64_t s = start[tile], e = start[tile + 1];
  if (s == e) return;
  const int t = threadIdx.x;
  const int c = (blockIdx.x % tiles_x) * RENDER_TILE + (t & (RENDER_TILE - 1));
  const int r = (blockIdx.x / tiles_x) * RENDER_TILE + (t / RENDER_TILE);
  const int32_t px = 256 * c + 128, py = 256 * r + 128;
  float bz = INFINITY;
  int32_t bid = -1;
  for (int64_t k0 = s; k0 < e; k0 += RENDER_THREADS) {
    __syncthreads();
    if (k0 + t < e) s_rec[t] = rec[list[k0 + t]];
    __syncthreads();
    const int n = (int)min((int64_t)RENDER_THREADS, e - k0);
    for (int j = 0; j < n; ++j) {
      const RenderRec q = s_rec[j];
      const int64_t e0 = render_edge(q.x1, q.y1, q.x2, q.y2, px, py);
      if (e0 < (int64_t)((q.tl & 1) ? 0 : 1)) continue;
      const int64_t e1 = render_edge(q.x2, q.y2, q.x0, q.y0, px, py);
      if (e1 < (int64_t)((q.tl & 2) ? 0 : 1)) continue;
      const int64_t e2 = render_edge(q.x0, q.y0, q.x1, q.y1, px, py);
      if (e2 < (int64_t)((q.tl & 4) ? 0 : 1)) continue;
      float w = (float)e0 * q.iz0;
      w = w + (float)e1 * q.iz1;
      w = w + (float)e2 * q.iz2;
      const float z = q.area / w;
      if (!(z >= znear && z <= zfar)) continue;
      if (z < bz || (z == bz && q.id < bid)) {
        bz = z;
        bid = q.id;
      }
    }
  }
  if (c < W && r < H && bid >= 0) {
    const int64_t o = ((int64_t)b * H + r) * W + c;
    depth[o] = bz;
    if (tri_id) tri_id[o] = bid;
  }
}

struct RenderLayout {
  int64_t rec, bin, count, start, list, bytes;
};

static bool render_layout(int B, int64_t total, int H, int W, int64_t cap, RenderLayout* L) {
  if (B < 1 || B > 65535 || total < 0 || total > 0x7fffffffLL || H < 1 || W < 1 || H > RENDER_MAX_DIM || W > RENDER_MAX_DIM ||
      cap < 0 || cap > 0x7fffffffLL)
    return false;
  const int64_t tiles = (int64_t)B * ((W + RENDER_TILE - 1) / RENDER_TILE) * ((H + RENDER_TILE - 1) / RENDER_TILE);
  L->rec = 0;
  L->bin = L->rec + align_up(total * (int64_t)sizeof(RenderRec), 256);
  L->count = L->bin + align_up(total * (int64_t)sizeof(RenderBin), 256);
  L->start = L->count + align_up(tiles * 4, 256);
  L->list = L->start + align_up((tiles + 1) * 8, 256);
  L->bytes = L->list + align_up(cap * 4, 256);
  return true;
}

extern "C" int64_t cppf_render_depth_workspace_bytes(int B, int64_t total_tris, int H, int W, int64_t list_capacity) {
  RenderLayout L;
  if (!render_layout(B, total_tris, H, W, list_capacity, &L)) return CPPF_EINVAL;
  return L.bytes;
}

extern "C" int cppf_render_depth(int B, const float* verts, int64_t num_verts, const int32_t* tris, const int32_t* tri_off,
                                 int64_t total_tris, const float* poses, const double* h_K, int H, int W, float znear, float zfar,
                                 int cull, float* depth, int32_t* tri_id, int64_t* status, void* workspace, int64_t workspace_bytes,
                                 int64_t list_capacity, void* stream) {
  RenderLayout L;
  CPPF_CHECK_ARG(render_layout(B, total_tris, H, W, list_capacity, &L));
  CPPF_CHECK_ARG(tri_off && poses && h_K && depth && status && workspace && workspace_bytes >= L.bytes);
  CPPF_CHECK_ARG(total_tris == 0 || (verts && tris && num_verts > 0 && num_verts <= 0x7fffffffLL));
  CPPF_CHECK_ARG(cull == 0 || cull == 1);
  CPPF_CHECK_ARG(znear > 0.0f && zfar > znear);
  for (int i = 0; i < 4; ++i) CPPF_CHECK_ARG(h_K[i] == h_K[i] && fabs(h_K[i]) < 1e30);
  CPPF_CHECK_ARG(h_K[0] > 0.0 && h_K[1] > 0.0);
  hipStream_t st = (hipStream_t)stream;
  const int tiles_x = (W + RENDER_TILE - 1) / RENDER_TILE, tiles_y = (H + RENDER_TILE - 1) / RENDER_TILE;
  const int64_t tiles = (int64_t)B * tiles_x * tiles_y;
  char* ws = (char*)workspace;
  RenderRec* rec = (RenderRec*)(ws + L.rec);
  RenderBin* bin = (RenderBin*)(ws + L.bin);
  int32_t* count = (int32_t*)(ws + L.count);
  int64_t* start = (int64_t*)(ws + L.start);
  int32_t* list = (int32_t*)(ws + L.list);
  unsigned long long* stat = (unsigned long long*)status;
  const size_t pixels = (size_t)B * H * W;
  CPPF_HIP(hipMemsetAsync(depth, 0, pixels * sizeof(float), st));
  if (tri_id) CPPF_HIP(hipMemsetAsync(tri_id, 0xff, pixels * sizeof(int32_t), st));
  CPPF_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int64_t), st));
  CPPF_HIP(hipMemsetAsync(count, 0, (size_t)tiles * 4, st));
  const int64_t blocks = (total_tris + RENDER_THREADS - 1) / RENDER_THREADS;
  if (blocks > 0)
    hipLaunchKernelGGL(render_setup_kernel, dim3((unsigned)blocks), dim3(RENDER_THREADS), 0, st, verts, num_verts, tris, tri_off, B,
                       total_tris, poses, (float)h_K[0], (float)h_K[1], (float)h_K[2], (float)h_K[3], H, W, tiles_x, tiles_y, znear,
                       cull, rec, bin, count, stat);
  CPPF_LAUNCH_CHECK();
  hipLaunchKernelGGL(render_scan_kernel, dim3(1), dim3(RENDER_SCAN_THREADS), 0, st, count, tiles, start, stat);
  CPPF_LAUNCH_CHECK();
  if (blocks > 0)
    hipLaunchKernelGGL(render_scatter_kernel, dim3((unsigned)blocks), dim3(RENDER_THREADS), 0, st, bin, total_tris, tiles_x, tiles_y,
                       count, start, list, list_capacity, stat);
  CPPF_LAUNCH_CHECK();
  hipLaunchKernelGGL(render_raster_kernel, dim3(tiles_x * tiles_y, B), dim3(RENDER_THREADS), 0, st, rec, start, list, list_capacity,
                     stat, H, W, tiles_x, znear, zfar, depth, tri_id);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
