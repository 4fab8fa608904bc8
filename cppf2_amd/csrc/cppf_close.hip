// A fused volume closed where no view saw it: the space that is enclosed and never observed becomes inside, and an optional
// support plane cuts the solid off at the table (cppf2_amd/fuse.py's close).  The reference has no such
// step.  gfx950 only.  tests/close_ref.py restates every definition below in NumPy; the build's -ffp-contract=off keeps every
// float32 operation where it is written and the divide is correctly rounded.
//
// cppf_tsdf_close reads the volume of cppf_tsdf_integrate (cppf_fuse.hip: acc float32, wsum int32, [nx,ny,nz], z fastest, linear
//   node index lin = (i * ny + j) * nz + k) and writes a NEW volume acc_out / wsum_out plus state uint8 per node and stats int64
//   [4], the nodes per state.  The plane is (a, b, c, d) with unit normal, the object on the positive side, rounded to float32
//   once.  Per node, float32, left to right:
//     known = wsum >= min_weight;   t = known ? acc / (float)wsum : -1
//     plane:     x = ox + (float)i * voxel, y, z alike (as integrate computes them);  h = ((a*x + b*y) + c*z) + d
//                q = (-h) / trunc;  b = q < -1 ? -1 : (q > 1 ? 1 : q);  below = h <= 0
//     no plane:  b = -1, below = false
//     candidate = !known && !below.  Candidates are joined by 6-connectivity; a component is OPEN iff it holds a node on a face
//                of the volume (an index of 0 or n-1 on any axis: on an axis of length 1 every node).
//     open candidate:    acc_out = 0, wsum_out = 0, state = 3      (still unknown: cppf_tsdf_extract skips its cells)
//     every other node:  acc_out = (b > t) ? b : t, wsum_out = 1, state = 0 known, 1 enclosed candidate, 2 unseen and below
//   i.e. the solid (observed, or enclosed and never seen) intersected with the half-space above the plane; acc_out / 1 is the
//   value cppf_tsdf_extract(min_weight = 1) sees, bit for bit.  A NaN t of a known node stays NaN (b > NaN is false).
//
//   The stats are cleared and four launches follow on the stream, 256 threads, one lane per node in linear order (lanes run
//   along z: coalesced rows), no host synchronisation and no loop "until nothing changes".  Launches 1 and 4 count, so their
//   blocks (2 048 at most) stride over the nodes: with one block per 256 nodes the two atomics per block on the same two words
//   were the whole launch (measured: 6 ns each, 0.79 ms at 256^3).
//   1 init     every node's outputs as if no candidate were open (a candidate: the enclosed values, state 1);
//              label[lin] = candidate ? lin : -1;  stats[0], stats[2] (ballots, one integer atomic per counter and block)
//   2 merge    cppf_mask.hip's label-equivalence union-find (cppf_cc.h) over the 3-D lattice: each candidate unites itself
//              with its +z, +y and +x neighbour when that is a candidate too (read from state, which this launch does not
//              write).  At the end every root is its component's lowest linear index, whatever the schedule.
//   3 flag     every candidate on a face finds its root r and stores state[r] = 3.  Roots do not change after launch 2 (find
//              only shortens paths), and 3 is the only value this launch stores, so the order does not matter.
//   4 resolve  every candidate finds its root; if state[root] == 3 it takes the open outputs.  state[root] is written in this
//              launch only by the root's own lane and only with the value it already holds.  stats[1], stats[3] as in launch 1.
//   The outputs depend on component membership only, so they are bit-reproducible.  The union-find words go through agent-scope
//   atomic loads and atomicMin (cppf_cc.h); everything else is plain vector loads and stores of values that are constant within
//   the launch that reads them.  workspace: the labels, int32 [nx ny nz] (2^27 nodes fit).
//   Not done: a tile merged in LDS before the global merge (it would cut the global atomics per node from 3 to the tile's
//   surface) -- not built because both forms would have to be measured side by side.
#include "cppf_common.h"
#include "cppf_cc.h"

#include <math.h>

#define CLOSE_THREADS 256
#define CLOSE_WAVES (CLOSE_THREADS / CPPF_WAVE)
#define CLOSE_MAX_NODES (1LL << 27)       // cppf_tsdf_integrate's limit
#define CLOSE_MAX_BLOCKS 2048             // blocks of the two counting launches at most (8 per CU): they stride over the nodes

struct CloseGrid {
  float ox, oy, oz, voxel;
  int nx, ny, nz;
};

struct ClosePlane {
  float a, b, c, d;
  int on;
};

// (i,j,k) of the linear node index
__device__ __forceinline__ void close_ijk(int64_t lin, const CloseGrid& g, int* i, int* j, int* k) {
  *k = (int)(lin % g.nz);
  const int64_t ij = lin / g.nz;
  *j = (int)(ij % g.ny);
  *i = (int)(ij / g.ny);
}

__device__ __forceinline__ bool close_on_face(int i, int j, int k, const CloseGrid& g) {
  return i == 0 || i == g.nx - 1 || j == 0 || j == g.ny - 1 || k == 0 || k == g.nz - 1;
}

// The wavefronts' counts cp and cq (every lane of a wavefront holds its wavefront's) summed over the block and added to *np and
// *nq.  Every thread of the block calls it.
__device__ __forceinline__ void close_count(uint32_t cp, uint32_t cq, unsigned long long* np, unsigned long long* nq) {
  __shared__ uint32_t s_p[CLOSE_WAVES], s_q[CLOSE_WAVES];
  if (wave_lane() == 0) {
    s_p[threadIdx.x / CPPF_WAVE] = cp;
    s_q[threadIdx.x / CPPF_WAVE] = cq;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sp = 0, sq = 0;
#pragma unroll
    for (int w = 0; w < CLOSE_WAVES; ++w) { sp += s_p[w]; sq += s_q[w]; }
    if (sp) atomicAdd(np, (unsigned long long)sp);
    if (sq) atomicAdd(nq, (unsigned long long)sq);
  }
}

__global__ __launch_bounds__(CLOSE_THREADS) void close_init_kernel(const float* __restrict__ acc, const int32_t* __restrict__ wsum,
                                                                   CloseGrid g, float trunc, int min_weight, ClosePlane pl,
                                                                   int64_t nodes, float* __restrict__ acc_out,
                                                                   int32_t* __restrict__ wsum_out, uint8_t* __restrict__ state,
                                                                   int* __restrict__ labels, unsigned long long* __restrict__ stats) {
  uint32_t n_known = 0, n_below = 0;
  for (int64_t l0 = (int64_t)blockIdx.x * CLOSE_THREADS; l0 < nodes; l0 += (int64_t)gridDim.x * CLOSE_THREADS) {      // uniform
    const int64_t lin = l0 + threadIdx.x;
    bool is_known = false, is_below = false;
    if (lin < nodes) {
      const int32_t w = wsum[lin];
      const bool known = w >= min_weight;
      const float t = known ? acc[lin] / (float)w : -1.0f;
      float b = -1.0f;
      bool below = false;
      if (pl.on) {
        int i, j, k;
        close_ijk(lin, g, &i, &j, &k);
        const float x = g.ox + (float)i * g.voxel, y = g.oy + (float)j * g.voxel, z = g.oz + (float)k * g.voxel;
        const float h = ((pl.a * x + pl.b * y) + pl.c * z) + pl.d;
        const float q = (-h) / trunc;
        b = q < -1.0f ? -1.0f : (q > 1.0f ? 1.0f : q);
        below = h <= 0.0f;
      }
      const bool cand = !known && !below;
      acc_out[lin] = (b > t) ? b : t;
      wsum_out[lin] = 1;
      state[lin] = known ? (uint8_t)0 : (below ? (uint8_t)2 : (uint8_t)1);
      labels[lin] = cand ? (int)lin : -1;
      is_known = known;
      is_below = !known && below;
    }
    n_known += (uint32_t)__popcll(wave_ballot(is_known));            // every lane of the wavefront holds the wavefront's count
    n_below += (uint32_t)__popcll(wave_ballot(is_below));
  }
  close_count(n_known, n_below, stats + 0, stats + 2);
}

__global__ __launch_bounds__(CLOSE_THREADS) void close_merge_kernel(CloseGrid g, int64_t nodes, const uint8_t* __restrict__ state,
                                                                    int* __restrict__ labels) {
  const int64_t lin = (int64_t)blockIdx.x * CLOSE_THREADS + threadIdx.x;
  if (lin >= nodes || state[lin] != 1) return;
  int i, j, k;
  close_ijk(lin, g, &i, &j, &k);
  const int64_t sy = g.nz, sx = (int64_t)g.ny * g.nz;
  if (k + 1 < g.nz && state[lin + 1] == 1) cc_union(labels, (int)lin, (int)(lin + 1));
  if (j + 1 < g.ny && state[lin + sy] == 1) cc_union(labels, (int)lin, (int)(lin + sy));
  if (i + 1 < g.nx && state[lin + sx] == 1) cc_union(labels, (int)lin, (int)(lin + sx));
}

__global__ __launch_bounds__(CLOSE_THREADS) void close_flag_kernel(CloseGrid g, int64_t nodes, int* __restrict__ labels,
                                                                   uint8_t* __restrict__ state) {
  const int64_t lin = (int64_t)blockIdx.x * CLOSE_THREADS + threadIdx.x;
  if (lin >= nodes) return;
  int i, j, k;
  close_ijk(lin, g, &i, &j, &k);
  if (!close_on_face(i, j, k, g)) return;
  if (cc_load(labels + lin) < 0) return;
  state[cc_find(labels, (int)lin)] = 3;
}

__global__ __launch_bounds__(CLOSE_THREADS) void close_resolve_kernel(int64_t nodes, int* __restrict__ labels,
                                                                      float* __restrict__ acc_out, int32_t* __restrict__ wsum_out,
                                                                      uint8_t* __restrict__ state,
                                                                      unsigned long long* __restrict__ stats) {
  uint32_t n_enclosed = 0, n_open = 0;
  for (int64_t l0 = (int64_t)blockIdx.x * CLOSE_THREADS; l0 < nodes; l0 += (int64_t)gridDim.x * CLOSE_THREADS) {      // uniform
    const int64_t lin = l0 + threadIdx.x;
    bool enclosed = false, open = false;
    if (lin < nodes && cc_load(labels + lin) >= 0) {
      const int root = cc_find(labels, (int)lin);
      open = state[root] == 3;
      enclosed = !open;
      if (open) {
        acc_out[lin] = 0.0f;
        wsum_out[lin] = 0;
        state[lin] = 3;
      }
    }
    n_enclosed += (uint32_t)__popcll(wave_ballot(enclosed));
    n_open += (uint32_t)__popcll(wave_ballot(open));
  }
  close_count(n_enclosed, n_open, stats + 1, stats + 3);
}

static bool close_positive(float x) { return x > 0.0f && x < INFINITY; }

static bool close_sizes(int nx, int ny, int nz) {
  return nx >= 1 && ny >= 1 && nz >= 1 && (int64_t)nx * ny <= CLOSE_MAX_NODES && (int64_t)nx * ny * nz <= CLOSE_MAX_NODES;
}

// cppf_tsdf_extract's volume checks
static bool close_grid(const double* h_origin, float voxel, int nx, int ny, int nz, CloseGrid* g) {
  if (!h_origin || !close_sizes(nx, ny, nz) || !close_positive(voxel)) return false;
  g->ox = (float)h_origin[0]; g->oy = (float)h_origin[1]; g->oz = (float)h_origin[2];
  g->voxel = voxel; g->nx = nx; g->ny = ny; g->nz = nz;
  return __builtin_isfinite(g->ox) && __builtin_isfinite(g->oy) && __builtin_isfinite(g->oz);
}

// finite in float64 and after the rounding to float32, and a unit normal
static bool close_plane(const double* h_plane, ClosePlane* pl) {
  pl->a = pl->b = pl->c = pl->d = 0.0f;
  pl->on = h_plane != nullptr;
  if (!h_plane) return true;
  for (int q = 0; q < 4; ++q)
    if (!__builtin_isfinite(h_plane[q]) || !__builtin_isfinite((float)h_plane[q])) return false;
  const double n2 = h_plane[0] * h_plane[0] + h_plane[1] * h_plane[1] + h_plane[2] * h_plane[2];
  if (!(fabs(n2 - 1.0) <= 1e-3)) return false;
  pl->a = (float)h_plane[0]; pl->b = (float)h_plane[1]; pl->c = (float)h_plane[2]; pl->d = (float)h_plane[3];
  return true;
}

static bool close_disjoint(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x + (uintptr_t)na <= y || y + (uintptr_t)nb <= x;
}

extern "C" int64_t cppf_tsdf_close_workspace_bytes(int nx, int ny, int nz) {
  if (!close_sizes(nx, ny, nz)) return -1;
  return (int64_t)nx * ny * nz * (int64_t)sizeof(int);
}

extern "C" int cppf_tsdf_close(const float* acc, const int32_t* wsum, const double* h_origin, float voxel, int nx, int ny, int nz,
                               float trunc, int min_weight, const double* h_plane, float* acc_out, int32_t* wsum_out,
                               uint8_t* state, int64_t* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  CloseGrid g;
  ClosePlane pl;
  CPPF_CHECK_ARG(close_grid(h_origin, voxel, nx, ny, nz, &g));
  CPPF_CHECK_ARG(close_positive(trunc));
  CPPF_CHECK_ARG(min_weight >= 1);
  CPPF_CHECK_ARG(close_plane(h_plane, &pl));
  CPPF_CHECK_ARG(acc && wsum && acc_out && wsum_out && state && stats && workspace);
  const int64_t need = cppf_tsdf_close_workspace_bytes(nx, ny, nz);
  CPPF_CHECK_ARG(workspace_bytes >= need);
  const int64_t nodes = (int64_t)nx * ny * nz;
  const void* in[2] = {acc, wsum};
  const void* out[5] = {acc_out, wsum_out, state, stats, workspace};
  const int64_t out_bytes[5] = {4 * nodes, 4 * nodes, nodes, 4 * (int64_t)sizeof(int64_t), need};
  for (int o = 0; o < 5; ++o) {
    for (int q = 0; q < 2; ++q) CPPF_CHECK_ARG(close_disjoint(out[o], out_bytes[o], in[q], 4 * nodes));      // an output aliases an input
    for (int p = 0; p < o; ++p) CPPF_CHECK_ARG(close_disjoint(out[o], out_bytes[o], out[p], out_bytes[p]));  // two outputs overlap
  }
  hipStream_t st = (hipStream_t)stream;
  int* labels = (int*)workspace;
  unsigned long long* counts = (unsigned long long*)stats;
  const unsigned int nb = (unsigned int)((nodes + CLOSE_THREADS - 1) / CLOSE_THREADS);
  const unsigned int nbc = nb < CLOSE_MAX_BLOCKS ? nb : CLOSE_MAX_BLOCKS;      // the counting launches stride
  CPPF_HIP(hipMemsetAsync(stats, 0, 4 * sizeof(int64_t), st));
  hipLaunchKernelGGL(close_init_kernel, dim3(nbc), dim3(CLOSE_THREADS), 0, st, acc, wsum, g, trunc, min_weight, pl, nodes, acc_out,
                     wsum_out, state, labels, counts);
  CPPF_LAUNCH_CHECK();
  hipLaunchKernelGGL(close_merge_kernel, dim3(nb), dim3(CLOSE_THREADS), 0, st, g, nodes, (const uint8_t*)state, labels);
  CPPF_LAUNCH_CHECK();
  hipLaunchKernelGGL(close_flag_kernel, dim3(nb), dim3(CLOSE_THREADS), 0, st, g, nodes, labels, state);
  CPPF_LAUNCH_CHECK();
  hipLaunchKernelGGL(close_resolve_kernel, dim3(nbc), dim3(CLOSE_THREADS), 0, st, nodes, labels, acc_out, wsum_out, state, counts);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
