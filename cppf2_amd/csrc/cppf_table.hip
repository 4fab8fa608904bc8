// cppf_table.hip -- pair-feature tables: the bins of a tuple looked up from its point-pair feature instead of drawn from an MLP's
// logits.  cppf_pair_keys builds a table's keys and payload, cppf_pair_table_draw fills pipe.bins from one.
// gfx950 only.  See include/cppf_hip.h for the contract of each entry point; pair_key() lives in cppf_common.h.
#include "cppf_common.h"

#define TAB_BLOCK 256
#define TAB_HIT_SCENES 8        // scenes of one workgroup whose hit counts are summed in LDS (tuples of further scenes: one atomic each)

// largest b with off[b] <= row (cppf_core.hip's find_scene)
__device__ __forceinline__ int table_scene(const int32_t* __restrict__ off, int B, int64_t row) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)off[mid] <= row) lo = mid; else hi = mid;
  }
  return lo;
}

// one coordinate of the payload: the bin decode_targets_kernel maps back to bin / (nb - 1) - 0.5
__device__ __forceinline__ uint32_t canon_bin(float x, float nbm1) {
  return (uint32_t)(int)floorf((fminf(fmaxf(x, -0.5f), 0.5f) + 0.5f) * nbm1 + 0.5f);
}

__global__ __launch_bounds__(TAB_BLOCK) void pair_keys_kernel(int B, const float* __restrict__ pts, const float* __restrict__ normals,
                                                              const float* __restrict__ canon, const int32_t* __restrict__ idx, int k,
                                                              const int32_t* __restrict__ pt_off, const int32_t* __restrict__ tup_off,
                                                              int64_t total, int nd, float d_step, int na,
                                                              const float* __restrict__ edges, int nb, int32_t* __restrict__ keys,
                                                              uint2* __restrict__ payload) {
  const int64_t t = (int64_t)blockIdx.x * TAB_BLOCK + threadIdx.x;
  if (t >= total) return;
  const int b = table_scene(tup_off, B, t);
  const int64_t p0 = pt_off[b];
  const int64_t i0 = p0 + idx[t * k + 0], i1 = p0 + idx[t * k + 1];
  const PairKey pk = pair_key(pts + 3 * i0, pts + 3 * i1, normals + 3 * i0, normals + 3 * i1, nd, d_step, na, edges);
  keys[t] = pk.key;
  if (payload) {
    const float nbm1 = (float)(nb - 1);
    const float* ca = canon + 3 * i0;
    const float* cb = canon + 3 * i1;
    uint2 e;
    e.x = canon_bin(ca[0], nbm1) | (canon_bin(ca[1], nbm1) << 8) | (canon_bin(ca[2], nbm1) << 16) | (canon_bin(cb[0], nbm1) << 24);
    e.y = canon_bin(cb[1], nbm1) | (canon_bin(cb[2], nbm1) << 8);
    payload[t] = e;
  }
}

// One thread per tuple; a latency-bound chain of dependent gathers (tuple row -> two points and normals -> the cell's range ->
// one entry), so the kernel keeps its registers few (no arrays, no double) and lets the occupancy hide the chain.  The 24-byte
// bin rows of a workgroup are contiguous: staged in LDS and written as consecutive words.  Hit counts: summed per wavefront
// (ballot), then per workgroup in LDS, then one integer atomic per (scene, source) with a non-zero count.
__global__ __launch_bounds__(TAB_BLOCK) void pair_table_draw_kernel(int B, const float* __restrict__ pts, const float* __restrict__ normals,
                                                                    const int32_t* __restrict__ idx, int k,
                                                                    const int32_t* __restrict__ pt_off,
                                                                    const int32_t* __restrict__ tup_off, int64_t total, int nd,
                                                                    float d_step, int na, const float* __restrict__ edges,
                                                                    const int32_t* __restrict__ cell_off,
                                                                    const uint2* __restrict__ entries, int E,
                                                                    const float* __restrict__ uniforms, int32_t* __restrict__ bins,
                                                                    int32_t* __restrict__ hits) {
  __shared__ int32_t s_bins[TAB_BLOCK * 6];
  __shared__ int s_hits[TAB_HIT_SCENES * 3];
  const int64_t tbase = (int64_t)blockIdx.x * TAB_BLOCK;
  const int64_t t = tbase + threadIdx.x;
  const bool live = t < total;
  if (threadIdx.x < TAB_HIT_SCENES * 3) s_hits[threadIdx.x] = 0;
  __syncthreads();
  const int b_first = table_scene(tup_off, B, tbase);
  int b = b_first, source = 2;
  if (live) {
    b = table_scene(tup_off, B, t);
    const float u0 = uniforms[t * 6];
    const int64_t p0 = pt_off[b];
    const int64_t i0 = p0 + idx[t * k + 0], i1 = p0 + idx[t * k + 1];
    const PairKey pk = pair_key(pts + 3 * i0, pts + 3 * i1, normals + 3 * i0, normals + 3 * i1, nd, d_step, na, edges);
    int start = 0, n = E;
    if (pk.key >= 0) {
      const int s0 = cell_off[pk.key], s1 = cell_off[pk.key + 1];
      if (s1 > s0) {
        start = s0; n = s1 - s0; source = 0;
      } else {
        // the first non-empty cell among bd-1, bd+1, a1-1, a1+1, a2-1, a2+1, a3-1, a3+1
        const int na2 = na * na;
        for (int j = 0; j < 8 && source == 2; ++j) {
          const int c = j >> 1, dir = (j & 1) ? 1 : -1;
          const int v = (c == 0 ? pk.bd : c == 1 ? pk.a1 : c == 2 ? pk.a2 : pk.a3) + dir;
          if (v < 0 || v >= (c == 0 ? nd : na)) continue;
          const int nk = pk.key + dir * (c == 0 ? na2 * na : c == 1 ? na2 : c == 2 ? na : 1);
          const int n0 = cell_off[nk], n1 = cell_off[nk + 1];
          if (n1 > n0) { start = n0; n = n1 - n0; source = 1; }
        }
      }
    }
    const int pick = max(min((int)(u0 * (float)n), n - 1), 0);      // (u0 is in [0, 1): the lower clamp only keeps a bad one in range)
    const uint2 e = entries[start + pick];
    int32_t* row = s_bins + threadIdx.x * 6;
    row[0] = (int32_t)(e.x & 255u); row[1] = (int32_t)((e.x >> 8) & 255u); row[2] = (int32_t)((e.x >> 16) & 255u);
    row[3] = (int32_t)(e.x >> 24); row[4] = (int32_t)(e.y & 255u); row[5] = (int32_t)((e.y >> 8) & 255u);
  }
  // hit counts of this wavefront: one LDS add per source when all its tuples belong to one scene (the usual case)
  {
    const int bw = __builtin_amdgcn_readfirstlane(b);
    const bool one_scene = wave_ballot(live && b != bw) == 0ull && bw - b_first < TAB_HIT_SCENES;
    if (one_scene) {
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int cnt = __popcll(wave_ballot(live && source == s));
        if (wave_lane() == 0 && cnt) atomicAdd(&s_hits[(bw - b_first) * 3 + s], cnt);
      }
    } else if (live) {
      if (b - b_first < TAB_HIT_SCENES) atomicAdd(&s_hits[(b - b_first) * 3 + source], 1);
      else atomicAdd(&hits[b * 3 + source], 1);
    }
  }
  __syncthreads();
  if (threadIdx.x < TAB_HIT_SCENES * 3) {
    const int cnt = s_hits[threadIdx.x];
    const int bb = b_first + threadIdx.x / 3;
    if (cnt && bb < B) atomicAdd(&hits[bb * 3 + threadIdx.x % 3], cnt);
  }
  const int64_t words = (total - tbase < TAB_BLOCK ? total - tbase : TAB_BLOCK) * 6;
  int32_t* out = bins + tbase * 6;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int w = j * TAB_BLOCK + threadIdx.x;
    if (w < words) out[w] = s_bins[w];
  }
}

static int table_geometry_ok(int nd, float d_step, int na) {
  if (!(nd >= 1 && na >= 2 && na <= 1024 && d_step > 0.0f && d_step <= 3.0e38f)) return 0;
  return (int64_t)nd * na * na * na < (int64_t)INT32_MAX;
}

extern "C" int cppf_pair_keys(int B, const float* pts, const float* normals, const float* canon, const int32_t* idx, int k,
                              const int32_t* pt_off, const int32_t* tup_off, int64_t total_tuples, int nd, float d_step, int na,
                              const float* edges, int nb, int32_t* keys_out, uint8_t* payload_out, void* stream) {
  CPPF_CHECK_ARG(B > 0 && pts && normals && idx && pt_off && tup_off && edges && keys_out);
  CPPF_CHECK_ARG(k >= 2 && k <= 8);
  CPPF_CHECK_ARG(table_geometry_ok(nd, d_step, na));
  CPPF_CHECK_ARG((canon == nullptr) == (payload_out == nullptr));
  CPPF_CHECK_ARG(canon == nullptr || (nb >= 2 && nb <= 256));
  CPPF_CHECK_ARG(((uintptr_t)payload_out & 7) == 0);
  if (total_tuples <= 0) return CPPF_OK;
  hipLaunchKernelGGL(pair_keys_kernel, dim3((unsigned)((total_tuples + TAB_BLOCK - 1) / TAB_BLOCK)), dim3(TAB_BLOCK), 0,
                     (hipStream_t)stream, B, pts, normals, canon, idx, k, pt_off, tup_off, total_tuples, nd, d_step, na, edges, nb,
                     keys_out, reinterpret_cast<uint2*>(payload_out));
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}

extern "C" int cppf_pair_table_draw(int B, const float* pts, const float* normals, const int32_t* idx, int k, const int32_t* pt_off,
                                    const int32_t* tup_off, int64_t total_tuples, int nd, float d_step, int na, const float* edges,
                                    const int32_t* cell_off, const uint8_t* entries, int64_t E, const float* uniforms,
                                    int32_t* bins_out, int32_t* hits, void* stream) {
  CPPF_CHECK_ARG(B > 0 && pts && normals && idx && pt_off && tup_off && edges && cell_off && entries && uniforms && bins_out && hits);
  CPPF_CHECK_ARG(k >= 2 && k <= 8);
  CPPF_CHECK_ARG(table_geometry_ok(nd, d_step, na));
  CPPF_CHECK_ARG(E > 0 && E <= (int64_t)INT32_MAX);
  CPPF_CHECK_ARG(((uintptr_t)entries & 7) == 0);
  if (total_tuples <= 0) return CPPF_OK;
  hipLaunchKernelGGL(pair_table_draw_kernel, dim3((unsigned)((total_tuples + TAB_BLOCK - 1) / TAB_BLOCK)), dim3(TAB_BLOCK), 0,
                     (hipStream_t)stream, B, pts, normals, idx, k, pt_off, tup_off, total_tuples, nd, d_step, na, edges, cell_off,
                     reinterpret_cast<const uint2*>(entries), (int)E, uniforms, bins_out, hits);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
