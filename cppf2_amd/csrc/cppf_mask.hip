// Detector masks (COCO run-length encoded detections of the BOP challenge's "default detections" files): decoding them on the
// device and cutting each down to its largest depth-connected component.  The reference uses a mask as given (eval.py:173-201)
// and has neither step; cppf2_amd/masks.py drives both entry points.  Integers only: no floating-point sum anywhere, so a
// mask's output bytes do not depend on the grid, the batch or the order.  gfx950 only.
//
// cppf_rle_decode: one launch, grid (ceil(groups / 256), D), 256 threads.  COCO's rule: the runs of a mask are column-major
//   (position p = c * H + r) and alternate 0s and 1s, starting with 0s (so a mask whose first pixel is set begins with a run of
//   length 0).  The output is row-major, so each lane owns 4 consecutive output pixels of the row-major image -- one aligned
//   32-bit vector store of mask bytes, cppf_gt_visibility's layout (the first and last group of a mask may be partial and are
//   stored byte by byte) -- and looks up the run of each of its pixels' positions.  The block scans the mask's runs into inclusive
//   prefix sums (the runs' end positions) in LDS, RLE_CHUNK runs at a time (8 per lane, the DPP wavefront scan, the 4
//   wavefronts' totals through LDS); a pixel whose position falls into the chunk's span [base, end) finds its run by binary
//   search for the first end position above it, and is 255 when that run's index is odd.  Most masks fit one chunk; one with
//   more runs goes through the same loop again with the running total as base (every block scans all runs of its mask: they
//   are few next to the pixels).  Positions past the last run's end are 0.  The sums are formed in uint32; the wrapper
//   (cppf2_amd/masks.py) rejects negative runs and runs that do not sum to H * W before any launch, and whatever the runs
//   hold every access stays inside the arrays: run_off is clamped to [0, total_runs] and every store is bounded by H * W.
//
// cppf_mask_components: the largest 4-connected component of each mask's valid pixels, five launches on the stream after the
//   stats and the arg-max words are cleared; grid (nbx <= 64, D), 256 threads, the nbx blocks of mask d stride over its pixels.
//     valid(i)      = mask[d][i] != 0 && depth > 0 && depth < +inf         (depth = depths[img_idx[d]][i]; NaN fails d > 0)
//     connected     = both valid, 4-neighbours, fabsf(d_a - d_b) <= jump   (one float32 subtraction: symmetric)
//     label         = the lowest flat index r * W + c of the component
//   1 init     label[i] = valid ? i : -1, size[i] = 0; stats[d][3] += #valid (ballots, one integer atomic per block)
//   2 merge    label-equivalence union-find (Komura; Playne and Hawick; Allegretti et al.'s "block-based union find"
//              without the blocks): each valid pixel unites itself with its right and its lower neighbour when connected.
//              find walks parents (always <= the index, so there are no cycles) with agent-scope loads, which bypass the
//              CU's L1; union lowers the larger root to the smaller with atomicMin and, when the word was no root any more,
//              goes on with what it held.  A link that an atomicMin replaces is re-established by that continuation, so at
//              the end of the launch the trees span exactly the components and every root is its component's lowest index
//              -- unique, whatever the schedule.  Each find also lowers its start to the root it found (one atomicMin),
//              which keeps the chains of long one-pixel-wide paths short.
//   3 compress label[i] = its root; size[root] += 1: lanes of a wavefront that share the first pending lane's root add once
//              (up to 4 rounds of ballots, then one atomic per remaining lane)
//   4 select   every root: stats[d][0] += 1; if size >= min_pixels, key = size << 32 | (0xFFFFFFFF - label) enters a 64-bit
//              atomicMax (wavefront, LDS, then one global atomic per block): the most pixels, ties to the lowest label --
//              cppf_grid_peaks' key
//   5 write    out[d][i] = label[i] == kept ? 255 : 0 in groups of 4 bytes as above; stats[d][1] = kept label or -1,
//              stats[d][2] = its pixels or 0
//   A mask whose img_idx lies outside [0, I) has no valid pixel: stats (0, -1, 0, 0), mask 0.
//
// cppf_mask_segments: the M largest components instead of the largest one (mask proposals: cppf2_amd/segment.py).  Launches 1-3
//   are cppf_mask_components' own kernels, unchanged; then
//   4 rank     M launches of one kernel: round k takes the 64-bit atomicMax of cc_select_kernel's key over the roots with
//              size >= min_pixels whose key lies below round k - 1's winner (round 0: all of them), into keys[d][k]: the
//              components by size, descending, ties to the lowest label.  Round 0 also counts stats[d][0] (components) and
//              stats[d][2] (components of at least min_pixels); a round whose predecessor found nothing returns at once.
//   5 mark     grid (1, D), 64 threads: seg[d][k] = (label, pixels, INT_MAX, INT_MAX, -1, -1) for a kept rank, six -1 for an
//              unused row; size[label] = -1 - k (the sizes are not needed any more: the word now maps a root to its rank);
//              stats[d][1] = kept ranks
//   6 write    rank[d][i] = the rank of label[i]'s component or 255, in groups of 4 bytes as above; the inclusive box of each
//              rank by integer atomicMin / atomicMax, first in LDS, then one set of global atomics per rank and block
//   The result is a pure function of the integer sizes and labels.  A mask whose img_idx lies outside [0, I): stats
//   (0, 0, 0, 0), rank 255, seg -1.
#include "cppf_common.h"
#include "cppf_cc.h"

#define MASK_THREADS 256
#define MASK_MAX_DIM 8192          // H, W: H * W <= 2^26 fits int32 with room for c * H + r
#define MASK_MAX_BLOCKS 64         // blocks per mask at most in the striding kernels
#define MASK_PX 4                  // consecutive pixels per lane: one 32-bit store of mask bytes
#define RLE_PER_LANE 8
#define RLE_CHUNK (MASK_THREADS * RLE_PER_LANE)        // runs per LDS pass (8 KiB of end positions)
#define CC_ROUNDS 4                // wavefront-shared size adds before the per-lane fallback
#define SEG_MAX 64                 // segments kept per mask at most (cppf_mask_segments)

__global__ __launch_bounds__(MASK_THREADS) void rle_decode_kernel(const int32_t* __restrict__ runs, int64_t total_runs,
                                                                  const int32_t* __restrict__ run_off, int H, int W,
                                                                  uint8_t* __restrict__ out) {
  __shared__ uint32_t s_end[RLE_CHUNK];
  __shared__ uint32_t s_w[MASK_THREADS / CPPF_WAVE];
  const int d = blockIdx.y;
  const int HW = H * W;
  int64_t a = run_off[d], b = run_off[d + 1];
  a = a < 0 ? 0 : (a > total_runs ? total_runs : a);
  b = b < a ? a : (b > total_runs ? total_runs : b);
  const int64_t n = b - a;                                // the same for the whole block
  const int32_t* rn = runs + a;
  uint8_t* mk = out + (int64_t)d * HW;
  // group q holds pixels 4q - m .. 4q - m + 3: m = the mask's misalignment, so that mk + 4q - m is 4-byte aligned
  const int m = (int)((uintptr_t)mk & 3);
  const int nq = (HW + m + MASK_PX - 1) / MASK_PX;
  const int q = blockIdx.x * MASK_THREADS + threadIdx.x;
  const int i0 = MASK_PX * q - m;
  const bool have = q < nq;
  uint32_t pos[MASK_PX];
  bool in[MASK_PX];
#pragma unroll
  for (int j = 0; j < MASK_PX; ++j) {
    const int i = i0 + j;
    in[j] = have && i >= 0 && i < HW;
    const int r = in[j] ? i / W : 0, c = in[j] ? i - r * W : 0;
    pos[j] = (uint32_t)(c * H + r);
  }
  const int lane = wave_lane(), w = threadIdx.x / CPPF_WAVE;
  uint32_t bytes = 0, base = 0;
  for (int64_t k0 = 0; k0 < n; k0 += RLE_CHUNK) {
    const int cnt = (int)(n - k0 < RLE_CHUNK ? n - k0 : RLE_CHUNK);
    uint32_t v[RLE_PER_LANE], sum = 0;
#pragma unroll
    for (int e = 0; e < RLE_PER_LANE; ++e) {
      const int t = threadIdx.x * RLE_PER_LANE + e;
      sum += t < cnt ? (uint32_t)rn[k0 + t] : 0u;
      v[e] = sum;
    }
    const uint32_t incl = wave_inclusive_scan_u32(sum);
    __syncthreads();                                      // the last chunk's searches are done with s_end and s_w
    if (lane == CPPF_WAVE - 1) s_w[w] = incl;
    __syncthreads();
    uint32_t before = base + incl - sum;
#pragma unroll
    for (int k = 0; k < MASK_THREADS / CPPF_WAVE; ++k) before += k < w ? s_w[k] : 0u;
#pragma unroll
    for (int e = 0; e < RLE_PER_LANE; ++e) s_end[threadIdx.x * RLE_PER_LANE + e] = before + v[e];
    __syncthreads();
    const uint32_t end = s_end[cnt - 1];
#pragma unroll
    for (int j = 0; j < MASK_PX; ++j) {
      if (in[j] && pos[j] >= base && pos[j] < end) {
        int lo = 0, hi = cnt - 1;                         // the first t with s_end[t] > pos: it exists (s_end[cnt - 1] = end)
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_end[mid] > pos[j]) hi = mid; else lo = mid + 1;
        }
        if ((k0 + lo) & 1) bytes |= 0xffu << (8 * j);
      }
    }
    base = end;
  }
  if (have) {
    if (in[0] && in[MASK_PX - 1]) {
      *reinterpret_cast<uint32_t*>(mk + i0) = bytes;
    } else {
#pragma unroll
      for (int j = 0; j < MASK_PX; ++j)
        if (in[j]) mk[i0 + j] = (uint8_t)(bytes >> (8 * j));
    }
  }
}

// ---- components ------------------------------------------------------------------------------------------------------------
// cc_load, cc_find, cc_union: cppf_cc.h (shared with cppf_close.hip)
__global__ __launch_bounds__(MASK_THREADS) void cc_init_kernel(const uint8_t* __restrict__ masks, const float* __restrict__ depths,
                                                               int I, const int32_t* __restrict__ img_idx, int HW,
                                                               int* __restrict__ labels, int* __restrict__ sizes,
                                                               int* __restrict__ stats) {
  __shared__ uint32_t s_c[MASK_THREADS / CPPF_WAVE];
  const int d = blockIdx.y;
  const int ti = img_idx[d];
  const bool ok = ti >= 0 && ti < I;                      // the same for the whole block
  const uint8_t* mk = masks + (int64_t)d * HW;
  const float* dp = depths + (int64_t)(ok ? ti : 0) * HW;
  int* L = labels + (int64_t)d * HW;
  int* S = sizes + (int64_t)d * HW;
  uint32_t mine = 0;
  for (int i0 = blockIdx.x * MASK_THREADS; i0 < HW; i0 += gridDim.x * MASK_THREADS) {
    const int i = i0 + threadIdx.x;
    bool valid = false;
    if (i < HW) {
      const float z = ok ? dp[i] : 0.0f;
      valid = mk[i] != 0 && z > 0.0f && z < __builtin_inff();
      L[i] = valid ? i : -1;
      S[i] = 0;
    }
    mine += (uint32_t)__popcll(wave_ballot(valid));       // every lane of the wavefront holds the wavefront's count
  }
  if (wave_lane() == 0) s_c[threadIdx.x / CPPF_WAVE] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < MASK_THREADS / CPPF_WAVE; ++k) s += s_c[k];
    if (s) atomicAdd(&stats[4 * d + 3], (int)s);
  }
}

__global__ __launch_bounds__(MASK_THREADS) void cc_merge_kernel(const float* __restrict__ depths, int I,
                                                                const int32_t* __restrict__ img_idx, int H, int W, float jump,
                                                                int* __restrict__ labels) {
  const int d = blockIdx.y;
  const int ti = img_idx[d];
  if (ti < 0 || ti >= I) return;                          // the same for the whole block: no valid pixel
  const int HW = H * W;
  const float* dp = depths + (int64_t)ti * HW;
  int* L = labels + (int64_t)d * HW;
  for (int i = blockIdx.x * MASK_THREADS + threadIdx.x; i < HW; i += gridDim.x * MASK_THREADS) {
    if (cc_load(L + i) < 0) continue;                     // (a word's sign never changes after the init launch)
    const int r = i / W, c = i - r * W;
    const float z = dp[i];
    if (c + 1 < W && cc_load(L + i + 1) >= 0 && fabsf(z - dp[i + 1]) <= jump) cc_union(L, i, i + 1);
    if (r + 1 < H && cc_load(L + i + W) >= 0 && fabsf(z - dp[i + W]) <= jump) cc_union(L, i, i + W);
  }
}

__global__ __launch_bounds__(MASK_THREADS) void cc_compress_kernel(int HW, int* __restrict__ labels, int* __restrict__ sizes) {
  const int d = blockIdx.y;
  int* L = labels + (int64_t)d * HW;
  int* S = sizes + (int64_t)d * HW;
  const int lane = wave_lane();
  for (int i0 = blockIdx.x * MASK_THREADS; i0 < HW; i0 += gridDim.x * MASK_THREADS) {
    const int i = i0 + threadIdx.x;
    int root = -1;
    if (i < HW) {
      root = cc_load(L + i);
      if (root >= 0) {
        int p;
        while ((p = cc_load(L + root)) != root) root = p;   // (other lanes store roots meanwhile: every value read is an ancestor)
        __hip_atomic_store(L + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    bool pending = root >= 0;
#pragma unroll
    for (int k = 0; k < CC_ROUNDS; ++k) {
      const unsigned long long todo = wave_ballot(pending);
      if (!todo) break;                                   // uniform
      const int leader = __ffsll((long long)todo) - 1;
      const int lr = __shfl(root, leader);
      const bool same = pending && root == lr;
      const unsigned long long grp = wave_ballot(same);
      if (lane == leader) atomicAdd(S + lr, (int)__popcll(grp));
      pending = pending && !same;
    }
    if (pending) atomicAdd(S + root, 1);
  }
}

__global__ __launch_bounds__(MASK_THREADS) void cc_select_kernel(int HW, int min_pixels, const int* __restrict__ labels,
                                                                 const int* __restrict__ sizes, int* __restrict__ stats,
                                                                 unsigned long long* __restrict__ best) {
  __shared__ uint32_t s_c[MASK_THREADS / CPPF_WAVE];
  __shared__ unsigned long long s_best;
  const int d = blockIdx.y;
  const int* L = labels + (int64_t)d * HW;
  const int* S = sizes + (int64_t)d * HW;
  if (threadIdx.x == 0) s_best = 0;
  __syncthreads();
  uint32_t mine = 0;
  unsigned long long key = 0;
  for (int i0 = blockIdx.x * MASK_THREADS; i0 < HW; i0 += gridDim.x * MASK_THREADS) {
    const int i = i0 + threadIdx.x;
    const bool root = i < HW && L[i] == i;
    if (root) {
      const int s = S[i];
      if (s >= min_pixels) {
        const unsigned long long k = ((unsigned long long)(uint32_t)s << 32) | (0xFFFFFFFFu - (uint32_t)i);
        key = k > key ? k : key;
      }
    }
    mine += (uint32_t)__popcll(wave_ballot(root));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off);
    key = o > key ? o : key;
  }
  if (wave_lane() == 0) {
    s_c[threadIdx.x / CPPF_WAVE] = mine;
    if (key) atomicMax(&s_best, key);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < MASK_THREADS / CPPF_WAVE; ++k) s += s_c[k];
    if (s) atomicAdd(&stats[4 * d], (int)s);
    if (s_best) atomicMax(&best[d], s_best);
  }
}

__global__ __launch_bounds__(MASK_THREADS) void cc_write_kernel(int HW, const int* __restrict__ labels,
                                                                const unsigned long long* __restrict__ best,
                                                                int* __restrict__ stats, uint8_t* __restrict__ out) {
  const int d = blockIdx.y;
  const int* L = labels + (int64_t)d * HW;
  const unsigned long long key = best[d];
  const int kept = key ? (int)(0xFFFFFFFFu - (uint32_t)key) : -1;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    stats[4 * d + 1] = kept;
    stats[4 * d + 2] = (int)(key >> 32);
  }
  uint8_t* mk = out + (int64_t)d * HW;
  const int m = (int)((uintptr_t)mk & 3);                 // groups as in rle_decode_kernel
  const int nq = (HW + m + MASK_PX - 1) / MASK_PX;
  for (int q = blockIdx.x * MASK_THREADS + threadIdx.x; q < nq; q += gridDim.x * MASK_THREADS) {
    const int i0 = MASK_PX * q - m;
    uint32_t bytes = 0;
#pragma unroll
    for (int j = 0; j < MASK_PX; ++j) {
      const int i = i0 + j;
      if (i >= 0 && i < HW && kept >= 0 && L[i] == kept) bytes |= 0xffu << (8 * j);
    }
    if (i0 >= 0 && i0 + MASK_PX - 1 < HW) {
      *reinterpret_cast<uint32_t*>(mk + i0) = bytes;
    } else {
#pragma unroll
      for (int j = 0; j < MASK_PX; ++j)
        if (i0 + j >= 0 && i0 + j < HW) mk[i0 + j] = (uint8_t)(bytes >> (8 * j));
    }
  }
}

// ---- segments: the M largest components ----------------------------------------------------------------------------------
__global__ __launch_bounds__(MASK_THREADS) void cc_rank_kernel(int HW, int min_pixels, int M, int round, const int* __restrict__ labels,
                                                               const int* __restrict__ sizes, int* __restrict__ stats,
                                                               unsigned long long* __restrict__ keys) {
  __shared__ uint32_t s_c[MASK_THREADS / CPPF_WAVE], s_b[MASK_THREADS / CPPF_WAVE];
  __shared__ unsigned long long s_best;
  const int d = blockIdx.y;
  const unsigned long long bound = round ? keys[(int64_t)d * M + round - 1] : ~0ull;     // the same for the whole block
  if (bound == 0) return;                                 // the round before found nothing (keys[d][round] stays 0)
  const int* L = labels + (int64_t)d * HW;
  const int* S = sizes + (int64_t)d * HW;
  if (threadIdx.x == 0) s_best = 0;
  __syncthreads();
  uint32_t roots = 0, big = 0;
  unsigned long long key = 0;
  for (int i0 = blockIdx.x * MASK_THREADS; i0 < HW; i0 += gridDim.x * MASK_THREADS) {
    const int i = i0 + threadIdx.x;
    const bool root = i < HW && L[i] == i;
    bool enough = false;
    if (root) {
      const int s = S[i];
      enough = s >= min_pixels;
      if (enough) {
        const unsigned long long k = ((unsigned long long)(uint32_t)s << 32) | (0xFFFFFFFFu - (uint32_t)i);
        key = k < bound && k > key ? k : key;
      }
    }
    roots += (uint32_t)__popcll(wave_ballot(root));
    big += (uint32_t)__popcll(wave_ballot(enough));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off);
    key = o > key ? o : key;
  }
  if (wave_lane() == 0) {
    s_c[threadIdx.x / CPPF_WAVE] = roots;
    s_b[threadIdx.x / CPPF_WAVE] = big;
    if (key) atomicMax(&s_best, key);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (round == 0) {
      uint32_t s = 0, b = 0;
#pragma unroll
      for (int k = 0; k < MASK_THREADS / CPPF_WAVE; ++k) { s += s_c[k]; b += s_b[k]; }
      if (s) atomicAdd(&stats[4 * d], (int)s);
      if (b) atomicAdd(&stats[4 * d + 2], (int)b);
    }
    if (s_best) atomicMax(&keys[(int64_t)d * M + round], s_best);
  }
}

__global__ __launch_bounds__(CPPF_WAVE) void cc_mark_kernel(int HW, int M, const unsigned long long* __restrict__ keys,
                                                            int* __restrict__ sizes, int* __restrict__ seg, int* __restrict__ stats) {
  const int d = blockIdx.x, k = threadIdx.x;
  const unsigned long long key = k < M ? keys[(int64_t)d * M + k] : 0ull;
  if (k < M) {
    int* row = seg + ((int64_t)d * M + k) * 6;
    if (key) {
      const int label = (int)(0xFFFFFFFFu - (uint32_t)key);
      row[0] = label; row[1] = (int)(key >> 32);
      row[2] = 0x7fffffff; row[3] = 0x7fffffff; row[4] = -1; row[5] = -1;
      sizes[(int64_t)d * HW + label] = -1 - k;
    } else {
#pragma unroll
      for (int j = 0; j < 6; ++j) row[j] = -1;
    }
  }
  const int kept = (int)__popcll(wave_ballot(key != 0));
  if (k == 0) stats[4 * d + 1] = kept;
}

__global__ __launch_bounds__(MASK_THREADS) void cc_rank_write_kernel(int W, int HW, int M, const int* __restrict__ labels,
                                                                     const int* __restrict__ sizes, int* __restrict__ seg,
                                                                     uint8_t* __restrict__ out) {
  __shared__ int s_box[SEG_MAX][4];
  const int d = blockIdx.y;
  const int* L = labels + (int64_t)d * HW;
  const int* S = sizes + (int64_t)d * HW;
  if (threadIdx.x < SEG_MAX) {
    s_box[threadIdx.x][0] = 0x7fffffff; s_box[threadIdx.x][1] = 0x7fffffff;
    s_box[threadIdx.x][2] = -1; s_box[threadIdx.x][3] = -1;
  }
  __syncthreads();
  uint8_t* mk = out + (int64_t)d * HW;
  const int m = (int)((uintptr_t)mk & 3);                 // groups as in rle_decode_kernel
  const int nq = (HW + m + MASK_PX - 1) / MASK_PX;
  for (int q = blockIdx.x * MASK_THREADS + threadIdx.x; q < nq; q += gridDim.x * MASK_THREADS) {
    const int i0 = MASK_PX * q - m;
    uint32_t bytes = 0;
#pragma unroll
    for (int j = 0; j < MASK_PX; ++j) {
      const int i = i0 + j;
      int rank = 255;
      if (i >= 0 && i < HW) {
        const int l = L[i];
        const int s = l >= 0 ? S[l] : 0;                  // a kept root's word is -1 - rank, every other root's its size >= 1
        if (s < 0 && -1 - s < M) {                        // (-1 - s < M always holds: the mark launch wrote it)
          rank = -1 - s;
          const int r = i / W, c = i - r * W;
          atomicMin(&s_box[rank][0], c); atomicMin(&s_box[rank][1], r);
          atomicMax(&s_box[rank][2], c); atomicMax(&s_box[rank][3], r);
        }
      }
      bytes |= (uint32_t)rank << (8 * j);
    }
    if (i0 >= 0 && i0 + MASK_PX - 1 < HW) {
      *reinterpret_cast<uint32_t*>(mk + i0) = bytes;
    } else {
#pragma unroll
      for (int j = 0; j < MASK_PX; ++j)
        if (i0 + j >= 0 && i0 + j < HW) mk[i0 + j] = (uint8_t)(bytes >> (8 * j));
    }
  }
  __syncthreads();
  if (threadIdx.x < M && s_box[threadIdx.x][2] >= 0) {
    int* row = seg + ((int64_t)d * M + threadIdx.x) * 6;
    atomicMin(row + 2, s_box[threadIdx.x][0]); atomicMin(row + 3, s_box[threadIdx.x][1]);
    atomicMax(row + 4, s_box[threadIdx.x][2]); atomicMax(row + 5, s_box[threadIdx.x][3]);
  }
}

static int64_t cc_best_bytes(int D) { return ((int64_t)D * 8 + 255) / 256 * 256; }

extern "C" int64_t cppf_mask_components_workspace_bytes(int D, int H, int W) {
  if (D <= 0 || H <= 0 || W <= 0 || D > 65535 || H > MASK_MAX_DIM || W > MASK_MAX_DIM) return 0;
  return cc_best_bytes(D) + (int64_t)D * H * W * 2 * (int64_t)sizeof(int32_t);
}

extern "C" int cppf_rle_decode(int D, int H, int W, const int32_t* runs, int64_t total_runs, const int32_t* run_off, uint8_t* out,
                               void* stream) {
  CPPF_CHECK_ARG(D >= 0 && D <= 65535);
  CPPF_CHECK_ARG(H >= 1 && W >= 1 && H <= MASK_MAX_DIM && W <= MASK_MAX_DIM);
  CPPF_CHECK_ARG(total_runs >= 0 && total_runs <= 0x7fffffff);
  if (D == 0) return CPPF_OK;
  CPPF_CHECK_ARG(run_off && out && (runs || total_runs == 0));
  const int nq = H * W / MASK_PX + 2;                     // groups of a mask, misaligned start and partial end included
  hipLaunchKernelGGL(rle_decode_kernel, dim3((nq + MASK_THREADS - 1) / MASK_THREADS, D), dim3(MASK_THREADS), 0,
                     (hipStream_t)stream, runs, total_runs, run_off, H, W, out);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}

extern "C" int cppf_mask_components(int D, int I, int H, int W, const uint8_t* masks, const float* depths, const int32_t* img_idx,
                                    float jump, int min_pixels, uint8_t* out_mask, int32_t* stats, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  CPPF_CHECK_ARG(D >= 0 && D <= 65535);
  CPPF_CHECK_ARG(I >= 1 && H >= 1 && W >= 1 && H <= MASK_MAX_DIM && W <= MASK_MAX_DIM);
  CPPF_CHECK_ARG(jump >= 0.0f && jump < __builtin_inff());
  CPPF_CHECK_ARG(min_pixels >= 0);
  if (D == 0) return CPPF_OK;
  CPPF_CHECK_ARG(masks && depths && img_idx && out_mask && stats);
  CPPF_CHECK_ARG(workspace && (uintptr_t)workspace % 8 == 0);
  CPPF_CHECK_ARG(workspace_bytes >= cppf_mask_components_workspace_bytes(D, H, W));
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W;
  unsigned long long* best = (unsigned long long*)workspace;
  int* labels = (int*)((char*)workspace + cc_best_bytes(D));
  int* sizes = labels + (int64_t)D * HW;
  CPPF_HIP(hipMemsetAsync(best, 0, (size_t)cc_best_bytes(D), st));
  CPPF_HIP(hipMemsetAsync(stats, 0, (size_t)D * 4 * sizeof(int32_t), st));
  const int blocks = (HW + MASK_THREADS - 1) / MASK_THREADS;
  const dim3 grid(blocks < MASK_MAX_BLOCKS ? blocks : MASK_MAX_BLOCKS, D), block(MASK_THREADS);
  hipLaunchKernelGGL(cc_init_kernel, grid, block, 0, st, masks, depths, I, img_idx, HW, labels, sizes, (int*)stats);
  hipLaunchKernelGGL(cc_merge_kernel, grid, block, 0, st, depths, I, img_idx, H, W, jump, labels);
  hipLaunchKernelGGL(cc_compress_kernel, grid, block, 0, st, HW, labels, sizes);
  hipLaunchKernelGGL(cc_select_kernel, grid, block, 0, st, HW, min_pixels, (const int*)labels, (const int*)sizes, (int*)stats, best);
  hipLaunchKernelGGL(cc_write_kernel, grid, block, 0, st, HW, (const int*)labels, (const unsigned long long*)best, (int*)stats,
                     out_mask);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}

static int64_t cc_keys_bytes(int D, int M) { return ((int64_t)D * M * 8 + 255) / 256 * 256; }

extern "C" int64_t cppf_mask_segments_workspace_bytes(int D, int H, int W, int max_segments) {
  if (D <= 0 || H <= 0 || W <= 0 || D > 65535 || H > MASK_MAX_DIM || W > MASK_MAX_DIM) return 0;
  if (max_segments < 1 || max_segments > SEG_MAX) return 0;
  return cc_keys_bytes(D, max_segments) + (int64_t)D * H * W * 2 * (int64_t)sizeof(int32_t);
}

extern "C" int cppf_mask_segments(int D, int I, int H, int W, const uint8_t* masks, const float* depths, const int32_t* img_idx,
                                  float jump, int min_pixels, int max_segments, uint8_t* out_rank, int32_t* seg, int32_t* stats,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  CPPF_CHECK_ARG(D >= 0 && D <= 65535);
  CPPF_CHECK_ARG(I >= 1 && H >= 1 && W >= 1 && H <= MASK_MAX_DIM && W <= MASK_MAX_DIM);
  CPPF_CHECK_ARG(jump >= 0.0f && jump < __builtin_inff());
  CPPF_CHECK_ARG(min_pixels >= 0);
  CPPF_CHECK_ARG(max_segments >= 1 && max_segments <= SEG_MAX);
  if (D == 0) return CPPF_OK;
  CPPF_CHECK_ARG(masks && depths && img_idx && out_rank && seg && stats);
  CPPF_CHECK_ARG(workspace && (uintptr_t)workspace % 8 == 0);
  CPPF_CHECK_ARG(workspace_bytes >= cppf_mask_segments_workspace_bytes(D, H, W, max_segments));
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W, M = max_segments;
  unsigned long long* keys = (unsigned long long*)workspace;
  int* labels = (int*)((char*)workspace + cc_keys_bytes(D, M));
  int* sizes = labels + (int64_t)D * HW;
  CPPF_HIP(hipMemsetAsync(keys, 0, (size_t)cc_keys_bytes(D, M), st));
  CPPF_HIP(hipMemsetAsync(stats, 0, (size_t)D * 4 * sizeof(int32_t), st));
  const int blocks = (HW + MASK_THREADS - 1) / MASK_THREADS;
  const dim3 grid(blocks < MASK_MAX_BLOCKS ? blocks : MASK_MAX_BLOCKS, D), block(MASK_THREADS);
  hipLaunchKernelGGL(cc_init_kernel, grid, block, 0, st, masks, depths, I, img_idx, HW, labels, sizes, (int*)stats);
  hipLaunchKernelGGL(cc_merge_kernel, grid, block, 0, st, depths, I, img_idx, H, W, jump, labels);
  hipLaunchKernelGGL(cc_compress_kernel, grid, block, 0, st, HW, labels, sizes);
  for (int k = 0; k < M; ++k)
    hipLaunchKernelGGL(cc_rank_kernel, grid, block, 0, st, HW, min_pixels, M, k, (const int*)labels, (const int*)sizes, (int*)stats,
                       keys);
  hipLaunchKernelGGL(cc_mark_kernel, dim3(D), dim3(CPPF_WAVE), 0, st, HW, M, (const unsigned long long*)keys, sizes, (int*)seg,
                     (int*)stats);
  hipLaunchKernelGGL(cc_rank_write_kernel, grid, block, 0, st, W, HW, M, (const int*)labels, (const int*)sizes, (int*)seg, out_rank);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
