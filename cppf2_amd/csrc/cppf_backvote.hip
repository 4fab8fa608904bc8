// cppf_backvote.hip -- back-vote filter, pose assembly with the scale median (both on the radix select below), kept-row
// lists.  gfx950 only.  See include/cppf_hip.h for the contract of each entry point.
#include "cppf_common.h"

// =============================================================================================
// a7. back-vote filter + importance weights (eval.py:251-275).  One workgroup per scene (BV_THREADS threads: cppf_common.h).
// =============================================================================================

// k-th smallest (0-based) of n uint32 keys by 3-pass (11/11/10 bit) radix select; key(i) yields the i-th key.
// Returns the key; *n_le = number of keys <= it.  Whole workgroup must call it (blockDim.x multiple of 64).
template <typename KeyFn>
__device__ uint32_t radix_select_keys(KeyFn key, int n, int kth, uint32_t* s_hist /*[2048]*/, int* s_misc /*[4]*/,
                                      int* n_le) {
  uint32_t prefix = 0;      // bits fixed so far
  int remaining = kth;      // rank inside the current candidate set
  int below = 0;            // keys strictly below the candidate set
  const int shifts[3] = {21, 10, 0};
  const int widths[3] = {11, 11, 10};
  uint32_t mask_fixed = 0;
  for (int pass = 0; pass < 3; ++pass) {
    const int sh = shifts[pass], nbins = 1 << widths[pass];
    for (int i = threadIdx.x; i < nbins; i += blockDim.x) s_hist[i] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const uint32_t bits = key(i);
      if ((bits & mask_fixed) == prefix) atomicAdd(&s_hist[(bits >> sh) & (nbins - 1)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 64) {
      // 64 lanes x (nbins/64) consecutive bins
      const int per = nbins / 64;
      uint32_t sum = 0;
      for (int j = 0; j < per; ++j) sum += s_hist[threadIdx.x * per + j];
      uint32_t incl = sum;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off);
        if ((int)threadIdx.x >= off) incl += o;
      }
      const uint32_t excl = incl - sum;
      if ((uint32_t)remaining >= excl && (uint32_t)remaining < incl) {
        uint32_t run = excl;
        for (int j = 0; j < per; ++j) {
          const uint32_t c = s_hist[threadIdx.x * per + j];
          if ((uint32_t)remaining < run + c) {
            s_misc[0] = threadIdx.x * per + j;   // chosen bin
            s_misc[1] = (int)run;                // keys of the candidate set below the chosen bin
            s_misc[2] = (int)c;                  // keys in the chosen bin
            break;
          }
          run += c;
        }
      }
    }
    __syncthreads();
    const int bin = s_misc[0];
    below += s_misc[1];
    remaining -= s_misc[1];
    prefix |= ((uint32_t)bin) << sh;
    mask_fixed |= ((uint32_t)(nbins - 1)) << sh;
    if (pass == 2) *n_le = below + s_misc[2];
    __syncthreads();
  }
  return prefix;
}

// non-negative floats: bit order == value order, NaN last
__device__ uint32_t radix_select(const float* __restrict__ v, int n, int kth, uint32_t* s_hist, int* s_misc,
                                 int* n_le) {
  return radix_select_keys([v](int i) { return __float_as_uint(v[i]); }, n, kth, s_hist, s_misc, n_le);
}

// order-preserving map float -> uint32 (negative values included)
__device__ __forceinline__ uint32_t float_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// 1. back-projected vote parameters of the real pairs w.r.t. the voted centre (eval.py:252-257): throughput work, so it
// runs as its own grid over the pairs instead of on the one CU that owns the scene's order statistics
__global__ __launch_bounds__(256) void backvote_errs_kernel(const float* __restrict__ pts,
                                                            const int32_t* __restrict__ pt_off,
                                                            const int32_t* __restrict__ idx, int k,
                                                            const int32_t* __restrict__ tup_off,
                                                            const float* __restrict__ tr,
                                                            const double* __restrict__ centers, Axes9 axes,
                                                            float* __restrict__ errs) {
  const int b = blockIdx.y;
  const float* p = pts + 3 * (int64_t)pt_off[b];
  const int t0 = tup_off[b], nt = tup_off[b + 1] - t0;
  const double cx = centers[3 * b], cy = centers[3 * b + 1], cz = centers[3 * b + 2];
  for (int t = blockIdx.x * 256 + threadIdx.x; t < nt; t += gridDim.x * 256) {
    const int64_t row = (int64_t)(t0 + t);
    const float* a = p + 3 * (int64_t)idx[row * k];
    const float* bb = p + 3 * (int64_t)idx[row * k + 1];
    float tb[2];
    target_pair(a[0], a[1], a[2], bb[0], bb[1], bb[2], cx, cy, cz, axes.a, tb, nullptr);
    const float d0 = tr[row * 2] - tb[0], d1 = tr[row * 2 + 1] - tb[1];
    errs[row] = __builtin_sqrtf(d0 * d0 + d1 * d1);
  }
}

__global__ __launch_bounds__(BV_THREADS) void backvote_kernel(
    const float* __restrict__ pts, const int32_t* __restrict__ pt_off, const int32_t* __restrict__ idx, int k,
    const int32_t* __restrict__ tup_off, const float* __restrict__ tr, const double* __restrict__ centers,
    Axes9 axes, const int32_t* __restrict__ kidx, const float* __restrict__ gammas, double margin, int num_rots,
    uint8_t* __restrict__ mask, int32_t* __restrict__ kept_tuple, int32_t* __restrict__ kept_count,
    double* __restrict__ kept_wt, int32_t* __restrict__ kept_row0, float* __restrict__ errs,
    float* __restrict__ thr_out, int32_t* __restrict__ hits) {
  __shared__ uint32_t s_hist[2048];
  __shared__ int s_misc[4];
  __shared__ int s_wave[BV_THREADS / 64];
  __shared__ float s_f[BV_THREADS / 64];
  const int b = blockIdx.x;
  const int p0 = pt_off[b];
  const float* p = pts + 3 * (int64_t)p0;
  const int t0 = tup_off[b], nt = tup_off[b + 1] - t0;
  float* e = errs + t0;
  if (nt <= 0) {
    if (threadIdx.x == 0) { kept_count[b] = 0; if (thr_out) thr_out[b] = NAN; }
    return;
  }
  // 1. (backvote_errs_kernel, spread over the chip) left the back-projection errors in errs[]
  // 2. np.percentile(back_errs, ratio*100), method 'linear' (eval.py:258): order statistics kq and kq+1
  int kq = kidx[b];
  if (kq > nt - 1) kq = nt - 1;
  const float gamma = gammas[b];
  int n_le = 0;
  const uint32_t bits_lo = radix_select(e, nt, kq, s_hist, s_misc, &n_le);
  const float v_lo = __uint_as_float(bits_lo);
  float v_hi = v_lo;
  if (kq + 1 <= nt - 1 && kq + 1 >= n_le) {
    // next order statistic = smallest element strictly above v_lo (bit order == value order for x >= 0, NaN last)
    uint32_t mn = 0xffffffffu;
    for (int i = threadIdx.x; i < nt; i += BV_THREADS) {
      const uint32_t bits = __float_as_uint(e[i]);
      if (bits > bits_lo && bits < mn) mn = bits;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, off));
    if (wave_lane() == 0) s_hist[threadIdx.x >> 6] = mn;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < BV_THREADS / 64; ++w) mn = min(mn, s_hist[w]);
      s_hist[64] = mn;
    }
    __syncthreads();
    v_hi = __uint_as_float(s_hist[64]);
    __syncthreads();
  }
  // numpy _lerp in float32: a + (b-a)*t, replaced by b - (b-a)*(1-t) where t >= 0.5
  const float diff = v_hi - v_lo;
  float thr = v_lo + diff * gamma;
  if (gamma >= 0.5f) thr = v_hi - diff * (1.0f - gamma);
  if (threadIdx.x == 0 && thr_out) thr_out[b] = thr;
  // 3. mask + ordered compaction (eval.py:258-268)
  int kept = 0;
  for (int base = 0; base < nt; base += BV_THREADS) {
    const int t = base + threadIdx.x;
    const bool keep = (t < nt) && (e[t] < thr);
    if (t < nt) mask[t0 + t] = keep ? 1 : 0;
    int tot;
    const int pos = block_scan_flag(keep, s_wave, &tot);
    if (keep) kept_tuple[t0 + kept + pos] = t;
    kept += tot;
  }
  if (threadIdx.x == 0) kept_count[b] = kept;
  __syncthreads();
  // 4. per-point hit histogram (eval.py:264-265), hits[] was zeroed by the host wrapper
  int32_t* h = hits + p0;
  for (int j = threadIdx.x; j < kept; j += BV_THREADS) {
    const int64_t row = (int64_t)(t0 + kept_tuple[t0 + j]);
    atomicAdd(&h[idx[row * k]], 1);
    atomicAdd(&h[idx[row * k + 1]], 1);
  }
  __threadfence();
  __syncthreads();
  int hmax = 0;
  for (int j = threadIdx.x; j < kept; j += BV_THREADS) {
    const int64_t row = (int64_t)(t0 + kept_tuple[t0 + j]);
    hmax = max(hmax, __hip_atomic_load(&h[idx[row * k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    hmax = max(hmax, __hip_atomic_load(&h[idx[row * k + 1]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) hmax = max(hmax, __shfl_xor(hmax, off));
  if (wave_lane() == 0) s_wave[threadIdx.x >> 6] = hmax;
  __syncthreads();
  hmax = 0;
  for (int w = 0; w < BV_THREADS / 64; ++w) hmax = max(hmax, s_wave[w]);
  __syncthreads();
  const double dmax = (double)hmax;
  // 5. pair weights (eval.py:274-275) + row of each pair in vote_rotation's compacted candidate list
  int rank = 0;
  for (int base = 0; base < kept; base += BV_THREADS) {
    const int j = base + threadIdx.x;
    bool valid = false;
    if (j < kept) {
      const int64_t row = (int64_t)(t0 + kept_tuple[t0 + j]);
      const int i0 = idx[row * k], i1 = idx[row * k + 1];
      const double w0 = (double)__hip_atomic_load(&h[i0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) / dmax;
      const double w1 = (double)__hip_atomic_load(&h[i1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) / dmax;
      kept_wt[t0 + j] = (w0 + w1) + margin;
      const float dx = p[3 * i0] - p[3 * i1], dy = p[3 * i0 + 1] - p[3 * i1 + 1], dz = p[3 * i0 + 2] - p[3 * i1 + 2];
      valid = norm3_fused(dx, dy, dz) > 1e-7f;                        // train_dino.py:223
    }
    int tot;
    const int pos = block_scan_flag(valid, s_wave, &tot);
    if (j < kept) kept_row0[t0 + j] = valid ? (rank + pos) * num_rots : -1;
    rank += tot;
  }
  (void)s_f;
}

extern "C" int64_t cppf_backvote_workspace_bytes(int64_t total_points, int B) {
  (void)B;
  return align_up(total_points * 4, 256);
}

extern "C" int cppf_backvote_filter(int B, const float* pts, const int32_t* pt_off, const int32_t* idx, int k,
                                    const int32_t* tup_off, const float* tr, const double* centers,
                                    const double* h_axes, const int32_t* kidx, const float* gammas,
                                    double imp_wt_margin, int num_rots, uint8_t* mask, int32_t* kept_tuple,
                                    int32_t* kept_count, double* kept_wt, int32_t* kept_row0, float* back_errs,
                                    float* thr, void* workspace, int64_t workspace_bytes, void* stream) {
  CPPF_CHECK_ARG(B > 0 && pts && pt_off && idx && tup_off && tr && centers && h_axes && kidx && gammas);
  CPPF_CHECK_ARG(mask && kept_tuple && kept_count && kept_wt && kept_row0 && back_errs);
  CPPF_CHECK_ARG(workspace && workspace_bytes > 0);
  Axes9 ax;
  for (int i = 0; i < 9; ++i) ax.a[i] = h_axes[i];
  CPPF_HIP(hipMemsetAsync(workspace, 0, (size_t)workspace_bytes, (hipStream_t)stream));
  hipLaunchKernelGGL(backvote_errs_kernel, dim3(B >= 32 ? 16 : 64, B), dim3(256), 0, (hipStream_t)stream, pts, pt_off,
                     idx, k, tup_off, tr, centers, ax, back_errs);
  CPPF_LAUNCH_CHECK();
  hipLaunchKernelGGL(backvote_kernel, dim3(B), dim3(BV_THREADS), 0, (hipStream_t)stream, pts, pt_off, idx, k, tup_off,
                     tr, centers, ax, kidx, gammas, imp_wt_margin, num_rots, mask, kept_tuple, kept_count, kept_wt,
                     kept_row0, back_errs, thr, (int32_t*)workspace);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}

// =============================================================================================
// a11. pose assembly (eval.py:295-313) + lower median of the scale head over kept pairs (eval.py:309)
// =============================================================================================
#define ASM_STAGE 4096
__global__ __launch_bounds__(256) void assemble_pose_kernel(
    const float* __restrict__ sphere, const int32_t* __restrict__ up_idx, const float* __restrict__ up_count,
    const int32_t* __restrict__ right_idx, const float* __restrict__ right_count, int up_axis, int right_axis,
    const int64_t* __restrict__ argmax, const uint32_t* __restrict__ peak, const double* __restrict__ world,
    const CppfSceneGrid* __restrict__ grids, const float* __restrict__ pred_scales,
    const int32_t* __restrict__ tup_off, const int32_t* __restrict__ kept_tuple,
    const int32_t* __restrict__ kept_count, CppfSceneResult* __restrict__ out) {
  const int b = blockIdx.x;
  __shared__ float s_med[3];
  const int kept = kept_count ? kept_count[b] : 0;
  if (threadIdx.x < 3) s_med[threadIdx.x] = NAN;
  __syncthreads();
  if (pred_scales && kept > 0) {
    // lower median (torch.median) = order statistic (kept-1)/2 of each column, by radix select
    __shared__ uint32_t s_hist[2048];
    __shared__ int s_misc[4];
    const int t0 = tup_off[b];
    const int target = (kept - 1) / 2;
    // the kept pairs' rows are scattered over the [T,3] scale-head output: fetch them once (order-preserving keys) and
    // select from LDS; longer lists than the staging area select straight from memory
    __shared__ uint32_t s_keys[3][ASM_STAGE];
    const bool staged = kept <= ASM_STAGE;
    if (staged) {
      for (int i = threadIdx.x; i < kept; i += blockDim.x) {
        const float* row = pred_scales + (int64_t)(t0 + kept_tuple[t0 + i]) * 3;
        s_keys[0][i] = float_key(row[0]); s_keys[1][i] = float_key(row[1]); s_keys[2][i] = float_key(row[2]);
      }
      __syncthreads();
    }
    for (int col = 0; col < 3; ++col) {
      int n_le;
      uint32_t k;
      if (staged) {
        const uint32_t* keys = s_keys[col];
        k = radix_select_keys([=](int i) { return keys[i]; }, kept, target, s_hist, s_misc, &n_le);
      } else {
        k = radix_select_keys(
            [=](int i) { return float_key(pred_scales[(int64_t)(t0 + kept_tuple[t0 + i]) * 3 + col]); }, kept, target,
            s_hist, s_misc, &n_le);
      }
      if (threadIdx.x == 0) s_med[col] = key_float(k);
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  CppfSceneResult r;
  r.argmax = argmax[b];
  r.peak = peak ? peak[b] : 0u;
  r.t[0] = world[3 * b]; r.t[1] = world[3 * b + 1]; r.t[2] = world[3 * b + 2];
  r.up_idx = up_idx[b]; r.right_idx = right_idx[b];
  r.up_count = up_count ? up_count[b] : 0.0f;
  r.right_count = right_count ? right_count[b] : 0.0f;
  r.kept = kept;
  r.flags = (grids ? grids[b].flags : 0) | ((peak && peak[b] == 0xFFFFFFFFu) ? 4 : 0);
  r.ncell = grids ? grids[b].ncell : 0;
  r.pad_[0] = r.pad_[1] = r.pad_[2] = 0;
  r.scale[0] = s_med[0]; r.scale[1] = s_med[1]; r.scale[2] = s_med[2];
  pose_from_bins(sphere, r.up_idx, r.right_idx, up_axis, right_axis, r.R);   // eval.py:295-313
  out[b] = r;
}

extern "C" int cppf_assemble_pose(int B, const float* sphere, const int32_t* up_idx, const float* up_count,
                                  const int32_t* right_idx, const float* right_count, int up_axis, int right_axis,
                                  const int64_t* argmax, const uint32_t* peak, const double* world,
                                  const CppfSceneGrid* grids, const float* pred_scales, const int32_t* tup_off,
                                  const int32_t* kept_tuple, const int32_t* kept_count, CppfSceneResult* out,
                                  void* stream) {
  CPPF_CHECK_ARG(B > 0 && sphere && up_idx && right_idx && argmax && world && out);
  CPPF_CHECK_ARG(up_axis >= 0 && up_axis < 3 && right_axis >= 0 && right_axis < 3 && up_axis != right_axis);
  CPPF_CHECK_ARG(pred_scales == nullptr || (tup_off && kept_tuple && kept_count));
  hipLaunchKernelGGL(assemble_pose_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, sphere, up_idx, up_count,
                     right_idx, right_count, up_axis, right_axis, argmax, peak, world, grids, pred_scales, tup_off,
                     kept_tuple, kept_count, out);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}

// =============================================================================================
// Kept-row lists: global tuple rows of the pairs that survived the back-vote filter, fixed shape [B, max_kept], as int32 (what the
// gathering MLP kernel and cppf_reslayer_tail index with) or int64 (what a caller gathers / scatters per-pair tensors with,
// without a host sync).  Padding contract: entries past a scene's count hold the scene's first tuple row, or row 0 for a scene
// without tuples -- always a valid row, never written through (cppf_reslayer_tail skips them by kept_count).
// =============================================================================================
template <typename RowT>
__global__ __launch_bounds__(256) void kept_rows_kernel(int B, const int32_t* __restrict__ tup_off,
                                                        const int32_t* __restrict__ kept_tuple,
                                                        const int32_t* __restrict__ kept_count, int max_kept,
                                                        RowT* __restrict__ rows) {
  const int64_t n = (int64_t)B * max_kept;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / max_kept), j = (int)(i - (int64_t)b * max_kept);
    const int t0 = tup_off[b];
    rows[i] = (j < kept_count[b]) ? (RowT)t0 + kept_tuple[t0 + j] : (t0 < tup_off[b + 1] ? (RowT)t0 : 0);
  }
}

template <typename RowT>
static int kept_rows_launch(int B, const int32_t* tup_off, const int32_t* kept_tuple, const int32_t* kept_count, int max_kept,
                            RowT* rows, void* stream) {
  CPPF_CHECK_ARG(B > 0 && tup_off && kept_tuple && kept_count && rows && max_kept >= 0);
  if (max_kept == 0) return CPPF_OK;
  const int64_t n = (int64_t)B * max_kept;
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(kept_rows_kernel<RowT>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, B, tup_off, kept_tuple, kept_count,
                     max_kept, rows);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}

extern "C" int cppf_kept_rows(int B, const int32_t* tup_off, const int32_t* kept_tuple, const int32_t* kept_count,
                              int max_kept, int64_t* rows, void* stream) {
  return kept_rows_launch(B, tup_off, kept_tuple, kept_count, max_kept, rows, stream);
}

extern "C" int cppf_kept_rows32(int B, const int32_t* tup_off, const int32_t* kept_tuple, const int32_t* kept_count,
                                int max_kept, int32_t* rows, void* stream) {
  return kept_rows_launch(B, tup_off, kept_tuple, kept_count, max_kept, rows, stream);
}
