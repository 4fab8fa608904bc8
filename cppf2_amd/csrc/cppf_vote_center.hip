// cppf_vote_center.hip -- centre Hough vote + first maximum, further grid peaks.  gfx950 only.  See include/cppf_hip.h for
// the contract of each entry point.
#include "cppf_common.h"

// =============================================================================================
// a6. vote_center (train_dino.py:171-215)
//
// MI355X design.  The vote grid of a scene (1.6e5 .. 1e6 uint32 cells) is cut into slabs of VC_SLAB_CELLS
// consecutive flat cells (whole-or-partial x-layers) that fit the 160 KiB LDS of one CU.
//   1. vote_frames_kernel: once per pair, the circle frame (centre c, in-plane axes x, y, all the IEEE
//      sqrt/div work of train_dino.py:176-192) goes to a structure-of-arrays workspace, together with the
//      amplitude/phase of the circle's x-coordinate.
//   2. vote_slab_item: a workgroup takes one (scene, slab) item, streams the frames (coalesced), and for every pair
//      derives the rotation indices that can reach the slab's x-layers (two arcs of the circle, from the
//      amplitude/phase) -- so the work per scene stays ~one pass over the votes no matter how many slabs the
//      grid needs.  Votes are counted with LDS atomics; arcs are very uneven in length, so a wavefront cuts its
//      64 arcs into quanta of VC_QUANTUM rotations and deals the quanta out evenly over its lanes (owner frame
//      pulled across lanes with ds_bpermute).  The cell of a vote is found without an IEEE division on the fast path
//      (multiply by the rounded reciprocal, exact division only when the result lands within rounding distance
//      of a cell boundary), which keeps the grid bit-identical to the reference's float32 pipeline.
//      The slab is streamed out with plain coalesced stores (or not at all when the caller only wants the
//      peak) and its first maximum is reduced in place: no global atomics, no memset, no grid re-read.
//   3. Scheduling: vote_worklist_kernel lists the slabs that exist (scene bounds live on the device), centre-out so
//      the heavy central slabs start first, and vote_center_persist_kernel runs one workgroup per CU that pulls items
//      from the list.  When there are fewer slabs than CUs (small batches) the list kernel splits every slab's pair
//      list into parts; the parts merge through a zeroed area with device atomics and a ticket per slab.
// vote_center_slab_kernel (one item per workgroup, (scene, part, rank) launch) remains for the exhaustive A/B mode and
// on request (mode bit VC_MODE_NO_PERSIST); there the parts of a small batch merge into the zeroed global grid.
// Mode 2 (global atomics, one thread per pair, exhaustive sweep) is the independent A/B reference; mode 3 is
// the slab kernel with the exhaustive rotation sweep and exact divisions.
// =============================================================================================
#define VC_THREADS 1024
#ifndef VC_SLAB_CELLS
#define VC_SLAB_CELLS 36864            // 144 KiB of uint32 counters
#endif
#define VC_ARG_BLOCKS 32
#ifndef VC_MAX_LDS_ROTS
#define VC_MAX_LDS_ROTS 512            // rotation tables kept in LDS (twice, so a quantum never wraps): 2 x (2*512+4) floats
#endif
#define VC_TAB_LEN (2 * VC_MAX_LDS_ROTS + 4)
#define VC_LDS_WORDS (VC_SLAB_CELLS + 2 * VC_TAB_LEN + (VC_THREADS / 64) * 64)
#ifndef VC_MIN_SLAB_CELLS
#define VC_MIN_SLAB_CELLS 8192         // finest cut of a small grid (vote_worklist_kernel)
#endif
#ifndef VC_MIN_WAVES
#define VC_MIN_WAVES 4
#endif
#define VC_FRAME_FLOATS 12             // cx cy cz xx xy xz yx yy yz invA phi weight(uint bits)
#define VC_WT_SCALE 256.0f             // fixed-point unit of weighted votes (weights in [0, 4])
#ifndef VC_QUANTUM
#define VC_QUANTUM 4
#endif
#ifndef VC_ARC_MARGIN
#define VC_ARC_MARGIN 0.02f
#endif

struct SlabBest {
  int64_t idx;
  uint32_t val;
  uint32_t pad;
};

struct VoteSetup {
  float cx, cy, cz, xx, xy, xz, yx, yy, yz;
  bool ok;
};

__device__ __forceinline__ VoteSetup vote_setup(const float* __restrict__ p, int i0, int i1, float proj, float od,
                                                float res) {
  VoteSetup s;
  const PairFrame f = pair_frame(p, i0, i1);
  s.ok = (f.nrm > 1e-7f) & (od > res);                                  // train_dino.py:182
  s.cx = f.ax - f.ux * proj; s.cy = f.ay - f.uy * proj; s.cz = f.az - f.uz * proj;   // :186
  s.xx = f.cox / f.nco * od; s.xy = f.coy / f.nco * od; s.xz = f.coz / f.nco * od;   // :191
  s.yx = cross_term(s.xy, f.uz, s.xz, f.uy);                            // :192 torch.cross(x, ab)
  s.yy = cross_term(s.xz, f.ux, s.xx, f.uz);
  s.yz = cross_term(s.xx, f.uy, s.xy, f.ux);
  return s;
}

// exact vote: flat cell index or -1 (train_dino.py:195-203), IEEE divisions
__device__ __forceinline__ int vote_cell(float cx, float cy, float cz, float xx, float xy, float xz, float yx,
                                         float yy, float yz, float cs, float sn, float c0x, float c0y, float c0z,
                                         float res, int gx, int gy, int gz) {
  const float ox = cs * xx + sn * yx;
  const float oy = cs * xy + sn * yy;
  const float oz = cs * xz + sn * yz;
  const float fx = ((cx + ox) - c0x) / res + 0.5f;
  const float fy = ((cy + oy) - c0y) / res + 0.5f;
  const float fz = ((cz + oz) - c0z) / res + 0.5f;
  // (f).long() > 0  <=>  f >= 1 ; (f).long() < g  <=>  f < g   (NaN/inf fail both, like the int64 cast)
  const bool ok = (fx >= 1.0f) & (fy >= 1.0f) & (fz >= 1.0f) & (fx < (float)gx) & (fy < (float)gy) & (fz < (float)gz);
  if (!ok) return -1;
  return ((int)fx * gy + (int)fy) * gz + (int)fz;
}

// Vote weight in accumulator units: 1 per vote when no weights are given (the reference, train_dino.py:204);
// otherwise round(w * 256), w clamped to [0, 4] (deterministic integer accumulation: the "uncertainty-weighted"
// accumulator of BASELINE config 5; not in the reference -- w == 1 gives exactly 256 x the reference grid).
__device__ __forceinline__ uint32_t vote_weight(const float* __restrict__ vote_wt, int64_t row) {
  if (!vote_wt) return 1u;
  const float w = fminf(fmaxf(vote_wt[row], 0.0f), 4.0f);
  return (uint32_t)(w * VC_WT_SCALE + 0.5f);
}

// 1. per-pair frames -> SoA workspace fr[VC_FRAME_FLOATS][total]
__global__ __launch_bounds__(256) void vote_frames_kernel(const float* __restrict__ pts,
                                                          const int32_t* __restrict__ pt_off,
                                                          const int32_t* __restrict__ idx, int k,
                                                          const int32_t* __restrict__ tup_off,
                                                          const float* __restrict__ tr,
                                                          const float* __restrict__ vote_wt, float res, int num_rots,
                                                          int64_t total, float* __restrict__ fr) {
  const int b = blockIdx.y;
  const float* p = pts + 3 * (int64_t)pt_off[b];
  const int t0 = tup_off[b], nt = tup_off[b + 1] - t0;
  const float kappa = (float)num_rots * 0.15915494309189535f;           // R / (2 pi)
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += gridDim.x * blockDim.x) {
    const int64_t row = (int64_t)(t0 + t);
    VoteSetup v = vote_setup(p, idx[row * k], idx[row * k + 1], tr[row * 2], tr[row * 2 + 1], res);
    if (!v.ok) v.cx = NAN;                                              // NaN centre: every vote is invalid
    const float A = sqrtf(v.xx * v.xx + v.yx * v.yx);                   // x(theta) - cx = A cos(theta - phi)
    fr[0 * total + row] = v.cx; fr[1 * total + row] = v.cy; fr[2 * total + row] = v.cz;
    fr[3 * total + row] = v.xx; fr[4 * total + row] = v.xy; fr[5 * total + row] = v.xz;
    fr[6 * total + row] = v.yx; fr[7 * total + row] = v.yy; fr[8 * total + row] = v.yz;
    fr[9 * total + row] = (A > 1e-12f) ? 1.0f / A : 0.0f;
    fr[10 * total + row] = atan2f(v.yx, v.xx) * kappa;
    fr[11 * total + row] = __uint_as_float(vote_weight(vote_wt, row));
  }
}

// Rotation indices whose vote can fall into x-layers [xl, xh] of the grid: cos(theta - phi) in [L, U]/A gives
// two arcs symmetric about phi, widened by VC_ARC_MARGIN steps and merged where they touch, so the ranges are
// disjoint modulo num_rots.  Indices outside them provably vote outside the slab; indices inside are still
// tested exactly, so the grid is identical to the exhaustive sweep (tests compare modes 1, 2 and 3).
struct ArcSet {
  int a0, n0, a1, n1;   // start index (may be negative / exceed num_rots: taken modulo) and length of each arc
};

__device__ __forceinline__ ArcSet slab_arcs(float cx, float invA, float phi, float c0x, float res, int xl, int xh,
                                            int num_rots) {
  ArcSet o;
  o.a0 = 0; o.n0 = 0; o.a1 = 0; o.n1 = 0;
  const float slop = 0.01f * res + 4e-7f * (fabsf(cx) + fabsf(c0x));
  const float L = ((float)xl - 0.5f) * res + c0x - cx - slop;
  const float U = ((float)xh + 0.5f) * res + c0x - cx + slop;
  if (!(L <= U)) return o;                                   // NaN / inf centre: every vote is invalid anyway
  if (invA == 0.0f) {
    if (L <= 0.0f && 0.0f <= U) o.n0 = num_rots;
    return o;
  }
  const float cl = L * invA - 1e-6f, cu = U * invA + 1e-6f;
  if (cl > 1.0f || cu < -1.0f) return o;
  const float kappa = (float)num_rots * 0.15915494309189535f;
  const float amin = acosf(fminf(cu, 1.0f)) * kappa;
  const float amax = acosf(fmaxf(cl, -1.0f)) * kappa;
  const float half = 0.5f * (float)num_rots;
  // |theta - phi| in [amin, amax] (rotation-index units): the integer rotations inside each arc, rounded INWARD --
  // everything that makes the bounds uncertain (rounding of the vote's x, of A, phi, acosf, the table's angles) is
  // covered by `slop`, the 1e-6 in cosine space and VC_ARC_MARGIN, so no whole extra rotation per arc end is needed.
  // The two arcs are merged where fewer than one rotation separates them (they would otherwise share an index).
  const bool near_merge = amin <= 0.5f;
  const bool far_merge = (half - amax) <= 0.5f;
  if (near_merge && far_merge) { o.n0 = num_rots; return o; }
  int b0;
  if (near_merge) {
    o.a0 = (int)ceilf(phi - amax - VC_ARC_MARGIN); b0 = (int)floorf(phi + amax + VC_ARC_MARGIN);
  } else if (far_merge) {
    o.a0 = (int)ceilf(phi + amin - VC_ARC_MARGIN); b0 = (int)floorf(phi + (float)num_rots - amin + VC_ARC_MARGIN);
  } else {
    o.a0 = (int)ceilf(phi + amin - VC_ARC_MARGIN); b0 = (int)floorf(phi + amax + VC_ARC_MARGIN);
    o.a1 = (int)ceilf(phi - amax - VC_ARC_MARGIN);
    o.n1 = max((int)floorf(phi - amin + VC_ARC_MARGIN) - o.a1 + 1, 0);
  }
  o.n0 = max(b0 - o.a0 + 1, 0);
  if (o.n0 >= num_rots) { o.a0 = 0; o.n0 = num_rots; o.n1 = 0; }
  return o;
}

// ---- wavefront scans on the DPP cross-lane path (no LDS round trip): Hillis-Steele inside each row of 16 lanes
// (row_shr 1,2,4,8), then the row totals ripple with row_bcast15 (rows 1,3) and row_bcast31 (rows 2,3).
#define VC_DPP(x, ctrl, rmask) __builtin_amdgcn_update_dpp(0, (x), (ctrl), (rmask), 0xf, false)
__device__ __forceinline__ int wave_incl_scan_add(int x) {
  x += VC_DPP(x, 0x111, 0xf);
  x += VC_DPP(x, 0x112, 0xf);
  x += VC_DPP(x, 0x114, 0xf);
  x += VC_DPP(x, 0x118, 0xf);
  x += VC_DPP(x, 0x142, 0xa);
  x += VC_DPP(x, 0x143, 0xc);
  return x;
}
__device__ __forceinline__ int wave_incl_scan_max(int x) {   // values >= 0
  x = max(x, VC_DPP(x, 0x111, 0xf));
  x = max(x, VC_DPP(x, 0x112, 0xf));
  x = max(x, VC_DPP(x, 0x114, 0xf));
  x = max(x, VC_DPP(x, 0x118, 0xf));
  x = max(x, VC_DPP(x, 0x142, 0xa));
  x = max(x, VC_DPP(x, 0x143, 0xc));
  return x;
}

typedef float vc_f2 __attribute__((ext_vector_type(2)));

struct GridFast {
  float c0x, c0y, c0z, rinv;
  float lo_m, hi_m;             // a fractional part inside [lo_m, hi_m] is farther than the rounding margin from a cell boundary
  int gx, gy, gz;
};

__device__ __forceinline__ vc_f2 vc_pk_fma(vc_f2 a, vc_f2 b, vc_f2 c) {
  vc_f2 d;
  asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ int vc_flr(float t) {
  int i;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(i) : "v"(t));
  return i;
}
__device__ __forceinline__ int vc_mad24(int a, int b, int c) {
  int d;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(b), "v"(c));
  return d;
}
__device__ __forceinline__ float vc_min3(float a, float b, float c) {
  float d;
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
__device__ __forceinline__ float vc_max3(float a, float b, float c) {
  float d;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

// One coordinate of two consecutive rotations on the packed-fp32 pipe: t = fma((c + (cs*a + sn*b)) - c0, 1/res, half),
// every operation rounded where the reference rounds it (train_dino.py:195-197: mul, mul, add, add, sub; the division by
// res is replaced by the fused multiply with the rounded reciprocal -- see the decision procedure below).
__device__ __forceinline__ vc_f2 vc_coord2(vc_f2 cs, vc_f2 sn, float a, float b, float c, float c0, vc_f2 rinv2,
                                           vc_f2 half2) {
  const vc_f2 o = cs * a + sn * b;
  const vc_f2 nrm = (c + o) - c0;
  return vc_pk_fma(nrm, rinv2, half2);
}

// The VC_QUANTUM = 4 votes of one quantum (consecutive rotations rr .. rr+3 of one pair) on the fast path: relative cell
// index of each vote (unsigned: anything >= n is "not in this slab"), validity bits, and `sure`, cleared when any
// of the 12 coordinates lands within the rounding margin of a cell boundary -- or is NaN / huge -- in which case the
// caller redoes the quantum with the exact IEEE divisions (vote_cell_exact below).
//   num = (c+off)-c0 exactly as the reference computes it; the reference's value is t_ref = fl(fl(num/res) + 0.5).
//   t = fma(num, rinv, 0.5) differs from it by at most (|q|+1) * 3e-7 (rounded reciprocal + one rounding vs quotient
//   rounding + add rounding), so whenever t is farther than m = (g+2)*1e-6 from every integer, floor(t) ==
//   trunc(t_ref) and both validity tests (cell > 0, cell < g) agree.
// y and z are evaluated one cell lower (half = -0.5): floor gives cell - 1 directly, which is what the validity test
// 0 < cell < g  <=>  (unsigned)(cell - 1) < g - 1 wants; the constant is folded into `base`.  x is clamped to [0, gx]
// instead of tested: layer gx lies beyond the last slab, and layer 0 (train_dino.py:199 keeps indices > 0) is wiped
// by the caller after the votes.  Rotation pairs travel as one register pair (v_pk_*), cos/sin come from LDS tables
// laid out twice in a row so that rr + 3 never wraps.
struct QuantumCells {
  unsigned rel[VC_QUANTUM];
  bool ok[VC_QUANTUM];
  float fmin[VC_QUANTUM], fmax[VC_QUANTUM];   // smallest / largest fractional part of each vote's three coordinates
};

__device__ __forceinline__ QuantumCells vote_quantum(float cx, float cy, float cz, float xx, float xy, float xz, float yx,
                                                     float yy, float yz, const float* s_cos, const float* s_sin, int rr,
                                                     const GridFast& gc, unsigned base, bool& sure) {
  static_assert(VC_QUANTUM == 4, "vote_quantum is written for quanta of 4 rotations");
  const vc_f2 c01 = {s_cos[rr], s_cos[rr + 1]}, c23 = {s_cos[rr + 2], s_cos[rr + 3]};
  const vc_f2 s01 = {s_sin[rr], s_sin[rr + 1]}, s23 = {s_sin[rr + 2], s_sin[rr + 3]};
  const vc_f2 rinv2 = {gc.rinv, gc.rinv}, hp = {0.5f, 0.5f}, hm = {-0.5f, -0.5f};
  const vc_f2 tx01 = vc_coord2(c01, s01, xx, yx, cx, gc.c0x, rinv2, hp), tx23 = vc_coord2(c23, s23, xx, yx, cx, gc.c0x, rinv2, hp);
  const vc_f2 ty01 = vc_coord2(c01, s01, xy, yy, cy, gc.c0y, rinv2, hm), ty23 = vc_coord2(c23, s23, xy, yy, cy, gc.c0y, rinv2, hm);
  const vc_f2 tz01 = vc_coord2(c01, s01, xz, yz, cz, gc.c0z, rinv2, hm), tz23 = vc_coord2(c23, s23, xz, yz, cz, gc.c0z, rinv2, hm);
  const float tx[4] = {tx01.x, tx01.y, tx23.x, tx23.y}, ty[4] = {ty01.x, ty01.y, ty23.x, ty23.y},
              tz[4] = {tz01.x, tz01.y, tz23.x, tz23.y};
  float fr[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    fr[3 * j] = __builtin_amdgcn_fractf(tx[j]); fr[3 * j + 1] = __builtin_amdgcn_fractf(ty[j]);
    fr[3 * j + 2] = __builtin_amdgcn_fractf(tz[j]);
  }
  QuantumCells q;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    q.fmin[j] = vc_min3(fr[3 * j], fr[3 * j + 1], fr[3 * j + 2]);
    q.fmax[j] = vc_max3(fr[3 * j], fr[3 * j + 1], fr[3 * j + 2]);
  }
  const float mn = fminf(vc_min3(q.fmin[0], q.fmin[1], q.fmin[2]), q.fmin[3]);
  const float mx = fmaxf(vc_max3(q.fmax[0], q.fmax[1], q.fmax[2]), q.fmax[3]);
  sure = (mn >= gc.lo_m) & (mx <= gc.hi_m);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int ix = vc_flr(tx[j]);
    const int iy = vc_flr(ty[j]), iz = vc_flr(tz[j]);                 // cell - 1
    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(ix) : "v"(ix), "s"(gc.gx));
    q.ok[j] = ((unsigned)iy < (unsigned)(gc.gy - 1)) & ((unsigned)iz < (unsigned)(gc.gz - 1));
    q.rel[j] = (unsigned)vc_mad24(vc_mad24(ix, gc.gy, iy), gc.gz, iz) + base;   // flat cell - first cell of the slab
  }
  return q;
}

// the same vote with the reference's arithmetic (train_dino.py:195-203); out of line (rare) and with every argument by
// value: a reference to the grid constants would force them into scratch memory for the whole kernel
__device__ __noinline__ int vote_cell_exact(float cx, float cy, float cz, float xx, float xy, float xz, float yx,
                                            float yy, float yz, float cs, float sn, float c0x, float c0y, float c0z,
                                            float res, int gx, int gy, int gz) {
  return vote_cell(cx, cy, cz, xx, xy, xz, yx, yy, yz, cs, sn, c0x, c0y, c0z, res, gx, gy, gz);
}

struct FrameRegs {
  float cx, cy, cz, xx, xy, xz, yx, yy, yz, invA, phi;
  uint32_t wv;
};

// one pair's frame from the SoA workspace (a NaN centre = "no votes" for rows past the end)
__device__ __forceinline__ FrameRegs load_frame(const float* __restrict__ fr, int64_t total, int64_t row, bool in) {
  FrameRegs f;
  f.cx = NAN; f.cy = 0.0f; f.cz = 0.0f; f.xx = 0.0f; f.xy = 0.0f; f.xz = 0.0f; f.yx = 0.0f; f.yy = 0.0f; f.yz = 0.0f;
  f.invA = 0.0f; f.phi = 0.0f; f.wv = 0u;
  if (in) {
    f.cx = fr[0 * total + row]; f.cy = fr[1 * total + row]; f.cz = fr[2 * total + row];
    f.xx = fr[3 * total + row]; f.xy = fr[4 * total + row]; f.xz = fr[5 * total + row];
    f.yx = fr[6 * total + row]; f.yy = fr[7 * total + row]; f.yz = fr[8 * total + row];
    f.invA = fr[9 * total + row]; f.phi = fr[10 * total + row];
    f.wv = __float_as_uint(fr[11 * total + row]);
  }
  return f;
}

// The quantum a lane works on in one window and the frame of the pair that owns it.
struct OwnerRegs {
  float cx, cy, cz, xx, xy, xz, yx, yy, yz;
  int rr, len;          // first rotation (index into the doubled tables) and rotations left in the arc (<= 0: idle lane)
  uint32_t wv;
};

// Lane l of the window starting at quantum qb takes quantum qb + l of the wavefront's arcs.  Its owner pair is found
// without a search: every owner drops (window tag | lane id) at the window slot of its first quantum in a 64-entry LDS
// strip, and a DPP max-scan of the strip spreads it over the owner's quanta (stale entries of older windows carry
// smaller tags, so the strip is never cleared).  The owner's frame then comes across lanes with ds_bpermute.
template <bool WEIGHTED>
__device__ __forceinline__ OwnerRegs find_owner(int qb, int WQ, int incl, int excl, int nq, int pk0, int pk1, uint32_t wv,
                                                float cx, float cy, float cz, float xx, float xy, float xz, float yx,
                                                float yy, float yz, int lane, uint32_t* s_mark, int& tag) {
  tag += 64;
  const int first = __popcll(__ballot(incl <= qb));            // owner of quantum qb (< 64 because qb < WQ)
  const unsigned wslot = (unsigned)(excl - qb);
  if (nq > 0 && wslot < 64u) s_mark[wslot] = (uint32_t)(tag | lane);
  __builtin_amdgcn_wave_barrier();
  int m = (int)s_mark[lane];
  __builtin_amdgcn_wave_barrier();
  m = (lane == 0) ? (tag | first) : m;
  const int src = wave_incl_scan_max(m) & 63;
  OwnerRegs o;
  o.cx = __shfl(cx, src); o.cy = __shfl(cy, src); o.cz = __shfl(cz, src);
  o.xx = __shfl(xx, src); o.xy = __shfl(xy, src); o.xz = __shfl(xz, src);
  o.yx = __shfl(yx, src); o.yy = __shfl(yy, src); o.yz = __shfl(yz, src);
  const int opk0 = __shfl(pk0, src), opk1 = __shfl(pk1, src);
  const int ql = qb + lane - __shfl(excl, src);                 // quantum index inside the owner
  o.wv = WEIGHTED ? (uint32_t)__shfl((int)wv, src) : 1u;
  const int onq0 = opk0 >> 21;
  const bool second = ql >= onq0;
  const int qa = (second ? ql - onq0 : ql) * VC_QUANTUM;
  const int opk = second ? opk1 : opk0;
  o.rr = (opk & 1023) + qa;                                     // < 2 R: the tables are laid out twice in a row
  const int len = ((opk >> 10) & 2047) - qa;
  o.len = (qb + lane < WQ) ? len : 0;
  return o;
}

// One work item of the slab scheme: scene b, slab s (n cells from flat cell lo), part pc of Pl of the scene's pair
// list.  Called by the one-item-per-workgroup kernel (small batches) and by the persistent kernel (work list).
// LDS: slab[VC_SLAB_CELLS] counters | cos[VC_TAB_LEN] | sin[VC_TAB_LEN] (the table twice in a row + 4) | 64 owner
// marks per wavefront.
template <bool ARCS, bool WEIGHTED>
__device__ __forceinline__ void vote_slab_item(
    uint32_t* slab, int& tag, int b, int s, int slab_cells, int pc, int Pl,
    const CppfSceneGrid& g, int G, const float* __restrict__ fr, int64_t total, const int32_t* __restrict__ tup_off,
    float res, int num_rots, const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
    uint32_t* __restrict__ grid, const int64_t* __restrict__ grid_off, int64_t cells_cap,
    SlabBest* __restrict__ slab_best, int s_max, int P, uint32_t* __restrict__ part, int* __restrict__ tickets) {
#ifdef VC_DIAG
  const long long t_start = wall_clock64();
#endif
  const float* s_cos = reinterpret_cast<const float*>(slab + VC_SLAB_CELLS);
  const float* s_sin = s_cos + VC_TAB_LEN;
  uint32_t* s_mark = slab + VC_SLAB_CELLS + 2 * VC_TAB_LEN + (threadIdx.x >> 6) * 64;     // this wavefront's strip
  const int lo = s * slab_cells;                               // slab_cells <= VC_SLAB_CELLS: the counters of this item
  const int n = min(slab_cells, G - lo);
  for (int i = threadIdx.x; i < n; i += VC_THREADS) slab[i] = 0u;
  __syncthreads();
#ifdef VC_DIAG
  const long long t_a = wall_clock64();
  int nwin = 0;
#endif

  const int t0 = tup_off[b], nt = tup_off[b + 1] - t0;
  const int per = (nt + Pl - 1) / Pl;
  const int ts = pc * per, te = min(nt, ts + per);
  const int gx = g.g[0], gy = g.g[1], gz = g.g[2];
  const float c0x = g.c0[0], c0y = g.c0[1], c0z = g.c0[2];
  const int gyz = gy * gz;
  const int xl = lo / gyz, xh = (lo + n - 1) / gyz;            // x-layers this slab touches
  GridFast gf;
  gf.c0x = c0x; gf.c0y = c0y; gf.c0z = c0z; gf.rinv = 1.0f / res;
  gf.lo_m = (float)(max(gx, max(gy, gz)) + 2) * 1e-6f;
  gf.hi_m = 1.0f - gf.lo_m;
  gf.gx = gx; gf.gy = gy; gf.gz = gz;
  // the packed cell index uses 24-bit multiplies: (gx + 1) * gy must stay below 2^23 (any grid the reference
  // accepts, eval.py:200, is far below); wider grids take the exhaustive sweep with 32-bit arithmetic
  const bool narrow = (int64_t)(gx + 1) * gy < (1 << 23) && gz < (1 << 23);
  // vote_quantum works with (cell_y - 1, cell_z - 1): flat cell = (ix*gy + iy')*gz + iz' + (gz + 1); relative to the slab
  const unsigned base = (unsigned)(gz + 1 - lo);
  const int lane = wave_lane();
  // frames of the next block of pairs are requested before the current block is processed (register double buffer)
  FrameRegs nf = load_frame(fr, total, (int64_t)t0 + ts + (int)threadIdx.x, ts + (int)threadIdx.x < te);
  for (int tb = ts; tb < te; tb += VC_THREADS) {
    const float cx = nf.cx, cy = nf.cy, cz = nf.cz, xx = nf.xx, xy = nf.xy, xz = nf.xz, yx = nf.yx, yy = nf.yy,
                yz = nf.yz, invA = nf.invA, phi = nf.phi;
    const uint32_t wv = nf.wv;
    {
      const int tn = tb + VC_THREADS + (int)threadIdx.x;
      nf = load_frame(fr, total, (int64_t)t0 + tn, tn < te);
    }
    if (ARCS && narrow) {
      // Arc lengths are very uneven (a circle lying in the slab's layers keeps all its rotations, most keep a
      // handful, many none), so the wavefront's arcs are cut into quanta of VC_QUANTUM rotations (never straddling
      // the two arcs of a pair) and the quanta are dealt out evenly, 64 at a time (find_owner).
      ArcSet arcs = slab_arcs(cx, invA, phi, c0x, res, xl, xh, num_rots);
      arcs.a0 += (arcs.a0 < 0) ? num_rots : 0; arcs.a0 += (arcs.a0 < 0) ? num_rots : 0;
      arcs.a0 -= (arcs.a0 >= num_rots) ? num_rots : 0; arcs.a0 -= (arcs.a0 >= num_rots) ? num_rots : 0;
      arcs.a1 += (arcs.a1 < 0) ? num_rots : 0; arcs.a1 += (arcs.a1 < 0) ? num_rots : 0;
      arcs.a1 -= (arcs.a1 >= num_rots) ? num_rots : 0; arcs.a1 -= (arcs.a1 >= num_rots) ? num_rots : 0;
      const int nq0 = (arcs.n0 + VC_QUANTUM - 1) / VC_QUANTUM;
      const int nq = nq0 + (arcs.n1 + VC_QUANTUM - 1) / VC_QUANTUM;
      const int pk0 = arcs.a0 | (arcs.n0 << 10) | (nq0 << 21);       // a < 1024, n <= 1024, nq0 <= 1024
      const int pk1 = arcs.a1 | (arcs.n1 << 10);
      const int incl = wave_incl_scan_add(nq);
      const int excl = incl - nq;
      const int WQ = __builtin_amdgcn_readlane(incl, 63);
      for (int qb = 0; qb < WQ; qb += 64) {
#ifdef VC_DIAG
        ++nwin;
#endif
        // (issuing the lookup of window w + 1 before the votes of window w -- a depth-2 software pipeline -- was measured:
        // 125 VGPRs and 3 % slower; the four wavefronts per SIMD already cover the lookup's latency)
        const OwnerRegs cur = find_owner<WEIGHTED>(qb, WQ, incl, excl, nq, pk0, pk1, wv, cx, cy, cz, xx, xy, xz, yx, yy, yz,
                                                   lane, s_mark, tag);
        bool sure;
        QuantumCells q = vote_quantum(cur.cx, cur.cy, cur.cz, cur.xx, cur.xy, cur.xz, cur.yx, cur.yy, cur.yz, s_cos, s_sin,
                                      cur.rr, gf, base, sure);
        const int len = cur.len, rr = cur.rr;
        if (__builtin_expect(!sure && len > 0, 0)) {
          // rare (a coordinate within the rounding margin of a cell boundary): the reference's own arithmetic decides,
          // for the votes concerned only
#pragma unroll
          for (int jj = 0; jj < VC_QUANTUM; ++jj) {
            if (jj < len && !((q.fmin[jj] >= gf.lo_m) & (q.fmax[jj] <= gf.hi_m))) {
              const int lin = vote_cell_exact(cur.cx, cur.cy, cur.cz, cur.xx, cur.xy, cur.xz, cur.yx, cur.yy, cur.yz,
                                              s_cos[rr + jj], s_sin[rr + jj], c0x, c0y, c0z, res, gx, gy, gz);
              q.ok[jj] = lin >= 0;
              q.rel[jj] = (unsigned)(lin - lo);
            }
          }
        }
        const uint32_t owv = WEIGHTED ? cur.wv : 1u;
#pragma unroll
        for (int jj = 0; jj < VC_QUANTUM; ++jj)
          if (q.ok[jj] && jj < len && q.rel[jj] < (unsigned)n) atomicAdd(&slab[q.rel[jj]], owv);
      }
    } else if (cx == cx) {
      for (int r = 0; r < num_rots; ++r) {
        const int lin = vote_cell(cx, cy, cz, xx, xy, xz, yx, yy, yz, cos_tab[r], sin_tab[r], c0x, c0y, c0z, res, gx,
                                  gy, gz);
        const unsigned rel = (unsigned)(lin - lo);
        if (lin >= 0 && rel < (unsigned)n) atomicAdd(&slab[rel], wv);
      }
    }
  }
  __syncthreads();
  if (ARCS && narrow && lo < gyz) {
    // x-layer 0 is never a valid cell (train_dino.py:199 keeps indices > 0); the fast path clamps x instead of testing
    // it, so whatever landed there is wiped here (the layer may span several small slabs)
    for (int i = threadIdx.x; i < min(n, gyz - lo); i += VC_THREADS) slab[i] = 0u;
    __syncthreads();
  }
#ifdef VC_DIAG
  const long long t_b = wall_clock64();
#endif

  if (part != nullptr && Pl > 1) {
    // Persistent kernel with the pair list of an item split Pl ways (small batches: fewer slabs than CUs): every part adds
    // its non-zero cells to the zeroed merge area with device atomics and takes a ticket; the part holding the last
    // ticket reads the merged slab back and carries on to the arg-max.  No part waits for another one.
    __shared__ int s_ticket;
    uint32_t* pp = part + (int64_t)b * cells_cap + lo;
    for (int i = threadIdx.x; i < n; i += VC_THREADS) {
      const uint32_t c = slab[i];
      if (c) atomicAdd(&pp[i], c);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      __threadfence();
      s_ticket = atomicAdd(&tickets[(int64_t)b * s_max + s], 1);
      __threadfence();
    }
    __syncthreads();
    if (s_ticket != Pl - 1) return;
    for (int i = threadIdx.x; i < n; i += VC_THREADS)
      slab[i] = __hip_atomic_load(&pp[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
  }
  const int64_t goff = grid ? (grid_off ? grid_off[b] : (int64_t)b * cells_cap) : 0;
  if (P == 1) {
    uint32_t bv = 0;
    int64_t bi = INT64_MAX;
    for (int i = threadIdx.x; i < n; i += VC_THREADS) {
      const uint32_t c = slab[i];
      if (grid) grid[goff + lo + i] = c;
      argmax_combine(bv, bi, c, (int64_t)(lo + i));
    }
    wave_argmax(bv, bi);
    __shared__ uint32_t s_v[VC_THREADS / 64];
    __shared__ int64_t s_i[VC_THREADS / 64];
    if (wave_lane() == 0) { s_v[threadIdx.x >> 6] = bv; s_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < VC_THREADS / 64; ++w) argmax_combine(bv, bi, s_v[w], s_i[w]);
      SlabBest o; o.idx = bi; o.val = bv;
      o.pad = 0;
#ifdef VC_DIAG
      o.pad = (uint32_t)(wall_clock64() - t_start);     // item duration in 100 MHz ticks (scratch/vc_bench.py, DIAG=1)
      if (VC_DIAG == 1) o.pad = (uint32_t)(t_a - t_start);
      if (VC_DIAG == 2) o.pad = (uint32_t)(t_b - t_a);
      if (VC_DIAG == 3) o.pad = (uint32_t)(wall_clock64() - t_b);
      if (VC_DIAG == 4) o.pad = (uint32_t)nwin * 100;
#endif
      slab_best[(int64_t)b * s_max + s] = o;
    }
  } else {
    for (int i = threadIdx.x; i < n; i += VC_THREADS) {
      const uint32_t c = slab[i];
      if (c) atomicAdd(&grid[goff + lo + i], c);
    }
  }
}


// (scene, part, slab rank) -> one item per workgroup: small batches (pair lists split P ways, merged with global
// atomics) and the exhaustive A/B mode
// rotation tables into LDS, twice in a row (+4) so that the 4 rotations of a quantum never wrap; owner marks cleared
__device__ __forceinline__ void vote_stage_tables(uint32_t* slab, int num_rots, const float* __restrict__ cos_tab,
                                                  const float* __restrict__ sin_tab) {
  float* s_cos = reinterpret_cast<float*>(slab + VC_SLAB_CELLS);
  float* s_sin = s_cos + VC_TAB_LEN;
  for (int i = threadIdx.x; i < 2 * num_rots + 4; i += VC_THREADS) {
    const int r = i % num_rots;
    s_cos[i] = cos_tab[r];
    s_sin[i] = sin_tab[r];
  }
  slab[VC_SLAB_CELLS + 2 * VC_TAB_LEN + threadIdx.x] = 0u;
}

// (scene, part, slab rank) -> one item per workgroup: small batches (pair lists split P ways, merged with global
// atomics) and the exhaustive A/B mode
template <bool ARCS, bool WEIGHTED>
__global__ __launch_bounds__(VC_THREADS, VC_MIN_WAVES) void vote_center_slab_kernel(
    const float* __restrict__ fr, int64_t total, const int32_t* __restrict__ tup_off, float res, int num_rots,
    const float* __restrict__ cos_tab, const float* __restrict__ sin_tab, const CppfSceneGrid* __restrict__ grids,
    uint32_t* __restrict__ grid, const int64_t* __restrict__ grid_off, int64_t cells_cap,
    SlabBest* __restrict__ slab_best, int s_max, int P) {
  extern __shared__ __attribute__((aligned(16))) uint32_t slab[];
  int tag = 0;
  const int pc = blockIdx.y, rank = blockIdx.z;
  const int b = (blockIdx.x + rank) % gridDim.x;
  const CppfSceneGrid g = grids[b];
  const int G = ((int64_t)g.ncell <= cells_cap) ? g.ncell : 0;
  const int nslab = (G + VC_SLAB_CELLS - 1) / VC_SLAB_CELLS;
  if (rank >= nslab) return;
  // centre-out permutation of 0..nslab-1: mid, mid-1, mid+1, mid-2, ... (heavy central slabs dispatched first)
  const int mid = nslab >> 1, dd = (rank + 1) >> 1;
  const int s = (rank & 1) ? mid - dd : mid + dd;
  if (ARCS) vote_stage_tables(slab, num_rots, cos_tab, sin_tab);
  vote_slab_item<ARCS, WEIGHTED>(slab, tag, b, s, VC_SLAB_CELLS, pc, P, g, G, fr, total, tup_off, res, num_rots, cos_tab, sin_tab,
                                 grid, grid_off, cells_cap, slab_best, s_max, P, nullptr, nullptr);
}

// Work list of the persistent kernel: one entry (scene | slab << 16) per existing slab, in the order they should start
// -- slab rank (centre-out, heavy slabs first) outermost, scenes rotated by the rank.  One workgroup, block scans.
// (Halving the pair lists of the heavy slabs over two workgroups that merge through memory was built and measured:
// perfectly balanced CUs, but the extra zero / reduce / merge passes cost what the balance gained.)
__global__ __launch_bounds__(1024) void vote_worklist_kernel(const CppfSceneGrid* __restrict__ grids, int B,
                                                             int64_t cells_cap, int s_max, int max_parts, int target,
                                                             uint32_t* __restrict__ list, int* __restrict__ ctl) {
  __shared__ int s_wave[16];
  __shared__ int s_base, s_maxg, s_cells;
  __shared__ unsigned long long s_sumg;
  if (threadIdx.x == 0) { s_base = 0; s_maxg = 0; s_sumg = 0ull; }
  __syncthreads();
  // Cells per slab.  A throughput-sized batch of SMALL grids (64 objects of 8e4 cells: 2.2 LDS-sized slabs each = 170 items for
  // 256 CUs, the heavy central ones a third of a scene's votes) is cut finer than the LDS allows, so that the batch still
  // makes about `target` work items (two per CU): a slab is any run of consecutive flat cells, the arcs adapt to its
  // x-layers.  Never below VC_MIN_SLAB_CELLS (short arcs waste rotation quanta; every item streams its scene's frame list)
  // and never into more slabs than the per-scene partial-maximum table holds (s_max).  Batches small enough for the pair-list
  // split (max_parts > 1) keep LDS-sized slabs: equal parts of a slab balance better than unequal thin slabs (measured,
  // docs/measurements.md 11.6).
  int mx = 0;
  unsigned long long sm = 0ull;
  for (int b = threadIdx.x; b < B; b += 1024) {
    const int G = ((int64_t)grids[b].ncell <= cells_cap) ? grids[b].ncell : 0;
    mx = max(mx, G);
    sm += (unsigned long long)G;
  }
  if (mx > 0) { atomicMax(&s_maxg, mx); atomicAdd(&s_sumg, sm); }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t sc = max_parts > 1 ? (int64_t)VC_SLAB_CELLS : ((int64_t)s_sumg + target - 1) / max(target, 1);
    sc = max(sc, (int64_t)VC_MIN_SLAB_CELLS);
    sc = max(sc, ((int64_t)s_maxg + s_max - 1) / max(s_max, 1));
    sc = (sc + 255) / 256 * 256;
    s_cells = (int)min(sc, (int64_t)VC_SLAB_CELLS);
  }
  __syncthreads();
  const int slab_cells = s_cells;
  const int s_maxn = (s_maxg + slab_cells - 1) / slab_cells;       // slabs of the largest scene bound the ranks that exist
  const int64_t cand = (int64_t)B * min(s_maxn, s_max);             // (rank, scene slot) candidates, rank-major
  for (int64_t base = 0; base < cand; base += 1024) {
    const int64_t c = base + threadIdx.x;
    int cnt = 0, b = 0, s = 0;
    if (c < cand) {
      const int rank = (int)(c / B), x = (int)(c % B);
      b = (x + rank) % B;
      const int G = ((int64_t)grids[b].ncell <= cells_cap) ? grids[b].ncell : 0;
      const int nslab = (G + slab_cells - 1) / slab_cells;
      if (rank < nslab) {
        cnt = 1;
        const int mid = nslab >> 1, dd = (rank + 1) >> 1;
        s = (rank & 1) ? mid - dd : mid + dd;
      }
    }
    const int incl = wave_incl_scan_add(cnt);
    if (wave_lane() == 63) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    int off = s_base;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) off += s_wave[w];
    off += incl - cnt;
    if (cnt) list[off] = (uint32_t)b | ((uint32_t)s << 16);
    __syncthreads();
    if (threadIdx.x == 1023) s_base = off + cnt;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    // fewer slabs than `target` work items (about two per CU): split every slab's pair list into P parts
    const int items = s_base;
    int P = 1;
    if (max_parts > 1 && items > 0 && items < target) P = min(max_parts, (target + items - 1) / items);
    ctl[0] = 0; ctl[1] = items * P; ctl[2] = P;               // next work item, work item count, parts per slab
    ctl[3] = slab_cells;
  }
}

// Persistent form for throughput-sized batches: one workgroup per CU pulls (scene, slab) items from the work
// list -- no empty workgroups (the (scene, rank) launch has ~5 per real one, each needing a CU's whole LDS just to
// exit), list scheduling in the intended order regardless of the dispatcher, the table staged once per CU.
template <bool WEIGHTED>
__global__ __launch_bounds__(VC_THREADS, VC_MIN_WAVES) void vote_center_persist_kernel(
    const float* __restrict__ fr, int64_t total, const int32_t* __restrict__ tup_off, float res, int num_rots,
    const float* __restrict__ cos_tab, const float* __restrict__ sin_tab, const CppfSceneGrid* __restrict__ grids,
    uint32_t* __restrict__ grid, const int64_t* __restrict__ grid_off, int64_t cells_cap,
    SlabBest* __restrict__ slab_best, int s_max, const uint32_t* __restrict__ list, int* __restrict__ ctl,
    uint32_t* __restrict__ part, int* __restrict__ tickets) {
  extern __shared__ __attribute__((aligned(16))) uint32_t slab[];
  __shared__ int s_item;
  int tag = 0;
  vote_stage_tables(slab, num_rots, cos_tab, sin_tab);
  const int count = ctl[1], parts = ctl[2], slab_cells = ctl[3];
  for (;;) {
    __syncthreads();                                   // previous item's epilogue is done with the slab and s_item
    if (threadIdx.x == 0) s_item = atomicAdd(&ctl[0], 1);
    __syncthreads();
    const int item = s_item;
    if (item >= count) break;
    const uint32_t e = list[item / parts];                // the parts of a slab are consecutive work items
    const int b = (int)(e & 0xffffu), s = (int)(e >> 16);
    const CppfSceneGrid g = grids[b];
    vote_slab_item<true, WEIGHTED>(slab, tag, b, s, slab_cells, item % parts, parts, g, g.ncell, fr, total, tup_off, res, num_rots,
                                   cos_tab, sin_tab, grid, grid_off, cells_cap, slab_best, s_max, 1, part, tickets);
  }
}

__global__ __launch_bounds__(256) void vote_center_global_kernel(
    const float* __restrict__ pts, const int32_t* __restrict__ pt_off, const int32_t* __restrict__ idx, int k,
    const int32_t* __restrict__ tup_off, const float* __restrict__ tr, const float* __restrict__ vote_wt, float res,
    int num_rots, const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
    const CppfSceneGrid* __restrict__ grids, uint32_t* __restrict__ grid, const int64_t* __restrict__ grid_off,
    int64_t cells_cap) {
  const int b = blockIdx.y;
  const CppfSceneGrid g = grids[b];
  if ((int64_t)g.ncell > cells_cap || g.ncell <= 0) return;
  const float* p = pts + 3 * (int64_t)pt_off[b];
  const int t0 = tup_off[b], nt = tup_off[b + 1] - t0;
  uint32_t* gb = grid + (grid_off ? grid_off[b] : (int64_t)b * cells_cap);
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += gridDim.x * blockDim.x) {
    const int64_t row = (int64_t)(t0 + t);
    const VoteSetup v = vote_setup(p, idx[row * k], idx[row * k + 1], tr[row * 2], tr[row * 2 + 1], res);
    if (!v.ok) continue;
    const uint32_t wv = vote_weight(vote_wt, row);
    for (int r = 0; r < num_rots; ++r) {
      const int lin = vote_cell(v.cx, v.cy, v.cz, v.xx, v.xy, v.xz, v.yx, v.yy, v.yz, cos_tab[r], sin_tab[r],
                                g.c0[0], g.c0[1], g.c0[2], res, g.g[0], g.g[1], g.g[2]);
      if (lin >= 0) atomicAdd(&gb[lin], wv);
    }
  }
}

// first maximum of a uint32 grid, stage 1: VC_ARG_BLOCKS partials per scene
__global__ __launch_bounds__(256) void grid_argmax_partial_kernel(const uint32_t* __restrict__ grid,
                                                                  const int64_t* __restrict__ grid_off,
                                                                  int64_t cells_cap,
                                                                  const CppfSceneGrid* __restrict__ grids,
                                                                  SlabBest* __restrict__ partial, int s_max) {
  const int b = blockIdx.y;
  const int G = ((int64_t)grids[b].ncell <= cells_cap) ? grids[b].ncell : 0;
  const uint32_t* gb = grid + (grid_off ? grid_off[b] : (int64_t)b * cells_cap);
  const int per = (G + gridDim.x - 1) / gridDim.x;
  const int lo = blockIdx.x * per, hi = min(G, lo + per);
  uint32_t bv = 0;
  int64_t bi = INT64_MAX;
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) argmax_combine(bv, bi, gb[i], (int64_t)i);
  wave_argmax(bv, bi);
  __shared__ uint32_t s_v[4];
  __shared__ int64_t s_i[4];
  if (wave_lane() == 0) { s_v[threadIdx.x >> 6] = bv; s_i[threadIdx.x >> 6] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) argmax_combine(bv, bi, s_v[w], s_i[w]);
    SlabBest o; o.idx = bi; o.val = bv; o.pad = 0;
    partial[(int64_t)b * s_max + blockIdx.x] = o;
  }
}

// Cell (ix, iy, iz) of a flat C-order index of a scene's grid, and the cell's world coordinates (train_dino.py:212-213): the
// one definition grid_argmax_final_kernel and the grid_peaks kernels share, so that peak 0 of cppf_grid_peaks and the arg-max
// of cppf_vote_center cannot drift apart.
struct GridCell {
  int64_t ix, iy, iz;
};
__device__ __forceinline__ GridCell grid_unravel(const CppfSceneGrid& g, int64_t i) {
  const int64_t gyz = (int64_t)g.g[1] * g.g[2];
  GridCell c;
  c.ix = gyz > 0 ? i / gyz : 0;
  const int64_t rem = gyz > 0 ? i - c.ix * gyz : 0;
  c.iy = g.g[2] > 0 ? rem / g.g[2] : 0;
  c.iz = g.g[2] > 0 ? rem - c.iy * g.g[2] : 0;
  return c;
}
__device__ __forceinline__ void grid_cell_world(const CppfSceneGrid& g, int64_t i, double res, double* __restrict__ out) {
  const GridCell c = grid_unravel(g, i);
  out[0] = (double)g.c0[0] + (double)c.ix * res;
  out[1] = (double)g.c0[1] + (double)c.iy * res;
  out[2] = (double)g.c0[2] + (double)c.iz * res;
}

// stage 2: combine partials, unravel, world coordinates (train_dino.py:212-213)
__global__ __launch_bounds__(64) void grid_argmax_final_kernel(const SlabBest* __restrict__ partial, int s_max,
                                                               int fixed_parts, const int* __restrict__ ctl,
                                                               const CppfSceneGrid* __restrict__ grids,
                                                               int64_t cells_cap, double res,
                                                               int64_t* __restrict__ out_argmax,
                                                               uint32_t* __restrict__ out_peak,
                                                               double* __restrict__ out_world) {
  const int b = blockIdx.x;
  const CppfSceneGrid g = grids[b];
  const int G = ((int64_t)g.ncell <= cells_cap) ? g.ncell : 0;
  const int slab_cells = ctl ? ctl[3] : VC_SLAB_CELLS;        // the persistent kernel's work list chose the slab size
  const int parts = fixed_parts > 0 ? fixed_parts : (G + slab_cells - 1) / slab_cells;
  uint32_t bv = 0;
  int64_t bi = INT64_MAX;
  for (int i = threadIdx.x; i < parts; i += 64) {
    const SlabBest sb = partial[(int64_t)b * s_max + i];
    argmax_combine(bv, bi, sb.val, sb.idx);
  }
  wave_argmax(bv, bi);
  if (threadIdx.x == 0) {
    if (bi == INT64_MAX) bi = 0;
    out_argmax[b] = bi;
    // a scene whose grid exceeds cells_cap received no votes: its peak is the sentinel 0xFFFFFFFF
    if (out_peak) out_peak[b] = ((int64_t)g.ncell > cells_cap) ? 0xFFFFFFFFu : bv;
    if (out_world) grid_cell_world(g, bi, res, out_world + 3 * b);
  }
}

// ---- separated peaks of the vote grid: greedy non-maximum suppression, exact, integer arithmetic only ---------------------
// Per scene, on the uint32 grid cppf_vote_center wrote (G = ncell cells, C order; G = 0 for a scene above cells_cap):
//   peak 0 = the first maximum of the grid (largest value, lowest flat index on ties; index 0 for an all-zero grid or G = 0):
//            what grid_argmax_final_kernel reports;
//   peak k = the first maximum over the cells with a value > 0 that no earlier peak suppresses; a cell (ix, iy, iz) is
//            suppressed by a peak (px, py, pz) when (ix-px)^2 + (iy-py)^2 + (iz-pz)^2 <= sep_cells^2 (int64);
//   no cell left: the scene has run out of peaks (n_peaks = peaks found, at least 1).
// One masked first-maximum pass over the grid per peak (grid_peaks_pass_kernel, launched K times): pass k reads the k earlier
// peaks' cells into LDS, each thread keeps the largest 64-bit key (value << 32 | 0xFFFFFFFF - index) of its unsuppressed cells
// -- a larger key IS the first-maximum order, so the order of evaluation cannot matter --, the workgroup reduces its threads'
// keys and merges with one 64-bit atomic max into keys[b, k] (zeroed before pass 0).  An integer max is associative and
// commutative: the atomics cannot affect the result, and a scene's keys do not depend on the batch.  A cell is unravelled and
// tested against the earlier peaks only when its key beats the thread's best so far.  Key 0 = no peak (every real key has a
// value > 0).  grid_peaks_final_kernel turns the keys into the outputs.
#define GP_MAX_K 16
#define GP_THREADS 256

__device__ __forceinline__ uint32_t grid_peak_index(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t)key; }

__global__ __launch_bounds__(GP_THREADS) void grid_peaks_pass_kernel(const uint32_t* __restrict__ grid,
                                                                     const int64_t* __restrict__ grid_off, int64_t cells_cap,
                                                                     const CppfSceneGrid* __restrict__ grids,
                                                                     unsigned long long* __restrict__ keys, int K, int k,
                                                                     long long sep2) {
  const int b = blockIdx.y;
  const CppfSceneGrid g = grids[b];
  const int G = ((int64_t)g.ncell <= cells_cap) ? g.ncell : 0;
  if (G <= 0) return;
  unsigned long long* kb = keys + (int64_t)b * K;
  __shared__ int s_p[GP_MAX_K * 3];
  __shared__ int s_stop;
  __shared__ unsigned long long s_w[GP_THREADS / 64];
  if (threadIdx.x == 0) s_stop = 0;
  __syncthreads();
  if ((int)threadIdx.x < k) {                     // the earlier passes' keys are final: they were written by earlier launches
    const unsigned long long pk = kb[threadIdx.x];
    if (pk == 0ull) {
      s_stop = 1;                                 // the scene ran out of peaks before this pass
    } else {
      const GridCell c = grid_unravel(g, (int64_t)grid_peak_index(pk));
      s_p[3 * threadIdx.x + 0] = (int)c.ix;
      s_p[3 * threadIdx.x + 1] = (int)c.iy;
      s_p[3 * threadIdx.x + 2] = (int)c.iz;
    }
  }
  __syncthreads();
  if (s_stop) return;
  const uint32_t* gb = grid + (grid_off ? grid_off[b] : (int64_t)b * cells_cap);
  const uint32_t gz = (uint32_t)g.g[2], gyz = (uint32_t)g.g[1] * (uint32_t)g.g[2];
  unsigned long long best = 0ull;
  auto consider = [&](uint32_t v, int i) {
    const unsigned long long key = ((unsigned long long)v << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
    if (v == 0u || key <= best) return;
    if (k > 0) {
      const uint32_t ix = (uint32_t)i / gyz, rem = (uint32_t)i - ix * gyz, iy = rem / gz, iz = rem - iy * gz;
      for (int j = 0; j < k; ++j) {               // k is uniform: LDS broadcast reads
        const long long dx = (long long)ix - s_p[3 * j], dy = (long long)iy - s_p[3 * j + 1], dz = (long long)iz - s_p[3 * j + 2];
        if (dx * dx + dy * dy + dz * dz <= sep2) return;
      }
    }
    best = key;
  };
  // 16-byte loads over the aligned body of the scene's range; the (< 4)-cell head and tail go to workgroup 0
  const int head = min(G, (int)((0u - (uint32_t)((uintptr_t)gb >> 2)) & 3u));
  const int nvec = (G - head) >> 2;
  const uint4* gv = (const uint4*)(gb + head);
  for (int v = blockIdx.x * GP_THREADS + threadIdx.x; v < nvec; v += gridDim.x * GP_THREADS) {
    const uint4 q = gv[v];
    const int i0 = head + 4 * v;
    consider(q.x, i0);
    consider(q.y, i0 + 1);
    consider(q.z, i0 + 2);
    consider(q.w, i0 + 3);
  }
  if (blockIdx.x == 0 && threadIdx.x < 4) {
    if ((int)threadIdx.x < head) consider(gb[threadIdx.x], (int)threadIdx.x);
    const int t = head + 4 * nvec + (int)threadIdx.x;
    if (t < G) consider(gb[t], t);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(best, off);
    best = o > best ? o : best;
  }
  if (wave_lane() == 0) s_w[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < GP_THREADS / 64; ++w) best = s_w[w] > best ? s_w[w] : best;
    if (best != 0ull) atomicMax(&kb[k], best);
  }
}

// keys -> peak_idx int64[B,K], peak_val uint32[B,K], peak_world float64[B,K,3], n_peaks int32[B]; one wavefront per scene
__global__ __launch_bounds__(64) void grid_peaks_final_kernel(const unsigned long long* __restrict__ keys, int K,
                                                              const CppfSceneGrid* __restrict__ grids, int64_t cells_cap,
                                                              double res, int64_t* __restrict__ peak_idx,
                                                              uint32_t* __restrict__ peak_val, double* __restrict__ peak_world,
                                                              int32_t* __restrict__ n_peaks) {
  const int b = blockIdx.x, t = threadIdx.x;
  const CppfSceneGrid g = grids[b];
  const bool over = (int64_t)g.ncell > cells_cap;
  const unsigned long long key = (t < K && !over && g.ncell > 0) ? keys[(int64_t)b * K + t] : 0ull;
  const int found = __popcll(wave_ballot(key != 0ull));       // the non-zero keys are the leading ones (a pass stops at a gap)
  if (t == 0 && n_peaks) n_peaks[b] = max(found, 1);
  if (t >= K) return;
  const int64_t o = (int64_t)b * K + t;
  if (t == 0 || key != 0ull) {
    // peak 0 always exists: index 0 / value 0 for an all-zero grid; a scene above cells_cap received no votes and carries
    // cppf_vote_center's sentinel
    const int64_t i = key != 0ull ? (int64_t)grid_peak_index(key) : 0;
    peak_idx[o] = i;
    if (peak_val) peak_val[o] = over ? 0xFFFFFFFFu : (uint32_t)(key >> 32);
    if (peak_world) grid_cell_world(g, i, res, peak_world + 3 * o);
  } else {
    peak_idx[o] = -1;
    if (peak_val) peak_val[o] = 0u;
    if (peak_world) {
      const double nan = __longlong_as_double(0x7ff8000000000000ll);
      peak_world[3 * o + 0] = nan;
      peak_world[3 * o + 1] = nan;
      peak_world[3 * o + 2] = nan;
    }
  }
}

// zero the caller's grid ranges (offsets live on the device)
__global__ __launch_bounds__(256) void grid_zero_kernel(uint32_t* __restrict__ grid,
                                                        const int64_t* __restrict__ grid_off, int64_t cells_cap,
                                                        const CppfSceneGrid* __restrict__ grids) {
  const int b = blockIdx.y;
  const int G = ((int64_t)grids[b].ncell <= cells_cap) ? grids[b].ncell : 0;
  uint32_t* gb = grid + (grid_off ? grid_off[b] : (int64_t)b * cells_cap);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < G; i += gridDim.x * blockDim.x) gb[i] = 0u;
}

// slabs of a grid of cells_cap cells, and at least VC_ARG_BLOCKS: entries per scene of the partial-maximum table
static inline int vc_parts(int64_t cells_cap) {
  return (int)std::max<int64_t>((cells_cap + VC_SLAB_CELLS - 1) / VC_SLAB_CELLS, VC_ARG_BLOCKS);
}

// Byte offsets of the workspace.  best: the partial-maximum table; ctl, list: the persistent kernel's control words (next item,
// item count, parts per slab, slab cells) and work list; tickets: one arrival counter per (scene, slab) of the pair-split merge;
// grid: the merge area, or the accumulator when the caller passes no grid; frames: the per-pair circle frames.
struct VcLayout {
  int64_t best, ctl, list, tickets, grid, frames, bytes;
};

static VcLayout vc_layout(int B, int64_t cells_cap, int64_t total_tuples) {
  const int64_t parts = (int64_t)B * vc_parts(cells_cap);
  VcLayout L;
  L.best = 0;
  L.ctl = L.best + align_up(parts * (int64_t)sizeof(SlabBest), 256);
  L.list = L.ctl + 256;
  L.tickets = L.ctl + align_up(parts * 4 + 256, 256);
  L.grid = L.tickets + align_up(parts * 4, 256);
  L.frames = L.grid + align_up((int64_t)B * cells_cap * 4, 256);
  L.bytes = L.frames + align_up(total_tuples * VC_FRAME_FLOATS * 4, 256);
  return L;
}

extern "C" int64_t cppf_vote_center_workspace_bytes(int B, int64_t cells_cap, int64_t total_tuples) {
  if (B <= 0 || cells_cap <= 0 || total_tuples < 0) return 0;
  return vc_layout(B, cells_cap, total_tuples).bytes;
}

// mode bit: the arcs path launches one (scene, slab) item per workgroup (vote_center_slab_kernel), not the persistent kernel
constexpr int VC_MODE_NO_PERSIST = 0x800;

enum VcPath { VC_PERSIST, VC_SLAB, VC_GLOBAL };

// Every launch decision of one call, taken before any launch.  P: VC_SLAB splits each slab's pair list P ways, merged with
// atomics into a zeroed grid.  max_parts: the most parts VC_PERSIST's work-list kernel may split a slab into (> 1 costs a zeroed
// merge area and tickets).  prepare / vote: the halves of the two-call form this call runs.
struct VcPlan {
  VcPath path;
  bool arcs, weighted, prepare, vote;
  int P, max_parts, s_max, s_max_parts;
};

static int vc_plan(int mode, int B, int max_t, int num_rots, int64_t cells_cap, bool weighted, VcPlan* p) {
  const int s_max = (int)((cells_cap + VC_SLAB_CELLS - 1) / VC_SLAB_CELLS);
  int m = mode & 0xff;
  if (m == 0) m = (s_max <= 64) ? 1 : 2;
  if (max_t <= 0) m = 2;
  if (m < 1 || m > 3) {
    snprintf(g_cppf_err, sizeof(g_cppf_err), "cppf_vote_center: unknown mode %d", m);
    return CPPF_EINVAL;
  }
  // arcs need >1 slab to pay off and the table in LDS; mode 3 is the exhaustive sweep (A/B reference).  The persistent work-list
  // kernel serves every batch size of the arcs path; the one-item-per-workgroup launch remains for mode 3 and on request.
  const bool arcs = m == 1 && s_max > 1 && num_rots <= VC_MAX_LDS_ROTS && num_rots >= 8;
  const bool persist = arcs && B <= 0xffff && s_max <= 0xffff && !(mode & VC_MODE_NO_PERSIST);
  // two-call form (lets a caller put events around the vote kernel alone): CPPF_VC_FRAMES_ONLY runs the preparation (frames,
  // work list) and returns, CPPF_VC_FRAMES_READY skips it; the global path ignores both bits
  *p = VcPlan{m == 2 ? VC_GLOBAL : persist ? VC_PERSIST : VC_SLAB, arcs, weighted, m == 2 || !(mode & CPPF_VC_FRAMES_READY),
              m == 2 || !(mode & CPPF_VC_FRAMES_ONLY), 1, 1, s_max, vc_parts(cells_cap)};
  // Small batches may have fewer slabs than CUs.  How many is only known on the device (scene bounds), so the persistent path's
  // work-list kernel picks the parts per slab; the host only bounds them (parts of at least VC_THREADS pairs).  The slab path
  // splits when its (scene, slab) workgroups cannot fill 256 CUs.
  const int pmax_t = (max_t + VC_THREADS - 1) / VC_THREADS;
  const int64_t wgs = (int64_t)B * s_max;
  if (persist && B <= 48) p->max_parts = std::min(pmax_t, 64);
  if (p->path == VC_SLAB && wgs < 256) p->P = (int)std::min<int64_t>((256 + wgs - 1) / wgs, pmax_t);
  return CPPF_OK;
}

extern "C" int cppf_vote_center(int B, const float* pts, const int32_t* pt_off, const int32_t* idx, int k,
                                const int32_t* tup_off, int max_t, int64_t total_tuples, const float* tr,
                                const float* vote_wt, double res, int num_rots, const float* cos_tab, const float* sin_tab, const CppfSceneGrid* grids,
                                uint32_t* grid, const int64_t* grid_off, int64_t cells_cap, int mode,
                                void* workspace, int64_t workspace_bytes, int64_t* out_argmax, uint32_t* out_peak,
                                double* out_world, void* stream) {
  CPPF_CHECK_ARG(B > 0 && pts && pt_off && idx && tup_off && tr && cos_tab && sin_tab && grids && out_argmax);
  CPPF_CHECK_ARG(k >= 2 && num_rots > 0 && res > 0.0 && cells_cap > 0 && cells_cap <= 0x7fffffffLL);
  CPPF_CHECK_ARG(total_tuples >= 0 && max_t >= 0 && (int64_t)max_t <= total_tuples);
  const VcLayout L = vc_layout(B, cells_cap, total_tuples);
  CPPF_CHECK_ARG(workspace && workspace_bytes >= L.bytes);
  CPPF_CHECK_ARG(grid == nullptr || grid_off != nullptr);
  VcPlan p;
  CPPF_TRY(vc_plan(mode, B, max_t, num_rots, cells_cap, vote_wt != nullptr, &p));
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  SlabBest* best = (SlabBest*)(ws + L.best);
  int *ctl = (int*)(ws + L.ctl), *tickets = (int*)(ws + L.tickets);
  uint32_t *list = (uint32_t*)(ws + L.list), *ws_grid = (uint32_t*)(ws + L.grid);
  float* frames = (float*)(ws + L.frames);
  const float res32 = (float)res;
  const int lds_bytes = VC_LDS_WORDS * 4;
  int dev = 0, num_cus = 0;
  if (p.path != VC_GLOBAL) {
    // per device, on first use: the kernels' dynamic-LDS limit (cppf_common.h)
    CPPF_TRY(cppf_device_cus(&dev, &num_cus));
    const void* fns[] = {(const void*)vote_center_slab_kernel<true, false>, (const void*)vote_center_slab_kernel<true, true>,
                         (const void*)vote_center_slab_kernel<false, false>, (const void*)vote_center_slab_kernel<false, true>,
                         (const void*)vote_center_persist_kernel<false>, (const void*)vote_center_persist_kernel<true>};
    for (const void* f : fns) CPPF_TRY(cppf_allow_dynamic_lds(f, dev, lds_bytes));
  }
  // The global path and a split slab path merge with atomics into a zeroed grid: the caller's, else the workspace's.  Both calls
  // of the two-call form zero it.
  const bool merge = p.path == VC_GLOBAL || p.P > 1;
  uint32_t* target = (merge && !grid) ? ws_grid : grid;
  const int64_t* target_off = (merge && !grid) ? nullptr : grid_off;
  if (merge) {
    hipLaunchKernelGGL(grid_zero_kernel, dim3(64, B), dim3(256), 0, st, target, target_off, cells_cap, grids);
    CPPF_LAUNCH_CHECK();
  }
  if (p.prepare && p.path != VC_GLOBAL) {
    hipLaunchKernelGGL(vote_frames_kernel, dim3((max_t + 255) / 256, B), dim3(256), 0, st, pts, pt_off, idx, k, tup_off, tr, vote_wt,
                       res32, num_rots, total_tuples, frames);
    if (p.path == VC_PERSIST) {
      hipLaunchKernelGGL(vote_worklist_kernel, dim3(1), dim3(1024), 0, st, grids, B, cells_cap, p.s_max_parts, p.max_parts,
                         2 * num_cus, list, ctl);
      if (p.max_parts > 1) {
        hipLaunchKernelGGL(grid_zero_kernel, dim3(64, B), dim3(256), 0, st, ws_grid, (const int64_t*)nullptr, cells_cap, grids);
        CPPF_HIP(hipMemsetAsync(tickets, 0, (size_t)B * p.s_max_parts * 4, st));
      }
    }
    CPPF_LAUNCH_CHECK();
  }
  if (!p.vote) return CPPF_OK;
  if (p.path == VC_PERSIST)
    hipLaunchKernelGGL((p.weighted ? vote_center_persist_kernel<true> : vote_center_persist_kernel<false>), dim3(num_cus),
                       dim3(VC_THREADS), lds_bytes, st, frames, total_tuples, tup_off, res32, num_rots, cos_tab, sin_tab, grids, grid,
                       grid_off, cells_cap, best, p.s_max_parts, list, ctl, p.max_parts > 1 ? ws_grid : nullptr, tickets);
  else if (p.path == VC_SLAB)
    hipLaunchKernelGGL((p.arcs ? (p.weighted ? vote_center_slab_kernel<true, true> : vote_center_slab_kernel<true, false>)
                               : (p.weighted ? vote_center_slab_kernel<false, true> : vote_center_slab_kernel<false, false>)),
                       dim3(B, p.P, p.s_max), dim3(VC_THREADS), lds_bytes, st, frames, total_tuples, tup_off, res32, num_rots, cos_tab,
                       sin_tab, grids, target, target_off, cells_cap, best, p.s_max_parts, p.P);
  else if (max_t > 0)
    hipLaunchKernelGGL(vote_center_global_kernel, dim3((max_t + 255) / 256, B), dim3(256), 0, st, pts, pt_off, idx, k, tup_off, tr,
                       vote_wt, res32, num_rots, cos_tab, sin_tab, grids, target, target_off, cells_cap);
  CPPF_LAUNCH_CHECK();
  // first maximum: of the per-slab maxima the vote kernel left or, after an atomic merge, of a pass over the grid
  if (merge)
    hipLaunchKernelGGL(grid_argmax_partial_kernel, dim3(VC_ARG_BLOCKS, B), dim3(256), 0, st, target, target_off, cells_cap, grids,
                       best, p.s_max_parts);
  hipLaunchKernelGGL(grid_argmax_final_kernel, dim3(B), dim3(64), 0, st, best, p.s_max_parts, merge ? VC_ARG_BLOCKS : 0,
                     p.path == VC_PERSIST ? ctl : nullptr, grids, cells_cap, res, out_argmax, out_peak, out_world);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}

// workspace of cppf_grid_peaks: the 64-bit keys, one per (scene, peak)
extern "C" int64_t cppf_grid_peaks_workspace_bytes(int B, int K) {
  if (B <= 0 || K < 1 || K > GP_MAX_K) return 0;
  return align_up((int64_t)B * K * 8, 256);
}

extern "C" int cppf_grid_peaks(int B, const CppfSceneGrid* grids, const uint32_t* grid, const int64_t* grid_off,
                               int64_t cells_cap, double res, int K, int sep_cells, int64_t* peak_idx, uint32_t* peak_val,
                               double* peak_world, int32_t* n_peaks, void* workspace, int64_t workspace_bytes, void* stream) {
  CPPF_CHECK_ARG(B > 0 && B <= 0xffff && grids && grid && peak_idx);
  CPPF_CHECK_ARG(K >= 1 && K <= GP_MAX_K && sep_cells >= 0 && res > 0.0 && cells_cap > 0 && cells_cap <= 0x7fffffffLL);
  const int64_t need = cppf_grid_peaks_workspace_bytes(B, K);
  CPPF_CHECK_ARG(workspace && workspace_bytes >= need);
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)workspace;
  CPPF_HIP(hipMemsetAsync(keys, 0, (size_t)B * K * 8, st));
  // 16 cells per thread and round of the grid-stride loop; at most ~8192 workgroups per pass
  int nbx = (int)std::min<int64_t>(std::max<int64_t>((cells_cap + GP_THREADS * 16 - 1) / (GP_THREADS * 16), 1), 256);
  if ((int64_t)nbx * B > 8192) nbx = std::max(1, 8192 / B);
  const long long sep2 = (long long)sep_cells * sep_cells;
  for (int k = 0; k < K; ++k)
    hipLaunchKernelGGL(grid_peaks_pass_kernel, dim3(nbx, B), dim3(GP_THREADS), 0, st, grid, grid_off, cells_cap, grids, keys, K, k,
                       sep2);
  hipLaunchKernelGGL(grid_peaks_final_kernel, dim3(B), dim3(64), 0, st, keys, K, grids, cells_cap, res, peak_idx, peak_val,
                     peak_world, n_peaks);
  CPPF_LAUNCH_CHECK();
  return CPPF_OK;
}
