// The label-equivalence union-find that cppf_mask.hip's cc_* kernels (4-connected pixels) and cppf_close.hip's close_* kernels
// (6-connected volume nodes) share.  L[x] is x's parent, always <= x (so there are no cycles), a root has L[x] == x, a word that
// takes no part is negative and never changes sign after the launch that wrote it.  Every access of a word that another
// workgroup may change in the same launch is an agent-scope atomic: plain loads are served by the CU's L1 and are not coherent
// across XCDs within a launch.  How the merge launch uses them is stated in cppf_mask.hip's header under "merge".
#pragma once
#include "cppf_common.h"

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's tree as far as this lane sees it; x's own word is lowered to it
__device__ __forceinline__ int cc_find(int* __restrict__ L, int x) {
  int r = x, p;
  while ((p = cc_load(L + r)) != r) r = p;
  if (r != x) atomicMin(L + x, r);
  return r;
}

__device__ __forceinline__ void cc_union(int* __restrict__ L, int a, int b) {
  a = cc_find(L, a);
  b = cc_find(L, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }         // a > b: lower a's word to b
    const int old = atomicMin(L + a, b);
    if (old == a) break;                                  // a was a root: linked
    a = cc_find(L, old);                                  // it was not: what it held (< a) still has to meet b
    b = cc_find(L, b);
  }
}
