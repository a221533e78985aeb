// diverse_math.h - the arithmetic of diverse-of-K IK (diverse_kernels.hip; the definition: include/ikflow_amd_diverse.h): the squared joint
// distance of two candidate rows, the update of a candidate's distance to the kept set, the two orders (slot 0: lowest score; every later
// slot: farthest from the kept set) with their "best so far" pairs and merges, the stop rule, and the launch geometry.  Like rank_math.h and
// path_math.h it holds nothing of the HIP runtime, so the same source compiles with g++: tests/test_diverse_math_host.py runs it on the CPU
// against sequential numpy float32 arithmetic and against brute force over all subsets.
//
// Rounding: every function that adds or multiplies is compiled without contraction (#pragma clang fp contract(off), as path_math.h), so
// dist2 is a subtract, [a multiply by the weight,] a multiply and an add per joint in source order.  Given the row scores, the selection is
// therefore a function of its inputs alone, not of the compiler.
#pragma once
#include <cstddef>

#include "rank_math.h"
#include "../../include/ikflow_amd_diverse.h"

#if defined(__HIPCC__)
#define IKF_DIVERSE_HOST_DEVICE __host__ __device__ inline
#else
#define IKF_DIVERSE_HOST_DEVICE inline
#endif

namespace ikf {

constexpr int IKF_DIVERSE_MIN_BLOCK = 64;    // threads of the select workgroup: one wave ...
constexpr int IKF_DIVERSE_MAX_BLOCK = 256;   // ... to four
constexpr int IKF_DIVERSE_PER_THREAD = 4;    // candidates a thread owns at most (their near2 stay in registers)
static_assert(IKF_DIVERSE_MAX_K <= IKF_DIVERSE_MAX_BLOCK * IKF_DIVERSE_PER_THREAD, "every candidate needs an owner");
static_assert(IKF_DIVERSE_MAX_KEEP <= IKF_RANK_MAX_KEEP, "slot 0 is the ranking's first choice");

// dist2(a, b); w: the joint weights, or null
template <int NDOF>
IKF_HD float diverse_dist2(const float* a, const float* b, const float* w) {
#pragma clang fp contract(off)
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NDOF; ++j) {
    float d = a[j] - b[j];
    if (w) d = d * w[j];
    s = s + d * d;
  }
  return s;
}
// near2 of a candidate after one more row was kept at squared distance d2 (a NaN d2 leaves it as it is)
IKF_HD float diverse_near2(float near2, float d2) { return d2 < near2 ? d2 : near2; }
IKF_HD float diverse_sep2(float min_separation) {
#pragma clang fp contract(off)
  return min_separation * min_separation;
}

// Slot 0: the best candidate found so far in the order (lower score, then lower r).  Empty: (+inf, INT32_MAX); a score that is not below
// +inf is never offered.
struct DiverseFirst {
  float s;
  int r;
};
IKF_HD DiverseFirst diverse_first_none() { return DiverseFirst{rank_inf(), 0x7fffffff}; }
IKF_HD void diverse_first_offer(DiverseFirst& b, float score, int r) {
  if (!(score < rank_inf())) return;
  if (score < b.s || (score == b.s && r < b.r)) { b.s = score; b.r = r; }
}
IKF_HD void diverse_first_merge(DiverseFirst& a, const DiverseFirst& o) { diverse_first_offer(a, o.s, o.r); }

// Slot i >= 1: the best candidate found so far in the order (greater near2, then lower r).  Empty: (-1, INT32_MAX) - a near2 is never
// negative, so every offer beats it, and a NaN near2 beats nothing.  Both orders are strict and total, so a pose's pick does not depend on
// how its candidates are split over threads or in which order the parts are merged.
struct DiverseBest {
  float n;
  int r;
};
IKF_HD DiverseBest diverse_none() { return DiverseBest{-1.f, 0x7fffffff}; }
IKF_HD void diverse_offer(DiverseBest& b, float near2, int r) {
  if (near2 > b.n || (near2 == b.n && r < b.r)) { b.n = near2; b.r = r; }
}
IKF_HD void diverse_merge(DiverseBest& a, const DiverseBest& o) {
  if (o.r != 0x7fffffff) diverse_offer(a, o.n, o.r);
}
// the stop rule of a slot i >= 1: nothing left, or the farthest candidate is not min_separation away from the kept set
IKF_HD bool diverse_stop(const DiverseBest& b, float sep2) { return b.r == 0x7fffffff || !(b.n >= sep2); }

// ---- the launch geometry, pure integer arithmetic; the kernel derives its roles from the same function --------------
// threads of a pose's workgroup: the least power of two in 64 .. 256 that leaves a thread at most IKF_DIVERSE_PER_THREAD candidates
IKF_DIVERSE_HOST_DEVICE int diverse_block(int k) {
  int b = IKF_DIVERSE_MIN_BLOCK;
  while (b < IKF_DIVERSE_MAX_BLOCK && b * IKF_DIVERSE_PER_THREAD < k) b <<= 1;
  return b;
}
// floats of a candidate row in LDS: odd, so that lanes reading the same joint of consecutive rows hit different banks
IKF_DIVERSE_HOST_DEVICE int diverse_row_stride(int ndof) { return ndof | 1; }
// dynamic LDS of a pose's workgroup: its k rows and their scores
inline size_t diverse_lds_bytes(int ndof, int k) { return sizeof(float) * ((size_t)k * diverse_row_stride(ndof) + (size_t)k); }

}  // namespace ikf
