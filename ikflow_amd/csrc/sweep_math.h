// sweep_math.h - the arithmetic of swept collision checks along edges (sweep_kernels.hip; the definitions: include/ikflow_amd_sweep.h): the
// sample configurations between two rows, the verdict of one edge (its first blocked sample) from capsule_endpoints / capsule_clearance
// (rank_math.h) and world_clearance (world_math.h) unchanged, and the geometry of the lattice's "edge free" mask.  Like world_math.h it holds
// nothing of the HIP runtime, so the same source compiles with g++: tests/test_sweep_math_host.py runs it on the CPU against sequential numpy
// float32 (the samples, bit for bit) and an fp64 reference (the verdicts).
//
// Rounding: sweep_sample is compiled without contraction (#pragma clang fp contract(off), as path_math.h), so a sample is one division, one
// subtraction, one multiplication and one addition per joint, each rounded on its own.
#pragma once
#include "world_math.h"
#include "../../include/ikflow_amd_sweep.h"

#if defined(__HIPCC__)
#define IKF_SWEEP_HOST_DEVICE __host__ __device__ inline
#else
#define IKF_SWEEP_HOST_DEVICE inline
#endif

namespace ikf {

// sample i = 1 .. S of the edge a -> b: q_out[j] = a[j] + f * (b[j] - a[j]), f = (float)i / (float)(S + 1)
template <int NDOF>
IKF_HD void sweep_sample(const float* a, const float* b, int i, int S, float* q_out) {
#pragma clang fp contract(off)
  const float f = (float)i / (float)(S + 1);
#pragma unroll
  for (int j = 0; j < NDOF; ++j) {
    const float d = b[j] - a[j];
    const float p = f * d;
    q_out[j] = a[j] + p;
  }
}

// The first blocked sample (0-based) of the edge a -> b, -1 when the edge is free.  Samples in ascending order, stopping at the first blocked
// one.  Self rule (reject_self): capsule_clearance < self_min; world rule (n_obs > 0): world_clearance < world_min - on the end points the
// self rule's chain walk has left in w when it ran, as rank_row_score_world does.  w: 6 floats per capsule, owned by the caller.
template <int NDOF>
IKF_HD int sweep_edge(const Chain* __restrict__ ch, const CollisionModel* __restrict__ cm, const WorldObstacle* obs, int n_obs, float world_min,
                      bool reject_self, float self_min, const float* a, const float* b, int S, float* w) {
  for (int i = 1; i <= S; ++i) {
    float qv[NDOF];
    sweep_sample<NDOF>(a, b, i, S, qv);
    bool blocked = false;
    if (reject_self) blocked = capsule_clearance<NDOF>(ch, cm, qv, w) < self_min;
    if (!blocked && n_obs > 0) {
      if (!reject_self) capsule_endpoints<NDOF>(ch, cm, qv, w);
      blocked = world_clearance(obs, n_obs, cm, w).clearance < world_min;
    }
    if (blocked) return i - 1;
  }
  return -1;
}

// ---- the "edge free" mask of a T x k lattice, pure integer arithmetic -------------------------------------------------
// edge_free[t][r][word]: bit j of word j / 64 is set when the edge from candidate j of waypoint t - 1 to candidate r of waypoint t may be taken
// as far as the sweep is concerned; row t = 0 carries the start edge q_start -> q[0][r] in bit 0 of word 0.  One wave of the sweep kernel
// produces one word; the lattice kernel reads the words of its destination.
constexpr int IKF_SWEEP_LANES = 64;
IKF_SWEEP_HOST_DEVICE int sweep_words(int k) { return (k + IKF_SWEEP_LANES - 1) / IKF_SWEEP_LANES; }
IKF_SWEEP_HOST_DEVICE long long sweep_mask_words(long long T, int k) { return T * k * sweep_words(k); }
IKF_SWEEP_HOST_DEVICE long long sweep_word_index(long long t, int r, int word, int k) { return (t * k + r) * sweep_words(k) + word; }
// wave `wave` of the lattice source -> its waypoint, destination and block of 64 predecessors (the inverse of sweep_word_index)
IKF_SWEEP_HOST_DEVICE void sweep_wave_role(long long wave, int k, long long* t, int* r, int* word) {
  const int words = sweep_words(k);
  *word = (int)(wave % words);
  const long long node = wave / words;
  *r = (int)(node % k);
  *t = node / k;
}
// the lanes of word `word` that stand for a predecessor j < k
IKF_SWEEP_HOST_DEVICE unsigned long long sweep_live_lanes(int k, int word) {
  const int left = k - word * IKF_SWEEP_LANES;
  return left >= IKF_SWEEP_LANES ? ~0ULL : left <= 0 ? 0ULL : (1ULL << left) - 1ULL;
}
IKF_SWEEP_HOST_DEVICE bool sweep_bit(const unsigned long long* words_of_destination, int j) {
  return (words_of_destination[j / IKF_SWEEP_LANES] >> (j % IKF_SWEEP_LANES)) & 1ULL;
}
// waves of the pair source: a lane per edge
IKF_SWEEP_HOST_DEVICE long long sweep_pair_waves(long long n) { return (n + IKF_SWEEP_LANES - 1) / IKF_SWEEP_LANES; }

}  // namespace ikf
