// rank_math.h - the per-row and per-pose arithmetic of best-of-K ranking (rank_kernels.hip): the capsule clearance of a configuration (shared
// with k_self_collision), the score and admissibility of a candidate row, and the fixed-capacity sorted list that selects a pose's best
// candidates.  Like kin_math.h it holds nothing of the HIP runtime, so the same source compiles with g++: tests/test_rank_math_host.py runs it
// on the CPU against the oracle and against numpy.  The product only ever runs it on the GPU.
#pragma once
#include "kin_math.h"
#include "../../include/ikflow_amd_rank.h"

namespace ikf {

// IKF_MAX_CAPSULES (24) comes from include/ikflow_amd.h
constexpr int IKF_MAX_CAPSULE_PAIRS = IKF_MAX_CAPSULES * (IKF_MAX_CAPSULES - 1) / 2;
struct CollisionModel {
  int n_caps, n_pairs;
  int frame[IKF_MAX_CAPSULES];      // 0 = base, j + 1 = the frame that follows actuated joint j
  float p0[IKF_MAX_CAPSULES][3], p1[IKF_MAX_CAPSULES][3], radius[IKF_MAX_CAPSULES];
  uint8_t pair_a[IKF_MAX_CAPSULE_PAIRS], pair_b[IKF_MAX_CAPSULE_PAIRS];
};

// closest points of two segments after Ericson, "Real-Time Collision Detection", 5.1.9
IKF_HD float segment_segment_dist(const float* p1, const float* q1, const float* p2, const float* q2) {
  const float d1[3] = {q1[0] - p1[0], q1[1] - p1[1], q1[2] - p1[2]};
  const float d2[3] = {q2[0] - p2[0], q2[1] - p2[1], q2[2] - p2[2]};
  const float r[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};
  const float a = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2];
  const float e = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2];
  const float f = d2[0] * r[0] + d2[1] * r[1] + d2[2] * r[2];
  const float EPS = 1e-12f;
  float sN, tN;
  if (a <= EPS && e <= EPS) {
    sN = 0.f; tN = 0.f;
  } else if (a <= EPS) {
    sN = 0.f; tN = fminf(fmaxf(f / e, 0.f), 1.f);
  } else {
    const float c = d1[0] * r[0] + d1[1] * r[1] + d1[2] * r[2];
    if (e <= EPS) {
      tN = 0.f; sN = fminf(fmaxf(-c / a, 0.f), 1.f);
    } else {
      const float b = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2];
      const float denom = a * e - b * b;
      sN = denom > EPS ? fminf(fmaxf((b * f - c * e) / denom, 0.f), 1.f) : 0.f;
      tN = (b * sN + f) / e;
      if (tN < 0.f) { tN = 0.f; sN = fminf(fmaxf(-c / a, 0.f), 1.f); }
      else if (tN > 1.f) { tN = 1.f; sN = fminf(fmaxf((b - c) / a, 0.f), 1.f); }
    }
  }
  const float dx = r[0] + d1[0] * sN - d2[0] * tN, dy = r[1] + d1[1] * sN - d2[1] * tN, dz = r[2] + d1[2] * sN - d2[2] * tN;
  return sqrtf(dx * dx + dy * dy + dz * dz);
}

// Signed clearance of the closest listed capsule pair of one configuration (3.0e38 without pairs).  w: 6 floats per capsule of scratch owned by
// the caller (the world end points; the kernels keep them in LDS, one slice per thread).
template <int NDOF>
IKF_HD float capsule_clearance(const Chain* __restrict__ ch, const CollisionModel* __restrict__ cm, const float qv[NDOF], float* w) {
  float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, p[3] = {0.f, 0.f, 0.f};
  const int nc = cm->n_caps;
  for (int f = 0; f <= NDOF; ++f) {
    if (f > 0) {
      compose<float>(R, p, ch->joints[f - 1].pre);
      apply_joint<float>(R, p, ch->joints[f - 1].kind, ch->joints[f - 1].axis, qv[f - 1]);
    }
    for (int c = 0; c < nc; ++c) {
      if (cm->frame[c] != f) continue;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float* pl = e == 0 ? cm->p0[c] : cm->p1[c];
#pragma unroll
        for (int r = 0; r < 3; ++r) w[c * 6 + e * 3 + r] = R[3 * r + 0] * pl[0] + R[3 * r + 1] * pl[1] + R[3 * r + 2] * pl[2] + p[r];
      }
    }
  }
  float best = 3.0e38f;
  for (int k = 0; k < cm->n_pairs; ++k) {
    const int a = cm->pair_a[k], b = cm->pair_b[k];
    const float d = segment_segment_dist(w + a * 6, w + a * 6 + 3, w + b * 6, w + b * 6 + 3) - cm->radius[a] - cm->radius[b];
    best = fminf(best, d);
  }
  return best;
}

// The chain walk of capsule_clearance alone: the world end points of every capsule into w (6 floats per capsule), the same arithmetic.  For
// the world clearance (world_math.h) of a row whose self-collision walk did not run.
template <int NDOF>
IKF_HD void capsule_endpoints(const Chain* __restrict__ ch, const CollisionModel* __restrict__ cm, const float qv[NDOF], float* w) {
  float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, p[3] = {0.f, 0.f, 0.f};
  const int nc = cm->n_caps;
  for (int f = 0; f <= NDOF; ++f) {
    if (f > 0) {
      compose<float>(R, p, ch->joints[f - 1].pre);
      apply_joint<float>(R, p, ch->joints[f - 1].kind, ch->joints[f - 1].axis, qv[f - 1]);
    }
    for (int c = 0; c < nc; ++c) {
      if (cm->frame[c] != f) continue;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float* pl = e == 0 ? cm->p0[c] : cm->p1[c];
#pragma unroll
        for (int r = 0; r < 3; ++r) w[c * 6 + e * 3 + r] = R[3 * r + 0] * pl[0] + R[3 * r + 1] * pl[1] + R[3 * r + 2] * pl[2] + p[r];
      }
    }
  }
}

IKF_HD float rank_inf() { return __builtin_huge_valf(); }

// Score of one candidate row, +inf exactly when the row is inadmissible (include/ikflow_amd_rank.h).  q_ref: the pose's reference
// configuration, read only when has_ref; cm / w: the collision model and its scratch, read only when o.reject_collisions.
template <int NDOF>
IKF_HD float rank_row_score(const Chain* __restrict__ ch, const CollisionModel* __restrict__ cm, const float qv[NDOF], const float* __restrict__ tgt,
                            const float* __restrict__ q_ref, bool has_ref, const ikf_rank_options& o, float* w) {
  float pe, re;
  pose_error_f32<NDOF>(ch, qv, tgt, &pe, &re);
  float score = pe + o.rot_weight * re;
  if (has_ref) {
    float d2 = 0.f;
#pragma unroll
    for (int j = 0; j < NDOF; ++j) {
      const float d = qv[j] - q_ref[j];
      d2 += d * d;
    }
    score += o.ref_weight * sqrtf(d2);
  }
  bool ok = score == score;
  if (o.max_pos_err >= 0.f) ok = ok && (pe < o.max_pos_err);   // strict, as ikflow_solver.py:211
  if (o.max_rot_err >= 0.f) ok = ok && (re < o.max_rot_err);
  if (o.reject_limits) {
#pragma unroll
    for (int j = 0; j < NDOF; ++j) ok = ok && !(qv[j] > ch->hi[j]) && !(qv[j] < ch->lo[j]);   // strict, as k_limits_exceeded
  }
  if (o.reject_collisions) ok = ok && !(capsule_clearance<NDOF>(ch, cm, qv, w) < o.min_clearance);
  return ok ? score : rank_inf();
}

// The best NKEEP of a pose's candidates: (score, repeat index) pairs in the strict total order "(lower score, then lower index)", ascending.
// A free slot is (+inf, INT32_MAX); a candidate with score +inf is never kept.  Every loop is unrolled on NKEEP, so the list stays in
// registers.  Because the order is total, the list of a set of candidates does not depend on how the set was split or in which order the
// parts were inserted and merged.
template <int NKEEP>
struct TopList {
  float s[NKEEP];
  int i[NKEEP];
  IKF_HD void clear() {
#pragma unroll
    for (int t = 0; t < NKEEP; ++t) { s[t] = rank_inf(); i[t] = 0x7fffffff; }
  }
  IKF_HD void insert(float score, int index) {
    if (!(score < rank_inf())) return;
    float cs = score;
    int ci = index;
#pragma unroll
    for (int t = 0; t < NKEEP; ++t) {
      const bool before = cs < s[t] || (cs == s[t] && ci < i[t]);
      const float ts = s[t];
      const int ti = i[t];
      s[t] = before ? cs : ts;
      i[t] = before ? ci : ti;
      cs = before ? ts : cs;
      ci = before ? ti : ci;
    }
  }
  IKF_HD void merge(const TopList<NKEEP>& o) {
#pragma unroll
    for (int t = 0; t < NKEEP; ++t) insert(o.s[t], o.i[t]);
  }
};

// ---- the launch geometry, pure host arithmetic -----------------------------------------------------------------------
constexpr int IKF_RANK_BLOCK = 128;       // threads of a stage-1 workgroup (two waves)
constexpr int IKF_RANK_MAX_CHUNKS = 64;
constexpr int IKF_RANK_MIN_ROWS = 4;      // a thread is not given fewer candidate rows than this for the sake of more workgroups
// poses per workgroup tile: the next power of two >= n_poses, at most 64 (one wave's lanes); the block's other threads split the repeats
inline int rank_tile_poses(long long n_poses) {
  int tp = 1;
  while (tp < 64 && tp < n_poses) tp <<= 1;
  return tp;
}
// K-chunks of a call: as many as it takes to put two workgroups on every CU, while every thread keeps IKF_RANK_MIN_ROWS rows; 1 .. 64, and no
// chunk is empty.
inline int rank_chunks(long long n_poses, int k, int n_cu) {
  if (n_poses < 1 || k < 1) return 1;
  const int tp = rank_tile_poses(n_poses);
  const int slices = IKF_RANK_BLOCK / tp;
  const long long tiles = (n_poses + tp - 1) / tp;
  long long by_rows = k / (slices * IKF_RANK_MIN_ROWS);
  long long by_cus = (2LL * (n_cu > 0 ? n_cu : 1) + tiles - 1) / tiles;
  long long c = by_rows < by_cus ? by_rows : by_cus;
  if (c > IKF_RANK_MAX_CHUNKS) c = IKF_RANK_MAX_CHUNKS;
  if (c < 1) c = 1;
  const int per = (int)((k + c - 1) / c);   // repeats per chunk
  return (k + per - 1) / per;
}

}  // namespace ikf
