// Best-of-K ranking for gfx950 (include/ikflow_amd_rank.h): K candidate rows per target pose - the flow's samples, or the caller's - scored,
// the inadmissible ones dropped, the best n_keep of every pose selected.  What a user of the reference does with evaluate_solutions
// (ikflow/evaluation_utils.py) and a sort over the 50 solutions per pose that scripts/evaluate.py draws.
//
// Stage 1, k_rank_candidates: grid (pose tiles x K-chunks), 128 threads.  A workgroup owns tile_poses consecutive poses (a power of two, at
// most 64) and one chunk of repeats; thread t = (slice t / tile_poses, pose t % tile_poses), so at a fixed repeat adjacent lanes read the
// rows of adjacent poses.  A thread walks the repeats slice, slice + S, ... of its pose (S = 128 / tile_poses), scores each row
// (rank_math.h: one chain walk for the pose error, the capsule walk of k_self_collision on top when collisions are rejected) and keeps
// its best NKEEP in registers (TopList).  The slices of a pose are merged by __shfl_xor inside a wave and through LDS between the two waves.
// With one chunk the workgroup writes the call's outputs; with more it writes its lists to the handle's scratch and stage 2, k_rank_merge
// (a thread per pose), merges the chunks.  No atomics, no waiting between workgroups: the selection order is total, so every split gives
// the same lists.  LDS per workgroup (dynamic): tile_poses x (2 NKEEP + 1) words for the wave hand-over (<= 8448 B) + 128 x ((6 n_caps) | 1)
// floats of capsule end points when collisions are rejected (<= 74240 B at 24 capsules): at most 82688 B of a CU's 160 KiB.
// WORLD (a world is set on the handle, include/ikflow_amd_world.h): the obstacle table (4096 B) is staged between the two areas, every
// thread has its capsule slice whatever reject_collisions says, and the score is rank_row_score_world: at most 86784 B.  WORLD = false is the
// kernel as it was.  A point cloud on the handle (include/ikflow_amd_cloud.h) costs both forms one run-time test of a pointer per row: with
// RankArgs::cloud_clearance set, a row whose precomputed cloud clearance is below the cloud's threshold scores +inf before anything sees its score.
#include "ikf_internal.h"

namespace ikf {

template <int NDOF, int NKEEP>
__device__ __forceinline__ void rank_write_final(const RankArgs& a, long long j, const TopList<NKEEP>& top, int count) {
  const int nk = a.opt.n_keep;
#pragma unroll
  for (int t = 0; t < NKEEP; ++t) {
    if (t >= nk) continue;   // (no break: the loop must unroll for the list to stay in registers)
    const bool valid = top.s[t] < rank_inf();
    const long long slot = j * nk + t;
    if (a.score_out) a.score_out[slot] = valid ? top.s[t] : rank_inf();
    if (a.index_out) a.index_out[slot] = valid ? top.i[t] : -1;
    const long long row = valid ? (long long)top.i[t] * a.m + j : 0;
#pragma unroll
    for (int d = 0; d < NDOF; ++d) a.q_out[slot * NDOF + d] = valid ? a.q[row * NDOF + d] : 0.f;
  }
  if (a.count_out) a.count_out[j] = count;
}

template <int NDOF, int NKEEP, bool WORLD>
__global__ __launch_bounds__(IKF_RANK_BLOCK) void k_rank_candidates(const RankArgs a) {
  extern __shared__ float rank_lds[];
  const int tp = a.tile_poses, slices = IKF_RANK_BLOCK / tp;
  const int t = threadIdx.x, pl = t & (tp - 1), sl = t / tp;
  const long long j = (long long)blockIdx.x * tp + pl;
  const bool live = j < a.m;
  const int r_begin = blockIdx.y * a.per_chunk;
  const int r_end = r_begin + a.per_chunk < a.k ? r_begin + a.per_chunk : a.k;
  float* const hand = rank_lds;                                           // [2 NKEEP + 1][tp]
  float* const w = rank_lds + tp * (2 * NKEEP + 1) + (WORLD ? IKF_WORLD_TABLE_WORDS : 0) + t * a.cap_stride;   // this thread's capsule end points
  const WorldObstacle* const obs = reinterpret_cast<const WorldObstacle*>(rank_lds + tp * (2 * NKEEP + 1));     // WORLD: the staged table
  int n_obs = 0;
  if constexpr (WORLD) {
    n_obs = a.world->n;
    const float* const src = reinterpret_cast<const float*>(a.world->obs);
    for (int i = t; i < n_obs * IKF_WORLD_OBSTACLE_WORDS; i += IKF_RANK_BLOCK) rank_lds[tp * (2 * NKEEP + 1) + i] = src[i];
    __syncthreads();
  }

  TopList<NKEEP> top;
  top.clear();
  int count = 0;
  if (live) {
    float tg[7], qr[NDOF];
#pragma unroll
    for (int i = 0; i < 7; ++i) tg[i] = a.poses[j * 7 + i];
#pragma unroll
    for (int d = 0; d < NDOF; ++d) qr[d] = a.q_ref ? a.q_ref[j * NDOF + d] : 0.f;
    for (int r = r_begin + sl; r < r_end; r += slices) {
      const long long row = (long long)r * a.m + j;
      float qv[NDOF];
      load_q<NDOF>(a.q, row, qv);
      float score;
      if constexpr (WORLD) score = rank_row_score_world<NDOF>(a.ch, a.cm, qv, tg, qr, a.q_ref != nullptr, a.opt, w, obs, n_obs, a.world_min_clearance);
      else score = rank_row_score<NDOF>(a.ch, a.cm, qv, tg, qr, a.q_ref != nullptr, a.opt, w);
      // a point cloud on the handle (include/ikflow_amd_cloud.h): the row's clearance from it was computed in front of this launch
      if (a.cloud_clearance && a.cloud_clearance[row] < a.cloud_min_clearance) score = rank_inf();
      if (a.row_score) a.row_score[row] = score;
      if (score < rank_inf()) ++count;
      top.insert(score, r);
    }
  }
  // the slices of a pose that share this wave: lanes pl, pl + tp, ...  (a dead lane has an empty list; lanes of one pose are dead together)
  for (int off = tp; off < 64; off <<= 1) {
    TopList<NKEEP> o;
#pragma unroll
    for (int e = 0; e < NKEEP; ++e) {
      o.s[e] = __shfl_xor(top.s[e], off);
      o.i[e] = __shfl_xor(top.i[e], off);
    }
    top.merge(o);
    count += __shfl_xor(count, off);
  }
  // the second wave hands its lists to the first
  const int lane = t & 63, wave = t >> 6;
  if (wave == 1 && lane < tp) {
#pragma unroll
    for (int e = 0; e < NKEEP; ++e) {
      hand[e * tp + lane] = top.s[e];
      hand[(NKEEP + e) * tp + lane] = __int_as_float(top.i[e]);
    }
    hand[2 * NKEEP * tp + lane] = __int_as_float(count);
  }
  __syncthreads();
  if (wave != 0 || lane >= tp || !live) return;
  {
    TopList<NKEEP> o;
#pragma unroll
    for (int e = 0; e < NKEEP; ++e) {
      o.s[e] = hand[e * tp + lane];
      o.i[e] = __float_as_int(hand[(NKEEP + e) * tp + lane]);
    }
    top.merge(o);
    count += __float_as_int(hand[2 * NKEEP * tp + lane]);
  }
  if (a.chunks == 1) {
    rank_write_final<NDOF, NKEEP>(a, j, top, count);
    return;
  }
  const int nk = a.opt.n_keep;
  const long long base = ((long long)blockIdx.y * a.m + j) * nk;
#pragma unroll
  for (int e = 0; e < NKEEP; ++e) {
    if (e >= nk) continue;
    a.part_score[base + e] = top.s[e];
    a.part_index[base + e] = top.i[e];
  }
  a.part_count[(long long)blockIdx.y * a.m + j] = count;
}

// Stage 2: the chunks' lists of a pose, merged by one thread; writes the call's outputs.
template <int NDOF, int NKEEP>
__global__ __launch_bounds__(256) void k_rank_merge(const RankArgs a) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.m) return;
  const int nk = a.opt.n_keep;
  TopList<NKEEP> top;
  top.clear();
  int count = 0;
  for (int c = 0; c < a.chunks; ++c) {
    const long long base = ((long long)c * a.m + j) * nk;
#pragma unroll
    for (int e = 0; e < NKEEP; ++e) {
      if (e >= nk) continue;
      top.insert(a.part_score[base + e], a.part_index[base + e]);
    }
    count += a.part_count[(long long)c * a.m + j];
  }
  rank_write_final<NDOF, NKEEP>(a, j, top, count);
}

static inline int rank_keep_capacity(int n_keep) { return n_keep <= 1 ? 1 : n_keep <= 4 ? 4 : IKF_RANK_MAX_KEEP; }

size_t rank_lds_bytes(const RankArgs& a) {
  return sizeof(float) * ((size_t)a.tile_poses * (2 * rank_keep_capacity(a.opt.n_keep) + 1) + (a.world ? IKF_WORLD_TABLE_WORDS : 0) +
                          (size_t)IKF_RANK_BLOCK * a.cap_stride);
}
constexpr size_t kRankMaxLds =
    sizeof(float) * (64 * (2 * IKF_RANK_MAX_KEEP + 1) + IKF_WORLD_TABLE_WORDS + (size_t)IKF_RANK_BLOCK * (IKF_MAX_CAPSULES * 6 + 1));
static_assert(kRankMaxLds == 82688 + 4096, "hand-over area + obstacle table + capsule slices");
static_assert(kRankMaxLds <= 160 * 1024, "a stage-1 workgroup must fit the LDS of a CU");

template <int NDOF, int NKEEP, bool WORLD>
static hipError_t launch_rank_as(const RankArgs& a, hipStream_t s) {
  static bool lds_opt_in[64];
  const size_t lds = rank_lds_bytes(a);
  if (lds > 48 * 1024) {
    if (hipError_t e = ensure_dynamic_lds(k_rank_candidates<NDOF, NKEEP, WORLD>, kRankMaxLds, lds_opt_in); e != hipSuccess) return e;
  }
  const unsigned tiles = (unsigned)(((long long)a.m + a.tile_poses - 1) / a.tile_poses);
  hipLaunchKernelGGL((k_rank_candidates<NDOF, NKEEP, WORLD>), dim3(tiles, a.chunks), dim3(IKF_RANK_BLOCK), lds, s, a);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (a.chunks > 1) hipLaunchKernelGGL((k_rank_merge<NDOF, NKEEP>), dim3((unsigned)(((long long)a.m + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_rank(int ndof, const RankArgs& a, hipStream_t s) {
  if (a.m <= 0) return hipSuccess;
  if (a.k < 1 || a.opt.n_keep < 1 || a.opt.n_keep > IKF_RANK_MAX_KEEP || a.opt.n_keep > a.k || a.chunks < 1 || a.per_chunk < 1 ||
      (long long)a.chunks * a.per_chunk < a.k || a.chunks > 65535 || a.tile_poses != rank_tile_poses(a.m) ||
      ((a.opt.reject_collisions || a.world) && (!a.cm || a.cap_stride < 1 || a.cap_stride > IKF_MAX_CAPSULES * 6 + 1)) ||
      (a.chunks > 1 && (!a.part_score || !a.part_index || !a.part_count)))
    return hipErrorInvalidValue;
  if (a.world) {
    switch (rank_keep_capacity(a.opt.n_keep)) {
      case 1: IKF_NDOF_DISPATCH(ndof, return (launch_rank_as<ND, 1, true>(a, s))); break;
      case 4: IKF_NDOF_DISPATCH(ndof, return (launch_rank_as<ND, 4, true>(a, s))); break;
      default: IKF_NDOF_DISPATCH(ndof, return (launch_rank_as<ND, IKF_RANK_MAX_KEEP, true>(a, s))); break;
    }
    return hipErrorInvalidValue;
  }
  switch (rank_keep_capacity(a.opt.n_keep)) {
    case 1: IKF_NDOF_DISPATCH(ndof, return (launch_rank_as<ND, 1, false>(a, s))); break;
    case 4: IKF_NDOF_DISPATCH(ndof, return (launch_rank_as<ND, 4, false>(a, s))); break;
    default: IKF_NDOF_DISPATCH(ndof, return (launch_rank_as<ND, IKF_RANK_MAX_KEEP, false>(a, s))); break;
  }
  return hipErrorInvalidValue;
}

}  // namespace ikf
