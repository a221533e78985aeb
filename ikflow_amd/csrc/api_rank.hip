// C-ABI of libikflow_amd.so, best-of-K ranking (include/ikflow_amd_rank.h): K candidates per pose - the caller's, or the flow's through the tiling
// pose source of the exact path - ranked by k_rank_candidates / k_rank_merge (rank_kernels.hip).  Same frame as run_exact: stream scope,
// handle-owned buffers grown on demand, nothing read back to the host.
#include "ikf_model.h"

// Partial lists (one per chunk and pose) that any call of up to `poses` poses can need on this device, whatever its k: chunks <= 64, and
// chunks <= 2 n_cu / tiles + 1 with tiles >= poses / 64.  Monotone in `poses`, so a reservation covers every smaller call.
static long long rank_list_bound(const ikf_model* m, long long poses) {
  const long long by_chunks = IKF_RANK_MAX_CHUNKS * poses, by_cus = 128LL * m->n_cu + poses;
  return by_chunks < by_cus ? by_chunks : by_cus;
}
ikf_status ikf::ensure_rank_lists(ikf_model* m, long long poses) {   // (also the node stage of path IK, api_path.hip)
  const long long lists = rank_list_bound(m, poses);
  if (lists <= m->rk_lists) return IKF_OK;
  if (m->rk_part_score) (void)hipFree(m->rk_part_score);
  if (m->rk_part_index) (void)hipFree(m->rk_part_index);
  if (m->rk_part_count) (void)hipFree(m->rk_part_count);
  m->rk_part_score = nullptr; m->rk_part_index = nullptr; m->rk_part_count = nullptr;
  m->rk_lists = 0;
  IKF_HIP(hipMalloc(&m->rk_part_score, sizeof(float) * (size_t)lists * IKF_RANK_MAX_KEEP));
  IKF_HIP(hipMalloc(&m->rk_part_index, sizeof(int) * (size_t)lists * IKF_RANK_MAX_KEEP));
  IKF_HIP(hipMalloc(&m->rk_part_count, sizeof(int) * (size_t)lists));
  m->rk_lists = lists;
  return IKF_OK;
}
ikf_status ikf::ensure_rank_rows(ikf_model* m, long long rows) {   // (also the candidate rows of path IK, api_path.hip)
  if (rows <= m->rk_rows) return IKF_OK;
  if (m->rk_q) (void)hipFree(m->rk_q);
  m->rk_q = nullptr;
  m->rk_rows = 0;
  IKF_HIP(hipMalloc(&m->rk_q, sizeof(float) * (size_t)rows * m->dims.ndof));
  m->rk_rows = rows;
  return IKF_OK;
}

// With obstacles set on the handle (ikf_set_world) every launch of k_rank_candidates - the ranking's, the node stage of path IK, the score stage
// of diverse-of-K - takes its WORLD form; that form needs every thread's capsule slice whether or not self-collisions are rejected.
void ikf::rank_args_world(const ikf_model* m, RankArgs* a) {
  if (m->world_n < 1) return;
  a->world = m->d_world;
  a->world_min_clearance = m->world_min_clearance;
  a->cap_stride = (m->n_caps * 6) | 1;
}

// what both entries check once the handle is known to be there; *nothing_to_do: n_poses == 0
static ikf_status rank_check(ikf_model* m, const std::string& who, int64_t n, int k, const ikf_rank_options* opt, const void* d_poses,
                             const void* d_rows, const void* d_q_out, bool* nothing_to_do) {
  *nothing_to_do = false;
  if (!opt) return fail(IKF_ERR_NULL_POINTER, who + ": null options");
  if (n < 0) return fail(IKF_ERR_BAD_ARGUMENT, who + ": n_poses must be >= 0");
  if (k < 1) return fail(IKF_ERR_BAD_ARGUMENT, who + ": k must be >= 1");
  if (opt->n_keep < 1 || opt->n_keep > IKF_RANK_MAX_KEEP || opt->n_keep > k)
    return fail(IKF_ERR_BAD_ARGUMENT, who + ": n_keep must be in 1 .. min(k, 16)");
  if (n > 0x7fffffffLL || n * (long long)k > 0x7fffffffLL) return fail(IKF_ERR_BAD_ARGUMENT, who + ": k * n_poses must be at most 2^31 - 1");
  if (opt->reject_collisions && !m->d_collision) return fail(IKF_ERR_BAD_ARGUMENT, who + ": reject_collisions without a collision model");
  if (n == 0) { *nothing_to_do = true; return IKF_OK; }
  if (!d_poses || !d_rows || !d_q_out) return fail(IKF_ERR_NULL_POINTER, who + ": null device pointer");
  return IKF_OK;
}

static ikf_status run_rank(ikf_model* m, const float* d_poses, int64_t n, int k, const float* d_q, const float* d_q_ref,
                           const ikf_rank_options* opt, float* d_q_out, float* d_score_out, int32_t* d_index_out, int32_t* d_count_out,
                           float* d_row_score_out, hipStream_t s) {
  RankArgs a{};
  a.ch = m->d_chain;
  a.cm = m->d_collision;
  a.poses = d_poses;
  a.q = d_q;
  a.q_ref = d_q_ref;
  a.opt = *opt;
  a.m = (int)n;
  a.k = k;
  a.chunks = rank_chunks(n, k, m->n_cu);
  a.per_chunk = (k + a.chunks - 1) / a.chunks;
  a.tile_poses = rank_tile_poses(n);
  a.cap_stride = opt->reject_collisions ? ((m->n_caps * 6) | 1) : 0;
  rank_args_world(m, &a);
  a.row_score = d_row_score_out;
  a.q_out = d_q_out;
  a.score_out = d_score_out;
  a.index_out = d_index_out;
  a.count_out = d_count_out;
  if (a.chunks > 1) {
    ikf_status st = ensure_rank_lists(m, n);
    if (st != IKF_OK) return st;
    a.part_score = m->rk_part_score;
    a.part_index = m->rk_part_index;
    a.part_count = m->rk_part_count;
  }
  IKF_HIP(launch_rank(m->dims.ndof, a, s));
  return IKF_OK;
}

extern "C" ikf_status ikf_rank_candidates(ikf_model* m, const float* d_target_poses, int64_t n_poses, int k, const float* d_q, const float* d_q_ref,
                                          const ikf_rank_options* opt, float* d_q_out, float* d_score_out, int32_t* d_index_out,
                                          int32_t* d_count_out, float* d_row_score_out, void* stream) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_rank_candidates: null model");
  bool nothing = false;
  ikf_status st = rank_check(m, "ikf_rank_candidates", n_poses, k, opt, d_target_poses, d_q, d_q_out, &nothing);
  if (st != IKF_OK || nothing) return st;
  IKF_ON_DEVICE(m)
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  st = run_rank(m, d_target_poses, n_poses, k, d_q, d_q_ref, opt, d_q_out, d_score_out, d_index_out, d_count_out, d_row_score_out, s);
  if (st != IKF_OK) return st;
  IKF_HIP(scope.leave());
  return IKF_OK;
}

extern "C" ikf_status ikf_generate_ranked(ikf_model* m, const float* d_target_poses, int64_t n_poses, int k, const float* d_latent,
                                          int clamp_to_limits, const float* d_q_ref, const ikf_rank_options* opt, float* d_q_out,
                                          float* d_score_out, int32_t* d_index_out, int32_t* d_count_out, float* d_row_score_out, void* stream) {
  ikf_status st = check_ready(m, "ikf_generate_ranked");
  if (st != IKF_OK) return st;
  bool nothing = false;
  st = rank_check(m, "ikf_generate_ranked", n_poses, k, opt, d_target_poses, d_latent, d_q_out, &nothing);
  if (st != IKF_OK || nothing) return st;
  IKF_ON_DEVICE(m)
  const long long rows = n_poses * (long long)k;
  st = ensure_rank_rows(m, rows);
  if (st != IKF_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  // the conditional of row r * n_poses + j is pose j: the tiling pose source of the exact path, without an index list
  const PoseSource ps{d_target_poses, nullptr, (long long)n_poses, 7, 0.0f};
  st = run_flow_guarded(m, ps, d_latent, rows, clamp_to_limits ? 1 : 0, m->rk_q, s);
  if (st != IKF_OK) return st;
  st = run_rank(m, d_target_poses, n_poses, k, m->rk_q, d_q_ref, opt, d_q_out, d_score_out, d_index_out, d_count_out, d_row_score_out, s);
  if (st != IKF_OK) return st;
  IKF_HIP(scope.leave());
  return IKF_OK;
}

extern "C" ikf_status ikf_reserve_ranked(ikf_model* m, int64_t max_poses, int max_k) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_reserve_ranked: null model");
  if (max_poses < 1 || max_k < 1 || max_poses > 0x7fffffffLL || max_poses * (long long)max_k > 0x7fffffffLL)
    return fail(IKF_ERR_BAD_ARGUMENT, "ikf_reserve_ranked: max_poses and max_k must be positive (product < 2^31)");
  IKF_ON_DEVICE(m)
  const long long rows = max_poses * (long long)max_k;
  ikf_status st = ensure_rank_rows(m, rows);
  if (st == IKF_OK) st = ensure_rank_lists(m, max_poses);
  if (st == IKF_OK && m->loaded) st = ikf_reserve(m, rows);   // the flow's scratch (and, where that path can be reached, its weight image)
  return st;
}

extern "C" int ikf_rank_chunks(const ikf_model* m, int64_t n_poses, int k) { return m ? rank_chunks(n_poses, k, m->n_cu) : 0; }
