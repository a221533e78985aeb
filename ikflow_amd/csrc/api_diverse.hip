// C-ABI of libikflow_amd.so, diverse-of-K IK (include/ikflow_amd_diverse.h): k candidates per pose - the caller's, or the flow's through the
// tiling pose source of the exact path - scored by the ranking kernel and thinned to a far-apart set by k_diverse_select (diverse_kernels.hip).
// The frame of api_path.hip: stream scope, handle-owned buffers grown on demand (the candidate rows and partial lists are the ranking's),
// nothing read back to the host.
#include "ikf_model.h"

// the row scores [rows] of a call that does not ask for them
static ikf_status ensure_diverse_score(ikf_model* m, long long rows) {
  if (rows <= m->dv_rows) return IKF_OK;
  if (m->dv_score) (void)hipFree(m->dv_score);
  m->dv_score = nullptr;
  m->dv_rows = 0;
  IKF_HIP(hipMalloc(&m->dv_score, sizeof(float) * (size_t)rows));
  m->dv_rows = rows;
  return IKF_OK;
}

// what both entries check once the handle is known to be there; *nothing_to_do: n_poses == 0
static ikf_status diverse_check(ikf_model* m, const std::string& who, int64_t n, int k, const ikf_diverse_options* opt, const void* d_poses,
                                const void* d_rows, const void* d_q_out, const void* d_index_out, bool* nothing_to_do) {
  *nothing_to_do = false;
  if (!opt) return fail(IKF_ERR_NULL_POINTER, who + ": null options");
  if (n < 0) return fail(IKF_ERR_BAD_ARGUMENT, who + ": n_poses must be >= 0");
  if (k < 1 || k > IKF_DIVERSE_MAX_K) return fail(IKF_ERR_BAD_ARGUMENT, who + ": k must be in 1 .. 1024");
  if (opt->n_keep < 1 || opt->n_keep > IKF_DIVERSE_MAX_KEEP || opt->n_keep > k)
    return fail(IKF_ERR_BAD_ARGUMENT, who + ": n_keep must be in 1 .. min(k, 16)");
  if (n > 0x7fffffffLL || n * (long long)k > 0x7fffffffLL) return fail(IKF_ERR_BAD_ARGUMENT, who + ": k * n_poses must be at most 2^31 - 1");
  if (!(opt->min_separation >= 0.f)) return fail(IKF_ERR_BAD_ARGUMENT, who + ": min_separation must be >= 0");
  if (opt->reject_collisions && !m->d_collision) return fail(IKF_ERR_BAD_ARGUMENT, who + ": reject_collisions without a collision model");
  if (n == 0) { *nothing_to_do = true; return IKF_OK; }
  if (!d_poses || !d_rows || !d_q_out || !d_index_out) return fail(IKF_ERR_NULL_POINTER, who + ": null device pointer");
  return IKF_OK;
}

static ikf_status run_diverse(ikf_model* m, const float* d_poses, int64_t n, int k, const float* d_q, const float* d_joint_weight,
                              const ikf_diverse_options* opt, float* d_q_out, float* d_score_out, int32_t* d_index_out, float* d_separation_out,
                              int32_t* d_kept_out, int32_t* d_count_out, float* d_row_score_out, hipStream_t s) {
  // Row scores: the ranking kernel itself, n_keep = 1 - so score[r * n + j] IS ikf_rank_candidates' row score of the row.  Its one kept row
  // per pose goes to d_q_out, which the select launch behind it overwrites in full.
  float* const score = d_row_score_out ? d_row_score_out : m->dv_score;
  RankArgs ra{};
  ra.ch = m->d_chain;
  ra.cm = m->d_collision;
  ra.poses = d_poses;
  ra.q = d_q;
  ra.opt.n_keep = 1;
  ra.opt.rot_weight = opt->rot_weight;
  ra.opt.max_pos_err = opt->max_pos_err;
  ra.opt.max_rot_err = opt->max_rot_err;
  ra.opt.reject_limits = opt->reject_limits;
  ra.opt.reject_collisions = opt->reject_collisions;
  ra.opt.min_clearance = opt->min_clearance;
  ra.m = (int)n;
  ra.k = k;
  ra.chunks = rank_chunks(n, k, m->n_cu);
  ra.per_chunk = (k + ra.chunks - 1) / ra.chunks;
  ra.tile_poses = rank_tile_poses(n);
  ra.cap_stride = opt->reject_collisions ? ((m->n_caps * 6) | 1) : 0;
  rank_args_world(m, &ra);
  ra.row_score = score;
  ra.q_out = d_q_out;
  if (ra.chunks > 1) {
    ikf_status st = ensure_rank_lists(m, n);   // (sized by ikf_reserve_diverse: allocates only without a reservation)
    if (st != IKF_OK) return st;
    ra.part_score = m->rk_part_score;
    ra.part_index = m->rk_part_index;
    ra.part_count = m->rk_part_count;
  }
  IKF_HIP(launch_rank(m->dims.ndof, ra, s));
  DiverseArgs a{};
  a.q = d_q;
  a.score = score;
  a.w = d_joint_weight;
  a.n = (int)n;
  a.k = k;
  a.n_keep = opt->n_keep;
  a.min_separation = opt->min_separation;
  a.q_out = d_q_out;
  a.score_out = d_score_out;
  a.index_out = d_index_out;
  a.sep_out = d_separation_out;
  a.kept_out = d_kept_out;
  a.count_out = d_count_out;
  IKF_HIP(prof_mark(m, s));   // between ikf_profile_begin / _end the select stage is bracketed (tools/diverse_timing.py); otherwise nothing is recorded
  IKF_HIP(launch_diverse_select(m->dims.ndof, a, s));
  IKF_HIP(prof_mark(m, s));
  return IKF_OK;
}

extern "C" ikf_status ikf_diverse_select(ikf_model* m, const float* d_target_poses, int64_t n_poses, int k, const float* d_q,
                                         const float* d_joint_weight, const ikf_diverse_options* opt, float* d_q_out, float* d_score_out,
                                         int32_t* d_index_out, float* d_separation_out, int32_t* d_kept_out, int32_t* d_count_out,
                                         float* d_row_score_out, void* stream) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_diverse_select: null model");
  bool nothing = false;
  ikf_status st = diverse_check(m, "ikf_diverse_select", n_poses, k, opt, d_target_poses, d_q, d_q_out, d_index_out, &nothing);
  if (st != IKF_OK || nothing) return st;
  IKF_ON_DEVICE(m)
  if (!d_row_score_out) {
    st = ensure_diverse_score(m, n_poses * (long long)k);
    if (st != IKF_OK) return st;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  st = run_diverse(m, d_target_poses, n_poses, k, d_q, d_joint_weight, opt, d_q_out, d_score_out, d_index_out, d_separation_out, d_kept_out,
                   d_count_out, d_row_score_out, s);
  if (st != IKF_OK) return st;
  IKF_HIP(scope.leave());
  return IKF_OK;
}

extern "C" ikf_status ikf_generate_diverse(ikf_model* m, const float* d_target_poses, int64_t n_poses, int k, const float* d_latent,
                                           int clamp_to_limits, const float* d_joint_weight, const ikf_diverse_options* opt, float* d_q_out,
                                           float* d_score_out, int32_t* d_index_out, float* d_separation_out, int32_t* d_kept_out,
                                           int32_t* d_count_out, float* d_row_score_out, void* stream) {
  ikf_status st = check_ready(m, "ikf_generate_diverse");
  if (st != IKF_OK) return st;
  bool nothing = false;
  st = diverse_check(m, "ikf_generate_diverse", n_poses, k, opt, d_target_poses, d_latent, d_q_out, d_index_out, &nothing);
  if (st != IKF_OK || nothing) return st;
  IKF_ON_DEVICE(m)
  const long long rows = n_poses * (long long)k;
  st = ensure_rank_rows(m, rows);
  if (st == IKF_OK && !d_row_score_out) st = ensure_diverse_score(m, rows);
  if (st != IKF_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  // the conditional of row r * n_poses + j is pose j: the tiling pose source of the exact path, without an index list
  const PoseSource ps{d_target_poses, nullptr, (long long)n_poses, 7, 0.0f};
  st = run_flow_guarded(m, ps, d_latent, rows, clamp_to_limits ? 1 : 0, m->rk_q, s);
  if (st != IKF_OK) return st;
  st = run_diverse(m, d_target_poses, n_poses, k, m->rk_q, d_joint_weight, opt, d_q_out, d_score_out, d_index_out, d_separation_out, d_kept_out,
                   d_count_out, d_row_score_out, s);
  if (st != IKF_OK) return st;
  IKF_HIP(scope.leave());
  return IKF_OK;
}

extern "C" ikf_status ikf_reserve_diverse(ikf_model* m, int64_t max_poses, int max_k) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_reserve_diverse: null model");
  if (max_poses < 1 || max_k < 1 || max_k > IKF_DIVERSE_MAX_K || max_poses > 0x7fffffffLL || max_poses * (long long)max_k > 0x7fffffffLL)
    return fail(IKF_ERR_BAD_ARGUMENT, "ikf_reserve_diverse: max_poses must be positive and max_k in 1 .. 1024 (product < 2^31)");
  IKF_ON_DEVICE(m)
  const long long rows = max_poses * (long long)max_k;
  ikf_status st = ensure_rank_rows(m, rows);
  if (st == IKF_OK) st = ensure_rank_lists(m, max_poses);
  if (st == IKF_OK) st = ensure_diverse_score(m, rows);
  if (st == IKF_OK && m->loaded) st = ikf_reserve(m, rows);   // the flow's scratch (and, where that path can be reached, its weight image)
  return st;
}
