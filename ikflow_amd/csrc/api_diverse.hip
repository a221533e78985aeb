// C-ABI of libikflow_amd.so, diverse-of-K IK (include/ikflow_amd_diverse.h): k candidates per pose - the caller's, or the flow's through the
// tiling pose source of the exact path - scored by the ranking kernel and thinned to a far-apart set by k_diverse_select (diverse_kernels.hip).
// The frame of api_path.hip: stream scope, handle-owned buffers grown on demand (the candidate rows and partial lists are the ranking's),
// nothing read back to the host.
#include "ikf_model.h"

// the row scores [rows] of a call that does not ask for them
static ikf_status ensure_diverse_score(ikf_model* m, long long rows) {
  IKF_HIP(m->dv_score.ensure(rows));
  return IKF_OK;
}

// diverse-of-K's own rules; the pointers both of its entries need
static ikf_status diverse_check(ikf_model* m, const char* who, int64_t n, int k, const ikf_diverse_options* opt, const void* d_poses,
                                const void* d_rows, const void* d_q_out, const void* d_index_out, bool* nothing_to_do) {
  const char* fault = nullptr;
  if (opt && (opt->n_keep < 1 || opt->n_keep > IKF_DIVERSE_MAX_KEEP || opt->n_keep > k)) fault = "n_keep must be in 1 .. min(k, 16)";
  else if (opt && !(opt->min_separation >= 0.f)) fault = "min_separation must be >= 0";
  return check_candidates(m, who, "n_poses", n, k, IKF_DIVERSE_MAX_K, opt, opt && opt->reject_collisions, fault,
                          d_poses && d_rows && d_q_out && d_index_out, nothing_to_do);
}

static ikf_status run_diverse(ikf_model* m, const float* d_poses, int64_t n, int k, const float* d_q, const float* d_joint_weight,
                              const ikf_diverse_options* opt, float* d_q_out, float* d_score_out, int32_t* d_index_out, float* d_separation_out,
                              int32_t* d_kept_out, int32_t* d_count_out, float* d_row_score_out, hipStream_t s) {
  // Row scores: the ranking kernel itself, n_keep = 1 - so score[r * n + j] IS ikf_rank_candidates' row score of the row.  Its one kept row
  // per pose goes to d_q_out, which the select launch behind it overwrites in full.
  float* const score = d_row_score_out ? d_row_score_out : m->dv_score.p;
  ikf_status st = score_candidates(m, d_poses, n, k, d_q, nullptr, scoring_options(*opt), d_q_out, nullptr, nullptr, nullptr, score, s);
  if (st != IKF_OK) return st;
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
  st = flow_candidates(m, d_target_poses, n_poses, k, d_latent, clamp_to_limits, s);
  if (st != IKF_OK) return st;
  st = run_diverse(m, d_target_poses, n_poses, k, m->rk_q.p, d_joint_weight, opt, d_q_out, d_score_out, d_index_out, d_separation_out, d_kept_out,
                   d_count_out, d_row_score_out, s);
  if (st != IKF_OK) return st;
  IKF_HIP(scope.leave());
  return IKF_OK;
}

extern "C" ikf_status ikf_reserve_diverse(ikf_model* m, int64_t max_poses, int max_k) {
  ikf_status st = reserve_candidates(m, "ikf_reserve_diverse", "max_poses must be positive and max_k in 1 .. 1024 (product < 2^31)", max_poses, max_k,
                                     IKF_DIVERSE_MAX_K);
  if (st != IKF_OK) return st;
  IKF_ON_DEVICE(m)
  return ensure_diverse_score(m, max_poses * (long long)max_k);
}
