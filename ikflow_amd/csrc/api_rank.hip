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
static ikf_status ensure_rank_lists(ikf_model* m, long long poses) {
  const long long lists = rank_list_bound(m, poses);
  IKF_HIP(m->rk_part_score.ensure(lists * IKF_RANK_MAX_KEEP));
  IKF_HIP(m->rk_part_index.ensure(lists * IKF_RANK_MAX_KEEP));
  IKF_HIP(m->rk_part_count.ensure(lists));
  return IKF_OK;
}
ikf_status ikf::ensure_rank_rows(ikf_model* m, long long rows) {
  IKF_HIP(m->rk_q.ensure(rows * m->dims.ndof));
  return IKF_OK;
}

ikf_status ikf::check_candidates(const ikf_model* m, const std::string& who, const char* count, int64_t n, int k, int k_max, const void* opt,
                                 bool reject_collisions, const char* rule_fault, bool have_pointers, bool* nothing_to_do) {
  *nothing_to_do = false;
  if (!opt) return fail(IKF_ERR_NULL_POINTER, who + ": null options");
  if (n < 0) return fail(IKF_ERR_BAD_ARGUMENT, who + ": " + count + " must be >= 0");
  if (k < 1 || (k_max && k > k_max))
    return fail(IKF_ERR_BAD_ARGUMENT, who + (k_max ? ": k must be in 1 .. " + std::to_string(k_max) : std::string(": k must be >= 1")));
  if (rule_fault) return fail(IKF_ERR_BAD_ARGUMENT, who + ": " + rule_fault);
  if (n > 0x7fffffffLL || n * (long long)k > 0x7fffffffLL)
    return fail(IKF_ERR_BAD_ARGUMENT, who + ": k * " + count + " must be at most 2^31 - 1");
  if (reject_collisions && !m->d_collision) return fail(IKF_ERR_BAD_ARGUMENT, who + ": reject_collisions without a collision model");
  if (n == 0) { *nothing_to_do = true; return IKF_OK; }
  if (!have_pointers) return fail(IKF_ERR_NULL_POINTER, who + ": null device pointer");
  return IKF_OK;
}
// the ranking's own rule; the pointers both of its entries need
static ikf_status rank_check(ikf_model* m, const char* who, int64_t n, int k, const ikf_rank_options* opt, const void* d_poses, const void* d_rows,
                             const void* d_q_out, bool* nothing_to_do) {
  const bool bad_keep = opt && (opt->n_keep < 1 || opt->n_keep > IKF_RANK_MAX_KEEP || opt->n_keep > k);
  return check_candidates(m, who, "n_poses", n, k, 0, opt, opt && opt->reject_collisions, bad_keep ? "n_keep must be in 1 .. min(k, 16)" : nullptr,
                          d_poses && d_rows && d_q_out, nothing_to_do);
}

ikf_status ikf::flow_candidates(ikf_model* m, const float* d_poses, int64_t n, int k, const float* d_latent, int clamp_to_limits, hipStream_t s) {
  const PoseSource ps{d_poses, nullptr, (long long)n, 7, 0.0f};   // the tiling pose source of the exact path, without an index list
  ikf_status st = run_flow_guarded(m, ps, d_latent, n * (long long)k, clamp_to_limits ? 1 : 0, m->rk_q.p, s);
  if (st != IKF_OK || m->refine_steps == 0) return st;
  // refined candidates (include/ikflow_amd_refine.h): the one hook of ranked, diverse and path IK, in place on the rows the flow has just written
  IKF_HIP(launch_refine(m->d_chain, m->dims.ndof, d_poses, n, k, m->rk_q.p, m->rk_q.p, m->refine_steps, m->refine_pos_tol, m->refine_rot_tol, nullptr,
                        nullptr, m->lm_precision, s));
  return IKF_OK;
}

ikf_status ikf::score_candidates(ikf_model* m, const float* d_poses, int64_t n, int k, const float* d_q, const float* d_q_ref,
                                 const ikf_rank_options& opt, float* d_q_out, float* d_score_out, int32_t* d_index_out, int32_t* d_count_out,
                                 float* d_row_score, hipStream_t s) {
  RankArgs a{};
  a.ch = m->d_chain;
  a.cm = m->d_collision;
  a.poses = d_poses;
  a.q = d_q;
  a.q_ref = d_q_ref;
  a.opt = opt;
  a.m = (int)n;
  a.k = k;
  a.chunks = rank_chunks(n, k, m->n_cu);
  a.per_chunk = (k + a.chunks - 1) / a.chunks;
  a.tile_poses = rank_tile_poses(n);
  // With obstacles set on the handle (ikf_set_world) every launch takes the kernel's WORLD form; that form needs every thread's capsule slice
  // whether or not self-collisions are rejected.
  if (m->world_n > 0) {
    a.world = m->d_world;
    a.world_min_clearance = m->world_min_clearance;
  }
  a.cap_stride = (opt.reject_collisions || m->world_n > 0) ? ((m->n_caps * 6) | 1) : 0;
  // With a point cloud set on the handle (ikf_set_world_cloud) the rows' cloud clearances are computed first, on the same stream, into the
  // handle's buffer; the ranking kernel reads one float per row.
  if (m->cloud_n > 0) {
    const long long rows = n * (long long)k;
    IKF_HIP(m->cloud_row.ensure(rows));
    ikf_status st = run_cloud_clearance(m, d_q, rows, m->cloud_row.p, nullptr, s);
    if (st != IKF_OK) return st;
    a.cloud_clearance = m->cloud_row.p;
    a.cloud_min_clearance = m->cloud_min_clearance;
  }
  // With a manipulability floor set on the handle (ikf_set_min_manipulability) the same buffer is the rows' gate: k_manip_rows puts -inf on every
  // row below the floor - under any cloud threshold, which is finite - and leaves the clearances of the others; with no cloud it writes -inf / +inf
  // against a threshold of 0.
  if (m->manip_min > 0.f) {
    const long long rows = n * (long long)k;
    IKF_HIP(m->cloud_row.ensure(rows));
    IKF_HIP(launch_manip_rows(m->d_chain, m->dims.ndof, d_q, rows, m->manip_part, m->manip_min, nullptr, nullptr, m->cloud_row.p,
                              m->cloud_n > 0 ? 1 : 0, s));
    if (m->cloud_n == 0) {
      a.cloud_clearance = m->cloud_row.p;
      a.cloud_min_clearance = 0.f;
    }
  }
  a.row_score = d_row_score;
  a.q_out = d_q_out;
  a.score_out = d_score_out;
  a.index_out = d_index_out;
  a.count_out = d_count_out;
  if (a.chunks > 1) {   // (sized by the ikf_reserve_* of the family: allocates only without a reservation)
    ikf_status st = ensure_rank_lists(m, n);
    if (st != IKF_OK) return st;
    a.part_score = m->rk_part_score.p;
    a.part_index = m->rk_part_index.p;
    a.part_count = m->rk_part_count.p;
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
  st = score_candidates(m, d_target_poses, n_poses, k, d_q, d_q_ref, *opt, d_q_out, d_score_out, d_index_out, d_count_out, d_row_score_out, s);
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
  st = ensure_rank_rows(m, n_poses * (long long)k);
  if (st != IKF_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  st = flow_candidates(m, d_target_poses, n_poses, k, d_latent, clamp_to_limits, s);
  if (st != IKF_OK) return st;
  st = score_candidates(m, d_target_poses, n_poses, k, m->rk_q.p, d_q_ref, *opt, d_q_out, d_score_out, d_index_out, d_count_out, d_row_score_out, s);
  if (st != IKF_OK) return st;
  IKF_HIP(scope.leave());
  return IKF_OK;
}

ikf_status ikf::reserve_candidates(ikf_model* m, const char* who, const char* rule, int64_t max_poses, int max_k, int k_max) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, std::string(who) + ": null model");
  if (max_poses < 1 || max_k < 1 || (k_max && max_k > k_max) || max_poses > 0x7fffffffLL || max_poses * (long long)max_k > 0x7fffffffLL)
    return fail(IKF_ERR_BAD_ARGUMENT, std::string(who) + ": " + rule);
  IKF_ON_DEVICE(m)
  const long long rows = max_poses * (long long)max_k;
  ikf_status st = ensure_rank_rows(m, rows);
  if (st == IKF_OK) st = ensure_rank_lists(m, max_poses);
  if (st == IKF_OK && (m->cloud_n > 0 || m->manip_min > 0.f)) IKF_HIP(m->cloud_row.ensure(rows));   // the rows' gate, under the cloud / the floor set now
  if (st == IKF_OK && m->cloud_n > 0) st = ensure_cloud_partials(m, rows);   // the cloud's partial minima
  if (st == IKF_OK && m->loaded) st = ikf_reserve(m, rows);   // the flow's scratch (and, where that path can be reached, its weight image)
  return st;
}
extern "C" ikf_status ikf_reserve_ranked(ikf_model* m, int64_t max_poses, int max_k) {
  return reserve_candidates(m, "ikf_reserve_ranked", "max_poses and max_k must be positive (product < 2^31)", max_poses, max_k, 0);
}

extern "C" int ikf_rank_chunks(const ikf_model* m, int64_t n_poses, int k) { return m ? rank_chunks(n_poses, k, m->n_cu) : 0; }
