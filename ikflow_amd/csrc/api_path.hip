// C-ABI of libikflow_amd.so, path IK (include/ikflow_amd_path.h): k candidates per waypoint - the caller's, or the flow's through the tiling
// pose source of the exact path - scored by the ranking kernel and searched by k_path_lattice (path_kernels.hip).  The frame of api_rank.hip: stream
// scope, handle-owned buffers grown on demand (the candidate rows are the ranking's), nothing read back to the host.
#include "ikf_model.h"

// node costs [rows] and back-pointers (a byte per node) of a lattice of up to `rows` nodes
static ikf_status ensure_path_scratch(ikf_model* m, long long rows) {
  if (rows <= m->pt_rows) return IKF_OK;
  if (m->pt_node) (void)hipFree(m->pt_node);
  if (m->pt_bp) (void)hipFree(m->pt_bp);
  m->pt_node = nullptr; m->pt_bp = nullptr;
  m->pt_rows = 0;
  IKF_HIP(hipMalloc(&m->pt_node, sizeof(float) * (size_t)rows));
  IKF_HIP(hipMalloc(&m->pt_bp, (size_t)path_bp_bytes(rows, 1)));
  m->pt_rows = rows;
  return IKF_OK;
}
// the shared latent expanded to one row per candidate row
static ikf_status ensure_path_latent(ikf_model* m, long long rows) {
  if (rows <= m->pt_latent_rows) return IKF_OK;
  if (m->pt_latent) (void)hipFree(m->pt_latent);
  m->pt_latent = nullptr;
  m->pt_latent_rows = 0;
  IKF_HIP(hipMalloc(&m->pt_latent, sizeof(float) * (size_t)rows * m->dims.D));
  m->pt_latent_rows = rows;
  return IKF_OK;
}

// what both entries check once the handle is known to be there; *nothing_to_do: T == 0
static ikf_status path_check(ikf_model* m, const std::string& who, int64_t T, int k, const ikf_path_options* opt, const void* d_waypoints,
                             const void* d_rows, const void* d_path_out, const void* d_index_out, const void* d_cost_out, bool* nothing_to_do) {
  *nothing_to_do = false;
  if (!opt) return fail(IKF_ERR_NULL_POINTER, who + ": null options");
  if (T < 0) return fail(IKF_ERR_BAD_ARGUMENT, who + ": T must be >= 0");
  if (k < 1 || k > IKF_PATH_MAX_K) return fail(IKF_ERR_BAD_ARGUMENT, who + ": k must be in 1 .. 256");
  if (T > 0x7fffffffLL || T * (long long)k > 0x7fffffffLL) return fail(IKF_ERR_BAD_ARGUMENT, who + ": k * T must be at most 2^31 - 1");
  if (!(opt->node_weight >= 0.f)) return fail(IKF_ERR_BAD_ARGUMENT, who + ": node_weight must be >= 0");
  if (opt->reject_collisions && !m->d_collision) return fail(IKF_ERR_BAD_ARGUMENT, who + ": reject_collisions without a collision model");
  if (T == 0) { *nothing_to_do = true; return IKF_OK; }
  if (!d_waypoints || !d_rows || !d_path_out || !d_index_out || !d_cost_out) return fail(IKF_ERR_NULL_POINTER, who + ": null device pointer");
  return IKF_OK;
}

static ikf_status run_path(ikf_model* m, const float* d_waypoints, int64_t T, int k, const float* d_q, const float* d_q_start,
                           const ikf_path_options* opt, float* d_path_out, int32_t* d_index_out, float* d_cost_out, int32_t* d_reachable_out,
                           float* d_node_cost_out, hipStream_t s) {
  // Node costs: the ranking kernel itself, the waypoints as its poses, n_keep = 1 - so node[t][r] IS ikf_rank_candidates' row score of the row.
  // Its one kept row per waypoint goes to d_path_out, which the lattice launch behind it overwrites in full.
  float* const node = d_node_cost_out ? d_node_cost_out : m->pt_node;
  RankArgs ra{};
  ra.ch = m->d_chain;
  ra.cm = m->d_collision;
  ra.poses = d_waypoints;
  ra.q = d_q;
  ra.opt.n_keep = 1;
  ra.opt.rot_weight = opt->rot_weight;
  ra.opt.max_pos_err = opt->max_pos_err;
  ra.opt.max_rot_err = opt->max_rot_err;
  ra.opt.reject_limits = opt->reject_limits;
  ra.opt.reject_collisions = opt->reject_collisions;
  ra.opt.min_clearance = opt->min_clearance;
  ra.m = (int)T;
  ra.k = k;
  ra.chunks = rank_chunks(T, k, m->n_cu);
  ra.per_chunk = (k + ra.chunks - 1) / ra.chunks;
  ra.tile_poses = rank_tile_poses(T);
  ra.cap_stride = opt->reject_collisions ? ((m->n_caps * 6) | 1) : 0;
  rank_args_world(m, &ra);
  ra.row_score = node;
  ra.q_out = d_path_out;
  if (ra.chunks > 1) {
    ikf_status st = ensure_rank_lists(m, T);   // (sized by ikf_reserve_path: allocates only without a reservation)
    if (st != IKF_OK) return st;
    ra.part_score = m->rk_part_score;
    ra.part_index = m->rk_part_index;
    ra.part_count = m->rk_part_count;
  }
  IKF_HIP(launch_rank(m->dims.ndof, ra, s));
  PathArgs a{};
  a.q = d_q;
  a.q_start = d_q_start;
  a.opt = *opt;
  a.T = (int)T;
  a.k = k;
  a.node = node;
  a.bp = m->pt_bp;
  a.path_out = d_path_out;
  a.index_out = d_index_out;
  a.cost_out = d_cost_out;
  a.reachable_out = d_reachable_out;
  IKF_HIP(prof_mark(m, s));   // between ikf_profile_begin / _end the sequential stage is bracketed (tools/path_timing.py); otherwise nothing is recorded
  IKF_HIP(launch_path_lattice(m->dims.ndof, a, s));
  IKF_HIP(prof_mark(m, s));
  return IKF_OK;
}

extern "C" ikf_status ikf_path_search(ikf_model* m, const float* d_waypoints, int64_t T, int k, const float* d_q, const float* d_q_start,
                                      const ikf_path_options* opt, float* d_path_out, int32_t* d_index_out, float* d_cost_out,
                                      int32_t* d_reachable_out, float* d_node_cost_out, void* stream) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_path_search: null model");
  bool nothing = false;
  ikf_status st = path_check(m, "ikf_path_search", T, k, opt, d_waypoints, d_q, d_path_out, d_index_out, d_cost_out, &nothing);
  if (st != IKF_OK || nothing) return st;
  IKF_ON_DEVICE(m)
  st = ensure_path_scratch(m, T * (long long)k);
  if (st != IKF_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  st = run_path(m, d_waypoints, T, k, d_q, d_q_start, opt, d_path_out, d_index_out, d_cost_out, d_reachable_out, d_node_cost_out, s);
  if (st != IKF_OK) return st;
  IKF_HIP(scope.leave());
  return IKF_OK;
}

extern "C" ikf_status ikf_generate_path(ikf_model* m, const float* d_waypoints, int64_t T, int k, const float* d_latent, int shared_latent,
                                        int clamp_to_limits, const float* d_q_start, const ikf_path_options* opt, float* d_path_out,
                                        int32_t* d_index_out, float* d_cost_out, int32_t* d_reachable_out, float* d_node_cost_out, void* stream) {
  ikf_status st = check_ready(m, "ikf_generate_path");
  if (st != IKF_OK) return st;
  bool nothing = false;
  st = path_check(m, "ikf_generate_path", T, k, opt, d_waypoints, d_latent, d_path_out, d_index_out, d_cost_out, &nothing);
  if (st != IKF_OK || nothing) return st;
  IKF_ON_DEVICE(m)
  const long long rows = T * (long long)k;
  st = ensure_rank_rows(m, rows);
  if (st == IKF_OK) st = ensure_path_scratch(m, rows);
  if (st == IKF_OK && shared_latent) st = ensure_path_latent(m, rows);
  if (st != IKF_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  if (shared_latent) {
    IKF_HIP(launch_path_expand_latent(d_latent, k, T, m->dims.D, m->pt_latent, s));
    d_latent = m->pt_latent;
  }
  // the conditional of row r * T + t is waypoint t: the tiling pose source of the exact path, without an index list
  const PoseSource ps{d_waypoints, nullptr, (long long)T, 7, 0.0f};
  st = run_flow_guarded(m, ps, d_latent, rows, clamp_to_limits ? 1 : 0, m->rk_q, s);
  if (st != IKF_OK) return st;
  st = run_path(m, d_waypoints, T, k, m->rk_q, d_q_start, opt, d_path_out, d_index_out, d_cost_out, d_reachable_out, d_node_cost_out, s);
  if (st != IKF_OK) return st;
  IKF_HIP(scope.leave());
  return IKF_OK;
}

extern "C" ikf_status ikf_reserve_path(ikf_model* m, int64_t max_waypoints, int max_k) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_reserve_path: null model");
  if (max_waypoints < 1 || max_k < 1 || max_k > IKF_PATH_MAX_K || max_waypoints > 0x7fffffffLL || max_waypoints * (long long)max_k > 0x7fffffffLL)
    return fail(IKF_ERR_BAD_ARGUMENT, "ikf_reserve_path: max_waypoints must be positive and max_k in 1 .. 256 (product < 2^31)");
  IKF_ON_DEVICE(m)
  const long long rows = max_waypoints * (long long)max_k;
  ikf_status st = ensure_rank_rows(m, rows);
  if (st == IKF_OK) st = ensure_path_scratch(m, rows);
  if (st == IKF_OK) st = ensure_rank_lists(m, max_waypoints);
  if (st == IKF_OK && m->loaded) st = ensure_path_latent(m, rows);
  if (st == IKF_OK && m->loaded) st = ikf_reserve(m, rows);   // the flow's scratch (and, where that path can be reached, its weight image)
  return st;
}
