// C-ABI of libikflow_amd.so, path IK (include/ikflow_amd_path.h): k candidates per waypoint - the caller's, or the flow's through the tiling
// pose source of the exact path - scored by the ranking kernel and searched by k_path_lattice (path_kernels.hip).  The frame of api_rank.hip: stream
// scope, handle-owned buffers grown on demand (the candidate rows are the ranking's), nothing read back to the host.  The last section is the same
// for P paths per call (include/ikflow_amd_path_batch.h): the candidate stage on P * T waypoints, the BATCH forms of the sweep and the lattice.
#include "ikf_model.h"

// node costs [rows] and back-pointers (a byte per node) of a lattice of up to `rows` nodes
static ikf_status ensure_path_scratch(ikf_model* m, long long rows) {
  IKF_HIP(m->pt_node.ensure(rows));
  IKF_HIP(m->pt_bp.ensure(path_bp_bytes(rows, 1)));
  return IKF_OK;
}
// the sweep's verdicts of a lattice of up to `rows` nodes of k candidates each (sweep_math.h): rows * ceil(k / 64) words
static ikf_status ensure_path_mask(ikf_model* m, long long rows, int k) {
  IKF_HIP(m->pt_edge_free.ensure(rows * sweep_words(k)));
  return IKF_OK;
}
// the shared latent expanded to one row per candidate row
static ikf_status ensure_path_latent(ikf_model* m, long long rows) {
  IKF_HIP(m->pt_latent.ensure(rows * m->dims.D));
  return IKF_OK;
}

// path IK's own rule; the pointers both of its entries need
static ikf_status path_check(ikf_model* m, const char* who, int64_t T, int k, const ikf_path_options* opt, const void* d_waypoints,
                             const void* d_rows, const void* d_path_out, const void* d_index_out, const void* d_cost_out, bool* nothing_to_do) {
  const bool bad_weight = opt && !(opt->node_weight >= 0.f);
  return check_candidates(m, who, "T", T, k, IKF_PATH_MAX_K, opt, opt && opt->reject_collisions, bad_weight ? "node_weight must be >= 0" : nullptr,
                          d_waypoints && d_rows && d_path_out && d_index_out && d_cost_out, nothing_to_do);
}

// P == 0: one path of T waypoints.  P > 0 (include/ikflow_amd_path_batch.h): P paths of T waypoints in one candidate layout of n = P * T waypoints -
// the candidate stage sees n poses, the sweep and the lattice are told where one path ends and the next begins (no world track: refused by the entries).
static ikf_status run_path(ikf_model* m, const float* d_waypoints, int64_t P, int64_t T, int k, const float* d_q, const float* d_q_start,
                           const ikf_path_options* opt, float* d_path_out, int32_t* d_index_out, float* d_cost_out, int32_t* d_reachable_out,
                           float* d_node_cost_out, hipStream_t s) {
  // Node costs: the ranking kernel itself, the waypoints as its poses, n_keep = 1 - so node[t][r] IS ikf_rank_candidates' row score of the row.
  // Its one kept row per waypoint goes to d_path_out, which the lattice launch behind it overwrites in full.
  const int64_t n = P > 0 ? P * T : T;
  float* const node = d_node_cost_out ? d_node_cost_out : m->pt_node.p;
  ikf_status st = score_candidates(m, d_waypoints, n, k, d_q, nullptr, scoring_options(*opt), d_path_out, nullptr, nullptr, nullptr, node, s);
  if (st != IKF_OK) return st;
  st = track_mask_nodes(m, d_q, n, k, node, s);   // a world track: +inf in place where a row hits its waypoint's key frame; nothing without one
  if (st != IKF_OK) return st;
  PathArgs a{};
  a.P = (int)P;
  a.q = d_q;
  a.q_start = d_q_start;
  a.opt = *opt;
  a.T = (int)T;
  a.k = k;
  a.node = node;
  a.bp = m->pt_bp.p;
  a.path_out = d_path_out;
  a.index_out = d_index_out;
  a.cost_out = d_cost_out;
  a.reachable_out = d_reachable_out;
  if (path_sweeps(m, opt)) {   // the edges of the lattice, S samples each, between the node stage and the search; the mask was sized by the caller
    SweepArgs w{};
    w.ch = m->d_chain;
    w.cm = m->d_collision;
    w.world = m->d_world;
    w.n_obs = m->world_n;
    w.n_caps = m->n_caps;
    w.world_min_clearance = m->world_min_clearance;
    w.reject_self = opt->reject_collisions ? 1 : 0;
    w.self_min_clearance = opt->min_clearance;
    w.n_samples = m->path_sweep;
    w.lattice = 1;
    w.q = d_q;
    w.q_start = d_q_start;
    w.node = node;
    w.T = (int)T;
    w.P = (int)P;
    w.k = k;
    w.max_joint_step = opt->max_joint_step;
    w.edge_free = m->pt_edge_free.p;
    track_fill_sweep(m, &w);
    IKF_HIP(prof_mark(m, s));   // bracketed like the sequential stage (tools/sweep_timing.py)
    IKF_HIP(launch_sweep_edges(m->dims.ndof, w, s));
    IKF_HIP(prof_mark(m, s));
    a.edge_free = m->pt_edge_free.p;
  }
  IKF_HIP(prof_mark(m, s));   // between ikf_profile_begin / _end the sequential stage is bracketed (tools/path_timing.py); otherwise nothing is recorded
  IKF_HIP(launch_path_lattice(m->dims.ndof, a, s));
  IKF_HIP(prof_mark(m, s));
  // the path optimiser behind the lattice while it is set on the handle (include/ikflow_amd_path_opt.h): path_out and cost_out in place
  if (m->popt_iters > 0) return path_opt_behind(m, d_waypoints, P > 0 ? P : 1, T, d_q_start, opt, d_path_out, d_cost_out, s);
  return IKF_OK;
}

extern "C" ikf_status ikf_path_search(ikf_model* m, const float* d_waypoints, int64_t T, int k, const float* d_q, const float* d_q_start,
                                      const ikf_path_options* opt, float* d_path_out, int32_t* d_index_out, float* d_cost_out,
                                      int32_t* d_reachable_out, float* d_node_cost_out, void* stream) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_path_search: null model");
  bool nothing = false;
  ikf_status st = path_check(m, "ikf_path_search", T, k, opt, d_waypoints, d_q, d_path_out, d_index_out, d_cost_out, &nothing);
  if (st != IKF_OK || nothing) return st;
  st = track_check_T(m, "ikf_path_search", T);
  if (st != IKF_OK) return st;
  IKF_ON_DEVICE(m)
  st = ensure_path_scratch(m, T * (long long)k);
  if (st == IKF_OK && path_sweeps(m, opt)) st = ensure_path_mask(m, T * (long long)k, k);
  if (st == IKF_OK && m->popt_iters > 0) st = path_opt_ensure(m, 1, T, opt);
  if (st != IKF_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  st = run_path(m, d_waypoints, 0, T, k, d_q, d_q_start, opt, d_path_out, d_index_out, d_cost_out, d_reachable_out, d_node_cost_out, s);
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
  st = track_check_T(m, "ikf_generate_path", T);
  if (st != IKF_OK) return st;
  IKF_ON_DEVICE(m)
  const long long rows = T * (long long)k;
  st = ensure_rank_rows(m, rows);
  if (st == IKF_OK) st = ensure_path_scratch(m, rows);
  if (st == IKF_OK && shared_latent) st = ensure_path_latent(m, rows);
  if (st == IKF_OK && path_sweeps(m, opt)) st = ensure_path_mask(m, rows, k);
  if (st == IKF_OK && m->popt_iters > 0) st = path_opt_ensure(m, 1, T, opt);
  if (st != IKF_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  if (shared_latent) {
    IKF_HIP(launch_path_expand_latent(d_latent, k, T, m->dims.D, m->pt_latent.p, s));
    d_latent = m->pt_latent.p;
  }
  st = flow_candidates(m, d_waypoints, T, k, d_latent, clamp_to_limits, s);
  if (st != IKF_OK) return st;
  st = run_path(m, d_waypoints, 0, T, k, m->rk_q.p, d_q_start, opt, d_path_out, d_index_out, d_cost_out, d_reachable_out, d_node_cost_out, s);
  if (st != IKF_OK) return st;
  IKF_HIP(scope.leave());
  return IKF_OK;
}

extern "C" ikf_status ikf_reserve_path(ikf_model* m, int64_t max_waypoints, int max_k) {
  ikf_status st = reserve_candidates(m, "ikf_reserve_path", "max_waypoints must be positive and max_k in 1 .. 256 (product < 2^31)", max_waypoints,
                                     max_k, IKF_PATH_MAX_K);
  if (st != IKF_OK) return st;
  IKF_ON_DEVICE(m)
  const long long rows = max_waypoints * (long long)max_k;
  st = ensure_path_scratch(m, rows);
  if (st == IKF_OK && m->loaded) st = ensure_path_latent(m, rows);
  if (st == IKF_OK && m->path_sweep > 0) st = ensure_path_mask(m, rows, max_k);   // (a sweep set later sizes its mask at the first call)
  if (st == IKF_OK && m->track_F > 0) {   // a world track set by now: the zero node costs of ikf_sweep_lattice (its fine table was sized when it was set)
    IKF_HIP(m->tk_zero_node.ensure(rows));
  }
  return st;
}

// ---- P paths per call (include/ikflow_amd_path_batch.h): the candidate stage with n = P * T poses, one lattice workgroup per path --------------------

// node costs [k * P * T] and P blocks of back-pointers (path_batch_math.h); both monotone in P, T and k, so a reservation covers every smaller call
static ikf_status ensure_path_batch_scratch(ikf_model* m, long long P, long long T, int k) {
  IKF_HIP(m->pt_node.ensure(P * T * k));
  IKF_HIP(m->pt_bp.ensure(path_batch_bp_bytes(P, T, k)));
  return IKF_OK;
}
// P * T as the candidate stage's pose count: -1 when either is negative, 0 when either is 0, 2^31 (refused as too large) beyond the range
static int64_t path_batch_count(int64_t P, int64_t T) {
  if (P < 0 || T < 0) return -1;
  if (P == 0 || T == 0) return 0;
  if (P > 0x7fffffffLL || T > 0x7fffffffLL || P * T > 0x7fffffffLL) return 0x80000000LL;
  return P * T;
}
// the checks of a single path call on P * T waypoints, then the one rule of the batch: no world track
static ikf_status path_batch_check(ikf_model* m, const char* who, int64_t P, int64_t T, int k, const ikf_path_options* opt, const void* d_waypoints,
                                   const void* d_rows, const void* d_path_out, const void* d_index_out, const void* d_cost_out, bool* nothing_to_do) {
  const bool bad_weight = opt && !(opt->node_weight >= 0.f);
  ikf_status st = check_candidates(m, who, "P * T", path_batch_count(P, T), k, IKF_PATH_MAX_K, opt, opt && opt->reject_collisions,
                                   bad_weight ? "node_weight must be >= 0" : nullptr,
                                   d_waypoints && d_rows && d_path_out && d_index_out && d_cost_out, nothing_to_do);
  if (st != IKF_OK || *nothing_to_do) return st;
  if (m->track_F > 0)
    return fail(IKF_ERR_BAD_ARGUMENT, std::string(who) + ": a world track is set (ikf_set_world_track); frames per batched path are not covered - "
                                                         "clear the track or call the single-path entry per path");
  return IKF_OK;
}

extern "C" ikf_status ikf_path_search_batch(ikf_model* m, const float* d_waypoints, int64_t P, int64_t T, int k, const float* d_q,
                                            const float* d_q_start, const ikf_path_options* opt, float* d_path_out, int32_t* d_index_out,
                                            float* d_cost_out, int32_t* d_reachable_out, float* d_node_cost_out, void* stream) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_path_search_batch: null model");
  bool nothing = false;
  ikf_status st = path_batch_check(m, "ikf_path_search_batch", P, T, k, opt, d_waypoints, d_q, d_path_out, d_index_out, d_cost_out, &nothing);
  if (st != IKF_OK || nothing) return st;
  IKF_ON_DEVICE(m)
  const long long rows = P * T * (long long)k;
  st = ensure_path_batch_scratch(m, P, T, k);
  if (st == IKF_OK && path_sweeps(m, opt)) st = ensure_path_mask(m, rows, k);
  if (st == IKF_OK && m->popt_iters > 0) st = path_opt_ensure(m, P, T, opt);
  if (st != IKF_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  st = run_path(m, d_waypoints, P, T, k, d_q, d_q_start, opt, d_path_out, d_index_out, d_cost_out, d_reachable_out, d_node_cost_out, s);
  if (st != IKF_OK) return st;
  IKF_HIP(scope.leave());
  return IKF_OK;
}

extern "C" ikf_status ikf_generate_path_batch(ikf_model* m, const float* d_waypoints, int64_t P, int64_t T, int k, const float* d_latent,
                                              int shared_latent, int clamp_to_limits, const float* d_q_start, const ikf_path_options* opt,
                                              float* d_path_out, int32_t* d_index_out, float* d_cost_out, int32_t* d_reachable_out,
                                              float* d_node_cost_out, void* stream) {
  ikf_status st = check_ready(m, "ikf_generate_path_batch");
  if (st != IKF_OK) return st;
  bool nothing = false;
  st = path_batch_check(m, "ikf_generate_path_batch", P, T, k, opt, d_waypoints, d_latent, d_path_out, d_index_out, d_cost_out, &nothing);
  if (st != IKF_OK || nothing) return st;
  IKF_ON_DEVICE(m)
  const long long n = P * T, rows = n * k;
  st = ensure_rank_rows(m, rows);
  if (st == IKF_OK) st = ensure_path_batch_scratch(m, P, T, k);
  if (st == IKF_OK && shared_latent) st = ensure_path_latent(m, rows);
  if (st == IKF_OK && path_sweeps(m, opt)) st = ensure_path_mask(m, rows, k);
  if (st == IKF_OK && m->popt_iters > 0) st = path_opt_ensure(m, P, T, opt);
  if (st != IKF_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  if (shared_latent) {   // candidate r uses latent r at every waypoint of every path: the single path's expansion over P * T waypoints
    IKF_HIP(launch_path_expand_latent(d_latent, k, n, m->dims.D, m->pt_latent.p, s));
    d_latent = m->pt_latent.p;
  }
  st = flow_candidates(m, d_waypoints, n, k, d_latent, clamp_to_limits, s);
  if (st != IKF_OK) return st;
  st = run_path(m, d_waypoints, P, T, k, m->rk_q.p, d_q_start, opt, d_path_out, d_index_out, d_cost_out, d_reachable_out, d_node_cost_out, s);
  if (st != IKF_OK) return st;
  IKF_HIP(scope.leave());
  return IKF_OK;
}

extern "C" ikf_status ikf_reserve_path_batch(ikf_model* m, int64_t max_paths, int64_t max_waypoints, int max_k) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_reserve_path_batch: null model");
  const char* const rule = "max_paths and max_waypoints must be positive and max_k in 1 .. 256 (product < 2^31)";
  if (max_paths < 1 || max_waypoints < 1) return fail(IKF_ERR_BAD_ARGUMENT, std::string("ikf_reserve_path_batch: ") + rule);
  ikf_status st = reserve_candidates(m, "ikf_reserve_path_batch", rule, path_batch_count(max_paths, max_waypoints), max_k, IKF_PATH_MAX_K);
  if (st != IKF_OK) return st;
  IKF_ON_DEVICE(m)
  const long long rows = max_paths * max_waypoints * (long long)max_k;
  st = ensure_path_batch_scratch(m, max_paths, max_waypoints, max_k);
  if (st == IKF_OK && m->loaded) st = ensure_path_latent(m, rows);
  if (st == IKF_OK && m->path_sweep > 0) st = ensure_path_mask(m, rows, max_k);   // (a sweep set later sizes its mask at the first call)
  return st;
}
