// C-ABI of libikflow_amd.so, the path optimiser (include/ikflow_amd_path_opt.h): the caller's own paths through k_path_opt and the evaluator
// (path_opt_kernels.hip), the evaluator alone as a query, the state that puts the optimiser behind every lattice (api_path.hip calls
// path_opt_ensure / path_opt_behind), the info words and the reservation.  The frame of api_path.hip: stream scope, handle-owned buffers grown on
// demand, nothing read back to the host by a call.
//
// The evaluator is the lattice's own code on a lattice of k = 1: score_candidates with one row per waypoint (so candidate refinement, which
// flow_candidates applies to the flow's rows, never touches an optimised row), track_mask_nodes, and the LATTICE source of k_sweep_edges with
// k = 1 - one mask word per waypoint, bit 0 the edge that ends there - which carries the world track and the start edge exactly as a path call
// does.  k_path_opt_commit folds them.
#include "ikf_model.h"
#include "path_opt_math.h"

static ikf_status ensure_path_opt(ikf_model* m, long long P, long long T, bool sweeps) {
  const long long n = P * T;
  const int nd = m->dims.ndof;
  IKF_HIP(m->po_q.ensure(path_opt_iterate_floats(P, T, nd)));
  IKF_HIP(m->po_prev.ensure(path_opt_iterate_floats(P, T, nd)));
  IKF_HIP(m->po_keep.ensure(n * nd));
  IKF_HIP(m->po_work.ensure(path_opt_scratch_doubles(P, T, nd)));
  IKF_HIP(m->po_node_in.ensure(n));
  IKF_HIP(m->po_node_opt.ensure(n));
  if (sweeps) {
    IKF_HIP(m->po_edge_in.ensure(n));
    IKF_HIP(m->po_edge_opt.ensure(n));
  }
  IKF_HIP(m->po_iters.ensure(P));
  IKF_HIP(m->po_info.ensure(P * 4));
  // what score_candidates needs for n rows under the rules set now (api_rank.hip)
  if (m->cloud_n > 0 || m->manip_min > 0.f) IKF_HIP(m->cloud_row.ensure(n));
  if (m->cloud_n > 0) return ensure_cloud_partials(m, n);
  return IKF_OK;
}

// node scores [P * T] and - `edge` non-null - mask words [P * T] of one row per waypoint, by the lattice's own stages
static ikf_status evaluate_rows(ikf_model* m, const float* d_waypoints, long long P, long long T, const float* d_path, const float* d_q_start,
                                const ikf_path_options* opt, float* node, uint64_t* edge, hipStream_t s) {
  const long long n = P * T;
  ikf_status st = score_candidates(m, d_waypoints, n, 1, d_path, nullptr, scoring_options(*opt), m->po_keep.p, nullptr, nullptr, nullptr, node, s);
  if (st != IKF_OK) return st;
  st = track_mask_nodes(m, d_path, n, 1, node, s);   // (a track: P == 1, the entries have seen to it)
  if (st != IKF_OK || !edge) return st;
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
  w.q = d_path;
  w.q_start = d_q_start;
  w.node = node;
  w.T = (int)T;
  w.P = P > 1 ? (int)P : 0;   // (one path: the single lattice's form, the one a world track runs under)
  w.k = 1;
  w.max_joint_step = opt->max_joint_step;
  w.edge_free = edge;
  track_fill_sweep(m, &w);
  IKF_HIP(launch_sweep_edges(m->dims.ndof, w, s));
  return IKF_OK;
}

// optimise, evaluate, commit; d_path_out may be d_path_in.  skip_cost: PathOptArgs::skip_cost.
static ikf_status run_path_opt(ikf_model* m, const float* d_waypoints, long long P, long long T, const float* d_path_in, const float* d_q_start,
                               const ikf_path_options* opt, int n_iters, float smooth_weight, int validate, const float* d_skip_cost,
                               float* d_path_out, float* d_cost_out, int32_t* d_info_out, hipStream_t s) {
  const bool sweeps = path_sweeps(m, opt);
  if (validate) {
    ikf_status st = evaluate_rows(m, d_waypoints, P, T, d_path_in, d_q_start, opt, m->po_node_in.p, sweeps ? m->po_edge_in.p : nullptr, s);
    if (st != IKF_OK) return st;
  }
  PathOptArgs a{};
  a.ch = m->d_chain;
  a.waypoints = d_waypoints;
  a.path_in = d_path_in;
  a.q_start = d_q_start;
  a.skip_cost = d_skip_cost;
  a.P = (int)P;
  a.T = (int)T;
  a.n_iters = n_iters;
  a.w = (double)smooth_weight;
  a.q = m->po_q.p;
  a.q_prev = m->po_prev.p;
  a.work = m->po_work.p;
  a.iters_out = m->po_iters.p;
  IKF_HIP(prof_mark(m, s));   // between ikf_profile_begin / _end the optimiser's launch is bracketed (tools/path_opt_timing.py)
  IKF_HIP(launch_path_opt(m->dims.ndof, a, s));
  IKF_HIP(prof_mark(m, s));
  ikf_status st = evaluate_rows(m, d_waypoints, P, T, m->po_q.p, d_q_start, opt, m->po_node_opt.p, sweeps ? m->po_edge_opt.p : nullptr, s);
  if (st != IKF_OK) return st;
  PathOptCommitArgs c{};
  c.path_in = d_path_in;
  c.path_opt = m->po_q.p;
  c.q_start = d_q_start;
  c.node_in = m->po_node_in.p;
  c.edge_in = sweeps ? m->po_edge_in.p : nullptr;
  c.node_opt = m->po_node_opt.p;
  c.edge_opt = sweeps ? m->po_edge_opt.p : nullptr;
  c.iters = m->po_iters.p;
  c.skip_cost = d_skip_cost;
  c.P = (int)P;
  c.T = (int)T;
  c.node_weight = opt->node_weight;
  c.max_joint_step = opt->max_joint_step;
  c.validate = validate ? 1 : 0;
  c.path_out = d_path_out;
  c.cost_out = d_cost_out;
  c.info_out = d_info_out;
  c.info_keep = m->po_info.p;
  IKF_HIP(launch_path_opt_commit(m->dims.ndof, c, s));
  m->po_info_paths = P;
  return IKF_OK;
}

static const char* weight_fault(float w) { return (std::isfinite(w) && w >= 0.f) ? nullptr : "smooth_weight must be finite and >= 0"; }

// what ikf_path_optimize and ikf_path_cost check alike once the handle is there: options, P and T, the family's rule, P * T, reject_collisions
// without a collision model, the empty call, null pointers, the world track
static ikf_status path_opt_check(ikf_model* m, const char* who, int64_t P, int64_t T, const ikf_path_options* opt, const char* rule_fault,
                                 bool have_pointers, bool* nothing_to_do) {
  int64_t n = -1;
  if (P >= 0 && T >= 0) n = (P == 0 || T == 0) ? 0 : ((P > 0x7fffffffLL || T > 0x7fffffffLL || P * T > 0x7fffffffLL) ? 0x80000000LL : P * T);
  const bool bad_weight = opt && !(opt->node_weight >= 0.f);
  ikf_status st = check_candidates(m, who, "P * T", n, 1, 1, opt, opt && opt->reject_collisions,
                                   rule_fault ? rule_fault : (bad_weight ? "node_weight must be >= 0" : nullptr), have_pointers, nothing_to_do);
  if (st != IKF_OK || *nothing_to_do) return st;
  if (m->track_F > 0 && P > 1)
    return fail(IKF_ERR_BAD_ARGUMENT, std::string(who) + ": a world track is set (ikf_set_world_track); frames per batched path are not covered - "
                                                         "clear the track or call with P = 1 per path");
  return track_check_T(m, who, T);
}

extern "C" ikf_status ikf_path_optimize(ikf_model* m, const float* d_waypoints, int64_t P, int64_t T, const float* d_path_in, const float* d_q_start,
                                        const ikf_path_options* opt, int n_iters, float smooth_weight, int validate, float* d_path_out,
                                        float* d_cost_out, int32_t* d_info_out, void* stream) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_path_optimize: null model");
  const char* rule = (n_iters < 1 || n_iters > IKF_PATH_OPT_MAX_ITERS) ? "n_iters must be in 1 .. 32" : weight_fault(smooth_weight);
  bool nothing = false;
  ikf_status st = path_opt_check(m, "ikf_path_optimize", P, T, opt, rule, d_waypoints && d_path_in && d_path_out && d_cost_out, &nothing);
  if (st != IKF_OK || nothing) return st;
  IKF_ON_DEVICE(m)
  st = ensure_path_opt(m, P, T, path_sweeps(m, opt));
  if (st != IKF_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  st = run_path_opt(m, d_waypoints, P, T, d_path_in, d_q_start, opt, n_iters, smooth_weight, validate, nullptr, d_path_out, d_cost_out, d_info_out, s);
  if (st != IKF_OK) return st;
  IKF_HIP(scope.leave());
  return IKF_OK;
}

extern "C" ikf_status ikf_path_cost(ikf_model* m, const float* d_waypoints, int64_t P, int64_t T, const float* d_path, const float* d_q_start,
                                    const ikf_path_options* opt, float* d_cost_out, int32_t* d_info_out, void* stream) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_path_cost: null model");
  bool nothing = false;
  ikf_status st = path_opt_check(m, "ikf_path_cost", P, T, opt, nullptr, d_waypoints && d_path && d_cost_out, &nothing);
  if (st != IKF_OK || nothing) return st;
  IKF_ON_DEVICE(m)
  const bool sweeps = path_sweeps(m, opt);
  st = ensure_path_opt(m, P, T, sweeps);
  if (st != IKF_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  st = evaluate_rows(m, d_waypoints, P, T, d_path, d_q_start, opt, m->po_node_in.p, sweeps ? m->po_edge_in.p : nullptr, s);
  if (st != IKF_OK) return st;
  PathOptCommitArgs c{};
  c.path_in = d_path;
  c.q_start = d_q_start;
  c.node_in = m->po_node_in.p;
  c.edge_in = sweeps ? m->po_edge_in.p : nullptr;
  c.P = (int)P;
  c.T = (int)T;
  c.node_weight = opt->node_weight;
  c.max_joint_step = opt->max_joint_step;
  c.cost_out = d_cost_out;
  c.info_out = d_info_out;
  c.info_keep = m->po_info.p;
  IKF_HIP(launch_path_opt_commit(m->dims.ndof, c, s));
  m->po_info_paths = P;
  IKF_HIP(scope.leave());
  return IKF_OK;
}

extern "C" ikf_status ikf_set_path_optimize(ikf_model* m, int n_iters, float smooth_weight) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_set_path_optimize: null model");
  if (n_iters < 0 || n_iters > IKF_PATH_OPT_MAX_ITERS) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_path_optimize: n_iters must be in 0 .. 32");
  if (weight_fault(smooth_weight)) return fail(IKF_ERR_BAD_ARGUMENT, std::string("ikf_set_path_optimize: ") + weight_fault(smooth_weight));
  m->popt_iters = n_iters;
  m->popt_weight = n_iters ? smooth_weight : 0.f;
  return IKF_OK;
}

extern "C" ikf_status ikf_get_path_optimize(const ikf_model* m, int* n_iters_out, float* smooth_weight_out) {
  if (n_iters_out) *n_iters_out = m ? m->popt_iters : 0;
  if (smooth_weight_out) *smooth_weight_out = m ? m->popt_weight : 0.f;
  return m ? IKF_OK : fail(IKF_ERR_NULL_POINTER, "ikf_get_path_optimize: null model");
}

extern "C" ikf_status ikf_path_optimize_info(ikf_model* m, int64_t P, int32_t* h_info) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_path_optimize_info: null model");
  if (P < 0 || P > m->po_info_paths)
    return fail(IKF_ERR_BAD_ARGUMENT, "ikf_path_optimize_info: P must be in 0 .. " + std::to_string(m->po_info_paths) + ", the paths of the last optimising call");
  if (P == 0) return IKF_OK;
  if (!h_info) return fail(IKF_ERR_NULL_POINTER, "ikf_path_optimize_info: null output");
  IKF_ON_DEVICE(m)
  if (m->tail_valid) IKF_HIP(hipStreamSynchronize(m->tail_stream));   // the last call's work, whatever stream it went to
  IKF_HIP(hipMemcpy(h_info, m->po_info, sizeof(int32_t) * 4 * (size_t)P, hipMemcpyDeviceToHost));
  return IKF_OK;
}

extern "C" ikf_status ikf_reserve_path_opt(ikf_model* m, int64_t max_paths, int64_t max_waypoints) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_reserve_path_opt: null model");
  if (max_paths < 1 || max_waypoints < 1 || max_paths > 0x7fffffffLL || max_waypoints > 0x7fffffffLL || max_paths * max_waypoints > 0x7fffffffLL)
    return fail(IKF_ERR_BAD_ARGUMENT, "ikf_reserve_path_opt: max_paths and max_waypoints must be positive (product < 2^31)");
  IKF_ON_DEVICE(m)
  return ensure_path_opt(m, max_paths, max_waypoints, m->path_sweep > 0);   // (a sweep set later sizes its words at the first call)
}

namespace ikf {

ikf_status path_opt_ensure(ikf_model* m, long long P, long long T, const ikf_path_options* opt) { return ensure_path_opt(m, P, T, path_sweeps(m, opt)); }

ikf_status path_opt_behind(ikf_model* m, const float* d_waypoints, long long P, long long T, const float* d_q_start, const ikf_path_options* opt,
                           float* d_path, float* d_cost, hipStream_t s) {
  return run_path_opt(m, d_waypoints, P, T, d_path, d_q_start, opt, m->popt_iters, m->popt_weight, 1, d_cost, d_path, d_cost, nullptr, s);
}

}  // namespace ikf
