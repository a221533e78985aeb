// C-ABI of libikflow_amd.so, swept collision checks along edges (include/ikflow_amd_sweep.h): the samples per lattice edge of path IK as state of
// the handle, and the query on the caller's own edges (k_sweep_edges, sweep_kernels.hip, pair source).  What the sweep does to a path call is in
// run_path (api_path.hip).
#include "ikf_model.h"

extern "C" ikf_status ikf_set_path_sweep(ikf_model* m, int n_samples) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_set_path_sweep: null model");
  if (n_samples < 0 || n_samples > IKF_SWEEP_MAX_SAMPLES) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_path_sweep: n_samples must be in 0 .. 16");
  // a world track's fine frames are those of the sweep (include/ikflow_amd_track.h): rebuilt first, and a refused blend keeps the old value
  ikf_status st = track_rebuild(m, "ikf_set_path_sweep", n_samples);
  if (st != IKF_OK) return st;
  m->path_sweep = n_samples;
  return IKF_OK;
}

extern "C" int ikf_get_path_sweep(const ikf_model* m) { return m ? m->path_sweep : 0; }

extern "C" ikf_status ikf_sweep_edges(ikf_model* m, const float* d_q_a, const float* d_q_b, int64_t n, int n_samples, int reject_self,
                                      float self_min_clearance, uint8_t* d_blocked_out, int32_t* d_first_out, void* stream) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_sweep_edges: null model");
  if (n < 0) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_sweep_edges: n must be >= 0");
  if (n_samples < 1 || n_samples > IKF_SWEEP_MAX_SAMPLES) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_sweep_edges: n_samples must be in 1 .. 16");
  if (!m->d_collision) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_sweep_edges: no collision model has been set");
  if (n == 0) return IKF_OK;
  if (!d_q_a || !d_q_b) return fail(IKF_ERR_NULL_POINTER, "ikf_sweep_edges: null device pointer");
  if (!d_blocked_out && !d_first_out) return fail(IKF_ERR_NULL_POINTER, "ikf_sweep_edges: both outputs are null");
  IKF_ON_DEVICE(m)
  SweepArgs a{};
  a.ch = m->d_chain;
  a.cm = m->d_collision;
  a.world = m->d_world;
  a.n_obs = m->world_n;
  a.n_caps = m->n_caps;
  a.world_min_clearance = m->world_min_clearance;
  a.reject_self = reject_self ? 1 : 0;
  a.self_min_clearance = self_min_clearance;
  a.n_samples = n_samples;
  a.qa = d_q_a;
  a.qb = d_q_b;
  a.n = n;
  a.blocked_out = d_blocked_out;
  a.first_out = d_first_out;
  IKF_HIP(launch_sweep_edges(m->dims.ndof, a, static_cast<hipStream_t>(stream)));
  return IKF_OK;
}
