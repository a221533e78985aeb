// C-ABI of libikflow_amd.so, world collision (include/ikflow_amd_world.h): the caller's obstacles as state of the handle, validated and normalised
// on the host, and the per-row clearance query (k_world_clearance, world_kernels.hip).  What the obstacles do to the selection entry points is
// in score_candidates (api_rank.hip).
#include "ikf_model.h"

static bool all_finite(const float* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

extern "C" ikf_status ikf_set_world(ikf_model* m, const ikf_obstacle* h_obstacles, int n_obstacles, float min_clearance) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_set_world: null model");
  if (n_obstacles < 0 || n_obstacles > IKF_WORLD_MAX_OBSTACLES) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_world: n_obstacles must be in 0 .. 64");
  if (!std::isfinite(min_clearance)) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_world: min_clearance must be finite");
  if (n_obstacles == 0) {   // clears; the table stays allocated for the next world
    m->world_n = 0;
    m->world_min_clearance = min_clearance;
    return IKF_OK;
  }
  if (!h_obstacles) return fail(IKF_ERR_NULL_POINTER, "ikf_set_world: null obstacle table");
  if (!m->d_collision) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_world: obstacles without a collision model (ikf_set_collision_model)");
  std::vector<WorldModel> host(1);   // (4 KB: not on the stack of a caller's thread)
  WorldModel& wm = host[0];
  memset(&wm, 0, sizeof(wm));
  wm.n = n_obstacles;
  for (int i = 0; i < n_obstacles; ++i) {
    const ikf_obstacle& in = h_obstacles[i];
    const std::string who = "ikf_set_world: obstacle " + std::to_string(i);
    if (in.kind < IKF_OBSTACLE_SPHERE || in.kind > IKF_OBSTACLE_BOX) return fail(IKF_ERR_BAD_ARGUMENT, who + ": unknown kind " + std::to_string(in.kind));
    if (!all_finite(in.a, 3) || !all_finite(in.b, 3) || !all_finite(in.quat, 4) || !std::isfinite(in.radius))
      return fail(IKF_ERR_BAD_ARGUMENT, who + ": non-finite number");
    if (in.radius < 0.f) return fail(IKF_ERR_BAD_ARGUMENT, who + ": radius must be >= 0");
    WorldObstacle& o = wm.obs[i];
    o.kind = in.kind;
    o.radius = in.radius;
    for (int c = 0; c < 3; ++c) { o.a[c] = in.a[c]; o.b[c] = in.b[c]; }
    o.quat[0] = 1.f;
    if (in.kind == IKF_OBSTACLE_HALF_SPACE) {
      const double nn = std::sqrt((double)in.a[0] * in.a[0] + (double)in.a[1] * in.a[1] + (double)in.a[2] * in.a[2]);
      if (!(nn > 0.0)) return fail(IKF_ERR_BAD_ARGUMENT, who + ": zero normal");
      for (int c = 0; c < 3; ++c) o.a[c] = (float)(in.a[c] / nn);
      o.b[0] = (float)(in.b[0] / nn);   // n.x <= d describes the same solid after both sides are divided by |n|
    } else if (in.kind == IKF_OBSTACLE_BOX) {
      if (!(in.b[0] > 0.f) || !(in.b[1] > 0.f) || !(in.b[2] > 0.f)) return fail(IKF_ERR_BAD_ARGUMENT, who + ": half extents must be > 0");
      double qq = 0.0;
      for (int c = 0; c < 4; ++c) qq += (double)in.quat[c] * in.quat[c];
      if (!(qq > 0.0)) return fail(IKF_ERR_BAD_ARGUMENT, who + ": zero quaternion");
      for (int c = 0; c < 4; ++c) o.quat[c] = (float)(in.quat[c] / std::sqrt(qq));
    }
  }
  IKF_ON_DEVICE(m)
  IKF_HIP(m->d_world.ensure(1));
  IKF_HIP(hipMemcpy(m->d_world, &wm, sizeof(WorldModel), hipMemcpyHostToDevice));
  m->world_n = n_obstacles;
  m->world_min_clearance = min_clearance;
  return IKF_OK;
}

extern "C" int ikf_world_size(const ikf_model* m) { return m ? m->world_n : 0; }

extern "C" ikf_status ikf_world_clearance(ikf_model* m, const float* d_q, int64_t n, float* d_clearance_out, int32_t* d_obstacle_out,
                                          int32_t* d_capsule_out, uint8_t* d_colliding_out, void* stream) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_world_clearance: null model");
  if (n < 0) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_world_clearance: n must be >= 0");
  if (!m->d_collision) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_world_clearance: no collision model has been set");
  if (n == 0) return IKF_OK;
  if (!d_q) return fail(IKF_ERR_NULL_POINTER, "ikf_world_clearance: null device pointer");
  IKF_ON_DEVICE(m)
  IKF_HIP(launch_world_clearance(m->d_chain, m->d_collision, m->n_caps, m->d_world, m->world_n, m->world_min_clearance, m->dims.ndof, d_q, n,
                                 d_clearance_out, d_obstacle_out, d_capsule_out, d_colliding_out, static_cast<hipStream_t>(stream)));
  return IKF_OK;
}
