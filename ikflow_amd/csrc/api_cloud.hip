// C-ABI of libikflow_amd.so, world point cloud (include/ikflow_amd_cloud.h): the sensed scene as state of the handle, validated and padded on the
// host, and the per-row clearance query (k_cloud_clearance / k_cloud_merge, cloud_kernels.hip).  What the cloud does to the selection entry
// points is in score_candidates (api_rank.hip).
#include "ikf_model.h"

extern "C" ikf_status ikf_set_world_cloud(ikf_model* m, const float* h_points, int64_t n_points, float point_radius, float min_clearance) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_set_world_cloud: null model");
  if (n_points < 0 || n_points > IKF_CLOUD_MAX_POINTS) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_world_cloud: n_points must be in 0 .. 1048576");
  if (!std::isfinite(point_radius) || point_radius < 0.f) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_world_cloud: point_radius must be finite and >= 0");
  if (!std::isfinite(min_clearance)) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_world_cloud: min_clearance must be finite");
  if (n_points == 0) {   // clears; the array stays allocated for the next cloud
    m->cloud_n = 0;
    m->cloud_radius = point_radius;
    m->cloud_min_clearance = min_clearance;
    return IKF_OK;
  }
  if (!h_points) return fail(IKF_ERR_NULL_POINTER, "ikf_set_world_cloud: null point table");
  if (!m->d_collision) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_world_cloud: points without a collision model (ikf_set_collision_model)");
  const long long padded = cloud_tiles(n_points) * IKF_CLOUD_TILE;
  std::vector<CloudPoint> host((size_t)padded);
  for (long long i = 0; i < n_points; ++i) {
    const float* p = h_points + 3 * i;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]))
      return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_world_cloud: point " + std::to_string(i) + ": non-finite coordinate");
    host[(size_t)i] = CloudPoint{p[0], p[1], p[2], 0.f};
  }
  for (long long i = n_points; i < padded; ++i) host[(size_t)i] = host[(size_t)n_points - 1];   // a duplicate cannot change a minimum
  IKF_ON_DEVICE(m)
  if (padded > m->d_cloud.cap) m->cloud_n = 0;   // (the array is about to be replaced: should that fail, the handle has no cloud)
  IKF_HIP(m->d_cloud.ensure(padded));
  IKF_HIP(hipMemcpy(m->d_cloud, host.data(), sizeof(CloudPoint) * (size_t)padded, hipMemcpyHostToDevice));
  m->cloud_n = n_points;
  m->cloud_radius = point_radius;
  m->cloud_min_clearance = min_clearance;
  return IKF_OK;
}

extern "C" int64_t ikf_world_cloud_size(const ikf_model* m) { return m ? m->cloud_n : 0; }

ikf_status ikf::ensure_cloud_partials(ikf_model* m, long long rows) {
  // (a cloud of one tile never splits; otherwise the bound of every call up to `rows`, not this call's plan: a smaller call may split further)
  if (m->cloud_n > IKF_CLOUD_TILE) IKF_HIP(m->cloud_part.ensure(cloud_partial_bound(rows, m->n_cu)));
  return IKF_OK;
}

ikf_status ikf::run_cloud_clearance(ikf_model* m, const float* d_q, long long rows, float* d_clearance, uint8_t* d_colliding, hipStream_t s) {
  ikf_status st = ensure_cloud_partials(m, rows);   // (sized by a reservation: allocates only without one)
  if (st != IKF_OK) return st;
  IKF_HIP(launch_cloud_clearance(m->d_chain, m->d_collision, m->n_caps, m->d_cloud, m->cloud_n, m->cloud_radius, m->cloud_min_clearance,
                                 m->dims.ndof, d_q, rows, m->n_cu, d_clearance, d_colliding, m->cloud_part.p, s));
  return IKF_OK;
}

extern "C" ikf_status ikf_cloud_clearance(ikf_model* m, const float* d_q, int64_t n, float* d_clearance_out, uint8_t* d_colliding_out, void* stream) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_cloud_clearance: null model");
  if (n < 0) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_cloud_clearance: n must be >= 0");
  if (!m->d_collision) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_cloud_clearance: no collision model has been set");
  if (n == 0) return IKF_OK;
  if (!d_q) return fail(IKF_ERR_NULL_POINTER, "ikf_cloud_clearance: null device pointer");
  IKF_ON_DEVICE(m)
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);   // (the partial minima are the handle's: a call on another stream waits for the one before)
  IKF_HIP(scope.enter());
  ikf_status st = run_cloud_clearance(m, d_q, n, d_clearance_out, d_colliding_out, s);
  if (st != IKF_OK) return st;
  IKF_HIP(scope.leave());
  return IKF_OK;
}
