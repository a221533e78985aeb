// C-ABI of libikflow_amd.so, the world track (include/ikflow_amd_track.h): F key frames of obstacles as state of the handle, validated and
// normalised on the host as ikf_set_world does, the fine frames between them interpolated in double precision (track_math.h) and uploaded as one
// table; the per-row query against key frames (k_track_clearance, track_kernels.hip) and the lattice's edge mask as a query
// (k_sweep_edges, sweep_kernels.hip, lattice source).  What the track does to a path call is in run_path (api_path.hip), through the four
// functions at the end of this unit.
#include "ikf_model.h"

static bool all_finite(const float* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// The fine table of `keys` [F][n] under S samples per edge -> fine [track_fine_frames(F, S)][n]; host only, nothing of a handle is touched.
static ikf_status build_fine(const std::string& who, const std::vector<WorldObstacle>& keys, int F, int n, int S, std::vector<WorldObstacle>* fine) {
  fine->assign((size_t)track_fine_frames(F, S) * n, WorldObstacle{});
  for (int t = 0; t < F; ++t)
    for (int i = 0; i <= (t + 1 < F ? S : 0); ++i)
      for (int o = 0; o < n; ++o) {
        const WorldObstacle& a = keys[(size_t)t * n + o];
        const WorldObstacle& b = keys[(size_t)(t + 1 < F ? t + 1 : t) * n + o];
        if (!track_interpolate(a, b, i, S, &(*fine)[(size_t)track_fine_index(t, i, S) * n + o]))
          return fail(IKF_ERR_BAD_ARGUMENT, who + ": frame " + std::to_string(t) + " obstacle " + std::to_string(o) + ": the normal blended with frame " +
                                                std::to_string(t + 1) + "'s at sample " + std::to_string(i) + " of " + std::to_string(S) + " is shorter than 1e-6");
      }
  return IKF_OK;
}

static ikf_status upload_fine(ikf_model* m, const std::vector<WorldObstacle>& fine) {
  IKF_ON_DEVICE(m)
  IKF_HIP(m->d_track.ensure((long long)fine.size()));
  IKF_HIP(hipMemcpy(m->d_track, fine.data(), sizeof(WorldObstacle) * fine.size(), hipMemcpyHostToDevice));
  return IKF_OK;
}

extern "C" ikf_status ikf_set_world_track(ikf_model* m, const ikf_obstacle* h_frames, int n_frames, int n_obstacles, float min_clearance) {
  const std::string fn = "ikf_set_world_track";
  if (!m) return fail(IKF_ERR_NULL_POINTER, fn + ": null model");
  if (n_frames < 0 || n_frames > IKF_WORLD_TRACK_MAX_FRAMES) return fail(IKF_ERR_BAD_ARGUMENT, fn + ": n_frames must be in 0 .. 1024");
  if (n_frames == 0) {   // clears; the tables stay allocated for the next track
    m->track_F = 0;
    m->track_n = 0;
    m->track_keys.clear();
    m->track_fine.clear();
    return IKF_OK;
  }
  if (n_obstacles < 1 || n_obstacles > IKF_WORLD_MAX_OBSTACLES) return fail(IKF_ERR_BAD_ARGUMENT, fn + ": n_obstacles must be in 1 .. 64");
  if (!std::isfinite(min_clearance)) return fail(IKF_ERR_BAD_ARGUMENT, fn + ": min_clearance must be finite");
  if (!h_frames) return fail(IKF_ERR_NULL_POINTER, fn + ": null frame table");
  if (!m->d_collision) return fail(IKF_ERR_BAD_ARGUMENT, fn + ": a track without a collision model (ikf_set_collision_model)");
  std::vector<WorldObstacle> keys((size_t)n_frames * n_obstacles, WorldObstacle{});
  for (int t = 0; t < n_frames; ++t)
    for (int i = 0; i < n_obstacles; ++i) {
      const ikf_obstacle& in = h_frames[(size_t)t * n_obstacles + i];
      const std::string who = fn + ": frame " + std::to_string(t) + " obstacle " + std::to_string(i);
      if (in.kind < IKF_OBSTACLE_SPHERE || in.kind > IKF_OBSTACLE_BOX) return fail(IKF_ERR_BAD_ARGUMENT, who + ": unknown kind " + std::to_string(in.kind));
      if (in.kind != h_frames[i].kind)
        return fail(IKF_ERR_BAD_ARGUMENT, who + ": kind " + std::to_string(in.kind) + " differs from frame 0's kind " + std::to_string(h_frames[i].kind));
      if (!all_finite(in.a, 3) || !all_finite(in.b, 3) || !all_finite(in.quat, 4) || !std::isfinite(in.radius))
        return fail(IKF_ERR_BAD_ARGUMENT, who + ": non-finite number");
      if (in.radius < 0.f) return fail(IKF_ERR_BAD_ARGUMENT, who + ": radius must be >= 0");
      WorldObstacle& o = keys[(size_t)t * n_obstacles + i];   // normalised exactly as ikf_set_world does
      o.kind = in.kind;
      o.radius = in.radius;
      for (int c = 0; c < 3; ++c) { o.a[c] = in.a[c]; o.b[c] = in.b[c]; }
      o.quat[0] = 1.f;
      if (in.kind == IKF_OBSTACLE_HALF_SPACE) {
        const double nn = std::sqrt((double)in.a[0] * in.a[0] + (double)in.a[1] * in.a[1] + (double)in.a[2] * in.a[2]);
        if (!(nn > 0.0)) return fail(IKF_ERR_BAD_ARGUMENT, who + ": zero normal");
        for (int c = 0; c < 3; ++c) o.a[c] = (float)(in.a[c] / nn);
        o.b[0] = (float)(in.b[0] / nn);
      } else if (in.kind == IKF_OBSTACLE_BOX) {
        if (!(in.b[0] > 0.f) || !(in.b[1] > 0.f) || !(in.b[2] > 0.f)) return fail(IKF_ERR_BAD_ARGUMENT, who + ": half extents must be > 0");
        double qq = 0.0;
        for (int c = 0; c < 4; ++c) qq += (double)in.quat[c] * in.quat[c];
        if (!(qq > 0.0)) return fail(IKF_ERR_BAD_ARGUMENT, who + ": zero quaternion");
        for (int c = 0; c < 4; ++c) o.quat[c] = (float)(in.quat[c] / std::sqrt(qq));
      }
    }
  std::vector<WorldObstacle> fine;
  ikf_status st = build_fine(fn, keys, n_frames, n_obstacles, m->path_sweep, &fine);
  if (st != IKF_OK) return st;   // (nothing of the handle has changed: the previous track stays in force)
  st = upload_fine(m, fine);
  if (st != IKF_OK) return st;
  m->track_keys.swap(keys);
  m->track_fine.swap(fine);
  m->track_F = n_frames;
  m->track_n = n_obstacles;
  m->track_S = m->path_sweep;
  m->track_min_clearance = min_clearance;
  return IKF_OK;
}

extern "C" ikf_status ikf_world_track_size(const ikf_model* m, int* n_frames, int* n_obstacles) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_world_track_size: null model");
  if (n_frames) *n_frames = m->track_F;
  if (n_obstacles) *n_obstacles = m->track_n;
  return IKF_OK;
}

extern "C" ikf_status ikf_world_track_frame(const ikf_model* m, int t, int i, ikf_obstacle* h_out) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_world_track_frame: null model");
  if (m->track_F == 0) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_world_track_frame: no track has been set");
  if (t < 0 || t >= m->track_F || i < 0 || i > m->track_S || (t == m->track_F - 1 && i != 0))
    return fail(IKF_ERR_BAD_ARGUMENT, "ikf_world_track_frame: t must be in 0 .. F - 1 and i in 0 .. S (0 behind the last key frame)");
  if (!h_out) return fail(IKF_ERR_NULL_POINTER, "ikf_world_track_frame: null output");
  const WorldObstacle* src = m->track_fine.data() + (size_t)track_fine_index(t, i, m->track_S) * m->track_n;
  for (int o = 0; o < m->track_n; ++o) {
    h_out[o].kind = src[o].kind;
    h_out[o].radius = src[o].radius;
    for (int c = 0; c < 3; ++c) { h_out[o].a[c] = src[o].a[c]; h_out[o].b[c] = src[o].b[c]; }
    for (int c = 0; c < 4; ++c) h_out[o].quat[c] = src[o].quat[c];
  }
  return IKF_OK;
}

// what the two queries share: T >= 0, k in 1 .. 256, k * T < 2^31
static ikf_status lattice_shape(const std::string& who, int64_t T, int k) {
  if (T < 0) return fail(IKF_ERR_BAD_ARGUMENT, who + ": T must be >= 0");
  if (k < 1 || k > IKF_PATH_MAX_K) return fail(IKF_ERR_BAD_ARGUMENT, who + ": k must be in 1 .. 256");
  if (T * (long long)k > 0x7fffffffLL) return fail(IKF_ERR_BAD_ARGUMENT, who + ": k * T must be < 2^31");
  return IKF_OK;
}

extern "C" ikf_status ikf_world_track_clearance(ikf_model* m, const float* d_q, int64_t T, int k, float* d_clearance_out, int32_t* d_obstacle_out,
                                                int32_t* d_capsule_out, uint8_t* d_colliding_out, void* stream) {
  const std::string fn = "ikf_world_track_clearance";
  if (!m) return fail(IKF_ERR_NULL_POINTER, fn + ": null model");
  ikf_status st = lattice_shape(fn, T, k);
  if (st != IKF_OK) return st;
  if (m->track_F == 0) return fail(IKF_ERR_BAD_ARGUMENT, fn + ": no track has been set");
  if (!m->d_collision) return fail(IKF_ERR_BAD_ARGUMENT, fn + ": no collision model has been set");
  st = track_check_T(m, fn, T);
  if (st != IKF_OK) return st;
  if (T == 0) return IKF_OK;
  if (!d_q) return fail(IKF_ERR_NULL_POINTER, fn + ": null device pointer");
  IKF_ON_DEVICE(m)
  TrackArgs a{};
  a.ch = m->d_chain;
  a.cm = m->d_collision;
  a.frames = m->d_track;
  a.n_obs = m->track_n;
  a.n_caps = m->n_caps;
  a.frame_stride = m->track_S + 1;
  a.min_clearance = m->track_min_clearance;
  a.q = d_q;
  a.T = (int)T;
  a.k = k;
  a.clearance = d_clearance_out;
  a.obstacle = d_obstacle_out;
  a.capsule = d_capsule_out;
  a.colliding = d_colliding_out;
  IKF_HIP(launch_track_clearance(m->dims.ndof, a, static_cast<hipStream_t>(stream)));
  return IKF_OK;
}

extern "C" ikf_status ikf_sweep_lattice(ikf_model* m, const float* d_q, int64_t T, int k, const float* d_q_start, int reject_self,
                                        float self_min_clearance, uint64_t* d_edge_free_out, void* stream) {
  const std::string fn = "ikf_sweep_lattice";
  if (!m) return fail(IKF_ERR_NULL_POINTER, fn + ": null model");
  ikf_status st = lattice_shape(fn, T, k);
  if (st != IKF_OK) return st;
  if (m->path_sweep < 1) return fail(IKF_ERR_BAD_ARGUMENT, fn + ": no sweep is set on the handle (ikf_set_path_sweep)");
  if (!m->d_collision) return fail(IKF_ERR_BAD_ARGUMENT, fn + ": no collision model has been set");
  st = track_check_T(m, fn, T);
  if (st != IKF_OK) return st;
  if (T == 0) return IKF_OK;
  if (!d_q || !d_edge_free_out) return fail(IKF_ERR_NULL_POINTER, fn + ": null device pointer");
  IKF_ON_DEVICE(m)
  const long long rows = T * (long long)k;
  IKF_HIP(m->tk_zero_node.ensure(rows));
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  IKF_HIP(hipMemsetAsync(m->tk_zero_node.p, 0, sizeof(float) * (size_t)rows, s));   // every node admissible: nothing is pruned
  SweepArgs a{};
  a.ch = m->d_chain;
  a.cm = m->d_collision;
  a.world = m->d_world;
  a.n_obs = m->world_n;
  a.n_caps = m->n_caps;
  a.world_min_clearance = m->world_min_clearance;
  a.reject_self = reject_self ? 1 : 0;
  a.self_min_clearance = self_min_clearance;
  a.n_samples = m->path_sweep;
  a.lattice = 1;
  a.q = d_q;
  a.q_start = d_q_start;
  a.node = m->tk_zero_node.p;
  a.T = (int)T;
  a.k = k;
  a.max_joint_step = -1.f;   // no step gate
  a.edge_free = d_edge_free_out;
  track_fill_sweep(m, &a);
  IKF_HIP(launch_sweep_edges(m->dims.ndof, a, s));
  IKF_HIP(scope.leave());
  return IKF_OK;
}

namespace ikf {

ikf_status track_rebuild(ikf_model* m, const std::string& who, int S) {
  if (m->track_F == 0 || S == m->track_S) return IKF_OK;
  std::vector<WorldObstacle> fine;
  ikf_status st = build_fine(who, m->track_keys, m->track_F, m->track_n, S, &fine);
  if (st != IKF_OK) return st;
  st = upload_fine(m, fine);
  if (st != IKF_OK) return st;
  m->track_fine.swap(fine);
  m->track_S = S;
  return IKF_OK;
}

ikf_status track_check_T(const ikf_model* m, const std::string& who, int64_t T) {
  if (m->track_F > 0 && T > m->track_F)
    return fail(IKF_ERR_BAD_ARGUMENT, who + ": T = " + std::to_string((long long)T) + " waypoints, but the world track has " + std::to_string(m->track_F) + " frames");
  return IKF_OK;
}

ikf_status track_mask_nodes(ikf_model* m, const float* d_q, int64_t T, int k, float* d_node, hipStream_t s) {
  if (m->track_F == 0) return IKF_OK;
  TrackArgs a{};
  a.ch = m->d_chain;
  a.cm = m->d_collision;
  a.frames = m->d_track;
  a.n_obs = m->track_n;
  a.n_caps = m->n_caps;
  a.frame_stride = m->track_S + 1;
  a.min_clearance = m->track_min_clearance;
  a.q = d_q;
  a.T = (int)T;
  a.k = k;
  a.node = d_node;
  IKF_HIP(launch_track_clearance(m->dims.ndof, a, s));
  return IKF_OK;
}

void track_fill_sweep(const ikf_model* m, SweepArgs* a) {
  if (m->track_F == 0) return;
  a->track = m->d_track;
  a->n_track = m->track_n;
  a->track_frames = m->track_F;
  a->track_min_clearance = m->track_min_clearance;
}

}  // namespace ikf
