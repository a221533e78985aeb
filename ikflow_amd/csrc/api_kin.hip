// C-ABI of libikflow_amd.so, kinematics and exact IK: the per-row kinematics entries, the collision model, the model-free evaluation helpers and
// the exact-IK entries (what replaces _generate_exact_ik_solutions, ikflow/ikflow_solver.py:119-247, 345-411).  See include/ikflow_amd.h for the contract.
#include "ikf_model.h"

#define IKF_KIN_PROLOGUE(fn)                                                         \
  if (!m) return fail(IKF_ERR_NULL_POINTER, fn ": null model");                      \
  if (n < 0) return fail(IKF_ERR_BAD_ARGUMENT, fn ": n must be >= 0");               \
  if (n == 0) return IKF_OK;                                                         \
  IKF_ON_DEVICE(m)                                                                   \
  hipStream_t s = static_cast<hipStream_t>(stream);

extern "C" ikf_status ikf_forward_kinematics(ikf_model* m, const float* d_q, int64_t n, float* d_poses_out, void* stream) {
  IKF_KIN_PROLOGUE("ikf_forward_kinematics")
  if (!d_q || !d_poses_out) return fail(IKF_ERR_NULL_POINTER, "ikf_forward_kinematics: null device pointer");
  IKF_HIP(launch_fk(m->d_chain, m->dims.ndof, d_q, n, d_poses_out, s));
  return IKF_OK;
}
extern "C" ikf_status ikf_pose_error(ikf_model* m, const float* d_q, const float* d_target_poses, int64_t n,
                                     float* d_pos_err, float* d_rot_err, void* stream) {
  IKF_KIN_PROLOGUE("ikf_pose_error")
  if (!d_q || !d_target_poses || !d_pos_err || !d_rot_err) return fail(IKF_ERR_NULL_POINTER, "ikf_pose_error: null device pointer");
  IKF_HIP(launch_pose_error(m->d_chain, m->dims.ndof, d_q, d_target_poses, n, d_pos_err, d_rot_err, s));
  return IKF_OK;
}
extern "C" ikf_status ikf_lm_step(ikf_model* m, const float* d_target_poses, const float* d_q, int64_t n, float* d_q_out,
                                  void* stream) {
  IKF_KIN_PROLOGUE("ikf_lm_step")
  if (!d_q || !d_target_poses || !d_q_out) return fail(IKF_ERR_NULL_POINTER, "ikf_lm_step: null device pointer");
  IKF_HIP(launch_lm_step(m->d_chain, m->dims.ndof, d_target_poses, d_q, n, d_q_out, m->lm_precision, s));
  return IKF_OK;
}
extern "C" ikf_status ikf_jacobian(ikf_model* m, const float* d_q, int64_t n, float* d_jac_out, void* stream) {
  IKF_KIN_PROLOGUE("ikf_jacobian")
  if (!d_q || !d_jac_out) return fail(IKF_ERR_NULL_POINTER, "ikf_jacobian: null device pointer");
  IKF_HIP(launch_jacobian(m->d_chain, m->dims.ndof, d_q, n, d_jac_out, s));
  return IKF_OK;
}
extern "C" ikf_status ikf_clamp_to_joint_limits(ikf_model* m, const float* d_q, int64_t n, float* d_q_out, void* stream) {
  IKF_KIN_PROLOGUE("ikf_clamp_to_joint_limits")
  if (!d_q || !d_q_out) return fail(IKF_ERR_NULL_POINTER, "ikf_clamp_to_joint_limits: null device pointer");
  IKF_HIP(launch_clamp(m->d_chain, m->dims.ndof, d_q, n, d_q_out, s));
  return IKF_OK;
}
extern "C" ikf_status ikf_joint_limits_exceeded(ikf_model* m, const float* d_q, int64_t n, uint8_t* d_exceeded_out,
                                                void* stream) {
  IKF_KIN_PROLOGUE("ikf_joint_limits_exceeded")
  if (!d_q || !d_exceeded_out) return fail(IKF_ERR_NULL_POINTER, "ikf_joint_limits_exceeded: null device pointer");
  IKF_HIP(launch_limits_exceeded(m->d_chain, m->dims.ndof, d_q, n, d_exceeded_out, s));
  return IKF_OK;
}

extern "C" ikf_status ikf_set_collision_model(ikf_model* m, const ikf_capsule* h_capsules, int n_capsules,
                                              const int32_t* h_pairs, int n_pairs) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_set_collision_model: null model");
  if (n_capsules < 0 || n_capsules > IKF_MAX_CAPSULES || n_pairs < 0 || n_pairs > IKF_MAX_CAPSULE_PAIRS)
    return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_collision_model: at most 24 capsules and 276 pairs");
  if ((n_capsules > 0 && !h_capsules) || (n_pairs > 0 && !h_pairs))
    return fail(IKF_ERR_NULL_POINTER, "ikf_set_collision_model: null table");
  CollisionModel cm{};
  cm.n_caps = n_capsules;
  cm.n_pairs = n_pairs;
  for (int c = 0; c < n_capsules; ++c) {
    if (h_capsules[c].frame < 0 || h_capsules[c].frame > m->dims.ndof || !(h_capsules[c].radius >= 0.f))
      return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_collision_model: capsule frame must be in [0, ndof] and radius >= 0");
    cm.frame[c] = h_capsules[c].frame;
    cm.radius[c] = h_capsules[c].radius;
    for (int k = 0; k < 3; ++k) { cm.p0[c][k] = h_capsules[c].p0[k]; cm.p1[c][k] = h_capsules[c].p1[k]; }
  }
  for (int k = 0; k < n_pairs; ++k) {
    const int a = h_pairs[2 * k], b = h_pairs[2 * k + 1];
    if (a < 0 || a >= n_capsules || b < 0 || b >= n_capsules || a == b)
      return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_collision_model: pair index out of range");
    cm.pair_a[k] = (uint8_t)a;
    cm.pair_b[k] = (uint8_t)b;
  }
  IKF_ON_DEVICE(m)
  IKF_HIP(m->d_collision.ensure(1));
  IKF_HIP(hipMemcpy(m->d_collision, &cm, sizeof(CollisionModel), hipMemcpyHostToDevice));
  m->n_caps = n_capsules;
  return IKF_OK;
}

extern "C" ikf_status ikf_self_collision(ikf_model* m, const float* d_q, int64_t n, float* d_min_dist_out,
                                         uint8_t* d_colliding_out, void* stream) {
  IKF_KIN_PROLOGUE("ikf_self_collision")
  if (!m->d_collision) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_self_collision: no collision model has been set");
  if (!d_q || (!d_min_dist_out && !d_colliding_out)) return fail(IKF_ERR_NULL_POINTER, "ikf_self_collision: null device pointer");
  IKF_HIP(launch_self_collision(m->d_chain, m->d_collision, m->dims.ndof, d_q, n, d_min_dist_out, d_colliding_out, s));
  return IKF_OK;
}

// model-free evaluation helpers (current device; evaluation_utils.py:37-51, :100-112)
extern "C" ikf_status ikf_pose_distance(const float* d_poses_a, const float* d_poses_b, int64_t n, float acos_epsilon,
                                        float* d_pos_err, float* d_rot_err, void* stream) {
  if (n < 0) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_pose_distance: n must be >= 0");
  if (n == 0) return IKF_OK;
  if (!d_poses_a || !d_poses_b || !d_pos_err || !d_rot_err)
    return fail(IKF_ERR_NULL_POINTER, "ikf_pose_distance: null device pointer");
  IKF_HIP(launch_pose_distance(d_poses_a, d_poses_b, n, acos_epsilon, d_pos_err, d_rot_err,
                               static_cast<hipStream_t>(stream)));
  return IKF_OK;
}

extern "C" ikf_status ikf_limits_exceeded(const float* d_q, int64_t n, int n_cols, const float* h_lower,
                                          const float* h_upper, uint8_t* d_exceeded_out, void* stream) {
  if (n < 0) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_limits_exceeded: n must be >= 0");
  if (n_cols < 1 || n_cols > IKF_MAX_LIMIT_COLS)
    return fail(IKF_ERR_BAD_ARGUMENT, "ikf_limits_exceeded: n_cols must be in [1, 32]");
  if (n == 0) return IKF_OK;
  if (!d_q || !h_lower || !h_upper || !d_exceeded_out)
    return fail(IKF_ERR_NULL_POINTER, "ikf_limits_exceeded: null pointer");
  IKF_HIP(launch_limits_exceeded_table(h_lower, h_upper, n_cols, d_q, n, d_exceeded_out,
                                       static_cast<hipStream_t>(stream)));
  return IKF_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// exact IK
// ---------------------------------------------------------------------------------------------------------------
// The retry schedule of generate_exact_ik_solutions (:345-411) over rounds of _generate_exact_ik_solutions (:119-247).
// Seeds of a round come from the flow (latent_fn) or, for parity runs, from the caller (seed_fn).
static ikf_status run_exact(ikf_model* m, const float* d_target_poses, int64_t n, const int32_t* repeat_counts,
                            int n_rounds, int n_lm_steps, float pos_thr, float rot_thr, ikf_latent_fn latent_fn,
                            ikf_seed_fn seed_fn, void* user, float* d_q_out, uint8_t* d_valid_out, int64_t* h_stats,
                            hipStream_t s, const char* fn) {
  const std::string who(fn);
  if (n < 0) return fail(IKF_ERR_BAD_ARGUMENT, who + ": n must be >= 0");
  if (!repeat_counts || n_rounds < 1 || n_rounds > IKF_MAX_ROUNDS)
    return fail(IKF_ERR_BAD_ARGUMENT, who + ": repeat_counts must hold 1..8 rounds");
  if (n_lm_steps < 1 || n_lm_steps > 255) return fail(IKF_ERR_BAD_ARGUMENT, who + ": n_lm_steps must be in 1..255");
  int max_repeat = 0;
  for (int r = 0; r < n_rounds; ++r) {
    if (repeat_counts[r] < 1) return fail(IKF_ERR_BAD_ARGUMENT, who + ": repeat counts must be >= 1");
    max_repeat = repeat_counts[r] > max_repeat ? repeat_counts[r] : max_repeat;
  }
  if (h_stats) memset(h_stats, 0, sizeof(int64_t) * 4 * n_rounds);
  bool rule = false;  // the exact collision rule has something to test against (api_exact_world.hip)
  ikf_status st = n > 0 ? exact_rule_begin(m, who, &rule) : IKF_OK;
  if (st != IKF_OK) return st;
  if (n == 0) return IKF_OK;
  if (!d_target_poses || !d_q_out || !d_valid_out) return fail(IKF_ERR_NULL_POINTER, who + ": null device pointer");
  if (n > 0x7fffffffLL / 64 || n * (long long)repeat_counts[0] > 0x7fffffffLL) return fail(IKF_ERR_BAD_ARGUMENT, who + ": n too large");
  const int ndof = m->dims.ndof;
  // Row state: when the worst case of the schedule (all n poses still unsolved in the round with the largest repeat count) is
  // small it is sized once, before any work is enqueued, so no allocation (= device-wide synchronisation) happens between the
  // rounds; a larger worst case - or whatever ikf_reserve_exact has already provided - is not allocated for: the call
  // starts with round 0's rows and each later round grows to its measured n_active * R if it has to.
  const long long worst_rows = n * (long long)max_repeat;
  st = ensure_exact(m, n, worst_rows <= m->exact_upfront_rows ? worst_rows : n * (long long)repeat_counts[0]);
  if (st != IKF_OK) return st;
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());

  // (no memset of the outputs: round 0's selection writes every pose - its solution, or zeros and valid = 0 (:197))
  long long n_active = n;
  for (int r = 0; r < n_rounds; ++r) {
    const int R = repeat_counts[r];
    // active pose list = ordered indices of still-invalid poses (every pose in round 0)
    if (r == 0) IKF_HIP(launch_all_active(n, m->ex_pose_idx, m->ex_count, s));
    else IKF_HIP(launch_compact_invalid(d_valid_out, n, m->ex_pose_idx, m->ex_count, m->ex_block_scratch, s));
    if (r > 0) {
      IKF_HIP(hipMemcpyAsync(m->h_count, m->ex_count, sizeof(int), hipMemcpyDeviceToHost, s));
      IKF_HIP(hipStreamSynchronize(s));
      n_active = *m->h_count;
      if (h_stats) h_stats[4 * (r - 1) + 3] = h_stats[4 * (r - 1) + 0] - n_active;
      if (n_active == 0) break;  // everything converged (:383-385, :402-408)
    }
    const long long rows = n_active * R;
    if (rows > 0x7fffffffLL) return fail(IKF_ERR_BAD_ARGUMENT, who + ": a retry round has more than 2^31 - 1 rows");
    if (rows > m->exact_rows) {  // r > 0 only (round 0 was sized above); the stream is idle: the count was just read
      st = ensure_exact_rows(m, rows);
      if (st != IKF_OK) return st;
    }
    const float* d_q_seed = m->ex_q;
    if (seed_fn) {
      d_q_seed = seed_fn(user, r, n_active, R, m->ex_pose_idx, ndof);  // read in place by the LM kernel (no copy)
      if (!d_q_seed) return fail(IKF_ERR_NULL_POINTER, who + ": seed_fn returned null");
    } else {
      const float* d_latent = latent_fn(user, r, rows, m->dims.D);
      if (!d_latent) return fail(IKF_ERR_NULL_POINTER, who + ": latent_fn returned null");
      PoseSource ps{d_target_poses, m->ex_pose_idx, n_active, 7, 0.0f};
      st = run_flow_guarded(m, ps, d_latent, rows, /*clamp=*/1, m->ex_q, s);  // seeds (:188)
      if (st != IKF_OK) return st;
    }
    // all LM iterations of the round in one launch + one selection (kin_kernels.hip: k_exact_lm_iters; under the rule: api_exact_world.hip)
    st = exact_round_lm(m, rule, r, d_target_poses, (int)n_active, R, n_lm_steps, d_q_seed, pos_thr, rot_thr, s);
    if (st != IKF_OK) return st;
    IKF_HIP(launch_exact_select_first(ndof, m->ex_pose_idx, (int)n_active, R, m->ex_q, m->ex_row_valid, d_q_out, d_valid_out,
                                      r == 0 ? 1 : 0, s));
    if (h_stats) {
      h_stats[4 * r + 0] = n_active;
      h_stats[4 * r + 1] = rows;
      h_stats[4 * r + 2] = rows * n_lm_steps;  // upper bound: a row stops at its first valid iteration, or once a sibling repeat was valid earlier
    }
  }
  if (h_stats && n_active > 0) {
    IKF_HIP(launch_compact_invalid(d_valid_out, n, m->ex_pose_idx, m->ex_count, m->ex_block_scratch, s));
    IKF_HIP(hipMemcpyAsync(m->h_count, m->ex_count, sizeof(int), hipMemcpyDeviceToHost, s));
    IKF_HIP(hipStreamSynchronize(s));
    h_stats[4 * (n_rounds - 1) + 3] = h_stats[4 * (n_rounds - 1) + 0] - *m->h_count;
  }
  IKF_HIP(scope.leave());
  return IKF_OK;
}

extern "C" ikf_status ikf_generate_exact(ikf_model* m, const float* d_target_poses, int64_t n,
                                         const int32_t* repeat_counts, int n_rounds, int n_lm_steps,
                                         float pos_thr, float rot_thr, ikf_latent_fn latent_fn, void* latent_user,
                                         float* d_q_out, uint8_t* d_valid_out, int64_t* h_stats, void* stream) {
  ikf_status st = check_ready(m, "ikf_generate_exact");
  if (st != IKF_OK) return st;
  if (!latent_fn) return fail(IKF_ERR_NULL_POINTER, "ikf_generate_exact: latent_fn is required");
  IKF_ON_DEVICE(m)
  return run_exact(m, d_target_poses, n, repeat_counts, n_rounds, n_lm_steps, pos_thr, rot_thr, latent_fn, nullptr,
                   latent_user, d_q_out, d_valid_out, h_stats, static_cast<hipStream_t>(stream), "ikf_generate_exact");
}

extern "C" ikf_status ikf_generate_exact_seeded(ikf_model* m, const float* d_target_poses, int64_t n,
                                                const int32_t* repeat_counts, int n_rounds, int n_lm_steps,
                                                float pos_thr, float rot_thr, ikf_seed_fn seed_fn, void* seed_user,
                                                float* d_q_out, uint8_t* d_valid_out, int64_t* h_stats, void* stream) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_generate_exact_seeded: null model");
  if (!seed_fn) return fail(IKF_ERR_NULL_POINTER, "ikf_generate_exact_seeded: seed_fn is required");
  IKF_ON_DEVICE(m)
  return run_exact(m, d_target_poses, n, repeat_counts, n_rounds, n_lm_steps, pos_thr, rot_thr, nullptr, seed_fn,
                   seed_user, d_q_out, d_valid_out, h_stats, static_cast<hipStream_t>(stream),
                   "ikf_generate_exact_seeded");
}

static const float* fixed_seeds(void* user, int, int64_t, int, const int32_t*, int) { return static_cast<const float*>(user); }

extern "C" ikf_status ikf_refine_exact(ikf_model* m, const float* d_target_poses, int64_t n, int repeat,
                                       const float* d_seeds_q, int n_lm_steps, float pos_thr, float rot_thr,
                                       float* d_q_out, uint8_t* d_valid_out, void* stream) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_refine_exact: null model");
  if (n > 0 && !d_seeds_q) return fail(IKF_ERR_NULL_POINTER, "ikf_refine_exact: null device pointer");
  IKF_ON_DEVICE(m)
  const int32_t rc[1] = {repeat};
  return run_exact(m, d_target_poses, n, rc, 1, n_lm_steps, pos_thr, rot_thr, nullptr, fixed_seeds,
                   const_cast<float*>(d_seeds_q), d_q_out, d_valid_out, nullptr, static_cast<hipStream_t>(stream),
                   "ikf_refine_exact");
}

extern "C" ikf_status ikf_set_exact_upfront_rows(ikf_model* m, int64_t max_rows) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_set_exact_upfront_rows: null model");
  if (max_rows < 0) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_exact_upfront_rows: max_rows must be >= 0");
  m->exact_upfront_rows = max_rows;
  return IKF_OK;
}
