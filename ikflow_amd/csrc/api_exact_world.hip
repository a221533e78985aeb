// C-ABI of libikflow_amd.so, exact IK that obeys the world (include/ikflow_amd_exact_world.h): the exact collision rule as state of the handle,
// the choice of a retry round's LM launch by "is there anything to test against", the launches of the rule (k_exact_lm_iters_clear,
// k_exact_mask_rows: exact_world_kernels.hip; k_cloud_clearance through run_cloud_clearance) and the rejected rows' counter.  run_exact
// (api_kin.hip) keeps its control flow and calls in here.
#include "ikf_model.h"

extern "C" ikf_status ikf_set_exact_collision(ikf_model* m, int on, int reject_self, float self_min_clearance) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_set_exact_collision: null model");
  if (!std::isfinite(self_min_clearance)) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_exact_collision: self_min_clearance must be finite");
  m->ex_rule_on = on ? 1 : 0;
  m->ex_reject_self = on && reject_self ? 1 : 0;
  m->ex_self_min_clearance = on ? self_min_clearance : 0.f;
  return IKF_OK;
}

extern "C" ikf_status ikf_get_exact_collision(const ikf_model* m, int* on_out, int* reject_self_out, float* self_min_clearance_out) {
  if (on_out) *on_out = m ? m->ex_rule_on : 0;
  if (reject_self_out) *reject_self_out = m ? m->ex_reject_self : 0;
  if (self_min_clearance_out) *self_min_clearance_out = m ? m->ex_self_min_clearance : 0.f;
  return m ? IKF_OK : fail(IKF_ERR_NULL_POINTER, "ikf_get_exact_collision: null model");
}

extern "C" ikf_status ikf_exact_collision_rejected(ikf_model* m, int64_t* h_rows) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_exact_collision_rejected: null model");
  if (!h_rows) return fail(IKF_ERR_NULL_POINTER, "ikf_exact_collision_rejected: null output");
  for (int r = 0; r < IKF_MAX_ROUNDS; ++r) h_rows[r] = 0;
  if (!m->ex_rejected_live) return IKF_OK;
  IKF_ON_DEVICE(m)
  if (m->tail_valid) IKF_HIP(hipStreamSynchronize(m->tail_stream));   // the last call's work, whatever stream it went to
  unsigned long long host[IKF_MAX_ROUNDS];
  IKF_HIP(hipMemcpy(host, m->ex_rejected, sizeof(host), hipMemcpyDeviceToHost));
  for (int r = 0; r < IKF_MAX_ROUNDS; ++r) h_rows[r] = (int64_t)host[r];
  return IKF_OK;
}

ikf_status ikf::exact_rule_begin(ikf_model* m, const std::string& who, bool* active) {
  *active = false;
  m->ex_rejected_live = false;
  if (!m->ex_rule_on) return IKF_OK;
  if (m->world_n == 0 && m->cloud_n == 0 && !m->ex_reject_self) return IKF_OK;   // nothing to test against: the plain call
  if (!m->d_collision) return fail(IKF_ERR_BAD_ARGUMENT, who + ": the exact collision rule without a collision model (ikf_set_collision_model)");
  IKF_HIP(m->ex_rejected.ensure(IKF_MAX_ROUNDS));
  *active = true;
  m->ex_rejected_live = true;
  return IKF_OK;
}

ikf_status ikf::exact_rule_rows(ikf_model* m, long long rows) {
  if (!m->ex_rule_on || m->cloud_n == 0 || rows <= 0) return IKF_OK;
  IKF_HIP(m->ex_cloud_row.ensure(rows));
  return ensure_cloud_partials(m, rows);
}

ikf_status ikf::exact_round_lm(ikf_model* m, bool active, int round, const float* d_target_poses, int n_active, int repeat, int n_lm_steps,
                               const float* d_q_seed, float pos_thr, float rot_thr, hipStream_t s) {
  const int ndof = m->dims.ndof;
  if (!active) {   // all LM iterations of the round in one launch (kin_kernels.hip: k_exact_lm_iters)
    IKF_HIP(launch_exact_lm_iters(m->d_chain, ndof, d_target_poses, m->ex_pose_idx, n_active, repeat, n_lm_steps, d_q_seed, m->ex_q,
                                  m->ex_row_valid, m->ex_pose_first, pos_thr, rot_thr, m->lm_precision, s));
    return IKF_OK;
  }
  if (round == 0) IKF_HIP(hipMemsetAsync(m->ex_rejected, 0, sizeof(unsigned long long) * IKF_MAX_ROUNDS, s));
  unsigned long long* const counter = m->ex_rejected + round;
  if (m->world_n > 0 || m->ex_reject_self) {   // the loop and the world / self rule in one launch
    ExactClearArgs a{};
    a.ch = m->d_chain;
    a.cm = m->d_collision;
    a.world = m->d_world;
    a.n_obs = m->world_n;
    a.n_caps = m->n_caps;
    a.world_min = m->world_min_clearance;
    a.reject_self = m->ex_reject_self;
    a.self_min = m->ex_self_min_clearance;
    a.poses = d_target_poses;
    a.pose_idx = m->ex_pose_idx;
    a.n_active = n_active;
    a.repeat = repeat;
    a.n_steps = n_lm_steps;
    a.q_in = d_q_seed;
    a.q = m->ex_q;
    a.row_valid_iter = m->ex_row_valid;
    a.pos_thr = pos_thr;
    a.rot_thr = rot_thr;
    a.lm_precision = m->lm_precision;
    a.rejected_rows = counter;
    IKF_HIP(launch_exact_lm_iters_clear(a, ndof, s));
  } else {         // a cloud alone: the plain loop - without pose_first, a sibling's candidate may yet be rejected - and the mask below
    IKF_HIP(launch_exact_lm_iters(m->d_chain, ndof, d_target_poses, m->ex_pose_idx, n_active, repeat, n_lm_steps, d_q_seed, m->ex_q,
                                  m->ex_row_valid, nullptr, pos_thr, rot_thr, m->lm_precision, s));
  }
  if (m->cloud_n > 0) {
    const long long rows = (long long)n_active * repeat;
    ikf_status st = exact_rule_rows(m, rows > m->exact_rows ? rows : m->exact_rows);   // (sized with the row state: allocates only for a cloud set since)
    if (st != IKF_OK) return st;
    st = run_cloud_clearance(m, m->ex_q, rows, m->ex_cloud_row, nullptr, s);
    if (st != IKF_OK) return st;
    IKF_HIP(launch_exact_mask_rows(m->ex_row_valid, m->ex_cloud_row, m->cloud_min_clearance, rows, counter, s));
  }
  return IKF_OK;
}
