// C-ABI of libikflow_amd.so, refined candidates (include/ikflow_amd_refine.h): the LM steps on the flow's candidate rows as state of the handle,
// and the same loop on the caller's own rows (k_refine_candidates, refine_kernels.hip).  What the state does to a ranked / diverse / path call is
// in flow_candidates (api_rank.hip).  The frame of api_rank.hip: stream scope, nothing read back to the host.
#include "ikf_model.h"

// what both entries refuse in a refinement; `lowest`: 0 for the handle's state (off), 1 for a call
static const char* refine_fault(int n_steps, int lowest, float pos_tol, float rot_tol) {
  if (n_steps < lowest || n_steps > IKF_REFINE_MAX_STEPS) return lowest ? "n_steps must be in 1 .. 16" : "n_steps must be in 0 .. 16";
  if (!(pos_tol >= 0.f) || !std::isfinite(pos_tol)) return "pos_tol must be finite and >= 0";
  if (!(rot_tol >= 0.f) || !std::isfinite(rot_tol)) return "rot_tol must be finite and >= 0";
  return nullptr;
}

extern "C" ikf_status ikf_set_candidate_refine(ikf_model* m, int n_steps, float pos_tol, float rot_tol) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_set_candidate_refine: null model");
  if (const char* fault = refine_fault(n_steps, 0, pos_tol, rot_tol)) return fail(IKF_ERR_BAD_ARGUMENT, std::string("ikf_set_candidate_refine: ") + fault);
  m->refine_steps = n_steps;
  m->refine_pos_tol = n_steps ? pos_tol : 0.f;
  m->refine_rot_tol = n_steps ? rot_tol : 0.f;
  return IKF_OK;
}

extern "C" int ikf_get_candidate_refine(const ikf_model* m, float* pos_tol_out, float* rot_tol_out) {
  if (pos_tol_out) *pos_tol_out = m ? m->refine_pos_tol : 0.f;
  if (rot_tol_out) *rot_tol_out = m ? m->refine_rot_tol : 0.f;
  return m ? m->refine_steps : 0;
}

extern "C" ikf_status ikf_refine_candidates(ikf_model* m, const float* d_target_poses, int64_t n_poses, int k, const float* d_q, int n_steps,
                                            float pos_tol, float rot_tol, float* d_q_out, uint8_t* d_steps_out, uint8_t* d_converged_out,
                                            void* stream) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_refine_candidates: null model");
  bool nothing = false;
  // (no options struct: the handle stands in for it; no k limit, no collision rule)
  ikf_status st = check_candidates(m, "ikf_refine_candidates", "n_poses", n_poses, k, 0, m, false, refine_fault(n_steps, 1, pos_tol, rot_tol),
                                   d_target_poses && d_q && d_q_out, &nothing);
  if (st != IKF_OK || nothing) return st;
  IKF_ON_DEVICE(m)
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  IKF_HIP(launch_refine(m->d_chain, m->dims.ndof, d_target_poses, n_poses, k, d_q, d_q_out, n_steps, pos_tol, rot_tol, d_steps_out, d_converged_out,
                        m->lm_precision, s));
  IKF_HIP(scope.leave());
  return IKF_OK;
}
