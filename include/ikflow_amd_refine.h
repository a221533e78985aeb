/*
 * ikflow_amd_refine.h - refined candidates: a few Levenberg-Marquardt steps on every candidate row BEFORE it is scored, so that best-of-K
 * (include/ikflow_amd_rank.h), path IK (include/ikflow_amd_path.h, include/ikflow_amd_sweep.h) and diverse-of-K (include/ikflow_amd_diverse.h)
 * test, compare and return rows that reach the pose the way ikf_generate_exact's rows do.  An extension of the boundary
 * (include/ikflow_amd.h), beside those headers and include/ikflow_amd_world.h and with their conventions: device pointers of the handle's
 * device, row-major f32, `stream` a hipStream_t (null: the default stream), no host synchronisation, nothing read back, every element of
 * every non-null output written, ikf_last_error for the message behind a status.
 *
 * Definitions (these are this project's own):
 *   parameters   a refinement has n_steps in 1 .. IKF_REFINE_MAX_STEPS and two tolerances pos_tol (metres) and rot_tol (radians), each >= 0
 *                and finite.
 *   the loop     candidate row r of pose j = r % n_poses (tile-major, as everywhere) goes through
 *                  for it in 0 .. n_steps - 1:
 *                      q <- LM step of q towards pose j        (ikf_lm_step's step: the arithmetic chosen by ikf_set_lm_precision; it clamps
 *                                                               q to the joint limits)
 *                      (pe, re) <- f32 pose error of q          (ikf_pose_error's)
 *                      if pe < pos_tol and re < rot_tol: converged; stop
 *   steps        the number of steps applied to the row, 1 .. n_steps.
 *   converged    1 when the loop stopped on its test, else 0.
 *   tolerance 0  never stops a row: all n_steps run and converged is 0.
 *   first step   a row that is inside the tolerances when it arrives still takes one step (the test follows the step), as the reference's
 *                loop and ikf_generate_exact's do.
 *   rot_tol      the f32 rotation error is clamped from below: the quaternion dot product is limited to 1 - 1e-7 before the arc cosine, so no
 *                row reports less than 2 acosf(1 - 1e-7), about 9.77e-4 rad.  A rot_tol at or below that value never stops a row.
 *   non-finite   gets no treatment of its own: the row comes out as that many LM steps leave it.  (The clamp that ends a step maps a NaN joint
 *                to a limit, so a row that arrives with a NaN goes on from there as an ordinary row; a comparison with a NaN error is false.)
 *   independence no row waits on, or is stopped by, another row - unlike ikf_generate_exact's round, where a solved repeat stops its siblings.
 *
 * While a refinement is set on the handle (ikf_set_candidate_refine), ikf_generate_ranked, ikf_generate_diverse and ikf_generate_path (both
 * latent forms) run that loop on the flow's candidate rows, in place, between the flow and the scoring.  Scores, thresholds, joint-limit /
 * self-collision / world rejection, diverse distances, lattice edges, the sweep and every returned row then refer to the refined rows: such a
 * call equals ikf_generate_approx on the tiled poses, ikf_refine_candidates, and ikf_rank_candidates / ikf_diverse_select / ikf_path_search on
 * the result, bit for bit.  The entries that take the caller's own rows (ikf_rank_candidates, ikf_diverse_select, ikf_path_search,
 * ikf_sweep_edges) never refine: those rows are const - refine them first with ikf_refine_candidates.  With no refinement set (the default)
 * every call is bit for bit what it is without this header.
 */
#ifndef IKFLOW_AMD_REFINE_H
#define IKFLOW_AMD_REFINE_H

#include "ikflow_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IKF_REFINE_MAX_STEPS 16

/* The refinement of the flow's candidates on this handle; n_steps = 0 (the default): none, the tolerances are then ignored and kept as 0.
 * n_steps outside 0 .. 16, or a tolerance that is negative or not finite: IKF_ERR_BAD_ARGUMENT, the previous state stays in force.  State of
 * the handle, like the world and the path sweep.  Must not be called while calls on the handle are in flight. */
ikf_status ikf_set_candidate_refine(ikf_model* m, int n_steps, float pos_tol, float rot_tol);
/* -> n_steps (0: off, and for a null handle); the tolerances through the non-null outputs (0 for a null handle). */
int ikf_get_candidate_refine(const ikf_model* m, float* pos_tol_out, float* rot_tol_out);
/* The loop on the caller's rows: d_q [k * n_poses x ndof] tile-major against d_target_poses [n_poses x 7], n_steps in 1 .. 16 ->
 * d_q_out [k * n_poses x ndof] (may be d_q itself: in place), steps [k * n_poses] and converged [k * n_poses] (each nullable).  Needs the
 * handle's chain, not weights and not the handle's refinement state; k >= 1 without an upper limit, k * n_poses at most 2^31 - 1;
 * n_poses = 0: nothing to do. */
ikf_status ikf_refine_candidates(ikf_model* m, const float* d_target_poses, int64_t n_poses, int k, const float* d_q, int n_steps,
                                 float pos_tol, float rot_tol, float* d_q_out, uint8_t* d_steps_out, uint8_t* d_converged_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IKFLOW_AMD_REFINE_H */
