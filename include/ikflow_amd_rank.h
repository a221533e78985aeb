/*
 * ikflow_amd_rank.h - best-of-K IK: K candidates per target pose, the inadmissible ones dropped, the rest ordered by pose error, the best
 * n_keep returned.  An extension of the boundary (include/ikflow_amd.h, which stays "what a binding of the reference needs"): same
 * conventions - device pointers of the handle's device, row-major f32, `stream` a hipStream_t (null: the default stream), no host
 * synchronisation, ikf_last_error for the message behind a status.
 *
 * Candidate layout (tile-major, as the exact path's): row r * n_poses + j is candidate r of pose j.
 *   score of a row  = pos_err + rot_weight * rot_err [+ ref_weight * ||q - q_ref[j]||_2, no angle wrapping]   (errors as ikf_pose_error)
 *   inadmissible    = score NaN, or not pos_err < max_pos_err (bound >= 0), or not rot_err < max_rot_err, or (reject_limits) a joint
 *                     strictly outside its limits, or (reject_collisions) clearance < min_clearance: such a row scores +inf exactly
 *   order of a pose = (lower score, then lower candidate index r): a strict total order, so the result is unique
 * Outputs per pose j, i < min(count, n_keep): q_out[j][i][:] the candidate row, score_out[j][i], index_out[j][i] = r; every further slot
 * q = 0, score = +inf, index = -1; count_out[j] = number of admissible candidates.  Every element of every non-null output is written.
 * Refined candidates: while a refinement is set on the handle (include/ikflow_amd_refine.h), ikf_generate_ranked ranks and returns LM-refined rows.
 */
#ifndef IKFLOW_AMD_RANK_H
#define IKFLOW_AMD_RANK_H

#include "ikflow_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IKF_RANK_MAX_KEEP 16
typedef struct ikf_rank_options {
  int32_t n_keep;            /* 1 .. min(k, IKF_RANK_MAX_KEEP) */
  float rot_weight;          /* metres per radian */
  float ref_weight;          /* metres per radian of joint distance; used only with d_q_ref */
  float max_pos_err, max_rot_err;   /* < 0: no bound */
  int32_t reject_limits;
  int32_t reject_collisions; /* IKF_ERR_BAD_ARGUMENT without a collision model */
  float min_clearance;
} ikf_rank_options;

/* candidates supplied by the caller: needs no weights */
ikf_status ikf_rank_candidates(ikf_model* m, const float* d_target_poses, int64_t n_poses, int k, const float* d_q /* [k*n_poses x ndof] tile-major */,
                               const float* d_q_ref /* [n_poses x ndof], nullable */, const ikf_rank_options* opt,
                               float* d_q_out /* [n_poses x n_keep x ndof] */, float* d_score_out, int32_t* d_index_out, int32_t* d_count_out,
                               float* d_row_score_out /* [k*n_poses], nullable */, void* stream);
/* flow + ranking: d_latent [k*n_poses x D] tile-major, candidates clamped when clamp_to_limits */
ikf_status ikf_generate_ranked(ikf_model* m, const float* d_target_poses, int64_t n_poses, int k, const float* d_latent, int clamp_to_limits,
                               const float* d_q_ref, const ikf_rank_options* opt, float* d_q_out, float* d_score_out, int32_t* d_index_out,
                               int32_t* d_count_out, float* d_row_score_out, void* stream);
ikf_status ikf_reserve_ranked(ikf_model* m, int64_t max_poses, int max_k);   /* flow scratch + candidate rows + partial lists: later calls allocate nothing */

#ifdef __cplusplus
}
#endif
#endif /* IKFLOW_AMD_RANK_H */
