/*
 * ikflow_amd_diverse.h - diverse-of-K IK: K candidates per target pose, the inadmissible ones dropped, and of the rest a set of up to n_keep
 * configurations that are far apart in joint space - the distinct ways of reaching the pose (elbow up or down, wrist flipped), not n_keep
 * near-copies of the best one - chosen on the GPU by farthest-point selection.  An extension of the boundary (include/ikflow_amd.h), beside
 * include/ikflow_amd_rank.h and include/ikflow_amd_path.h and with their conventions: device pointers of the handle's device, row-major f32,
 * `stream` a hipStream_t (null: the default stream), no host synchronisation, nothing read back, every element of every non-null output
 * written, ikf_last_error for the message behind a status.
 *
 * Candidates (tile-major, as the ranking's): row r * n_poses + j is candidate r of pose j; 1 <= k <= IKF_DIVERSE_MAX_K,
 * 1 <= n_keep <= min(k, IKF_DIVERSE_MAX_KEEP), k * n_poses <= 2^31 - 1, n_poses >= 0 (n_poses = 0: nothing to do, IKF_OK).  Per pose:
 *   score[r]    = pos_err + rot_weight * rot_err of the row against the pose, +inf exactly when the row is inadmissible: score NaN, an error
 *                 not below its bound (bound >= 0), a joint strictly outside its limits (reject_limits), clearance < min_clearance
 *                 (reject_collisions) - the row score of the ranking without a reference configuration (include/ikflow_amd_rank.h), computed
 *                 by the ranking's own kernel, so it is ikf_rank_candidates' row score of the row bit for bit
 *   dist2(a, b) = sum over j = 0 .. ndof - 1, in that order, of d_j * d_j, with d_j = a_j - b_j, or d_j = (a_j - b_j) * w_j with
 *                 d_joint_weight ([ndof]; every w_j finite and >= 0 is the CALLER's contract: the weights are not read by the host - with a
 *                 NaN or infinite weight a distance can be NaN, which leaves near2 as it is); no angle wrapping
 *   slot 0      = the admissible candidate lowest in (score, then r): the ranking's first choice
 *   slot i >= 1 : near2[r] = the minimum of dist2(q_r, q_p) over the kept p, for every admissible candidate r not yet kept; the pick is the
 *                 greatest in (near2, then lower r), a strict total order.  The selection stops when no candidate is left, and when
 *                 !(near2 >= sep2) for the pick, sep2 = min_separation * min_separation (one f32 product, min_separation >= 0)
 * Every operation is rounded on its own (no fused multiply-add), so the selection is reproducible bit for bit by sequential f32 arithmetic.
 * Outputs per pose j, slot i < kept: q_out[j][i][:] the candidate row, score_out[j][i] its score, index_out[j][i] = r,
 * separation_out[j][i] = sqrtf(near2[r]) at the moment of the pick (+inf in slot 0); every further slot 0 / +inf / -1 / +inf;
 * kept_out[j] = slots filled, count_out[j] = admissible candidates, row_score_out[k * n_poses] the scores in the candidate layout.
 *
 * Two guarantees follow from the definition, both in this f32 arithmetic:
 *   1. kept rows are pairwise at least min_separation apart: dist2 >= sep2 for every two of them (dist2 is symmetric bit for bit);
 *   2. when kept < n_keep, every admissible row that was not kept is closer than min_separation to a kept one: its near2 < sep2.
 * Greedy farthest-point selection is not the best subset, but its smallest pairwise distance is at least half of the best subset's (the
 * farthest-first bound), from whichever first pick.
 * Refined candidates: while a refinement is set on the handle (include/ikflow_amd_refine.h), ikf_generate_diverse selects among LM-refined rows.
 */
#ifndef IKFLOW_AMD_DIVERSE_H
#define IKFLOW_AMD_DIVERSE_H

#include "ikflow_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IKF_DIVERSE_MAX_K 1024
#define IKF_DIVERSE_MAX_KEEP 16
typedef struct ikf_diverse_options {
  int32_t n_keep;            /* 1 .. min(k, IKF_DIVERSE_MAX_KEEP) */
  float rot_weight;          /* metres per radian */
  float max_pos_err, max_rot_err;   /* < 0: no bound */
  int32_t reject_limits;
  int32_t reject_collisions; /* IKF_ERR_BAD_ARGUMENT without a collision model */
  float min_clearance;
  float min_separation;      /* radians (weighted when d_joint_weight is given), >= 0; 0: stop only when no candidate is left */
} ikf_diverse_options;

/* candidates supplied by the caller: needs no weights */
ikf_status ikf_diverse_select(ikf_model* m, const float* d_target_poses /* [n_poses x 7] */, int64_t n_poses, int k,
                              const float* d_q /* [k*n_poses x ndof] tile-major */, const float* d_joint_weight /* [ndof], nullable */,
                              const ikf_diverse_options* opt, float* d_q_out /* [n_poses x n_keep x ndof] */,
                              float* d_score_out /* [n_poses x n_keep], nullable */, int32_t* d_index_out /* [n_poses x n_keep] */,
                              float* d_separation_out /* [n_poses x n_keep], nullable */, int32_t* d_kept_out /* [n_poses], nullable */,
                              int32_t* d_count_out /* [n_poses], nullable */, float* d_row_score_out /* [k*n_poses], nullable */, void* stream);
/* flow + selection: d_latent [k*n_poses x D] tile-major, candidates clamped when clamp_to_limits */
ikf_status ikf_generate_diverse(ikf_model* m, const float* d_target_poses, int64_t n_poses, int k, const float* d_latent, int clamp_to_limits,
                                const float* d_joint_weight, const ikf_diverse_options* opt, float* d_q_out, float* d_score_out,
                                int32_t* d_index_out, float* d_separation_out, int32_t* d_kept_out, int32_t* d_count_out,
                                float* d_row_score_out, void* stream);
ikf_status ikf_reserve_diverse(ikf_model* m, int64_t max_poses, int max_k);   /* flow scratch + candidate rows + partial lists + row scores: later calls allocate nothing */

#ifdef __cplusplus
}
#endif
#endif /* IKFLOW_AMD_DIVERSE_H */
