/*
 * ikflow_amd_path.h - path IK: T waypoints (end-effector poses in order), k candidate configurations per waypoint, and the one joint-space
 * path through the k x T lattice that is cheapest in pose error and joint motion, found on the GPU.  An extension of the boundary
 * (include/ikflow_amd.h), beside include/ikflow_amd_rank.h and with its conventions: device pointers of the handle's device, row-major f32,
 * `stream` a hipStream_t (null: the default stream), no host synchronisation, nothing read back, every element of every non-null output
 * written, ikf_last_error for the message behind a status.
 *
 * Lattice (tile-major, as the ranking's candidates): row r * T + t is candidate r of waypoint t; 1 <= k <= IKF_PATH_MAX_K, T >= 0 (T = 0:
 * nothing to do, IKF_OK), k * T <= 2^31 - 1.
 *   node[t][r]  = pos_err + rot_weight * rot_err of the row against waypoint t, +inf exactly when the row is inadmissible: score NaN, an
 *                 error not below its bound (bound >= 0), a joint strictly outside its limits (reject_limits), clearance < min_clearance
 *                 (reject_collisions) - the row score of the ranking without a reference configuration
 *   edge(a, b)  = sqrt(sum_j (b_j - a_j)^2), j = 0 .. ndof - 1 in that order, no angle wrapping; forbidden (never taken) when
 *                 max_joint_step >= 0 and some |b_j - a_j| > max_joint_step
 *   cost[0][r]  = [edge(q_start, q[0][r]) +] node_weight * node[0][r]                        (the edge only with d_q_start, under the same gate)
 *   cost[t][r]  = min_j (cost[t-1][j] + edge(q[t-1][j], q[t][r])) + node_weight * node[t][r]
 *                 a predecessor j with cost +inf is skipped before its edge is looked at; the order among predecessors is (lower sum, then
 *                 lower j), a strict total order; an inadmissible node, a node without an admissible predecessor and a sum that is not below
 *                 +inf all give cost +inf and no back-pointer (so neither a NaN nor node_weight = 0 times +inf ever enters a sum)
 *   end         = argmin_r cost[T-1][r], the lower r on ties; the path follows the back-pointers from there
 * Every step is rounded on its own (no fused multiply-add), so the search is reproducible bit for bit by sequential f32 arithmetic.
 * Outputs: path_out[t][:] the chosen row of waypoint t, index_out[t] its candidate r, cost_out[0] the total, reachable_out[t] the number of
 * r with cost[t][r] < +inf (where a path breaks), node_cost_out the node costs in the candidate layout (unweighted).  No path (total +inf):
 * path rows 0, indices -1, cost +inf.
 * Refined candidates: while a refinement is set on the handle (include/ikflow_amd_refine.h), ikf_generate_path builds its lattice from LM-refined rows.
 * A world that moves along the path - one frame of obstacles per waypoint - is include/ikflow_amd_track.h.
 */
#ifndef IKFLOW_AMD_PATH_H
#define IKFLOW_AMD_PATH_H

#include "ikflow_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IKF_PATH_MAX_K 256
typedef struct ikf_path_options {
  float rot_weight;          /* metres per radian */
  float max_pos_err, max_rot_err;   /* < 0: no bound */
  int32_t reject_limits;
  int32_t reject_collisions; /* IKF_ERR_BAD_ARGUMENT without a collision model */
  float min_clearance;
  float node_weight;         /* radians per metre of node cost, >= 0 */
  float max_joint_step;      /* radians (metres on a prismatic joint); < 0: no gate */
} ikf_path_options;

/* candidates supplied by the caller: needs no weights */
ikf_status ikf_path_search(ikf_model* m, const float* d_waypoints /* [T x 7] */, int64_t T, int k, const float* d_q /* [k*T x ndof] tile-major */,
                           const float* d_q_start /* [ndof], nullable */, const ikf_path_options* opt, float* d_path_out /* [T x ndof] */,
                           int32_t* d_index_out /* [T] */, float* d_cost_out /* [1] */, int32_t* d_reachable_out /* [T], nullable */,
                           float* d_node_cost_out /* [k*T], nullable */, void* stream);
/* flow + search: shared_latent != 0: d_latent [k x D], candidate r uses latent r at every waypoint; else d_latent [k*T x D] tile-major */
ikf_status ikf_generate_path(ikf_model* m, const float* d_waypoints, int64_t T, int k, const float* d_latent, int shared_latent, int clamp_to_limits,
                             const float* d_q_start, const ikf_path_options* opt, float* d_path_out, int32_t* d_index_out, float* d_cost_out,
                             int32_t* d_reachable_out, float* d_node_cost_out, void* stream);
ikf_status ikf_reserve_path(ikf_model* m, int64_t max_waypoints, int max_k);   /* flow scratch + candidate rows + lattice scratch: later calls allocate nothing */

#ifdef __cplusplus
}
#endif
#endif /* IKFLOW_AMD_PATH_H */
