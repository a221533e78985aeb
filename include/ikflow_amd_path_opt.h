/*
 * ikflow_amd_path_opt.h - path IK, third stage: a least-squares pass over a whole joint-space path on the GPU.  The lattice of
 * include/ikflow_amd_path.h returns one of k discrete samples per waypoint; this stage moves those rows, all waypoints coupled, towards lower pose
 * error and less joint motion, and hands the result back only when the lattice's own rules allow it and the lattice's own cost says it is better.
 * An extension of include/ikflow_amd_path_batch.h with its conventions: device pointers of the handle's device, row-major f32, `stream` a
 * hipStream_t (null: the default stream), no host synchronisation, every element of every non-null output written, ikf_last_error for the message
 * behind a status.  P >= 0 paths of T >= 0 waypoints in the path-batch layout (global waypoint g = p * T + t), P * T <= 2^31 - 1; P * T == 0:
 * nothing to do, IKF_OK, nothing written.  A refused call leaves every output untouched.
 *
 * A path is Q = [q_0 .. q_{T-1}], [T x ndof] f32, with waypoints [T x 7] and an optional q_start [ndof].  All arithmetic is fp64; the iterate is
 * rounded to f32 after every step.
 *   residual   e_t(q_t): the 6-vector of the LM step (ikf_lm_step): roll / pitch / yaw of q_target * conj(q_current), then p_target - p_current.
 *              J_t: its geometric Jacobian, angular rows first.
 *   objective  F(Q) = sum_t f_t,  f_t = |e_t|^2 + w |q_t - q_{t-1}|^2   (the second term for t > 0, and for t = 0 against q_start when given);
 *              w = smooth_weight, finite and >= 0; summed over t ascending, |e_t|^2 over its 6 entries and the difference over the joints in order.
 *   step       (blockdiag(J_t^T J_t) + lambda I + w (L (x) I)) d = g,  lambda = 1e-4, L the Laplacian of the path graph (+ 1 at (0, 0) with q_start),
 *              g_t = J_t^T e_t + w ((q_{t-1} - q_t) + (q_{t+1} - q_t))  (each difference where the neighbour exists, q_start as q_{-1});
 *              q_t <- clamp(f32(q_t + d_t), lo, hi).
 *   solve      block Cholesky (Thomas) recurrence, sequential in t:  S_0 = H_00,  S_t = H_tt - w^2 S_{t-1}^-1,  y_t = g_t + w S_{t-1}^-1 y_{t-1};
 *              d_{T-1} = S_{T-1}^-1 y_{T-1},  d_t = S_t^-1 (y_t + w d_{t+1}).  Every S_t goes through its Cholesky factor; no fused multiply-adds.
 *              With w = 0 every waypoint's step is the fp64 LM step of ikf_lm_step.
 *   loop       up to n_iters steps, 1 <= n_iters <= IKF_PATH_OPT_MAX_ITERS.  A step is kept only if F of the new f32 iterate is < F of the old one;
 *              otherwise the old iterate is restored and the loop ends (a NaN anywhere therefore ends it).  iters = steps kept.
 *   evaluator  the lattice's rules on ONE row per waypoint: node[t] = the row score of include/ikflow_amd_path.h of q_t against waypoint t under
 *              every rule set on the handle (world, cloud, manipulability floor, the world track's frame t), edges under max_joint_step and - a
 *              sweep set with something to test against - the sweep, the start edge included;
 *              cost = [edge(q_start, q_0) +] node_weight * node_0, then (cost + edge(q_{t-1}, q_t)) + node_weight * node_t, each step rounded in f32.
 *              For a path made of lattice rows this is the lattice's cost_out, bit for bit.  An inadmissible node or a forbidden edge: +inf.
 *   commit     validate != 0: the optimised path is returned only if iters > 0, it is admissible under the evaluator and its cost is strictly
 *              below the input path's cost by the same evaluator; otherwise the input path is returned bit for bit.  validate == 0: the
 *              optimiser's iterate as it is, with the evaluator's cost.
 * Outputs per path: path_out [T x ndof] (may be the input), cost_out the evaluator's cost of what is returned, info_out[4] int32
 * {iters, committed, reason, where}: reason IKF_PATH_OPT_* below, judged on the optimised path (validate == 0: committed = 1 and the reason tells
 * whether the evaluator admits it); where = the first offending waypoint (reason 2) or the waypoint the forbidden edge ends at (reason 3; 0: the
 * start edge), else -1.
 *
 * World track (include/ikflow_amd_track.h): P > 1 is refused with IKF_ERR_BAD_ARGUMENT as the batch entries refuse; P == 1 needs T <= frames.
 * Candidate refinement (include/ikflow_amd_refine.h) is a rule of the flow's rows and is not applied to the optimised rows.
 * Not covered: collision or clearance as residual terms (the world enters through the commit rule alone), adaptive damping, angle wrapping.
 */
#ifndef IKFLOW_AMD_PATH_OPT_H
#define IKFLOW_AMD_PATH_OPT_H

#include "ikflow_amd_path_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IKF_PATH_OPT_MAX_ITERS 32
#define IKF_PATH_OPT_COMMITTED 0        /* reason: the optimised path is returned */
#define IKF_PATH_OPT_NO_DESCENT 1       /* no step lowered F (or the path is a lattice's "no path") */
#define IKF_PATH_OPT_NODE 2             /* a node of the optimised path is inadmissible */
#define IKF_PATH_OPT_EDGE 3             /* an edge of the optimised path is forbidden */
#define IKF_PATH_OPT_COST 4             /* the optimised path does not cost less */

/* the caller's own paths: needs no weights */
ikf_status ikf_path_optimize(ikf_model* m, const float* d_waypoints /* [P*T x 7] */, int64_t P, int64_t T, const float* d_path_in /* [P*T x ndof] */,
                             const float* d_q_start /* [P x ndof], nullable */, const ikf_path_options* opt, int n_iters, float smooth_weight,
                             int validate, float* d_path_out /* [P*T x ndof] */, float* d_cost_out /* [P] */, int32_t* d_info_out /* [P x 4], nullable */,
                             void* stream);
/* the evaluator alone: info {0, admissible, reason 0 / 2 / 3, where} */
ikf_status ikf_path_cost(ikf_model* m, const float* d_waypoints, int64_t P, int64_t T, const float* d_path, const float* d_q_start,
                         const ikf_path_options* opt, float* d_cost_out /* [P] */, int32_t* d_info_out /* [P x 4], nullable */, void* stream);
/* State of the handle, like the sweep: n_iters == 0 (the default) is off.  While set, ikf_path_search, ikf_generate_path and both batch forms run
 * the optimiser with validate = 1 behind the lattice, on the same stream: path_out and cost_out are the committed path's; index_out, reachable_out
 * and node_cost_out stay the lattice's (index_out names the rows the optimisation started from); a path the lattice did not find stays the
 * "no path" output. */
ikf_status ikf_set_path_optimize(ikf_model* m, int n_iters, float smooth_weight);
ikf_status ikf_get_path_optimize(const ikf_model* m, int* n_iters_out, float* smooth_weight_out);
/* the info words [P x 4] of the handle's last optimising call (one of the two above, or a path call while the state is set); waits for that call */
ikf_status ikf_path_optimize_info(ikf_model* m, int64_t P, int32_t* h_info);
/* the optimiser's and the evaluator's scratch for up to max_paths x max_waypoints: a later call of that size or smaller allocates nothing - under
 * the rules that are set on the handle when it is called.  The evaluator's mask words are sized only while a sweep is set (ikf_set_path_sweep), its
 * cloud clearances and partial minima only while a cloud or a manipulability floor is set: one set afterwards sizes its buffers at the first call. */
ikf_status ikf_reserve_path_opt(ikf_model* m, int64_t max_paths, int64_t max_waypoints);

#ifdef __cplusplus
}
#endif
#endif /* IKFLOW_AMD_PATH_OPT_H */
