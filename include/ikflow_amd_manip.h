/*
 * ikflow_amd_manip.h - singularity rule: Yoshikawa's manipulability measure of a configuration, and a floor under it that the candidate stage
 * obeys.  An extension of the boundary (include/ikflow_amd.h), with the conventions of include/ikflow_amd_cloud.h: device pointers of the handle's
 * device, row-major f32, `stream` a hipStream_t (null: the default stream), no host synchronisation, nothing read back, every element of every
 * non-null output written, ikf_last_error for the message behind a status.
 *
 * The measure of a configuration q, computed in fp64 and returned as f32:
 *   J     the 6 x ndof geometric Jacobian of ikf_jacobian: rows 0-2 angular, rows 3-5 linear; a column per actuated joint - revolute
 *         [axis; axis x (p_ee - origin)], prismatic [0; axis]
 *   part  IKF_MANIP_FULL all 6 rows, IKF_MANIP_LINEAR rows 3-5, IKF_MANIP_ANGULAR rows 0-2: r rows
 *   w     sqrt(det G), G = J J^T when ndof >= r, else J^T J: the product of the min(r, ndof) singular values of those rows
 * The full measure mixes radians and metres - Yoshikawa's measure as published; the two parts are there for callers who mind.  w = 0 exactly
 * where the factorisation of G meets a pivot <= 0; w = NaN for a row with a NaN joint.  A row is BELOW a floor f exactly when !(w >= f): a NaN
 * row is below every floor.
 *
 * While a floor > 0 is set on the handle, a candidate row of ikf_rank_candidates, ikf_generate_ranked, ikf_path_search, ikf_generate_path,
 * ikf_diverse_select and ikf_generate_diverse is ALSO inadmissible (scores +inf exactly) when it is below the floor - beside the pose-error
 * bounds, the limits, self-collision and whatever ikf_set_world, ikf_set_world_cloud and ikf_set_world_track set.  Under
 * ikf_set_candidate_refine the refined rows are tested.  With no floor set those calls are what they were, launch for launch and bit for bit.
 *
 * Not covered: a manipulability term in the score (the rule only drops rows, it does not rank them); the rule inside exact IK
 * (ikf_generate_exact); the rule on the swept samples of a lattice edge (ikf_set_path_sweep tests path IK's NODES against the floor, not what
 * lies between them); the smallest singular value as a second measure.
 */
#ifndef IKFLOW_AMD_MANIP_H
#define IKFLOW_AMD_MANIP_H

#include "ikflow_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IKF_MANIP_FULL 0
#define IKF_MANIP_LINEAR 1
#define IKF_MANIP_ANGULAR 2

/* min_manipulability = 0 clears the rule, a finite value > 0 sets it.  A negative, NaN or infinite floor or a part outside 0 .. 2:
 * IKF_ERR_BAD_ARGUMENT, the state as it was.  Must not be called while calls on the handle are in flight. */
ikf_status ikf_set_min_manipulability(ikf_model* m, int part, float min_manipulability);
ikf_status ikf_min_manipulability(const ikf_model* m, int* part_out, float* min_out);   /* both outputs nullable */
/* per row of d_q [n x ndof]: the measure of `part` and !(w >= min_manipulability) - the call's own floor (finite, >= 0), not the handle's.
 * Needs neither weights nor a collision model.  n = 0: nothing to do; n < 0: IKF_ERR_BAD_ARGUMENT; both outputs null: IKF_ERR_NULL_POINTER. */
ikf_status ikf_manipulability(ikf_model* m, const float* d_q, int64_t n, int part, float min_manipulability,
                              float* d_w_out /* nullable */, uint8_t* d_below_out /* nullable */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IKFLOW_AMD_MANIP_H */
