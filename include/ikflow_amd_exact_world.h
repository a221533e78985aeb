/*
 * ikflow_amd_exact_world.h - exact IK that obeys the world: "in collision" as a reason for a repeat of the exact-IK retry loop not to count.
 * An extension of the boundary (include/ikflow_amd.h), beside include/ikflow_amd_world.h, include/ikflow_amd_cloud.h and
 * include/ikflow_amd_sweep.h and with their conventions: device pointers of the handle's device, row-major f32, `stream` a hipStream_t,
 * ikf_last_error for the message behind a status.  ABI version 3 as before: nothing that existed changes.
 *
 * Definitions (these are this project's own).  The handle carries an "exact collision rule": on, reject_self, self_min_clearance; the
 * default is off.  While it is on, ikf_generate_exact, ikf_generate_exact_seeded and ikf_refine_exact change as follows.
 *   candidate row    a row (repeat r of active pose j) is stepped exactly as without the rule.  Its candidate configuration is its q after the
 *                    first LM iteration `it` that leaves it below both thresholds: the same q and the same `it` the plain call records.  A row
 *                    never inside both thresholds has no candidate.  A row is not stepped further after its candidate, clear or not: the LM
 *                    step has no obstacle term, further steps would not move it away.
 *   admissible row   a row with a candidate is admissible when none of these rules rejects it:
 *                      (world rule) a world of n > 0 obstacles is set (ikf_set_world) and the candidate's world clearance
 *                                   (ikf_world_clearance) is < the world's min_clearance;
 *                      (cloud rule) a cloud of n > 0 points is set (ikf_set_world_cloud) and its cloud clearance (ikf_cloud_clearance) is <
 *                                   the cloud's min_clearance;
 *                      (self rule, only with reject_self) its capsule clearance (ikf_self_collision) is < self_min_clearance.
 *                    Each comparison is a strict `<`: a clearance equal to its threshold is admissible.
 *   selection        a pose is solved in a round by its admissible row of the earliest iteration, and among those the highest repeat: the
 *                    plain call's rule over admissible rows instead of candidate rows.  A pose with candidates but no admissible row is not
 *                    solved: it keeps zeros and valid = 0 in round 0, enters the next round's active list like any unsolved pose, and h_stats
 *                    column 3 does not count it.
 *   timing           the outputs - rows, valid flags, stats and the rejected counts below - are those of this definition for every
 *                    interleaving of the rows: under the rule no row is stopped by a sibling (the plain round's early-exit hint is not used).
 *   nothing to test  with the rule off, or on with an empty world, no cloud and reject_self == 0, the call launches the plain call's kernels and
 *                    is the plain call bit for bit.
 *   missing model    reject_self, or a non-empty world or cloud, without a collision model (ikf_set_collision_model) at call time:
 *                    IKF_ERR_BAD_ARGUMENT before any work is enqueued.
 *   joint limits     need no rule: the LM step clamps.
 */
#ifndef IKFLOW_AMD_EXACT_WORLD_H
#define IKFLOW_AMD_EXACT_WORLD_H

#include "ikflow_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The exact collision rule of this handle.  on == 0 (the default): off, reject_self and self_min_clearance are then ignored and kept as 0.
 * A self_min_clearance that is not finite: IKF_ERR_BAD_ARGUMENT, the previous state stays in force.  State of the handle, like the world
 * and the path sweep.  Must not be called while calls on the handle are in flight. */
ikf_status ikf_set_exact_collision(ikf_model* m, int on, int reject_self, float self_min_clearance);
/* The state through the non-null outputs; zeros for a null handle (the status is then IKF_ERR_NULL_POINTER). */
ikf_status ikf_get_exact_collision(const ikf_model* m, int* on_out, int* reject_self_out, float* self_min_clearance_out);
/* Per round of the handle's last exact call: the number of rows that had a candidate and were rejected; zeros for rounds that did not run
 * and for a call that ran the plain kernels (rule off, or nothing to test against).  Reads a device counter back: it waits for the handle's
 * last call.  The exact call itself synchronises no more than without the rule (once per retry round, for the count). */
ikf_status ikf_exact_collision_rejected(ikf_model* m, int64_t h_rows[IKF_MAX_ROUNDS]);

#ifdef __cplusplus
}
#endif
#endif /* IKFLOW_AMD_EXACT_WORLD_H */
