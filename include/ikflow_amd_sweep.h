/*
 * ikflow_amd_sweep.h - swept collision checks along edges: the configurations between two rows, sampled, against the handle's world
 * (include/ikflow_amd_world.h) and, when asked for, the robot against itself.  An extension of the boundary (include/ikflow_amd.h), beside
 * include/ikflow_amd_rank.h, include/ikflow_amd_path.h, include/ikflow_amd_diverse.h and include/ikflow_amd_world.h and with their
 * conventions: device pointers of the handle's device, row-major f32, `stream` a hipStream_t (null: the default stream), no host
 * synchronisation, nothing read back, every element of every non-null output written, ikf_last_error for the message behind a status.
 *
 * Definitions (these are this project's own):
 *   samples         a sweep has S interior samples, 1 <= S <= IKF_SWEEP_MAX_SAMPLES.
 *   configurations  for an edge from configuration a to configuration b (rows of ndof floats) sample i = 1 .. S is
 *                     q_i[j] = a[j] + f_i * (b[j] - a[j]),   f_i = (float)i / (float)(S + 1)
 *                   every operation rounded on its own (no fused multiply-add), so sequential f32 arithmetic reproduces them bit for bit.  A
 *                   prismatic joint interpolates the same way.  The end points are not sampled: they are nodes.
 *   blocked sample  a sample is blocked when
 *                     (world rule) a world of n > 0 obstacles is set and the world clearance of q_i is < the world's min_clearance, or
 *                     (self rule, only when asked for) the capsule clearance of q_i (ikf_self_collision) is < self_min_clearance.
 *   joint limits    are not tested along an edge: the limits are a box, so every sample between two rows inside it is inside it.
 *   blocked edge    an edge is blocked when any of its samples is; its first blocked sample is the lowest such i - 1 (0-based), -1 when the
 *                   edge is free.
 *
 * In path IK (include/ikflow_amd_path.h): while a sweep of S > 0 is set on the handle (ikf_set_path_sweep), an edge of the lattice -
 * the start edge q_start -> q[0][r] included - is forbidden, exactly as a step-gate violation forbids it, when it is blocked.  The world rule
 * uses the handle's world and its min_clearance; the self rule applies when opt->reject_collisions, with opt->min_clearance.  Everything else
 * of that header stays as written: node costs, the order among predecessors, the no-path outputs, reachable_out.  With a sweep set but no
 * world and reject_collisions == 0 there is nothing to test against: the call is the call without a sweep, bit for bit.
 *
 * Resolution: with max_joint_step = s >= 0, consecutive tested configurations of an admitted edge differ by at most s / (S + 1) per joint.
 * The sweep is SAMPLED, not conservative: what the arm crosses between two samples is not seen.  The caller covers that gap with
 * min_clearance.  Obstacles that move along the path are a world track (include/ikflow_amd_track.h), swept beside these rules.
 */
#ifndef IKFLOW_AMD_SWEEP_H
#define IKFLOW_AMD_SWEEP_H

#include "ikflow_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IKF_SWEEP_MAX_SAMPLES 16

/* Samples per lattice edge of ikf_path_search / ikf_generate_path on this handle; 0 (the default): no sweep.  A value outside 0 .. 16:
 * IKF_ERR_BAD_ARGUMENT, the previous value stays in force.  State of the handle, like the world.  Must not be called while calls on the
 * handle are in flight. */
ikf_status ikf_set_path_sweep(ikf_model* m, int n_samples);
int ikf_get_path_sweep(const ikf_model* m);   /* 0 for a null handle */
/* The caller's own edges: row i of d_q_a -> row i of d_q_b ([n x ndof] each), n_samples in 1 .. 16 -> blocked [n] (0 / 1) and the first
 * blocked sample [n] (-1: free).  The world rule with the handle's world; the self rule when reject_self != 0.  Needs a collision model, not
 * weights; the outputs are nullable, but not both; n = 0: nothing to do.  An empty world with reject_self == 0: every edge is free. */
ikf_status ikf_sweep_edges(ikf_model* m, const float* d_q_a, const float* d_q_b, int64_t n, int n_samples, int reject_self,
                           float self_min_clearance, uint8_t* d_blocked_out, int32_t* d_first_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IKFLOW_AMD_SWEEP_H */
