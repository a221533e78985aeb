/*
 * ikflow_amd_cloud.h - world point cloud: the sensed scene as points, held by the handle, against the robot's capsules
 * (ikf_set_collision_model).  An extension of the boundary (include/ikflow_amd.h), beside include/ikflow_amd_world.h and with its conventions:
 * device pointers of the handle's device, row-major f32, `stream` a hipStream_t (null: the default stream), no host synchronisation, nothing read
 * back, every element of every non-null output written, ikf_last_error for the message behind a status.
 *
 * The cloud is a second world on the handle, independent of the primitives of ikf_set_world: n points p_i in the base frame - the frame
 * ikf_forward_kinematics reports poses in -, 0 <= n <= IKF_CLOUD_MAX_POINTS, each a sphere of the one point_radius r >= 0, with the cloud's own
 * min_clearance.  These definitions are this project's own:
 *   squared distance of p from a capsule axis e0-e1:   d = e1 - e0, a = d.d, inv = a <= 1e-12f ? 0 : 1 / a   (once per capsule)
 *                                                      t = clamp(((p - e0).d) * inv, 0, 1), v = (p - e0) - d t, dist2 = v.v
 *   cloud clearance of a configuration:                min over capsules c of ( sqrtf( min over i of dist2(p_i, axis_c) ) - rc_c ) - r
 * The inner minimum is taken in squared distance, there is one sqrtf per capsule, rc_c comes off per capsule and r once at the end.  3.0e38 with
 * an empty cloud or a capsule model of no capsules; negative when penetrating - as for the sphere of ikf_set_world NOT by a penetration depth:
 * a point on an axis has distance 0 however deep it lies in the capsule.  sqrtf and x - rc are monotone, so the minimum over any partition of
 * the points gives the same bits: the value does not depend on how a call splits the points over waves, tiles or workgroups.
 *
 * While a cloud of n > 0 points is set, a candidate row of ikf_rank_candidates, ikf_generate_ranked, ikf_path_search, ikf_generate_path,
 * ikf_diverse_select and ikf_generate_diverse is ALSO inadmissible (scores +inf exactly) when its cloud clearance is < the cloud's
 * min_clearance - whatever reject_collisions says, and beside whatever ikf_set_world set.  Under ikf_set_candidate_refine the refined rows are
 * tested.
 *
 * Not covered: the sweep - while a cloud is set, ikf_set_path_sweep and ikf_sweep_edges keep testing the primitives and the robot itself only
 * (path IK tests its NODES against the cloud; edges times samples against 10^4 .. 10^6 points need a broad phase); a closest (point, capsule)
 * pair; a device-side source of points; per-point radii; culling of any kind.  Exact IK obeys the cloud only while the exact collision rule is
 * on (include/ikflow_amd_exact_world.h).
 */
#ifndef IKFLOW_AMD_CLOUD_H
#define IKFLOW_AMD_CLOUD_H

#include "ikflow_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IKF_CLOUD_MAX_POINTS (1 << 20)

/* h_points: HOST array [n_points x 3]; n_points = 0 clears the cloud (its device array stays allocated).  Validated on the host (n outside
 * 0 .. 2^20, non-finite or negative point_radius, non-finite min_clearance, n > 0 without a collision model, a non-finite coordinate:
 * IKF_ERR_BAD_ARGUMENT, the message names the point; a null table with n > 0: IKF_ERR_NULL_POINTER), copied synchronously like ikf_set_world;
 * a refused call leaves the previous cloud in force.  Must not be called while calls on the handle are in flight. */
ikf_status ikf_set_world_cloud(ikf_model* m, const float* h_points, int64_t n_points, float point_radius, float min_clearance);
int64_t ikf_world_cloud_size(const ikf_model* m);   /* points set; 0 for a null handle */
/* per row of d_q [n x ndof]: the cloud clearance (3.0e38 with an empty cloud) and clearance < min_clearance.  Needs a collision model; both
 * outputs are nullable; n = 0: nothing to do. */
ikf_status ikf_cloud_clearance(ikf_model* m, const float* d_q, int64_t n, float* d_clearance_out, uint8_t* d_colliding_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IKFLOW_AMD_CLOUD_H */
