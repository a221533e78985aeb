/*
 * ikflow_amd_world.h - world collision: static obstacles of the caller's scene, held by the handle, against the robot's capsules
 * (ikf_set_collision_model).  An extension of the boundary (include/ikflow_amd.h), beside include/ikflow_amd_rank.h, include/ikflow_amd_path.h
 * and include/ikflow_amd_diverse.h and with their conventions: device pointers of the handle's device, row-major f32, `stream` a hipStream_t
 * (null: the default stream), no host synchronisation, nothing read back, every element of every non-null output written, ikf_last_error for
 * the message behind a status.
 *
 * The world is up to IKF_WORLD_MAX_OBSTACLES obstacles in the base frame - the frame ikf_forward_kinematics reports poses in.  The clearance of
 * one robot capsule (segment e0-e1, radius rc) from one obstacle, by kind (these definitions are this project's own):
 *   IKF_OBSTACLE_SPHERE      a = centre, radius = r                         dist(a, segment) - r - rc
 *   IKF_OBSTACLE_CAPSULE     a, b = the segment's ends, radius = r          dist(segment a-b, segment) - r - rc
 *   IKF_OBSTACLE_HALF_SPACE  a = normal n, b[0] = offset d                  min(n.e0, n.e1) - d - rc        (solid where n.x <= d)
 *   IKF_OBSTACLE_BOX         a = centre, b = half extents h > 0,            min over t in [0, 1] of sdBox(R^T (e(t) - a), h) - r - rc
 *                            quat = (w, x, y, z) of R, radius = rounding r >= 0
 * with sdBox(p, h) = |max(|p| - h, 0)| + min(max_i(|p_i| - h_i), 0), the signed distance to an axis-aligned box.  Fields a kind does not name
 * are ignored (but must be finite).  A normal and a quaternion need not be normalised: ikf_set_world does it, in double precision.
 * World clearance of a configuration = the minimum over (robot capsule, obstacle); 3.0e38 in an empty world; negative when penetrating - for a
 * box and a half-space by the depth of the capsule's axis below the surface (plus radii), for a sphere and a capsule NOT by a penetration depth:
 * two axes that cross have distance 0 however deep they lie in each other.  Closest pair: on equal clearance the lower obstacle index, then the
 * lower capsule index.
 *
 * While a world of n > 0 obstacles is set, a candidate row of ikf_rank_candidates, ikf_generate_ranked, ikf_path_search, ikf_generate_path,
 * ikf_diverse_select and ikf_generate_diverse is ALSO inadmissible (scores +inf exactly) when its world clearance is < the world's
 * min_clearance - whatever reject_collisions says: that flag and the options' own min_clearance keep meaning the robot against itself.
 * Path IK tests its nodes; the configurations along its edges only while a sweep is set (include/ikflow_amd_sweep.h).
 * Exact IK obeys the world only while the exact collision rule is on (include/ikflow_amd_exact_world.h).
 * These obstacles stand still; obstacles that move along a path are a world track (include/ikflow_amd_track.h).
 */
#ifndef IKFLOW_AMD_WORLD_H
#define IKFLOW_AMD_WORLD_H

#include "ikflow_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IKF_WORLD_MAX_OBSTACLES 64
enum { IKF_OBSTACLE_SPHERE = 0, IKF_OBSTACLE_CAPSULE = 1, IKF_OBSTACLE_HALF_SPACE = 2, IKF_OBSTACLE_BOX = 3 };
typedef struct ikf_obstacle {
  int32_t kind;
  float a[3];
  float b[3];
  float quat[4];
  float radius;
} ikf_obstacle;   /* 48 bytes */

/* h_obstacles: HOST array; n_obstacles = 0 clears the world.  Validated on the host (unknown kind, non-finite number, radius < 0, half
 * extent <= 0, zero normal or quaternion, n outside 0 .. 64, non-finite min_clearance, n > 0 without a collision model: IKF_ERR_BAD_ARGUMENT,
 * the message names the obstacle), copied synchronously like ikf_set_collision_model.  Must not be called while calls on the handle are in
 * flight. */
ikf_status ikf_set_world(ikf_model* m, const ikf_obstacle* h_obstacles, int n_obstacles, float min_clearance);
int ikf_world_size(const ikf_model* m);   /* obstacles set; 0 for a null handle */
/* per row of d_q [n x ndof]: the world clearance, the closest pair (obstacle, capsule; -1 in an empty world) and clearance < min_clearance.
 * Needs a collision model; every output is nullable; n = 0: nothing to do. */
ikf_status ikf_world_clearance(ikf_model* m, const float* d_q, int64_t n, float* d_clearance_out, int32_t* d_obstacle_out,
                               int32_t* d_capsule_out, uint8_t* d_colliding_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IKFLOW_AMD_WORLD_H */
