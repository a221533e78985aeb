/*
 * ikflow_amd_track.h - a world that moves along a path: one frame of obstacles per waypoint of path IK, its nodes tested against their own
 * frame and the samples of its swept edges against frames interpolated in between.  An extension of the boundary (include/ikflow_amd.h), beside
 * include/ikflow_amd_world.h, include/ikflow_amd_path.h and include/ikflow_amd_sweep.h and with their conventions: device pointers of the
 * handle's device, row-major f32, `stream` a hipStream_t (null: the default stream), no host synchronisation, nothing read back, every element
 * of every non-null output written, ikf_last_error for the message behind a status.  ikf_path_options and ABI version 3 are as they were.
 *
 * Definitions (these are this project's own):
 *   world track   F key frames, 1 <= F <= IKF_WORLD_TRACK_MAX_FRAMES, each the same n obstacles (1 <= n <= IKF_WORLD_MAX_OBSTACLES) as
 *                 ikf_obstacle records; obstacle o has the same kind in every frame.  An obstacle that appears or disappears is moved far
 *                 away by the caller.  The track has its own min_clearance.  It is state of the handle beside the static world
 *                 (ikf_set_world) and the cloud (ikf_set_world_cloud) and independent of them: all of them apply when set.
 *   nodes         while a track is set, ikf_path_search / ikf_generate_path ALSO treat candidate r of waypoint t (row r * T + t) as
 *                 inadmissible - its node costs +inf exactly - when the world clearance (include/ikflow_amd_world.h) of the row against key
 *                 frame t is < the track's min_clearance, whatever reject_collisions says.  A call with T > F: IKF_ERR_BAD_ARGUMENT, before
 *                 anything is enqueued.  Ranked and diverse IK have no time axis and do not read the track.
 *   fine frames   between key frames t and t + 1 lie S fine frames, S the handle's ikf_get_path_sweep(); fine frame i = 1 .. S is
 *                 interpolated at u = i / (S + 1), on the host, in double precision, from the normalised key frames, and rounded once to f32:
 *                   sphere, capsule   a, b and radius linear
 *                   half-space        the unit normals linear, then normalised; the offset linear.  A blended normal shorter than 1e-6 is
 *                                     refused (the message names frame and obstacle)
 *                   box               centre, half extents and rounding linear; the second quaternion negated when its dot product with
 *                                     the first is < 0, then both blended linearly and normalised
 *                 The fine table has (F - 1) (S + 1) + 1 frames of n records; index t (S + 1) + i is fine frame i after key frame t, and
 *                 i = 0 is the key frame itself, bit for bit.  ikf_set_world_track and ikf_set_path_sweep rebuild it, synchronously.
 *   edges         while a track and a sweep S > 0 are set, sample i of the lattice edge into waypoint t >= 1 is ALSO blocked when the world
 *                 clearance of q_i against fine frame (t - 1) (S + 1) + i is < the track's min_clearance; the samples of the start edge
 *                 q_start -> q[0][r] are tested against key frame 0.  The world rule and the self rule of include/ikflow_amd_sweep.h apply
 *                 unchanged beside it, and a track alone is enough for the edges to be swept.  With a track but S = 0 only nodes are tested.
 * Not covered: continuous time within an edge (the obstacle is where its fine frame puts it at each sample, nothing in between), a track
 * for the cloud, ranked or diverse IK.
 */
#ifndef IKFLOW_AMD_TRACK_H
#define IKFLOW_AMD_TRACK_H

#include "ikflow_amd_world.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IKF_WORLD_TRACK_MAX_FRAMES 1024

/* h_frames: HOST array [n_frames][n_obstacles]; n_frames = 0 clears the track.  Every record is validated as ikf_set_world validates it, and
 * further: n_frames in 0 .. 1024, n_obstacles in 1 .. 64, equal kinds across frames, blended normals under the sweep that is set, a finite
 * min_clearance, a collision model - IKF_ERR_BAD_ARGUMENT, the message names frame and obstacle, and the previous track stays in force.
 * Copied synchronously.  Must not be called while calls on the handle are in flight. */
ikf_status ikf_set_world_track(ikf_model* m, const ikf_obstacle* h_frames, int n_frames, int n_obstacles, float min_clearance);
/* key frames and obstacles per frame of the track that is set (0, 0 without one); either output is nullable */
ikf_status ikf_world_track_size(const ikf_model* m, int* n_frames, int* n_obstacles);
/* the f32 records the device reads for fine frame i (0 .. S; 0 only for the last key frame) after key frame t -> h_out [n_obstacles], HOST */
ikf_status ikf_world_track_frame(const ikf_model* m, int t, int i, ikf_obstacle* h_out);
/* per row of d_q [k * T x ndof] tile-major: row r * T + t against key frame t -> as ikf_world_clearance, colliding = clearance < the track's
 * min_clearance.  Needs a track with T <= F; every output is nullable; T = 0: nothing to do. */
ikf_status ikf_world_track_clearance(ikf_model* m, const float* d_q, int64_t T, int k, float* d_clearance_out, int32_t* d_obstacle_out,
                                     int32_t* d_capsule_out, uint8_t* d_colliding_out, void* stream);
/* The mask a path call builds from these rows, in its layout: d_edge_free_out [T][k][ceil(k / 64)] words; bit j % 64 of word j / 64 of
 * [t][r] is set when the edge from candidate j of waypoint t - 1 to candidate r of waypoint t is free; row t = 0 carries the start edge
 * q_start -> q[0][r] in bit 0 of word 0 (all ones without q_start).  The handle's S (S = 0: IKF_ERR_BAD_ARGUMENT) against the static world,
 * the track (T <= F) and - reject_self - the robot itself, whichever are set; nothing is pruned by node costs or a step gate.  With k = 1 it is
 * the check of one timed path.  Needs a collision model; T = 0: nothing to do. */
ikf_status ikf_sweep_lattice(ikf_model* m, const float* d_q, int64_t T, int k, const float* d_q_start, int reject_self, float self_min_clearance,
                             uint64_t* d_edge_free_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IKFLOW_AMD_TRACK_H */
