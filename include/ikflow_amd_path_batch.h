/*
 * ikflow_amd_path_batch.h - path IK for many paths per call: P paths of T waypoints each (the same T and the same k for every path), searched side
 * by side on the GPU - one lattice workgroup per path - behind ONE candidate stage of P * T waypoints.  An extension of include/ikflow_amd_path.h
 * with its conventions: device pointers of the handle's device, row-major f32, `stream` a hipStream_t (null: the default stream), no host
 * synchronisation, nothing read back, every element of every non-null output written, ikf_last_error for the message behind a status.
 *
 * Layout: global waypoint g = p * T + t is waypoint t of path p.  Row r * (P * T) + g of d_q (or of d_latent) is candidate r of that waypoint:
 * the tile-major candidate layout of include/ikflow_amd_rank.h with n_poses = P * T.  d_waypoints, d_path_out, d_index_out and d_reachable_out are
 * indexed by g, d_q_start and d_cost_out by p, d_node_cost_out like d_q.
 *
 * Definition: path p is what ikf_path_search returns for its own k x T lattice - the rows r * (P * T) + p * T + t gathered into [k * T]
 * tile-major - with d_q_start + p * ndof as its start: the node costs, the edge, the step gate, the total order, the "no path" outputs (rows 0,
 * indices -1, cost +inf) and the rounding of every step of include/ikflow_amd_path.h.  No edge joins the last waypoint of one path to the first
 * of the next, and the outputs of path p depend on nothing outside path p.
 *
 * 1 <= k <= IKF_PATH_MAX_K, P >= 0, T >= 0, k * P * T <= 2^31 - 1.  P == 0 or T == 0: nothing to do, IKF_OK, nothing written.  A refused call leaves
 * every output untouched.  What is set on the handle and a single path call obeys is obeyed per path: ikf_set_world, ikf_set_world_cloud,
 * ikf_set_min_manipulability, ikf_set_candidate_refine - on the flow's rows, so in ikf_generate_path_batch alone - and ikf_set_path_sweep, the
 * start edge of every path, from d_q_start[p], included.
 *
 * Not covered:
 *   - a world track (include/ikflow_amd_track.h): while ikf_set_world_track has frames set, both entries return IKF_ERR_BAD_ARGUMENT and say so in
 *     ikf_last_error.  A track is one frame per waypoint of ONE path; frames per batched path are a separate piece of work.
 *   - per-path lengths, per-path k, per-path options: one T, one k and one ikf_path_options for the whole call.
 */
#ifndef IKFLOW_AMD_PATH_BATCH_H
#define IKFLOW_AMD_PATH_BATCH_H

#include "ikflow_amd_path.h"

#ifdef __cplusplus
extern "C" {
#endif

/* candidates supplied by the caller: needs no weights */
ikf_status ikf_path_search_batch(ikf_model* m, const float* d_waypoints /* [P*T x 7] */, int64_t P, int64_t T, int k,
                                 const float* d_q /* [k*P*T x ndof] */, const float* d_q_start /* [P x ndof], nullable */,
                                 const ikf_path_options* opt, float* d_path_out /* [P*T x ndof] */, int32_t* d_index_out /* [P*T] */,
                                 float* d_cost_out /* [P] */, int32_t* d_reachable_out /* [P*T], nullable */,
                                 float* d_node_cost_out /* [k*P*T], nullable */, void* stream);
/* flow + search: shared_latent != 0: d_latent [k x D], candidate r uses latent r at every waypoint of every path; else d_latent [k*P*T x D] in the
 * candidate layout */
ikf_status ikf_generate_path_batch(ikf_model* m, const float* d_waypoints, int64_t P, int64_t T, int k, const float* d_latent, int shared_latent,
                                   int clamp_to_limits, const float* d_q_start, const ikf_path_options* opt, float* d_path_out,
                                   int32_t* d_index_out, float* d_cost_out, int32_t* d_reachable_out, float* d_node_cost_out, void* stream);
/* flow scratch + candidate rows + lattice scratch of up to max_paths x max_waypoints x max_k: a later call of that size or smaller allocates nothing */
ikf_status ikf_reserve_path_batch(ikf_model* m, int64_t max_paths, int64_t max_waypoints, int max_k);

#ifdef __cplusplus
}
#endif
#endif /* IKFLOW_AMD_PATH_BATCH_H */
