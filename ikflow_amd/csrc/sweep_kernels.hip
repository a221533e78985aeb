// Swept collision checks along edges for gfx950 (include/ikflow_amd_sweep.h): S interpolated configurations of every edge against the handle's
// obstacles and, when asked for, the robot against itself.  The arithmetic is sweep_math.h; this kernel only places it.
//
// k_sweep_edges is ONE kernel with two edge sources, and both sources reach sweep_edge through the same call: the same source inlined into two
// kernels was seen to be contracted differently, and a sample within an ulp of a threshold must get the same verdict
// from ikf_sweep_edges and from a path call.
//   pair source     lane = edge i of the caller's rows qa[i] -> qb[i]; writes a byte flag and the first blocked sample.
//   lattice source  one wave per (waypoint t, destination r, block of 64 predecessors); lane = predecessor j of waypoint t - 1, the destination
//                   row is wave-uniform.  The verdicts of a wave leave as ONE 64-bit word, __ballot(free), stored by one lane into
//                   edge_free[t][r][word] - no atomics, no two waves touch a word.  Row t = 0 carries the start edge in bit 0 (all ones
//                   without q_start).  A lane does no samples and reports 0 when its predecessor's or its destination's node cost is +inf or
//                   the step gate forbids its edge: the search never takes such an edge, so no result depends on the pruned bit.
// The geometry of k_world_clearance: 64-thread workgroups, the lane's capsule end points in LDS (one slice per lane, stride (6 n_caps) | 1: odd,
// so the lanes' slices start in different banks), the obstacle table staged once per workgroup and read as a broadcast.  A workgroup walks
// waves blockIdx.x, blockIdx.x + gridDim.x, ...  Samples in ascending order; a lane stops at its first blocked sample.
//
// TRACK (the lattice source under a world track, include/ikflow_amd_track.h; taken only while a track is set): the waypoint t of a wave is
// wave-uniform, so the fine frame a sample reads is too.  Per sample the wave stages that frame's n_track records into LDS behind the static
// table (the start edge's key frame 0 once), every lane reads it as a broadcast like the static table, the lanes that are still undecided test
// the sample (track_sample_blocked, track_math.h), and the wave leaves the sample loop when every lane is decided.  TRACK = false is the kernel
// as it was, instruction for instruction (profiles/sweep_kernel_resources.txt).
//
// BATCH (the lattice source over P paths in one layout of P T waypoints, include/ikflow_amd_path_batch.h; taken only by the batch entries): a
// wave's waypoint g of the layout gives its path p = g / T and its waypoint t = g % T inside it (path_batch_math.h).  t == 0 is the start edge
// of path p, from q_start[p]; otherwise the predecessor row is j P T + g - 1.  The mask is sweep_word_index over P T waypoints, so wave = word
// as before.  Never together with TRACK.  BATCH = false is the kernel as it was.
#include "ikf_internal.h"

namespace ikf {

constexpr size_t kSweepMaxLds = sizeof(float) * ((size_t)IKF_WORLD_TABLE_WORDS + IKF_SWEEP_LANES * (size_t)(IKF_MAX_CAPSULES * 6 + 1));
static_assert(kSweepMaxLds == 4096 + 37120, "obstacle table + one wave's capsule slices");
static_assert(kSweepMaxLds <= 48 * 1024 && kSweepMaxLds <= 160 * 1024, "a sweep workgroup fits the default dynamic LDS and a CU");
constexpr size_t kSweepTrackMaxLds = kSweepMaxLds + sizeof(float) * (size_t)IKF_WORLD_TABLE_WORDS;
static_assert(kSweepTrackMaxLds == 4096 + 4096 + 37120, "obstacle table + one fine frame + one wave's capsule slices");
static_assert(kSweepTrackMaxLds <= 48 * 1024, "a tracked sweep workgroup fits the dynamic LDS that needs no opt-in");
constexpr long long kSweepMaxGrid = 1LL << 20;

template <int NDOF, bool TRACK, bool BATCH>
__global__ __launch_bounds__(IKF_SWEEP_LANES) void k_sweep_edges(const SweepArgs a) {
  static_assert(!(TRACK && BATCH), "a world track has one frame per waypoint of ONE path");
  extern __shared__ float sweep_lds[];   // [n_obs x 16] obstacle table, then [64][cap_stride] capsule end points
  const int lane = threadIdx.x;
  const int n_obs = a.n_obs;
  float* const OBS = sweep_lds;
  const float* const src = n_obs > 0 ? reinterpret_cast<const float*>(a.world->obs) : nullptr;
  for (int i = lane; i < n_obs * IKF_WORLD_OBSTACLE_WORDS; i += IKF_SWEEP_LANES) OBS[i] = src[i];
  __syncthreads();
  const int n_track = TRACK ? a.n_track : 0;
  float* const FRAME = sweep_lds + n_obs * IKF_WORLD_OBSTACLE_WORDS;   // TRACK: [n_track x 16] the fine frame of the sample in hand
  float* const w = FRAME + n_track * IKF_WORLD_OBSTACLE_WORDS + lane * ((a.n_caps * 6) | 1);
  const bool lattice = a.lattice != 0;
  const long long T = a.T;
  const int k = a.k;
  const long long G = BATCH ? path_batch_waypoints(a.P, T) : T;   // waypoints of the layout: the row stride of q and node
  const long long n_waves = lattice ? sweep_mask_words(G, k) : sweep_pair_waves(a.n);
  for (long long wave = blockIdx.x; wave < n_waves; wave += gridDim.x) {
    float ea[NDOF], eb[NDOF];
#pragma unroll
    for (int d = 0; d < NDOF; ++d) { ea[d] = 0.f; eb[d] = 0.f; }
    bool active = false, all_free = false;
    const long long i = wave * IKF_SWEEP_LANES + lane;   // pair source: the lane's edge
    if (lattice) {
      long long g, t;   // the wave's waypoint in the layout, and inside its path (the same without a batch)
      int r, word;
      sweep_wave_role(wave, k, &g, &r, &word);
      t = g;
      const float* q_start = a.q_start;
      if constexpr (BATCH) {   // t == 0 is the start edge of path p: nothing joins it to the last waypoint of path p - 1
        const PathBatchRole role = path_batch_role(g, T);
        t = role.t;
        if (q_start) q_start += role.p * NDOF;
      }
      const int j = word * IKF_SWEEP_LANES + lane;
      const bool dest_ok = a.node[(long long)r * G + g] < rank_inf();
      const float* pa = nullptr;
      if (t == 0) {
        all_free = q_start == nullptr;
        if (q_start && j == 0 && dest_ok) pa = q_start;
      } else if (j < k && dest_ok && a.node[(long long)j * G + g - 1] < rank_inf()) {
        pa = a.q + ((long long)j * G + g - 1) * NDOF;
      }
      if (pa) {
        const float* const pb = a.q + ((long long)r * G + g) * NDOF;
        active = true;
#pragma unroll
        for (int d = 0; d < NDOF; ++d) {
          ea[d] = pa[d];
          eb[d] = pb[d];
          const float df = eb[d] - ea[d];   // the step gate of path_edge
          if (a.max_joint_step >= 0.f && fabsf(df) > a.max_joint_step) active = false;
        }
      }
    } else if (i < a.n) {
      active = true;
      load_q<NDOF>(a.qa, i, ea);
      load_q<NDOF>(a.qb, i, eb);
    }
    int first = -1;
    if constexpr (TRACK) {
      long long t;
      int r, word;
      sweep_wave_role(wave, k, &t, &r, &word);
      const int S = a.n_samples;
      bool undecided = active;
      for (int i = 1; i <= S; ++i) {
        if (__ballot(undecided) == 0ULL) break;   // wave-uniform: the barriers below are reached by all 64 lanes or by none
        if (i == 1 || t > 0) {
          const float* const fsrc = reinterpret_cast<const float*>(a.track + track_sample_frame(t, i, S) * n_track);
          __syncthreads();   // (the previous sample's readers are done with FRAME)
          for (int x = lane; x < n_track * IKF_WORLD_OBSTACLE_WORDS; x += IKF_SWEEP_LANES) FRAME[x] = fsrc[x];
          __syncthreads();
        }
        if (undecided && track_sample_blocked<NDOF>(a.ch, a.cm, reinterpret_cast<const WorldObstacle*>(OBS), n_obs, a.world_min_clearance,
                                                    a.reject_self != 0, a.self_min_clearance, reinterpret_cast<const WorldObstacle*>(FRAME),
                                                    n_track, a.track_min_clearance, ea, eb, i, S, w)) {
          first = i - 1;
          undecided = false;
        }
      }
      __syncthreads();   // (the next wave of this workgroup restages FRAME)
    } else if (active)
      first = sweep_edge<NDOF>(a.ch, a.cm, reinterpret_cast<const WorldObstacle*>(OBS), n_obs, a.world_min_clearance, a.reject_self != 0,
                               a.self_min_clearance, ea, eb, a.n_samples, w);
    if (lattice) {
      const unsigned long long verdicts = __ballot(active && first < 0);
      if (lane == 0) a.edge_free[wave] = all_free ? ~0ULL : verdicts;
    } else if (i < a.n) {
      if (a.blocked_out) a.blocked_out[i] = first >= 0 ? 1 : 0;
      if (a.first_out) a.first_out[i] = first;
    }
  }
}

hipError_t launch_sweep_edges(int ndof, const SweepArgs& a, hipStream_t s) {
  if (!a.ch || !a.cm || a.n_caps < 0 || a.n_caps > IKF_MAX_CAPSULES || a.n_obs < 0 || a.n_obs > IKF_WORLD_MAX_OBSTACLES || (a.n_obs > 0 && !a.world) ||
      a.n_samples < 1 || a.n_samples > IKF_SWEEP_MAX_SAMPLES)
    return hipErrorInvalidValue;
  long long waves;
  if (a.lattice) {
    const long long paths = a.P > 0 ? a.P : 1;
    if (a.T < 1 || a.k < 1 || a.k > IKF_PATH_MAX_K || a.P < 0 || (long long)a.k * a.T * paths > 0x7fffffffLL || !a.q || !a.node || !a.edge_free)
      return hipErrorInvalidValue;
    waves = sweep_mask_words(a.T * paths, a.k);
  } else {
    if (a.n <= 0) return hipSuccess;
    if (!a.qa || !a.qb || (!a.blocked_out && !a.first_out)) return hipErrorInvalidValue;
    waves = sweep_pair_waves(a.n);
  }
  const bool track = a.lattice && a.track != nullptr && a.n_track > 0;
  if (track && (a.n_track > IKF_WORLD_MAX_OBSTACLES || a.track_frames < 1 || a.T > a.track_frames)) return hipErrorInvalidValue;
  const size_t lds = sizeof(float) * (((size_t)a.n_obs + (track ? a.n_track : 0)) * IKF_WORLD_OBSTACLE_WORDS +
                                      IKF_SWEEP_LANES * (size_t)((a.n_caps * 6) | 1));
  const unsigned grid = (unsigned)(waves < kSweepMaxGrid ? waves : kSweepMaxGrid);
  const bool batch = a.lattice && a.P > 0;
  if (track && batch) return hipErrorInvalidValue;   // frames per batched path: not covered (include/ikflow_amd_path_batch.h)
  if (track) {
    IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_sweep_edges<ND, true, false>), dim3(grid), dim3(IKF_SWEEP_LANES), lds, s, a));
  } else if (batch) {
    IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_sweep_edges<ND, false, true>), dim3(grid), dim3(IKF_SWEEP_LANES), lds, s, a));
  } else {
    IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_sweep_edges<ND, false, false>), dim3(grid), dim3(IKF_SWEEP_LANES), lds, s, a));
  }
  return hipGetLastError();
}

}  // namespace ikf
