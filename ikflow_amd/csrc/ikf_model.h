// The handle behind the C-ABI (struct ikf_model) and what the API units api_handle / api_weights / api_flow / api_kin share: error
// reporting, the device and stream scopes, the profiling mark, and the few host functions that cross a unit boundary.  Included by
// those units (and api_rank / api_path / api_diverse / api_world / api_cloud / api_sweep / api_refine / api_exact_world / api_manip) only; the kernel-launch interface is ikf_internal.h.
#pragma once
#include <cstddef>
#include <cstring>
#include <string>
#include <chrono>
#include <cmath>
#include <utility>
#include <unordered_map>
#include <vector>

#include "ikf_internal.h"
#include "device_buf.h"  // DeviceBuf / PinnedBuf: every allocation of the handle is owned by a member of one of these types

using namespace ikf;  // (this header is for the API units alone)

#define IKF_HIP(call)                                                                                          \
  do {                                                                                                         \
    hipError_t e_ = (call);                                                                                    \
    if (e_ != hipSuccess)                                                                                      \
      return fail(IKF_ERR_HIP, std::string(#call) + " failed: " + hipGetErrorString(e_) + " (" __FILE__ ":" + \
                                   std::to_string(__LINE__) + ")");                                            \
  } while (0)

// Every entry point runs on the handle's device and leaves the caller's current device as it found it.
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int device) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != device) err = hipSetDevice(device);
    else if (err == hipSuccess) prev = -1;  // nothing to restore
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define IKF_ON_DEVICE(m)                                                                                       \
  DeviceGuard dev_guard_((m)->device);                                                                         \
  if (dev_guard_.err != hipSuccess)                                                                            \
    return fail(IKF_ERR_HIP, std::string("hipSetDevice failed: ") + hipGetErrorString(dev_guard_.err));

struct ikf_model {
  int device = 0;
  // the per-handle scratch is shared by all calls: a call that arrives on a different stream than the previous one
  // first waits for the event recorded behind the previous call's work
  hipEvent_t tail_event = nullptr;
  hipStream_t tail_stream = nullptr;
  bool tail_valid = false;
  ikf_model_desc desc{};
  FlowDims dims{};
  bool loaded = false;
  int gemm_variant = -1;  // -1 = choose by batch size
  int tile_cfg = -1;      // fused pipeline: -1 = choose by batch size, 0..3 forced (variant 100..103)
  int fuse_entry = 1;     // small batches: entry kernel + first hidden contraction as one launch (0: always two launches)
  // the next subnet's entry phase in the tail of the last hidden contraction (TailSync).  OFF by default: measured slower than the
  // k_subnet_entry launch it replaces (r03: +3.6 % per call at 4096 rows, +7.4 % at 512) - kept as a tested,
  // bit-identical opt-in (ikf_set_gemm_variant 121) because it is the priced answer to "hand over inside the launch"
  int tune = IKF_TUNE_DEFAULT;  // IKF_TUNE_* switches of the small-batch kernels (ikf_set_gemm_variant 150 .. 163)
  int fuse_tail = 0;
  // Activation stores write-through (sc1): the lines go to memory as they are written instead of sitting dirty in the XCD L2s until the
  // launch's end flushes them (r03, tools/variant_ab.py: 3.261 -> 3.229 ms per call at 4096 rows with the contractions' stores
  // write-through, 1.831 -> 1.796 at 2048 and 0.721 -> 0.706 at 512 with the entry kernel's too; the entry kernel's 16-byte stores do
  // not pay at 4096 rows).  bit 0 contractions, bit 1 entry kernel; -1 = by batch size (contractions always, entry kernel <= 2048 rows)
  int wt_stores = -1;
  // <= 128 rows: the whole subnet chain in one launch, hand-over inside each XCD (k_flow_chain16, flow_fused.hip).  OFF by default:
  // bit-identical to the per-layer launches but slower (r03: 0.422 against 0.365 ms per call at 128 rows, 0.362 against 0.271 at 1 row) -
  // a hand-over inside an XCD needs the ROWS partitioned over the XCDs, so every XCD's L2 pulls the whole 4.2 MB weight matrix of every
  // layer (8 x the traffic of the per-layer launches, whose column tiles are spread over the XCDs), and small batches are bound by
  // exactly that stream.  Kept as the tested, priced answer to "XCD-local synchronisation".
  //   chain_mode: 0 off, 1 on (ikf_set_gemm_variant 170 / 171); chain_census: -1 not yet taken, 0 the dispatcher does not hand 32
  //   workgroups to each of 8 XCDs on this device (the chain is never used), 1 verified
  int chain_mode = 0, chain_census = -1;
  DeviceBuf<ChainSubnet> d_chain_tab;  // [2 nb_nodes] per-subnet arguments, rebuilt when the weights or the scratch change
  bool chain_tab_valid = false;
  DeviceBuf<unsigned> d_chain_ctl;     // [IKF_CHAIN_CTL_WORDS], zero between calls (the launch's last workgroup re-zeroes it)
  DeviceBuf<unsigned> d_arrive;  // [kArriveWords] row-tile arrival counters of the fused tail (zeroed by every call's first entry kernel)
  PinnedBuf<int> h_give_up;      // pinned, device-visible: set by a workgroup whose in-launch wait ran out
  int precision = 0;      // 0: hidden contractions on the exact-f32 MFMA; 1: error-compensated 3x f16 MFMA split
  int lm_precision = 1;   // LM step: 1 fp64 inside (Cholesky), 0 the reference's fp32 arithmetic (LU, partial pivoting) - ikf_set_lm_precision
  DeviceBuf<uint16_t> split_arena;  // split-32 images of the hidden Linear weights
  std::vector<const void*> w_mid_split;  // [subnet][layer] -> device pointer (flattened: subnet*3 + layer)
  DeviceBuf<float> split_frag_arena;     // fragment-major copies of the split-32 images (small-batch f16-split kernel)
  std::vector<const void*> w_mid_split_frag;
  // fragment-major images of the hidden Linear weights (small-batch per-layer kernels, <= 512 rows): built by the first chunk that needs
  // them, or ahead of time by ikf_reserve - a handle whose small batches run the cluster form never pays the 201 MB / the pack launches
  DeviceBuf<float> wfrag_arena;
  bool wfrag_built = false;
  double load_ms = 0.0, frag_ms = 0.0;   // host wall time of the last ikf_load_weights (device work included) / of building these images
  std::vector<const float*> w_mid_frag;  // [subnet][layer], same flattening; null when the width does not fit

  // Row-owner form (flow_rowowner.hip): the whole inverse pass of a batch in ONE launch, a workgroup per 16 rows, weights streamed past
  // them from `ro_stream` (the subnets' parameters in execution and consumption order, +203 MB for Panda).  Taken for the full rounds of
  // n_cu x 16 rows of a batch and for a last partial round of at least ro_min_tail rows; the rest runs on the per-layer kernels.
  //   ro_mode: -1 by batch size, 0 never, 1 always (ikf_set_gemm_variant 180 / 181 / 182)
  DeviceBuf<float> ro_stream;
  DeviceBuf<RoSubnet> d_ro_sub;
  int ro_mode = -1, ro_nbuf = 4;
  int n_cu = 256;
  long long ro_min_tail = -1;  // -1: the last partial round goes to whatever plan_tail finds cheapest; >= 0 (probes): to the row-owner launch from that many rows on
  // Cluster form (k_flow_cluster<G>, flow_rowowner.hip) for what is left below a round: G = 8 / 4 / 2 workgroups per 16-row tile split the
  // hidden columns and exchange activations inside the launch (<= 512 / 1024 / 2048 rows).  Every cluster launch is followed by a
  // predicated row-owner launch of the same rows that runs only if a wait ran out (cl_abort set): results are valid either way, and the
  // handle stops using the form (cl_give_up).   cl_mode: -1 by batch size, 0 never, 1 whenever the grid fits (ikf_set_gemm_variant 185 / 186 / 187)
  int cl_mode = -1;
  long long cl_rows = 0;          // row capacity of the exchange buffers
  DeviceBuf<float> cl_xbuf;       // [tiles][16][1024]
  DeviceBuf<float> cl_sync;       // partial sums, epoch words, abort word (one memset per launch)
  // The drain-free hand-over (r05, flow_rowowner.hip TAG): every exchanged float carries its subnet's parity in the last mantissa bit, so a
  // producer neither drains its stores nor publishes an epoch and a consumer validates what it reads.  Taken for G = 2 .. 16 (- 3 .. 4.5 %
  // per call, and no memset in front of the launch; with 32 members the early re-reads of whole slices cost more than the epoch words).
  // Its buffers are its own: every float in them has parity 1 between calls (created as 0xff bytes; n_sub is even), which an epoch-word
  // launch's zeroing memset or untagged payload would break.  cl_tag_dirty: a tagged launch gave up - the buffers are re-created in front of
  // the next one (until then every tagged launch returns at once and its repair launch does the work: the abort word stays set).
  //   cl_tagged: 1 (default) / 0 (ikf_set_gemm_variant 193 / 192)
  int cl_tagged = 1;
  DeviceBuf<float> cl_xbuf_t;
  DeviceBuf<float> cl_sync_t;
  size_t cl_sync_t_bytes = 0;
  bool cl_tag_dirty = false;
  PinnedBuf<int> h_cl_give_up;    // pinned, device-visible
  int cl_drop_next = 0;           // tests: the next cluster launch runs one workgroup short (ikf_set_gemm_variant 188): its tile's waits run out
  ClusterBackoff cl_back;         // give-ups seen so far and the pause they cost (flow_plan.h; ikf_cluster_repairs / ikf_cluster_backoff)
  int cl_census_ok = -1;         // the placement census at load: workgroups b and b + 8 k share an XCD (1) or not (0); -1 not asked
  int cl_far_next = 0;            // tests (ikf_set_gemm_variant 191): the next XCD-local launch's workgroup 0 publishes a wrong XCC_ID
  unsigned cl_launch_seq = 0;     // tagged + XCD-local launches carry a 24-bit sequence number in their placement words (RcArgs::launch_seq)
  int cl_tl_nrt = 0, cl_tl_G = 0; // row tiles / members of the most recent tagged + XCD-local launch (whose placement words a give-up makes the host
                                  // read: cluster_tagged_xcc_words); 0 again when the buffers are released
  int cl_local = 1;               // G = 4 / 8 / 16: the form with a row tile's members on one XCD (hand-over through its L2); 0 after a member met a
                                  // peer on another XCD (placement is verified in the launch, never assumed) or by ikf_set_gemm_variant 189

  // packed weights (one arena)
  DeviceBuf<float> arena;
  size_t arena_floats = 0;
  std::vector<SubnetWeights> subnets;  // [2*block + (which-1)]
  DeviceBuf<int> d_perm_inv;           // [nb_nodes][D]
  DeviceBuf<float> d_Minv;             // [D][D]
  // forward (training-direction) pass, ikf_flow_forward
  DeviceBuf<float> d_M;                // [D][D] FixedLinearTransform forward matrix (module_list.0.M, or the fp64 inverse of M_inv)
  DeviceBuf<int> d_perm;               // [nb_nodes][D] PermuteRandom forward: perm[perm_inv[k]] = k
  float log_det_M = 0.f;               // logDetM = log|det M|, fp64 at load
  float log_det_Minv = 0.f;            // log|det M_inv| of the M_inv that is uploaded (ikf_flow_inverse), fp64 at load - not -log_det_M
  DeviceBuf<RoSubnet> d_ro_sub_fwd;    // the row-owner table in forward execution order (rowowner_fwd_table)
  DeviceBuf<float> d_blin;             // [D]
  DeviceBuf<Chain> d_chain;            // robot chain + limits
  DeviceBuf<CollisionModel> d_collision;  // capsules + pairs (ikf_set_collision_model), or null

  // scratch
  long long chunk_rows = 0;  // capacity of the per-chunk flow scratch
  DeviceBuf<float> xbuf;     // [chunk][D]
  DeviceBuf<float> xbuf2;    // [chunk][D]   second state buffer (fused path ping-pongs the state)
  DeviceBuf<float> pbuf;     // [slots][chunk][IKF_PSTRIDE] last-Linear partial sums (fused path)
  float* pbuf_alt = nullptr; // second set for odd subnets when a subnet has ONE hidden contraction (see ensure_scratch); else == pbuf
  DeviceBuf<float> hA;       // [chunk][width]
  DeviceBuf<float> hB;
  // exact-IK scratch
  long long exact_rows = 0, exact_poses = 0;
  long long exact_upfront_rows = 32LL << 20;  // ikf_set_exact_upfront_rows
  DeviceBuf<float> ex_q;          // [rows][ndof]
  DeviceBuf<uint8_t> ex_row_valid;  // [rows]
  DeviceBuf<unsigned> ex_pose_first;  // [poses] earliest valid iteration over a pose's repeats in the running round (early-exit hint)
  DeviceBuf<int> ex_pose_idx;     // [poses]
  DeviceBuf<int> ex_block_scratch;  // [2 * compact_blocks(poses)] per-block counts / offsets of the ordered compaction
  DeviceBuf<int> ex_count;        // device
  PinnedBuf<int> h_count;         // pinned host
  // exact collision rule (api_exact_world.hip): off by default; while on, a repeat whose candidate hits the world, the cloud or - reject_self -
  // the robot itself does not count
  int ex_rule_on = 0, ex_reject_self = 0;
  float ex_self_min_clearance = 0.f;
  DeviceBuf<float> ex_cloud_row;  // [rows] the round's rows' cloud clearances (sized with the row state while a cloud is set)
  DeviceBuf<unsigned long long> ex_rejected;  // [IKF_MAX_ROUNDS] rows with a candidate that a rule rejected, per round of the last call
  bool ex_rejected_live = false;  // the last exact call ran under the rule (else ikf_exact_collision_rejected reports zeros)
  // best-of-K ranking scratch (api_rank.hip): the flow's candidate rows and the K-chunks' partial lists
  int n_caps = 0;                 // capsules of d_collision (sizes the ranking kernel's LDS)
  DeviceBuf<float> rk_q;          // [rows][ndof]
  DeviceBuf<float> rk_part_score; // [lists][IKF_RANK_MAX_KEEP]   (the three part_* arrays are grown together, from one list count)
  DeviceBuf<int> rk_part_index;   // [lists][IKF_RANK_MAX_KEEP]
  DeviceBuf<int> rk_part_count;   // [lists]
  // path IK scratch (api_path.hip; the candidate rows are rk_q): node costs and back-pointers of the lattice, the shared latent expanded
  DeviceBuf<float> pt_node;       // [rows]
  DeviceBuf<uint8_t> pt_bp;       // [rows] a byte per node (+ padding: path_bp_bytes)
  DeviceBuf<float> pt_latent;     // [latent rows][D]
  // swept edges of path IK (api_sweep.hip, api_path.hip): samples per lattice edge (0: no sweep) and the sweep kernel's verdicts, a bit per edge
  int path_sweep = 0;
  DeviceBuf<uint64_t> pt_edge_free;  // [T][k][sweep_words(k)]
  // world track (api_track.hip, api_path.hip): key frames as they were set (normalised, f32), the fine table under track_S samples per edge on
  // the host and on the device, and the zero node costs ikf_sweep_lattice hands the sweep kernel.  track_F == 0: no track.
  int track_F = 0, track_n = 0, track_S = 0;
  float track_min_clearance = 0.f;
  std::vector<WorldObstacle> track_keys;   // [track_F][track_n]
  std::vector<WorldObstacle> track_fine;   // [track_fine_frames(track_F, track_S)][track_n]
  DeviceBuf<WorldObstacle> d_track;        // the same on the device
  DeviceBuf<float> tk_zero_node;           // [rows]
  // path optimiser (api_path_opt.hip, api_path.hip): steps behind every lattice (0: off) and their smooth_weight; the iterate, the previous iterate
  // and the per-waypoint fp64 scratch of k_path_opt; the k = 1 node scores and mask words of the input and of the optimised path, the ranking
  // kernel's kept rows (not used), the steps kept and the info words of the last optimising call
  int popt_iters = 0;
  float popt_weight = 0.f;
  DeviceBuf<float> po_q, po_prev, po_keep, po_node_in, po_node_opt;
  DeviceBuf<double> po_work;
  DeviceBuf<uint64_t> po_edge_in, po_edge_opt;
  DeviceBuf<int> po_iters, po_info;
  long long po_info_paths = 0;   // paths of the last optimising call (ikf_path_optimize_info)
  // refined candidates (api_refine.hip, api_rank.hip): LM steps on the flow's candidate rows before they are scored (0: none) and their tolerances
  int refine_steps = 0;
  float refine_pos_tol = 0.f, refine_rot_tol = 0.f;
  // diverse-of-K scratch (api_diverse.hip; the candidate rows are rk_q, the partial lists the ranking's): the row scores
  DeviceBuf<float> dv_score;      // [rows]
  // world collision (api_world.hip): the caller's obstacles; with world_n > 0 the ranking kernel also rejects rows closer than world_min_clearance
  DeviceBuf<WorldModel> d_world;  // allocated by the first ikf_set_world with obstacles
  int world_n = 0;
  float world_min_clearance = 0.f;
  // world point cloud (api_cloud.hip): the sensed scene; with cloud_n > 0 the candidate stage also rejects rows closer than cloud_min_clearance
  DeviceBuf<CloudPoint> d_cloud;  // [cloud_n rounded up to IKF_CLOUD_TILE] (x, y, z, 0), the padding copies of the last point
  long long cloud_n = 0;
  float cloud_radius = 0.f, cloud_min_clearance = 0.f;
  DeviceBuf<float> cloud_row;     // [rows] the candidate rows' GATE (score_candidates): their cloud clearances while a cloud is set, with -inf on the
                                  // rows under the manipulability floor; -inf / +inf with a floor and no cloud
  DeviceBuf<float> cloud_part;    // [chunks][rows] partial minima of a call whose plan has more than one chunk
  // singularity rule (api_manip.hip, api_rank.hip): with manip_min > 0 the candidate stage also rejects rows whose measure of manip_part is not >= it
  int manip_part = IKF_MANIP_FULL;
  float manip_min = 0.f;
  // f16x3 range guard
  DeviceBuf<int> d_split_flag;    // device word OR'ed by every kernel that produces a split operand out of the f16 range
  PinnedBuf<int> h_split_flag;    // pinned host
  int split_guard = 1;
  long long split_fallbacks = 0;

  // optional per-launch HIP-event timing of the dominant kernel (ikf_profile_begin/_end)
  bool prof_on = false;
  std::vector<hipEvent_t> prof_ev;  // pairs
  size_t prof_used = 0;
  double last_event_overhead_ms = 0.0;
};

// The inverse pass runs the coupling blocks last to first, s1 then s2 of each: the subnet at execution index sidx of 2 * NB
struct SubnetPos {
  int b, which, si;  // coupling block, 1 = s1 / 2 = s2, index into ikf_model::subnets
};
static inline SubnetPos subnet_at(int NB, int sidx) {
  const int b = NB - 1 - sidx / 2, which = 1 + (sidx & 1);
  return {b, which, 2 * b + which - 1};
}

static const int kArriveWords = 256; // >= row tiles of any launch that hands over inside the launch (<= 256 tiles)
static const size_t kProfMaxPairs = 8192;
static inline hipError_t prof_mark(ikf_model* m, hipStream_t s) {
  if (!m->prof_on || m->prof_used >= 2 * kProfMaxPairs) return hipSuccess;
  // the pool grows by whole pairs in front of a pair's FIRST record only: a hipEventCreate between a launch and its closing record
  // would delay that record on the host - behind a 3 ms launch the first creations were seen to add 0.3 ms to the measured pair
  if (m->prof_used >= m->prof_ev.size() && (m->prof_used & 1) == 0) {
    for (int i = 0; i < 64; ++i) {
      hipEvent_t e;
      hipError_t r = hipEventCreate(&e);
      if (r != hipSuccess) return r;
      m->prof_ev.push_back(e);
    }
  }
  if (m->prof_used >= m->prof_ev.size()) return hipErrorInvalidValue;
  return hipEventRecord(m->prof_ev[m->prof_used++], s);
}

static inline hipError_t stream_enter(ikf_model* m, hipStream_t s) {
  if (m->tail_valid && s != m->tail_stream) return hipStreamWaitEvent(s, m->tail_event, 0);
  return hipSuccess;
}
static inline hipError_t stream_leave(ikf_model* m, hipStream_t s) {
  if (!m->tail_event) {
    hipError_t e = hipEventCreateWithFlags(&m->tail_event, hipEventDisableTiming);
    if (e != hipSuccess) return e;
  }
  m->tail_stream = s;
  m->tail_valid = true;
  return hipEventRecord(m->tail_event, s);
}
// Records the handle's tail event behind whatever a call has enqueued, on EVERY exit path (an error return in the middle of
// a call leaves kernels in flight that still use the shared scratch; the next call on another stream must wait for them).
struct StreamScope {
  ikf_model* m;
  hipStream_t s;
  bool armed = false;
  StreamScope(ikf_model* m_, hipStream_t s_) : m(m_), s(s_) {}
  hipError_t enter() {
    hipError_t e = stream_enter(m, s);
    armed = (e == hipSuccess);
    return e;
  }
  hipError_t leave() {  // the success path: reports the record's own status
    armed = false;
    return stream_leave(m, s);
  }
  ~StreamScope() {
    if (armed) (void)stream_leave(m, s);
  }
  StreamScope(const StreamScope&) = delete;
  StreamScope& operator=(const StreamScope&) = delete;
};

// A sweep is set (ikf_set_path_sweep) and there is something to test against: obstacles on the handle, a world track (include/ikflow_amd_track.h),
// or the call rejects self-collisions.  (api_path.hip, api_path_opt.hip)
static inline bool path_sweeps(const ikf_model* m, const ikf_path_options* opt) {
  return m->path_sweep > 0 && (m->world_n > 0 || m->track_F > 0 || opt->reject_collisions);
}

static const long long kMaxChunkRows = 16384;  // keeps the [chunk x width] activations (64 MB each at width 1024) inside the 256 MB L3
// The kernels tile the hidden width in units of 256.  Any other coeff_fn_internal_size (ikflow/model.py:51-96 accepts any)
// is run at the next multiple of 256 with zero weights and biases in the padding: a padded unit outputs lrelu(0) = 0 and
// feeds 0 * 0 into every later sum, so the results are those of the unpadded network exactly.
static const int kWidthUnit = 256;
static const int kMaxWidth = 4096;

// What crosses a unit boundary (everything else is static in its unit), defined in api_handle / api_weights / api_flow / api_rank in this order;
// none of it is part of the library's ABI.
#pragma GCC visibility push(hidden)
namespace ikf {
ikf_status fail(ikf_status code, const std::string& msg);  // records the message that ikf_last_error returns
ikf_status ensure_scratch(ikf_model* m, long long rows);
ikf_status ensure_exact_rows(ikf_model* m, long long rows);
ikf_status ensure_exact(ikf_model* m, long long poses, long long rows);
ikf_status ensure_cluster_scratch(ikf_model* m, long long rows);
unsigned* cluster_tagged_abort_word(const ikf_model* m);   // where the tagged hand-over's words sit in cl_sync_t (null: no buffer)
unsigned* cluster_tagged_xcc_words(const ikf_model* m);
ikf_status build_split_weights(ikf_model* m);
ikf_status build_frag_weights(ikf_model* m);
ikf_status check_ready(ikf_model* m, const char* fn);
ikf_status run_flow_guarded(ikf_model* m, PoseSource ps, const float* d_latent, long long rows, int clamp_limits, float* d_q_out, hipStream_t s);
// The candidate stage of ranked / path / diverse IK (api_rank.hip): k candidates per pose, tile-major, scored by k_rank_candidates.
ikf_status ensure_rank_rows(ikf_model* m, long long rows);   // the candidate rows rk_q
// The checks the six entries share once the handle is there, in this order: options, count >= 0 (named `count`: "n_poses" / "T"), k in
// 1 .. k_max (0: no upper limit), the family's own rule (`rule_fault`: what to report, or null), k * count, reject_collisions without a
// collision model, then the empty call (*nothing_to_do) and, last, null device pointers (`have_pointers`: the family's required ones).
ikf_status check_candidates(const ikf_model* m, const std::string& who, const char* count, int64_t n, int k, int k_max, const void* opt,
                            bool reject_collisions, const char* rule_fault, bool have_pointers, bool* nothing_to_do);
// The flow on k tiled candidates per pose (latent [k * n][D]; the conditional of row r * n + j is pose j) into rk_q, which the caller has sized -
// and, while a refinement is set on the handle (ikf_set_candidate_refine), its LM steps on those rows, in place: whatever follows sees refined rows.
ikf_status flow_candidates(ikf_model* m, const float* d_poses, int64_t n, int k, const float* d_latent, int clamp_to_limits, hipStream_t s);
// The one place that fills a RankArgs and launches the ranking kernel: chunking, capsule slices, the handle's world, the partial lists.
ikf_status score_candidates(ikf_model* m, const float* d_poses, int64_t n, int k, const float* d_q, const float* d_q_ref,
                            const ikf_rank_options& opt, float* d_q_out, float* d_score_out, int32_t* d_index_out, int32_t* d_count_out,
                            float* d_row_score, hipStream_t s);
// Path and diverse score with the ranking's rule: n_keep = 1, no reference configuration, their six scoring fields as they are.
template <class Opt>
inline ikf_rank_options scoring_options(const Opt& o) {
  ikf_rank_options r{};
  r.n_keep = 1;
  r.rot_weight = o.rot_weight;
  r.max_pos_err = o.max_pos_err;
  r.max_rot_err = o.max_rot_err;
  r.reject_limits = o.reject_limits;
  r.reject_collisions = o.reject_collisions;
  r.min_clearance = o.min_clearance;
  return r;
}
// What ikf_reserve_ranked / _path / _diverse share: the argument test (`rule`: the family's message), candidate rows, partial lists and,
// with weights loaded, the flow's own reservation.
ikf_status reserve_candidates(ikf_model* m, const char* who, const char* rule, int64_t max_poses, int max_k, int k_max);
// The world point cloud (api_cloud.hip): the partial minima a call of `rows` rows needs under the cloud that is set (nothing without one), and the
// launch of k_cloud_clearance on the handle's cloud - both outputs nullable, the caller holds the stream scope.
ikf_status ensure_cloud_partials(ikf_model* m, long long rows);
ikf_status run_cloud_clearance(ikf_model* m, const float* d_q, long long rows, float* d_clearance, uint8_t* d_colliding, hipStream_t s);
// The exact collision rule (api_exact_world.hip).  exact_rule_begin: before a call enqueues anything - is there anything to test against
// (*active), and is the collision model there that it needs.  exact_rule_rows: the rule's own per-row buffer for `rows` rows while the rule is on and
// a cloud is set (ensure_exact_rows calls it).  exact_round_lm: a round's LM launch on the rows in ex_q - launch_exact_lm_iters as it was when !active,
// else the launches of the rule; either way ex_row_valid is what launch_exact_select_first reads next.
// The world track (api_track.hip).  track_rebuild: the fine table of the handle's key frames under S samples per edge, host and device
// (nothing without a track; ikf_set_path_sweep calls it BEFORE it takes S - a refused blend reports frame and obstacle and leaves the table as
// it was).  track_check_T: T <= F while a track is set.  track_mask_nodes: the node sink of k_track_clearance on a path call's node costs
// (nothing without a track).  track_fill_sweep: the track's fields of a lattice SweepArgs (nothing without a track).
// The path optimiser behind a lattice (api_path_opt.hip; called by api_path.hip while ikf_set_path_optimize is set).  path_opt_ensure: the scratch
// of P x T, before the stream scope.  path_opt_behind: optimise d_path in place with validate = 1 on the caller's stream, inside its scope; d_cost
// [P] is the lattice's cost on entry (+inf: the path is left alone) and the committed path's on exit.
ikf_status path_opt_ensure(ikf_model* m, long long P, long long T, const ikf_path_options* opt);
ikf_status path_opt_behind(ikf_model* m, const float* d_waypoints, long long P, long long T, const float* d_q_start, const ikf_path_options* opt,
                           float* d_path, float* d_cost, hipStream_t s);
ikf_status track_rebuild(ikf_model* m, const std::string& who, int S);
ikf_status track_check_T(const ikf_model* m, const std::string& who, int64_t T);
ikf_status track_mask_nodes(ikf_model* m, const float* d_q, int64_t T, int k, float* d_node, hipStream_t s);
void track_fill_sweep(const ikf_model* m, SweepArgs* a);
ikf_status exact_rule_begin(ikf_model* m, const std::string& who, bool* active);
ikf_status exact_rule_rows(ikf_model* m, long long rows);
ikf_status exact_round_lm(ikf_model* m, bool active, int round, const float* d_target_poses, int n_active, int repeat, int n_lm_steps,
                          const float* d_q_seed, float pos_thr, float rot_thr, hipStream_t s);
}  // namespace ikf
#pragma GCC visibility pop
