// C-ABI of libikflow_amd.so, the handle: ikf_last_error, ikf_create / ikf_destroy, the scratch allocators (ensure_*, ikf_reserve*) and
// every setting, getter and profiling hook that only reads or writes the handle.  See include/ikflow_amd.h for the contract.
#include "ikf_model.h"
#include <cassert>

static thread_local std::string g_last_error;

ikf_status ikf::fail(ikf_status code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

extern "C" const char* ikf_last_error(void) { return g_last_error.c_str(); }
extern "C" int ikf_abi_version(void) { return IKF_ABI_VERSION; }
extern "C" const char* ikf_dominant_kernel_name(void) { return fused_kernel_name(); }
extern "C" const char* ikf_split_kernel_name(void) { return split_kernel_name(); }

static void free_scratch(ikf_model* m) {
  m->xbuf.release();
  m->hA.release();
  m->hB.release();
  m->xbuf2.release();
  m->pbuf.release();
  m->pbuf_alt = nullptr;
  m->chunk_rows = 0;
  m->chain_tab_valid = false;  // (the table holds these pointers)
}

extern "C" ikf_status ikf_create(const ikf_model_desc* desc, int device, ikf_model** out) {
  if (!desc || !out) return fail(IKF_ERR_NULL_POINTER, "ikf_create: null argument");
  *out = nullptr;
  if (desc->abi_version != IKF_ABI_VERSION)
    return fail(IKF_ERR_BAD_ARGUMENT, "ikf_create: ABI version mismatch (header " + std::to_string(IKF_ABI_VERSION) +
                                          ", caller " + std::to_string(desc->abi_version) + ")");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(IKF_ERR_NO_DEVICE, "ikf_create: no HIP device visible (this engine has no CPU path)");
  if (device < 0 || device >= ndev) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_create: device index out of range");
  const int D = desc->dim;
  if (desc->nb_nodes < 1 || D < 2 || D > IKF_MAX_DIM) return fail(IKF_ERR_BAD_SHAPE, "ikf_create: nb_nodes/dim out of range (2 <= D <= 16)");
  if (desc->dim_cond != 7 && desc->dim_cond != 8) return fail(IKF_ERR_BAD_SHAPE, "ikf_create: dim_cond must be 7 or 8");
  if (desc->sigmoid_on_output && desc->dim_cond != 7)
    return fail(IKF_ERR_BAD_ARGUMENT, "sigmoid_on_output and softflow are incompatible, disable one or the other");
  if (desc->n_hidden < 1 || desc->n_hidden > 4) return fail(IKF_ERR_BAD_SHAPE, "ikf_create: Number of layers `n_layers` must be in [1, ..., 4]");
  if (desc->width < 1 || desc->width > kMaxWidth)
    return fail(IKF_ERR_BAD_SHAPE, "ikf_create: coeff_fn_internal_size must be in [1, 4096]");
  if (desc->ndof < 4 || desc->ndof > IKF_MAX_DOF || desc->ndof > D)
    return fail(IKF_ERR_BAD_SHAPE, "ikf_create: ndof must be in [4, 8] and <= dim");
  DeviceGuard dev_guard_(device);
  if (dev_guard_.err != hipSuccess) return fail(IKF_ERR_HIP, std::string("hipSetDevice failed: ") + hipGetErrorString(dev_guard_.err));

  ikf_model* m = new ikf_model();
  m->device = device;
  {
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && n_cu > 0) m->n_cu = n_cu;
  }
  m->desc = *desc;
  m->dims.D = D;
  m->dims.L1 = D / 2;  // ikflow/model.py:336 (old FrEIA rule)
  m->dims.L2 = D - D / 2;
  m->dims.width = (desc->width + kWidthUnit - 1) / kWidthUnit * kWidthUnit;
  m->dims.n_hidden = desc->n_hidden;
  m->dims.ndof = desc->ndof;
  m->dims.n_pose = 7;
  m->dims.clamp = desc->clamp;
  m->dims.slope = desc->leaky_slope;

  Chain ch{};
  ch.ndof = desc->ndof;
  for (int j = 0; j < desc->ndof; ++j) {
    ch.joints[j] = desc->chain[j];
    ch.lo[j] = desc->joint_lo[j];
    ch.hi[j] = desc->joint_hi[j];
    if (ch.joints[j].kind != 1 && ch.joints[j].kind != 2) {
      delete m;
      return fail(IKF_ERR_BAD_ARGUMENT, "ikf_create: chain joint kind must be 1 (revolute) or 2 (prismatic)");
    }
  }
  memcpy(ch.tool, desc->tool, sizeof(ch.tool));
  hipError_t e = m->d_chain.ensure(1);
  if (e == hipSuccess) e = hipMemcpy(m->d_chain, &ch, sizeof(Chain), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = m->ex_count.ensure(1);
  if (e == hipSuccess) e = m->h_count.alloc(1);
  if (e == hipSuccess) e = m->d_split_flag.ensure(1);
  if (e == hipSuccess) e = hipMemset(m->d_split_flag, 0, sizeof(int));
  if (e == hipSuccess) e = m->h_split_flag.alloc(1);
  if (e == hipSuccess) e = m->d_arrive.ensure(kArriveWords);
  if (e == hipSuccess) e = hipMemset(m->d_arrive, 0, sizeof(unsigned) * kArriveWords);
  if (e == hipSuccess) e = m->h_give_up.alloc(1, hipHostMallocMapped);
  if (e == hipSuccess) *m->h_give_up = 0;
  if (e == hipSuccess) e = m->h_cl_give_up.alloc(1, hipHostMallocMapped);
  if (e == hipSuccess) *m->h_cl_give_up = 0;
  if (e == hipSuccess) e = m->d_chain_ctl.ensure(IKF_CHAIN_CTL_WORDS);
  if (e == hipSuccess) e = hipMemset(m->d_chain_ctl, 0, sizeof(unsigned) * IKF_CHAIN_CTL_WORDS);
  if (e == hipSuccess) e = m->d_chain_tab.ensure(2 * (long long)desc->nb_nodes);
  if (e != hipSuccess) {
    ikf_destroy(m);
    return fail(IKF_ERR_HIP, std::string("ikf_create: allocation failed: ") + hipGetErrorString(e));
  }
  *out = m;
  return IKF_OK;
}

extern "C" void ikf_destroy(ikf_model* m) {
  if (!m) return;
  DeviceGuard dev_guard_(m->device);
  for (hipEvent_t e : m->prof_ev) (void)hipEventDestroy(e);
  if (m->tail_event) (void)hipEventDestroy(m->tail_event);
  delete m;  // (every buffer is a DeviceBuf / PinnedBuf member: freed here, on the handle's device)
}

extern "C" int ikf_weights_loaded(const ikf_model* m) { return (m && m->loaded) ? 1 : 0; }

// ---------------------------------------------------------------------------------------------------------------
// scratch
// ---------------------------------------------------------------------------------------------------------------
static long long chunk_cap(const ikf_model* m) {  // rows per chunk: 16384 up to width 1024, fewer for wider subnets
  const long long w = m->dims.width > 1024 ? m->dims.width : 1024;
  return kMaxChunkRows * 1024 / w / 128 * 128;
}

ikf_status ikf::ensure_scratch(ikf_model* m, long long rows) {
  const long long cap = chunk_cap(m);
  long long want = rows < cap ? rows : cap;
  want = (want + 127) / 128 * 128;  // the contraction kernels store whole 128-row tiles (no row predicate)
  if (want <= m->chunk_rows) return IKF_OK;
  free_scratch(m);
  IKF_HIP(m->xbuf.ensure(want * m->dims.D));
  IKF_HIP(m->hA.ensure(want * m->dims.width));
  IKF_HIP(m->hB.ensure(want * m->dims.width));
  IKF_HIP(m->xbuf2.ensure(want * m->dims.D));
  const size_t slots = (size_t)(fused_max_slots(m->dims.width) > 0 ? fused_max_slots(m->dims.width) : 1);
  // With ONE hidden contraction per subnet (coeff_fn_config 2, e.g. TINY_MODEL_PARAMS) the one-launch subnet head (k_entry_gemm_skinny*) is
  // also the subnet's LAST contraction: the same launch reads the previous subnet's partial sums (pending coupling, every slot of its row
  // tile) and writes its own.  In one buffer that is a write-after-read hazard between the workgroups of a row tile - harmless only while all
  // of them start together; when another process holds CUs a late workgroup read slots a finished sibling had already overwritten (r06: the
  // red two-ranks-on-one-GPU test of round 5, tools/two_tenant_determinism.py).  Such shapes alternate between two sets by subnet parity.
  const size_t pset = slots * (size_t)want * IKF_PSTRIDE;
  const bool two_sets = m->dims.n_hidden == 2;
  IKF_HIP(m->pbuf.ensure((long long)(pset * (two_sets ? 2 : 1))));
  m->pbuf_alt = two_sets ? m->pbuf + pset : m->pbuf;
  m->chunk_rows = want;
  return IKF_OK;
}

// exact-IK state: per-pose buffers (active list, solved flags, compaction scratch) and per-row buffers (q, row validity) grow
// independently - the row buffers carry nothing from one retry round to the next, so they may be regrown between rounds
// (right after the round's count has been read, i.e. with the stream idle) without touching the active-pose list.
static ikf_status ensure_exact_poses(ikf_model* m, long long poses) {
  if (poses <= m->exact_poses) return IKF_OK;
  m->ex_pose_idx.release();
  m->ex_block_scratch.release();
  m->ex_pose_first.release();
  m->exact_poses = 0;
  IKF_HIP(m->ex_pose_idx.ensure(poses));
  IKF_HIP(m->ex_pose_first.ensure(poses));
  IKF_HIP(m->ex_block_scratch.ensure(2 * (long long)(compact_blocks(poses) + 1)));
  m->exact_poses = poses;
  return IKF_OK;
}
ikf_status ikf::ensure_exact_rows(ikf_model* m, long long rows) {
  if (rows <= m->exact_rows) return exact_rule_rows(m, m->exact_rows);   // (nothing, unless the rule or a cloud was set since the rows were sized)
  m->ex_q.release();
  m->ex_row_valid.release();
  m->exact_rows = 0;
  IKF_HIP(m->ex_q.ensure(rows * m->dims.ndof));
  IKF_HIP(m->ex_row_valid.ensure(rows));
  m->exact_rows = rows;
  return exact_rule_rows(m, rows);   // (the exact collision rule's cloud clearances, while a cloud is set: api_exact_world.hip)
}
ikf_status ikf::ensure_exact(ikf_model* m, long long poses, long long rows) {
  ikf_status st = ensure_exact_poses(m, poses);
  return st != IKF_OK ? st : ensure_exact_rows(m, rows);
}
// Worst-case row state (every pose unsolved in the round with the largest repeat count) is reserved up front only while it is
// small (ikf_set_exact_upfront_rows, default 32 Mi rows); beyond that a call starts with round 0's rows and grows per round from the measured survivor count, so a
// large n with a big last-round repeat but few survivors neither allocates nor is rejected for the worst case.
extern "C" ikf_status ikf_reserve_exact(ikf_model* m, int64_t max_poses, int max_repeat) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_reserve_exact: null model");
  if (max_poses < 1 || max_repeat < 1 || max_poses * (long long)max_repeat > 0x7fffffffLL)
    return fail(IKF_ERR_BAD_ARGUMENT, "ikf_reserve_exact: max_poses and max_repeat must be positive (product < 2^31)");
  IKF_ON_DEVICE(m)
  return ensure_exact(m, max_poses, max_poses * (long long)max_repeat);
}

ikf_status ikf::ensure_cluster_scratch(ikf_model* m, long long rows) {
  if (rows <= m->cl_rows) return IKF_OK;
  m->cl_xbuf.release();
  m->cl_sync.release();
  m->cl_xbuf_t.release();
  m->cl_sync_t.release();
  m->cl_rows = 0;
  m->cl_tl_nrt = m->cl_tl_G = 0;   // (the placement words of the last tagged + XCD-local launch went with cl_sync_t: a give-up folded from here on reads nothing)
  const long long cap = (long long)m->n_cu / 2 * IKF_RO_ROWS;   // the largest chunk the form takes (G = 2)
  const int tiles = (int)((cap + IKF_RO_ROWS - 1) / IKF_RO_ROWS);
  const size_t sync_bytes = cluster_sync_bytes(tiles, 8);   // (sized for G = 8 on every tile: 4.6 KB per tile)
  assert(sync_bytes % sizeof(float) == 0);   // (cl_sync / cl_sync_t are float arrays sized in bytes: whole words by construction)
  IKF_HIP(m->cl_xbuf.ensure((long long)cluster_xbuf_floats(tiles)));
  IKF_HIP(m->cl_sync.ensure((long long)(sync_bytes / sizeof(float))));
  // the tagged hand-over's own pair (same sizes; its abort word is the block's LAST word, wherever a launch's partial sums end)
  m->cl_sync_t_bytes = sync_bytes;
  IKF_HIP(m->cl_xbuf_t.ensure((long long)cluster_xbuf_floats(tiles)));
  IKF_HIP(m->cl_sync_t.ensure((long long)(sync_bytes / sizeof(float))));
  m->cl_tag_dirty = true;   // (created by the first launch that uses them, on its stream)
  m->cl_rows = cap;
  return IKF_OK;
}
// The tagged buffers' abort word: the last 128-byte line of cl_sync_t (what is in front of it is created as parity-1 floats).
unsigned* ikf::cluster_tagged_abort_word(const ikf_model* m) {
  if (m->cl_sync_t.p == nullptr) return nullptr;
  return reinterpret_cast<unsigned*>(reinterpret_cast<char*>(m->cl_sync_t.p) + m->cl_sync_t_bytes - 128);
}
// The members' placement words [row tile][32]: behind the partial sums of the largest launch (the epoch-word form's flag area, unused here).
unsigned* ikf::cluster_tagged_xcc_words(const ikf_model* m) {
  if (m->cl_sync_t.p == nullptr) return nullptr;
  return reinterpret_cast<unsigned*>(m->cl_sync_t.p) + (size_t)(m->cl_rows / IKF_RO_ROWS) * 8 * 256;
}

extern "C" ikf_status ikf_reserve(ikf_model* m, int64_t max_rows) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_reserve: null model");
  if (max_rows < 1) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_reserve: max_rows must be positive");
  IKF_ON_DEVICE(m)
  ikf_status st = ensure_scratch(m, max_rows);
  // the small-batch per-layer kernels' weight image (201 MB at the released shape): also on a handle whose small batches normally take the
  // cluster form - during a back-off pause (another process held CUs) they run these kernels, and that is the worst moment for a hipMalloc,
  // 48 pack launches and a device-wide synchronisation inside a call
  if (st == IKF_OK && m->loaded && !m->wfrag_built) st = build_frag_weights(m);
  return st;
}

extern "C" int ikf_probes_build(void) {
#ifdef IKF_PROBES
  return 1;
#else
  return 0;
#endif
}

extern "C" ikf_status ikf_set_gemm_variant(ikf_model* m, int variant) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_set_gemm_variant: null model");
#ifndef IKF_PROBES
  if (variant == 121 || variant == 163 || variant == 164 || variant == 171 || variant == 106 || variant == 108)
    return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_gemm_variant(" + std::to_string(variant) + "): a priced-and-rejected form of rounds 2 - 3 (in-launch entry phase, "
                "one-launch chain for <= 128 rows, tile configurations 5 / 7 / 11) - compiled only into the probes library "
                "(ikflow_amd/lib/libikflow_amd_probes.so, python -m ikflow_amd.build --probes)");
#endif
  if (variant >= 110 && variant <= 112) {  // small-batch one-launch form (entry + first contraction): off / auto / forced
    m->fuse_entry = variant - 110;
    return IKF_OK;
  }
  if (variant == 152 || variant == 153) {  // 16-row kernels: whole operand stream up front off / on
    m->tune = variant == 153 ? (m->tune | IKF_TUNE_DEEP16) : (m->tune & ~IKF_TUNE_DEEP16);
    return IKF_OK;
  }
  if (variant == 150 || variant == 151) {  // <= 128 rows on 16x32 tiles (v_mfma_f32_16x16x4_f32): off / on
    m->tune = variant == 151 ? (m->tune | IKF_TUNE_ROWS16) : (m->tune & ~IKF_TUNE_ROWS16);
    return IKF_OK;
  }
  if (variant >= 130 && variant <= 134) {  // write-through activation stores: none / contractions / entry kernel / both / by batch size
    m->wt_stores = variant == 134 ? -1 : variant - 130;
    return IKF_OK;
  }
  if (variant == 192 || variant == 193) {  // cluster form, G = 2 .. 16: hand-over by epoch words / by parity-tagged payload (default)
    m->cl_tagged = variant - 192;
    return IKF_OK;
  }
  if (variant == 191) {  // tests of the placement check: the next XCD-local cluster launch is told that workgroup 0 sits on another XCD
    m->cl_far_next = 1;
    return IKF_OK;
  }
  if (variant == 189 || variant == 190) {  // cluster form, G = 4 / 8 / 16: a row tile's members spread over the XCDs / on one XCD (default)
    if (variant == 190 && m->cl_census_ok == 0)
      return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_gemm_variant(190): on this device workgroups b and b + 8 k of a grid do not share an XCD");
    m->cl_local = variant - 189;
    return IKF_OK;
  }
  if (variant == 188) {  // tests of the repair path: the next cluster launch is one workgroup short
    m->cl_drop_next = 1;
    return IKF_OK;
  }
  if (variant >= 185 && variant <= 187) {  // cluster form for the rows below a round: never / by batch size / whenever the grid fits
    m->cl_mode = variant == 185 ? 0 : (variant == 186 ? -1 : 1);
    return IKF_OK;
  }
  if (variant >= 180 && variant <= 182) {  // row-owner form (one launch per call, rows resident on chip): never / by batch size / always
    if (variant == 182 && m->loaded && m->ro_stream == nullptr)
      return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_gemm_variant(182): the row-owner kernel needs coeff_fn_internal_size 1024 and coeff_fn_config 3");
    m->ro_mode = variant == 180 ? 0 : (variant == 181 ? -1 : 1);
    return IKF_OK;
  }
  if (variant == 170 || variant == 171) {  // <= 128 rows: the whole subnet chain in one launch (XCD-local hand-over): off / on
    m->chain_mode = variant - 170;
    return IKF_OK;
  }
  if (variant == 120 || variant == 121) {  // next subnet's entry phase in the tail of the last hidden contraction: off / on
    m->fuse_tail = variant - 120;
    return IKF_OK;
  }
  if (variant == 162 || variant == 163) {  // 129 .. 256 rows on 32x32 tiles built from 16x16x4 MFMAs: off (default) / on
    m->tune = variant == 163 ? (m->tune | IKF_TUNE_ROWS32_V2) : (m->tune & ~IKF_TUNE_ROWS32_V2);
    return IKF_OK;
  }
  if (variant == 164) {  // ... forced (tile config 11)
    m->gemm_variant = 100;
    m->tile_cfg = 11;
    return IKF_OK;
  }
  if (variant == 160 || variant == 161) {  // fused pipeline with the 16x32 / 16x16 small-batch tiles forced (tile config 9 / 10)
    m->gemm_variant = 100;
    m->tile_cfg = variant - 151;
    return IKF_OK;
  }
  if (variant == 158 || variant == 159) {  // <= 64 rows on 16x16 tiles: off / on
    m->tune = variant == 159 ? (m->tune | IKF_TUNE_TILES16) : (m->tune & ~IKF_TUNE_TILES16);
    return IKF_OK;
  }
  if (variant >= 100 && variant <= 108) {  // fused pipeline; 100 = tile by batch size, 101..108 = tile config 0..7
    m->gemm_variant = 100;
    m->tile_cfg = variant - 101;
    return IKF_OK;
  }
  if (variant < -1 || variant >= gemm_variant_count())
    return fail(IKF_ERR_BAD_ARGUMENT, "unknown gemm variant (-1 auto, 0..N-1 unfused tile shapes, 100 fused by batch size, 101..108 fused with tile configuration 0..7, 110 / 111 / 112 one-launch small-batch form off / auto / forced, 120 / 121 in-launch entry phase off / on, 130..134 write-through activation stores none / contractions / entry / both / by batch size, 150 / 151 16-row tiles for <= 128 rows off / on, 152 / 153 their whole-stream prefetch off / on, 158 / 159 16 x 16 tiles for <= 64 rows off / on, 160 / 161 / 164 small-batch tile configurations 9 / 10 / 11 forced, 162 / 163 configuration 11 for 129..256 rows off / on, 170 / 171 one-launch subnet chain for <= 128 rows off / on, 180 / 181 / 182 row-owner launch never / by plan / always, 185 / 186 / 187 cluster form never / by plan / whenever the grid fits, 188 / 191 tests of its repair paths, 189 / 190 its members spread / on one XCD, 192 / 193 its hand-over by epoch words / tagged payload; see include/ikflow_amd_debug.h)");
  m->gemm_variant = variant;
  m->tile_cfg = -1;
  return IKF_OK;
}

extern "C" ikf_status ikf_profile_begin(ikf_model* m) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_profile_begin: null model");
  m->prof_on = true;
  m->prof_used = 0;
  return IKF_OK;
}

extern "C" ikf_status ikf_profile_end(ikf_model* m, int64_t* n_launches, double* total_ms, void* stream) {
  if (!m || !n_launches || !total_ms) return fail(IKF_ERR_NULL_POINTER, "ikf_profile_end: null argument");
  IKF_ON_DEVICE(m)
  hipStream_t s = static_cast<hipStream_t>(stream);
  m->prof_on = false;
  // calibrate what an (otherwise empty) event pair measures on this stream and take it off every bracketed launch
  const int ncal = 32;
  hipEvent_t cal[2 * ncal];
  for (int i = 0; i < 2 * ncal; ++i) IKF_HIP(hipEventCreate(&cal[i]));
  for (int i = 0; i < ncal; ++i) {
    IKF_HIP(hipEventRecord(cal[2 * i], s));
    IKF_HIP(hipEventRecord(cal[2 * i + 1], s));
  }
  IKF_HIP(hipStreamSynchronize(s));
  double empty = 0.0;
  for (int i = 0; i < ncal; ++i) {
    float ms = 0.f;
    IKF_HIP(hipEventElapsedTime(&ms, cal[2 * i], cal[2 * i + 1]));
    empty += ms;
  }
  empty /= ncal;
  for (int i = 0; i < 2 * ncal; ++i) (void)hipEventDestroy(cal[i]);
  double tot = 0.0;
  const size_t pairs = m->prof_used / 2;
  for (size_t i = 0; i < pairs; ++i) {
    float ms = 0.f;
    IKF_HIP(hipEventElapsedTime(&ms, m->prof_ev[2 * i], m->prof_ev[2 * i + 1]));
    tot += (ms > empty ? ms - empty : 0.0);
  }
  *n_launches = (int64_t)pairs;
  *total_ms = tot;
  m->prof_used = 0;
  m->last_event_overhead_ms = empty;
  return IKF_OK;
}
extern "C" double ikf_profile_event_overhead_ms(const ikf_model* m) { return m ? m->last_event_overhead_ms : 0.0; }

extern "C" ikf_status ikf_set_precision(ikf_model* m, int mode) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_set_precision: null model");
  if (mode != 0 && mode != 1) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_precision: mode must be 0 (f32 MFMA) or 1 (3x f16 split)");
  if (mode == 1 && (m->dims.n_hidden < 2 || m->dims.width % 128 != 0))
    return fail(IKF_ERR_BAD_SHAPE, "ikf_set_precision: the f16-split contraction needs a width that is a multiple of 128 and >= 2 hidden layers");
  m->precision = mode;
  if (mode == 1) {
    IKF_ON_DEVICE(m)
    return build_split_weights(m);
  }
  return IKF_OK;
}
extern "C" int ikf_get_precision(const ikf_model* m) { return m ? m->precision : -1; }
extern "C" ikf_status ikf_set_lm_precision(ikf_model* m, int mode) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_set_lm_precision: null model");
  if (mode != 0 && mode != 1) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_lm_precision: mode must be 0 (fp32, the reference's arithmetic) or 1 (fp64 inside the step)");
  m->lm_precision = mode;
  return IKF_OK;
}
extern "C" int ikf_get_lm_precision(const ikf_model* m) { return m ? m->lm_precision : -1; }

extern "C" ikf_status ikf_set_split_guard(ikf_model* m, int guard) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_set_split_guard: null model");
  if (guard != 0 && guard != 1) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_split_guard: guard must be 0 or 1");
  m->split_guard = guard;
  return IKF_OK;
}
extern "C" int64_t ikf_split_fallback_count(const ikf_model* m) { return m ? (int64_t)m->split_fallbacks : 0; }
