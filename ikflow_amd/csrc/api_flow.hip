// C-ABI of libikflow_amd.so, the flow (what replaces IKFlowSolver._run_inference, ikflow/ikflow_solver.py:85-110): the planner (flow_plan.h) applied to a handle, the host
// side of every flow launch sequence, the entries ikf_generate_approx / ikf_flow_forward / ikf_flow_inverse.  See include/ikflow_amd.h for the contract.
#include "ikf_model.h"

static int pick_variant(const ikf_model* m, long long rows) {
  if (m->gemm_variant >= 0) return m->gemm_variant;
  const int W = m->dims.width;
  // fill the 256 CUs: 128x128 tiles when that already gives >= 256 tiles, smaller tiles for smaller batches
  const long long t128 = ((rows + 127) / 128) * (W / 128);
  if (t128 >= 256) return 0;
  const long long t12864 = ((rows + 127) / 128) * (W / 64);
  if (t12864 >= 256) return 2;
  return 4;
}

// ---------------------------------------------------------------------------------------------------------------
// flow inverse pass over `rows` rows (chunked); replaces nn_model(latent, c=cond, rev=True) + slice + clamp
// ---------------------------------------------------------------------------------------------------------------
static const float* chain_lo(const ikf_model* m) {
  return reinterpret_cast<const float*>(reinterpret_cast<const char*>(m->d_chain.p) + offsetof(Chain, lo));
}
static const float* chain_hi(const ikf_model* m) {
  return reinterpret_cast<const float*>(reinterpret_cast<const char*>(m->d_chain.p) + offsetof(Chain, hi));
}

// fn(r0, nr) for consecutive pieces of at most `piece` rows of [r_base, r_base + rows); stops at the first status that is not IKF_OK
template <class Fn> static ikf_status for_each_piece(long long r_base, long long rows, long long piece, Fn fn) {
  ikf_status st = IKF_OK;
  for (long long r0 = r_base, end = r_base + rows; st == IKF_OK && r0 < end; r0 += piece) st = fn(r0, end - r0 < piece ? end - r0 : piece);
  return st;
}
// the per-layer kernels work through the handle's scratch: sized once for the rows at hand, then one chunk of it at a time
template <class Fn> static ikf_status for_each_chunk(ikf_model* m, long long r_base, long long rows, Fn fn) {
  const ikf_status st = ensure_scratch(m, rows);
  return st != IKF_OK ? st : for_each_piece(r_base, rows, m->chunk_rows, fn);
}
static const long long kMaxLaunchRows = 1LL << 24;  // rows of one row-owner launch

// the small-batch tile configurations take their W fragments straight from the fragment-major image (narrow models pick them for
// larger batches too: the choice goes by tile count, not by rows)
static bool cfg_reads_frag_image(int cfg) {
  return cfg == fused_skinny_cfg() || cfg == fused_skinny32_cfg() || cfg == fused_skinny16_cfg() || cfg == fused_skinny16x16_cfg() ||
         cfg == fused_skinny32v2_cfg();
}
// fragment-major image of hidden layer l of subnet si, or null (not built for this width / not loaded)
static const float* frag_image(const ikf_model* m, int si, int l) {
  const size_t i = (size_t)si * 3 + l;
  return i < m->w_mid_frag.size() ? m->w_mid_frag[i] : nullptr;
}

static bool fused_ok(const ikf_model* m) {
  const FlowDims& d = m->dims;
  if (m->gemm_variant >= 0 && m->gemm_variant != 100) return false;
  return d.n_hidden >= 2 && fused_pick_cfg(128, d.width) >= 0 && d.D <= 16 && 2 * d.L2 <= 16 &&
         d.L1 + d.n_pose >= 8 && d.L2 + d.n_pose <= 15;
}

// three kernels per subnet (flow_fused.hip): entry (pending coupling + first Linear), hidden contraction(s), the last
// of which reduces the last Linear to partial sums; one finalize kernel after the last subnet
// ---- <= 128 rows: the subnet chain in one launch (k_flow_chain16) + the finalize kernel
// One-time check per handle that a chain-shaped launch gets 32 workgroups on each of 8 XCDs (the kernel would notice and give up;
// this keeps a device in another partition mode, or with masked CUs, from ever trying).  Synchronous: first use only.
static ikf_status chain_census(ikf_model* m, hipStream_t s) {
  if (m->chain_census >= 0) return IKF_OK;
  m->chain_census = 0;
  hipDeviceProp_t prop{};
  IKF_HIP(hipGetDeviceProperties(&prop, m->device));
  if (prop.multiProcessorCount != IKF_CHAIN_XCDS * IKF_CHAIN_PER_XCD) return IKF_OK;
  DeviceBuf<unsigned> d_out;
  IKF_HIP(d_out.ensure(256));
  hipError_t e = launch_xcd_census(d_out, s);
  unsigned h[256];
  if (e == hipSuccess) e = hipMemcpyAsync(h, d_out, sizeof(h), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  IKF_HIP(e);
  int per[16] = {};
  for (int b = 0; b < 256; ++b) per[h[b] & 15]++;
  bool ok = true;
  for (int x = 0; x < 16; ++x) ok = ok && per[x] == (x < IKF_CHAIN_XCDS ? IKF_CHAIN_PER_XCD : 0);
  m->chain_census = ok ? 1 : 0;
  return IKF_OK;
}
static bool chain_usable(const ikf_model* m, long long nr) {
  const FlowDims& d = m->dims;
  if (m->chain_mode == 0 || m->chain_census == 0 || m->tile_cfg >= 0 || m->fuse_entry != 1 || m->fuse_tail != 0 || m->prof_on) return false;
  if ((m->tune & (IKF_TUNE_ROWS16 | IKF_TUNE_DEEP16)) != (IKF_TUNE_ROWS16 | IKF_TUNE_DEEP16)) return false;
  if (!flow_chain16_ok(nr, d.width, d.D, 2 * (d.L1 > d.L2 ? d.L1 : d.L2), d.n_hidden)) return false;
  for (int si = 0; si < 2 * m->desc.nb_nodes; ++si)
    if (m->subnets[si].n_x + d.n_pose > 15) return false;
  return true;
}
// The pending coupling a subnet leaves behind (its last Linear exists only as partial sums: `slots` sets of them in P)
static PendingCoupling pending_of(const ikf_model* m, const SubnetPos& p, const float* P, int slots) {
  const SubnetWeights& w = m->subnets[p.si];
  PendingCoupling pc{};
  pc.P = P;
  pc.b_last = w.b_last;
  pc.perm_inv = m->d_perm_inv + (size_t)p.b * m->dims.D;
  pc.slot_stride = m->chunk_rows * IKF_PSTRIDE;
  pc.slots = slots;
  pc.which = p.which;
  pc.n_out = w.n_out;
  return pc;
}
// What the entry phase of the subnet at execution index sidx is given whatever the call: weights, widths, offsets, h_out, x_dst
static void entry_fixed(const ikf_model* m, int sidx, EntryArgs& e) {
  const FlowDims& d = m->dims;
  const SubnetPos p = subnet_at(m->desc.nb_nodes, sidx);
  const SubnetWeights& w = m->subnets[p.si];
  e.x_dst = (sidx & 1) ? m->xbuf2 : m->xbuf;
  e.D = d.D; e.L1 = d.L1; e.clamp = d.clamp;
  e.x_off = (p.which == 1) ? 0 : d.L1; e.n_x = w.n_x;
  e.w1t = w.w_first_t; e.w1soft = w.w_soft; e.b1 = w.b_first;
  e.width = d.width; e.slope = d.slope; e.h_out = m->hA;
}
// the finalize kernel behind the last subnet of a chunk: its pending coupling, the linear transform, the limits
static FinalizeArgs finalize_args(const ikf_model* m, const PendingCoupling& pend, const float* x_src, long long r0, long long nr, int clamp_limits,
                                  float* d_q_out) {
  const FlowDims& d = m->dims;
  FinalizeArgs f{};
  f.pend = pend; f.x_src = x_src; f.M = (int)nr; f.D = d.D; f.L1 = d.L1; f.ndof = d.ndof; f.clamp = d.clamp;
  f.M_inv = m->d_Minv; f.b_lin = m->d_blin; f.lo = chain_lo(m); f.hi = chain_hi(m);
  f.clamp_limits = clamp_limits; f.sigmoid = m->desc.sigmoid_on_output ? 1 : 0; f.q_out = d_q_out + (size_t)r0 * d.ndof;
  return f;
}
static ikf_status chain_table(ikf_model* m) {
  if (m->chain_tab_valid) return IKF_OK;
  const FlowDims& d = m->dims;
  const int NB = m->desc.nb_nodes;
  std::vector<ChainSubnet> tab((size_t)2 * NB);
  PendingCoupling pend{};
  const float* x_src = nullptr;
  for (int sidx = 0; sidx < 2 * NB; ++sidx) {
    const SubnetPos p = subnet_at(NB, sidx);
    const SubnetWeights& w = m->subnets[p.si];
    if (frag_image(m, p.si, 0) == nullptr || frag_image(m, p.si, 1) == nullptr) return fail(IKF_ERR_HIP, "chain_table: no fragment image");
    ChainSubnet& c = tab[sidx];
    memset(&c, 0, sizeof(c));
    EntryArgs& e = c.e;
    entry_fixed(m, sidx, e);
    e.pend = pend;
    e.x_src = x_src;
    c.n_in = w.n_x + d.n_pose;
    for (int l = 0; l < 2; ++l) {
      FusedGemmArgs& g = c.g[l];
      g.N = d.width; g.K = d.width; g.slope = d.slope; g.tune = m->tune;
      g.w_last = w.w_last; g.n_out = w.n_out; g.P_out = m->pbuf; g.p_slot_stride = m->chunk_rows * IKF_PSTRIDE;
      g.W = w.w_mid[l]; g.bias = w.b_mid[l]; g.Wf = frag_image(m, p.si, l);
    }
    c.g[0].A = m->hA; c.g[0].C = m->hB;   // (the head keeps the first Linear's output in registers: A is unused)
    c.g[1].A = m->hB; c.g[1].C = nullptr;
    pend = pending_of(m, p, m->pbuf, fused_slots(fused_skinny16_cfg(), d.width));
    x_src = e.x_dst;
  }
  IKF_HIP(hipMemcpy(m->d_chain_tab, tab.data(), sizeof(ChainSubnet) * tab.size(), hipMemcpyHostToDevice));
  m->chain_tab_valid = true;
  return IKF_OK;
}
static ikf_status run_flow_chunk_chain(ikf_model* m, const PoseSource& ps, const float* d_latent, long long r0, long long nr,
                                       int clamp_limits, float* d_q_out, hipStream_t s) {
  const FlowDims& d = m->dims;
  const int NB = m->desc.nb_nodes;
  ikf_status st = chain_table(m);
  if (st != IKF_OK) return st;
  ChainCall call{};
  call.ps = ps; call.x0 = d_latent + (size_t)r0 * d.D; call.row0 = r0; call.M = (int)nr;
  ChainSync cs{};
  cs.ctl = m->d_chain_ctl; cs.give_up = m->h_give_up; cs.row_tiles = (int)((nr + 15) / 16);
  IKF_HIP(launch_flow_chain16(m->d_chain_tab, 2 * NB, call, cs, d.width, s));
  // the last subnet in execution order (block 0, s2) left its coupling pending and the state in xbuf2 (an odd execution index)
  const PendingCoupling pend = pending_of(m, subnet_at(NB, 2 * NB - 1), m->pbuf, fused_slots(fused_skinny16_cfg(), d.width));
  IKF_HIP(launch_flow_finalize(finalize_args(m, pend, m->xbuf2, r0, nr, clamp_limits, d_q_out), s));
  return IKF_OK;
}

static ikf_status run_flow_chunk_fused(ikf_model* m, const PoseSource& ps, const float* d_latent, long long r0,
                                       long long nr, int clamp_limits, float* d_q_out, hipStream_t s) {
  const FlowDims& d = m->dims;
  const int NB = m->desc.nb_nodes;
  const long long rows_pad = m->chunk_rows;
  if (!m->wfrag_built && (chain_usable(m, nr) || cfg_reads_frag_image((m->tile_cfg >= 0) ? m->tile_cfg : fused_pick_cfg(nr, d.width, m->tune)))) {
    // the first chunk on this path that reads the fragment-major image since the weights were loaded (or ikf_reserve built it already)
    ikf_status fst = build_frag_weights(m);
    if (fst != IKF_OK) return fst;
  }
  if (chain_usable(m, nr)) {
    if (m->chain_census < 0) {
      ikf_status cst = chain_census(m, s);
      if (cst != IKF_OK) return cst;
    }
    if (m->chain_census == 1) return run_flow_chunk_chain(m, ps, d_latent, r0, nr, clamp_limits, d_q_out, s);
  }
  const int cfg = (m->tile_cfg >= 0) ? m->tile_cfg : fused_pick_cfg(nr, d.width, m->tune);
  // f16x3 mode: its own tile choice; the partial-sum slots follow the kernel that writes them
  // (f16x3 mode, batches that pick the 16-row f32 tiles - <= 128 rows: the exact-f32 kernels are the faster ones there since round 3,
  // 0.43 against 0.46 ms per call, so the mode steps aside; a forced tile configuration keeps the split kernels)
  // (also when such a tile configuration is FORCED - ikf_set_gemm_variant 160 / 161 / 164: the split kernels number their tiles differently)
  const bool split = (m->precision == 1) && m->split_arena != nullptr && !(cfg == fused_skinny16_cfg() || cfg == fused_skinny16x16_cfg() || cfg == fused_skinny32v2_cfg());
  int scfg = -1;
  if (split) {
    scfg = (m->tile_cfg >= 0) ? m->tile_cfg : split_pick_cfg(nr, d.width);
    if (split_cfg_needs_frag(scfg) && m->split_frag_arena == nullptr) scfg = 3;
  }
  const int slots = split ? split_slots(scfg, d.width) : fused_slots(cfg, d.width);
  // In-launch hand-over (TailSync): the last hidden contraction of subnet s also runs subnet s+1's entry phase, so only the
  // first subnet of the call has an entry launch.  Taken when every workgroup of that contraction is resident at once.
  const bool tail = !split && m->fuse_tail != 0 && d.n_hidden >= 2 && NB * 2 > 1 &&
                    fused_tail_ok(cfg, nr, d.width, d.D, 2 * (d.L1 > d.L2 ? d.L1 : d.L2)) &&
                    (cfg != fused_skinny_cfg() || frag_image(m, 0, d.n_hidden - 2) != nullptr);
  int tails_done = 0;
  bool entry_done = false;  // this subnet's entry phase already ran in the previous subnet's last launch
  PendingCoupling pend{};
  pend.P = nullptr;
  const float* x_src = d_latent + (size_t)r0 * d.D;
  float* const pb[2] = {m->pbuf, m->pbuf_alt};   // partial sums of even / odd subnets (the same buffer unless a launch both reads and writes them)
  auto entry_args = [&](int sidx, const PendingCoupling& pc, const float* xs) {
    EntryArgs e{};
    entry_fixed(m, sidx, e);
    e.pend = pc;
    e.x_src = xs;
    e.M = (int)nr; e.ps = ps; e.row0 = r0;
    e.split_out = split ? 1 : 0;
    e.split_flag = split ? m->d_split_flag : nullptr;
    e.wt_stores = m->wt_stores < 0 ? (nr <= 2048 ? 1 : 0) : (m->wt_stores >> 1) & 1;
    return e;
  };
  for (int sidx = 0; sidx < 2 * NB; ++sidx) {
    const SubnetPos p = subnet_at(NB, sidx);
    const SubnetWeights& w = m->subnets[p.si];
    EntryArgs e = entry_args(sidx, pend, x_src);
    if (tail && sidx == 0) { e.zero_words = m->d_arrive; e.n_zero = kArriveWords; }
    FusedGemmArgs g{};
    g.M = (int)nr; g.N = d.width; g.K = d.width; g.slope = d.slope;
    g.wt_stores = m->wt_stores < 0 ? 1 : (m->wt_stores & 1);
    g.tune = m->tune;
    g.w_last = w.w_last; g.n_out = w.n_out; g.P_out = pb[sidx & 1]; g.p_slot_stride = rows_pad * IKF_PSTRIDE;
    const int n_mid = d.n_hidden - 1;
    // small batches: the entry kernel and the first hidden contraction run as one launch (k_entry_gemm_skinny).  In the
    // chain it pays with the 32x32 tiles (129 .. 256 rows: 0.56 -> 0.53 ms per call) and the 16-row tiles (<= 128 rows, where it
    // exists only in this form worth having: r03); with the 32x64 tiles (257..512 rows) the
    // one launch takes as long as the two it replaces (18.4 us against 5.5 + 13.0), so those keep the two-launch form
    // unless it is forced (fuse_entry == 2, ikf_set_gemm_variant 112)
    const bool one_launch = !tail && !split &&
                            (m->fuse_entry == 2 || (m->fuse_entry == 1 && (cfg == fused_skinny32_cfg() || cfg == fused_skinny16_cfg() || cfg == fused_skinny16x16_cfg() || cfg == fused_skinny32v2_cfg()))) &&
                            entry_gemm_ok(cfg, nr, d.width, d.D, pend.P ? pend.n_out : 0) &&
                            frag_image(m, p.si, 0) != nullptr;
    if (!one_launch && !entry_done) IKF_HIP(launch_subnet_entry(w.n_x + d.n_pose, e, s));
    entry_done = false;
    const PendingCoupling mine = pending_of(m, p, pb[sidx & 1], slots);
    float* cur = m->hA;
    float* nxt = m->hB;
    for (int l = 0; l < n_mid; ++l) {
      const bool last = (l == n_mid - 1);
      IKF_HIP(prof_mark(m, s));
      if (split) {
        SplitGemmArgs sg{};
        sg.A = cur; sg.C = last ? nullptr : nxt; sg.W = m->w_mid_split[(size_t)p.si * 3 + l];
        sg.Wf = m->w_mid_split_frag.empty() ? nullptr : m->w_mid_split_frag[(size_t)p.si * 3 + l];
        sg.bias = w.b_mid[l]; sg.M = (int)nr; sg.N = d.width; sg.K = d.width; sg.slope = d.slope;
        sg.w_last = w.w_last; sg.n_out = w.n_out; sg.P_out = pb[sidx & 1]; sg.p_slot_stride = rows_pad * IKF_PSTRIDE;
        sg.flag = m->d_split_flag;
        IKF_HIP(launch_split_gemm(last, scfg, sg, s));
      } else {
        g.A = cur; g.C = last ? nullptr : nxt; g.W = w.w_mid[l]; g.bias = w.b_mid[l];
        g.Wf = frag_image(m, p.si, l);
        if (l == 0 && one_launch) IKF_HIP(launch_entry_gemm(w.n_x + d.n_pose, last, cfg, e, g, s));
        else if (last && tail && sidx + 1 < 2 * NB) {
          // subnet sidx+1's entry phase rides in this launch's tail: its pending coupling is what this launch produces, its
          // state source is the state this subnet's entry phase published
          const EntryArgs e2 = entry_args(sidx + 1, mine, e.x_dst);
          TailSync ts{};
          ts.arrive = m->d_arrive;
          ts.target = (unsigned)(tails_done + 1) * (unsigned)fused_tail_col_tiles(cfg, d.width);
          ts.give_up = m->h_give_up;
          ts.n_in = e2.n_x + d.n_pose;
          IKF_HIP(launch_flow_gemm_tail(cfg, g, e2, ts, s));
          ++tails_done;
          entry_done = true;
        } else IKF_HIP(launch_flow_gemm(last, cfg, g, s));
      }
      IKF_HIP(prof_mark(m, s));
      float* tmp = cur; cur = nxt; nxt = tmp;
    }
    pend = mine;
    x_src = e.x_dst;
  }
  IKF_HIP(launch_flow_finalize(finalize_args(m, pend, x_src, r0, nr, clamp_limits, d_q_out), s));
  return IKF_OK;
}

// A subnet up to its last Linear on the unfused kernels (flow_kernels.hip): the first Linear into hA, then the hidden contractions ping-ponging
// between hA and hB (`mark`: each inside a profiling pair).  Returns the buffer that holds the last activations, or null (the error is recorded).
static float* run_hidden_stack(ikf_model* m, const SubnetWeights& w, const float* x_src, int x_off, const PoseSource& ps, long long r0,
                               long long nr, int variant, bool mark, hipStream_t s) {
  const FlowDims& d = m->dims;
  float* cur = m->hA;
  float* nxt = m->hB;
  const ikf_status st = [&]() -> ikf_status {
    IKF_HIP(launch_first_layer(w, d, x_src, x_off, ps, r0, nr, m->hA, s));
    for (int l = 0; l < d.n_hidden - 1; ++l) {
      if (mark) IKF_HIP(prof_mark(m, s));
      IKF_HIP(launch_gemm_lrelu(variant, cur, w.w_mid[l], w.b_mid[l], nxt, nr, d.width, d.width, d.slope, s));
      if (mark) IKF_HIP(prof_mark(m, s));
      float* tmp = cur; cur = nxt; nxt = tmp;
    }
    return IKF_OK;
  }();
  return st == IKF_OK ? cur : nullptr;
}

// four-plus kernels per subnet (flow_kernels.hip): first Linear, hidden contractions, last Linear + coupling
static ikf_status run_flow_chunk_unfused(ikf_model* m, const PoseSource& ps, const float* d_latent, long long r0,
                                         long long nr, int clamp_limits, float* d_q_out, hipStream_t s) {
  const FlowDims& d = m->dims;
  const int NB = m->desc.nb_nodes;
  const int variant = pick_variant(m, nr);
  for (int b = NB - 1; b >= 0; --b) {
    const float* x_in = (b == NB - 1) ? d_latent + (size_t)r0 * d.D : m->xbuf;
    for (int which = 1; which <= 2; ++which) {
      const SubnetWeights& w = m->subnets[2 * b + which - 1];
      const float* x_src = (which == 1) ? x_in : m->xbuf;
      const float* cur = run_hidden_stack(m, w, x_src, which == 1 ? 0 : d.L1, ps, r0, nr, variant, /*mark=*/true, s);
      if (!cur) return IKF_ERR_HIP;
      CouplingArgs ca{};
      ca.x_in = x_in;
      ca.x_out = m->xbuf;
      ca.perm_inv = m->d_perm_inv + (size_t)b * d.D;
      ca.M_inv = m->d_Minv;
      ca.b_lin = m->d_blin;
      ca.lo = chain_lo(m);
      ca.hi = chain_hi(m);
      ca.q_out = d_q_out + (size_t)r0 * d.ndof;
      ca.which = which;
      ca.is_final = (b == 0 && which == 2) ? 1 : 0;
      ca.clamp_limits = clamp_limits;
      ca.sigmoid = m->desc.sigmoid_on_output ? 1 : 0;
      IKF_HIP(launch_last_layer_coupling(w, d, cur, ca, nr, s));
    }
  }
  return IKF_OK;
}

// ---- which form runs which rows of a batch: flow_plan.h decides (plan_rows, ClusterBackoff); here is what a handle brings to it ----
static bool rowowner_allowed(const ikf_model* m) {
  return m->ro_stream != nullptr && m->ro_mode != 0 && m->precision == 0 && m->loaded &&
         (m->ro_mode == 1 || (m->gemm_variant < 0 && m->tile_cfg < 0 && m->fuse_tail == 0));
}
// A wait of a tagged + XCD-local launch ran out: was it placement?  Every member of that launch wrote (launch number << 8 | XCC_ID) into its word
// at its start (flow_rowowner.hip); launches queued behind the one that gave up returned before they wrote anything, so the largest launch number
// found is the failed launch's.  Members of one row tile that ran it on different XCDs = the XCD-local form was used where it must not be.
// Rare path (a 5 ms stall has just happened): one device synchronisation and a copy of a few KB.
static bool cluster_tagged_local_misplaced(ikf_model* m) {
  DeviceGuard guard(m->device);
  const unsigned* words = cluster_tagged_xcc_words(m);
  if (guard.err != hipSuccess || words == nullptr) return false;
  const int n_rt = m->cl_tl_nrt, G = m->cl_tl_G;
  std::vector<unsigned> w((size_t)n_rt * 32, 0xffffffffu);
  if (hipDeviceSynchronize() != hipSuccess) return false;
  if (hipMemcpy(w.data(), words, w.size() * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return false;
  unsigned seq = 0;
  bool any = false;
  for (int rt = 0; rt < n_rt; ++rt)
    for (int j = 0; j < G; ++j) {
      const unsigned v = w[(size_t)rt * 32 + j];
      if (v == 0xffffffffu) continue;
      if (!any || (((v >> 8) - seq) & 0xffffffu) < 0x800000u) seq = v >> 8;   // (24-bit sequence numbers wrap)
      any = true;
    }
  if (!any) return false;
  for (int rt = 0; rt < n_rt; ++rt) {
    int first = -1;
    for (int j = 0; j < G; ++j) {
      const unsigned v = w[(size_t)rt * 32 + j];
      if (v == 0xffffffffu || (v >> 8) != seq) continue;
      if (first < 0) first = (int)(v & 0xffu);
      else if ((int)(v & 0xffu) != first) return true;
    }
  }
  return false;
}
// folds a pending give-up word into the handle's state (no side effect otherwise)
static void cluster_fold_give_up(ikf_model* m) {
  if (!m->h_cl_give_up || *m->h_cl_give_up == 0) return;
  // an earlier call's cluster launch gave up (its rows were recomputed by the repair launch)
  int why = *m->h_cl_give_up;
  *m->h_cl_give_up = 0;
  if (why == 1 && m->cl_local != 0 && m->cl_tl_nrt > 0 && cluster_tagged_local_misplaced(m)) why = 2;
  m->cl_tag_dirty = true;                            // (whichever hand-over it was: the tagged buffers are re-created before their next use)
  if (m->cl_back.give_up(why)) m->cl_local = 0;      // a member of the XCD-local form met a peer on another XCD: back to the spread form
}
// everything but the pause: the handle has the form and its settings leave the choice to the planner
static bool cluster_enabled(const ikf_model* m) {
  if (m->ro_stream == nullptr || m->cl_mode == 0 || m->precision != 0 || !m->loaded) return false;
  return m->cl_mode == 1 || (m->gemm_variant < 0 && m->tile_cfg < 0 && m->fuse_tail == 0 && m->ro_mode != 0);
}
// `consume`: this plan is about to run (it counts against a pause of the cluster form and towards its clean streak); the describing entry
// points pass false and only look at the pause
static std::vector<FlowChunk> plan_flow(ikf_model* m, long long rows, bool consume = false) {
  if (rows <= 0) return {};
  cluster_fold_give_up(m);
  const bool may = consume ? m->cl_back.ask() : !m->cl_back.paused();
  const bool ro = rowowner_allowed(m), cl = may && cluster_enabled(m);
  std::vector<FlowChunk> plan = plan_rows(rows, m->n_cu, ro, cl, m->ro_mode, m->cl_mode, m->ro_min_tail);
  if (consume) {
    bool cluster_chunk = false;
    for (const FlowChunk& c : plan) cluster_chunk = cluster_chunk || c.form >= 2;
    m->cl_back.used(cluster_chunk);
  }
  return plan;
}
static RoArgs rowowner_args(ikf_model* m, const PoseSource& ps, const float* d_latent, long long r0, long long nr, int clamp_limits, float* d_q_out) {
  const FlowDims& d = m->dims;
  RoArgs a{};
  a.stream = m->ro_stream;
  a.stream_bytes = (unsigned)(rowowner_stream_floats(2 * m->desc.nb_nodes) * sizeof(float));
  a.sub = m->d_ro_sub; a.n_sub = 2 * m->desc.nb_nodes;
  a.x0 = d_latent + (size_t)r0 * d.D;
  a.ps = ps; a.row0 = r0; a.M = (int)nr; a.D = d.D; a.L1 = d.L1; a.ndof = d.ndof; a.clamp = d.clamp; a.slope = d.slope;
  a.M_inv = m->d_Minv; a.b_lin = m->d_blin; a.lo = chain_lo(m); a.hi = chain_hi(m);
  a.clamp_limits = clamp_limits; a.sigmoid = m->desc.sigmoid_on_output ? 1 : 0;
  a.q_out = d_q_out + (size_t)r0 * d.ndof;
  return a;
}
static ikf_status run_flow_rowowner(ikf_model* m, const PoseSource& ps, const float* d_latent, long long r_base, long long rows,
                                    int clamp_limits, float* d_q_out, hipStream_t s) {
  return for_each_piece(r_base, rows, kMaxLaunchRows, [&](long long r0, long long nr) -> ikf_status {
    const RoArgs a = rowowner_args(m, ps, d_latent, r0, nr, clamp_limits, d_q_out);
    IKF_HIP(prof_mark(m, s));
    IKF_HIP(launch_flow_rowowner(a, m->ro_nbuf, s));
    IKF_HIP(prof_mark(m, s));
    return IKF_OK;
  });
}

static ikf_status run_flow_cluster(ikf_model* m, int G, const PoseSource& ps, const float* d_latent, long long r0, long long nr,
                                   int clamp_limits, float* d_q_out, hipStream_t s) {
  ikf_status st = ensure_cluster_scratch(m, nr);
  if (st != IKF_OK) return st;
  RcArgs c{};
  c.ro = rowowner_args(m, ps, d_latent, r0, nr, clamp_limits, d_q_out);
  c.n_rt = (int)((nr + IKF_RO_ROWS - 1) / IKF_RO_ROWS);
  const bool tagged = m->cl_tagged != 0 && G <= 16;   // (the parity argument needs an even number of subnets: 2 per coupling block)
  const bool local = m->cl_local != 0 && cluster_local_form(G) && cluster_grid(c.n_rt, G, true) <= (unsigned)m->n_cu;
  c.give_up = m->h_cl_give_up;
  if (tagged) {
    unsigned* const abort_t = cluster_tagged_abort_word(m);
    if (m->cl_tag_dirty) {
      IKF_HIP(cluster_tagged_init(m->cl_xbuf_t, cluster_xbuf_floats((int)(m->cl_rows / IKF_RO_ROWS)), m->cl_sync_t, m->cl_sync_t_bytes - 128, abort_t, s));
      m->cl_tag_dirty = false;
    }
    c.xbuf = m->cl_xbuf_t;
    c.pbuf = m->cl_sync_t;
    c.flags = nullptr;
    c.abort_word = abort_t;
    c.test_far = local ? m->cl_far_next : 0;   // (variant 191: honoured by the tagged form's placement check too)
    if (local) m->cl_far_next = 0;
    c.xcc_words = cluster_tagged_xcc_words(m);
    m->cl_launch_seq = (m->cl_launch_seq + 1) & 0xffffffu;
    if (m->cl_launch_seq == 0xffffffu) m->cl_launch_seq = 0;
    c.launch_seq = m->cl_launch_seq;
    if (local) { m->cl_tl_nrt = c.n_rt; m->cl_tl_G = G; }
    IKF_HIP(prof_mark(m, s));
    IKF_HIP(launch_flow_cluster_tagged(c, G, s, m->cl_drop_next, local));
  } else {
    c.xbuf = m->cl_xbuf;
    c.pbuf = m->cl_sync;
    c.flags = reinterpret_cast<unsigned*>(m->cl_sync.p) + (size_t)c.n_rt * G * 256;
    c.abort_word = c.flags + (size_t)c.n_rt * G * 32;
    c.test_far = local ? m->cl_far_next : 0;
    if (local) m->cl_far_next = 0;
    IKF_HIP(prof_mark(m, s));
    IKF_HIP(launch_flow_cluster(c, G, s, m->cl_drop_next, local));
  }
  m->cl_drop_next = 0;
  IKF_HIP(prof_mark(m, s));
  // the repair launch: the same rows through the row-owner kernel, which returns at once unless a wait of the cluster launch ran out
  RoArgs rep = c.ro;
  rep.run_if = c.abort_word;
  IKF_HIP(launch_flow_rowowner(rep, m->ro_nbuf, s));
  return IKF_OK;
}

// "rowowner:4096 cluster16:200" - the chunks run_flow would cut a call of `rows` rows into (tests / tools)
extern "C" ikf_status ikf_plan_describe(ikf_model* m, int64_t rows, char* buf, int buf_len) {
  if (!m || !buf || buf_len < 1) return fail(IKF_ERR_NULL_POINTER, "ikf_plan_describe: null argument");
  const std::string out = plan_text(plan_flow(m, rows));
  if ((int)out.size() + 1 > buf_len) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_plan_describe: buffer too small");
  memcpy(buf, out.c_str(), out.size() + 1);
  return IKF_OK;
}
// the same decision without a handle or a device: a chip of n_cu CUs, the resident-row forms allowed or not (released shape, f32)
extern "C" ikf_status ikf_plan_describe_for(int n_cu, int64_t rows, int rowowner_allowed, int cluster_allowed, char* buf, int buf_len) {
  if (!buf || buf_len < 1) return fail(IKF_ERR_NULL_POINTER, "ikf_plan_describe_for: null argument");
  if (n_cu <= 0) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_plan_describe_for: n_cu must be positive");
  const std::string out = plan_text(plan_rows(rows, n_cu, rowowner_allowed != 0, cluster_allowed != 0, -1, -1, -1));
  if ((int)out.size() + 1 > buf_len) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_plan_describe_for: buffer too small");
  memcpy(buf, out.c_str(), out.size() + 1);
  return IKF_OK;
}
// 1: cluster launches with 4 / 8 / 16 members hand over through one XCD's L2 (the load-time placement census agreed and no launch has met a
// member elsewhere since); 0: through memory
extern "C" int ikf_cluster_local(ikf_model* m) {
  if (!m) return 0;
  cluster_fold_give_up(m);
  return (m->cl_local != 0 && m->cl_mode != 0 && m->ro_stream != nullptr) ? 1 : 0;
}
extern "C" int64_t ikf_cluster_repairs(ikf_model* m) {
  if (!m) return 0;
  cluster_fold_give_up(m);
  return (int64_t)m->cl_back.repairs();
}
// calls the cluster form still sits out after a wait of one of its launches ran out (0: in use / never paused)
extern "C" int64_t ikf_cluster_backoff(ikf_model* m) {
  if (!m) return 0;
  cluster_fold_give_up(m);
  return (int64_t)m->cl_back.pause_left();
}
extern "C" const char* ikf_dominant_kernel_for(const ikf_model* m, int64_t rows) {
  if (m && rows > 0) {
    long long by_form[3] = {0, 0, 0};
    for (const FlowChunk& c : plan_flow(const_cast<ikf_model*>(m), rows)) by_form[c.form >= 2 ? 2 : c.form] += c.rows;
    if (by_form[1] >= by_form[0] && by_form[1] >= by_form[2] && by_form[1] > 0) return rowowner_kernel_name();
    if (by_form[2] >= by_form[0] && by_form[2] > 0) return "k_flow_cluster";
  }
  return (m && m->precision == 1 && m->split_arena) ? split_kernel_name() : fused_kernel_name();
}
static ikf_status run_flow(ikf_model* m, PoseSource ps, const float* d_latent, long long rows, int clamp_limits,
                           float* d_q_out, hipStream_t s) {
  const std::vector<FlowChunk> plan = plan_flow(m, rows, /*consume=*/true);
  const bool fused = fused_ok(m);
  long long r_base = 0;
  for (const FlowChunk& c : plan) {
    ikf_status st = IKF_OK;
    if (c.form == 1) st = run_flow_rowowner(m, ps, d_latent, r_base, c.rows, clamp_limits, d_q_out, s);
    else if (c.form >= 2 && cluster_grid((int)((c.rows + IKF_RO_ROWS - 1) / IKF_RO_ROWS), c.form, false) <= (unsigned)m->n_cu)   // (every workgroup of a cluster launch must be resident)
      st = run_flow_cluster(m, c.form, ps, d_latent, r_base, c.rows, clamp_limits, d_q_out, s);
    else
      st = for_each_chunk(m, r_base, c.rows, [&](long long r0, long long nr) {
        return fused ? run_flow_chunk_fused(m, ps, d_latent, r0, nr, clamp_limits, d_q_out, s)
                     : run_flow_chunk_unfused(m, ps, d_latent, r0, nr, clamp_limits, d_q_out, s);
      });
    if (st != IKF_OK) return st;
    r_base += c.rows;
  }
  return IKF_OK;
}

// f16x3 range guard: read the overflow word after the flow of a call / round; true -> the caller re-runs on the f32 path
static ikf_status split_overflowed(ikf_model* m, hipStream_t s, bool* out) {
  *out = false;
  if (m->precision != 1 || !m->split_arena || !m->d_split_flag) return IKF_OK;
  IKF_HIP(hipMemcpyAsync(m->h_split_flag, m->d_split_flag, sizeof(int), hipMemcpyDeviceToHost, s));
  IKF_HIP(hipStreamSynchronize(s));
  if (*m->h_split_flag != 0) {
    *out = true;
    IKF_HIP(hipMemsetAsync(m->d_split_flag, 0, sizeof(int), s));
  }
  return IKF_OK;
}

// flow with the range guard applied (guard on + f16x3 mode: one flag read per call; out of range -> f32 re-run)
ikf_status ikf::run_flow_guarded(ikf_model* m, PoseSource ps, const float* d_latent, long long rows, int clamp_limits,
                                 float* d_q_out, hipStream_t s) {
  ikf_status st = run_flow(m, ps, d_latent, rows, clamp_limits, d_q_out, s);
  if (st != IKF_OK || m->precision != 1 || !m->split_guard) return st;
  bool bad = false;
  st = split_overflowed(m, s, &bad);
  if (st != IKF_OK || !bad) return st;
  m->precision = 0;
  st = run_flow(m, ps, d_latent, rows, clamp_limits, d_q_out, s);
  m->precision = 1;
  ++m->split_fallbacks;
  return st;
}
extern "C" int ikf_split_overflow_pending(ikf_model* m, void* stream) {
  if (!m) return 0;
  DeviceGuard dev_guard_(m->device);
  if (dev_guard_.err != hipSuccess) return 0;
  bool bad = false;
  const int saved = m->precision;
  if (m->split_arena) m->precision = 1;  // the flag is meaningful whenever the split images exist
  (void)split_overflowed(m, static_cast<hipStream_t>(stream), &bad);
  m->precision = saved;
  return bad ? 1 : 0;
}

ikf_status ikf::check_ready(ikf_model* m, const char* fn) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, std::string(fn) + ": null model");
  if (m->h_give_up && *m->h_give_up != 0) {
    // a workgroup of an EARLIER call gave up waiting for a sibling inside a launch (it was never resident: the device is
    // shared or partitioned in a way the launcher did not expect).  That call's results are invalid; the hand-over is
    // switched off for this handle and every later call uses the plain launch boundary.
    *m->h_give_up = 0;
    m->fuse_tail = 0;
    m->chain_mode = 0;
    if (m->d_chain_ctl) (void)hipMemset(m->d_chain_ctl, 0, sizeof(unsigned) * IKF_CHAIN_CTL_WORDS);
    return fail(IKF_ERR_HIP, std::string(fn) + ": an in-launch hand-over of a PREVIOUS call timed out - that call's results are invalid; "
                                               "the in-launch hand-over is now disabled for this handle, repeat the call");
  }
  if (!m->loaded)
    return fail(IKF_ERR_NOT_LOADED, "Model weights have not been loaded. Call load_state_dict(...)");
  return IKF_OK;
}

// The frame of the flow entries: the handle is ready, n is sane (0 rows: nothing to do), the entry's own pointers are there
// (`null_args`: what is wrong with them, or null), then `body(ps, s)` on the handle's device inside the stream scope.  `d_idx` / `n_mod`: the
// pose source's list and modulus (batch form: null / n, single pose: null / 1, tiling: anything else, ikf_internal.h).
template <class Body> static ikf_status flow_call(ikf_model* m, const char* fn, int64_t n, const char* null_args, const float* d_poses,
                                                  const int32_t* d_idx, int64_t n_mod, float softflow_scale, void* stream, Body body) {
  ikf_status st = check_ready(m, fn);
  if (st != IKF_OK) return st;
  if (n < 0) return fail(IKF_ERR_BAD_ARGUMENT, std::string(fn) + ": n must be >= 0");
  if (n_mod < 1) return fail(IKF_ERR_BAD_ARGUMENT, std::string(fn) + ": n_mod must be >= 1");
  if (n == 0) return IKF_OK;
  if (null_args) return fail(IKF_ERR_NULL_POINTER, std::string(fn) + ": " + null_args);
  IKF_ON_DEVICE(m)
  const PoseSource ps{d_poses, d_idx, (long long)n_mod, 7, softflow_scale};
  hipStream_t s = static_cast<hipStream_t>(stream);
  StreamScope scope(m, s);
  IKF_HIP(scope.enter());
  st = body(ps, s);
  if (st != IKF_OK) return st;
  IKF_HIP(scope.leave());
  return IKF_OK;
}

// the modulus of the two pose sources the public entries build: one pose per row, or one pose for every row (n <= 0 is flow_call's to answer)
static int64_t batch_mod(int pose_broadcast, int64_t n) { return (pose_broadcast || n < 1) ? 1 : n; }

extern "C" ikf_status ikf_generate_approx(ikf_model* m, const float* d_poses, int pose_broadcast, const float* d_latent,
                                          int64_t n, int clamp_to_limits, float softflow_scale, float* d_q_out,
                                          void* stream) {
  const char* null_args = (!d_poses || !d_latent || !d_q_out) ? "null device pointer" : nullptr;
  return flow_call(m, "ikf_generate_approx", n, null_args, d_poses, nullptr, batch_mod(pose_broadcast, n), softflow_scale, stream,
                   [&](const PoseSource& ps, hipStream_t s) { return run_flow_guarded(m, ps, d_latent, n, clamp_to_limits, d_q_out, s); });
}

// ikf_generate_approx under the tiling pose source of exact IK (run_exact) and of the candidate stage (flow_candidates): tests (ikflow_amd_debug.h)
extern "C" ikf_status ikf_generate_approx_tiled(ikf_model* m, const float* d_poses, const int32_t* d_idx, int64_t n_mod, const float* d_latent,
                                                int64_t n, int clamp_to_limits, float softflow_scale, float* d_q_out, void* stream) {
  const char* null_args = (!d_poses || !d_latent || !d_q_out) ? "null device pointer" : nullptr;
  return flow_call(m, "ikf_generate_approx_tiled", n, null_args, d_poses, d_idx, n_mod, softflow_scale, stream,
                   [&](const PoseSource& ps, hipStream_t s) { return run_flow_guarded(m, ps, d_latent, n, clamp_to_limits, d_q_out, s); });
}

// ---------------------------------------------------------------------------------------------------------------
// forward (training-direction) pass: nn_model(x, c=cond, jac=True) of ikflow/training/lt_model.py:156
// ---------------------------------------------------------------------------------------------------------------
// The released width (1024, 3 hidden layers): one k_flow_rowowner_fwd launch for any batch size (no cluster form).  Every other shape: the
// per-layer kernels, chunked like the inverse pass (state in xbuf, running log-det in xbuf2).
static ikf_status run_forward_rowowner(ikf_model* m, const PoseSource& ps, const float* d_x, long long rows, float* d_z, float* d_ld,
                                       hipStream_t s) {
  const FlowDims& d = m->dims;
  return for_each_piece(0, rows, kMaxLaunchRows, [&](long long r0, long long nr) -> ikf_status {
    RoArgs a = rowowner_args(m, ps, d_x, r0, nr, 0, nullptr);
    a.sub = m->d_ro_sub_fwd;
    a.M_inv = nullptr; a.q_out = nullptr;
    RoFwd f{};
    f.M = m->d_M;
    f.perm0 = m->d_perm;
    f.log_det0 = m->log_det_M;
    f.z_out = d_z ? d_z + (size_t)r0 * d.D : nullptr;
    f.ld_out = d_ld ? d_ld + r0 : nullptr;
    IKF_HIP(launch_flow_rowowner_fwd(a, f, s));
    return IKF_OK;
  });
}
static ikf_status run_forward_chunk_per_layer(ikf_model* m, const PoseSource& ps, const float* d_x, long long r0, long long nr, float* d_z,
                                              float* d_ld, hipStream_t s) {
  const FlowDims& d = m->dims;
  const int NB = m->desc.nb_nodes;
  const int variant = pick_variant(m, nr);
  FwdEntryArgs ea{};
  ea.x = d_x + (size_t)r0 * d.D;
  ea.M = m->d_M; ea.b_lin = m->d_blin; ea.perm0 = m->d_perm; ea.log_det0 = m->log_det_M;
  ea.D = d.D; ea.sigmoid = m->desc.sigmoid_on_output ? 1 : 0;
  ea.state = m->xbuf; ea.ld = m->xbuf2;
  IKF_HIP(launch_fwd_entry(ea, nr, s));
  for (int b = 0; b < NB; ++b) {
    for (int which = 2; which >= 1; --which) {
      const SubnetWeights& w = m->subnets[2 * b + which - 1];
      const float* cur = run_hidden_stack(m, w, m->xbuf, which == 1 ? 0 : d.L1, ps, r0, nr, variant, /*mark=*/false, s);
      if (!cur) return IKF_ERR_HIP;
      FwdCouplingArgs ca{};
      ca.state = m->xbuf;
      ca.perm_next = (which == 1 && b + 1 < NB) ? m->d_perm + (size_t)(b + 1) * d.D : nullptr;
      ca.ld = m->xbuf2;
      ca.which = which;
      ca.is_final = (b == NB - 1 && which == 1) ? 1 : 0;
      ca.z_out = d_z ? d_z + (size_t)r0 * d.D : nullptr;
      ca.ld_out = d_ld ? d_ld + r0 : nullptr;
      IKF_HIP(launch_last_layer_coupling_fwd(w, d, cur, ca, nr, s));
    }
  }
  return IKF_OK;
}

extern "C" ikf_status ikf_flow_forward(ikf_model* m, const float* d_x, int64_t n, const float* d_poses, int pose_broadcast,
                                       float softflow_scale, float* d_z_out, float* d_log_det_out, void* stream) {
  const char* null_args = (!d_x || !d_poses) ? "null device pointer"
                          : (!d_z_out && !d_log_det_out) ? "d_z_out and d_log_det_out are both null" : nullptr;
  return flow_call(m, "ikf_flow_forward", n, null_args, d_poses, nullptr, batch_mod(pose_broadcast, n), softflow_scale, stream,
                   [&](const PoseSource& ps, hipStream_t s) {
    if (m->d_ro_sub_fwd != nullptr) return run_forward_rowowner(m, ps, d_x, n, d_z_out, d_log_det_out, s);
    return for_each_chunk(m, 0, n, [&](long long r0, long long nr) { return run_forward_chunk_per_layer(m, ps, d_x, r0, nr, d_z_out, d_log_det_out, s); });
  });
}

// ---------------------------------------------------------------------------------------------------------------
// inverse pass with its log-determinant: nn_model(latent, c=cond, rev=True) -> (output_rev, log_jac_det) (ikflow_solver.py:98)
// ---------------------------------------------------------------------------------------------------------------
// The released width (1024, 3 hidden layers): one k_flow_rowowner_ld launch for any batch size (never the cluster form).  Every other shape:
// the per-layer kernels, chunked (state in xbuf, running log-det in xbuf2).  Always the f32 contractions, like ikf_flow_forward.
static ikf_status run_inverse_ld_rowowner(ikf_model* m, const PoseSource& ps, const float* d_latent, long long rows, int clamp_limits,
                                          float* d_x, float* d_q, float* d_ld, hipStream_t s) {
  const FlowDims& d = m->dims;
  return for_each_piece(0, rows, kMaxLaunchRows, [&](long long r0, long long nr) -> ikf_status {
    RoArgs a = rowowner_args(m, ps, d_latent, r0, nr, clamp_limits, nullptr);
    a.q_out = d_q ? d_q + (size_t)r0 * d.ndof : nullptr;
    RoFwd f{};
    f.log_det0 = m->log_det_Minv;
    f.z_out = d_x ? d_x + (size_t)r0 * d.D : nullptr;
    f.ld_out = d_ld ? d_ld + r0 : nullptr;
    IKF_HIP(launch_flow_rowowner_ld(a, f, s));
    return IKF_OK;
  });
}
static ikf_status run_inverse_ld_chunk_per_layer(ikf_model* m, const PoseSource& ps, const float* d_latent, long long r0, long long nr,
                                                 int clamp_limits, float* d_x, float* d_q, float* d_ld, hipStream_t s) {
  const FlowDims& d = m->dims;
  const int NB = m->desc.nb_nodes;
  const int variant = pick_variant(m, nr);
  for (int b = NB - 1; b >= 0; --b) {
    for (int which = 1; which <= 2; ++which) {
      const SubnetWeights& w = m->subnets[2 * b + which - 1];
      const bool first = b == NB - 1 && which == 1;
      const float* x_src = first ? d_latent + (size_t)r0 * d.D : m->xbuf;
      const float* cur = run_hidden_stack(m, w, x_src, which == 1 ? 0 : d.L1, ps, r0, nr, variant, /*mark=*/false, s);
      if (!cur) return IKF_ERR_HIP;
      InvCouplingArgs ca{};
      ca.x_in = x_src;
      ca.state = m->xbuf;
      ca.perm_inv = m->d_perm_inv + (size_t)b * d.D;
      ca.ld = m->xbuf2;
      ca.which = which;
      ca.first = first ? 1 : 0;
      IKF_HIP(launch_last_layer_coupling_inv(w, d, cur, ca, nr, s));
    }
  }
  InvExitArgs ea{};
  ea.state = m->xbuf; ea.ld = m->xbuf2;
  ea.M_inv = m->d_Minv; ea.b_lin = m->d_blin; ea.lo = chain_lo(m); ea.hi = chain_hi(m);
  ea.log_det0 = m->log_det_Minv;
  ea.D = d.D; ea.ndof = d.ndof; ea.sigmoid = m->desc.sigmoid_on_output ? 1 : 0; ea.clamp_limits = clamp_limits;
  ea.x_out = d_x ? d_x + (size_t)r0 * d.D : nullptr;
  ea.q_out = d_q ? d_q + (size_t)r0 * d.ndof : nullptr;
  ea.ld_out = d_ld ? d_ld + r0 : nullptr;
  IKF_HIP(launch_inv_exit(ea, nr, s));
  return IKF_OK;
}

extern "C" ikf_status ikf_flow_inverse(ikf_model* m, const float* d_latent, int64_t n, const float* d_poses, int pose_broadcast,
                                       float softflow_scale, int clamp_to_limits, float* d_x_out, float* d_q_out,
                                       float* d_log_det_out, void* stream) {
  const char* null_args = (!d_latent || !d_poses) ? "null device pointer"
                          : (!d_x_out && !d_q_out && !d_log_det_out) ? "d_x_out, d_q_out and d_log_det_out are all null" : nullptr;
  return flow_call(m, "ikf_flow_inverse", n, null_args, d_poses, nullptr, batch_mod(pose_broadcast, n), softflow_scale, stream,
                   [&](const PoseSource& ps, hipStream_t s) {
    if (m->ro_stream != nullptr && m->d_ro_sub != nullptr)   // (the row-owner image exists: the released shape)
      return run_inverse_ld_rowowner(m, ps, d_latent, n, clamp_to_limits, d_x_out, d_q_out, d_log_det_out, s);
    return for_each_chunk(m, 0, n, [&](long long r0, long long nr) {
      return run_inverse_ld_chunk_per_layer(m, ps, d_latent, r0, nr, clamp_to_limits, d_x_out, d_q_out, d_log_det_out, s);
    });
  });
}

// ---------------------------------------------------------------------------------------------------------------
// measurement hook
// ---------------------------------------------------------------------------------------------------------------
extern "C" ikf_status ikf_time_gemm(ikf_model* m, int64_t rows, int iters, float* ms_out, void* stream) {
  ikf_status st = check_ready(m, "ikf_time_gemm");
  if (st != IKF_OK) return st;
  if (!ms_out || rows < 1 || iters < 1) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_time_gemm: bad argument");
  if (m->dims.n_hidden < 2) return fail(IKF_ERR_BAD_SHAPE, "ikf_time_gemm: model has no width x width layer");
  IKF_ON_DEVICE(m)
  hipStream_t s = static_cast<hipStream_t>(stream);
  st = ensure_scratch(m, rows);
  if (st != IKF_OK) return st;
  if (cfg_reads_frag_image((m->tile_cfg >= 0) ? m->tile_cfg : fused_pick_cfg(rows, m->dims.width, m->tune))) {
    st = build_frag_weights(m);
    if (st != IKF_OK) return st;
  }
  if (rows > m->chunk_rows) rows = m->chunk_rows;
  const SubnetWeights& w = m->subnets[0];
  const int variant = pick_variant(m, rows);
  const bool fused = fused_ok(m) && m->dims.n_hidden >= 3;
  hipEvent_t e0, e1;
  IKF_HIP(hipEventCreate(&e0));
  IKF_HIP(hipEventCreate(&e1));
  FusedGemmArgs g{};
  if (fused) {
    // the contraction that reads its A operand from HBM and reduces the last Linear in its epilogue (h -> partials)
    g.M = (int)rows; g.N = m->dims.width; g.K = m->dims.width; g.slope = m->dims.slope;
    g.tune = m->tune;
    g.A = m->hA; g.W = w.w_mid[m->dims.n_hidden - 2]; g.bias = w.b_mid[m->dims.n_hidden - 2];
    g.Wf = frag_image(m, 0, m->dims.n_hidden - 2);
    g.w_last = w.w_last; g.n_out = w.n_out; g.P_out = m->pbuf; g.p_slot_stride = m->chunk_rows * IKF_PSTRIDE;
  }
  auto launch = [&]() -> hipError_t {
    if (fused) return launch_flow_gemm(true, (m->tile_cfg >= 0) ? m->tile_cfg : fused_pick_cfg(rows, m->dims.width, m->tune), g, s);
    return launch_gemm_lrelu(variant, m->hA, w.w_mid[0], w.b_mid[0], m->hB, rows, m->dims.width, m->dims.width,
                             m->dims.slope, s);
  };
  IKF_HIP(launch());
  IKF_HIP(hipEventRecord(e0, s));
  for (int i = 0; i < iters; ++i) IKF_HIP(launch());
  IKF_HIP(hipEventRecord(e1, s));
  IKF_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  IKF_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *ms_out = ms / iters;
  return IKF_OK;
}
