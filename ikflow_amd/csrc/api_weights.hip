// C-ABI of libikflow_amd.so, the weights: ikf_load_weights (state-dict validation, the packed fp32 arena) and the device-side images
// built from it (split-32, fragment-major, the row-owner stream).  See include/ikflow_amd.h for the contract.
#include "ikf_model.h"

static const ikf_tensor* find_tensor(const std::unordered_map<std::string, const ikf_tensor*>& idx, const std::string& k) {
  auto it = idx.find(k);
  return it == idx.end() ? nullptr : it->second;
}

static ikf_status need(const std::unordered_map<std::string, const ikf_tensor*>& idx, const std::string& key, int dtype,
                       std::initializer_list<int64_t> shape, const ikf_tensor** out) {
  const ikf_tensor* t = find_tensor(idx, key);
  if (!t) return fail(IKF_ERR_MISSING_TENSOR, "Missing key(s) in state_dict: \"" + key + "\"");
  if (!t->h_data) return fail(IKF_ERR_NULL_POINTER, "state_dict tensor \"" + key + "\" has a null data pointer");
  if (t->dtype != dtype) return fail(IKF_ERR_MISSING_TENSOR, "state_dict tensor \"" + key + "\" has the wrong dtype");
  bool ok = (t->ndim == (int)shape.size());
  int i = 0;
  if (ok)
    for (int64_t s : shape) ok = ok && (t->shape[i++] == s);
  if (!ok) {
    std::string got = "(", want = "(";
    for (int k = 0; k < t->ndim; ++k) got += std::to_string(t->shape[k]) + (k + 1 < t->ndim ? ", " : "");
    i = 0;
    for (int64_t s : shape) want += std::to_string(s) + (++i < (int)shape.size() ? ", " : "");
    return fail(IKF_ERR_MISSING_TENSOR, "size mismatch for " + key + ": copying a param with shape " + got +
                                            ") from checkpoint, the shape in current model is " + want + ").");
  }
  *out = t;
  return IKF_OK;
}

static size_t align64(size_t n) { return (n + 63) & ~size_t(63); }  // 64 floats = 256 B

// split-32 images (same bytes as fp32) of every hidden Linear weight, converted on the device from the fp32 arena
ikf_status ikf::build_split_weights(ikf_model* m) {
  const FlowDims& d = m->dims;
  const int NB = m->desc.nb_nodes, W = d.width;
  if (m->split_arena || d.n_hidden < 2 || W % 128 != 0 || !m->loaded) return IKF_OK;
  const size_t per = (size_t)W * W * 2;  // uint16 elements per layer
  const size_t n_layers = (size_t)2 * NB * (d.n_hidden - 1);
  // the range word is shared with the activation guard: take what is pending out of it so that only the weight packs below
  // can set it, and put the pending bits back afterwards (they belong to ikf_split_overflow_pending)
  int pending_flag = 0;
  IKF_HIP(hipDeviceSynchronize());
  IKF_HIP(hipMemcpy(&pending_flag, m->d_split_flag, sizeof(int), hipMemcpyDeviceToHost));
  IKF_HIP(hipMemset(m->d_split_flag, 0, sizeof(int)));
  IKF_HIP(m->split_arena.ensure((long long)(per * n_layers)));
  m->w_mid_split.assign((size_t)2 * NB * 3, nullptr);
  size_t li = 0;
  for (int si = 0; si < 2 * NB; ++si)
    for (int l = 0; l < d.n_hidden - 1; ++l, ++li) {
      uint16_t* dst = m->split_arena + li * per;
      IKF_HIP(launch_split32_pack(m->subnets[si].w_mid[l], W, W, dst, m->d_split_flag, nullptr));
      m->w_mid_split[(size_t)si * 3 + l] = dst;
    }
  // fragment-major copies for the small-batch kernel (same bytes again)
  m->w_mid_split_frag.assign((size_t)2 * NB * 3, nullptr);
  if (split_cfg_needs_frag(split_pick_cfg(1, W))) {
    const size_t per_f = (size_t)W * W;  // dwords
    IKF_HIP(m->split_frag_arena.ensure((long long)(per_f * n_layers)));
    li = 0;
    for (int si = 0; si < 2 * NB; ++si)
      for (int l = 0; l < d.n_hidden - 1; ++l, ++li) {
        float* dstf = m->split_frag_arena + li * per_f;
        IKF_HIP(launch_wfrag_pack_split(m->w_mid_split[(size_t)si * 3 + l], W, W, dstf, nullptr));
        m->w_mid_split_frag[(size_t)si * 3 + l] = dstf;
      }
  }
  IKF_HIP(hipDeviceSynchronize());
  // a weight beyond the f16 range cannot be split: the mode is refused (the f32 path is unaffected)
  int wflag = 0;
  IKF_HIP(hipMemcpy(&wflag, m->d_split_flag, sizeof(int), hipMemcpyDeviceToHost));
  IKF_HIP(hipMemcpy(m->d_split_flag, &pending_flag, sizeof(int), hipMemcpyHostToDevice));
  if (wflag != 0) {
    m->split_arena.release();
    m->split_frag_arena.release();
    m->w_mid_split.assign((size_t)2 * NB * 3, nullptr);
    m->w_mid_split_frag.assign((size_t)2 * NB * 3, nullptr);
    m->precision = 0;
    return fail(IKF_ERR_BAD_ARGUMENT, "f16x3 precision refused: a hidden Linear weight is non-finite or exceeds the f16 range (65504); staying on f32");
  }
  return IKF_OK;
}

// fragment-major images (k_wfrag_pack) of every hidden Linear weight for k_flow_gemm_skinny (rows <= 512): the second
// copy costs width^2 * 4 B per layer (201 MB for the Panda model) of the 288 GB
static void drop_frag_weights(ikf_model* m) {
  m->wfrag_arena.release();
  m->w_mid_frag.assign((size_t)2 * m->desc.nb_nodes * 3, nullptr);
  m->wfrag_built = false;
}
ikf_status ikf::build_frag_weights(ikf_model* m) {
  const FlowDims& d = m->dims;
  const int NB = m->desc.nb_nodes, W = d.width;
  if (m->wfrag_built) return IKF_OK;
  const auto t0 = std::chrono::steady_clock::now();
  drop_frag_weights(m);
  m->wfrag_built = true;   // (also when the shape has no such image: nothing to build)
  if (d.n_hidden < 2 || fused_pick_cfg(512, W) != fused_skinny_cfg()) return IKF_OK;
  const size_t per = (size_t)W * W;
  const size_t n_layers = (size_t)2 * NB * (d.n_hidden - 1);
  IKF_HIP(m->wfrag_arena.ensure((long long)(per * n_layers)));
  size_t li = 0;
  for (int si = 0; si < 2 * NB; ++si)
    for (int l = 0; l < d.n_hidden - 1; ++l, ++li) {
      float* dst = m->wfrag_arena + li * per;
      IKF_HIP(launch_wfrag_pack(m->subnets[si].w_mid[l], W, W, dst, nullptr));
      m->w_mid_frag[(size_t)si * 3 + l] = dst;
    }
  IKF_HIP(hipDeviceSynchronize());
  m->chain_tab_valid = false;  // (the chain's argument table carries these pointers)
  m->frag_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return IKF_OK;
}

// the row-owner kernel's parameter stream: every subnet's weights in execution order (block NB-1 .. 0, s1 then s2) and, inside a subnet,
// in the order the kernel consumes them (k_rowowner_pack), plus the small per-subnet table (last-Linear bias, perm_inv, split)
static void drop_rowowner_stream(ikf_model* m) {
  m->ro_stream.release();
  m->d_ro_sub.release();
  m->d_ro_sub_fwd.release();
}
// The forward pass walks the same stream with the subnets in reverse order (k_flow_rowowner_fwd, ro_fwd_offset); its table lists them in
// forward execution order (block 0 .. NB-1, subnet 2 then subnet 1).  PermuteRandom forward of block b + 1 rides on block b's subnet-1 entry
// (identity on the last block); block 0's goes to the kernel as RoFwd::perm0.
static std::vector<RoSubnet> rowowner_fwd_table(const std::vector<RoSubnet>& inv, int NB, int D, const std::vector<int>& perm_fwd) {
  const int n_sub = 2 * NB;
  std::vector<RoSubnet> tab(n_sub);
  for (int s = 0; s < n_sub; ++s) {
    RoSubnet r = inv[n_sub - 1 - s];
    const int b = s / 2;
    for (int k = 0; k < 16; ++k) r.perm_inv[k] = (r.which == 1 && b + 1 < NB && k < D) ? perm_fwd[(size_t)(b + 1) * D + k] : k;
    tab[s] = r;
  }
  return tab;
}
// Nothing here is needed by the per-layer kernels: whatever fails (the second 203 MB, the census launch, the exchange buffers) leaves the
// handle WITHOUT the resident-row forms - rowowner_allowed / cluster_allowed test ro_stream - and ikf_load_weights still succeeds; the
// reason is kept for ikf_last_error.
static hipError_t build_rowowner_stream_hip(ikf_model* m, const std::vector<int>& perm_host, const std::vector<int>& perm_fwd) {
  const FlowDims& d = m->dims;
  const int NB = m->desc.nb_nodes, n_sub = 2 * NB;
  const size_t floats = rowowner_stream_floats(n_sub);
  hipError_t e = m->ro_stream.ensure((long long)floats);
  if (e != hipSuccess) return e;
  if ((e = hipMemset(m->ro_stream, 0, sizeof(float) * floats)) != hipSuccess) return e;
  if ((e = m->d_ro_sub.ensure(n_sub)) != hipSuccess) return e;
  std::vector<RoSubnet> tab(n_sub);
  for (int sidx = 0; sidx < n_sub; ++sidx) {
    const auto [b, which, si] = subnet_at(NB, sidx);
    const SubnetWeights& w = m->subnets[si];
    if ((e = launch_rowowner_pack(w, m->ro_stream + (size_t)sidx * rowowner_subnet_floats(), nullptr)) != hipSuccess) return e;
    RoSubnet& r = tab[sidx];
    memset(&r, 0, sizeof(r));
    if ((e = hipMemcpy(r.b_last, w.b_last, sizeof(float) * w.n_out, hipMemcpyDeviceToHost)) != hipSuccess) return e;
    for (int k = 0; k < 16; ++k) r.perm_inv[k] = k < d.D ? perm_host[(size_t)b * d.D + k] : k;
    r.which = which; r.n_x = w.n_x; r.x_off = which == 1 ? 0 : d.L1; r.n_half = w.n_out / 2;
  }
  if ((e = hipMemcpy(m->d_ro_sub, tab.data(), sizeof(RoSubnet) * n_sub, hipMemcpyHostToDevice)) != hipSuccess) return e;
  const std::vector<RoSubnet> fwd = rowowner_fwd_table(tab, NB, d.D, perm_fwd);
  if ((e = m->d_ro_sub_fwd.ensure(n_sub)) != hipSuccess) return e;
  if ((e = hipMemcpy(m->d_ro_sub_fwd, fwd.data(), sizeof(RoSubnet) * n_sub, hipMemcpyHostToDevice)) != hipSuccess) return e;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return e;
  // the XCD-local hand-over of the cluster form (G = 4 / 8 / 16) needs workgroups b and b + 8 k of a grid on one XCD: asked of the device once
  // (and checked again by every such launch among its own members)
  bool grouped = false;
  if ((e = cluster_placement_census(m->n_cu, &grouped)) != hipSuccess) return e;
  m->cl_census_ok = grouped ? 1 : 0;
  if (!grouped) m->cl_local = 0;
  return hipSuccess;
}
static ikf_status build_rowowner_stream(ikf_model* m, const std::vector<int>& perm_host, const std::vector<int>& perm_fwd) {
  const FlowDims& d = m->dims;
  const int n_sub = 2 * m->desc.nb_nodes;
  drop_rowowner_stream(m);
  if (!rowowner_shape_ok(d, n_sub) || d.slope < 0.f || d.slope > 1.f) return IKF_OK;
  if (rowowner_stream_floats(n_sub) * 4 >= (size_t)1 << 32) return IKF_OK;  // (one 32-bit buffer descriptor)
  hipError_t e = build_rowowner_stream_hip(m, perm_host, perm_fwd);
  // the cluster form's exchange buffers have one size (8 MB + 1.2 MB): reserved here, so that no call ever allocates for them
  if (e == hipSuccess && ensure_cluster_scratch(m, 1) != IKF_OK) e = hipErrorOutOfMemory;
  if (e != hipSuccess) {
    (void)hipGetLastError();   // (a refused allocation is sticky only until it is read)
    drop_rowowner_stream(m);
    (void)fail(IKF_ERR_HIP, std::string("ikf_load_weights: the resident-row forms are not available on this handle (") + hipGetErrorString(e) +
                                "); every batch size runs the per-layer kernels");
  }
  return IKF_OK;
}

extern "C" ikf_status ikf_load_weights(ikf_model* m, const ikf_tensor* tensors, int n_tensors) {
  if (!m || !tensors) return fail(IKF_ERR_NULL_POINTER, "ikf_load_weights: null argument");
  IKF_ON_DEVICE(m)
  const auto t_load0 = std::chrono::steady_clock::now();
  std::unordered_map<std::string, const ikf_tensor*> idx;
  for (int i = 0; i < n_tensors; ++i)
    if (tensors[i].name) idx[tensors[i].name] = &tensors[i];

  const FlowDims& d = m->dims;
  const int D = d.D, W = d.width, NB = m->desc.nb_nodes, C = m->desc.dim_cond;
  const int Wu = m->desc.width;  // width of the tensors in the file; W >= Wu is the padded width the kernels run at
  const int n_lin = d.n_hidden + 1;

  // pass 1: sizes
  size_t total = 0;
  for (int b = 0; b < NB; ++b)
    for (int which = 1; which <= 2; ++which) {
      const int n_x = (which == 1) ? d.L1 : d.L2;
      const int n_out = 2 * ((which == 1) ? d.L2 : d.L1);
      total += align64((size_t)(n_x + 7) * W) + 2 * align64(W);           // first (transposed), soft column, bias
      total += (size_t)(d.n_hidden - 1) * (align64((size_t)W * W) + align64(W));
      total += align64((size_t)n_out * W) + align64(n_out);
    }
  std::vector<float> host(total, 0.f);
  std::vector<SubnetWeights> subs(2 * NB);
  std::vector<size_t> off_first(2 * NB), off_soft(2 * NB), off_bfirst(2 * NB), off_last(2 * NB), off_blast(2 * NB);
  std::vector<std::vector<size_t>> off_mid(2 * NB), off_bmid(2 * NB);
  std::vector<int> perm_host((size_t)NB * D);

  size_t cur = 0;
  for (int b = 0; b < NB; ++b) {
    const int moff = m->desc.sigmoid_on_output ? 1 : 0;
    const std::string pkey = "module_list." + std::to_string(2 * b + 1 + moff) + ".perm_inv";
    const ikf_tensor* tp = nullptr;
    ikf_status st = need(idx, pkey, 1, {D}, &tp);
    if (st != IKF_OK) return st;
    std::vector<char> seen(D, 0);
    for (int k = 0; k < D; ++k) {
      const int64_t v = static_cast<const int64_t*>(tp->h_data)[k];
      if (v < 0 || v >= D || seen[v]) return fail(IKF_ERR_MISSING_TENSOR, pkey + " is not a permutation of range(D)");
      seen[v] = 1;
      perm_host[(size_t)b * D + k] = (int)v;
    }
    for (int which = 1; which <= 2; ++which) {
      const int si = 2 * b + which - 1;
      const int n_x = (which == 1) ? d.L1 : d.L2;
      const int n_out = 2 * ((which == 1) ? d.L2 : d.L1);
      const std::string base = "module_list." + std::to_string(2 * b + 2 + moff) + ".subnet" + std::to_string(which) + ".";
      // first Linear: weight [W][n_x + C] -> transposed [n_x + 7][W] (+ softflow column apart)
      const ikf_tensor *tw = nullptr, *tb = nullptr;
      st = need(idx, base + "0.weight", 0, {Wu, n_x + C}, &tw);
      if (st != IKF_OK) return st;
      st = need(idx, base + "0.bias", 0, {Wu}, &tb);
      if (st != IKF_OK) return st;
      const float* w0 = static_cast<const float*>(tw->h_data);
      off_first[si] = cur;
      for (int k = 0; k < n_x + 7; ++k)
        for (int c = 0; c < Wu; ++c) host[cur + (size_t)k * W + c] = w0[(size_t)c * (n_x + C) + k];
      cur += align64((size_t)(n_x + 7) * W);
      off_soft[si] = cur;
      if (C == 8)
        for (int c = 0; c < Wu; ++c) host[cur + c] = w0[(size_t)c * (n_x + C) + n_x + 7];
      cur += align64(W);
      off_bfirst[si] = cur;
      memcpy(&host[cur], tb->h_data, sizeof(float) * Wu);
      cur += align64(W);
      for (int l = 1; l < d.n_hidden; ++l) {
        st = need(idx, base + std::to_string(2 * l) + ".weight", 0, {Wu, Wu}, &tw);
        if (st != IKF_OK) return st;
        st = need(idx, base + std::to_string(2 * l) + ".bias", 0, {Wu}, &tb);
        if (st != IKF_OK) return st;
        off_mid[si].push_back(cur);
        for (int r = 0; r < Wu; ++r)
          memcpy(&host[cur + (size_t)r * W], static_cast<const float*>(tw->h_data) + (size_t)r * Wu, sizeof(float) * Wu);
        cur += align64((size_t)W * W);
        off_bmid[si].push_back(cur);
        memcpy(&host[cur], tb->h_data, sizeof(float) * Wu);
        cur += align64(W);
      }
      st = need(idx, base + std::to_string(2 * (n_lin - 1)) + ".weight", 0, {n_out, Wu}, &tw);
      if (st != IKF_OK) return st;
      st = need(idx, base + std::to_string(2 * (n_lin - 1)) + ".bias", 0, {n_out}, &tb);
      if (st != IKF_OK) return st;
      off_last[si] = cur;
      for (int r = 0; r < n_out; ++r)
        memcpy(&host[cur + (size_t)r * W], static_cast<const float*>(tw->h_data) + (size_t)r * Wu, sizeof(float) * Wu);
      cur += align64((size_t)n_out * W);
      off_blast[si] = cur;
      memcpy(&host[cur], tb->h_data, sizeof(float) * n_out);
      cur += align64(n_out);
      subs[si].n_x = n_x;
      subs[si].n_out = n_out;
    }
  }
  if (cur != total) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_load_weights: internal packing size mismatch");

  const ikf_tensor* tM = nullptr;
  ikf_status st = need(idx, "module_list.0.M_inv", 0, {D, D}, &tM);
  if (st != IKF_OK) return st;
  std::vector<float> blin(D, 0.f);
  if (m->desc.sigmoid_on_output && !find_tensor(idx, "module_list.0.b"))  // the scaling node's offset is never zero
    return fail(IKF_ERR_MISSING_TENSOR, "Missing key(s) in state_dict: \"module_list.0.b\"");
  if (const ikf_tensor* tb = find_tensor(idx, "module_list.0.b")) {
    if (tb->dtype != 0 || !tb->h_data) return fail(IKF_ERR_MISSING_TENSOR, "module_list.0.b has the wrong dtype");
    int64_t numel = 1;
    for (int k = 0; k < tb->ndim; ++k) numel *= tb->shape[k];
    if (numel != D) return fail(IKF_ERR_MISSING_TENSOR, "size mismatch for module_list.0.b");
    memcpy(blin.data(), tb->h_data, sizeof(float) * D);
  }

  // forward pass: M (the file's, or the fp64 inverse of M_inv), logDetM = log|det M| in fp64, PermuteRandom forward tables
  std::vector<double> M64((size_t)D * D), Minv64((size_t)D * D);
  for (int k = 0; k < D * D; ++k) Minv64[k] = static_cast<const float*>(tM->h_data)[k];
  const ikf_tensor* tMf = find_tensor(idx, "module_list.0.M");
  if (tMf) {
    int64_t numel = 1;
    for (int k = 0; k < tMf->ndim; ++k) numel *= tMf->shape[k];
    if (tMf->dtype != 0 || !tMf->h_data || numel != (int64_t)D * D) return fail(IKF_ERR_MISSING_TENSOR, "size mismatch for module_list.0.M");
    for (int k = 0; k < D * D; ++k) M64[k] = static_cast<const float*>(tMf->h_data)[k];
  }
  double log_det = 0.0;
  {
    // LU with partial pivoting of M (or of M_inv: log|det M| = -log|det M_inv|), fp64; M_inv is inverted on the side when M is absent
    std::vector<double> A = tMf ? M64 : Minv64;
    std::vector<double> X((size_t)D * D, 0.0);
    for (int k = 0; k < D; ++k) X[(size_t)k * D + k] = 1.0;
    for (int c = 0; c < D; ++c) {
      int p = c;
      for (int r = c + 1; r < D; ++r)
        if (fabs(A[(size_t)r * D + c]) > fabs(A[(size_t)p * D + c])) p = r;
      if (A[(size_t)p * D + c] == 0.0) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_load_weights: the FixedLinearTransform matrix is singular");
      if (p != c)
        for (int k = 0; k < D; ++k) {
          std::swap(A[(size_t)p * D + k], A[(size_t)c * D + k]);
          std::swap(X[(size_t)p * D + k], X[(size_t)c * D + k]);
        }
      log_det += log(fabs(A[(size_t)c * D + c]));
      for (int r = 0; r < D; ++r) {
        if (r == c) continue;
        const double f = A[(size_t)r * D + c] / A[(size_t)c * D + c];
        if (f == 0.0) continue;
        for (int k = 0; k < D; ++k) {
          A[(size_t)r * D + k] -= f * A[(size_t)c * D + k];
          X[(size_t)r * D + k] -= f * X[(size_t)c * D + k];
        }
      }
    }
    if (!tMf) {
      log_det = -log_det;
      for (int r = 0; r < D; ++r)
        for (int k = 0; k < D; ++k) M64[(size_t)r * D + k] = X[(size_t)r * D + k] / A[(size_t)r * D + r];
    }
  }
  // the inverse pass reports the Jacobian of the map it computes: log|det M_inv| from the f32 M_inv itself (M and M_inv of a file are
  // not exact inverses of each other), fp64 elimination with partial pivoting
  double log_det_inv = 0.0;
  {
    std::vector<double> A = Minv64;
    for (int c = 0; c < D; ++c) {
      int p = c;
      for (int r = c + 1; r < D; ++r)
        if (fabs(A[(size_t)r * D + c]) > fabs(A[(size_t)p * D + c])) p = r;
      if (A[(size_t)p * D + c] == 0.0) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_load_weights: module_list.0.M_inv is singular");
      if (p != c)
        for (int k = 0; k < D; ++k) std::swap(A[(size_t)p * D + k], A[(size_t)c * D + k]);
      log_det_inv += log(fabs(A[(size_t)c * D + c]));
      for (int r = c + 1; r < D; ++r) {
        const double f = A[(size_t)r * D + c] / A[(size_t)c * D + c];
        if (f == 0.0) continue;
        for (int k = c; k < D; ++k) A[(size_t)r * D + k] -= f * A[(size_t)c * D + k];
      }
    }
  }
  std::vector<float> M32((size_t)D * D);
  for (int k = 0; k < D * D; ++k) M32[k] = (float)M64[k];
  std::vector<int> perm_fwd((size_t)NB * D);
  for (int b = 0; b < NB; ++b)
    for (int k = 0; k < D; ++k) perm_fwd[(size_t)b * D + perm_host[(size_t)b * D + k]] = k;

  // upload
  m->arena.release();  // (a reload always reallocates: released first, so that ensure's grow-only test cannot keep the old array)
  IKF_HIP(m->d_perm_inv.ensure((long long)NB * D));
  IKF_HIP(m->d_Minv.ensure(D * D));
  IKF_HIP(m->d_M.ensure(D * D));
  IKF_HIP(m->d_perm.ensure((long long)NB * D));
  IKF_HIP(m->d_blin.ensure(D));
  IKF_HIP(m->arena.ensure((long long)total));
  m->arena_floats = total;
  IKF_HIP(hipMemcpy(m->arena, host.data(), sizeof(float) * total, hipMemcpyHostToDevice));
  IKF_HIP(hipMemcpy(m->d_perm_inv, perm_host.data(), sizeof(int) * (size_t)NB * D, hipMemcpyHostToDevice));
  IKF_HIP(hipMemcpy(m->d_Minv, tM->h_data, sizeof(float) * D * D, hipMemcpyHostToDevice));
  IKF_HIP(hipMemcpy(m->d_M, M32.data(), sizeof(float) * D * D, hipMemcpyHostToDevice));
  IKF_HIP(hipMemcpy(m->d_perm, perm_fwd.data(), sizeof(int) * (size_t)NB * D, hipMemcpyHostToDevice));
  m->log_det_M = (float)log_det;
  m->log_det_Minv = (float)log_det_inv;
  IKF_HIP(hipMemcpy(m->d_blin, blin.data(), sizeof(float) * D, hipMemcpyHostToDevice));
  for (int si = 0; si < 2 * NB; ++si) {
    SubnetWeights& s = subs[si];
    s.w_first_t = m->arena + off_first[si];
    s.w_soft = m->arena + off_soft[si];
    s.b_first = m->arena + off_bfirst[si];
    for (int l = 0; l < 3; ++l) {
      s.w_mid[l] = (l < (int)off_mid[si].size()) ? m->arena + off_mid[si][l] : nullptr;
      s.b_mid[l] = (l < (int)off_bmid[si].size()) ? m->arena + off_bmid[si][l] : nullptr;
    }
    s.w_last = m->arena + off_last[si];
    s.b_last = m->arena + off_blast[si];
  }
  m->subnets = subs;
  // the split-32 weight images of the f16-split contraction are built on the device when that mode is selected
  m->split_arena.release();
  m->split_frag_arena.release();
  m->w_mid_split.assign((size_t)2 * NB * 3, nullptr);
  m->w_mid_split_frag.assign((size_t)2 * NB * 3, nullptr);
  // The f32 images first and unconditionally: whatever happens to the f16x3 images below, every batch size of the f32 path
  // must see the NEW weights (the <= 512-row kernels read the fragment-major copy).
  m->loaded = false;
  m->chain_tab_valid = false;  // (the chain's argument table points into the weight arenas)
  drop_frag_weights(m);        // (rebuilt from the new arena by the first chunk that needs them, or by ikf_reserve)
  ikf_status fst = build_rowowner_stream(m, perm_host, perm_fwd);
  if (fst != IKF_OK) return fst;
  m->loaded = true;
  m->cl_back.forget();
  if (m->precision == 1) {
    ikf_status sst = build_split_weights(m);  // refusal: precision falls back to f32, the handle stays usable
    if (sst != IKF_OK) return sst;
  }
  IKF_HIP(hipDeviceSynchronize());
  m->load_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_load0).count();
  return IKF_OK;
}
// host wall time of the last ikf_load_weights (pack launches and the device-side images included) and of building the small-batch
// per-layer kernels' weight image (0 until a chunk or ikf_reserve needed it)
extern "C" double ikf_load_time_ms(const ikf_model* m) { return m ? m->load_ms : 0.0; }
extern "C" double ikf_frag_image_time_ms(const ikf_model* m) { return m ? m->frag_ms : 0.0; }
