// Path IK for gfx950 (include/ikflow_amd_path.h): T waypoints, k candidate rows per waypoint - the flow's samples under k latents held fixed
// along the path (what the reference's visualizations.py oscillate_target(fixed_latent=True) draws), or the caller's - and the cheapest path
// through the k x T lattice, by dynamic programming.  The arithmetic is path_math.h; these kernels only place it.
//
// k_path_expand_latent: [k x D] -> [k T x D] tile-major, so that the flow's latent source stays what it is.
// Node costs: k_rank_candidates itself (rank_kernels.hip), launched by api_path.hip with the waypoints as its poses and n_keep = 1 - the
//   ranking's row score of every candidate row, bit for bit, because it is the same kernel - writes node[k T].
// k_path_lattice: the sequential part, ONE workgroup of 256 threads.  The rows of IKF_PATH_STAGE waypoints are loaded together (per candidate a
//   segment of STAGE * ndof contiguous floats, adjacent lanes adjacent addresses) into LDS rows of 8 floats, double buffered: the loads of the
//   next stage are in flight while this one is relaxed.  Thread = (destination r = thread % span, slice = thread / span) with span the next
//   power of two >= k; a slice walks the predecessors slice, slice + S, ... - its lanes read the same predecessor row (an LDS broadcast, two
//   128-bit reads).  The slices' minima are merged by __shfl_xor inside a wave and through LDS between waves, under the total order (lower sum,
//   lower j): every split gives the same node.  Back-pointers: a byte per node in the handle's scratch.  The walk back stages
//   IKF_PATH_BT_CHUNK waypoints of back-pointers into LDS with coalesced loads and follows them there; the chosen rows of a chunk are then
//   gathered by all threads.  No atomics, no second workgroup, nothing read by the host.
// LDS of the lattice workgroup (static): rows 2 x STAGE x 256 x 32 B = 32 KiB (reused by the walk back: 64 x 256 B = 16 KiB), node costs 4 KiB,
// accumulated costs 2 KiB, wave hand-over 2 KiB: 40.3 KiB of a CU's 160 KiB.
// SWEEP (a sweep is set on the handle and there is something to test against, include/ikflow_amd_sweep.h): PathArgs::edge_free holds the verdicts
//   of k_sweep_edges, a bit per edge.  A thread keeps the (k + 63) / 64 words of its destination for the waypoints of the running stage in
//   registers; those of the next stage are loaded with the stage prefetch that is in flight anyway, not on the sequential chain (at most
//   4 x 64 bit per thread and waypoint).  Bit j is tested before predecessor j is offered to path_relax, bit 0 of row 0 before path_start with
//   a q_start.  SWEEP = false is the kernel as it was.
// BATCH (include/ikflow_amd_path_batch.h): P paths of T waypoints in one candidate layout of P * T waypoints, grid = P, ONE workgroup per path with
//   the geometry and the LDS plan above.  Workgroup p shifts its arguments to its own path (path_batch_view: waypoints p T .. p T + T - 1, its
//   q_start, its block of back-pointers, its outputs, its mask words) and runs the single path's code with the batch's row stride P T - the
//   waypoints of a path stay adjacent, so a stage is still k contiguous segments.  No workgroup reads what another writes; no atomics.
//   BATCH = false is the kernel as it was.
#include "ikf_internal.h"

namespace ikf {

__global__ __launch_bounds__(256) void k_path_expand_latent(const float* __restrict__ in, int k, long long T, int D, float* __restrict__ out) {
  const long long total = (long long)k * T * D;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / D;
    const int d = (int)(i - row * D);
    out[i] = in[(row / T) * D + d];
  }
}

constexpr int kPathRowVecs = 2 * IKF_PATH_STAGE * IKF_PATH_BLOCK * (IKF_PATH_ROW / 4);   // float4s of the two row buffers
constexpr size_t kPathLatticeLds = sizeof(float) * (4 * (size_t)kPathRowVecs + 2 * IKF_PATH_STAGE * IKF_PATH_BLOCK + 2 * IKF_PATH_BLOCK + 2 * IKF_PATH_BLOCK +
                                                    8 + IKF_PATH_BT_CHUNK + 1);
static_assert(kPathLatticeLds <= 64 * 1024, "the lattice workgroup's static LDS");
static_assert((size_t)IKF_PATH_BT_CHUNK * IKF_PATH_MAX_K + 4 <= sizeof(float) * 4 * (size_t)kPathRowVecs, "a chunk of back-pointers must fit the row buffers");

// the rows and node costs of waypoints t0 .. t0 + wn - 1 into registers: element i = thread + 256 u of the k segments of wn * NDOF floats;
// `stride`: waypoints between two candidates of one waypoint (T; P * T in a batch, where consecutive waypoints of a path are still adjacent)
template <int NDOF>
__device__ __forceinline__ void path_stage_load(const PathArgs& a, long long stride, long long t0, int wn, float (&pre)[IKF_PATH_STAGE * NDOF],
                                                float (&prn)[IKF_PATH_STAGE]) {
  const int seg = wn * NDOF;
#pragma unroll
  for (int u = 0; u < IKF_PATH_STAGE * NDOF; ++u) {
    const int i = (int)threadIdx.x + IKF_PATH_BLOCK * u;
    const int r = i / seg, e = i - r * seg;
    pre[u] = r < a.k ? a.q[((long long)r * stride + t0) * NDOF + e] : 0.f;
  }
#pragma unroll
  for (int w = 0; w < IKF_PATH_STAGE; ++w) prn[w] = ((int)threadIdx.x < a.k && w < wn) ? a.node[(long long)threadIdx.x * stride + t0 + w] : rank_inf();
}
template <int NDOF>
__device__ __forceinline__ void path_stage_store(const PathArgs& a, int buf, int wn, const float (&pre)[IKF_PATH_STAGE * NDOF], const float (&prn)[IKF_PATH_STAGE],
                                                 float* rows, float* node) {
  const int seg = wn * NDOF;
#pragma unroll
  for (int u = 0; u < IKF_PATH_STAGE * NDOF; ++u) {
    const int i = (int)threadIdx.x + IKF_PATH_BLOCK * u;
    const int r = i / seg, e = i - r * seg;
    const int w = e / NDOF, d = e - w * NDOF;
    if (r < a.k) rows[((buf * IKF_PATH_STAGE + w) * IKF_PATH_BLOCK + r) * IKF_PATH_ROW + d] = pre[u];
  }
#pragma unroll
  for (int w = 0; w < IKF_PATH_STAGE; ++w) node[(buf * IKF_PATH_STAGE + w) * IKF_PATH_BLOCK + threadIdx.x] = prn[w];
}

constexpr int kPathMaskWords = (IKF_PATH_MAX_K + IKF_SWEEP_LANES - 1) / IKF_SWEEP_LANES;
// the mask words of destination r for waypoints t0 .. t0 + wn - 1 into registers
__device__ __forceinline__ void path_mask_load(const PathArgs& a, long long t0, int wn, int r, bool live, int words,
                                               unsigned long long (&m)[IKF_PATH_STAGE][kPathMaskWords]) {
#pragma unroll
  for (int w = 0; w < IKF_PATH_STAGE; ++w)
#pragma unroll
    for (int x = 0; x < kPathMaskWords; ++x) m[w][x] = (live && w < wn && x < words) ? a.edge_free[sweep_word_index(t0 + w, r, x, a.k)] : 0ULL;
}
// bit j of the words of waypoint w of the stage (selects, so that the words stay in registers)
__device__ __forceinline__ bool path_mask_bit(const unsigned long long (&m)[IKF_PATH_STAGE][kPathMaskWords], int w, int j) {
  unsigned long long word = 0ULL;
  const int x = j / IKF_SWEEP_LANES;
#pragma unroll
  for (int ww = 0; ww < IKF_PATH_STAGE; ++ww)
#pragma unroll
    for (int xx = 0; xx < kPathMaskWords; ++xx) word = (ww == w && xx == x) ? m[ww][xx] : word;
  return (word >> (j % IKF_SWEEP_LANES)) & 1ULL;
}

// What workgroup `p` of a batched launch works on: the arguments of its own path inside the layout of P * T waypoints (path_batch_math.h).  From
// here on the path is addressed as a single one with the batch's row stride.
template <int NDOF, bool SWEEP>
__device__ __forceinline__ PathArgs path_batch_view(const PathArgs& b, long long p) {
  PathArgs a = b;
  const long long g0 = path_batch_offset(p, b.T);
  a.q += g0 * NDOF;
  a.node += g0;
  if (a.q_start) a.q_start += p * NDOF;
  a.bp += path_batch_bp_offset(p, b.T, b.k);
  a.path_out += g0 * NDOF;
  a.index_out += g0;
  a.cost_out += p;
  if (a.reachable_out) a.reachable_out += g0;
  if constexpr (SWEEP) a.edge_free += path_batch_mask_offset(p, b.T, b.k);
  return a;
}

template <int NDOF, bool SWEEP, bool BATCH>
__global__ __launch_bounds__(IKF_PATH_BLOCK) void k_path_lattice(const PathArgs a0) {
  PathArgs view{};
  if constexpr (BATCH) view = path_batch_view<NDOF, SWEEP>(a0, blockIdx.x);
  const PathArgs& a = BATCH ? view : a0;
  const long long stride = BATCH ? path_batch_waypoints(a0.P, a0.T) : (long long)a0.T;   // waypoints between two candidates of a waypoint
  __shared__ float4 s_rows[kPathRowVecs];                               // [2][STAGE][256] rows of 8 floats
  __shared__ float s_node[2 * IKF_PATH_STAGE * IKF_PATH_BLOCK];        // [2][STAGE][256]
  __shared__ float s_cost[2 * IKF_PATH_BLOCK];                          // [parity of t][256]
  __shared__ float s_part_c[IKF_PATH_BLOCK];                            // the waves' partial minima
  __shared__ int s_part_j[IKF_PATH_BLOCK];
  __shared__ int s_wcnt[2 * 4];                                         // [parity of t][wave] reachable nodes
  __shared__ int s_idx[IKF_PATH_BT_CHUNK];
  __shared__ int s_carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = a.k;
  const long long T = a.T;
  const int kp = path_span(k), S = IKF_PATH_BLOCK / kp;
  const int r = tid & (kp - 1), sl = tid / kp;
  const bool live = r < k, owner = tid < k;                             // owner: slice 0 of destination r = tid
  const int wspan = kp > 64 ? kp : 64, ws = tid / wspan, wslices = IKF_PATH_BLOCK / wspan;   // slices of a destination that sit in different waves
  const float step = a.opt.max_joint_step, nw = a.opt.node_weight;
  float* const rows = reinterpret_cast<float*>(s_rows);

  for (int i = tid; i < kPathRowVecs; i += IKF_PATH_BLOCK) s_rows[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  float qs[IKF_PATH_ROW];
#pragma unroll
  for (int d = 0; d < IKF_PATH_ROW; ++d) qs[d] = (a.q_start && d < NDOF) ? a.q_start[d] : 0.f;
  __syncthreads();

  const long long nstage = path_stages(T);
  float pre[IKF_PATH_STAGE * NDOF], prn[IKF_PATH_STAGE];
  unsigned long long mask[IKF_PATH_STAGE][kPathMaskWords], mask_next[IKF_PATH_STAGE][kPathMaskWords];   // SWEEP: this stage's words, the next one's
  const int mwords = SWEEP ? sweep_words(k) : 0;
  (void)mask; (void)mask_next; (void)mwords;
  {
    const int wn0 = T < IKF_PATH_STAGE ? (int)T : IKF_PATH_STAGE;
    if constexpr (SWEEP) path_mask_load(a, 0, wn0, r, live, mwords, mask_next);
    path_stage_load<NDOF>(a, stride, 0, wn0, pre, prn);
    path_stage_store<NDOF>(a, 0, wn0, pre, prn, rows, s_node);
  }
  __syncthreads();

  for (long long s = 0; s < nstage; ++s) {
    const int cur = (int)(s & 1);
    const long long t0 = s * IKF_PATH_STAGE;
    const int wn = T - t0 < IKF_PATH_STAGE ? (int)(T - t0) : IKF_PATH_STAGE;
    const bool more = s + 1 < nstage;
    const int wn_next = !more ? 0 : (T - t0 - IKF_PATH_STAGE < IKF_PATH_STAGE ? (int)(T - t0 - IKF_PATH_STAGE) : IKF_PATH_STAGE);
    if constexpr (SWEEP) {
#pragma unroll
      for (int w = 0; w < IKF_PATH_STAGE; ++w)
#pragma unroll
        for (int x = 0; x < kPathMaskWords; ++x) mask[w][x] = mask_next[w][x];
      if (more) path_mask_load(a, t0 + IKF_PATH_STAGE, wn_next, r, live, mwords, mask_next);
    }
    if (more) path_stage_load<NDOF>(a, stride, t0 + IKF_PATH_STAGE, wn_next, pre, prn);   // in flight while this stage is relaxed
    for (int w = 0; w < wn; ++w) {
      const long long t = t0 + w;
      const int cb = (int)(t & 1), pb = cb ^ 1;
      float me[IKF_PATH_ROW];
      {
        const float4 lo = s_rows[((cur * IKF_PATH_STAGE + w) * IKF_PATH_BLOCK + r) * 2], hi = s_rows[((cur * IKF_PATH_STAGE + w) * IKF_PATH_BLOCK + r) * 2 + 1];
        me[0] = lo.x; me[1] = lo.y; me[2] = lo.z; me[3] = lo.w; me[4] = hi.x; me[5] = hi.y; me[6] = hi.z; me[7] = hi.w;
      }
      PathBest best = path_none();
      if (t == 0) {
        bool start_ok = true;
        if constexpr (SWEEP) start_ok = a.q_start == nullptr || path_mask_bit(mask, w, 0);
        if (live && sl == 0 && start_ok) best = path_start<NDOF>(qs, a.q_start != nullptr, me, step);
      } else if (live) {
        const int pbuf = w > 0 ? cur : cur ^ 1, pw = w > 0 ? w - 1 : IKF_PATH_STAGE - 1;   // waypoint t - 1: in this stage, or the last of the one before
        const float4* const pr = s_rows + (pbuf * IKF_PATH_STAGE + pw) * IKF_PATH_BLOCK * 2;
        const float* const pc = s_cost + pb * IKF_PATH_BLOCK;
        for (int j = sl; j < k; j += S) {
          if constexpr (SWEEP) {
            if (!path_mask_bit(mask, w, j)) continue;
          }
          const float4 lo = pr[2 * j], hi = pr[2 * j + 1];
          const float pj[IKF_PATH_ROW] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
          path_relax<NDOF>(best, pc[j], pj, j, me, step);
        }
      }
      // the slices of a destination that share this wave: lanes r, r + kp, ...
      for (int off = kp; off < 64; off <<= 1) {
        PathBest o;
        o.c = __shfl_xor(best.c, off);
        o.j = __shfl_xor(best.j, off);
        path_merge(best, o);
      }
      if (wslices > 1) {   // ... and those in other waves, through LDS
        if (lane < kp) {
          s_part_c[ws * kp + r] = best.c;
          s_part_j[ws * kp + r] = best.j;
        }
        __syncthreads();
        if (tid < kp) {
          for (int w2 = 1; w2 < wslices; ++w2) {
            const PathBest o{s_part_c[w2 * kp + r], s_part_j[w2 * kp + r]};
            path_merge(best, o);
          }
        }
      }
      bool reach = false;
      if (owner) {
        const float c = path_finish(best, s_node[(cur * IKF_PATH_STAGE + w) * IKF_PATH_BLOCK + tid], nw);
        s_cost[cb * IKF_PATH_BLOCK + tid] = c;
        reach = c < rank_inf();
        a.bp[t * k + tid] = (uint8_t)(reach ? best.j : 0);
      }
      const int cnt = __popcll(__ballot(reach));
      if (lane == 0) s_wcnt[cb * 4 + wave] = cnt;
      __syncthreads();
      if (tid == 0 && a.reachable_out) a.reachable_out[t] = s_wcnt[cb * 4] + s_wcnt[cb * 4 + 1] + s_wcnt[cb * 4 + 2] + s_wcnt[cb * 4 + 3];
    }
    if (more) path_stage_store<NDOF>(a, cur ^ 1, wn_next, pre, prn, rows, s_node);
    __syncthreads();
  }

  // the end of the path
  const float* const fc = s_cost + (int)((T - 1) & 1) * IKF_PATH_BLOCK;
  if (tid == 0) {
    const int e = path_argmin(fc, k);
    s_carry = e;
    a.cost_out[0] = e >= 0 ? fc[e] : rank_inf();
  }
  __syncthreads();
  if (s_carry < 0) {   // no path
    for (long long i = tid; i < T * NDOF; i += IKF_PATH_BLOCK) a.path_out[i] = 0.f;
    for (long long i = tid; i < T; i += IKF_PATH_BLOCK) a.index_out[i] = -1;
    return;
  }
  // the walk back, a chunk of back-pointer rows at a time (the row buffers are free now)
  uint8_t* const bpl = reinterpret_cast<uint8_t*>(s_rows);
  uint32_t* const bpw = reinterpret_cast<uint32_t*>(s_rows);
  for (long long c = path_bt_chunks(T) - 1; c >= 0; --c) {
    const long long tc = c * IKF_PATH_BT_CHUNK;
    const int n = T - tc < IKF_PATH_BT_CHUNK ? (int)(T - tc) : IKF_PATH_BT_CHUNK;
    __syncthreads();   // every reader of s_carry, s_idx and the staged chunk is done
    const uint32_t* const g = reinterpret_cast<const uint32_t*>(a.bp + tc * k);   // tc * k is a multiple of 64 (BATCH: from the path's own aligned block)
    const int words = (n * k + 3) / 4;                                            // (the scratch is padded: path_bp_bytes)
    for (int i = tid; i < words; i += IKF_PATH_BLOCK) bpw[i] = g[i];
    __syncthreads();
    if (tid == 0) s_carry = path_backtrack_chunk(bpl, k, n, s_carry, s_idx);
    __syncthreads();
    for (int i = tid; i < n; i += IKF_PATH_BLOCK) a.index_out[tc + i] = s_idx[i];
    for (int i = tid; i < n * NDOF; i += IKF_PATH_BLOCK) {
      const int w = i / NDOF, d = i - w * NDOF;
      a.path_out[(tc + w) * NDOF + d] = a.q[((long long)s_idx[w] * stride + tc + w) * NDOF + d];
    }
  }
}

hipError_t launch_path_expand_latent(const float* latent, int k, long long T, int D, float* out, hipStream_t s) {
  if (k < 1 || T < 1 || D < 1 || !latent || !out) return hipErrorInvalidValue;
  const long long total = (long long)k * T * D, blocks = (total + 255) / 256;
  hipLaunchKernelGGL(k_path_expand_latent, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, latent, k, T, D, out);
  return hipGetLastError();
}

static bool path_args_ok(const PathArgs& a) {
  const long long paths = a.P > 0 ? a.P : 1;
  return a.T >= 1 && a.k >= 1 && a.k <= IKF_PATH_MAX_K && a.P >= 0 && (long long)a.k * a.T * paths <= 0x7fffffffLL && a.q && a.node;
}

hipError_t launch_path_lattice(int ndof, const PathArgs& a, hipStream_t s) {
  if (!path_args_ok(a) || !a.bp || !a.path_out || !a.index_out || !a.cost_out) return hipErrorInvalidValue;
  if (a.P > 0) {   // batched: a workgroup per path (the grid's x extent holds any P that passed path_args_ok)
    const dim3 grid((unsigned)a.P);
    if (a.edge_free) {
      IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_path_lattice<ND, true, true>), grid, dim3(IKF_PATH_BLOCK), 0, s, a); return hipGetLastError());
      return hipErrorInvalidValue;
    }
    IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_path_lattice<ND, false, true>), grid, dim3(IKF_PATH_BLOCK), 0, s, a); return hipGetLastError());
    return hipErrorInvalidValue;
  }
  if (a.edge_free) {
    IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_path_lattice<ND, true, false>), dim3(1), dim3(IKF_PATH_BLOCK), 0, s, a); return hipGetLastError());
    return hipErrorInvalidValue;
  }
  IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_path_lattice<ND, false, false>), dim3(1), dim3(IKF_PATH_BLOCK), 0, s, a); return hipGetLastError());
  return hipErrorInvalidValue;
}

}  // namespace ikf
