// Diverse-of-K IK for gfx950 (include/ikflow_amd_diverse.h): k candidate rows per target pose - the flow's samples, or the caller's - and of the
// admissible ones up to n_keep that are far apart in joint space, by greedy farthest-point selection.  The arithmetic is diverse_math.h; this
// kernel only places it.
//
// Row scores: k_rank_candidates itself (rank_kernels.hip), launched by api_diverse.hip with n_keep = 1 - the ranking's row score of every
//   candidate row, bit for bit, because it is the same kernel - writes score[k n_poses].
// k_diverse_select: ONE workgroup per pose, diverse_block(k) = 64 / 128 / 256 threads (k <= 256 / 512 / 1024).  The pose's k rows are gathered
//   once into LDS (row stride NDOF | 1 floats: lanes that read the same joint of consecutive rows hit different banks) with their scores.
//   Thread t owns the candidates t, t + B, t + 2 B, t + 3 B and keeps their near2 in registers.  Slot 0 is the lowest (score, r).  Every later
//   round: all threads read the last pick's row from LDS (a broadcast), update the near2 of their candidates, take their local best in the
//   order (greater near2, lower r), and the workgroup reduces - __shfl_xor over the 64 lanes of a wave, one LDS word pair per wave between
//   waves (double buffered on the round's parity: one barrier per round, none with a single wave).  Every thread ends a round with the same
//   pick, so the stop rule is uniform and the barriers are too.  At most 15 rounds; the run time is bounded by k and n_keep alone: no atomics,
//   nothing exchanged between workgroups, no wait loop, nothing read by the host.
// LDS (dynamic): k x ((NDOF | 1) + 1) floats, 40 KiB at k = 1024 and 8 joints, + 80 B static for the wave hand-over.
#include "ikf_internal.h"

namespace ikf {

constexpr int kDiverseWaves = IKF_DIVERSE_MAX_BLOCK / 64;

template <int NDOF>
__global__ __launch_bounds__(IKF_DIVERSE_MAX_BLOCK) void k_diverse_select(const DiverseArgs a) {
  extern __shared__ float dv_lds[];
  __shared__ float s_part_v[2][kDiverseWaves];   // [parity of the round][wave]: the waves' bests ...
  __shared__ int s_part_r[2][kDiverseWaves];
  __shared__ int s_part_cnt[kDiverseWaves];      // ... and their admissible candidates
  constexpr int RS = NDOF | 1;
  const int tid = threadIdx.x, B = blockDim.x, lane = tid & 63, wave = tid >> 6, waves = B >> 6;
  const long long j = blockIdx.x, n = a.n;
  const int k = a.k, nk = a.n_keep;
  float* const rows = dv_lds;             // [k][RS]
  float* const sc = dv_lds + k * RS;      // [k]

  for (int i = tid; i < k * NDOF; i += B) {
    const int r = i / NDOF, d = i - r * NDOF;
    rows[r * RS + d] = a.q[((long long)r * n + j) * NDOF + d];
  }
  for (int r = tid; r < k; r += B) sc[r] = a.score[(long long)r * n + j];
  float w[NDOF];
#pragma unroll
  for (int d = 0; d < NDOF; ++d) w[d] = a.w ? a.w[d] : 1.f;
  const bool weighted = a.w != nullptr;
  const float sep2 = diverse_sep2(a.min_separation);
  __syncthreads();

  // slot 0: the lowest (score, r) of the admissible candidates, and their number
  float near2[IKF_DIVERSE_PER_THREAD];
  bool alive[IKF_DIVERSE_PER_THREAD];
  DiverseFirst first = diverse_first_none();
  int count = 0;
#pragma unroll
  for (int c = 0; c < IKF_DIVERSE_PER_THREAD; ++c) {
    const int r = tid + c * B;
    near2[c] = rank_inf();
    alive[c] = r < k && sc[r < k ? r : 0] < rank_inf();
    if (alive[c]) {
      diverse_first_offer(first, sc[r], r);
      ++count;
    }
  }
  for (int off = 1; off < 64; off <<= 1) {
    DiverseFirst o;
    o.s = __shfl_xor(first.s, off);
    o.r = __shfl_xor(first.r, off);
    diverse_first_merge(first, o);
    count += __shfl_xor(count, off);
  }
  if (waves > 1) {
    if (lane == 0) {
      s_part_v[0][wave] = first.s;
      s_part_r[0][wave] = first.r;
      s_part_cnt[wave] = count;
    }
    __syncthreads();
    first = diverse_first_none();
    count = 0;
    for (int v = 0; v < waves; ++v) {
      diverse_first_merge(first, DiverseFirst{s_part_v[0][v], s_part_r[0][v]});
      count += s_part_cnt[v];
    }
  }

  int kept = 0;
  int p = first.r;   // the last pick; every thread holds the same value
  if (count > 0) {
    const long long slot = j * nk;
    if (tid < NDOF) a.q_out[slot * NDOF + tid] = rows[p * RS + tid];
    if (tid == 0) {
      if (a.score_out) a.score_out[slot] = sc[p];
      a.index_out[slot] = p;
      if (a.sep_out) a.sep_out[slot] = rank_inf();
    }
    kept = 1;
    for (int i = 1; i < nk; ++i) {
      float pr[NDOF];
#pragma unroll
      for (int d = 0; d < NDOF; ++d) pr[d] = rows[p * RS + d];
      DiverseBest best = diverse_none();
#pragma unroll
      for (int c = 0; c < IKF_DIVERSE_PER_THREAD; ++c) {
        const int r = tid + c * B;
        if (alive[c] && r == p) alive[c] = false;
        if (alive[c]) {
          const float d2 = weighted ? diverse_dist2<NDOF>(rows + r * RS, pr, w) : diverse_dist2<NDOF>(rows + r * RS, pr, nullptr);
          near2[c] = diverse_near2(near2[c], d2);
          diverse_offer(best, near2[c], r);
        }
      }
      for (int off = 1; off < 64; off <<= 1) {
        DiverseBest o;
        o.n = __shfl_xor(best.n, off);
        o.r = __shfl_xor(best.r, off);
        diverse_merge(best, o);
      }
      if (waves > 1) {
        const int par = i & 1;
        if (lane == 0) {
          s_part_v[par][wave] = best.n;
          s_part_r[par][wave] = best.r;
        }
        __syncthreads();
        best = diverse_none();
        for (int v = 0; v < waves; ++v) diverse_merge(best, DiverseBest{s_part_v[par][v], s_part_r[par][v]});
      }
      if (diverse_stop(best, sep2)) break;
      p = best.r;
      const long long sl = slot + i;
      if (tid < NDOF) a.q_out[sl * NDOF + tid] = rows[p * RS + tid];
      if (tid == 0) {
        if (a.score_out) a.score_out[sl] = sc[p];
        a.index_out[sl] = p;
        if (a.sep_out) a.sep_out[sl] = sqrtf(best.n);
      }
      kept = i + 1;
    }
  }
  // the unfilled slots
  const long long free0 = j * nk + kept;
  for (int e = tid; e < (nk - kept) * NDOF; e += B) a.q_out[free0 * NDOF + e] = 0.f;
  for (int e = tid; e < nk - kept; e += B) {
    if (a.score_out) a.score_out[free0 + e] = rank_inf();
    a.index_out[free0 + e] = -1;
    if (a.sep_out) a.sep_out[free0 + e] = rank_inf();
  }
  if (tid == 0) {
    if (a.kept_out) a.kept_out[j] = kept;
    if (a.count_out) a.count_out[j] = count;
  }
}

hipError_t launch_diverse_select(int ndof, const DiverseArgs& a, hipStream_t s) {
  if (a.n < 1 || a.k < 1 || a.k > IKF_DIVERSE_MAX_K || a.n_keep < 1 || a.n_keep > IKF_DIVERSE_MAX_KEEP || a.n_keep > a.k ||
      (long long)a.k * a.n > 0x7fffffffLL || !a.q || !a.score || !a.q_out || !a.index_out)
    return hipErrorInvalidValue;
  const int block = diverse_block(a.k);
  IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_diverse_select<ND>), dim3((unsigned)a.n), dim3(block), diverse_lds_bytes(ND, a.k), s, a);
                    return hipGetLastError());
  return hipErrorInvalidValue;
}

}  // namespace ikf
