// Singularity rule for gfx950 (include/ikflow_amd_manip.h; the arithmetic: manip_math.h): the manipulability measure of every row's configuration.
//
// k_manip_rows: a thread per row, blocks of 256.  The row's chain walk, the Gram matrix of its Jacobian and the Cholesky pivots are fp64 and stay
// in registers (no LDS, no scratch at any chain length: profiles/manip_kernel_resources.txt); a row costs ndof sincos and a few hundred fp64
// multiply-adds, which is nothing beside the ranking launch that follows it.  Three sinks, each nullable: the measure, the verdict, and the
// rows' GATE - the one float per row that k_rank_candidates compares with a threshold (RankArgs::cloud_clearance): a row below the floor gets
// -inf there, a passing row keeps what the buffer holds (gate_keep: the cloud clearance that run_cloud_clearance has just written) or gets +inf.
// No atomics, no inline assembly.  Rows beyond n do nothing.
#include "ikf_internal.h"

namespace ikf {

template <int NDOF>
__global__ __launch_bounds__(256) void k_manip_rows(const Chain* __restrict__ ch, const float* __restrict__ q, long long n, int part, float floor,
                                                    float* __restrict__ w_out, uint8_t* __restrict__ below_out, float* __restrict__ gate,
                                                    int gate_keep) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  float qv[NDOF];
  load_q<NDOF>(q, row, qv);
  const float w = manip_row<NDOF>(ch, qv, part);
  const bool below = manip_below(w, floor);
  if (w_out) w_out[row] = w;
  if (below_out) below_out[row] = below ? 1 : 0;
  if (gate) {
    if (below) gate[row] = -INFINITY;
    else if (!gate_keep) gate[row] = INFINITY;
  }
}

hipError_t launch_manip_rows(const Chain* ch, int ndof, const float* q, long long n, int part, float floor, float* w_out, uint8_t* below_out,
                             float* gate, int gate_keep, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (!ch || !q || part < IKF_MANIP_FULL || part > IKF_MANIP_ANGULAR || n > 0x7fffffffLL * 256) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + 255) / 256));
  IKF_NDOF_DISPATCH(ndof, hipLaunchKernelGGL((k_manip_rows<ND>), grid, dim3(256), 0, s, ch, q, n, part, floor, w_out, below_out, gate, gate_keep));
  return hipGetLastError();
}

}  // namespace ikf
