// C-ABI of libikflow_amd.so, singularity rule (include/ikflow_amd_manip.h): the floor as state of the handle and the per-row query
// (k_manip_rows, manip_kernels.hip).  What the floor does to the selection entry points is in score_candidates (api_rank.hip).
#include "ikf_model.h"

static bool manip_part_ok(int part) { return part >= IKF_MANIP_FULL && part <= IKF_MANIP_ANGULAR; }

extern "C" ikf_status ikf_set_min_manipulability(ikf_model* m, int part, float min_manipulability) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_set_min_manipulability: null model");
  if (!manip_part_ok(part)) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_min_manipulability: part must be in 0 .. 2");
  if (!std::isfinite(min_manipulability) || min_manipulability < 0.f)
    return fail(IKF_ERR_BAD_ARGUMENT, "ikf_set_min_manipulability: min_manipulability must be finite and >= 0");
  m->manip_part = part;
  m->manip_min = min_manipulability;
  return IKF_OK;
}

extern "C" ikf_status ikf_min_manipulability(const ikf_model* m, int* part_out, float* min_out) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_min_manipulability: null model");
  if (part_out) *part_out = m->manip_part;
  if (min_out) *min_out = m->manip_min;
  return IKF_OK;
}

extern "C" ikf_status ikf_manipulability(ikf_model* m, const float* d_q, int64_t n, int part, float min_manipulability, float* d_w_out,
                                         uint8_t* d_below_out, void* stream) {
  if (!m) return fail(IKF_ERR_NULL_POINTER, "ikf_manipulability: null model");
  if (n < 0) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_manipulability: n must be >= 0");
  if (!manip_part_ok(part)) return fail(IKF_ERR_BAD_ARGUMENT, "ikf_manipulability: part must be in 0 .. 2");
  if (!std::isfinite(min_manipulability) || min_manipulability < 0.f)
    return fail(IKF_ERR_BAD_ARGUMENT, "ikf_manipulability: min_manipulability must be finite and >= 0");
  if (n == 0) return IKF_OK;
  if (!d_q) return fail(IKF_ERR_NULL_POINTER, "ikf_manipulability: null device pointer");
  if (!d_w_out && !d_below_out) return fail(IKF_ERR_NULL_POINTER, "ikf_manipulability: both outputs are null");
  IKF_ON_DEVICE(m)
  // (reads the chain alone, none of the handle's scratch: no stream scope)
  IKF_HIP(launch_manip_rows(m->d_chain, m->dims.ndof, d_q, n, part, min_manipulability, d_w_out, d_below_out, nullptr, 0,
                            static_cast<hipStream_t>(stream)));
  return IKF_OK;
}
