// Test harness (CPU): the loop of one refined candidate row - ikflow_amd/csrc/refine_math.h over kin_math.h, the very source the GPU runs -
// compiled with g++ and driven row by row with the kernel's placement (the pose of row r is r % n_poses), so that tests/test_refine_math_host.py
// can hold it against a loop of the oracle without a GPU.  Not part of the product.
#include "../ikflow_amd/csrc/refine_math.h"

using ikf::Chain;

template <int N>
static void run(const Chain* ch, int f64, const float* poses, long long n_poses, const float* q, long long rows, int n_steps, float pos_tol,
                float rot_tol, float* q_out, unsigned char* steps_out, unsigned char* converged_out) {
  for (long long i = 0; i < rows; ++i) {
    float qv[N];
    for (int j = 0; j < N; ++j) qv[j] = q[i * N + j];
    int steps, converged;
    const float* tgt = poses + (i % n_poses) * 7;
    if (f64) ikf::refine_row<N, double>(ch, tgt, qv, n_steps, pos_tol, rot_tol, &steps, &converged);
    else ikf::refine_row<N, float>(ch, tgt, qv, n_steps, pos_tol, rot_tol, &steps, &converged);
    for (int j = 0; j < N; ++j) q_out[i * N + j] = qv[j];
    if (steps_out) steps_out[i] = (unsigned char)steps;
    if (converged_out) converged_out[i] = (unsigned char)converged;
  }
}

extern "C" int refine_math_host(const void* chain, int f64, const float* poses, long long n_poses, const float* q, long long rows, int n_steps,
                                float pos_tol, float rot_tol, float* q_out, unsigned char* steps_out, unsigned char* converged_out) {
  const Chain* ch = static_cast<const Chain*>(chain);
  if (n_poses < 1) return 1;
  switch (ch->ndof) {
    case 4: run<4>(ch, f64, poses, n_poses, q, rows, n_steps, pos_tol, rot_tol, q_out, steps_out, converged_out); return 0;
    case 5: run<5>(ch, f64, poses, n_poses, q, rows, n_steps, pos_tol, rot_tol, q_out, steps_out, converged_out); return 0;
    case 6: run<6>(ch, f64, poses, n_poses, q, rows, n_steps, pos_tol, rot_tol, q_out, steps_out, converged_out); return 0;
    case 7: run<7>(ch, f64, poses, n_poses, q, rows, n_steps, pos_tol, rot_tol, q_out, steps_out, converged_out); return 0;
    case 8: run<8>(ch, f64, poses, n_poses, q, rows, n_steps, pos_tol, rot_tol, q_out, steps_out, converged_out); return 0;
    default: return 1;
  }
}
extern "C" int refine_math_chain_bytes() { return (int)sizeof(Chain); }
extern "C" int refine_math_max_steps() { return IKF_REFINE_MAX_STEPS; }
extern "C" long long refine_math_blocks(long long rows) { return ikf::refine_blocks(rows); }
