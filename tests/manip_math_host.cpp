// Test harness (CPU): the arithmetic of the singularity rule - ikflow_amd/csrc/manip_math.h, the very source the GPU runs - compiled with g++ and
// driven row by row, so that tests/test_manip_math_host.py can hold it against an fp64 singular-value reference without a GPU.  Not part of the
// product.
#include "../ikflow_amd/csrc/manip_math.h"

using ikf::Chain;

extern "C" int manip_host_chain_bytes() { return (int)sizeof(Chain); }
extern "C" int manip_host_part(int which) { return which == 0 ? IKF_MANIP_FULL : which == 1 ? IKF_MANIP_LINEAR : IKF_MANIP_ANGULAR; }

template <int N>
static void rows(const Chain* ch, const float* q, long long n, int part, float floor, float* w_out, unsigned char* below_out) {
  for (long long r = 0; r < n; ++r) {
    float qv[N];
    for (int d = 0; d < N; ++d) qv[d] = q[r * N + d];
    const float w = ikf::manip_row<N>(ch, qv, part);
    w_out[r] = w;
    below_out[r] = ikf::manip_below(w, floor) ? 1 : 0;
  }
}

// the rows of q [n][ndof]: the measure of `part` and the rule against `floor`
extern "C" int manip_host_rows(const void* chain, const float* q, long long n, int part, float floor, float* w_out, unsigned char* below_out) {
  const Chain* ch = static_cast<const Chain*>(chain);
  switch (ch->ndof) {
    case 4: rows<4>(ch, q, n, part, floor, w_out, below_out); return 0;
    case 5: rows<5>(ch, q, n, part, floor, w_out, below_out); return 0;
    case 6: rows<6>(ch, q, n, part, floor, w_out, below_out); return 0;
    case 7: rows<7>(ch, q, n, part, floor, w_out, below_out); return 0;
    case 8: rows<8>(ch, q, n, part, floor, w_out, below_out); return 0;
    default: return 1;
  }
}
