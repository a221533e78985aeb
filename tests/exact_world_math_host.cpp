// Test harness (CPU): the arithmetic of exact IK under the exact collision rule - ikflow_amd/csrc/exact_world_math.h, the very source the GPU runs -
// compiled with g++ and driven row by row, so that tests/test_exact_world_math_host.py can hold it against a numpy statement of the definition
// without a GPU.  Not part of the product.
#include "../ikflow_amd/csrc/exact_world_math.h"

using ikf::Chain;
using ikf::CollisionModel;
using ikf::WorldObstacle;

static CollisionModel g_cm;
static WorldObstacle g_obs[IKF_WORLD_MAX_OBSTACLES];
static int g_n_obs = 0;

extern "C" int exact_world_host_chain_bytes() { return (int)sizeof(Chain); }

// capsules in engine frames (ikf_capsule) and index pairs, as ikf_set_collision_model takes them
extern "C" void exact_world_host_set_capsules(const ikf_capsule* caps, int n_caps, const int32_t* pairs, int n_pairs) {
  g_cm = CollisionModel{};
  g_cm.n_caps = n_caps;
  g_cm.n_pairs = n_pairs;
  for (int p = 0; p < n_pairs; ++p) { g_cm.pair_a[p] = (uint8_t)pairs[2 * p]; g_cm.pair_b[p] = (uint8_t)pairs[2 * p + 1]; }
  for (int c = 0; c < n_caps; ++c) {
    g_cm.frame[c] = caps[c].frame;
    g_cm.radius[c] = caps[c].radius;
    for (int i = 0; i < 3; ++i) { g_cm.p0[c][i] = caps[c].p0[i]; g_cm.p1[c][i] = caps[c].p1[i]; }
  }
}

// obstacles as the DEVICE reads them: normals and quaternions already of unit length (the caller normalises in fp64, as ikf_set_world does)
extern "C" int exact_world_host_set_world(const ikf_obstacle* obs, int n) {
  if (n < 0 || n > IKF_WORLD_MAX_OBSTACLES) return 1;
  g_n_obs = n;
  for (int i = 0; i < n; ++i) {
    g_obs[i] = WorldObstacle{};
    g_obs[i].kind = obs[i].kind;
    g_obs[i].radius = obs[i].radius;
    for (int c = 0; c < 3; ++c) { g_obs[i].a[c] = obs[i].a[c]; g_obs[i].b[c] = obs[i].b[c]; }
    for (int c = 0; c < 4; ++c) g_obs[i].quat[c] = obs[i].quat[c];
  }
  return 0;
}

template <int N>
static void rows(const Chain* ch, const float* q, long long n, int use_world, float world_min, int reject_self, float self_min, uint8_t* rejected,
                 float* world_cl, float* self_cl) {
  float w[IKF_MAX_CAPSULES * 6 + 1];
  for (long long r = 0; r < n; ++r) {
    rejected[r] = ikf::exact_row_rejected<N>(ch, &g_cm, g_obs, use_world ? g_n_obs : 0, world_min, reject_self != 0, self_min, q + r * N, w) ? 1 : 0;
    // the clearances on their own, through the functions exact_row_rejected calls
    self_cl[r] = ikf::capsule_clearance<N>(ch, &g_cm, q + r * N, w);
    world_cl[r] = ikf::world_clearance(g_obs, g_n_obs, &g_cm, w).clearance;
  }
}

// exact_row_rejected of n configurations under the capsules and (use_world) the world set above, and the two clearances of every row
extern "C" int exact_world_host_rows(const void* chain, const float* q, long long n, int use_world, float world_min, int reject_self, float self_min,
                                     uint8_t* rejected, float* world_cl, float* self_cl) {
  const Chain* ch = static_cast<const Chain*>(chain);
  switch (ch->ndof) {
    case 4: rows<4>(ch, q, n, use_world, world_min, reject_self, self_min, rejected, world_cl, self_cl); return 0;
    case 5: rows<5>(ch, q, n, use_world, world_min, reject_self, self_min, rejected, world_cl, self_cl); return 0;
    case 6: rows<6>(ch, q, n, use_world, world_min, reject_self, self_min, rejected, world_cl, self_cl); return 0;
    case 7: rows<7>(ch, q, n, use_world, world_min, reject_self, self_min, rejected, world_cl, self_cl); return 0;
    case 8: rows<8>(ch, q, n, use_world, world_min, reject_self, self_min, rejected, world_cl, self_cl); return 0;
    default: return 1;
  }
}

// the admissibility predicate on clearance tables [rows], and the cloud rule's mask applied to row_valid_iter in place (as k_exact_mask_rows does);
// -> rows the mask rejected
extern "C" void exact_world_host_predicate(long long rows, int has_world, const float* world_cl, float world_min, int has_cloud, const float* cloud_cl,
                                           float cloud_min, int reject_self, const float* self_cl, float self_min, uint8_t* rejected) {
  for (long long r = 0; r < rows; ++r)
    rejected[r] = ikf::exact_clearances_rejected(has_world != 0, world_cl[r], world_min, has_cloud != 0, cloud_cl[r], cloud_min, reject_self != 0,
                                                 self_cl[r], self_min) ? 1 : 0;
}
extern "C" long long exact_world_host_mask(long long rows, uint8_t* row_valid_iter, const float* cloud_cl, float cloud_min) {
  long long count = 0;
  for (long long r = 0; r < rows; ++r)
    if (ikf::exact_cloud_rejected(row_valid_iter[r], cloud_cl[r], cloud_min)) { row_valid_iter[r] = 0; ++count; }
  return count;
}
// the selection over a masked table: winner[j] = the repeat, -1: none
extern "C" void exact_world_host_select(const uint8_t* row_valid_iter, long long n_active, int repeat, int* winner) {
  for (long long j = 0; j < n_active; ++j) winner[j] = ikf::exact_select_repeat(row_valid_iter, n_active, repeat, j);
}

// launch geometry
extern "C" int exact_world_host_threads() { return ikf::IKF_EXACT_WORLD_THREADS; }
extern "C" long long exact_world_host_blocks(long long rows) { return ikf::exact_world_blocks(rows); }
extern "C" int exact_world_host_cap_stride(int n_caps) { return ikf::exact_world_cap_stride(n_caps); }
extern "C" long long exact_world_host_lds_bytes(int n_obs, int n_caps) { return (long long)ikf::exact_world_lds_bytes(n_obs, n_caps); }
