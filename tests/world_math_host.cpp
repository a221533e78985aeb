// Test harness (CPU): the arithmetic of world collision - ikflow_amd/csrc/world_math.h, the very source the GPU runs - compiled with g++ and driven
// pair by pair / row by row, so that tests/test_world_math_host.py can hold it against an fp64 reference without a GPU.  Not part of the product.
#include "../ikflow_amd/csrc/world_math.h"

using ikf::Chain;
using ikf::CollisionModel;
using ikf::WorldObstacle;

static CollisionModel g_cm;
static WorldObstacle g_obs[IKF_WORLD_MAX_OBSTACLES];
static int g_n_obs = 0;

extern "C" int world_host_chain_bytes() { return (int)sizeof(Chain); }
extern "C" int world_host_obstacle_words() { return (int)(sizeof(WorldObstacle) / 4); }

// capsules in engine frames (ikf_capsule) and index pairs, as ikf_set_collision_model takes them (the world itself does not read the pairs)
extern "C" void world_host_set_capsules(const ikf_capsule* caps, int n_caps, const int32_t* pairs, int n_pairs) {
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
extern "C" int world_host_set_world(const ikf_obstacle* obs, int n) {
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

// n independent (obstacle i, capsule i) pairs: seg [n][6] the capsule's end points, rc [n] its radius -> the clearance of each pair
extern "C" void world_host_pairs(const ikf_obstacle* obs, const float* seg, const float* rc, long long n, float* out) {
  for (long long i = 0; i < n; ++i) {
    CollisionModel cm{};
    cm.n_caps = 1;
    cm.radius[0] = rc[i];
    world_host_set_world(obs + i, 1);
    out[i] = ikf::world_clearance(g_obs, 1, &cm, seg + 6 * i).clearance;
  }
  g_n_obs = 0;
}

// the world set above against n_caps capsules given by their end points (w [n_caps][6]) and radii: clearance and closest pair
extern "C" void world_host_hit(const float* w, const float* radius, int n_caps, float* clearance, int* obstacle, int* capsule) {
  CollisionModel cm{};
  cm.n_caps = n_caps;
  for (int c = 0; c < n_caps; ++c) cm.radius[c] = radius[c];
  const ikf::WorldHit h = ikf::world_clearance(g_obs, g_n_obs, &cm, w);
  *clearance = h.clearance;
  *obstacle = h.obstacle;
  *capsule = h.capsule;
}

template <int N>
static void rows(const Chain* ch, const float* q, long long n, float* clearance, int* obstacle, int* capsule) {
  float w[IKF_MAX_CAPSULES * 6];
  for (long long r = 0; r < n; ++r) {
    float qv[N];
    for (int d = 0; d < N; ++d) qv[d] = q[r * N + d];
    ikf::capsule_endpoints<N>(ch, &g_cm, qv, w);
    const ikf::WorldHit h = ikf::world_clearance(g_obs, g_n_obs, &g_cm, w);
    clearance[r] = h.clearance;
    obstacle[r] = h.obstacle;
    capsule[r] = h.capsule;
  }
}

// whole rows: the chain walk and the world set above
extern "C" int world_host_rows(const void* chain, const float* q, long long n, float* clearance, int* obstacle, int* capsule) {
  const Chain* ch = static_cast<const Chain*>(chain);
  switch (ch->ndof) {
    case 4: rows<4>(ch, q, n, clearance, obstacle, capsule); return 0;
    case 5: rows<5>(ch, q, n, clearance, obstacle, capsule); return 0;
    case 6: rows<6>(ch, q, n, clearance, obstacle, capsule); return 0;
    case 7: rows<7>(ch, q, n, clearance, obstacle, capsule); return 0;
    case 8: rows<8>(ch, q, n, clearance, obstacle, capsule); return 0;
    default: return 1;
  }
}

template <int N>
static void scores(const Chain* ch, const ikf_rank_options* o, const float* poses, const float* q, long long m, int k, float min_clearance, float* out) {
  float w[IKF_MAX_CAPSULES * 6];
  for (int r = 0; r < k; ++r)
    for (long long j = 0; j < m; ++j) {
      const long long row = r * m + j;
      float qv[N], qr[N];
      for (int d = 0; d < N; ++d) { qv[d] = q[row * N + d]; qr[d] = 0.f; }
      out[row] = ikf::rank_row_score_world<N>(ch, &g_cm, qv, poses + j * 7, qr, false, *o, w, g_obs, g_n_obs, min_clearance);
    }
}

// rank_row_score_world of k candidates of each of m poses, tile-major, under the capsules and the world set above
extern "C" int world_host_scores(const void* chain, const ikf_rank_options* o, const float* poses, const float* q, long long m, int k,
                                 float min_clearance, float* out) {
  const Chain* ch = static_cast<const Chain*>(chain);
  switch (ch->ndof) {
    case 4: scores<4>(ch, o, poses, q, m, k, min_clearance, out); return 0;
    case 5: scores<5>(ch, o, poses, q, m, k, min_clearance, out); return 0;
    case 6: scores<6>(ch, o, poses, q, m, k, min_clearance, out); return 0;
    case 7: scores<7>(ch, o, poses, q, m, k, min_clearance, out); return 0;
    case 8: scores<8>(ch, o, poses, q, m, k, min_clearance, out); return 0;
    default: return 1;
  }
}
