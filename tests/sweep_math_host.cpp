// Test harness (CPU): the arithmetic of swept collision checks - ikflow_amd/csrc/sweep_math.h, the very source the GPU runs - compiled with g++ and
// driven edge by edge, so that tests/test_sweep_math_host.py can hold it against numpy float32 and an fp64 reference without a GPU.  Not part of
// the product.
#include "../ikflow_amd/csrc/sweep_math.h"

using ikf::Chain;
using ikf::CollisionModel;
using ikf::WorldObstacle;

static CollisionModel g_cm;
static WorldObstacle g_obs[IKF_WORLD_MAX_OBSTACLES];
static int g_n_obs = 0;

extern "C" int sweep_host_chain_bytes() { return (int)sizeof(Chain); }
extern "C" int sweep_host_max_samples() { return IKF_SWEEP_MAX_SAMPLES; }

// capsules in engine frames (ikf_capsule) and index pairs, as ikf_set_collision_model takes them
extern "C" void sweep_host_set_capsules(const ikf_capsule* caps, int n_caps, const int32_t* pairs, int n_pairs) {
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
extern "C" int sweep_host_set_world(const ikf_obstacle* obs, int n) {
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
static void samples(const float* a, const float* b, long long n, int S, float* out) {
  for (long long e = 0; e < n; ++e)
    for (int i = 1; i <= S; ++i) ikf::sweep_sample<N>(a + e * N, b + e * N, i, S, out + (e * S + (i - 1)) * N);
}

// the S sample configurations of n edges: out [n][S][ndof]
extern "C" int sweep_host_samples(int ndof, const float* a, const float* b, long long n, int S, float* out) {
  switch (ndof) {
    case 4: samples<4>(a, b, n, S, out); return 0;
    case 5: samples<5>(a, b, n, S, out); return 0;
    case 6: samples<6>(a, b, n, S, out); return 0;
    case 7: samples<7>(a, b, n, S, out); return 0;
    case 8: samples<8>(a, b, n, S, out); return 0;
    default: return 1;
  }
}

template <int N>
static void edges(const Chain* ch, const float* a, const float* b, long long n, int S, int use_world, float world_min, int reject_self, float self_min,
                  int* first) {
  float w[IKF_MAX_CAPSULES * 6];
  for (long long e = 0; e < n; ++e)
    first[e] = ikf::sweep_edge<N>(ch, &g_cm, g_obs, use_world ? g_n_obs : 0, world_min, reject_self != 0, self_min, a + e * N, b + e * N, S, w);
}

// sweep_edge of n edges under the capsules and (use_world) the world set above: the first blocked sample of each, -1 when free
extern "C" int sweep_host_edges(const void* chain, const float* a, const float* b, long long n, int S, int use_world, float world_min, int reject_self,
                                float self_min, int* first) {
  const Chain* ch = static_cast<const Chain*>(chain);
  switch (ch->ndof) {
    case 4: edges<4>(ch, a, b, n, S, use_world, world_min, reject_self, self_min, first); return 0;
    case 5: edges<5>(ch, a, b, n, S, use_world, world_min, reject_self, self_min, first); return 0;
    case 6: edges<6>(ch, a, b, n, S, use_world, world_min, reject_self, self_min, first); return 0;
    case 7: edges<7>(ch, a, b, n, S, use_world, world_min, reject_self, self_min, first); return 0;
    case 8: edges<8>(ch, a, b, n, S, use_world, world_min, reject_self, self_min, first); return 0;
    default: return 1;
  }
}

// the mask geometry
extern "C" int sweep_host_words(int k) { return ikf::sweep_words(k); }
extern "C" long long sweep_host_mask_words(long long T, int k) { return ikf::sweep_mask_words(T, k); }
extern "C" long long sweep_host_word_index(long long t, int r, int word, int k) { return ikf::sweep_word_index(t, r, word, k); }
extern "C" void sweep_host_wave_role(long long wave, int k, long long* t, int* r, int* word) { ikf::sweep_wave_role(wave, k, t, r, word); }
extern "C" unsigned long long sweep_host_live_lanes(int k, int word) { return ikf::sweep_live_lanes(k, word); }
extern "C" int sweep_host_bit(const unsigned long long* words, int j) { return ikf::sweep_bit(words, j) ? 1 : 0; }
extern "C" long long sweep_host_pair_waves(long long n) { return ikf::sweep_pair_waves(n); }
