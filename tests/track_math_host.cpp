// Test harness (CPU): the arithmetic of a world track - ikflow_amd/csrc/track_math.h, the very source the API unit and the kernels compile - built
// with g++ as a stand-alone program, so that tests/test_track_math_host.py can hold it against a numpy fp64 restatement and the fp64 references
// without a GPU (and so that it can be built with -fsanitize=address,undefined and run on its own).  Not part of the product.
//
//   track_math_host interp IN OUT     IN:  int32 F, n, S, then F * n ikf_obstacle records (normalised key frames)
//                                     OUT: track_fine_frames(F, S) * n ikf_obstacle records; exit 2 (and "t o i" on stdout) on a refused blend
//   track_math_host samples IN OUT    IN:  the Chain bytes, int32 n_caps, n_pairs, the ikf_capsule records, 2 * n_pairs int32; int32 n_obs and its
//                                          ikf_obstacle records (the static world, normalised), float world_min, int32 reject_self, float self_min,
//                                          int32 n_track, float track_min; int32 n_edges, S; then per edge ndof floats a, ndof floats b and
//                                          S * n_track ikf_obstacle records (the fine frame of each of its samples)
//                                     OUT: n_edges * S bytes, 1 where track_sample_blocked says blocked
//   track_math_host self              a small built-in check of both (exit 0 when it holds)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../ikflow_amd/csrc/track_math.h"

using ikf::Chain;
using ikf::CollisionModel;
using ikf::WorldObstacle;

static WorldObstacle to_record(const ikf_obstacle& in) {
  WorldObstacle o{};
  o.kind = in.kind;
  o.radius = in.radius;
  for (int c = 0; c < 3; ++c) { o.a[c] = in.a[c]; o.b[c] = in.b[c]; }
  for (int c = 0; c < 4; ++c) o.quat[c] = in.quat[c];
  return o;
}
static ikf_obstacle from_record(const WorldObstacle& in) {
  ikf_obstacle o{};
  o.kind = in.kind;
  o.radius = in.radius;
  for (int c = 0; c < 3; ++c) { o.a[c] = in.a[c]; o.b[c] = in.b[c]; }
  for (int c = 0; c < 4; ++c) o.quat[c] = in.quat[c];
  return o;
}

static bool read_all(const char* path, std::vector<unsigned char>* out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  out->resize((size_t)n);
  const bool ok = n == 0 || fread(out->data(), 1, (size_t)n, f) == (size_t)n;
  fclose(f);
  return ok;
}
static bool write_all(const char* path, const void* p, size_t n) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = n == 0 || fwrite(p, 1, n, f) == n;
  fclose(f);
  return ok;
}

struct Reader {
  const unsigned char* p;
  const unsigned char* end;
  bool ok = true;
  template <class T>
  T get() {
    T v{};
    take(&v, sizeof(T));
    return v;
  }
  void take(void* dst, size_t n) {
    if ((size_t)(end - p) < n) { ok = false; memset(dst, 0, n); return; }
    memcpy(dst, p, n);
    p += n;
  }
};

// -> 0, or 2 with *bad = {t, o, i}
static int interpolate(const std::vector<WorldObstacle>& keys, int F, int n, int S, std::vector<WorldObstacle>* fine, int bad[3]) {
  fine->assign((size_t)ikf::track_fine_frames(F, S) * n, WorldObstacle{});
  for (int t = 0; t < F; ++t)
    for (int i = 0; i <= (t + 1 < F ? S : 0); ++i)
      for (int o = 0; o < n; ++o) {
        const WorldObstacle& a = keys[(size_t)t * n + o];
        const WorldObstacle& b = keys[(size_t)(t + 1 < F ? t + 1 : t) * n + o];
        if (!ikf::track_interpolate(a, b, i, S, &(*fine)[(size_t)ikf::track_fine_index(t, i, S) * n + o])) {
          bad[0] = t; bad[1] = o; bad[2] = i;
          return 2;
        }
      }
  return 0;
}

static int run_interp(const char* in_path, const char* out_path) {
  std::vector<unsigned char> buf;
  if (!read_all(in_path, &buf)) return 1;
  Reader r{buf.data(), buf.data() + buf.size()};
  const int F = r.get<int32_t>(), n = r.get<int32_t>(), S = r.get<int32_t>();
  if (!r.ok || F < 1 || F > IKF_WORLD_TRACK_MAX_FRAMES || n < 1 || n > IKF_WORLD_MAX_OBSTACLES || S < 0 || S > IKF_SWEEP_MAX_SAMPLES) return 1;
  std::vector<WorldObstacle> keys((size_t)F * n);
  for (auto& k : keys) k = to_record(r.get<ikf_obstacle>());
  if (!r.ok) return 1;
  std::vector<WorldObstacle> fine;
  int bad[3];
  if (interpolate(keys, F, n, S, &fine, bad) != 0) {
    printf("%d %d %d\n", bad[0], bad[1], bad[2]);
    return 2;
  }
  std::vector<ikf_obstacle> out(fine.size());
  for (size_t i = 0; i < fine.size(); ++i) out[i] = from_record(fine[i]);
  return write_all(out_path, out.data(), out.size() * sizeof(ikf_obstacle)) ? 0 : 1;
}

template <int N>
static void samples(const Chain* ch, const CollisionModel* cm, const WorldObstacle* obs, int n_obs, float world_min, int reject_self, float self_min,
                    int n_track, float track_min, int n_edges, int S, Reader* r, unsigned char* out) {
  float w[IKF_MAX_CAPSULES * 6];
  std::vector<WorldObstacle> frame((size_t)n_track);
  for (int e = 0; e < n_edges; ++e) {
    float a[N], b[N];
    r->take(a, sizeof(a));
    r->take(b, sizeof(b));
    for (int i = 1; i <= S; ++i) {
      for (auto& f : frame) f = to_record(r->get<ikf_obstacle>());
      out[(size_t)e * S + (i - 1)] =
          ikf::track_sample_blocked<N>(ch, cm, obs, n_obs, world_min, reject_self != 0, self_min, frame.data(), n_track, track_min, a, b, i, S, w) ? 1 : 0;
    }
  }
}

static int run_samples(const char* in_path, const char* out_path) {
  std::vector<unsigned char> buf;
  if (!read_all(in_path, &buf)) return 1;
  Reader r{buf.data(), buf.data() + buf.size()};
  std::vector<Chain> chain(1);
  r.take(&chain[0], sizeof(Chain));
  std::vector<CollisionModel> cmv(1);
  CollisionModel& cm = cmv[0];
  cm = CollisionModel{};
  cm.n_caps = r.get<int32_t>();
  cm.n_pairs = r.get<int32_t>();
  if (!r.ok || cm.n_caps < 0 || cm.n_caps > IKF_MAX_CAPSULES || cm.n_pairs < 0 || cm.n_pairs > (int)(sizeof(cm.pair_a) / sizeof(cm.pair_a[0]))) return 1;
  for (int c = 0; c < cm.n_caps; ++c) {
    const ikf_capsule cap = r.get<ikf_capsule>();
    cm.frame[c] = cap.frame;
    cm.radius[c] = cap.radius;
    for (int i = 0; i < 3; ++i) { cm.p0[c][i] = cap.p0[i]; cm.p1[c][i] = cap.p1[i]; }
  }
  for (int p = 0; p < cm.n_pairs; ++p) {
    cm.pair_a[p] = (uint8_t)r.get<int32_t>();
    cm.pair_b[p] = (uint8_t)r.get<int32_t>();
  }
  const int n_obs = r.get<int32_t>();
  if (!r.ok || n_obs < 0 || n_obs > IKF_WORLD_MAX_OBSTACLES) return 1;
  std::vector<WorldObstacle> obs((size_t)n_obs);
  for (auto& o : obs) o = to_record(r.get<ikf_obstacle>());
  const float world_min = r.get<float>();
  const int reject_self = r.get<int32_t>();
  const float self_min = r.get<float>();
  const int n_track = r.get<int32_t>();
  const float track_min = r.get<float>();
  const int n_edges = r.get<int32_t>(), S = r.get<int32_t>();
  if (!r.ok || n_track < 1 || n_track > IKF_WORLD_MAX_OBSTACLES || n_edges < 0 || S < 1 || S > IKF_SWEEP_MAX_SAMPLES) return 1;
  std::vector<unsigned char> out((size_t)n_edges * S);
  const Chain* ch = &chain[0];
  switch (ch->ndof) {
    case 4: samples<4>(ch, &cm, obs.data(), n_obs, world_min, reject_self, self_min, n_track, track_min, n_edges, S, &r, out.data()); break;
    case 5: samples<5>(ch, &cm, obs.data(), n_obs, world_min, reject_self, self_min, n_track, track_min, n_edges, S, &r, out.data()); break;
    case 6: samples<6>(ch, &cm, obs.data(), n_obs, world_min, reject_self, self_min, n_track, track_min, n_edges, S, &r, out.data()); break;
    case 7: samples<7>(ch, &cm, obs.data(), n_obs, world_min, reject_self, self_min, n_track, track_min, n_edges, S, &r, out.data()); break;
    case 8: samples<8>(ch, &cm, obs.data(), n_obs, world_min, reject_self, self_min, n_track, track_min, n_edges, S, &r, out.data()); break;
    default: return 1;
  }
  if (!r.ok) return 1;
  return write_all(out_path, out.data(), out.size()) ? 0 : 1;
}

// a sphere moving 1 m in x over one edge and a half-space whose normal turns by 90 degrees: the key frames bit for bit, the middle frames known
static int run_self() {
  const int F = 2, n = 2, S = 3;
  std::vector<WorldObstacle> keys((size_t)F * n, WorldObstacle{});
  for (int t = 0; t < F; ++t) {
    WorldObstacle& s = keys[(size_t)t * n];
    s.kind = IKF_OBSTACLE_SPHERE;
    s.a[0] = (float)t;
    s.radius = 0.1f;
    s.quat[0] = 1.f;
    WorldObstacle& h = keys[(size_t)t * n + 1];
    h.kind = IKF_OBSTACLE_HALF_SPACE;
    h.a[t] = 1.f;   // (1, 0, 0) then (0, 1, 0)
    h.quat[0] = 1.f;
  }
  std::vector<WorldObstacle> fine;
  int bad[3];
  if (interpolate(keys, F, n, S, &fine, bad) != 0) return 1;
  if (fine.size() != (size_t)5 * n) return 1;
  if (memcmp(&fine[0], &keys[0], sizeof(WorldObstacle) * n) != 0 || memcmp(&fine[(size_t)4 * n], &keys[n], sizeof(WorldObstacle) * n) != 0) return 1;
  const WorldObstacle& mid_s = fine[(size_t)2 * n];
  const WorldObstacle& mid_h = fine[(size_t)2 * n + 1];
  if (mid_s.a[0] != 0.5f || mid_s.radius != 0.1f) return 1;
  if (std::fabs(mid_h.a[0] - 0.70710678f) > 1e-7f || std::fabs(mid_h.a[1] - 0.70710678f) > 1e-7f) return 1;
  keys[(size_t)n + 1].a[1] = 0.f;   // opposite normals: the middle blend vanishes and is refused
  keys[(size_t)n + 1].a[0] = -1.f;
  if (interpolate(keys, F, n, 1, &fine, bad) != 2 || bad[0] != 0 || bad[1] != 1 || bad[2] != 1) return 1;
  if (ikf::track_sample_frame(0, 3, 4) != 0 || ikf::track_sample_frame(2, 3, 4) != 8 || ikf::track_fine_frames(1024, 16) != 17392) return 1;
  puts("ok");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "self")) return run_self();
  if (argc == 2 && !strcmp(argv[1], "chain_bytes")) return printf("%d\n", (int)sizeof(Chain)) > 0 ? 0 : 1;
  if (argc == 4 && !strcmp(argv[1], "interp")) return run_interp(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "samples")) return run_samples(argv[2], argv[3]);
  fprintf(stderr, "usage: track_math_host self | interp IN OUT | samples IN OUT\n");
  return 64;
}
