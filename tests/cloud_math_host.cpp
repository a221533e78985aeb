// Test harness (CPU): the arithmetic of the world point cloud - ikflow_amd/csrc/cloud_math.h, the very source the GPU runs - compiled with g++ and
// driven term by term / row by row, so that tests/test_cloud_math_host.py can hold it against an fp64 reference without a GPU.  Not part of the product.
#include "../ikflow_amd/csrc/cloud_math.h"

#include <vector>

using ikf::Chain;
using ikf::CloudAxis;
using ikf::CloudPoint;
using ikf::CollisionModel;

static CollisionModel g_cm;

extern "C" int cloud_host_chain_bytes() { return (int)sizeof(Chain); }
extern "C" int cloud_host_point_bytes() { return (int)sizeof(CloudPoint); }
extern "C" int cloud_host_max_points() { return IKF_CLOUD_MAX_POINTS; }
extern "C" int cloud_host_tile() { return ikf::IKF_CLOUD_TILE; }

// capsules in engine frames (ikf_capsule), as ikf_set_collision_model takes them (the cloud does not read the pairs)
extern "C" void cloud_host_set_capsules(const ikf_capsule* caps, int n_caps) {
  g_cm = CollisionModel{};
  g_cm.n_caps = n_caps;
  for (int c = 0; c < n_caps; ++c) {
    g_cm.frame[c] = caps[c].frame;
    g_cm.radius[c] = caps[c].radius;
    for (int i = 0; i < 3; ++i) { g_cm.p0[c][i] = caps[c].p0[i]; g_cm.p1[c][i] = caps[c].p1[i]; }
  }
}

// n independent (point i, axis i) terms: seg [n][6] the axis' end points, p [n][3] -> dist2 of each
extern "C" void cloud_host_dist2(const float* seg, const float* p, long long n, float* out) {
  for (long long i = 0; i < n; ++i) {
    const CloudAxis ax = ikf::cloud_axis(seg + 6 * i, seg + 6 * i + 3);
    out[i] = ikf::point_segment_dist2(p[3 * i], p[3 * i + 1], p[3 * i + 2], ax);
  }
}

// The rows of q against the points pts [n_pts] (x, y, z, 0) under the capsules set above.  cuts [n_cuts] ascending in 0 .. n_pts split the points
// into n_cuts + 1 spans (n_cuts = 0: the whole cloud at once); level: where the spans' minima meet - 0 in dist2 (cloud_capsule_min2 per span),
// 1 after sqrtf and the capsule's radius, 2 after the whole cloud_clearance_row of each span.
template <int N>
static void rows(const Chain* ch, const float* q, long long n, const CloudPoint* pts, long long n_pts, float radius, const long long* cuts,
                 int n_cuts, int level, float* out) {
  float w[IKF_MAX_CAPSULES * 6 + 1];
  std::vector<long long> edge(1, 0);
  for (int i = 0; i < n_cuts; ++i) edge.push_back(cuts[i]);
  edge.push_back(n_pts);
  for (long long r = 0; r < n; ++r) {
    float qv[N];
    for (int d = 0; d < N; ++d) qv[d] = q[r * N + d];
    ikf::capsule_endpoints<N>(ch, &g_cm, qv, w);
    if (n_cuts == 0) { out[r] = ikf::cloud_clearance_row(pts, n_pts, radius, &g_cm, w); continue; }
    if (n_pts <= 0 || g_cm.n_caps <= 0) { out[r] = ikf::IKF_CLOUD_EMPTY; continue; }
    float best = ikf::IKF_CLOUD_EMPTY;
    if (level == 2) {
      for (size_t s = 0; s + 1 < edge.size(); ++s)
        if (edge[s + 1] > edge[s]) best = fminf(best, ikf::cloud_clearance_row(pts + edge[s], edge[s + 1] - edge[s], radius, &g_cm, w));
      out[r] = best;
      continue;
    }
    for (int c = 0; c < g_cm.n_caps; ++c) {
      const CloudAxis ax = ikf::cloud_axis(w + c * 6, w + c * 6 + 3);
      float m2 = ikf::IKF_CLOUD_EMPTY;
      for (size_t s = 0; s + 1 < edge.size(); ++s) {
        const float part = ikf::cloud_capsule_min2(pts + edge[s], edge[s + 1] - edge[s], ax);
        if (level == 0) m2 = fminf(m2, part);
        else best = fminf(best, sqrtf(part) - g_cm.radius[c]);   // the kernel's form: one running register
      }
      if (level == 0) best = fminf(best, sqrtf(m2) - g_cm.radius[c]);
    }
    out[r] = best - radius;
  }
}

extern "C" int cloud_host_rows(const void* chain, const float* q, long long n, const void* pts, long long n_pts, float radius, const long long* cuts,
                               int n_cuts, int level, float* out) {
  const Chain* ch = static_cast<const Chain*>(chain);
  const CloudPoint* p = static_cast<const CloudPoint*>(pts);
  switch (ch->ndof) {
    case 4: rows<4>(ch, q, n, p, n_pts, radius, cuts, n_cuts, level, out); return 0;
    case 5: rows<5>(ch, q, n, p, n_pts, radius, cuts, n_cuts, level, out); return 0;
    case 6: rows<6>(ch, q, n, p, n_pts, radius, cuts, n_cuts, level, out); return 0;
    case 7: rows<7>(ch, q, n, p, n_pts, radius, cuts, n_cuts, level, out); return 0;
    case 8: rows<8>(ch, q, n, p, n_pts, radius, cuts, n_cuts, level, out); return 0;
    default: return 1;
  }
}

extern "C" void cloud_host_plan(long long rows, long long n_points, int n_cu, int* chunks, int* tiles_per_chunk) {
  const ikf::CloudPlan p = ikf::cloud_plan(rows, n_points, n_cu);
  *chunks = p.chunks;
  *tiles_per_chunk = p.tiles_per_chunk;
}
extern "C" long long cloud_host_partial_bound(long long rows, int n_cu) { return ikf::cloud_partial_bound(rows, n_cu); }
