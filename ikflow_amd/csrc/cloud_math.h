// cloud_math.h - the arithmetic of the world point cloud (cloud_kernels.hip): the squared distance of a point from a capsule axis, its minimum
// over a span of points, the cloud clearance of one configuration, and the launch plan of k_cloud_clearance.  Like rank_math.h and world_math.h
// it holds nothing of the HIP runtime, so the same source compiles with g++: tests/test_cloud_math_host.py runs it on the CPU against an fp64
// reference.  Definitions: include/ikflow_amd_cloud.h.
//
// Split independence: the cloud clearance is min over capsules of (sqrtf(min over points of dist2) - rc) - r.  fminf is exact, sqrtf and x - rc
// are monotone (non-decreasing, correctly rounded), so the minimum over ANY partition of the points - taken in dist2, after the square root or
// after the radius - has the same bits.  The kernel relies on it: a wave folds sqrtf(min2) - rc of every (capsule, tile) into one register.
#pragma once
#include "rank_math.h"
#include "../../include/ikflow_amd_cloud.h"

namespace ikf {

constexpr int IKF_CLOUD_TILE = 512;        // points of one LDS tile; the stored array is padded to a multiple of it with copies of the last point
constexpr int IKF_CLOUD_ROWS = 64;         // rows of one workgroup: a wave's lanes
constexpr int IKF_CLOUD_BLOCK = 256;       // threads: four waves, each owns a quarter of every tile
constexpr int IKF_CLOUD_MAX_CHUNKS = IKF_CLOUD_MAX_POINTS / IKF_CLOUD_TILE;   // 2048: a chunk holds at least one tile
constexpr float IKF_CLOUD_EMPTY = 3.0e38f;

// One stored point: (x, y, z, 0), 16 bytes - one global load, one LDS broadcast.
struct alignas(16) CloudPoint {
  float x, y, z, w;
};
static_assert(sizeof(CloudPoint) == 16, "a point is four words");

// A capsule axis as the inner loop reads it: e0, d = e1 - e0 and inv = 1 / d.d (0 for an axis shorter than 1e-6), computed once per capsule.
struct CloudAxis {
  float e0[3], d[3], inv;
};
IKF_HD CloudAxis cloud_axis(const float* e0, const float* e1) {
  CloudAxis ax;
#pragma unroll
  for (int i = 0; i < 3; ++i) { ax.e0[i] = e0[i]; ax.d[i] = e1[i] - e0[i]; }
  const float a = ax.d[0] * ax.d[0] + ax.d[1] * ax.d[1] + ax.d[2] * ax.d[2];
  ax.inv = a <= 1e-12f ? 0.f : 1.f / a;
  return ax;
}

// Squared distance of p from the axis: the direct form of point_segment_dist (world_math.h) without the square root.
IKF_HD float point_segment_dist2(float px, float py, float pz, const CloudAxis& ax) {
  const float rx = px - ax.e0[0], ry = py - ax.e0[1], rz = pz - ax.e0[2];
  const float t = fminf(fmaxf((rx * ax.d[0] + ry * ax.d[1] + rz * ax.d[2]) * ax.inv, 0.f), 1.f);
  const float x = rx - ax.d[0] * t, y = ry - ax.d[1] * t, z = rz - ax.d[2] * t;
  return x * x + y * y + z * z;
}

// min of dist2 over the points [0, n) of pts; 3.0e38 for an empty span.
IKF_HD float cloud_capsule_min2(const CloudPoint* pts, long long n, const CloudAxis& ax) {
  float m2 = IKF_CLOUD_EMPTY;
  for (long long i = 0; i < n; ++i) m2 = fminf(m2, point_segment_dist2(pts[i].x, pts[i].y, pts[i].z, ax));
  return m2;
}

// Cloud clearance of a configuration whose capsule end points are in w (6 floats per capsule: capsule_endpoints): 3.0e38 with no points or no
// capsules.
IKF_HD float cloud_clearance_row(const CloudPoint* pts, long long n, float point_radius, const CollisionModel* __restrict__ cm, const float* w) {
  const int nc = cm->n_caps;
  if (n <= 0 || nc <= 0) return IKF_CLOUD_EMPTY;
  float best = IKF_CLOUD_EMPTY;
  for (int c = 0; c < nc; ++c) {
    const CloudAxis ax = cloud_axis(w + c * 6, w + c * 6 + 3);
    best = fminf(best, sqrtf(cloud_capsule_min2(pts, n, ax)) - cm->radius[c]);
  }
  return best - point_radius;
}

// ---- the launch plan, pure integer arithmetic --------------------------------------------------------------------------
// Grid (row tiles of 64 rows) x (chunks of whole point tiles): as many chunks as it takes to put two workgroups on every CU - the ranking's
// factor, not measured for this kernel - and never more than there are tiles.  No chunk is empty; chunks <= 2048.
struct CloudPlan {
  int chunks, tiles_per_chunk;
};
inline long long cloud_tiles(long long n_points) { return (n_points + IKF_CLOUD_TILE - 1) / IKF_CLOUD_TILE; }
inline CloudPlan cloud_plan(long long rows, long long n_points, int n_cu) {
  const long long tiles = cloud_tiles(n_points);
  if (rows < 1 || tiles < 1) return {1, 0};
  const long long row_tiles = (rows + IKF_CLOUD_ROWS - 1) / IKF_CLOUD_ROWS;
  long long want = (2LL * (n_cu > 0 ? n_cu : 1) + row_tiles - 1) / row_tiles;
  if (want < 1) want = 1;
  const long long split = tiles < want ? tiles : want;
  const long long per = (tiles + split - 1) / split;
  return {(int)((tiles + per - 1) / per), (int)per};
}
// Floats of partial[chunk][row] that any call of up to `rows` rows can need, whatever the cloud: chunks > 1 only while row_tiles < 2 n_cu
// (rows < 128 n_cu), and then chunks * rows <= (2 n_cu / row_tiles + 1) * 64 row_tiles <= 128 n_cu + 64 + rows.  Monotone in `rows`, so a
// reservation covers every smaller call; at most 256 n_cu + 64 floats.
inline long long cloud_partial_bound(long long rows, int n_cu) {
  const long long cus = n_cu > 0 ? n_cu : 1;
  const long long by_chunks = (long long)IKF_CLOUD_MAX_CHUNKS * rows, by_cus = 128 * cus + 64 + (rows < 128 * cus ? rows : 128 * cus);
  return by_chunks < by_cus ? by_chunks : by_cus;
}

}  // namespace ikf
