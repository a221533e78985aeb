// world_math.h - the arithmetic of world collision (world_kernels.hip, and rank_kernels.hip when a world is set): the clearance of one robot
// capsule from one obstacle of each kind, the world clearance of a configuration with its closest pair, and the row score of the ranking with
// the world rule on top.  Like rank_math.h it holds nothing of the HIP runtime, so the same source compiles with g++:
// tests/test_world_math_host.py runs it on the CPU against an fp64 reference.  Definitions: include/ikflow_amd_world.h.
//
// A negative clearance means penetration.  For a box and a half-space it is the depth of the capsule's axis below the surface (plus the radii);
// for a sphere and a capsule it is NOT a penetration depth: the distance between two crossing axes is 0 however deep they lie in each other.
#pragma once
#include "rank_math.h"
#include "../../include/ikflow_amd_world.h"

namespace ikf {

constexpr int IKF_WORLD_OBSTACLE_WORDS = 16;
// One obstacle as the kernels read it: the fields of ikf_obstacle, normal and quaternion already of unit length (the host normalises in
// fp64 when the world is set; the device never does), padded to 16 words.
struct WorldObstacle {
  int kind;
  float a[3], b[3], quat[4], radius;
  float pad[4];
};
static_assert(sizeof(WorldObstacle) == 4 * IKF_WORLD_OBSTACLE_WORDS, "an obstacle is 16 words");
struct WorldModel {
  int n;
  int pad[15];
  WorldObstacle obs[IKF_WORLD_MAX_OBSTACLES];
};
constexpr int IKF_WORLD_TABLE_WORDS = IKF_WORLD_MAX_OBSTACLES * IKF_WORLD_OBSTACLE_WORDS;   // 4 KB when staged in LDS

IKF_HD float point_segment_dist(const float* c, const float* e0, const float* e1) {
  const float d[3] = {e1[0] - e0[0], e1[1] - e0[1], e1[2] - e0[2]};
  const float r[3] = {c[0] - e0[0], c[1] - e0[1], c[2] - e0[2]};
  const float a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  const float t = a <= 1e-12f ? 0.f : fminf(fmaxf((r[0] * d[0] + r[1] * d[1] + r[2] * d[2]) / a, 0.f), 1.f);
  const float x = r[0] - d[0] * t, y = r[1] - d[1] * t, z = r[2] - d[2] * t;
  return sqrtf(x * x + y * y + z * z);
}

IKF_HD float half_space_dist(const float* n, float d, const float* e0, const float* e1) {
  const float s0 = n[0] * e0[0] + n[1] * e0[1] + n[2] * e0[2], s1 = n[0] * e1[0] + n[1] * e1[1] + n[2] * e1[2];
  return fminf(s0, s1) - d;
}

// signed distance of p (in the box's own frame) to the axis-aligned box of half extents h
IKF_HD float sd_box(float px, float py, float pz, const float* h) {
  const float qx = fabsf(px) - h[0], qy = fabsf(py) - h[1], qz = fabsf(pz) - h[2];
  const float ox = fmaxf(qx, 0.f), oy = fmaxf(qy, 0.f), oz = fmaxf(qz, 0.f);
  return sqrtf(ox * ox + oy * oy + oz * oz) + fminf(fmaxf(qx, fmaxf(qy, qz)), 0.f);
}

// rows of R^T for the unit quaternion (w, x, y, z) of R: box-frame coordinates of a base-frame vector v are Rt v
IKF_HD void quat_to_rt(const float* q, float Rt[9]) {
  const float w = q[0], x = q[1], y = q[2], z = q[3];
  Rt[0] = 1.f - 2.f * (y * y + z * z); Rt[1] = 2.f * (x * y + w * z);       Rt[2] = 2.f * (x * z - w * y);
  Rt[3] = 2.f * (x * y - w * z);       Rt[4] = 1.f - 2.f * (x * x + z * z); Rt[5] = 2.f * (y * z + w * x);
  Rt[6] = 2.f * (x * z + w * y);       Rt[7] = 2.f * (y * z - w * x);       Rt[8] = 1.f - 2.f * (x * x + y * y);
}

constexpr int IKF_BOX_SEARCH_STEPS = 32;
// min over t in [0, 1] of sd_box(Rt (e(t) - centre), h): t -> sd_box is convex and 1-Lipschitz in arc length, so a golden-section search
// brackets its minimum; a fixed 32 steps (no early exit: every lane of a wave does the same work) leave 0.618^32 = 2.1e-7 of the segment.
// The least value SEEN is kept, the end points included, so a flat minimum or a rounding tie costs nothing.
IKF_HD float box_segment_dist(const float* centre, const float Rt[9], const float* h, const float* e0, const float* e1) {
  const float r0[3] = {e0[0] - centre[0], e0[1] - centre[1], e0[2] - centre[2]};
  const float r1[3] = {e1[0] - centre[0], e1[1] - centre[1], e1[2] - centre[2]};
  float l0[3], dl[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    l0[i] = Rt[3 * i] * r0[0] + Rt[3 * i + 1] * r0[1] + Rt[3 * i + 2] * r0[2];
    dl[i] = Rt[3 * i] * r1[0] + Rt[3 * i + 1] * r1[1] + Rt[3 * i + 2] * r1[2] - l0[i];
  }
  const float G = 0.6180339887f;
  float lo = 0.f, hi = 1.f, x1 = 1.f - G, x2 = G;
  float f1 = sd_box(l0[0] + dl[0] * x1, l0[1] + dl[1] * x1, l0[2] + dl[2] * x1, h);
  float f2 = sd_box(l0[0] + dl[0] * x2, l0[1] + dl[1] * x2, l0[2] + dl[2] * x2, h);
  float best = fminf(fminf(sd_box(l0[0], l0[1], l0[2], h), sd_box(l0[0] + dl[0], l0[1] + dl[1], l0[2] + dl[2], h)), fminf(f1, f2));
  for (int it = 0; it < IKF_BOX_SEARCH_STEPS; ++it) {
    const bool left = f1 < f2;   // the minimum is in [lo, x2]; otherwise in [x1, hi]
    lo = left ? lo : x1;
    hi = left ? x2 : hi;
    const float xn = left ? hi - G * (hi - lo) : lo + G * (hi - lo);
    const float fn = sd_box(l0[0] + dl[0] * xn, l0[1] + dl[1] * xn, l0[2] + dl[2] * xn, h);
    best = fminf(best, fn);
    const float ox1 = x1, of1 = f1;
    x1 = left ? xn : x2;
    f1 = left ? fn : f2;
    x2 = left ? ox1 : xn;
    f2 = left ? of1 : fn;
  }
  return best;
}

struct WorldHit {
  float clearance;
  int obstacle, capsule;   // the closest pair; -1 in an empty world
};

// World clearance of a configuration whose capsule end points are in w (6 floats per capsule: capsule_endpoints).  Obstacle outside, capsule
// inside, strict `<`: on a tie the lower obstacle index wins, then the lower capsule index.  obs and n_obs are the same for every lane.
IKF_HD WorldHit world_clearance(const WorldObstacle* obs, int n_obs, const CollisionModel* __restrict__ cm, const float* w) {
  WorldHit hit = {3.0e38f, -1, -1};
  const int nc = cm->n_caps;
  for (int o = 0; o < n_obs; ++o) {
    const WorldObstacle& ob = obs[o];
    const int kind = ob.kind;
    float Rt[9];
    if (kind == IKF_OBSTACLE_BOX) quat_to_rt(ob.quat, Rt);
    for (int c = 0; c < nc; ++c) {
      const float* e0 = w + c * 6;
      const float* e1 = e0 + 3;
      float d;
      if (kind == IKF_OBSTACLE_SPHERE) d = point_segment_dist(ob.a, e0, e1);
      else if (kind == IKF_OBSTACLE_CAPSULE) d = segment_segment_dist(e0, e1, ob.a, ob.b);
      else if (kind == IKF_OBSTACLE_HALF_SPACE) d = half_space_dist(ob.a, ob.b[0], e0, e1);
      else d = box_segment_dist(ob.a, Rt, ob.b, e0, e1);
      if (kind != IKF_OBSTACLE_HALF_SPACE) d -= ob.radius;
      d -= cm->radius[c];
      if (d < hit.clearance) { hit.clearance = d; hit.obstacle = o; hit.capsule = c; }
    }
  }
  return hit;
}

// rank_row_score plus the world rule: a row that is admissible so far is inadmissible when its world clearance is < world_min_clearance,
// whatever o.reject_collisions says.  (Here and not in rank_math.h, which this header includes for segment_segment_dist.)  w: as for
// rank_row_score, but ALWAYS provided; the self-collision walk has filled it when o.reject_collisions let an admissible row through.
template <int NDOF>
IKF_HD float rank_row_score_world(const Chain* __restrict__ ch, const CollisionModel* __restrict__ cm, const float qv[NDOF], const float* __restrict__ tgt,
                                  const float* __restrict__ q_ref, bool has_ref, const ikf_rank_options& o, float* w, const WorldObstacle* obs,
                                  int n_obs, float world_min_clearance) {
  const float score = rank_row_score<NDOF>(ch, cm, qv, tgt, q_ref, has_ref, o, w);
  if (!(score < rank_inf())) return score;
  if (!o.reject_collisions) capsule_endpoints<NDOF>(ch, cm, qv, w);
  return world_clearance(obs, n_obs, cm, w).clearance < world_min_clearance ? rank_inf() : score;
}

}  // namespace ikf
