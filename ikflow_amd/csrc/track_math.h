// track_math.h - the arithmetic of a world track (track_kernels.hip, sweep_kernels.hip TRACK; the definitions: include/ikflow_amd_track.h): the
// fine frame between two key frames, in double precision on the host, and the verdict of one sample of a tracked edge from sweep_sample
// (sweep_math.h), capsule_endpoints / capsule_clearance (rank_math.h) and world_clearance (world_math.h), called and not restated.  Like
// world_math.h it holds nothing of the HIP runtime, so the same source compiles with g++: tests/test_track_math_host.py runs the interpolation
// against a numpy fp64 restatement and the sample test against the fp64 references.
#pragma once
#include <cmath>
#include "sweep_math.h"
#include "../../include/ikflow_amd_track.h"

namespace ikf {

// frames of the fine table of F key frames under S samples per edge, and the index of fine frame i after key frame t
IKF_SWEEP_HOST_DEVICE long long track_fine_frames(int F, int S) { return F < 1 ? 0 : (long long)(F - 1) * (S + 1) + 1; }
IKF_SWEEP_HOST_DEVICE long long track_fine_index(long long t, int i, int S) { return t * (S + 1) + i; }
// the fine frame that sample i = 1 .. S of the edge into waypoint t reads: the start edge (t = 0) stays on key frame 0
IKF_SWEEP_HOST_DEVICE long long track_sample_frame(long long t, int i, int S) { return t == 0 ? 0 : track_fine_index(t - 1, i, S); }

constexpr double IKF_TRACK_MIN_NORMAL = 1e-6;

// Fine frame i = 0 .. S between the normalised key-frame records a and b of one obstacle (the same kind): u = i / (S + 1), every field
// x_a + u (x_b - x_a) in double, rounded once to f32.  i = 0 is a, bit for bit.  Half-space: the blended normal is normalised - false when
// it is shorter than IKF_TRACK_MIN_NORMAL (*out is then not to be used).  Box: b's quaternion negated when its dot product with a's is < 0,
// then blended and normalised.  Host only: the device reads the table this fills.
inline bool track_interpolate(const WorldObstacle& a, const WorldObstacle& b, int i, int S, WorldObstacle* out) {
  *out = a;
  if (i == 0) return true;
  const double u = (double)i / (double)(S + 1);
  auto mix = [u](float x, float y) { return (double)x + u * ((double)y - (double)x); };
  for (int c = 0; c < 3; ++c) {
    out->a[c] = (float)mix(a.a[c], b.a[c]);
    out->b[c] = (float)mix(a.b[c], b.b[c]);
  }
  out->radius = (float)mix(a.radius, b.radius);
  if (a.kind == IKF_OBSTACLE_HALF_SPACE) {
    double n[3], nn = 0.0;
    for (int c = 0; c < 3; ++c) {
      n[c] = mix(a.a[c], b.a[c]);
      nn += n[c] * n[c];
    }
    nn = std::sqrt(nn);
    if (!(nn >= IKF_TRACK_MIN_NORMAL)) return false;
    for (int c = 0; c < 3; ++c) out->a[c] = (float)(n[c] / nn);
  } else if (a.kind == IKF_OBSTACLE_BOX) {
    double dot = 0.0;
    for (int c = 0; c < 4; ++c) dot += (double)a.quat[c] * (double)b.quat[c];
    const double sign = dot < 0.0 ? -1.0 : 1.0;
    double q[4], qq = 0.0;
    for (int c = 0; c < 4; ++c) {
      q[c] = (double)a.quat[c] + u * (sign * (double)b.quat[c] - (double)a.quat[c]);
      qq += q[c] * q[c];
    }
    qq = std::sqrt(qq);
    if (!(qq > 0.0)) return false;   // (two unit quaternions in one hemisphere blend to at least 1 / sqrt 2)
    for (int c = 0; c < 4; ++c) out->quat[c] = (float)(q[c] / qq);
  }
  return true;
}

// Is sample i = 1 .. S of the edge a -> b blocked?  The rules of sweep_edge in its order - self rule (reject_self), static world (n_obs > 0) -
// and then the track: world_clearance against `frame`, the n_track records of the sample's fine frame, < track_min.  The end points are those
// the first rule that ran has left in w (6 floats per capsule, owned by the caller).  frame and n_track are the same for every lane.
template <int NDOF>
IKF_HD bool track_sample_blocked(const Chain* __restrict__ ch, const CollisionModel* __restrict__ cm, const WorldObstacle* obs, int n_obs,
                                 float world_min, bool reject_self, float self_min, const WorldObstacle* frame, int n_track, float track_min,
                                 const float* a, const float* b, int i, int S, float* w) {
  float qv[NDOF];
  sweep_sample<NDOF>(a, b, i, S, qv);
  bool blocked = false;
  if (reject_self) blocked = capsule_clearance<NDOF>(ch, cm, qv, w) < self_min;
  if (!blocked && n_obs > 0) {
    if (!reject_self) capsule_endpoints<NDOF>(ch, cm, qv, w);
    blocked = world_clearance(obs, n_obs, cm, w).clearance < world_min;
  }
  if (!blocked) {
    if (!reject_self && n_obs <= 0) capsule_endpoints<NDOF>(ch, cm, qv, w);
    blocked = world_clearance(frame, n_track, cm, w).clearance < track_min;
  }
  return blocked;
}

}  // namespace ikf
