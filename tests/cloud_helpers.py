"""World point cloud: the fp64 reference of a cloud clearance, the scenes and the rows shared by the host build of ikflow_amd/csrc/cloud_math.h
(tests/test_cloud_math_host.py) and the GPU tests (tests/test_cloud.py).

The reference shares no code with the kernel: capsule end points from the oracle's URDF walk (world_helpers.capsule_ends), the distance of a point
from an axis by world_helpers._point_segment (a division, a norm - not the kernel's reciprocal and squared form), the minimum over all (capsule,
point) pairs of dist - rc - r.  Tolerances are the project's (world_helpers.py): 2e-5 on a clearance, a band of 1e-4 around min_clearance in which
admissibility is not compared.

A scene: the end points of the chain's moving capsules at 256 sampled configurations, the outer half by distance from the base; of those,
min(16, max(1, n_points // 8)) centres; every point a centre plus N(0, s^2), s in 0.03 .. 0.10 m per centre, rounded to f32; radius 0.01 m.  The rows
are world_helpers' 257 (66 with a capsule model by name); the threshold is the median reference clearance."""
import numpy as np
import torch

import rank_helpers as RH
import world_helpers as WH
from world_helpers import BAND, CLEARANCE_TOL, _point_segment, band_shares, capsule_ends  # noqa: F401  (shared with the test modules)

EMPTY = 3.0e38
POINT_RADIUS = 0.01
SIZES = (1, 511, 512, 513, 4097)          # one point; one tile less one, exactly, plus one; nine tiles
HOST_SIZES = (1, 255, 513, 4097)
RANK_POINTS = 513
_CLOUDS, _ROWS, _RANK = {}, {}, {}


def _draw(ends, n_points, seed):
    rng = np.random.default_rng(seed)
    n_centres = min(16, max(1, n_points // 8))
    centres = ends[rng.integers(len(ends), size=n_centres)]
    sigma = rng.uniform(0.03, 0.10, n_centres)
    of = rng.integers(n_centres, size=n_points)
    return np.ascontiguousarray((centres[of] + rng.standard_normal((n_points, 3)) * sigma[of, None]).astype(np.float32))


def _scene(which, n_points, caps):
    """The cloud, the rows and their reference, computed once.  A draw is kept only when, from the fp64 reference alone, it meets the conditions the
    GPU tests rest on (at most 5 % of the rows in the band around the median, at least 20 % on either side and - with the small capsule model - a
    spread of a decimetre): the device of world_helpers.scene, which redraws an obstacle until the moving capsules come near it."""
    key = (which, n_points, caps)
    if key not in _ROWS:
        import helpers as H

        _, orob = H.kin_robots(which)
        model = RH.capsules(which, caps)
        qs = torch.tensor(orob.sample_joint_angles(256, 0.0, np.random.default_rng(77)))
        E0, E1, _ = capsule_ends(orob, model, qs)
        ends = np.concatenate([E0[:, 1:], E1[:, 1:]], 1).reshape(-1, 3)   # (capsule 0 rides on the base)
        dist = np.linalg.norm(ends, axis=1)
        ends = ends[dist >= np.median(dist)]
        n = WH.N_ROWS if caps is None else WH.N_ROWS_LARGE
        q = torch.tensor(orob.sample_joint_angles(n, 0.0, np.random.default_rng(300))).float().contiguous()
        for attempt in range(20):
            pts = _draw(ends, n_points, 9000 + n_points + sum(map(ord, which)) + 100000 * attempt)
            ref = reference(orob, model, pts, POINT_RADIUS, q)
            thr = float(np.median(ref))
            band, below, above, spread = conditions(ref, thr)
            if band <= 0.05 and below >= 0.20 and above >= 0.20 and (spread >= 0.1 or caps is not None):
                break
        else:
            raise AssertionError(f"cloud of {n_points} points for {which}: no draw met the conditions")
        _CLOUDS[key], _ROWS[key] = pts, (q, ref, thr)
    return _CLOUDS[key], _ROWS[key]


def cloud(which, n_points, caps=None):
    """-> [n_points x 3] float32 numpy, fixed seeds."""
    return _scene(which, n_points, caps)[0]


def axis_distance(points, E0, E1):
    """min over the points of the distance from each capsule axis -> [n x n_caps] fp64 (inf without points)."""
    best = np.full(E0.shape[:2], np.inf)
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    step = max(1, (1 << 21) // max(1, E0.shape[0] * E0.shape[1]))
    for s in range(0, len(pts), step):
        best = np.minimum(best, _point_segment(pts[s:s + step, None, None, :], E0[None], E1[None]).min(0))
    return best


def reference(orob, caps, points, point_radius, q):
    """Cloud clearance of the rows of q, fp64 -> [n] (3.0e38 with no points or no capsules)."""
    n = q.shape[0]
    if len(points) == 0 or len(caps) == 0:
        return np.full(n, EMPTY)
    E0, E1, radii = capsule_ends(orob, caps, q)
    return (axis_distance(points, E0, E1) - radii[None, :]).min(1) - point_radius


def rows_and_reference(which, n_points, caps=None):
    """-> (q [257 or 66 x ndof] f32 torch, reference clearances of those rows, threshold = their median), computed once."""
    return _scene(which, n_points, caps)[1]


def conditions(ref, thr):
    """The conditions on a scene that the tests rest on, from the reference alone -> (band share, below, above, spread)."""
    band, below, above = band_shares(ref, thr)
    return band, below, above, float(ref.max() - ref.min())


def rank_case(which, m, k):
    """The candidates of world_helpers.rank_case with the reference CLOUD clearances of the k * m rows (cloud of RANK_POINTS points) and their
    median -> (poses, q, q_ref, world clearances, world threshold, cloud clearances, cloud threshold)."""
    if (which, m, k) not in _RANK:
        import helpers as H

        robot, orob = H.kin_robots(which)
        poses, q, q_ref, wcl, wthr = WH.rank_case(which, m, k)
        cl = reference(orob, RH.capsules(which, None), cloud(which, RANK_POINTS), POINT_RADIUS, q)
        _RANK[(which, m, k)] = (poses, q, q_ref, wcl, wthr, cl, float(np.median(cl)))
    return _RANK[(which, m, k)]


def rank_reference(orob, robot_caps, world_cl, world_thr, cloud_cl, cloud_thr, poses, q, k, rot_weight, **kw):
    """world_helpers.rank_reference (world_cl None: no primitive world) with admissibility extended by `cloud clearance >= cloud_thr` and its band."""
    ref = WH.rank_reference(orob, robot_caps, world_cl, world_thr, poses, q, k, rot_weight, **kw)
    ref["admissible"] = ref["admissible"] & ~(cloud_cl < cloud_thr)
    ref["near"] = ref["near"] | (np.abs(cloud_cl - cloud_thr) <= BAND)
    return ref
