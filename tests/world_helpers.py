"""World collision: the fp64 reference of a world clearance, the scenes and the threshold device shared by the host build of
ikflow_amd/csrc/world_math.h (tests/test_world_math_host.py) and the GPU tests (tests/test_world.py).

The reference shares no code with the kernel: capsule end points from the oracle's URDF walk (ko._link_frames, as oracle/kinematics_oracle.py:
capsule_clearance builds them); sphere and half-space in closed form; capsule as the least of the four end-point-to-segment distances and the
interior critical point of the two lines (not Ericson's clamping, which the kernel uses); box by a 2001-point grid on t polished by 60
golden-section steps (the oracle's own method for capsule pairs).  Tolerances are the project's: 2e-5 on a clearance (tests/test_kinematics.py),
a band of 1e-4 around min_clearance in which admissibility is not compared (tests/rank_helpers.py)."""
import numpy as np
import torch

import rank_helpers as RH
from ikflow_amd.world import BOX, CAPSULE, HALF_SPACE, SPHERE, World
from oracle import kinematics_oracle as ko

CLEARANCE_TOL = 2e-5
BAND = 1e-4
PAIR_AMBIGUITY = 4e-5   # two pairs whose reference clearances are this close may swap under two errors of CLEARANCE_TOL
EMPTY = 3.0e38


# ---- capsule end points of the rows, fp64 ----------------------------------------------------------------------------------------------------
def capsule_ends(orob, caps, q):
    """-> (E0, E1 [n x n_caps x 3] float64 numpy, radii [n_caps]) in the base frame; caps as given to Robot.set_collision_capsules."""
    names = [j.name for j in orob.joints]
    per_joint = ko._link_frames(orob, q)
    n = q.shape[0]
    e0, e1, rad = [], [], []
    for after, p0, p1, r in caps:
        T = torch.eye(4, dtype=torch.float64).repeat(n, 1, 1) if after is None else per_joint[names.index(after)]
        e0.append((T @ torch.tensor([*p0, 1.0], dtype=torch.float64))[:, :3].numpy())
        e1.append((T @ torch.tensor([*p1, 1.0], dtype=torch.float64))[:, :3].numpy())
        rad.append(float(r))
    return np.stack(e0, 1), np.stack(e1, 1), np.asarray(rad)


# ---- one term per kind: distance of the capsules' AXES [..., 3] from the obstacle's core (radii come off outside) ------------------------------
def _point_segment(c, e0, e1):
    d = e1 - e0
    dd = (d * d).sum(-1)
    t = np.where(dd > 0.0, ((c - e0) * d).sum(-1) / np.where(dd > 0.0, dd, 1.0), 0.0).clip(0.0, 1.0)
    return np.linalg.norm(e0 + d * t[..., None] - c, axis=-1)


def _segment_segment(a, b, e0, e1):
    best = np.minimum(np.minimum(_point_segment(a, e0, e1), _point_segment(b, e0, e1)),
                      np.minimum(_point_segment(e0, a, np.broadcast_to(b, e0.shape)), _point_segment(e1, a, np.broadcast_to(b, e1.shape))))
    u, v, w0 = np.broadcast_to(b - a, e0.shape), e1 - e0, a - e0
    uu, uv, vv, uw, vw = (u * u).sum(-1), (u * v).sum(-1), (v * v).sum(-1), (u * w0).sum(-1), (v * w0).sum(-1)
    den = uu * vv - uv * uv
    ok = den > 1e-18 * np.maximum(uu * vv, 1e-300)
    sden = np.where(ok, den, 1.0)
    s, t = (uv * vw - vv * uw) / sden, (uu * vw - uv * uw) / sden
    inside = ok & (s > 0.0) & (s < 1.0) & (t > 0.0) & (t < 1.0)
    d = np.linalg.norm(w0 + u * s[..., None] - v * t[..., None], axis=-1)
    return np.where(inside, np.minimum(best, d), best)


def _quat_matrix(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _sd_box_line(a, d, t, h):
    """sd_box of a + d t for a, d [n x 3] and t [n x T] -> [n x T], one axis at a time (no [n x T x 3] temporaries)."""
    out2, inner = 0.0, None
    for i in range(3):
        qi = np.abs(a[:, i, None] + d[:, i, None] * t) - h[i]
        out2 = out2 + np.square(np.maximum(qi, 0.0))
        inner = qi if inner is None else np.maximum(inner, qi)
    return np.sqrt(out2) + np.minimum(inner, 0.0)


def _box_segment(centre, quat, h, e0, e1):
    R = _quat_matrix(quat)
    l0, l1 = (e0 - centre) @ R, (e1 - centre) @ R   # rows times R = R^T applied to each vector
    d = l1 - l0
    grid = np.linspace(0.0, 1.0, 2001)
    out = np.empty(l0.shape[:-1])
    flat0, flatd, flat_out = l0.reshape(-1, 3), d.reshape(-1, 3), out.reshape(-1)
    for s in range(0, flat0.shape[0], 1024):
        a, dd = flat0[s:s + 1024], flatd[s:s + 1024]
        g = lambda t: _sd_box_line(a, dd, t, h)
        vals = g(grid[None, :])
        i0 = vals.argmin(1)
        lo, hi = grid[np.maximum(i0 - 1, 0)], grid[np.minimum(i0 + 1, 2000)]
        for _ in range(60):
            m1, m2 = lo + (hi - lo) * 0.381966011250105, lo + (hi - lo) * 0.618033988749895
            take = g(m1[:, None])[:, 0] < g(m2[:, None])[:, 0]
            hi, lo = np.where(take, m2, hi), np.where(take, lo, m1)
        flat_out[s:s + 1024] = np.minimum(vals.min(1), g(((lo + hi) / 2)[:, None])[:, 0])
    return out


def normalised(ob):
    """(kind, a, b, quat, radius) in fp64 with the normal / quaternion of unit length, as ikf_set_world stores it."""
    kind, a, b, quat, radius = ob
    a, b, quat = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(quat, np.float64)
    if kind == HALF_SPACE:
        nn = np.linalg.norm(a)
        a, b = a / nn, b / nn
    if kind == BOX:
        quat = quat / np.linalg.norm(quat)
    return kind, a, b, quat, float(radius)


def pair_clearance(ob, e0, e1, rc):
    """Clearance of capsules (axes e0-e1 [... x 3], radii rc broadcastable to [...]) from one obstacle, fp64."""
    kind, a, b, quat, radius = normalised(ob)
    if kind == SPHERE:
        return _point_segment(a, e0, e1) - radius - rc
    if kind == CAPSULE:
        return _segment_segment(a, b, e0, e1) - radius - rc
    if kind == HALF_SPACE:
        return np.minimum(e0 @ a, e1 @ a) - b[0] - rc
    return _box_segment(a, quat, b, e0, e1) - radius - rc


def clearance_matrix(world, E0, E1, radii):
    """[n x n_obstacles x n_caps] fp64."""
    obs = world.obstacles if isinstance(world, World) else world
    return np.stack([pair_clearance(ob, E0, E1, radii[None, :]) for ob in obs], 1) if len(obs) else np.empty((E0.shape[0], 0, E0.shape[1]))


def reference(orob, caps, world, q):
    """-> dict over the rows: clearance (3.0e38 in an empty world), obstacle, capsule (closest pair: lower obstacle, then lower capsule on a
    tie; -1 / -1 in an empty world), ambiguous (the two best pairs are within PAIR_AMBIGUITY of each other)."""
    E0, E1, radii = capsule_ends(orob, caps, q)
    D = clearance_matrix(world, E0, E1, radii)
    n, no, nc = D.shape
    if no == 0:
        return {"clearance": np.full(n, EMPTY), "obstacle": np.full(n, -1), "capsule": np.full(n, -1), "ambiguous": np.zeros(n, bool)}
    flat = D.reshape(n, no * nc)
    best = flat.argmin(1)   # (the first minimum in obstacle-major order: the tie rule)
    part = np.partition(flat, 1, axis=1) if no * nc > 1 else np.concatenate([flat, np.full((n, 1), np.inf)], 1)
    return {"clearance": flat.min(1), "obstacle": best // nc, "capsule": best % nc, "ambiguous": (part[:, 1] - part[:, 0]) <= PAIR_AMBIGUITY}


def threshold(ref_clearance):
    """The world's min_clearance of a test: the median of the reference clearances of its rows (the device of rank_helpers.clearance_threshold),
    so that every chain and scene has rejected and admitted rows."""
    return float(np.median(ref_clearance))


def band_shares(ref_clearance, thr):
    """(share of rows inside the 1e-4 band, share surely below, share surely above)."""
    c = np.asarray(ref_clearance)
    return float((np.abs(c - thr) <= BAND).mean()), float((c < thr - BAND).mean()), float((c > thr + BAND).mean())


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
SCENES = ("sphere", "capsule", "half_space", "box", "mixed7", "full64")
_KINDS = {"sphere": [SPHERE], "capsule": [CAPSULE], "half_space": [HALF_SPACE], "box": [BOX],
          "mixed7": [SPHERE, CAPSULE, HALF_SPACE, BOX, BOX, SPHERE, CAPSULE]}
_SCENE_CACHE = {}


def scene(which, name, caps=None):
    """The World `name` for chain `which` (fixed seeds) and its capsule model `caps` (a name of rank_helpers.capsule_models; None: the small
    model of rank_helpers.collision_capsules).  Obstacles sit where the robot's moving capsules pass - around end points of those capsules at
    random configurations, in the outer half of the reach - so that clearances spread over decimetres with both signs."""
    if (which, name, caps) in _SCENE_CACHE:
        return _SCENE_CACHE[(which, name, caps)]
    import helpers as H

    robot, orob = H.kin_robots(which)
    caps_name, caps = caps, RH.capsules(which, caps)
    rng = np.random.default_rng(7000 + 13 * SCENES.index(name) + sum(map(ord, which)))
    qs = torch.tensor(orob.sample_joint_angles(256, 0.0, np.random.default_rng(77)))
    E0, E1, radii = capsule_ends(orob, caps, qs)
    cloud = np.concatenate([E0[:, 1:], E1[:, 1:]], 1).reshape(-1, 3)   # (capsule 0 rides on the base)
    dist = np.linalg.norm(cloud, axis=1)
    cloud = cloud[dist >= np.median(dist)]
    kinds = _KINDS[name] if name in _KINDS else [int(rng.integers(0, 4)) for _ in range(64)]
    w = World()
    for i, kind in enumerate(kinds):
        for _ in range(200):
            c = cloud[rng.integers(len(cloud))] + rng.uniform(-0.05, 0.05, 3)
            zero, unit = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0)
            if kind == SPHERE:
                ob = (SPHERE, c, zero, unit, rng.uniform(0.03, 0.12))
            elif kind == CAPSULE:
                ob = (CAPSULE, c, c + rng.uniform(-0.3, 0.3, 3), unit, rng.uniform(0.02, 0.08))
            elif kind == HALF_SPACE:   # a wall beyond 0.55 .. 0.8 of the way to c, seen from the base; the normal is left unnormalised on purpose
                nrm = -c / np.linalg.norm(c) * rng.uniform(0.5, 2.0)
                ob = (HALF_SPACE, nrm, (float(nrm @ c) * rng.uniform(0.55, 0.8), 0.0, 0.0), unit, 0.0)
            else:
                ob = (BOX, c, rng.uniform(0.02, 0.25, 3), rng.standard_normal(4) * rng.uniform(0.5, 2.0), 0.0 if i % 2 == 0 else rng.uniform(0.005, 0.04))
            # The base capsule does not move: its clearance is the same in every row.  An obstacle is kept only when the moving capsules come
            # closer than that in three quarters of the sampled configurations, so that no threshold (a median) can sit on that constant.
            # (every 4th of the sampled configurations; every 16th with a model of rank_helpers.capsule_models, whose 24 capsules cost five times as much)
            every = 4 if caps_name is None else 16
            d = pair_clearance(ob, E0[::every], E1[::every], radii[None, :])
            if d[0, 0] > np.quantile(d[:, 1:].min(1), 0.75):
                break
        else:
            raise AssertionError(f"scene {name} of {which}: no place found for obstacle {i}")
        w._add(*ob)
    _SCENE_CACHE[(which, name, caps_name)] = w
    return w


def far_world():
    """Obstacles of every kind 50 m away: nothing any chain can reach."""
    w = World()
    w.add_sphere((50.0, 0.0, 0.0), 0.5)
    w.add_capsule((0.0, 50.0, 0.0), (1.0, 50.0, 0.0), 0.2)
    w.add_half_space((0.0, 0.0, 1.0), -50.0)
    w.add_box((-50.0, 0.0, 0.0), (1.0, 2.0, 3.0), (0.9, 0.1, 0.3, 0.2), 0.1)
    return w


N_ROWS = 257
N_ROWS_LARGE = 66     # with a capsule model of rank_helpers.capsule_models: the reference's cost grows with capsules x obstacles
_ROWS_CACHE = {}


def rows_and_reference(which, name, caps=None):
    """The 257 configurations (inside the limits, f32) on which chain `which` meets scene `name`, their fp64 reference and the scene's threshold
    (the median of these rows' clearances) - computed once; the GPU tests run slices rows[:n] of them.  caps: a name of
    rank_helpers.capsule_models (then 66 rows: one workgroup and two threads), None: the small model."""
    if (which, name, caps) not in _ROWS_CACHE:
        import helpers as H

        robot, orob = H.kin_robots(which)
        q = torch.tensor(orob.sample_joint_angles(N_ROWS if caps is None else N_ROWS_LARGE, 0.0, np.random.default_rng(300))).float().contiguous()
        ref = reference(orob, RH.capsules(which, caps), scene(which, name, caps), q)
        _ROWS_CACHE[(which, name, caps)] = (q, ref, threshold(ref["clearance"]))
    return _ROWS_CACHE[(which, name, caps)]


# The ranking with a world: one scene, the shapes of tests/test_world.py, and per (chain, shape) the candidates with their reference clearances
# and the world's min_clearance - the median of those rows.  (A shape of 1 or 15 rows has no shares worth checking: the CPU condition is
# checked from 130 rows on.)
RANK_SCENE = "mixed7"
RANK_SHAPES = [(1, 1), (3, 5), (65, 2), (64, 16), (1, 1024)]
_RANK_CASES = {}


def rank_case(which, m, k, caps=None, seed=None):
    """-> (poses, q, q_ref, reference world clearance of the k * m rows, threshold).  caps: a name of rank_helpers.capsule_models (the scene is
    then the one built for that model), None: the small model; seed: of the candidates, m + k by default."""
    if (which, m, k, caps, seed) not in _RANK_CASES:
        import helpers as H

        robot, orob = H.kin_robots(which)
        # (noise from 0.03 rad up: with the family's 0.001 rad a third of one pose's 1024 candidates would share a clearance to within the band)
        poses, q, q_ref = RH.candidates(orob, m, k, seed=m + k if seed is None else seed, lo_exp=-1.5)
        cl = reference(orob, RH.capsules(which, caps), scene(which, RANK_SCENE, caps), q)["clearance"]
        _RANK_CASES[(which, m, k, caps, seed)] = (poses, q, q_ref, cl, threshold(cl))
    return _RANK_CASES[(which, m, k, caps, seed)]


# ---- the ranking's reference with the world rule on top ----------------------------------------------------------------------------------------
def rank_reference(orob, robot_caps, world_cl, world_min_clearance, poses, q, k, rot_weight, self_collisions=False, min_clearance=0.0, **kw):
    """rank_helpers.reference(...) with admissibility extended by `world clearance >= world_min_clearance` and its 1e-4 band; world_cl: the
    reference world clearances of the rows (None: no world)."""
    if not self_collisions:
        kw.pop("self_clearance", None)
    ref = RH.reference(orob, poses, q, k, rot_weight, caps=robot_caps if self_collisions else None, min_clearance=min_clearance, **kw)
    if world_cl is not None:
        ref["admissible"] = ref["admissible"] & ~(world_cl < world_min_clearance)
        ref["near"] = ref["near"] | (np.abs(world_cl - world_min_clearance) <= BAND)
    return ref
