"""A world track (include/ikflow_amd_track.h): the records ikf_set_world_track stores and the fine frames between them restated in numpy fp64, moving
scenes from fixed seeds, and the fp64 references of the node and edge rules - shared by the host tests (tests/test_track_host.py,
tests/test_track_math_host.py) and the GPU tests (tests/test_track.py).

The references are the project's existing ones: world_helpers.reference on a World built from one frame's records, sweep_helpers.verdicts with its
band (world_helpers.BAND, 1e-4) around a threshold.  A record is 11 numbers - a[3], b[3], quat[4], radius - beside its kind."""
import numpy as np
import torch

import helpers as H
import rank_helpers as RH
import sweep_helpers as SH
import world_helpers as WH
from ikflow_amd.world import BOX, CAPSULE, HALF_SPACE, SPHERE, World

F32 = np.float32
MAX_FRAMES = 1024


# ---- records -------------------------------------------------------------------------------------------------------------------------------------
def stored(world):
    """-> (kinds [n] int, records [n x 11] f32): what ikf_set_world_track keeps of a World's obstacles - the inputs rounded to f32, the normal
    (with its offset) and the quaternion normalised in fp64 from those, rounded once; the quaternion of any other kind is (1, 0, 0, 0)."""
    kinds, recs = [], []
    for kind, a, b, quat, radius in world.obstacles:
        a, b, quat = (np.asarray(v, F32).astype(np.float64) for v in (a, b, quat))
        q = np.array([1.0, 0.0, 0.0, 0.0])
        if kind == HALF_SPACE:
            nn = np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
            a, b = a / nn, np.array([b[0] / nn, b[1], b[2]])
        elif kind == BOX:
            q = quat / np.sqrt(quat[0] * quat[0] + quat[1] * quat[1] + quat[2] * quat[2] + quat[3] * quat[3])
        kinds.append(int(kind))
        recs.append(np.concatenate([a, b, q, [float(F32(radius))]]).astype(F32))
    return np.asarray(kinds), np.stack(recs)


def stored_track(worlds):
    """-> (kinds [n], keys [F x n x 11] f32)."""
    parts = [stored(w) for w in worlds]
    assert all(np.array_equal(p[0], parts[0][0]) for p in parts)
    return parts[0][0], np.stack([p[1] for p in parts])


def records_of(world):
    """(kinds, records [n x 11] f32) of a World as Engine.world_track_frame returns it: the numbers as they are."""
    obs = world.obstacles
    return np.asarray([o[0] for o in obs]), np.stack([np.concatenate([o[1], o[2], o[3], [o[4]]]).astype(F32) for o in obs])


def world_of(kinds, recs):
    w = World()
    for kind, r in zip(kinds, np.asarray(recs, np.float64)):
        w._add(int(kind), r[0:3], r[3:6], r[6:10], float(r[10]))
    return w


def fine_index(t, i, S):
    return t * (S + 1) + i


def interp_ref(kinds, keys, S):
    """The fine table [(F - 1)(S + 1) + 1][n][11] f32 of keys [F][n][11] f32, restated: u = i / (S + 1), every number linear in fp64, a half-space's
    normal then normalised, a box's second quaternion negated when its dot product with the first is < 0 before the blend and the blend
    normalised; rounded once.  i = 0 is the key frame."""
    F, n, _ = keys.shape
    K = keys.astype(np.float64)
    out = np.empty(((F - 1) * (S + 1) + 1, n, 11), F32)
    for t in range(F):
        out[fine_index(t, 0, S)] = keys[t]
        if t + 1 == F:
            break
        for i in range(1, S + 1):
            u = i / (S + 1)
            v = K[t] + u * (K[t + 1] - K[t])
            for o in range(n):
                if kinds[o] == HALF_SPACE:
                    v[o, 0:3] = v[o, 0:3] / np.sqrt((v[o, 0:3] ** 2).sum())
                elif kinds[o] == BOX:
                    qa, qb = K[t, o, 6:10], K[t + 1, o, 6:10]
                    if (qa * qb).sum() < 0.0:
                        qb = -qb
                    q = qa + u * (qb - qa)
                    v[o, 6:10] = q / np.sqrt((q ** 2).sum())
                else:
                    v[o, 6:10] = K[t, o, 6:10]
            out[fine_index(t, i, S)] = v.astype(F32)
    return out


def ulp_excess(got, ref):
    """max over the numbers of |got - ref| / ulp_f32(max(1, |ref|)): both sides compute in fp64 and round once, so at most 1."""
    got, ref = np.asarray(got, F32), np.asarray(ref, F32)
    ulp = np.spacing(np.maximum(np.abs(ref), F32(1.0)).astype(F32)).astype(np.float64)
    return float((np.abs(got.astype(np.float64) - ref.astype(np.float64)) / ulp).max())


# ---- moving scenes ---------------------------------------------------------------------------------------------------------------------------------
def _quat_mul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def _axis_angle(axis, angle):
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def _rotate(v, axis, angle):
    axis = axis / np.linalg.norm(axis)
    return v * np.cos(angle) + np.cross(axis, v) * np.sin(angle) + axis * (axis @ v) * (1 - np.cos(angle))


BASES = {"one": ("sphere", None), "mixed7": ("mixed7", None), "cheap5": ("mixed7", (0, 1, 2, 5, 6)), "full64": ("full64", None)}
_TRACKS = {}


def moving_track(which, F, base="mixed7", seed=0, caps=None):
    """F Worlds: the obstacles of world_helpers.scene(which, ...) in frame 0 - "one" the sphere scene, "mixed7" all four kinds with two boxes,
    "cheap5" its spheres, capsules and half-space (closed-form references), "full64" - each moving with its own constant velocity (up to 3 cm
    per frame and axis), capsules and boxes turning (up to 0.2 rad per frame), normals tilting (up to 0.05 rad per frame), radii, half extents
    and offsets drifting.  Fixed seeds; computed once."""
    key = (which, F, base, seed, caps)
    if key not in _TRACKS:
        name, pick = BASES[base]
        obs = WH.scene(which, name, caps).obstacles
        obs = [obs[i] for i in pick] if pick is not None else list(obs)
        rng = np.random.default_rng(8800 + 31 * seed + sum(map(ord, which + base)))
        motion = [(rng.uniform(-0.03, 0.03, 3), rng.standard_normal(3), rng.uniform(-0.2, 0.2), rng.uniform(-0.002, 0.002), rng.uniform(-0.01, 0.01))
                  for _ in obs]
        worlds = []
        for t in range(F):
            w = World()
            for (kind, a, b, quat, radius), (vel, axis, spin, grow, drift) in zip(obs, motion):
                a, b, quat = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(quat, np.float64)
                r = max(radius + grow * t, 0.0)
                if kind == SPHERE:
                    w._add(kind, a + vel * t, b, quat, r)
                elif kind == CAPSULE:
                    mid, half = 0.5 * (a + b) + vel * t, _rotate(0.5 * (b - a), axis, spin * t)
                    w._add(kind, mid - half, mid + half, quat, r)
                elif kind == HALF_SPACE:
                    w._add(kind, _rotate(a, axis, 0.25 * spin * t), (b[0] + drift * t, 0.0, 0.0), quat, 0.0)
                else:
                    w._add(kind, a + vel * t, b * (1.0 + 0.02 * t), _quat_mul(_axis_angle(axis, spin * t), quat / np.linalg.norm(quat)), r)
            worlds.append(w)
        _TRACKS[key] = worlds
    return _TRACKS[key]


def far_track(F):
    """Obstacles of every kind 100 m away, drifting: nothing any chain can reach."""
    worlds = []
    for t in range(F):
        w = World()
        w.add_sphere((100.0 + t, 0.0, 0.0), 0.5)
        w.add_capsule((0.0, 100.0, t), (1.0, 100.0, t), 0.2)
        w.add_half_space((0.0, 0.0, 1.0), -100.0 - t)
        w.add_box((-100.0, 0.0, t), (1.0, 2.0, 3.0), (0.9, 0.1, 0.3 + 0.1 * t, 0.2), 0.1)
        worlds.append(w)
    return worlds


def host_frames(worlds, S):
    """(t, i) -> World of fine frame i after key frame t, by interp_ref on the stored records: the frames of the CPU tests."""
    kinds, keys = stored_track(worlds)
    table = interp_ref(kinds, keys, S)
    return lambda t, i: world_of(kinds, table[fine_index(t, i, S)])


# ---- the node rule -----------------------------------------------------------------------------------------------------------------------------------
NODE_T, NODE_K = 5, 65
NODE_SHAPES = [(T, k) for T in (1, 2, 5) for k in (1, 63, 64, 65)]
# (chain, base, capsule model): every chain size on the 7 obstacles of all four kinds; 1 and 64 obstacles and 1 and 24 capsules on the Panda.  With
# 64 obstacles the fp64 reference costs 14 ms per row: its lattice is waypoints 0 and 1 of every candidate and the further waypoints of candidate 0.
NODE_CASES = [(which, "mixed7", None) for which in SH.CHAINS] + [("panda", "one", None), ("panda", "full64", None), ("panda", "mixed7", "caps1"),
                                                                 ("panda", "mixed7", "caps24")]
_NODES = {}


def sub_lattice(q_big, T, k):
    """Candidates r < k of waypoints t < T of the (NODE_T, NODE_K) lattice, tile-major [k * T x nd]."""
    nd = q_big.shape[1]
    return q_big.reshape(NODE_K, NODE_T, nd)[:k, :T].reshape(k * T, nd).contiguous()


def node_case(which, base, caps, frames=None):
    """-> dict: worlds (NODE_T of them), q (the big lattice), ref: clearance / obstacle / capsule / ambiguous as [NODE_K x NODE_T] arrays (nan /
    -2 where a 64-obstacle case leaves a row out), thr: the median of the clearances.  frames: (t) -> World of key frame t (default: the stored
    records); the reference is cached for the default only."""
    key = (which, base, caps)
    if frames is None and key in _NODES:
        return _NODES[key]
    orob = H.kin_robots(which)[1]
    model = RH.capsules(which, caps)
    worlds = moving_track(which, NODE_T, base, 0, None if caps == "caps1" else caps)   # (one capsule: no scene of its own, the small model's)
    _, q, _ = SH.path_inputs(orob, NODE_T, NODE_K, 70 + len(base))
    kinds, keys = stored_track(worlds)
    ref = {"clearance": np.full((NODE_K, NODE_T), np.nan), "obstacle": np.full((NODE_K, NODE_T), -2), "capsule": np.full((NODE_K, NODE_T), -2),
           "ambiguous": np.ones((NODE_K, NODE_T), bool)}
    g = q.reshape(NODE_K, NODE_T, -1)
    for t in range(NODE_T):
        rows = NODE_K if (base != "full64" or t < 2) else 1
        r = WH.reference(orob, model, world_of(kinds, keys[t]) if frames is None else frames(t), g[:rows, t].contiguous())
        for name in ref:
            ref[name][:rows, t] = r[name]
    c = dict(worlds=worlds, q=q, ref=ref, thr=float(np.nanmedian(ref["clearance"])), full=base != "full64")
    if frames is None:
        _NODES[key] = c
    return c


def node_shapes(c):
    """The (T, k) of NODE_SHAPES whose rows the case's reference covers."""
    return [(T, k) for T, k in NODE_SHAPES if c["full"] or T <= 2 or k == 1]


# ---- the edge rule -----------------------------------------------------------------------------------------------------------------------------------
# (T, k, S, rule, base of the track): rule "track" - the track alone; "world" - track + the static scene mixed7; "all" - and the self rule.  A
# track with boxes where the lattice is small, one of closed-form kinds where 2 * 65 * 65 edges of 16 samples are referenced.
MASK_CASES = ([(2, 3, S, rule, "mixed7") for S in (1, 3, 16) for rule in ("track", "world", "all")] +
              [(5, 8, 1, "track", "cheap5"), (5, 8, 3, "all", "mixed7"), (5, 8, 3, "world", "mixed7"), (5, 8, 16, "track", "cheap5"),
               (3, 65, 1, "track", "cheap5"), (3, 65, 3, "track", "cheap5"), (3, 65, 16, "track", "cheap5")])
MASK_CHAIN = "panda"
_MASKS = {}


def track_sample_clearances(orob, model, frames, samples, T, k, S, with_start):
    """fp64 clearance of every sample [n x S x nd] (sweep_helpers.lattice_edges' order) against ITS fine frame: sample i of an edge into waypoint
    t against frames(t - 1, i), the samples of the k start edges against frames(0, 0).  -> [n x S]."""
    n = samples.shape[0]
    out = np.empty((n, S))
    for t in range(1, T):
        block = slice((t - 1) * k * k, t * k * k)
        for i in range(1, S + 1):
            out[block, i - 1] = WH.reference(orob, model, frames(t - 1, i), torch.tensor(samples[block, i - 1]))["clearance"]
    if with_start:
        start = slice((T - 1) * k * k, n)
        w0 = frames(0, 0)
        for i in range(1, S + 1):
            out[start, i - 1] = WH.reference(orob, model, w0, torch.tensor(samples[start, i - 1]))["clearance"]
    return out


def edge_threshold(cl):
    """The median, over the edges, of the minimum over their samples."""
    return float(np.median(cl.min(1)))


def mask_inputs(T, k, S, base, seed):
    orob = H.kin_robots(MASK_CHAIN)[1]
    _, q, q_true = SH.path_inputs(orob, T, k, 900 + seed)
    q_start = (q_true[0] + 0.05).contiguous()
    return q, q_start, moving_track(MASK_CHAIN, T, base, seed)


def mask_case(T, k, S, rule, base, seed, frames=None):
    """-> dict of one lattice under one rule set: q, q_start, worlds, world (the static scene or None), samples [n x S x nd] of all edges (the k
    start edges last), track_cl / world_cl / self_cl [n x S] fp64 (None where the rule is off), their thresholds (edge_threshold), and
    v / v_nostart: sweep_helpers.verdicts over all edges / over the edges without the start edges.  frames: (t, i) -> World (default:
    host_frames); cached for the default only."""
    key = (T, k, S, rule, base, seed)
    if frames is None and key in _MASKS:
        return _MASKS[key]
    robot, orob = H.kin_robots(MASK_CHAIN)
    model = RH.collision_capsules(robot)
    q, q_start, worlds = mask_inputs(T, k, S, base, seed)
    a, b = SH.lattice_edges(q.numpy(), T, k, q_start.numpy())
    smp = SH.samples_f32(a, b, S)
    tc = track_sample_clearances(orob, model, host_frames(worlds, S) if frames is None else frames, smp, T, k, S, True)
    world = WH.scene(MASK_CHAIN, "mixed7") if rule in ("world", "all") else None
    wc, sc = SH.sample_clearances(orob, model, world, smp, want_world=world is not None, want_self=rule == "all")
    c = dict(q=q, q_start=q_start, worlds=worlds, world=world, samples=smp, track_cl=tc, world_cl=wc, self_cl=sc, track_thr=edge_threshold(tc),
             world_thr=None if wc is None else edge_threshold(wc), self_thr=None if sc is None else edge_threshold(sc))
    # the two world-like rules as one: a sample is surely blocked when either is below its threshold by the band, surely free when both are above
    shifted = tc - c["track_thr"] if wc is None else np.minimum(tc - c["track_thr"], wc - c["world_thr"])
    n_lat = (T - 1) * k * k
    c["v"] = SH.verdicts(shifted, 0.0, sc, c["self_thr"] or 0.0)
    c["v_nostart"] = SH.verdicts(shifted[:n_lat], 0.0, None if sc is None else sc[:n_lat], c["self_thr"] or 0.0)
    if frames is None:
        _MASKS[key] = c
    return c


# Seeds of MASK_CASES: the first of 0 .. 9 for which, by the references alone, sweep_helpers.shares_hold - the surely blocked share strictly between
# 10 % and 90 %, at most 2 % of the edges in the band - with the start edges and without them (tests/test_track_host.py asserts it on the CPU,
# tests/test_track.py again in front of the GPU case).  A case that is not listed takes seed 0.
MASK_SEEDS = {(2, 3, 1, "all", "mixed7"): 1}


def mask_seed(T, k, S, rule, base):
    return MASK_SEEDS.get((T, k, S, rule, base), 0)


def find_mask_seed(T, k, S, rule, base):
    for seed in range(10):
        c = mask_case(T, k, S, rule, base, seed)
        if SH.shares_hold(c["v"]) and SH.shares_hold(c["v_nostart"]):
            return seed
    return None


# ---- the lattices of "the path equals its parts" --------------------------------------------------------------------------------------------------
PATH_TRACK_BASE = "cheap5"
_PATH_THR = {}


def path_track(which, T, seed):
    return moving_track(which, T, PATH_TRACK_BASE, seed)


def path_track_threshold(which, T, k, seed, q):
    """The lower quartile of the fp64 clearances of the k * T rows from their key frames (sweep_helpers.LATTICE_QUANTILE, and never so high that a
    waypoint is left without an admissible candidate): three quarters of the nodes stay admissible."""
    key = (which, T, k, seed)
    if key not in _PATH_THR:
        robot, orob = H.kin_robots(which)
        model = RH.collision_capsules(robot)
        g = q.reshape(k, T, -1)
        cl = np.stack([WH.reference(orob, model, w, g[:, t].contiguous())["clearance"] for t, w in enumerate(path_track(which, T, seed))], 1)   # [k][T]
        _PATH_THR[key] = float(min(np.quantile(cl, SH.LATTICE_QUANTILE), cl.max(0).min() - 1e-3))
    return _PATH_THR[key]


# ---- the obstacle really moves ----------------------------------------------------------------------------------------------------------------------
def moving_crossing_case(on="edge"):
    """T = 3, k = 3 on the Panda, S = 1, built like sweep_helpers.crossing_case: candidate r of waypoint t is a0 + 0.8 r on joint 3 (so that
    the candidates' last capsules are decimetres apart), moved by
    0.3 t rad on joint 1.  One sphere of radius 0.03 in three key frames.
      on = "edge": it sits on the end point of the last capsule at the middle sample of the edge (waypoint 0, candidate 0) -> (waypoint 1,
                   candidate 0) in FINE frame (0, 1) only: key frames 0 and 1 put it the same distance to either side (so their midpoint is that
                   point), 2 m away each, key frame 2 far away too.
      on = "node": it sits on the end point of the last capsule of (waypoint 1, candidate 0) in key frame 1 only, far away in key frames 0 and 2.
    -> dict: poses, q tile-major [9 x nd], worlds, spot (the point), model."""
    robot, orob = H.kin_robots("panda")
    model = RH.collision_capsules(robot)
    nd = orob.ndof
    a0 = np.asarray(orob.sample_joint_angles(1, 0.4, np.random.default_rng(9)), np.float64)[0]
    rows = np.stack([np.stack([a0 + np.eye(nd)[3] * 0.8 * r + np.eye(nd)[1] * 0.3 * t for t in range(3)]) for r in range(3)]).astype(F32)   # [r][t]
    q = np.ascontiguousarray(rows.reshape(9, nd))
    if on == "edge":
        at = SH.samples_f32(rows[:1, 0], rows[:1, 1], 1)[:, 0]
    else:
        at = rows[:1, 1]
    E0, E1, _ = WH.capsule_ends(orob, model, torch.tensor(at))
    spot = E1[0, -1]
    off = np.array([0.0, 2.0, 0.0])
    places = [spot - off, spot + off, spot + 5 * off] if on == "edge" else [spot + 5 * off, spot, spot - 5 * off]
    worlds = []
    for p in places:
        w = World()
        w.add_sphere(tuple(float(x) for x in p), 0.03)
        worlds.append(w)
    from oracle import kinematics_oracle as ko

    poses = ko.forward_kinematics(orob, torch.tensor(rows[0]).double()).float().contiguous()
    return dict(poses=poses, q=torch.tensor(q), worlds=worlds, spot=spot, model=model)


def crossing_reference(c):
    """fp64, S = 1: (nodes [t][r] against key frame t, mids [t - 1][r][j]: the middle sample of the edge (t - 1, j) -> (t, r) against fine frame
    (t - 1, 1), per_key: the same middle samples against each KEY frame set as a static world, [key][t - 1][r][j])."""
    orob = H.kin_robots("panda")[1]
    g = c["q"].numpy().reshape(3, 3, -1)
    nodes = np.stack([WH.reference(orob, c["model"], c["worlds"][t], torch.tensor(g[:, t]))["clearance"] for t in range(3)])
    a, b = SH.lattice_edges(c["q"].numpy(), 3, 3)
    mid = torch.tensor(SH.samples_f32(a, b, 1)[:, 0])
    frames = host_frames(c["worlds"], 1)
    mids = np.stack([WH.reference(orob, c["model"], frames(t - 1, 1), mid[(t - 1) * 9:t * 9])["clearance"].reshape(3, 3) for t in (1, 2)])
    per_key = np.stack([WH.reference(orob, c["model"], w, mid)["clearance"].reshape(2, 3, 3) for w in c["worlds"]])
    return nodes, mids, per_key
