"""Swept collision checks along edges (include/ikflow_amd_sweep.h): the sample configurations as sequential numpy float32, the fp64 verdicts of
an edge, the lattice with forbidden edges, and the inputs shared by the host build of ikflow_amd/csrc/sweep_math.h
(tests/test_sweep_math_host.py) and the GPU tests (tests/test_sweep.py).

The references are the project's existing ones, applied to every sample: world_helpers.reference for the world rule, the oracle's
capsule_clearance (what rank_helpers uses) for the self rule.  Tolerance: world_helpers.BAND (1e-4) around a threshold, inside which a
verdict is not compared.  A sample is surely blocked when some rule in force has clearance < threshold - BAND, surely free when every rule in
force has clearance > threshold + BAND, and in the band otherwise.  An edge is surely blocked when a sample is, surely free when every sample
is, and in the band otherwise - the reference cannot decide it.  Its first blocked sample is compared when no earlier sample is in the band."""
import numpy as np
import torch

import helpers as H
import path_helpers as PH
import rank_helpers as RH
import world_helpers as WH
from oracle import kinematics_oracle as ko

F = np.float32
INF = F(np.inf)
BAND = WH.BAND
MAX_SAMPLES = 16
# ndof 7, 8 and 5 (one prismatic joint), then both 4- and both 6-joint synthetic chains: every k_sweep_edges<ND> the library builds, ND = 4 .. 8
CHAINS = ("panda", "fetch", "syn5p", "syn4r", "syn4p", "syn6r", "syn6p")
NDOF = {"panda": 7, "fetch": 8, "syn5p": 5, "syn4r": 4, "syn4p": 4, "syn6r": 6, "syn6p": 6}
N_EDGES = 257
N_EDGES_FULL64 = 130                          # (the fp64 reference costs about 14 ms per configuration in the 64-obstacle scene)
EDGE_CASES = [("mixed7", 1), ("mixed7", 3), ("mixed7", 16), ("full64", 1)]
SIZES = {"mixed7": (1, 63, 64, 65, 257), "full64": (1, 63, 64, 65, 130)}


def samples_f32(a, b, S):
    """a, b [n x nd] -> [n x S x nd] f32: sample i = 1 .. S is a + f * (b - a) with f = f32(i) / f32(S + 1), every operation a float32 numpy
    operation in the header's order."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    out = np.empty((a.shape[0], S, a.shape[1]), F)
    for i in range(1, S + 1):
        f = F(i) / F(S + 1)
        d = b - a
        p = f * d
        out[:, i - 1] = a + p
    assert out.dtype == F
    return out


def sample_clearances(orob, caps, world, samples, want_world=True, want_self=True):
    """fp64 clearances of every sample [n x S x nd] -> (world [n x S] or None, self [n x S] or None)."""
    n, S, nd = samples.shape
    q = torch.tensor(samples.reshape(n * S, nd))
    wc = WH.reference(orob, caps, world, q)["clearance"].reshape(n, S) if (want_world and world is not None and len(world)) else None
    sc = ko.capsule_clearance(orob, caps, (), q.double()).numpy().reshape(n, S) if want_self else None
    return wc, sc


def verdicts(world_cl=None, world_thr=0.0, self_cl=None, self_thr=0.0):
    """The rules in force are those whose clearances are given.  -> dict over the edges: blocked / free (sure), band, first (the first surely
    blocked sample, -1 without one), first_sure (no sample in front of `first` - or, on a free edge, no sample at all - is in the band)."""
    rules = [(c, t) for c, t in ((world_cl, world_thr), (self_cl, self_thr)) if c is not None]
    n, S = rules[0][0].shape if rules else (0, 0)
    s_blocked = np.zeros((n, S), bool)
    s_free = np.ones((n, S), bool)
    for c, t in rules:
        s_blocked |= c < t - BAND
        s_free &= c > t + BAND
    s_band = ~s_blocked & ~s_free
    blocked = s_blocked.any(1)
    free = s_free.all(1)
    first = np.where(blocked, s_blocked.argmax(1), -1).astype(np.int32)
    upto = np.where(blocked, first, S)
    first_sure = ~(s_band & (np.arange(S)[None, :] < upto[:, None])).any(1)
    return {"blocked": blocked, "free": free, "band": ~blocked & ~free, "first": first, "first_sure": first_sure}


def shares(v):
    """(share of edges in the band, surely blocked, surely free)."""
    return float(v["band"].mean()), float(v["blocked"].mean()), float(v["free"].mean())


def check_edges(blocked, first, v, what=""):
    """Engine (or kernel source) verdicts against verdicts(...): flags exact outside the band, first exact when no earlier sample is in the band."""
    blocked, first = np.asarray(blocked).astype(bool), np.asarray(first)
    sure = ~v["band"]
    bad = sure & (blocked != v["blocked"])
    assert not bad.any(), f"{what}: {int(bad.sum())} verdicts differ from the fp64 reference outside the band, first {np.flatnonzero(bad)[:5]}"
    assert np.array_equal(first >= 0, blocked), f"{what}: the flag and the first blocked sample disagree"
    cmp = sure & v["first_sure"]
    badf = cmp & (first != v["first"])
    assert not badf.any(), f"{what}: the first blocked sample differs on {int(badf.sum())} edges, first {np.flatnonzero(badf)[:5]}"


# ---- the edges of the GPU tests, from fixed seeds ------------------------------------------------------------------------------------------------
_EDGES = {}
_CASES = {}


def edges(which, seed=0):
    """257 edges of chain `which`: a inside the limits, b = a + U(-0.3, 0.3) per joint, both f32."""
    if (which, seed) not in _EDGES:
        orob = H.kin_robots(which)[1]
        rng = np.random.default_rng(4100 + sum(map(ord, which)) + 1000 * seed)
        a = np.asarray(orob.sample_joint_angles(N_EDGES, 0.0, rng), np.float64)
        b = a + rng.uniform(-0.3, 0.3, a.shape)
        _EDGES[(which, seed)] = (np.ascontiguousarray(a, F), np.ascontiguousarray(b, F))
    return _EDGES[(which, seed)]


N_EDGES_LARGE = 66     # with a capsule model of rank_helpers.capsule_models: one workgroup and two threads
# Seeds of the edges of the 24-capsule cases: the first of 0 .. 9 under which, by the fp64 references alone, the share of surely blocked edges lies
# strictly between 10 % and 90 % and at most 2 % of the edges are in the band, under the world rule and under both rules
# (tests/test_sweep_math_host.py asserts it on the CPU).  A chain that is not listed takes seed 0.
LARGE_SEEDS = {"syn4r": 1}


def edge_case(which, scene, S, caps=None, seed=None):
    """-> dict: a, b [n x nd] f32, samples, world (the scene), world_cl / self_cl [n x S] fp64, world_thr - the median over the edges of the
    minimum reference clearance over their samples -, self_thr - rank_helpers.clearance_threshold on the samples.  Computed once.
    caps: a name of rank_helpers.capsule_models (66 edges of seed LARGE_SEEDS, the scene built for that model; self_cl and self_thr are None until
    with_self_rule fills them in: the oracle's self clearance of a large model costs as much as the rest), None: the small model."""
    seed = (0 if caps is None else LARGE_SEEDS.get(which, 0)) if seed is None else seed
    key = (which, scene, S, caps, seed)
    if key not in _CASES:
        orob = H.kin_robots(which)[1]
        model = RH.capsules(which, caps)
        a, b = edges(which, seed)
        n = N_EDGES_LARGE if caps is not None else N_EDGES_FULL64 if scene == "full64" else N_EDGES
        a, b = a[:n], b[:n]
        world = WH.scene(which, scene, caps)
        smp = samples_f32(a, b, S)
        wc, sc = sample_clearances(orob, model, world, smp, want_self=caps is None)
        _CASES[key] = dict(a=a, b=b, samples=smp, world=world, world_cl=wc, self_cl=sc, world_thr=float(np.median(wc.min(1))), which=which, caps=caps,
                           self_thr=None if sc is None else RH.clearance_threshold(orob, model, torch.tensor(smp.reshape(-1, a.shape[1]))))
    return _CASES[key]


def with_self_rule(c):
    """The self clearances and their median of an edge_case of a large capsule model, computed once, on demand."""
    if c["self_cl"] is None:
        orob = H.kin_robots(c["which"])[1]
        n, S, nd = c["samples"].shape
        c["self_cl"] = RH.clearance(orob, RH.capsules(c["which"], c["caps"]), torch.tensor(c["samples"].reshape(n * S, nd))).reshape(n, S)
        c["self_thr"] = float(np.median(c["self_cl"]))
    return c


def shares_hold(v):
    """The condition of the 24-capsule cases on verdicts(...): blocked share strictly between 10 % and 90 %, at most 2 % of the edges in the band."""
    band, blocked, free = shares(v)
    return band <= 0.02 and 0.1 < blocked < 0.9


def case_verdicts(c, rule, n=None):
    """verdicts of the first n edges of an edge_case under rule "world", "self" or "both"."""
    sl = slice(None, n)
    return verdicts(c["world_cl"][sl] if rule in ("world", "both") else None, c["world_thr"],
                    c["self_cl"][sl] if rule in ("self", "both") else None, c["self_thr"])


# ---- the lattice with forbidden edges ---------------------------------------------------------------------------------------------------------------
def dp_f32_masked(q, node, T, k, edge_free=None, start_free=None, q_start=None, node_weight=1.0, max_step=None):
    """path_helpers.dp_f32 with two more forbidden-edge predicates: edge_free [T][k][k] bool (edge_free[t][r][j]: the edge from candidate j of
    waypoint t - 1 to candidate r of waypoint t may be taken; row 0 is not read) and start_free [k] (the start edge to candidate r, read
    only with q_start).  None: no predicate - then it IS dp_f32.  Same outputs, same float32 operations in the same order."""
    q = np.ascontiguousarray(q, dtype=F)
    nd = q.shape[1]
    q = q.reshape(k, T, nd)
    node = np.asarray(node, dtype=F).reshape(k, T)
    nw = F(node_weight)
    step = None if max_step is None or max_step < 0 else F(max_step)
    cost = np.full((T, k), INF, F)
    back = np.zeros((T, k), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        def edges_(a, b):
            s = np.zeros((a.shape[0], b.shape[0]), F)
            ok = np.ones(s.shape, bool)
            for j in range(nd):
                d = b[None, :, j] - a[:, None, j]
                if step is not None:
                    ok &= ~(np.abs(d) > step)
                s = s + d * d
            return np.sqrt(s), ok

        for t in range(T):
            if t == 0:
                if q_start is None:
                    sums = np.zeros((1, k), F)
                else:
                    e, ok = edges_(np.asarray(q_start, F).reshape(1, nd), q[:, 0])
                    if start_free is not None:
                        ok = ok & np.asarray(start_free, bool)[None, :]
                    sums = np.where(ok, F(0.0) + e, INF)
            else:
                e, ok = edges_(q[:, t - 1], q[:, t])
                if edge_free is not None:
                    ok = ok & np.asarray(edge_free[t], bool).T   # [j][r]
                sums = cost[t - 1][:, None] + e
                sums = np.where(ok & (cost[t - 1] < INF)[:, None], sums, INF)
            sums = np.where(sums < INF, sums, INF).astype(F)
            j = np.argmin(sums, axis=0)
            best = sums[j, np.arange(k)]
            c = best + nw * node[:, t]
            c = np.where((node[:, t] < INF) & (best < INF) & (c < INF), c, INF).astype(F)
            cost[t], back[t] = c, j
    reach = (cost < INF).sum(1).astype(np.int32)
    if not (cost[T - 1] < INF).any():
        return np.zeros((T, nd), F), np.full(T, -1, np.int32), INF, reach
    index = np.zeros(T, np.int32)
    index[T - 1] = int(np.argmin(cost[T - 1]))
    for t in range(T - 1, 0, -1):
        index[t - 1] = back[t, index[t]]
    return q[index, np.arange(T)].copy(), index, cost[T - 1, index[T - 1]], reach


def lattice_edges(q, T, k, q_start=None):
    """All edges of a tile-major lattice as two row arrays, in the order [t = 1 .. T - 1][r][j] (k * k * (T - 1) rows), followed - with q_start -
    by the k start edges q_start -> q[0][r]."""
    nd = q.shape[1]
    g = np.ascontiguousarray(q, F).reshape(k, T, nd)
    a = np.broadcast_to(g[None, :, :T - 1].transpose(2, 0, 1, 3), (T - 1, k, k, nd)).reshape(-1, nd)      # [t][r][j] <- g[j][t - 1]
    b = np.broadcast_to(g[:, None, 1:].transpose(2, 0, 1, 3), (T - 1, k, k, nd)).reshape(-1, nd)          # [t][r][j] <- g[r][t]
    if q_start is not None:
        a = np.concatenate([a, np.broadcast_to(np.asarray(q_start, F).reshape(1, nd), (k, nd))])
        b = np.concatenate([b, g[:, 0]])
    return np.array(a, F, order="C"), np.array(b, F, order="C")   # (copies: a broadcast view is read-only)


def split_lattice_verdicts(free, T, k, with_start):
    """free [k * k * (T - 1) (+ k)] bool in lattice_edges' order -> (edge_free [T][k][k] with row 0 all True, start_free [k] or None)."""
    free = np.asarray(free, bool)
    ef = np.ones((T, k, k), bool)
    ef[1:] = free[:k * k * (T - 1)].reshape(T - 1, k, k)
    return ef, (free[k * k * (T - 1):] if with_start else None)


def path_inputs(orob, T, k, seed, step=0.04):
    """T waypoints along a moving configuration (a random walk of `step` rad per joint and waypoint) and k candidates each - the truth plus
    noise of scale logspace(-3, -0.3, k) per candidate, clamped to the limits -, tile-major [k * T x ndof]: the inputs of tests/test_path.py
    with the stride of the walk as a parameter.  -> (poses [T x 7], q, q_true)."""
    g = torch.Generator().manual_seed(500 + seed)
    nd = orob.ndof
    lo, hi = RH.limits(orob)
    start = 0.5 * (lo + hi) + 0.15 * (hi - lo) * torch.randn(1, nd, generator=g)
    q_true = start + torch.cumsum(step * torch.randn(T, nd, generator=g), 0)
    q_true = torch.minimum(torch.maximum(q_true, lo + 0.01), hi - 0.01)
    poses = ko.forward_kinematics(orob, q_true.double()).float().contiguous()
    q = q_true[None] + torch.randn(k, T, nd, generator=g) * torch.logspace(-3, -0.3, k)[:, None, None]
    q = ko.clamp_to_joint_limits(orob, q.reshape(k * T, nd))
    return poses, q.float().contiguous(), q_true.float()


# ---- the lattices of the GPU tests ------------------------------------------------------------------------------------------------------------------
# Thresholds of a lattice case: the lower quartile of the fp64 clearances of its k * T rows (world: the scene "mixed7"; self: the capsule model), so
# that three quarters of the nodes stay admissible and paths exist, while edges between admissible nodes near the threshold dip below it.  The seed
# of a case is the first one for which - by the references and the host build of sweep_math.h, on the CPU - an unswept and a swept path exist and
# the edges between admissible nodes hold blocked and free ones; tests/test_sweep.py asserts the same of the engine's own outputs.
LATTICE_SCENE = "mixed7"
LATTICE_QUANTILE = 0.25
_LATTICES = {}


def lattice_inputs(which, T, k, seed, caps=None):
    """-> dict: poses [T x 7], q [k * T x nd] tile-major, q_start (the truth of waypoint 0 plus 0.05 rad), world, world_cl / self_cl [k * T] fp64,
    world_thr, self_thr.  Computed once.  caps: a name of rank_helpers.capsule_models (and the scene built for it), None: the small model."""
    key = (which, T, k, seed, caps)
    if key not in _LATTICES:
        orob = H.kin_robots(which)[1]
        caps = RH.capsules(which, caps)
        poses, q, q_true = path_inputs(orob, T, k, seed)
        world = WH.scene(which, LATTICE_SCENE, key[4])
        wc = WH.reference(orob, caps, world, q)["clearance"]
        sc = RH.clearance(orob, caps, q)
        # ... but never so high that a waypoint is left without an admissible candidate (few candidates, all close to one colliding truth)
        thr = lambda c: float(min(np.quantile(c, LATTICE_QUANTILE), c.reshape(k, T).max(0).min() - 1e-3))
        _LATTICES[key] = dict(poses=poses, q=q, q_start=(q_true[0] + 0.05).contiguous(), world=world, world_cl=wc, self_cl=sc,
                              world_thr=thr(wc), self_thr=thr(sc))
    return _LATTICES[key]


# seeds of the lattice cases of tests/test_sweep.py, found as described above; at (65, 33) the seed is also the first under which the swept path
# differs from the unswept one and costs more (what the test asserts of that shape).  syn6r: seed 1 is the first by that rule, but the one blocked
# edge of its unswept path lies 3.4e-5 under the threshold, inside the band, where the GPU's verdict need not be the host build's; 7 is the first
# seed under which an edge of the unswept path is surely blocked by the fp64 reference (syn4p at seed 1: three such edges, the deepest 0.033 m).
LATTICE_SEEDS = {("panda", 1, 1): 1, ("panda", 1, 5): 2, ("panda", 2, 3): 3, ("panda", 9, 1): 0, ("panda", 7, 64): 0, ("panda", 3, 65): 0,
                 ("panda", 65, 33): 1, ("panda", 5, 256): 0, ("syn5p", 65, 33): 1, ("fetch", 65, 33): 9,
                 ("syn4p", 65, 33): 1, ("syn6r", 65, 33): 7, ("panda", 3, 128): 0, ("panda", 3, 129): 0, ("panda", 3, 193): 0, ("panda", 66, 65): 0}
# the swept lattice of the 24-capsule model (chain, T, k, samples per edge): the seed is the first of 0 .. 9 for which, by the references and the
# host build on the CPU (tests/test_sweep_math_host.py), a swept path exists and the edges between admissible nodes hold blocked and free ones
LARGE_LATTICE = ("panda", 6, 8, 2)
LARGE_LATTICE_SEED = 1
SELF_RULE_SEED = 3      # (65, 33) with the self rule on top of the world: under seed 1 no swept path is left
STEP_GATE = 0.8         # (65, 33) with a step gate: under 0.5 rad no swept path is left


def crossing_case():
    """Test 6: T = 2, k = 3 on the Panda; the candidates of waypoint 1 are those of waypoint 0 moved by 0.6 rad on joint 1, and a sphere of radius
    0.03 sits on the end point of the last capsule at the middle sample of the edge 0 -> 0.  -> (poses, q tile-major, world, nodes' fp64
    clearances [6], the 9 edges' middle samples' fp64 clearances [9])."""
    from ikflow_amd.world import World

    robot, orob = H.kin_robots("panda")
    caps = RH.collision_capsules(robot)
    a0 = np.asarray(orob.sample_joint_angles(1, 0.4, np.random.default_rng(9)), np.float64)[0]
    a = np.stack([a0 + np.eye(orob.ndof)[3] * 2e-3 * r for r in range(3)]).astype(F)
    b = a.copy()
    b[:, 1] += F(0.6)
    q = np.ascontiguousarray(np.stack([a, b], 1).reshape(6, orob.ndof))   # tile-major: row r * 2 + t
    ea, eb = lattice_edges(q, 2, 3)
    mid = samples_f32(ea, eb, 1)[:, 0]
    E0, _, _ = WH.capsule_ends(orob, caps, torch.tensor(samples_f32(a[:1], b[:1], 1)[:, 0]))
    world = World()
    world.add_sphere(tuple(float(x) for x in E0[0, -1]), 0.03)
    nodes = WH.reference(orob, caps, world, torch.tensor(q))["clearance"]
    mids = WH.reference(orob, caps, world, torch.tensor(mid))["clearance"]
    poses = ko.forward_kinematics(orob, torch.tensor(np.stack([a[0], b[0]])).double()).float().contiguous()
    return poses, torch.tensor(q), world, nodes, mids
