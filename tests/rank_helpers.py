"""Inputs, the fp64 reference and the tolerance of a best-of-K row score, shared by the host build of ikflow_amd/csrc/rank_math.h
(tests/test_rank_math_host.py) and the GPU tests (tests/test_ranked.py).

Tolerance of a row score, from the project's existing figures only (position error 2e-6; rotation error 2e-5 above helpers.ROT_FLOOR and, below
it, the f32 noise that include/ikflow_amd.h documents as 9.3e-4, rounded up to 1e-3; 1e-6 relative on the joint distance):
    eps = 2e-6 + rot_weight * (2e-5 if the fp64 angle > ROT_FLOOR else 1e-3) + 1e-6 * ref_weight * max(1, joint distance)
Admissibility is compared exactly except on rows inside a band around a decision: eps around the position threshold, the rotation figure of eps
(2e-5 / 1e-3, radians) around the rotation threshold, 1e-4 around min_clearance (as test_capsule_geometry_against_the_oracle), one ulp around a limit."""
import numpy as np
import torch

import helpers as H
from oracle import kinematics_oracle as ko

INF = float("inf")


def collision_capsules(robot):
    """The small capsule model of tests/test_kinematics.py (_collision_capsules), rebuilt: base, three moving links, a sphere."""
    act = [j.name for j in robot.joints if j.actuated]
    rng = np.random.default_rng(5)
    caps = [(None, (0.0, 0.0, 0.0), (0.0, 0.0, 0.2), 0.05)]
    for nm in (act[1], act[2], act[-1]):
        caps.append((nm, tuple(rng.uniform(-0.08, 0.08, 3)), tuple(rng.uniform(-0.15, 0.15, 3)), float(rng.uniform(0.03, 0.08))))
    caps.append((act[-1], (0.01, 0.02, 0.03), (0.01, 0.02, 0.03), 0.04))
    return caps


# ---- capsule models by size ---------------------------------------------------------------------------------------------------------------------
# The dynamic LDS of k_rank_candidates, k_world_clearance and k_sweep_edges is sized by the capsule count: a slice of (6 n) | 1 floats per thread.
# k_rank_candidates takes its opt-in for more than 48 KiB between 13 and 14 capsules (tile 64, capacity 16), between 15 and 16 (tile 1, capacity
# 1) and, with a world, between 11 and 12 (tile 64, capacity 16); 24 is IKF_MAX_CAPSULES.  0 and 1 capsules: a slice of one float, no pair.
CAPSULE_COUNTS = (0, 1, 5, 11, 12, 13, 14, 15, 16, 24)
LARGE_COUNTS = CAPSULE_COUNTS[3:]
LDS_OPT_IN = 49152
# (name of the count below, of the count above, tile_poses, n_keep, world) of each crossing of the opt-in line
CROSSINGS = (("caps13", "caps14", 64, 16, False), ("caps15", "caps16", 1, 1, False), ("caps11", "caps12", 64, 16, True))


def capsule_models(robot):
    """{name: capsules} of CAPSULE_COUNTS for this chain: "caps0" (none), "caps1" (one capsule on the last frame), "caps5" (collision_capsules)
    and, from 11 capsules up, the first n of one list of 24 thin capsules (radii 5 .. 15 mm, 2 .. 12 cm long, up to 6 cm off their frame's
    origin): the first ndof + 1 of them sit on the frames 0 .. ndof in turn, the others on frames drawn at random, so every large model occupies
    every frame and some frames carry several capsules.  With such thin capsules no pair overlaps for every q and the closest pair of a row
    changes with q (tests/test_rank_math_host.py asserts on the CPU that the capsules behind the 5th and behind the 16th decide rows)."""
    act = [j.name for j in robot.joints if j.actuated]
    frames = [None] + act
    rng = np.random.default_rng(2400 + len(act))
    order = list(range(len(frames))) + [int(f) for f in rng.integers(0, len(frames), 24 - len(frames))]
    big = []
    for f in order:
        p0 = rng.uniform(-0.06, 0.06, 3)
        d = rng.standard_normal(3)
        p1 = p0 + d / np.linalg.norm(d) * rng.uniform(0.02, 0.12)
        big.append((frames[f], tuple(float(x) for x in p0), tuple(float(x) for x in p1), float(rng.uniform(0.005, 0.015))))
    models = {"caps0": [], "caps1": [(act[-1], (0.01, 0.02, 0.03), (0.04, -0.02, 0.08), 0.04)], "caps5": collision_capsules(robot)}
    for n in LARGE_COUNTS:
        models[f"caps{n}"] = big[:n]
    return models


_MODEL_CACHE = {}


def capsules(which, model=None):
    """The capsule list `model` (a name of capsule_models; None: collision_capsules, the model of the earlier tests) of chain `which`."""
    if (which, model) not in _MODEL_CACHE:
        robot = H.kin_robots(which)[0]
        _MODEL_CACHE[(which, model)] = collision_capsules(robot) if model is None else capsule_models(robot)[model]
    return _MODEL_CACHE[(which, model)]


def tile_poses(m):
    """rank_math.h: rank_tile_poses - the next power of two >= m, at most 64."""
    tp = 1
    while tp < 64 and tp < m:
        tp <<= 1
    return tp


def keep_capacity(n_keep):
    return 1 if n_keep <= 1 else 4 if n_keep <= 4 else 16


def rank_lds_bytes(m, n_keep, n_caps, world=False, slices=True):
    """Dynamic LDS of a k_rank_candidates workgroup (rank_kernels.hip): the hand-over area, the obstacle table with a world, and - `slices`:
    with a world or with reject_collisions - 128 capsule slices."""
    return 4 * (tile_poses(m) * (2 * keep_capacity(n_keep) + 1) + (1024 if world else 0) + (128 * ((6 * n_caps) | 1) if slices else 0))


def all_pairs(n):
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


def clearance(orob, caps, q):
    """ko.capsule_clearance of the rows, fp64 numpy (+inf without a tested pair).  The oracle's cost is one small tensor operation after another -
    some 20 ms per capsule pair, whatever the row count - and more than four threads only slow those down."""
    threads = torch.get_num_threads()
    torch.set_num_threads(min(threads, 4))
    try:
        return ko.capsule_clearance(orob, caps, (), q.double()).numpy()
    finally:
        torch.set_num_threads(threads)


# The ranking cases of the capsule models: (m, k, n_keep).  tile1: one pose, tile 1, capacity 1, one chunk; tile64: tile 64, capacity 16 (a keep
# count inside the class), one chunk; chunked: tile 64, capacity 16, two chunks (528 rows: run with a 14-capsule model, whose reference is cheap).
CASE_SHAPES = {"tile1": (1, 200, 1), "tile64": (33, 5, 5), "chunked": (33, 16, 16)}
CASE_CHAINS = ("syn4r", "panda", "fetch")     # 4, 7 and 8 joints
REJECTING = ("caps5",) + tuple(f"caps{n}" for n in LARGE_COUNTS)
# Seeds of the candidates of a case: the first of 0 .. 9 under which, by the fp64 reference alone, the inadmissible share of the rows lies
# strictly between 10 % and 90 % and at most 2 % of the rows lie inside a band (tests/test_rank_math_host.py asserts both for every case on the
# CPU).  A case that is not listed takes seed 0.  The ranking with a world (tests/test_world.py) runs the tile64 rows of 11, 12 and 24 capsules:
# under these seeds the condition also holds with the world rule, with and without reject_collisions (tests/test_world_math_host.py).
CASE_SEEDS = {('syn4r', 'caps11', 'tile1'): 2, ('syn4r', 'caps11', 'tile64'): 1, ('syn4r', 'caps12', 'tile1'): 2, ('syn4r', 'caps12', 'tile64'): 1,
              ('syn4r', 'caps13', 'tile1'): 2, ('syn4r', 'caps15', 'tile1'): 2, ('syn4r', 'caps15', 'tile64'): 1, ('syn4r', 'caps16', 'tile1'): 2,
              ('syn4r', 'caps16', 'tile64'): 1, ('syn4r', 'caps24', 'tile1'): 5, ('panda', 'caps5', 'tile1'): 2, ('panda', 'caps11', 'tile64'): 7,
              ('panda', 'caps12', 'tile64'): 7, ('panda', 'caps13', 'tile64'): 7, ('panda', 'caps14', 'tile64'): 7,
              ('panda', 'caps14', 'chunked'): 7, ('panda', 'caps15', 'tile64'): 7, ('panda', 'caps16', 'tile64'): 7, ('fetch', 'caps11', 'tile1'): 2,
              ('fetch', 'caps12', 'tile1'): 2, ('fetch', 'caps13', 'tile1'): 2, ('fetch', 'caps14', 'tile1'): 2, ('fetch', 'caps15', 'tile1'): 2,
              ('fetch', 'caps16', 'tile1'): 2, ('fetch', 'caps24', 'tile1'): 1, ('panda', 'caps24', 'chunked'): 1}
_CASES = {}


def capsule_case(which, model, shape, seed=None):
    """-> dict: poses, q, q_ref (rank_helpers.candidates with noise from 0.03 rad up, as world_helpers.rank_case), m, k, n_keep, clearance (the
    fp64 self clearance of the k * m rows under capsule model `model`), min_clearance (its median).  Computed once."""
    seed = CASE_SEEDS.get((which, model, shape), 0) if seed is None else seed
    key = (which, model, shape, seed)
    if key not in _CASES:
        orob = H.kin_robots(which)[1]
        m, k, n_keep = CASE_SHAPES[shape]
        poses, q, q_ref = candidates(orob, m, k, seed=seed, lo_exp=-1.5)
        cl = clearance(orob, capsules(which, model), q)
        _CASES[key] = dict(poses=poses, q=q, q_ref=q_ref, m=m, k=k, n_keep=n_keep, clearance=cl, min_clearance=float(np.median(cl)))
    return _CASES[key]


def shares(ref):
    """(share of the rows inside a band, share of inadmissible rows) of a reference(...)."""
    return float(ref["near"].mean()), float((~ref["admissible"]).mean())


def shares_hold(ref):
    near, bad = shares(ref)
    return near <= 0.02 and 0.1 < bad < 0.9


def limits(orob):
    lo = torch.tensor([l[0] for l in orob.actuated_joints_limits], dtype=torch.float32)
    hi = torch.tensor([l[1] for l in orob.actuated_joints_limits], dtype=torch.float32)
    return lo, hi


def candidates(orob, m, k, seed=0, lo_exp=-3.0, hi_exp=0.0, wild=False):
    """m reachable poses and k candidates each, tile-major [k * m x ndof]: the truth plus noise of scale logspace(lo_exp, hi_exp, k) per repeat,
    clamped to the limits - or, `wild`, left unclamped and stretched so that many rows leave the limits.  Also a reference configuration per pose."""
    g = torch.Generator().manual_seed(1000 + seed)
    q_true, poses = H.reachable_poses(orob, m, 40 + seed)
    scale = torch.logspace(lo_exp, hi_exp, k)
    noise = torch.randn(k, m, orob.ndof, generator=g) * scale[:, None, None]
    q = q_true[None] + noise
    if wild:
        lo, hi = limits(orob)
        q = q + 0.3 * (hi - lo) * torch.randn(k, m, orob.ndof, generator=g) * (torch.rand(k, m, 1, generator=g) < 0.3)
    else:
        q = ko.clamp_to_joint_limits(orob, q.reshape(k * m, -1)).reshape(k, m, -1)
    q_ref = ko.clamp_to_joint_limits(orob, q_true + 0.2 * torch.randn(m, orob.ndof, generator=g))
    return poses.float().contiguous(), q.reshape(k * m, orob.ndof).float().contiguous(), q_ref.float().contiguous()


def clearance_threshold(orob, caps, q):
    """min_clearance for the tests with capsules: the median of the fp64 oracle's clearances of these rows, so that on every chain about half of
    the rows are rejected (with a fixed value every row of a short chain collides with this capsule model, and nothing would be compared)."""
    return float(np.median(ko.capsule_clearance(orob, caps, (), q.double()).numpy()))


def reference(orob, poses, q, k, rot_weight, q_ref=None, ref_weight=0.0, max_pos=None, max_rot=None, reject_limits=False, caps=None,
              min_clearance=0.0, dtype=torch.float64, self_clearance=None):
    """-> dict of numpy arrays over the k * m rows: score (fp64 arithmetic on the f32 inputs, or `dtype`), eps, admissible, near (inside a band).
    self_clearance: the oracle's capsule clearances of these rows under `caps`, where the caller has them already (capsule_case)."""
    m = poses.shape[0]
    tgt = poses.repeat((k, 1))
    pe, re = ko.calculate_pose_error(orob, q.to(dtype), tgt.to(dtype))
    _, re64 = (pe, re) if dtype == torch.float64 else ko.calculate_pose_error(orob, q.double(), tgt.double())
    pe, re, re64 = pe.double().numpy(), re.double().numpy(), re64.numpy()
    rot_fig = np.where(re64 > H.ROT_FLOOR, 2e-5, 1e-3)
    score = pe + rot_weight * re
    eps = 2e-6 + rot_weight * rot_fig
    if q_ref is not None:
        dist = torch.norm(q.to(dtype) - q_ref.repeat((k, 1)).to(dtype), dim=1).double().numpy()
        score = score + ref_weight * dist
        eps = eps + 1e-6 * ref_weight * np.maximum(1.0, dist)
    adm = np.isfinite(score)
    near = np.zeros_like(adm)
    if max_pos is not None:
        adm &= pe < max_pos
        near |= np.abs(pe - max_pos) <= eps
    if max_rot is not None:
        adm &= re < max_rot
        near |= np.abs(re - max_rot) <= rot_fig
    if reject_limits:
        adm &= ~ko.calculate_joint_limits_exceeded(q, orob.actuated_joints_limits).numpy()
        lo, hi = limits(orob)
        qn = q.numpy()
        ulp = np.spacing(np.maximum(np.abs(lo.numpy()), np.abs(hi.numpy())))
        near |= ((np.abs(qn - lo.numpy()) <= ulp) | (np.abs(qn - hi.numpy()) <= ulp)).any(1)
    if caps is not None:
        cl = ko.capsule_clearance(orob, caps, (), q.double()).numpy() if self_clearance is None else np.asarray(self_clearance)
        adm &= ~(cl < min_clearance)
        near |= np.abs(cl - min_clearance) <= 1e-4
    return {"score": score, "eps": eps, "admissible": adm, "near": near}


def check_row_scores(got, ref, what=""):
    """`got` [k * m] f32 row scores (+inf = inadmissible) against reference(...): admissibility exact outside the bands, every admissible row
    within its eps.  Returns the worst |difference| / eps (printed by the callers)."""
    got = np.asarray(got, dtype=np.float64)
    sure = ~ref["near"]
    bad = sure & (np.isfinite(got) != ref["admissible"])
    assert not bad.any(), f"{what}: admissibility differs on {int(bad.sum())} rows outside every band, first {np.flatnonzero(bad)[:5]}"
    both = np.isfinite(got) & ref["admissible"]
    assert both.any(), f"{what}: no admissible row to compare"
    ratio = np.abs(got[both] - ref["score"][both]) / ref["eps"][both]
    assert ratio.max() <= 1.0, f"{what}: a row score is {ratio.max():.2f} x its tolerance from the fp64 reference"
    return float(ratio.max())


def select(row_scores, m, k, n_keep):
    """numpy selection of a pose's best n_keep: stable lexsort (score, then repeat index) of its finite scores -> (index [m x n_keep] int32,
    score [m x n_keep] f32, count [m] int32); unfilled slots -1 / +inf."""
    s = np.asarray(row_scores, dtype=np.float32).reshape(k, m)
    idx = np.full((m, n_keep), -1, np.int32)
    sc = np.full((m, n_keep), np.inf, np.float32)
    cnt = np.isfinite(s).sum(0).astype(np.int32)
    rep = np.arange(k)
    for j in range(m):
        order = np.lexsort((rep, s[:, j]))
        order = order[np.isfinite(s[order, j])][:n_keep]
        idx[j, :len(order)] = order
        sc[j, :len(order)] = s[order, j]
    return idx, sc, cnt
