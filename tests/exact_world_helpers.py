"""Exact IK under the exact collision rule (include/ikflow_amd_exact_world.h): the cases, the fp64 references and the host statement of the
definition that the oracle-only checks (tests/test_exact_world_inputs.py) and the GPU tests (tests/test_exact_world.py) share.

Nothing here is a new tolerance.  Rows come from the project's oracle loop (refine_helpers.oracle_refine: ko.lm_step, ko.calculate_pose_error),
clearances from world_helpers.reference, cloud_helpers.reference and rank_helpers.clearance (ko.capsule_clearance), the band is world_helpers.BAND
(1e-4 m) around a threshold, and a threshold is the median of the candidate rows' reference clearances (world_helpers.threshold; between two
rows' values also for an odd count: threshold_between).

One departure, with its reason: three rules at their medians reject a row when ANY of them does, so the admissible share of a case with all three
can fall far below a half (an eighth if the clearances were independent).  A case with more than one rule therefore takes, for every rule, the
quantile 1 - 0.5 ** (1 / rules) of that rule's clearances - the median for one rule, 0.29 for two, 0.21 for three - which rejects about half of the
candidates overall if the rules were independent.  The share conditions (>= 20 % rejected, >= 20 % admissible, <= 5 % of the poses in the band)
are asserted per case on the CPU."""
import collections
import functools

import numpy as np
import torch

import cloud_helpers as CH
import exact_helpers as X
import helpers as H
import rank_helpers as RH
import refine_helpers as RF
import world_helpers as WH
from ikflow_amd.world import World
from oracle import kinematics_oracle as ko

POS_THR, ROT_THR = X.POS_THR, X.ROT_THR
BAND = WH.BAND
BAND_SHARE_CAP = 0.05
MIN_SHARE = 0.20
ELBOW = 2             # capsule of the small model that rides behind the third actuated joint: where it is depends on the first three joints only
SPHERE_RADIUS = 0.05
CALM = (0.01, 0.05, 0.2)   # noise levels of the seeds (rad or m): most rows arrive within three steps, at different iterations

# name: chain, LM arithmetic, n_lm_steps, active poses, repeats, capsule model (None: the small one of rank_helpers.collision_capsules = "caps5"),
#       world (None / "one" / "mixed7" / "full64"), cloud points (0: none), self rule, seed
Case = collections.namedtuple("Case", "name which lm steps n R caps world cloud reject_self seed")
CASES = (
    Case("syn4r-world", "syn4r", "f64", 3, 64, 1, None, "mixed7", 0, False, 11),
    Case("syn5p-one-f32-1step", "syn5p", "f32", 1, 13, 5, None, "one", 0, False, 12),
    Case("syn6r-self-20steps", "syn6r", "f64", 20, 64, 1, None, None, 0, True, 13),
    Case("panda-cloud512", "panda", "f64", 3, 65, 1, None, None, 512, False, 14),
    Case("fetch-all-f32", "fetch", "f32", 3, 257, 1, None, "mixed7", 513, True, 15),
    Case("panda-world-200x10", "panda", "f64", 3, 200, 10, None, "mixed7", 0, False, 16),
    Case("panda-caps24-full64-f32", "panda", "f32", 3, 7, 9, "caps24", "full64", 0, False, 17),
    Case("panda-caps1-cloud1", "panda", "f64", 3, 65, 1, "caps1", "mixed7", 1, False, 18),
    Case("panda-full64-1step", "panda", "f64", 1, 257, 1, None, "full64", 0, False, 19),
    Case("syn6r-world-self-f32-20steps", "syn6r", "f32", 20, 65, 1, None, "mixed7", 0, True, 20),
    Case("fetch-cloud4096", "fetch", "f64", 3, 65, 1, None, None, 4096, False, 21),
    Case("syn5p-world-cloud", "syn5p", "f64", 3, 64, 1, None, "full64", 513, False, 22),
)
CASE_BY_NAME = {c.name: c for c in CASES}
LM_DTYPE = {"f64": torch.float64, "f32": torch.float32}


def capsules_of(case):
    """"elbow3": the first three capsules of the small model (base and the two behind the second and third joint) - none rides on the tool, so
    the clearance of a configuration is not fixed by the pose it reaches."""
    if case.caps == "elbow3":
        return RH.capsules(case.which, None)[:3]
    return RH.capsules(case.which, case.caps)


def world_of(case):
    """The case's World (None without one).  The scenes are world_helpers'; a model of one capsule has no moving end points to build a scene
    around, so it meets the scene of the small model; "one": the first obstacle of mixed7."""
    if case.world is None:
        return None
    scene_caps = None if case.caps in (None, "caps1", "caps0", "elbow3") else case.caps
    if case.world == "one":
        w = World()
        w._add(*WH.scene(case.which, "mixed7", scene_caps).obstacles[0])
        return w
    return WH.scene(case.which, case.world, scene_caps)


def cloud_of(case):
    if not case.cloud:
        return None
    return CH.cloud(case.which, case.cloud, None if case.caps in (None, "caps1", "caps0", "elbow3") else case.caps)


def _draw(c, seed):
    q_true = X.truth(c.which, c.n, seed)
    poses = ko.forward_kinematics(X.orob_of(c.which), q_true)
    seeds = X.seed_tables(c.which, q_true, (c.R,), 1000 + seed, sigmas=CALM)[0].reshape(c.R * c.n, -1).contiguous()
    return poses, seeds


def _rows_of(c, poses, seeds):
    q, steps, conv, margins = RF.oracle_refine(X.orob_of(c.which), poses.repeat(c.R, 1), seeds, c.steps, POS_THR, ROT_THR, lm_dtype=LM_DTYPE[c.lm])
    first = torch.where(conv, steps, torch.zeros_like(steps)).numpy()
    cl = reference_clearances(c, q)
    cand = first > 0
    quant = 1.0 - 0.5 ** (1.0 / max(1, len(cl)))
    thr = {k: threshold_between(v[cand], quant) for k, v in cl.items()}
    return q, first, cl, thr, RF.band_of(margins, POS_THR, ROT_THR)


def _shares_of(c, first, cl, thr):
    cand = first > 0
    rej, near = rejected_of(cl, thr), in_band(cl, thr)
    return (int(cand.sum()), float((cand & rej & ~near).sum() / max(1, cand.sum())), float((cand & ~rej & ~near).sum() / max(1, cand.sum())),
            float(band_poses(first, near, c.n, c.R).mean()))


@functools.lru_cache(maxsize=None)
def _chosen(name):
    """The case's draw: the first of the seeds c.seed, c.seed + 100, ... whose rows meet, by the oracle and the fp64 references alone, the
    conditions the GPU test rests on (the device of cloud_helpers._scene and world_helpers.scene, which redraw until theirs hold).  With 7 or 13
    poses a single pose in the band is 14 % or 8 %: such a case needs a draw with none."""
    c = CASE_BY_NAME[name]
    for attempt in range(16):
        poses, seeds = _draw(c, c.seed + 100 * attempt)
        rows = _rows_of(c, poses, seeds)
        cand, rejected, admissible, band = _shares_of(c, *rows[1:4])
        if cand >= 0.3 * c.n * c.R and band <= BAND_SHARE_CAP and rejected >= MIN_SHARE and admissible >= MIN_SHARE:
            return poses, seeds, rows
    raise AssertionError(f"{name}: no draw met the conditions")


def inputs(name):
    """-> (poses [n x 7] f32, seeds [R * n x ndof] f32 tile-major: row r * n + j = repeat r of pose j)."""
    return _chosen(name)[:2]


def reference_clearances(case, q):
    """fp64 reference clearances of the rows q under every rule the case applies -> {"world" / "cloud" / "self": [rows] float64}."""
    orob, caps = X.orob_of(case.which), capsules_of(case)
    out = {}
    if case.world is not None:
        out["world"] = WH.reference(orob, caps, world_of(case), q)["clearance"]
    if case.cloud:
        out["cloud"] = CH.reference(orob, caps, cloud_of(case), CH.POINT_RADIUS, q)
    if case.reject_self:
        out["self"] = RH.clearance(orob, caps, q)
    return out


def oracle_rows(name):
    """The round's rows by the oracle alone: -> (q [rows x ndof] f32 at the row's last step, first [rows] int64 - the 1-based iteration of the
    candidate, 0: none -, reference clearances of every row at that q, thresholds per rule).  Thresholds: see the module text."""
    return _chosen(name)[2][:4]


def oracle_lm_band(name):
    """Rows for which some iteration of the oracle's loop had a pose error within rounding of its threshold (refine_helpers.band_of)."""
    return _chosen(name)[2][4]


def threshold_between(values, quant):
    """The quantile `quant` of `values` as the midpoint between two neighbouring values of the sorted list: world_helpers.threshold (the median)
    for an even count and quant 0.5.  For an odd count numpy's median IS one row's own clearance, which would put that row's pose in the band by
    construction (one pose of 7 is 14 %); the midpoint below the middle value is the median of the rows without the largest one."""
    v = np.sort(np.asarray(values, np.float64))
    assert len(v) >= 2
    k = min(max(int(np.floor(quant * len(v))), 1), len(v) - 1)
    return float(0.5 * (v[k - 1] + v[k]))


def rejected_of(cl, thr):
    """The admissibility predicate of the definition on clearance tables: a row is rejected when any applicable clearance is < its threshold."""
    rej = np.zeros(len(next(iter(cl.values()))), bool) if cl else np.zeros(0, bool)
    for k, v in cl.items():
        rej |= np.asarray(v) < thr[k]
    return rej


def in_band(cl, thr):
    near = np.zeros(len(next(iter(cl.values()))), bool)
    for k, v in cl.items():
        near |= np.abs(np.asarray(v, np.float64) - thr[k]) <= BAND
    return near


def select(first, rejected, n, R):
    """The selection of the definition, on the host: per pose the admissible row of the earliest iteration, among those the highest repeat.
    first [R * n] (0: no candidate), rejected [R * n] bool -> winner [n] int64 (the repeat, -1: none)."""
    it = np.where((first > 0) & ~rejected, first, 1 << 30).reshape(R, n).astype(np.int64)
    best = it.min(0)
    winner = np.full(n, -1, np.int64)
    for r in range(R):   # ascending: a later (higher) repeat of the same iteration overwrites
        winner[(it[r] == best) & (best < (1 << 30))] = r
    return winner


def band_poses(first, near, n, R):
    """Poses one of whose CANDIDATE rows has a reference clearance within the band of an applicable threshold."""
    return ((first > 0) & near).reshape(R, n).any(0)


def shares(name):
    """From the oracle alone -> (candidate rows, share of them surely rejected, share surely admissible, share of poses in the band)."""
    _, first, cl, thr = oracle_rows(name)
    return _shares_of(CASE_BY_NAME[name], first, cl, thr)


# ---- 4. a colliding sibling stops nobody -----------------------------------------------------------------------------------------------------
SIBLING_CASES = {"R2": ("panda", 300, 2, 31), "R10": ("panda", 80, 10, 32)}
SIBLING_MIN = 5
SIBLING_STEPS = 5
SIBLING_RADIUS = 0.005
CLOUD_QUANTILE = 0.2


def elbow_world(which, radius=SPHERE_RADIUS):
    """-> (World of one sphere of that radius on the middle of the elbow capsule's axis at a fixed configuration qe, qe [1 x ndof])."""
    orob = X.orob_of(which)
    qe = torch.tensor(orob.sample_joint_angles(1, 0.3, np.random.default_rng(55))).float()
    E0, E1, _ = WH.capsule_ends(orob, RH.capsules(which, None), qe)
    world = World()
    world.add_sphere(0.5 * (E0[0, ELBOW] + E1[0, ELBOW]), radius)
    return world, qe


@functools.lru_cache(maxsize=None)
def sibling_case(name, with_cloud=False):
    """Poses with a repeat that is a candidate at iteration 1 and rejected, and another repeat that is a candidate at iteration >= 2 and
    admissible and that the definition selects.  Every pose is FK(q0) with q0 = qe in its first three joints: its elbow capsule sits on the
    sphere of elbow_world (5 mm; min_clearance 0; SIBLING_STEPS LM steps).  Seeds are exact_helpers.seed_tables' with the noise levels mixed WITHIN a pose (seed_tables draws
    one level per pose): repeat r of pose j comes from a calm table (0.01, 0.05) when r + j is even and from a wide one (0.3, 0.6) otherwise - the
    calm repeats arrive at once, next to q0 and inside the sphere; the wide ones arrive later, elsewhere on the pose's solution family, some of
    them outside; the early repeat is the lower one for half of the poses and the higher one for the others.  with_cloud: also a cloud of 513
    points (cloud_helpers) at the 0.2 quantile of the candidates' reference clearances.
    -> dict(case, poses, seeds, n, R, world, thr, first, rejected, winner, siblings: bool [n], by the oracle and outside the band)."""
    which, n, R, seed = SIBLING_CASES[name]
    c = Case(f"sibling-{name}", which, "f64", SIBLING_STEPS, n, R, None, "elbow", 513 if with_cloud else 0, False, seed)
    orob = X.orob_of(which)
    world, qe = elbow_world(which, SIBLING_RADIUS)
    q_true = X.truth(which, n, seed, eps=0.3)
    q_true[:, :3] = qe[0, :3]
    poses = ko.forward_kinematics(orob, q_true)
    calm = X.seed_tables(which, q_true, (R,), 2000 + seed, sigmas=(0.01, 0.05))[0]
    wide = X.seed_tables(which, q_true, (R,), 3000 + seed, sigmas=(0.3, 0.6))[0]
    even = ((torch.arange(R)[:, None] + torch.arange(n)[None, :]) % 2 == 0)[:, :, None]
    seeds = torch.where(even, calm, wide).reshape(R * n, -1).contiguous()
    q, steps, conv, _ = RF.oracle_refine(orob, poses.repeat(R, 1), seeds, SIBLING_STEPS, POS_THR, ROT_THR)
    first = torch.where(conv, steps, torch.zeros_like(steps)).numpy()
    caps = RH.capsules(which, None)
    cl = {"world": WH.reference(orob, caps, world, q)["clearance"]}
    thr = {"world": 0.0}
    if with_cloud:
        cl["cloud"] = CH.reference(orob, caps, cloud_of(c), CH.POINT_RADIUS, q)
        thr["cloud"] = threshold_between(cl["cloud"][first > 0], CLOUD_QUANTILE)
    rej, near = rejected_of(cl, thr), in_band(cl, thr)
    winner = select(first, rej, n, R)
    siblings = sibling_poses(first, rej, winner, n, R) & ~band_poses(first, near, n, R)
    return dict(case=c, poses=poses, seeds=seeds, n=n, R=R, world=world, thr=thr, first=first, rejected=rej, winner=winner, siblings=siblings)


@functools.lru_cache(maxsize=None)
def sibling_cloud_case(name):
    """sibling_case with the sphere as a CLOUD and no primitive: one point at the sphere's centre (point radius cloud_helpers.POINT_RADIUS,
    min_clearance 0) - the round then runs the plain loop in front of the cloud's mask, the path on which an early-exit hint would be live."""
    which, n, R, seed = SIBLING_CASES[name]
    s = sibling_case(name)
    orob, caps = X.orob_of(which), RH.capsules(which, None)
    points = np.asarray([s["world"].obstacles[0][1]], np.float32)
    q, steps, conv, _ = RF.oracle_refine(orob, s["poses"].repeat(R, 1), s["seeds"], SIBLING_STEPS, POS_THR, ROT_THR)
    first = torch.where(conv, steps, torch.zeros_like(steps)).numpy()
    cl = {"cloud": CH.reference(orob, caps, points, CH.POINT_RADIUS, q)}
    thr = {"cloud": 0.0}
    rej, near = rejected_of(cl, thr), in_band(cl, thr)
    winner = select(first, rej, n, R)
    siblings = sibling_poses(first, rej, winner, n, R) & ~band_poses(first, near, n, R)
    return dict(which=which, poses=s["poses"], seeds=s["seeds"], n=n, R=R, points=points, thr=thr, first=first, rejected=rej, winner=winner, siblings=siblings)


def sibling_poses(first, rejected, winner, n, R):
    early_rejected = ((first == 1) & rejected).reshape(R, n).any(0)
    win_it = np.where(winner >= 0, first.reshape(R, n)[np.maximum(winner, 0), np.arange(n)], 0)
    return early_rejected & (win_it >= 2)


# ---- 5. retry rounds: round 0's truth seeds sit inside an obstacle ----------------------------------------------------------------------------
ROUNDS_CHAIN = "panda"
MARGIN = 0.01         # metres, by fp64: how deep round 0's candidates sit in the sphere, and how clear round 1's are
ROUNDS_RC = (2, 3)


@functools.lru_cache(maxsize=None)
def blocked_case(n, kind, seed=0):
    """The three_round_case variant of the rule.  One sphere of 5 cm sits on the middle of the elbow capsule's axis at a configuration qe; the
    world's min_clearance is 0.  A BLOCKED pose (exact_helpers.make_pattern(kind, n) marks them; "all": every pose) is FK(q0) with q0 = qe in its
    first three joints and random behind them - so its elbow capsule is where qe's is, at least SPHERE_RADIUS + its own radius deep - and its
    round-0 seeds are q0 (valid after one step, exact_helpers.pattern_inputs).  Its round-1 seeds are q1: another solution of the same pose,
    found by the oracle's LM from q0 with the first three joints moved by 0.6 .. 1.2 rad, kept only when the oracle finds it valid after one more
    step and clear of the sphere by MARGIN; a pose without such a q1 is drawn again.  A FREE pose is FK(q0) of a random q0 that is clear by
    MARGIN; q0 is its seed in both rounds (round 1 never sees it).
    -> dict(poses, seeds0 [n x ndof], seeds1 [n x ndof], blocked bool [n], world)."""
    orob = X.orob_of(ROUNDS_CHAIN)
    caps = RH.capsules(ROUNDS_CHAIN, None)
    blocked = np.ones(n, bool) if kind == "all" else X.make_pattern(kind, n, seed)
    rng = np.random.default_rng(5000 + n + seed)
    world, qe = elbow_world(ROUNDS_CHAIN)

    def clear(q):
        return WH.reference(orob, caps, world, q)["clearance"]

    def one_step(poses, q):
        qq, _, conv, margins = RF.oracle_refine(orob, poses, q, 1, POS_THR, ROT_THR)
        return qq, conv.numpy() & ~RF.band_of(margins, POS_THR, ROT_THR)

    q0 = torch.zeros(n, orob.ndof)
    q1 = torch.zeros(n, orob.ndof)
    todo = np.arange(n)
    for attempt in range(40):
        if len(todo) == 0:
            break
        m = len(todo)
        draw = torch.tensor(orob.sample_joint_angles(m, 0.3, np.random.default_rng(int(rng.integers(1 << 30))))).float()
        is_b = torch.from_numpy(blocked[todo])
        draw[is_b, :3] = qe[0, :3]
        poses = ko.forward_kinematics(orob, draw)
        c0, ok0 = one_step(poses, draw)
        cl0 = clear(c0)
        alt = draw.clone()
        sign = torch.from_numpy(rng.choice([-1.0, 1.0], (m, 3))).float()
        alt[:, :3] += sign * torch.from_numpy(rng.uniform(0.6, 1.2, (m, 3))).float()
        alt = ko.clamp_to_joint_limits(orob, alt)
        alt, _, conv, _ = RF.oracle_refine(orob, poses, alt, 30, 1e-5, 2e-3)
        c1, ok1 = one_step(poses, alt)
        cl1 = clear(c1)
        good_b = ok0 & (cl0 <= -MARGIN) & conv.numpy() & ok1 & (cl1 >= MARGIN)
        good_f = ok0 & (cl0 >= MARGIN)
        good = np.where(is_b.numpy(), good_b, good_f)
        q0[todo[good]] = draw[good]
        q1[todo[good]] = torch.where(is_b[good][:, None], alt[good], draw[good])
        todo = todo[~good]
    assert len(todo) == 0, f"blocked_case({n}, {kind}): {len(todo)} poses found no configuration"
    return dict(poses=ko.forward_kinematics(orob, q0), seeds0=q0.contiguous(), seeds1=q1.contiguous(), blocked=blocked, world=world)


def blocked_margins(c):
    """From the oracle alone: (deepest allowed clearance of the blocked poses' round-0 candidates - their maximum -, the least clearance of
    round 1's candidates of the blocked poses, the least clearance of the free poses' round-0 candidates, all candidates valid outside the band)."""
    orob, caps = X.orob_of(ROUNDS_CHAIN), RH.capsules(ROUNDS_CHAIN, None)
    b = c["blocked"]
    out, valid = [], True
    for seeds, rows in ((c["seeds0"], b), (c["seeds1"], b), (c["seeds0"], ~b)):
        if not rows.any():
            out.append(None)
            continue
        idx = torch.from_numpy(np.flatnonzero(rows))
        q, _, conv, margins = RF.oracle_refine(orob, c["poses"][idx], seeds[idx], 1, POS_THR, ROT_THR)
        valid = valid and bool(conv.all()) and not RF.band_of(margins, POS_THR, ROT_THR).any()
        out.append(WH.reference(orob, caps, c["world"], q)["clearance"])
    return (None if out[0] is None else float(out[0].max()), None if out[1] is None else float(out[1].min()),
            None if out[2] is None else float(out[2].min()), valid)
