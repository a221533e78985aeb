"""Exact IK that obeys the world on the GPU (include/ikflow_amd_exact_world.h; ikflow_amd/csrc/exact_world_kernels.hip, exact_world_math.h,
api_exact_world.hip and the call site in run_exact, api_kin.hip).

1.  Off means off: rule off, and rule on with nothing to test against, equal the plain call bit for bit (sol, valid, all four stats columns), with
    64 guard rows around the outputs.
2.  Equals its parts: every row's (first iteration, candidate bits) is rebuilt from ikf_refine_exact with the rule off at 1 .. N steps, the rows'
    clearances come from ikf_world_clearance / ikf_cloud_clearance / ikf_self_collision, the selection is predicted on the host, and the rule-on
    call must give exactly that: flags, rows bit for bit, the rejected count.  Poses with a candidate whose fp64 reference clearance is within 1e-4 of
    a threshold are held to "one of its candidate rows, or zeros".
3.  By fp64, independent of the engine's clearances: what is returned valid reaches the pose and is clear by the references; the flags are the
    oracle schedule's outside the bands.
4.  A colliding sibling stops nobody.   5.  Retry rounds.   6.  The flow in.   7.  Statuses and wrappers.

The conditions these inputs rest on are checked on the CPU by tests/test_exact_world_inputs.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import cloud_helpers as CH
import exact_helpers as X
import exact_world_helpers as EW
import helpers as H
import rank_helpers as RH
import refine_helpers as RF
import world_helpers as WH
from ikflow_amd import _lib
from oracle import kinematics_oracle as ko

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
NAN_BITS = 0x7FC00000
POS, ROT = EW.POS_THR, EW.ROT_THR
_ENGINES = {}


def _eng(which, tag="a"):
    """An engine of this module's own per (chain, tag): the rule, the world and the cloud are state of the handle, and the handles of
    kinematics_engine_for are shared with every other test module."""
    if (which, tag) not in _ENGINES:
        from ikflow_amd.engine import Engine
        from ikflow_amd.model import FlowLayout

        robot = H.kin_robots(which)[0]
        _ENGINES[(which, tag)] = Engine(FlowLayout(nb_nodes=1, dim=max(robot.ndof, 2), dim_cond=8, width=256, n_hidden=1, clamp=2.5, ndof=robot.ndof), robot, DEV)
    return _ENGINES[(which, tag)]


def _set_capsules(eng, which, caps):
    """The capsule list on the engine, folded by the robot as everywhere; the shared robot gets its small model back."""
    robot = H.kin_robots(which)[0]
    robot.set_collision_capsules(caps)
    eng.set_collision_model(*robot._collision_model)
    robot.set_collision_capsules(RH.collision_capsules(robot))


def _scene(eng, which, caps, world=None, world_thr=0.0, cloud=None, cloud_thr=0.0, rule=(False, False, 0.0), lm="f64"):
    _set_capsules(eng, which, caps)
    if world is None:
        eng.clear_world()
    else:
        eng.set_world(world, world_thr)
    if cloud is None:
        eng.clear_world_cloud()
    else:
        eng.set_world_cloud(cloud, CH.POINT_RADIUS, cloud_thr)
    eng.set_exact_collision(*rule)
    eng.set_lm_precision(lm)


@pytest.fixture(autouse=True)
def _plain_engines_afterwards():
    yield
    for eng in _ENGINES.values():
        eng.set_exact_collision(False)
        eng.clear_world()
        eng.clear_world_cloud()
        eng.set_lm_precision("f64")


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


def _windows(n, ndof):
    q = torch.full((n + 2 * GUARD, ndof), float("nan"), dtype=torch.float32, device=DEV)
    v = torch.full((n + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    return q, v, q[GUARD:GUARD + n], v[GUARD:GUARD + n]


def _guards_untouched(q, v, n):
    for part in (q[:GUARD], q[GUARD + n:]):
        assert bool((part.view(torch.int32) == NAN_BITS).all()), "a row outside the window of sol was written"
    for part in (v[:GUARD], v[GUARD + n:]):
        assert bool((part == 0xAB).all()), "a flag outside the window of valid was written"


def _gather(n):
    def rows(idx):
        assert idx.dtype == np.int32
        if len(idx):
            assert idx.min() >= 0 and idx.max() < n, (int(idx.min()), int(idx.max()), n)
        return torch.from_numpy(idx.astype(np.int64)).to(DEV)
    return rows


def _table_seed_fn(tables, n):
    """tables: per round [R x n x ndof] on the device -> the callback of run_seeded_raw (the rows of the engine's list, tile-major)."""
    rows = _gather(n)
    return lambda rnd, idx, repeat: tables[rnd][:, rows(idx)].reshape(-1, tables[rnd].shape[2]).contiguous()


def _seeded(eng, poses, rc, steps, seed_fn, guarded=True):
    n, ndof = poses.shape[0], eng.layout.ndof
    q, v, sol, valid = _windows(n, ndof)
    out = X.run_seeded_raw(eng, poses, rc, POS, ROT, steps, seed_fn, sol=sol, valid=valid, stats_fill=-1)
    _guards_untouched(q, v, n)
    return sol.clone(), valid.clone(), out[2], out[3]


def _refine_raw(eng, poses, seeds, R, steps, expect=_lib.IKF_OK):
    """ikf_refine_exact through eng.lib on guarded windows -> (sol, valid uint8); on a refused call the windows must be untouched."""
    n, ndof = poses.shape[0], eng.layout.ndof
    q, v, sol, valid = _windows(n, ndof)
    torch.cuda.synchronize()
    code = eng.lib.ikf_refine_exact(eng._h, poses.data_ptr(), n, R, seeds.data_ptr(), steps, POS, ROT, sol.data_ptr(), valid.data_ptr(), eng._stream())
    torch.cuda.synchronize()
    assert code == expect, (code, _lib.last_error(eng.lib))
    _guards_untouched(q, v, n)
    if expect != _lib.IKF_OK:
        assert bool((sol.view(torch.int32) == NAN_BITS).all()) and bool((valid == 0xAB).all()), "a refused call wrote to its outputs"
    return sol.clone(), valid.clone()


# ---- 1. off means off ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,n", [("panda", 200), ("syn4r", 17), ("fetch", 17)])
def test_rule_off_and_nothing_to_test_against_are_the_plain_call_bit_for_bit(which, n):
    """ikf_generate_exact_seeded with rc (1, 3, 10) and ikf_refine_exact (R = 3): plain; rule on with an empty world, no cloud and reject_self off;
    rule on then off again with a world set; and a world set but the rule off - all four give the same sol, valid and stats, bit for bit."""
    eng = _eng(which)
    rc = (1, 3, 10)
    q_true = X.truth(which, n, 90 + n)
    poses = ko.forward_kinematics(X.orob_of(which), q_true).to(DEV).contiguous()
    tables = [t.to(DEV) for t in X.seed_tables(which, q_true, rc, 91 + n)]
    fn = _table_seed_fn(tables, n)
    seeds3 = tables[1].reshape(3 * n, -1).contiguous()
    caps = RH.capsules(which, None)
    world = WH.scene(which, "mixed7")

    def both():
        return _seeded(eng, poses, rc, 3, fn), _refine_raw(eng, poses, seeds3, 3, 3)

    _scene(eng, which, caps)
    plain = both()
    assert plain[0][2][0, 3] < n and plain[0][2][:, 3].sum() > 0            # several rounds ran, something was solved
    assert eng.exact_collision_rejected() == [0] * 8
    states = {"on, nothing to test against": dict(rule=(True, False, 0.0)),
              "on with a self threshold but reject_self off": dict(rule=(True, False, 0.5)),
              "off with a world": dict(world=world, world_thr=10.0),
              "off with a world and a cloud": dict(world=world, world_thr=10.0, cloud=CH.cloud(which, 513), cloud_thr=10.0)}
    for label, kw in states.items():
        _scene(eng, which, caps, **kw)
        got = both()
        assert _same(got[0][0], plain[0][0]) and _same(got[0][1], plain[0][1]) and np.array_equal(got[0][2], plain[0][2]), (which, label)
        assert all(np.array_equal(a, b) for a, b in zip(got[0][3], plain[0][3])), (which, label)
        assert _same(got[1][0], plain[1][0]) and _same(got[1][1], plain[1][1]), (which, label)
        assert eng.exact_collision_rejected() == [0] * 8, (which, label)


@pytest.mark.parametrize("name,n", [("T", 200), ("R8", 17)])
def test_rule_off_and_nothing_to_test_against_are_the_plain_flow_call_bit_for_bit(name, n):
    """ikf_generate_exact (the flow in) on the tiny panda model at 200 poses and the 8-joint model at 17."""
    from test_exact_flow import _case
    from test_flow_sample import _eng as flow_eng

    case = f"{name}-{n}"
    _, P, lats, rc, pos_thr, rot_thr = _case(case)
    eng = flow_eng(name)
    try:
        plain = X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, X.FLOW_STEPS, lats, stats_fill=-1)
        eng.set_exact_collision(True, False, 0.0)
        got = X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, X.FLOW_STEPS, lats, stats_fill=-1)
        assert _same(got[0], plain[0]) and _same(got[1], plain[1]) and np.array_equal(got[2], plain[2]) and got[3] == plain[3], case
        assert eng.exact_collision_rejected() == [0] * 8
    finally:
        eng.set_exact_collision(False)


# ---- 2. equals its parts --------------------------------------------------------------------------------------------------------------------------
def _reconstruct(eng, poses_tiled, seeds, steps):
    """With the rule off: ikf_refine_exact with repeat 1 on the tiled poses at n_lm_steps = 1 .. steps.  The first N at which a row is valid is its
    iteration, that call's row its candidate; a row valid at N keeps its bits at every later N (it is not stepped further).
    -> (first [rows] int64 numpy, candidate [rows x ndof] device)."""
    assert eng.exact_collision()[0] is False
    rows = seeds.shape[0]
    first = torch.zeros(rows, dtype=torch.int64, device=DEV)
    cand = torch.zeros_like(seeds)
    for N in range(1, steps + 1):
        sol, valid = eng.refine_exact(poses_tiled, seeds, 1, POS, ROT, n_lm_steps=N)
        seen = first > 0
        assert bool(valid[seen].all()) and _same(sol[seen], cand[seen]), N
        new = valid & ~seen
        first[new] = N
        cand[new] = sol[new]
    return first.cpu().numpy(), cand


def _engine_rejected(eng, c, thr, cand):
    """The rows' verdicts from the engine's own clearance entries (f32 clearance < f32 threshold, each applicable rule)."""
    rej = np.zeros(cand.shape[0], bool)
    if c.world is not None:
        rej |= eng.world_clearance(cand)[0].cpu().numpy() < np.float32(thr["world"])
    if c.cloud:
        rej |= eng.cloud_clearance(cand)[0].cpu().numpy() < np.float32(thr["cloud"])
    if c.reject_self:
        rej |= eng.self_collision(cand)[0].cpu().numpy() < np.float32(thr["self"])
    return rej


def _setup_case(eng, c, thr, on):
    _scene(eng, c.which, EW.capsules_of(c), EW.world_of(c), thr.get("world", 0.0), EW.cloud_of(c), thr.get("cloud", 0.0),
           (on, c.reject_self, thr.get("self", 0.0)) if on else (False, False, 0.0), c.lm)


def _run_case(name, eng=None):
    """-> everything tests 2 and 3 look at, for one case."""
    c = EW.CASE_BY_NAME[name]
    eng = _eng(c.which) if eng is None else eng
    poses_cpu, seeds_cpu = EW.inputs(name)
    _, _, _, thr = EW.oracle_rows(name)
    poses, seeds = poses_cpu.to(DEV).contiguous(), seeds_cpu.to(DEV).contiguous()
    _setup_case(eng, c, thr, on=False)
    first, cand = _reconstruct(eng, poses.repeat(c.R, 1).contiguous(), seeds, c.steps)
    rej = _engine_rejected(eng, c, thr, cand) & (first > 0)
    _setup_case(eng, c, thr, on=True)
    assert eng.exact_collision() == (True, c.reject_self, pytest.approx(thr.get("self", 0.0), rel=1e-6))
    sol, valid = _refine_raw(eng, poses, seeds, c.R, c.steps)
    rejected_rows = eng.exact_collision_rejected()
    return dict(c=c, eng=eng, thr=thr, first=first, cand=cand, rej=rej, sol=sol, valid=valid, rejected_rows=rejected_rows, poses=poses, seeds=seeds)


@pytest.mark.parametrize("name", [c.name for c in EW.CASES])
def test_a_round_under_the_rule_equals_its_parts(name):
    r = _run_case(name)
    c, first, rej, cand = r["c"], r["first"], r["rej"], r["cand"]
    n, R = c.n, c.R
    winner = EW.select(first, rej, n, R)
    cl = EW.reference_clearances(c, cand.cpu())
    near = EW.band_poses(first, EW.in_band(cl, r["thr"]), n, R)
    share = float(near.mean())
    cand_rows = int((first > 0).sum())
    print(f"{name}: rows {n * R}, candidates {cand_rows}, rejected by the engine's clearances {int(rej.sum())}, reported {r['rejected_rows'][0]}, poses "
          f"solved {int((winner >= 0).sum())} of {n}, poses in the band {int(near.sum())} ({share:.4f})")
    assert share <= EW.BAND_SHARE_CAP, (name, share)
    assert 0.2 * cand_rows <= rej.sum() <= 0.8 * cand_rows, (name, int(rej.sum()), cand_rows)
    valid = r["valid"].cpu().numpy()
    sol = r["sol"]
    strict = ~near
    assert np.array_equal(valid[strict], (winner >= 0).astype(np.uint8)[strict]), name
    j = np.arange(n)
    want = torch.where(torch.from_numpy(winner >= 0).to(DEV)[:, None], cand[torch.from_numpy(np.maximum(winner, 0) * n + j).to(DEV)], torch.zeros_like(sol))
    diff = (_bits(sol) != _bits(want)).any(1).cpu().numpy()
    assert not diff[strict].any(), (name, np.flatnonzero(diff & strict)[:8].tolist())
    for p in np.flatnonzero(near):                       # the weaker check: one of its candidate rows, bit for bit, or zeros with valid 0
        if valid[p]:
            rows = [rr * n + p for rr in range(R) if first[rr * n + p] > 0]
            assert any(_same(sol[p], cand[row]) for row in rows), (name, int(p))
        else:
            assert not bool(_bits(sol[p]).any()), (name, int(p))
    if not near.any():
        assert r["rejected_rows"] == [int(rej.sum())] + [0] * 7, (name, r["rejected_rows"], int(rej.sum()))
    else:   # a row in the band may be counted either way
        band_rows = int(((first > 0) & EW.in_band(cl, r["thr"])).sum())
        assert abs(r["rejected_rows"][0] - int(rej.sum())) <= band_rows and r["rejected_rows"][1:] == [0] * 7, (name, r["rejected_rows"])
    # the call on a stream of its own gives the same bits
    if name == "syn4r-world":
        side = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            sol2, valid2 = _refine_raw(r["eng"], r["poses"], r["seeds"], c.R, c.steps)
            assert r["eng"].exact_collision_rejected() == r["rejected_rows"]
        assert _same(sol2, sol) and _same(valid2, r["valid"])


def test_a_model_without_capsules_or_without_pairs_rejects_nothing():
    """caps0 (no capsule: world and cloud clearance 3.0e38) under the world rule and caps1 (one capsule: no pair, self clearance 3.0e38) under the
    self rule: the fused launch runs, rejects nothing and returns the plain call's bits."""
    which, n, R = "panda", 65, 3
    eng = _eng(which)
    q_true = X.truth(which, n, 7)
    poses = ko.forward_kinematics(X.orob_of(which), q_true).to(DEV).contiguous()
    seeds = X.seed_tables(which, q_true, (R,), 8, sigmas=EW.CALM)[0].reshape(R * n, -1).to(DEV).contiguous()
    world = WH.scene(which, "mixed7")
    for caps, kw in (("caps0", dict(world=world, world_thr=10.0)), ("caps1", dict()), ("caps1", dict(world=world, world_thr=-10.0))):
        _scene(eng, which, RH.capsules(which, caps), **kw)
        plain = _refine_raw(eng, poses, seeds, R, 3)
        _scene(eng, which, RH.capsules(which, caps), rule=(True, True, 10.0), **kw)
        got = _refine_raw(eng, poses, seeds, R, 3)
        assert _same(got[0], plain[0]) and _same(got[1], plain[1]) and bool(plain[1].any()), caps
        assert eng.exact_collision_rejected() == [0] * 8


# ---- 3. by fp64, independent of the engine's clearances -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in EW.CASES])
def test_what_is_returned_is_valid_and_clear_by_fp64_and_the_flags_are_the_oracles(name):
    r = _run_case(name)
    c, thr = r["c"], r["thr"]
    n, R = c.n, c.R
    orob = X.orob_of(c.which)
    valid = r["valid"].cpu().numpy().astype(bool)
    sol = r["sol"].cpu()
    poses = EW.inputs(name)[0]
    assert valid.any()
    pe, re = ko.calculate_pose_error(orob, sol[valid].double(), poses[valid].double())
    assert bool((pe < POS + 1e-4 * POS + 5e-7).all()) and bool((re < ROT + 1e-4 * ROT + 6e-7 / ROT).all()), (name, float(pe.max()), float(re.max()))
    cl = EW.reference_clearances(c, sol[valid])
    for k, v in cl.items():
        assert (v >= thr[k] - EW.BAND).all(), (name, k, float(v.min()), thr[k])
    assert not bool(_bits(sol[~valid]).any())
    # the oracle schedule with the same mask applied from the fp64 references
    _, first, ocl, _ = EW.oracle_rows(name)
    rej = EW.rejected_of(ocl, thr)
    want = EW.select(first, rej, n, R) >= 0
    unsure = EW.band_poses(first, EW.in_band(ocl, thr), n, R) | EW.oracle_lm_band(name).reshape(R, n).any(0)
    unsure |= EW.band_poses(r["first"], EW.in_band(EW.reference_clearances(c, r["cand"].cpu()), thr), n, R)
    print(f"{name}: valid {int(valid.sum())} of {n}, the oracle's {int(want.sum())}, poses in a band {int(unsure.sum())}")
    assert unsure.mean() <= 0.10, (name, float(unsure.mean()))      # (two bands: the clearances' 5 % and the pose thresholds' 3 %)
    assert np.array_equal(valid[~unsure], want[~unsure]), (name, np.flatnonzero((valid != want) & ~unsure)[:8].tolist())
    assert int(valid[~unsure].sum()) == int(want[~unsure].sum())


# ---- 4. a colliding sibling stops nobody ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_cloud", (False, True))
@pytest.mark.parametrize("name", sorted(EW.SIBLING_CASES))
def test_a_colliding_sibling_stops_nobody(name, with_cloud):
    """Poses with a repeat that is a candidate at iteration 1 and rejected, and another repeat - lower or higher - that is a candidate at iteration
    >= 2, admissible and the definition's choice: the later row must be returned.  Counted again here, from the reconstruction on the GPU."""
    s = EW.sibling_case(name, with_cloud)
    c, n, R, thr = s["case"], s["n"], s["R"], s["thr"]
    eng = _eng(c.which)
    poses, seeds = s["poses"].to(DEV).contiguous(), s["seeds"].to(DEV).contiguous()
    caps = RH.capsules(c.which, None)
    cloud = EW.cloud_of(c)
    _scene(eng, c.which, caps, s["world"], thr["world"], cloud, thr.get("cloud", 0.0))
    first, cand = _reconstruct(eng, poses.repeat(R, 1).contiguous(), seeds, c.steps)
    rej = (eng.world_clearance(cand)[0].cpu().numpy() < np.float32(thr["world"]))
    if with_cloud:
        rej |= eng.cloud_clearance(cand)[0].cpu().numpy() < np.float32(thr["cloud"])
    rej &= first > 0
    winner = EW.select(first, rej, n, R)
    cl = {"world": WH.reference(X.orob_of(c.which), caps, s["world"], cand.cpu())["clearance"]}
    if with_cloud:
        cl["cloud"] = CH.reference(X.orob_of(c.which), caps, cloud, CH.POINT_RADIUS, cand.cpu())
    near = EW.band_poses(first, EW.in_band(cl, thr), n, R)
    sib = EW.sibling_poses(first, rej, winner, n, R) & ~near
    lower = int((sib & (winner < np.where(((first == 1) & rej).reshape(R, n), np.arange(R)[:, None], -1).max(0))).sum())
    print(f"sibling {name} cloud {with_cloud}: {int(sib.sum())} poses on the GPU ({int(s['siblings'].sum())} by the oracle), the later row is the lower repeat in {lower}")
    assert sib.sum() >= EW.SIBLING_MIN, (name, with_cloud, int(sib.sum()))
    _scene(eng, c.which, caps, s["world"], thr["world"], cloud, thr.get("cloud", 0.0), rule=(True, False, 0.0))
    sol, valid = _refine_raw(eng, poses, seeds, R, c.steps)
    idx = np.flatnonzero(sib)
    assert bool(valid[torch.from_numpy(idx).to(DEV)].all()), (name, with_cloud)
    want = cand[torch.from_numpy(winner[idx] * n + idx).to(DEV)]
    assert _same(sol[torch.from_numpy(idx).to(DEV)], want), (name, with_cloud)
    strict = ~near
    assert np.array_equal(valid.cpu().numpy()[strict], (winner >= 0).astype(np.uint8)[strict])


@pytest.mark.parametrize("name", sorted(EW.SIBLING_CASES))
def test_a_sibling_rejected_by_the_cloud_alone_stops_nobody(name):
    """The same poses with the sphere as a cloud of one point and no primitive: the plain loop runs in front of the cloud's mask, and it must run
    without the early-exit hint - a row inside the thresholds at iteration 1 is not yet known to be admissible."""
    s = EW.sibling_cloud_case(name)
    which, n, R = s["which"], s["n"], s["R"]
    eng = _eng(which)
    caps = RH.capsules(which, None)
    poses, seeds = s["poses"].to(DEV).contiguous(), s["seeds"].to(DEV).contiguous()
    _scene(eng, which, caps, None, 0.0, s["points"], 0.0)
    first, cand = _reconstruct(eng, poses.repeat(R, 1).contiguous(), seeds, EW.SIBLING_STEPS)
    rej = (eng.cloud_clearance(cand)[0].cpu().numpy() < np.float32(0.0)) & (first > 0)
    winner = EW.select(first, rej, n, R)
    near = EW.band_poses(first, EW.in_band({"cloud": CH.reference(X.orob_of(which), caps, s["points"], CH.POINT_RADIUS, cand.cpu())}, s["thr"]), n, R)
    sib = EW.sibling_poses(first, rej, winner, n, R) & ~near
    print(f"sibling {name}, cloud alone: {int(sib.sum())} poses on the GPU ({int(s['siblings'].sum())} by the oracle)")
    assert sib.sum() >= EW.SIBLING_MIN, (name, int(sib.sum()))
    _scene(eng, which, caps, None, 0.0, s["points"], 0.0, rule=(True, False, 0.0))
    sol, valid = _refine_raw(eng, poses, seeds, R, EW.SIBLING_STEPS)
    idx = torch.from_numpy(np.flatnonzero(sib)).to(DEV)
    assert bool(valid[idx].all()), name
    assert _same(sol[idx], cand[torch.from_numpy(winner[np.flatnonzero(sib)] * n + np.flatnonzero(sib)).to(DEV)]), name
    assert np.array_equal(valid.cpu().numpy()[~near], (winner >= 0).astype(np.uint8)[~near])
    assert eng.exact_collision_rejected()[0] == int(rej.sum()) or near.any()


@pytest.mark.parametrize("rule", ("world", "cloud", "self"))
def test_a_threshold_above_every_clearance_rejects_every_candidate_down_to_the_last_row(rule):
    """65 x 3 rows, each rule alone with a threshold of 10 m: every candidate row is rejected - the last row of the round included -, no pose is
    solved, every output row is zero and the count is the number of candidates."""
    which, n, R = "panda", 65, 3
    eng = _eng(which)
    caps = RH.capsules(which, None)
    q_true = X.truth(which, n, 7)
    poses = ko.forward_kinematics(X.orob_of(which), q_true).to(DEV).contiguous()
    seeds = X.seed_tables(which, q_true, (R,), 8, sigmas=(0.01,))[0].reshape(R * n, -1).to(DEV).contiguous()
    _scene(eng, which, caps)
    first, _ = _reconstruct(eng, poses.repeat(R, 1).contiguous(), seeds, 3)
    assert first[-1] > 0 and first[0] > 0 and (first > 0).sum() >= 0.9 * n * R          # the first and the last row of the round are candidates
    kw = {"world": dict(world=WH.scene(which, "mixed7"), world_thr=10.0), "cloud": dict(cloud=CH.cloud(which, 513), cloud_thr=10.0), "self": dict()}[rule]
    _scene(eng, which, caps, rule=(True, rule == "self", 10.0), **kw)
    sol, valid = _refine_raw(eng, poses, seeds, R, 3)
    assert not bool(valid.any()) and not bool(_bits(sol).any()), rule
    assert eng.exact_collision_rejected() == [int((first > 0).sum())] + [0] * 7, rule


# ---- 5. retry rounds ------------------------------------------------------------------------------------------------------------------------------
def _blocked_call(eng, c, cloud=None):
    n = len(c["blocked"])
    R0, R1 = EW.ROUNDS_RC
    _scene(eng, EW.ROUNDS_CHAIN, RH.capsules(EW.ROUNDS_CHAIN, None), c["world"], 0.0, cloud, 0.0, rule=(True, False, 0.0))
    dev = {k: c[k].to(DEV).contiguous() for k in ("poses", "seeds0", "seeds1")}
    rows = _gather(n)

    def seed_fn(rnd, idx, repeat):
        return dev["seeds0" if rnd == 0 else "seeds1"][rows(idx)].repeat(repeat, 1).contiguous()

    sol, valid, stats, lists = _seeded(eng, dev["poses"], EW.ROUNDS_RC, 1, seed_fn)
    return sol, valid, stats, lists, eng.exact_collision_rejected()


@pytest.mark.parametrize("n,kind", [(64, "all"), (1, "all"), (255, "half"), (257, "runs16"), (4099, "half")])
def test_poses_blocked_in_round_0_fall_through_to_round_1(n, kind):
    """Round 0's seeds of the blocked poses sit in the sphere (every repeat is a candidate and is rejected), round 1's are clear: blocked poses are
    unsolved after round 0 and solved in round 1; the engine's lists are arange(n) and flatnonzero(blocked), element for element; the stats
    and the rejected rows are the constructed counts."""
    c = EW.blocked_case(n, kind)
    b = c["blocked"]
    nb = int(b.sum())
    R0, R1 = EW.ROUNDS_RC
    sol, valid, stats, lists, rejected = _blocked_call(_eng(EW.ROUNDS_CHAIN), c)
    assert len(lists) == 2 and np.array_equal(lists[0], np.arange(n, dtype=np.int32)) and np.array_equal(lists[1], np.flatnonzero(b).astype(np.int32))
    assert stats.tolist() == [[n, n * R0, n * R0, n - nb], [nb, nb * R1, nb * R1, nb]], stats.tolist()
    assert rejected == [nb * R0, 0] + [0] * 6, rejected
    assert bool(valid.all())
    one = _seeded(_eng(EW.ROUNDS_CHAIN), c["poses"].to(DEV).contiguous(), (R0,), 1,
                  lambda rnd, idx, repeat: c["seeds0"].to(DEV)[torch.from_numpy(idx.astype(np.int64)).to(DEV)].repeat(repeat, 1).contiguous())
    assert np.array_equal(one[1].cpu().numpy(), (~b).astype(np.uint8)) and not bool(_bits(one[0][torch.from_numpy(b).to(DEV)]).any())   # after round 0 alone
    assert one[2].tolist() == [[n, n * R0, n * R0, n - nb]]


def test_a_growing_handle_with_a_cloud_gives_the_bits_of_the_reserved_one():
    """ikf_set_exact_upfront_rows(0) on a fresh handle and a cloud set: the rows' cloud clearances are sized with the row state, which grows
    between round 0 (2 n rows) and round 1 (3 n rows)."""
    c = EW.blocked_case(257, "all")
    far = np.array([[50.0, 0.0, 0.0], [0.0, 50.0, 0.0]], np.float32)
    reserved = _eng(EW.ROUNDS_CHAIN)
    reserved.reserve_exact(257, 3)
    want = _blocked_call(reserved, c, cloud=far)
    grow = _eng(EW.ROUNDS_CHAIN, "growing")
    grow.set_exact_upfront_rows(0)
    got = _blocked_call(grow, c, cloud=far)
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[4] == want[4] == [257 * 2] + [0] * 7
    assert all(np.array_equal(a, b) for a, b in zip(got[3], want[3]))
    again = _blocked_call(grow, c, cloud=far)        # the counter is zeroed at the start of every call
    assert again[4] == want[4] and _same(again[0], want[0])


# ---- 6. the flow in -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["R-200", "T-17"])
def test_the_flow_call_under_the_rule_has_the_bits_of_its_parts(case):
    """ikf_generate_exact with fixed latents equals the seeded rule-on call on the seeds of ikf_generate_approx_tiled (exact_helpers.parts), with
    mixed7 and the self rule at the medians of 257 random configurations."""
    from test_exact_flow import _assert_same, _case
    from test_flow_sample import _eng as flow_eng
    from test_flow_sample import _no_cluster_repair

    name, P, lats, rc, pos_thr, rot_thr = _case(case)
    eng = flow_eng(name)
    robot, orob = H.kin_robots("panda")
    q, ref, world_thr = WH.rows_and_reference("panda", "mixed7")
    self_thr = float(np.quantile(RH.clearance(orob, RH.capsules("panda", None), q), 0.25))
    robot.set_collision_capsules(RH.collision_capsules(robot))
    try:
        eng.set_collision_model(*robot._collision_model)
        eng._collision_source = None
        eng.set_world(WH.scene("panda", "mixed7"), float(np.quantile(ref["clearance"], 0.25)))
        plain = X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, X.FLOW_STEPS, lats)
        eng.set_exact_collision(True, True, self_thr)
        with _no_cluster_repair(eng):
            one = X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, X.FLOW_STEPS, lats)
            rejected = eng.exact_collision_rejected()
            two = X.parts(eng, P, rc, pos_thr, rot_thr, X.FLOW_STEPS, lats)
        _assert_same(one, two, case)
        print(f"[exact+flow under the rule] {case}: active {one[2][:, 0].tolist()}, solved {one[2][:, 3].tolist()} (plain {plain[2][:, 3].tolist()}), rejected rows {rejected}")
        assert sum(rejected) > 0 and not _same(one[0], plain[0])          # the rule did something
        assert int(one[1].sum()) == int(one[2][:, 3].sum())
    finally:
        eng.set_exact_collision(False)
        eng.clear_world()


# ---- 7. statuses and wrappers ---------------------------------------------------------------------------------------------------------------------
def test_statuses_getters_and_two_handles():
    which = "panda"
    a, b = _eng(which), _eng(which, "b")
    lib = a.lib
    _scene(a, which, RH.capsules(which, None), rule=(True, True, 0.02))
    assert a.exact_collision() == (True, True, pytest.approx(0.02))
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert lib.ikf_set_exact_collision(a._h, 1, 0, bad) == _lib.IKF_ERR_BAD_ARGUMENT
        assert "self_min_clearance must be finite" in _lib.last_error(lib)
        assert a.exact_collision() == (True, True, pytest.approx(0.02))          # a refused call leaves the state alone
    on = C.c_int(7)
    assert lib.ikf_get_exact_collision(a._h, C.byref(on), None, None) == _lib.IKF_OK and on.value == 1
    assert lib.ikf_exact_collision_rejected(a._h, None) == _lib.IKF_ERR_NULL_POINTER
    a.set_exact_collision(False, True, 0.3)
    assert a.exact_collision() == (False, False, 0.0)                            # off: the rest is dropped
    # two handles, two rules: one rejects by the self rule, the other runs plain - on the same inputs, one after the other and back
    name = "syn6r-self-20steps"
    c = EW.CASE_BY_NAME[name]
    ea, eb = _eng(c.which), _eng(c.which, "b")
    r = _run_case(name, ea)
    _scene(eb, c.which, EW.capsules_of(c))
    plain = _refine_raw(eb, r["poses"], r["seeds"], c.R, c.steps)
    again = _refine_raw(ea, r["poses"], r["seeds"], c.R, c.steps)
    assert _same(again[0], r["sol"]) and _same(again[1], r["valid"]) and not _same(plain[1], r["valid"])
    assert ea.exact_collision_rejected()[0] == r["rejected_rows"][0] > 0 and eb.exact_collision_rejected() == [0] * 8
    assert eb.exact_collision() == (False, False, 0.0)


def test_the_rule_without_a_collision_model_is_refused_before_any_work():
    which = "syn5p"
    eng = _eng(which, "no model")       # never given a capsule model
    n, R = 17, 2
    q_true = X.truth(which, n, 3)
    poses = ko.forward_kinematics(X.orob_of(which), q_true).to(DEV).contiguous()
    seeds = q_true.repeat(R, 1).to(DEV).contiguous()
    eng.set_exact_collision(True, True, 0.0)
    _refine_raw(eng, poses, seeds, R, 3, expect=_lib.IKF_ERR_BAD_ARGUMENT)
    assert "without a collision model" in _lib.last_error(eng.lib)
    assert eng.exact_collision_rejected() == [0] * 8
    eng.set_exact_collision(True, False, 0.0)      # nothing to test against: the plain call, no model needed
    sol, valid = _refine_raw(eng, poses, seeds, R, 3)
    assert bool(valid.all())


def test_a_solver_whose_rule_was_set_before_its_engine_existed_and_the_wrapper():
    """IKFlowSolver.set_exact_collision before the first engine: the engine is created with the collision model, the world and then the rule;
    generate_exact_ik_solutions with fixed latents equals the raw call on that engine."""
    from ikflow_amd.ikflow_solver import IKFlowSolver

    robot, hp, lay, sd = H.tiny_model()
    robot.set_collision_capsules(RH.collision_capsules(robot))
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    q, ref, _ = WH.rows_and_reference("panda", "mixed7")
    world_thr = float(np.quantile(ref["clearance"], 0.25))
    s.set_exact_collision(reject_self_collisions=True, min_clearance=0.01)
    assert s._engine is None
    s.set_world(WH.scene("panda", "mixed7"), world_thr)
    eng = s.engine(DEV)
    assert eng.exact_collision() == (True, True, pytest.approx(0.01)) and eng.world_size == 7
    from test_exact_flow import _case

    name, P, lats, rc, pos_thr, rot_thr = _case("T-200")
    raw = X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, 3, lats)
    rejected = eng.exact_collision_rejected()
    sol, valid = s.generate_exact_ik_solutions(P, repeat_counts=tuple(rc), pos_error_threshold=pos_thr, rot_error_threshold=rot_thr, latents=lats)
    assert _same(sol, raw[0]) and np.array_equal(valid.cpu().numpy(), raw[1].cpu().numpy().astype(bool))
    assert eng.exact_collision_rejected() == rejected and sum(rejected) > 0
    s.set_exact_collision(enabled=False)
    assert eng.exact_collision() == (False, False, 0.0)
    plain = s.generate_exact_ik_solutions(P, repeat_counts=tuple(rc), pos_error_threshold=pos_thr, rot_error_threshold=rot_thr, latents=lats)
    assert not _same(plain[0], sol) and eng.exact_collision_rejected() == [0] * 8
