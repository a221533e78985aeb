"""World collision on the GPU (include/ikflow_amd_world.h; ikflow_amd/csrc/world_kernels.hip, world_math.h, api_world.hip, and the WORLD form of
k_rank_candidates): ikf_world_clearance against the fp64 reference of tests/world_helpers.py, guarded buffers, the ranking / path IK / diverse-of-K
with a world set on the handle, switching the world on and off, two handles, status codes.

Tolerances are the project's (world_helpers.py): 2e-5 on a clearance, a band of 1e-4 around min_clearance in which admissibility is not compared,
row scores by rank_helpers.check_row_scores.  The threshold of a case is the median of the reference clearances of its rows;
tests/test_world_math_host.py checks on the CPU that this leaves at most 5 % of the rows in the band and at least 20 % on either side."""
import ctypes as C

import numpy as np
import pytest
import torch

import diverse_helpers as DH
import helpers as H
import path_helpers as PH
import rank_helpers as RH
import world_helpers as WH
from ikflow_amd import _lib
from ikflow_amd.world import World
from test_ranked import _check_selection, _check_the_straddle, _eng_with, _opt, _rank, _small_model_back  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
NAN_BITS = 0x7FC00000
INT_SENTINEL = -1414812757   # 0xABABABAB
BYTE_SENTINEL = 0xAB
_USED = []


def _eng(which):
    """The shared kinematics engine of the chain with the test capsule model (as tests/test_ranked.py's); its world is cleared after every test."""
    from ikflow_amd.engine import kinematics_engine_for

    robot = H.kin_robots(which)[0]
    eng = kinematics_engine_for(robot, DEV)
    robot.set_collision_capsules(RH.collision_capsules(robot))
    eng.set_collision_model(*robot._collision_model)
    eng._collision_source = robot._collision_model
    if eng not in _USED:
        _USED.append(eng)
    return eng


@pytest.fixture(autouse=True)
def _no_world_left_behind():
    yield
    for eng in _USED:
        eng.clear_world()   # (the engines are shared with the other test modules)


OUTPUTS = ("clearance", "obstacle", "capsule", "colliding")
_DTYPES = {"clearance": torch.float32, "obstacle": torch.int32, "capsule": torch.int32, "colliding": torch.uint8}
_FILL = {"clearance": float("nan"), "obstacle": INT_SENTINEL, "capsule": INT_SENTINEL, "colliding": BYTE_SENTINEL}


def _untouched(part, name):
    if name == "clearance":
        return bool((part.view(torch.int32) == NAN_BITS).all())
    return bool((part == _FILL[name]).all())


def _clearance(eng, q, null=(), n=None, stream=None, expect=_lib.IKF_OK):
    """ikf_world_clearance through eng.lib on guarded buffers -> {name: cpu numpy window}; `null`: the outputs passed as null; n: the row count
    passed (default: all rows of q)."""
    rows = q.shape[0]
    n = rows if n is None else n
    bufs = {o: torch.full((rows + 2 * GUARD,), _FILL[o], dtype=_DTYPES[o], device=DEV) for o in OUTPUTS if o not in null}
    ptr = [bufs[o][GUARD:].data_ptr() if o in bufs else None for o in OUTPUTS]
    qd = q.to(DEV).contiguous()
    torch.cuda.synchronize()
    s = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(0)
    code = eng.lib.ikf_world_clearance(eng._h, qd.data_ptr() if rows else None, n, *ptr, s)
    assert code == expect, (code, _lib.last_error(eng.lib))
    torch.cuda.synchronize()
    out = {}
    for o, b in bufs.items():
        assert _untouched(b[:GUARD], o) and _untouched(b[GUARD + n:], o), f"{o}: an element outside the window was written"
        win = b[GUARD:GUARD + n]
        if n:
            written = ~torch.isnan(win) if o == "clearance" else win != _FILL[o]
            assert bool(written.all()), f"{o}: an element inside the window was not written"
        out[o] = win.cpu().numpy().copy()
    return out


def _check_against_reference(out, ref, thr, n, what):
    cl = ref["clearance"][:n]
    err = float(np.abs(out["clearance"].astype(np.float64) - cl).max())
    print(f"{what} n {n}: worst |engine - fp64 reference| {err:.2e}")
    assert err <= WH.CLEARANCE_TOL, (what, n, err)
    sure = ~ref["ambiguous"][:n]
    assert np.array_equal(out["obstacle"][sure], ref["obstacle"][:n][sure]) and np.array_equal(out["capsule"][sure], ref["capsule"][:n][sure]), what
    decided = np.abs(cl - thr) > WH.BAND
    assert np.array_equal(out["colliding"][decided], (cl < thr)[decided].astype(np.uint8)), what
    assert set(np.unique(out["colliding"])) <= {0, 1}


# ---- 1. ikf_world_clearance against the fp64 reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WH.SCENES)
@pytest.mark.parametrize("which", H.KIN_ALL)
def test_world_clearance_against_the_fp64_reference(which, name):
    """1, 63, 64, 65 and 130 rows (one thread short of a workgroup, one workgroup, one thread more, three workgroups) of every chain in every scene:
    clearance within 2e-5, the closest pair the reference's unless its two best pairs are within 4e-5, flags exact outside the band."""
    eng = _eng(which)
    world = WH.scene(which, name)
    q, ref, thr = WH.rows_and_reference(which, name)
    eng.set_world(world, thr)
    assert eng.world_size == len(world)
    for n in (1, 63, 64, 65, 130):
        _check_against_reference(_clearance(eng, q[:n]), ref, thr, n, f"{which} {name}")


# ---- 2. buffers ----------------------------------------------------------------------------------------------------------------------------------
def test_outputs_are_nullable_n_zero_is_a_no_op_and_an_empty_world_is_far_away():
    which, name = "panda", "mixed7"
    eng = _eng(which)
    q, ref, thr = WH.rows_and_reference(which, name)
    eng.set_world(WH.scene(which, name), thr)
    full = _clearance(eng, q[:130])
    for null in [("clearance",), ("obstacle",), ("capsule",), ("colliding",), ("obstacle", "capsule", "colliding"), ("clearance", "obstacle", "capsule"), OUTPUTS]:
        got = _clearance(eng, q[:130], null=null)
        assert set(got) == set(OUTPUTS) - set(null) and all(np.array_equal(got[o].view(np.uint8), full[o].view(np.uint8)) for o in got)
    side = torch.cuda.Stream(device=DEV)
    got = _clearance(eng, q[:130], stream=side)
    assert all(np.array_equal(got[o].view(np.uint8), full[o].view(np.uint8)) for o in OUTPUTS)
    _clearance(eng, q[:130], n=0)                                  # n = 0: nothing is written (every element still carries its sentinel)
    _clearance(eng, q[:0])                                         # ... and null pointers are fine
    _clearance(eng, q[:4], n=-1, expect=_lib.IKF_ERR_BAD_ARGUMENT)
    eng.clear_world()
    assert eng.world_size == 0
    empty = _clearance(eng, q[:130])
    assert (empty["clearance"] == np.float32(3.0e38)).all() and (empty["obstacle"] == -1).all() and (empty["capsule"] == -1).all() and (empty["colliding"] == 0).all()
    eng.set_world(World(), 5.0)                                    # an empty World clears too, whatever its threshold
    assert eng.world_size == 0 and (_clearance(eng, q[:65])["colliding"] == 0).all()


def test_robot_environment_queries_and_the_engine_wrapper():
    which, name = "fetch", "mixed7"
    robot = H.kin_robots(which)[0]
    eng = _eng(which)
    world = WH.scene(which, name)
    q, ref, thr = WH.rows_and_reference(which, name)
    qd = q.to(DEV)
    dist = robot.env_collision_distances(qd, world).cpu().numpy()
    assert np.abs(dist - ref["clearance"]).max() <= WH.CLEARANCE_TOL
    assert eng.world_size == 0   # (the shared engine is left without a world)
    col = robot.config_collides_with_env(qd, world, thr).cpu().numpy()
    decided = np.abs(ref["clearance"] - thr) > WH.BAND
    assert col.dtype == np.bool_ and np.array_equal(col[decided], (ref["clearance"] < thr)[decided])
    one = int(np.flatnonzero(decided)[0])
    assert robot.config_collides_with_env(qd[one], world, thr) is bool(ref["clearance"][one] < thr)
    eng.set_world(world, thr)
    cl, ob, cp, flag = eng.world_clearance(qd)
    assert cl.dtype == torch.float32 and ob.dtype == torch.int32 and cp.dtype == torch.int32 and flag.dtype == torch.bool
    assert np.array_equal(cl.cpu().numpy(), dist) and np.array_equal(flag.cpu().numpy(), col)


# ---- 3. the ranking with a world ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k", WH.RANK_SHAPES)
@pytest.mark.parametrize("which", H.KIN_ALL)
def test_ranking_with_a_world(which, m, k):
    """ikf_rank_candidates while a world is set, with and without reject_collisions, n_keep 1, 4 and 16 where k allows: row scores by
    rank_helpers.check_row_scores against the reference whose admissibility carries the world term and its band; the selection against
    rank_helpers.select on the engine's own row scores, bit for bit.  (64, 16) and (1, 1024) run in two chunks."""
    robot, orob = H.kin_robots(which)
    eng = _eng(which)
    caps = RH.collision_capsules(robot)
    poses, q, _, cl, thr = WH.rank_case(which, m, k)
    eng.set_world(WH.scene(which, WH.RANK_SCENE), thr)
    if (m, k) in ((64, 16), (1, 1024)):
        assert eng.rank_chunks(m, k) == 2
    for collisions in (False, True):
        self_thr = RH.clearance_threshold(orob, caps, q) if collisions else 0.0
        ref = WH.rank_reference(orob, caps, cl, thr, poses, q, k, 0.01, self_collisions=collisions, min_clearance=self_thr)
        for n_keep in [n for n in (1, 4, 16) if n <= k]:
            out = _rank(eng, poses, q, k, _opt(n_keep=n_keep, collisions=collisions, min_clearance=self_thr))
            if np.isfinite(out["row_score"]).any() or ref["admissible"][~ref["near"]].any():
                worst = RH.check_row_scores(out["row_score"], ref, f"{which} m {m} k {k} collisions {collisions}")
            else:
                worst = 0.0   # (a shape of one or a few rows, all of them rejected)
            _check_selection(out, q, m, k, n_keep, f"{which} m {m} k {k} n_keep {n_keep}")
        print(f"ranking with a world {which} m {m} k {k} collisions {collisions}: worst {worst:.3f} of eps, {int((~ref['admissible']).sum())} of {k * m} rows inadmissible")
        if m * k >= 130:
            world_only = (cl < thr - WH.BAND) & np.isfinite(ref["score"])
            assert world_only.sum() >= 0.2 * k * m and np.isposinf(out["row_score"][world_only]).all()


# ---- 4. switching --------------------------------------------------------------------------------------------------------------------------------
def test_clearing_the_world_and_a_far_world_give_the_call_without_a_world_bit_for_bit():
    which, m, k = "panda", 64, 16
    robot, orob = H.kin_robots(which)
    eng = _eng(which)
    poses, q, q_ref, cl, thr = WH.rank_case(which, m, k)
    self_thr = RH.clearance_threshold(orob, RH.collision_capsules(robot), q)
    for collisions in (False, True):
        opt = _opt(n_keep=4, ref_weight=0.05, limits=True, collisions=collisions, min_clearance=self_thr)
        eng.clear_world()
        before = _rank(eng, poses, q, k, opt, q_ref)
        eng.set_world(WH.scene(which, WH.RANK_SCENE), thr)
        during = _rank(eng, poses, q, k, opt, q_ref)
        assert np.isposinf(during["row_score"]).sum() > np.isposinf(before["row_score"]).sum()
        both = np.isfinite(during["row_score"])
        assert H.same_bits(during["row_score"][both], before["row_score"][both])   # (an admitted row keeps its score)
        eng.clear_world()
        after = _rank(eng, poses, q, k, opt, q_ref)
        assert all(H.same_bits(after[n], before[n]) for n in before)
        far = WH.far_world()
        eng.set_world(far, 1.0)
        assert eng.world_size == len(far) and float(eng.world_clearance(q.to(DEV))[0].min()) > 1.0
        distant = _rank(eng, poses, q, k, opt, q_ref)
        assert all(H.same_bits(distant[n], before[n]) for n in before)


# ---- 5. path IK and diverse-of-K -----------------------------------------------------------------------------------------------------------------
def _small_case(which, m, k, seed):
    """m poses x k candidates of the ranking's family whose every pose keeps a candidate that the world surely admits."""
    robot, orob = H.kin_robots(which)
    poses, q, _ = RH.candidates(orob, m, k, seed=seed, lo_exp=-1.5)
    cl = WH.reference(orob, RH.collision_capsules(robot), WH.scene(which, WH.RANK_SCENE), q)["clearance"]
    thr = WH.threshold(cl)
    rejected, admitted = cl < thr - WH.BAND, cl > thr + WH.BAND
    assert rejected.any() and admitted.reshape(k, m).any(0).all()   # (every pose keeps a candidate the world surely admits)
    return poses, q, thr, rejected


def _path_case(which, T, k, seed):
    """T neighbouring waypoints (0.04 rad apart in joint space) and k candidates each, 0.3 rad of noise around the truth: clearances differ more
    between the candidates of a waypoint than between waypoints, so the median of all rows rejects some and admits some at every waypoint."""
    from oracle import kinematics_oracle as ko

    robot, orob = H.kin_robots(which)
    g = torch.Generator().manual_seed(seed)
    q0, _ = H.reachable_poses(orob, 1, seed)
    step = torch.randn(1, orob.ndof, generator=g, dtype=torch.float64)
    q_true = ko.clamp_to_joint_limits(orob, q0 + torch.arange(T, dtype=torch.float64)[:, None] * (0.04 * step / step.norm()))
    poses = ko.forward_kinematics(orob, q_true).float().contiguous()
    noise = torch.randn(k, T, orob.ndof, generator=g, dtype=torch.float64) * 0.3
    q = ko.clamp_to_joint_limits(orob, (q_true[None] + noise).reshape(k * T, -1)).float().contiguous()
    cl = WH.reference(orob, RH.collision_capsules(robot), WH.scene(which, WH.RANK_SCENE), q)["clearance"]
    thr = WH.threshold(cl)
    rejected, admitted = cl < thr - WH.BAND, cl > thr + WH.BAND
    assert rejected.reshape(k, T).any(0).all() and admitted.reshape(k, T).any(0).all()
    return poses, q, thr, rejected


def test_path_search_never_walks_through_a_rejected_node():
    which, T, k = "panda", 5, 4
    eng = _eng(which)
    poses, q, thr, rejected = _path_case(which, T, k, 3)
    eng.set_world(WH.scene(which, WH.RANK_SCENE), thr)
    opt = eng.path_options(reject_limits=False, node_weight=20.0)
    path, index, cost, reach, node = [t.cpu().numpy() for t in eng.path_search(poses.to(DEV), k, q.to(DEV), opt, node_costs=True)]
    assert np.isposinf(node[rejected]).all() and np.isfinite(cost[0]) and (index >= 0).all()
    assert not rejected[index * T + np.arange(T)].any()
    want_path, want_index, want_cost, want_reach = PH.dp_f32(q.numpy(), node, T, k, None, opt.node_weight, opt.max_joint_step)
    assert np.array_equal(index, want_index) and PH.same_bits(cost, np.array([want_cost], np.float32)) and PH.same_bits(path, want_path)
    assert np.array_equal(reach, want_reach)
    ranked = _rank(eng, poses, q, k, _opt(n_keep=1))
    assert PH.same_bits(node, ranked["row_score"])   # (the node costs are the ranking's row scores under the same world)
    eng.clear_world()
    free = eng.path_search(poses.to(DEV), k, q.to(DEV), opt, node_costs=True)
    assert np.isfinite(free[4].cpu().numpy()).all()   # (without the world every node is open)


def test_diverse_select_never_keeps_a_rejected_row():
    which, m, k, n_keep = "panda", 3, 8, 4
    eng = _eng(which)
    poses, q, thr, rejected = _small_case(which, m, k, 12)
    eng.set_world(WH.scene(which, WH.RANK_SCENE), thr)
    opt = eng.diverse_options(n_keep=n_keep, reject_limits=False, min_separation=0.05)
    q_out, score, index, sep, kept, count, rows = [t.cpu().numpy() for t in eng.diverse_select(poses.to(DEV), k, q.to(DEV), opt, row_scores=True)]
    assert np.isposinf(rows[rejected]).all() and (kept >= 1).all()
    taken = index[index >= 0].astype(np.int64) * m + np.nonzero(index >= 0)[0]
    assert not rejected[taken].any()
    want = DH.select_poses(q.numpy(), rows, m, k, n_keep, 0.05)
    got = {"q_out": q_out, "score": score, "index": index, "sep": sep, "kept": kept, "count": count}
    assert all(DH.same_bits(got[n], want[n]) for n in DH.NAMES), [n for n in DH.NAMES if not DH.same_bits(got[n], want[n])]
    ranked = _rank(eng, poses, q, k, _opt(n_keep=1))
    assert DH.same_bits(rows, ranked["row_score"])


# ---- 6. the flow in front ------------------------------------------------------------------------------------------------------------------------
def test_generate_ranked_with_a_world_equals_the_flow_then_rank_candidates():
    """IKFlowSolver.set_world reaches the solver's own handle; ikf_generate_ranked under it equals generate_ik_solutions on the tiled poses followed
    by ikf_rank_candidates on the same handle, bit for bit; the solvers' path and diverse calls see the same world."""
    from ikflow_amd.ikflow_solver import IKFlowSolver, mm_to_m

    robot, hp, lay, sd = H.tiny_model()
    robot.set_collision_capsules(RH.collision_capsules(robot))
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    m, k, n_keep = 65, 16, 4
    _, poses = H.reachable_poses(robot, m, 6)
    y, L = poses.float().to(DEV), H.latents(k * m, lay.dim, 8).to(DEV)
    q = s.generate_ik_solutions(y.repeat((k, 1)), latent=L)
    world = WH.scene("panda", WH.RANK_SCENE)   # (the tiny model's robot is the Panda)
    without = s.generate_ranked_ik_solutions(y, k, n_keep, latent=L, reject_self_collisions=False, return_row_scores=True)
    s.set_world(world, 0.0)
    eng = s.engine(DEV)
    assert eng.world_size == len(world)
    # not an accuracy claim: only a threshold that rejects about half of these rows, and is no row's own clearance
    thr = float(eng.world_clearance(q)[0].median()) + 5e-5
    s.set_world(world, thr)
    got = s.generate_ranked_ik_solutions(y, k, n_keep, latent=L, reject_self_collisions=False, return_row_scores=True)
    opt = eng.rank_options(n_keep, mm_to_m(1) / 0.1, 0.0, None, None, True, False, 0.0)
    two_step = eng.rank_candidates(y, k, q, opt, row_scores=True)
    for a, b in zip(got, two_step):
        assert H.same_bits(a.cpu().numpy(), b.cpu().numpy())
    n_inf, n_inf_without = int(torch.isinf(got.row_scores).sum()), int(torch.isinf(without.row_scores).sum())
    assert n_inf_without < n_inf < k * m
    far_rows = torch.isinf(got.row_scores) & ~torch.isinf(without.row_scores)
    assert bool((eng.world_clearance(q)[0][far_rows] < thr + 1e-5).all())
    one = s.generate_ranked_ik_solutions(y, k, 1, latent=L, reject_self_collisions=False, return_row_scores=True)
    div = s.generate_diverse_ik_solutions(y, k, n_keep, latent=L, reject_self_collisions=False, return_row_scores=True)
    assert H.same_bits(div.row_scores.cpu().numpy(), one.row_scores.cpu().numpy())   # (the score stage of diverse-of-K is the ranking with n_keep = 1)
    assert np.array_equal(np.isinf(one.row_scores.cpu().numpy()), np.isinf(got.row_scores.cpu().numpy()))
    s.set_world(None)
    assert eng.world_size == 0
    again = s.generate_ranked_ik_solutions(y, k, n_keep, latent=L, reject_self_collisions=False, return_row_scores=True)
    for a, b in zip(again, without):
        assert H.same_bits(a.cpu().numpy(), b.cpu().numpy())


# ---- 7. two handles --------------------------------------------------------------------------------------------------------------------------------
def test_a_world_on_one_handle_does_not_change_another():
    from ikflow_amd.engine import Engine

    which, m, k = "panda", 65, 2
    robot, _ = H.kin_robots(which)
    eng = _eng(which)
    other = Engine(eng.layout, eng.robot, DEV)
    other.set_collision_model(*robot._collision_model)
    poses, q, _, cl, thr = WH.rank_case(which, m, k)
    opt = _opt(n_keep=2)
    before_a, before_b = _rank(eng, poses, q, k, opt), _rank(other, poses, q, k, opt)
    assert all(H.same_bits(before_a[n], before_b[n]) for n in before_a)
    eng.set_world(WH.scene(which, WH.RANK_SCENE), thr)
    assert eng.world_size == 7 and other.world_size == 0
    after_a, after_b = _rank(eng, poses, q, k, opt), _rank(other, poses, q, k, opt)
    assert all(H.same_bits(after_b[n], before_b[n]) for n in before_b)
    assert np.isposinf(after_a["row_score"]).sum() > np.isposinf(before_a["row_score"]).sum()
    assert (_clearance(other, q)["clearance"] == np.float32(3.0e38)).all()


# ---- 8. status codes -------------------------------------------------------------------------------------------------------------------------------
def _table(*obstacles):
    arr = (_lib.ikf_obstacle * len(obstacles))()
    for o, (kind, a, b, quat, radius) in zip(arr, obstacles):
        o.kind, o.radius = kind, radius
        for i in range(3):
            o.a[i], o.b[i] = a[i], b[i]
        for i in range(4):
            o.quat[i] = quat[i]
    return arr


def test_status_codes_name_the_obstacle_and_leave_the_world_as_it_was():
    from ikflow_amd.engine import Engine

    eng = _eng("panda")
    lib = eng.lib
    unit, zero = (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
    good = (0, (5.0, 0.0, 0.0), zero, unit, 0.1)
    nan = float("nan")
    fresh = Engine(eng.layout, eng.robot, DEV)   # no collision model
    assert lib.ikf_set_world(fresh._h, _table(good), 1, 0.0) == _lib.IKF_ERR_BAD_ARGUMENT and "without a collision model" in _lib.last_error(lib)
    assert lib.ikf_set_world(fresh._h, None, 0, 0.0) == _lib.IKF_OK   # (clearing needs none)
    q = torch.zeros(4, eng.layout.ndof, device=DEV)
    out = torch.empty(4, device=DEV)
    assert lib.ikf_world_clearance(fresh._h, q.data_ptr(), 4, out.data_ptr(), None, None, None, None) == _lib.IKF_ERR_BAD_ARGUMENT
    assert "no collision model" in _lib.last_error(lib)
    assert lib.ikf_world_clearance(eng._h, None, 4, out.data_ptr(), None, None, None, None) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_set_world(eng._h, _table(good, good), 2, 0.25) == _lib.IKF_OK and eng.world_size == 2
    bad = [
        ((7, zero, zero, unit, 0.1), "obstacle 1: unknown kind 7"),
        ((-1, zero, zero, unit, 0.1), "obstacle 1: unknown kind -1"),
        ((0, (nan, 0.0, 0.0), zero, unit, 0.1), "obstacle 1: non-finite number"),
        ((1, zero, (0.0, float("inf"), 0.0), unit, 0.1), "obstacle 1: non-finite number"),
        ((0, zero, zero, unit, -0.1), "obstacle 1: radius must be >= 0"),
        ((2, zero, (0.1, 0.0, 0.0), unit, 0.0), "obstacle 1: zero normal"),
        ((3, zero, (0.1, 0.0, 0.1), unit, 0.0), "obstacle 1: half extents must be > 0"),
        ((3, zero, (0.1, 0.1, 0.1), (0.0, 0.0, 0.0, 0.0), 0.0), "obstacle 1: zero quaternion"),
        ((3, zero, (0.1, 0.1, 0.1), (1.0, nan, 0.0, 0.0), 0.0), "obstacle 1: non-finite number"),
    ]
    for ob, msg in bad:
        assert lib.ikf_set_world(eng._h, _table(good, ob), 2, 0.0) == _lib.IKF_ERR_BAD_ARGUMENT
        assert msg in _lib.last_error(lib), (msg, _lib.last_error(lib))
    big = _table(*[good] * 65)
    assert lib.ikf_set_world(eng._h, big, 65, 0.0) == _lib.IKF_ERR_BAD_ARGUMENT and "0 .. 64" in _lib.last_error(lib)
    assert lib.ikf_set_world(eng._h, big, -1, 0.0) == _lib.IKF_ERR_BAD_ARGUMENT
    assert lib.ikf_set_world(eng._h, _table(good), 1, nan) == _lib.IKF_ERR_BAD_ARGUMENT and "min_clearance" in _lib.last_error(lib)
    assert lib.ikf_set_world(eng._h, None, 1, 0.0) == _lib.IKF_ERR_NULL_POINTER
    assert eng.world_size == 2   # every refused call left the world of two obstacles in force ...
    got = _clearance(eng, q.cpu())
    assert (got["obstacle"] == 0).all() and (got["colliding"] == 0).all() and (got["clearance"] > 3.0).all()   # ... with its threshold of 0.25
    assert lib.ikf_set_world(eng._h, big, 64, 0.0) == _lib.IKF_OK and eng.world_size == 64
    with pytest.raises(Exception, match="at most 64 obstacles"):
        eng.set_world([good] * 65)
    torch.cuda.synchronize()


# ---- 9. every capsule count: the LDS slices of k_world_clearance at their maximum, of the ranking with a world around its opt-in -------------
def _eng_model(which, model, used):
    eng = _eng_with(which, model, used)
    if eng not in _USED:
        _USED.append(eng)
    return eng


@pytest.mark.parametrize("name", ["mixed7", "full64"])
@pytest.mark.parametrize("which", RH.CASE_CHAINS)
def test_world_clearance_with_24_capsules(which, name, _small_model_back):
    """k_world_clearance with the 24-capsule model on chains of 4, 7 and 8 joints; with the 64 obstacles of full64 its dynamic LDS is at the
    maximum, 41216 B.  1, 63, 64, 65 and 66 rows against the fp64 reference, as test_world_clearance_against_the_fp64_reference."""
    eng = _eng_model(which, "caps24", _small_model_back)
    world = WH.scene(which, name, "caps24")
    q, ref, thr = WH.rows_and_reference(which, name, "caps24")
    eng.set_world(world, thr)
    assert eng.world_size == len(world) and 4 * (len(world) * 16 + 64 * ((6 * 24) | 1)) == (41216 if name == "full64" else 37568)
    assert len(set(ref["capsule"].tolist())) >= 5 and ref["capsule"].max() >= 16   # (the closest capsule changes with the row, late ones among them)
    for n in (1, 63, 64, 65, 66):
        _check_against_reference(_clearance(eng, q[:n]), ref, thr, n, f"{which} {name} caps24")


@pytest.mark.parametrize("which", RH.CASE_CHAINS)
def test_world_clearance_without_capsules(which, _small_model_back):
    """A model of no capsules (a slice of one float per thread): 3.0e38, no pair and no flag on every row, every element written."""
    eng = _eng_model(which, "caps0", _small_model_back)
    q = WH.rows_and_reference(which, "mixed7")[0]
    eng.set_world(WH.scene(which, "mixed7"), 0.05)
    for n in (1, 64, 130):
        out = _clearance(eng, q[:n])
        assert (out["clearance"] == np.float32(3.0e38)).all() and (out["obstacle"] == -1).all() and (out["capsule"] == -1).all() and (out["colliding"] == 0).all()


WORLD_MODELS = ("caps11", "caps12", "caps24")


def _world_rank_case(which, model):
    """The tile64 case of rank_helpers.capsule_case with the reference world clearances of its rows in the scene built for the model
    -> (case, world, world clearances, world threshold)."""
    seed = RH.CASE_SEEDS.get((which, model, "tile64"), 0)
    c = RH.capsule_case(which, model, "tile64")
    poses, q, _, cl, thr = WH.rank_case(which, c["m"], c["k"], model, seed)
    assert torch.equal(q, c["q"]) and torch.equal(poses, c["poses"])
    return c, WH.scene(which, WH.RANK_SCENE, model), cl, thr


@pytest.mark.parametrize("model", WORLD_MODELS)
@pytest.mark.parametrize("which", RH.CASE_CHAINS)
def test_ranking_with_a_world_around_the_opt_in_line(which, model, _small_model_back):
    """k_rank_candidates<.., WORLD> with 11 capsules (46848 B of LDS: under the opt-in line), 12 (49920 B: over it) and 24 (86784 B, the documented
    maximum), tile 64 and capacity 16, with and without reject_collisions: row scores by check_row_scores against the reference with the world
    term, the selection bit for bit."""
    orob = H.kin_robots(which)[1]
    c, world, cl, thr = _world_rank_case(which, model)
    m, k, n_keep = c["m"], c["k"], c["n_keep"]
    caps = RH.capsules(which, model)
    eng = _eng_model(which, model, _small_model_back)
    eng.set_world(world, thr)
    lds = RH.rank_lds_bytes(m, n_keep, len(caps), world=True)
    _check_the_straddle(model, m, n_keep, lds, world=True)
    assert lds == {"caps11": 46848, "caps12": 49920, "caps24": 86784}[model]
    for collisions in (False, True):
        self_thr = c["min_clearance"] if collisions else 0.0
        ref = WH.rank_reference(orob, caps, cl, thr, c["poses"], c["q"], k, 0.01, self_collisions=collisions, min_clearance=self_thr,
                                self_clearance=c["clearance"])
        assert RH.shares_hold(ref), (which, model, collisions, RH.shares(ref))
        out = _rank(eng, c["poses"], c["q"], k, _opt(n_keep=n_keep, collisions=collisions, min_clearance=self_thr))
        worst = RH.check_row_scores(out["row_score"], ref, f"{which} {model} collisions {collisions}")
        _check_selection(out, c["q"], m, k, n_keep, f"{which} {model} collisions {collisions}")
        print(f"ranking with a world {which} {model} collisions {collisions}: {lds} B of LDS, worst {worst:.3f} of eps, shares {RH.shares(ref)}")


_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
import rank_helpers as RH, world_helpers as WH
import test_world as TW
from test_ranked import _opt, _rank, OUTPUTS
d = np.load(sys.argv[2])
which, model = "panda", "caps24"
eng = TW._eng_with(which, model, [])
eng.set_world(WH.scene(which, WH.RANK_SCENE, model), float(d["thr"]))
out = _rank(eng, torch.tensor(d["poses"]), torch.tensor(d["q"]), int(d["k"]), _opt(n_keep=int(d["n_keep"]), collisions=True, min_clearance=float(d["self_thr"])))
np.savez(sys.argv[3], **out)
print("child ok")
"""


def test_the_24_capsule_world_call_as_the_first_ranking_call_of_a_process(tmp_path, _small_model_back):
    """The opt-in for more than 48 KiB of dynamic LDS is taken once per process and kernel: only in a fresh process is the largest call (86784 B)
    the first one.  The child's outputs have the bits of the same call in this process, which has ranked many smaller calls before."""
    import os
    import subprocess
    import sys

    which, model = "panda", "caps24"
    c, world, cl, thr = _world_rank_case(which, model)
    eng = _eng_model(which, model, _small_model_back)
    eng.set_world(world, thr)
    here = _rank(eng, c["poses"], c["q"], c["k"], _opt(n_keep=c["n_keep"], collisions=True, min_clearance=c["min_clearance"]))
    assert 0 < np.isposinf(here["row_score"]).sum() < len(here["row_score"])
    tests = os.path.dirname(os.path.abspath(__file__))
    np.savez(tmp_path / "in.npz", poses=c["poses"].numpy(), q=c["q"].numpy(), k=c["k"], n_keep=c["n_keep"], thr=thr, self_thr=c["min_clearance"])
    r = subprocess.run([sys.executable, "-c", _CHILD, tests, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True,
                       timeout=120, cwd=os.path.dirname(tests))
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    there = np.load(tmp_path / "out.npz")
    assert all(H.same_bits(there[n], here[n]) for n in here), [n for n in here if not H.same_bits(there[n], here[n])]
