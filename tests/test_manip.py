"""Singularity rule on the GPU (include/ikflow_amd_manip.h): ikf_manipulability against the singular-value reference of tests/manip_helpers.py on
every chain and part, and the floor as a rule of the candidate stage - ranked, diverse and path IK, beside a cloud, under a refinement, set and
cleared, reserved.  Tolerance: 4 x MANIP_TOL_ABS (measured on the CPU, tests/test_manip_math_host.py) plus one f32 ulp of w_ref; the rule is
compared outside a band of 8 x MANIP_TOL_ABS around the floor, which next to no row of these draws falls into (asserted on the CPU)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import cloud_helpers as CH
import helpers as H
import manip_helpers as MH
import rank_helpers as RH
from ikflow_amd import _lib
from test_ranked import _check_selection, _opt, _rank

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
W_SENTINEL = 0x7FC01234   # a NaN no arithmetic produces: a NaN measure is a legitimate output
BYTE_SENTINEL = 0xAB
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)
OUTPUTS = ("w", "below")
_USED = []


def _eng(which, collisions=False):
    """The shared kinematics engine of the chain (as tests/test_ranked.py's); its floor and its cloud are cleared after every test."""
    from ikflow_amd.engine import kinematics_engine_for

    robot = H.kin_robots(which)[0]
    eng = kinematics_engine_for(robot, DEV)
    if collisions:
        robot.set_collision_capsules(RH.collision_capsules(robot))
        eng.set_collision_model(*robot._collision_model)
        eng._collision_source = robot._collision_model
    if eng not in _USED:
        _USED.append(eng)
    return eng


def _fresh(which="panda"):
    from ikflow_amd.engine import Engine

    base = _eng(which)
    return Engine(base.layout, base.robot, DEV)


@pytest.fixture(autouse=True)
def _no_floor_left_behind():
    yield
    for eng in _USED:
        eng.set_min_manipulability(0.0)   # (the engines are shared with the other test modules)
        eng.clear_world_cloud()


def _manip(eng, q, part, floor=0.0, null=(), n=None, stream=None, expect=_lib.IKF_OK):
    """ikf_manipulability through eng.lib on guarded buffers -> {name: cpu numpy window}; `null`: the outputs passed as null; n: the row count
    passed (default: all rows of q); part: a name of manip_helpers.PARTS or a raw int."""
    q = torch.as_tensor(q)
    rows = q.shape[0]
    n = rows if n is None else n
    bufs = {}
    if "w" not in null:
        bufs["w"] = torch.full((rows + 2 * GUARD,), W_SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    if "below" not in null:
        bufs["below"] = torch.full((rows + 2 * GUARD,), BYTE_SENTINEL, dtype=torch.uint8, device=DEV)
    ptr = [bufs[o][GUARD:].data_ptr() if o in bufs else None for o in OUTPUTS]
    qd = q.to(DEV).contiguous()
    torch.cuda.synchronize()
    s = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(0)
    code = eng.lib.ikf_manipulability(eng._h, qd.data_ptr() if rows else None, n, _lib.MANIP_PARTS.get(part, part), float(floor), *ptr, s)
    assert code == expect, (code, _lib.last_error(eng.lib))
    torch.cuda.synchronize()
    out = {}
    for o, b in bufs.items():
        untouched = (lambda part_: bool((part_.view(torch.int32) == W_SENTINEL).all())) if o == "w" else (lambda part_: bool((part_ == BYTE_SENTINEL).all()))
        wrote = max(n, 0) if expect == _lib.IKF_OK else 0
        assert untouched(b[:GUARD]) and untouched(b[GUARD + wrote:]), f"{o}: an element outside the window was written"
        win = b[GUARD:GUARD + wrote]
        written = win.view(torch.int32) != W_SENTINEL if o == "w" else win != BYTE_SENTINEL
        assert bool(written.all()), f"{o}: an element inside the window was not written"
        out[o] = win.cpu().numpy().copy()
    return out


def _check(out, ref, floor, what):
    n = len(ref)
    if "w" in out:
        d = np.abs(out["w"].astype(np.float64) - ref.astype(np.float32))
        print(f"{what} n {n}: worst |engine - f32(w_ref)| {d.max():.3e} (allowed {MH.gpu_tol(ref).min():.3e} and up)")
        assert (d <= MH.gpu_tol(ref)).all(), (what, n, float(d.max()))
    if "below" in out:
        want, decided = MH.below_ref(ref, floor)
        assert np.array_equal(out["below"][decided], want[decided].astype(np.uint8)), what
        assert set(np.unique(out["below"])) <= {0, 1}


# ---- 1. the measure ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", MH.PARTS)
@pytest.mark.parametrize("which", MH.CHAINS)
def test_manipulability_against_the_singular_value_reference(which, part):
    """Every chain, every part, row counts around the wave and the block (1, 63, 64, 65, 255, 256, 257) and 1000: every element of both outputs
    written, nothing outside; w within the tolerance, the verdict against the median as the floor exact outside the band."""
    eng = _eng(which)
    q, ref = MH.draws(which), MH.reference(which, part)
    floor = float(np.median(ref[:1000]))
    for n in ROW_COUNTS:
        out = _manip(eng, q[:n], part, floor)
        _check(out, ref[:n], floor, f"{which} {part}")
    assert 300 <= out["below"].sum() <= 700


def test_outputs_are_nullable_streams_and_status_codes():
    """w only, below only and both give the same bits; a non-default stream; n = 0 is a no-op even with null pointers; n < 0, a part outside
    0 .. 2 and a negative, NaN or infinite floor are IKF_ERR_BAD_ARGUMENT, both outputs null IKF_ERR_NULL_POINTER - and nothing is written."""
    which, part = "fetch", "linear"
    eng = _eng(which)
    q, ref = MH.draws(which)[:257], MH.reference(which, part)[:257]
    floor = float(np.median(ref))
    both = _manip(eng, q, part, floor)
    _check(both, ref, floor, "both")
    assert H.same_bits(_manip(eng, q, part, floor, null=("below",))["w"], both["w"])
    assert H.same_bits(_manip(eng, q, part, floor, null=("w",))["below"], both["below"])
    side = torch.cuda.Stream(device=DEV)
    on_side = _manip(eng, q, part, floor, stream=side)
    assert H.same_bits(on_side["w"], both["w"]) and H.same_bits(on_side["below"], both["below"])
    _manip(eng, q, part, floor, n=0)
    assert eng.lib.ikf_manipulability(eng._h, None, 0, 0, 0.0, None, None, None) == _lib.IKF_OK
    _manip(eng, q, part, floor, n=-1, expect=_lib.IKF_ERR_BAD_ARGUMENT)
    _manip(eng, q, part, floor, null=OUTPUTS, expect=_lib.IKF_ERR_NULL_POINTER)
    for bad_part in (-1, 3):
        _manip(eng, q, bad_part, floor, expect=_lib.IKF_ERR_BAD_ARGUMENT)
    for bad_floor in (-0.1, float("nan"), float("inf")):
        _manip(eng, q, part, bad_floor, expect=_lib.IKF_ERR_BAD_ARGUMENT)
    assert eng.min_manipulability == (0.0, "full")   # (the query's floor is the call's own)


def test_nan_rows_and_the_gantry_on_the_device():
    """A NaN joint gives NaN and a row below every floor, 0 included; the gantry's known answers are exact on the device too."""
    eng = _eng("panda")
    q = MH.draws("panda")[:9].copy()
    for j in range(7):
        q[j, j] = np.nan
    for part in MH.PARTS:
        for floor in (0.0, 0.05):
            out = _manip(eng, q, part, floor)
            assert np.isnan(out["w"][:7]).all() and (out["below"][:7] == 1).all() and np.isfinite(out["w"][7:]).all()
    from ikflow_amd.engine import kinematics_engine_for

    gantry = MH.gantry()
    geng = kinematics_engine_for(gantry, DEV)
    qg = np.array([[0.0, 0.0, 0.0, 0.0], [0.3, -0.7, 0.25, 1.1]], np.float32)
    for part, want in (("linear", 1.0), ("angular", 0.0), ("full", 1.0)):
        out = _manip(geng, qg, part, 0.5)
        assert (out["w"] == np.float32(want)).all() and (out["below"] == (0 if want else 1)).all(), (part, out)


def test_refusals_leave_the_floor_as_it_was_and_the_getter_round_trips():
    eng = _fresh()
    lib, h = eng.lib, eng._h
    assert eng.min_manipulability == (0.0, "full")
    eng.set_min_manipulability(0.05, "linear")
    assert eng.min_manipulability == (float(np.float32(0.05)), "linear")
    for part, floor in ((1, -0.1), (1, float("nan")), (1, float("inf")), (1, -float("inf")), (3, 0.1), (-1, 0.1)):
        assert lib.ikf_set_min_manipulability(h, part, floor) == _lib.IKF_ERR_BAD_ARGUMENT
        assert "ikf_set_min_manipulability" in _lib.last_error(lib)
        assert eng.min_manipulability == (float(np.float32(0.05)), "linear")
    part, floor = C.c_int(-7), C.c_float(-7.0)
    assert lib.ikf_min_manipulability(h, C.byref(part), None) == _lib.IKF_OK and part.value == 1
    assert lib.ikf_min_manipulability(h, None, C.byref(floor)) == _lib.IKF_OK and floor.value == np.float32(0.05)
    eng.set_min_manipulability(0.0, "angular")
    assert eng.min_manipulability == (0.0, "angular")


# ---- 2. the gate in the ranking ----------------------------------------------------------------------------------------------------------------------
def _gate_inputs(which, m, k):
    orob = H.kin_robots(which)[1]
    q_all, ref_all, floor, part = MH.gate_case(which)
    _, poses = H.reachable_poses(orob, m, 50)
    return poses.float().contiguous(), torch.tensor(q_all[:m * k]), ref_all[:m * k], floor, part


@pytest.mark.parametrize("k", [1, 3, 16, 64])
@pytest.mark.parametrize("m", [1, 5, 65])
@pytest.mark.parametrize("which", list(MH.GATE_CASES))
def test_ranking_under_the_floor(which, m, k):
    """ikf_rank_candidates on the caller's rows: the row scores are those of the same call without the floor, bit for bit, with +inf exactly where
    the reference says below (band rows exempt); count_out, the kept rows and their indices follow; a floor above every row leaves nothing."""
    eng = _eng(which)
    poses, q, ref, floor, part = _gate_inputs(which, m, k)
    n_keep = min(4, k)
    opt = _opt(n_keep=n_keep, limits=True)
    off = _rank(eng, poses, q, k, opt)
    eng.set_min_manipulability(floor, part)
    on = _rank(eng, poses, q, k, opt)
    below, decided = MH.below_ref(ref, floor)
    want = off["row_score"].copy()
    want[below] = np.inf
    assert decided.mean() >= 0.99
    assert H.same_bits(on["row_score"][decided], want[decided]), f"{which} m {m} k {k}"
    loose = ~decided   # a band row is either of the two
    assert (np.isposinf(on["row_score"][loose]) | (on["row_score"][loose] == off["row_score"][loose])).all()
    _check_selection(on, q, m, k, n_keep, f"{which} m {m} k {k}")
    assert np.array_equal(on["count"], np.isfinite(on["row_score"]).reshape(k, m).sum(0))
    if m * k >= 80:
        assert np.isposinf(on["row_score"]).sum() > np.isposinf(off["row_score"]).sum() and np.isfinite(on["row_score"]).any()
    eng.set_min_manipulability(1.0e30, part)
    none = _rank(eng, poses, q, k, opt)
    assert (none["count"] == 0).all() and (none["index"] == -1).all() and np.isposinf(none["score"]).all() and np.isposinf(none["row_score"]).all()
    assert (none["q_out"] == 0).all()


def test_two_handles_with_different_floors():
    """The floor is the handle's: two engines of one robot, two floors and parts, the same rows - each drops what its own reference drops."""
    which, m, k = "panda", 65, 16
    poses, q, ref_full, floor_full, _ = _gate_inputs(which, m, k)
    ref_lin = MH.w_ref(MH.table_rows(H.kin_robots(which)[0]), q.numpy(), "linear")
    floor_lin = float(np.quantile(ref_lin, 0.25))
    a, b = _fresh(which), _fresh(which)
    opt = _opt(n_keep=4)
    plain = _rank(a, poses, q, k, opt)["row_score"]
    a.set_min_manipulability(floor_full, "full")
    b.set_min_manipulability(floor_lin, "linear")
    for eng, ref, floor in ((a, ref_full, floor_full), (b, ref_lin, floor_lin), (a, ref_full, floor_full)):
        below, decided = MH.below_ref(ref, floor)
        want = plain.copy()
        want[below] = np.inf
        assert decided.mean() >= 0.99 and H.same_bits(_rank(eng, poses, q, k, opt)["row_score"][decided], want[decided])
    assert a.min_manipulability[1] == "full" and b.min_manipulability[1] == "linear"


# ---- 3. beside a cloud -------------------------------------------------------------------------------------------------------------------------------
def test_ranking_under_the_floor_and_a_cloud():
    """A row is rejected exactly when either rule rejects it - the gate buffer carries both; afterwards ikf_cloud_clearance on the same rows still
    returns the clearances it returned before the floor was set."""
    which, m, k = "panda", 64, 16
    eng = _eng(which, collisions=True)
    poses, q, q_ref, _, _, cl, thr = CH.rank_case(which, m, k)
    ref = MH.w_ref(MH.table_rows(H.kin_robots(which)[0]), q.numpy(), "full")
    floor = float(np.median(ref))
    below, decided = MH.below_ref(ref, floor)
    assert decided.mean() >= 0.99
    opt = _opt(n_keep=4, ref_weight=0.05, limits=True)
    before = _rank(eng, poses, q, k, opt, q_ref)
    eng.set_world_cloud(CH.cloud(which, CH.RANK_POINTS), CH.POINT_RADIUS, thr)
    clearance, hit = eng.cloud_clearance(q.to(DEV))
    clearance, hit = clearance.cpu().numpy(), hit.cpu().numpy()
    cloud_only = _rank(eng, poses, q, k, opt, q_ref)
    eng.set_min_manipulability(floor, "full")
    both = _rank(eng, poses, q, k, opt, q_ref)
    want = before["row_score"].copy()
    want[hit | below] = np.inf
    assert H.same_bits(both["row_score"][decided], want[decided])
    live = np.isfinite(before["row_score"])
    assert (hit & ~below & live).sum() >= 0.1 * k * m and (below & ~hit & live).sum() >= 0.1 * k * m and (~hit & ~below & live).any()
    _check_selection(both, q, m, k, 4, "floor and cloud")
    again, hit_again = eng.cloud_clearance(q.to(DEV))
    assert H.same_bits(again.cpu().numpy(), clearance) and np.array_equal(hit_again.cpu().numpy(), hit)
    assert float(np.abs(clearance.astype(np.float64) - cl).max()) <= CH.CLEARANCE_TOL
    eng.set_min_manipulability(0.0)
    back = _rank(eng, poses, q, k, opt, q_ref)
    assert all(H.same_bits(back[o], cloud_only[o]) for o in back)   # (the cloud alone again)


# ---- 4. diverse-of-K and path IK ---------------------------------------------------------------------------------------------------------------------
def _outside_limits(q, rejected, orob):
    """A copy of the rows in which every rejected row is replaced by one beyond the first joint's upper limit."""
    out = q.clone()
    bad = q[0].clone()
    bad[0] = float(orob.actuated_joints_limits[0][1]) + 1.0
    out[torch.tensor(rejected)] = bad
    return out


def test_diverse_select_and_path_search_under_the_floor_equal_the_calls_on_rows_put_outside_the_limits():
    """ikf_diverse_select and ikf_path_search with the floor equal the same calls without it on a copy of the rows in which every row the reference
    rejects is an out-of-limits row under reject_limits - every output, bit for bit.  A waypoint whose candidates are all below the floor has
    reachable_out 0."""
    which, T, k = "panda", 5, 16
    eng = _eng(which)
    orob = H.kin_robots(which)[1]
    poses, q, ref, floor, part = _gate_inputs(which, T, k)
    q_all, ref_all, _, _ = MH.gate_case(which)
    below, decided = MH.below_ref(ref, floor)
    assert decided.all() and (~below).reshape(k, T).any(0).all() and below.any()
    yd = poses.to(DEV)
    dopt = eng.diverse_options(n_keep=4, reject_limits=True, min_separation=0.05)
    popt = eng.path_options(reject_limits=True, node_weight=20.0)

    def calls(rows):
        outs = list(eng.diverse_select(yd, k, rows.to(DEV), dopt, row_scores=True)) + list(eng.path_search(yd, k, rows.to(DEV), popt, node_costs=True))
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in outs]

    want = calls(_outside_limits(q, below, orob))
    plain = calls(q)
    eng.set_min_manipulability(floor, part)
    got = calls(q)
    assert all(H.same_bits(g, w) for g, w in zip(got, want))
    assert not all(H.same_bits(g, p) for g, p in zip(got, plain))   # (the floor does something here)
    rows_d, node = got[6], got[11]
    assert np.isposinf(rows_d[below]).all() and np.isfinite(rows_d[~below]).all() and H.same_bits(rows_d, node)
    reach = got[10]
    assert (reach > 0).all() and np.isfinite(got[9][0])
    # waypoint 2: every candidate a row surely below the floor
    low = q_all[np.flatnonzero(ref_all < floor - MH.BAND)[:k]]
    q2 = q.clone().reshape(k, T, -1)
    q2[:, 2] = torch.tensor(low)
    q2 = q2.reshape(k * T, -1)
    below2 = below.reshape(k, T).copy()
    below2[:, 2] = True
    got2 = calls(q2)
    eng.set_min_manipulability(0.0)
    want2 = calls(_outside_limits(q2, below2.reshape(-1), orob))
    assert all(H.same_bits(g, w) for g, w in zip(got2, want2))
    # (reachable_out counts the candidates a path can arrive at: nothing is reachable from an empty waypoint on)
    assert (got2[10][:2] > 0).all() and (got2[10][2:] == 0).all() and np.isposinf(got2[9][0]) and got2[5][2] == 0


# ---- 5. the flow in front ----------------------------------------------------------------------------------------------------------------------------
def _solver(model="tiny"):
    from ikflow_amd.ikflow_solver import IKFlowSolver

    robot, hp, lay, sd = H.tiny_model() if model == "tiny" else H.panda_model()
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    return s, robot, lay


def _floor_in_a_gap(ref):
    """A floor between the 30 % and the 70 % quantile of the reference values, in the middle of the widest gap between two neighbours there:
    refined candidates of one pose gather on a few solutions, and a median would sit inside such a cluster, i.e. inside the band."""
    v = np.sort(ref)
    v = v[int(0.3 * len(v)):int(0.7 * len(v))]
    i = int(np.argmax(np.diff(v)))
    return float(0.5 * (v[i] + v[i + 1]))


@pytest.mark.parametrize("refine", [0, 2])
def test_generate_ranked_under_the_floor_equals_the_flow_then_rank_candidates(refine):
    """ikf_generate_ranked under a floor (through IKFlowSolver.set_min_manipulability and generate_ranked_ik_solutions) equals its parts - the flow
    rows of ikf_generate_approx on the tiled inputs (and, with a refinement set, their LM steps), then ikf_rank_candidates under the floor - bit for
    bit: under refinement the REFINED rows are tested.  The new +inf rows are the reference's; clearing the floor gives the first call's bits."""
    from ikflow_amd.ikflow_solver import mm_to_m

    s, robot, lay = _solver()
    m, k, n_keep = 65, 16, 4
    _, poses = H.reachable_poses(robot, m, 6)
    y, L = poses.float().to(DEV), H.latents(k * m, lay.dim, 8).to(DEV)
    q = s.generate_ik_solutions(y.repeat((k, 1)), latent=L)
    eng = s.engine(DEV)
    if refine:
        q = eng.refine_candidates(y, k, q, refine, 0.0, 0.0)
        s.set_candidate_refine(refine, 0.0, 0.0)
    without = s.generate_ranked_ik_solutions(y, k, n_keep, latent=L, reject_self_collisions=False, return_row_scores=True)
    ref = MH.w_ref(MH.table_rows(robot), q.cpu().numpy(), "full")
    floor = _floor_in_a_gap(ref)
    below, decided = MH.below_ref(ref, floor)
    s.set_min_manipulability(floor)
    assert eng.min_manipulability == (float(np.float32(floor)), "full")
    got = s.generate_ranked_ik_solutions(y, k, n_keep, latent=L, reject_self_collisions=False, return_row_scores=True)
    opt = eng.rank_options(n_keep, mm_to_m(1) / 0.1, 0.0, None, None, True, False, 0.0)
    two_step = eng.rank_candidates(y, k, q, opt, row_scores=True)
    for a, b in zip(got, two_step):
        assert H.same_bits(a.cpu().numpy(), b.cpu().numpy())
    rows, rows_without = got.row_scores.cpu().numpy(), without.row_scores.cpu().numpy()
    want = rows_without.copy()
    want[below] = np.inf
    assert decided.mean() >= 0.99 and H.same_bits(rows[decided], want[decided])
    assert np.isposinf(rows_without).sum() < np.isposinf(rows).sum() < k * m
    s.set_min_manipulability(0.0)
    again = s.generate_ranked_ik_solutions(y, k, n_keep, latent=L, reject_self_collisions=False, return_row_scores=True)
    for a, b in zip(again, without):
        assert H.same_bits(a.cpu().numpy(), b.cpu().numpy())
    s.set_candidate_refine(0)


def test_solver_floor_set_before_the_engine_exists_reaches_it():
    s, robot, lay = _solver()
    s.set_min_manipulability(0.04, "linear")
    assert s.engine(DEV).min_manipulability == (float(np.float32(0.04)), "linear")
    s.set_min_manipulability(0)
    assert s.engine(DEV).min_manipulability == (0.0, "full")


# ---- 6. off means off --------------------------------------------------------------------------------------------------------------------------------
def test_a_cleared_floor_gives_every_entry_point_the_bits_of_a_handle_that_never_had_one():
    from ikflow_amd.engine import Engine

    s, robot, lay = _solver()
    m, k = 9, 16
    _, poses = H.reachable_poses(robot, m, 4)
    y, L = poses.float().to(DEV), H.latents(k * m, lay.dim, 9).to(DEV)
    rows = s.generate_ik_solutions(y.repeat((k, 1)), latent=L)

    def engine():
        eng = Engine(s.layout, robot, DEV)
        eng.load_state_dict(s._state_dict_np)
        return eng

    def six(eng):
        ro, po, do = eng.rank_options(n_keep=4, reject_limits=True), eng.path_options(reject_limits=True), eng.diverse_options(n_keep=4, min_separation=0.05)
        outs = list(eng.generate_ranked(y, k, L, True, ro, row_scores=True))
        outs += list(eng.generate_path(y, k, L[:k], True, True, po))
        outs += list(eng.generate_diverse(y, k, L, True, do))
        outs += list(eng.rank_candidates(y, k, rows, ro, row_scores=True))
        outs += list(eng.path_search(y, k, rows, po, node_costs=True))
        outs += list(eng.diverse_select(y, k, rows, do, row_scores=True))
        torch.cuda.synchronize()
        return [None if t is None else t.cpu().numpy() for t in outs]

    same = lambda xs, ys: all((a is None and b is None) or H.same_bits(a, b) for a, b in zip(xs, ys))
    never = six(engine())
    eng = engine()
    eng.set_min_manipulability(float(eng.manipulability(rows)[0].median()) + 1e-4, "full")
    assert not same(six(eng), never)   # (the floor does something here)
    eng.set_min_manipulability(0.0)
    assert same(six(eng), never), "cleared"
    eng.set_min_manipulability(0.0, "angular")
    assert same(six(eng), never), "a part without a floor"


# ---- 7. memory ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_reservation_made_under_the_floor_covers_the_gate():
    """After ikf_reserve_ranked with the floor set, a call of the reserved size allocates nothing: the device's free memory moves by no more than
    torch's own reserve (the accounting of tests/test_handle_memory.py)."""
    which, m, k = "panda", 4096, 256
    orob = H.kin_robots(which)[1]
    _, poses = H.reachable_poses(orob, m, 3)
    rng = np.random.default_rng(5)
    yd = poses.float().to(DEV)
    qd = torch.tensor(H.kin_robots(which)[0].sample_joint_angles(m * k, 0.0, rng)).to(DEV)
    floor = 0.03

    def call(eng):
        outs = eng.rank_candidates(yd, k, qd, eng.rank_options(n_keep=4), row_scores=True)
        torch.cuda.synchronize()
        count = outs[3].cpu().numpy()
        del outs
        return count

    warm = _fresh(which)   # (the kernels' code objects and torch's blocks for the outputs are there before anything is measured)
    warm.set_min_manipulability(floor)
    want = call(warm)
    del warm
    eng = _fresh(which)
    eng.set_min_manipulability(floor)
    eng.reserve_ranked(m, k)
    gc.collect()
    torch.cuda.synchronize()
    free0, stat0 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    got = call(eng)
    free1, stat1 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    assert np.array_equal(got, want) and 0 < got.sum() < m * k
    assert free0 - free1 <= stat1 - stat0, f"the reserved call took {free0 - free1 - (stat1 - stat0)} bytes of device memory"


# ---- 8. the Python face ------------------------------------------------------------------------------------------------------------------------------
def test_robot_manipulability():
    robot = H.kin_robots("fetch")[0]
    q = torch.tensor(MH.draws("fetch")[:300]).to(DEV)
    for part in MH.PARTS:
        w = robot.manipulability(q, part)
        ref = MH.reference("fetch", part)[:300]
        assert w.shape == (300,) and w.dtype == torch.float32 and w.device.type == "cuda"
        assert (np.abs(w.cpu().numpy().astype(np.float64) - ref.astype(np.float32)) <= MH.gpu_tol(ref)).all()
    assert H.same_bits(robot.manipulability(q).cpu().numpy(), robot.manipulability(q, "full").cpu().numpy())
    with pytest.raises(KeyError):
        robot.manipulability(q, "position")
