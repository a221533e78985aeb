"""Refined candidates on the GPU (include/ikflow_amd_refine.h; ikflow_amd/csrc/refine_kernels.hip, refine_math.h, api_refine.hip and the hook in
flow_candidates, api_rank.hip): ikf_refine_candidates against a loop of the oracle (tests/refine_helpers.py) on guarded buffers, the same rows
through ikf_lm_step / ikf_pose_error iterated from Python, the composition flow -> refine -> rank / diverse / path against the one-call entries bit
for bit, the calls a refinement must not change, the purpose judged by fp64 alone, status codes and the Python wrappers.

Criterion of tests 1 and 2: that of test_exact_ik_seeded_is_row_exact_against_the_oracle (tests/test_gpu_parity.py), row by row - see
refine_helpers.check_against_oracle.  The band may hold at most 3 % of the rows of a case's shapes taken together (a 1-row shape cannot carry a
share) and of its 600-row shape alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H
import rank_helpers as RH
import refine_helpers as RF
import sweep_helpers as SH
import world_helpers as WH
from ikflow_amd import _lib
from oracle import kinematics_oracle as ko
from test_diverse import OUTPUTS as DIVERSE_OUTPUTS, _div, _dopt
from test_path import OUTPUTS as PATH_OUTPUTS, _path, _popt
from test_ranked import DEV, GUARD, NAN_BITS, OUTPUTS as RANK_OUTPUTS, _eng, _opt, _rank

pytestmark = pytest.mark.gpu
BYTE_SENTINEL = 0xAB
SHAPES = [(1, 1), (1, 255), (3, 85), (3, 86), (257, 1), (100, 6)]   # n_poses x k: 1, 255 (3 x 85 too), 258 (the 256th row and two more), 257, 600 rows
_TOUCHED = []


@pytest.fixture(autouse=True)
def _no_refinement_left_behind():
    yield
    for eng in _TOUCHED:   # (the kinematics engines are shared with the other test modules)
        eng.set_candidate_refine(0)
        eng.set_lm_precision("f64")
        eng.set_path_sweep(0)
        eng.clear_world()
    del _TOUCHED[:]


def _touch(eng):
    _TOUCHED.append(eng)
    return eng


def _refine(eng, poses, q, k, n_steps, pos_tol, rot_tol, null=(), inplace=False, stream=None, n_poses=None, expect=_lib.IKF_OK):
    """ikf_refine_candidates through eng.lib on guarded buffers -> {"q": f32 [rows x nd], "steps": uint8 [rows], "converged": uint8 [rows]} (cpu
    numpy); `null`: info outputs passed as null; `inplace`: d_q_out = d_q (the guards then surround the input rows)."""
    rows, nd = q.shape[0], eng.layout.ndof
    n_poses = poses.shape[0] if n_poses is None else n_poses
    live = 0 if expect != _lib.IKF_OK else rows if n_poses == poses.shape[0] else max(n_poses, 0) * k   # rows the call must write
    qbuf = torch.full((rows + 2 * GUARD, nd), float("nan"), dtype=torch.float32, device=DEV)
    q_d = torch.as_tensor(q).to(DEV).contiguous()
    if inplace:
        qbuf[GUARD:GUARD + rows] = q_d
        q_d = qbuf[GUARD:]
    info = {o: torch.full((rows + 2 * GUARD,), BYTE_SENTINEL, dtype=torch.uint8, device=DEV) for o in ("steps", "converged") if o not in null}
    ptr = [info[o][GUARD:].data_ptr() if o in info else None for o in ("steps", "converged")]
    poses_d = torch.as_tensor(poses).to(DEV).contiguous()
    torch.cuda.synchronize()
    s = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(0)
    code = eng.lib.ikf_refine_candidates(eng._h, poses_d.data_ptr(), n_poses, k, q_d.data_ptr(), n_steps, pos_tol, rot_tol, qbuf[GUARD:].data_ptr(),
                                         *ptr, s)
    assert code == expect, (code, _lib.last_error(eng.lib))
    torch.cuda.synchronize()
    bits = qbuf.view(torch.int32)
    assert bool((bits[:GUARD] == NAN_BITS).all()) and bool((bits[GUARD + rows:] == NAN_BITS).all()), "q_out: a row outside the window was written"
    win = qbuf[GUARD:GUARD + rows]
    assert not bool(torch.isnan(win[:live]).any()), "q_out: an element inside the window was not written"
    if not inplace:
        assert bool((win.view(torch.int32)[live:] == NAN_BITS).all()), "q_out: a refused or empty call wrote an output"
    out = {"q": win.cpu().numpy().copy()}
    for o, buf in info.items():
        assert bool((buf[:GUARD] == BYTE_SENTINEL).all()) and bool((buf[GUARD + live:] == BYTE_SENTINEL).all()), f"{o}: an element outside the window was written"
        assert bool((buf[GUARD:GUARD + live] != BYTE_SENTINEL).all()), f"{o}: an element inside the window was not written"
        out[o] = buf[GUARD:GUARD + rows].cpu().numpy().copy()
    return out


# ---- 1. ikf_refine_candidates against the oracle loop -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos_tol,rot_tol", RF.TOLERANCES)
@pytest.mark.parametrize("which", RF.CHAINS)
def test_refine_candidates_against_a_loop_of_the_oracle(which, pos_tol, rot_tol):
    """Every shape of SHAPES, 4 steps.  fp64 mode: steps, converged and the rows against the oracle loop; f32 mode: the statistical form of check_lm
    on the final rows, pooled over the shapes.  In place == out of place bit for bit; each info output null in turn and a second stream give the
    same bits."""
    eng = _touch(_eng(which))
    n_band, n_rows, parts = 0, 0, []
    for n_poses, k in SHAPES:
        case = RF.oracle_case(which, n_poses, k, pos_tol, rot_tol)
        poses, seeds = case["poses"], case["seeds"]
        label = f"{which} {n_poses} x {k}"
        for mode in ("f64", "f32"):
            eng.set_lm_precision(mode)
            out = _refine(eng, poses, seeds, k, RF.N_STEPS, pos_tol, rot_tol)
            assert set(np.unique(out["converged"])) <= {0, 1} and out["steps"].min() >= 1 and out["steps"].max() <= RF.N_STEPS
            assert ((out["steps"] < RF.N_STEPS) <= (out["converged"] == 1)).all()       # a row that stopped early stopped on its test
            same = _refine(eng, poses, seeds, k, RF.N_STEPS, pos_tol, rot_tol, inplace=True)
            assert all(H.same_bits(same[o], out[o]) for o in out), f"{label} {mode}: in place differs from out of place"
            if mode == "f64":
                band = RF.check_against_oracle(case, out["q"], out["steps"], out["converged"], label)
                n_band, n_rows = n_band + band, n_rows + len(seeds)
                if n_poses * k == 600:
                    assert band <= RF.BAND_CAP * 600, band
            else:
                parts.append(RF.f32_distances(case, out["q"]))
            if (n_poses, k) == (100, 6):
                for null in (("steps",), ("converged",), ("steps", "converged")):
                    got = _refine(eng, poses, seeds, k, RF.N_STEPS, pos_tol, rot_tol, null=null, inplace=null == ("steps",))
                    assert set(got) == {"q", "steps", "converged"} - set(null) and all(H.same_bits(got[o], out[o]) for o in got)
                side = _refine(eng, poses, seeds, k, RF.N_STEPS, pos_tol, rot_tol, stream=torch.cuda.Stream(device=DEV))
                assert all(H.same_bits(side[o], out[o]) for o in out)
    print(f"{which} tol ({pos_tol:g}, {rot_tol:g}): {n_band} of {n_rows} rows in the band")
    assert n_band <= RF.BAND_CAP * n_rows, (n_band, n_rows)
    RF.check_f32_against_oracle(parts, f"{which} tol ({pos_tol:g}, {rot_tol:g}), all shapes")


def test_every_step_count_occurs_and_the_edge_cases():
    """panda at (1e-3, 0.1), the 600 x 1 rows of the host test: every step count 1 .. 4 occurs.  Tolerance 0 runs all steps, converged 0; n_steps =
    1 is one ikf_lm_step (within 5e-6 in fp64 mode; whether bit for bit is printed - tests/test_refine_math_host.py asserts it of the source);
    rot_tol = 9e-4 never converges; a NaN row comes out clamped and finite (the step's clamp maps a NaN joint to a limit) and leaves its
    neighbours alone; n_steps = 16 is accepted."""
    eng = _touch(_eng("panda"))
    case = RF.oracle_case("panda", 600, 1, 1e-3, 0.1)
    poses, seeds = case["poses"], case["seeds"]
    out = _refine(eng, poses, seeds, 1, RF.N_STEPS, 1e-3, 0.1)
    RF.check_against_oracle(case, out["q"], out["steps"], out["converged"], "panda 600 x 1")
    counts = np.bincount(out["steps"], minlength=RF.N_STEPS + 1)[1:]
    print("steps 1 .. 4:", counts.tolist())
    assert (counts > 0).all()
    for mode in ("f64", "f32"):
        eng.set_lm_precision(mode)
        all16 = _refine(eng, poses, seeds, 1, 16, 0.0, 0.0)
        assert (all16["steps"] == 16).all() and (all16["converged"] == 0).all()
        one = _refine(eng, poses, seeds, 1, 1, 10.0, 10.0)
        assert (one["steps"] == 1).all() and (one["converged"] == 1).all()
        step = eng.lm_step(poses.to(DEV), seeds.to(DEV)).cpu().numpy()    # another kernel around the same source: contraction may differ, so no bit claim
        print(f"{mode}: n_steps = 1 bit-equal to ikf_lm_step: {H.same_bits(one['q'], step)}, max |d| {np.abs(one['q'] - step).max():.2e}")
        if mode == "f64":
            assert np.abs(one["q"] - step).max() <= 5e-6
        never = _refine(eng, poses, seeds, 1, 6, 1.0, 9e-4)
        assert (never["steps"] == 6).all() and (never["converged"] == 0).all()
        bad = seeds.clone()
        bad[300, 2] = float("nan")
        good = _refine(eng, poses, seeds, 1, RF.N_STEPS, 1e-3, 0.1)
        qbuf = torch.full((600 + 2 * GUARD, 7), float("nan"), dtype=torch.float32, device=DEV)   # (the NaN row defeats _refine's written-check)
        st = torch.full((600,), BYTE_SENTINEL, dtype=torch.uint8, device=DEV)
        cv = torch.full((600,), BYTE_SENTINEL, dtype=torch.uint8, device=DEV)
        pd, bd = poses.to(DEV), bad.to(DEV)
        assert eng.lib.ikf_refine_candidates(eng._h, pd.data_ptr(), 600, 1, bd.data_ptr(), RF.N_STEPS, 1e-3, 0.1, qbuf[GUARD:].data_ptr(), st.data_ptr(),
                                             cv.data_ptr(), None) == _lib.IKF_OK
        torch.cuda.synchronize()
        got = qbuf[GUARD:GUARD + 600].cpu().numpy()
        others = np.arange(600) != 300
        assert 1 <= int(st[300]) <= RF.N_STEPS and int(cv[300]) in (0, 1)
        assert H.same_bits(got[others], good["q"][others]) and np.array_equal(st.cpu().numpy()[others], good["steps"][others])
        assert bool((qbuf[:GUARD].view(torch.int32) == NAN_BITS).all()) and bool((qbuf[GUARD + 600:].view(torch.int32) == NAN_BITS).all())
        lo, hi = RH.limits(case["orob"])
        assert np.isfinite(got[300]).all() and (got[300] >= lo.numpy()).all() and (got[300] <= hi.numpy()).all()   # as LM steps leave it: clamped, finite


# ---- 2. the same rows through ikf_lm_step / ikf_pose_error iterated from Python ---------------------------------------------------------------------
@pytest.mark.parametrize("which", RF.CHAINS)
def test_the_python_loop_over_lm_step_and_pose_error_meets_the_same_criterion(which):
    eng = _touch(_eng(which))
    exact = []
    for pos_tol, rot_tol in RF.TOLERANCES:
        case = RF.oracle_case(which, 100, 6, pos_tol, rot_tol)
        tiled, q = case["tiled"].to(DEV), case["seeds"].to(DEV)
        rows = q.shape[0]
        steps = torch.zeros(rows, dtype=torch.int64, device=DEV)
        conv = torch.zeros(rows, dtype=torch.bool, device=DEV)
        active = torch.ones(rows, dtype=torch.bool, device=DEV)
        for it in range(RF.N_STEPS):
            q = torch.where(active[:, None], eng.lm_step(tiled, q), q)
            steps = torch.where(active, torch.full_like(steps, it + 1), steps)
            pe, re = eng.pose_error(q, tiled)
            done = active & (pe < torch.tensor(pos_tol, dtype=torch.float32, device=DEV)) & (re < torch.tensor(rot_tol, dtype=torch.float32, device=DEV))
            conv |= done
            active &= ~done
        RF.check_against_oracle(case, q.cpu().numpy(), steps.cpu().numpy(), conv.cpu().numpy(), f"{which} 100 x 6, python loop")
        one = _refine(eng, case["poses"], case["seeds"], 6, RF.N_STEPS, pos_tol, rot_tol)
        exact.append(H.same_bits(one["q"], q.cpu().numpy()) and np.array_equal(one["steps"], steps.cpu().numpy()) and np.array_equal(one["converged"] == 1, conv.cpu().numpy()))
    print(f"{which}: ikf_refine_candidates bit-equal to the python loop over ikf_lm_step / ikf_pose_error: {exact}")   # (reported, not asserted)


# ---- 3. composition, bit for bit ----------------------------------------------------------------------------------------------------------------------
_SOLVERS = {}


def _solver(model):
    """(solver, robot, layout) with a robot of this module's own: its capsule model must not reach the solvers other modules share."""
    from ikflow_amd.ikflow_solver import IKFlowSolver

    if model not in _SOLVERS:
        robot, hp, lay, sd = H.tiny_model() if model == "tiny" else H.panda_model()
        robot.set_collision_capsules(RH.collision_capsules(robot))
        s = IKFlowSolver(hp, robot)
        s.load_state_dict_tensors(sd)
        eng = s.engine(DEV)
        eng.set_collision_model(*robot._collision_model)
        eng._collision_source = robot._collision_model
        _SOLVERS[model] = (s, robot, lay)
    return _SOLVERS[model]


def _same(a, b, names):
    return all(H.same_bits(a[n], b[n]) for n in names)


@pytest.mark.parametrize("m,k", [(1, 1), (5, 13), (65, 4), (1, 5000)])
@pytest.mark.parametrize("model", ["tiny", "panda"])
def test_flow_then_refine_then_the_own_rows_entry_equals_the_one_call_entry(model, m, k):
    """With a refinement set: ikf_generate_approx on the tiled poses -> ikf_refine_candidates -> ikf_rank_candidates / ikf_diverse_select /
    ikf_path_search == ikf_generate_ranked / _diverse / _path (both latent forms; a world and a sweep of 2 set), every output bit for bit.
    (1, 5000) is a chunked ranking call: beyond the k limits of the other two families, so ranking only."""
    s, robot, lay = _solver(model)
    eng = _touch(s.engine(DEV))
    steps, pos_tol, rot_tol = 3, 1e-3, 0.1
    eng.set_candidate_refine(steps, pos_tol, rot_tol)
    _, poses = H.reachable_poses(robot, m, 16)
    poses = poses.float()
    L = H.latents(k * m, lay.dim, 18)
    flow = eng.generate_approx(poses.to(DEV).repeat((k, 1)), L.to(DEV), True)
    ref = _refine(eng, poses, flow.cpu(), k, steps, pos_tol, rot_tol)
    rows = torch.from_numpy(ref["q"])
    print(f"{model} ({m}, {k}): steps {np.bincount(ref['steps'], minlength=steps + 1)[1:].tolist()}, converged {int(ref['converged'].sum())} of {k * m}")
    ropt = _opt(n_keep=min(k, 4), limits=True, max_pos=0.3, max_rot=2.0, collisions=True, min_clearance=-0.02)
    if m == 1 and k == 5000:
        assert eng.rank_chunks(m, k) > 1
    assert _same(_rank(eng, poses, rows, k, ropt), _rank(eng, poses, None, k, ropt, latent=L), RANK_OUTPUTS)
    assert not H.same_bits(rows.numpy(), flow.cpu().numpy())                                           # (here the refinement does matter)
    if k > 1024:
        return
    dopt = _dopt(n_keep=min(k, 3), limits=True, max_pos=0.3, max_rot=2.0, min_sep=0.05)
    assert _same(_div(eng, poses, rows, k, dopt), _div(eng, poses, None, k, dopt, latent=L), DIVERSE_OUTPUTS)
    world = WH.scene("panda", SH.LATTICE_SCENE)   # (both models' robot is the Panda)
    eng.set_world(world, 0.0)
    eng.set_world(world, float(torch.quantile(eng.world_clearance(rows.to(DEV))[0], 0.25)))   # not an accuracy claim: a threshold that rejects a quarter of these rows
    eng.set_path_sweep(2)
    popt = _popt(limits=True)
    two = _path(eng, poses, rows, k, popt)
    assert _same(two, _path(eng, poses, None, k, popt, latent=L, shared=False), PATH_OUTPUTS)
    Lk = L[:k].contiguous()
    expanded = Lk[:, None, :].expand(k, m, lay.dim).reshape(k * m, lay.dim).contiguous()
    flow_s = eng.generate_approx(poses.to(DEV).repeat((k, 1)), expanded.to(DEV), True)
    rows_s = torch.from_numpy(_refine(eng, poses, flow_s.cpu(), k, steps, pos_tol, rot_tol)["q"])
    assert _same(_path(eng, poses, rows_s, k, popt), _path(eng, poses, None, k, popt, latent=Lk, shared=True), PATH_OUTPUTS)
    assert _same(_rank(eng, poses, rows, k, ropt), _rank(eng, poses, None, k, ropt, latent=L), RANK_OUTPUTS)   # ... and ranking under that world


# ---- 4. off means off ------------------------------------------------------------------------------------------------------------------------------------
def test_refinement_off_and_another_handle_give_the_calls_of_before_bit_for_bit():
    from ikflow_amd.engine import Engine

    s, robot, lay = _solver("tiny")
    eng = _touch(s.engine(DEV))
    other = Engine(s.layout, robot, DEV)
    other.load_state_dict(s._state_dict_np)
    other.set_collision_model(*robot._collision_model)
    m, k = 33, 20
    _, poses = H.reachable_poses(robot, m, 26)
    poses = poses.float()
    L = H.latents(k * m, lay.dim, 28)
    rows = eng.generate_approx(poses.to(DEV).repeat((k, 1)), L.to(DEV), True).cpu()
    ropt, dopt, popt = _opt(n_keep=3, limits=True), _dopt(n_keep=3, limits=True, min_sep=0.05), _popt(limits=True)

    def six(e):
        return [(_rank(e, poses, rows, k, ropt), RANK_OUTPUTS), (_rank(e, poses, None, k, ropt, latent=L), RANK_OUTPUTS),
                (_div(e, poses, rows, k, dopt), DIVERSE_OUTPUTS), (_div(e, poses, None, k, dopt, latent=L), DIVERSE_OUTPUTS),
                (_path(e, poses, rows, k, popt), PATH_OUTPUTS), (_path(e, poses, None, k, popt, latent=L, shared=False), PATH_OUTPUTS)]

    same = lambda x, y: [_same(a[0], b[0], a[1]) for a, b in zip(x, y)]
    assert eng.candidate_refine() == (0, 0.0, 0.0) and other.candidate_refine() == (0, 0.0, 0.0)
    before, before_b = six(eng), six(other)
    assert all(same(before, before_b))
    eng.set_candidate_refine(4, 1e-3, 0.1)
    assert eng.candidate_refine()[0] == 4 and other.candidate_refine() == (0, 0.0, 0.0)
    assert same(six(eng), before) == [True, False, True, False, True, False]    # the own-rows entries never refine; the flow entries now do
    assert all(same(six(other), before_b))                                      # a refinement on handle A leaves handle B alone
    eng.set_candidate_refine(0)
    assert eng.candidate_refine() == (0, 0.0, 0.0)
    assert all(same(six(eng), before))
    fresh = Engine(s.layout, robot, DEV)
    fresh.load_state_dict(s._state_dict_np)
    fresh.set_collision_model(*robot._collision_model)
    assert all(same(six(fresh), before))


# ---- 5. the purpose, judged by fp64 alone -----------------------------------------------------------------------------------------------------------------
def test_refined_best_of_k_returns_rows_that_reach_the_pose_and_pass_every_rule():
    """Panda width, seeded weights, 64 reachable poses, k = 32, thresholds 1 mm / 0.1 rad, joint limits, the capsule model and a world.  The oracle
    loop (fp64 step) runs on the engine's own flow output; a pose counts when that loop leaves it a candidate that the fp64 references of
    rank_helpers / world_helpers admit, clear of their bands and of the loop's own.  For every such pose the refined call returns a row whose fp64
    pose error is under both thresholds and whose fp64 self and world clearances are at or above the minimum (less world_helpers.BAND).  Without
    refinement strictly fewer poses have an admissible candidate."""
    s, robot, lay = _solver("panda")
    orob = H.O(robot)
    eng = _touch(s.engine(DEV))
    m, k, pos_thr, rot_thr, self_min, world_min = 64, 32, 1e-3, 0.1, -0.03, -0.1   # (each minimum rejects about a tenth of the refined rows)
    caps = RH.collision_capsules(robot)
    world = WH.scene("panda", "mixed7")
    eng.set_world(world, world_min)
    _, poses = H.reachable_poses(robot, m, 6)
    poses = poses.float()
    L = H.latents(k * m, lay.dim, 8)
    opt = _opt(n_keep=1, limits=True, max_pos=pos_thr, max_rot=rot_thr, collisions=True, min_clearance=self_min)
    plain = _rank(eng, poses, None, k, opt, latent=L)
    eng.set_candidate_refine(4, pos_thr, rot_thr)
    refined = _rank(eng, poses, None, k, opt, latent=L)
    flow = eng.generate_approx(poses.to(DEV).repeat((k, 1)), L.to(DEV), True).cpu()
    tiled = poses.repeat((k, 1))
    rq, _, conv, margins = RF.oracle_refine(orob, tiled, flow, 4, pos_thr, rot_thr)
    wcl = WH.reference(orob, caps, world, rq.double())["clearance"]
    ref = WH.rank_reference(orob, caps, wcl, world_min, poses, rq, k, 0.01, self_collisions=True, min_clearance=self_min, max_pos=pos_thr,
                            max_rot=rot_thr, reject_limits=False)
    inside = ~ko.calculate_joint_limits_exceeded(rq, orob.actuated_joints_limits).numpy()      # (the loop clamps: every row is inside, many ON a limit)
    sure = ref["admissible"] & ~ref["near"] & inside & ~RF.band_of(margins, pos_thr, rot_thr) & conv.numpy()
    solved = sure.reshape(k, m).any(0)
    n_plain, n_refined = int((plain["count"] > 0).sum()), int((refined["count"] > 0).sum())
    print(f"poses with an admissible candidate: {n_plain} without refinement, {n_refined} with; the oracle loop is sure of {int(solved.sum())}")
    assert solved.sum() >= 1
    assert (refined["count"][solved] > 0).all()
    got = torch.from_numpy(refined["q_out"][:, 0, :][solved])
    pe, re = ko.calculate_pose_error(orob, got.double(), poses[solved].double())
    assert bool((pe < pos_thr).all()) and bool((re < rot_thr).all()), (float(pe.max()), float(re.max()))
    assert not ko.calculate_joint_limits_exceeded(got, orob.actuated_joints_limits).any()
    assert ko.capsule_clearance(orob, caps, (), got.double()).numpy().min() >= self_min - WH.BAND
    assert WH.reference(orob, caps, world, got.double())["clearance"].min() >= world_min - WH.BAND
    assert n_plain < n_refined


# ---- 6. status codes and the Python wrappers -------------------------------------------------------------------------------------------------------------
def test_status_codes_and_messages():
    eng = _touch(_eng("panda"))
    lib = eng.lib
    case = RF.oracle_case("panda", 100, 6, 1e-3, 0.1)
    poses, seeds = case["poses"], case["seeds"]
    nan, inf = float("nan"), float("inf")
    for kw, msg in ((dict(n_steps=0), "n_steps must be in 1 .. 16"), (dict(n_steps=17), "n_steps must be in 1 .. 16"), (dict(n_steps=-1), "n_steps must be in 1 .. 16"),
                    (dict(pos_tol=-1e-9), "pos_tol must be finite and >= 0"), (dict(pos_tol=nan), "pos_tol must be finite and >= 0"),
                    (dict(pos_tol=inf), "pos_tol must be finite and >= 0"), (dict(rot_tol=-0.1), "rot_tol must be finite and >= 0"),
                    (dict(rot_tol=nan), "rot_tol must be finite and >= 0"), (dict(rot_tol=inf), "rot_tol must be finite and >= 0")):
        a = dict(n_steps=4, pos_tol=1e-3, rot_tol=0.1)
        a.update(kw)
        _refine(eng, poses, seeds, 6, a["n_steps"], a["pos_tol"], a["rot_tol"], expect=_lib.IKF_ERR_BAD_ARGUMENT)   # (and wrote nothing)
        assert "ikf_refine_candidates: " + msg in _lib.last_error(lib)
    _refine(eng, poses, seeds, 0, 4, 1e-3, 0.1, expect=_lib.IKF_ERR_BAD_ARGUMENT)
    assert "k must be >= 1" in _lib.last_error(lib)
    _refine(eng, poses, seeds, 6, 4, 1e-3, 0.1, n_poses=-1, expect=_lib.IKF_ERR_BAD_ARGUMENT)
    assert "n_poses must be >= 0" in _lib.last_error(lib)
    _refine(eng, poses, seeds, 6, 4, 1e-3, 0.1, n_poses=0)                       # nothing to do: nothing written
    assert lib.ikf_refine_candidates(eng._h, None, 0, 6, None, 4, 1e-3, 0.1, None, None, None, None) == _lib.IKF_OK
    assert lib.ikf_refine_candidates(eng._h, None, 2 ** 31, 1, None, 4, 1e-3, 0.1, None, None, None, None) == _lib.IKF_ERR_BAD_ARGUMENT
    assert "k * n_poses must be at most 2^31 - 1" in _lib.last_error(lib)
    assert lib.ikf_refine_candidates(eng._h, None, 2 ** 30, 2, None, 4, 1e-3, 0.1, None, None, None, None) == _lib.IKF_ERR_BAD_ARGUMENT
    pd, qd = poses.to(DEV), seeds.to(DEV)
    out = torch.zeros_like(qd)
    for args in ((None, qd.data_ptr(), out.data_ptr()), (pd.data_ptr(), None, out.data_ptr()), (pd.data_ptr(), qd.data_ptr(), None)):
        assert lib.ikf_refine_candidates(eng._h, args[0], 100, 6, args[1], 4, 1e-3, 0.1, args[2], None, None, None) == _lib.IKF_ERR_NULL_POINTER
        assert "ikf_refine_candidates: null device pointer" in _lib.last_error(lib)
    assert lib.ikf_refine_candidates(None, pd.data_ptr(), 100, 6, qd.data_ptr(), 4, 1e-3, 0.1, out.data_ptr(), None, None, None) == _lib.IKF_ERR_NULL_POINTER
    torch.cuda.synchronize()
    assert bool((out == 0).all())
    # ikf_set_candidate_refine: every message; a refused call keeps the previous state; 0 steps drops the tolerances
    assert eng.candidate_refine() == (0, 0.0, 0.0)
    eng.set_candidate_refine(5, 2e-3, 0.25)
    for a, msg in (((-1, 1e-3, 0.1), "n_steps must be in 0 .. 16"), ((17, 1e-3, 0.1), "n_steps must be in 0 .. 16"),
                   ((4, -1.0, 0.1), "pos_tol must be finite and >= 0"), ((4, nan, 0.1), "pos_tol must be finite and >= 0"), ((4, inf, 0.1), "pos_tol must be finite and >= 0"),
                   ((4, 1e-3, -1.0), "rot_tol must be finite and >= 0"), ((4, 1e-3, nan), "rot_tol must be finite and >= 0"), ((4, 1e-3, inf), "rot_tol must be finite and >= 0"),
                   ((0, -1.0, 0.1), "pos_tol must be finite and >= 0")):
        assert lib.ikf_set_candidate_refine(eng._h, *a) == _lib.IKF_ERR_BAD_ARGUMENT and "ikf_set_candidate_refine: " + msg in _lib.last_error(lib)
        assert eng.candidate_refine() == (5, float(np.float32(2e-3)), 0.25)
    assert lib.ikf_get_candidate_refine(eng._h, None, None) == 5
    eng.set_candidate_refine(16)
    assert eng.candidate_refine() == (16, 0.0, 0.0)
    eng.set_candidate_refine(0, 1.0, 1.0)
    assert eng.candidate_refine() == (0, 0.0, 0.0)


def test_python_wrappers():
    from ikflow_amd.ikflow_solver import IKFlowSolver

    # Engine.refine_candidates == ikf_refine_candidates
    eng = _touch(_eng("panda"))
    case = RF.oracle_case("panda", 100, 6, 1e-3, 0.1)
    raw = _refine(eng, case["poses"], case["seeds"], 6, RF.N_STEPS, 1e-3, 0.1)
    q, steps, conv = eng.refine_candidates(case["poses"].to(DEV), 6, case["seeds"].to(DEV), RF.N_STEPS, 1e-3, 0.1, return_info=True)
    assert steps.dtype == torch.uint8 and conv.dtype == torch.bool and q.dtype == torch.float32
    assert H.same_bits(q.cpu().numpy(), raw["q"]) and np.array_equal(steps.cpu().numpy(), raw["steps"]) and np.array_equal(conv.cpu().numpy(), raw["converged"] == 1)
    only = eng.refine_candidates(case["poses"].to(DEV), 6, case["seeds"].to(DEV), RF.N_STEPS, 1e-3, 0.1)
    assert isinstance(only, torch.Tensor) and torch.equal(only, q)
    full = eng.refine_candidates(case["poses"].to(DEV), 6, case["seeds"].to(DEV), 2)            # tolerances default to 0: every step runs
    assert H.same_bits(full.cpu().numpy(), _refine(eng, case["poses"], case["seeds"], 6, 2, 0.0, 0.0)["q"])
    # IKFlowSolver.set_candidate_refine reaches the solver's handle, every engine it creates later, and the three generate_* methods
    robot, hp, lay, sd = H.tiny_model()
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    s.set_candidate_refine(3)                                                                   # before any engine exists
    first = s.engine(DEV)
    assert first.candidate_refine() == (3, float(np.float32(1e-3)), float(np.float32(0.1)))
    s.set_candidate_refine(2, 5e-4, 0.05)
    assert first.candidate_refine() == (2, float(np.float32(5e-4)), float(np.float32(0.05)))
    s._engine = None                                                                            # the next call builds a new handle: the state follows
    second = s.engine(DEV)
    assert second is not first and second.candidate_refine() == first.candidate_refine()
    if torch.cuda.device_count() > 1:                                                           # ... on another device too
        far = s.engine("cuda:1")
        assert far.device.index == 1 and far.candidate_refine() == first.candidate_refine()
        second = s.engine(DEV)
        assert second.candidate_refine() == first.candidate_refine()
    m, k = 9, 12
    y = H.reachable_poses(robot, m, 31)[1].float().to(DEV)
    L = H.latents(k * m, lay.dim, 32).to(DEV)
    rows = second.refine_candidates(y, k, second.generate_approx(y.repeat((k, 1)), L, True), 2, 5e-4, 0.05)
    ranked = s.generate_ranked_ik_solutions(y, k, 2, latent=L, return_row_scores=True)
    ref = second.rank_candidates(y, k, rows, second.rank_options(2, rot_weight=0.01), row_scores=True)
    assert torch.equal(ranked.solutions, ref[0]) and torch.equal(ranked.row_scores, ref[4]) and torch.equal(ranked.repeat_index, ref[2])
    div = s.generate_diverse_ik_solutions(y, k, 3, latent=L, return_row_scores=True)
    assert torch.equal(div.row_scores, ref[4])
    path = s.generate_ik_path(y, k, latent=L, shared_latent=False, return_node_costs=True)
    assert torch.equal(path.node_costs, ref[4])
    s.set_candidate_refine(0)
    assert second.candidate_refine() == (0, 0.0, 0.0)
    off = s.generate_ranked_ik_solutions(y, k, 2, latent=L, return_row_scores=True)
    assert not torch.equal(off.row_scores, ranked.row_scores)
    with pytest.raises(AssertionError, match="n_steps must be an int in 0 .. 16"):
        s.set_candidate_refine(17)
