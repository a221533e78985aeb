"""Path IK for P paths per call on the GPU (include/ikflow_amd_path_batch.h; the BATCH forms of k_path_lattice and k_sweep_edges, path_batch_math.h,
api_path.hip): by definition path p of a batch is what ikf_path_search returns for its own lattice, so every test holds the batch against P single
calls - path, index, cost, reach and node costs, bit for bit - and, where a reference exists, against sequential numpy float32 on the engine's node
costs (tests/path_helpers.py).  Per-path starts, the boundary between two paths, independence and permutation, what is set on the handle, the sweep,
the flow in front, status codes, the reservation and IKFlowSolver.generate_ik_paths.

Every call goes through _bpath(): outputs are windows inside sentinel-filled buffers with guard rows in front and behind, as in tests/test_path.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H
import manip_helpers as MH
import path_batch_helpers as PB
import path_helpers as PH
import rank_helpers as RH
import sweep_helpers as SH
import world_helpers as WH
from ikflow_amd import _lib
from test_path import OUTPUTS, _check_against_dp, _check_nodes_are_rank_scores, _inputs, _path, _popt
from test_ranked import DEV, GUARD, _check_window, _eng, _solver, _window
from test_world import _USED, _eng as _eng_rules

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _nothing_left_on_the_shared_handles():
    yield
    for eng in _USED:   # (the engines are shared with the other test modules)
        eng.set_path_sweep(0)
        eng.clear_world()
        eng.clear_world_track()
        eng.set_min_manipulability(0.0)


def _bpath(eng, poses, q, P, T, k, opt, q_start=None, stream=None, null=(), latent=None, shared=True, clamp=True):
    """ikf_path_search_batch (or, with `latent`, ikf_generate_path_batch) through eng.lib on guarded buffers -> {name: cpu numpy window}."""
    n, nd = P * T, eng.layout.ndof
    shapes = {"path": (n, nd, torch.float32), "index": (n, 1, torch.int32), "cost": (P, 1, torch.float32), "reach": (n, 1, torch.int32),
              "node": (k * n, 1, torch.float32)}
    bufs = {o: _window(*shapes[o]) for o in OUTPUTS if o not in null}
    ptr = [bufs[o][GUARD:].data_ptr() if o in bufs else None for o in OUTPUTS]
    poses_d = poses.to(DEV).contiguous()
    rows_d = (q if latent is None else latent).to(DEV).contiguous()
    start_d = None if q_start is None else q_start.to(DEV).contiguous()
    sp = None if start_d is None else start_d.data_ptr()
    torch.cuda.synchronize()
    s = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(0)
    if latent is None:
        code = eng.lib.ikf_path_search_batch(eng._h, poses_d.data_ptr(), P, T, k, rows_d.data_ptr(), sp, C.byref(opt), *ptr, s)
    else:
        code = eng.lib.ikf_generate_path_batch(eng._h, poses_d.data_ptr(), P, T, k, rows_d.data_ptr(), int(shared), int(clamp), sp, C.byref(opt), *ptr, s)
    assert code == _lib.IKF_OK, (code, _lib.last_error(eng.lib))
    torch.cuda.synchronize()
    out = {o: _check_window(b, shapes[o][0], o).cpu().numpy() for o, b in bufs.items()}
    return {o: (v if o == "path" else v.reshape(-1)) for o, v in out.items()}


def _singles(eng, poses, q, P, T, k, opt, q_start=None):
    """The P single ikf_path_search calls of the definition: path p's rows gathered into its own tile-major lattice, its own start."""
    qn = q.numpy()
    return [_path(eng, poses[p * T:(p + 1) * T], torch.tensor(PB.from_batch(qn, P, T, k, p)), k, opt, None if q_start is None else q_start[p])
            for p in range(P)]


def _assert_batch_is_the_singles(out, singles, P, T, k, what=""):
    for p, (got, want) in enumerate(zip(PB.split(out, P, T, k), singles)):
        for o in want:
            assert PH.same_bits(got[o], want[o]), f"{what}: {o} of path {p} differs from the single call's"


def _batch_inputs(which, P, T, k, seed=0, wild=False):
    """P lattices of tests/test_path.py's _inputs (one seed each) in the batch layout -> (poses [P * T x 7], q [k * P * T x nd], truths [P][T x nd])."""
    orob = H.kin_robots(which)[1]
    parts = [_inputs(orob, T, k, seed=1000 * seed + 100 * p + T + k, wild=wild) for p in range(P)]
    return torch.cat([x[0] for x in parts]).contiguous(), PB.to_batch([x[1] for x in parts], k), [x[2] for x in parts]


# ---- 1. the batch equals P single calls and the numpy lattice of every path ---------------------------------------------------------------------------
SHAPES = {
    "P1_T1_k1": (1, 1, 1, "panda"),
    "P3_T1_k5": (3, 1, 5, "panda"),
    "P3_T3_k5": (3, 3, 5, "panda"),          # T * k = 15: the back-pointer blocks need their padded stride
    "P2_T2_k17": (2, 2, 17, "panda"),
    "P5_T3_k64": (5, 3, 64, "panda"),
    "P2_T5_k129": (2, 5, 129, "panda"),
    "P4_T65_k33": (4, 65, 33, "panda"),      # crosses the 64-waypoint chunk of the walk back; an odd T for the two-waypoint stage
    "P2_T66_k256": (2, 66, 256, "panda"),
    "P300_T4_k6": (300, 4, 6, "panda"),      # more paths than the device has CUs
    "ndof4": (4, 65, 33, "syn4p"),           # k_path_lattice<4 .. 8, false, true>
    "ndof5": (4, 65, 33, "syn5p"),
    "ndof6": (4, 65, 33, "syn6r"),
    "ndof8": (4, 65, 33, "fetch"),
}


@pytest.mark.parametrize("case", list(SHAPES))
def test_batch_equals_the_single_calls_and_the_numpy_lattice_of_every_path(case):
    P, T, k, which = SHAPES[case]
    eng = _eng(which)
    poses, q, _ = _batch_inputs(which, P, T, k)
    opt = _popt()
    out = _bpath(eng, poses, q, P, T, k, opt)
    assert np.isfinite(out["node"]).all() and np.isfinite(out["cost"]).all() and (out["index"] >= 0).all()
    _assert_batch_is_the_singles(out, _singles(eng, poses, q, P, T, k, opt), P, T, k, case)
    qn = q.numpy()
    for p, one in enumerate(PB.split(out, P, T, k)):
        if p < 8 or p >= P - 2:   # (the numpy lattice of the first and the last paths; every path is held against its single call above)
            _check_against_dp(one, torch.tensor(PB.from_batch(qn, P, T, k, p)), T, k, opt, what=f"{case} path {p}")
    if case == "P4_T65_k33":
        _check_nodes_are_rank_scores(eng, out, poses, q, k, opt)   # the candidate stage on P * T poses: the ranking's row scores of the same rows


# ---- 2. a start per path ---------------------------------------------------------------------------------------------------------------------------------
def _start_case():
    """P = 3 copies of ONE lattice (T = 3, k = 5); path p starts exactly on candidate (p + 1) % 3 of waypoint 0.  node_weight = 0: the lattice is
    then a function of the rows alone, so the numpy reference needs no node costs from the engine."""
    P, T, k = 3, 3, 5
    orob = H.kin_robots("panda")[1]
    poses1, q1, _ = _inputs(orob, T, k, seed=T + k)
    starts = torch.stack([q1.reshape(k, T, -1)[(p + 1) % 3, 0] for p in range(P)]).contiguous()
    return P, T, k, poses1.repeat((P, 1)).contiguous(), PB.to_batch([q1] * P, k), q1, starts


def test_every_path_starts_from_its_own_q_start():
    P, T, k, poses, q, q1, starts = _start_case()
    opt = _popt(node_weight=0.0)
    zeros = np.zeros(k * T, np.float32)
    want = [PH.dp_f32(q1.numpy(), zeros, T, k, starts[p].numpy(), 0.0, None)[1] for p in range(P)]
    for p in range(P):   # by the numpy reference alone: another path's start gives path p another index
        for other in range(P):
            if other != p:
                assert not np.array_equal(want[p], want[other]), f"the starts of paths {p} and {other} give the same index: the case tests nothing"
    eng = _eng("panda")
    out = _bpath(eng, poses, q, P, T, k, opt, starts)
    assert np.isfinite(out["node"]).all()
    for p, one in enumerate(PB.split(out, P, T, k)):
        assert np.array_equal(one["index"], want[p]), (p, one["index"], want[p])
        _check_against_dp(one, q1, T, k, opt, starts[p], what=f"start of path {p}")
    _assert_batch_is_the_singles(out, _singles(eng, poses, q, P, T, k, opt, starts), P, T, k, "q_start")


# ---- 3. no edge across the boundary between two paths ------------------------------------------------------------------------------------------------------
BOUNDARY_STEP = 0.25


def test_no_edge_joins_the_end_of_a_path_to_the_start_of_the_next():
    """Three paths from seeds far apart in joint space under a step gate every path passes on its own.  The batch layout read as ONE lattice of P * T
    waypoints - what a search that took p * T for an interior waypoint would see - has no path, by the numpy reference; the batch has one per p."""
    P, T, k = 3, 3, 5
    eng = _eng("panda")
    poses, q, truths = _batch_inputs("panda", P, T, k, seed=3)
    opt = _popt(max_step=BOUNDARY_STEP)
    for p in range(P - 1):
        assert float((truths[p + 1][0] - truths[p][-1]).abs().max()) > 4 * BOUNDARY_STEP
    out = _bpath(eng, poses, q, P, T, k, opt)
    assert np.isfinite(out["node"]).all()
    joined = PH.dp_f32(q.numpy(), out["node"], P * T, k, None, opt.node_weight, opt.max_joint_step)
    assert np.isposinf(joined[2]) and (joined[1] == -1).all() and joined[3][T - 1] > 0 and (joined[3][T:] == 0).all()
    qn = q.numpy()
    for p, one in enumerate(PB.split(out, P, T, k)):
        index = _check_against_dp(one, torch.tensor(PB.from_batch(qn, P, T, k, p)), T, k, opt, what=f"boundary path {p}")
        assert (index >= 0).all() and np.isfinite(one["cost"][0]) and (one["reach"] > 0).all()


# ---- 4. independence ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["nan_column", "step_gate"])
def test_an_impossible_path_in_the_middle_changes_nothing_around_it(how):
    P, T, k = 3, 5, 6
    eng = _eng("panda")
    poses, q, _ = _batch_inputs("panda", P, T, k, seed=4)
    g = q.reshape(k, P, T, -1).clone()
    if how == "nan_column":
        g[:, 1, 2] = float("nan")       # every candidate of waypoint 2 of path 1
        opt, first_dead = _popt(), 2
    else:
        g[:, 1, 3:] += 1.0              # path 1 jumps by 1 rad on every joint between waypoints 2 and 3
        opt, first_dead = _popt(max_step=0.5), 3
    q = g.reshape(k * P * T, -1).contiguous()
    out = _bpath(eng, poses, q, P, T, k, opt)
    parts = PB.split(out, P, T, k)
    mid = parts[1]
    assert (mid["path"] == 0).all() and (mid["index"] == -1).all() and np.isposinf(mid["cost"][0])
    assert (mid["reach"][:first_dead] > 0).all() and (mid["reach"][first_dead:] == 0).all(), mid["reach"]
    singles = _singles(eng, poses, q, P, T, k, opt)
    _assert_batch_is_the_singles(out, singles, P, T, k, how)
    qn = q.numpy()
    for p in (0, 2):
        index = _check_against_dp(parts[p], torch.tensor(PB.from_batch(qn, P, T, k, p)), T, k, opt, what=f"{how} neighbour {p}")
        assert (index >= 0).all() and np.isfinite(parts[p]["cost"][0])
    # permuting the paths permutes the outputs
    perm = [2, 0, 1]
    gp = q.reshape(k, P, T, -1)[:, perm].reshape(k * P * T, -1).contiguous()
    pp = poses.reshape(P, T, 7)[perm].reshape(P * T, 7).contiguous()
    moved = PB.split(_bpath(eng, pp, gp, P, T, k, opt), P, T, k)
    for i, p in enumerate(perm):
        assert all(PH.same_bits(moved[i][o], parts[p][o]) for o in OUTPUTS), f"{how}: path {p} moved to slot {i} changed"


# ---- 5. what is set on the handle -------------------------------------------------------------------------------------------------------------------------------
def test_thresholds_limits_a_world_and_a_manipulability_floor_are_obeyed_per_path():
    """wild rows under pose-error thresholds and the joint limits, the mixed7 world at the median of the rows' reference clearances and a floor at the
    median of their reference manipulability: each rule drops rows, some rows stay, and the batch equals the P single calls on the same handle."""
    P, T, k, which = 3, 9, 17, "panda"
    eng = _eng_rules(which)
    robot, orob = H.kin_robots(which)
    poses, q, _ = _batch_inputs(which, P, T, k, seed=5, wild=True)
    world = WH.scene(which, "mixed7")
    eng.set_world(world, WH.threshold(WH.reference(orob, RH.collision_capsules(robot), world, q)["clearance"]))
    eng.set_min_manipulability(float(np.median(MH.w_ref(MH.table_rows(robot), q.numpy(), "full"))), "full")
    opt = _popt(max_pos=0.2, max_rot=1.0, limits=True)
    out = _bpath(eng, poses, q, P, T, k, opt)
    n_bad = int(np.isinf(out["node"]).sum())
    print(f"rules: {n_bad} of {k * P * T} rows inadmissible, costs {out['cost']}")
    assert 0 < n_bad < k * P * T
    _assert_batch_is_the_singles(out, _singles(eng, poses, q, P, T, k, opt), P, T, k, "rules")
    eng.set_min_manipulability(0.0)
    eng.clear_world()
    plain = _bpath(eng, poses, q, P, T, k, opt)
    assert 0 < int(np.isinf(plain["node"]).sum()) < n_bad   # (thresholds and limits alone drop fewer rows: the world and the floor do something)


# ---- 6. the sweep ---------------------------------------------------------------------------------------------------------------------------------------------------
SWEEP_CASES = [(P, T, k, S, ws) for (P, T, k) in ((3, 5, 6), (2, 9, 65)) for S in (1, 4) for ws in (False, True)]


@pytest.mark.parametrize("P,T,k,S,with_start", SWEEP_CASES)
def test_swept_batch_equals_the_swept_single_calls(P, T, k, S, with_start):
    """World and self rule, S samples per edge, with and without a start per path.  The inputs are those of path_batch_helpers.sweep_case, whose
    condition - no unpruned edge of any of the P lattices and no live node within sweep_helpers.BAND of a threshold, by the fp64 reference - is
    asserted first, on the reference alone; under it the BATCH and the single form of the sweep kernel must reach the same verdict on every edge a
    search can take."""
    c = PB.sweep_case(P, T, k, S, with_start)
    print(f"sweep {P, T, k, S, with_start}: per lattice (unpruned, blocked, free, band) {c['counts']}, gaps {c['gaps']}, thresholds {c['world_thr']:.5f} {c['self_thr']:.5f}")
    assert all(band == 0 for _, _, _, band in c["counts"]) and c["node_band"] == 0, "an unpruned edge or a live node lies in the band: another seed"
    assert PB.sweep_condition_holds(c), "the batch holds no surely blocked or no surely free unpruned edge: another seed"
    eng = _eng_rules(PB.SWEEP_WHICH)
    eng.set_world(c["world"], c["world_thr"])
    eng.set_path_sweep(S)
    opt = _popt(collisions=True, min_clearance=c["self_thr"], max_step=c["gate"])
    out = _bpath(eng, c["poses"], c["q"], P, T, k, opt, c["q_start"])
    _assert_batch_is_the_singles(out, _singles(eng, c["poses"], c["q"], P, T, k, opt, c["q_start"]), P, T, k, "sweep")
    eng.set_path_sweep(0)
    unswept = _bpath(eng, c["poses"], c["q"], P, T, k, opt, c["q_start"])
    assert PH.same_bits(unswept["node"], out["node"])
    changed = [p for p in range(P) if not np.array_equal(out["index"][p * T:(p + 1) * T], unswept["index"][p * T:(p + 1) * T])]
    print(f"sweep {P, T, k, S, with_start}: the sweep changes the index of paths {changed}; costs {out['cost']} against {unswept['cost']} unswept")
    assert (out["cost"] >= unswept["cost"]).all()


def test_the_sweep_changes_a_path_of_the_batch():
    """Two (65, 33) lattices of tests/sweep_helpers.py in one batch under the first one's world - the lattice and the seed for which the single
    call's swept path differs from its unswept path (tests/test_sweep.py): in the batch the sweep changes that path's index too, and costs more."""
    P, T, k, S = 2, 65, 33, 4
    first = SH.lattice_inputs("panda", T, k, SH.LATTICE_SEEDS[("panda", T, k)])
    second = SH.lattice_inputs("panda", T, k, 2)
    eng = _eng_rules("panda")
    eng.set_world(first["world"], first["world_thr"])
    poses = torch.cat([first["poses"], second["poses"]]).contiguous()
    q = PB.to_batch([first["q"], second["q"]], k)
    opt = _popt()
    unswept = _bpath(eng, poses, q, P, T, k, opt)
    eng.set_path_sweep(S)
    swept = _bpath(eng, poses, q, P, T, k, opt)
    assert PH.same_bits(unswept["node"], swept["node"])
    changed = [p for p in range(P) if not np.array_equal(swept["index"][p * T:(p + 1) * T], unswept["index"][p * T:(p + 1) * T])]
    print(f"the sweep changes the index of paths {changed}; costs {swept['cost']} against {unswept['cost']} unswept")
    assert 0 in changed and np.isfinite(swept["cost"][0]) and swept["cost"][0] > unswept["cost"][0]
    assert (swept["cost"] >= unswept["cost"]).all() and (swept["reach"] <= unswept["reach"]).all()


# ---- 7. the flow in front ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [0, 2])
@pytest.mark.parametrize("P,T,k", [(3, 33, 20), (2, 5, 256)])
def test_generate_batch_equals_the_flow_then_the_batched_search(P, T, k, refine):
    """ikf_generate_path_batch with k shared latents == the same call with the latent expanded to [k * P * T x D] == the flow on the repeated
    waypoints in one call of the same row count (under ikf_set_candidate_refine: followed by ikf_refine_candidates) and ikf_path_search_batch on its
    rows == the P single ikf_path_search calls on those rows; node costs are ikf_rank_candidates' row scores of those rows."""
    s, robot, lay, sd = _solver("tiny")
    eng = s.engine(DEV)
    n = P * T
    _, poses = H.reachable_poses(robot, n, 41)
    poses = poses.float()
    L = H.latents(k, lay.dim, 42)
    expanded = L[:, None, :].expand(k, n, lay.dim).reshape(k * n, lay.dim).contiguous()
    opt = _popt(limits=True, max_step=3.0)
    starts = torch.zeros(P, robot.ndof)
    try:
        eng.set_candidate_refine(refine)
        shared = _bpath(eng, poses, None, P, T, k, opt, starts, latent=L, shared=True)
        explicit = _bpath(eng, poses, None, P, T, k, opt, starts, latent=expanded, shared=False)
        assert all(PH.same_bits(shared[o], explicit[o]) for o in OUTPUTS)
        rows = s.generate_ik_solutions(poses.to(DEV).repeat((k, 1)), latent=expanded.to(DEV))
        if refine:
            rows = eng.refine_candidates(poses.to(DEV), k, rows, refine)
        rows = rows.cpu()
        two_step = _bpath(eng, poses, rows, P, T, k, opt, starts)
        assert all(PH.same_bits(shared[o], two_step[o]) for o in OUTPUTS)
        _assert_batch_is_the_singles(shared, _singles(eng, poses, rows, P, T, k, opt, starts), P, T, k, f"generate refine {refine}")
        _check_nodes_are_rank_scores(eng, shared, poses, rows, k, opt)
        if not refine:
            other = _bpath(eng, poses, None, P, T, k, opt, starts, latent=H.latents(k * n, lay.dim, 43), shared=False)   # a latent per node: another lattice
            assert not PH.same_bits(other["node"], shared["node"])
    finally:
        eng.set_candidate_refine(0)


# ---- 8. status codes, untouched outputs, null outputs, another stream -----------------------------------------------------------------------------------------------
def test_status_codes_and_untouched_outputs():
    from ikflow_amd.engine import Engine
    from ikflow_amd.world import World

    eng = _eng_rules("panda")
    lib, h = eng.lib, eng._h
    P, T, k = 3, 4, 5
    poses, q, _ = _batch_inputs("panda", P, T, k, seed=8)
    Y, Q = poses.to(DEV), q.to(DEV)
    path = torch.full((P * T, 7), 7.0, device=DEV)
    index = torch.full((P * T,), 7, dtype=torch.int32, device=DEV)
    cost = torch.full((P,), 7.0, device=DEV)
    opt = _popt()
    call = lambda h_, y, p_, t_, k_, q_, o, po, io, co: lib.ikf_path_search_batch(h_, y, p_, t_, k_, q_, None, o, po, io, co, None, None, None)
    ok = (h, Y.data_ptr(), P, T, k, Q.data_ptr(), C.byref(opt), path.data_ptr(), index.data_ptr(), cost.data_ptr())
    bad = [
        ((None,) + ok[1:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:1] + (None,) + ok[2:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:5] + (None,) + ok[6:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:6] + (None,) + ok[7:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:7] + (None,) + ok[8:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:8] + (None,) + ok[9:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:9] + (None,), _lib.IKF_ERR_NULL_POINTER),
        (ok[:2] + (-1,) + ok[3:], _lib.IKF_ERR_BAD_ARGUMENT),                                # P < 0
        (ok[:3] + (-1,) + ok[4:], _lib.IKF_ERR_BAD_ARGUMENT),                                # T < 0
        (ok[:2] + (-1, 0) + ok[4:], _lib.IKF_ERR_BAD_ARGUMENT),                              # (a negative count is refused before the empty call is seen)
        (ok[:4] + (0,) + ok[5:], _lib.IKF_ERR_BAD_ARGUMENT),
        (ok[:4] + (257,) + ok[5:], _lib.IKF_ERR_BAD_ARGUMENT),
        (ok[:2] + (2 ** 12, 2 ** 11, 256) + ok[5:], _lib.IKF_ERR_BAD_ARGUMENT),              # k * P * T = 2^31
        (ok[:2] + (2 ** 40, 2 ** 40, 1) + ok[5:], _lib.IKF_ERR_BAD_ARGUMENT),                # (P * T itself beyond int64's comfort)
        (ok[:6] + (C.byref(_popt(node_weight=-1.0)),) + ok[7:], _lib.IKF_ERR_BAD_ARGUMENT),
    ]
    for args, code in bad:
        assert call(*args) == code, (args, code, _lib.last_error(lib))
    fresh = Engine(eng.layout, eng.robot, DEV)                                               # (no collision model, no weights)
    assert call(fresh._h, *ok[1:6], C.byref(_popt(collisions=True)), *ok[7:]) == _lib.IKF_ERR_BAD_ARGUMENT
    assert "reject_collisions without a collision model" in _lib.last_error(lib)
    lat = torch.zeros(k, eng.layout.dim, device=DEV)
    gen = lambda h_: lib.ikf_generate_path_batch(h_, Y.data_ptr(), P, T, k, lat.data_ptr(), 1, 1, None, C.byref(opt), path.data_ptr(), index.data_ptr(),
                                                 cost.data_ptr(), None, None, None)
    assert gen(fresh._h) == _lib.IKF_ERR_NOT_LOADED and gen(None) == _lib.IKF_ERR_NULL_POINTER
    # a world track: both entries refuse, and say why
    frames = []
    for t in range(T):
        w = World()
        w.add_sphere((0.4 + 0.01 * t, 0.0, 0.5), 0.05)
        frames.append(w)
    eng.set_world_track(frames, 0.0)
    assert call(*ok) == _lib.IKF_ERR_BAD_ARGUMENT and "world track" in _lib.last_error(lib)
    s, _, lay, _ = _solver("tiny")
    trobot = H.tiny_model()[0]   # (a robot of this test's own: a track needs a capsule model, which must not reach the solvers other modules share)
    trobot.set_collision_capsules(RH.collision_capsules(trobot))
    seng = Engine(s.layout, trobot, DEV)
    seng.load_state_dict(s._state_dict_np)
    seng.set_collision_model(*trobot._collision_model)
    seng.set_world_track(frames, 0.0)
    lat2 = torch.zeros(k, lay.dim, device=DEV)
    code = seng.lib.ikf_generate_path_batch(seng._h, Y.data_ptr(), P, T, k, lat2.data_ptr(), 1, 1, None, C.byref(opt), path.data_ptr(), index.data_ptr(),
                                            cost.data_ptr(), None, None, None)
    seng.clear_world_track()
    assert code == _lib.IKF_ERR_BAD_ARGUMENT and "world track" in _lib.last_error(seng.lib)
    assert call(h, None, 0, T, k, None, C.byref(opt), None, None, None) == _lib.IKF_OK      # nothing to do, even under the track: null buffers are fine
    eng.clear_world_track()
    # P = 0 and T = 0: IKF_OK, nothing written
    assert call(ok[0], ok[1], 0, T, *ok[4:]) == _lib.IKF_OK and call(ok[0], ok[1], P, 0, *ok[4:]) == _lib.IKF_OK
    assert call(h, None, P, 0, k, None, C.byref(opt), None, None, None) == _lib.IKF_OK
    for args in ((None, 4, 4, 4), (fresh._h, 0, 4, 4), (fresh._h, 4, 0, 4), (fresh._h, 4, 4, 0), (fresh._h, 4, 4, 257), (fresh._h, -1, 4, 4),
                 (fresh._h, 2 ** 12, 2 ** 11, 256)):
        assert lib.ikf_reserve_path_batch(*args) == (_lib.IKF_ERR_NULL_POINTER if args[0] is None else _lib.IKF_ERR_BAD_ARGUMENT), args
    assert lib.ikf_reserve_path_batch(fresh._h, 10, 10, 50) == _lib.IKF_OK
    torch.cuda.synchronize()
    assert (path == 7.0).all() and (index == 7).all() and (cost == 7.0).all()                # none of these calls touched an output
    assert call(*ok) == _lib.IKF_OK
    torch.cuda.synchronize()
    assert (index >= 0).all() and (index < k).all() and torch.isfinite(cost).all()


def test_null_optional_outputs_and_another_stream():
    P, T, k = 3, 20, 7
    eng = _eng("panda")
    poses, q, truths = _batch_inputs("panda", P, T, k, seed=9)
    starts = torch.stack([t[0] + 0.05 for t in truths]).contiguous()
    ref = _bpath(eng, poses, q, P, T, k, _popt(), starts)
    for null in (("reach",), ("node",), ("reach", "node")):
        got = _bpath(eng, poses, q, P, T, k, _popt(), starts, null=null)
        assert set(got) == set(OUTPUTS) - set(null) and all(PH.same_bits(ref[o], got[o]) for o in got)
    again = _bpath(eng, poses, q, P, T, k, _popt(), starts, stream=torch.cuda.Stream(device=DEV))
    assert all(PH.same_bits(ref[o], again[o]) for o in OUTPUTS)


# ---- 9. ikf_reserve_path_batch ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweep", [0, 2])
def test_after_reserve_path_batch_a_call_of_that_size_allocates_nothing(sweep):
    """The method of tests/test_path.py::test_after_reserve_path_a_call_of_that_size_allocates_nothing: the device's free memory over calls at and
    under the reserved size, in both latent forms, shrinks by no more than torch's own allocator grew; with a world and a sweep set first, the
    mask is part of the reservation.  The reservation changes no result."""
    from ikflow_amd.engine import Engine
    from ikflow_amd.ikflow_solver import IKFlowSolver

    robot, hp, lay, sd = H.tiny_model()   # (a robot of this test's own: the capsule model must not reach the solvers other modules share)
    robot.set_collision_capsules(RH.collision_capsules(robot))
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    P, T, k = 6, 50, 64
    _, poses = H.reachable_poses(robot, P * T, 3)
    poses = poses.float()
    L, Lfull = H.latents(k, lay.dim, 5), H.latents(k * P * T, lay.dim, 6)
    opt = _popt(limits=True)

    def engine():
        eng = Engine(s.layout, robot, DEV)
        eng.load_state_dict(s._state_dict_np)
        eng.set_collision_model(*robot._collision_model)
        if sweep:
            eng.set_world(WH.scene("panda", SH.LATTICE_SCENE), -0.05)
            eng.set_path_sweep(sweep)
        return eng

    def run(eng, pp, tt, kk, shared=True):
        return _bpath(eng, poses[:pp * tt], None, pp, tt, kk, opt, latent=L[:kk] if shared else Lfull[:kk * pp * tt], shared=shared)

    eng = engine()
    eng.reserve_path_batch(P, T, k)
    torch.cuda.synchronize()
    run(eng, 2, 4, 4)                                                  # (torch's caching allocator warm for the test's own buffers)
    torch.cuda.synchronize()
    free0, stat0 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    full = run(eng, P, T, k)
    run(eng, P, T, k, shared=False)
    run(eng, 3, 50, 50)
    run(eng, 6, 1, 64)
    run(eng, 1, 50, 33)
    torch.cuda.synchronize()
    free1, stat1 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    grown_by_torch = stat1 - stat0                                     # (the guarded windows of the larger calls come from torch)
    assert free0 - free1 <= grown_by_torch, f"the engine allocated {free0 - free1 - grown_by_torch} bytes after ikf_reserve_path_batch"
    fresh = engine()
    assert all(PH.same_bits(full[o], v) for o, v in run(fresh, P, T, k).items())   # (the reservation changes no result)


# ---- 10. the Python method ------------------------------------------------------------------------------------------------------------------------------------------
def test_generate_ik_paths_end_to_end():
    s, robot, lay, sd = _solver("tiny")
    eng = s.engine(DEV)
    P, T, k = 3, 11, 20
    _, poses = H.reachable_poses(robot, P * T, 51)
    w = poses.float().reshape(P, T, 7).to(DEV)
    L = H.latents(k, lay.dim, 52).to(DEV)
    got = s.generate_ik_paths(w, k, latent=L, return_node_costs=True)
    assert got._fields == ("paths", "index", "cost", "n_reachable", "node_costs")
    assert got.paths.shape == (P, T, robot.ndof) and got.index.shape == (P, T) and got.index.dtype == torch.int32
    assert got.cost.shape == (P,) and got.n_reachable.shape == (P, T) and got.n_reachable.dtype == torch.int32 and got.node_costs.shape == (k, P, T)
    four = s.generate_ik_paths(w, k, latent=L)
    assert four._fields == ("paths", "index", "cost", "n_reachable") and torch.equal(four.index, got.index) and torch.equal(four.paths, got.paths)
    # the rows the flow writes for these latents and poses, and the numpy lattice of every path on the engine's node costs
    n = P * T
    expanded = L[:, None, :].expand(k, n, lay.dim).reshape(k * n, lay.dim).contiguous()
    rows = s.generate_ik_solutions(w.reshape(n, 7).repeat((k, 1)), latent=expanded).cpu().numpy()
    out = {"path": got.paths.reshape(n, -1).cpu().numpy(), "index": got.index.reshape(-1).cpu().numpy(), "cost": got.cost.cpu().numpy(),
           "reach": got.n_reachable.reshape(-1).cpu().numpy(), "node": got.node_costs.reshape(-1).cpu().numpy()}
    for p, one in enumerate(PB.split(out, P, T, k)):
        index = _check_against_dp(one, torch.tensor(PB.from_batch(rows, P, T, k, p)), T, k, eng.path_options(rot_weight=0.01), what=f"generate_ik_paths {p}")
        assert (index >= 0).all()
    # a start per path; a latent per node is another draw
    starts = got.paths[:, 0].contiguous()
    per_node = s.generate_ik_paths(w, k, latent=H.latents(k * n, lay.dim, 53).to(DEV), shared_latent=False, q_start=starts, max_joint_step=6.0)
    assert per_node.paths.shape == (P, T, robot.ndof)
    with pytest.raises(AssertionError, match=rf"q_start must be \[{P} x {robot.ndof}\]"):
        s.generate_ik_paths(w, k, latent=L, q_start=starts[0])
    torch.manual_seed(77)
    a = s.generate_ik_paths(w, k)
    torch.manual_seed(77)
    b = s.generate_ik_paths(w, k, latent=torch.randn((k, lay.dim), device=DEV))
    assert torch.equal(a.paths, b.paths) and torch.equal(a.cost, b.cost)
    # refine_steps = 2 on the paths that exist; a path that does not exist stays at zeros.  Path 1 is made impossible by a start 10 rad away
    # under a step gate its own waypoints pass.
    gate = 6.0
    far = starts.clone()
    far[1] += 10.0
    mixed = s.generate_ik_paths(w, k, latent=L, q_start=far, max_joint_step=gate)
    refined = s.generate_ik_paths(w, k, latent=L, q_start=far, max_joint_step=gate, refine_steps=2)
    assert torch.isposinf(mixed.cost[1]) and torch.isfinite(mixed.cost[[0, 2]]).all()
    assert (refined.paths[1] == 0).all() and (refined.index[1] == -1).all() and torch.isposinf(refined.cost[1])
    for p in (0, 2):
        want = eng.lm_step(w[p], eng.lm_step(w[p], mixed.paths[p].contiguous()))
        assert torch.equal(refined.paths[p], want)
    assert torch.equal(refined.index, mixed.index) and torch.equal(refined.cost, mixed.cost)
    none = s.generate_ik_paths(w, k, latent=L, pos_error_threshold=0.0, refine_steps=2)
    assert torch.isposinf(none.cost).all() and (none.index == -1).all() and (none.paths == 0).all() and (none.n_reachable == 0).all()
