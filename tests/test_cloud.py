"""World point cloud on the GPU (include/ikflow_amd_cloud.h; ikflow_amd/csrc/cloud_kernels.hip, cloud_math.h, api_cloud.hip, and the cloud test of
k_rank_candidates): ikf_cloud_clearance against the fp64 reference of tests/cloud_helpers.py on guarded buffers, the same bits under every launch
plan, the ranking / path IK / diverse-of-K with a cloud set on the handle, switching it on and off, two handles, status codes, memory.

Tolerances are the project's (world_helpers.py): 2e-5 on a clearance, a band of 1e-4 around min_clearance in which admissibility is not compared,
row scores by rank_helpers.check_row_scores.  The threshold of a case is the median of the reference clearances of its rows;
tests/test_cloud_math_host.py checks on the CPU that this leaves at most 5 % of the rows in the band and at least 20 % on either side."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import cloud_helpers as CH
import helpers as H
import rank_helpers as RH
import world_helpers as WH
from ikflow_amd import _lib
from test_ranked import _check_selection, _eng_with, _opt, _rank, _small_model_back  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
NAN_BITS = 0x7FC00000
BYTE_SENTINEL = 0xAB
R = CH.POINT_RADIUS
_USED = []


def _eng(which):
    """The shared kinematics engine of the chain with the test capsule model (as tests/test_world.py's); its cloud is cleared after every test."""
    from ikflow_amd.engine import kinematics_engine_for

    robot = H.kin_robots(which)[0]
    eng = kinematics_engine_for(robot, DEV)
    robot.set_collision_capsules(RH.collision_capsules(robot))
    eng.set_collision_model(*robot._collision_model)
    eng._collision_source = robot._collision_model
    if eng not in _USED:
        _USED.append(eng)
    return eng


def _eng_model(which, model, used):
    eng = _eng_with(which, model, used)
    if eng not in _USED:
        _USED.append(eng)
    return eng


@pytest.fixture(autouse=True)
def _no_cloud_left_behind():
    yield
    for eng in _USED:
        eng.clear_world_cloud()   # (the engines are shared with the other test modules)
        eng.clear_world()


OUTPUTS = ("clearance", "colliding")


def _clearance(eng, q, null=(), n=None, stream=None, expect=_lib.IKF_OK):
    """ikf_cloud_clearance through eng.lib on guarded buffers -> {name: cpu numpy window}; `null`: the outputs passed as null; n: the row count
    passed (default: all rows of q)."""
    rows = q.shape[0]
    n = rows if n is None else n
    bufs = {}
    if "clearance" not in null:
        bufs["clearance"] = torch.full((rows + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    if "colliding" not in null:
        bufs["colliding"] = torch.full((rows + 2 * GUARD,), BYTE_SENTINEL, dtype=torch.uint8, device=DEV)
    ptr = [bufs[o][GUARD:].data_ptr() if o in bufs else None for o in OUTPUTS]
    qd = q.to(DEV).contiguous()
    torch.cuda.synchronize()
    s = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(0)
    code = eng.lib.ikf_cloud_clearance(eng._h, qd.data_ptr() if rows else None, n, *ptr, s)
    assert code == expect, (code, _lib.last_error(eng.lib))
    torch.cuda.synchronize()
    out = {}
    for o, b in bufs.items():
        untouched = (lambda part: bool((part.view(torch.int32) == NAN_BITS).all())) if o == "clearance" else (lambda part: bool((part == BYTE_SENTINEL).all()))
        assert untouched(b[:GUARD]) and untouched(b[GUARD + max(n, 0):]), f"{o}: an element outside the window was written"
        win = b[GUARD:GUARD + max(n, 0)]
        if n > 0 and expect == _lib.IKF_OK:
            written = ~torch.isnan(win) if o == "clearance" else win != BYTE_SENTINEL
            assert bool(written.all()), f"{o}: an element inside the window was not written"
        out[o] = win.cpu().numpy().copy()
    return out


def _check_against_reference(out, ref, thr, n, what):
    cl = ref[:n]
    err = float(np.abs(out["clearance"].astype(np.float64) - cl).max())
    print(f"{what} n {n}: worst |engine - fp64 reference| {err:.2e}")
    assert err <= CH.CLEARANCE_TOL, (what, n, err)
    decided = np.abs(cl - thr) > CH.BAND
    assert np.array_equal(out["colliding"][decided], (cl < thr)[decided].astype(np.uint8)), what
    assert set(np.unique(out["colliding"])) <= {0, 1}


# ---- 1. ikf_cloud_clearance against the fp64 reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_points", CH.SIZES)
@pytest.mark.parametrize("which", H.KIN_ALL)
def test_cloud_clearance_against_the_fp64_reference(which, n_points):
    """1, 63, 64, 65 and 257 rows (one lane, a tile less one, a tile, a tile and one, five tiles) of every chain against clouds of 1, 511, 512, 513
    and 4097 points (the padding at its longest, absent, and after one point; nine tiles - with few rows a chunk each): clearance within 2e-5,
    flags exact outside the band."""
    eng = _eng(which)
    q, ref, thr = CH.rows_and_reference(which, n_points)
    eng.set_world_cloud(CH.cloud(which, n_points), R, thr)
    assert eng.world_cloud_size == n_points
    for n in (1, 63, 64, 65, 257):
        _check_against_reference(_clearance(eng, q[:n]), ref, thr, n, f"{which} {n_points} points")


# ---- 2. 24 capsules and no capsules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", RH.CASE_CHAINS)
def test_cloud_clearance_with_24_capsules(which, _small_model_back):
    """k_cloud_clearance with the 24-capsule model on chains of 4, 7 and 8 joints: its dynamic LDS at the maximum, 46336 B."""
    eng = _eng_model(which, "caps24", _small_model_back)
    q, ref, thr = CH.rows_and_reference(which, 513, "caps24")
    eng.set_world_cloud(CH.cloud(which, 513, "caps24"), R, thr)
    assert 8192 + 1024 + 4 * 64 * ((6 * 24) | 1) == 46336
    for n in (1, 65, 66):
        _check_against_reference(_clearance(eng, q[:n]), ref, thr, n, f"{which} caps24")


@pytest.mark.parametrize("which", RH.CASE_CHAINS)
def test_cloud_clearance_without_capsules(which, _small_model_back):
    """A model of no capsules (a slice of one float per lane): 3.0e38 and no flag on every row, every element written."""
    eng = _eng_model(which, "caps0", _small_model_back)
    q = CH.rows_and_reference(which, 513)[0]
    for n_points in (513, 4097):
        eng.set_world_cloud(CH.cloud(which, n_points), R, 0.05)
        for n in (1, 64, 130):
            out = _clearance(eng, q[:n])
            assert (out["clearance"] == np.float32(CH.EMPTY)).all() and (out["colliding"] == 0).all()


# ---- 3. the same bits under every plan --------------------------------------------------------------------------------------------------------------
def test_clearance_is_bit_for_bit_the_same_under_every_plan():
    """Panda against 20481 points (41 tiles): 4096 rows in one call (7 chunks of 6 tiles on 256 CUs), the same rows in 64 calls of 64 rows (41
    chunks of one tile) and 32 of them as single rows - the values of a row are bit-equal, and 257 of them within 2e-5 of the reference."""
    which, n_points = "panda", 20481
    eng = _eng(which)
    _, orob = H.kin_robots(which)
    pts = CH.cloud(which, n_points)
    q257, ref, thr = CH.rows_and_reference(which, n_points)
    q = torch.cat([q257, torch.tensor(orob.sample_joint_angles(4096 - 257, 0.0, np.random.default_rng(301))).float()]).contiguous()
    eng.set_world_cloud(pts, R, thr)
    whole = _clearance(eng, q)
    _check_against_reference({k: v[:257] for k, v in whole.items()}, ref, thr, 257, f"{which} {n_points} points")
    qd = q.to(DEV)
    cl = torch.full((4096,), float("nan"), device=DEV)
    col = torch.full((4096,), BYTE_SENTINEL, dtype=torch.uint8, device=DEV)
    for i in range(64):
        a, b = cl[64 * i:], col[64 * i:]
        assert eng.lib.ikf_cloud_clearance(eng._h, qd[64 * i:].data_ptr(), 64, a.data_ptr(), b.data_ptr(), None) == _lib.IKF_OK
    torch.cuda.synchronize()
    assert H.same_bits(cl.cpu().numpy(), whole["clearance"]) and np.array_equal(col.cpu().numpy(), whole["colliding"])
    for i in np.random.default_rng(3).choice(4096, 32, replace=False):
        one = _clearance(eng, q[i:i + 1])
        assert H.same_bits(one["clearance"], whole["clearance"][i:i + 1]) and one["colliding"][0] == whole["colliding"][i]


# ---- 4. outputs, streams, two handles -----------------------------------------------------------------------------------------------------------------
def test_outputs_are_nullable_n_zero_is_a_no_op_and_an_empty_cloud_is_far_away():
    which, n_points = "panda", 4097
    eng = _eng(which)
    q, ref, thr = CH.rows_and_reference(which, n_points)
    eng.set_world_cloud(CH.cloud(which, n_points), R, thr)
    full = _clearance(eng, q[:130])
    for null in [("clearance",), ("colliding",), OUTPUTS]:
        got = _clearance(eng, q[:130], null=null)
        assert set(got) == set(OUTPUTS) - set(null) and all(np.array_equal(got[o].view(np.uint8), full[o].view(np.uint8)) for o in got)
    side = torch.cuda.Stream(device=DEV)
    got = _clearance(eng, q[:130], stream=side)
    assert all(np.array_equal(got[o].view(np.uint8), full[o].view(np.uint8)) for o in OUTPUTS)
    _clearance(eng, q[:130], n=0)                                  # n = 0: nothing is written (every element still carries its sentinel)
    _clearance(eng, q[:0])                                         # ... and null pointers are fine
    _clearance(eng, q[:4], n=-1, expect=_lib.IKF_ERR_BAD_ARGUMENT)
    cl, flag = eng.cloud_clearance(q[:130].to(DEV))
    assert cl.dtype == torch.float32 and flag.dtype == torch.bool and H.same_bits(cl.cpu().numpy(), full["clearance"])
    assert np.array_equal(flag.cpu().numpy(), full["colliding"].astype(bool))
    eng.clear_world_cloud()
    assert eng.world_cloud_size == 0
    empty = _clearance(eng, q[:130])
    assert (empty["clearance"] == np.float32(CH.EMPTY)).all() and (empty["colliding"] == 0).all()
    eng.set_world_cloud(np.zeros((0, 3), np.float32), R, 5.0)     # an empty cloud clears too, whatever its threshold
    assert eng.world_cloud_size == 0 and (_clearance(eng, q[:65])["colliding"] == 0).all()


def test_a_cloud_on_one_handle_does_not_change_another():
    from ikflow_amd.engine import Engine

    which, m, k = "panda", 65, 2
    robot, _ = H.kin_robots(which)
    eng = _eng(which)
    other = Engine(eng.layout, eng.robot, DEV)
    other.set_collision_model(*robot._collision_model)
    poses, q, _, _, _, cl, thr = CH.rank_case(which, m, k)
    opt = _opt(n_keep=2)
    before_a, before_b = _rank(eng, poses, q, k, opt), _rank(other, poses, q, k, opt)
    assert all(H.same_bits(before_a[n], before_b[n]) for n in before_a)
    eng.set_world_cloud(CH.cloud(which, CH.RANK_POINTS), R, thr)
    assert eng.world_cloud_size == CH.RANK_POINTS and other.world_cloud_size == 0
    after_a, after_b = _rank(eng, poses, q, k, opt), _rank(other, poses, q, k, opt)
    assert all(H.same_bits(after_b[n], before_b[n]) for n in before_b)
    assert np.isposinf(after_a["row_score"]).sum() > np.isposinf(before_a["row_score"]).sum()
    assert (_clearance(other, q)["clearance"] == np.float32(CH.EMPTY)).all()


# ---- 5. status codes -------------------------------------------------------------------------------------------------------------------------------
def test_status_codes_name_the_point_and_leave_the_cloud_as_it_was():
    from ikflow_amd.engine import Engine

    eng = _eng("panda")
    lib = eng.lib
    nan, inf = float("nan"), float("inf")

    def put(h, pts, n, radius=0.01, thr=0.0):
        arr = None if pts is None else np.ascontiguousarray(pts, np.float32)
        return lib.ikf_set_world_cloud(h, None if arr is None else arr.ctypes.data, n, radius, thr)

    good = np.array([[5.0, 0.0, 0.0], [5.0, 1.0, 0.0], [5.0, 0.0, 1.0]], np.float32)
    fresh = Engine(eng.layout, eng.robot, DEV)   # no collision model
    assert put(fresh._h, good, 3) == _lib.IKF_ERR_BAD_ARGUMENT and "without a collision model" in _lib.last_error(lib)
    assert put(fresh._h, None, 0) == _lib.IKF_OK   # (clearing needs none)
    q = torch.zeros(4, eng.layout.ndof, device=DEV)
    out = torch.empty(4, device=DEV)
    assert lib.ikf_cloud_clearance(fresh._h, q.data_ptr(), 4, out.data_ptr(), None, None) == _lib.IKF_ERR_BAD_ARGUMENT
    assert "no collision model" in _lib.last_error(lib)
    assert lib.ikf_cloud_clearance(eng._h, None, 4, out.data_ptr(), None, None) == _lib.IKF_ERR_NULL_POINTER
    assert put(eng._h, good, 3, 0.02, 0.25) == _lib.IKF_OK and eng.world_cloud_size == 3
    for coord, bad in ((0, nan), (1, inf), (2, -inf)):
        pts = good.copy()
        pts[2, coord] = bad
        assert put(eng._h, pts, 3) == _lib.IKF_ERR_BAD_ARGUMENT
        assert "point 2: non-finite coordinate" in _lib.last_error(lib), _lib.last_error(lib)
    assert put(eng._h, good, -1) == _lib.IKF_ERR_BAD_ARGUMENT and "0 .. 1048576" in _lib.last_error(lib)
    assert put(eng._h, good, (1 << 20) + 1) == _lib.IKF_ERR_BAD_ARGUMENT and "0 .. 1048576" in _lib.last_error(lib)
    for radius in (-0.01, nan, inf):
        assert put(eng._h, good, 3, radius) == _lib.IKF_ERR_BAD_ARGUMENT and "point_radius" in _lib.last_error(lib)
    for thr in (nan, inf):
        assert put(eng._h, good, 3, 0.01, thr) == _lib.IKF_ERR_BAD_ARGUMENT and "min_clearance" in _lib.last_error(lib)
    assert put(eng._h, None, 3) == _lib.IKF_ERR_NULL_POINTER
    assert eng.world_cloud_size == 3   # every refused call left the cloud of three points in force ...
    got = _clearance(eng, q.cpu())
    assert (got["colliding"] == 0).all() and (got["clearance"] > 3.0).all() and (got["clearance"] < 6.0).all()   # ... with its threshold of 0.25
    with pytest.raises(Exception, match="at most 1048576 points"):
        eng.set_world_cloud(np.zeros(((1 << 20) + 1, 3), np.float32), 0.01)
    assert eng.world_cloud_size == 3
    torch.cuda.synchronize()


# ---- 6. the ranking with a cloud -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k", WH.RANK_SHAPES)
@pytest.mark.parametrize("which", RH.CASE_CHAINS)
def test_ranking_with_a_cloud(which, m, k):
    """ikf_rank_candidates while a cloud is set - alone and beside a primitive world, with and without reject_collisions: row scores by
    rank_helpers.check_row_scores against the reference whose admissibility carries the cloud term (and the world's) with their bands; the
    selection against rank_helpers.select on the engine's own row scores, bit for bit."""
    robot, orob = H.kin_robots(which)
    eng = _eng(which)
    caps = RH.collision_capsules(robot)
    poses, q, _, wcl, wthr, cl, thr = CH.rank_case(which, m, k)
    eng.set_world_cloud(CH.cloud(which, CH.RANK_POINTS), R, thr)
    n_keep = min(4, k)
    for with_world in (False, True):
        if with_world:
            eng.set_world(WH.scene(which, WH.RANK_SCENE), wthr)
        for collisions in (False, True):
            self_thr = RH.clearance_threshold(orob, caps, q) if collisions else 0.0
            ref = CH.rank_reference(orob, caps, wcl if with_world else None, wthr, cl, thr, poses, q, k, 0.01, self_collisions=collisions,
                                    min_clearance=self_thr)
            out = _rank(eng, poses, q, k, _opt(n_keep=n_keep, collisions=collisions, min_clearance=self_thr))
            if np.isfinite(out["row_score"]).any() or ref["admissible"][~ref["near"]].any():
                RH.check_row_scores(out["row_score"], ref, f"{which} m {m} k {k} world {with_world} collisions {collisions}")
            _check_selection(out, q, m, k, n_keep, f"{which} m {m} k {k}")
            if m * k >= 130 and not with_world:
                cloud_only = (cl < thr - CH.BAND) & np.isfinite(ref["score"])
                assert cloud_only.sum() >= 0.2 * k * m and np.isposinf(out["row_score"][cloud_only]).all()


# ---- 7. composition ----------------------------------------------------------------------------------------------------------------------------------
def test_ranking_with_a_cloud_is_the_ranking_without_one_with_the_rejected_rows_at_infinity():
    which, m, k = "panda", 64, 16
    eng = _eng(which)
    poses, q, q_ref, _, _, cl, thr = CH.rank_case(which, m, k)
    opt = _opt(n_keep=4, ref_weight=0.05, limits=True)
    before = _rank(eng, poses, q, k, opt, q_ref)
    eng.set_world_cloud(CH.cloud(which, CH.RANK_POINTS), R, thr)
    rejected = _clearance(eng, q)["colliding"].astype(bool)
    during = _rank(eng, poses, q, k, opt, q_ref)
    assert 0.2 * k * m <= rejected.sum() <= 0.8 * k * m
    assert np.isposinf(during["row_score"][rejected]).all() and H.same_bits(during["row_score"][~rejected], before["row_score"][~rejected])
    want = before["row_score"].copy()
    want[rejected] = np.inf
    assert H.same_bits(during["row_score"], want)
    _check_selection(during, q, m, k, 4, "composition")
    assert np.array_equal(during["count"], np.isfinite(want).reshape(k, m).sum(0))


# ---- 8. path IK, diverse-of-K, the flow in front ----------------------------------------------------------------------------------------------------
def test_path_search_and_diverse_select_never_take_a_rejected_row():
    which, T, k = "panda", 5, 8
    eng = _eng(which)
    robot, orob = H.kin_robots(which)
    poses, q, _ = RH.candidates(orob, T, k, seed=12, lo_exp=-1.5)
    pts = CH.cloud(which, CH.RANK_POINTS)
    cl = CH.reference(orob, RH.collision_capsules(robot), pts, R, q)
    thr = float(np.median(cl))
    rejected, admitted = cl < thr - CH.BAND, cl > thr + CH.BAND
    assert rejected.any() and admitted.reshape(k, T).any(0).all()   # (every pose keeps a candidate the cloud surely admits)
    eng.set_world_cloud(pts, R, thr)
    ranked = _rank(eng, poses, q, k, _opt(n_keep=1))
    popt = eng.path_options(reject_limits=False, node_weight=20.0)
    path, index, cost, reach, node = [t.cpu().numpy() for t in eng.path_search(poses.to(DEV), k, q.to(DEV), popt, node_costs=True)]
    assert np.isposinf(node[rejected]).all() and np.isfinite(cost[0]) and (index >= 0).all()
    assert not rejected[index * T + np.arange(T)].any()
    assert H.same_bits(node, ranked["row_score"])   # (the node costs are the ranking's row scores under the same cloud)
    dopt = eng.diverse_options(n_keep=4, reject_limits=False, min_separation=0.05)
    q_out, score, index, sep, kept, count, rows = [t.cpu().numpy() for t in eng.diverse_select(poses.to(DEV), k, q.to(DEV), dopt, row_scores=True)]
    assert np.isposinf(rows[rejected]).all() and (kept >= 1).all() and H.same_bits(rows, ranked["row_score"])
    taken = index[index >= 0].astype(np.int64) * T + np.nonzero(index >= 0)[0]
    assert not rejected[taken].any()


def _solver(model):
    from ikflow_amd.ikflow_solver import IKFlowSolver

    robot, hp, lay, sd = H.tiny_model() if model == "tiny" else H.panda_model()
    robot.set_collision_capsules(RH.collision_capsules(robot))
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    return s, robot, lay


@pytest.mark.parametrize("model,refine", [("tiny", 0), ("tiny", 2), ("panda", 0)])
def test_generate_ranked_with_a_cloud_equals_the_flow_then_rank_candidates(model, refine):
    """ikf_generate_ranked under a cloud equals the flow (and, with a refinement set, its LM steps) followed by ikf_rank_candidates on the same
    handle, bit for bit: under refinement the REFINED rows are tested against the cloud."""
    from ikflow_amd.ikflow_solver import mm_to_m

    s, robot, lay = _solver(model)
    m, k, n_keep = 65, 16, 4
    _, poses = H.reachable_poses(robot, m, 6)
    y, L = poses.float().to(DEV), H.latents(k * m, lay.dim, 8).to(DEV)
    q = s.generate_ik_solutions(y.repeat((k, 1)), latent=L)
    eng = s.engine(DEV)
    if refine:
        q = eng.refine_candidates(y, k, q, refine, 0.0, 0.0)
        s.set_candidate_refine(refine, 0.0, 0.0)
    without = s.generate_ranked_ik_solutions(y, k, n_keep, latent=L, reject_self_collisions=False, return_row_scores=True)
    pts = CH.cloud("panda", CH.RANK_POINTS)   # (both models' robot is the Panda)
    s.set_world_cloud(pts, R, 0.0)
    assert eng.world_cloud_size == len(pts)
    # not an accuracy claim: only a threshold that rejects about half of these rows, and is no row's own clearance
    thr = float(eng.cloud_clearance(q)[0].median()) + 5e-5
    s.set_world_cloud(torch.tensor(pts, device=DEV), R, thr)
    got = s.generate_ranked_ik_solutions(y, k, n_keep, latent=L, reject_self_collisions=False, return_row_scores=True)
    opt = eng.rank_options(n_keep, mm_to_m(1) / 0.1, 0.0, None, None, True, False, 0.0)
    two_step = eng.rank_candidates(y, k, q, opt, row_scores=True)
    for a, b in zip(got, two_step):
        assert H.same_bits(a.cpu().numpy(), b.cpu().numpy())
    n_inf, n_inf_without = int(torch.isinf(got.row_scores).sum()), int(torch.isinf(without.row_scores).sum())
    assert n_inf_without < n_inf < k * m
    new_inf = torch.isinf(got.row_scores) & ~torch.isinf(without.row_scores)
    assert torch.equal(new_inf, eng.cloud_clearance(q)[1] & ~torch.isinf(without.row_scores))
    s.set_world_cloud(None, R)
    assert eng.world_cloud_size == 0
    again = s.generate_ranked_ik_solutions(y, k, n_keep, latent=L, reject_self_collisions=False, return_row_scores=True)
    for a, b in zip(again, without):
        assert H.same_bits(a.cpu().numpy(), b.cpu().numpy())


# ---- 9. off means off ----------------------------------------------------------------------------------------------------------------------------------
def test_a_cleared_cloud_and_a_far_cloud_give_every_entry_point_the_bits_of_a_handle_without_one():
    from ikflow_amd.engine import Engine

    s, robot, lay = _solver("tiny")
    m, k = 9, 16
    _, poses = H.reachable_poses(robot, m, 4)
    y, L = poses.float().to(DEV), H.latents(k * m, lay.dim, 9).to(DEV)

    def engine():
        eng = Engine(s.layout, robot, DEV)
        eng.load_state_dict(s._state_dict_np)
        eng.set_collision_model(*robot._collision_model)
        return eng

    def six(eng):
        ro, po, do = eng.rank_options(n_keep=4, reject_limits=True), eng.path_options(reject_limits=True), eng.diverse_options(n_keep=4, min_separation=0.05)
        outs = list(eng.generate_ranked(y, k, L, True, ro, row_scores=True))
        outs += list(eng.generate_path(y, k, L[:k], True, True, po))
        outs += list(eng.generate_diverse(y, k, L, True, do))
        rows = s.generate_ik_solutions(y.repeat((k, 1)), latent=L)
        outs += list(eng.rank_candidates(y, k, rows, ro, row_scores=True))
        outs += list(eng.path_search(y, k, rows, po, node_costs=True))
        outs += list(eng.diverse_select(y, k, rows, do, row_scores=True))
        torch.cuda.synchronize()
        return [None if t is None else t.cpu().numpy() for t in outs]

    never = six(engine())
    eng = engine()
    rows = s.generate_ik_solutions(y.repeat((k, 1)), latent=L)
    eng.set_world_cloud(CH.cloud("panda", CH.RANK_POINTS), R, 0.05)
    under = six(eng)
    assert any(not ((a is None and b is None) or H.same_bits(a, b)) for a, b in zip(under, never))   # (the cloud does something here)
    eng.clear_world_cloud()
    got = six(eng)
    assert all((a is None and b is None) or H.same_bits(a, b) for a, b in zip(got, never)), "cleared"
    far = CH.cloud("panda", 4097) + np.array([50.0, 0.0, 0.0], np.float32)
    eng.set_world_cloud(far, R, 1.0)
    assert eng.world_cloud_size == 4097 and float(eng.cloud_clearance(rows)[0].min()) > 1.0
    got = six(eng)
    assert all((a is None and b is None) or H.same_bits(a, b) for a, b in zip(got, never)), "far"


# ---- 10. memory ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_clouds_buffers_regrow_and_are_released_with_the_handle():
    """set / regrow / clear / set on one engine, the clearance and a chunked ranking under each cloud with the bits of a fresh engine; then the
    engine goes and the device's free memory is back (the accounting of tests/test_handle_memory.py: mem_get_info against torch's own reserve)."""
    from ikflow_amd.engine import Engine

    which = "panda"
    robot, _ = H.kin_robots(which)
    base = _eng(which)
    poses, q, _, _, _, _, thr = CH.rank_case(which, 64, 16)
    qd, yd = q.to(DEV), poses.to(DEV)

    def engine():
        eng = Engine(base.layout, base.robot, DEV)
        eng.set_collision_model(*robot._collision_model)
        return eng

    def run(eng, n_points):
        if n_points:
            eng.set_world_cloud(CH.cloud(which, n_points), R, thr)
        else:
            eng.clear_world_cloud()
        outs = list(eng.cloud_clearance(qd)) + list(eng.rank_candidates(yd, 16, qd, eng.rank_options(n_keep=4), row_scores=True))
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in outs]

    sequence = (513, 4097, 0, 511, 4097)
    want = {}
    for n_points in set(sequence):
        fresh = engine()
        want[n_points] = run(fresh, n_points)
        del fresh
    gc.collect()
    torch.cuda.synchronize()
    free0, stat0 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    eng = engine()
    for n_points in sequence:
        got = run(eng, n_points)
        assert eng.world_cloud_size == n_points and all(H.same_bits(g, w) for g, w in zip(got, want[n_points])), n_points
    del eng
    gc.collect()
    torch.cuda.synchronize()
    free1, stat1 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    assert free0 - free1 <= stat1 - stat0, f"{free0 - free1 - (stat1 - stat0)} bytes of device memory did not come back with the handle"


# ---- 11. the solver ----------------------------------------------------------------------------------------------------------------------------------------
def test_solver_set_world_cloud_before_and_after_the_engine_exists():
    """A cloud given before the first GPU call reaches the engine that call creates (collision model first); one given afterwards reaches the
    engine at once; a ranked call drops what the reference drops."""
    pts = CH.cloud("panda", CH.RANK_POINTS)
    m, k = 65, 16
    early, robot, lay = _solver("tiny")
    assert early._engine is None or early._engine.world_cloud_size == 0
    early.set_world_cloud(pts, R, 0.0)   # (on a GPU machine this creates the engine; the cloud is remembered either way)
    _, poses = H.reachable_poses(robot, m, 6)
    y, L = poses.float().to(DEV), H.latents(k * m, lay.dim, 8).to(DEV)
    eng = early.engine(DEV)
    assert eng.world_cloud_size == len(pts)
    late, _, _ = _solver("tiny")
    q = late.generate_ik_solutions(y.repeat((k, 1)), latent=L)
    assert late.engine(DEV).world_cloud_size == 0
    orob = H.O(robot)
    cl = CH.reference(orob, RH.collision_capsules(robot), pts, R, q.cpu())
    thr = float(np.median(cl))
    results = []
    for s in (early, late):
        s.set_world_cloud(pts, R, thr)
        assert s.engine(DEV).world_cloud_size == len(pts)
        results.append(s.generate_ranked_ik_solutions(y, k, 4, latent=L, reject_self_collisions=False, return_row_scores=True))
    for a, b in zip(*results):
        assert H.same_bits(a.cpu().numpy(), b.cpu().numpy())
    rows = results[0].row_scores.cpu().numpy()
    decided = np.abs(cl - thr) > CH.BAND
    assert np.isposinf(rows[decided & (cl < thr)]).all() and (decided & (cl < thr)).sum() >= 0.2 * k * m
    late.set_world_cloud(None, R)
    free = late.generate_ranked_ik_solutions(y, k, 4, latent=L, reject_self_collisions=False, return_row_scores=True).row_scores.cpu().numpy()
    kept = decided & (cl > thr)
    assert H.same_bits(rows[kept], free[kept])   # (what the cloud admits keeps its score)
