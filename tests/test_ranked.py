"""Best-of-K ranking on the GPU (include/ikflow_amd_rank.h; ikflow_amd/csrc/rank_kernels.hip, rank_math.h, api_rank.hip): row scores against
the fp64 oracle, the selection against numpy on the engine's own row scores (bit for bit), independence of batch size / position / chunking,
buffers and status codes, the flow + ranking call against generate_ik_solutions and the oracle, and ikf_reserve_ranked.

The tolerance of a row score and the bands around the admissibility decisions are defined in tests/rank_helpers.py from the project's existing
figures; tests/test_rank_math_host.py shows on the CPU that the f32 oracle itself stays inside that tolerance on these input families.
Every call below goes through _rank(): outputs are windows inside sentinel-filled buffers with guard rows in front and behind (the scheme of
tests/test_kinematics.py::_run, rebuilt here), so every test also checks that nothing outside is written and everything inside is."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H
import rank_helpers as RH
from ikflow_amd import _lib
from oracle import flow_oracle as fo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
NAN_BITS = 0x7FC00000
INT_SENTINEL = -1414812757   # 0xABABABAB


def _eng(which, collisions=False):
    from ikflow_amd.engine import kinematics_engine_for

    robot = H.kin_robots(which)[0]
    eng = kinematics_engine_for(robot, DEV)
    if collisions:
        robot.set_collision_capsules(RH.collision_capsules(robot))
        eng.set_collision_model(*robot._collision_model)
        eng._collision_source = robot._collision_model
    return eng


def _opt(n_keep=1, rot_weight=0.01, ref_weight=0.0, max_pos=None, max_rot=None, limits=False, collisions=False, min_clearance=0.0):
    return _lib.ikf_rank_options(n_keep, rot_weight, ref_weight, -1.0 if max_pos is None else max_pos, -1.0 if max_rot is None else max_rot,
                                 int(limits), int(collisions), min_clearance)


def _window(rows, cols, dtype):
    if dtype == torch.float32:
        return torch.full((rows + 2 * GUARD, cols), float("nan"), dtype=torch.float32, device=DEV)
    return torch.full((rows + 2 * GUARD, cols), INT_SENTINEL, dtype=torch.int32, device=DEV)


def _check_window(buf, rows, name):
    win = buf[GUARD:GUARD + rows]
    if buf.dtype == torch.float32:
        bits = buf.view(torch.int32)
        assert (bits[:GUARD] == NAN_BITS).all() and (bits[GUARD + rows:] == NAN_BITS).all(), f"{name}: a row outside the window was written"
        assert not torch.isnan(win).any(), f"{name}: an element inside the window was not written"
    else:
        assert (buf[:GUARD] == INT_SENTINEL).all() and (buf[GUARD + rows:] == INT_SENTINEL).all(), f"{name}: a row outside the window was written"
        assert (win != INT_SENTINEL).all(), f"{name}: an element inside the window was not written"
    return win.clone()


OUTPUTS = ("q_out", "score", "index", "count", "row_score")


def _rank(eng, poses, q, k, opt, q_ref=None, stream=None, null=(), latent=None, clamp=True, expect=_lib.IKF_OK):
    """ikf_rank_candidates (or, with `latent`, ikf_generate_ranked) through eng.lib on guarded buffers -> {name: cpu numpy window}; `null`: the
    nullable outputs passed as null."""
    m, nd, nk = poses.shape[0], eng.layout.ndof, opt.n_keep
    shapes = {"q_out": (m * nk, nd, torch.float32), "score": (m * nk, 1, torch.float32), "index": (m * nk, 1, torch.int32),
              "count": (m, 1, torch.int32), "row_score": (k * m, 1, torch.float32)}
    bufs = {n: _window(*shapes[n]) for n in OUTPUTS if n not in null}
    ptr = [bufs[n][GUARD:].data_ptr() if n in bufs else None for n in OUTPUTS]
    poses_d = poses.to(DEV).contiguous()
    rows_d = (q if latent is None else latent).to(DEV).contiguous()
    ref_d = None if q_ref is None else q_ref.to(DEV).contiguous()
    torch.cuda.synchronize()
    s = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(0)
    if latent is None:
        code = eng.lib.ikf_rank_candidates(eng._h, poses_d.data_ptr(), m, k, rows_d.data_ptr(), None if ref_d is None else ref_d.data_ptr(), C.byref(opt), *ptr, s)
    else:
        code = eng.lib.ikf_generate_ranked(eng._h, poses_d.data_ptr(), m, k, rows_d.data_ptr(), int(clamp), None if ref_d is None else ref_d.data_ptr(),
                                           C.byref(opt), *ptr, s)
    assert code == expect, (code, _lib.last_error(eng.lib))
    torch.cuda.synchronize()
    out = {n: _check_window(b, shapes[n][0], n).cpu().numpy() for n, b in bufs.items()}
    for n in ("score", "index"):
        if n in out:
            out[n] = out[n].reshape(m, nk)
    if "q_out" in out:
        out["q_out"] = out["q_out"].reshape(m, nk, nd)
    for n in ("count", "row_score"):
        if n in out:
            out[n] = out[n].reshape(-1)
    return out


def _check_selection(out, q, m, k, n_keep, what=""):
    """The returned lists against the stable lexsort of the engine's own row scores of each pose - no tolerance."""
    idx, sc, cnt = RH.select(out["row_score"], m, k, n_keep)
    assert np.array_equal(out["index"], idx), f"{what}: index_out is not the lexsort of the row scores, first pose {np.flatnonzero((out['index'] != idx).any(1))[:3]}"
    assert H.same_bits(out["score"], sc), f"{what}: score_out"
    assert np.array_equal(out["count"], cnt), f"{what}: count_out"
    qn = q.numpy().reshape(k, m, -1)
    want_q = np.where((idx >= 0)[..., None], qn[np.maximum(idx, 0), np.arange(m)[:, None]], np.float32(0.0))
    assert H.same_bits(out["q_out"], want_q.astype(np.float32)), f"{what}: q_out is not the candidate rows at index_out"
    assert np.isposinf(out["score"][idx < 0]).all() and (out["q_out"][idx < 0] == 0).all()


# ---- 1. row scores against the fp64 oracle ---------------------------------------------------------------------------------------------------
VARIANTS = {
    "plain": dict(),
    "q_ref": dict(ref_weight=0.05),
    "thresholds": dict(max_pos=0.02, max_rot=0.3),
    "limits_wild": dict(limits=True),
    "collisions": dict(collisions=True),   # min_clearance: rank_helpers.clearance_threshold of the rows
}


@pytest.mark.parametrize("rot_weight", [0.01, 1.0])
@pytest.mark.parametrize("which", H.KIN_ALL)
def test_row_scores_against_the_fp64_oracle(which, rot_weight):
    """m = 257 poses x k = 50 candidates (truth + noise of scale logspace(-3, 0, k), clamped): every row of d_row_score_out within its eps of the fp64
    oracle, admissibility exact outside the bands; with and without q_ref, with thresholds, with the limit test on unclamped rows, with capsules."""
    robot, orob = H.kin_robots(which)
    eng = _eng(which, collisions=True)
    caps = RH.collision_capsules(robot)
    m, k = 257, 50
    for name, v in VARIANTS.items():
        poses, q, q_ref = RH.candidates(orob, m, k, seed=3, wild=name == "limits_wild")
        use_ref = name == "q_ref"
        if name == "collisions":
            v = dict(v, min_clearance=RH.clearance_threshold(orob, caps, q))
        out = _rank(eng, poses, q, k, _opt(n_keep=4, rot_weight=rot_weight, **v), q_ref if use_ref else None)
        ref = RH.reference(orob, poses, q, k, rot_weight, q_ref if use_ref else None, v.get("ref_weight", 0.0), v.get("max_pos"), v.get("max_rot"),
                           v.get("limits", False), caps if v.get("collisions") else None, v.get("min_clearance", 0.0))
        worst = RH.check_row_scores(out["row_score"], ref, f"{which} {name}")
        n_bad = int((~ref["admissible"]).sum())
        print(f"row scores {which} rot_weight {rot_weight} {name}: worst {worst:.3f} of eps, {n_bad} of {k * m} rows inadmissible")
        if name not in ("plain", "q_ref"):
            assert 0 < n_bad < k * m
        _check_selection(out, q, m, k, 4, f"{which} {name}")


# ---- 2. the selection is exact -----------------------------------------------------------------------------------------------------------------
SHAPES = [(m, k) for m in (1, 63, 64, 65, 257, 1000) for k in (1, 2, 50, 64, 65)] + [(1, 5000), (3, 1000)]


def test_the_shape_list_holds_chunked_and_unchunked_calls():
    eng = _eng("panda")
    chunks = {s: eng.rank_chunks(*s) for s in SHAPES}
    print("K-chunks per (m, k):", chunks)
    assert min(chunks.values()) == 1 and max(chunks.values()) > 1 and chunks[(1, 5000)] > 1
    assert all(1 <= c <= 64 for c in chunks.values())


@pytest.mark.parametrize("m,k", SHAPES)
def test_selection_equals_the_lexsort_of_the_engines_row_scores(m, k):
    """(index, score) bit-equal to the stable lexsort of the engine's own row scores of the pose, q_out the candidate rows at those indices, count
    the number of finite row scores, unfilled slots 0 / +inf / -1 - for n_keep 1, 4, 16 and min(k, 16).  The position threshold makes about half
    of the candidates inadmissible, so partly filled and empty lists occur."""
    orob = H.kin_robots("panda")[1]
    eng = _eng("panda")
    poses, q, _ = RH.candidates(orob, m, k, seed=m + k)
    for n_keep in sorted({min(n, k) for n in (1, 4, 16, min(k, 16))}):
        out = _rank(eng, poses, q, k, _opt(n_keep=n_keep, max_pos=0.03, limits=True))
        _check_selection(out, q, m, k, n_keep, f"m {m} k {k} n_keep {n_keep}")
    if m >= 63 and k >= 50:
        assert (out["count"] < k).all() and (out["count"] > 0).any()   # (the threshold does reject candidates, and not all of them)


@pytest.mark.parametrize("k", [50, 1000])
def test_selection_on_hand_made_poses(k):
    """Pose 0: every candidate identical (ties: indices 0 .. n_keep - 1).  Pose 1: all inadmissible.  Pose 2: exactly one admissible, the last repeat.
    Pose 3: a NaN row among ordinary ones.  Pose 4: ordinary.  k = 50 runs in one chunk, k = 1000 in several."""
    orob = H.kin_robots("panda")[1]
    eng = _eng("panda")
    m, nd = 5, orob.ndof
    poses, q, _ = RH.candidates(orob, m, k, seed=9, lo_exp=-3.0, hi_exp=-2.0)
    lo, hi = RH.limits(orob)
    q = q.reshape(k, m, nd).clone()
    q[:, 0] = q[0, 0]
    q[:, 1] = hi + 0.5
    q[:, 2] = hi + 0.5
    q[k - 1, 2] = 0.5 * (lo + hi)
    q[2, 3] = float("nan")
    q[7, 3, 1] = float("nan")
    q = q.reshape(k * m, nd).contiguous()
    assert (eng.rank_chunks(m, k) > 1) == (k == 1000)
    for n_keep in (1, 4, 16):
        out = _rank(eng, poses, q, k, _opt(n_keep=n_keep, limits=True))
        _check_selection(out, q, m, k, n_keep, f"hand-made k {k} n_keep {n_keep}")
        assert np.array_equal(out["index"][0], np.arange(n_keep)) and out["count"][0] == k
        assert out["count"][1] == 0 and (out["index"][1] == -1).all() and np.isposinf(out["score"][1]).all() and (out["q_out"][1] == 0).all()
        assert out["count"][2] == 1 and out["index"][2, 0] == k - 1 and (out["index"][2, 1:] == -1).all()
        rs = out["row_score"].reshape(k, m)
        assert np.isposinf(rs[2, 3]) and np.isposinf(rs[7, 3]) and out["count"][3] == k - 2 and 2 not in out["index"][3] and 7 not in out["index"][3]
        assert out["count"][4] == k


# ---- 3. independence -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [50, 1000])
def test_a_pose_ranked_alone_equals_the_pose_inside_a_batch(k):
    """m = 1 against the same pose as first, middle and last of m = 257 (another tile width, another chunking): bit-identical row scores, lists, rows."""
    orob = H.kin_robots("panda")[1]
    eng = _eng("panda")
    m = 257
    poses, q, q_ref = RH.candidates(orob, m, k, seed=17)
    opt = _opt(n_keep=4, max_pos=0.05, limits=True, ref_weight=0.02)
    full = _rank(eng, poses, q, k, opt, q_ref)
    assert eng.rank_chunks(1, k) != eng.rank_chunks(m, k) or k == 50
    q3 = q.reshape(k, m, -1)
    for j in (0, 128, 256):
        alone = _rank(eng, poses[j:j + 1], q3[:, j].contiguous(), k, opt, q_ref[j:j + 1])
        assert H.same_bits(alone["row_score"], full["row_score"].reshape(k, m)[:, j]), j
        for n in ("score", "index", "q_out"):
            assert H.same_bits(alone[n][0], full[n][j]), (n, j)
        assert alone["count"][0] == full["count"][j]


def test_permuting_a_poses_candidates_permutes_the_indices():
    orob = H.kin_robots("fetch")[1]
    eng = _eng("fetch")
    m, k = 65, 200
    poses, q, _ = RH.candidates(orob, m, k, seed=23)
    opt = _opt(n_keep=16, max_pos=0.05)
    a = _rank(eng, poses, q, k, opt)
    perm = torch.randperm(k, generator=torch.Generator().manual_seed(1))
    b = _rank(eng, poses, q.reshape(k, m, -1)[perm].reshape(k * m, -1).contiguous(), k, opt)
    back = np.where(b["index"] >= 0, perm.numpy()[np.maximum(b["index"], 0)], -1)
    assert H.same_bits(a["score"], b["score"]) and np.array_equal(a["count"], b["count"])
    rs = a["row_score"].reshape(k, m)
    distinct = np.array([len(np.unique(rs[:, j][np.isfinite(rs[:, j])])) == np.isfinite(rs[:, j]).sum() for j in range(m)])
    assert distinct.mean() >= 0.9                                       # (without ties the order is the scores' alone, so it must carry over exactly)
    assert np.array_equal(back[distinct], a["index"][distinct]) and H.same_bits(a["q_out"][distinct], b["q_out"][distinct])
    for j in np.flatnonzero(~distinct):                                 # (with a tie the index decides: the same scores, perhaps other rows)
        assert len(set(back[j].tolist())) == len(set(a["index"][j].tolist()))


# ---- 4. buffers, streams, null outputs, status codes --------------------------------------------------------------------------------------------
def test_non_default_stream_and_null_outputs():
    orob = H.kin_robots("syn6p")[1]
    eng = _eng("syn6p")
    for m, k in ((65, 50), (3, 1000)):
        poses, q, _ = RH.candidates(orob, m, k, seed=2)
        opt = _opt(n_keep=4, max_pos=0.05)
        ref = _rank(eng, poses, q, k, opt)
        got = _rank(eng, poses, q, k, opt, stream=torch.cuda.Stream(device=DEV))
        assert all(H.same_bits(ref[n], got[n]) for n in OUTPUTS)
        for null in OUTPUTS[1:]:
            got = _rank(eng, poses, q, k, opt, null=(null,))
            assert null not in got and all(H.same_bits(ref[n], got[n]) for n in got)
        got = _rank(eng, poses, q, k, opt, null=OUTPUTS[1:])
        assert H.same_bits(ref["q_out"], got["q_out"])


def test_status_codes():
    orob = H.kin_robots("panda")[1]
    eng = _eng("panda")
    lib, h = eng.lib, eng._h
    m, k = 4, 5
    poses, q, _ = RH.candidates(orob, m, k)
    P, Q = poses.to(DEV), q.to(DEV)
    out = torch.empty(m * 4 * 7, device=DEV)
    opt = _opt(n_keep=2)
    call = lambda h_, p, n, k_, q_, o, qo: lib.ikf_rank_candidates(h_, p, n, k_, q_, None, o, qo, None, None, None, None, None)
    ok = (h, P.data_ptr(), m, k, Q.data_ptr(), C.byref(opt), out.data_ptr())
    assert call(*ok) == _lib.IKF_OK
    assert call(None, *ok[1:]) == _lib.IKF_ERR_NULL_POINTER
    assert call(h, None, m, k, Q.data_ptr(), C.byref(opt), out.data_ptr()) == _lib.IKF_ERR_NULL_POINTER
    assert call(h, P.data_ptr(), m, k, None, C.byref(opt), out.data_ptr()) == _lib.IKF_ERR_NULL_POINTER
    assert call(h, P.data_ptr(), m, k, Q.data_ptr(), None, out.data_ptr()) == _lib.IKF_ERR_NULL_POINTER
    assert call(h, P.data_ptr(), m, k, Q.data_ptr(), C.byref(opt), None) == _lib.IKF_ERR_NULL_POINTER
    assert call(h, P.data_ptr(), -1, k, Q.data_ptr(), C.byref(opt), out.data_ptr()) == _lib.IKF_ERR_BAD_ARGUMENT
    assert call(h, P.data_ptr(), m, 0, Q.data_ptr(), C.byref(opt), out.data_ptr()) == _lib.IKF_ERR_BAD_ARGUMENT
    for n_keep in (0, 6, 17):
        assert call(h, P.data_ptr(), m, k, Q.data_ptr(), C.byref(_opt(n_keep=n_keep)), out.data_ptr()) == _lib.IKF_ERR_BAD_ARGUMENT
    assert call(h, P.data_ptr(), 2 ** 30, 2, Q.data_ptr(), C.byref(opt), out.data_ptr()) == _lib.IKF_ERR_BAD_ARGUMENT   # k * n_poses = 2^31
    assert call(h, None, 0, k, None, C.byref(opt), None) == _lib.IKF_OK                                                 # nothing to do: null buffers are fine
    # reject_collisions without a collision model, and ikf_generate_ranked without weights: a fresh handle (the cached one may carry a model)
    from ikflow_amd.engine import Engine

    fresh = Engine(eng.layout, eng.robot, DEV)
    assert lib.ikf_rank_candidates(fresh._h, P.data_ptr(), m, k, Q.data_ptr(), None, C.byref(_opt(n_keep=2, collisions=True)), out.data_ptr(),
                                   None, None, None, None, None) == _lib.IKF_ERR_BAD_ARGUMENT
    lat = torch.zeros(m * k, eng.layout.dim, device=DEV)
    gen = lambda h_: lib.ikf_generate_ranked(h_, P.data_ptr(), m, k, lat.data_ptr(), 1, None, C.byref(opt), out.data_ptr(), None, None, None, None, None)
    assert gen(fresh._h) == _lib.IKF_ERR_NOT_LOADED and gen(None) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_reserve_ranked(None, 4, 4) == _lib.IKF_ERR_NULL_POINTER and lib.ikf_reserve_ranked(fresh._h, 0, 4) == _lib.IKF_ERR_BAD_ARGUMENT
    assert lib.ikf_reserve_ranked(fresh._h, 2 ** 30, 2) == _lib.IKF_ERR_BAD_ARGUMENT and lib.ikf_reserve_ranked(fresh._h, 100, 50) == _lib.IKF_OK
    torch.cuda.synchronize()


# ---- 5. end to end with the flow ---------------------------------------------------------------------------------------------------------------
def _clear_poses(score, eps, n_keep, crude=False):
    """score, eps [k x m] (fp64 oracle).  A pose is clear when the eps-intervals of its kept candidates and of the first one left out are disjoint from
    every other candidate's (crude: every interval as wide as the pose's largest eps)."""
    k, m = score.shape
    clear = np.zeros(m, bool)
    for j in range(m):
        s, e = score[:, j], (np.full(k, eps[:, j].max()) if crude else eps[:, j])
        order = np.argsort(s, kind="stable")
        ok = True
        for i in order[:min(n_keep + 1, k)]:
            gap = np.abs(s - s[i]) - (e + e[i])
            gap[i] = np.inf
            ok = ok and bool((gap > 0).all())
        clear[j] = ok
    return clear


def _check_against_oracle_order(out, ref, m, k, n_keep, min_clear, what, crude=False):
    score, eps = ref["score"].reshape(k, m), ref["eps"].reshape(k, m)
    score = np.where(ref["admissible"].reshape(k, m), score, np.inf)
    clear = _clear_poses(score, eps, n_keep, crude)
    order = np.argsort(score, axis=0, kind="stable")[:n_keep].T                        # [m x n_keep]
    kept = np.take_along_axis(score, order.T, 0).T
    want = np.where(np.isfinite(kept), order, -1)
    share = clear.mean()
    print(f"{what}: {share:.3f} of the poses are clear")
    assert share >= min_clear, (what, share)
    assert np.array_equal(out["index"][clear], want[clear]), f"{what}: the kept indices differ from the oracle's on a clear pose"
    rest = ~clear
    bound = eps.max(0)[rest, None]
    fin = np.isfinite(kept[rest])
    assert np.array_equal(np.isfinite(out["score"][rest]), fin)
    assert (np.abs(out["score"][rest].astype(np.float64) - kept[rest])[fin] <= np.broadcast_to(bound, kept[rest].shape)[fin]).all(), f"{what}: order-statistic bound"
    return clear, want


_MODELS = {}


def _solver(model):
    from ikflow_amd.ikflow_solver import IKFlowSolver

    if model not in _MODELS:
        robot, hp, lay, sd = H.tiny_model() if model == "tiny" else H.panda_model()
        s = IKFlowSolver(hp, robot)
        s.load_state_dict_tensors(sd)
        _MODELS[model] = (s, robot, lay, sd)
    return _MODELS[model]


@pytest.mark.parametrize("shape", [(65, 50, 4), (1, 300, 4)])
@pytest.mark.parametrize("model", ["tiny", "panda"])
def test_flow_and_ranking_in_one_call(model, shape):
    """generate_ranked_ik_solutions(..., latent=L): the kept rows are bit-equal to generate_ik_solutions(y.repeat((k, 1)), latent=L) at rows
    index * m + j; against the oracle's flow and fp64 scores the indices agree on every clear pose (at least 0.95 of them) and the rest meets the
    order-statistic bound."""
    m, k, n_keep = shape
    s, robot, lay, sd = _solver(model)
    orob = H.O(robot)
    _, poses = H.reachable_poses(robot, m, 6)
    poses = poses.float()
    L = H.latents(k * m, lay.dim, 8)
    y = poses.to(DEV) if m > 1 else poses[0].to(DEV)
    q_or = fo.generate_ik_solutions_torch(sd, lay, robot, poses.repeat((k, 1)), L, clamp=True)
    for rot_weight in (0.01, 1.0):
        got = s.generate_ranked_ik_solutions(y, k, n_keep, latent=L.to(DEV), rot_weight=rot_weight, return_row_scores=True)
        assert got._fields == ("solutions", "scores", "repeat_index", "n_admissible", "row_scores")
        plain = s.generate_ik_solutions(poses.to(DEV).repeat((k, 1)), latent=L.to(DEV)).cpu()
        out = {"q_out": got.solutions.cpu().numpy(), "score": got.scores.cpu().numpy(), "index": got.repeat_index.cpu().numpy(),
               "count": got.n_admissible.cpu().numpy(), "row_score": got.row_scores.cpu().numpy()}
        assert out["index"].dtype == np.int32 and out["count"].dtype == np.int32 and out["q_out"].shape == (m, n_keep, orob.ndof)
        _check_selection(out, plain, m, k, n_keep, f"{model} {shape}")     # (q_out = the plain call's rows at index * m + j, bit for bit)
        ref = RH.reference(orob, poses, q_or, k, rot_weight, reject_limits=True)
        _check_against_oracle_order(out, ref, m, k, n_keep, 0.95, f"{model} m {m} k {k} rot_weight {rot_weight}")
    four = s.generate_ranked_ik_solutions(y, k, n_keep, latent=L.to(DEV), rot_weight=1.0)
    assert four._fields == ("solutions", "scores", "repeat_index", "n_admissible") and torch.equal(four.repeat_index, got.repeat_index)


def test_same_seed_gives_the_candidates_of_generate_ik_solutions():
    s, robot, lay, sd = _solver("tiny")
    m, k = 33, 20
    _, poses = H.reachable_poses(robot, m, 1)
    y = poses.float().to(DEV)
    torch.manual_seed(1234)
    got = s.generate_ranked_ik_solutions(y, k, 2)
    torch.manual_seed(1234)
    plain = s.generate_ik_solutions(y.repeat((k, 1)))
    idx = got.repeat_index.long()
    rows = plain.reshape(k, m, -1)[idx.clamp(min=0), torch.arange(m, device=DEV)[:, None]]
    assert torch.equal(torch.where((idx >= 0)[..., None], rows, torch.zeros_like(rows)), got.solutions)


def test_collision_model_of_the_robot_reaches_the_solvers_own_handle():
    """reject_self_collisions=None means "when the robot carries a capsule model"; the solver pushes the model to its own engine handle."""
    from ikflow_amd.ikflow_solver import IKFlowSolver

    robot, hp, lay, sd = H.tiny_model()
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    m, k = 40, 30
    _, poses = H.reachable_poses(robot, m, 2)
    y, L = poses.float().to(DEV), H.latents(k * m, lay.dim, 4).to(DEV)
    before = s.generate_ranked_ik_solutions(y, k, 4, latent=L, return_row_scores=True)
    robot.set_collision_capsules(RH.collision_capsules(robot))
    after = s.generate_ranked_ik_solutions(y, k, 4, latent=L, return_row_scores=True)
    q = s.generate_ik_solutions(y.repeat((k, 1)), latent=L)
    clearance = robot.self_collision_distances(q)
    colliding, sure = clearance < 0.0, clearance.abs() > 1e-4           # (the band of test_capsule_geometry_against_the_oracle around the decision)
    assert 0 < int(colliding.sum()) < k * m
    assert torch.equal(torch.isinf(after.row_scores)[sure], (colliding | torch.isinf(before.row_scores))[sure])
    assert torch.equal(after.row_scores[~colliding & sure], before.row_scores[~colliding & sure])
    off = s.generate_ranked_ik_solutions(y, k, 4, latent=L, reject_self_collisions=False, return_row_scores=True)
    assert torch.equal(off.row_scores, before.row_scores)


@pytest.mark.parametrize("which", ["panda", "fetch", "syn4r", "syn5p", "syn6p", "syn8p"])
def test_seeded_candidates_against_the_oracles_order(which):
    """Candidates 0.2 .. 1 rad off the truth (logspace(-0.7, 0, k)), m = 257, k = 50, n_keep = 4, rot_weight 0.01: indices equal to the fp64 oracle's
    on every clear pose (cruder interval: the pose's largest eps; at least 0.9 of the poses), and the f32 oracle agrees with the fp64 one there."""
    orob = H.kin_robots(which)[1]
    eng = _eng(which)
    m, k, n_keep = 257, 50, 4
    poses, q, _ = RH.candidates(orob, m, k, seed=31, lo_exp=-0.7, hi_exp=0.0)
    out = _rank(eng, poses, q, k, _opt(n_keep=n_keep, rot_weight=0.01))
    ref = RH.reference(orob, poses, q, k, 0.01)
    clear, want = _check_against_oracle_order(out, ref, m, k, n_keep, 0.9, which, crude=True)
    r32 = RH.reference(orob, poses, q, k, 0.01, dtype=torch.float32)
    o32 = np.argsort(r32["score"].reshape(k, m), axis=0, kind="stable")[:n_keep].T
    assert np.array_equal(o32[clear], want[clear])


# ---- 6. ikf_reserve_ranked ---------------------------------------------------------------------------------------------------------------------
def test_after_reserve_ranked_a_call_of_that_size_allocates_nothing():
    """The debug header has no allocation counter, so what is checked is the device's free memory (hipMemGetInfo through torch.cuda.mem_get_info,
    which sees the library's hipMalloc as well as torch's) over a call of the reserved size and two smaller ones: it shrinks by no more than torch's
    own allocator grew for the test's buffers.  The reservation changes no result (a fresh handle that allocates on demand gives the same bits)."""
    from ikflow_amd.engine import Engine

    s, robot, lay, sd = _solver("tiny")
    m, k = 300, 64
    _, poses = H.reachable_poses(robot, m, 3)
    poses = poses.float()
    L = H.latents(k * m, lay.dim, 5)
    opt = _opt(n_keep=4, limits=True)

    def run(eng, mm, kk):
        return _rank(eng, poses[:mm], None, kk, opt, latent=L[:kk * mm])

    eng = Engine(s.layout, robot, DEV)
    eng.load_state_dict(s._state_dict_np)
    eng.reserve_ranked(m, k)
    assert eng.rank_chunks(m, k) > 1 and eng._h.value
    torch.cuda.synchronize()
    run(eng, 8, 4)                                                     # (torch's caching allocator warm for the test's own buffers)
    torch.cuda.synchronize()
    free0, stat0 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    full = run(eng, m, k)
    run(eng, 100, 50)
    run(eng, 1, 64)
    torch.cuda.synchronize()
    free1, stat1 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    grown_by_torch = stat1 - stat0                                     # (the guarded windows of the larger calls come from torch)
    assert free0 - free1 <= grown_by_torch, f"the engine allocated {free0 - free1 - grown_by_torch} bytes after ikf_reserve_ranked"
    fresh = Engine(s.layout, robot, DEV)
    fresh.load_state_dict(s._state_dict_np)
    assert all(H.same_bits(full[n], v) for n, v in run(fresh, m, k).items())   # (the reservation changes no result)


# ---- 7. the grow-only buffers of the candidate stage, shared by ranked / path / diverse IK --------------------------------------------------
def test_candidate_buffers_regrow_across_families_and_are_released_with_the_handle():
    """One engine takes, for ranked, path and diverse IK in turn, a small call (m = 3, k = 5: one chunk), then one that regrows every buffer of
    the candidate stage and uses the partial lists (m = 70, k = 130), then the small call again - interleaved, so the candidate rows and lists
    one family grew are what the next one finds.  Every result has the bits of the same call on a fresh engine.  Path IK runs without node costs
    and with a shared latent, diverse-of-K without row scores, so the handle's own node, back-pointer, latent and score arrays are in use.
    Then the engine goes, and the device's free memory (the accounting of the three reserve tests) is back to what it was before the engine was
    created, up to what torch's own cache grew.  That baseline is taken after the fresh engines of the references are gone: what the runtime
    loads once, with the first launch of a kernel, is not the engine's."""
    import gc

    from ikflow_amd.engine import Engine

    s, robot, lay, sd = _solver("tiny")
    sizes = [(3, 5), (70, 130), (3, 5)]
    _, poses = H.reachable_poses(robot, 70, 3)
    poses = poses.float().to(DEV)
    L = H.latents(130 * 70, lay.dim, 5).to(DEV)

    def engine():
        eng = Engine(s.layout, robot, DEV)
        eng.load_state_dict(s._state_dict_np)
        return eng

    def ranked(eng, m, k):
        return eng.generate_ranked(poses[:m], k, L[:k * m], True, eng.rank_options(n_keep=4, reject_limits=True), row_scores=True)

    def path(eng, m, k):
        return eng.generate_path(poses[:m], k, L[:k], True, True, eng.path_options(reject_limits=True))

    def diverse(eng, m, k):
        return eng.generate_diverse(poses[:m], k, L[:k * m], True, eng.diverse_options(n_keep=4, min_separation=0.05))

    def bits(outs):
        torch.cuda.synchronize()
        return [None if t is None else t.cpu().numpy() for t in outs]

    families = (ranked, path, diverse)
    want = {}
    for call in families:
        for m, k in sizes[:2]:
            fresh = engine()
            want[call, m, k] = bits(call(fresh, m, k))
            del fresh
    gc.collect()
    torch.cuda.synchronize()
    free0, stat0 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    eng = engine()
    assert eng.rank_chunks(3, 5) == 1 and eng.rank_chunks(70, 130) > 1
    for m, k in sizes:
        for call in families:
            got = bits(call(eng, m, k))
            assert len(got) == len(want[call, m, k])
            for i, (g, w) in enumerate(zip(got, want[call, m, k])):
                assert (g is None and w is None) or H.same_bits(g, w), f"{call.__name__} m={m} k={k}: output {i} differs from a fresh engine's"
    del eng
    gc.collect()
    torch.cuda.synchronize()
    free1, stat1 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    assert free0 - free1 <= stat1 - stat0, f"{free0 - free1 - (stat1 - stat0)} bytes of device memory did not come back with the handle"


# ---- 8. every capsule count: the LDS slices of k_rank_candidates on both sides of its 48 KiB opt-in --------------------------------------------
@pytest.fixture
def _small_model_back():
    """The engines are shared with the other test modules: after a test that set another capsule model, the small one is back."""
    used = []
    yield used
    for which in used:
        _eng(which, collisions=True)


def _eng_with(which, model, used, every_pair=False):
    """The shared engine of the chain with capsule model `model` of rank_helpers.capsule_models; every_pair: with all n (n - 1) / 2 pairs listed,
    same-frame ones included, instead of the pairs Robot.set_collision_capsules generates."""
    from ikflow_amd.engine import kinematics_engine_for

    robot = H.kin_robots(which)[0]
    eng = kinematics_engine_for(robot, DEV)
    robot.set_collision_capsules(RH.capsules(which, model))
    folded, pairs = robot._collision_model
    eng.set_collision_model(folded, RH.all_pairs(len(folded)) if every_pair else pairs)
    eng._collision_source = None if every_pair else robot._collision_model
    used.append(which)
    return eng


def _check_the_straddle(model, m, n_keep, lds, world=False):
    """The call of the count below a crossing of the opt-in line stays at or under 49152 B, the call of the count above exceeds it."""
    for below, above, tile, keep, w in RH.CROSSINGS:
        if (tile, keep, w) == (RH.tile_poses(m), RH.keep_capacity(n_keep), world):
            if model == below:
                assert lds <= RH.LDS_OPT_IN, (model, lds)
            if model == above:
                assert lds > RH.LDS_OPT_IN, (model, lds)


def test_the_crossings_of_the_opt_in_line_are_where_the_models_stand():
    """From the formula of rank_kernels.hip alone: each crossing named in rank_helpers.CROSSINGS lies between two models of CAPSULE_COUNTS that are
    one capsule apart, the shapes of the capsule cases have the tile and capacity of a crossing, and 24 capsules give the documented maxima."""
    for below, above, tile, keep, world in RH.CROSSINGS:
        nb, na = int(below[4:]), int(above[4:])
        assert na == nb + 1 and nb in RH.CAPSULE_COUNTS and na in RH.CAPSULE_COUNTS
        m = 1 if tile == 1 else 33
        assert RH.tile_poses(m) == tile
        assert RH.rank_lds_bytes(m, keep, nb, world) <= RH.LDS_OPT_IN < RH.rank_lds_bytes(m, keep, na, world)
    for shape in ("tile1", "tile64", "chunked"):
        m, k, n_keep = RH.CASE_SHAPES[shape]
        assert (RH.tile_poses(m), RH.keep_capacity(n_keep)) == ((1, 1) if shape == "tile1" else (64, 16)) and n_keep <= k
    assert RH.rank_lds_bytes(64, 16, 24) == 82688 and RH.rank_lds_bytes(64, 16, 24, world=True) == 86784
    assert RH.rank_lds_bytes(64, 16, 5) < RH.LDS_OPT_IN // 2   # (the small model of every earlier test is nowhere near the line)


CAPSULE_CASES = [(w, mo, sh) for w in RH.CASE_CHAINS for mo in RH.REJECTING for sh in ("tile1", "tile64")] + \
                [(w, "caps14", "chunked") for w in RH.CASE_CHAINS] + [("panda", "caps24", "chunked")]


@pytest.mark.parametrize("which,model,shape", CAPSULE_CASES)
def test_row_scores_and_selection_with_every_capsule_count(which, model, shape, _small_model_back):
    """reject_collisions with 5, 11 .. 16 and 24 capsules on chains of 4, 7 and 8 joints, min_clearance the median of the fp64 clearances: row
    scores by check_row_scores, the selection bit for bit.  tile1: tile 1, capacity 1; tile64: tile 64, capacity 16; chunked: two chunks, keep 16
    (with 14 capsules, and on the Panda with 24: the documented maximum of 82688 B).  The LDS bytes of the call come from the kernel's formula:
    the count below a crossing stays under the opt-in line, the count above is over it."""
    orob = H.kin_robots(which)[1]
    c = RH.capsule_case(which, model, shape)
    m, k, n_keep = c["m"], c["k"], c["n_keep"]
    caps = RH.capsules(which, model)
    eng = _eng_with(which, model, _small_model_back)
    lds = RH.rank_lds_bytes(m, n_keep, len(caps))
    _check_the_straddle(model, m, n_keep, lds)
    assert eng.rank_chunks(m, k) == (2 if shape == "chunked" else 1)
    if model == "caps24" and shape != "tile1":
        assert lds == 82688
    ref = RH.reference(orob, c["poses"], c["q"], k, 0.01, caps=caps, min_clearance=c["min_clearance"], self_clearance=c["clearance"])
    assert RH.shares_hold(ref), RH.shares(ref)
    out = _rank(eng, c["poses"], c["q"], k, _opt(n_keep=n_keep, collisions=True, min_clearance=c["min_clearance"]))
    worst = RH.check_row_scores(out["row_score"], ref, f"{which} {model} {shape}")
    print(f"{which} {model} {shape}: {lds} B of LDS, worst {worst:.3f} of eps, shares (near, inadmissible) {RH.shares(ref)}")
    _check_selection(out, c["q"], m, k, n_keep, f"{which} {model} {shape}")


@pytest.mark.parametrize("which", RH.CASE_CHAINS)
def test_every_pair_of_24_capsules_rejects_at_least_what_the_generated_pairs_reject(which, _small_model_back):
    """All 276 pairs listed, same-frame ones included (the longest pair loop).  The oracle skips same-frame pairs, so its clearance is an upper
    bound: every row it surely rejects is rejected, no row is admitted that the generated pairs reject, and a row that is admitted keeps its
    score.  (The clearance of a same-frame pair does not depend on q; where such a pair lies under the threshold every row is rejected.)  With a
    threshold no pair can reach - the radii are 15 mm at most - the long loop rejects nothing and every output has the bits of the short one's."""
    c = RH.capsule_case(which, "caps24", "tile64")
    m, k, n_keep = c["m"], c["k"], c["n_keep"]
    for thr in (c["min_clearance"], -1.0):
        opt = _opt(n_keep=n_keep, collisions=True, min_clearance=thr)
        generated = _rank(_eng_with(which, "caps24", _small_model_back), c["poses"], c["q"], k, opt)
        every = _rank(_eng_with(which, "caps24", _small_model_back, every_pair=True), c["poses"], c["q"], k, opt)
        surely_rejected = c["clearance"] < thr - 1e-4
        assert np.isposinf(every["row_score"][surely_rejected]).all() and surely_rejected.any() == (thr > -1.0)
        assert (np.isposinf(every["row_score"]) | ~np.isposinf(generated["row_score"])).all()   # (more pairs never admit a row)
        both = np.isfinite(every["row_score"])
        assert H.same_bits(every["row_score"][both], generated["row_score"][both])
        _check_selection(every, c["q"], m, k, n_keep, f"{which} every pair")
    assert both.all() and all(H.same_bits(every[n], generated[n]) for n in OUTPUTS)


@pytest.mark.parametrize("model", ["caps0", "caps1"])
@pytest.mark.parametrize("which", RH.CASE_CHAINS)
def test_a_model_without_pairs_rejects_nothing(which, model, _small_model_back):
    """No capsule (a slice of one float per thread) and one capsule (no pair): with reject_collisions the kernel takes the collision branch, and
    every output has the bits of the same call without the rule - on every shape of the capsule cases, with limits rejected so that lists differ."""
    orob = H.kin_robots(which)[1]
    eng = _eng_with(which, model, _small_model_back)
    for shape, (m, k, n_keep) in RH.CASE_SHAPES.items():
        poses, q, q_ref = RH.candidates(orob, m, k, seed=3, wild=True)
        without = _rank(eng, poses, q, k, _opt(n_keep=n_keep, limits=True, ref_weight=0.05), q_ref)
        with_rule = _rank(eng, poses, q, k, _opt(n_keep=n_keep, limits=True, ref_weight=0.05, collisions=True, min_clearance=0.05), q_ref)
        assert all(H.same_bits(with_rule[n], without[n]) for n in OUTPUTS), (which, model, shape)
        assert 0 < np.isposinf(without["row_score"]).sum() < k * m
        _check_selection(with_rule, q, m, k, n_keep, f"{which} {model} {shape}")


# ---- 9. the tile widths, keep counts and chains the selection had not met ---------------------------------------------------------------------
# (m, k): every pose count of 2, 9, 16, 17, 32 and 33 with a k that runs in one chunk and a k that runs in several
WIDTH_SHAPES = [(2, 40), (2, 1009), (9, 12), (9, 200), (16, 20), (16, 150), (17, 12), (17, 100), (32, 12), (32, 70), (33, 7), (33, 40)]


def test_the_width_shapes_hold_every_width_with_one_chunk_and_with_several():
    eng = _eng("panda")
    seen = {(RH.tile_poses(m), eng.rank_chunks(m, k) > 1) for m, k in WIDTH_SHAPES}
    print("tile width and chunks per (m, k):", {s: (RH.tile_poses(s[0]), eng.rank_chunks(*s)) for s in WIDTH_SHAPES})
    for width in (2, 16, 32, 64):
        assert (width, False) in seen and (width, True) in seen, (width, seen)
    for m in (2, 9, 16, 17, 32, 33):
        chunked = {eng.rank_chunks(mm, k) > 1 for mm, k in WIDTH_SHAPES if mm == m}
        assert chunked == {False, True}, (m, chunked)
    assert [RH.tile_poses(m) for m in (1, 2, 3, 9, 16, 17, 32, 33, 64, 65)] == [1, 2, 4, 16, 16, 32, 32, 64, 64, 64]


@pytest.mark.parametrize("m,k", WIDTH_SHAPES)
def test_selection_at_the_widths_2_16_and_32(m, k):
    """The check of test_selection_equals_the_lexsort_of_the_engines_row_scores at the widths whose __shfl_xor steps and wave hand-over had not
    run, for every capacity and for keep counts strictly inside one (2, 3, 5, 15)."""
    orob = H.kin_robots("panda")[1]
    eng = _eng("panda")
    poses, q, _ = RH.candidates(orob, m, k, seed=m + k)
    for n_keep in sorted({min(n, k) for n in (1, 2, 3, 4, 5, 15, 16)}):
        out = _rank(eng, poses, q, k, _opt(n_keep=n_keep, max_pos=0.03, limits=True))
        _check_selection(out, q, m, k, n_keep, f"m {m} k {k} n_keep {n_keep}")
    if k >= 40:
        assert (out["count"] < k).any() and (out["count"] > 0).any()


@pytest.mark.parametrize("m,k", [(2, 1009), (3, 1009), (64, 65), (257, 50)])
def test_keep_counts_inside_a_capacity_class_on_chunked_shapes(m, k):
    """n_keep 2, 3, 5 and 15: the partial lists of a chunk have stride n_keep while the register list holds 4 or 16 entries.  k = 1009 is prime,
    so the last chunk is shorter than the others."""
    orob = H.kin_robots("panda")[1]
    eng = _eng("panda")
    chunks = eng.rank_chunks(m, k)
    assert chunks > 1 and (k != 1009 or k % -(-k // chunks) != 0)
    poses, q, _ = RH.candidates(orob, m, k, seed=m + k)
    for n_keep in (2, 3, 5, 15):
        out = _rank(eng, poses, q, k, _opt(n_keep=n_keep, max_pos=0.03, limits=True))
        _check_selection(out, q, m, k, n_keep, f"m {m} k {k} n_keep {n_keep}")
    assert (out["count"] < k).any() and (out["count"] > 0).any()


@pytest.mark.parametrize("which", ["syn4p", "syn5r", "syn6p", "syn8r"])
def test_chunked_selection_on_chains_of_4_5_6_and_8_joints(which):
    """Exact selection over several chunks, without capsules, on the chain sizes that had met it only with keep counts 1, 4 and 16."""
    orob = H.kin_robots(which)[1]
    eng = _eng(which)
    for m, k in ((3, 1009), (65, 64)):
        assert eng.rank_chunks(m, k) > 1
        poses, q, _ = RH.candidates(orob, m, k, seed=m + k)
        for n_keep in (1, 3, 4, 15, 16):
            out = _rank(eng, poses, q, k, _opt(n_keep=n_keep, max_pos=0.03, limits=True))
            _check_selection(out, q, m, k, n_keep, f"{which} m {m} k {k} n_keep {n_keep}")
        assert (out["count"] < k).any() and (out["count"] > 0).any()


# (m, k, n_keep): one chunk each; the second wave of the workgroup holds at least n_keep of the k repeats of a pose
SECOND_WAVE_SHAPES = [(1, 200, 16), (2, 100, 16), (3, 80, 16), (5, 100, 16), (9, 40, 16), (16, 60, 15), (17, 12, 4), (33, 12, 4), (64, 9, 4), (1, 130, 1)]


@pytest.mark.parametrize("m,k,n_keep", SECOND_WAVE_SHAPES)
def test_a_list_whose_every_entry_comes_from_the_second_wave(m, k, n_keep):
    """The n_keep best candidates of every pose are 1 mm-scale perturbations of the truth placed at repeats that threads of the second wave own
    (repeat r belongs to slice r mod S, S = 128 / tile_poses; the slices S / 2 .. S - 1 are the second wave's); all the others are 0.3 rad off.
    Then every entry of the result, the last one of a full register list included, has crossed the LDS hand-over between the waves."""
    orob = H.kin_robots("panda")[1]
    eng = _eng("panda")
    assert eng.rank_chunks(m, k) == 1
    S = 128 // RH.tile_poses(m)
    second = [r for r in range(k) if r % S >= S // 2][:n_keep]
    assert len(second) == n_keep
    g = torch.Generator().manual_seed(m + k)
    q_true, poses = H.reachable_poses(orob, m, 70 + m)
    scale = torch.full((k,), 0.3)
    scale[second] = 1e-3 * (1.0 + torch.rand(n_keep, generator=g))
    from oracle import kinematics_oracle as ko

    q = ko.clamp_to_joint_limits(orob, (q_true[None] + torch.randn(k, m, orob.ndof, generator=g) * scale[:, None, None]).reshape(k * m, -1)).float().contiguous()
    out = _rank(eng, poses.float().contiguous(), q, k, _opt(n_keep=n_keep))
    _check_selection(out, q, m, k, n_keep, f"m {m} k {k} n_keep {n_keep}")
    assert (np.sort(out["index"], axis=1) == np.array(second)).all(), "the best candidates are not the ones placed in the second wave"
