"""Diverse-of-K IK on the GPU (include/ikflow_amd_diverse.h; ikflow_amd/csrc/diverse_kernels.hip, diverse_math.h, api_diverse.hip): the selection
against sequential numpy float32 arithmetic on the engine's own row scores (bit for bit: every step of it is rounded on its own), the row scores
and slot 0 against the ranking (the same kernel), independence of the batch, buffers and null outputs, the flow + selection call against
generate_ik_solutions + ikf_diverse_select, ikf_reserve_diverse, status codes, and IKFlowSolver.generate_diverse_ik_solutions end to end.

Every call goes through _div(): outputs are windows inside sentinel-filled buffers with guard rows in front and behind (the scheme of
tests/test_ranked.py), so every test also checks that nothing outside is written and everything inside is.  What is tested is the arithmetic and
the selection; the weights are synthetic, so nothing here says how far apart the solution families of a trained model are."""
import ctypes as C

import numpy as np
import pytest
import torch

import diverse_helpers as DH
import helpers as H
import rank_helpers as RH
from ikflow_amd import _lib
from test_ranked import DEV, GUARD, _check_window, _eng, _eng_with, _opt as _rank_opt, _rank, _small_model_back, _solver, _window  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
OUTPUTS = ("q_out", "score", "index", "sep", "kept", "count", "row_score")
NULLABLE = ("score", "sep", "kept", "count", "row_score")


def _dopt(n_keep=1, rot_weight=0.01, max_pos=None, max_rot=None, limits=False, collisions=False, min_clearance=0.0, min_sep=0.0):
    return _lib.ikf_diverse_options(n_keep, rot_weight, -1.0 if max_pos is None else max_pos, -1.0 if max_rot is None else max_rot, int(limits),
                                    int(collisions), min_clearance, min_sep)


def _div(eng, poses, q, k, opt, w=None, stream=None, null=(), latent=None, clamp=True, expect=_lib.IKF_OK):
    """ikf_diverse_select (or, with `latent`, ikf_generate_diverse) through eng.lib on guarded buffers -> {name: cpu numpy window}; `null`: the
    nullable outputs passed as null."""
    m, nd, nk = poses.shape[0], eng.layout.ndof, opt.n_keep
    shapes = {"q_out": (m * nk, nd, torch.float32), "score": (m * nk, 1, torch.float32), "index": (m * nk, 1, torch.int32),
              "sep": (m * nk, 1, torch.float32), "kept": (m, 1, torch.int32), "count": (m, 1, torch.int32), "row_score": (k * m, 1, torch.float32)}
    bufs = {n: _window(*shapes[n]) for n in OUTPUTS if n not in null}
    ptr = [bufs[n][GUARD:].data_ptr() if n in bufs else None for n in OUTPUTS]
    poses_d = poses.to(DEV).contiguous()
    rows_d = (q if latent is None else latent).to(DEV).contiguous()
    w_d = None if w is None else torch.as_tensor(w, dtype=torch.float32).to(DEV).contiguous()
    wp = None if w_d is None else w_d.data_ptr()
    torch.cuda.synchronize()
    s = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(0)
    if latent is None:
        code = eng.lib.ikf_diverse_select(eng._h, poses_d.data_ptr(), m, k, rows_d.data_ptr(), wp, C.byref(opt), *ptr, s)
    else:
        code = eng.lib.ikf_generate_diverse(eng._h, poses_d.data_ptr(), m, k, rows_d.data_ptr(), int(clamp), wp, C.byref(opt), *ptr, s)
    assert code == expect, (code, _lib.last_error(eng.lib))
    torch.cuda.synchronize()
    out = {n: _check_window(b, shapes[n][0], n).cpu().numpy() for n, b in bufs.items()}
    for n in out:
        out[n] = out[n].reshape(m, nk, nd) if n == "q_out" else out[n].reshape(m, nk) if n in ("score", "index", "sep") else out[n].reshape(-1)
    return out


def _same(a, b, names=None):
    return all(DH.same_bits(a[n], b[n]) for n in (names or a))


def _check_against_numpy(out, q, m, k, opt, w=None, what=""):
    """Every output against the numpy float32 selection on the engine's own row scores - no tolerance - and the header's two guarantees."""
    want = DH.select_poses(q.numpy(), out["row_score"], m, k, opt.n_keep, opt.min_separation, w)
    for n in DH.NAMES:
        bad = np.flatnonzero((np.asarray(out[n]).reshape(m, -1).view(np.int32) != np.asarray(want[n]).reshape(m, -1).view(np.int32)).any(1))
        assert bad.size == 0, f"{what}: {n} differs from the numpy selection on poses {bad[:3]}: {out[n][bad[0]]} != {want[n][bad[0]]}"
    qk, sk = q.numpy().reshape(k, m, -1), out["row_score"].reshape(k, m)
    for j in sorted({0, m // 2, m - 1}):
        DH.check_guarantees(qk[:, j], sk[:, j], out["index"][j], out["kept"][j], opt.n_keep, opt.min_separation, w)
    return want


# ---- 1. the selection against sequential numpy float32, on every shape at which the kernel takes another path -------------------------------------
# (k = 512 and 513: k_diverse_select goes from 128 to 256 threads between them)
SHAPES = [(1, 1), (1, 2), (2, 63), (1, 64), (3, 65), (65, 16), (1, 255), (2, 256), (1, 257), (2, 1024), (1, 512), (1, 513)]
ROBOTS = ("panda", "fetch", "fetch_arm", "syn4r", "syn5p", "syn6r", "syn7p", "syn8r")
VARIANTS = ("thresholds", "limits_wild", "collisions", "weights", "early_stop")


@pytest.mark.parametrize("m,k", SHAPES)
def test_selection_equals_sequential_numpy_float32_on_the_engines_row_scores(m, k):
    """Per robot (Panda, Fetch, FetchArm, a synthetic chain per ndof 4 .. 8): the plain options with n_keep 1 / 2 / 16 where k allows, and one of
    the option sets - thresholds, limits on unclamped rows, capsules, joint weights (one of them 0), a min_separation that stops early - taken in
    turn, so that every set meets every robot and every shape's neighbours; from k = 63 up each set is held to its purpose."""
    si = SHAPES.index((m, k))
    for ri, which in enumerate(ROBOTS):
        robot, orob = H.kin_robots(which)
        variant = VARIANTS[(si + ri) % len(VARIANTS)]
        eng = _eng(which, collisions=variant == "collisions")
        poses, q, _ = RH.candidates(orob, m, k, seed=m + k)
        nks = [n for n in (1, 2, 16) if n <= k]
        for nk in nks:
            out = _div(eng, poses, q, k, _dopt(nk))
            _check_against_numpy(out, q, m, k, _dopt(nk), what=f"{which} m {m} k {k} n_keep {nk}")
            assert (out["count"] == k).all() and (out["kept"] == nk).all()
        nk, w, v = nks[-1], None, {}
        if variant == "thresholds":
            v = dict(max_pos=0.03, max_rot=0.5)
        elif variant == "limits_wild":
            poses, q, _ = RH.candidates(orob, m, k, seed=m + k, wild=True)
            v = dict(limits=True)
        elif variant == "collisions":
            v = dict(collisions=True, min_clearance=RH.clearance_threshold(orob, RH.collision_capsules(robot), q))
        elif variant == "weights":
            w = np.linspace(0.0, 2.0, orob.ndof).astype(np.float32)
        elif variant == "early_stop":
            seps = out["sep"][:, 1:][np.isfinite(out["sep"][:, 1:])]
            if seps.size == 0:
                continue
            v = dict(min_sep=float(np.median(seps)))
        opt = _dopt(nk, **v)
        got = _div(eng, poses, q, k, opt, w)
        _check_against_numpy(got, q, m, k, opt, w, what=f"{which} m {m} k {k} {variant}")
        if k >= 63:   # (large enough for every option set to bite; below that it may or may not)
            if variant in ("thresholds", "limits_wild", "collisions"):
                assert (got["count"] < k).any() and (got["count"] > 0).any(), f"{which} {variant} rejects nothing or everything"
            elif variant == "early_stop":
                assert (got["kept"] < np.minimum(got["count"], nk)).any(), f"{which}: min_separation {opt.min_separation} stops no pose early"
            else:
                assert not DH.same_bits(got["index"], out["index"]), f"{which}: the weights change no pick"


# ---- 2. the row scores and slot 0 are the ranking's ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,m,k", [("panda", 65, 16), ("fetch", 2, 1024), ("syn5p", 3, 65)])
def test_row_scores_and_slot_0_are_the_rankings(which, m, k):
    """d_row_score_out bit-equal to ikf_rank_candidates' row_score_out of the same rows and options, count_out to its count, slot 0 to its
    n_keep = 1 result - with thresholds and limits on unclamped rows, and with capsules."""
    robot, orob = H.kin_robots(which)
    eng = _eng(which, collisions=True)
    poses, q, _ = RH.candidates(orob, m, k, seed=7, wild=True)
    cl = RH.clearance_threshold(orob, RH.collision_capsules(robot), q)
    for v in (dict(max_pos=0.05, max_rot=1.0, limits=True), dict(collisions=True, min_clearance=cl), dict(rot_weight=1.0)):
        out = _div(eng, poses, q, k, _dopt(min(k, 4), **v))
        r = _rank(eng, poses, q, k, _rank_opt(1, v.get("rot_weight", 0.01), 0.0, v.get("max_pos"), v.get("max_rot"), v.get("limits", False),
                                              v.get("collisions", False), v.get("min_clearance", 0.0)))
        assert DH.same_bits(out["row_score"], r["row_score"]), "row scores differ from ikf_rank_candidates' of the same rows"
        assert np.array_equal(out["count"], r["count"])
        assert DH.same_bits(out["index"][:, :1], r["index"]) and DH.same_bits(out["score"][:, :1], r["score"]) and DH.same_bits(out["q_out"][:, :1], r["q_out"])
        assert np.isposinf(out["sep"][:, 0]).all()
        if "rot_weight" not in v:
            assert 0 < int(np.isinf(out["row_score"]).sum()) < k * m


# ---- 3. a pose alone and inside a batch -----------------------------------------------------------------------------------------------------------
def test_a_pose_alone_equals_the_pose_as_number_64_of_65():
    orob = H.kin_robots("panda")[1]
    eng = _eng("panda")
    m, k = 65, 100
    poses, q, _ = RH.candidates(orob, m, k, seed=17, wild=True)
    w = np.array([1.0, 0.5, 2.0, 1.0, 0.0, 1.0, 3.0], np.float32)
    opt = _dopt(16, max_pos=0.08, limits=True, min_sep=0.3)
    full = _div(eng, poses, q, k, opt, w)
    _check_against_numpy(full, q, m, k, opt, w, what="batch of 65")
    for j in (64, 0):
        alone = _div(eng, poses[j:j + 1], q.reshape(k, m, -1)[:, j].contiguous(), k, opt, w)
        assert DH.same_bits(alone["row_score"], full["row_score"].reshape(k, m)[:, j])
        assert all(DH.same_bits(alone[n][0], full[n][j]) for n in ("q_out", "score", "index", "sep", "kept", "count")), j


# ---- 4. buffers: hand-made poses, null outputs, another stream ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [6, 300])
def test_hand_made_poses_fill_every_slot(k):
    """Pose 0: every candidate the same row (ties: indices 0 .. n_keep - 1, separations 0; with a positive min_separation only slot 0).  Pose 1: all
    inadmissible.  Pose 2: exactly one admissible, the last candidate.  Pose 3: a NaN row among ordinary ones.  Pose 4: ordinary.  Every element
    of every output is written (the windows' sentinels are gone), unfilled slots hold 0 / +inf / -1 / +inf."""
    orob = H.kin_robots("panda")[1]
    eng = _eng("panda")
    m, nd, nk = 5, orob.ndof, 6
    poses, q, _ = RH.candidates(orob, m, k, seed=9, lo_exp=-3.0, hi_exp=-1.0)
    lo, hi = RH.limits(orob)
    q = q.reshape(k, m, nd).clone()
    q[:, 0] = q[0, 0]
    q[:, 1] = hi + 0.5
    q[:, 2] = hi + 0.5
    q[k - 1, 2] = 0.5 * (lo + hi)
    q[3, 3] = float("nan")
    q = q.reshape(k * m, nd).contiguous()
    for sep in (0.0, 1e-3):
        opt = _dopt(nk, limits=True, min_sep=sep)
        out = _div(eng, poses, q, k, opt)
        _check_against_numpy(out, q, m, k, opt, what=f"hand-made k {k} min_separation {sep}")
        assert list(out["count"]) == [k, 0, 1, k - 1, k]
        assert list(out["kept"][1:3]) == [0, 1] and out["kept"][0] == (nk if sep == 0.0 else 1)
        assert list(out["index"][0]) == (list(range(nk)) if sep == 0.0 else [0] + [-1] * (nk - 1))
        assert (out["sep"][0, 1:] == (0.0 if sep == 0.0 else np.inf)).all()
        assert (out["index"][1] == -1).all() and (out["q_out"][1] == 0).all() and np.isposinf(out["score"][1]).all() and np.isposinf(out["sep"][1]).all()
        assert list(out["index"][2]) == [k - 1] + [-1] * (nk - 1) and 3 not in out["index"][3] and np.isfinite(out["q_out"][3]).all()


def test_null_outputs_and_a_non_default_stream():
    orob = H.kin_robots("syn6p")[1]
    eng = _eng("syn6p")
    for m, k in ((65, 50), (3, 1000)):
        poses, q, _ = RH.candidates(orob, m, k, seed=2)
        opt = _dopt(8, max_pos=0.05, min_sep=0.2)
        ref = _div(eng, poses, q, k, opt)
        got = _div(eng, poses, q, k, opt, stream=torch.cuda.Stream(device=DEV))
        assert _same(ref, got)
        for null in [(n,) for n in NULLABLE] + [NULLABLE]:
            got = _div(eng, poses, q, k, opt, null=null)
            assert set(got) == set(OUTPUTS) - set(null) and _same(got, ref, got)


# ---- 5. flow + selection -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k", [(8, 64), (1, 257)])
@pytest.mark.parametrize("model", ["tiny", "panda"])
def test_flow_and_selection_in_one_call(model, m, k):
    """ikf_generate_diverse == generate_ik_solutions on the tiled poses followed by ikf_diverse_select: every output bit for bit (and so, through
    the checks above, the numpy selection on the flow's own rows)."""
    s, robot, lay, sd = _solver(model)
    eng = s.engine(DEV)
    _, poses = H.reachable_poses(robot, m, 11)
    poses = poses.float()
    L = H.latents(k * m, lay.dim, 12)
    w = np.linspace(0.5, 1.5, robot.ndof).astype(np.float32)
    opt = _dopt(16, limits=True, min_sep=0.05)
    one = _div(eng, poses, None, k, opt, w, latent=L)
    rows = s.generate_ik_solutions(poses.to(DEV).repeat((k, 1)), latent=L.to(DEV)).cpu()
    two = _div(eng, poses, rows, k, opt, w)
    assert _same(one, two)
    _check_against_numpy(one, rows, m, k, opt, w, what=f"{model} m {m} k {k}")
    unclamped = _div(eng, poses, None, k, opt, w, latent=L, clamp=False)
    assert (unclamped["count"] <= one["count"]).all()


# ---- 6. ikf_reserve_diverse ----------------------------------------------------------------------------------------------------------------------
def test_after_reserve_diverse_a_call_of_that_size_allocates_nothing():
    """The handle's buffer pointers are not visible through the C-ABI, so - as tests/test_ranked.py checks ikf_reserve_ranked - what is checked is
    the device's free memory over a call of the reserved size, with and without d_row_score_out, and two smaller ones: it shrinks by no more than
    torch's own allocator grew for the test's buffers (a buffer that had to grow would be freed and allocated anew).  The limit of this check: a
    buffer freed and allocated again at the SAME size leaves the free memory where it was and would pass unnoticed; the ensure_* functions
    return before they free anything when the capacity suffices, which only reading the code shows.  The reservation changes no result."""
    from ikflow_amd.engine import Engine

    s, robot, lay, sd = _solver("tiny")
    m, k = 40, 1024
    _, poses = H.reachable_poses(robot, m, 3)
    poses = poses.float()
    L = H.latents(k * m, lay.dim, 5)
    opt = _dopt(16, limits=True)

    def run(eng, mm, kk, null=()):
        lat = L.reshape(k, m, -1)[:kk, :mm].reshape(kk * mm, -1).contiguous()
        return _div(eng, poses[:mm], None, kk, opt, latent=lat, null=null)

    eng = Engine(s.layout, robot, DEV)
    eng.load_state_dict(s._state_dict_np)
    eng.reserve_diverse(m, k)
    torch.cuda.synchronize()
    run(eng, 2, 16)                                                    # (torch's caching allocator warm for the test's own buffers)
    torch.cuda.synchronize()
    free0, stat0 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    full = run(eng, m, k)
    run(eng, m, k, null=("row_score",))
    run(eng, 30, 50)
    run(eng, 1, 64, null=("row_score",))
    torch.cuda.synchronize()
    free1, stat1 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    grown_by_torch = stat1 - stat0                                     # (the guarded windows of the larger calls come from torch)
    assert free0 - free1 <= grown_by_torch, f"the engine allocated {free0 - free1 - grown_by_torch} bytes after ikf_reserve_diverse"
    fresh = Engine(s.layout, robot, DEV)
    fresh.load_state_dict(s._state_dict_np)
    assert _same(full, run(fresh, m, k))                               # (the reservation changes no result)


# ---- 7. status codes -------------------------------------------------------------------------------------------------------------------------------
def test_status_codes_and_untouched_outputs():
    from ikflow_amd.engine import Engine

    orob = H.kin_robots("panda")[1]
    eng = _eng("panda")
    lib, h = eng.lib, eng._h
    m, k, nk = 4, 5, 2
    poses, q, _ = RH.candidates(orob, m, k, seed=1)
    P, Q = poses.to(DEV), q.to(DEV)
    q_out = torch.full((m * nk, 7), 7.0, device=DEV)
    index = torch.full((m * nk,), 7, dtype=torch.int32, device=DEV)
    opt = _dopt(nk)
    call = lambda h_, p, n, k_, q_, o, qo, io: lib.ikf_diverse_select(h_, p, n, k_, q_, None, o, qo, None, io, None, None, None, None, None)
    ok = (h, P.data_ptr(), m, k, Q.data_ptr(), C.byref(opt), q_out.data_ptr(), index.data_ptr())
    nan = float("nan")
    bad = [
        ((None,) + ok[1:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:1] + (None,) + ok[2:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:4] + (None,) + ok[5:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:5] + (None,) + ok[6:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:6] + (None,) + ok[7:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:7] + (None,), _lib.IKF_ERR_NULL_POINTER),
        (ok[:2] + (-1,) + ok[3:], _lib.IKF_ERR_BAD_ARGUMENT),
        (ok[:3] + (0,) + ok[4:], _lib.IKF_ERR_BAD_ARGUMENT),
        (ok[:3] + (1025,) + ok[4:], _lib.IKF_ERR_BAD_ARGUMENT),
        (ok[:2] + (2 ** 21, 1024) + ok[4:], _lib.IKF_ERR_BAD_ARGUMENT),                     # k * n_poses = 2^31
        (ok[:5] + (C.byref(_dopt(0)),) + ok[6:], _lib.IKF_ERR_BAD_ARGUMENT),
        (ok[:5] + (C.byref(_dopt(k + 1)),) + ok[6:], _lib.IKF_ERR_BAD_ARGUMENT),
        (ok[:3] + (64,) + ok[4:5] + (C.byref(_dopt(17)),) + ok[6:], _lib.IKF_ERR_BAD_ARGUMENT),
        (ok[:5] + (C.byref(_dopt(nk, min_sep=-0.5)),) + ok[6:], _lib.IKF_ERR_BAD_ARGUMENT),
        (ok[:5] + (C.byref(_dopt(nk, min_sep=nan)),) + ok[6:], _lib.IKF_ERR_BAD_ARGUMENT),
    ]
    for args, code in bad:
        assert call(*args) == code, (args, code)
    fresh = Engine(eng.layout, eng.robot, DEV)                                              # (no collision model, no weights)
    assert call(fresh._h, *ok[1:5], C.byref(_dopt(nk, collisions=True)), *ok[6:]) == _lib.IKF_ERR_BAD_ARGUMENT
    lat = torch.zeros(k * m, eng.layout.dim, device=DEV)
    gen = lambda h_, o=opt, qo=q_out, lt=lat: lib.ikf_generate_diverse(h_, P.data_ptr(), m, k, None if lt is None else lt.data_ptr(), 1, None, C.byref(o),
                                                                       None if qo is None else qo.data_ptr(), None, index.data_ptr(), None, None, None, None, None)
    assert gen(fresh._h) == _lib.IKF_ERR_NOT_LOADED and gen(None) == _lib.IKF_ERR_NULL_POINTER
    s = _solver("tiny")[0]
    loaded = s.engine(DEV)
    assert gen(loaded._h, qo=None) == _lib.IKF_ERR_NULL_POINTER and gen(loaded._h, lt=None) == _lib.IKF_ERR_NULL_POINTER
    assert gen(loaded._h, o=_dopt(k + 1)) == _lib.IKF_ERR_BAD_ARGUMENT and gen(loaded._h, o=_dopt(nk, min_sep=-1.0)) == _lib.IKF_ERR_BAD_ARGUMENT
    assert call(h, None, 0, k, None, C.byref(opt), None, None) == _lib.IKF_OK               # nothing to do: null buffers are fine
    for args in ((None, 4, 4), (fresh._h, 0, 4), (fresh._h, 4, 0), (fresh._h, 4, 1025), (fresh._h, 2 ** 21, 1024)):
        assert lib.ikf_reserve_diverse(*args) == (_lib.IKF_ERR_NULL_POINTER if args[0] is None else _lib.IKF_ERR_BAD_ARGUMENT)
    assert lib.ikf_reserve_diverse(fresh._h, 100, 50) == _lib.IKF_OK
    torch.cuda.synchronize()
    assert (q_out == 7.0).all() and (index == 7).all()                                      # none of the refused calls touched an output
    assert call(*ok) == _lib.IKF_OK
    torch.cuda.synchronize()
    assert (index >= 0).all() and (index < k).all() and torch.isfinite(q_out).all()


# ---- 8. the Python method ------------------------------------------------------------------------------------------------------------------------------
def test_generate_diverse_ik_solutions_end_to_end():
    s, robot, lay, sd = _solver("tiny")
    eng = s.engine(DEV)
    m, k, nk = 33, 40, 5
    _, poses = H.reachable_poses(robot, m, 21)
    y = poses.float().to(DEV)
    L = H.latents(k * m, lay.dim, 22).to(DEV)
    w = torch.linspace(0.5, 2.0, robot.ndof)
    got = s.generate_diverse_ik_solutions(y, k, nk, min_separation=0.1, joint_weights=w, latent=L, return_row_scores=True)
    assert got._fields == ("solutions", "scores", "repeat_index", "separation", "n_kept", "n_admissible", "row_scores")
    assert got.solutions.shape == (m, nk, robot.ndof) and got.scores.shape == got.separation.shape == got.repeat_index.shape == (m, nk)
    assert got.repeat_index.dtype == got.n_kept.dtype == got.n_admissible.dtype == torch.int32 and got.row_scores.shape == (k * m,)
    rows = s.generate_ik_solutions(y.repeat((k, 1)), latent=L).cpu()
    out = {"q_out": got.solutions.cpu().numpy(), "score": got.scores.cpu().numpy(), "index": got.repeat_index.cpu().numpy(),
           "sep": got.separation.cpu().numpy(), "kept": got.n_kept.cpu().numpy(), "count": got.n_admissible.cpu().numpy(),
           "row_score": got.row_scores.cpu().numpy()}
    opt = eng.diverse_options(nk, rot_weight=0.01, min_separation=0.1)
    _check_against_numpy(out, rows, m, k, opt, w.numpy(), what="generate_diverse_ik_solutions")
    assert (got.n_kept >= 1).all()
    six = s.generate_diverse_ik_solutions(y, k, nk, min_separation=0.1, joint_weights=w.to(DEV), latent=L)
    assert six._fields == got._fields[:6] and all(torch.equal(a, b) for a, b in zip(six, got[:6]))
    # slot 0 is generate_ranked_ik_solutions' first choice; the same torch seed draws the same latent
    ranked = s.generate_ranked_ik_solutions(y, k, 1, latent=L)
    assert torch.equal(ranked.solutions[:, 0], got.solutions[:, 0]) and torch.equal(ranked.repeat_index[:, 0], got.repeat_index[:, 0])
    torch.manual_seed(77)
    a = s.generate_diverse_ik_solutions(y, k, nk)
    torch.manual_seed(77)
    b = s.generate_diverse_ik_solutions(y, k, nk, latent=torch.randn((k * m, lay.dim), device=DEV))
    assert torch.equal(a.solutions, b.solutions) and torch.equal(a.separation, b.separation)
    single = s.generate_diverse_ik_solutions(y[0], 1024, 16, min_separation=0.5)
    assert single.solutions.shape == (1, 16, robot.ndof) and int(single.n_kept[0]) >= 1
    # nothing admissible: nothing kept
    none = s.generate_diverse_ik_solutions(y, k, nk, latent=L, pos_error_threshold=0.0)
    assert (none.n_kept == 0).all() and (none.n_admissible == 0).all() and (none.repeat_index == -1).all() and (none.solutions == 0).all()
    assert torch.isposinf(none.scores).all() and torch.isposinf(none.separation).all()


# ---- 9. the 24-capsule model, and ties of a farthest-point round across lanes and waves -----------------------------------------------------------
def test_row_scores_with_24_capsules_are_the_rankings(_small_model_back):
    """The score stage under the 24-capsule model (k_rank_candidates with 74240 B of capsule slices): row scores, counts and slot 0 bit-equal to
    ikf_rank_candidates' on the same rows, the selection the numpy selection on them.  min_clearance: the median of the fp64 clearances."""
    which = "panda"
    c = RH.capsule_case(which, "caps24", "tile64")
    m, k = c["m"], c["k"]
    eng = _eng_with(which, "caps24", _small_model_back)
    opt = _dopt(4, collisions=True, min_clearance=c["min_clearance"], min_sep=0.05)
    out = _div(eng, c["poses"], c["q"], k, opt)
    r = _rank(eng, c["poses"], c["q"], k, _rank_opt(1, collisions=True, min_clearance=c["min_clearance"]))
    assert DH.same_bits(out["row_score"], r["row_score"]) and np.array_equal(out["count"], r["count"])
    assert DH.same_bits(out["index"][:, :1], r["index"]) and DH.same_bits(out["score"][:, :1], r["score"]) and DH.same_bits(out["q_out"][:, :1], r["q_out"])
    sure = np.abs(c["clearance"] - c["min_clearance"]) > 1e-4
    assert np.array_equal(np.isposinf(out["row_score"])[sure], (c["clearance"] < c["min_clearance"])[sure]) and 0.1 < np.isposinf(out["row_score"]).mean() < 0.9
    _check_against_numpy(out, c["q"], m, k, opt, what="caps24")


def _tie_case(k, seed):
    """One pose, k candidates on a grid of 2^-8 rad, so that every difference, square and sum of a dist2 is exact in float32.  Row P is the
    configuration whose pose is asked for (the lowest score: slot 0).  Fourteen rows are P +- 0.25 rad along each of the Panda's seven joints:
    pairs mirrored about P.  After any picks among them every one of those still alive has near2 = 0.0625 exactly - its distance to P; to a
    picked row it is 0.125 or 0.25 - so every round is a tie among all of them, and the lowest index must win.  The other rows lie within
    0.0625 rad per joint of P and are never the farthest.  -> (poses, q tile-major, P, the tied indices ascending)."""
    orob = H.kin_robots("panda")[1]
    rng = np.random.default_rng(seed)
    lo, hi = RH.limits(orob)
    mid = (0.5 * (lo + hi)).numpy().astype(np.float64)
    qp = np.round(mid * 256.0) / 256.0
    q = qp[None, :] + rng.integers(-16, 17, (k, 7)) / 256.0
    tied = np.sort(rng.choice(np.arange(1, k), 14, replace=False))
    P = 0
    for i, r in enumerate(rng.permutation(tied)):
        q[r] = qp + (0.25 if i % 2 == 0 else -0.25) * np.eye(7)[i // 2]
    q[P] = qp
    assert (q > lo.numpy() + 0.01).all() and (q < hi.numpy() - 0.01).all() and (q.astype(np.float32) == q).all()
    from oracle import kinematics_oracle as ko

    poses = ko.forward_kinematics(orob, torch.tensor(qp[None])).float().contiguous()
    return poses, torch.tensor(q, dtype=torch.float32).contiguous(), P, tied


@pytest.mark.parametrize("k", [200, 300, 1000])
def test_a_tie_of_a_farthest_point_round_goes_to_the_lower_index_in_whatever_lane_or_wave(k):
    """k = 200: one wave, the tied rows in different lanes (__shfl_xor steps of diverse_merge); k = 300: two waves; k = 1000: four waves, up to
    four candidates per thread.  Candidate r sits in thread r mod B, wave (r mod B) / 64: among the tied rows a lower index sits in a higher
    wave (or lane) than a higher index and the other way round, so neither the order of the lanes nor of the waves gives the right row by
    itself.  Every output bit for bit against DH.select_poses; the picks are the tied indices in ascending order."""
    eng = _eng("panda")
    poses, q, P, tied = _tie_case(k, seed=k)
    B = 64 if k <= 256 else 128 if k <= 512 else 256
    place = (tied % B) // 64 if B > 64 else tied % 64   # wave, or lane within the one wave
    assert len(set(place.tolist())) >= 2 and (np.diff(place) < 0).any() and (np.diff(place) > 0).any()
    n_keep = 12
    opt = _dopt(n_keep)
    out = _div(eng, poses, q, k, opt)
    _check_against_numpy(out, q, 1, k, opt, what=f"tie k {k}")
    assert out["index"][0].tolist() == [P] + tied[:n_keep - 1].tolist(), (out["index"][0], tied)
    assert (out["sep"][0, 1:] == np.float32(0.25)).all() and out["kept"][0] == n_keep and out["count"][0] == k
