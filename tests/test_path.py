"""Path IK on the GPU (include/ikflow_amd_path.h; ikflow_amd/csrc/path_kernels.hip, path_math.h, api_path.hip): the lattice against sequential numpy
float32 arithmetic on the engine's own node costs (bit for bit: every step of the search is rounded on its own), the node costs against the
ranking's row scores (the same function), every chain size (4 .. 8 joints) and every span of the lattice workgroup, ties between slices and waves
(constructed: bit-equal candidates), the "no path" outputs, null outputs, the flow + search call in both latent forms against
generate_ik_solutions + ikf_path_search, status codes, ikf_reserve_path, and IKFlowSolver.generate_ik_path end to end.

Every call goes through _path(): outputs are windows inside sentinel-filled buffers with guard rows in front and behind (the scheme of
tests/test_ranked.py), so every test also checks that nothing outside is written and everything inside is.  What is tested is the arithmetic and
the search; the weights are synthetic, so nothing here says how smooth a path of a trained model is."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H
import path_helpers as PH
import rank_helpers as RH
from ikflow_amd import _lib
from oracle import kinematics_oracle as ko
from test_ranked import DEV, GUARD, _check_window, _eng, _opt as _rank_opt, _rank, _solver, _window

pytestmark = pytest.mark.gpu
CHUNK = PH.backtrack_chunk()
OUTPUTS = ("path", "index", "cost", "reach", "node")


def _popt(rot_weight=0.01, max_pos=None, max_rot=None, limits=False, collisions=False, min_clearance=0.0, node_weight=20.0, max_step=None):
    return _lib.ikf_path_options(rot_weight, -1.0 if max_pos is None else max_pos, -1.0 if max_rot is None else max_rot, int(limits), int(collisions),
                                 min_clearance, node_weight, -1.0 if max_step is None else max_step)


def _inputs(orob, T, k, seed, wild=False):
    """T waypoints along a slowly moving configuration and k candidates each (the truth plus noise of scale logspace(-3, -0.3, k) per candidate),
    tile-major [k * T x ndof]; clamped to the limits, or - `wild` - left as drawn, so that rows leave the limits and miss the thresholds."""
    g = torch.Generator().manual_seed(500 + seed)
    nd = orob.ndof
    lo, hi = RH.limits(orob)
    start = 0.5 * (lo + hi) + 0.15 * (hi - lo) * torch.randn(1, nd, generator=g)
    q_true = start + torch.cumsum(0.04 * torch.randn(T, nd, generator=g), 0)
    q_true = torch.minimum(torch.maximum(q_true, lo + 0.01), hi - 0.01)
    poses = ko.forward_kinematics(orob, q_true.double()).float().contiguous()
    q = q_true[None] + torch.randn(k, T, nd, generator=g) * torch.logspace(-3, -0.3, k)[:, None, None]
    q = q.reshape(k * T, nd)
    if wild:
        q = q + 0.5 * (hi - lo) * torch.randn(k * T, nd, generator=g) * (torch.rand(k * T, 1, generator=g) < 0.2)
    else:
        q = ko.clamp_to_joint_limits(orob, q)
    return poses, q.float().contiguous(), q_true.float()


def _path(eng, poses, q, k, opt, q_start=None, stream=None, null=(), latent=None, shared=True, clamp=True, expect=_lib.IKF_OK):
    """ikf_path_search (or, with `latent`, ikf_generate_path) through eng.lib on guarded buffers -> {name: cpu numpy window}."""
    T, nd = poses.shape[0], eng.layout.ndof
    shapes = {"path": (T, nd, torch.float32), "index": (T, 1, torch.int32), "cost": (1, 1, torch.float32), "reach": (T, 1, torch.int32),
              "node": (k * T, 1, torch.float32)}
    bufs = {n: _window(*shapes[n]) for n in OUTPUTS if n not in null}
    ptr = [bufs[n][GUARD:].data_ptr() if n in bufs else None for n in OUTPUTS]
    poses_d = poses.to(DEV).contiguous()
    rows_d = (q if latent is None else latent).to(DEV).contiguous()
    start_d = None if q_start is None else q_start.to(DEV).contiguous()
    sp = None if start_d is None else start_d.data_ptr()
    torch.cuda.synchronize()
    s = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(0)
    if latent is None:
        code = eng.lib.ikf_path_search(eng._h, poses_d.data_ptr(), T, k, rows_d.data_ptr(), sp, C.byref(opt), *ptr, s)
    else:
        code = eng.lib.ikf_generate_path(eng._h, poses_d.data_ptr(), T, k, rows_d.data_ptr(), int(shared), int(clamp), sp, C.byref(opt), *ptr, s)
    assert code == expect, (code, _lib.last_error(eng.lib))
    torch.cuda.synchronize()
    out = {n: _check_window(b, shapes[n][0], n).cpu().numpy() for n, b in bufs.items()}
    return {n: (v if n == "path" else v.reshape(-1)) for n, v in out.items()}


def _check_against_dp(out, q, T, k, opt, q_start=None, what=""):
    """Path, indices, cost and n_reachable against the numpy float32 lattice on the engine's own node costs - no tolerance."""
    path, index, cost, reach = PH.dp_f32(q.numpy(), out["node"], T, k, None if q_start is None else q_start.numpy(), opt.node_weight, opt.max_joint_step)
    print(f"{what}: cost {float(out['cost'][0]):.6f} (numpy {float(cost):.6f}), reachable min {int(out['reach'].min())} of {k}, "
          f"{int(np.isinf(out['node']).sum())} of {k * T} nodes inadmissible")
    assert np.array_equal(out["index"], index), f"{what}: index_out differs from the numpy lattice, first waypoint {np.flatnonzero(out['index'] != index)[:3]}"
    assert PH.same_bits(out["cost"], np.array([cost], np.float32)), f"{what}: cost_out {out['cost'][0]!r} != {cost!r}"
    assert PH.same_bits(out["path"], path), f"{what}: path_out is not the candidate rows at index_out"
    assert np.array_equal(out["reach"], reach), f"{what}: reachable_out"
    return index


def _check_nodes_are_rank_scores(eng, out, poses, q, k, opt):
    r = _rank(eng, poses, q, k, _rank_opt(1, opt.rot_weight, 0.0, None if opt.max_pos_err < 0 else opt.max_pos_err, None if opt.max_rot_err < 0 else opt.max_rot_err,
                                          bool(opt.reject_limits), bool(opt.reject_collisions), opt.min_clearance))
    assert PH.same_bits(out["node"], r["row_score"]), "node costs differ from ikf_rank_candidates' row scores of the same rows"


# ---- 1. the lattice against sequential numpy float32, on every shape at which the kernel takes another path ---------------------------------------
CASES = {
    "T1_k1": (1, 1, "panda", {}),
    "T1_k5": (1, 5, "panda", {}),
    "T2_k3": (2, 3, "panda", {}),
    "T9_k1": (9, 1, "panda", {}),
    "T7_k64": (7, 64, "panda", {}),
    "T65_k33": (65, 33, "panda", {}),
    "T40_k256": (40, 256, "panda", {}),
    "chunk-1": (CHUNK - 1, 5, "panda", {}),
    "chunk": (CHUNK, 5, "panda", {}),
    "chunk+1": (CHUNK + 1, 5, "panda", {}),
    "2chunk+1": (2 * CHUNK + 1, 5, "panda", {}),
    # every span: kp = path_span(k) = 2, 4, 16, 64 (four slices in four waves), 128 (two slices, merged through LDS) and 256 (one slice, no merge;
    # at k = 129 and 255 with dead destinations) ...
    "T5_k2": (5, 2, "panda", {}),
    "T5_k4": (5, 4, "panda", {}),
    "T5_k16": (5, 16, "panda", {}),
    "T5_k63": (5, 63, "panda", {}),
    "T5_k65": (5, 65, "panda", {}),
    "T5_k127": (5, 127, "panda", {}),
    "T5_k128": (5, 128, "panda", {}),
    "T5_k129": (5, 129, "panda", {}),
    "T5_k255": (5, 255, "panda", {}),
    # ... and the walk back across a chunk of back-pointers at kp = 128 and 256
    "T66_k65": (CHUNK + 2, 65, "panda", {}),
    "T66_k129": (CHUNK + 2, 129, "panda", {}),
    "ndof4": (65, 33, "syn4p", {}),     # k_path_lattice<4 .. 8, false>: a prismatic chain at 4 and 5 joints, a revolute one at 6
    "ndof5": (65, 33, "syn5p", {}),
    "ndof6": (65, 33, "syn6r", {}),
    "ndof8": (65, 33, "fetch", {}),
    "q_start": (65, 33, "panda", dict(q_start=True)),
    "step_gate": (65, 33, "panda", dict(max_step=0.12)),   # (forbids edges of the free lattice's path; at 0.1 no path is left)
    "thresholds_limits": (65, 33, "panda", dict(max_pos=0.2, max_rot=1.0, limits=True, wild=True)),
    "collisions": (65, 33, "panda", dict(collisions=True)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_lattice_equals_sequential_numpy_float32_on_the_engines_node_costs(case):
    T, k, which, v = CASES[case]
    v = dict(v)
    robot, orob = H.kin_robots(which)
    eng = _eng(which, collisions=v.get("collisions", False))
    poses, q, q_true = _inputs(orob, T, k, seed=T + k, wild=v.pop("wild", False))
    q_start = (q_true[0] + 0.05).contiguous() if v.pop("q_start", False) else None
    if v.get("collisions"):
        v["min_clearance"] = RH.clearance_threshold(orob, RH.collision_capsules(robot), q)
    opt = _popt(**v)
    out = _path(eng, poses, q, k, opt, q_start)
    _check_nodes_are_rank_scores(eng, out, poses, q, k, opt)
    index = _check_against_dp(out, q, T, k, opt, q_start, case)
    n_bad = int(np.isinf(out["node"]).sum())
    if case in ("thresholds_limits", "collisions"):
        assert 0 < n_bad < k * T, f"{case} rejects {n_bad} of {k * T} rows, so it does not test the rule"
    else:
        assert n_bad == 0 and (index >= 0).all()
    if case == "step_gate":
        free = _path(eng, poses, q, k, _popt())
        assert (index >= 0).all() and out["cost"][0] > free["cost"][0] and (index != free["index"]).any() and (out["reach"] <= free["reach"]).all()
    if case == "T65_k33":   # the same call on another stream
        again = _path(eng, poses, q, k, opt, stream=torch.cuda.Stream(device=DEV))
        assert all(PH.same_bits(out[n], again[n]) for n in OUTPUTS)


# ---- 1b. ties between slices and waves ---------------------------------------------------------------------------------------------------------------
TIE_T = 9
# k = 6 and 17: the duplicates sit in slices of one wave (merged by __shfl_xor); 33: in different waves (kp = 64, merged through LDS); 65 and 128:
# kp = 128, the two slices of a destination; 129 and 256: kp = 256, one slice - the tie is path_relax's own.  The end of the path is path_argmin's.
TIE_KS = (6, 17, 33, 65, 128, 129, 256)
TIE_SEEDS = {}   # k -> seed of _inputs where TIE_T + k does not serve (see the condition in the test)


def _tie_inputs(k):
    """_inputs at (TIE_T, k) with, at every waypoint, candidate 0's row copied onto candidate k - 1 and candidate 1's row onto candidate k / 2:
    the copies have bit-equal node costs and bit-equal edge sums to every destination."""
    orob = H.kin_robots("panda")[1]
    poses, q, q_true = _inputs(orob, TIE_T, k, seed=TIE_SEEDS.get(k, TIE_T + k))
    g = q.reshape(k, TIE_T, -1).clone()
    g[k - 1] = g[0]
    g[k // 2] = g[1]
    return poses, g.reshape(k * TIE_T, -1).contiguous(), q_true


@pytest.mark.parametrize("k", TIE_KS)
def test_ties_between_slices_and_waves_go_to_the_lower_index(k):
    """What tests/test_path_math_host.py::test_ties_go_to_the_lower_index proves of path_before, on the GPU, where the tie is resolved inside a
    slice, by __shfl_xor, through s_part_c / s_part_j and by path_argmin at the end: two pairs of bit-equal candidates per waypoint.  The result is
    the numpy lattice's (np.argmin: the first minimum), and neither copy is ever chosen.  Condition, checked with the numpy lattice on the
    engine's node costs: the path goes through candidate 0 or 1 somewhere - there the copy ties with it."""
    T = TIE_T
    eng = _eng("panda")
    poses, q, _ = _tie_inputs(k)
    opt = _popt()
    out = _path(eng, poses, q, k, opt)
    node = out["node"].reshape(k, T)
    assert PH.same_bits(node[k - 1], node[0]) and PH.same_bits(node[k // 2], node[1]) and np.isfinite(node).all()
    index = _check_against_dp(out, q, T, k, opt, what=f"ties k {k}")
    n_tied = int(np.isin(index, (0, 1)).sum())
    print(f"ties k {k}: the path takes candidate 0 or 1 at {n_tied} of {T} waypoints, index {index.tolist()}")
    assert n_tied >= 1, f"k {k}: the path never takes a duplicated candidate - the case does not test the tie (another seed: TIE_SEEDS)"
    assert not np.isin(out["index"], (k - 1, k // 2)).any(), f"k {k}: a copy was chosen over its lower-indexed original: {out['index'].tolist()}"


@pytest.mark.parametrize("k", TIE_KS)
def test_a_lattice_of_equal_candidates_takes_candidate_zero_everywhere(k):
    """Every candidate of a waypoint is the same row, and q_start is set: every predecessor of every node ties, and so do all k ends."""
    T = TIE_T
    orob = H.kin_robots("panda")[1]
    eng = _eng("panda")
    poses, q, q_true = _inputs(orob, T, k, seed=T + k)
    g = q.reshape(k, T, -1)
    q = g[:1].expand(k, T, g.shape[2]).reshape(k * T, -1).contiguous()
    q_start = (q_true[0] + 0.05).contiguous()
    opt = _popt()
    out = _path(eng, poses, q, k, opt, q_start)
    assert np.isfinite(out["node"]).all() and np.isfinite(out["cost"][0])
    _check_against_dp(out, q, T, k, opt, q_start, what=f"equal candidates k {k}")
    assert (out["index"] == 0).all(), out["index"].tolist()
    assert (out["reach"] == k).all(), out["reach"].tolist()


# ---- 2. no path; null outputs ----------------------------------------------------------------------------------------------------------------------
def test_blocked_lattice_and_nan_column_give_the_no_path_outputs():
    orob = H.kin_robots("panda")[1]
    eng = _eng("panda")
    T, k = 2 * CHUNK + 3, 5
    poses, q, _ = _inputs(orob, T, k, seed=3)
    blocked = _path(eng, poses, q, k, _popt(max_step=0.0))          # no two rows are equal: every edge is forbidden
    assert np.isposinf(blocked["cost"][0]) and (blocked["index"] == -1).all() and (blocked["path"] == 0).all()
    assert blocked["reach"][0] == k and (blocked["reach"][1:] == 0).all()
    _check_against_dp(blocked, q, T, k, _popt(max_step=0.0), what="blocked")
    qn = q.reshape(k, T, -1).clone()
    qn[:, 70] = float("nan")                                         # every candidate of waypoint 70
    qn[2, 5, 3] = float("nan")                                       # and one row elsewhere
    qn = qn.reshape(k * T, -1).contiguous()
    out = _path(eng, poses, qn, k, _popt())
    node = out["node"].reshape(k, T)
    assert np.isposinf(node[:, 70]).all() and np.isposinf(node[2, 5]) and np.isfinite(np.delete(node, 70, 1)).sum() == k * (T - 1) - 1
    assert np.isposinf(out["cost"][0]) and (out["index"] == -1).all() and (out["path"] == 0).all()
    assert (out["reach"][:5] == k).all() and out["reach"][5] == k - 1 and (out["reach"][6:70] == k).all() and (out["reach"][70:] == 0).all()
    qn2 = q.reshape(k, T, -1).clone()
    qn2[2, 5, 3] = float("nan")                                      # the single NaN row alone: never chosen, the path exists
    out2 = _path(eng, poses, qn2.reshape(k * T, -1).contiguous(), k, _popt())
    idx = _check_against_dp(out2, qn2.reshape(k * T, -1), T, k, _popt(), what="one NaN row")
    assert np.isfinite(out2["cost"][0]) and idx[5] != 2 and np.isfinite(out2["path"]).all()


def test_null_optional_outputs_are_accepted():
    orob = H.kin_robots("panda")[1]
    eng = _eng("panda")
    T, k = 20, 7
    poses, q, _ = _inputs(orob, T, k, seed=4)
    ref = _path(eng, poses, q, k, _popt())
    for null in (("reach",), ("node",), ("reach", "node")):
        got = _path(eng, poses, q, k, _popt(), null=null)
        assert set(got) == set(OUTPUTS) - set(null) and all(PH.same_bits(ref[n], got[n]) for n in got)


# ---- 3. flow + search ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,k", [(33, 20), (5, 256)])
def test_shared_latent_equals_the_expanded_latent_and_the_two_step_route(T, k):
    """ikf_generate_path with k shared latents == the same call with the latent expanded to [k * T x D] tile-major == generate_ik_solutions on the
    repeated waypoints followed by ikf_path_search: every output bit for bit."""
    s, robot, lay, sd = _solver("tiny")
    eng = s.engine(DEV)
    _, poses = H.reachable_poses(robot, T, 11)
    poses = poses.float()
    L = H.latents(k, lay.dim, 12)
    expanded = L[:, None, :].expand(k, T, lay.dim).reshape(k * T, lay.dim).contiguous()
    opt = _popt(limits=True, max_step=3.0)
    shared = _path(eng, poses, None, k, opt, latent=L, shared=True)
    explicit = _path(eng, poses, None, k, opt, latent=expanded, shared=False)
    assert all(PH.same_bits(shared[n], explicit[n]) for n in OUTPUTS)
    rows = s.generate_ik_solutions(poses.to(DEV).repeat((k, 1)), latent=expanded.to(DEV)).cpu()
    two_step = _path(eng, poses, rows, k, opt)
    assert all(PH.same_bits(shared[n], two_step[n]) for n in OUTPUTS)
    _check_against_dp(shared, rows, T, k, opt, what=f"tiny T {T} k {k}")
    other = _path(eng, poses, None, k, opt, latent=H.latents(k * T, lay.dim, 13), shared=False)    # (a latent per node is another lattice)
    assert not PH.same_bits(other["node"], shared["node"])


EXPAND_MAX_THREADS = 8192 * 256   # launch_path_expand_latent caps the grid at 8192 workgroups of 256: beyond it a thread copies a second element


def test_shared_latent_equals_the_expanded_latent_beyond_the_expansion_grid():
    """k = 256 and the smallest T with k * T * D > 8192 * 256: k_path_expand_latent's grid-stride loop takes a second trip.  An element it left
    out would keep what the handle's latent buffer held, and the flow's rows, the node costs and the path would differ from the expanded call's."""
    s, robot, lay, sd = _solver("tiny")
    eng = s.engine(DEV)
    k = 256
    T = EXPAND_MAX_THREADS // (k * lay.dim) + 1
    assert k * (T - 1) * lay.dim <= EXPAND_MAX_THREADS < k * T * lay.dim
    _, poses = H.reachable_poses(robot, T, 31)
    poses = poses.float()
    L = H.latents(k, lay.dim, 32)
    expanded = L[:, None, :].expand(k, T, lay.dim).reshape(k * T, lay.dim).contiguous()
    opt = _popt(limits=True, max_step=3.0)
    other = _path(eng, poses, None, k, opt, latent=H.latents(k, lay.dim, 33), shared=True)   # (the handle's buffer now holds OTHER latents, expanded)
    shared = _path(eng, poses, None, k, opt, latent=L, shared=True)
    explicit = _path(eng, poses, None, k, opt, latent=expanded, shared=False)
    print(f"T {T} k {k} D {lay.dim}: {k * T * lay.dim} latent elements, cost {float(shared['cost'][0]):.6f}")
    assert all(PH.same_bits(shared[n], explicit[n]) for n in OUTPUTS)
    assert not PH.same_bits(other["node"], shared["node"])


# ---- 4. status codes -------------------------------------------------------------------------------------------------------------------------------
def test_status_codes_and_untouched_outputs():
    from ikflow_amd.engine import Engine

    orob = H.kin_robots("panda")[1]
    eng = _eng("panda")
    lib, h = eng.lib, eng._h
    T, k = 4, 5
    poses, q, _ = _inputs(orob, T, k, seed=1)
    P, Q = poses.to(DEV), q.to(DEV)
    path = torch.full((T, 7), 7.0, device=DEV)
    index = torch.full((T,), 7, dtype=torch.int32, device=DEV)
    cost = torch.full((1,), 7.0, device=DEV)
    opt = _popt()
    call = lambda h_, p, n, k_, q_, o, po, io, co: lib.ikf_path_search(h_, p, n, k_, q_, None, o, po, io, co, None, None, None)
    ok = (h, P.data_ptr(), T, k, Q.data_ptr(), C.byref(opt), path.data_ptr(), index.data_ptr(), cost.data_ptr())
    bad = [
        ((None,) + ok[1:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:1] + (None,) + ok[2:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:4] + (None,) + ok[5:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:5] + (None,) + ok[6:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:6] + (None,) + ok[7:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:7] + (None,) + ok[8:], _lib.IKF_ERR_NULL_POINTER),
        (ok[:8] + (None,), _lib.IKF_ERR_NULL_POINTER),
        (ok[:2] + (-1,) + ok[3:], _lib.IKF_ERR_BAD_ARGUMENT),
        (ok[:3] + (0,) + ok[4:], _lib.IKF_ERR_BAD_ARGUMENT),
        (ok[:3] + (257,) + ok[4:], _lib.IKF_ERR_BAD_ARGUMENT),
        (ok[:2] + (2 ** 23, 256) + ok[4:], _lib.IKF_ERR_BAD_ARGUMENT),                      # k * T = 2^31
        (ok[:5] + (C.byref(_popt(node_weight=-1.0)),) + ok[6:], _lib.IKF_ERR_BAD_ARGUMENT),
    ]
    for args, code in bad:
        assert call(*args) == code, (args, code)
    fresh = Engine(eng.layout, eng.robot, DEV)                                              # (no collision model, no weights)
    assert call(fresh._h, *ok[1:5], C.byref(_popt(collisions=True)), *ok[6:]) == _lib.IKF_ERR_BAD_ARGUMENT
    lat = torch.zeros(k, eng.layout.dim, device=DEV)
    gen = lambda h_: lib.ikf_generate_path(h_, P.data_ptr(), T, k, lat.data_ptr(), 1, 1, None, C.byref(opt), path.data_ptr(), index.data_ptr(), cost.data_ptr(),
                                           None, None, None)
    assert gen(fresh._h) == _lib.IKF_ERR_NOT_LOADED and gen(None) == _lib.IKF_ERR_NULL_POINTER
    assert call(h, None, 0, k, None, C.byref(opt), None, None, None) == _lib.IKF_OK         # nothing to do: null buffers are fine
    for args in ((None, 4, 4), (fresh._h, 0, 4), (fresh._h, 4, 0), (fresh._h, 4, 257), (fresh._h, 2 ** 23, 256)):
        assert lib.ikf_reserve_path(*args) == (_lib.IKF_ERR_NULL_POINTER if args[0] is None else _lib.IKF_ERR_BAD_ARGUMENT)
    assert lib.ikf_reserve_path(fresh._h, 100, 50) == _lib.IKF_OK
    torch.cuda.synchronize()
    assert (path == 7.0).all() and (index == 7).all() and (cost == 7.0).all()               # none of the refused calls touched an output
    assert call(*ok) == _lib.IKF_OK
    torch.cuda.synchronize()
    assert (index >= 0).all() and (index < k).all() and torch.isfinite(cost).all()


# ---- 5. ikf_reserve_path -----------------------------------------------------------------------------------------------------------------------------
def test_after_reserve_path_a_call_of_that_size_allocates_nothing():
    """As tests/test_ranked.py checks ikf_reserve_ranked: the device's free memory over a call of the reserved size, in both latent forms, and two
    smaller ones shrinks by no more than torch's own allocator grew for the test's buffers; the reservation changes no result."""
    from ikflow_amd.engine import Engine

    s, robot, lay, sd = _solver("tiny")
    T, k = 300, 64
    _, poses = H.reachable_poses(robot, T, 3)
    poses = poses.float()
    L, Lfull = H.latents(k, lay.dim, 5), H.latents(k * T, lay.dim, 6)
    opt = _popt(limits=True)

    def run(eng, tt, kk, shared=True):
        return _path(eng, poses[:tt], None, kk, opt, latent=L[:kk] if shared else Lfull[:kk * tt], shared=shared)

    eng = Engine(s.layout, robot, DEV)
    eng.load_state_dict(s._state_dict_np)
    eng.reserve_path(T, k)
    torch.cuda.synchronize()
    run(eng, 8, 4)                                                     # (torch's caching allocator warm for the test's own buffers)
    torch.cuda.synchronize()
    free0, stat0 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    full = run(eng, T, k)
    run(eng, T, k, shared=False)
    run(eng, 100, 50)
    run(eng, 1, 64)
    torch.cuda.synchronize()
    free1, stat1 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    grown_by_torch = stat1 - stat0                                     # (the guarded windows of the larger calls come from torch)
    assert free0 - free1 <= grown_by_torch, f"the engine allocated {free0 - free1 - grown_by_torch} bytes after ikf_reserve_path"
    fresh = Engine(s.layout, robot, DEV)
    fresh.load_state_dict(s._state_dict_np)
    assert all(PH.same_bits(full[n], v) for n, v in run(fresh, T, k).items())   # (the reservation changes no result)


# ---- 6. the Python method ------------------------------------------------------------------------------------------------------------------------------
def test_generate_ik_path_end_to_end():
    s, robot, lay, sd = _solver("tiny")
    eng = s.engine(DEV)
    T, k = 33, 20
    _, poses = H.reachable_poses(robot, T, 21)
    w = poses.float().to(DEV)
    L = H.latents(k, lay.dim, 22).to(DEV)
    got = s.generate_ik_path(w, k, latent=L, return_node_costs=True)
    assert got._fields == ("path", "index", "cost", "n_reachable", "node_costs")
    assert got.path.shape == (T, robot.ndof) and got.index.dtype == torch.int32 and got.n_reachable.dtype == torch.int32 and got.cost.shape == ()
    expanded = L[:, None, :].expand(k, T, lay.dim).reshape(k * T, lay.dim).contiguous()
    rows = s.generate_ik_solutions(w.repeat((k, 1)), latent=expanded).cpu()
    out = {"path": got.path.cpu().numpy(), "index": got.index.cpu().numpy(), "cost": got.cost.reshape(1).cpu().numpy(),
           "reach": got.n_reachable.cpu().numpy(), "node": got.node_costs.cpu().numpy()}
    index = _check_against_dp(out, rows, T, k, eng.path_options(rot_weight=0.01), what="generate_ik_path")
    assert (index >= 0).all()
    four = s.generate_ik_path(w, k, latent=L)
    assert four._fields == ("path", "index", "cost", "n_reachable") and torch.equal(four.index, got.index) and torch.equal(four.path, got.path)
    # the same torch seed draws the same k latents; a latent per node is another draw
    torch.manual_seed(77)
    a = s.generate_ik_path(w, k)
    torch.manual_seed(77)
    b = s.generate_ik_path(w, k, latent=torch.randn((k, lay.dim), device=DEV))
    assert torch.equal(a.path, b.path) and torch.equal(a.cost, b.cost)
    per_node = s.generate_ik_path(w, k, latent=H.latents(k * T, lay.dim, 23).to(DEV), shared_latent=False, q_start=got.path[0], max_joint_step=6.0)
    assert per_node.path.shape == (T, robot.ndof)
    # refine_steps = 2: two LM steps on the returned rows; index and cost still describe the lattice
    refined = s.generate_ik_path(w, k, latent=L, refine_steps=2)
    want = eng.lm_step(w, eng.lm_step(w, got.path))
    assert torch.equal(refined.path, want) and torch.equal(refined.index, got.index) and torch.equal(refined.cost, got.cost)
    pe0, _ = eng.pose_error(got.path, w)
    pe2, _ = eng.pose_error(refined.path, w)
    print(f"generate_ik_path: position error median {float(pe0.median()):.4f} -> {float(pe2.median()):.4f} m after two LM steps")
    # no path: nothing is refined
    none = s.generate_ik_path(w, k, latent=L, pos_error_threshold=0.0, refine_steps=2)
    assert torch.isposinf(none.cost) and (none.index == -1).all() and (none.path == 0).all() and (none.n_reachable == 0).all()
