"""Swept collision checks along edges on the GPU (include/ikflow_amd_sweep.h; ikflow_amd/csrc/sweep_kernels.hip, sweep_math.h, api_sweep.hip, and the
SWEEP form of k_path_lattice): ikf_sweep_edges against the fp64 reference of tests/sweep_helpers.py on guarded buffers, the lattice with a sweep
against sequential numpy float32 on the engine's own node costs and verdicts (bit for bit), the purpose against fp64, the calls a sweep must not
change (also at more mask words than the sweep's grid has workgroups), a blocked crossing, the flow in front, handle behaviour and the Python
wrappers.  sweep_helpers.CHAINS and the lattice cases run k_sweep_edges<ND> and k_path_lattice<ND, true> for every ND = 4 .. 8.

Tolerance: world_helpers.BAND (1e-4) around a threshold, inside which a verdict is not compared; tests/test_sweep_math_host.py checks on the CPU
that this leaves at most 5 % of the edges undecided and enough on either side."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H
import path_helpers as PH
import rank_helpers as RH
import sweep_helpers as SH
import world_helpers as WH
from ikflow_amd import _lib
from test_path import CHUNK, OUTPUTS, _check_nodes_are_rank_scores, _path, _popt
from test_ranked import DEV, GUARD, INT_SENTINEL, _small_model_back  # noqa: F401  (a fixture)
from test_world import _USED, _eng, _eng_model

pytestmark = pytest.mark.gpu
BYTE_SENTINEL = 0xAB


@pytest.fixture(autouse=True)
def _no_sweep_and_no_world_left_behind():
    yield
    for eng in _USED:   # (the engines are shared with the other test modules)
        eng.set_path_sweep(0)
        eng.clear_world()


def _sweep(eng, a, b, S, reject_self=False, self_min=0.0, null=(), n=None, stream=None, expect=_lib.IKF_OK):
    """ikf_sweep_edges through eng.lib on guarded buffers -> {"blocked": uint8 [n], "first": int32 [n]} (cpu numpy); `null`: outputs passed as null."""
    rows = a.shape[0]
    n = rows if n is None else n
    fill = {"blocked": (BYTE_SENTINEL, torch.uint8), "first": (INT_SENTINEL, torch.int32)}
    bufs = {o: torch.full((rows + 2 * GUARD,), fill[o][0], dtype=fill[o][1], device=DEV) for o in fill if o not in null}
    ptr = [bufs[o][GUARD:].data_ptr() if o in bufs else None for o in fill]
    ad, bd = torch.as_tensor(a).to(DEV).contiguous(), torch.as_tensor(b).to(DEV).contiguous()
    torch.cuda.synchronize()
    s = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(0)
    code = eng.lib.ikf_sweep_edges(eng._h, ad.data_ptr() if rows else None, bd.data_ptr() if rows else None, n, S, int(reject_self), float(self_min), *ptr, s)
    assert code == expect, (code, _lib.last_error(eng.lib))
    torch.cuda.synchronize()
    out = {}
    for o, buf in bufs.items():
        assert bool((buf[:GUARD] == fill[o][0]).all()) and bool((buf[GUARD + max(n, 0):] == fill[o][0]).all()), f"{o}: an element outside the window was written"
        win = buf[GUARD:GUARD + max(n, 0)]
        if expect == _lib.IKF_OK:
            assert bool((win != fill[o][0]).all()), f"{o}: an element inside the window was not written"
        else:
            assert bool((win == fill[o][0]).all()), f"{o}: a refused call wrote an output"
        out[o] = win.cpu().numpy().copy()
    return out


# ---- 1. ikf_sweep_edges against the fp64 reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,S", SH.EDGE_CASES)
@pytest.mark.parametrize("which", SH.CHAINS)
def test_sweep_edges_against_the_fp64_reference(which, scene, S):
    """Every chain size, 4 .. 8 joints: 1, 63, 64, 65 and 257 edges (130 in the 64-obstacle scene: the cost of its fp64 reference) under the world
    rule alone, the self rule alone and both: flags exact outside the band, the first blocked sample exact when no earlier sample is in the band."""
    eng = _eng(which)
    c = SH.edge_case(which, scene, S)
    for rule in ("world", "self", "both"):
        if rule == "self":
            eng.clear_world()
        else:
            eng.set_world(c["world"], c["world_thr"])
        for n in SH.SIZES[scene]:
            out = _sweep(eng, c["a"][:n], c["b"][:n], S, reject_self=rule != "world", self_min=c["self_thr"])
            assert set(np.unique(out["blocked"])) <= {0, 1} and ((out["first"] >= -1) & (out["first"] < S)).all()
            SH.check_edges(out["blocked"], out["first"], SH.case_verdicts(c, rule, n), f"{which} {scene} S {S} {rule} n {n}")
        print(f"{which} {scene} S {S} {rule}: {int(out['blocked'].sum())} of {len(out['blocked'])} edges blocked")
        assert 0 < out["blocked"].sum() < len(out["blocked"])


# ---- 2. buffers and status codes --------------------------------------------------------------------------------------------------------------------
def test_nullable_outputs_empty_calls_and_status_codes():
    from ikflow_amd.engine import Engine

    which = "panda"
    eng = _eng(which)
    lib = eng.lib
    c = SH.edge_case(which, "mixed7", 3)
    a, b = c["a"][:130], c["b"][:130]
    eng.set_world(c["world"], c["world_thr"])
    full = _sweep(eng, a, b, 3, True, c["self_thr"])
    for null in (("blocked",), ("first",)):
        got = _sweep(eng, a, b, 3, True, c["self_thr"], null=null)
        assert set(got) == {"blocked", "first"} - set(null) and all(H.same_bits(got[o], full[o]) for o in got)
    side = _sweep(eng, a, b, 3, True, c["self_thr"], stream=torch.cuda.Stream(device=DEV))
    assert all(H.same_bits(side[o], full[o]) for o in full)
    # n = 0: nothing is written (every element still carries its sentinel), and null pointers are fine
    _sweep(eng, a, b, 3, n=0)
    bufs = _sweep(eng, a[:0], b[:0], 3)
    assert all(v.size == 0 for v in bufs.values())
    assert lib.ikf_sweep_edges(eng._h, None, None, 0, 3, 0, 0.0, None, None, None) == _lib.IKF_OK
    # an empty world without the self rule: every edge is free
    eng.clear_world()
    free = _sweep(eng, a, b, 16)
    assert (free["blocked"] == 0).all() and (free["first"] == -1).all()
    # status codes and messages; a refused call writes nothing
    eng.set_world(c["world"], c["world_thr"])
    for S in (0, 17, -1):
        _sweep(eng, a, b, S, expect=_lib.IKF_ERR_BAD_ARGUMENT)
        assert "n_samples must be in 1 .. 16" in _lib.last_error(lib)
    _sweep(eng, a, b, 3, null=("blocked", "first"), expect=_lib.IKF_ERR_NULL_POINTER)
    assert "both outputs are null" in _lib.last_error(lib)
    _sweep(eng, a, b, 3, n=-1, expect=_lib.IKF_ERR_BAD_ARGUMENT)
    assert "n must be >= 0" in _lib.last_error(lib)
    ad = torch.as_tensor(a).to(DEV)
    out = torch.zeros(130, dtype=torch.uint8, device=DEV)
    assert lib.ikf_sweep_edges(eng._h, None, ad.data_ptr(), 130, 3, 0, 0.0, out.data_ptr(), None, None) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_sweep_edges(eng._h, ad.data_ptr(), None, 130, 3, 0, 0.0, out.data_ptr(), None, None) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_sweep_edges(None, ad.data_ptr(), ad.data_ptr(), 130, 3, 0, 0.0, out.data_ptr(), None, None) == _lib.IKF_ERR_NULL_POINTER
    fresh = Engine(eng.layout, eng.robot, DEV)   # no collision model
    assert lib.ikf_sweep_edges(fresh._h, ad.data_ptr(), ad.data_ptr(), 130, 3, 0, 0.0, out.data_ptr(), None, None) == _lib.IKF_ERR_BAD_ARGUMENT
    assert "no collision model" in _lib.last_error(lib)
    torch.cuda.synchronize()
    assert (out == 0).all()
    # ikf_set_path_sweep: 0 .. 16; a refused value keeps the old one
    assert eng.path_sweep == 0 and fresh.path_sweep == 0
    eng.set_path_sweep(5)
    for bad in (-1, 17, 1000):
        assert lib.ikf_set_path_sweep(eng._h, bad) == _lib.IKF_ERR_BAD_ARGUMENT and "n_samples must be in 0 .. 16" in _lib.last_error(lib)
        assert eng.path_sweep == 5
    eng.set_path_sweep(16)
    assert eng.path_sweep == 16
    eng.set_path_sweep(0)
    assert eng.path_sweep == 0 and lib.ikf_get_path_sweep(None) == 0


# ---- 3. the lattice with a sweep against sequential numpy float32 --------------------------------------------------------------------------------
def _mask_of(eng, q, T, k, S, opt, q_start):
    """The verdicts of ikf_sweep_edges on all k * k * (T - 1) (+ k start) edges of the lattice -> (edge_free [T][k][k], start_free [k] or None)."""
    a, b = SH.lattice_edges(q.numpy(), T, k, None if q_start is None else q_start.numpy())
    if a.shape[0] == 0:
        return np.ones((T, k, k), bool), None
    sw = _sweep(eng, a, b, S, reject_self=bool(opt.reject_collisions), self_min=opt.min_clearance)
    return SH.split_lattice_verdicts(sw["blocked"] == 0, T, k, q_start is not None)


def _check_against_masked_dp(out, q, T, k, opt, ef, sf, q_start, what):
    path, index, cost, reach = SH.dp_f32_masked(q.numpy(), out["node"], T, k, ef, sf, None if q_start is None else q_start.numpy(), opt.node_weight,
                                                opt.max_joint_step)
    print(f"{what}: cost {float(out['cost'][0]):.6f} (numpy {float(cost):.6f}), reachable min {int(out['reach'].min())} of {k}, "
          f"{int(np.isinf(out['node']).sum())} of {k * T} nodes inadmissible")
    assert np.array_equal(out["index"], index), f"{what}: index_out differs from the masked numpy lattice, first waypoint {np.flatnonzero(out['index'] != index)[:3]}"
    assert PH.same_bits(out["cost"], np.array([cost], np.float32)), f"{what}: cost_out {out['cost'][0]!r} != {cost!r}"
    assert PH.same_bits(out["path"], path), f"{what}: path_out is not the candidate rows at index_out"
    assert np.array_equal(out["reach"], reach), f"{what}: reachable_out"


def _admissible_edge_counts(node, ef, sf, T, k):
    """(blocked, free) among the edges whose two nodes are admissible (the start edge: whose destination is)."""
    adm = np.isfinite(np.asarray(node).reshape(k, T))
    both = adm.T[1:, :, None] & adm.T[:-1, None, :]
    nb, nf = int((~ef[1:] & both).sum()), int((ef[1:] & both).sum())
    if sf is not None:
        nb, nf = nb + int((~sf & adm[:, 0]).sum()), nf + int((sf & adm[:, 0]).sum())
    return nb, nf


CASES = {
    "T1_k1": (1, 1, "panda", {}),
    "T1_k1_start": (1, 1, "panda", dict(q_start=True)),
    "T1_k5": (1, 5, "panda", {}),
    "T1_k5_start": (1, 5, "panda", dict(q_start=True)),
    "T2_k3": (2, 3, "panda", {}),
    "T9_k1": (9, 1, "panda", {}),
    "T7_k64": (7, 64, "panda", {}),
    "T3_k65": (3, 65, "panda", {}),
    "T65_k33": (65, 33, "panda", {}),
    "T5_k256": (5, 256, "panda", {}),
    # kp = 128 with both slices full (k = 128, sweep_words = 2); kp = 256 with dead destinations and a last mask word of one live bit: the third
    # of three at k = 129 (sweep_words = 3 of kPathMaskWords = 4), the fourth of four at k = 193; kp = 128 across a chunk of back-pointers
    "T3_k128": (3, 128, "panda", {}),
    "T3_k129": (3, 129, "panda", {}),
    "T3_k193": (3, 193, "panda", {}),
    "T66_k65": (CHUNK + 2, 65, "panda", {}),
    "2chunk+1": (2 * CHUNK + 1, 5, "panda", {}),
    "ndof4": (65, 33, "syn4p", {}),     # k_path_lattice<4 .. 8, true>: a prismatic chain at 4 and 5 joints, a revolute one at 6
    "ndof5": (65, 33, "syn5p", {}),
    "ndof6": (65, 33, "syn6r", {}),
    "ndof8": (65, 33, "fetch", {}),
    "q_start": (65, 33, "panda", dict(q_start=True)),
    "step_gate": (65, 33, "panda", dict(max_step=SH.STEP_GATE)),
    "self_rule": (65, 33, "panda", dict(collisions=True, seed=SH.SELF_RULE_SEED)),
    "S1": (65, 33, "panda", dict(S=1)),
    "S16": (65, 33, "panda", dict(S=16)),
}


def _lattice_case(case):
    T, k, which, v = CASES[case]
    v = dict(v)
    seed = v.pop("seed", SH.LATTICE_SEEDS.get((which, T, k), 0))
    L = SH.lattice_inputs(which, T, k, seed)
    S = v.pop("S", 4)
    q_start = L["q_start"] if v.pop("q_start", False) else None
    if v.get("collisions"):
        v["min_clearance"] = L["self_thr"]
    return T, k, which, L, S, q_start, _popt(**v)


@pytest.mark.parametrize("case", list(CASES))
def test_lattice_with_a_sweep_equals_the_masked_numpy_lattice(case):
    """ikf_path_search under a sweep == sweep_helpers.dp_f32_masked on the engine's own node costs and the verdicts of ikf_sweep_edges on every edge
    of the same rows: path, index, cost and reachable_out bit for bit.  Cases with edges and k >= 3 hold blocked and free edges between admissible
    nodes; at (65, 33) the swept path differs from the unswept path of the same lattice and costs more."""
    T, k, which, L, S, q_start, opt = _lattice_case(case)
    eng = _eng(which)
    eng.set_world(L["world"], L["world_thr"])
    eng.set_path_sweep(S)
    out = _path(eng, L["poses"], L["q"], k, opt, q_start)
    ef, sf = _mask_of(eng, L["q"], T, k, S, opt, q_start)
    _check_against_masked_dp(out, L["q"], T, k, opt, ef, sf, q_start, case)
    nb, nf = _admissible_edge_counts(out["node"], ef, sf, T, k)
    print(f"{case}: {nb} blocked and {nf} free edges between admissible nodes")
    if k >= 3 and (T > 1 or q_start is not None):
        assert nb > 0 and nf > 0, f"{case}: {nb} blocked, {nf} free edges between admissible nodes - the case does not test the mask"
    if T * k == 65 * 33:
        eng.set_path_sweep(0)
        unswept = _path(eng, L["poses"], L["q"], k, opt, q_start)
        assert PH.same_bits(unswept["node"], out["node"])
        assert np.isfinite(out["cost"][0]) and (out["index"] >= 0).all(), f"{case}: no swept path"
        assert (out["index"] != unswept["index"]).any() and out["cost"][0] > unswept["cost"][0], f"{case}: the sweep did not change the path"
        assert (out["reach"] <= unswept["reach"]).all()
    if case == "T65_k33":   # the same call on another stream
        eng.set_path_sweep(S)
        again = _path(eng, L["poses"], L["q"], k, opt, q_start, stream=torch.cuda.Stream(device=DEV))
        assert all(PH.same_bits(out[n], again[n]) for n in OUTPUTS)


# ---- 4. the purpose, against fp64 ---------------------------------------------------------------------------------------------------------------------
def _path_edge_verdicts(which, L, rows, S):
    """fp64 verdicts (world rule) of the edges between consecutive rows of a path [T x nd]."""
    robot, orob = H.kin_robots(which)
    smp = SH.samples_f32(rows[:-1], rows[1:], S)
    wc, _ = SH.sample_clearances(orob, RH.collision_capsules(robot), L["world"], smp, want_self=False)
    return SH.verdicts(wc, L["world_thr"])


def test_the_swept_path_crosses_nothing_where_the_unswept_path_does():
    """(65, 33) on mixed7: every edge of the path returned under a sweep is free by the fp64 reference (or in the band); the unswept path of the same
    call has at least one surely blocked edge - the seed is the one for which the reference says so."""
    T, k, which, L, S, q_start, opt = _lattice_case("T65_k33")
    eng = _eng(which)
    eng.set_world(L["world"], L["world_thr"])
    unswept = _path(eng, L["poses"], L["q"], k, opt)
    eng.set_path_sweep(S)
    swept = _path(eng, L["poses"], L["q"], k, opt)
    assert np.isfinite(unswept["cost"][0]) and np.isfinite(swept["cost"][0])
    vu, vs = _path_edge_verdicts(which, L, unswept["path"], S), _path_edge_verdicts(which, L, swept["path"], S)
    print(f"unswept path: {int(vu['blocked'].sum())} surely blocked edges of {T - 1}; swept path: {int(vs['blocked'].sum())} ({int(vs['band'].sum())} in the band)")
    assert vu["blocked"].sum() >= 1
    assert not vs["blocked"].any()
    got = _sweep(eng, swept["path"][:-1], swept["path"][1:], S)
    assert (got["blocked"] == 0).all()   # (the engine's own verdict of its own path)


# ---- 5. calls a sweep must not change ----------------------------------------------------------------------------------------------------------------
def test_sweep_off_nothing_to_test_against_and_a_far_world_give_the_unswept_call_bit_for_bit():
    T, k, which, L, S, _, opt = _lattice_case("T65_k33")
    eng = _eng(which)
    q_start = L["q_start"]
    for collisions in (False, True):
        o = _popt(collisions=collisions, min_clearance=L["self_thr"] if collisions else 0.0, max_step=2.0)
        eng.clear_world()
        eng.set_path_sweep(0)
        plain = _path(eng, L["poses"], L["q"], k, o, q_start)
        eng.set_world(L["world"], L["world_thr"])
        world_only = _path(eng, L["poses"], L["q"], k, o, q_start)
        eng.set_path_sweep(S)
        changed = _path(eng, L["poses"], L["q"], k, o, q_start)
        assert not all(PH.same_bits(changed[n], world_only[n]) for n in OUTPUTS)   # (here the sweep does matter)
        eng.set_path_sweep(0)                                                        # sweep off
        off = _path(eng, L["poses"], L["q"], k, o, q_start)
        assert all(PH.same_bits(off[n], world_only[n]) for n in OUTPUTS)
        eng.set_path_sweep(S)
        eng.set_world(WH.far_world(), 1.0)                                           # a world nothing reaches
        far = _path(eng, L["poses"], L["q"], k, o, q_start)
        if not collisions:
            assert all(PH.same_bits(far[n], plain[n]) for n in OUTPUTS)
            eng.clear_world()                                                        # nothing to test against
            nothing = _path(eng, L["poses"], L["q"], k, o, q_start)
            assert all(PH.same_bits(nothing[n], plain[n]) for n in OUTPUTS)
        else:   # (with reject_collisions the self rule sweeps whatever the world is: far world == no world, and both differ from no sweep)
            eng.clear_world()
            self_only = _path(eng, L["poses"], L["q"], k, o, q_start)
            assert all(PH.same_bits(far[n], self_only[n]) for n in OUTPUTS)
            assert PH.same_bits(self_only["node"], plain["node"])


# ---- 5b. more mask words than the sweep's grid has workgroups -----------------------------------------------------------------------------------------
SWEEP_MAX_GRID = 2 ** 20   # kSweepMaxGrid of sweep_kernels.hip: beyond it a workgroup walks wave, wave + gridDim.x, ...


def test_a_lattice_of_more_mask_words_than_the_sweep_grid_has_workgroups():
    """T = 1025, k = 256: 1,049,600 mask words, 1,024 more than kSweepMaxGrid - those of the last waypoint's destinations are second trips of the
    sweep kernel's strided loop.  (1) A sphere around the whole arm makes every node inadmissible: the "no path" outputs, and every mask word past
    waypoint 0 is written as zero.  (2) The same handle and shape under a far world and S = 1: every edge is free, so every output equals the
    unswept call's bit for bit (and that the numpy lattice); a word the sweep skipped is still zero and takes its destination's predecessors away."""
    import time

    from ikflow_amd.world import World
    from test_path import _check_against_dp, _inputs

    T, k = 1025, 256
    assert T * k * ((k + 63) // 64) > SWEEP_MAX_GRID >= (T - 1) * k * ((k + 63) // 64)   # the smallest T that crosses the cap
    orob = H.kin_robots("panda")[1]
    eng = _eng("panda")
    poses, q, _ = _inputs(orob, T, k, seed=T + k)
    opt = _popt()
    around = World()
    around.add_sphere((0.0, 0.0, 0.3), 10.0)
    eng.set_world(around, 0.0)
    eng.set_path_sweep(1)
    none = _path(eng, poses, q, k, opt)
    assert np.isposinf(none["node"]).all()
    assert np.isposinf(none["cost"][0]) and (none["index"] == -1).all() and (none["path"] == 0).all() and (none["reach"] == 0).all()
    far = World()
    far.add_sphere((50.0, 0.0, 0.0), 0.5)
    eng.set_world(far, 1.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    swept = _path(eng, poses, q, k, opt)
    t1 = time.perf_counter()
    eng.set_path_sweep(0)
    unswept = _path(eng, poses, q, k, opt)
    t2 = time.perf_counter()
    print(f"T {T} k {k}: {T * k * 4} mask words, {k * k * (T - 1)} swept edges; the call with the sweep {t1 - t0:.3f} s, without {t2 - t1:.3f} s (guarded buffers included)")
    assert np.isfinite(unswept["node"]).all() and np.isfinite(unswept["cost"][0])
    for n in OUTPUTS:
        assert PH.same_bits(swept[n], unswept[n]), f"{n}: the call under a sweep that blocks nothing differs from the unswept call, reachable_out tail {swept['reach'][-3:]}"
    _check_against_dp(unswept, q, T, k, opt, what="T1025_k256")


# ---- 6. a blocked crossing ---------------------------------------------------------------------------------------------------------------------------
def test_a_blocked_crossing_gives_the_no_path_outputs():
    """T = 2, k = 3: every candidate of waypoint 1 is one of waypoint 0 moved by 0.6 rad on one joint; a sphere of radius 0.03 sits on the last
    capsule's end point at the middle sample.  By the fp64 reference both nodes of every edge clear it by more than 1e-3 and every middle sample
    penetrates by more than 1e-3: without a sweep there is a path, with S = 1 there is none."""
    poses, q, world, nodes, mids = SH.crossing_case()
    assert nodes.min() > 1e-3 and mids.max() < -1e-3 and len(mids) == 9
    eng = _eng("panda")
    eng.set_world(world, 0.0)
    opt = _popt()
    free = _path(eng, poses, q, 3, opt)
    assert np.isfinite(free["node"]).all() and np.isfinite(free["cost"][0]) and (free["index"] >= 0).all() and (free["reach"] == 3).all()
    eng.set_path_sweep(1)
    out = _path(eng, poses, q, 3, opt)
    assert PH.same_bits(out["node"], free["node"])
    assert (out["path"] == 0).all() and (out["index"] == -1).all() and np.isposinf(out["cost"][0]) and list(out["reach"]) == [3, 0]
    a, b = SH.lattice_edges(q.numpy(), 2, 3)
    got = _sweep(eng, a, b, 1)
    assert (got["blocked"] == 1).all() and (got["first"] == 0).all()
    eng.set_path_sweep(2)   # two samples straddle the middle: at 1/3 and 2/3 of 0.6 rad the sphere is 0.1 rad of arc away - decided by the engine alone
    two = _path(eng, poses, q, 3, opt)
    ef, sf = _mask_of(eng, q, 2, 3, 2, opt, None)
    _check_against_masked_dp(two, q, 2, 3, opt, ef, sf, None, "crossing S 2")


# ---- 7. the flow in front ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False])
def test_generate_path_with_a_sweep_equals_the_flow_then_path_search(shared):
    from ikflow_amd.ikflow_solver import IKFlowSolver

    robot, hp, lay, sd = H.tiny_model()
    robot.set_collision_capsules(RH.collision_capsules(robot))
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    T, k, S = 33, 20, 4
    _, poses = H.reachable_poses(robot, T, 11)
    poses = poses.float()
    L = H.latents(k if shared else k * T, lay.dim, 12)
    expanded = L[:, None, :].expand(k, T, lay.dim).reshape(k * T, lay.dim).contiguous() if shared else L
    rows = s.generate_ik_solutions(poses.to(DEV).repeat((k, 1)), latent=expanded.to(DEV))
    world = WH.scene("panda", SH.LATTICE_SCENE)   # (the tiny model's robot is the Panda)
    s.set_world(world, 0.0)
    eng = s.engine(DEV)
    # not an accuracy claim: only a threshold that rejects about a quarter of these rows
    thr = float(torch.quantile(eng.world_clearance(rows)[0], 0.25))
    s.set_world(world, thr)
    s.set_path_sweep(S)
    assert eng.path_sweep == S
    opt = _popt(limits=True)
    one = _path(eng, poses, None, k, opt, latent=L, shared=shared)
    two = _path(eng, poses, rows.cpu(), k, opt)
    assert all(PH.same_bits(one[n], two[n]) for n in OUTPUTS)
    ef, sf = _mask_of(eng, rows.cpu(), T, k, S, opt, None)
    _check_against_masked_dp(one, rows.cpu(), T, k, opt, ef, sf, None, f"tiny shared {shared}")
    nb, nf = _admissible_edge_counts(one["node"], ef, sf, T, k)
    assert nb > 0 and nf > 0
    s.set_path_sweep(0)
    s.set_world(None)


# ---- 8. handle behaviour ---------------------------------------------------------------------------------------------------------------------------------
def test_after_set_path_sweep_and_reserve_path_a_call_of_that_size_allocates_nothing():
    """The method of tests/test_path.py::test_after_reserve_path_a_call_of_that_size_allocates_nothing, with a world and a sweep on the handle."""
    from ikflow_amd.engine import Engine
    from ikflow_amd.ikflow_solver import IKFlowSolver

    robot, hp, lay, sd = H.tiny_model()   # (a robot of this test's own: the capsule model must not reach the solvers other modules share)
    robot.set_collision_capsules(RH.collision_capsules(robot))
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    T, k = 300, 64
    _, poses = H.reachable_poses(robot, T, 3)
    poses = poses.float()
    Lk = H.latents(k, lay.dim, 5)
    opt = _popt(limits=True)

    def engine():
        eng = Engine(s.layout, robot, DEV)
        eng.load_state_dict(s._state_dict_np)
        eng.set_collision_model(*robot._collision_model)
        eng.set_world(WH.scene("panda", SH.LATTICE_SCENE), -0.05)
        eng.set_path_sweep(2)
        return eng

    def run(eng, tt, kk):
        return _path(eng, poses[:tt], None, kk, opt, latent=Lk[:kk], shared=True)

    eng = engine()
    eng.reserve_path(T, k)
    torch.cuda.synchronize()
    run(eng, 8, 4)                                                     # (torch's caching allocator warm for the test's own buffers)
    torch.cuda.synchronize()
    free0, stat0 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    full = run(eng, T, k)
    run(eng, 100, 50)
    run(eng, 1, 64)
    torch.cuda.synchronize()
    free1, stat1 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    grown_by_torch = stat1 - stat0
    assert free0 - free1 <= grown_by_torch, f"the engine allocated {free0 - free1 - grown_by_torch} bytes after ikf_set_path_sweep + ikf_reserve_path"
    fresh = engine()
    assert all(PH.same_bits(full[n], v) for n, v in run(fresh, T, k).items())   # (the reservation changes no result)


def test_a_sweep_on_one_handle_does_not_change_another():
    from ikflow_amd.engine import Engine

    T, k, which, L, S, q_start, opt = _lattice_case("T65_k33")
    robot, _ = H.kin_robots(which)
    eng = _eng(which)
    other = Engine(eng.layout, eng.robot, DEV)
    other.set_collision_model(*robot._collision_model)
    for e in (eng, other):
        e.set_world(L["world"], L["world_thr"])
    before_a, before_b = _path(eng, L["poses"], L["q"], k, opt), _path(other, L["poses"], L["q"], k, opt)
    assert all(PH.same_bits(before_a[n], before_b[n]) for n in OUTPUTS)
    eng.set_path_sweep(S)
    assert eng.path_sweep == S and other.path_sweep == 0
    after_a, after_b = _path(eng, L["poses"], L["q"], k, opt), _path(other, L["poses"], L["q"], k, opt)
    assert all(PH.same_bits(after_b[n], before_b[n]) for n in OUTPUTS)
    assert not PH.same_bits(after_a["index"], before_a["index"])


# ---- 9. the Python wrappers ------------------------------------------------------------------------------------------------------------------------------
def test_python_wrappers():
    from ikflow_amd.ikflow_solver import IKFlowSolver

    # Engine.sweep_edges == ikf_sweep_edges
    which = "panda"
    eng = _eng(which)
    c = SH.edge_case(which, "mixed7", 3)
    eng.set_world(c["world"], c["world_thr"])
    raw = _sweep(eng, c["a"], c["b"], 3, True, c["self_thr"])
    blocked, first = eng.sweep_edges(torch.tensor(c["a"]).to(DEV), torch.tensor(c["b"]).to(DEV), 3, reject_self=True, min_clearance=c["self_thr"])
    assert blocked.dtype == torch.bool and first.dtype == torch.int32
    assert np.array_equal(blocked.cpu().numpy(), raw["blocked"].astype(bool)) and np.array_equal(first.cpu().numpy(), raw["first"])
    # IKFlowSolver.set_path_sweep reaches the solver's handle; generate_ik_path honours it; path_collides of the path of test 4 is all False
    robot, hp, lay, sd = H.tiny_model()
    robot.set_collision_capsules(RH.collision_capsules(robot))
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    T, k, _, L, S, _, opt = _lattice_case("T65_k33")
    s.set_world(L["world"], L["world_thr"])
    s.set_path_sweep(S)
    seng = s.engine(DEV)
    assert seng.path_sweep == S and seng.world_size == len(L["world"])
    swept = seng.path_search(L["poses"].to(DEV), k, L["q"].to(DEV), opt)
    flags = s.path_collides(swept[0], S)
    assert flags.dtype == torch.bool and flags.shape == (T - 1,) and not bool(flags.any())
    v = _path_edge_verdicts("panda", L, swept[0].cpu().numpy(), S)
    assert not v["blocked"].any()
    s.set_path_sweep(0)
    unswept = seng.path_search(L["poses"].to(DEV), k, L["q"].to(DEV), opt)
    hit = s.path_collides(unswept[0], S).cpu().numpy()
    vu = _path_edge_verdicts("panda", L, unswept[0].cpu().numpy(), S)
    assert hit.any() and np.array_equal(hit[~vu["band"]], vu["blocked"][~vu["band"]])
    assert s.path_collides(unswept[0][:1], S).shape == (0,)
    # generate_ik_path under a sweep == without one on the same latents, except where the sweep forbids an edge; its signature is unchanged
    w = H.reachable_poses(robot, 33, 21)[1].float().to(DEV)
    Lk = H.latents(20, lay.dim, 22).to(DEV)
    rows = s.generate_ik_solutions(w.repeat((20, 1)), latent=Lk[:, None, :].expand(20, 33, lay.dim).reshape(660, lay.dim).contiguous())
    s.set_world(L["world"], float(torch.quantile(seng.world_clearance(rows)[0], 0.25)))
    a = s.generate_ik_path(w, 20, latent=Lk, reject_self_collisions=False, return_node_costs=True)
    s.set_path_sweep(S)
    b = s.generate_ik_path(w, 20, latent=Lk, reject_self_collisions=False, return_node_costs=True)
    assert torch.equal(a.node_costs, b.node_costs) and a._fields == b._fields
    if bool(torch.isfinite(b.cost)):
        assert not bool(s.path_collides(b.path, S).any()) and float(b.cost) >= float(a.cost)
    s.set_path_sweep(0)
    s.set_world(None)


# ---- 11. the 24-capsule model: the LDS slices of k_sweep_edges at their maximum, and a swept lattice ------------------------------------------------
LARGE_CHAINS = ("syn4r", "syn6r", "fetch")   # 4, 6 and 8 joints


@pytest.mark.parametrize("rule", ["world", "both"])
@pytest.mark.parametrize("which", LARGE_CHAINS)
def test_sweep_edges_with_24_capsules_in_the_64_obstacle_scene(which, rule, _small_model_back):
    """k_sweep_edges with 24 capsules and 64 obstacles - 41216 B of dynamic LDS, its maximum - on 1, 63, 64, 65 and 66 edges: flags exact outside
    the band, the first blocked sample exact when no earlier sample is in the band, under the world rule and under both rules (the self rule
    walks all the pairs of the model).  By the references alone the blocked share lies strictly between 10 % and 90 %, at most 2 % in the band."""
    eng = _eng_model(which, "caps24", _small_model_back)
    c = SH.edge_case(which, "full64", 1, "caps24")
    if rule == "both":
        SH.with_self_rule(c)
    assert 4 * (len(c["world"]) * 16 + 64 * ((6 * len(RH.capsules(which, "caps24"))) | 1)) == 41216
    eng.set_world(c["world"], c["world_thr"])
    v = SH.case_verdicts(c, rule)
    assert SH.shares_hold(v), SH.shares(v)
    for n in (1, 63, 64, 65, SH.N_EDGES_LARGE):
        out = _sweep(eng, c["a"][:n], c["b"][:n], 1, reject_self=rule == "both", self_min=c["self_thr"] or 0.0)
        assert set(np.unique(out["blocked"])) <= {0, 1} and ((out["first"] >= -1) & (out["first"] < 1)).all()
        SH.check_edges(out["blocked"], out["first"], SH.case_verdicts(c, rule, n), f"{which} full64 caps24 {rule} n {n}")
    print(f"{which} full64 caps24 {rule}: {int(out['blocked'].sum())} of {len(out['blocked'])} edges blocked, shares (band, blocked, free) {SH.shares(v)}")


def test_swept_lattice_with_24_capsules(_small_model_back):
    """k_path_lattice<7, true> with the 24-capsule model, the world and the self rule: the node costs are ikf_rank_candidates' row scores of the same
    rows under the same world, bit for bit; the path is the masked numpy lattice's on the verdicts of ikf_sweep_edges; blocked and free edges
    between admissible nodes both occur."""
    which, T, k, S = SH.LARGE_LATTICE
    L = SH.lattice_inputs(which, T, k, SH.LARGE_LATTICE_SEED, "caps24")
    eng = _eng_model(which, "caps24", _small_model_back)
    eng.set_world(L["world"], L["world_thr"])
    opt = _popt(collisions=True, min_clearance=L["self_thr"])
    eng.set_path_sweep(S)
    out = _path(eng, L["poses"], L["q"], k, opt)
    _check_nodes_are_rank_scores(eng, out, L["poses"], L["q"], k, opt)
    sure = (np.abs(L["world_cl"] - L["world_thr"]) > SH.BAND) & (np.abs(L["self_cl"] - L["self_thr"]) > SH.BAND)
    rejected = (L["world_cl"] < L["world_thr"]) | (L["self_cl"] < L["self_thr"])
    assert np.array_equal(np.isposinf(out["node"])[sure], rejected[sure]) and 0 < rejected[sure].sum() < sure.sum()
    ef, sf = _mask_of(eng, L["q"], T, k, S, opt, None)
    _check_against_masked_dp(out, L["q"], T, k, opt, ef, sf, None, "caps24 lattice")
    nb, nf = _admissible_edge_counts(out["node"], ef, sf, T, k)
    print(f"caps24 lattice: {nb} blocked and {nf} free edges between admissible nodes")
    assert nb > 0 and nf > 0 and np.isfinite(out["cost"][0])
