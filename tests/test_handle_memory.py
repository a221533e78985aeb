"""The handle's own device and pinned memory (ikflow_amd/csrc/device_buf.h, struct ikf_model): one engine is taken through the calls that
create, regrow and re-create its buffers - flow scratch, exact-IK rows and poses, the weight arena and the images built from it, the
cluster form's exchange buffers, the collision model and the world - and every result has the bits of the same call on a fresh engine.
Then the engine goes, and the device's free memory is back to what it was before the engine was created, up to what torch's own cache
grew (the accounting of tests/test_ranked.py::test_candidate_buffers_regrow_across_families_and_are_released_with_the_handle: the
baseline is taken after the fresh engines of the references are gone, since what the runtime loads with the first launch of a kernel
is not the engine's).  That check sees what is large enough to move the device's free-memory figure - arenas, images, scratch, exchange
buffers; the single words and tables (collision model, world, the create-time and pinned words) are below its grain: for them this file
checks results only, and tests/device_buf_host.cpp that an owning member frees what it holds."""
import gc

import pytest
import torch

import helpers as H
import rank_helpers as RH
from ikflow_amd import _lib
from ikflow_amd.engine import Engine
from ikflow_amd.ikflow_solver import IKFlowSolver

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(outs):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (outs if isinstance(outs, (tuple, list)) else (outs,))]


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert H.same_bits(g, w), f"{what}: output {i} differs from a fresh engine's"


def _state_dicts(hp, robot, sds):
    """The engine's own numpy form of each state dict, through the solver's loader."""
    out = []
    for sd in sds:
        s = IKFlowSolver(hp, robot)
        s.load_state_dict_tensors(sd)
        out.append(s._state_dict_np)
    return s.layout, out


def _check_released(free0, stat0):
    gc.collect()
    torch.cuda.synchronize()
    free1, stat1 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    assert free0 - free1 <= stat1 - stat0, f"{free0 - free1 - (stat1 - stat0)} bytes of device memory did not come back with the handle"


def test_tiny_model_scratch_regrows_weights_reload_and_everything_is_released():
    """TINY model (per-layer kernels at every size).  Approximate calls of 100, 700 and 100 rows regrow the flow scratch; exact IK after
    reserve_exact for 8 poses runs 200 poses with repeat counts (1, 3, 10) and no up-front worst case, so the pose buffers regrow at the
    call's start and the row buffers between the rounds (the per-round flow rows of the statistics must rise, or nothing regrew).  Then a
    second state dict (seed 2) is loaded into the same handle and the same calls have the bits of a fresh engine of those weights."""
    robot, hp, lay, sd0 = H.tiny_model()
    sd2 = H.tiny_model(seed=2)[3]
    layout, sds = _state_dicts(hp, robot, (sd0, sd2))
    n_exact, repeats = 200, (1, 3, 10)
    _, poses = H.reachable_poses(robot, 700, 3)
    poses = poses.float().to(DEV)
    L = H.latents(700, lay.dim, 5).to(DEV)
    LX = [H.latents(n_exact * r, lay.dim, 7 + i).to(DEV) for i, r in enumerate(repeats)]

    def engine(sd):
        eng = Engine(layout, robot, DEV)
        eng.load_state_dict(sd)
        eng.set_exact_upfront_rows(0)   # (rows for round 0 only; later rounds grow to their measured survivors)
        return eng

    def approx(eng, n):
        return eng.generate_approx(poses[:n], L[:n], True)

    def exact(eng, n):
        sol, valid, stats = eng.generate_exact(poses[:n], repeats, 1e-4, 1e-3, latents=LX, n_lm_steps=1, return_stats=True)
        rows = [int(r) for r in stats[:, 1]]
        assert rows[0] == n and rows[0] < rows[1] < rows[2], f"the row state did not grow between the rounds: flow rows {rows}"
        return sol, valid

    calls = [(approx, 100), (approx, 700), (approx, 100), (exact, n_exact)]
    want = []
    for sd in sds:
        for call, n in calls[1:]:
            fresh = engine(sd)
            want.append(_bits(call(fresh, n)))
            del fresh
    want = {(w, call, n): want[w * 3 + i] for w in range(2) for i, (call, n) in enumerate(calls[1:])}
    gc.collect()
    torch.cuda.synchronize()
    free0, stat0 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    eng = engine(sds[0])
    eng.reserve_exact(8, 10)
    for w, sd in enumerate(sds):
        if w:
            eng.load_state_dict(sd)
        for call, n in calls:
            _same(_bits(call(eng, n)), want[w, call, n], f"weights {w}: {call.__name__} of {n}")
    del eng
    _check_released(free0, stat0)


def test_resident_row_model_every_image_and_buffer_is_rebuilt_by_a_reload_and_released():
    """The smallest model that takes the resident-row forms (2 blocks, 3 hidden layers of width 1024): 16, 200 and 4096 rows plan the
    cluster form with 32 and 16 members and the row-owner launch (the row-owner stream, its tables, the exchange buffers); 100 and 700
    rows with both forms switched off (ikf_set_gemm_variant 180 / 185) run the per-layer kernels, which build the fragment image and
    regrow the flow scratch; 300 rows in the f16x3 mode build the split images.  The seed-2 weights are then loaded while that mode is
    still on (the reload rebuilds the split images itself) and all calls are repeated against fresh engines of those weights.  Last, a
    collision model and a one-sphere world are set and read, again with the bits of a fresh engine."""
    robot, hp, lay, sd0 = H.custom_model(nb_nodes=2, n_hidden=3, width=1024)
    sd2 = H.custom_model(nb_nodes=2, n_hidden=3, width=1024, seed=2)[3]
    layout, sds = _state_dicts(hp, robot, (sd0, sd2))
    _, poses = H.reachable_poses(robot, 4096, 3)
    poses = poses.float().to(DEV)
    L = H.latents(4096, lay.dim, 5).to(DEV)
    # (name, rows, resident-row forms on, precision, the plan)
    calls = [("cluster32", 16, True, "f32", "cluster32:16"), ("cluster16", 200, True, "f32", "cluster16:200"),
             ("rowowner", 4096, True, "f32", "rowowner:4096"), ("perlayer", 100, False, "f32", "perlayer:100"),
             ("perlayer", 700, False, "f32", "perlayer:700"), ("f16x3", 300, True, "f16x3", "perlayer:300")]

    def engine(sd):
        eng = Engine(layout, robot, DEV)
        eng.load_state_dict(sd)
        return eng

    def run(eng, name, n, resident, precision, plan):
        eng.set_precision(precision)
        eng.set_gemm_variant(181 if resident else 180)
        eng.set_gemm_variant(186 if resident else 185)
        assert eng.plan(n) == plan, (name, n, eng.plan(n))
        return eng.generate_approx(poses[:n], L[:n], True)

    robot.set_collision_capsules(RH.collision_capsules(robot))

    def world(eng):
        eng.set_collision_model(*robot._collision_model)
        eng.set_world([(_lib.IKF_OBSTACLE_SPHERE, (0.4, 0.0, 0.5), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), 0.1)], 0.0)
        assert eng.world_size == 1
        q = run(eng, *calls[0])
        return eng.self_collision(q) + eng.world_clearance(q)

    def sequence(eng):
        for w, sd in enumerate(sds):
            if w:
                assert eng.precision == "f16x3"
                eng.load_state_dict(sd)
            for c in calls:
                _same(_bits(run(eng, *c)), want[w, c], f"weights {w}: {c[0]} of {c[1]} rows")
            assert eng.frag_image_time_ms > 0.0 and eng.cluster_repairs == 0
        _same(_bits(world(eng)), want_world, "self collision and world clearance")

    want = {}
    for w, sd in enumerate(sds):
        for c in calls:
            fresh = engine(sd)
            want[w, c] = _bits(run(fresh, *c))
            del fresh
    fresh = engine(sds[1])
    want_world = _bits(world(fresh))
    del fresh
    gc.collect()
    torch.cuda.synchronize()
    free0, stat0 = torch.cuda.mem_get_info(DEV)[0], torch.cuda.memory_reserved(DEV)
    eng = engine(sds[0])
    sequence(eng)
    del eng
    _check_released(free0, stat0)
