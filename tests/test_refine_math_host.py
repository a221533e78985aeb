"""The loop of one refined candidate row (ikflow_amd/csrc/refine_math.h over kin_math.h) compiled for the HOST with g++ and held against a loop of
the oracle (tests/refine_helpers.py) - the kernel's own source, checked without a GPU.  The GPU tests check the same code where it ships
(tests/test_refine.py).  Test infrastructure: nothing in ikflow_amd/ loads it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import refine_helpers as RH
from oracle import kinematics_oracle as ko
from test_kin_math_host import _chain_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("refine_math") / "librefine_math_host.so"
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "refine_math_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(str(out))
    lib.refine_math_host.restype = C.c_int
    lib.refine_math_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_float, C.c_float,
                                     C.c_void_p, C.c_void_p, C.c_void_p]
    lib.refine_math_blocks.restype = C.c_longlong
    lib.refine_math_blocks.argtypes = [C.c_longlong]
    lib.kin_math_chain_bytes = lib.refine_math_chain_bytes   # (what _chain_bytes asks for)
    return lib


def _refine(lib, which, poses, q, n_steps, pos_tol, rot_tol, mode="f64", info=True):
    robot = H.kin_robots(which)[0]
    chain = _chain_bytes(robot, lib)
    poses = np.ascontiguousarray(poses, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    rows = q.shape[0]
    out = np.full_like(q, 7.0)
    steps, conv = np.full(rows, 99, np.uint8), np.full(rows, 99, np.uint8)
    assert lib.refine_math_host(chain, 1 if mode == "f64" else 0, poses.ctypes.data, poses.shape[0], q.ctypes.data, rows, n_steps, pos_tol, rot_tol,
                                out.ctypes.data, steps.ctypes.data if info else None, conv.ctypes.data if info else None) == 0
    return out, steps, conv


@pytest.mark.parametrize("pos_tol,rot_tol", RH.TOLERANCES)
@pytest.mark.parametrize("which", RH.CHAINS)
def test_refine_row_against_a_loop_of_the_oracle(host_lib, which, pos_tol, rot_tol):
    """600 rows of truth + 0.05 rad, 4 steps.  fp64 mode: steps, converged and the rows against the oracle loop outside the band (at most 3 % of
    the rows), |dq| <= 5e-6 + 8 x the row's own twin sensitivity.  f32 mode: the statistical form of check_lm on the final rows."""
    case = RH.oracle_case(which, 600, 1, pos_tol, rot_tol)
    q, steps, conv = _refine(host_lib, which, case["poses"].numpy(), case["seeds"].numpy(), RH.N_STEPS, pos_tol, rot_tol)
    assert set(np.unique(conv)) <= {0, 1}
    n_band = RH.check_against_oracle(case, q, steps, conv)
    assert n_band <= RH.BAND_CAP * 600, n_band
    if which == "panda" and (pos_tol, rot_tol) == (1e-3, 0.1):
        counts = np.bincount(case["ref"][1].numpy(), minlength=RH.N_STEPS + 1)[1:]
        assert (counts > 0).all() and (np.bincount(steps, minlength=RH.N_STEPS + 1)[1:] > 0).all(), counts   # every step count 1 .. 4 occurs
    q32, _, _ = _refine(host_lib, which, case["poses"].numpy(), case["seeds"].numpy(), RH.N_STEPS, pos_tol, rot_tol, mode="f32")
    RH.check_f32_against_oracle([RH.f32_distances(case, q32)], f"{which} tol ({pos_tol:g}, {rot_tol:g})")


@pytest.mark.parametrize("which", ["panda", "syn4p", "syn8p"])
def test_refine_row_edge_cases(host_lib, which):
    """Tolerance 0 runs every step and never converges; n_steps = 1 is one lm_step_row, bit for bit, in both arithmetics; a rot_tol at or below
    the f32 rotation error's floor (2 acosf(1 - 1e-7) = 9.77e-4) never converges; a NaN row comes out as that many lm_step_row calls leave it (the
    step's clamp maps a NaN joint to a limit) and leaves the other rows as they are without it; the tile position picks the pose; every output inside the limits exactly; null info outputs."""
    robot, orob = H.kin_robots(which)
    poses, seeds = RH.refine_inputs(which, 50, 3, seed=5)
    poses, seeds = poses.numpy(), seeds.numpy()
    lo = np.array([l[0] for l in orob.actuated_joints_limits], np.float32)
    hi = np.array([l[1] for l in orob.actuated_joints_limits], np.float32)
    for mode in ("f64", "f32"):
        q, steps, conv = _refine(host_lib, which, poses, seeds, 5, 0.0, 0.0, mode)
        assert (steps == 5).all() and (conv == 0).all() and (q >= lo).all() and (q <= hi).all()
        for tol in ((0.0, 1.0), (1.0, 0.0)):                                  # one tolerance of 0 is enough to never stop
            _, s2, c2 = _refine(host_lib, which, poses, seeds, 5, *tol, mode)
            assert (s2 == 5).all() and (c2 == 0).all()
        q1, s1, c1 = _refine(host_lib, which, poses, seeds, 1, 10.0, 10.0, mode)   # already inside the tolerances: still one step
        assert (s1 == 1).all() and (c1 == 1).all()
        one = _one_lm_step(host_lib, which, np.tile(poses, (3, 1)), seeds, mode)
        assert H.same_bits(q1, one)
        q9, s9, c9 = _refine(host_lib, which, poses, seeds, 6, 1.0, 9e-4, mode)
        assert (s9 == 6).all() and (c9 == 0).all()
        assert 9e-4 < H.ACOS_CLAMP_ANGLE < 9.8e-4
        qn, sn, cn = _refine(host_lib, which, poses, seeds, 6, 1.0, np.float32(H.ACOS_CLAMP_ANGLE), mode)   # at the floor: `<` is never true
        assert (sn == 6).all() and (cn == 0).all()
        bad = seeds.copy()
        bad[7, 1] = np.nan
        qb, sb, cb = _refine(host_lib, which, poses, bad, 4, 1e-3, 0.1, mode)
        qg, sg, cg = _refine(host_lib, which, poses, seeds, 4, 1e-3, 0.1, mode)
        assert 1 <= sb[7] <= 4 and cb[7] in (0, 1)
        others = np.arange(len(seeds)) != 7
        assert H.same_bits(qb[others], qg[others]) and np.array_equal(sb[others], sg[others]) and np.array_equal(cb[others], cg[others])
        assert H.same_bits(qb[7], _iterate_lm(host_lib, which, poses[7:8], bad[7:8], int(sb[7]), mode)[0])   # as lm_step_row leaves it
        assert (qg >= lo).all() and (qg <= hi).all()
        tiled, _, _ = _refine(host_lib, which, np.tile(poses, (3, 1)), seeds, 4, 1e-3, 0.1, mode)   # row r of 150 poses = pose r % 50 of 50
        assert H.same_bits(tiled, qg)
        quiet, s0, c0 = _refine(host_lib, which, poses, seeds, 4, 1e-3, 0.1, mode, info=False)
        assert H.same_bits(quiet, qg) and (s0 == 99).all() and (c0 == 99).all()


def _one_lm_step(lib, which, tiled_poses, q, mode):
    """One lm_step_row per row through the kin_math host build (tests/kin_math_host.cpp), compiled here with the flags of refine_math_host.cpp."""
    if not hasattr(_one_lm_step, "lib"):
        import tempfile

        out = os.path.join(tempfile.mkdtemp(prefix="kin_math_"), "libkin_math_host.so")
        cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "kin_math_host.cpp"), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        klib = C.CDLL(out)
        klib.kin_math_host.restype = C.c_int
        klib.kin_math_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
        _one_lm_step.lib = klib
    klib = _one_lm_step.lib
    robot = H.kin_robots(which)[0]
    chain = _chain_bytes(robot, klib)
    q = np.ascontiguousarray(q, np.float32)
    tgt = np.ascontiguousarray(tiled_poses, np.float32)
    res = np.zeros_like(q)
    dummy = np.zeros(q.shape[0], np.float32)
    assert klib.kin_math_host(chain, 3 if mode == "f64" else 2, tgt.ctypes.data, q.ctypes.data, q.shape[0], res.ctypes.data, dummy.ctypes.data) == 0
    return res


def _iterate_lm(lib, which, poses, q, n, mode):
    for _ in range(n):
        q = _one_lm_step(lib, which, poses, q, mode)
    return q


def test_refine_launch_geometry(host_lib):
    assert [host_lib.refine_math_blocks(r) for r in (1, 255, 256, 257, 2 ** 31 - 1)] == [1, 1, 1, 2, 2 ** 23]
    assert host_lib.refine_math_max_steps() == 16
