"""The per-row arithmetic of the kinematics kernels (ikflow_amd/csrc/kin_math.h: chain walk, quaternion, pose error, the LM step in both of its
arithmetics) compiled for the HOST with g++ and held against the oracle - the kernels' own source, checked without a GPU.  The GPU tests check the
same code where it ships (tests/test_gpu_parity.py); this one pins its arithmetic on every CPU run, and is how round 6 told a compiler effect
(fused multiply-adds in the fp32 LU elimination on the device) from an algorithmic one.  Test infrastructure: nothing in ikflow_amd/ loads it."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
from helpers import reachable_poses
from ikflow_amd.engine import fold_chain
from ikflow_amd.robots import get_robot
from oracle import kinematics_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("kin_math") / "libkin_math_host.so"
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "kin_math_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(str(out))
    lib.kin_math_host.restype = C.c_int
    lib.kin_math_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
    return lib


def _chain_bytes(robot, lib):
    joints, tool = fold_chain(robot)
    b = struct.pack("i", robot.ndof)
    for j in range(8):
        if j < len(joints):
            kind, ax, pre = joints[j]
            b += struct.pack("i", kind) + np.asarray(ax, dtype=np.float32).tobytes() + np.asarray(pre, dtype=np.float32).reshape(-1).tobytes()
        else:
            b += bytes(4 + 12 + 48)
    b += np.asarray(tool, dtype=np.float32).reshape(-1).tobytes()
    lo, hi = np.zeros(8, np.float32), np.zeros(8, np.float32)
    for i, (l, h) in enumerate(robot.actuated_joints_limits):
        lo[i], hi[i] = l, h
    b += lo.tobytes() + hi.tobytes()
    assert len(b) == lib.kin_math_chain_bytes()
    return C.create_string_buffer(b, len(b))


def _call(lib, chain, what, tgt, q, out_cols, two=False):
    n = q.shape[0]
    q = np.ascontiguousarray(q, dtype=np.float32)
    tgt = np.ascontiguousarray(tgt, dtype=np.float32) if tgt is not None else np.zeros((n, 7), np.float32)
    out = np.zeros((n, out_cols) if out_cols > 1 else (n,), np.float32)
    out2 = np.zeros(n, np.float32)
    assert lib.kin_math_host(chain, what, tgt.ctypes.data, q.ctypes.data, n, out.ctypes.data, out2.ctypes.data) == 0
    return (out, out2) if two else out


@pytest.mark.parametrize("which", ["panda", "fetch", "fetch_arm"])
def test_fk_and_pose_error_of_the_kernel_source_on_the_host(host_lib, which):
    robot = get_robot(which)
    chain = _chain_bytes(robot, host_lib)
    n = 2000
    q_true, poses = reachable_poses(robot, n, 11)
    fk = _call(host_lib, chain, 0, None, q_true.numpy(), 7)
    ref = ko.forward_kinematics(robot, q_true.double()).numpy()
    sign = np.sign((fk[:, 3:] * ref[:, 3:]).sum(1))[:, None]     # (q and -q are the same rotation)
    assert np.abs(fk[:, :3] - ref[:, :3]).max() <= 2e-6 and np.abs(fk[:, 3:] * sign - ref[:, 3:]).max() <= 2e-6
    seeds = ko.clamp_to_joint_limits(robot, q_true + 0.05 * torch.randn(q_true.shape, generator=torch.Generator().manual_seed(2)))
    pe, re = _call(host_lib, chain, 1, poses.numpy(), seeds.numpy(), 1, two=True)
    rpe, rre = ko.calculate_pose_error(robot, seeds, poses)
    assert np.abs(pe - rpe.numpy()).max() <= 2e-6 and np.abs(re - rre.numpy()).max() <= 3e-5


def test_lm_step_of_the_kernel_source_on_the_host_in_both_arithmetics(host_lib):
    """fp64 inside: within 5e-6 of the oracle's fp64 step on every row.  fp32 (the reference's arithmetic): the reference's own noise - in units of
    cond x 2^-24 x |dq| as close to the fp64 truth as the oracle's fp32 step (torch: bmm + sgesv), the rows next to a singularity included."""
    robot = get_robot("panda")
    chain = _chain_bytes(robot, host_lib)
    n = 4096
    q_true, poses = reachable_poses(robot, n, 0)
    seeds = ko.clamp_to_joint_limits(robot, q_true + 0.05 * torch.randn(q_true.shape, generator=torch.Generator().manual_seed(3)))
    ref64 = ko.lm_step(robot, poses.double(), seeds.double()).numpy()
    ref32 = ko.lm_step(robot, poses, seeds).numpy()
    J = ko.jacobian(robot, seeds.double())
    cond = torch.linalg.cond(J.transpose(1, 2) @ J + 1e-4 * torch.eye(7, dtype=torch.float64)).numpy()
    unit = cond * 2.0 ** -24 * np.maximum(np.abs(ref64 - seeds.numpy()).max(1), 1e-3)
    got64 = _call(host_lib, chain, 3, poses.numpy(), seeds.numpy(), 7)
    got32 = _call(host_lib, chain, 2, poses.numpy(), seeds.numpy(), 7)
    assert np.abs(got64 - ref64).max() <= 5e-6
    e32, eo = np.abs(got32 - ref64).max(1) / unit, np.abs(ref32 - ref64).max(1) / unit
    q = lambda e: (float(np.median(e)), float(np.quantile(e, 0.99)), float(e.max()))
    print("host build of the kernel source, fp32 step vs truth (median, p99, max in units of cond eps |dq|):", q(e32), " oracle fp32:", q(eo))
    assert cond.min() >= 1e3                                   # (rank-6 J^T J: no well-conditioned pose exists on a 7-joint arm)
    assert q(e32)[0] <= 1.5 * q(eo)[0] and q(e32)[1] <= 1.5 * q(eo)[1] and q(e32)[2] <= 4.0 and q(eo)[2] <= 4.0


# ---- every chain size and joint kind: the inputs and criteria of tests/test_kinematics.py (tests/helpers.py) through the host build ----------
class _Host:
    """The host build behind the backend interface of the shared checks in tests/helpers.py."""

    def __init__(self, lib, which):
        self.lib, self.robot = lib, H.kin_robots(which)[0]
        self.chain = _chain_bytes(self.robot, lib)

    def fk(self, q):
        return _call(self.lib, self.chain, 0, None, q, 7)

    def pose_error(self, q, tgt):
        return _call(self.lib, self.chain, 1, tgt, q, 1, two=True)

    def lm(self, tgt, q, mode):
        return _call(self.lib, self.chain, 3 if mode == "f64" else 2, tgt, q, self.robot.ndof)


@pytest.mark.parametrize("which", H.KIN_ALL)
def test_fk_and_position_error_on_every_chain_on_the_host(host_lib, which):
    b = _Host(host_lib, which)
    H.check_fk(b.fk, which)
    H.check_position_error(b.pose_error, which)


@pytest.mark.parametrize("noise", [0.15, 1.0])
@pytest.mark.parametrize("which", H.KIN_ALL)
def test_lm_step_on_hard_inputs_on_the_host(host_lib, which, noise):
    H.check_lm(_Host(host_lib, which).lm, which, noise)


@pytest.mark.parametrize("which", H.KIN_ALL)
def test_rotation_error_where_the_clamp_and_the_wrap_decide_on_the_host(host_lib, which):
    b = _Host(host_lib, which)
    orob = H.kin_robots(which)[1]
    parts = []
    for case, (q, tgt) in H.pose_error_cases(orob, 20000).items():
        pe, re = b.pose_error(q.numpy(), tgt.numpy())
        ref_pe, _ = ko.calculate_pose_error(orob, q.double(), tgt.double())
        assert np.abs(pe - ref_pe.numpy()).max() <= 2e-6
        parts.append(H.check_rot_error(case, re, *H.rot_reference(orob, q, tgt)))
    H.check_rot_below_floor(which, parts)


def test_rotation_error_floor_is_where_the_f32_oracle_meets_1e_5():
    """H.ROT_FLOOR is derived, not tuned: over every chain and seed distance the f32 oracle is within 1e-5 of the fp64 oracle on every row whose
    fp64 angle is above it (and it is not idle: below it the f32 oracle does leave 1e-5)."""
    worst_above, highest_bad = 0.0, 0.0
    for which in H.KIN_ALL:
        orob = H.kin_robots(which)[1]
        for case, (q, tgt) in H.pose_error_cases(orob, 20000).items():
            if not case.startswith("noise"):
                continue
            r64, r32 = H.rot_reference(orob, q, tgt)
            d = np.abs(r32 - r64)
            worst_above = max(worst_above, float(d[r64 > H.ROT_FLOOR].max(initial=0.0)))
            highest_bad = max(highest_bad, float(r64[d > 1e-5].max(initial=0.0)))
    print(f"f32 oracle vs fp64: worst above the floor {worst_above:.2e}; highest angle with more than 1e-5: {highest_bad:.4f} rad")
    assert worst_above <= 1e-5 and 0.0 < highest_bad <= H.ROT_FLOOR


def test_spread_of_the_f32_oracles_own_maximum():
    """Where H.LM_MAX_MARGIN comes from - the oracle alone, no kernel: the maximum of the f32 oracle's error over the even rows
    against the maximum over the odd rows of the same sample, the worst ratio over every chain.  The margin of the LM maximum is that spread rounded
    up (1.5 x would refuse the oracle's own odd rows against its even rows); for the rotation error below the floor 1.5 x covers it."""
    half = lambda e: max(e[0::2].max(), e[1::2].max()) / min(e[0::2].max(), e[1::2].max())
    lm, rot = 0.0, 0.0
    for which in H.KIN_ALL:
        orob = H.kin_robots(which)[1]
        for noise in (0.15, 1.0):
            poses, seeds, _ = H.lm_inputs(orob, 20000, noise, 21)
            keep = ~H.lm_near_branch(orob, poses, seeds)
            ref64 = ko.lm_step(orob, poses.double(), seeds.double()).numpy()
            ref32 = ko.lm_step(orob, poses, seeds).numpy().astype(np.float64)
            J = ko.jacobian(orob, seeds.double())
            cond = torch.linalg.cond(J.transpose(1, 2) @ J + 1e-4 * torch.eye(orob.ndof, dtype=torch.float64)).numpy()
            unit = cond * 2.0 ** -24 * np.maximum(np.abs(ref64 - seeds.numpy()).max(1), 1e-3)
            lm = max(lm, half((np.abs(ref32 - ref64).max(1) / unit)[keep]))
        low = []
        for case, (q, tgt) in H.pose_error_cases(orob, 20000).items():
            if case.startswith("noise"):
                r64, r32 = H.rot_reference(orob, q, tgt)
                low.append(np.abs(r32 - r64)[r64 <= H.ROT_FLOOR])
        rot = max(rot, half(np.concatenate(low)))
    print(f"f32 oracle, maximum over the even rows against the odd rows, worst chain: LM step {lm:.2f} x, rotation error below the floor {rot:.2f} x")
    assert 1.5 < lm <= H.LM_MAX_MARGIN and rot <= H.LM_MARGIN
