"""The kinematics half of the C-ABI (ikflow_amd/csrc/kin_kernels.hip, kin_math.h) at every chain size, joint kind and batch edge.

Every kernel of IKF_NDOF_DISPATCH (ndof 4 .. 8) runs here, on synthetic chains with oblique axes, fixed joints in between and prismatic joints
first, in the middle and last (helpers.synthetic_chain: the same URDF text through the product's reader and the oracle's own), next to Panda,
FetchArm and Fetch; every row is compared with the oracle in fp64.  The inputs and criteria of FK, position / rotation error and the LM step
are shared with the host build of the same source (tests/helpers.py, tests/test_kin_math_host.py), which runs them on every CPU run.

Tolerances are the project's: FK and position error 2e-6, Jacobian 3e-6, rotation error 2e-5 (above helpers.ROT_FLOOR), capsule clearance 2e-5,
LM step 5e-6 where it is known to hold (built-in robots, seeds 0.15 rad off); clamp, limit flags and batch-edge comparisons are bit-exact.  The
statistical criteria of the new inputs (kernel quantile <= margin x the f32 oracle's quantile on the same rows) are stated in helpers.check_lm /
check_rot_below_floor; the ratios measured on the MI355X are in the docstrings below."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import helpers as H
from ikflow_amd import _lib
from oracle import kinematics_oracle as ko
from oracle import robot_tables as rt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCH_SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]   # a block is 256 threads (64 for k_self_collision)
GUARD = 64                                           # guard rows in front of and behind every input and output window
NAN_BITS = 0x7FC00000


def _eng(which):
    from ikflow_amd.engine import kinematics_engine_for

    return kinematics_engine_for(H.kin_robots(which)[0], DEV)


class _Gpu:
    """The HIP path behind the backend interface of the shared checks in tests/helpers.py."""

    def __init__(self, which):
        self.eng = _eng(which)

    def fk(self, q):
        return self.eng.forward_kinematics(torch.from_numpy(q).to(DEV)).cpu().numpy()

    def pose_error(self, q, tgt):
        pe, re = self.eng.pose_error(torch.from_numpy(q).to(DEV), torch.from_numpy(tgt).to(DEV))
        return pe.cpu().numpy(), re.cpu().numpy()

    def lm(self, tgt, q, mode):
        self.eng.set_lm_precision(mode)
        try:
            return self.eng.lm_step(torch.from_numpy(tgt).to(DEV), torch.from_numpy(q).to(DEV)).cpu().numpy()
        finally:
            self.eng.set_lm_precision("f64")


# ---- 1. FK, position error, Jacobian, clamp, limit flags on every chain ------------------------------------------------------------------
@pytest.mark.parametrize("which", H.KIN_ALL)
def test_fk_and_position_error_on_every_chain(which):
    b = _Gpu(which)
    H.check_fk(b.fk, which)
    H.check_position_error(b.pose_error, which)


def _fd_jacobian(orob, q, h=1e-6):
    """Central differences of the oracle's fp64 FK: position columns, and angular columns from R(q + h) R(q - h)^T = I + 2h [w]x + O(h^3).
    Truncation O(h^2) = 1e-12, rounding 1e-16 / 2h = 5e-11: nothing next to the 3e-6 it is compared at."""
    n, nd = q.shape
    J = torch.zeros(n, 6, nd, dtype=torch.float64)
    for j in range(nd):
        qp, qm = q.clone(), q.clone()
        qp[:, j] += h
        qm[:, j] -= h
        Tp, Tm = ko._chain_transforms(orob, qp)[0], ko._chain_transforms(orob, qm)[0]
        dR = Tp[:, :3, :3] @ Tm[:, :3, :3].transpose(1, 2)
        J[:, 0, j] = (dR[:, 2, 1] - dR[:, 1, 2]) / (4 * h)
        J[:, 1, j] = (dR[:, 0, 2] - dR[:, 2, 0]) / (4 * h)
        J[:, 2, j] = (dR[:, 1, 0] - dR[:, 0, 1]) / (4 * h)
        J[:, 3:, j] = (Tp[:, :3, 3] - Tm[:, :3, 3]) / (2 * h)
    return J


@pytest.mark.parametrize("which", H.KIN_ALL)
def test_jacobian_against_the_oracle_and_against_central_differences_of_its_fk(which):
    """k_jacobian has its own copy of the Jacobian columns.  Against the oracle's Jacobian in fp64, and - so that a convention shared by the two
    cannot hide - against central differences of the oracle's FK, both at the project's 3e-6."""
    robot, orob = H.kin_robots(which)
    q = torch.tensor(orob.sample_joint_angles(4000, 0.0, np.random.default_rng(9)))
    J = _eng(which).jacobian(q.to(DEV)).cpu().double()
    d_ref = (J - ko.jacobian(orob, q.double())).abs().max().item()
    d_fd = (J - _fd_jacobian(orob, q.double())).abs().max().item()
    print(f"jacobian {which}: vs oracle {d_ref:.2e}, vs central differences of the oracle's FK {d_fd:.2e}")
    assert d_ref <= 3e-6 and d_fd <= 3e-6, (d_ref, d_fd)
    kinds = [j.kind for j in orob.joints if j.actuated]
    for j, kind in enumerate(kinds):   # a prismatic column has no angular part, exactly
        if kind == rt.PRISMATIC:
            assert (J[:, :3, j] == 0).all() and (J[:, 3:, j].norm(dim=1) - 1).abs().max().item() <= 3e-6


@pytest.mark.parametrize("which", H.KIN_ALL)
def test_clamp_and_limit_flags_are_bit_equal_to_the_oracle(which):
    robot, orob = H.kin_robots(which)
    eng = _eng(which)
    lims = orob.actuated_joints_limits
    wild = 5.0 * torch.randn(3001, orob.ndof, generator=torch.Generator().manual_seed(1))   # (3001 x ndof: i % ndof walks every joint in every block)
    edge, exceeded = H.limit_edge_rows(orob)
    edge = torch.from_numpy(edge)
    for cfg in (wild, edge):
        cl = eng.clamp_to_joint_limits(cfg.to(DEV)).cpu()
        assert torch.equal(cl, ko.clamp_to_joint_limits(orob, cfg))
        ex = eng.joint_limits_exceeded(cfg.to(DEV)).cpu()
        assert torch.equal(ex, ko.calculate_joint_limits_exceeded(cfg, lims))
        from ikflow_amd import evaluation_utils as eu

        assert torch.equal(eu.calculate_joint_limits_exceeded(cfg.to(DEV), lims).cpu(), ex)     # ikf_limits_exceeded, the same table
    assert np.array_equal(eng.joint_limits_exceeded(edge.to(DEV)).cpu().numpy(), exceeded)        # on a limit: not exceeded; one ulp beyond: exceeded
    inside = eng.clamp_to_joint_limits(edge.to(DEV)).cpu().numpy()
    assert np.array_equal(inside != edge.numpy(), (edge.numpy() > np.array([l[1] for l in lims], np.float32)) | (edge.numpy() < np.array([l[0] for l in lims], np.float32)))


# ---- 2. / 3. batch edges, guards, aliasing: every entry point through eng.lib ---------------------------------------------------------------
class _EntryPoint:
    def __init__(self, name, inputs, outputs, call, before=None):
        self.name, self.inputs, self.outputs, self.call, self.before = name, inputs, outputs, call, before


def _collision_capsules(robot):
    """A small capsule model for any chain: base, three moving links, a sphere."""
    act = [j.name for j in robot.joints if j.actuated]
    rng = np.random.default_rng(5)
    caps = [(None, (0.0, 0.0, 0.0), (0.0, 0.0, 0.2), 0.05)]
    for nm in (act[1], act[2], act[-1]):
        caps.append((nm, tuple(rng.uniform(-0.08, 0.08, 3)), tuple(rng.uniform(-0.15, 0.15, 3)), float(rng.uniform(0.03, 0.08))))
    caps.append((act[-1], (0.01, 0.02, 0.03), (0.01, 0.02, 0.03), 0.04))
    return caps


_EP_CACHE = {}


def _entry_points(which):
    """Every kinematics entry point of include/ikflow_amd.h with 1000 rows of input: {name: _EntryPoint}."""
    if which in _EP_CACHE:
        return _EP_CACHE[which]
    robot, orob = H.kin_robots(which)
    eng = _eng(which)
    lib, h, nd = eng.lib, eng._h, orob.ndof
    n = 1000
    q = torch.tensor(orob.sample_joint_angles(n, 0.0, np.random.default_rng(2)))
    _, tgt = H.reachable_poses(orob, n, 3)
    near = ko.clamp_to_joint_limits(orob, torch.tensor(orob.sample_joint_angles(n, 0.0, np.random.default_rng(3))) + 0.3 * torch.randn(n, nd, generator=torch.Generator().manual_seed(4)))
    lo = torch.tensor([l[0] for l in orob.actuated_joints_limits], dtype=torch.float32)
    hi = torch.tensor([l[1] for l in orob.actuated_joints_limits], dtype=torch.float32)
    wild = lo + (hi - lo) * (1.4 * torch.rand(n, nd, generator=torch.Generator().manual_seed(5)) - 0.2)
    poses_a = ko.forward_kinematics(orob, near)
    h_lo, h_hi = (C.c_float * nd)(*lo.tolist()), (C.c_float * nd)(*hi.tolist())
    robot.set_collision_capsules(_collision_capsules(robot))

    def collision_model():
        eng.set_collision_model(*robot._collision_model)

    def lm(mode):
        return lambda: eng.set_lm_precision(mode)

    f32, u8 = torch.float32, torch.uint8
    eps = [
        _EntryPoint("ikf_forward_kinematics", [q], [(7, f32)], lambda i, m, o, s: lib.ikf_forward_kinematics(h, i[0], m, o[0], s)),
        _EntryPoint("ikf_pose_error", [near, tgt], [(1, f32), (1, f32)], lambda i, m, o, s: lib.ikf_pose_error(h, i[0], i[1], m, o[0], o[1], s)),
        _EntryPoint("ikf_lm_step[f64]", [tgt, near], [(nd, f32)], lambda i, m, o, s: lib.ikf_lm_step(h, i[0], i[1], m, o[0], s), lm("f64")),
        _EntryPoint("ikf_lm_step[f32]", [tgt, near], [(nd, f32)], lambda i, m, o, s: lib.ikf_lm_step(h, i[0], i[1], m, o[0], s), lm("f32")),
        _EntryPoint("ikf_jacobian", [q], [(6 * nd, f32)], lambda i, m, o, s: lib.ikf_jacobian(h, i[0], m, o[0], s)),
        _EntryPoint("ikf_clamp_to_joint_limits", [wild], [(nd, f32)], lambda i, m, o, s: lib.ikf_clamp_to_joint_limits(h, i[0], m, o[0], s)),
        _EntryPoint("ikf_joint_limits_exceeded", [wild], [(1, u8)], lambda i, m, o, s: lib.ikf_joint_limits_exceeded(h, i[0], m, o[0], s)),
        _EntryPoint("ikf_self_collision", [q], [(1, f32), (1, u8)], lambda i, m, o, s: lib.ikf_self_collision(h, i[0], m, o[0], o[1], s), collision_model),
        _EntryPoint("ikf_pose_distance", [poses_a, tgt], [(1, f32), (1, f32)], lambda i, m, o, s: lib.ikf_pose_distance(i[0], i[1], m, -1.0, o[0], o[1], s)),
        _EntryPoint("ikf_limits_exceeded", [wild], [(1, u8)], lambda i, m, o, s: lib.ikf_limits_exceeded(i[0], m, nd, h_lo, h_hi, o[0], s)),
    ]
    for ep in eps:
        ep.inputs = [t.to(DEV) for t in ep.inputs]
        ep.eng = eng
    _EP_CACHE[which] = {ep.name: ep for ep in eps}
    return _EP_CACHE[which]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _run(ep, idx, stream=None, alias=None):
    """Call `ep` on the input rows `idx`.  Inputs and outputs are windows of len(idx) rows inside buffers with GUARD rows in front and behind
    (inputs: zeros; outputs: NaN, or 0xAB for bytes).  Checks the status, that both guards of every output are untouched and that every element of
    the window was written.  alias = (k_out, k_in): output k_out is written over input k_in.  Returns the output windows (device tensors)."""
    idx = torch.as_tensor(idx, device=DEV)
    m = int(idx.numel())
    ins = []
    for t in ep.inputs:
        buf = torch.zeros((m + 2 * GUARD, t.shape[1]), dtype=t.dtype, device=DEV)
        buf[GUARD:GUARD + m] = t[idx]
        ins.append(buf)
    outs = []
    for k, (cols, dt) in enumerate(ep.outputs):
        if alias is not None and alias[0] == k:
            outs.append(ins[alias[1]])
            continue
        buf = torch.full((m + 2 * GUARD, cols), float("nan"), dtype=torch.float32, device=DEV) if dt == torch.float32 else \
            torch.full((m + 2 * GUARD, cols), 0xAB, dtype=torch.uint8, device=DEV)
        outs.append(buf)
    if ep.before is not None:
        ep.before()
    torch.cuda.synchronize()
    s = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(0)
    try:
        code = ep.call([b[GUARD:].data_ptr() for b in ins], m, [b[GUARD:].data_ptr() for b in outs], s)
    finally:
        ep.eng.set_lm_precision("f64")
    assert code == _lib.IKF_OK, (ep.name, code, _lib.last_error(ep.eng.lib))
    torch.cuda.synchronize()
    res = []
    for k, (buf, (cols, dt)) in enumerate(zip(outs, ep.outputs)):
        win = buf[GUARD:GUARD + m]
        if alias is not None and alias[0] == k:   # (the guards of an aliased buffer are input guards: zeros)
            assert not buf[:GUARD].any() and not buf[GUARD + m:].any(), f"{ep.name}: a row outside the {m} rows was written"
        elif dt == torch.float32:
            assert (_bits(buf[:GUARD]) == NAN_BITS).all() and (_bits(buf[GUARD + m:]) == NAN_BITS).all(), f"{ep.name}: a row outside the {m} rows was written"
            assert not torch.isnan(win).any(), f"{ep.name}: a row inside the {m} rows was not written"
        else:
            assert (buf[:GUARD] == 0xAB).all() and (buf[GUARD + m:] == 0xAB).all(), f"{ep.name}: a row outside the {m} rows was written"
            assert (win <= 1).all(), f"{ep.name}: a row inside the {m} rows was not written"
        res.append(win.clone())
    return res


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("n", BATCH_SIZES)
@pytest.mark.parametrize("which", H.KIN_ALL)
def test_batch_edges_of_every_entry_point(which, n):
    """n rows inside guarded, sentinel-filled buffers: nothing outside the window is written, everything inside is; the first n rows of the
    1000-row call, a row computed alone and the same row as the last of a 257-row call are bit-identical."""
    for name, ep in _entry_points(which).items():
        if "full" not in ep.__dict__:
            ep.full = _run(ep, torch.arange(1000))
        got = _run(ep, torch.arange(n))
        assert _same(got, [t[:n] for t in ep.full]), f"{name}: the result of a row depends on the batch size ({n} against 1000)"
        for i in sorted({0, n // 2, n - 1}):
            alone = _run(ep, [i])
            assert _same(alone, [t[i:i + 1] for t in got]), f"{name}: row {i} computed alone differs"
            last = _run(ep, [(i + 1 + k) % 1000 for k in range(256)] + [i])
            assert _same([t[256:] for t in last], [t[i:i + 1] for t in got]), f"{name}: row {i} as the last row of a 257-row call differs"


@pytest.mark.parametrize("which", ["syn5p", "fetch"])
def test_every_entry_point_on_a_non_default_stream(which):
    st = torch.cuda.Stream(device=DEV)
    for name, ep in _entry_points(which).items():
        ref = _run(ep, torch.arange(257))
        got = _run(ep, torch.arange(257), stream=st)
        assert _same(got, ref), name


@pytest.mark.parametrize("which", H.KIN_ALL)
def test_output_may_alias_the_input_where_the_header_says_so(which):
    """ikf_lm_step (both precisions) and ikf_clamp_to_joint_limits with d_q_out == d_q, 257 rows: bit-identical to the call with a buffer of its own."""
    eps = _entry_points(which)
    for name, k_in in (("ikf_lm_step[f64]", 1), ("ikf_lm_step[f32]", 1), ("ikf_clamp_to_joint_limits", 0)):
        ref = _run(eps[name], torch.arange(257))
        got = _run(eps[name], torch.arange(257), alias=(0, k_in))
        assert _same(got, ref), name
        assert not torch.equal(ref[0], eps[name].inputs[k_in][:257]), name   # (the call does change its input, so the comparison says something)


# ---- 4. the LM step on hard inputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [0.15, 1.0])
@pytest.mark.parametrize("which", H.KIN_ALL)
def test_lm_step_on_hard_inputs(which, noise):
    """Seeds 0.15 and 1 rad off the truth plus the hand-made rows (helpers.lm_inputs); criteria in helpers.check_lm.
    Measured on the MI355X, kernel quantile / f32 oracle quantile on the same rows (median / p99 / maximum), worst chain of each kind:
      fp64 mode  7- and 8-joint chains and the built-in robots <= 0.01 / 0.01 / 0.01; 4 joints 0.37 / 0.15 / 0.07; 5 joints 0.38 / 0.06 / 0.07;
                 6 joints 0.13 / 0.01 / 0.02 - no margin needed.  Absolute: <= 9.9e-7 on the built-in robots at 0.15 rad (the project's 5e-6),
                 up to 1.4e-4 at 1 rad (syn6p), where the f32 oracle is 7.5e-3 off.
      f32 mode   median 0.86 .. 1.02, p99 0.85 .. 1.02 on every chain (margin 1.5); maximum 0.41 .. 2.50 (syn6r at 0.15 rad 2.50, syn4r 1.73, syn7p
                 at 1 rad 1.55, fetch_arm at 1 rad 1.48; the host build of the same source: 2.43, 1.08, 1.17, 1.51) against the 3.8 x by which
                 the f32 oracle's own maximum differs between the even and the odd rows of these samples (margin helpers.LM_MAX_MARGIN = 4).
    At most 0.65 % of the rows are left out near a branch point; 2.5 % to 96 % of the rows end with a joint on a limit."""
    H.check_lm(_Gpu(which).lm, which, noise)


# ---- 5. pose error where the clamp and the wrap decide --------------------------------------------------------------------------------------
def _pose_distance(a, b, eps):
    n = a.shape[0]
    a, b = a.to(DEV).contiguous(), b.to(DEV).contiguous()
    pe, re = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    code = _lib.load().ikf_pose_distance(a.data_ptr(), b.data_ptr(), n, eps, pe.data_ptr(), re.data_ptr(), C.c_void_p(0))
    assert code == _lib.IKF_OK, code
    torch.cuda.synchronize()
    return pe.cpu().numpy(), re.cpu().numpy()


@pytest.mark.parametrize("which", H.KIN_ALL)
def test_pose_error_where_the_clamp_and_the_wrap_decide(which):
    """ikf_pose_error with identical, antipodal, half- and double-length target quaternions and seeds 1e-4 .. 0.3 rad off: position error at 2e-6
    everywhere, rotation error by helpers.check_rot_error / check_rot_below_floor.
    Measured on the MI355X: above the floor <= 6.6e-6 (the project's 2e-5); below it the kernel is up to 9.3e-4 from fp64, as the f32 oracle is -
    kernel / oracle quantile of that distance 0.79 .. 1.21 at the median, 0.72 .. 1.28 at p99, 0.84 .. 1.27 at the maximum (margin 1.5;
    ikf_pose_distance on the oracle's own FK: 0.96 .. 0.98, 0.94 .. 0.97, 0.90 .. 1.12).  Identical and antipodal targets: 9.766e-4 .. 1.953e-3."""
    b = _Gpu(which)
    orob = H.kin_robots(which)[1]
    parts = []
    for case, (q, tgt) in H.pose_error_cases(orob, 20000).items():
        pe, re = b.pose_error(q.numpy(), tgt.numpy())
        ref_pe, _ = ko.calculate_pose_error(orob, q.double(), tgt.double())
        assert np.abs(pe - ref_pe.numpy()).max() <= 2e-6
        parts.append(H.check_rot_error(case, re, *H.rot_reference(orob, q, tgt)))
    H.check_rot_below_floor(which, parts)


EXPLICIT_EPS = 2.0 ** -10   # exact in f32 and fp64, so kernel and oracle clamp at the same value
DOT_ROUNDING = 3.5 * 2.0 ** -24   # four products and three sums of magnitude <= 1, each rounded to 2^-25 at most (fused or not)
WRAP_ROUNDING = 2e-6              # acosf to 2 ulp at pi, doubled (9.5e-7); d + pi rounded at 3 pi (4.8e-7); pi in f32 twice (1.7e-7): 1.6e-6, rounded up


def _geodesic_of_dot(dot):
    """The kernel's formula in fp64, with its f32 clamp values."""
    d = 2.0 * np.arccos(np.clip(dot, float(np.float32(-1.0 + 1e-7)), float(np.float32(1.0 - 1e-7))))
    return np.abs(np.mod(d + np.pi, 2.0 * np.pi) - np.pi)


@pytest.mark.parametrize("which", H.KIN_ALL)
def test_pose_distance_on_the_same_cases(which):
    """The same cases through the model-free ikf_pose_distance (targets against the f32 oracle's FK of the seeds, so kernel and oracle are given the
    same numbers).  Default epsilon: the criteria of ikf_pose_error, except where the clamp decides (identical, antipodal, doubled): there the exact
    dot product of the inputs is known, so every ROW is held to the window that the rounding of an f32 dot product allows around it.  (The maximum
    of the f32 oracle is no bound here: the kernel's fused dot product and torch's unfused one land on different multiples of 2^-24 - on syn6r
    the exact minimum is 1 - 8.5 x 2^-24, torch gives 8, the kernel 10, i.e. 2.18e-3 rad against 1.95e-3.)  Explicit epsilon 2^-10: every angle
    below 2 acos(1 - 2^-10) = 0.088 is clamped, so one ulp of the dot product is worth at most 2.4e-7 / 0.088 = 2.7e-6 and the project's 2e-5
    against fp64 holds on every row."""
    orob = H.kin_robots(which)[1]
    parts = []
    for case, (q, tgt) in H.pose_error_cases(orob, 20000).items():
        real = ko.forward_kinematics(orob, q)
        pe, re = _pose_distance(tgt, real, -1.0)
        assert np.abs(pe - torch.norm(tgt[:, :3].double() - real[:, :3].double(), dim=1).numpy()).max() <= 2e-6
        if case in ("identical", "antipodal", "double"):
            dot = (tgt[:, 3:].double() * real[:, 3:].double()).sum(1).numpy()
            w = DOT_ROUNDING * np.maximum(1.0, np.abs(dot))
            g1, g2 = _geodesic_of_dot(dot - w), _geodesic_of_dot(dot + w)
            assert (re >= np.minimum(g1, g2) - WRAP_ROUNDING).all() and (re <= np.maximum(g1, g2) + WRAP_ROUNDING).all(), case
            assert re.min() >= H.ACOS_CLAMP_ANGLE - 1e-6 and re.max() < 0.01
        else:
            r64 = ko.geodesic_distance_between_quaternions(tgt[:, 3:].double(), real[:, 3:].double()).numpy()
            r32 = ko.geodesic_distance_between_quaternions(tgt[:, 3:], real[:, 3:]).numpy().astype(np.float64)
            parts.append(H.check_rot_error(case, re, r64, r32))
        _, re_eps = _pose_distance(tgt, real, EXPLICIT_EPS)
        r64e = ko.geodesic_distance_between_quaternions(tgt[:, 3:].double(), real[:, 3:].double(), EXPLICIT_EPS).numpy()
        d = float(np.abs(re_eps - r64e).max())
        assert d <= 2e-5, (case, d)
    H.check_rot_below_floor(which, parts)


# ---- 6. capsules ----------------------------------------------------------------------------------------------------------------------------
def _panda_capsule_models():
    """{name: capsules} on Panda, each pair alone (the minimum over the pairs of a model would hide all but the closest) and all of them in one
    model padded to IKF_MAX_CAPSULES.  Frames: a capsule rides on the child link of the named joint."""
    joints = {j.name: j for j in rt.robot("panda").joints}
    j4 = joints["panda_joint4"]
    o = np.array(j4.origin_xyz)
    u = rt.rpy_matrix(j4.origin_rpy) @ np.array([0.0, 0.0, 1.0])            # the axis of joint 4 in the frame of link 3
    perp = np.cross(u, [1.0, 0.0, 0.0])
    perp /= np.linalg.norm(perp)
    perp2 = np.cross(u, perp)

    def beside_axis(angle):    # a segment 0.12 m beside the axis of joint 4, at `angle` to it (the angle does not depend on q)
        d = math.cos(angle) * u + math.sin(angle) * perp2
        return ("panda_joint3", tuple(o + 0.12 * perp - 0.10 * d), tuple(o + 0.12 * perp + 0.15 * d), 0.03)

    on_axis = ("panda_joint4", (0.0, 0.0, -0.05), (0.0, 0.0, 0.2), 0.04)     # on the axis of joint 4: parallel to beside_axis(0) for every q
    sphere2 = ("panda_joint2", (0.02, 0.03, -0.05), (0.02, 0.03, -0.05), 0.05)
    sphere5 = ("panda_joint5", (0.01, -0.02, 0.04), (0.01, -0.02, 0.04), 0.04)
    caps2 = ("panda_joint2", (0.0, 0.0, -0.1), (0.05, 0.1, 0.1), 0.04)
    caps5 = ("panda_joint5", (0.0, 0.0, -0.1), (0.05, 0.1, 0.1), 0.04)
    models = {
        "parallel": [beside_axis(0.0), on_axis],
        "angle1e-4": [beside_axis(1e-4), on_axis],
        "angle1e-3": [beside_axis(1e-3), on_axis],
        # a chord 0.1 m from the axis of joint 1 against a base segment through that axis' plane: they cross while cos(q1) >= 0.2
        "crossing": [(None, (0.05, 0.0, 0.333), (0.5, 0.0, 0.333), 0.02), ("panda_joint1", (0.1, -0.6, 0.0), (0.1, 0.6, 0.0), 0.03)],
        "sphere_capsule": [sphere2, caps5],     # first segment degenerate: the a <= EPS branch
        "capsule_sphere": [caps2, sphere5],     # second segment degenerate: the e <= EPS branch
        "sphere_sphere": [sphere2, sphere5],
    }
    rng = np.random.default_rng(17)
    names = [None] + [f"panda_joint{i}" for i in range(1, 8)]
    for k in range(3):                          # end-point and interior cases of the general branch
        a, b = rng.choice(8, 2, replace=False)
        models[f"random{k}"] = [(names[f], tuple(rng.uniform(-0.15, 0.15, 3)), tuple(rng.uniform(-0.25, 0.25, 3)), float(rng.uniform(0.02, 0.06))) for f in (a, b)]
    padded = [c for m in ("parallel", "angle1e-4", "angle1e-3", "crossing", "sphere_capsule", "capsule_sphere") for c in models[m]]
    k = 0
    while len(padded) < _lib.IKF_MAX_CAPSULES:
        padded.append((names[k % 8], tuple(rng.uniform(-0.1, 0.1, 3)), tuple(rng.uniform(-0.2, 0.2, 3)), float(rng.uniform(0.02, 0.05))))
        k += 1
    models["padded24"] = padded
    return models


@pytest.mark.parametrize("model", ["parallel", "angle1e-4", "angle1e-3", "crossing", "sphere_capsule", "capsule_sphere", "sphere_sphere",
                                   "random0", "random1", "random2", "padded24"])
def test_capsule_geometry_against_the_oracle(model):
    """Parallel and nearly parallel segments, segments that cross, both one-sided degenerate branches, sphere against sphere and a model with all
    24 capsules, against ko.capsule_clearance at the project's 2e-5; flags equal wherever |clearance| > 1e-4."""
    from ikflow_amd.robots import Panda

    robot, orob = Panda(), rt.robot("panda")
    capsules = _panda_capsule_models()[model]
    robot.set_collision_capsules(capsules)
    n = 200 if model == "padded24" else 3000
    q = torch.tensor(orob.sample_joint_angles(n, 0.0, np.random.default_rng(13)))
    ref = ko.capsule_clearance(orob, capsules, [], q)
    dist = robot.self_collision_distances(q.to(DEV)).cpu().double()
    d = (dist - ref).abs().max().item()
    print(f"capsules {model}: |d clearance| {d:.2e}, clearance in [{ref.min():.4f}, {ref.max():.4f}]")
    assert d <= 2e-5, d
    col = robot.config_self_collides(q.to(DEV)).cpu()
    clear = ref.abs() > 1e-4
    assert torch.equal(col[clear], (ref < 0)[clear])
    if model == "parallel":
        assert (ref - (0.12 - 0.07)).abs().max().item() <= 1e-9           # parallel for every q: the distance between the lines
    if model == "crossing":
        crossing = torch.cos(q[:, 0].double()) >= 0.21
        assert 0 < int(crossing.sum()) < n
        assert (dist[crossing] + 0.05).abs().max().item() <= 2e-5         # segments that cross: -(r_a + r_b)
        assert (ref[torch.cos(q[:, 0].double()) <= 0.19] > -0.05 + 1e-4).all()
    if model == "padded24":
        folded, pairs = robot._collision_model
        assert len(folded) == 24 and len(pairs) == 276 - sum(c * (c - 1) // 2 for c in np.bincount([f[0] for f in folded]))
        eng = robot._engine(q.to(DEV))
        eng.set_collision_model(folded, [(a, b) for a in range(24) for b in range(a + 1, 24)])   # every pair, same-frame ones included: accepted
        all_pairs = eng.self_collision(q.to(DEV))[0].cpu().double()
        assert torch.isfinite(all_pairs).all() and (all_pairs <= dist).all()
        eng.set_collision_model(folded, pairs)


def test_collision_model_errors():
    eng = _eng("panda")
    lib, h = eng.lib, eng._h
    caps = (_lib.ikf_capsule * 25)()
    for c in caps:
        c.frame, c.radius = 0, 0.05
    pairs = (C.c_int32 * 2)(0, 1)
    ptr = lambda a: C.cast(a, C.c_void_p)
    assert lib.ikf_set_collision_model(h, ptr(caps), 24, ptr(pairs), 1) == _lib.IKF_OK
    assert lib.ikf_set_collision_model(h, ptr(caps), 25, ptr(pairs), 1) == _lib.IKF_ERR_BAD_ARGUMENT
    caps[1].radius = -0.01
    assert lib.ikf_set_collision_model(h, ptr(caps), 2, ptr(pairs), 1) == _lib.IKF_ERR_BAD_ARGUMENT
    caps[1].radius = 0.05
    for bad in ((0, 2), (-1, 1), (1, 1)):
        assert lib.ikf_set_collision_model(h, ptr(caps), 2, ptr((C.c_int32 * 2)(*bad)), 1) == _lib.IKF_ERR_BAD_ARGUMENT, bad
    caps[1].frame = 8
    assert lib.ikf_set_collision_model(h, ptr(caps), 2, ptr(pairs), 1) == _lib.IKF_ERR_BAD_ARGUMENT
    eng._collision_source = None   # (the handle now holds this test's capsules: the next Robot sets its own)


# ---- 7. status codes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndof", [3, 9])
def test_create_refuses_a_chain_size_without_kernels(ndof):
    from ikflow_amd.engine import _make_desc
    from ikflow_amd.model import FlowLayout

    robot = H.kin_robots("panda")[0]
    desc = _make_desc(FlowLayout(nb_nodes=1, dim=16, dim_cond=8, width=256, n_hidden=1, clamp=2.5, ndof=7), robot)
    desc.ndof = ndof
    out = C.c_void_p()
    assert _lib.load().ikf_create(C.byref(desc), 0, C.byref(out)) == _lib.IKF_ERR_BAD_SHAPE
    assert not out.value


@pytest.mark.parametrize("which", ["syn4p", "fetch"])
def test_status_codes_of_every_kinematics_entry_point(which):
    """IKF_ERR_NULL_POINTER for each null argument (the model included), IKF_ERR_BAD_ARGUMENT for n < 0, IKF_OK for n = 0 with null buffers."""
    eps = _entry_points(which)
    eng = _eng(which)
    nd = H.kin_robots(which)[1].ndof
    null = C.c_void_p(0)
    for name, ep in eps.items():
        if ep.before is not None:
            ep.before()
        try:
            ins = [t[:4].contiguous() for t in ep.inputs]
            outs = [torch.zeros((4, cols), dtype=dt, device=DEV) for cols, dt in ep.outputs]
            ip, op = [t.data_ptr() for t in ins], [t.data_ptr() for t in outs]
            assert ep.call(ip, 4, op, null) == _lib.IKF_OK, name
            assert ep.call(ip, -1, op, null) == _lib.IKF_ERR_BAD_ARGUMENT, name
            assert ep.call([0] * len(ip), 0, [0] * len(op), null) == _lib.IKF_OK, name
            for k in range(len(ip)):
                assert ep.call([0 if j == k else p for j, p in enumerate(ip)], 4, op, null) == _lib.IKF_ERR_NULL_POINTER, (name, "input", k)
            if name == "ikf_self_collision":   # each output is nullable on its own, not both
                assert ep.call(ip, 4, [0, op[1]], null) == _lib.IKF_OK and ep.call(ip, 4, [op[0], 0], null) == _lib.IKF_OK
                assert ep.call(ip, 4, [0, 0], null) == _lib.IKF_ERR_NULL_POINTER
            else:
                for k in range(len(op)):
                    assert ep.call(ip, 4, [0 if j == k else p for j, p in enumerate(op)], null) == _lib.IKF_ERR_NULL_POINTER, (name, "output", k)
        finally:
            eng.set_lm_precision("f64")
    torch.cuda.synchronize()
    lib, q, out = eng.lib, eps["ikf_forward_kinematics"].inputs[0].data_ptr(), torch.zeros(4, 6 * nd, device=DEV).data_ptr()
    u8 = torch.zeros(4, dtype=torch.uint8, device=DEV).data_ptr()
    assert lib.ikf_forward_kinematics(None, q, 4, out, null) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_pose_error(None, q, out, 4, out, out, null) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_lm_step(None, out, q, 4, out, null) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_jacobian(None, q, 4, out, null) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_clamp_to_joint_limits(None, q, 4, out, null) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_joint_limits_exceeded(None, q, 4, u8, null) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_self_collision(None, q, 4, out, u8, null) == _lib.IKF_ERR_NULL_POINTER
    lims = (C.c_float * nd)()
    assert lib.ikf_limits_exceeded(q, 4, nd, None, lims, u8, null) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_limits_exceeded(q, 4, nd, lims, None, u8, null) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_limits_exceeded(q, 4, 0, lims, lims, u8, null) == _lib.IKF_ERR_BAD_ARGUMENT
    assert lib.ikf_limits_exceeded(q, 4, 33, lims, lims, u8, null) == _lib.IKF_ERR_BAD_ARGUMENT
