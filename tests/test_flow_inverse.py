"""The inverse pass WITH its log-determinant: ikf_flow_inverse -> Engine.flow_inverse -> IKFlowSolver.nn_inverse / sample_and_log_prob.

x (all D columns, unclamped) against the oracle's fp64 inverse (oracle.flow_inverse_f64) on every row; log|det dx/dz| against minus the
fp64 forward log-det evaluated at that x (tests/flow_logdet.py) AND against slogdet of a central-difference Jacobian of the inverse map
itself (so the formula is not trusted twice); consistency with generate_approx and flow_forward on the device; a row's result does not
depend on its place in the batch, on the batch size or on which outputs are asked for.  Both device paths everywhere: the row-owner launch
(k_flow_rowowner_ld: width padded to 1024, 3 hidden layers) and the per-layer kernels (flow_inverse.hip: every other shape).
Tolerances: x 1e-5 relative to max(1, |x|) (the inverse-parity class), log-det 1e-4 absolute, flat: the weights of this file have gains up
to 2.0 on inputs where an f32 evaluation of the references stays inside them, so the f32-noise clause of test_flow_forward._check is not
needed here.  Gain-2.5 weights (saturated couplings), every D, depth, padded width and forced contraction variant, the launch split at 2^24
rows and random shapes are in tests/test_flow_inverse_shapes.py; the references and the guarded call both files use are in
tests/flow_inverse_helpers.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from flow_inverse_helpers import DEV, FLOW_TOL, LD_TOL, _check, _cond, _edge_rows, _guarded_inverse, _refs, _rel
from flow_logdet import fd_logdet
from helpers import (O, _dense_fixed_transform, custom_model, fetch_arm_model, latents, panda_model, reachable_poses, released_model,
                     tiny_model)
from ikflow_amd import _lib
from ikflow_amd.ikflow_solver import IKFlowSolver
from oracle import flow_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_TOL = 3e-5       # forward(inverse(z)) = z on the device: the round-trip bound of tests/test_flow_forward.py
CHUNK = 16384
LOG_2PI = math.log(2.0 * math.pi)


def _solver(model):
    robot, hp, lay, sd = model
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    return s


def _inputs(model, n, seed):
    """Reachable target poses and N(0, 1) latent rows."""
    robot, hp, lay, sd = model
    _, poses = reachable_poses(robot, n, seed)
    return latents(n, lay.dim, seed + 1), poses


def _fd_agrees(a, fd, tol=1e-5):
    """A central difference whose +-h step crosses a LeakyReLU kink is off in that row: 99 % of the rows to tol, every row to 1e-3.
    tol 1e-5 for the fp64 formula, LD_TOL for the f32 kernel."""
    d = np.abs(a - fd)
    return float(np.mean(d <= tol)) >= 0.99 and float(d.max()) <= 1e-3


# ---- 1. CPU: the symbol, its ctypes signature, the solver's methods ------------------------------------------------------------------
_CTYPE = {"ikf_model*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p, "int64_t": C.c_int64,
          "int": C.c_int, "float": C.c_float}


def test_flow_inverse_is_exported_and_its_ctypes_signature_matches_the_header():
    header = open(os.path.join(ROOT, "include", "ikflow_amd.h")).read()
    m = re.search(r"ikf_status\s+ikf_flow_inverse\s*\(([^;]*)\)\s*;", header)
    assert m, "ikf_flow_inverse is not declared in include/ikflow_amd.h"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    types = [re.match(r"(.*?)\s*\b\w+$", p).group(1).replace(" *", "*").strip() for p in params]
    assert len(types) == 11
    restype, argtypes = _lib.SIGNATURES["ikf_flow_inverse"]
    assert restype is C.c_int
    assert argtypes == [_CTYPE[t] for t in types], (types, argtypes)
    for flavour in ("", "probes"):
        assert hasattr(_lib.load(flavour), "ikf_flow_inverse")
    assert _lib.load().ikf_abi_version() == _lib.IKF_ABI_VERSION == 3   # additive change


def test_solver_has_the_methods_and_without_a_gpu_they_raise_the_no_cpu_path_error():
    from ikflow_amd.engine import Engine, EngineError

    assert callable(getattr(IKFlowSolver, "sample_and_log_prob")) and callable(getattr(IKFlowSolver, "nn_inverse"))
    assert callable(getattr(Engine, "flow_inverse"))
    robot, hp, lay, sd = tiny_model()
    s = IKFlowSolver(hp, robot)
    with pytest.raises(AssertionError, match="Model weights have not been loaded"):
        s.sample_and_log_prob(torch.zeros(7), n=4)
    with pytest.raises(AssertionError, match="Model weights have not been loaded"):
        s.nn_inverse(torch.zeros(4, lay.dim), torch.zeros(4, 8))
    s.load_state_dict_tensors(sd)
    if not torch.cuda.is_available():
        with pytest.raises(EngineError, match="no CPU path"):
            s.sample_and_log_prob(torch.zeros(7), n=4)
        with pytest.raises(EngineError, match="no CPU path"):
            s.nn_inverse(torch.zeros(4, lay.dim), torch.zeros(4, 8))


# ---- 2. x and log-det against the fp64 references, every row ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which,n", [("panda", 4096), ("fetch_arm", 8192), ("tiny", 4096), ("custom512", 1000), ("custom1024x2", 777),
                                     ("panda_lite_tpm", 1000), ("fetch_full_temp_nsc_tpm", 1000), ("fetch__large__ns183_9.75m", 1000)])
def test_x_and_log_det_match_the_fp64_references_on_every_row(which, n):
    """Row-owner: Panda, FetchArm and the three other released architectures; per-layer: TINY, width 512 x 3 hidden, width 1024 x 2 hidden."""
    make = {"panda": panda_model, "fetch_arm": fetch_arm_model, "tiny": tiny_model,
            "custom512": lambda: custom_model(nb_nodes=3, dim=9, n_hidden=3, width=512, seed=5),
            "custom1024x2": lambda: custom_model(nb_nodes=2, dim=8, n_hidden=2, width=1024, seed=6)}
    model = make[which]() if which in make else released_model(which, seed=4)
    robot, hp, lay, sd = model
    eng = _solver(model).engine(DEV)
    z, poses = _inputs(model, n, 31)
    x, q, ld = eng.flow_inverse(z.to(DEV), poses.to(DEV))
    assert x.shape == (n, lay.dim) and q.shape == (n, lay.ndof) and ld.shape == (n,)
    _check(f"{which} B={n}", sd, lay, z, _cond(lay, poses.numpy()), x, ld)
    assert torch.equal(x[:, : lay.ndof], q)


# ---- 3. log-det against a finite-difference Jacobian of the inverse map ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny", "d16", "sigmoid", "fetch_arm", "n_hidden1"])
def test_log_det_against_a_finite_difference_jacobian_of_the_inverse_map(which):
    """Panda and FetchArm (row-owner); TINY, a D = 16 model (OUT = 16), a sigmoid graph and a one-hidden-layer model (per-layer).
    The references alone meet the cap on these inputs (checked on the CPU: 100 % / 100 % / 100 % / 99.7 % of 300 rows within 1e-5 for
    TINY / D = 16 / sigmoid / Panda); f32 evaluation noise of the log-det formula on them is <= 3.2e-6."""
    seed = 8 if which == "sigmoid" else 3
    model = {"panda": lambda: panda_model(seed=3, gain=2.0), "tiny": lambda: tiny_model(seed=3, gain=2.0),
             "d16": lambda: custom_model(nb_nodes=3, dim=16, n_hidden=2, width=256, seed=3, gain=2.0),
             "sigmoid": lambda: custom_model(nb_nodes=3, dim=7, n_hidden=2, width=256, softflow=False, sigmoid=True, seed=8),
             "fetch_arm": lambda: fetch_arm_model(seed=3, gain=2.0),
             "n_hidden1": lambda: custom_model(nb_nodes=3, dim=9, n_hidden=1, width=512, seed=3, gain=2.0)}[which]()
    robot, hp, lay, sd = model
    eng = _solver(model).engine(DEV)
    n = 200 if which == "fetch_arm" else 300   # (FetchArm: 21 fp64 passes of 16 blocks per row)
    z, poses = _inputs(model, n, seed)
    cond = _cond(lay, poses.numpy())
    _, _, ld = eng.flow_inverse(z.to(DEV), poses.to(DEV))
    ld = ld.cpu().numpy().astype(np.float64)
    z64 = z.numpy().astype(np.float64)
    fd = fd_logdet(lambda v: fo.flow_inverse_f64(sd, lay, v, cond), z64)
    _, analytic = _refs(sd, lay, z64, cond)
    err, err_fd = float(np.abs(ld - analytic).max()), np.abs(ld - fd)
    print(f"{which}: max |log_det - analytic| {err:.2e}; vs fd slogdet: median {np.median(err_fd):.2e}, max {err_fd.max():.2e}; "
          f"analytic vs fd max {np.abs(analytic - fd).max():.2e}; |log_det| up to {np.abs(fd).max():.1f}")
    assert _fd_agrees(analytic, fd) and _fd_agrees(ld, fd, LD_TOL)
    assert err <= LD_TOL, err


# ---- 4. consistency with the existing calls, on the device --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny"])
@pytest.mark.parametrize("n", [1, 17, 512, 4096])
def test_consistent_with_generate_approx_and_flow_forward(which, n):
    model = panda_model(seed=2) if which == "panda" else tiny_model(seed=2)
    robot, hp, lay, sd = model
    eng = _solver(model).engine(DEV)
    z, poses = _inputs(model, n, 51)
    Z, P = z.to(DEV), poses.to(DEV)
    x, q, ld = eng.flow_inverse(Z, P)
    assert torch.equal(x[:, : lay.ndof], q)
    for clamp in (False, True):
        qc = eng.flow_inverse(Z, P, clamp=clamp)[1]
        ref = eng.generate_approx(P, Z, clamp=clamp)
        err = _rel(qc, ref.cpu().numpy().astype(np.float64))
        print(f"{which} B={n} clamp={clamp}: q_out vs generate_approx max rel {err:.2e}")
        assert err <= FLOW_TOL, err
        if clamp:
            lo = torch.tensor([l[0] for l in O(robot).actuated_joints_limits], device=DEV)
            hi = torch.tensor([l[1] for l in O(robot).actuated_joints_limits], device=DEV)
            assert torch.equal(qc, torch.minimum(torch.maximum(q, lo), hi))
    zb, ldf = eng.flow_forward(x, P)
    rt, dl = float((zb - Z).abs().max()), float((ldf + ld).abs().max())
    print(f"{which} B={n}: max |forward(x_out) - z| {rt:.2e}, max |log_det_fwd + log_det_inv| {dl:.2e}")
    assert rt <= RT_TOL and dl <= LD_TOL, (rt, dl)


# ---- 5. the solver's methods ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny"])
def test_sample_and_log_prob(which):
    model = panda_model(seed=7) if which == "panda" else tiny_model(seed=7)
    robot, hp, lay, sd = model
    s = _solver(model)
    n, D = 600, lay.dim
    _, poses = reachable_poses(robot, n, 71)
    P = poses.to(DEV)
    # the same torch seed: the same latent, so the same solutions as generate_ik_solutions
    for clamp in (False, True):
        torch.manual_seed(1234)
        ref = s.generate_ik_solutions(P, clamp_to_joint_limits=clamp)
        torch.manual_seed(1234)
        sol, lp = s.sample_and_log_prob(P, clamp_to_joint_limits=clamp)
        assert sol.shape == (n, lay.ndof) and lp.shape == (n,) and lp.dtype == torch.float32
        err = _rel(sol, ref.cpu().numpy().astype(np.float64))
        print(f"{which} clamp={clamp}: solutions vs generate_ik_solutions (same seed) max rel {err:.2e}")
        assert err <= FLOW_TOL, err
    # log_prob against fp64, with an explicit latent; pad rows through the existing two-pass log_prob
    z = latents(n, D, 72)
    Z = z.to(DEV)
    cond = _cond(lay, poses.numpy())
    x_ref, ld_ref = _refs(sd, lay, z, cond)
    z64 = z.numpy().astype(np.float64)
    lp_ref = -0.5 * (z64 * z64).sum(1) - 0.5 * D * LOG_2PI - ld_ref
    sol, lp, pad = s.sample_and_log_prob(P, latent=Z, return_pad=True)
    assert pad.shape == (n, D - lay.ndof)
    assert _rel(torch.cat([sol, pad], 1), x_ref) <= FLOW_TOL
    one = float(np.abs(lp.cpu().numpy() - lp_ref).max())
    two_pass = s.log_prob(sol, P, pad=pad)
    two = float(np.abs(two_pass.cpu().numpy() - lp_ref).max())
    both = float((two_pass - lp).abs().max())
    print(f"{which}: |log_prob - fp64| one pass {one:.2e}, two passes (generate + log_prob) {two:.2e}; one pass vs two passes {both:.2e}")
    assert one <= LD_TOL, one
    assert both <= 5 * LD_TOL, both
    sol2, lp2 = s.sample_and_log_prob(P, latent=Z)
    assert torch.equal(sol2, sol) and torch.equal(lp2, lp)
    # one pose for every row == that pose repeated
    a = s.sample_and_log_prob(P[3], n=n, latent=Z)
    b = s.sample_and_log_prob(P[3:4].expand(n, 7).contiguous(), latent=Z)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # other proposals: the value is still the MODEL's density of the sample
    for dist, scale in (("gaussian", 0.25), ("uniform", 0.25), ("uniform", 1.0)):
        torch.manual_seed(99)
        sol, lp = s.sample_and_log_prob(P, latent_distribution=dist, latent_scale=scale)
        torch.manual_seed(99)
        zz = (scale * torch.randn((n, D), device=DEV)) if dist == "gaussian" else (2 * scale * torch.rand((n, D), device=DEV) - scale)
        assert float(zz.abs().max()) <= (6 * scale if dist == "gaussian" else scale)
        x_r, ld_r = _refs(sd, lay, zz, cond)
        z64 = zz.cpu().numpy().astype(np.float64)
        want = -0.5 * (z64 * z64).sum(1) - 0.5 * D * LOG_2PI - ld_r
        e_sol, e_lp = _rel(sol, x_r[:, : lay.ndof]), float(np.abs(lp.cpu().numpy() - want).max())
        print(f"{which} {dist} x {scale}: solutions {e_sol:.2e}, log_prob {e_lp:.2e}")
        assert e_sol <= FLOW_TOL and e_lp <= LD_TOL, (e_sol, e_lp)
    with pytest.raises(AssertionError):
        s.sample_and_log_prob(P[0])   # a single pose needs n


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny"])
def test_nn_inverse_is_the_engine_call_and_honours_the_softflow_column(which):
    model = panda_model(seed=9) if which == "panda" else tiny_model(seed=9)
    robot, hp, lay, sd = model
    s = _solver(model)
    eng = s.engine(DEV)
    n = 333
    z, poses = _inputs(model, n, 73)
    Z, P = z.to(DEV), poses.to(DEV)
    x, _, ld = eng.flow_inverse(Z, P)
    x7, ld7 = s.nn_inverse(Z, P)
    x8, ld8 = s.nn_inverse(Z, torch.cat([P, torch.zeros(n, 1, device=DEV)], 1))
    assert torch.equal(x7, x) and torch.equal(ld7, ld) and torch.equal(x8, x) and torch.equal(ld8, ld)
    xs, _, lds = eng.flow_inverse(Z, P, softflow_scale=0.37)
    x37, ld37 = s.nn_inverse(Z, torch.cat([P, torch.full((n, 1), 0.37, device=DEV)], 1))
    assert torch.equal(x37, xs) and torch.equal(ld37, lds) and not torch.equal(xs, x)
    _check(f"{which} nn_inverse softflow 0.37", sd, lay, z, _cond(lay, poses.numpy(), 0.37), x37, ld37)
    varying = torch.cat([P, torch.linspace(0, 1, n, device=DEV).reshape(n, 1)], 1)
    with pytest.raises(AssertionError, match="softflow column"):
        s.nn_inverse(Z, varying)


# ---- 6. batch edges, stray stores, position independence, each output alone ---------------------------------------------------------
@pytest.mark.gpu
def test_rowowner_batch_edges_positions_and_no_stray_store():
    """Panda (row-owner): n around the 16-row tile and the 256 / 4096-row marks.  Rows 0 .. 4096 of a 20000-row call against the fp64
    references on every row, above that an edge sample; every smaller n gives the same bits as those rows; a row copied to other places of
    the batch gives the same bits there; each output alone gives the same bits as all three together; nothing past row n - 1 is written."""
    model = panda_model(seed=11)
    robot, hp, lay, sd = model
    eng = _solver(model).engine(DEV)
    N = 20000
    z, poses = _inputs(model, N, 91)
    for r in (4101, 9999, N - 1):
        z[r], poses[r] = z[0], poses[0]
    cond = _cond(lay, poses.numpy())
    Z, P = z.to(DEV), poses.to(DEV)
    x_all, q_all, ld_all = _guarded_inverse(eng, Z, P)
    rows = np.union1d(np.arange(4097), _edge_rows(N, range(4096, N, 1024), 256, 5))
    _check(f"panda n={N}", sd, lay, z, cond, x_all, ld_all, rows)
    for r in (4101, 9999, N - 1):
        assert torch.equal(x_all[r], x_all[0]) and torch.equal(q_all[r], q_all[0]) and torch.equal(ld_all[r], ld_all[0]), f"row {r}"
    for n in (1, 15, 16, 17, 31, 33, 255, 256, 257, 4095, 4096, 4097):
        x, q, ld = _guarded_inverse(eng, Z[:n].contiguous(), P[:n].contiguous())
        assert torch.equal(x, x_all[:n]) and torch.equal(q, q_all[:n]) and torch.equal(ld, ld_all[:n]), f"n={n}"
    print(f"panda: n = 1 .. 4097 bit-identical to the leading rows of the {N}-row call, tail rows unchanged")
    for n in (17, 4097):
        Zn, Pn = Z[:n].contiguous(), P[:n].contiguous()
        for k in range(3):
            want = tuple(i == k for i in range(3))
            got = _guarded_inverse(eng, Zn, Pn, want=want)[k]
            assert torch.equal(got, (x_all, q_all, ld_all)[k][:n]), f"n={n} output {k} alone"
    qc = _guarded_inverse(eng, Z, P, clamp=True)[1]
    lo = torch.tensor([l[0] for l in O(robot).actuated_joints_limits], device=DEV)
    hi = torch.tensor([l[1] for l in O(robot).actuated_joints_limits], device=DEV)
    assert torch.equal(qc, torch.minimum(torch.maximum(q_all, lo), hi))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["tiny", "width300"])
def test_per_layer_batch_edges_positions_and_no_stray_store(which):
    """Per-layer path: n around the 128-row contraction tile and the 16384-row chunk, and 40000 rows = 2 x 16384 + 7232 (r0 > 0 in the chunk
    loop).  The 40000-row call against the fp64 references on every row; every smaller n gives the same bits as its leading rows."""
    model = tiny_model(seed=12) if which == "tiny" else custom_model(nb_nodes=2, dim=10, n_hidden=3, width=300, robot_name="fetch_arm", seed=12)
    robot, hp, lay, sd = model
    eng = _solver(model).engine(DEV)
    N = 40000
    z, poses = _inputs(model, N, 92)
    for r in (130, 16384, 33000, N - 1):
        z[r], poses[r] = z[0], poses[0]
    cond = _cond(lay, poses.numpy())
    Z, P = z.to(DEV), poses.to(DEV)
    x_all, q_all, ld_all = _guarded_inverse(eng, Z, P)
    _check(f"{which} n={N}", sd, lay, z, cond, x_all, ld_all)
    for r in (130, 16384, 33000, N - 1):
        assert torch.equal(x_all[r], x_all[0]) and torch.equal(q_all[r], q_all[0]) and torch.equal(ld_all[r], ld_all[0]), f"row {r}"
    for n in (1, 3, 127, 128, 129, 16383, 16384, 16385):
        x, q, ld = _guarded_inverse(eng, Z[:n].contiguous(), P[:n].contiguous())
        assert torch.equal(x, x_all[:n]) and torch.equal(q, q_all[:n]) and torch.equal(ld, ld_all[:n]), f"n={n}"
    for n in (129, 16385):
        Zn, Pn = Z[:n].contiguous(), P[:n].contiguous()
        for k in range(3):
            want = tuple(i == k for i in range(3))
            got = _guarded_inverse(eng, Zn, Pn, want=want)[k]
            assert torch.equal(got, (x_all, q_all, ld_all)[k][:n]), f"n={n} output {k} alone"


# ---- 7. status codes, conditional forms, graph variants, load-time branches ---------------------------------------------------------
@pytest.mark.gpu
def test_cabi_status_codes():
    from ikflow_amd.engine import Engine

    model = tiny_model()
    robot, hp, lay, sd = model
    eng = Engine(lay, robot, DEV)
    lib = eng.lib
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    z = torch.zeros(4, lay.dim, device=DEV)
    p = torch.zeros(4, 7, device=DEV)
    p[:, 3] = 1.0
    x = torch.zeros(4, lay.dim, device=DEV)
    q = torch.zeros(4, lay.ndof, device=DEV)
    ld = torch.zeros(4, device=DEV)

    def call(h, zz, n, pp, xx, qq, ll):
        return lib.ikf_flow_inverse(h, zz, n, pp, 0, 0.0, 0, xx, qq, ll, stream)
    assert call(eng._h, z.data_ptr(), 4, p.data_ptr(), x.data_ptr(), q.data_ptr(), ld.data_ptr()) == _lib.IKF_ERR_NOT_LOADED
    assert "Model weights have not been loaded" in _lib.last_error()
    eng.load_state_dict(sd)
    assert call(None, z.data_ptr(), 4, p.data_ptr(), x.data_ptr(), q.data_ptr(), ld.data_ptr()) == _lib.IKF_ERR_NULL_POINTER
    assert call(eng._h, None, 4, p.data_ptr(), x.data_ptr(), q.data_ptr(), ld.data_ptr()) == _lib.IKF_ERR_NULL_POINTER
    assert call(eng._h, z.data_ptr(), 4, None, x.data_ptr(), q.data_ptr(), ld.data_ptr()) == _lib.IKF_ERR_NULL_POINTER
    assert call(eng._h, z.data_ptr(), 4, p.data_ptr(), None, None, None) == _lib.IKF_ERR_NULL_POINTER
    assert call(eng._h, z.data_ptr(), -1, p.data_ptr(), x.data_ptr(), q.data_ptr(), ld.data_ptr()) == _lib.IKF_ERR_BAD_ARGUMENT
    assert call(eng._h, None, 0, None, None, None, None) == _lib.IKF_OK
    assert call(eng._h, z.data_ptr(), 4, p.data_ptr(), x.data_ptr(), None, None) == _lib.IKF_OK
    assert call(eng._h, z.data_ptr(), 4, p.data_ptr(), None, q.data_ptr(), None) == _lib.IKF_OK
    assert call(eng._h, z.data_ptr(), 4, p.data_ptr(), None, None, ld.data_ptr()) == _lib.IKF_OK
    torch.cuda.synchronize()
    x2, q2, ld2 = eng.flow_inverse(z, p)
    assert torch.equal(x, x2) and torch.equal(q, q2) and torch.equal(ld, ld2)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny"])
def test_softflow_scale_and_pose_broadcast(which):
    """The 8th conditional entry against the oracle run on [pose, 0.37]; pose_broadcast = 1 is bit-identical to the pose repeated."""
    model = panda_model(seed=14) if which == "panda" else tiny_model(seed=14)
    robot, hp, lay, sd = model
    eng = _solver(model).engine(DEV)
    n = 600
    z, poses = _inputs(model, n, 93)
    Z, P = z.to(DEV), poses.to(DEV)
    x, q, ld = eng.flow_inverse(Z, P, softflow_scale=0.37)
    _check(f"{which} softflow 0.37", sd, lay, z, _cond(lay, poses.numpy(), 0.37), x, ld)
    assert not torch.equal(x, eng.flow_inverse(Z, P)[0])
    one = P[5].contiguous()
    a = eng.flow_inverse(Z, one, softflow_scale=0.37)
    b = eng.flow_inverse(Z, one.expand(n, 7).contiguous(), softflow_scale=0.37)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    _check(f"{which} broadcast", sd, lay, z, _cond(lay, poses[5:6].expand(n, 7).numpy(), 0.37), a[0], a[2])


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(nb_nodes=2, dim=7, n_hidden=3, width=1024), dict(nb_nodes=3, dim=7, n_hidden=2, width=256)])
def test_sigmoid_graph_on_both_paths(kw):
    """Row-owner (width 1024 x 3 hidden) and per-layer (width 256 x 2 hidden) sigmoid_on_output graphs, N(0, 1) latents.  (Latents wide
    enough to saturate the sigmoid have no usable reference here: the fp64 forward route re-enters through the file's f32 M, which is the
    inverse of the f32 M_inv only to 1e-7 - more than 1 - v at such a point.)"""
    model = custom_model(softflow=False, sigmoid=True, seed=8, **kw)
    robot, hp, lay, sd = model
    eng = _solver(model).engine(DEV)
    n = 300
    z, poses = _inputs(model, n, 61)
    Z, P = z.to(DEV), poses.to(DEV)
    x, q, ld = eng.flow_inverse(Z, P)
    _check(f"sigmoid {kw}", sd, lay, z, _cond(lay, poses.numpy()), x, ld)
    ref = eng.generate_approx(P, Z, clamp=False)
    assert _rel(q, ref.cpu().numpy().astype(np.float64)) <= FLOW_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny"])
def test_f16x3_precision_leaves_the_call_in_f32(which):
    model = panda_model(seed=20) if which == "panda" else tiny_model(seed=20)
    eng = _solver(model).engine(DEV)
    z, poses = _inputs(model, 1500, 98)
    Z, P = z.to(DEV), poses.to(DEV)
    ref = [t.clone() for t in eng.flow_inverse(Z, P)]
    eng.set_precision("f16x3")
    assert eng.precision == "f16x3"
    got = eng.flow_inverse(Z, P)
    assert all(torch.equal(u, v) for u, v in zip(ref, got))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny"])
@pytest.mark.parametrize("with_M", [True, False])
def test_dense_fixed_linear_transform_with_bias(which, with_M):
    """A dense, non-symmetric M with b != 0, with M in the state_dict and without it: a sign or transpose slip in log|det M_inv| or in
    (x - b).mm(M_inv) shows here.  log|det M_inv| of these matrices is several units away from 0."""
    model = _dense_fixed_transform(panda_model(seed=22) if which == "panda" else tiny_model(seed=22), 23)
    robot, hp, lay, sd = model
    if not with_M:
        sd = {k: v for k, v in sd.items() if k != "module_list.0.M"}
        model = (robot, hp, lay, sd)
    logdet_minv = float(np.linalg.slogdet(np.asarray(sd["module_list.0.M_inv"], dtype=np.float64))[1])
    assert abs(logdet_minv) > 1.0
    eng = _solver(model).engine(DEV)
    n = 700
    z, poses = _inputs(model, n, 101)
    x, q, ld = eng.flow_inverse(z.to(DEV), poses.to(DEV))
    print(f"log|det M_inv| = {logdet_minv:.3f}")
    _check(f"{which} dense M, b != 0, M {'given' if with_M else 'absent'}", sd, lay, z, _cond(lay, poses.numpy()), x, ld)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny"])
def test_reload_refreshes_the_tables_and_the_constant(which):
    """load A, call, load B (other weights, permutations and a dense M: another log|det M_inv|) on the same handle, call: bit-identical to
    a fresh handle loaded with B and right against fp64; then back to A."""
    make = panda_model if which == "panda" else tiny_model
    A, B = make(seed=17), _dense_fixed_transform(make(seed=18, gain=1.5), 19)
    n = 4100 if which == "panda" else 20000
    z, poses = _inputs(A, n, 96)
    Z, P = z.to(DEV), poses.to(DEV)
    s = _solver(A)
    eng = s.engine(DEV)
    a = [t.clone() for t in eng.flow_inverse(Z, P)]
    s.load_state_dict_tensors(B[3])
    b = eng.flow_inverse(Z, P)
    fresh = _solver(B).engine(DEV).flow_inverse(Z, P)
    assert all(torch.equal(u, v) for u, v in zip(b, fresh))
    assert not torch.equal(b[0], a[0])
    rows = _edge_rows(n, (CHUNK,), 128, 7)
    _check(f"{which} reloaded B", B[3], B[2], z, _cond(B[2], poses.numpy()), b[0], b[2], rows)
    s.load_state_dict_tensors(A[3])
    a2 = eng.flow_inverse(Z, P)
    assert all(torch.equal(u, v) for u, v in zip(a, a2))


# ---- 8. graph capture; interleaving with the other flow calls on one handle ---------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which,n", [("panda", 4096), ("tiny", 20000)])
def test_call_can_be_captured_into_a_hip_graph(which, n):
    """After ikf_load_weights + ikf_reserve the call allocates nothing and never synchronises: it can be captured.  TINY at 20000 rows: the
    per-layer chunk loop (16384 + 3616 rows) inside one graph."""
    model = {"panda": panda_model, "tiny": tiny_model}[which]()
    eng = _solver(model).engine(DEV)
    eng.reserve(max(8192, n))
    z, poses = _inputs(model, n, 81)
    Z, P = z.to(DEV), poses.to(DEV)
    ref = [t.clone() for t in eng.flow_inverse(Z, P, clamp=True)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            eng.flow_inverse(Z, P, clamp=True)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = eng.flow_inverse(Z, P, clamp=True)
    for _ in range(2):
        with torch.inference_mode():
            for t in out:
                t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(u, v) for u, v in zip(out, ref))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny"])
@pytest.mark.parametrize("two_streams", [False, True])
def test_interleaved_with_generate_approx_and_flow_forward_on_one_handle(which, two_streams):
    """flow_inverse, generate_approx and flow_forward alternating on one handle (shared per-layer scratch), at batch sizes on both sides of
    the chunk, from one stream or alternating between two without host synchronisation: every result bit-identical to the call made alone."""
    model = panda_model(seed=21) if which == "panda" else tiny_model(seed=21)
    robot, hp, lay, sd = model
    eng = _solver(model).engine(DEV)
    N = 20000
    z, poses = _inputs(model, N, 99)
    Z, P = z.to(DEV), poses.to(DEV)
    X = eng.flow_inverse(Z, P)[0].clone()
    torch.cuda.synchronize()
    plan = [("ld", 3000), ("fwd", 20000), ("ld", 20000), ("inv", 17000), ("ld", 129), ("fwd", 129), ("ld", 1), ("inv", 512), ("ld", 4097),
            ("inv", 20000), ("ld", 17000), ("fwd", 1)]

    def call(d, n):
        if d == "fwd":
            return eng.flow_forward(X[:n], P[:n])
        if d == "inv":
            return (eng.generate_approx(P[:n], Z[:n], clamp=False),)
        return eng.flow_inverse(Z[:n], P[:n], clamp=True)
    want = []
    for d, n in plan:
        want.append([t.clone() for t in call(d, n)])
        torch.cuda.synchronize()
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)] if two_streams else [torch.cuda.current_stream(DEV)]
    got = []
    for i, (d, n) in enumerate(plan):
        with torch.cuda.stream(streams[i % len(streams)]):
            got.append(call(d, n))
    torch.cuda.synchronize()
    for (d, n), a, b in zip(plan, want, got):
        assert all(torch.equal(u, v) for u, v in zip(a, b)), f"{d} n={n}"
