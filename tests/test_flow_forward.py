"""The forward (training-direction) pass: ikf_flow_forward -> Engine.flow_forward -> IKFlowSolver.log_prob / nll / nn_forward.

z against the oracle's fp64 forward (oracle.flow_forward_f64) on every row; log|det J| against an fp64 sum written in tests/flow_logdet.py
AND against slogdet of a central-difference Jacobian (so the formula is not trusted twice); round trips through the public inverse call;
a row's result does not depend on its place in the batch.  Tolerances: z 1e-5 relative to max(1, |z|), the inverse-parity class."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from flow_logdet import fd_logdet, forward_with_logdet
from helpers import (O, _dense_fixed_transform, custom_model, fetch_arm_model, latents, panda_model, reachable_poses, released_model,
                     tiny_model)
from ikflow_amd import _lib
from ikflow_amd.ikflow_solver import IKFlowSolver
from oracle import flow_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
Z_TOL = 1e-5        # relative to max(1, |z|)
LD_TOL = 1e-4       # absolute, log|det J| of O(10)


def _solver(model):
    robot, hp, lay, sd = model
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    return s


def _rows(model, n, seed, pad_scale=1e-3):
    """In-limit joint rows padded to dim_tot (pad = pad_scale randn), their poses and the oracle conditional [pose, 0]."""
    robot, hp, lay, sd = model
    q, poses = reachable_poses(robot, n, seed)
    pad = pad_scale * torch.randn(n, lay.dim - lay.ndof, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64)
    x = torch.cat([q.to(torch.float64), pad], 1).to(torch.float32)
    cond = poses.numpy().astype(np.float64)
    if lay.dim_cond == 8:
        cond = np.concatenate([cond, np.zeros((n, 1))], 1)
    return x, poses, cond


def _fd_agrees(a, fd, tol=1e-5):
    """A central difference whose +-h step crosses a LeakyReLU kink is off in that row: 99 % of the rows to tol, every row to 1e-3.
    tol 1e-5 for the fp64 sum (the formula check), LD_TOL for the f32 kernel."""
    d = np.abs(a - fd)
    return float(np.mean(d <= tol)) >= 0.99 and float(d.max()) <= 1e-3


def _zerr(z, ref):
    return float((np.abs(z - ref) / np.maximum(1.0, np.abs(ref))).max())


# ---- 6. CPU: the symbol and its ctypes signature --------------------------------------------------------------------------------------
_CTYPE = {"ikf_model*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p, "int64_t": C.c_int64,
          "int": C.c_int, "float": C.c_float}


def test_flow_forward_is_exported_and_its_ctypes_signature_matches_the_header():
    header = open(os.path.join(ROOT, "include", "ikflow_amd.h")).read()
    m = re.search(r"ikf_status\s+ikf_flow_forward\s*\(([^;]*)\)\s*;", header)
    assert m, "ikf_flow_forward is not declared in include/ikflow_amd.h"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    types = [re.match(r"(.*?)\s*\b\w+$", p).group(1).replace(" *", "*").strip() for p in params]
    restype, argtypes = _lib.SIGNATURES["ikf_flow_forward"]
    assert restype is C.c_int
    assert argtypes == [_CTYPE[t] for t in types], (types, argtypes)
    for flavour in ("", "probes"):
        assert hasattr(_lib.load(flavour), "ikf_flow_forward")


# ---- 1. z parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which,n", [("panda", 4096), ("fetch_arm", 8192), ("tiny", 4096), ("custom512", 1000), ("custom1024x2", 777)])
def test_z_matches_the_oracle_forward_on_every_row(which, n):
    model = {"panda": panda_model, "fetch_arm": fetch_arm_model, "tiny": tiny_model,
             "custom512": lambda: custom_model(nb_nodes=3, dim=9, n_hidden=3, width=512, seed=5),
             "custom1024x2": lambda: custom_model(nb_nodes=2, dim=8, n_hidden=2, width=1024, seed=6)}[which]()
    robot, hp, lay, sd = model
    s = _solver(model)
    x, poses, cond = _rows(model, n, 31)
    z, ld = s.engine(DEV).flow_forward(x.to(DEV), poses.to(DEV))
    z, ld = z.cpu().numpy(), ld.cpu().numpy()
    ref = fo.flow_forward_f64(sd, lay, x.numpy(), cond)
    err = _zerr(z, ref)
    print(f"{which} B={n}: max |dz| rel {err:.2e}")
    assert err <= Z_TOL, err
    _, ld_ref = forward_with_logdet(sd, lay, x.numpy(), cond)
    lerr = float(np.abs(ld - ld_ref).max())
    print(f"{which} B={n}: max |dlog_det| {lerr:.2e}")
    assert lerr <= LD_TOL, lerr
    assert np.isfinite(z).all() and np.isfinite(ld).all()


# ---- 2. log-det, independent of the recalled formula --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny", "fetch_arm", "d16", "n_hidden1"])
def test_log_det_against_a_finite_difference_jacobian(which):
    """Panda and FetchArm (D = 7, 10: row-owner), TINY, a D = 16 model (OUT = 16) and a one-hidden-layer model (per-layer)."""
    model = {"panda": lambda: panda_model(seed=3, gain=2.0), "tiny": lambda: tiny_model(seed=3, gain=2.0),
             "fetch_arm": lambda: fetch_arm_model(seed=3, gain=2.0),
             "d16": lambda: custom_model(nb_nodes=3, dim=16, n_hidden=2, width=256, seed=3, gain=2.0),
             "n_hidden1": lambda: custom_model(nb_nodes=3, dim=9, n_hidden=1, width=512, seed=3, gain=2.0)}[which]()
    robot, hp, lay, sd = model
    s = _solver(model)
    n = 200 if which == "fetch_arm" else 300   # (FetchArm: 21 fp64 passes of 16 blocks per row)
    x, poses, cond = _rows(model, n, 41)
    _, ld = s.engine(DEV).flow_forward(x.to(DEV), poses.to(DEV))
    ld = ld.cpu().numpy()
    xs = x.numpy().astype(np.float64)
    fd = fd_logdet(lambda v: fo.flow_forward_f64(sd, lay, v, cond), xs)
    _, analytic = forward_with_logdet(sd, lay, xs, cond)
    err, err_fd = float(np.abs(ld - analytic).max()), np.abs(ld - fd)
    print(f"{which}: max |log_det - analytic| {err:.2e}; vs fd slogdet: median {np.median(err_fd):.2e}, max {err_fd.max():.2e}; "
          f"|log_det| up to {np.abs(fd).max():.1f}")
    assert _fd_agrees(analytic, fd) and _fd_agrees(ld.astype(np.float64), fd, LD_TOL)
    assert err <= LD_TOL, err


# ---- 3. round trips on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 17, 512, 4096])
def test_inverse_of_forward_and_position_independence(n):
    model = panda_model(seed=2)
    robot, hp, lay, sd = model
    s = _solver(model)
    eng = s.engine(DEV)
    x, poses, _ = _rows(model, n, 51, pad_scale=0.0)
    x[n - 1], poses[n - 1] = x[0], poses[0]
    X, P = x.to(DEV), poses.to(DEV)
    z, ld = eng.flow_forward(X, P)
    back = eng.generate_approx(P, z, clamp=False).cpu()
    err = float((back - x[:, : lay.ndof]).abs().max())
    print(f"B={n}: max |inverse(forward(x)) - x| {err:.2e}")
    assert err <= 3e-5, err
    assert torch.equal(z[0], z[n - 1]) and torch.equal(ld[0], ld[n - 1])
    z1, ld1 = eng.flow_forward(X[:1].contiguous(), P[:1].contiguous())
    assert torch.equal(z1[0], z[0]) and torch.equal(ld1[0], ld[0])


# ---- 4. sigmoid graph ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(nb_nodes=2, dim=7, n_hidden=3, width=1024), dict(nb_nodes=3, dim=7, n_hidden=2, width=256)])
def test_sigmoid_graph_round_trip_and_log_det(kw):
    model = custom_model(softflow=False, sigmoid=True, seed=8, **kw)
    robot, hp, lay, sd = model
    s = _solver(model)
    eng = s.engine(DEV)
    n = 300
    x, poses, cond = _rows(model, n, 61)
    z, ld = eng.flow_forward(x.to(DEV), poses.to(DEV))
    back = eng.generate_approx(poses.to(DEV), z, clamp=False).cpu()
    err = float((back - x[:, : lay.ndof]).abs().max())
    xs = x.numpy().astype(np.float64)
    z_ref, analytic = forward_with_logdet(sd, lay, xs, cond)
    fd = fd_logdet(lambda v: forward_with_logdet(sd, lay, v, cond)[0], xs)
    ld = ld.cpu().numpy().astype(np.float64)
    zerr, lerr = _zerr(z.cpu().numpy(), z_ref), float(np.abs(ld - analytic).max())
    print(f"sigmoid {kw}: round trip {err:.2e}, z {zerr:.2e}, log_det vs analytic {lerr:.2e}, vs fd median {np.median(np.abs(ld - fd)):.2e}")
    assert _fd_agrees(analytic, fd) and _fd_agrees(ld, fd, LD_TOL)
    assert err <= 3e-5 and zerr <= Z_TOL and lerr <= LD_TOL, (err, zerr, lerr)


# ---- 5. API -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_log_prob_nll_nn_forward_padding_and_broadcast():
    model = tiny_model(seed=9)
    robot, hp, lay, sd = model
    s = _solver(model)
    n = 40
    x, poses, _ = _rows(model, n, 71, pad_scale=0.0)
    q, P = x[:, : lay.ndof].to(DEV), poses.to(DEV)
    lp = s.log_prob(q, P)
    nll = s.nll(q, P)
    assert lp.shape == (n,) and nll.shape == (n,) and lp.dtype == torch.float32
    torch.testing.assert_close(lp, -nll - 0.5 * lay.dim * math.log(2 * math.pi), rtol=0, atol=1e-4)
    zeros = torch.zeros(n, lay.dim - lay.ndof, device=DEV)
    assert torch.equal(s.log_prob(q, P, pad=zeros), lp)
    assert not torch.equal(s.log_prob(q, P, pad=zeros + 0.01), lp)
    # one pose for every row == that pose repeated
    one = s.log_prob(q, P[3])
    assert torch.equal(one, s.log_prob(q, P[3:4].expand(n, 7).contiguous()))
    # nn_forward: the reference's (z, log|det J|) with the conditional [pose, softflow]
    z, ld = s.nn_forward(x.to(DEV), torch.cat([P, torch.zeros(n, 1, device=DEV)], 1))
    assert torch.equal(nll, 0.5 * (z * z).sum(1) - ld)
    # the softflow column is honoured
    z5, _ = s.engine(DEV).flow_forward(x.to(DEV), P, softflow_scale=0.5)
    assert not torch.equal(z5, z)
    z5b, _ = s.nn_forward(x.to(DEV), torch.cat([P, torch.full((n, 1), 0.5, device=DEV)], 1))
    assert torch.equal(z5b, z5)


@pytest.mark.gpu
def test_cabi_status_codes():
    from ikflow_amd.engine import Engine

    model = tiny_model()
    robot, hp, lay, sd = model
    eng = Engine(lay, robot, DEV)
    lib = eng.lib
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.zeros(4, lay.dim, device=DEV)
    p = torch.zeros(4, 7, device=DEV)
    z = torch.zeros(4, lay.dim, device=DEV)
    ld = torch.zeros(4, device=DEV)
    code = lib.ikf_flow_forward(eng._h, x.data_ptr(), 4, p.data_ptr(), 0, 0.0, z.data_ptr(), ld.data_ptr(), stream)
    assert code == _lib.IKF_ERR_NOT_LOADED and "Model weights have not been loaded" in _lib.last_error()
    eng.load_state_dict(sd)
    assert lib.ikf_flow_forward(None, x.data_ptr(), 4, p.data_ptr(), 0, 0.0, z.data_ptr(), ld.data_ptr(), stream) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_flow_forward(eng._h, None, 4, p.data_ptr(), 0, 0.0, z.data_ptr(), ld.data_ptr(), stream) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_flow_forward(eng._h, x.data_ptr(), 4, None, 0, 0.0, z.data_ptr(), ld.data_ptr(), stream) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_flow_forward(eng._h, x.data_ptr(), 4, p.data_ptr(), 0, 0.0, None, None, stream) == _lib.IKF_ERR_NULL_POINTER
    assert lib.ikf_flow_forward(eng._h, x.data_ptr(), -1, p.data_ptr(), 0, 0.0, z.data_ptr(), ld.data_ptr(), stream) == _lib.IKF_ERR_BAD_ARGUMENT
    assert lib.ikf_flow_forward(eng._h, None, 0, None, 0, 0.0, None, None, stream) == _lib.IKF_OK
    # each output alone
    assert lib.ikf_flow_forward(eng._h, x.data_ptr(), 4, p.data_ptr(), 0, 0.0, z.data_ptr(), None, stream) == _lib.IKF_OK
    assert lib.ikf_flow_forward(eng._h, x.data_ptr(), 4, p.data_ptr(), 0, 0.0, None, ld.data_ptr(), stream) == _lib.IKF_OK
    torch.cuda.synchronize()
    z2, ld2 = eng.flow_forward(x, p)
    assert torch.equal(z, z2) and torch.equal(ld, ld2)


@pytest.mark.gpu
@pytest.mark.parametrize("which,n", [("panda", 4096), ("tiny", 1000), ("tiny", 20000)])
def test_forward_call_can_be_captured_into_a_hip_graph(which, n):
    """After ikf_load_weights + ikf_reserve the forward call allocates nothing and never synchronises: it can be captured.  TINY at
    20000 rows: the per-layer chunk loop (16384 + 3616 rows) inside one graph."""
    model = {"panda": panda_model, "tiny": tiny_model}[which]()
    s = _solver(model)
    eng = s.engine(DEV)
    eng.reserve(max(8192, n))
    x, poses, _ = _rows(model, n, 81)
    X, P = x.to(DEV), poses.to(DEV)
    ref = [t.clone() for t in eng.flow_forward(X, P)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            eng.flow_forward(X, P)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        z, ld = eng.flow_forward(X, P)
    for _ in range(2):
        with torch.inference_mode():
            z.zero_()
            ld.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(z, ref[0]) and torch.equal(ld, ref[1])


# ==== coverage of every shape, batch edge and input form (both device paths) ===========================================================
# Row-owner path: width padded to 1024 with 3 hidden layers (k_flow_rowowner_fwd, 16-row tiles, one launch per 2^24 rows).  Per-layer path:
# every other shape (k_fwd_entry, k_first_layer, k_gemm_lrelu, k_last_layer_coupling_fwd<OUT>, chunks of chunk_cap rows: 16384 up to width
# 1024, 16384 * 1024 / width above).  Where the fp64 references over every row would cost minutes on the CPU (width 1024 and above at
# tens of thousands of rows), a test compares a fixed seeded sample that always holds the first row, the last row and both rows at every
# tile / chunk edge it names - each test says which applies.
RO_ROWS = 16
CHUNK = 16384
SENTINEL = 0x7FC0DEAD   # a NaN whose payload no kernel writes


def _cond(lay, poses, soft=0.0):
    """The oracle's conditional: [pose] or [pose, softflow scale]."""
    c = np.asarray(poses, dtype=np.float64)
    if lay.dim_cond == 8:
        c = np.concatenate([c, np.full((c.shape[0], 1), soft)], 1)
    return c


def _refs(sd, lay, x, cond):
    """fp64 (z, log|det J|): z from the oracle's own forward (forward_with_logdet's on sigmoid graphs, which the oracle does not run)."""
    xs = np.asarray(x, dtype=np.float64)
    z_ld, ld_ref = forward_with_logdet(sd, lay, xs, cond)
    return (z_ld if lay.sigmoid_on_output else fo.flow_forward_f64(sd, lay, xs, cond)), ld_ref


def _edge_rows(n, edges=(), k=256, seed=0):
    """Row sample: first, last, both rows at every edge, k seeded random rows (sorted, unique)."""
    s = {0, n - 1}
    for e in edges:
        s.update(r for r in (e - 1, e) if 0 <= r < n)
    s.update(np.random.default_rng(seed).integers(0, n, size=min(k, n)).tolist())
    return np.array(sorted(s))


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _check(tag, sd, lay, x, cond, z, ld, rows=None, noise=False):
    """z (Z_TOL relative to max(1, |z|)) and log|det J| (LD_TOL absolute) against the fp64 references on `rows` (None: every row).
    noise=True (random trained-like weights): where an f32 evaluation of the same graph (forward_with_logdet, dt=float32) is itself
    further than the tolerance from fp64, the kernel may be up to 4x that f32 noise away instead - printed, so that the cause shows."""
    x, z, ld = _np(x), _np(z), _np(ld)
    idx = np.arange(z.shape[0]) if rows is None else np.asarray(rows)
    z_ref, ld_ref = _refs(sd, lay, x[idx], cond[idx])
    zerr, lerr = _zerr(z[idx], z_ref), float(np.abs(ld[idx] - ld_ref).max())
    line = (f"{tag}: {'every row' if rows is None else f'{len(idx)} sampled rows'} of {z.shape[0]}: max |dz| rel {zerr:.2e}, "
            f"max |dlog_det| {lerr:.2e} (|log_det| up to {np.abs(ld_ref).max():.1f})")
    assert np.isfinite(z[idx]).all() and np.isfinite(ld[idx]).all(), tag
    ztol, ltol = Z_TOL, LD_TOL
    if noise and (zerr > Z_TOL or lerr > LD_TOL):
        z32, ld32 = forward_with_logdet(sd, lay, x[idx], cond[idx], dt=np.float32)
        zn, ln = _zerr(z32, z_ref), float(np.abs(ld32.astype(np.float64) - ld_ref).max())
        line += f"; f32 evaluation noise: z {zn:.2e}, log_det {ln:.2e}"
        ztol, ltol = max(Z_TOL, 4 * zn), max(LD_TOL, 4 * ln)
    print(line)
    assert zerr <= ztol and lerr <= ltol, line
    return zerr, lerr


def _guarded_forward(eng, X, P, broadcast=False, soft=0.0):
    """ikf_flow_forward through the raw C-ABI into z / log_det with 64 extra rows of a NaN sentinel, which must come back bit-unchanged."""
    n, D = X.shape
    zb = torch.full((n + 64, D), SENTINEL, dtype=torch.int32, device=DEV)
    lb = torch.full((n + 64,), SENTINEL, dtype=torch.int32, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = eng.lib.ikf_flow_forward(eng._h, X.data_ptr(), n, P.data_ptr(), 1 if broadcast else 0, soft, zb.data_ptr(), lb.data_ptr(), stream)
    assert code == _lib.IKF_OK, _lib.last_error()
    torch.cuda.synchronize()
    assert bool((zb[n:] == SENTINEL).all()) and bool((lb[n:] == SENTINEL).all()), f"n={n}: store past row n - 1"
    return zb[:n].view(torch.float32), lb[:n].view(torch.float32)


# ---- 7. random and fixed configurations ---------------------------------------------------------------------------------------------
def _random_forward_configs(count, seed):
    """The forward twin of test_gpu_parity._random_flow_configs: any nb_nodes / dim / depth / width IkflowModelParameters can express."""
    rng = np.random.default_rng(seed)
    widths = [1, 16, 100, 255, 256, 257, 300, 512, 640, 768, 1000, 1024, 1100, 1280, 1536, 2048]
    out = []
    for _ in range(count):
        robot_name = str(rng.choice(["panda", "fetch", "fetch_arm"]))
        ndof = O(robot_name).ndof
        sigmoid = bool(rng.integers(0, 4) == 0)
        out.append(dict(nb_nodes=int(rng.integers(1, 5)), dim=int(rng.integers(ndof, 17)), n_hidden=int(rng.integers(1, 5)),
                        width=int(rng.choice(widths)), robot_name=robot_name, softflow=bool(rng.integers(0, 2)) and not sigmoid,
                        sigmoid=sigmoid, seed=int(rng.integers(0, 1000)), gain=float(rng.choice([1.0, 1.5, 2.5])),
                        n=int(rng.choice([1, 2, 15, 16, 17, 31, 33, 127, 128, 129, 255, 257, 513, 700])), soft=float(rng.choice([0.0, 0.37]))))
    return out


def _fixed_forward_configs():
    """Cases that run whatever the seed: D = 11 .. 16 (OUT = 12, 14, 16 of k_last_layer_coupling_fwd), one and four hidden layers, width
    300 (zero-padded to 512), width 2048 and 4096 above their chunk cap (8192 / 4096 rows: 2 and 3 chunks)."""
    base = dict(nb_nodes=2, n_hidden=2, width=256, robot_name="panda", softflow=True, sigmoid=False, gain=1.5, soft=0.0)
    out = [dict(base, dim=d, seed=10 + d, n=300 + d, soft=0.37 if d % 2 else 0.0) for d in range(11, 17)]
    out += [dict(base, dim=9, n_hidden=1, width=512, nb_nodes=3, seed=31, n=1025),
            dict(base, dim=9, n_hidden=4, width=256, nb_nodes=3, seed=32, n=700),
            dict(base, dim=10, width=300, seed=33, n=513, robot_name="fetch_arm"),
            dict(base, dim=8, width=2048, seed=34, n=8192 + 129, gain=1.0),
            dict(base, dim=9, width=4096, seed=35, n=4096 * 2 + 33, gain=1.0)]
    return out


def _cfg_id(c):
    return "-".join(str(v) for v in c.values())


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", _fixed_forward_configs() + _random_forward_configs(int(os.environ.get("IKF_FUZZ_FORWARD_COUNT", "32")),
                                                                                     int(os.environ.get("IKF_FUZZ_SEED", "20260928"))), ids=_cfg_id)
def test_forward_random_and_fixed_configurations(cfg):
    """z and log|det J| on every row against the fp64 references (width >= 2048 above 4096 rows: an edge sample, see _edge_rows) and the
    round trip through generate_approx.  Gain 2.5 draws may take the f32-noise bound of _check (printed)."""
    cfg = dict(cfg)
    n, soft = cfg.pop("n"), cfg.pop("soft")
    model = custom_model(**cfg)
    robot, hp, lay, sd = model
    soft = soft if lay.dim_cond == 8 else 0.0
    eng = _solver(model).engine(DEV)
    x, poses, _ = _rows(model, n, cfg["seed"] + 1)
    cond = _cond(lay, poses.numpy(), soft)
    X, P = x.to(DEV), poses.to(DEV)
    z, ld = eng.flow_forward(X, P, softflow_scale=soft)
    cap = CHUNK * 1024 // max(1024, -(-cfg["width"] // 256) * 256) // 128 * 128
    rows = None if (cfg["width"] < 2048 or n <= 4096) else _edge_rows(n, range(cap, n, cap), 256, cfg["seed"])
    _check(f"{_cfg_id(cfg)} n={n} soft={soft}", sd, lay, x, cond, z, ld, rows, noise=cfg["gain"] > 2.0)
    back = eng.generate_approx(P, z, clamp=False, softflow_scale=soft).cpu()
    err = float((back - x[:, : lay.ndof]).abs().max())
    print(f"   round trip {err:.2e}")
    assert err <= (3e-5 if cfg["gain"] < 2.0 else 3e-4), err


# ---- 8. batch edges, both paths; nothing is written past row n - 1 -----------------------------------------------------------------
@pytest.mark.gpu
def test_rowowner_batch_edges_and_no_store_past_the_batch():
    """Panda (row-owner): n around the 16-row tile and the 256 / 4096-row marks.  Rows 0 .. 4096 are compared with the fp64 references on
    every row; at 20000 rows, above that, an edge sample (every 1024th tile edge + 256 seeded rows).  The same row gives the same bits at
    every n (the launch computes a tile independently of the grid)."""
    model = panda_model(seed=11)
    robot, hp, lay, sd = model
    eng = _solver(model).engine(DEV)
    N = 20000
    x, poses, _ = _rows(model, N, 91)
    cond = _cond(lay, poses.numpy())
    X, P = x.to(DEV), poses.to(DEV)
    z_all, ld_all = _guarded_forward(eng, X, P)
    rows = np.union1d(np.arange(4097), _edge_rows(N, range(4096, N, 1024), 256, 5))
    _check(f"panda n={N}", sd, lay, x, cond, z_all, ld_all, rows)
    for n in (1, 15, 16, 17, 31, 33, 255, 257, 4095, 4097):
        z, ld = _guarded_forward(eng, X[:n].contiguous(), P[:n].contiguous())
        assert torch.equal(z, z_all[:n]) and torch.equal(ld, ld_all[:n]), f"n={n}"
        print(f"panda n={n}: bit-identical to rows 0..{n - 1} of the {N}-row call (compared above), tail rows unchanged")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["tiny", "width300"])
def test_per_layer_batch_edges_and_no_store_past_the_batch(which):
    """Per-layer path: n around the 128-row contraction tile and the 16384-row chunk (r0 > 0 in the chunk loop: 40000 = 2 x 16384 + 7232).
    Every row of every call against the fp64 references (these widths are cheap on the CPU)."""
    model = tiny_model(seed=12) if which == "tiny" else custom_model(nb_nodes=2, dim=10, n_hidden=3, width=300, robot_name="fetch_arm", seed=12)
    robot, hp, lay, sd = model
    eng = _solver(model).engine(DEV)
    N = 40000
    x, poses, _ = _rows(model, N, 92)
    cond = _cond(lay, poses.numpy())
    X, P = x.to(DEV), poses.to(DEV)
    for n in (1, 3, 127, 128, 129, 16383, 16384, 16385, N):
        z, ld = _guarded_forward(eng, X[:n].contiguous(), P[:n].contiguous())
        _check(f"{which} n={n}", sd, lay, x[:n], cond[:n], z, ld)


@pytest.mark.gpu
def test_rowowner_launch_split_at_two_to_the_24_rows():
    """2^24 + 33 Panda rows with per-row poses in ONE call: the row-owner path launches twice (r0 = 2^24 shifts x, the pose row, z and
    log_det).  fp64 references on every row of the window 2^24 +- 2048 and the last 33 rows; the second launch's rows are bit-identical
    to the same rows submitted on their own.  (Inputs drawn on the device: in-limit q, poses from the device FK.)"""
    model = panda_model(seed=13)
    robot, hp, lay, sd = model
    eng = _solver(model).engine(DEV)
    split = 1 << 24
    n = split + 33
    g = torch.Generator(device=DEV).manual_seed(6)
    lo = torch.tensor([l[0] for l in O(robot).actuated_joints_limits], device=DEV, dtype=torch.float32)
    hi = torch.tensor([l[1] for l in O(robot).actuated_joints_limits], device=DEV, dtype=torch.float32)
    X = lo + (hi - lo) * torch.rand((n, lay.dim), generator=g, device=DEV)
    P = robot.forward_kinematics(X[:, : lay.ndof].contiguous())
    z, ld = eng.flow_forward(X, P)
    torch.cuda.synchronize()
    rows = np.concatenate([np.arange(split - 2048, split + 33), np.arange(n - 33, n)])
    rows = torch.from_numpy(np.unique(rows)).to(DEV)
    _check("panda n=2^24+33", sd, lay, X[rows].cpu(), _cond(lay, P[rows].cpu().numpy()), z[rows], ld[rows])
    z2, ld2 = eng.flow_forward(X[split:].contiguous(), P[split:].contiguous())
    assert torch.equal(z2, z[split:]) and torch.equal(ld2, ld[split:])
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(ld).all())


# ---- 9. conditional forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny"])
@pytest.mark.parametrize("soft", [0.0, 0.37])
def test_softflow_scale_against_the_oracle(which, soft):
    """The 8th conditional entry on both paths (row-owner: RO_OFF_COND slot 7) against the oracle run on [pose, scale], every row."""
    model = panda_model(seed=14) if which == "panda" else tiny_model(seed=14)
    robot, hp, lay, sd = model
    eng = _solver(model).engine(DEV)
    n = 600
    x, poses, _ = _rows(model, n, 93)
    z, ld = eng.flow_forward(x.to(DEV), poses.to(DEV), softflow_scale=soft)
    _check(f"{which} softflow {soft}", sd, lay, x, _cond(lay, poses.numpy(), soft), z, ld)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny"])
def test_pose_broadcast_equals_the_repeated_pose(which):
    """pose_broadcast = 1 (one pose for every row) is bit-identical to that pose repeated, on the row-owner and the per-layer path, and
    matches the oracle; nn_forward with an 8-column conditional is the engine call with that scale."""
    model = panda_model(seed=15) if which == "panda" else tiny_model(seed=15)
    robot, hp, lay, sd = model
    s = _solver(model)
    eng = s.engine(DEV)
    n = 333
    x, poses, _ = _rows(model, n, 94)
    X = x.to(DEV)
    one = poses[5].to(DEV)
    z, ld = eng.flow_forward(X, one, softflow_scale=0.37)
    zr, ldr = eng.flow_forward(X, one.expand(n, 7).contiguous(), softflow_scale=0.37)
    assert torch.equal(z, zr) and torch.equal(ld, ldr)
    _check(f"{which} broadcast", sd, lay, x, _cond(lay, poses[5:6].expand(n, 7).numpy(), 0.37), z, ld)
    zc, ldc = s.nn_forward(X, torch.cat([one.expand(n, 7), torch.full((n, 1), 0.37, device=DEV)], 1))
    assert torch.equal(zc, z) and torch.equal(ldc, ld)


# ---- 10. load-time branches ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny"])
def test_state_dict_without_M(which):
    """No module_list.0.M: load inverts M_inv in fp64 and log|det M| = -log|det M_inv|.  Against the references, which do the same."""
    model = panda_model(seed=16, gain=1.5) if which == "panda" else tiny_model(seed=16, gain=1.5)
    robot, hp, lay, sd = model
    sd = {k: v for k, v in sd.items() if k != "module_list.0.M"}
    model = (robot, hp, lay, sd)
    eng = _solver(model).engine(DEV)
    n = 500
    x, poses, _ = _rows(model, n, 95)
    z, ld = eng.flow_forward(x.to(DEV), poses.to(DEV))
    _check(f"{which} without M", sd, lay, x, _cond(lay, poses.numpy()), z, ld)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny"])
@pytest.mark.parametrize("with_M", [True, False])
def test_dense_fixed_linear_transform_with_bias(which, with_M):
    """A dense M and a non-zero b (with M in the state_dict, and without it: inverted at load) against the references on every row,
    and the round trip through the inverse pass (which applies (x - b).mm(M_inv))."""
    model = _dense_fixed_transform(panda_model(seed=22) if which == "panda" else tiny_model(seed=22), 23)
    robot, hp, lay, sd = model
    if not with_M:
        sd = {k: v for k, v in sd.items() if k != "module_list.0.M"}
        model = (robot, hp, lay, sd)
    eng = _solver(model).engine(DEV)
    n = 700
    x, poses, _ = _rows(model, n, 101, pad_scale=0.0)
    P = poses.to(DEV)
    z, ld = eng.flow_forward(x.to(DEV), P)
    _check(f"{which} dense M, b != 0, M {'given' if with_M else 'from M_inv'}", sd, lay, x, _cond(lay, poses.numpy()), z, ld)
    back = eng.generate_approx(P, z, clamp=False).cpu()
    err = float((back - x[:, : lay.ndof]).abs().max())
    print(f"   round trip {err:.2e}")
    assert err <= 3e-5, err


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny"])
def test_reload_refreshes_every_forward_table(which):
    """load A, forward, load B (trained-like gain 2.5, different permutations and M) on the same handle, forward: bit-identical to a fresh
    handle loaded with B; then back to A."""
    make = panda_model if which == "panda" else tiny_model
    A, B = make(seed=17), make(seed=18, gain=2.5)
    n = 4100 if which == "panda" else 20000
    x, poses, _ = _rows(A, n, 96)
    X, P = x.to(DEV), poses.to(DEV)
    s = _solver(A)
    eng = s.engine(DEV)
    za, lda = [t.clone() for t in eng.flow_forward(X, P)]
    s.load_state_dict_tensors(B[3])
    zb, ldb = eng.flow_forward(X, P)
    fz, fld = _solver(B).engine(DEV).flow_forward(X, P)
    assert torch.equal(zb, fz) and torch.equal(ldb, fld)
    assert not torch.equal(zb, za)
    rows = _edge_rows(n, (CHUNK,), 128, 7)
    _check(f"{which} reloaded B", B[3], B[2], x, _cond(B[2], poses.numpy()), zb, ldb, rows, noise=True)
    s.load_state_dict_tensors(A[3])
    z2, ld2 = eng.flow_forward(X, P)
    assert torch.equal(z2, za) and torch.equal(ld2, lda)


# ---- 11. engine settings ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_hidden", [2, 3])
def test_forward_under_every_gemm_variant(n_hidden):
    """The per-layer forward picks its contraction with pick_variant: each forced variant 0 .. 8 against the references, partial tiles
    included (every row)."""
    model = custom_model(nb_nodes=2, dim=9, n_hidden=n_hidden, width=256, seed=19, gain=1.5)
    robot, hp, lay, sd = model
    eng = _solver(model).engine(DEV)
    n_max = 700
    x, poses, _ = _rows(model, n_max, 97)
    cond = _cond(lay, poses.numpy())
    X, P = x.to(DEV), poses.to(DEV)
    worst = (0.0, 0.0)
    for variant in range(9):
        eng.set_gemm_variant(variant)
        for n in (1, 100, 129, n_max):
            z, ld = eng.flow_forward(X[:n].contiguous(), P[:n].contiguous())
            z_ref, ld_ref = _refs(sd, lay, x.numpy()[:n], cond[:n])
            zerr, lerr = _zerr(z.cpu().numpy(), z_ref), float(np.abs(ld.cpu().numpy() - ld_ref).max())
            assert zerr <= Z_TOL and lerr <= LD_TOL, (variant, n, zerr, lerr)
            worst = (max(worst[0], zerr), max(worst[1], lerr))
    eng.set_gemm_variant(-1)
    print(f"n_hidden={n_hidden}, variants 0..8: max |dz| rel {worst[0]:.2e}, max |dlog_det| {worst[1]:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny"])
def test_f16x3_precision_leaves_the_forward_pass_in_f32(which):
    """set_precision("f16x3") selects the split contraction of the INVERSE pass only: ikf_flow_forward always runs the f32 contractions,
    so its result is bit-identical to the f32 mode on both paths (include/ikflow_amd.h, ikf_flow_forward)."""
    model = panda_model(seed=20) if which == "panda" else tiny_model(seed=20)
    eng = _solver(model).engine(DEV)
    x, poses, _ = _rows(model, 1500, 98)
    X, P = x.to(DEV), poses.to(DEV)
    ref = [t.clone() for t in eng.flow_forward(X, P)]
    eng.set_precision("f16x3")
    assert eng.precision == "f16x3"
    z, ld = eng.flow_forward(X, P)
    assert torch.equal(z, ref[0]) and torch.equal(ld, ref[1])


# ---- 12. both directions on one handle ----------------------------------------------------------------------------------------------
def _interleaved_calls(model, seed):
    robot, hp, lay, sd = model
    x, poses, _ = _rows(model, 20000, seed)
    X, P = x.to(DEV), poses.to(DEV)
    lat = latents(20000, lay.dim, seed + 1).to(DEV)
    # (direction, n): a per-layer forward above the chunk size between two inverse calls, small and odd sizes around it
    plan = [("inv", 3000), ("fwd", 20000), ("inv", 17000), ("fwd", 129), ("inv", 1), ("fwd", 4097), ("inv", 20000), ("fwd", 1)]

    def call(eng, d, n):
        if d == "fwd":
            return eng.flow_forward(X[:n], P[:n])
        return (eng.generate_approx(P[:n], lat[:n], clamp=False),)
    return plan, call


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "tiny"])
@pytest.mark.parametrize("two_streams", [False, True])
def test_forward_and_inverse_interleaved_on_one_handle(which, two_streams):
    """flow_forward and generate_approx alternating on one handle (shared per-layer scratch), at batch sizes on both sides of the chunk,
    from one stream or alternating between two without host synchronisation: every result bit-identical to the same call made alone."""
    model = panda_model(seed=21) if which == "panda" else tiny_model(seed=21)
    eng = _solver(model).engine(DEV)
    plan, call = _interleaved_calls(model, 99)
    want = []
    for d, n in plan:
        want.append([t.clone() for t in call(eng, d, n)])
        torch.cuda.synchronize()
    streams = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)] if two_streams else [torch.cuda.current_stream(DEV)]
    got = []
    for i, (d, n) in enumerate(plan):
        with torch.cuda.stream(streams[i % len(streams)]):
            got.append(call(eng, d, n))
    torch.cuda.synchronize()
    for (d, n), a, b in zip(plan, want, got):
        assert all(torch.equal(u, v) for u, v in zip(a, b)), f"{d} n={n}"


# ---- 13. released architectures -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("model_name", ["panda_lite_tpm", "fetch_full_temp_nsc_tpm", "fetch__large__ns183_9.75m"])
def test_every_released_architecture_forward(model_name):
    """The released architectures besides Panda-full and FetchArm (6-block Panda; 12- and 16-block Fetch, D = 8), every row."""
    model = released_model(model_name, seed=4)
    robot, hp, lay, sd = model
    eng = _solver(model).engine(DEV)
    n = 1000
    x, poses, _ = _rows(model, n, 100)
    z, ld = eng.flow_forward(x.to(DEV), poses.to(DEV))
    _check(model_name, sd, lay, x, _cond(lay, poses.numpy()), z, ld)
