"""The per-element arithmetic of the flow kernels (ikflow_amd/csrc/flow_math.h: pose row, affine coupling in both directions, the sigmoid layer
and the logit with their log-det terms, the FixedLinearTransform step, the limit clamp) compiled for the HOST with g++ and held against fp64 and
the oracle - the kernels' own source, checked without a GPU.  The GPU tests check the same code in every flow form where it ships
(tests/test_flow_forward.py, test_flow_inverse.py, test_flow_sample*.py, test_gpu_parity.py); this one pins the arithmetic they all share on every
CPU run.  Test infrastructure: nothing in ikflow_amd/ loads it.

Bounds of the scalar steps: the worst error of a numpy float32 evaluation of the same formula (every operation rounded on its own) against fp64
on the same inputs, times 4 - glibc's and numpy's atanf / expf / log1pf each differ by a few ulp and up to three of them chain.  Errors are
relative to max(1, |reference|).  Measured when this test was written (numpy's error, the bound = 4 x it, the header's error):
    coupling_scale            1.66e-07   6.65e-07   1.23e-07
    coupling_inv              2.15e-07   8.60e-07   1.64e-07     (the same figures for the factor / apply spelling of the wave kernels)
    coupling_fwd              2.99e-06   1.19e-05   1.93e-06     (e^s x + t cancels: operands up to 244, results down to 0)
    fwd(inv(x)) round trip    4.71e-06   1.88e-05   2.86e-06     (against x itself)
    sigmoid_rev               8.36e-08   3.34e-07   8.36e-08
    sigmoid_rev_ld            1.37e-07   5.46e-07   9.43e-08
    logit_fwd                 1.23e-07   4.92e-07   1.23e-07
    logit_fwd_ld              1.09e-07   4.37e-07   1.12e-07
Exit transform on TINY (dense FixedLinearTransform): x 5.5e-07 (plain) / 4.2e-07 (sigmoid) against FLOW_TOL 1e-5, log-det 6.7e-07 / 4.9e-06 against LD_TOL 1e-4.
The test computes numpy's error where it runs, so the bound follows the numpy it meets; the figures above are what to expect."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from flow_logdet import forward_with_logdet
from helpers import O, _dense_fixed_transform, tiny_model
from oracle import flow_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOW_TOL = 1e-5     # relative to max(1, |x|): tests/test_flow_inverse.py
LD_TOL = 1e-4       # absolute:                tests/test_flow_inverse.py
GAIN = np.float32(0.636)
CLAMP = np.float32(2.5)
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("flow_math") / "libflow_math_host.so"
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "flow_math_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(str(out))
    lib.flow_math_step.restype = C.c_int
    lib.flow_math_step.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.flow_math_pose_rows.restype = None
    lib.flow_math_pose_rows.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.flow_math_exit.restype = None
    lib.flow_math_exit.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def _step(lib, what, a, b=None, c=None):
    a = np.ascontiguousarray(a, dtype=f32)
    b = a if b is None else np.ascontiguousarray(np.broadcast_to(b, a.shape), dtype=f32)
    c = a if c is None else np.ascontiguousarray(np.broadcast_to(c, a.shape), dtype=f32)
    out = np.full(a.shape, np.nan, f32)
    assert lib.flow_math_step(what, a.ctypes.data, b.ctypes.data, c.ctypes.data, a.size, out.ctypes.data) == 0
    return out


# ---- pose row -------------------------------------------------------------------------------------------------------------------------------
N_ROWS = 37


@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("n_mod", [1, N_ROWS - 1, N_ROWS, N_ROWS + 1, 2 * N_ROWS + 3])
def test_pose_row_is_exact_at_every_seam_and_beyond_2_to_the_31(host_lib, n_mod, with_idx):
    """pose_row(r) == idx[r % n_mod] (r % n_mod without a list): every row of a call of N_ROWS rows, both sides of the first seams of the modulus,
    and r = 2^31 - 1, 2^31, 2^31 + 1 with the seams around them (row indices are 64-bit)."""
    rows = set(range(N_ROWS)) | {2**31 - 1, 2**31, 2**31 + 1}
    for k in list(range(1, 6)) + [2**31 // n_mod, 2**31 // n_mod + 1]:
        rows |= {k * n_mod - 1, k * n_mod, k * n_mod + 1}
    rows = np.array(sorted(r for r in rows if r >= 0), dtype=np.int64)
    idx = np.random.default_rng(n_mod).integers(0, 1000, size=n_mod).astype(np.int32) if with_idx else None
    out = np.full(rows.shape, -1, np.int64)
    host_lib.flow_math_pose_rows(idx.ctypes.data if with_idx else None, n_mod, rows.ctypes.data, rows.size, out.ctypes.data)
    want = [int(idx[int(r) % n_mod]) if with_idx else int(r) % n_mod for r in rows]
    assert out.tolist() == want


# ---- scalar steps against fp64 --------------------------------------------------------------------------------------------------------------
def _signed_log(lo, hi, n):
    m = np.logspace(np.log10(lo), np.log10(hi), n)
    return np.concatenate([-m[::-1], [0.0], m])


def _s_values():
    """s over +-1e4: log-spaced magnitudes from 1e-4 (atan's linear range) to 1e4 (its saturation), a dense linear run around 0, the ends."""
    return np.concatenate([_signed_log(1e-4, 1e4, 400), np.linspace(-8, 8, 801), [-1e4, 1e4]]).astype(f32)


def _coupling_inputs():
    """(x, t, s_cl): states and shifts over +-20, s_cl = the clamped scale of the s values above (|s_cl| <= 2.5), every combination of a
    coarse grid plus seeded random triples."""
    rng = np.random.default_rng(5)
    s_cl = (CLAMP * (GAIN * np.arctan(_s_values()))).astype(f32)
    g = np.linspace(-20, 20, 17).astype(f32)
    gx, gt, gs = np.meshgrid(g, g, s_cl[::16], indexing="ij")
    n = 20000
    x = np.concatenate([gx.ravel(), rng.uniform(-20, 20, n)]).astype(f32)
    t = np.concatenate([gt.ravel(), rng.uniform(-20, 20, n)]).astype(f32)
    s = np.concatenate([gs.ravel(), rng.choice(s_cl, n)]).astype(f32)
    return x, t, s


def _sigmoid_args():
    """+-88 (expf's range): log-spaced magnitudes, a dense run over +-20, and 17 .. 88 where sigmoid(x) rounds to 1 and log(v (1 - v)) written
    naively is log(0)."""
    return np.concatenate([_signed_log(1e-4, 88.0, 300), np.linspace(-20, 20, 2001), np.linspace(17, 88, 143), -np.linspace(17, 88, 143)]).astype(f32)


def _open_unit():
    """v in (0, 1) as the forward pass meets it: the f32 sigmoid of the arguments above, without the values that rounded to 0 or 1."""
    a = _sigmoid_args()
    v = (f32(1) / (f32(1) + np.exp(-a))).astype(f32)
    return v[(v > 0) & (v < 1)]


def _err(got, ref):
    return float((np.abs(got.astype(f64) - ref) / np.maximum(1.0, np.abs(ref))).max())


def _cases():
    x, t, s_cl = _coupling_inputs()
    s = _s_values()
    a = _sigmoid_args()
    v = _open_unit()
    X, T, S, A, V = (q.astype(f64) for q in (x, t, s_cl, a, v))
    one = f32(1)
    with np.errstate(over="ignore"):
        return {
            # name: (harness step, its operands, numpy float32 evaluation, fp64 reference)
            "coupling_scale": (0, (np.full_like(s, CLAMP), s), CLAMP * (GAIN * np.arctan(s)), f64(CLAMP) * (f64(GAIN) * np.arctan(s.astype(f64)))),
            "coupling_inv": (1, (x, t, s_cl), (x - t) * np.exp(-s_cl), (X - T) * np.exp(-S)),
            "coupling_fwd": (2, (x, t, s_cl), np.exp(s_cl) * x + t, np.exp(S) * X + T),
            "coupling_inv_2step": (3, (x, t, s_cl), (x - t) * np.exp(-s_cl), (X - T) * np.exp(-S)),
            "coupling_fwd_2step": (4, (x, t, s_cl), np.exp(s_cl) * x + t, np.exp(S) * X + T),
            "round_trip": (5, (x, t, s_cl), np.exp(s_cl) * ((x - t) * np.exp(-s_cl)) + t, X),
            "sigmoid_rev": (7, (a,), one / (one + np.exp(-a)), 1.0 / (1.0 + np.exp(-A))),
            "sigmoid_rev_ld": (8, (a,), -np.abs(a) - f32(2) * np.log1p(np.exp(-np.abs(a))), -np.abs(A) - 2.0 * np.log1p(np.exp(-np.abs(A)))),
            "logit_fwd": (9, (v,), np.log(v / (one - v)), np.log(V / (1.0 - V))),
            "logit_fwd_ld": (10, (v,), -(np.log(v) + np.log1p(-v)), -(np.log(V) + np.log1p(-V))),
        }


@pytest.mark.parametrize("name", ["coupling_scale", "coupling_inv", "coupling_fwd", "coupling_inv_2step", "coupling_fwd_2step", "round_trip",
                                  "sigmoid_rev", "sigmoid_rev_ld", "logit_fwd", "logit_fwd_ld"])
def test_scalar_step_of_the_kernel_source_against_fp64(host_lib, name):
    """The header's step within 4 x the error of a numpy float32 evaluation of the same formula, both against fp64 on the same f32 inputs,
    relative to max(1, |reference|) (figures: the module docstring).  round_trip: coupling_fwd(coupling_inv(x, t, s), t, s) against x itself."""
    what, operands, np32, ref = _cases()[name]
    assert np32.dtype == f32 and ref.dtype == f64
    got = _step(host_lib, what, *operands)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    e_np, e_got = _err(np32, ref), _err(got, ref)
    print(f"{name}: {got.size} elements: numpy float32 {e_np:.2e}, bound {4 * e_np:.2e}, header {e_got:.2e}")
    assert 0 < e_np < 3e-5      # the yardstick is f32 rounding noise - not zero, not a wrong formula: one ulp of the largest operand, 20 e^2.5 = 244
    assert e_got <= 4 * e_np, (e_got, e_np)


def test_the_two_log_det_shares_of_a_coupling_cancel_exactly(host_lib):
    """coupling_fwd_ld(s) + coupling_inv_ld(s) is +0.0f, bit for bit, for every clamped scale."""
    _, _, s_cl = _coupling_inputs()
    out = _step(host_lib, 6, s_cl, s_cl, s_cl)
    assert not out.view(np.uint32).any()


def test_sigmoid_log_det_where_the_naive_form_cancels(host_lib):
    """Beyond |x| = 17 the f32 sigmoid is 1 (or its mirror image underflows towards 0) and log(v (1 - v)) evaluated from v is -inf or off by
    O(1); the header's -|x| - 2 log1p(exp(-|x|)) stays within 4 x numpy's float32 error there (the subrange of the case above, alone)."""
    a = np.concatenate([np.linspace(17, 88, 143), -np.linspace(17, 88, 143)]).astype(f32)
    v = _step(host_lib, 7, a)
    with np.errstate(divide="ignore"):
        naive = np.log(v * (f32(1) - v))
    ref = -np.abs(a.astype(f64)) - 2.0 * np.log1p(np.exp(-np.abs(a.astype(f64))))
    np32 = -np.abs(a) - f32(2) * np.log1p(np.exp(-np.abs(a)))
    assert _err(naive, ref) > 1e-3            # the inputs do exercise the cancellation
    assert _err(_step(host_lib, 8, a), ref) <= 4 * _err(np32, ref)


# ---- the whole exit transform on the TINY layout ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp_limits", [0, 1])
@pytest.mark.parametrize("sigmoid", [False, True])
def test_exit_transform_composed_from_the_header_matches_the_oracle(host_lib, sigmoid, clamp_limits):
    """Sigmoid, (x - b).mm(M_inv), [:, :ndof], limit clamp and the rev log-det of a row, composed from the header's steps as k_inv_exit composes
    them, on the TINY layout with a dense FixedLinearTransform (b != 0): x against oracle.flow_inverse_f64 with no coupling block left in the graph
    (its exit arithmetic alone), q against run_inference_f64, the log-det against minus the fp64 forward log-det at that x - within FLOW_TOL
    (relative to max(1, |x|)) and LD_TOL of tests/test_flow_inverse.py."""
    robot, hp, lay, sd = tiny_model(seed=3)
    lay = dataclasses.replace(lay, sigmoid_on_output=sigmoid)
    sd = fo.make_state_dict(lay, "panda", seed=3)
    robot, hp, lay, sd = _dense_fixed_transform((robot, hp, lay, sd), seed=4)
    lay0 = dataclasses.replace(lay, nb_nodes=0)       # the graph's exit alone: no block runs in the oracle's loop
    D, ndof = lay.dim, lay.ndof
    n = 500
    rng = np.random.default_rng(6)
    state = (rng.standard_normal((n, D)) * rng.choice([0.3, 1.0, 3.0], size=(n, 1))).astype(f32)
    ld_in = rng.standard_normal(n).astype(f32) * f32(5)
    cond = np.zeros((n, lay.dim_cond))
    M_inv = np.ascontiguousarray(sd["module_list.0.M_inv"], dtype=f32)
    b = np.ascontiguousarray(sd["module_list.0.b"], dtype=f32).reshape(-1)
    limits = O(robot).actuated_joints_limits
    lo = np.array([l[0] for l in limits], dtype=f32)
    hi = np.array([l[1] for l in limits], dtype=f32)
    log_det0 = f32(np.linalg.slogdet(M_inv.astype(f64))[1])
    x_out, q_out, ld_out = np.full((n, D), np.nan, f32), np.full((n, ndof), np.nan, f32), np.full(n, np.nan, f32)
    host_lib.flow_math_exit(state.ctypes.data, ld_in.ctypes.data, n, D, ndof, int(sigmoid), clamp_limits, M_inv.ctypes.data, b.ctypes.data, lo.ctypes.data,
                            hi.ctypes.data, log_det0, x_out.ctypes.data, q_out.ctypes.data, ld_out.ctypes.data)
    x_ref = fo.flow_inverse_f64(sd, lay0, state.astype(f64), cond)
    q_ref = fo.run_inference_f64(sd, lay0, limits, state.astype(f64), cond, bool(clamp_limits))
    # the forward log-det at x_ref with M the fp64 inverse of the M_inv the exit used: with the stored f32 M, x_ref.mm(M) + b misses sigmoid(state)
    # by 1e-7, which log(1 - v) magnifies to 2e-3 at the |state| of 10 used here - an error of that reference, not of the arithmetic under test
    sd_fwd = dict(sd, **{"module_list.0.M": np.linalg.inv(M_inv.astype(f64))})
    ld_ref = ld_in.astype(f64) - forward_with_logdet(sd_fwd, lay0, x_ref, cond)[1]
    ex, eq, el = _err(x_out, x_ref), _err(q_out, q_ref), float(np.abs(ld_out.astype(f64) - ld_ref).max())
    print(f"sigmoid {sigmoid} clamp {clamp_limits}: max |dx| rel {ex:.2e}, max |dq| rel {eq:.2e}, max |dlog_det| {el:.2e} (|log_det| up to {np.abs(ld_ref).max():.1f})")
    if clamp_limits:
        assert (q_out >= lo).all() and (q_out <= hi).all() and (q_out != x_out[:, :ndof]).any()    # the clamp did bite
    else:
        assert np.array_equal(q_out, x_out[:, :ndof])
    assert ex <= FLOW_TOL and eq <= FLOW_TOL and el <= LD_TOL, (ex, eq, el)
