"""The path optimiser, what can be checked without a GPU: the binding table of include/ikflow_amd_path_opt.h against the header and both flavours
of the library, the null-handle statuses, the build lists, and the argument asserts of the Python layer.  The argument errors that need a handle
(n_iters, smooth_weight, null pointers, P * T overflow) are in tests/test_path_opt.py: without a device there is no handle to refuse them."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from helpers import tiny_model
from ikflow_amd import _lib
from ikflow_amd import build as B
from ikflow_amd.ikflow_solver import IKFlowSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ikf_path_optimize", "ikf_path_cost", "ikf_set_path_optimize", "ikf_get_path_optimize", "ikf_path_optimize_info", "ikf_reserve_path_opt"}
OTHER_TABLES = ("SIGNATURES", "RANK_SIGNATURES", "PATH_SIGNATURES", "PATH_BATCH_SIGNATURES", "DIVERSE_SIGNATURES", "WORLD_SIGNATURES", "CLOUD_SIGNATURES",
                "SWEEP_SIGNATURES", "REFINE_SIGNATURES", "EXACT_WORLD_SIGNATURES", "TRACK_SIGNATURES", "MANIP_SIGNATURES")


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ikflow_amd_path_opt.h")).read(), flags=re.S)


def test_path_opt_header_is_bound_and_exported_by_both_flavours():
    """Every ikf_ function the header declares is in _lib.PATH_OPT_SIGNATURES (and only those), none of them is in another table, its constants are
    the binding's, both flavours export the new symbols, the ABI version is still 3, and a null handle is refused by every entry."""
    code = _code()
    declared = set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", code))
    assert declared == NAMES == set(_lib.PATH_OPT_SIGNATURES)
    for table in OTHER_TABLES:
        assert not (declared & set(getattr(_lib, table))), table
    defines = dict(re.findall(r"#define (IKF_PATH_OPT_[A-Z_]+) (\d+)", code))
    assert int(defines["IKF_PATH_OPT_MAX_ITERS"]) == _lib.IKF_PATH_OPT_MAX_ITERS == 32
    reasons = {int(v): n for n, v in defines.items() if n != "IKF_PATH_OPT_MAX_ITERS"}
    assert sorted(reasons) == sorted(_lib.PATH_OPT_REASONS) == [0, 1, 2, 3, 4]
    assert _lib.IKF_ABI_VERSION == 3
    for flavour in ("", "probes"):
        lib = _lib.load(flavour)
        assert lib.ikf_abi_version() == 3
        for name, (restype, argtypes) in _lib.PATH_OPT_SIGNATURES.items():
            assert hasattr(lib, name), f"{name} is not exported by the {flavour or 'product'} library"
            assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype   # (load() applied the table)
        calls = {
            "ikf_path_optimize": (None, None, 1, 1, None, None, None, 1, 0.0, 1, None, None, None, None),
            "ikf_path_cost": (None, None, 1, 1, None, None, None, None, None, None),
            "ikf_set_path_optimize": (None, 1, 0.0),
            "ikf_get_path_optimize": (None, None, None),
            "ikf_path_optimize_info": (None, 1, None),
            "ikf_reserve_path_opt": (None, 4, 4),
        }
        for name, args in calls.items():   # (no handle, no device)
            assert getattr(lib, name)(*args) == _lib.IKF_ERR_NULL_POINTER, name
            assert f"{name}: null model" in _lib.last_error(lib)
        n, w = C.c_int(7), C.c_float(7.0)
        assert lib.ikf_get_path_optimize(None, C.byref(n), C.byref(w)) == _lib.IKF_ERR_NULL_POINTER and (n.value, w.value) == (0, 0.0)


def test_ctypes_argument_counts_and_kinds_match_the_header():
    code = _code()
    kind = {"int64_t": C.c_int64, "int": C.c_int, "float": C.c_float}
    for name, (restype, argtypes) in _lib.PATH_OPT_SIGNATURES.items():
        params = [p.strip() for p in re.search(rf"ikf_status {name}\s*\((.*?)\);", code, re.S).group(1).split(",")]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        assert restype == C.c_int
        for p, a in zip(params, argtypes):
            if "*" in p:
                typed = {"ikf_path_options": C.POINTER(_lib.ikf_path_options), "int32_t* h_info": C.POINTER(C.c_int32), "int* n_iters_out": C.POINTER(C.c_int),
                         "float* smooth_weight_out": C.POINTER(C.c_float)}
                want = [t for key, t in typed.items() if key in p]
                assert a == (want[0] if want else C.c_void_p), (name, p, a)
            else:
                assert a == kind[p.split()[0]], (name, p, a)


def test_the_new_units_are_in_the_build_lists():
    assert "path_opt_kernels.hip" in B.SOURCES and "api_path_opt.hip" in B.SOURCES
    headers = {os.path.basename(h) for h in B.HEADERS}
    assert {"path_opt_math.h", "ikflow_amd_path_opt.h"} <= headers
    for s in B.SOURCES:
        assert os.path.exists(os.path.join(B.CSRC, s)), s
    for h in B.HEADERS:
        assert os.path.exists(h), h
    # kin_math.h is not rewritten for the optimiser: it still holds the LM step whose expressions path_opt_math.h repeats
    assert "lm_step_row" in open(os.path.join(B.CSRC, "kin_math.h")).read() and "path_opt" not in open(os.path.join(B.CSRC, "kin_math.h")).read()


def test_solver_argument_asserts_fire_before_any_device_work():
    robot, hp, lay, sd = tiny_model()
    s = IKFlowSolver(hp, robot)
    assert inspect.signature(s.set_path_optimization).parameters["smooth_weight"].default is inspect.Parameter.empty   # no default: nobody has tuned one
    assert "ratio" in s.set_path_optimization.__doc__
    assert s.last_path_optimization() is None
    for args, msg in [((-1, 0.1), "n_iters must be an int in 0 .. 32"), ((33, 0.1), "n_iters must be an int in 0 .. 32"), ((2.0, 0.1), "n_iters must be an int"),
                      ((True, 0.1), "n_iters must be an int"), ((4, -0.1), "smooth_weight must be a finite number >= 0"),
                      ((4, float("nan")), "smooth_weight must be a finite number"), ((4, float("inf")), "smooth_weight must be a finite number"),
                      ((4, "1"), "smooth_weight must be a finite number")]:
        with pytest.raises(AssertionError, match=msg):
            s.set_path_optimization(*args)
    s.set_path_optimization(4, 0.5)          # (no engine yet: remembered, pushed when the handle is created)
    assert s._path_optimization == (4, 0.5)
    s.set_path_optimization(0, 0.5)
    assert s._path_optimization == (0, 0.0)
    nd = robot.ndof
    w, p = torch.zeros(5, 7), torch.zeros(5, nd)
    bad = [
        (dict(waypoints=[[0.0] * 7], path=p, n_iters=1, smooth_weight=0.1), "must be torch.Tensors"),
        (dict(waypoints=torch.zeros(5, 6), path=p, n_iters=1, smooth_weight=0.1), r"waypoints must be of shape \[T x 7\] or \[P x T x 7\]"),
        (dict(waypoints=w, path=torch.zeros(4, nd), n_iters=1, smooth_weight=0.1), "path must be"),
        (dict(waypoints=torch.zeros(2, 5, 7), path=p, n_iters=1, smooth_weight=0.1), "path must be"),
        (dict(waypoints=w, path=p, n_iters=0, smooth_weight=0.1), "n_iters must be an int in 1 .. 32"),
        (dict(waypoints=w, path=p, n_iters=33, smooth_weight=0.1), "n_iters must be an int in 1 .. 32"),
        (dict(waypoints=w, path=p, n_iters=1, smooth_weight=-1.0), "smooth_weight must be a finite number >= 0"),
        (dict(waypoints=w, path=p, n_iters=1, smooth_weight=float("nan")), "smooth_weight must be a finite number >= 0"),
        (dict(waypoints=w, path=p, n_iters=1, smooth_weight=0.1, q_start=torch.zeros(1, nd)), "q_start must be"),
        (dict(waypoints=torch.zeros(2, 5, 7), path=torch.zeros(2, 5, nd), n_iters=1, smooth_weight=0.1, q_start=torch.zeros(nd)), "q_start must be"),
        (dict(waypoints=w, path=p, n_iters=1, smooth_weight=0.1, node_weight=-1.0), "node_weight must be >= 0"),
        (dict(waypoints=w, path=p, n_iters=1, smooth_weight=0.1, max_joint_step=-0.5), "max_joint_step must be None"),
        (dict(waypoints=w, path=p, n_iters=1, smooth_weight=0.1, pos_error_threshold=-1.0), "pos_error_threshold"),
        (dict(waypoints=w, path=p, n_iters=1, smooth_weight=0.1, reject_self_collisions=True), "needs a collision model"),
    ]
    for kw, msg in bad:
        with pytest.raises(AssertionError, match=msg):
            s.optimize_ik_path(**kw)
    if not torch.cuda.is_available():      # a call that passes every assert gets as far as the engine, which has no CPU path (and needs no weights)
        from ikflow_amd.engine import EngineError

        with pytest.raises(EngineError, match="no CPU path"):
            s.optimize_ik_path(w, p, 1, 0.1)
