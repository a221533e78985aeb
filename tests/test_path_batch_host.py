"""Path IK for P paths per call, what can be checked without a GPU: the binding table of include/ikflow_amd_path_batch.h against the header and
both flavours of the library, and the argument asserts of IKFlowSolver.generate_ik_paths."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from helpers import tiny_model
from ikflow_amd import _lib
from ikflow_amd.ikflow_solver import IKFlowSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ikf_path_search_batch", "ikf_generate_path_batch", "ikf_reserve_path_batch"}
OTHER_TABLES = ("SIGNATURES", "RANK_SIGNATURES", "PATH_SIGNATURES", "DIVERSE_SIGNATURES", "WORLD_SIGNATURES", "CLOUD_SIGNATURES", "SWEEP_SIGNATURES",
                "REFINE_SIGNATURES", "EXACT_WORLD_SIGNATURES", "TRACK_SIGNATURES", "MANIP_SIGNATURES")


def _code(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def test_path_batch_header_is_bound_and_exported_by_both_flavours():
    """Every ikf_ function that include/ikflow_amd_path_batch.h declares is in _lib.PATH_BATCH_SIGNATURES (and only those), none of them is in
    another table, the path header still declares its own three, both flavours export the new ones, the ABI version is still 3, and the header
    says what is not covered."""
    code = _code("ikflow_amd_path_batch.h")
    declared = set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", code))
    assert declared == NAMES == set(_lib.PATH_BATCH_SIGNATURES)
    for table in OTHER_TABLES:
        assert not (declared & set(getattr(_lib, table))), table
    assert set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", _code("ikflow_amd_path.h"))) == set(_lib.PATH_SIGNATURES)
    assert not re.findall(r"#define (IKF_[A-Z_]+) ", code.replace("#define IKFLOW_AMD_PATH_BATCH_H", ""))   # (IKF_PATH_MAX_K is the path header's)
    text = open(os.path.join(ROOT, "include", "ikflow_amd_path_batch.h")).read()
    not_covered = text[text.index("Not covered"):]
    assert "world track" in not_covered and "ikf_set_world_track" in not_covered and "IKF_ERR_BAD_ARGUMENT" in not_covered
    assert "per-path lengths" in not_covered and "per-path k" in not_covered and "per-path options" in not_covered
    assert _lib.IKF_ABI_VERSION == 3
    for flavour in ("", "probes"):
        lib = _lib.load(flavour)
        assert lib.ikf_abi_version() == 3
        for name, (restype, argtypes) in _lib.PATH_BATCH_SIGNATURES.items():
            assert hasattr(lib, name), f"{name} is not exported by the {flavour or 'product'} library"
            assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype   # (load() applied the table)
        assert lib.ikf_reserve_path_batch(None, 4, 4, 4) == _lib.IKF_ERR_NULL_POINTER   # (no handle, no device)
        assert "ikf_reserve_path_batch: null model" in _lib.last_error(lib)
        assert lib.ikf_path_search_batch(None, None, 0, 0, 1, None, None, None, None, None, None, None, None, None) == _lib.IKF_ERR_NULL_POINTER
        assert "ikf_path_search_batch: null model" in _lib.last_error(lib)
        assert lib.ikf_generate_path_batch(None, None, 0, 0, 1, None, 1, 1, None, None, None, None, None, None, None, None) == _lib.IKF_ERR_NULL_POINTER


def test_ctypes_argument_counts_and_kinds_match_the_header():
    """Parameter by parameter: a pointer in the header is a pointer in the table, int64_t is c_int64, int is c_int; the batch entries are the single
    path's with `int64_t P` in front of T (and max_paths in front of max_waypoints)."""
    code = _code("ikflow_amd_path_batch.h")
    kind = {"int64_t": C.c_int64, "int": C.c_int}
    for name, (restype, argtypes) in _lib.PATH_BATCH_SIGNATURES.items():
        params = [p.strip() for p in re.search(rf"ikf_status {name}\s*\((.*?)\);", code, re.S).group(1).split(",")]
        assert len(params) == len(argtypes), (name, len(params), len(argtypes))
        assert restype == C.c_int
        for p, a in zip(params, argtypes):
            if "*" in p:
                assert a in (C.c_void_p, C.POINTER(_lib.ikf_path_options)), (name, p, a)
                assert (a == C.POINTER(_lib.ikf_path_options)) == ("ikf_path_options" in p), (name, p)
            else:
                assert a == kind[p.split()[0]], (name, p, a)
    single = {"ikf_path_search_batch": "ikf_path_search", "ikf_generate_path_batch": "ikf_generate_path", "ikf_reserve_path_batch": "ikf_reserve_path"}
    for name, base in single.items():
        want = list(_lib.PATH_SIGNATURES[base][1])
        at = 1 if base == "ikf_reserve_path" else 2
        want.insert(at, C.c_int64)
        assert _lib.PATH_BATCH_SIGNATURES[name][1] == want, name


def test_paths_solver_argument_asserts_fire_before_any_device_work():
    robot, hp, lay, sd = tiny_model()
    s = IKFlowSolver(hp, robot)
    w = torch.zeros(3, 4, 7)
    with pytest.raises(AssertionError, match="Model weights have not been loaded"):
        s.generate_ik_paths(w, 5)
    s.load_state_dict_tensors(sd)
    dim, nd = lay.dim, robot.ndof
    bad = [
        (dict(waypoints=[[[0.0] * 7]], k=5), "waypoints must be a torch.Tensor"),
        (dict(waypoints=torch.zeros(4, 7), k=5), r"waypoints must be of shape \[P x T x 7\]"),
        (dict(waypoints=torch.zeros(3, 4, 6), k=5), r"waypoints must be of shape \[P x T x 7\]"),
        (dict(waypoints=w, k=0), "k must be an int in 1 .. 256"),
        (dict(waypoints=w, k=257), "k must be an int in 1 .. 256"),
        (dict(waypoints=w, k=5.0), "k must be an int in 1 .. 256"),
        (dict(waypoints=w, k=5, latent_scale=1), None),
        (dict(waypoints=w, k=5, latent=np.zeros((5, dim))), "latent must either be"),
        (dict(waypoints=w, k=5, latent=torch.zeros(20, dim)), rf"latent must be \[5 x {dim}\]"),
        (dict(waypoints=w, k=5, latent=torch.zeros(5, dim), shared_latent=False), rf"latent must be \[60 x {dim}\]"),
        (dict(waypoints=w, k=5, q_start=torch.zeros(nd)), rf"q_start must be \[3 x {nd}\]"),
        (dict(waypoints=w, k=5, q_start=torch.zeros(4, nd)), rf"q_start must be \[3 x {nd}\]"),
        (dict(waypoints=w, k=5, q_start=[[0.0] * nd] * 3), rf"q_start must be \[3 x {nd}\]"),
        (dict(waypoints=w, k=5, reject_self_collisions=True), "needs a collision model"),
        (dict(waypoints=w, k=5, pos_error_threshold=-1.0), "pos_error_threshold"),
        (dict(waypoints=w, k=5, rot_error_threshold=-0.1), "rot_error_threshold"),
        (dict(waypoints=w, k=5, node_weight=-1.0), "node_weight must be >= 0"),
        (dict(waypoints=w, k=5, max_joint_step=-0.5), "max_joint_step must be None"),
        (dict(waypoints=w, k=5, refine_steps=-1), "refine_steps must be an int >= 0"),
        (dict(waypoints=w, k=5, refine_steps=1.0), "refine_steps must be an int >= 0"),
        (dict(waypoints=torch.empty(2 ** 12, 2 ** 11, 7), k=256), "at most 2"),   # (never touched: the assert fires first)
    ]
    for kw, msg in bad:
        with pytest.raises(AssertionError, match=msg):
            s.generate_ik_paths(**kw)
    if not torch.cuda.is_available():      # a call that passes every assert gets as far as the engine, which has no CPU path
        from ikflow_amd.engine import EngineError

        with pytest.raises(EngineError, match="no CPU path"):
            s.generate_ik_paths(w, 5)
