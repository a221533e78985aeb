"""Path IK, what can be checked without a GPU: the argument asserts of IKFlowSolver.generate_ik_path, and the binding table of
include/ikflow_amd_path.h against both flavours of the library."""
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


def test_path_solver_argument_asserts_fire_before_any_device_work():
    robot, hp, lay, sd = tiny_model()
    s = IKFlowSolver(hp, robot)
    w = torch.zeros(4, 7)
    with pytest.raises(AssertionError, match="Model weights have not been loaded"):
        s.generate_ik_path(w, 5)
    s.load_state_dict_tensors(sd)
    dim, nd = lay.dim, robot.ndof
    bad = [
        (dict(waypoints=[[0.0] * 7], k=5), "waypoints must be a torch.Tensor"),
        (dict(waypoints=torch.zeros(4, 6), k=5), "waypoints must be of shape"),
        (dict(waypoints=torch.zeros(7), k=5), "waypoints must be of shape"),
        (dict(waypoints=w, k=0), "k must be an int in 1 .. 256"),
        (dict(waypoints=w, k=257), "k must be an int in 1 .. 256"),
        (dict(waypoints=w, k=5.0), "k must be an int in 1 .. 256"),
        (dict(waypoints=w, k=5, latent_scale=1), None),
        (dict(waypoints=w, k=5, latent_distribution=None), None),
        (dict(waypoints=w, k=5, latent=np.zeros((5, dim))), "latent must either be"),
        (dict(waypoints=w, k=5, latent=torch.zeros(20, dim)), rf"latent must be \[5 x {dim}\]"),
        (dict(waypoints=w, k=5, latent=torch.zeros(5, dim), shared_latent=False), rf"latent must be \[20 x {dim}\]"),
        (dict(waypoints=w, k=5, q_start=torch.zeros(1, nd)), rf"q_start must be \[{nd}\]"),
        (dict(waypoints=w, k=5, q_start=[0.0] * nd), rf"q_start must be \[{nd}\]"),
        (dict(waypoints=w, k=5, reject_self_collisions=True), "needs a collision model"),
        (dict(waypoints=w, k=5, pos_error_threshold=-1.0), "pos_error_threshold"),
        (dict(waypoints=w, k=5, rot_error_threshold=-0.1), "rot_error_threshold"),
        (dict(waypoints=w, k=5, node_weight=-1.0), "node_weight must be >= 0"),
        (dict(waypoints=w, k=5, max_joint_step=-0.5), "max_joint_step must be None"),
        (dict(waypoints=w, k=5, refine_steps=-1), "refine_steps must be an int >= 0"),
        (dict(waypoints=w, k=5, refine_steps=1.0), "refine_steps must be an int >= 0"),
        (dict(waypoints=torch.empty(2 ** 23, 7), k=256), "at most 2"),   # (never touched: the assert fires first)
    ]
    for kw, msg in bad:
        with pytest.raises(AssertionError, match=msg):
            s.generate_ik_path(**kw)
    assert not robot.has_collision_model   # (so reject_self_collisions=None means "off" here)
    if not torch.cuda.is_available():      # a call that passes every assert gets as far as the engine, which has no CPU path
        from ikflow_amd.engine import EngineError

        with pytest.raises(EngineError, match="no CPU path"):
            s.generate_ik_path(w, 5)


def test_path_header_is_bound_and_exported_by_both_flavours():
    """Every ikf_ name that include/ikflow_amd_path.h declares is in _lib.PATH_SIGNATURES (and only those), none of them is in the boundary, debug
    or ranking tables, and both flavours of the library export them; the options struct of the binding has the header's fields in its order and
    size; the ABI version is still 3."""
    text = open(os.path.join(ROOT, "include", "ikflow_amd_path.h")).read()
    declared = set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", text))
    assert declared == {"ikf_path_search", "ikf_generate_path", "ikf_reserve_path"}
    assert declared == set(_lib.PATH_SIGNATURES) and not (declared & set(_lib.SIGNATURES)) and not (declared & set(_lib.RANK_SIGNATURES))
    body = re.search(r"typedef struct ikf_path_options \{(.*?)\} ikf_path_options;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [decl.strip().split(None, 1) for decl in body.split(";") if decl.strip()]
    fields = [n.strip() for _, names in decls for n in names.split(",")]
    assert fields == [f[0] for f in _lib.ikf_path_options._fields_]
    ctype = {"float": C.c_float, "int32_t": C.c_int32}
    assert [ctype[t] for t, names in decls for _ in names.split(",")] == [f[1] for f in _lib.ikf_path_options._fields_]
    assert C.sizeof(_lib.ikf_path_options) == 4 * len(fields)
    assert int(re.search(r"#define IKF_PATH_MAX_K (\d+)", text).group(1)) == _lib.IKF_PATH_MAX_K == 256
    assert _lib.IKF_ABI_VERSION == 3
    for flavour in ("", "probes"):
        lib = _lib.load(flavour)
        assert lib.ikf_abi_version() == 3
        for name in declared:
            assert hasattr(lib, name), f"{name} is not exported by the {flavour or 'product'} library"
        assert lib.ikf_reserve_path(None, 4, 4) == _lib.IKF_ERR_NULL_POINTER   # (no handle, no device)
        assert lib.ikf_path_search(None, None, 0, 1, None, None, None, None, None, None, None, None, None) == _lib.IKF_ERR_NULL_POINTER
