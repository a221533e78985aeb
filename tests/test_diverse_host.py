"""Diverse-of-K IK, what can be checked without a GPU: the argument asserts of IKFlowSolver.generate_diverse_ik_solutions, and the binding table of
include/ikflow_amd_diverse.h against both flavours of the library."""
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


def test_diverse_solver_argument_asserts_fire_before_any_device_work():
    robot, hp, lay, sd = tiny_model()
    s = IKFlowSolver(hp, robot)
    y = torch.zeros(4, 7)
    with pytest.raises(AssertionError, match="Model weights have not been loaded"):
        s.generate_diverse_ik_solutions(y, 5, 2)
    s.load_state_dict_tensors(sd)
    dim, nd = lay.dim, robot.ndof
    neg = torch.ones(nd)
    neg[1] = -0.5
    bad = [
        (dict(y=[[0.0] * 7], k=5, n_keep=2), "y must be a torch.Tensor"),
        (dict(y=torch.zeros(4, 6), k=5, n_keep=2), "y must be of shape"),
        (dict(y=y, k=0, n_keep=1), "k must be an int in 1 .. 1024"),
        (dict(y=y, k=1025, n_keep=1), "k must be an int in 1 .. 1024"),
        (dict(y=y, k=5.0, n_keep=1), "k must be an int in 1 .. 1024"),
        (dict(y=y, k=5, n_keep=0), "n_keep must be in 1 .. min"),
        (dict(y=y, k=5, n_keep=6), "n_keep must be in 1 .. min"),
        (dict(y=y, k=64, n_keep=17), "n_keep must be in 1 .. min"),
        (dict(y=y, k=5, n_keep=2.0), "n_keep must be in 1 .. min"),
        (dict(y=y, k=5, n_keep=2, min_separation=-0.1), "min_separation must be >= 0"),
        (dict(y=y, k=5, n_keep=2, min_separation=float("nan")), "min_separation must be >= 0"),
        (dict(y=y, k=5, n_keep=2, min_separation=None), "min_separation must be >= 0"),
        (dict(y=y, k=5, n_keep=2, joint_weights=[1.0] * nd), rf"joint_weights must be \[{nd}\]"),
        (dict(y=y, k=5, n_keep=2, joint_weights=torch.ones(nd + 1)), rf"joint_weights must be \[{nd}\]"),
        (dict(y=y, k=5, n_keep=2, joint_weights=neg), "joint_weights must all be finite and >= 0"),
        (dict(y=y, k=5, n_keep=2, joint_weights=torch.full((nd,), float("inf"))), "joint_weights must all be finite and >= 0"),
        (dict(y=y, k=5, n_keep=2, joint_weights=torch.full((nd,), float("nan"))), "joint_weights must all be finite and >= 0"),
        (dict(y=y, k=5, n_keep=2, latent_scale=1), None),
        (dict(y=y, k=5, n_keep=2, latent_distribution=None), None),
        (dict(y=y, k=5, n_keep=2, latent=np.zeros((20, dim))), "latent must either be"),
        (dict(y=y, k=5, n_keep=2, latent=torch.zeros(5, dim)), rf"latent must be \[20 x {dim}\]"),
        (dict(y=y, k=5, n_keep=2, reject_self_collisions=True), "needs a collision model"),
        (dict(y=y, k=5, n_keep=2, pos_error_threshold=-1.0), "pos_error_threshold"),
        (dict(y=y, k=5, n_keep=2, rot_error_threshold=-0.1), "rot_error_threshold"),
        (dict(y=torch.empty(2 ** 21, 7), k=1024, n_keep=2), "at most 2"),   # (never touched: the assert fires first)
    ]
    for kw, msg in bad:
        with pytest.raises(AssertionError, match=msg):
            s.generate_diverse_ik_solutions(**kw)
    assert not robot.has_collision_model   # (so reject_self_collisions=None means "off" here)
    if not torch.cuda.is_available():      # a call that passes every assert gets as far as the engine, which has no CPU path
        from ikflow_amd.engine import EngineError

        with pytest.raises(EngineError, match="no CPU path"):
            s.generate_diverse_ik_solutions(y, 5, 2, min_separation=0.1, joint_weights=torch.ones(nd))


def test_diverse_header_is_bound_and_exported_by_both_flavours():
    """Every ikf_ name that include/ikflow_amd_diverse.h declares is in _lib.DIVERSE_SIGNATURES (and only those), none of them is in the boundary,
    debug, ranking or path tables, and both flavours of the library export them; the options struct of the binding has the header's fields in
    its order and size; both #defines match; the ABI version is still 3."""
    text = open(os.path.join(ROOT, "include", "ikflow_amd_diverse.h")).read()
    declared = set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", text))
    assert declared == {"ikf_diverse_select", "ikf_generate_diverse", "ikf_reserve_diverse"}
    assert declared == set(_lib.DIVERSE_SIGNATURES)
    for table in (_lib.SIGNATURES, _lib.RANK_SIGNATURES, _lib.PATH_SIGNATURES):
        assert not (declared & set(table))
    body = re.search(r"typedef struct ikf_diverse_options \{(.*?)\} ikf_diverse_options;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [decl.strip().split(None, 1) for decl in body.split(";") if decl.strip()]
    fields = [n.strip() for _, names in decls for n in names.split(",")]
    assert fields == [f[0] for f in _lib.ikf_diverse_options._fields_]
    ctype = {"float": C.c_float, "int32_t": C.c_int32}
    assert [ctype[t] for t, names in decls for _ in names.split(",")] == [f[1] for f in _lib.ikf_diverse_options._fields_]
    assert C.sizeof(_lib.ikf_diverse_options) == 4 * len(fields) == 32
    assert int(re.search(r"#define IKF_DIVERSE_MAX_K (\d+)", text).group(1)) == _lib.IKF_DIVERSE_MAX_K == 1024
    assert int(re.search(r"#define IKF_DIVERSE_MAX_KEEP (\d+)", text).group(1)) == _lib.IKF_DIVERSE_MAX_KEEP == 16
    assert re.findall(r"#define (IKF_[A-Z_]+) ", text) == ["IKF_DIVERSE_MAX_K", "IKF_DIVERSE_MAX_KEEP"]
    assert _lib.IKF_ABI_VERSION == 3
    for flavour in ("", "probes"):
        lib = _lib.load(flavour)
        assert lib.ikf_abi_version() == 3
        for name, (restype, argtypes) in _lib.DIVERSE_SIGNATURES.items():
            assert hasattr(lib, name), f"{name} is not exported by the {flavour or 'product'} library"
            assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype   # (load() applied the table)
        assert lib.ikf_reserve_diverse(None, 4, 4) == _lib.IKF_ERR_NULL_POINTER   # (no handle, no device)
        assert lib.ikf_diverse_select(None, *[None, 0, 1] + [None] * 11) == _lib.IKF_ERR_NULL_POINTER
        assert lib.ikf_generate_diverse(None, *[None, 0, 1, None, 1] + [None] * 10) == _lib.IKF_ERR_NULL_POINTER
