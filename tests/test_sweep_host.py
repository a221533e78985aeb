"""Swept collision checks, what can be checked without a GPU: the binding table of include/ikflow_amd_sweep.h against both flavours of the library,
the null-handle statuses, and the asserts of IKFlowSolver.set_path_sweep / path_collides."""
import os
import re

import pytest
import torch

from helpers import tiny_model
from ikflow_amd import _lib
from ikflow_amd.ikflow_solver import IKFlowSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_header_is_bound_and_exported_by_both_flavours():
    """Every ikf_ function that include/ikflow_amd_sweep.h declares is in _lib.SWEEP_SIGNATURES (and only those), none of them is in the other
    tables, and both flavours of the library export them; the #define matches; the ABI version is still 3."""
    text = open(os.path.join(ROOT, "include", "ikflow_amd_sweep.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", code))
    assert declared == {"ikf_set_path_sweep", "ikf_get_path_sweep", "ikf_sweep_edges"}
    assert declared == set(_lib.SWEEP_SIGNATURES)
    for table in (_lib.SIGNATURES, _lib.RANK_SIGNATURES, _lib.PATH_SIGNATURES, _lib.DIVERSE_SIGNATURES, _lib.WORLD_SIGNATURES):
        assert not (declared & set(table))
    assert re.findall(r"#define (IKF_[A-Z_]+) ", code) == ["IKF_SWEEP_MAX_SAMPLES"]
    assert int(re.search(r"#define IKF_SWEEP_MAX_SAMPLES (\d+)", code).group(1)) == _lib.IKF_SWEEP_MAX_SAMPLES == 16
    assert _lib.IKF_ABI_VERSION == 3
    for flavour in ("", "probes"):
        lib = _lib.load(flavour)
        assert lib.ikf_abi_version() == 3
        for name, (restype, argtypes) in _lib.SWEEP_SIGNATURES.items():
            assert hasattr(lib, name), f"{name} is not exported by the {flavour or 'product'} library"
            assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype   # (load() applied the table)
        assert lib.ikf_set_path_sweep(None, 4) == _lib.IKF_ERR_NULL_POINTER   # (no handle, no device)
        assert "ikf_set_path_sweep: null model" in _lib.last_error(lib)
        assert lib.ikf_get_path_sweep(None) == 0
        assert lib.ikf_sweep_edges(None, None, None, 0, 1, 0, 0.0, None, None, None) == _lib.IKF_ERR_NULL_POINTER
        assert "ikf_sweep_edges: null model" in _lib.last_error(lib)


def test_the_extension_headers_the_sweep_leaves_alone_declare_what_they_declared():
    """The sweep lives in its own header: ikflow_amd_path.h and ikflow_amd_world.h keep their functions, and the world header points here."""
    names = lambda h: set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)))
    assert names("ikflow_amd_path.h") == set(_lib.PATH_SIGNATURES) and names("ikflow_amd_world.h") == set(_lib.WORLD_SIGNATURES)
    assert "ikflow_amd_sweep.h" in open(os.path.join(ROOT, "include", "ikflow_amd_world.h")).read()


def test_solver_sweep_asserts_fire_before_any_device_work():
    robot, hp, lay, sd = tiny_model()
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    for bad in (-1, 17, 1.0, None, True):
        with pytest.raises(AssertionError, match="n_samples must be an int in 0 .. 16"):
            s.set_path_sweep(bad)
    s.set_path_sweep(4)      # no engine yet: remembered for the engine of the first GPU call
    assert s._path_sweep == 4
    s.set_path_sweep(0)
    assert s._path_sweep == 0
    path = torch.zeros(5, robot.ndof)
    with pytest.raises(AssertionError, match="path must be"):
        s.path_collides(torch.zeros(5, robot.ndof + 1), 2)
    for bad in (0, 17, 2.0):
        with pytest.raises(AssertionError, match="n_samples must be an int in 1 .. 16"):
            s.path_collides(path, bad)
    assert not robot.has_collision_model
    with pytest.raises(AssertionError, match="path_collides needs a collision model"):
        s.path_collides(path, 2)
