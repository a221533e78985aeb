"""Exact IK that obeys the world, what can be checked without a GPU: the binding table of include/ikflow_amd_exact_world.h against both flavours
of the library, the null-handle statuses, the pointers in the neighbouring headers, and the state IKFlowSolver.set_exact_collision remembers.  What
needs a handle needs a device: tests/test_exact_world.py."""
import ctypes as C
import os
import re

import pytest

from helpers import tiny_model
from ikflow_amd import _lib
from ikflow_amd.ikflow_solver import IKFlowSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ikf_set_exact_collision", "ikf_get_exact_collision", "ikf_exact_collision_rejected"}


def _read(header):
    return open(os.path.join(ROOT, "include", header)).read()


def _declared(header):
    return set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", _read(header), flags=re.S)))


def test_exact_world_header_is_bound_and_exported_by_both_flavours():
    assert _declared("ikflow_amd_exact_world.h") == NAMES == set(_lib.EXACT_WORLD_SIGNATURES)
    for table in (_lib.SIGNATURES, _lib.RANK_SIGNATURES, _lib.PATH_SIGNATURES, _lib.DIVERSE_SIGNATURES, _lib.WORLD_SIGNATURES, _lib.CLOUD_SIGNATURES,
                  _lib.SWEEP_SIGNATURES, _lib.REFINE_SIGNATURES):
        assert not (NAMES & set(table))
    assert _lib.IKF_ABI_VERSION == 3
    for flavour in ("", "probes"):
        lib = _lib.load(flavour)
        assert lib.ikf_abi_version() == 3
        for name, (restype, argtypes) in _lib.EXACT_WORLD_SIGNATURES.items():
            assert hasattr(lib, name), f"{name} is not exported by the {flavour or 'product'} library"
            assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype   # (load() applied the table)
        assert lib.ikf_set_exact_collision(None, 1, 0, 0.0) == _lib.IKF_ERR_NULL_POINTER   # (no handle, no device)
        assert "ikf_set_exact_collision: null model" in _lib.last_error(lib)
        on, rs, mc = C.c_int(7), C.c_int(7), C.c_float(7.0)
        assert lib.ikf_get_exact_collision(None, C.byref(on), C.byref(rs), C.byref(mc)) == _lib.IKF_ERR_NULL_POINTER
        assert (on.value, rs.value, mc.value) == (0, 0, 0.0)
        assert lib.ikf_get_exact_collision(None, None, None, None) == _lib.IKF_ERR_NULL_POINTER
        rows = (C.c_int64 * _lib.IKF_MAX_ROUNDS)(*([5] * _lib.IKF_MAX_ROUNDS))
        assert lib.ikf_exact_collision_rejected(None, rows) == _lib.IKF_ERR_NULL_POINTER and list(rows) == [5] * _lib.IKF_MAX_ROUNDS


def test_the_neighbouring_headers_keep_their_functions_and_point_here():
    for header, table in (("ikflow_amd_world.h", _lib.WORLD_SIGNATURES), ("ikflow_amd_cloud.h", _lib.CLOUD_SIGNATURES),
                          ("ikflow_amd_sweep.h", _lib.SWEEP_SIGNATURES), ("ikflow_amd_refine.h", _lib.REFINE_SIGNATURES)):
        assert _declared(header) == set(table), header
    assert NAMES.isdisjoint(_declared("ikflow_amd.h"))
    for header in ("ikflow_amd_world.h", "ikflow_amd_cloud.h", "ikflow_amd.h"):
        assert "ikflow_amd_exact_world.h" in _read(header), header


def test_solver_remembers_the_rule_and_refuses_bad_arguments_before_any_device_work():
    robot, hp, lay, sd = tiny_model()
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    assert s._exact_collision == (False, False, 0.0)
    for bad in (float("nan"), float("inf"), None, "1", True):
        with pytest.raises(AssertionError, match="min_clearance must be a finite number"):
            s.set_exact_collision(min_clearance=bad)
    for bad in (1, None, "yes"):
        with pytest.raises(AssertionError, match="reject_self_collisions must be a bool"):
            s.set_exact_collision(reject_self_collisions=bad)
        with pytest.raises(AssertionError, match="enabled must be a bool"):
            s.set_exact_collision(enabled=bad)
    assert s._exact_collision == (False, False, 0.0)     # a refused call leaves the state alone
    s.set_exact_collision()                               # no engine yet: remembered for the engine of the first GPU call
    assert s._exact_collision == (True, False, 0.0) and s._engine is None
    if not robot.has_collision_model:
        with pytest.raises(AssertionError, match="needs a collision model"):
            s.set_exact_collision(reject_self_collisions=True)
        assert s._exact_collision == (True, False, 0.0)
    s.set_exact_collision(min_clearance=0.02)
    assert s._exact_collision == (True, False, 0.02)
    s.set_exact_collision(reject_self_collisions=False, min_clearance=5.0, enabled=False)   # off: the rest is dropped, as the handle drops it
    assert s._exact_collision == (False, False, 0.0)
