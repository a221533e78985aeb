"""Singularity rule, what can be checked without a GPU: the binding table of include/ikflow_amd_manip.h against both flavours of the library, that
the header is plain C, what the entry points answer without a handle, that the units are in the build, and the asserts of
IKFlowSolver.set_min_manipulability.  (A handle needs a device: refusals on a live handle and the getter's round trip are in tests/test_manip.py.)"""
import os
import re
import subprocess

import pytest

from helpers import tiny_model
from ikflow_amd import _lib
from ikflow_amd import build as B
from ikflow_amd.ikflow_solver import IKFlowSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ("SIGNATURES", "RANK_SIGNATURES", "PATH_SIGNATURES", "DIVERSE_SIGNATURES", "WORLD_SIGNATURES", "CLOUD_SIGNATURES", "SWEEP_SIGNATURES",
          "REFINE_SIGNATURES", "EXACT_WORLD_SIGNATURES", "TRACK_SIGNATURES")


def _declared(header):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", code)), code


def test_manip_header_is_bound_and_exported_by_both_flavours():
    """Every ikf_ function that include/ikflow_amd_manip.h declares is in _lib.MANIP_SIGNATURES (and only those), none of them is in another
    table, and both flavours of the library export them; the #defines match the binding; the ABI version is still 3; without a handle every entry
    answers IKF_ERR_NULL_POINTER and touches nothing."""
    declared, code = _declared("ikflow_amd_manip.h")
    assert declared == {"ikf_set_min_manipulability", "ikf_min_manipulability", "ikf_manipulability"}
    assert declared == set(_lib.MANIP_SIGNATURES)
    for table in TABLES:
        assert not (declared & set(getattr(_lib, table))), table
    assert re.findall(r"#define (IKF_[A-Z_]+) (\d+)", code) == [("IKF_MANIP_FULL", "0"), ("IKF_MANIP_LINEAR", "1"), ("IKF_MANIP_ANGULAR", "2")]
    assert (_lib.IKF_MANIP_FULL, _lib.IKF_MANIP_LINEAR, _lib.IKF_MANIP_ANGULAR) == (0, 1, 2)
    assert _lib.MANIP_PARTS == {"full": 0, "linear": 1, "angular": 2}
    assert _lib.IKF_ABI_VERSION == 3
    for flavour in ("", "probes"):
        lib = _lib.load(flavour)
        assert lib.ikf_abi_version() == 3
        for name, (restype, argtypes) in _lib.MANIP_SIGNATURES.items():
            assert hasattr(lib, name), f"{name} is not exported by the {flavour or 'product'} library"
            assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype   # (load() applied the table)
        assert lib.ikf_set_min_manipulability(None, 0, 0.1) == _lib.IKF_ERR_NULL_POINTER
        assert "null model" in _lib.last_error(lib)
        assert lib.ikf_min_manipulability(None, None, None) == _lib.IKF_ERR_NULL_POINTER
        assert lib.ikf_manipulability(None, None, 0, 0, 0.0, None, None, None) == _lib.IKF_ERR_NULL_POINTER


def test_manip_header_is_plain_c(tmp_path):
    """The header compiles as C11 (and as C++17) on its own, with every warning an error."""
    for compiler, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")):
        src = tmp_path / f"client.{ext}"
        src.write_text('#include "ikflow_amd_manip.h"\nint main(void) { return IKF_MANIP_FULL == 0 && IKF_MANIP_ANGULAR == 2 && '
                       'ikf_min_manipulability(0, 0, 0) != IKF_OK ? 0 : 1; }\n')
        r = subprocess.run([compiler, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_the_new_units_are_in_the_build():
    assert "manip_kernels.hip" in B.SOURCES and "api_manip.hip" in B.SOURCES
    names = {os.path.basename(h) for h in B.HEADERS}
    assert {"manip_math.h", "ikflow_amd_manip.h"} <= names
    assert all(os.path.exists(h) for h in B.HEADERS)


def test_solver_set_min_manipulability_asserts_fire_before_any_device_work():
    robot, hp, lay, sd = tiny_model()
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    for bad in (-0.01, float("nan"), float("inf"), -float("inf"), None, "0.1", True):
        with pytest.raises(AssertionError, match="min_manipulability must be a finite number >= 0"):
            s.set_min_manipulability(bad)
    for bad in ("Full", "position", 0, None):
        with pytest.raises(AssertionError, match="part must be"):
            s.set_min_manipulability(0.05, bad)
    assert s._min_manipulability == (0.0, "full")   # (a refused call leaves the state as it was)
    if s._engine is None:   # (no engine yet: remembered for the engine of the first GPU call, on any machine)
        s.set_min_manipulability(0.05, "linear")
        assert s._min_manipulability == (0.05, "linear")
        s.set_min_manipulability(0)
        assert s._min_manipulability == (0.0, "full")
