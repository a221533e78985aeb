"""Refined candidates, what can be checked without a GPU: the binding table of include/ikflow_amd_refine.h against both flavours of the library,
the null-handle statuses, and the asserts of IKFlowSolver.set_candidate_refine.  The validation messages of ikf_set_candidate_refine itself need
a handle, and a handle needs a device: they are in tests/test_refine.py (test_status_codes_and_messages)."""
import ctypes as C
import os
import re

import pytest

from helpers import tiny_model
from ikflow_amd import _lib
from ikflow_amd.ikflow_solver import IKFlowSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refine_header_is_bound_and_exported_by_both_flavours():
    """Every ikf_ function that include/ikflow_amd_refine.h declares is in _lib.REFINE_SIGNATURES (and only those), none of them is in the other
    tables, and both flavours of the library export them; the #define matches; the ABI version is still 3."""
    text = open(os.path.join(ROOT, "include", "ikflow_amd_refine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", code))
    assert declared == {"ikf_set_candidate_refine", "ikf_get_candidate_refine", "ikf_refine_candidates"}
    assert declared == set(_lib.REFINE_SIGNATURES)
    for table in (_lib.SIGNATURES, _lib.RANK_SIGNATURES, _lib.PATH_SIGNATURES, _lib.DIVERSE_SIGNATURES, _lib.WORLD_SIGNATURES, _lib.SWEEP_SIGNATURES):
        assert not (declared & set(table))
    assert re.findall(r"#define (IKF_[A-Z_]+) ", code) == ["IKF_REFINE_MAX_STEPS"]
    assert int(re.search(r"#define IKF_REFINE_MAX_STEPS (\d+)", code).group(1)) == _lib.IKF_REFINE_MAX_STEPS == 16
    assert _lib.IKF_ABI_VERSION == 3
    for flavour in ("", "probes"):
        lib = _lib.load(flavour)
        assert lib.ikf_abi_version() == 3
        for name, (restype, argtypes) in _lib.REFINE_SIGNATURES.items():
            assert hasattr(lib, name), f"{name} is not exported by the {flavour or 'product'} library"
            assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype   # (load() applied the table)
        assert lib.ikf_set_candidate_refine(None, 4, 1e-3, 0.1) == _lib.IKF_ERR_NULL_POINTER   # (no handle, no device)
        assert "ikf_set_candidate_refine: null model" in _lib.last_error(lib)
        pos, rot = C.c_float(7.0), C.c_float(7.0)
        assert lib.ikf_get_candidate_refine(None, C.byref(pos), C.byref(rot)) == 0 and pos.value == 0.0 and rot.value == 0.0
        assert lib.ikf_get_candidate_refine(None, None, None) == 0
        assert lib.ikf_refine_candidates(None, None, 0, 1, None, 4, 0.0, 0.0, None, None, None, None) == _lib.IKF_ERR_NULL_POINTER
        assert "ikf_refine_candidates: null model" in _lib.last_error(lib)


def test_the_extension_headers_the_refinement_leaves_alone_declare_what_they_declared():
    """The refinement lives in its own header: the rank, path, diverse, world and sweep headers keep their functions, and the three candidate
    families' headers point here."""
    read = lambda h: open(os.path.join(ROOT, "include", h)).read()
    names = lambda h: set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", read(h), flags=re.S)))
    for header, table in (("ikflow_amd_rank.h", _lib.RANK_SIGNATURES), ("ikflow_amd_path.h", _lib.PATH_SIGNATURES),
                          ("ikflow_amd_diverse.h", _lib.DIVERSE_SIGNATURES), ("ikflow_amd_world.h", _lib.WORLD_SIGNATURES),
                          ("ikflow_amd_sweep.h", _lib.SWEEP_SIGNATURES)):
        assert names(header) == set(table), header
    for header in ("ikflow_amd_rank.h", "ikflow_amd_path.h", "ikflow_amd_diverse.h"):
        assert "ikflow_amd_refine.h" in read(header), header


def test_solver_refine_asserts_fire_before_any_device_work():
    robot, hp, lay, sd = tiny_model()
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    assert s._candidate_refine == (0, 0.0, 0.0)
    for bad in (-1, 17, 1.0, None, True):
        with pytest.raises(AssertionError, match="n_steps must be an int in 0 .. 16"):
            s.set_candidate_refine(bad)
    for bad in (-1e-9, float("nan"), float("inf"), None, "1", True):
        with pytest.raises(AssertionError, match="pos_tol must be a finite number >= 0"):
            s.set_candidate_refine(4, pos_tol=bad)
        with pytest.raises(AssertionError, match="rot_tol must be a finite number >= 0"):
            s.set_candidate_refine(4, rot_tol=bad)
    assert s._candidate_refine == (0, 0.0, 0.0)        # a refused call leaves the state alone
    s.set_candidate_refine(4)                          # no engine yet: remembered for the engine of the first GPU call
    assert s._candidate_refine == (4, 1e-3, 0.1)       # generate_exact_ik_solutions' thresholds
    s.set_candidate_refine(16, 0, 0.0)
    assert s._candidate_refine == (16, 0.0, 0.0)
    with pytest.raises(AssertionError):
        s.set_candidate_refine(17)
    assert s._candidate_refine == (16, 0.0, 0.0)
    s.set_candidate_refine(0, 5.0, 5.0)                # off: the tolerances are dropped, as the handle drops them
    assert s._candidate_refine == (0, 0.0, 0.0)
