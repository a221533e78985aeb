"""World point cloud, what can be checked without a GPU: the binding table of include/ikflow_amd_cloud.h against both flavours of the library, that
the header is plain C, that the other extension headers still declare what their tables say, and the asserts of IKFlowSolver.set_world_cloud."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rank_helpers as RH
from helpers import tiny_model
from ikflow_amd import _lib
from ikflow_amd.ikflow_solver import IKFlowSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHERS = (("ikflow_amd_rank.h", "RANK_SIGNATURES"), ("ikflow_amd_path.h", "PATH_SIGNATURES"), ("ikflow_amd_diverse.h", "DIVERSE_SIGNATURES"),
          ("ikflow_amd_world.h", "WORLD_SIGNATURES"), ("ikflow_amd_sweep.h", "SWEEP_SIGNATURES"), ("ikflow_amd_refine.h", "REFINE_SIGNATURES"))


def _declared(header):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", code)), code


def test_cloud_header_is_bound_and_exported_by_both_flavours():
    """Every ikf_ function that include/ikflow_amd_cloud.h declares is in _lib.CLOUD_SIGNATURES (and only those), none of them is in the other
    tables, and both flavours of the library export them; the #define matches the binding; the ABI version is still 3."""
    declared, code = _declared("ikflow_amd_cloud.h")
    assert declared == {"ikf_set_world_cloud", "ikf_world_cloud_size", "ikf_cloud_clearance"}
    assert declared == set(_lib.CLOUD_SIGNATURES)
    for table in (_lib.SIGNATURES, _lib.RANK_SIGNATURES, _lib.PATH_SIGNATURES, _lib.DIVERSE_SIGNATURES, _lib.WORLD_SIGNATURES, _lib.SWEEP_SIGNATURES,
                  _lib.REFINE_SIGNATURES):
        assert not (declared & set(table))
    assert re.findall(r"#define (IKF_[A-Z_]+) ", code) == ["IKF_CLOUD_MAX_POINTS"]
    assert re.search(r"#define IKF_CLOUD_MAX_POINTS \(1 << 20\)", code) and _lib.IKF_CLOUD_MAX_POINTS == 1 << 20
    assert _lib.IKF_ABI_VERSION == 3
    for flavour in ("", "probes"):
        lib = _lib.load(flavour)
        assert lib.ikf_abi_version() == 3
        for name, (restype, argtypes) in _lib.CLOUD_SIGNATURES.items():
            assert hasattr(lib, name), f"{name} is not exported by the {flavour or 'product'} library"
            assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype   # (load() applied the table)
        assert lib.ikf_set_world_cloud(None, None, 0, 0.0, 0.0) == _lib.IKF_ERR_NULL_POINTER   # (no handle, no device)
        assert "null model" in _lib.last_error(lib)
        assert lib.ikf_cloud_clearance(None, None, 0, None, None, None) == _lib.IKF_ERR_NULL_POINTER
        assert lib.ikf_world_cloud_size(None) == 0


def test_the_other_extension_headers_still_declare_what_their_tables_say():
    for header, table in OTHERS:
        assert _declared(header)[0] == set(getattr(_lib, table)), header


def test_cloud_header_is_plain_c(tmp_path):
    """The header compiles as C11 (and as C++17) on its own, with every warning an error."""
    for compiler, std, ext in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")):
        src = tmp_path / f"client.{ext}"
        src.write_text('#include "ikflow_amd_cloud.h"\nint main(void) { return IKF_CLOUD_MAX_POINTS == 1048576 && ikf_world_cloud_size(0) == 0 ? 0 : 1; }\n')
        r = subprocess.run([compiler, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]


def test_solver_set_world_cloud_asserts_fire_before_any_device_work():
    robot, hp, lay, sd = tiny_model()
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    pts = np.array([[0.4, 0.0, 0.3], [0.5, 0.1, 0.2]])
    for bad in (np.zeros((4, 2)), np.zeros(6), torch.zeros(2, 3, 1)):
        with pytest.raises(AssertionError, match=re.escape("points must be [n x 3]")):
            s.set_world_cloud(bad, 0.01)
    with pytest.raises(AssertionError, match="points must be finite"):
        s.set_world_cloud(np.array([[0.0, float("nan"), 0.0]]), 0.01)
    with pytest.raises(AssertionError, match="points must be finite"):
        s.set_world_cloud(torch.tensor([[0.0, float("inf"), 0.0]]), 0.01)
    for bad in (float("nan"), float("inf"), None, "0", True):
        with pytest.raises(AssertionError, match="point_radius must be a finite number"):
            s.set_world_cloud(pts, bad)
        with pytest.raises(AssertionError, match="min_clearance must be a finite number"):
            s.set_world_cloud(pts, 0.01, bad)
    with pytest.raises(AssertionError, match="point_radius must be >= 0"):
        s.set_world_cloud(pts, -0.01)
    with pytest.raises(AssertionError, match="at most 1048576 points"):
        s.set_world_cloud(np.zeros(((1 << 20) + 1, 3), np.float32), 0.01)
    assert not robot.has_collision_model
    with pytest.raises(AssertionError, match="set_world_cloud needs a collision model"):
        s.set_world_cloud(pts, 0.01)
    s.set_world_cloud(None, 0.01)                 # no cloud, no engine yet: nothing to do, on any machine
    s.set_world_cloud(np.zeros((0, 3)), 0.01)     # an empty cloud is no cloud either
    s.set_world_cloud(torch.zeros(0, 3), 0.0)
    assert s._world_cloud is None
    robot.set_collision_capsules(RH.collision_capsules(robot))
    if not torch.cuda.is_available():   # a call that passes every assert gets as far as the engine, which has no CPU path
        from ikflow_amd.engine import EngineError

        with pytest.raises(EngineError, match="no CPU path"):
            s.set_world_cloud(torch.tensor(pts), 0.01, 0.02)
        got, radius, thr = s._world_cloud   # (remembered: the engine of the first GPU call gets it)
        assert got.dtype == np.float32 and got.shape == (2, 3) and np.array_equal(got, pts.astype(np.float32))
        assert math.isclose(radius, 0.01) and math.isclose(thr, 0.02)
