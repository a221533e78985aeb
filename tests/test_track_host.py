"""The world track, what can be checked without a GPU: the binding table of include/ikflow_amd_track.h against both flavours of the library, the
null-handle statuses, and the asserts of IKFlowSolver.set_world_track / timed_path_collides."""
import ctypes as C
import os
import re

import pytest
import torch

from helpers import tiny_model
from ikflow_amd import _lib
from ikflow_amd.ikflow_solver import IKFlowSolver
from ikflow_amd.world import World

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ikf_set_world_track", "ikf_world_track_size", "ikf_world_track_frame", "ikf_world_track_clearance", "ikf_sweep_lattice"}
OTHER_TABLES = ("SIGNATURES", "RANK_SIGNATURES", "PATH_SIGNATURES", "DIVERSE_SIGNATURES", "WORLD_SIGNATURES", "CLOUD_SIGNATURES", "SWEEP_SIGNATURES",
                "REFINE_SIGNATURES", "EXACT_WORLD_SIGNATURES")


def _declared(header):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", code)), code


def test_track_header_is_bound_and_exported_by_both_flavours():
    """Every ikf_ function that include/ikflow_amd_track.h declares is in _lib.TRACK_SIGNATURES (and only those), none of them is in another table,
    and both flavours of the library export them; the #define matches; the ABI version is still 3."""
    declared, code = _declared("ikflow_amd_track.h")
    assert declared == NAMES == set(_lib.TRACK_SIGNATURES)
    for table in OTHER_TABLES:
        assert not (declared & set(getattr(_lib, table))), table
    assert re.findall(r"#define (IKF_[A-Z_]+) ", code) == ["IKF_WORLD_TRACK_MAX_FRAMES"]
    assert int(re.search(r"#define IKF_WORLD_TRACK_MAX_FRAMES (\d+)", code).group(1)) == _lib.IKF_WORLD_TRACK_MAX_FRAMES == 1024
    assert _lib.IKF_ABI_VERSION == 3
    for flavour in ("", "probes"):
        lib = _lib.load(flavour)
        assert lib.ikf_abi_version() == 3
        for name, (restype, argtypes) in _lib.TRACK_SIGNATURES.items():
            assert hasattr(lib, name), f"{name} is not exported by the {flavour or 'product'} library"
            assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype   # (load() applied the table)
        one = (_lib.ikf_obstacle * 1)()
        f, n = C.c_int(7), C.c_int(7)
        for call, who in ((lambda: lib.ikf_set_world_track(None, one, 1, 1, 0.0), "ikf_set_world_track"),
                          (lambda: lib.ikf_world_track_size(None, C.byref(f), C.byref(n)), "ikf_world_track_size"),
                          (lambda: lib.ikf_world_track_frame(None, 0, 0, one), "ikf_world_track_frame"),
                          (lambda: lib.ikf_world_track_clearance(None, None, 0, 1, None, None, None, None, None), "ikf_world_track_clearance"),
                          (lambda: lib.ikf_sweep_lattice(None, None, 0, 1, None, 0, 0.0, None, None), "ikf_sweep_lattice")):
            assert call() == _lib.IKF_ERR_NULL_POINTER   # (no handle, no device)
            assert f"{who}: null model" in _lib.last_error(lib)
        assert (f.value, n.value) == (7, 7)


def test_the_headers_the_track_leaves_alone_declare_what_they_declared():
    """The track lives in its own header: every other extension header keeps exactly its table's functions, ikflow_amd.h is not touched by name,
    and the path, sweep and world headers point here."""
    for header, table in (("ikflow_amd_path.h", "PATH_SIGNATURES"), ("ikflow_amd_world.h", "WORLD_SIGNATURES"), ("ikflow_amd_sweep.h", "SWEEP_SIGNATURES"),
                          ("ikflow_amd_cloud.h", "CLOUD_SIGNATURES"), ("ikflow_amd_rank.h", "RANK_SIGNATURES"), ("ikflow_amd_diverse.h", "DIVERSE_SIGNATURES")):
        assert _declared(header)[0] == set(getattr(_lib, table)), header
    for header in ("ikflow_amd_path.h", "ikflow_amd_sweep.h", "ikflow_amd_world.h"):
        assert "ikflow_amd_track.h" in open(os.path.join(ROOT, "include", header)).read(), header
    assert "track" not in open(os.path.join(ROOT, "include", "ikflow_amd.h")).read()


def _frames(F, kinds=("sphere", "box")):
    out = []
    for t in range(F):
        w = World()
        for kind in kinds:
            if kind == "sphere":
                w.add_sphere((1.0 + 0.1 * t, 0.0, 0.5), 0.1)
            else:
                w.add_box((0.0, 1.0, 0.1 * t), (0.1, 0.2, 0.3))
        out.append(w)
    return out


def test_solver_track_asserts_fire_before_any_device_work():
    robot, hp, lay, sd = tiny_model()
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    assert not robot.has_collision_model
    with pytest.raises(AssertionError, match="set_world_track needs a collision model"):
        s.set_world_track(_frames(3))
    with pytest.raises(AssertionError, match="must be a sequence of ikflow_amd.world.World"):
        s.set_world_track([_frames(1)[0], "no world"])
    with pytest.raises(AssertionError, match="frame 2 holds 1 obstacles, frame 0 holds 2"):
        s.set_world_track(_frames(2) + _frames(1, ("sphere",)))
    with pytest.raises(AssertionError, match="frame 1 obstacle 1: kind 0 differs from frame 0's kind 3"):
        s.set_world_track(_frames(1) + _frames(1, ("sphere", "sphere")))
    with pytest.raises(AssertionError, match="frame 0 holds no obstacle"):
        s.set_world_track([World(), World()])
    with pytest.raises(AssertionError, match="at most 1024 frames"):
        s.set_world_track(_frames(1) * 1025)
    for bad in (float("nan"), float("inf"), None, True):
        with pytest.raises(AssertionError, match="min_clearance must be a finite number"):
            s.set_world_track(_frames(2), bad)
    assert s._world_track is None
    s.set_world_track(None)     # no engine yet: nothing to clear
    s.set_world_track([])
    assert s._world_track is None and s._engine is None
    path = torch.zeros(5, robot.ndof)
    with pytest.raises(AssertionError, match="path must be"):
        s.timed_path_collides(torch.zeros(5, robot.ndof + 1))
    with pytest.raises(AssertionError, match="q_start must be"):
        s.timed_path_collides(path, torch.zeros(robot.ndof + 1))
    with pytest.raises(AssertionError, match="timed_path_collides needs a sweep"):
        s.timed_path_collides(path)
    s.set_path_sweep(2)
    with pytest.raises(AssertionError, match="timed_path_collides needs a collision model"):
        s.timed_path_collides(path)
