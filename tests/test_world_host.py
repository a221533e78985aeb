"""World collision, what can be checked without a GPU: the binding table of include/ikflow_amd_world.h against both flavours of the library, the
validation messages of ikflow_amd.world.World, add_cuboid against add_box, and the asserts of IKFlowSolver.set_world."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import rank_helpers as RH
from helpers import tiny_model
from ikflow_amd import _lib
from ikflow_amd.ikflow_solver import IKFlowSolver
from ikflow_amd.world import BOX, CAPSULE, HALF_SPACE, MAX_OBSTACLES, SPHERE, World, rotation_to_quaternion, validate_obstacle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_world_header_is_bound_and_exported_by_both_flavours():
    """Every ikf_ function that include/ikflow_amd_world.h declares is in _lib.WORLD_SIGNATURES (and only those), none of them is in the other
    tables, and both flavours of the library export them; ikf_obstacle of the binding has the header's fields in its order, types and size; the
    #define and the kinds match; the ABI version is still 3."""
    text = open(os.path.join(ROOT, "include", "ikflow_amd_world.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", code))
    assert declared == {"ikf_set_world", "ikf_world_size", "ikf_world_clearance"}
    assert declared == set(_lib.WORLD_SIGNATURES)
    for table in (_lib.SIGNATURES, _lib.RANK_SIGNATURES, _lib.PATH_SIGNATURES, _lib.DIVERSE_SIGNATURES):
        assert not (declared & set(table))
    body = re.search(r"typedef struct ikf_obstacle \{(.*?)\} ikf_obstacle;", code, re.S).group(1)
    decls = [decl.strip().split(None, 1) for decl in body.split(";") if decl.strip()]
    got = []
    for typ, name in decls:
        arr = re.fullmatch(r"(\w+)\[(\d+)\]", name.strip())
        base = {"float": C.c_float, "int32_t": C.c_int32}[typ]
        got.append((arr.group(1), base * int(arr.group(2))) if arr else (name.strip(), base))
    assert [g[0] for g in got] == [f[0] for f in _lib.ikf_obstacle._fields_] == ["kind", "a", "b", "quat", "radius"]
    assert all(C.sizeof(g[1]) == C.sizeof(f[1]) and g[1]._type_ == f[1]._type_ for g, f in zip(got, _lib.ikf_obstacle._fields_))
    assert C.sizeof(_lib.ikf_obstacle) == 48
    assert int(re.search(r"#define IKF_WORLD_MAX_OBSTACLES (\d+)", code).group(1)) == _lib.IKF_WORLD_MAX_OBSTACLES == MAX_OBSTACLES == 64
    assert re.findall(r"#define (IKF_[A-Z_]+) ", code) == ["IKF_WORLD_MAX_OBSTACLES"]
    kinds = dict((n, int(v)) for n, v in re.findall(r"(IKF_OBSTACLE_[A-Z_]+) = (\d+)", code))
    assert kinds == {"IKF_OBSTACLE_SPHERE": SPHERE, "IKF_OBSTACLE_CAPSULE": CAPSULE, "IKF_OBSTACLE_HALF_SPACE": HALF_SPACE, "IKF_OBSTACLE_BOX": BOX}
    assert all(getattr(_lib, n) == v for n, v in kinds.items())
    assert _lib.IKF_ABI_VERSION == 3
    for flavour in ("", "probes"):
        lib = _lib.load(flavour)
        assert lib.ikf_abi_version() == 3
        for name, (restype, argtypes) in _lib.WORLD_SIGNATURES.items():
            assert hasattr(lib, name), f"{name} is not exported by the {flavour or 'product'} library"
            assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype   # (load() applied the table)
        assert lib.ikf_set_world(None, None, 0, 0.0) == _lib.IKF_ERR_NULL_POINTER   # (no handle, no device)
        assert "null model" in _lib.last_error(lib)
        assert lib.ikf_world_clearance(None, None, 0, None, None, None, None, None) == _lib.IKF_ERR_NULL_POINTER
        assert lib.ikf_world_size(None) == 0


def test_every_validation_message_of_world():
    unit = (1.0, 0.0, 0.0, 0.0)
    nan, inf = float("nan"), float("inf")
    w = World()
    assert w.add_sphere((0, 0, 1), 0.1) == 0 and w.add_capsule((0, 0, 1), (1, 0, 1), 0.0) == 1 and len(w) == 2
    bad = [
        (lambda: w.add_sphere((0, 0, nan), 0.1), "obstacle 2: non-finite number"),
        (lambda: w.add_sphere((0, 0, 1), inf), "obstacle 2: non-finite number"),
        (lambda: w.add_sphere((0, 0, 1), -0.1), "obstacle 2: radius must be >= 0"),
        (lambda: w.add_capsule((0, 0, 1), (inf, 0, 0), 0.1), "obstacle 2: non-finite number"),
        (lambda: w.add_capsule((0, 0, 1), (1, 0, 0), -1e-9), "obstacle 2: radius must be >= 0"),
        (lambda: w.add_half_space((0, 0, 0), 0.1), "obstacle 2: zero normal"),
        (lambda: w.add_half_space((0, 0, 1), nan), "obstacle 2: non-finite number"),
        (lambda: w.add_box((0, 0, 0), (0.1, 0.0, 0.1)), "obstacle 2: half extents must be > 0"),
        (lambda: w.add_box((0, 0, 0), (0.1, -0.2, 0.1)), "obstacle 2: half extents must be > 0"),
        (lambda: w.add_box((0, 0, 0), (0.1, 0.2, 0.1), (0, 0, 0, 0)), "obstacle 2: zero quaternion"),
        (lambda: w.add_box((0, 0, 0), (0.1, 0.2, 0.1), (1, 0, nan, 0)), "obstacle 2: non-finite number"),
        (lambda: w.add_box((0, 0, 0), (0.1, 0.2, 0.1), unit, -0.01), "obstacle 2: radius must be >= 0"),
        (lambda: w._add(4, (0, 0, 0), (0, 0, 0), unit, 0.0), "obstacle 2: unknown kind 4"),
        (lambda: w._add(-1, (0, 0, 0), (0, 0, 0), unit, 0.0), "obstacle 2: unknown kind -1"),
        (lambda: w._add("box", (0, 0, 0), (0, 0, 0), unit, 0.0), "obstacle 2: unknown kind 'box'"),
        (lambda: w.add_cuboid((0, 0, 0, 1, 1), np.eye(4)), "obstacle 2: a cuboid is 6 numbers and a 4 x 4 transform"),
        (lambda: w.add_cuboid((0, 0, 0, 1, 1, nan), np.eye(4)), "obstacle 2: non-finite number"),
        (lambda: w.add_cuboid((0, 0, 0, 1, 1, 1), np.diag([1.0, 1.0, 1.00001, 1.0])), "obstacle 2: T is not a rigid transform"),
        (lambda: w.add_cuboid((0, 0, 0, 1, 1, 1), np.diag([1.0, 1.0, -1.0, 1.0])), "obstacle 2: T is not a rigid transform"),
        (lambda: w.add_cuboid((0, 0, 0, 1, 0, 1), np.eye(4)), "obstacle 2: half extents must be > 0"),
    ]
    for call, msg in bad:
        with pytest.raises(ValueError, match=re.escape(msg)):
            call()
    assert len(w) == 2   # (a refused obstacle is not added)
    with pytest.raises(AssertionError, match="obstacle 2: a must have 3 numbers"):
        w.add_sphere((0, 0), 0.1)
    assert validate_obstacle(7, np.int64(BOX), (0, 0, 0), (1, 1, 1), (0, 2, 0, 0), 0)[0] == BOX
    full = World()
    for i in range(64):
        assert full.add_sphere((i, 0, 0), 0.1) == i
    with pytest.raises(ValueError, match="at most 64 obstacles"):
        full.add_sphere((0, 0, 0), 0.1)
    kind, a, b, quat, radius = w.obstacles[1]
    assert (kind, a, b, quat, radius) == (CAPSULE, (0.0, 0.0, 1.0), (1.0, 0.0, 1.0), unit, 0.0) and all(type(x) is float for x in (*a, *b, *quat, radius))
    hs = World()
    hs.add_half_space((0, 0, 2), 0.5)   # kept as given: ikf_set_world normalises, in double precision
    assert hs.obstacles[0] == (HALF_SPACE, (0.0, 0.0, 2.0), (0.5, 0.0, 0.0), unit, 0.0)


def test_add_cuboid_of_a_rotated_transform_equals_add_box_of_the_same_box():
    rng = np.random.default_rng(3)
    for _ in range(50):
        q = rng.standard_normal(4)
        q /= np.linalg.norm(q)
        if q[0] < 0:
            q = -q
        w_, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w_ * z), 2 * (x * z + w_ * y)],
                      [2 * (x * y + w_ * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w_ * x)],
                      [2 * (x * z - w_ * y), 2 * (y * z + w_ * x), 1 - 2 * (x * x + y * y)]])
        t = rng.uniform(-1, 1, 3)
        lo = rng.uniform(-0.5, 0.0, 3)
        hi = lo + rng.uniform(0.05, 0.6, 3)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        a, b = World(), World()
        a.add_cuboid((*lo, *hi), T)
        b.add_box(R @ (0.5 * (lo + hi)) + t, 0.5 * (hi - lo), q)
        (ka, ca, ha, qa, ra), (kb, cb, hb, qb, rb) = a.obstacles[0], b.obstacles[0]
        assert ka == kb == BOX and ra == rb == 0.0
        assert np.allclose(ca, cb, atol=1e-15) and np.allclose(ha, hb, atol=1e-15) and np.allclose(qa, qb, atol=1e-12)
    # every branch of the rotation-to-quaternion conversion: half turns about each axis, and the identity
    for q in [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0.5, 0.5, 0.5, 0.5), (0.1, 0.7, -0.7, 0.1)]:
        q = np.asarray(q, np.float64) / np.linalg.norm(q)
        w_, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w_ * z), 2 * (x * z + w_ * y)],
                      [2 * (x * y + w_ * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w_ * x)],
                      [2 * (x * z - w_ * y), 2 * (y * z + w_ * x), 1 - 2 * (x * x + y * y)]])
        got = np.asarray(rotation_to_quaternion(R))
        assert min(np.abs(got - q).max(), np.abs(got + q).max()) <= 1e-12 and abs(np.linalg.norm(got) - 1.0) <= 1e-15


def test_solver_set_world_asserts_fire_before_any_device_work():
    robot, hp, lay, sd = tiny_model()
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    w = World()
    w.add_box((0.4, 0.0, 0.3), (0.1, 0.2, 0.05))
    with pytest.raises(AssertionError, match="world must be a ikflow_amd.world.World or None"):
        s.set_world([(0, (0, 0, 0), (0, 0, 0), (1, 0, 0, 0), 0.1)])
    for bad in (float("nan"), float("inf"), None, "0"):
        with pytest.raises(AssertionError, match="min_clearance must be a finite number"):
            s.set_world(w, bad)
    assert not robot.has_collision_model
    with pytest.raises(AssertionError, match="set_world needs a collision model"):
        s.set_world(w)
    s.set_world(None)      # no scene, no engine yet: nothing to do, on any machine
    s.set_world(World())   # an empty world is no scene either
    assert s._world is None
    robot.set_collision_capsules(RH.collision_capsules(robot))
    if not torch.cuda.is_available():   # a call that passes every assert gets as far as the engine, which has no CPU path
        from ikflow_amd.engine import EngineError

        with pytest.raises(EngineError, match="no CPU path"):
            s.set_world(w, 0.01)
        assert math.isclose(s._world[1], 0.01)   # (remembered: the engine of the first GPU call gets it)
