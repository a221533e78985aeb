"""The caller's scene: up to 64 static obstacles in the robot's base frame (include/ikflow_amd_world.h), as plain numbers.

A ``World`` is handed to ``Engine.set_world`` / ``IKFlowSolver.set_world`` / ``Robot.env_collision_distances``; it validates what
``ikf_set_world`` validates, with the same wording, so a mistake is reported where the obstacle is added.  The definitions of the clearances are
this project's own (jrl solves a QP for its cuboids; nothing of it is used here)."""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np

MAX_OBSTACLES = 64
SPHERE, CAPSULE, HALF_SPACE, BOX = 0, 1, 2, 3
KIND_NAMES = ("sphere", "capsule", "half_space", "box")

Obstacle = Tuple[int, Tuple[float, float, float], Tuple[float, float, float], Tuple[float, float, float, float], float]


def _vec(v, n: int, what: str) -> Tuple[float, ...]:
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    assert a.shape == (n,), f"{what} must have {n} numbers, got shape {np.shape(v)}"
    return tuple(float(x) for x in a)


def validate_obstacle(i: int, kind, a, b, quat, radius) -> Obstacle:
    """One obstacle in the layout of ikf_obstacle -> the tuple a World stores; raises ValueError naming obstacle i, as ikf_set_world does."""
    who = f"obstacle {i}"
    if not isinstance(kind, (int, np.integer)) or not SPHERE <= int(kind) <= BOX:
        raise ValueError(f"{who}: unknown kind {kind!r}")
    a, b, quat, radius = _vec(a, 3, f"{who}: a"), _vec(b, 3, f"{who}: b"), _vec(quat, 4, f"{who}: quat"), float(radius)
    if not all(math.isfinite(x) for x in (*a, *b, *quat, radius)):
        raise ValueError(f"{who}: non-finite number")
    if radius < 0.0:
        raise ValueError(f"{who}: radius must be >= 0")
    if kind == HALF_SPACE and not math.sqrt(sum(x * x for x in a)) > 0.0:
        raise ValueError(f"{who}: zero normal")
    if kind == BOX:
        if not all(x > 0.0 for x in b):
            raise ValueError(f"{who}: half extents must be > 0")
        if not sum(x * x for x in quat) > 0.0:
            raise ValueError(f"{who}: zero quaternion")
    return (int(kind), a, b, quat, radius)


def rotation_to_quaternion(R) -> Tuple[float, float, float, float]:
    """Unit quaternion (w, x, y, z), w >= 0, of a 3 x 3 rotation matrix, in float64 (the largest of the four squares is divided by)."""
    R = np.asarray(R, dtype=np.float64)
    t = (R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1])
    i = int(np.argmax(t))
    s = 2.0 * math.sqrt(1.0 + t[i])
    if i == 0:
        q = (0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s)
    elif i == 1:
        q = ((R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s)
    elif i == 2:
        q = ((R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s)
    else:
        q = ((R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s)
    n = math.sqrt(sum(x * x for x in q))
    sign = -1.0 if q[0] < 0.0 else 1.0
    return tuple(float(sign * x / n) for x in q)


class World:
    """A list of obstacles.  Every add_* returns the obstacle's index - what ``world_clearance`` reports as the closest obstacle."""

    def __init__(self):
        self._obstacles: List[Obstacle] = []

    def __len__(self) -> int:
        return len(self._obstacles)

    @property
    def obstacles(self) -> Tuple[Obstacle, ...]:
        """(kind, a[3], b[3], quat[4], radius) per obstacle, the fields of ikf_obstacle."""
        return tuple(self._obstacles)

    def _add(self, kind, a, b, quat, radius) -> int:
        if len(self._obstacles) >= MAX_OBSTACLES:
            raise ValueError(f"a world holds at most {MAX_OBSTACLES} obstacles")
        self._obstacles.append(validate_obstacle(len(self._obstacles), kind, a, b, quat, radius))
        return len(self._obstacles) - 1

    def add_sphere(self, centre: Sequence[float], radius: float) -> int:
        return self._add(SPHERE, centre, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), radius)

    def add_capsule(self, a: Sequence[float], b: Sequence[float], radius: float) -> int:
        return self._add(CAPSULE, a, b, (1.0, 0.0, 0.0, 0.0), radius)

    def add_half_space(self, normal: Sequence[float], offset: float) -> int:
        """Solid where normal . x <= offset (a floor at height z0: normal (0, 0, 1), offset z0).  The normal need not be of unit length."""
        return self._add(HALF_SPACE, normal, (offset, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), 0.0)

    def add_box(self, centre: Sequence[float], half_extents: Sequence[float], quat: Sequence[float] = (1.0, 0.0, 0.0, 0.0), rounding: float = 0.0) -> int:
        """quat: (w, x, y, z) of the box's orientation in the base frame; rounding: the box grown by that radius (rounded edges)."""
        return self._add(BOX, centre, half_extents, quat, rounding)

    def add_cuboid(self, cuboid6: Sequence[float], T: Sequence[Sequence[float]]) -> int:
        """jrl's form: (xmin, ymin, zmin, xmax, ymax, zmax) in the cuboid's own frame and the homogeneous 4 x 4 transform of that frame in
        the base frame.  The rotation becomes a quaternion in float64; a T whose rotation block is not orthonormal to 1e-6 is refused."""
        c = np.asarray(cuboid6, dtype=np.float64).reshape(-1)
        T = np.asarray(T, dtype=np.float64)
        i = len(self._obstacles)
        if c.shape != (6,) or T.shape != (4, 4):
            raise ValueError(f"obstacle {i}: a cuboid is 6 numbers and a 4 x 4 transform")
        if not (np.isfinite(c).all() and np.isfinite(T).all()):
            raise ValueError(f"obstacle {i}: non-finite number")
        R = T[:3, :3]
        if np.abs(R.T @ R - np.eye(3)).max() > 1e-6 or np.linalg.det(R) < 0.0 or np.abs(T[3] - np.array([0.0, 0.0, 0.0, 1.0])).max() > 1e-6:
            raise ValueError(f"obstacle {i}: T is not a rigid transform (rotation block not orthonormal to 1e-6)")
        lo, hi = c[:3], c[3:]
        centre = R @ (0.5 * (lo + hi)) + T[:3, 3]
        return self._add(BOX, centre, 0.5 * (hi - lo), rotation_to_quaternion(R), 0.0)
