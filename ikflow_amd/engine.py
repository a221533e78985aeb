"""Python face of the C-ABI engine: owns an ``ikf_model`` handle, passes torch device pointers + the current HIP
stream through ctypes.  torch is used here only for device memory and streams."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ikflow_amd import _lib
from ikflow_amd.model import FlowLayout, LEAKY_RELU_SLOPE
from ikflow_amd.robots import JOINT_FIXED, Robot, rpy_to_matrix


class EngineError(RuntimeError):
    pass


def _raise(code: int, lib=None):
    msg = _lib.last_error(lib)
    if code == _lib.IKF_ERR_NOT_LOADED:
        raise AssertionError(msg)  # the reference asserts (ikflow_solver.py:310-311)
    if code == _lib.IKF_ERR_MISSING_TENSOR:
        raise RuntimeError("Error(s) in loading state_dict: " + msg)
    raise EngineError(f"libikflow_amd status {code}: {msg}")


def _check(code: int, lib=None):
    if code != _lib.IKF_OK:
        _raise(code, lib)


def fold_chain(robot: Robot) -> Tuple[List[Tuple[int, np.ndarray, np.ndarray]], np.ndarray]:
    """Fold the fixed URDF transforms into the actuated joints: [(kind, axis, pre 3x4)], tool 3x4 (float64 math)."""
    joints = []
    T = np.eye(4)
    for j in robot.joints:
        F = np.eye(4)
        F[:3, :3] = rpy_to_matrix(j.origin_rpy)
        F[:3, 3] = j.origin_xyz
        T = T @ F
        if j.kind == JOINT_FIXED:
            continue
        ax = np.asarray(j.axis, dtype=np.float64)
        ax = ax / np.linalg.norm(ax)
        joints.append((int(j.kind), ax, T[:3, :4].copy()))
        T = np.eye(4)
    return joints, T[:3, :4].copy()


def _make_desc(layout: FlowLayout, robot: Robot) -> _lib.ikf_model_desc:
    d = _lib.ikf_model_desc()
    d.abi_version = _lib.IKF_ABI_VERSION
    d.nb_nodes, d.dim, d.dim_cond = layout.nb_nodes, layout.dim, layout.dim_cond
    d.width, d.n_hidden = layout.width, layout.n_hidden
    d.clamp, d.leaky_slope = layout.clamp, LEAKY_RELU_SLOPE
    d.ndof = robot.ndof
    d.sigmoid_on_output = 1 if getattr(layout, "sigmoid_on_output", False) else 0
    if robot.ndof > _lib.IKF_MAX_DOF:
        raise EngineError(f"robot has {robot.ndof} dof; the engine supports at most {_lib.IKF_MAX_DOF}")
    for i, (lo, hi) in enumerate(robot.actuated_joints_limits):
        d.joint_lo[i], d.joint_hi[i] = lo, hi
    joints, tool = fold_chain(robot)
    for i, (kind, ax, pre) in enumerate(joints):
        d.chain[i].kind = kind
        for k in range(3):
            d.chain[i].axis[k] = float(ax[k])
        for k, v in enumerate(pre.reshape(-1)):
            d.chain[i].pre[k] = float(v)
    for k, v in enumerate(tool.reshape(-1)):
        d.tool[k] = float(v)
    return d


def _dev_index(device) -> int:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise EngineError(f"ikflow_amd runs on the GPU only; got device '{dev}' (there is no CPU path)")
    return dev.index if dev.index is not None else torch.cuda.current_device()


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor (got {type(t)})")
    if t.device.type != "cuda":
        raise EngineError(f"{name} is on '{t.device}'; ikflow_amd runs on the GPU only (there is no CPU path)")
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    return t.contiguous()


def _scoring_fields(rot_weight, max_pos_err, max_rot_err, reject_limits, reject_collisions, min_clearance) -> dict:
    """The six fields that ikf_rank_options, ikf_path_options and ikf_diverse_options share: no bound is -1, switches are 0 / 1."""
    return dict(rot_weight=float(rot_weight), max_pos_err=-1.0 if max_pos_err is None else float(max_pos_err),
                max_rot_err=-1.0 if max_rot_err is None else float(max_rot_err), reject_limits=1 if reject_limits else 0,
                reject_collisions=1 if reject_collisions else 0, min_clearance=float(min_clearance))


class Engine:
    """One ikf_model handle on one device."""

    def __init__(self, layout: FlowLayout, robot: Robot, device, flavour: str = ""):
        self.lib = _lib.load(flavour)
        self.flavour = flavour
        self.layout = layout
        self.robot = robot
        self.device = torch.device("cuda", _dev_index(device))
        self._h = C.c_void_p()
        desc = _make_desc(layout, robot)
        self._ck(self.lib.ikf_create(C.byref(desc), self.device.index, C.byref(self._h)))

    def _ck(self, code: int) -> None:
        _check(code, self.lib)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self.lib.ikf_destroy(h)
            except Exception:
                pass
            self._h = C.c_void_p()

    # -- helpers -------------------------------------------------------------------------------------
    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _on_device(self, t: torch.Tensor, name: str) -> torch.Tensor:
        t = _f32(t, name)
        if t.device != self.device:
            raise EngineError(f"{name} is on {t.device} but the engine lives on {self.device}")
        return t

    # -- weights -------------------------------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, np.ndarray]) -> None:
        """sd: {FrEIA key: numpy array (float32 / int64)} - see ikflow_amd.model for the key names."""
        items = list(sd.items())
        arr = (_lib.ikf_tensor * len(items))()
        keep = []
        for i, (k, v) in enumerate(items):
            v = np.ascontiguousarray(v)
            if v.dtype.kind == "f":
                v = v.astype(np.float32, copy=False)
                dt = 0
            elif v.dtype.kind in "iu":
                v = v.astype(np.int64, copy=False)
                dt = 1
            else:
                continue
            if v.ndim > 4:
                continue
            name = k.encode("utf-8")
            keep.append((name, v))
            arr[i].name = name
            arr[i].h_data = v.ctypes.data
            arr[i].dtype = dt
            arr[i].ndim = v.ndim
            for a, s in enumerate(v.shape):
                arr[i].shape[a] = s
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_load_weights(self._h, arr, len(items)))
        del keep

    @property
    def weights_loaded(self) -> bool:
        return bool(self.lib.ikf_weights_loaded(self._h))

    def reserve(self, max_rows: int) -> None:
        self._ck(self.lib.ikf_reserve(self._h, int(max_rows)))

    def reserve_exact(self, max_poses: int, max_repeat: int = 10) -> None:
        """Pre-size the exact-IK state (max_poses * max_repeat LM rows) so that generate_exact allocates nothing."""
        self._ck(self.lib.ikf_reserve_exact(self._h, int(max_poses), int(max_repeat)))

    def set_exact_upfront_rows(self, max_rows: int) -> None:
        """Largest worst-case exact-IK row state a call may reserve up front (0: always grow per retry round)."""
        self._ck(self.lib.ikf_set_exact_upfront_rows(self._h, int(max_rows)))

    PRECISIONS = {"f32": 0, "f16x3": 1}

    def set_precision(self, mode: str) -> None:
        """"f32": hidden contractions on the exact-f32 MFMA. "f16x3": error-compensated three-product f16 split."""
        self._ck(self.lib.ikf_set_precision(self._h, self.PRECISIONS[mode]))

    @property
    def precision(self) -> str:
        return {v: k for k, v in self.PRECISIONS.items()}[self.lib.ikf_get_precision(self._h)]

    LM_PRECISIONS = {"f32": 0, "f64": 1}

    def set_lm_precision(self, mode: str) -> None:
        """Arithmetic of the LM step (include/ikflow_amd.h ikf_set_lm_precision): "f64" (default) = fp64 inside the step, Cholesky; "f32" =
        the reference's own arithmetic (fp32 throughout, LU with partial pivoting as torch.linalg.solve, ikflow_solver.py:205,208)."""
        self._ck(self.lib.ikf_set_lm_precision(self._h, self.LM_PRECISIONS[mode]))

    @property
    def lm_precision(self) -> str:
        return {v: k for k, v in self.LM_PRECISIONS.items()}[self.lib.ikf_get_lm_precision(self._h)]

    def set_split_guard(self, on: bool) -> None:
        """f16x3 range guard (include/ikflow_amd.h ikf_set_split_guard): on (default) = one 4-byte flag read per call and an
        automatic f32 re-run when a hidden activation left the f16 range; off = no synchronisation, no re-run."""
        self._ck(self.lib.ikf_set_split_guard(self._h, 1 if on else 0))

    @property
    def split_fallback_count(self) -> int:
        return int(self.lib.ikf_split_fallback_count(self._h))

    def split_overflow_pending(self) -> bool:
        return bool(self.lib.ikf_split_overflow_pending(self._h, self._stream()))

    def set_gemm_variant(self, variant: int) -> None:
        self._ck(self.lib.ikf_set_gemm_variant(self._h, int(variant)))

    # -- approximate IK ------------------------------------------------------------------------------
    def generate_approx(self, poses: torch.Tensor, latent: torch.Tensor, clamp: bool, softflow_scale: float = 0.0) -> torch.Tensor:
        """poses [n x 7] or [7] (broadcast); latent [n x D] -> [n x ndof]."""
        latent = self._on_device(latent, "latent")
        poses = self._on_device(poses, "y")
        n = latent.shape[0]
        assert latent.ndim == 2 and latent.shape[1] == self.layout.dim, f"latent must be [n x {self.layout.dim}], got {tuple(latent.shape)}"
        broadcast = poses.numel() == 7
        if not broadcast:
            assert poses.ndim == 2 and poses.shape[1] == 7 and poses.shape[0] == n, f"{poses.shape[0]} != {n}"
        out = torch.empty((n, self.layout.ndof), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(
                self.lib.ikf_generate_approx(
                    self._h, poses.data_ptr(), 1 if broadcast else 0, latent.data_ptr(), n, 1 if clamp else 0,
                    float(softflow_scale), out.data_ptr(), self._stream(),
                )
            )
        return out

    # -- forward (training-direction) pass ----------------------------------------------------------
    def flow_forward(self, x: torch.Tensor, poses: torch.Tensor, softflow_scale: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
        """x [n x D] padded joint rows; poses [n x 7] or [7] (broadcast) -> (z [n x D], log_det [n]) (ikf_flow_forward)."""
        x = self._on_device(x, "x")
        poses = self._on_device(poses, "y")
        n = x.shape[0]
        assert x.ndim == 2 and x.shape[1] == self.layout.dim, f"x must be [n x {self.layout.dim}], got {tuple(x.shape)}"
        broadcast = poses.numel() == 7
        if not broadcast:
            assert poses.ndim == 2 and poses.shape[1] == 7 and poses.shape[0] == n, f"{poses.shape[0]} != {n}"
        z = torch.empty((n, self.layout.dim), dtype=torch.float32, device=self.device)
        log_det = torch.empty((n,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(
                self.lib.ikf_flow_forward(
                    self._h, x.data_ptr(), n, poses.data_ptr(), 1 if broadcast else 0, float(softflow_scale),
                    z.data_ptr(), log_det.data_ptr(), self._stream(),
                )
            )
        return z, log_det

    # -- inverse pass with its log-determinant ---------------------------------------------------------
    def flow_inverse(self, latent: torch.Tensor, poses: torch.Tensor, softflow_scale: float = 0.0,
                     clamp: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """latent [n x D]; poses [n x 7] or [7] (broadcast) -> (x [n x D] all columns, unclamped; q [n x ndof] = x[:, :ndof], clamped
        to the joint limits when `clamp`; log_det [n] = log|det dx/dz|) in one pass (ikf_flow_inverse)."""
        latent = self._on_device(latent, "latent")
        poses = self._on_device(poses, "y")
        n = latent.shape[0]
        assert latent.ndim == 2 and latent.shape[1] == self.layout.dim, f"latent must be [n x {self.layout.dim}], got {tuple(latent.shape)}"
        broadcast = poses.numel() == 7
        if not broadcast:
            assert poses.ndim == 2 and poses.shape[1] == 7 and poses.shape[0] == n, f"{poses.shape[0]} != {n}"
        x = torch.empty((n, self.layout.dim), dtype=torch.float32, device=self.device)
        q = torch.empty((n, self.layout.ndof), dtype=torch.float32, device=self.device)
        log_det = torch.empty((n,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(
                self.lib.ikf_flow_inverse(
                    self._h, latent.data_ptr(), n, poses.data_ptr(), 1 if broadcast else 0, float(softflow_scale),
                    1 if clamp else 0, x.data_ptr(), q.data_ptr(), log_det.data_ptr(), self._stream(),
                )
            )
        return x, q, log_det

    # -- kinematics ----------------------------------------------------------------------------------
    def _q(self, q: torch.Tensor) -> torch.Tensor:
        q = self._on_device(q, "q")
        assert q.ndim == 2 and q.shape[1] == self.layout.ndof, f"q must be [n x {self.layout.ndof}], got {tuple(q.shape)}"
        return q

    def forward_kinematics(self, q: torch.Tensor) -> torch.Tensor:
        q = self._q(q)
        out = torch.empty((q.shape[0], 7), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_forward_kinematics(self._h, q.data_ptr(), q.shape[0], out.data_ptr(), self._stream()))
        return out

    def pose_error(self, q: torch.Tensor, target_poses: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        q = self._q(q)
        tp = self._on_device(target_poses, "target_poses")
        assert tp.shape == (q.shape[0], 7)
        pe = torch.empty(q.shape[0], dtype=torch.float32, device=self.device)
        re = torch.empty_like(pe)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_pose_error(self._h, q.data_ptr(), tp.data_ptr(), q.shape[0], pe.data_ptr(), re.data_ptr(), self._stream()))
        return pe, re

    def lm_step(self, target_poses: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
        q = self._q(q)
        tp = self._on_device(target_poses, "target_poses")
        assert tp.shape == (q.shape[0], 7)
        out = torch.empty_like(q)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_lm_step(self._h, tp.data_ptr(), q.data_ptr(), q.shape[0], out.data_ptr(), self._stream()))
        return out

    def jacobian(self, q: torch.Tensor) -> torch.Tensor:
        q = self._q(q)
        out = torch.empty((q.shape[0], 6, self.layout.ndof), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_jacobian(self._h, q.data_ptr(), q.shape[0], out.data_ptr(), self._stream()))
        return out

    def clamp_to_joint_limits(self, q: torch.Tensor) -> torch.Tensor:
        q = self._q(q)
        out = torch.empty_like(q)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_clamp_to_joint_limits(self._h, q.data_ptr(), q.shape[0], out.data_ptr(), self._stream()))
        return out

    def joint_limits_exceeded(self, q: torch.Tensor) -> torch.Tensor:
        q = self._q(q)
        out = torch.empty(q.shape[0], dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_joint_limits_exceeded(self._h, q.data_ptr(), q.shape[0], out.data_ptr(), self._stream()))
        return out.to(torch.bool)

    # -- capsule self-collision (evaluation_utils.calculate_self_collisions mechanism) ------------------------
    def set_collision_model(self, capsules, pairs) -> None:
        """capsules: [(frame, p0[3], p1[3], radius)] in engine frames (0 = base, j + 1 = after actuated joint j);
        pairs: [(a, b)] capsule indices."""
        arr = (_lib.ikf_capsule * max(len(capsules), 1))()
        for c, (frame, p0, p1, r) in zip(arr, capsules):
            c.frame, c.radius = int(frame), float(r)
            for k in range(3):
                c.p0[k], c.p1[k] = float(p0[k]), float(p1[k])
        flat = (C.c_int32 * max(2 * len(pairs), 1))(*[int(v) for ab in pairs for v in ab])
        self._ck(self.lib.ikf_set_collision_model(self._h, C.cast(arr, C.c_void_p), len(capsules), C.cast(flat, C.c_void_p), len(pairs)))
        self._has_collision_model = True

    def self_collision(self, q: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """[n x ndof] -> (signed clearance of the closest pair [n] f32, colliding [n] bool)."""
        q = self._q(q)
        dist = torch.empty(q.shape[0], dtype=torch.float32, device=self.device)
        col = torch.empty(q.shape[0], dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_self_collision(self._h, q.data_ptr(), q.shape[0], dist.data_ptr(), col.data_ptr(), self._stream()))
        return dist, col.to(torch.bool)

    # -- world collision (include/ikflow_amd_world.h) --------------------------------------------------------
    def set_world(self, obstacles, min_clearance: float = 0.0) -> None:
        """obstacles: a ikflow_amd.world.World, or [(kind, a[3], b[3], quat[4], radius)] in the layout of ikf_obstacle (an empty one clears).
        While obstacles are set, rank_candidates / generate_ranked, path_search / generate_path and diverse_select / generate_diverse also
        drop every candidate whose world clearance is below min_clearance.  Not while calls on this engine are in flight on another stream."""
        obstacles = list(getattr(obstacles, "obstacles", obstacles))
        if len(obstacles) > _lib.IKF_WORLD_MAX_OBSTACLES:
            raise EngineError(f"a world holds at most {_lib.IKF_WORLD_MAX_OBSTACLES} obstacles, got {len(obstacles)}")
        arr = (_lib.ikf_obstacle * max(len(obstacles), 1))()
        for o, (kind, a, b, quat, radius) in zip(arr, obstacles):
            o.kind, o.radius = int(kind), float(radius)
            for k in range(3):
                o.a[k], o.b[k] = float(a[k]), float(b[k])
            for k in range(4):
                o.quat[k] = float(quat[k])
        self._ck(self.lib.ikf_set_world(self._h, arr, len(obstacles), float(min_clearance)))

    def clear_world(self) -> None:
        self._ck(self.lib.ikf_set_world(self._h, None, 0, 0.0))

    @property
    def world_size(self) -> int:
        return int(self.lib.ikf_world_size(self._h))

    def world_clearance(self, q: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """[n x ndof] -> (signed clearance of the closest (capsule, obstacle) pair [n] f32 - 3.0e38 in an empty world -, that obstacle's index
        [n] int32, that capsule's index [n] int32 (-1 in an empty world), clearance < the world's min_clearance [n] bool)."""
        q = self._q(q)
        n = q.shape[0]
        dist = torch.empty(n, dtype=torch.float32, device=self.device)
        obstacle = torch.empty(n, dtype=torch.int32, device=self.device)
        capsule = torch.empty(n, dtype=torch.int32, device=self.device)
        col = torch.empty(n, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_world_clearance(self._h, q.data_ptr(), n, dist.data_ptr(), obstacle.data_ptr(), capsule.data_ptr(),
                                                  col.data_ptr(), self._stream()))
        return dist, obstacle, capsule, col.to(torch.bool)

    # -- world point cloud (include/ikflow_amd_cloud.h) --------------------------------------------------------
    def set_world_cloud(self, points, point_radius: float, min_clearance: float = 0.0) -> None:
        """points: [n x 3] (numpy or torch, any device; at most 2^20; an empty one clears) in the base frame, each a sphere of point_radius.
        While a cloud is set, rank_candidates / generate_ranked, path_search / generate_path and diverse_select / generate_diverse also drop
        every candidate whose cloud clearance is below min_clearance - beside whatever set_world set; the sweep does not test the cloud.  Not
        while calls on this engine are in flight on another stream."""
        if isinstance(points, torch.Tensor):
            points = points.detach().cpu().numpy()
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 3))
        if len(pts) > _lib.IKF_CLOUD_MAX_POINTS:
            raise EngineError(f"a cloud holds at most {_lib.IKF_CLOUD_MAX_POINTS} points, got {len(pts)}")
        self._ck(self.lib.ikf_set_world_cloud(self._h, pts.ctypes.data if len(pts) else None, len(pts), float(point_radius), float(min_clearance)))

    def clear_world_cloud(self) -> None:
        self._ck(self.lib.ikf_set_world_cloud(self._h, None, 0, 0.0, 0.0))

    @property
    def world_cloud_size(self) -> int:
        return int(self.lib.ikf_world_cloud_size(self._h))

    def cloud_clearance(self, q: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """[n x ndof] -> (signed clearance of the closest (capsule, point) [n] f32 - 3.0e38 with an empty cloud -, clearance < the cloud's
        min_clearance [n] bool)."""
        q = self._q(q)
        n = q.shape[0]
        dist = torch.empty(n, dtype=torch.float32, device=self.device)
        col = torch.empty(n, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_cloud_clearance(self._h, q.data_ptr(), n, dist.data_ptr(), col.data_ptr(), self._stream()))
        return dist, col.to(torch.bool)

    # -- singularity rule (include/ikflow_amd_manip.h) ---------------------------------------------------------
    def set_min_manipulability(self, min_manipulability: float, part: str = "full") -> None:
        """A floor under the manipulability measure of `part` ("full", "linear", "angular") of every candidate (0: no rule, the default).  While
        a floor is set, rank_candidates / generate_ranked, path_search / generate_path and diverse_select / generate_diverse also drop every
        candidate whose measure is not >= it - under set_candidate_refine the refined one's.  Not while calls on this engine are in flight on
        another stream."""
        self._ck(self.lib.ikf_set_min_manipulability(self._h, _lib.MANIP_PARTS[part], float(min_manipulability)))

    @property
    def min_manipulability(self) -> Tuple[float, str]:
        """-> (floor, part) in force on this engine; floor 0: no rule."""
        part, floor = C.c_int(0), C.c_float(0.0)
        self._ck(self.lib.ikf_min_manipulability(self._h, C.byref(part), C.byref(floor)))
        return float(floor.value), {v: k for k, v in _lib.MANIP_PARTS.items()}[part.value]

    def manipulability(self, q: torch.Tensor, part: str = "full", min_manipulability: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
        """[n x ndof] -> (w [n] f32: sqrt(det(J J^T)) over the rows of `part` of the geometric Jacobian - J^T J for a chain of fewer joints than
        rows -, not (w >= min_manipulability) [n] bool).  The call's own floor: the engine's set_min_manipulability state plays no part."""
        q = self._q(q)
        n = q.shape[0]
        w = torch.empty(n, dtype=torch.float32, device=self.device)
        below = torch.empty(n, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_manipulability(self._h, q.data_ptr(), n, _lib.MANIP_PARTS[part], float(min_manipulability), w.data_ptr(),
                                                 below.data_ptr(), self._stream()))
        return w, below.to(torch.bool)

    # -- swept collision checks along edges (include/ikflow_amd_sweep.h) ------------------------------------
    def set_path_sweep(self, n_samples: int) -> None:
        """Samples per lattice edge of path_search / generate_path (0: no sweep, the default; at most 16).  While a sweep is set, an edge
        whose interpolated configurations come closer to the world than its min_clearance - or, with reject_collisions, to the robot itself than
        the options' min_clearance - is forbidden like a step-gate violation.  Not while calls on this engine are in flight on another stream."""
        self._ck(self.lib.ikf_set_path_sweep(self._h, int(n_samples)))

    @property
    def path_sweep(self) -> int:
        return int(self.lib.ikf_get_path_sweep(self._h))

    def sweep_edges(self, q_a: torch.Tensor, q_b: torch.Tensor, n_samples: int, reject_self: bool = False,
                    min_clearance: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
        """Edges q_a[i] -> q_b[i] ([n x ndof] each), n_samples interior samples per edge against the engine's world (and, reject_self, the robot
        itself with min_clearance) -> (blocked [n] bool, first blocked sample [n] int32, -1 where the edge is free)."""
        q_a, q_b = self._q(q_a), self._q(q_b)
        assert q_a.shape == q_b.shape, f"q_a and q_b must have the same shape, got {tuple(q_a.shape)} and {tuple(q_b.shape)}"
        n = q_a.shape[0]
        blocked = torch.empty(n, dtype=torch.uint8, device=self.device)
        first = torch.empty(n, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_sweep_edges(self._h, q_a.data_ptr(), q_b.data_ptr(), n, int(n_samples), 1 if reject_self else 0,
                                              float(min_clearance), blocked.data_ptr(), first.data_ptr(), self._stream()))
        return blocked.to(torch.bool), first

    # -- world track (include/ikflow_amd_track.h) ----------------------------------------------------------------
    @staticmethod
    def _obstacle_array(obstacles):
        arr = (_lib.ikf_obstacle * max(len(obstacles), 1))()
        for o, (kind, a, b, quat, radius) in zip(arr, obstacles):
            o.kind, o.radius = int(kind), float(radius)
            for k in range(3):
                o.a[k], o.b[k] = float(a[k]), float(b[k])
            for k in range(4):
                o.quat[k] = float(quat[k])
        return arr

    def set_world_track(self, frames, min_clearance: float = 0.0) -> None:
        """frames: a sequence of F ikflow_amd.world.World (or lists of (kind, a[3], b[3], quat[4], radius)), one per waypoint, each the same n
        obstacles with the same kinds (an empty sequence clears).  While a track is set, path_search / generate_path also drop candidate r of
        waypoint t when its world clearance against frame t is below min_clearance, and - under set_path_sweep - block an edge whose samples come
        closer than that to the frames interpolated between the two waypoints'.  Beside set_world and set_world_cloud, not instead of them.  Not
        while calls on this engine are in flight on another stream."""
        frames = [list(getattr(f, "obstacles", f)) for f in frames]
        if len(frames) > _lib.IKF_WORLD_TRACK_MAX_FRAMES:
            raise EngineError(f"a world track holds at most {_lib.IKF_WORLD_TRACK_MAX_FRAMES} frames, got {len(frames)}")
        n = len(frames[0]) if frames else 0
        for t, f in enumerate(frames):
            if len(f) != n:
                raise EngineError(f"frame {t} holds {len(f)} obstacles, frame 0 holds {n}: every frame of a world track holds the same obstacles")
        if n > _lib.IKF_WORLD_MAX_OBSTACLES:
            raise EngineError(f"a frame holds at most {_lib.IKF_WORLD_MAX_OBSTACLES} obstacles, got {n}")
        arr = self._obstacle_array([o for f in frames for o in f])
        self._ck(self.lib.ikf_set_world_track(self._h, arr, len(frames), n, float(min_clearance)))

    def clear_world_track(self) -> None:
        self._ck(self.lib.ikf_set_world_track(self._h, None, 0, 0, 0.0))

    @property
    def world_track_size(self) -> Tuple[int, int]:
        """(key frames, obstacles per frame); (0, 0) without a track."""
        f, n = C.c_int(0), C.c_int(0)
        self._ck(self.lib.ikf_world_track_size(self._h, C.byref(f), C.byref(n)))
        return int(f.value), int(n.value)

    def world_track_frame(self, t: int, i: int = 0):
        """The f32 records the device reads for fine frame i (0 .. path_sweep; 0: the key frame itself) after key frame t, as a World."""
        from ikflow_amd.world import World

        n = self.world_track_size[1]
        arr = (_lib.ikf_obstacle * max(n, 1))()
        self._ck(self.lib.ikf_world_track_frame(self._h, int(t), int(i), arr))
        w = World()
        for o in arr[:n]:
            w._add(int(o.kind), tuple(o.a), tuple(o.b), tuple(o.quat), float(o.radius))
        return w

    def world_track_clearance(self, q: torch.Tensor, T: int, k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """q [k * T x ndof] tile-major, row r * T + t against key frame t of the track -> what world_clearance returns, colliding against the
        track's min_clearance."""
        q = self._q(q)
        assert q.shape[0] == int(k) * int(T), f"q must be [{k * T} x {self.layout.ndof}], got {tuple(q.shape)}"
        n = q.shape[0]
        dist = torch.empty(n, dtype=torch.float32, device=self.device)
        obstacle = torch.empty(n, dtype=torch.int32, device=self.device)
        capsule = torch.empty(n, dtype=torch.int32, device=self.device)
        col = torch.empty(n, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_world_track_clearance(self._h, q.data_ptr(), int(T), int(k), dist.data_ptr(), obstacle.data_ptr(), capsule.data_ptr(),
                                                        col.data_ptr(), self._stream()))
        return dist, obstacle, capsule, col.to(torch.bool)

    def sweep_lattice(self, q: torch.Tensor, T: int, k: int, q_start: Optional[torch.Tensor] = None, reject_self: bool = False,
                      min_clearance: float = 0.0) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """The edge mask a path call builds from these rows (q [k * T x ndof] tile-major) under the engine's sweep, world and track and -
        reject_self - the robot itself with min_clearance, nothing pruned -> (edge_free [T][k][k] bool: [t][r][j] the edge from candidate j of
        waypoint t - 1 to candidate r of waypoint t, row 0 all True; start_free [k] bool for q_start -> q[0][r], None without q_start)."""
        q = self._q(q)
        T, k = int(T), int(k)
        assert q.shape[0] == k * T, f"q must be [{k * T} x {self.layout.ndof}], got {tuple(q.shape)}"
        if q_start is not None:
            q_start = self._on_device(q_start, "q_start")
            assert q_start.shape == (self.layout.ndof,), f"q_start must be [{self.layout.ndof}], got {tuple(q_start.shape)}"
        words = (k + 63) // 64
        mask = torch.zeros((T, k, words), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_sweep_lattice(self._h, q.data_ptr(), T, k, None if q_start is None else q_start.data_ptr(), 1 if reject_self else 0,
                                                float(min_clearance), mask.data_ptr(), self._stream()))
        shifts = torch.arange(64, dtype=torch.int64, device=self.device)
        bits = ((mask[..., None] >> shifts) & 1).to(torch.bool).reshape(T, k, words * 64)
        edge_free = bits[:, :, :k].clone()
        start_free = None
        if T > 0:
            if q_start is not None:
                start_free = bits[0, :, 0].clone()
            edge_free[0] = True
        return edge_free, start_free

    # -- refined candidates (include/ikflow_amd_refine.h) ------------------------------------------------------
    def set_candidate_refine(self, n_steps: int, pos_tol: float = 0.0, rot_tol: float = 0.0) -> None:
        """LM steps on every candidate row of generate_ranked / generate_diverse / generate_path, between the flow and the scoring (0: none, the
        default; at most 16).  A row stops after the first step that leaves it below both tolerances (metres, radians; 0: never - all steps run).
        While set, scores, thresholds, limit / collision / world rejection, distances, lattice edges, the sweep and the returned rows are those
        of the refined rows.  Not while calls on this engine are in flight on another stream."""
        self._ck(self.lib.ikf_set_candidate_refine(self._h, int(n_steps), float(pos_tol), float(rot_tol)))

    def candidate_refine(self) -> Tuple[int, float, float]:
        """-> (n_steps, pos_tol, rot_tol) in force on this engine; n_steps 0: no refinement."""
        pos, rot = C.c_float(0.0), C.c_float(0.0)
        n = int(self.lib.ikf_get_candidate_refine(self._h, C.byref(pos), C.byref(rot)))
        return n, float(pos.value), float(rot.value)

    def refine_candidates(self, target_poses: torch.Tensor, k: int, q: torch.Tensor, n_steps: int, pos_tol: float = 0.0, rot_tol: float = 0.0,
                          return_info: bool = False):
        """target_poses [m x 7]; q [k * m x ndof] tile-major (row r * m + j = candidate r of pose j): up to n_steps LM steps on every row, each
        stopping after the first step that leaves it below both tolerances -> q [k * m x ndof], or (q, steps [k * m] uint8, converged [k * m] bool)
        with return_info.  The caller's own rows: the engine's set_candidate_refine state plays no part."""
        tp = self._on_device(target_poses, "target_poses")
        assert tp.ndim == 2 and tp.shape[1] == 7, f"target_poses must be of shape [m x 7], got {tuple(tp.shape)}"
        m = tp.shape[0]
        q = self._q(q)
        assert q.shape[0] == k * m, f"q must be [{k * m} x {self.layout.ndof}] (tile-major), got {tuple(q.shape)}"
        out = torch.empty_like(q)
        steps = torch.empty(k * m, dtype=torch.uint8, device=self.device) if return_info else None
        conv = torch.empty(k * m, dtype=torch.uint8, device=self.device) if return_info else None
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_refine_candidates(
                self._h, tp.data_ptr(), m, int(k), q.data_ptr(), int(n_steps), float(pos_tol), float(rot_tol), out.data_ptr(),
                None if steps is None else steps.data_ptr(), None if conv is None else conv.data_ptr(), self._stream()))
        return (out, steps, conv.to(torch.bool)) if return_info else out

    # -- exact IK that obeys the world (include/ikflow_amd_exact_world.h) ----------------------------------------
    def set_exact_collision(self, on: bool = True, reject_self: bool = False, self_min_clearance: float = 0.0) -> None:
        """The exact collision rule (off by default).  While on, a repeat of generate_exact / refine_exact whose candidate - its q at the first
        LM iteration inside both thresholds - is closer to the world of set_world or the cloud of set_world_cloud than their min_clearance, or,
        with reject_self, to the robot itself than self_min_clearance, does not count: the pose is solved by its earliest admissible repeat or
        goes to the next retry round.  Not while calls on this engine are in flight on another stream."""
        self._ck(self.lib.ikf_set_exact_collision(self._h, 1 if on else 0, 1 if reject_self else 0, float(self_min_clearance)))

    def exact_collision(self) -> Tuple[bool, bool, float]:
        """-> (on, reject_self, self_min_clearance) in force on this engine."""
        on, rs, mc = C.c_int(0), C.c_int(0), C.c_float(0.0)
        self._ck(self.lib.ikf_get_exact_collision(self._h, C.byref(on), C.byref(rs), C.byref(mc)))
        return bool(on.value), bool(rs.value), float(mc.value)

    def exact_collision_rejected(self) -> List[int]:
        """Per retry round of this engine's last exact call: rows that had a candidate and were rejected (zeros for rounds that did not run and
        for a call with the rule off or nothing to test against).  Waits for that call."""
        rows = (C.c_int64 * _lib.IKF_MAX_ROUNDS)()
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_exact_collision_rejected(self._h, rows))
        return [int(v) for v in rows]

    # -- best-of-K ranking (include/ikflow_amd_rank.h) -----------------------------------------------------
    @property
    def has_collision_model(self) -> bool:
        return bool(getattr(self, "_has_collision_model", False))

    def rank_chunks(self, n_poses: int, k: int) -> int:
        """K-chunks a ranking call of that shape is split into on this device (1: one launch writes the results)."""
        return int(self.lib.ikf_rank_chunks(self._h, int(n_poses), int(k)))

    def reserve_ranked(self, max_poses: int, max_k: int) -> None:
        """Pre-size what generate_ranked needs for up to max_poses x max_k candidates, so that later calls allocate nothing."""
        self._ck(self.lib.ikf_reserve_ranked(self._h, int(max_poses), int(max_k)))

    @staticmethod
    def rank_options(n_keep: int = 1, rot_weight: float = 0.01, ref_weight: float = 0.0, max_pos_err: Optional[float] = None,
                     max_rot_err: Optional[float] = None, reject_limits: bool = True, reject_collisions: bool = False,
                     min_clearance: float = 0.0) -> "_lib.ikf_rank_options":
        return _lib.ikf_rank_options(n_keep=int(n_keep), ref_weight=float(ref_weight), **_scoring_fields(
            rot_weight, max_pos_err, max_rot_err, reject_limits, reject_collisions, min_clearance))

    def _rank_outputs(self, m: int, k: int, n_keep: int, row_scores: bool):
        q_out = torch.empty((m, n_keep, self.layout.ndof), dtype=torch.float32, device=self.device)
        score = torch.empty((m, n_keep), dtype=torch.float32, device=self.device)
        index = torch.empty((m, n_keep), dtype=torch.int32, device=self.device)
        count = torch.empty((m,), dtype=torch.int32, device=self.device)
        rows = torch.empty((k * m,), dtype=torch.float32, device=self.device) if row_scores else None
        return q_out, score, index, count, rows

    def _candidate_inputs(self, target_poses: torch.Tensor, k: int, rows: torch.Tensor, cols: int, what: str, opt, max_k: Optional[int],
                          max_keep: int, extra: Optional[torch.Tensor], extra_name: str, per_pose: bool):
        """What rank_candidates / generate_ranked and diverse_select / generate_diverse check alike: the poses, k against the family's limit
        (None: none), the tile-major rows, the family's optional tensor (q_ref per pose, joint_weights per joint) and n_keep."""
        tp = self._on_device(target_poses, "target_poses")
        assert tp.ndim == 2 and tp.shape[1] == 7, f"target_poses must be of shape [m x 7], got {tuple(tp.shape)}"
        assert max_k is None or 1 <= k <= max_k, f"k must be in 1 .. {max_k}, got {k}"
        m = tp.shape[0]
        rows = self._on_device(rows, what)
        assert rows.ndim == 2 and rows.shape == (k * m, cols), f"{what} must be [{k * m} x {cols}] (tile-major), got {tuple(rows.shape)}"
        if extra is not None:
            extra = self._on_device(extra, extra_name)
            shape = (m, self.layout.ndof) if per_pose else (self.layout.ndof,)
            assert extra.shape == shape, f"{extra_name} must be [{' x '.join(map(str, shape))}], got {tuple(extra.shape)}"
        assert 1 <= opt.n_keep <= min(k, max_keep), f"n_keep must be in 1 .. min(k, {max_keep}), got {opt.n_keep}"
        return tp, m, rows, extra

    def _rank_inputs(self, target_poses: torch.Tensor, k: int, rows: torch.Tensor, cols: int, q_ref: Optional[torch.Tensor], opt, what: str):
        return self._candidate_inputs(target_poses, k, rows, cols, what, opt, None, _lib.IKF_RANK_MAX_KEEP, q_ref, "q_ref", True)

    def rank_candidates(self, target_poses: torch.Tensor, k: int, q: torch.Tensor, opt, q_ref: Optional[torch.Tensor] = None,
                        row_scores: bool = False):
        """target_poses [m x 7]; q [k * m x ndof] tile-major (row r * m + j = candidate r of pose j); opt: rank_options(...)
        -> (q_out [m x n_keep x ndof], scores [m x n_keep], repeat_index [m x n_keep] int32, n_admissible [m] int32, row_scores [k * m] or None)."""
        tp, m, q, q_ref = self._rank_inputs(target_poses, k, q, self.layout.ndof, q_ref, opt, "q")
        outs = self._rank_outputs(m, k, opt.n_keep, row_scores)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_rank_candidates(
                self._h, tp.data_ptr(), m, int(k), q.data_ptr(), None if q_ref is None else q_ref.data_ptr(), C.byref(opt),
                *[None if t is None else t.data_ptr() for t in outs], self._stream()))
        return outs

    def generate_ranked(self, target_poses: torch.Tensor, k: int, latent: torch.Tensor, clamp: bool, opt,
                        q_ref: Optional[torch.Tensor] = None, row_scores: bool = False):
        """The flow on latent [k * m x D] (tile-major, pose j for row r * m + j) and the ranking of its samples, without a host round trip
        in between; same outputs as rank_candidates."""
        tp, m, latent, q_ref = self._rank_inputs(target_poses, k, latent, self.layout.dim, q_ref, opt, "latent")
        outs = self._rank_outputs(m, k, opt.n_keep, row_scores)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_generate_ranked(
                self._h, tp.data_ptr(), m, int(k), latent.data_ptr(), 1 if clamp else 0, None if q_ref is None else q_ref.data_ptr(),
                C.byref(opt), *[None if t is None else t.data_ptr() for t in outs], self._stream()))
        return outs

    # -- path IK (include/ikflow_amd_path.h) --------------------------------------------------------------
    def reserve_path(self, max_waypoints: int, max_k: int) -> None:
        """Pre-size what generate_path needs for up to max_waypoints x max_k candidates, so that later calls allocate nothing."""
        self._ck(self.lib.ikf_reserve_path(self._h, int(max_waypoints), int(max_k)))

    @staticmethod
    def path_options(rot_weight: float = 0.01, max_pos_err: Optional[float] = None, max_rot_err: Optional[float] = None,
                     reject_limits: bool = True, reject_collisions: bool = False, min_clearance: float = 0.0, node_weight: float = 1.0,
                     max_joint_step: Optional[float] = None) -> "_lib.ikf_path_options":
        return _lib.ikf_path_options(
            node_weight=float(node_weight), max_joint_step=-1.0 if max_joint_step is None else float(max_joint_step),
            **_scoring_fields(rot_weight, max_pos_err, max_rot_err, reject_limits, reject_collisions, min_clearance))

    def _path_inputs(self, waypoints: torch.Tensor, k: int, rows: torch.Tensor, shared: bool, cols: int, q_start: Optional[torch.Tensor], what: str):
        wp = self._on_device(waypoints, "waypoints")
        assert wp.ndim == 2 and wp.shape[1] == 7, f"waypoints must be of shape [T x 7], got {tuple(wp.shape)}"
        assert 1 <= k <= _lib.IKF_PATH_MAX_K, f"k must be in 1 .. {_lib.IKF_PATH_MAX_K}, got {k}"
        T = wp.shape[0]
        rows = self._on_device(rows, what)
        n_rows = k if shared else k * T
        assert rows.ndim == 2 and rows.shape == (n_rows, cols), f"{what} must be [{n_rows} x {cols}], got {tuple(rows.shape)}"
        if q_start is not None:
            q_start = self._on_device(q_start, "q_start")
            assert q_start.shape == (self.layout.ndof,), f"q_start must be [{self.layout.ndof}], got {tuple(q_start.shape)}"
        return wp, T, rows, q_start

    def _path_outputs(self, T: int, k: int, node_costs: bool):
        path = torch.empty((T, self.layout.ndof), dtype=torch.float32, device=self.device)
        index = torch.empty((T,), dtype=torch.int32, device=self.device)
        cost = torch.full((1,), float("inf"), dtype=torch.float32, device=self.device)   # (T = 0: the call writes nothing)
        reach = torch.empty((T,), dtype=torch.int32, device=self.device)
        nodes = torch.empty((k * T,), dtype=torch.float32, device=self.device) if node_costs else None
        return path, index, cost, reach, nodes

    def path_search(self, waypoints: torch.Tensor, k: int, q: torch.Tensor, opt, q_start: Optional[torch.Tensor] = None, node_costs: bool = False):
        """waypoints [T x 7]; q [k * T x ndof] tile-major (row r * T + t = candidate r of waypoint t); opt: path_options(...)
        -> (path [T x ndof], index [T] int32, cost [1], n_reachable [T] int32, node_costs [k * T] or None)."""
        wp, T, q, q_start = self._path_inputs(waypoints, k, q, False, self.layout.ndof, q_start, "q")
        outs = self._path_outputs(T, k, node_costs)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_path_search(
                self._h, wp.data_ptr(), T, int(k), q.data_ptr(), None if q_start is None else q_start.data_ptr(), C.byref(opt),
                *[None if t is None else t.data_ptr() for t in outs], self._stream()))
        return outs

    def generate_path(self, waypoints: torch.Tensor, k: int, latent: torch.Tensor, shared_latent: bool, clamp: bool, opt,
                      q_start: Optional[torch.Tensor] = None, node_costs: bool = False):
        """The flow on k candidates per waypoint - latent [k x D] held fixed along the path (shared_latent), or [k * T x D] tile-major - and
        the search through them, without a host round trip in between; same outputs as path_search."""
        wp, T, latent, q_start = self._path_inputs(waypoints, k, latent, bool(shared_latent), self.layout.dim, q_start, "latent")
        outs = self._path_outputs(T, k, node_costs)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_generate_path(
                self._h, wp.data_ptr(), T, int(k), latent.data_ptr(), 1 if shared_latent else 0, 1 if clamp else 0,
                None if q_start is None else q_start.data_ptr(), C.byref(opt), *[None if t is None else t.data_ptr() for t in outs], self._stream()))
        return outs

    # -- path IK, P paths per call (include/ikflow_amd_path_batch.h) ---------------------------------------
    def reserve_path_batch(self, max_paths: int, max_waypoints: int, max_k: int) -> None:
        """Pre-size what generate_paths needs for up to max_paths x max_waypoints x max_k candidates, so that later calls allocate nothing."""
        self._ck(self.lib.ikf_reserve_path_batch(self._h, int(max_paths), int(max_waypoints), int(max_k)))

    def _path_batch_inputs(self, waypoints: torch.Tensor, k: int, rows: torch.Tensor, shared: bool, cols: int, q_start: Optional[torch.Tensor], what: str):
        wp = self._on_device(waypoints, "waypoints")
        assert wp.ndim == 3 and wp.shape[2] == 7, f"waypoints must be of shape [P x T x 7], got {tuple(wp.shape)}"
        assert 1 <= k <= _lib.IKF_PATH_MAX_K, f"k must be in 1 .. {_lib.IKF_PATH_MAX_K}, got {k}"
        P, T = wp.shape[0], wp.shape[1]
        rows = self._on_device(rows, what)
        n_rows = k if shared else k * P * T
        assert rows.ndim == 2 and rows.shape == (n_rows, cols), f"{what} must be [{n_rows} x {cols}], got {tuple(rows.shape)}"
        if q_start is not None:
            q_start = self._on_device(q_start, "q_start")
            assert q_start.shape == (P, self.layout.ndof), f"q_start must be [{P} x {self.layout.ndof}], got {tuple(q_start.shape)}"
        return wp, P, T, rows, q_start

    def _path_batch_outputs(self, P: int, T: int, k: int, node_costs: bool):
        paths = torch.empty((P, T, self.layout.ndof), dtype=torch.float32, device=self.device)
        index = torch.empty((P, T), dtype=torch.int32, device=self.device)
        cost = torch.full((P,), float("inf"), dtype=torch.float32, device=self.device)   # (T = 0: the call writes nothing)
        reach = torch.empty((P, T), dtype=torch.int32, device=self.device)
        nodes = torch.empty((k, P, T), dtype=torch.float32, device=self.device) if node_costs else None
        return paths, index, cost, reach, nodes

    def path_search_batch(self, waypoints: torch.Tensor, k: int, q: torch.Tensor, opt, q_start: Optional[torch.Tensor] = None,
                          node_costs: bool = False):
        """waypoints [P x T x 7]; q [k * P * T x ndof] (row r * (P * T) + p * T + t = candidate r of waypoint t of path p); q_start [P x ndof];
        opt: path_options(...).  Path p is path_search on its own lattice
        -> (paths [P x T x ndof], index [P x T] int32, cost [P], n_reachable [P x T] int32, node_costs [k x P x T] or None)."""
        wp, P, T, q, q_start = self._path_batch_inputs(waypoints, k, q, False, self.layout.ndof, q_start, "q")
        outs = self._path_batch_outputs(P, T, k, node_costs)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_path_search_batch(
                self._h, wp.data_ptr(), P, T, int(k), q.data_ptr(), None if q_start is None else q_start.data_ptr(), C.byref(opt),
                *[None if t is None else t.data_ptr() for t in outs], self._stream()))
        return outs

    def generate_paths(self, waypoints: torch.Tensor, k: int, latent: torch.Tensor, shared_latent: bool, clamp: bool, opt,
                       q_start: Optional[torch.Tensor] = None, node_costs: bool = False):
        """The flow on k candidates per waypoint of P paths - latent [k x D] held fixed along every path (shared_latent), or [k * P * T x D] in
        the candidate layout - and the P searches through them, without a host round trip in between; same outputs as path_search_batch."""
        wp, P, T, latent, q_start = self._path_batch_inputs(waypoints, k, latent, bool(shared_latent), self.layout.dim, q_start, "latent")
        outs = self._path_batch_outputs(P, T, k, node_costs)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_generate_path_batch(
                self._h, wp.data_ptr(), P, T, int(k), latent.data_ptr(), 1 if shared_latent else 0, 1 if clamp else 0,
                None if q_start is None else q_start.data_ptr(), C.byref(opt), *[None if t is None else t.data_ptr() for t in outs], self._stream()))
        return outs

    # -- path IK, third stage: the path optimiser (include/ikflow_amd_path_opt.h) ---------------------------
    def reserve_path_opt(self, max_paths: int, max_waypoints: int) -> None:
        """Pre-size what path_optimize / path_cost need for up to max_paths x max_waypoints, so that later calls allocate nothing."""
        self._ck(self.lib.ikf_reserve_path_opt(self._h, int(max_paths), int(max_waypoints)))

    def set_path_optimize(self, n_iters: int, smooth_weight: float = 0.0) -> None:
        """n_iters > 0: path_search, generate_path and their batch forms run the optimiser (validate = 1) behind the lattice.  0: off (the default)."""
        self._ck(self.lib.ikf_set_path_optimize(self._h, int(n_iters), float(smooth_weight)))

    def path_optimize_state(self) -> Tuple[int, float]:
        n, w = C.c_int(0), C.c_float(0.0)
        self._ck(self.lib.ikf_get_path_optimize(self._h, C.byref(n), C.byref(w)))
        return n.value, w.value

    def _path_opt_inputs(self, waypoints: torch.Tensor, path: torch.Tensor, q_start: Optional[torch.Tensor]):
        wp = self._on_device(waypoints, "waypoints")
        assert wp.ndim == 3 and wp.shape[2] == 7, f"waypoints must be of shape [P x T x 7], got {tuple(wp.shape)}"
        P, T = wp.shape[0], wp.shape[1]
        path = self._on_device(path, "path")
        assert path.shape == (P, T, self.layout.ndof), f"path must be [{P} x {T} x {self.layout.ndof}], got {tuple(path.shape)}"
        if q_start is not None:
            q_start = self._on_device(q_start, "q_start")
            assert q_start.shape == (P, self.layout.ndof), f"q_start must be [{P} x {self.layout.ndof}], got {tuple(q_start.shape)}"
        return wp, P, T, path, q_start

    def path_optimize(self, waypoints: torch.Tensor, path: torch.Tensor, opt, n_iters: int, smooth_weight: float, validate: bool = True,
                      q_start: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
        """waypoints [P x T x 7]; path [P x T x ndof]; q_start [P x ndof]; opt: path_options(...); out: where the result goes (may be `path`)
        -> (paths [P x T x ndof], cost [P], info [P x 4] int32 = iters, committed, reason, where)."""
        wp, P, T, path, q_start = self._path_opt_inputs(waypoints, path, q_start)
        if out is None:
            out = torch.empty_like(path)
        assert out.is_contiguous() and out.shape == path.shape and out.dtype == torch.float32 and out.device == path.device, "out must be like path"
        cost = torch.full((P,), float("inf"), dtype=torch.float32, device=self.device)   # (P * T = 0: the call writes nothing)
        info = torch.zeros((P, 4), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_path_optimize(
                self._h, wp.data_ptr(), P, T, path.data_ptr(), None if q_start is None else q_start.data_ptr(), C.byref(opt), int(n_iters),
                float(smooth_weight), 1 if validate else 0, out.data_ptr(), cost.data_ptr(), info.data_ptr(), self._stream()))
        return out, cost, info

    def path_cost(self, waypoints: torch.Tensor, path: torch.Tensor, opt, q_start: Optional[torch.Tensor] = None):
        """The evaluator alone: the lattice's cost of one row per waypoint -> (cost [P], info [P x 4] int32 = 0, admissible, reason, where)."""
        wp, P, T, path, q_start = self._path_opt_inputs(waypoints, path, q_start)
        cost = torch.full((P,), float("inf"), dtype=torch.float32, device=self.device)
        info = torch.zeros((P, 4), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_path_cost(self._h, wp.data_ptr(), P, T, path.data_ptr(), None if q_start is None else q_start.data_ptr(), C.byref(opt),
                                            cost.data_ptr(), info.data_ptr(), self._stream()))
        return cost, info

    def path_optimize_info(self, n_paths: int) -> np.ndarray:
        """[n_paths x 4] int32 info words of the handle's last optimising call (waits for it)."""
        out = np.zeros((int(n_paths), 4), np.int32)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_path_optimize_info(self._h, int(n_paths), out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    # -- diverse-of-K IK (include/ikflow_amd_diverse.h) ---------------------------------------------------
    def reserve_diverse(self, max_poses: int, max_k: int) -> None:
        """Pre-size what generate_diverse needs for up to max_poses x max_k candidates, so that later calls allocate nothing."""
        self._ck(self.lib.ikf_reserve_diverse(self._h, int(max_poses), int(max_k)))

    @staticmethod
    def diverse_options(n_keep: int = 1, rot_weight: float = 0.01, max_pos_err: Optional[float] = None, max_rot_err: Optional[float] = None,
                        reject_limits: bool = True, reject_collisions: bool = False, min_clearance: float = 0.0,
                        min_separation: float = 0.0) -> "_lib.ikf_diverse_options":
        return _lib.ikf_diverse_options(n_keep=int(n_keep), min_separation=float(min_separation), **_scoring_fields(
            rot_weight, max_pos_err, max_rot_err, reject_limits, reject_collisions, min_clearance))

    def _diverse_inputs(self, target_poses: torch.Tensor, k: int, rows: torch.Tensor, cols: int, joint_weights: Optional[torch.Tensor], opt, what: str):
        return self._candidate_inputs(target_poses, k, rows, cols, what, opt, _lib.IKF_DIVERSE_MAX_K, _lib.IKF_DIVERSE_MAX_KEEP, joint_weights,
                                      "joint_weights", False)

    def _diverse_outputs(self, m: int, k: int, n_keep: int, row_scores: bool):
        q_out = torch.empty((m, n_keep, self.layout.ndof), dtype=torch.float32, device=self.device)
        score = torch.empty((m, n_keep), dtype=torch.float32, device=self.device)
        index = torch.empty((m, n_keep), dtype=torch.int32, device=self.device)
        sep = torch.empty((m, n_keep), dtype=torch.float32, device=self.device)
        kept = torch.empty((m,), dtype=torch.int32, device=self.device)
        count = torch.empty((m,), dtype=torch.int32, device=self.device)
        rows = torch.empty((k * m,), dtype=torch.float32, device=self.device) if row_scores else None
        return q_out, score, index, sep, kept, count, rows

    def diverse_select(self, target_poses: torch.Tensor, k: int, q: torch.Tensor, opt, joint_weights: Optional[torch.Tensor] = None,
                       row_scores: bool = False):
        """target_poses [m x 7]; q [k * m x ndof] tile-major (row r * m + j = candidate r of pose j); opt: diverse_options(...); joint_weights
        [ndof], every one finite and >= 0 (the caller's contract) -> (q_out [m x n_keep x ndof], scores [m x n_keep], repeat_index [m x n_keep] int32,
        separation [m x n_keep], n_kept [m] int32, n_admissible [m] int32, row_scores [k * m] or None)."""
        tp, m, q, w = self._diverse_inputs(target_poses, k, q, self.layout.ndof, joint_weights, opt, "q")
        outs = self._diverse_outputs(m, k, opt.n_keep, row_scores)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_diverse_select(
                self._h, tp.data_ptr(), m, int(k), q.data_ptr(), None if w is None else w.data_ptr(), C.byref(opt),
                *[None if t is None else t.data_ptr() for t in outs], self._stream()))
        return outs

    def generate_diverse(self, target_poses: torch.Tensor, k: int, latent: torch.Tensor, clamp: bool, opt,
                         joint_weights: Optional[torch.Tensor] = None, row_scores: bool = False):
        """The flow on latent [k * m x D] (tile-major, pose j for row r * m + j) and the farthest-point selection among its samples, without a
        host round trip in between; same outputs as diverse_select."""
        tp, m, latent, w = self._diverse_inputs(target_poses, k, latent, self.layout.dim, joint_weights, opt, "latent")
        outs = self._diverse_outputs(m, k, opt.n_keep, row_scores)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_generate_diverse(
                self._h, tp.data_ptr(), m, int(k), latent.data_ptr(), 1 if clamp else 0, None if w is None else w.data_ptr(),
                C.byref(opt), *[None if t is None else t.data_ptr() for t in outs], self._stream()))
        return outs

    # -- exact IK ------------------------------------------------------------------------------------
    def generate_exact(
        self,
        target_poses: torch.Tensor,
        repeat_counts: Sequence[int],
        pos_error_threshold: float,
        rot_error_threshold: float,
        latents: Optional[Sequence[torch.Tensor]] = None,
        n_lm_steps: int = 3,
        return_stats: bool = False,
        seed_fn=None,
    ):
        """Returns (solutions [n x ndof] f32, valids [n] bool) (+ stats [rounds x 4] if asked).

        ``latents``: optional per-round latent tensors ([>= n_r*R_r x D], tile-major) for parity runs; when None each
        round draws ``torch.randn((n_tiled, D), device=...)`` exactly like draw_latent() (ikflow_solver.py:187).
        ``seed_fn(round, active_idx [n_active] int64 device tensor, repeat) -> [n_active * repeat x ndof]``: parity runs with
        the flow taken out (ikf_generate_exact_seeded) - the returned seeds replace the flow's output of that round."""
        tp = self._on_device(target_poses, "target_poses")
        assert tp.ndim == 2 and tp.shape[1] == 7, f"target_poses must be of shape [n x 7], got {tuple(tp.shape)}"
        n = tp.shape[0]
        D = self.layout.dim
        nr = len(repeat_counts)
        sols = torch.empty((n, self.layout.ndof), dtype=torch.float32, device=self.device)
        valid = torch.empty(n, dtype=torch.uint8, device=self.device)
        keep: List[torch.Tensor] = []
        err: List[BaseException] = []

        def _latent_cb(_user, rnd, rows, dim):
            try:
                if latents is not None:
                    lt = self._on_device(latents[rnd], f"latents[{rnd}]")
                    assert lt.ndim == 2 and lt.shape[1] == dim and lt.shape[0] >= rows, (
                        f"latents[{rnd}] must be at least [{rows} x {dim}], got {tuple(lt.shape)}"
                    )
                else:
                    lt = 1.0 * torch.randn((rows, dim), device=self.device)
                keep.append(lt)
                return lt.data_ptr()
            except BaseException as e:  # never let an exception cross the C boundary
                err.append(e)
                return 0

        def _seed_cb(_user, rnd, n_active, repeat, _d_idx, ndof):
            try:
                # the still-unsolved poses, ascending: the same list the engine built (its stream is idle here)
                idx = torch.arange(n, device=self.device) if rnd == 0 else torch.nonzero(valid == 0)[:, 0]
                assert idx.numel() == n_active, (idx.numel(), n_active)
                sq = self._on_device(seed_fn(rnd, idx, repeat), f"seeds of round {rnd}")
                assert sq.shape == (n_active * repeat, ndof), f"seeds of round {rnd} must be [{n_active * repeat} x {ndof}], got {tuple(sq.shape)}"
                keep.append(sq)
                return sq.data_ptr()  # produced on the stream the engine enqueues its copy on: ordered
            except BaseException as e:
                err.append(e)
                return 0

        rc = (C.c_int32 * nr)(*[int(r) for r in repeat_counts])
        stats = (C.c_int64 * (4 * nr))()
        with torch.cuda.device(self.device):
            if seed_fn is not None:
                cb = _lib.SEED_FN(_seed_cb)
                code = self.lib.ikf_generate_exact_seeded(
                    self._h, tp.data_ptr(), n, rc, nr, int(n_lm_steps), float(pos_error_threshold),
                    float(rot_error_threshold), cb, None, sols.data_ptr(), valid.data_ptr(),
                    stats if return_stats else None, self._stream(),
                )
            else:
                cb = _lib.LATENT_FN(_latent_cb)
                code = self.lib.ikf_generate_exact(
                    self._h, tp.data_ptr(), n, rc, nr, int(n_lm_steps), float(pos_error_threshold),
                    float(rot_error_threshold), cb, None, sols.data_ptr(), valid.data_ptr(),
                    stats if return_stats else None, self._stream(),
                )
        if err:
            raise err[0]
        self._ck(code)
        # latents must outlive the enqueued kernels
        if keep:
            torch.cuda.current_stream(self.device).synchronize()
        out = (sols, valid.to(torch.bool))
        if return_stats:
            return out + (np.array(list(stats), dtype=np.int64).reshape(nr, 4),)
        return out

    def refine_exact(self, target_poses: torch.Tensor, seeds_q: torch.Tensor, repeat: int, pos_error_threshold: float,
                     rot_error_threshold: float, n_lm_steps: int = 3) -> Tuple[torch.Tensor, torch.Tensor]:
        """One round of _generate_exact_ik_solutions (ikflow_solver.py:119-247) given its flow output: seeds_q
        [n * repeat x ndof] tile-major -> (solutions [n x ndof], valids [n] bool)."""
        tp = self._on_device(target_poses, "target_poses")
        sq = self._q(seeds_q)
        n = tp.shape[0]
        assert tp.ndim == 2 and tp.shape[1] == 7 and sq.shape[0] == n * repeat, (tuple(tp.shape), tuple(sq.shape), repeat)
        sols = torch.empty((n, self.layout.ndof), dtype=torch.float32, device=self.device)
        valid = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._ck(self.lib.ikf_refine_exact(self._h, tp.data_ptr(), n, int(repeat), sq.data_ptr(), int(n_lm_steps),
                                         float(pos_error_threshold), float(rot_error_threshold), sols.data_ptr(),
                                         valid.data_ptr(), self._stream()))
        return sols, valid.to(torch.bool)

    # -- measurement ---------------------------------------------------------------------------------
    def time_gemm(self, rows: int, iters: int) -> float:
        ms = C.c_float(0.0)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_time_gemm(self._h, int(rows), int(iters), C.byref(ms), self._stream()))
        return float(ms.value)

    def profile_begin(self) -> None:
        self._ck(self.lib.ikf_profile_begin(self._h))

    def profile_end(self):
        """-> (number of dominant-kernel launches since profile_begin, sum of their HIP-event durations in ms)"""
        n, ms = C.c_int64(0), C.c_double(0.0)
        with torch.cuda.device(self.device):
            self._ck(self.lib.ikf_profile_end(self._h, C.byref(n), C.byref(ms), self._stream()))
        self.last_event_overhead_ms = float(self.lib.ikf_profile_event_overhead_ms(self._h))
        return int(n.value), float(ms.value)

    def plan(self, rows: int) -> str:
        """The chunks a call of `rows` rows is cut into, e.g. "rowowner:4096 cluster16:200" (DESIGN.md section 4.3)."""
        buf = C.create_string_buffer(256)
        self._ck(self.lib.ikf_plan_describe(self._h, int(rows), buf, 256))
        return buf.value.decode()

    @property
    def cluster_local(self) -> bool:
        """Cluster launches with 4 / 8 / 16 members hand over through one XCD's L2 (placement census at load + a check in every launch)."""
        return bool(self.lib.ikf_cluster_local(self._h))

    @property
    def cluster_repairs(self) -> int:
        """Calls whose cluster-form launch gave up waiting for a peer workgroup (recomputed by the repair launch; the form then sits out
        `cluster_backoff` calls and is tried again)."""
        return int(self.lib.ikf_cluster_repairs(self._h))

    @property
    def cluster_backoff(self) -> int:
        """Calls the cluster form still sits out after a give-up (16 after the first, doubling up to 65536; 0: in use)."""
        return int(self.lib.ikf_cluster_backoff(self._h))

    @property
    def load_time_ms(self) -> float:
        """Host wall time of the last ikf_load_weights on this handle (packing, upload, device-side images of the resident-row forms)."""
        return float(self.lib.ikf_load_time_ms(self._h))

    @property
    def frag_image_time_ms(self) -> float:
        """... of building the small-batch per-layer kernels' weight image (0 until a <= 512-row chunk on that path or ikf_reserve needed it)."""
        return float(self.lib.ikf_frag_image_time_ms(self._h))

    def dominant_kernel_name(self, rows: Optional[int] = None) -> str:
        """Name (as in a rocprofv3 kernel trace) of the kernel that carries a batch of `rows` rows; None: the per-layer contraction."""
        if rows is not None:
            return self.lib.ikf_dominant_kernel_for(self._h, int(rows)).decode()
        if self.precision == "f16x3":
            return self.lib.ikf_split_kernel_name().decode()
        return self.lib.ikf_dominant_kernel_name().decode()


# ---------------------------------------------------------------------------------------------------
# kinematics-only engines for Robot.forward_kinematics & co (no flow weights needed)
# ---------------------------------------------------------------------------------------------------
_KIN_CACHE: Dict[Tuple, Engine] = {}


def _robot_key(robot: Robot) -> Tuple:
    """Two robots share an engine only when their chains and limits are the same, whatever their names."""
    return (robot.name, tuple((j.kind, j.origin_xyz, j.origin_rpy, j.axis, j.limits) for j in robot.joints))


def kinematics_engine_for(robot: Robot, device=None) -> Engine:
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if not torch.cuda.is_available():
        raise EngineError("no GPU visible: ikflow_amd kinematics run on the MI355X only (there is no CPU path)")
    key = (_robot_key(robot), _dev_index(dev))
    if key not in _KIN_CACHE:
        lay = FlowLayout(nb_nodes=1, dim=max(robot.ndof, 2), dim_cond=8, width=256, n_hidden=1, clamp=2.5, ndof=robot.ndof)
        _KIN_CACHE[key] = Engine(lay, robot, dev)
    return _KIN_CACHE[key]
