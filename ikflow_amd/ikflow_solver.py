"""IKFlowSolver - drop-in for ``ikflow.ikflow_solver.IKFlowSolver`` (ikflow/ikflow_solver.py:32-441) whose compute runs on
the MI355X engine (libikflow_amd.so) instead of FrEIA / jrl / torch ops.

Same method names, argument meaning, return shapes/dtypes and assertion behaviour as the reference:
  generate_ik_solutions        ikflow_solver.py:254-343
  generate_exact_ik_solutions  ikflow_solver.py:345-411
  load_state_dict              ikflow_solver.py:413-441
  _run_inference / _calculate_pose_error   ikflow_solver.py:85-117
Differences, all documented in DESIGN.md:
  * there is no ``nn_model`` torch module - weights live packed in HBM inside the engine;
  * ``compile_model`` is accepted and ignored (nothing to trace); ``run_lma_on_cpu`` is accepted and ignored
    (LM runs on the GPU, resident with the batch);
  * ``generate_exact_ik_solutions`` takes an optional ``latents=`` (one tensor per retry round) so that
    "identical (pose, latent)" parity is testable - the reference draws them internally (:187);
  * ``return_detailed=True`` returns ``None`` in the self-collision slot (Klampt check, SURVEY 8 f-3, out of scope).
"""
from __future__ import annotations

import math
import pickle
import warnings
from time import time
from typing import Dict, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ikflow_amd import config
from ikflow_amd.model import (
    IkflowModelParameters,
    layout_from,
    random_state_dict,
    state_dict_to_numpy,
    validate_state_dict,
)
from ikflow_amd.robots import Robot


def mm_to_m(x: float) -> float:
    return x / 1000.0


class RankedSolutions(NamedTuple):
    """What generate_ranked_ik_solutions returns (row_scores only with return_row_scores=True, else the 4-tuple RankedSolutions4)."""
    solutions: torch.Tensor      # [m x n_keep x ndof]; unfilled slots are 0
    scores: torch.Tensor         # [m x n_keep]; unfilled slots are +inf
    repeat_index: torch.Tensor   # [m x n_keep] int32; unfilled slots are -1
    n_admissible: torch.Tensor   # [m] int32
    row_scores: torch.Tensor     # [k * m], tile-major; +inf for an inadmissible candidate


class RankedSolutions4(NamedTuple):
    solutions: torch.Tensor
    scores: torch.Tensor
    repeat_index: torch.Tensor
    n_admissible: torch.Tensor


class PathSolution(NamedTuple):
    """What generate_ik_path returns (node_costs only with return_node_costs=True, else the 4-tuple PathSolution4)."""
    path: torch.Tensor           # [T x ndof]; all 0 when there is no path
    index: torch.Tensor          # [T] int32, the candidate chosen per waypoint; -1 when there is no path
    cost: torch.Tensor           # [] the total of the lattice; +inf when there is no path
    n_reachable: torch.Tensor    # [T] int32, candidates of a waypoint that some admissible path reaches
    node_costs: torch.Tensor     # [k * T], tile-major; +inf for an inadmissible candidate


class PathSolution4(NamedTuple):
    path: torch.Tensor
    index: torch.Tensor
    cost: torch.Tensor
    n_reachable: torch.Tensor


class PathsSolution(NamedTuple):
    """What generate_ik_paths returns (node_costs only with return_node_costs=True, else the 4-tuple PathsSolution4)."""
    paths: torch.Tensor          # [P x T x ndof]; a path that does not exist is all 0
    index: torch.Tensor          # [P x T] int32, the candidate chosen per waypoint; -1 along a path that does not exist
    cost: torch.Tensor           # [P] the totals of the lattices; +inf where there is no path
    n_reachable: torch.Tensor    # [P x T] int32, candidates of a waypoint that some admissible path of its lattice reaches
    node_costs: torch.Tensor     # [k x P x T]; +inf for an inadmissible candidate


class PathsSolution4(NamedTuple):
    paths: torch.Tensor
    index: torch.Tensor
    cost: torch.Tensor
    n_reachable: torch.Tensor


class PathOptimization(NamedTuple):
    """One path's entry of last_path_optimization() (include/ikflow_amd_path_opt.h)."""
    iters: int                   # steps kept
    committed: bool              # the optimised path was returned
    reason: str                  # "committed", "no step lowered F", "node inadmissible", "edge forbidden", "cost not lower"
    where: int                   # the first offending waypoint (for an edge: the waypoint it ends at), or -1


class DiverseSolutions(NamedTuple):
    """What generate_diverse_ik_solutions returns (row_scores only with return_row_scores=True, else the 6-tuple DiverseSolutions6)."""
    solutions: torch.Tensor      # [m x n_keep x ndof]; unfilled slots are 0
    scores: torch.Tensor         # [m x n_keep]; unfilled slots are +inf
    repeat_index: torch.Tensor   # [m x n_keep] int32; unfilled slots are -1
    separation: torch.Tensor     # [m x n_keep] distance to the nearest row kept before it; +inf in slot 0 and in unfilled slots
    n_kept: torch.Tensor         # [m] int32, slots filled
    n_admissible: torch.Tensor   # [m] int32
    row_scores: torch.Tensor     # [k * m], tile-major; +inf for an inadmissible candidate


class DiverseSolutions6(NamedTuple):
    solutions: torch.Tensor
    scores: torch.Tensor
    repeat_index: torch.Tensor
    separation: torch.Tensor
    n_kept: torch.Tensor
    n_admissible: torch.Tensor


def draw_latent(latent_distribution: str, latent_scale: float, shape: Tuple[int, int], device):
    """Draw a sample from the latent noise distribution (ikflow_solver.py:16-29; torch's global generator)."""
    assert latent_distribution in ["gaussian", "uniform"]
    assert latent_scale > 0
    assert len(shape) == 2
    if latent_distribution == "gaussian":
        return latent_scale * torch.randn(shape, device=device)
    if latent_distribution == "uniform":
        return 2 * latent_scale * torch.rand(shape, device=device) - latent_scale


class IKFlowSolver:
    def __init__(self, hyper_parameters: IkflowModelParameters, robot: Robot, compile_model: Optional[Dict] = None):
        """Initialize an IKFlowSolver (ikflow_solver.py:33-68)."""
        assert isinstance(
            hyper_parameters, IkflowModelParameters
        ), f"hyper_parameters should be a IkflowModelParameters type, is {type(hyper_parameters)}"
        assert isinstance(robot, Robot), f"robot should be a Robot type, is {type(robot)}"
        assert isinstance(compile_model, (type(None), dict))

        if not hasattr(hyper_parameters, "sigmoid_on_output"):
            hyper_parameters.sigmoid_on_output = False
        if hyper_parameters.softflow_enabled:
            assert not hyper_parameters.sigmoid_on_output, (
                "sigmoid_on_output and softflow are incompatible, disable one or the other"
            )
        self._robot = robot
        self.dim_cond = 7
        if hyper_parameters.softflow_enabled:
            self.dim_cond = 8  # [x, ... q3, softflow_scale]   (softflow_scale should be 0 for inference)
        self._network_width = hyper_parameters.dim_latent_space
        self._hyper_parameters = hyper_parameters
        self._layout = layout_from(hyper_parameters, robot)
        if compile_model is not None:
            warnings.warn("compile_model is ignored: the MI355X engine runs hand-written HIP kernels, nothing is traced.")
        self._model_weights_loaded = False
        self._engine = None  # created on first use, on the device of the inputs
        self._world = None   # (World, min_clearance) of set_world: re-applied to every engine this solver creates
        self._world_cloud = None  # (points [n x 3] host f32, point_radius, min_clearance) of set_world_cloud: likewise
        self._path_sweep = 0  # samples per lattice edge of set_path_sweep: likewise
        self._last_path_opt_paths = None  # paths of the last call that ran the path optimiser (last_path_optimization)
        self._path_optimization = (0, 0.0)  # (n_iters, smooth_weight) of set_path_optimization: likewise
        self._world_track = None  # (worlds, min_clearance) of set_world_track: likewise (pushed after the collision model, the world and the sweep)
        self._candidate_refine = (0, 0.0, 0.0)  # (n_steps, pos_tol, rot_tol) of set_candidate_refine: likewise
        self._exact_collision = (False, False, 0.0)  # (enabled, reject_self_collisions, min_clearance) of set_exact_collision: likewise
        self._min_manipulability = (0.0, "full")  # (floor, part) of set_min_manipulability: likewise
        # tests / tools only: "probes" binds lib/libikflow_amd_probes.so (the product + the priced-and-rejected forms of rounds 2 - 3);
        # set before the first call
        self.library_flavour = ""
        self._precision = "f32"
        self._state_dict_np: Optional[Dict[str, np.ndarray]] = None
        self.ndof = self.robot.ndof

    # -- properties (ikflow_solver.py:68-83) ---------------------------------------------------------
    @property
    def robot(self) -> Robot:
        return self._robot

    @property
    def network_width(self) -> int:
        return self._network_width

    @property
    def conditional_size(self) -> int:
        return self.dim_cond

    @property
    def layout(self):
        return self._layout

    # -- engine --------------------------------------------------------------------------------------
    def engine(self, device=None):
        """The C-ABI handle for `device` (created lazily; weights are uploaded when it is created)."""
        from ikflow_amd.engine import Engine  # imports the ctypes binding: fails loudly without the built library

        from ikflow_amd.engine import _dev_index

        device = torch.device(config.DEVICE if device is None else device)
        # an index-less "cuda" means torch's current device (what Engine resolves it to)
        if self._engine is None or self._engine.device != torch.device("cuda", _dev_index(device)):
            eng = Engine(self._layout, self._robot, device, self.library_flavour)
            if self._state_dict_np is not None:
                eng.load_state_dict(self._state_dict_np)
            if self._precision != "f32":
                try:
                    eng.set_precision(self._precision)
                except Exception:
                    # the engine refused the mode for these weights (e.g. a hidden weight beyond the f16 range) and stays
                    # on f32: the solver follows it, so solver and engine never disagree, and reports the refusal once
                    self._precision = "f32"
                    self._engine = eng
                    raise
            if self._world is not None:
                self._push_world(eng)
            if self._world_cloud is not None:
                self._push_world_cloud(eng)
            if self._path_sweep:
                eng.set_path_sweep(self._path_sweep)
            if self._world_track is not None:
                self._push_world_track(eng)
            if self._candidate_refine[0]:
                eng.set_candidate_refine(*self._candidate_refine)
            if self._path_optimization[0]:
                eng.set_path_optimize(*self._path_optimization)
            if self._min_manipulability[0]:
                eng.set_min_manipulability(*self._min_manipulability)
            if self._exact_collision[0]:   # (after the collision model, the world and the cloud)
                self._push_exact_collision(eng)
            self._engine = eng
        return self._engine

    # -- the caller's scene --------------------------------------------------------------------------
    def set_world(self, world, min_clearance: float = 0.0):
        """Obstacles of the scene (ikflow_amd.world.World; None or an empty one: no scene).  While a world is set,
        generate_ranked_ik_solutions, generate_ik_path and generate_diverse_ik_solutions also drop every candidate whose clearance from an
        obstacle is below min_clearance - whatever reject_self_collisions says, which keeps meaning the robot against itself.  Needs the
        robot's capsule model (Robot.set_collision_capsules)."""
        from ikflow_amd.world import World

        assert world is None or isinstance(world, World), f"world must be a ikflow_amd.world.World or None (got {type(world)})"
        assert isinstance(min_clearance, (int, float)) and math.isfinite(min_clearance), f"min_clearance must be a finite number, got {min_clearance!r}"
        if world is None or len(world) == 0:
            self._world = None
            if self._engine is not None:
                self._engine.clear_world()
            return
        assert self._robot.has_collision_model, "set_world needs a collision model (Robot.set_collision_capsules)"
        self._world = (world, float(min_clearance))
        if self._engine is not None:
            self._push_world(self._engine)
        else:
            self.engine()

    def _push_collision_model(self, eng):
        if getattr(eng, "_collision_source", None) is not self._robot._collision_model:
            eng.set_collision_model(*self._robot._collision_model)   # the solver's own handle, not the one Robot.config_self_collides uses
            eng._collision_source = self._robot._collision_model

    def _push_world(self, eng):
        self._push_collision_model(eng)
        eng.set_world(*self._world)

    def set_world_cloud(self, points, point_radius: float, min_clearance: float = 0.0):
        """The sensed scene as points ([n x 3], numpy or torch on any device, base frame; at most 2^20; None or an empty one: no cloud), each a
        sphere of point_radius.  While a cloud is set, generate_ranked_ik_solutions, generate_ik_path and generate_diverse_ik_solutions also drop
        every candidate whose clearance from a point is below min_clearance - whatever reject_self_collisions says, and beside a world of
        set_world.  The swept edges of set_path_sweep do not test the cloud.  Needs the robot's capsule model (Robot.set_collision_capsules)."""
        for name, v in (("point_radius", point_radius), ("min_clearance", min_clearance)):
            assert isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v), f"{name} must be a finite number, got {v!r}"
        assert point_radius >= 0, f"point_radius must be >= 0, got {point_radius!r}"
        if points is not None:
            if isinstance(points, torch.Tensor):
                points = points.detach().cpu().numpy()
            points = np.asarray(points)
            assert points.size == 0 or (points.ndim == 2 and points.shape[1] == 3), f"points must be [n x 3], got {tuple(points.shape)}"
            points = np.ascontiguousarray(points.reshape(-1, 3), dtype=np.float32)
            assert len(points) <= 1 << 20, f"a cloud holds at most {1 << 20} points, got {len(points)}"
            assert bool(np.isfinite(points).all()), "points must be finite"
        if points is None or len(points) == 0:
            self._world_cloud = None
            if self._engine is not None:
                self._engine.clear_world_cloud()
            return
        assert self._robot.has_collision_model, "set_world_cloud needs a collision model (Robot.set_collision_capsules)"
        self._world_cloud = (points, float(point_radius), float(min_clearance))
        if self._engine is not None:
            self._push_world_cloud(self._engine)
        else:
            self.engine()

    def _push_world_cloud(self, eng):
        self._push_collision_model(eng)
        eng.set_world_cloud(*self._world_cloud)

    def set_world_track(self, worlds, min_clearance: float = 0.0):
        """A scene that moves along the path: one ikflow_amd.world.World per waypoint of generate_ik_path (None or an empty sequence: no track),
        each holding the same obstacles - the same number, the same kinds in the same order; one that appears or disappears is moved far away.
        While a track is set, generate_ik_path also drops candidate r of waypoint t when it is closer than min_clearance to frame t and - under
        set_path_sweep - avoids every edge whose samples come closer than that to the frames interpolated between its two waypoints' frames
        (include/ikflow_amd_track.h).  A path of more waypoints than frames is refused.  Beside set_world and set_world_cloud, which stay in force;
        ranked and diverse IK do not read it.  Needs the robot's capsule model (Robot.set_collision_capsules)."""
        from ikflow_amd.world import World

        assert isinstance(min_clearance, (int, float)) and not isinstance(min_clearance, bool) and math.isfinite(min_clearance), (
            f"min_clearance must be a finite number, got {min_clearance!r}")
        if worlds is None or len(worlds) == 0:
            self._world_track = None
            if self._engine is not None:
                self._engine.clear_world_track()
            return
        worlds = list(worlds)
        assert all(isinstance(w, World) for w in worlds), "worlds must be a sequence of ikflow_amd.world.World"
        assert len(worlds) <= 1024, f"a world track holds at most 1024 frames, got {len(worlds)}"
        n = len(worlds[0])
        assert n >= 1, "frame 0 holds no obstacle"
        for t, w in enumerate(worlds):
            assert len(w) == n, f"frame {t} holds {len(w)} obstacles, frame 0 holds {n}"
            for o, (ob, ob0) in enumerate(zip(w.obstacles, worlds[0].obstacles)):
                assert ob[0] == ob0[0], f"frame {t} obstacle {o}: kind {ob[0]} differs from frame 0's kind {ob0[0]}"
        assert self._robot.has_collision_model, "set_world_track needs a collision model (Robot.set_collision_capsules)"
        self._world_track = (worlds, float(min_clearance))
        if self._engine is not None:
            self._push_world_track(self._engine)
        else:
            self.engine()

    def _push_world_track(self, eng):
        self._push_collision_model(eng)
        eng.set_world_track(*self._world_track)

    def set_path_sweep(self, n_samples: int):
        """Samples per edge of generate_ik_path's lattice (0: no sweep, the default; at most 16).  While set, the path also avoids every edge
        whose n_samples interpolated configurations - q_i = a + i / (n_samples + 1) * (b - a) - come closer to the world of set_world than its
        min_clearance or, with reject_self_collisions, to the robot itself than min_clearance (include/ikflow_amd_sweep.h).  Sampled, not
        conservative: cover the gap between two samples with min_clearance."""
        assert isinstance(n_samples, int) and not isinstance(n_samples, bool) and 0 <= n_samples <= 16, f"n_samples must be an int in 0 .. 16, got {n_samples!r}"
        self._path_sweep = n_samples
        if self._engine is not None:
            self._engine.set_path_sweep(n_samples)

    def set_path_optimization(self, n_iters: int, smooth_weight: float):
        """A least-squares pass over the whole path behind the lattice of generate_ik_path / generate_ik_paths (0 iterations: off, the default; at
        most 32): up to n_iters damped Gauss-Newton steps on  sum_t |pose error_t|^2 + smooth_weight * sum_t |q_t - q_{t-1}|^2  (with q_start as
        q_{-1}), all waypoints coupled, each step kept only if it lowers that sum (include/ikflow_amd_path_opt.h).  The optimised path is
        returned only when every rule of the lattice admits it - thresholds, limits, self-collision, world, cloud, manipulability floor, world
        track, step gate, sweep - and its cost BY THE LATTICE'S OWN COST is strictly lower; otherwise the lattice's path comes back unchanged.
        ``index``, ``n_reachable`` and ``node_costs`` keep describing the lattice; ``cost`` is that of the returned path; last_path_optimization()
        tells what happened.

        smooth_weight has no default.  It is the ratio at which squared joint motion (rad^2 per waypoint) trades against squared pose error
        (m^2 and rad^2): at smooth_weight = 1 a step of 0.03 rad between neighbours weighs as much as 3 cm of position error, at 0 every waypoint
        is polished on its own (one fp64 LM step per iteration) and the motion between them is left as the lattice chose it.  The right value
        depends on the waypoint spacing and on node_weight; none has been tuned here."""
        assert isinstance(n_iters, int) and not isinstance(n_iters, bool) and 0 <= n_iters <= 32, f"n_iters must be an int in 0 .. 32, got {n_iters!r}"
        assert isinstance(smooth_weight, (int, float)) and not isinstance(smooth_weight, bool) and math.isfinite(smooth_weight) and smooth_weight >= 0, (
            f"smooth_weight must be a finite number >= 0, got {smooth_weight!r}")
        self._path_optimization = (n_iters, float(smooth_weight)) if n_iters else (0, 0.0)
        if self._engine is not None:
            self._engine.set_path_optimize(*self._path_optimization)

    def last_path_optimization(self):
        """What the optimiser did in the last generate_ik_path / generate_ik_paths / optimize_ik_path call: one named tuple (iters, committed,
        reason, where) per path - steps kept, whether the optimised path was returned, why not ("committed", "no step lowered F", "node
        inadmissible", "edge forbidden", "cost not lower") and the first offending waypoint or -1.  None before any such call."""
        if self._engine is None or self._last_path_opt_paths is None:
            return None
        from ikflow_amd import _lib

        info = self._engine.path_optimize_info(self._last_path_opt_paths)
        return [PathOptimization(int(r[0]), bool(r[1]), _lib.PATH_OPT_REASONS[int(r[2])], int(r[3])) for r in info]

    def optimize_ik_path(
        self,
        waypoints: torch.Tensor,
        path: torch.Tensor,
        n_iters: int,
        smooth_weight: float,
        validate: bool = True,
        rot_weight: float = mm_to_m(1) / 0.1,
        node_weight: float = 1.0,
        max_joint_step: Optional[float] = None,
        q_start: Optional[torch.Tensor] = None,
        pos_error_threshold: Optional[float] = None,
        rot_error_threshold: Optional[float] = None,
        reject_joint_limits: bool = True,
        reject_self_collisions: Optional[bool] = None,
        min_clearance: float = 0.0,
    ):
        """The optimiser of set_path_optimization on the caller's own path(s): waypoints [T x 7] with path [T x ndof] (q_start [ndof]), or
        [P x T x 7] with [P x T x ndof] ([P x ndof]).  The rule keywords are generate_ik_path's and define the evaluator; with validate (the
        default) the result is never a path those rules forbid nor one that costs more than the input.  Needs no weights.
        Returns (path like the input, cost - a scalar for one path, [P] otherwise); last_path_optimization() has the details."""
        assert isinstance(waypoints, torch.Tensor) and isinstance(path, torch.Tensor), "waypoints and path must be torch.Tensors"
        single = waypoints.ndim == 2
        assert waypoints.ndim in (2, 3) and waypoints.shape[-1] == 7, f"waypoints must be of shape [T x 7] or [P x T x 7], got {tuple(waypoints.shape)}"
        assert tuple(path.shape) == tuple(waypoints.shape[:-1]) + (self.ndof,), (
            f"path must be {list(waypoints.shape[:-1]) + [self.ndof]}, got {list(path.shape)}")
        assert isinstance(n_iters, int) and not isinstance(n_iters, bool) and 1 <= n_iters <= 32, f"n_iters must be an int in 1 .. 32, got {n_iters!r}"
        assert isinstance(smooth_weight, (int, float)) and not isinstance(smooth_weight, bool) and math.isfinite(smooth_weight) and smooth_weight >= 0, (
            f"smooth_weight must be a finite number >= 0, got {smooth_weight!r}")
        want = (self.ndof,) if single else (waypoints.shape[0], self.ndof)
        assert q_start is None or (isinstance(q_start, torch.Tensor) and tuple(q_start.shape) == want), f"q_start must be {list(want)}"
        assert node_weight >= 0, f"node_weight must be >= 0, got {node_weight!r}"
        assert max_joint_step is None or max_joint_step >= 0, "max_joint_step must be None (no gate) or >= 0"
        assert pos_error_threshold is None or pos_error_threshold >= 0, "pos_error_threshold must be None (no bound) or >= 0"
        assert rot_error_threshold is None or rot_error_threshold >= 0, "rot_error_threshold must be None (no bound) or >= 0"
        if reject_self_collisions is None:
            reject_self_collisions = self._robot.has_collision_model
        assert not reject_self_collisions or self._robot.has_collision_model, "reject_self_collisions needs a collision model (Robot.set_collision_capsules)"
        with torch.inference_mode():
            eng = self.engine(waypoints.device)
            if reject_self_collisions and getattr(eng, "_collision_source", None) is not self._robot._collision_model:
                eng.set_collision_model(*self._robot._collision_model)
                eng._collision_source = self._robot._collision_model
            opt = eng.path_options(rot_weight, pos_error_threshold, rot_error_threshold, reject_joint_limits, reject_self_collisions, min_clearance,
                                   node_weight, max_joint_step)
            wp3, path3 = (waypoints[None], path[None]) if single else (waypoints, path)
            qs = None if q_start is None else (q_start[None] if single else q_start)
            out, cost, _ = eng.path_optimize(wp3, path3, opt, n_iters, smooth_weight, validate=validate, q_start=qs)
        self._last_path_opt_paths = wp3.shape[0] if wp3.shape[1] > 0 else 0
        return (out[0], cost.reshape(())) if single else (out, cost)

    def set_candidate_refine(self, n_steps: int, pos_tol: float = mm_to_m(1), rot_tol: float = 0.1):
        """Levenberg-Marquardt steps on EVERY candidate of generate_ranked_ik_solutions, generate_diverse_ik_solutions and generate_ik_path,
        between the flow and the scoring (0: none, the default; at most 16).  A candidate stops after the first step that leaves its pose error
        below both tolerances (the defaults are generate_exact_ik_solutions' thresholds; 0: never, all steps run; a rot_tol at or below 9.77e-4
        rad never stops one).  While set, every threshold, joint-limit, self-collision, world and swept-edge test, every score and distance and
        every returned row is that of the refined candidate (include/ikflow_amd_refine.h)."""
        assert isinstance(n_steps, int) and not isinstance(n_steps, bool) and 0 <= n_steps <= 16, f"n_steps must be an int in 0 .. 16, got {n_steps!r}"
        for name, tol in (("pos_tol", pos_tol), ("rot_tol", rot_tol)):
            assert isinstance(tol, (int, float)) and not isinstance(tol, bool) and math.isfinite(tol) and tol >= 0, (
                f"{name} must be a finite number >= 0, got {tol!r}")
        self._candidate_refine = (n_steps, float(pos_tol), float(rot_tol)) if n_steps else (0, 0.0, 0.0)
        if self._engine is not None:
            self._engine.set_candidate_refine(*self._candidate_refine)

    def set_min_manipulability(self, min_manipulability: float, part: str = "full"):
        """A floor under Yoshikawa's manipulability measure w = sqrt(det(J J^T)) of every candidate of generate_ranked_ik_solutions,
        generate_diverse_ik_solutions and generate_ik_path (0: no rule, the default): a candidate whose w is not >= the floor is inadmissible
        like one beyond a limit - a near-singular configuration reaches the pose but cannot be left without large joint velocities.  part:
        "full" (all six rows of the geometric Jacobian; mixes radians and metres), "linear" (rows 3-5) or "angular" (rows 0-2).  Under
        set_candidate_refine the refined candidate is tested.  generate_exact_ik_solutions and the swept edges of set_path_sweep do not obey
        the floor (include/ikflow_amd_manip.h)."""
        assert isinstance(min_manipulability, (int, float)) and not isinstance(min_manipulability, bool) and math.isfinite(min_manipulability) \
            and min_manipulability >= 0, f"min_manipulability must be a finite number >= 0, got {min_manipulability!r}"
        assert part in ("full", "linear", "angular"), f'part must be "full", "linear" or "angular", got {part!r}'
        self._min_manipulability = (float(min_manipulability), part)
        if self._engine is not None:
            self._engine.set_min_manipulability(*self._min_manipulability)

    def set_exact_collision(self, reject_self_collisions: bool = False, min_clearance: float = 0.0, enabled: bool = True):
        """Make generate_exact_ik_solutions obey the scene (off by default).  While enabled, a repeat whose solution - its configuration at the
        first LM iteration inside both error thresholds - is closer to the world of set_world or the cloud of set_world_cloud than their
        min_clearance, or, with reject_self_collisions, to the robot itself than min_clearance, does not count: the pose is solved by its
        earliest clear repeat, or falls through to the next round's larger repeat count (include/ikflow_amd_exact_world.h).  With nothing to
        test against - no world, no cloud, reject_self_collisions False - the call is the plain one bit for bit."""
        assert isinstance(enabled, bool), f"enabled must be a bool, got {enabled!r}"
        assert isinstance(reject_self_collisions, bool), f"reject_self_collisions must be a bool, got {reject_self_collisions!r}"
        assert isinstance(min_clearance, (int, float)) and not isinstance(min_clearance, bool) and math.isfinite(min_clearance), (
            f"min_clearance must be a finite number, got {min_clearance!r}")
        assert not (enabled and reject_self_collisions) or self._robot.has_collision_model, (
            "reject_self_collisions needs a collision model (Robot.set_collision_capsules)")
        self._exact_collision = (True, reject_self_collisions, float(min_clearance)) if enabled else (False, False, 0.0)
        if self._engine is not None:
            self._push_exact_collision(self._engine)

    def _push_exact_collision(self, eng):
        enabled, reject_self, min_clearance = self._exact_collision
        if enabled and reject_self:
            self._push_collision_model(eng)
        eng.set_exact_collision(enabled, reject_self, min_clearance)

    def path_collides(self, path: torch.Tensor, n_samples: int, reject_self: bool = False, min_clearance: float = 0.0) -> torch.Tensor:
        """The swept check of a joint-space path [T x ndof]: per edge path[t] -> path[t + 1], whether one of its n_samples interpolated
        configurations is closer to the world of set_world than its min_clearance or - reject_self - to the robot itself than min_clearance.
        -> [T - 1] bool.  The rows themselves are not tested (Robot.config_collides_with_env does that)."""
        assert isinstance(path, torch.Tensor) and path.ndim == 2 and path.shape[1] == self.ndof, f"path must be [T x {self.ndof}]"
        assert isinstance(n_samples, int) and 1 <= n_samples <= 16, f"n_samples must be an int in 1 .. 16, got {n_samples!r}"
        assert self._robot.has_collision_model, "path_collides needs a collision model (Robot.set_collision_capsules)"
        with torch.inference_mode():
            eng = self.engine(path.device)
            if getattr(eng, "_collision_source", None) is not self._robot._collision_model:
                eng.set_collision_model(*self._robot._collision_model)
                eng._collision_source = self._robot._collision_model
            if path.shape[0] < 2:
                return torch.zeros(0, dtype=torch.bool, device=path.device)
            rows = path.to(torch.float32).contiguous()
            return eng.sweep_edges(rows[:-1].contiguous(), rows[1:].contiguous(), n_samples, reject_self, min_clearance)[0]

    def timed_path_collides(self, path: torch.Tensor, q_start: Optional[torch.Tensor] = None, reject_self: bool = False,
                            min_clearance: float = 0.0) -> torch.Tensor:
        """The swept check of a TIMED joint-space path [T x ndof] - row t is where the robot is at waypoint t: the lattice of one candidate per
        waypoint under the solver's sweep (set_path_sweep, at least 1), world, world track and - reject_self - the robot itself with
        min_clearance.  -> [T] bool: entry t >= 1, whether the edge path[t - 1] -> path[t] is blocked; entry 0, whether q_start -> path[0] is
        (False without q_start).  The rows themselves are not tested (Engine.world_track_clearance does that for the track)."""
        assert isinstance(path, torch.Tensor) and path.ndim == 2 and path.shape[1] == self.ndof, f"path must be [T x {self.ndof}]"
        assert q_start is None or (isinstance(q_start, torch.Tensor) and tuple(q_start.shape) == (self.ndof,)), f"q_start must be [{self.ndof}]"
        assert self._path_sweep >= 1, "timed_path_collides needs a sweep (set_path_sweep)"
        assert self._robot.has_collision_model, "timed_path_collides needs a collision model (Robot.set_collision_capsules)"
        with torch.inference_mode():
            eng = self.engine(path.device)
            self._push_collision_model(eng)
            T = path.shape[0]
            if T == 0:
                return torch.zeros(0, dtype=torch.bool, device=path.device)
            rows = path.to(torch.float32).contiguous()
            start = None if q_start is None else q_start.to(device=path.device, dtype=torch.float32).contiguous()
            edge_free, start_free = eng.sweep_lattice(rows, T, 1, start, reject_self, min_clearance)
            blocked = ~edge_free[:, 0, 0]
            blocked[0] = False if start_free is None else ~start_free[0]
            return blocked

    def set_precision(self, mode: str):
        """Arithmetic of the hidden Linear contractions: "f32" (exact f32 MFMA, default) or "f16x3" (error-compensated
        f16 split, measured at least as accurate against fp64; see include/ikflow_amd.h ikf_set_precision)."""
        assert mode in ("f32", "f16x3"), mode
        if self._engine is not None:
            self._engine.set_precision(mode)  # EngineError when the mode is refused: the solver then keeps its previous mode
        self._precision = mode

    def _ensure_initialized(self, allow_uninitialized: bool):
        """The reference runs its randomly initialised nn_model when allow_uninitialized=True
        (tests/ikflow_solver_test.py:89-117); the engine needs explicit weights, so draw the same kind
        (nn.Linear default init) once."""
        if self._state_dict_np is None and allow_uninitialized:
            self._state_dict_np = random_state_dict(self._layout, self._robot, seed=0)
            self._engine = None

    # -- inner path (ikflow_solver.py:85-117) ----------------------------------------------------------
    def _run_inference(self, latent: torch.Tensor, y: torch.Tensor, t0: float, clamp_to_joint_limits: bool, return_detailed: bool):
        t0 = time()
        eng = self.engine(latent.device)
        solutions = eng.generate_approx(y, latent, clamp_to_joint_limits)
        if return_detailed:
            n = solutions.shape[0]
            targets = y.reshape(1, 7).expand(n, 7).contiguous() if y.numel() == 7 else y
            pos_errors, rot_errors = eng.pose_error(solutions, targets)
            joint_limits_exceeded = eng.joint_limits_exceeded(solutions)
            # evaluation_utils.evaluate_solutions' fourth slot: filled when the robot carries a capsule model (jrl's
            # collision geometry is not available here), None otherwise
            self_colliding = self._robot.config_self_collides(solutions) if self._robot.has_collision_model else None
            return solutions, pos_errors, rot_errors, joint_limits_exceeded, self_colliding, time() - t0
        return solutions

    def _calculate_pose_error(self, qs: torch.Tensor, target_poses: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.engine(qs.device).pose_error(qs, target_poses)

    # -- public methods ----------------------------------------------------------------------------------
    def generate_ik_solutions(
        self,
        y: torch.Tensor,
        n: Optional[int] = None,
        latent: Optional[torch.Tensor] = None,
        latent_distribution: str = "gaussian",
        latent_scale: float = 1.0,
        clamp_to_joint_limits: bool = True,
        refine_solutions: bool = False,
        return_detailed: bool = False,
        allow_uninitialized: bool = False,
    ):
        """Run the flow in reverse to generate samples conditioned on a pose y (ikflow_solver.py:254-343).

        y: [7] single target pose (then `n` solutions are drawn) or [batch x 7]; latent: optional [n x network_width].
        Returns [n x ndof], or the 6-tuple (solutions, pos_errors, rot_errors, joint_limits_exceeded, self_colliding,
        runtime) when return_detailed.
        """
        t0 = time()
        if not allow_uninitialized:
            assert self._model_weights_loaded, "Model weights have not been loaded. Call load_state_dict(...)"
        assert isinstance(y, torch.Tensor), f"y must be a torch.Tensor (got {type(y)})."
        if y.numel() == 7:
            assert isinstance(n, int)
            assert n > 0
        else:
            assert y.shape[1] == 7, f"y must be of shape [7] or [n x 7], got {y.shape}"
        assert isinstance(latent_distribution, str)
        assert isinstance(latent_scale, float)
        assert isinstance(latent, torch.Tensor) or (
            latent is None
        ), f"latent must either be a torch.Tensor or None (got {type(latent)})."
        assert not refine_solutions, "refine_solutions is deprecated, use generate_exact_ik_solutions() instead"
        if "cuda" in str(config.DEVICE):
            assert "cpu" not in str(y.device), f"Cuda is available ('{config.DEVICE}'), but target_poses are on {y.device}"
        self._ensure_initialized(allow_uninitialized)

        n = y.shape[0] if n is None else n
        device = y.device
        with torch.inference_mode():
            # the conditional [y, 0] is assembled inside the first-layer kernel (ikflow_solver.py:333-338)
            if latent is None:
                latent = draw_latent(latent_distribution, latent_scale, (n, self._network_width), device)
            assert latent.shape[0] == n, f"{len(latent)} != {n}"
            return self._run_inference(latent, y, t0, clamp_to_joint_limits, return_detailed)

    def generate_exact_ik_solutions(
        self,
        target_poses: torch.Tensor,
        repeat_counts: Tuple[int] = (1, 3, 10),
        pos_error_threshold: float = mm_to_m(1),
        rot_error_threshold: float = 0.1,
        verbosity: int = 0,
        run_lma_on_cpu: bool = True,
        return_detailed: bool = False,
        latents: Optional[Sequence[torch.Tensor]] = None,
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Same as generate_ik_solutions() but refines the flow's seeds with Levenberg-Marquardt
        (ikflow_solver.py:345-411). Returns (solutions [n x ndof], valids [n] bool); unsolved rows are 0.  Under set_exact_collision a
        solution that collides with the scene (or the robot itself) does not count: its pose is retried like an unsolved one."""
        assert target_poses.shape[1] == 7, f"target_poses must be of shape [n x 7], got {target_poses.shape}"
        assert isinstance(repeat_counts, tuple), f"repeat_counts must be a tuple, got {type(repeat_counts)}"
        assert not return_detailed, "return_detailed is not currently supported for generate_exact_ik_solutions()"
        assert self._model_weights_loaded, "Model weights have not been loaded. Call load_state_dict(...)"
        t0 = time()
        n_opt_steps_max = 3
        with torch.inference_mode():
            eng = self.engine(target_poses.device)
            out = eng.generate_exact(
                target_poses, repeat_counts, pos_error_threshold, rot_error_threshold, latents=latents,
                n_lm_steps=n_opt_steps_max, return_stats=verbosity > 0,
            )
        if verbosity > 0:
            solutions, valids, stats = out
            for r, (n_in, rows, lm_rows, solved) in enumerate(stats.tolist()):
                print(f"  round {r}: repeat={repeat_counts[r]} poses={n_in} flow_rows={rows} lm_row_iters<={lm_rows} solved={solved}")
            print(f"  {int(valids.sum().item())}/{valids.numel()} valid ({time() - t0} seconds)")
            return solutions, valids
        return out

    # -- what the three candidate-consuming methods below share -----------------------------------------------------
    def _candidate_args(self, poses, name: str, count: str, k, k_max: Optional[int], latent, shared_latent: bool, latent_distribution,
                        latent_scale, reject_self_collisions: Optional[bool], pos_error_threshold, rot_error_threshold):
        """The asserts generate_ranked_ik_solutions, generate_diverse_ik_solutions and generate_ik_path have in common, before any device
        work.  `name` / `count`: what the poses are called ("y" / "m": one pose [7] is accepted too; "waypoints" / "T").
        -> (poses [count x 7], count, latent rows, reject_self_collisions resolved)"""
        assert self._model_weights_loaded, "Model weights have not been loaded. Call load_state_dict(...)"
        assert isinstance(poses, torch.Tensor), f"{name} must be a torch.Tensor (got {type(poses)})."
        if count == "m":
            assert poses.numel() == 7 or (poses.ndim == 2 and poses.shape[1] == 7), f"{name} must be of shape [7] or [m x 7], got {tuple(poses.shape)}"
        else:
            assert poses.ndim == 2 and poses.shape[1] == 7, f"{name} must be of shape [{count} x 7], got {tuple(poses.shape)}"
        if k_max is None:
            assert isinstance(k, int) and k > 0, f"k must be a positive int, got {k!r}"
        else:
            assert isinstance(k, int) and 1 <= k <= k_max, f"k must be an int in 1 .. {k_max}, got {k!r}"
        assert isinstance(latent_distribution, str)
        assert isinstance(latent_scale, float)
        assert isinstance(latent, torch.Tensor) or latent is None, f"latent must either be a torch.Tensor or None (got {type(latent)})."
        if reject_self_collisions is None:
            reject_self_collisions = self._robot.has_collision_model
        assert not reject_self_collisions or self._robot.has_collision_model, (
            "reject_self_collisions needs a collision model (Robot.set_collision_capsules)")
        poses2 = poses.reshape(1, 7) if poses.numel() == 7 and count == "m" else poses
        n = poses2.shape[0]
        assert k * n <= 2 ** 31 - 1, f"k * {count} must be at most 2^31 - 1, got {k * n}"
        assert pos_error_threshold is None or pos_error_threshold >= 0, "pos_error_threshold must be None (no bound) or >= 0"
        assert rot_error_threshold is None or rot_error_threshold >= 0, "rot_error_threshold must be None (no bound) or >= 0"
        n_latent = k if shared_latent else k * n
        assert latent is None or tuple(latent.shape) == (n_latent, self._network_width), (
            f"latent must be [{n_latent} x {self._network_width}], got {tuple(latent.shape) if latent is not None else None}")
        if "cuda" in str(config.DEVICE):
            assert "cpu" not in str(poses.device), f"Cuda is available ('{config.DEVICE}'), but target_poses are on {poses.device}"
        return poses2, n, n_latent, reject_self_collisions

    def _candidate_engine(self, device, reject_self_collisions: bool, latent, latent_distribution, latent_scale, n_latent: int):
        """-> (the engine of that device, with the robot's capsule model pushed when collisions are rejected; the latent, drawn when None)"""
        eng = self.engine(device)
        if reject_self_collisions and getattr(eng, "_collision_source", None) is not self._robot._collision_model:
            # the solver's own handle, not the one Robot.config_self_collides uses
            eng.set_collision_model(*self._robot._collision_model)
            eng._collision_source = self._robot._collision_model
        if latent is None:
            latent = draw_latent(latent_distribution, latent_scale, (n_latent, self._network_width), device)
        return eng, latent

    # -- best of K samples per pose ------------------------------------------------------------------------------
    def generate_ranked_ik_solutions(
        self,
        y: torch.Tensor,
        k: int,
        n_keep: int = 1,
        latent: Optional[torch.Tensor] = None,
        latent_distribution: str = "gaussian",
        latent_scale: float = 1.0,
        clamp_to_joint_limits: bool = True,
        rot_weight: float = mm_to_m(1) / 0.1,
        q_ref: Optional[torch.Tensor] = None,
        ref_weight: float = 0.0,
        pos_error_threshold: Optional[float] = None,
        rot_error_threshold: Optional[float] = None,
        reject_joint_limits: bool = True,
        reject_self_collisions: Optional[bool] = None,
        min_clearance: float = 0.0,
        return_row_scores: bool = False,
    ):
        """Draw k flow samples for every target pose, drop the inadmissible ones and return the best n_keep of each pose - flow and ranking
        on the GPU without a host round trip (include/ikflow_amd_rank.h).

        y: [7] or [m x 7].  The latent is drawn as ``draw_latent(..., (k * m, dim))``, tile-major: row r * m + j is sample r of pose j, so the
        same torch seed gives the candidates of ``generate_ik_solutions(y.repeat((k, 1)))``.  A candidate's score is
        ``pos_err + rot_weight * rot_err [+ ref_weight * ||q - q_ref[j]||]`` (metres; the default rot_weight is the ratio of
        generate_exact_ik_solutions' default thresholds, 1 mm / 0.1 rad).  Inadmissible: an error not below its threshold (when given), a
        joint strictly outside its limits (reject_joint_limits), a clearance below min_clearance (reject_self_collisions; None = when the
        robot carries a capsule model).  A world set by set_world is in force: a candidate closer to an obstacle than the world's
        min_clearance is inadmissible too.  Candidates are ordered by (score, sample index).  Under set_candidate_refine every candidate is
        LM-refined first, and all of the above is that of the refined candidate.

        Returns the named tuple (solutions [m x n_keep x ndof], scores [m x n_keep], repeat_index [m x n_keep] int32, n_admissible [m]
        int32[, row_scores [k * m]]); slots beyond a pose's admissible candidates hold 0 / +inf / -1."""
        y2, m, n_latent, reject_self_collisions = self._candidate_args(
            y, "y", "m", k, None, latent, False, latent_distribution, latent_scale, reject_self_collisions, pos_error_threshold, rot_error_threshold)
        assert isinstance(n_keep, int) and 1 <= n_keep <= min(k, 16), f"n_keep must be in 1 .. min(k, 16), got {n_keep!r}"
        assert q_ref is None or (isinstance(q_ref, torch.Tensor) and (tuple(q_ref.shape) == (m, self.ndof) or (m == 1 and tuple(q_ref.shape) == (self.ndof,)))), (
            f"q_ref must be [{m} x {self.ndof}], got {tuple(q_ref.shape) if isinstance(q_ref, torch.Tensor) else type(q_ref)}")

        with torch.inference_mode():
            eng, latent = self._candidate_engine(y.device, reject_self_collisions, latent, latent_distribution, latent_scale, n_latent)
            opt = eng.rank_options(n_keep, rot_weight, ref_weight, pos_error_threshold, rot_error_threshold, reject_joint_limits,
                                   reject_self_collisions, min_clearance)
            ref = None if q_ref is None else q_ref.reshape(m, self.ndof)
            sols, scores, index, count, rows = eng.generate_ranked(y2, k, latent, clamp_to_joint_limits, opt, q_ref=ref,
                                                                   row_scores=return_row_scores)
        if return_row_scores:
            return RankedSolutions(sols, scores, index, count, rows)
        return RankedSolutions4(sols, scores, index, count)

    # -- the distinct ways of reaching a pose -----------------------------------------------------------------------
    def generate_diverse_ik_solutions(
        self,
        y: torch.Tensor,
        k: int,
        n_keep: int,
        min_separation: float = 0.0,
        joint_weights: Optional[torch.Tensor] = None,
        latent: Optional[torch.Tensor] = None,
        latent_distribution: str = "gaussian",
        latent_scale: float = 1.0,
        clamp_to_joint_limits: bool = True,
        rot_weight: float = mm_to_m(1) / 0.1,
        pos_error_threshold: Optional[float] = None,
        rot_error_threshold: Optional[float] = None,
        reject_joint_limits: bool = True,
        reject_self_collisions: Optional[bool] = None,
        min_clearance: float = 0.0,
        return_row_scores: bool = False,
    ):
        """Draw k flow samples for every target pose, drop the inadmissible ones and return up to n_keep of each pose that are far apart in
        joint space - the distinct ways of reaching the pose, as seeds for a collision checker or alternatives for a planner - flow and
        selection on the GPU without a host round trip (include/ikflow_amd_diverse.h).

        y: [7] or [m x 7]; 1 <= k <= 1024, 1 <= n_keep <= min(k, 16).  Latent layout, scores and admissibility are those of
        generate_ranked_ik_solutions (without a reference configuration; a world set by set_world is in force; under set_candidate_refine the
        candidates are LM-refined first, and scores, admissibility and distances are those of the refined candidates).  Slot 0 is that method's first choice; every later slot is the
        admissible sample farthest (Euclidean in joint space, no angle wrapping; joint j scaled by a finite joint_weights[j] >= 0 when given) from
        the ones kept so far, ties to the lower sample index.  A pose's selection stops when no sample is left or the farthest one is
        closer than min_separation to a kept one: kept rows are pairwise at least min_separation apart, and when fewer than n_keep are
        kept every other admissible sample is closer than that to one of them.

        Returns the named tuple (solutions [m x n_keep x ndof], scores, repeat_index int32, separation [all m x n_keep], n_kept [m] int32,
        n_admissible [m] int32[, row_scores [k * m]]); unfilled slots hold 0 / +inf / -1 / +inf."""
        y2, m, n_latent, reject_self_collisions = self._candidate_args(
            y, "y", "m", k, 1024, latent, False, latent_distribution, latent_scale, reject_self_collisions, pos_error_threshold, rot_error_threshold)
        assert isinstance(n_keep, int) and 1 <= n_keep <= min(k, 16), f"n_keep must be in 1 .. min(k, 16), got {n_keep!r}"
        assert isinstance(min_separation, (int, float)) and min_separation >= 0, f"min_separation must be >= 0, got {min_separation!r}"
        assert joint_weights is None or (isinstance(joint_weights, torch.Tensor) and tuple(joint_weights.shape) == (self.ndof,)), (
            f"joint_weights must be [{self.ndof}], got {tuple(joint_weights.shape) if isinstance(joint_weights, torch.Tensor) else type(joint_weights)}")
        assert joint_weights is None or bool((torch.isfinite(joint_weights) & (joint_weights >= 0)).all().item()), (
            "joint_weights must all be finite and >= 0")

        with torch.inference_mode():
            eng, latent = self._candidate_engine(y.device, reject_self_collisions, latent, latent_distribution, latent_scale, n_latent)
            opt = eng.diverse_options(n_keep, rot_weight, pos_error_threshold, rot_error_threshold, reject_joint_limits,
                                      reject_self_collisions, min_clearance, min_separation)
            w = None if joint_weights is None else joint_weights.to(device=y.device, dtype=torch.float32)
            sols, scores, index, sep, kept, count, rows = eng.generate_diverse(y2, k, latent, clamp_to_joint_limits, opt, joint_weights=w,
                                                                               row_scores=return_row_scores)
        if return_row_scores:
            return DiverseSolutions(sols, scores, index, sep, kept, count, rows)
        return DiverseSolutions6(sols, scores, index, sep, kept, count)

    # -- one joint-space path through a sequence of poses ------------------------------------------------------------
    def generate_ik_path(
        self,
        waypoints: torch.Tensor,
        k: int,
        latent: Optional[torch.Tensor] = None,
        shared_latent: bool = True,
        latent_distribution: str = "gaussian",
        latent_scale: float = 1.0,
        clamp_to_joint_limits: bool = True,
        rot_weight: float = mm_to_m(1) / 0.1,
        node_weight: float = 1.0,
        max_joint_step: Optional[float] = None,
        q_start: Optional[torch.Tensor] = None,
        pos_error_threshold: Optional[float] = None,
        rot_error_threshold: Optional[float] = None,
        reject_joint_limits: bool = True,
        reject_self_collisions: Optional[bool] = None,
        min_clearance: float = 0.0,
        refine_steps: int = 0,
        return_node_costs: bool = False,
    ):
        """Draw k flow samples for every waypoint of a pose sequence and return the one joint-space path through them that is cheapest in
        pose error and joint motion - flow and search on the GPU without a host round trip (include/ikflow_amd_path.h).

        waypoints: [T x 7], in order.  With shared_latent (the default) the latent is drawn as ``draw_latent(..., (k, dim))`` and candidate r
        uses latent r at EVERY waypoint (the reference's visualizations.py oscillate_target(fixed_latent=True): under trained weights a fixed
        latent gives a solution that varies smoothly with the pose); otherwise as ``(k * T, dim)``, tile-major (row r * T + t is candidate r
        of waypoint t).  A candidate's node cost is ``pos_err + rot_weight * rot_err`` (metres), +inf when it is inadmissible (thresholds,
        joint limits, self-collision and a world set by set_world as in generate_ranked_ik_solutions; edges are swept only under set_path_sweep); the edge between consecutive candidates is their Euclidean joint
        distance (no angle wrapping), forbidden when a joint moves by more than max_joint_step.  The path minimises
        ``sum of edges + node_weight * sum of node costs`` (+ the edge from q_start to the first configuration when q_start is given); ties
        go to the lower candidate index.

        refine_steps > 0 applies that many Levenberg-Marquardt steps to the T chosen rows when a path exists; ``index`` and ``cost`` (and
        ``n_reachable``, ``node_costs``) still describe the unrefined lattice.  set_candidate_refine is the other order: it refines all k * T
        candidates BEFORE the lattice is built, so node costs, admissibility, edges, the step gate, the sweep, ``index``, ``cost`` and the
        returned rows all describe the refined rows - what refine_steps returns was never tested.  The two are independent and may be combined.

        Returns the named tuple (path [T x ndof], index [T] int32, cost, n_reachable [T] int32[, node_costs [k * T]]); without an admissible
        path: rows 0, indices -1, cost +inf, and n_reachable shows the first waypoint nothing reaches."""
        waypoints, T, n_latent, reject_self_collisions = self._candidate_args(
            waypoints, "waypoints", "T", k, 256, latent, shared_latent, latent_distribution, latent_scale, reject_self_collisions,
            pos_error_threshold, rot_error_threshold)
        assert isinstance(refine_steps, int) and refine_steps >= 0, f"refine_steps must be an int >= 0, got {refine_steps!r}"
        assert q_start is None or (isinstance(q_start, torch.Tensor) and tuple(q_start.shape) == (self.ndof,)), (
            f"q_start must be [{self.ndof}], got {tuple(q_start.shape) if isinstance(q_start, torch.Tensor) else type(q_start)}")
        assert node_weight >= 0, f"node_weight must be >= 0, got {node_weight!r}"
        assert max_joint_step is None or max_joint_step >= 0, "max_joint_step must be None (no gate) or >= 0"

        with torch.inference_mode():
            eng, latent = self._candidate_engine(waypoints.device, reject_self_collisions, latent, latent_distribution, latent_scale, n_latent)
            opt = eng.path_options(rot_weight, pos_error_threshold, rot_error_threshold, reject_joint_limits, reject_self_collisions,
                                   min_clearance, node_weight, max_joint_step)
            path, index, cost, reach, nodes = eng.generate_path(waypoints, k, latent, shared_latent, clamp_to_joint_limits, opt,
                                                                q_start=q_start, node_costs=return_node_costs)
            cost = cost.reshape(())
            self._last_path_opt_paths = 1 if (self._path_optimization[0] and T > 0) else None
            if refine_steps > 0 and T > 0 and bool(torch.isfinite(cost).item()):
                for _ in range(refine_steps):
                    path = eng.lm_step(waypoints, path)
        if return_node_costs:
            return PathSolution(path, index, cost, reach, nodes)
        return PathSolution4(path, index, cost, reach)

    # -- many joint-space paths per call ------------------------------------------------------------------------------
    def generate_ik_paths(
        self,
        waypoints: torch.Tensor,
        k: int,
        latent: Optional[torch.Tensor] = None,
        shared_latent: bool = True,
        latent_distribution: str = "gaussian",
        latent_scale: float = 1.0,
        clamp_to_joint_limits: bool = True,
        rot_weight: float = mm_to_m(1) / 0.1,
        node_weight: float = 1.0,
        max_joint_step: Optional[float] = None,
        q_start: Optional[torch.Tensor] = None,
        pos_error_threshold: Optional[float] = None,
        rot_error_threshold: Optional[float] = None,
        reject_joint_limits: bool = True,
        reject_self_collisions: Optional[bool] = None,
        min_clearance: float = 0.0,
        refine_steps: int = 0,
        return_node_costs: bool = False,
    ):
        """generate_ik_path for P pose sequences of T waypoints each in ONE call - one flow call on all P * T * k candidates and the P searches
        side by side on the GPU (include/ikflow_amd_path_batch.h).  Path p is what generate_ik_path returns for ``waypoints[p]`` with
        ``q_start[p]`` on the same candidates; nothing joins one path to the next.

        waypoints: [P x T x 7].  With shared_latent (the default) the latent is drawn as ``draw_latent(..., (k, dim))`` and candidate r uses
        latent r at every waypoint of every path; otherwise as ``(k * P * T, dim)``, row r * (P * T) + p * T + t for candidate r of waypoint t
        of path p.  q_start: [P x ndof] or None.  Every other argument, and what is set on the solver (world, cloud, manipulability floor,
        candidate refinement, sweep), is generate_ik_path's and applies to every path; a world track set by set_world_track is refused.

        refine_steps > 0 applies that many Levenberg-Marquardt steps to the rows of the paths that exist (finite cost); the others stay 0.

        Returns the named tuple (paths [P x T x ndof], index [P x T] int32, cost [P], n_reachable [P x T] int32[, node_costs [k x P x T]]);
        a path that does not exist: rows 0, indices -1, cost +inf."""
        assert isinstance(waypoints, torch.Tensor), f"waypoints must be a torch.Tensor (got {type(waypoints)})."
        assert waypoints.ndim == 3 and waypoints.shape[2] == 7, f"waypoints must be of shape [P x T x 7], got {tuple(waypoints.shape)}"
        P, T = waypoints.shape[0], waypoints.shape[1]
        # (the method's own asserts come first: the shared ones end with the device check, which a CPU tensor on a GPU machine does not pass)
        assert isinstance(refine_steps, int) and refine_steps >= 0, f"refine_steps must be an int >= 0, got {refine_steps!r}"
        assert q_start is None or (isinstance(q_start, torch.Tensor) and tuple(q_start.shape) == (P, self.ndof)), (
            f"q_start must be [{P} x {self.ndof}], got {tuple(q_start.shape) if isinstance(q_start, torch.Tensor) else type(q_start)}")
        assert node_weight >= 0, f"node_weight must be >= 0, got {node_weight!r}"
        assert max_joint_step is None or max_joint_step >= 0, "max_joint_step must be None (no gate) or >= 0"
        flat, n, n_latent, reject_self_collisions = self._candidate_args(
            waypoints.reshape(P * T, 7), "waypoints", "P * T", k, 256, latent, shared_latent, latent_distribution, latent_scale,
            reject_self_collisions, pos_error_threshold, rot_error_threshold)

        with torch.inference_mode():
            eng, latent = self._candidate_engine(waypoints.device, reject_self_collisions, latent, latent_distribution, latent_scale, n_latent)
            opt = eng.path_options(rot_weight, pos_error_threshold, rot_error_threshold, reject_joint_limits, reject_self_collisions,
                                   min_clearance, node_weight, max_joint_step)
            paths, index, cost, reach, nodes = eng.generate_paths(waypoints, k, latent, shared_latent, clamp_to_joint_limits, opt,
                                                                  q_start=q_start, node_costs=return_node_costs)
            self._last_path_opt_paths = P if (self._path_optimization[0] and n > 0) else None
            if refine_steps > 0 and n > 0:
                found = torch.isfinite(cost)
                if bool(found.any().item()):   # only the paths that exist: a no-path entry stays at zeros
                    targets = waypoints[found].reshape(-1, 7)
                    rows = paths[found].reshape(-1, self.ndof)
                    for _ in range(refine_steps):
                        rows = eng.lm_step(targets, rows)
                    paths = paths.clone()
                    paths[found] = rows.reshape(-1, T, self.ndof)
        if return_node_costs:
            return PathsSolution(paths, index, cost, reach, nodes)
        return PathsSolution4(paths, index, cost, reach)

    # -- log-likelihood (forward pass) ----------------------------------------------------------------------
    def _forward_inputs(self, solutions: torch.Tensor, target_poses: torch.Tensor, pad: Optional[torch.Tensor]):
        assert self._model_weights_loaded, "Model weights have not been loaded. Call load_state_dict(...)"
        assert isinstance(solutions, torch.Tensor) and solutions.ndim == 2, "solutions must be [n x ndof]"
        ndof, dim = self._robot.ndof, self._network_width
        n = solutions.shape[0]
        assert solutions.shape[1] == ndof, f"solutions must be [n x {ndof}], got {tuple(solutions.shape)}"
        assert target_poses.numel() == 7 or (target_poses.ndim == 2 and target_poses.shape == (n, 7)), (
            f"target_poses must be [7] or [{n} x 7], got {tuple(target_poses.shape)}")
        if pad is None:
            pad = torch.zeros((n, dim - ndof), dtype=torch.float32, device=solutions.device)
        assert pad.shape == (n, dim - ndof), f"pad must be [{n} x {dim - ndof}], got {tuple(pad.shape)}"
        x = torch.cat([solutions.to(torch.float32), pad.to(device=solutions.device, dtype=torch.float32)], 1)
        return x, target_poses

    def nn_forward(self, x: torch.Tensor, conditional: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The reference's ``nn_model(x, c=conditional, jac=True)`` (ikflow/training/lt_model.py:156): x [n x dim_tot] padded joint rows,
        conditional [n x dim_cond] = [pose (7), softflow scale (softflow models)] -> (z [n x dim_tot], log|det J| [n]).  The engine takes
        ONE softflow scale per call: a softflow column that varies across rows is refused."""
        assert self._model_weights_loaded, "Model weights have not been loaded. Call load_state_dict(...)"
        n = x.shape[0]
        assert conditional.ndim == 2 and conditional.shape[0] == n and conditional.shape[1] in (7, 8), (
            f"conditional must be [{n} x 7 or 8], got {tuple(conditional.shape)}")
        scale = 0.0
        if conditional.shape[1] == 8 and n > 0:
            col = conditional[:, 7]
            scale = float(col[0].item())
            assert bool((col == col[0]).all().item()), "the softflow column must hold one value for every row"
        poses = conditional[:, :7].contiguous()
        return self.engine(x.device).flow_forward(x, poses, scale)

    def log_prob(self, solutions: torch.Tensor, target_poses: torch.Tensor, pad: Optional[torch.Tensor] = None) -> torch.Tensor:
        """log p(q | pose) under the flow, per row: -0.5 |z|^2 - 0.5 D log(2 pi) + log|det dz/dx|, D = dim_tot - the FULL conditional
        log-density, Gaussian normaliser included (the reference's training loss drops it: see ``nll``).

        solutions: [n x ndof] joint angles; target_poses: [n x 7] or a single pose [7].  The flow runs on [n x dim_tot] rows: the columns
        beyond ndof come from ``pad`` ([n x (dim_tot - ndof)]) when given and are ZERO otherwise (the reference pads with 0.001 randn during
        training; nothing random is drawn here).  Rows outside the joint limits are not refused: they give a defined but meaningless value
        (NaN on sigmoid_on_output graphs)."""
        x, poses = self._forward_inputs(solutions, target_poses, pad)
        z, log_det = self.engine(x.device).flow_forward(x, poses)
        return -0.5 * (z * z).sum(1) - 0.5 * z.shape[1] * float(np.log(2.0 * np.pi)) + log_det

    def nll(self, solutions: torch.Tensor, target_poses: torch.Tensor, pad: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The reference's per-row training loss term, literally: 0.5 |z|^2 - log|det J| (ikflow/training/lt_model.py:157-158; no Gaussian
        normaliser, so the numbers compare with training logs).  Same arguments and padding rule as ``log_prob``."""
        x, poses = self._forward_inputs(solutions, target_poses, pad)
        z, log_det = self.engine(x.device).flow_forward(x, poses)
        return 0.5 * (z * z).sum(1) - log_det

    # -- sampling with the log-likelihood (inverse pass with its log-determinant) -----------------------------
    def nn_inverse(self, z: torch.Tensor, conditional: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The reference's ``nn_model(z, c=conditional, rev=True)`` (ikflow_solver.py:98) with BOTH of its values: z [n x dim_tot] latent
        rows, conditional [n x dim_cond] = [pose (7), softflow scale (softflow models)] -> (x [n x dim_tot] - every column, before
        ``[:, :ndof]`` and before any joint-limit clamp -, log|det dx/dz| [n]).  The engine takes ONE softflow scale per call: a softflow
        column that varies across rows is refused."""
        assert self._model_weights_loaded, "Model weights have not been loaded. Call load_state_dict(...)"
        n = z.shape[0]
        assert conditional.ndim == 2 and conditional.shape[0] == n and conditional.shape[1] in (7, 8), (
            f"conditional must be [{n} x 7 or 8], got {tuple(conditional.shape)}")
        scale = 0.0
        if conditional.shape[1] == 8 and n > 0:
            col = conditional[:, 7]
            scale = float(col[0].item())
            assert bool((col == col[0]).all().item()), "the softflow column must hold one value for every row"
        poses = conditional[:, :7].contiguous()
        x, _, log_det = self.engine(z.device).flow_inverse(z, poses, scale, clamp=False)
        return x, log_det

    def sample_and_log_prob(
        self,
        y: torch.Tensor,
        n: Optional[int] = None,
        latent: Optional[torch.Tensor] = None,
        latent_distribution: str = "gaussian",
        latent_scale: float = 1.0,
        clamp_to_joint_limits: bool = False,
        return_pad: bool = False,
    ):
        """Draw IK solutions as ``generate_ik_solutions`` does (same arguments, same ``draw_latent`` call: with the same torch seed both
        methods see the same latent) and return, from the same single pass, the model's log-density of every sample.

        Returns (solutions [n x ndof], log_prob [n]), plus pad [n x (dim_tot - ndof)] when ``return_pad``.  With x = g(z; y) the full
        dim_tot-column output of the flow, log_prob = log p(x | y) = -0.5 |z|^2 - 0.5 dim_tot log(2 pi) - log|det dx/dz|: exactly what
        ``log_prob(x[:, :ndof], y, pad=x[:, ndof:])`` returns for that row, without the second pass.  It is the MODEL's density at the
        sample, not the proposal's: with ``latent_scale != 1`` or ``latent_distribution="uniform"`` the samples are not drawn from it
        (use it as the target density of an importance weight).  It belongs to the UNCLAMPED row: with ``clamp_to_joint_limits=True`` a
        clamped solution is a different point and ``log_prob`` still refers to the row before the clamp."""
        assert self._model_weights_loaded, "Model weights have not been loaded. Call load_state_dict(...)"
        assert isinstance(y, torch.Tensor), f"y must be a torch.Tensor (got {type(y)})."
        if y.numel() == 7:
            assert isinstance(n, int)
            assert n > 0
        else:
            assert y.shape[1] == 7, f"y must be of shape [7] or [n x 7], got {y.shape}"
        assert isinstance(latent_distribution, str)
        assert isinstance(latent_scale, float)
        assert isinstance(latent, torch.Tensor) or (
            latent is None
        ), f"latent must either be a torch.Tensor or None (got {type(latent)})."
        if "cuda" in str(config.DEVICE):
            assert "cpu" not in str(y.device), f"Cuda is available ('{config.DEVICE}'), but target_poses are on {y.device}"

        n = y.shape[0] if n is None else n
        device = y.device
        with torch.inference_mode():
            if latent is None:
                latent = draw_latent(latent_distribution, latent_scale, (n, self._network_width), device)
            assert latent.shape[0] == n, f"{len(latent)} != {n}"
            x, solutions, log_det = self.engine(latent.device).flow_inverse(latent, y, 0.0, clamp=clamp_to_joint_limits)
            dim = self._network_width
            log_prob = -0.5 * (latent * latent).sum(1) - 0.5 * dim * float(np.log(2.0 * np.pi)) - log_det
            if return_pad:
                return solutions, log_prob, x[:, self._robot.ndof:].contiguous()
            return solutions, log_prob

    # -- weights -------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict_filename: str):
        """Set the model's weights from a pickled state_dict (ikflow_solver.py:413-441) or a .npz with the same keys."""
        if str(state_dict_filename).endswith(".npz"):
            with np.load(state_dict_filename) as z:
                state_dict = {k: z[k] for k in z.files}
        else:
            with open(state_dict_filename, "rb") as f:
                try:
                    state_dict = pickle.load(f)
                except pickle.UnpicklingError as e:
                    print(f"Error loading state dict from {state_dict_filename}: {e}")
                    raise e
        self.load_state_dict_tensors(state_dict)

    def load_state_dict_tensors(self, state_dict: Dict[str, Union[torch.Tensor, np.ndarray]]):
        """Extension: take the {key: tensor} mapping directly (what pickle.load returns in the reference)."""
        sd = state_dict_to_numpy(state_dict)
        sd = {(k[len("nn_model."):] if k.startswith("nn_model.") else k): v for k, v in sd.items()}
        sd = {(k[len("_orig_mod."):] if k.startswith("_orig_mod.") else k): v for k, v in sd.items()}  # torch.compile'd modules (:421-427)
        # older FrEIA releases named the two coupling subnets s1/s2 instead of subnet1/subnet2
        sd = {k.replace(".s1.", ".subnet1.").replace(".s2.", ".subnet2."): v for k, v in sd.items()}
        validate_state_dict(self._layout, sd)  # RuntimeError like nn.Module.load_state_dict on a bad file
        self._state_dict_np = sd
        if self._engine is not None:
            try:
                self._engine.load_state_dict(sd)
            finally:  # an f16x3 handle refuses out-of-range weights by falling back to f32: the solver follows its engine
                self._precision = self._engine.precision
        self._model_weights_loaded = True
