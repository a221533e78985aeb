"""Path IK among moving obstacles, what a world track costs (profiles/track_timing.json): Panda, five capsules, the seven-obstacle scene of
tools/sweep_timing.py, S = 4 samples per edge, cells (T, k) = (64, 64) and (64, 256), no step gate.  Candidate rows as there: a slowly moving
configuration plus 0.3 rad of noise, resident on the device.  The same ikf_path_search call in two modes:
  static   the seven obstacles as a static world (ikf_set_world) - the call as it was before there were tracks
  track    the same seven obstacles as a track of T key frames, each obstacle drifting with its own constant velocity (up to 1 mm per frame and
           axis; a box also turning by up to 0.005 rad per frame; the floor stays), no static world
Per mode:
  search       a device-event pair around the call, sweep set
  bracketed    the handle's prof_mark pairs with the sweep set: the pair around k_sweep_edges plus the pair around k_path_lattice<.., true>
  lattice_off  the one pair around k_path_lattice<.., false>, sweep off
  sweep        bracketed - lattice_off: the sweep stage;  sweep_share = sweep / search
  node         search - bracketed: the ranking kernel, in track mode also k_track_clearance's node sink, and the gaps between the launches
Both modes use one min_clearance: the lower quartile of the engine's static-world clearances of the rows.
  python tools/track_timing.py --out profiles/track_timing.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CELLS = [(64, 64), (64, 256)]
SAMPLES = 4


def moving_scene(T):
    """T Worlds: sweep_timing.scene() in frame 0, every obstacle drifting."""
    import numpy as np

    from ikflow_amd.world import BOX, CAPSULE, HALF_SPACE, World
    from sweep_timing import scene

    rng = np.random.default_rng(0)
    base = scene().obstacles
    vel = [rng.uniform(-0.001, 0.001, 3) for _ in base]
    spin = [rng.uniform(-0.005, 0.005) for _ in base]
    frames = []
    for t in range(T):
        w = World()
        for (kind, a, b, quat, radius), v, s in zip(base, vel, spin):
            a, b, quat = np.asarray(a), np.asarray(b), np.asarray(quat)
            if kind == HALF_SPACE:
                w._add(kind, a, b, quat, radius)   # the floor stays: the base capsule sits exactly min_clearance above it in every row
            elif kind == CAPSULE:
                w._add(kind, a + v * t, b + v * t, quat, radius)
            elif kind == BOX:
                c, sn = np.cos(0.5 * s * t), np.sin(0.5 * s * t)   # a turn about z in front of the box's own orientation
                qw, qx, qy, qz = quat
                w._add(kind, a + v * t, b, (c * qw - sn * qz, c * qx - sn * qy, c * qy + sn * qx, c * qz + sn * qw), radius)
            else:
                w._add(kind, a + v * t, b, quat, radius)
        frames.append(w)
    return frames


def measure(calls, cells):
    import torch

    from ikflow_amd.engine import kinematics_engine_for
    from ikflow_amd.robots import Panda
    from sweep_timing import scene

    dev = torch.device("cuda:0")
    robot = Panda()
    act = [j.name for j in robot.joints if j.actuated]
    robot.set_collision_capsules([(None, (0.0, 0.0, 0.0), (0.0, 0.0, 0.2), 0.06), (act[1], (0.0, 0.0, -0.05), (0.0, -0.15, 0.0), 0.06),
                                  (act[3], (0.0, 0.0, 0.0), (0.08, 0.1, 0.0), 0.06), (act[5], (0.0, 0.0, 0.0), (0.09, 0.0, 0.0), 0.05),
                                  (act[-1], (0.0, 0.0, 0.05), (0.0, 0.0, 0.1), 0.04)])
    eng = kinematics_engine_for(robot, dev)
    eng.set_collision_model(*robot._collision_model)
    g = torch.Generator(device=dev).manual_seed(0)
    lo = torch.tensor([l[0] for l in robot.actuated_joints_limits], dtype=torch.float32, device=dev)
    hi = torch.tensor([l[1] for l in robot.actuated_joints_limits], dtype=torch.float32, device=dev)
    out = {}
    for T, k in cells:
        centre = torch.minimum(torch.maximum(0.5 * (lo + hi) + torch.cumsum(0.02 * torch.randn(T, robot.ndof, device=dev, generator=g), 0), lo), hi)
        w = robot.forward_kinematics(centre)
        rows = centre[None] + 0.3 * torch.randn(k, T, robot.ndof, device=dev, generator=g)
        rows = torch.minimum(torch.maximum(rows, lo), hi).reshape(k * T, robot.ndof).contiguous()
        eng.set_world(scene(), 0.0)
        thr = float(torch.quantile(eng.world_clearance(rows)[0], 0.25))
        frames = moving_scene(T)
        opt = eng.path_options(rot_weight=0.01, reject_limits=False)
        cell = {"T": T, "k": k, "samples": SAMPLES, "world_min_clearance": round(thr, 4), "edges": (T - 1) * k * k}
        for mode in ("static", "track"):
            eng.clear_world()
            eng.clear_world_track()
            eng.set_path_sweep(SAMPLES)
            if mode == "static":
                eng.set_world(scene(), thr)
            else:
                eng.set_world_track(frames, thr)
            eng.reserve_path(T, k)

            def run(sweep):
                eng.set_path_sweep(SAMPLES if sweep else 0)
                return eng.path_search(w, k, rows, opt, node_costs=True)

            for _ in range(10):
                run(True)
                run(False)
            torch.cuda.synchronize()
            ms = {"search": [], "bracketed": [], "lattice_off": []}
            for _ in range(calls):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                eng.set_path_sweep(SAMPLES)
                t0.record()
                eng.path_search(w, k, rows, opt, node_costs=True)
                t1.record()
                torch.cuda.synchronize()
                ms["search"].append(t0.elapsed_time(t1))
                for name, sweep, pairs in (("bracketed", True, 2), ("lattice_off", False, 1)):
                    eng.set_path_sweep(SAMPLES if sweep else 0)
                    eng.profile_begin()
                    eng.path_search(w, k, rows, opt)
                    n_pairs, t = eng.profile_end()
                    assert n_pairs == pairs, (name, n_pairs)
                    ms[name].append(t)
            swept = run(True)
            adm = torch.isfinite(swept[4])
            res = {"nodes_admissible": round(float(adm.float().mean()), 4), "path_found": bool(torch.isfinite(swept[2]).item()), "cost": float(swept[2])}
            for n, v in ms.items():
                qs = statistics.quantiles(v, n=4)
                res[n] = {"median_ms": round(statistics.median(v), 5), "iqr_ms": round(qs[2] - qs[0], 5)}
            res["sweep"] = {"median_ms": round(res["bracketed"]["median_ms"] - res["lattice_off"]["median_ms"], 5)}
            res["node"] = {"median_ms": round(res["search"]["median_ms"] - res["bracketed"]["median_ms"], 5)}
            res["sweep_share"] = round(res["sweep"]["median_ms"] / res["search"]["median_ms"], 4)
            cell[mode] = res
        cell["track_over_static"] = round(cell["track"]["search"]["median_ms"] / cell["static"]["search"]["median_ms"], 4)
        out[f"T={T} k={k}"] = cell
        print(json.dumps(cell), flush=True)
        eng.set_path_sweep(0)
        eng.clear_world()
        eng.clear_world_track()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--cells", default=None, help="e.g. 64x64,64x256 (T x k)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cells = CELLS if a.cells is None else [tuple(int(v) for v in c.split("x")) for c in a.cells.split(",")]
    res = measure(a.calls, cells)
    doc = {"what": "ms per ikf_path_search call on caller-supplied rows, Panda, five capsules, seven obstacles, S = 4, medians after warm-up; static: the "
                   "obstacles as ikf_set_world (the call as it was before tracks); track: the same obstacles, drifting, as ikf_set_world_track of T "
                   "frames; search: a device-event pair around the call; sweep = (pairs around k_sweep_edges + k_path_lattice) - (pair around "
                   "k_path_lattice with the sweep off); sweep_share = sweep / search; node = search - bracketed",
           "calls_per_stage": a.calls, "cells": res}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
