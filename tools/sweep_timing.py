"""Swept path IK, what the stages of one ikf_path_search call cost (profiles/sweep_timing.json): Panda, the seven-obstacle scene of the tests'
kind (a sphere, a capsule, a half-space, two boxes, a sphere, a capsule around the arm's reach), S = 4 samples per edge, cells (T, k) = (64, 64)
and (64, 256), with and without max_joint_step.  Candidate rows: a slowly moving configuration plus 0.3 rad of noise, resident on the device.
  search        ikf_path_search, sweep set                                   (torch event pair around the call)
  search_off    the same call with the sweep off                             (torch event pair around the call)
  bracketed     what the handle's prof_mark pairs record between ikf_profile_begin and ikf_profile_end with the sweep set: the pair around
                k_sweep_edges plus the pair around k_path_lattice<.., true>   (ikf_profile_end reports their sum)
  lattice_off   the one pair around k_path_lattice<.., false>, sweep off
  sweep         bracketed - the lattice's own pair, which is taken as lattice_off (the SWEEP form adds one mask test per predecessor)
  node          search - bracketed: the ranking kernel that scores the nodes, and the gaps between the launches
The world's min_clearance is the lower quartile of the engine's own world clearances of the rows, so that three quarters of the nodes stay
admissible.  Also reported: the share of the T k^2 edges the pruning leaves to be sampled (both nodes admissible, step gate passed).
  python tools/sweep_timing.py --out profiles/sweep_timing.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = [(64, 64), (64, 256)]
SAMPLES = 4
GATE = 0.6


def scene():
    sys.path.insert(0, ROOT)
    from ikflow_amd.world import World

    w = World()
    w.add_sphere((0.45, 0.10, 0.55), 0.08)
    w.add_capsule((0.30, -0.40, 0.20), (0.55, -0.25, 0.60), 0.05)
    w.add_half_space((0.0, 0.0, 1.0), 0.02)
    w.add_box((0.55, 0.0, 0.20), (0.25, 0.40, 0.02))
    w.add_box((-0.35, 0.30, 0.45), (0.08, 0.12, 0.30), (0.92, 0.0, 0.0, 0.38), 0.01)
    w.add_sphere((0.10, 0.50, 0.70), 0.10)
    w.add_capsule((-0.20, -0.45, 0.60), (0.20, -0.55, 0.85), 0.04)
    return w


def measure(calls, cells):
    sys.path.insert(0, ROOT)
    import torch

    from ikflow_amd.engine import kinematics_engine_for
    from ikflow_amd.robots import Panda

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
        eng.set_world(scene(), thr)
        for gate in (None, GATE):
            opt = eng.path_options(rot_weight=0.01, reject_limits=False, max_joint_step=gate)
            eng.set_path_sweep(SAMPLES)
            eng.reserve_path(T, k)

            def run(sweep):
                eng.set_path_sweep(SAMPLES if sweep else 0)
                return eng.path_search(w, k, rows, opt, node_costs=True)

            for _ in range(10):
                run(True)
                run(False)
            torch.cuda.synchronize()
            ms = {"search": [], "search_off": [], "bracketed": [], "lattice_off": []}
            for _ in range(calls):
                for name, sweep in (("search", True), ("search_off", False)):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    run(sweep)
                    t1.record()
                    torch.cuda.synchronize()
                    ms[name].append(t0.elapsed_time(t1))
                for name, sweep, pairs in (("bracketed", True, 2), ("lattice_off", False, 1)):
                    eng.set_path_sweep(SAMPLES if sweep else 0)
                    eng.profile_begin()
                    eng.path_search(w, k, rows, opt)
                    n_pairs, t = eng.profile_end()
                    assert n_pairs == pairs, (name, n_pairs)
                    ms[name].append(t)
            swept, unswept = run(True), run(False)
            node = swept[4].reshape(k, T)
            adm = torch.isfinite(node)
            g3 = rows.reshape(k, T, -1)
            live = adm[:, None, 1:] & adm[None, :, :-1]                                   # [r][j][t]: destination r of t, predecessor j of t - 1
            if gate is not None:
                live &= ((g3[:, None, 1:] - g3[None, :, :-1]).abs() <= gate).all(-1)
            cell = {"T": T, "k": k, "samples": SAMPLES, "max_joint_step": gate, "world_min_clearance": round(thr, 4),
                    "nodes_admissible": round(float(adm.float().mean()), 4), "edges": (T - 1) * k * k, "edges_sampled_share": round(float(live.float().mean()), 4),
                    "path_found_swept": bool(torch.isfinite(swept[2]).item()), "path_found_unswept": bool(torch.isfinite(unswept[2]).item()),
                    "cost_swept": float(swept[2]), "cost_unswept": float(unswept[2])}
            for n, v in ms.items():
                qs = statistics.quantiles(v, n=4)
                cell[n] = {"median_ms": round(statistics.median(v), 5), "iqr_ms": round(qs[2] - qs[0], 5)}
            cell["sweep"] = {"median_ms": round(cell["bracketed"]["median_ms"] - cell["lattice_off"]["median_ms"], 5)}
            cell["node"] = {"median_ms": round(cell["search"]["median_ms"] - cell["bracketed"]["median_ms"], 5)}
            sampled = cell["edges_sampled_share"] * cell["edges"]
            cell["sweep_ns_per_sampled_edge"] = round(1e6 * cell["sweep"]["median_ms"] / sampled, 3) if sampled else None
            out[f"T={T} k={k} gate={gate}"] = cell
            print(json.dumps(cell), flush=True)
        eng.set_path_sweep(0)
        eng.clear_world()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--cells", default=None, help="e.g. 64x64,64x256 (T x k)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cells = CELLS if a.cells is None else [tuple(int(v) for v in c.split("x")) for c in a.cells.split(",")]
    res = measure(a.calls, cells)
    doc = {"what": "ms per ikf_path_search call on caller-supplied rows, Panda, seven obstacles, S = 4; search / search_off: a device-event pair around "
                   "the call with the sweep set / off; bracketed: the handle's pairs around k_sweep_edges and k_path_lattice (their sum); lattice_off: "
                   "the pair around k_path_lattice with the sweep off; sweep = bracketed - lattice_off; node = search - bracketed",
           "calls_per_stage": a.calls, "cells": res}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
