"""Path IK, what each stage of one ikf_generate_path call costs (profiles/path_timing.json), Panda released architecture with synthetic weights,
cells (T, k) = (256, 64) and (1024, 256), latent and waypoints resident, every stage between a device-event pair of its own:
  flow     generate_ik_solutions on the k T rows of the expanded latent               (torch event pair around the call)
  search   ikf_path_search on those rows: node stage + lattice stage                   (torch event pair around the call)
  lattice  k_path_lattice alone: the pair the handle records around that launch between ikf_profile_begin and ikf_profile_end
  node     search - lattice: the ranking kernel that scores the nodes, and the gap between the launches
  whole    generate_ik_path (shared latent): expand + flow + node + lattice            (torch event pair around the call)
The stages alternate call by call after every shape is warm.  Reported per cell: median and interquartile range of each, and the lattice's
time per waypoint.
  python tools/path_timing.py --out profiles/path_timing.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = [(256, 64), (1024, 256)]


def measure(calls, cells):
    sys.path.insert(0, ROOT)
    import torch

    from ikflow_amd.ikflow_solver import IKFlowSolver
    from ikflow_amd.model import hparams_for, layout_from, random_state_dict
    from ikflow_amd.robots import Panda

    dev = torch.device("cuda:0")
    hp = hparams_for("panda__full__lp191_5.25m")
    robot = Panda()
    lay = layout_from(hp, robot)
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(random_state_dict(lay, robot, 0))
    eng = s.engine(dev)
    opt = eng.path_options(rot_weight=0.01)
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}
    for T, k in cells:
        eng.reserve_path(T, k)
        # waypoints along a slowly moving configuration
        lo = torch.tensor([l[0] for l in robot.actuated_joints_limits], dtype=torch.float32, device=dev)
        hi = torch.tensor([l[1] for l in robot.actuated_joints_limits], dtype=torch.float32, device=dev)
        q = 0.5 * (lo + hi) + torch.cumsum(0.01 * torch.randn(T, robot.ndof, device=dev, generator=g), 0)
        w = robot.forward_kinematics(torch.minimum(torch.maximum(q, lo), hi))
        lat = torch.randn(k, lay.dim, device=dev, generator=g)
        expanded = lat[:, None, :].expand(k, T, lay.dim).reshape(k * T, lay.dim).contiguous()
        tiled = w.repeat((k, 1))
        rows = s.generate_ik_solutions(tiled, latent=expanded)

        def run_flow():
            return s.generate_ik_solutions(tiled, latent=expanded)

        def run_search():
            return eng.path_search(w, k, rows, opt)

        def run_whole():
            return s.generate_ik_path(w, k, latent=lat)

        runs = {"flow": run_flow, "search": run_search, "whole": run_whole}
        for _ in range(10):
            for f in runs.values():
                f()
        torch.cuda.synchronize()
        ev = {n: [] for n in runs}
        lattice = []
        for _ in range(calls):
            for n, f in runs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                f()
                t1.record()
                ev[n].append((t0, t1))
            eng.profile_begin()
            run_search()
            n_pairs, ms = eng.profile_end()
            assert n_pairs == 1, n_pairs
            lattice.append(ms)
        torch.cuda.synchronize()
        ms = {n: [t0.elapsed_time(t1) for t0, t1 in v] for n, v in ev.items()}
        ms["lattice"] = lattice
        ms["node"] = [a - b for a, b in zip(ms["search"], [statistics.median(lattice)] * calls)]
        res = s.generate_ik_path(w, k, latent=lat)
        cell = {"T": T, "k": k, "rows": k * T, "path_found": bool(torch.isfinite(res.cost).item()), "n_reachable_min": int(res.n_reachable.min().item())}
        for n, v in ms.items():
            qs = statistics.quantiles(v, n=4)
            cell[n] = {"median_ms": round(statistics.median(v), 5), "iqr_ms": round(qs[2] - qs[0], 5)}
        cell["lattice_us_per_waypoint"] = round(1000.0 * cell["lattice"]["median_ms"] / T, 4)
        out[f"T={T} k={k}"] = cell
        print(json.dumps(cell), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--cells", default=None, help="e.g. 256x64,1024x256 (T x k)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cells = CELLS if a.cells is None else [tuple(int(v) for v in c.split("x")) for c in a.cells.split(",")]
    res = measure(a.calls, cells)
    doc = {"what": "ms per call, a device-event pair around every stage, stages alternating call by call in one process after warm-up of every shape; "
                   "flow = generate_ik_solutions of the k T rows, search = ikf_path_search (node + lattice), lattice = the pair recorded around "
                   "k_path_lattice, node = search - median lattice, whole = generate_ik_path with a shared latent; Panda released architecture, "
                   "synthetic weights, rot_weight 0.01, node_weight 1",
           "calls_per_stage": a.calls, "cells": res}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
