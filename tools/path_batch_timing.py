"""Path IK for P paths per call against P single calls (profiles/path_batch_timing.json), Panda released architecture with synthetic weights,
T = 64, k = 32, P in {1, 8, 64, 512}, a shared latent, waypoints resident, every form between a device-event pair of its own:
  batch    one ikf_generate_path_batch call on the P paths                      (torch event pair around the call)
  singles  P consecutive ikf_generate_path calls on the same handle            (torch event pair around the P calls) - the baseline: the
           single-path entry, whose code the batch leaves as it was
  lattice_batch / lattice_singles   the lattice stage alone: the pairs the handle records around k_path_lattice between ikf_profile_begin and
           ikf_profile_end, in ikf_path_search_batch / P x ikf_path_search on the flow's rows of the same latents (the flow records pairs of
           its own) - one pair in the batch call, the sum of P pairs in the single calls
The two forms alternate call by call in one process after a warm-up of each shape.  Reported per P: median and interquartile range of each,
the ratios singles / batch, and whether the batch's median lies inside the singles' interquartile spread (asked of P = 1).
  python tools/path_batch_timing.py --out profiles/path_batch_timing.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, K = 64, 32
PATHS = [1, 8, 64, 512]


def measure(calls, paths):
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
    lo = torch.tensor([l[0] for l in robot.actuated_joints_limits], dtype=torch.float32, device=dev)
    hi = torch.tensor([l[1] for l in robot.actuated_joints_limits], dtype=torch.float32, device=dev)
    lat = torch.randn(K, lay.dim, device=dev, generator=g)
    eng.reserve_path_batch(max(paths), T, K)
    eng.reserve_path(T, K)
    out = {}
    for P in paths:
        # P pose sequences, each along its own slowly moving configuration
        start = 0.5 * (lo + hi) + 0.1 * (hi - lo) * torch.randn(P, 1, robot.ndof, device=dev, generator=g)
        q = start + torch.cumsum(0.01 * torch.randn(P, T, robot.ndof, device=dev, generator=g), 1)
        w = robot.forward_kinematics(torch.minimum(torch.maximum(q, lo), hi).reshape(P * T, -1)).reshape(P, T, 7).contiguous()

        def run_batch():
            return eng.generate_paths(w, K, lat, True, True, opt)

        def run_singles():
            for p in range(P):
                eng.generate_path(w[p], K, lat, True, True, opt)

        n_wp = P * T
        expanded = lat[:, None, :].expand(K, n_wp, lay.dim).reshape(K * n_wp, lay.dim).contiguous()
        rows = s.generate_ik_solutions(w.reshape(n_wp, 7).repeat((K, 1)), latent=expanded)
        rows_p = [rows.reshape(K, P, T, -1)[:, p].reshape(K * T, -1).contiguous() for p in range(P)]

        def search_batch():
            return eng.path_search_batch(w, K, rows, opt)

        def search_singles():
            for p in range(P):
                eng.path_search(w[p], K, rows_p[p], opt)

        runs = {"batch": run_batch, "singles": run_singles}
        searches = {"batch": search_batch, "singles": search_singles}
        for _ in range(5):
            for f in list(runs.values()) + list(searches.values()):
                f()
        torch.cuda.synchronize()
        ev = {form: [] for form in runs}
        lattice = {form: [] for form in runs}
        for _ in range(calls):
            for form, f in runs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                f()
                t1.record()
                ev[form].append((t0, t1))
            for form, f in searches.items():   # (the search entries on the flow's rows: the flow's own launches record pairs too)
                eng.profile_begin()
                f()
                n_pairs, ms = eng.profile_end()
                assert n_pairs == (1 if form == "batch" else P), (form, n_pairs)
                lattice[form].append(ms)
        torch.cuda.synchronize()
        ms = {form: [t0.elapsed_time(t1) for t0, t1 in v] for form, v in ev.items()}
        ms["lattice_batch"], ms["lattice_singles"] = lattice["batch"], lattice["singles"]
        res = run_batch()
        cell = {"P": P, "T": T, "k": K, "rows": P * T * K, "paths_found": int(torch.isfinite(res[2]).sum().item())}
        for form, v in ms.items():
            qs = statistics.quantiles(v, n=4)
            cell[form] = {"median_ms": round(statistics.median(v), 5), "iqr_ms": round(qs[2] - qs[0], 5), "q1_ms": round(qs[0], 5), "q3_ms": round(qs[2], 5)}
        cell["ratio_singles_over_batch"] = round(cell["singles"]["median_ms"] / cell["batch"]["median_ms"], 3)
        cell["ratio_lattice_singles_over_batch"] = round(cell["lattice_singles"]["median_ms"] / cell["lattice_batch"]["median_ms"], 3)
        cell["batch_median_inside_singles_iqr"] = bool(cell["singles"]["q1_ms"] <= cell["batch"]["median_ms"] <= cell["singles"]["q3_ms"])
        out[f"P={P}"] = cell
        print(json.dumps(cell), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--paths", default=None, help="e.g. 1,8,64,512")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    paths = PATHS if a.paths is None else [int(v) for v in a.paths.split(",")]
    res = measure(a.calls, paths)
    doc = {"what": "ms per form, a device-event pair around one ikf_generate_path_batch call (batch) and around P consecutive ikf_generate_path "
                   "calls on the same handle (singles), the two alternating call by call in one process after a warm-up of each shape; "
                   "lattice_* = the pairs the handle records around k_path_lattice (one in the batch, the sum of P in the singles); Panda released "
                   "architecture, synthetic weights, shared latent, T 64, k 32, rot_weight 0.01, node_weight 1",
           "calls_per_form": a.calls, "cells": res}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
