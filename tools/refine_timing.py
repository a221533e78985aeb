"""Refined candidates, what the stage costs (profiles/refine_timing.json): Panda width, random weights, 4 LM steps, tolerance 0 (so every row runs
every step), cells (m, k) = (64, 64) and (256, 64); every figure a device-event pair around one call, median and IQR over --calls calls after 10
warm-up calls, inputs resident on the device.
  refine          ikf_refine_candidates on the flow's own output of the cell (the stage alone), and ns per row-step
  exact_round     ikf_refine_exact on the same rows, 4 steps, thresholds 0: k_exact_lm_iters (every row runs every step) + its selection kernel,
                  and ns per row-step - the existing kernel beside the new one
  ranked          ikf_generate_ranked, no refinement
  ranked_refined  ikf_generate_ranked with the refinement set on the handle
  approx512       ikf_generate_approx on 512 rows: the control that this change does not touch
--baseline measures `ranked` and `approx512` only, through entry points every earlier commit has; with --root it imports that tree's ikflow_amd, so
that a parent checkout can be measured in alternation with this one:
  python tools/refine_timing.py --out profiles/refine_timing.json
  python tools/refine_timing.py --baseline --root /path/to/parent/checkout"""
import argparse
import json
import os
import statistics
import sys

CELLS = [(64, 64), (256, 64)]
STEPS = 4


def _timed(torch, fn, calls):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    qs = statistics.quantiles(ms, n=4)
    return {"median_ms": round(statistics.median(ms), 5), "iqr_ms": round(qs[2] - qs[0], 5), "min_ms": round(min(ms), 5)}


def measure(root, calls, baseline):
    sys.path.insert(0, root)
    import torch

    from ikflow_amd.ikflow_solver import IKFlowSolver
    from ikflow_amd.model import hparams_for, layout_from, random_state_dict
    from ikflow_amd.robots import Panda

    dev = torch.device("cuda:0")
    robot = Panda()
    hp = hparams_for("panda__full__lp191_5.25m")
    lay = layout_from(hp, robot)
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(random_state_dict(lay, robot, 0))
    eng = s.engine(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    lo = torch.tensor([l[0] for l in robot.actuated_joints_limits], dtype=torch.float32, device=dev)
    hi = torch.tensor([l[1] for l in robot.actuated_joints_limits], dtype=torch.float32, device=dev)
    out = {}
    y512 = robot.forward_kinematics(lo + (hi - lo) * torch.rand(512, robot.ndof, device=dev, generator=g))
    z512 = torch.randn(512, lay.dim, device=dev, generator=g)
    out["approx512"] = _timed(torch, lambda: eng.generate_approx(y512, z512, True), calls)
    for m, k in CELLS:
        y = robot.forward_kinematics(lo + (hi - lo) * torch.rand(m, robot.ndof, device=dev, generator=g))
        z = torch.randn(k * m, lay.dim, device=dev, generator=g)
        opt = eng.rank_options(n_keep=1, rot_weight=0.01)
        eng.reserve_ranked(m, k)
        cell = {"m": m, "k": k, "rows": m * k}
        cell["ranked"] = _timed(torch, lambda: eng.generate_ranked(y, k, z, True, opt), calls)
        if not baseline:
            rows = eng.generate_approx(y.repeat((k, 1)), z, True)
            cell["refine"] = _timed(torch, lambda: eng.refine_candidates(y, k, rows, STEPS, 0.0, 0.0), calls)
            cell["refine"]["ns_per_row_step"] = round(1e6 * cell["refine"]["median_ms"] / (m * k * STEPS), 3)
            eng.reserve_exact(m, k)
            cell["exact_round"] = _timed(torch, lambda: eng.refine_exact(y, rows, k, 0.0, 0.0, n_lm_steps=STEPS), calls)
            cell["exact_round"]["ns_per_row_step"] = round(1e6 * cell["exact_round"]["median_ms"] / (m * k * STEPS), 3)
            eng.set_candidate_refine(STEPS, 0.0, 0.0)
            cell["ranked_refined"] = _timed(torch, lambda: eng.generate_ranked(y, k, z, True, opt), calls)
            eng.set_candidate_refine(0)
            cell["ranked_after"] = _timed(torch, lambda: eng.generate_ranked(y, k, z, True, opt), calls)
        out[f"m={m} k={k}"] = cell
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.root, a.calls, a.baseline)
    doc = {"what": "ms per call, device-event pair around the call, Panda width, random weights; refine: ikf_refine_candidates, 4 steps, tolerance 0; "
                   "exact_round: ikf_refine_exact, 4 steps, thresholds 0; ranked / ranked_refined / ranked_after: ikf_generate_ranked without, with and "
                   "again without a refinement on the handle; approx512: ikf_generate_approx on 512 rows",
           "calls_per_figure": a.calls, "baseline": a.baseline, "cells": res}
    print(json.dumps(doc), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
