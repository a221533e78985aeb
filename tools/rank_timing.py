"""Best-of-K ranking in one call against what the existing API offers, same process, alternating (profiles/rank_timing.json):
  a = generate_ranked_ik_solutions(y [m x 7], k, n_keep=4)                       flow + ranking, no host round trip
  b = generate_ik_solutions(y.repeat((k, 1)))                                     the flow on the same rows alone
  c = today's route with the existing API only: tiled generate_ik_solutions + pose_error + joint_limits_exceeded [+ self_collision] +
      torch reshape / topk / gather - nothing of this change in it, so it is what the parent commit costs
Panda released architecture (seeded weights), latent and poses resident, cells (m, k) = (64, 64), (1, 4096), (500, 50), (4096, 4), capsule model
off and on.  One device-event pair around every call; every shape is warmed up before anything is timed; the candidates alternate call by call.
Reported per cell: median and interquartile range of a, b, c, the ranking's own cost a - b next to the bytes it must read (k m ndof 4).
  python tools/rank_timing.py --out profiles/rank_timing.json
  rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/rank_timing.py --calls 30 --trace-run     (kernel durations: a run of its own)
  python tools/rank_timing.py --merge-into profiles/rank_timing.json --trace-stats DIR/.../t_results.db"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = [(64, 64), (1, 4096), (500, 50), (4096, 4)]
N_KEEP = 4
ROT_WEIGHT = 0.01


def measure(calls, cells, trace_run=False):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch

    import rank_helpers as RH
    from ikflow_amd.ikflow_solver import IKFlowSolver
    from ikflow_amd.model import hparams_for, layout_from, random_state_dict
    from ikflow_amd.robots import Panda

    dev = torch.device("cuda:0")
    hp = hparams_for("panda__full__lp191_5.25m")
    out = {}
    for collisions in (False, True):
        robot = Panda()
        lay = layout_from(hp, robot)
        s = IKFlowSolver(hp, robot)
        s.load_state_dict_tensors(random_state_dict(lay, robot, 0))
        if collisions:
            robot.set_collision_capsules(RH.collision_capsules(robot))
        eng = s.engine(dev)
        g = torch.Generator(device=dev).manual_seed(0)
        data = {}
        for m, k in cells:
            eng.reserve_ranked(m, k)
            q = torch.tensor(robot.sample_joint_angles(m, 0.0), dtype=torch.float32, device=dev)
            data[(m, k)] = (robot.forward_kinematics(q), torch.randn(k * m, lay.dim, device=dev, generator=g))

        def run_a(m, k):
            y, lat = data[(m, k)]
            return s.generate_ranked_ik_solutions(y, k, N_KEEP, latent=lat, rot_weight=ROT_WEIGHT)

        def run_b(m, k):
            y, lat = data[(m, k)]
            return s.generate_ik_solutions(y.repeat((k, 1)), latent=lat)

        def run_c(m, k):
            y, lat = data[(m, k)]
            tiled = y.repeat((k, 1))
            q = s.generate_ik_solutions(tiled, latent=lat)
            pe, re = eng.pose_error(q, tiled)
            bad = eng.joint_limits_exceeded(q)
            if collisions:
                bad = bad | robot.config_self_collides(q)
            score = torch.where(bad, torch.full_like(pe, float("inf")), pe + ROT_WEIGHT * re).reshape(k, m)
            best, idx = torch.topk(score, N_KEEP, dim=0, largest=False, sorted=True)
            rows = q.reshape(k, m, -1)[idx, torch.arange(m, device=dev)[None, :]]
            return rows.permute(1, 0, 2).contiguous(), best.t().contiguous(), idx.t().to(torch.int32), torch.isfinite(score).sum(0).to(torch.int32)

        runs = {"a": run_a, "b": run_b, "c": run_c}
        for cell in cells:                  # every shape warm before anything is timed
            for _ in range(10):
                for f in runs.values():
                    f(*cell)
        torch.cuda.synchronize()
        for m, k in cells:
            ra, rc = run_a(m, k), run_c(m, k)
            agree = float((ra.repeat_index == rc[2]).float().mean())   # (c's topk breaks ties its own way and rounds the score on its own: a sanity figure)
            ev = {n: [] for n in runs}
            for _ in range(calls):
                for n, f in runs.items():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    f(m, k)
                    t1.record()
                    ev[n].append((t0, t1))
            torch.cuda.synchronize()
            ms = {n: [t0.elapsed_time(t1) for t0, t1 in v] for n, v in ev.items()}
            cell = {"m": m, "k": k, "collisions": collisions, "chunks": eng.rank_chunks(m, k), "index_agreement_a_c": round(agree, 4),
                    "candidate_bytes": k * m * lay.ndof * 4}
            for n, v in ms.items():
                qs = statistics.quantiles(v, n=4)
                cell[n] = {"median_ms": round(statistics.median(v), 5), "iqr_ms": round(qs[2] - qs[0], 5)}
            cell["ranking_own_cost_ms"] = round(cell["a"]["median_ms"] - cell["b"]["median_ms"], 5)
            cell["a_faster_than_c"] = bool(cell["c"]["median_ms"] - cell["a"]["median_ms"] > max(cell["a"]["iqr_ms"], cell["c"]["iqr_ms"]))
            out[f"m={m} k={k} collisions={'on' if collisions else 'off'}"] = cell
            print(json.dumps(cell), flush=True)
        if trace_run:
            break
    return out


def fold_trace(path):
    import collections
    import sqlite3
    dur = collections.defaultdict(list)
    for name, start, end in sqlite3.connect(path).execute("select name, start, end from kernels"):
        if "k_rank" in name or "k_flow_rowowner" in name or "k_flow_cluster" in name or "k_pose_error" in name or "k_limits" in name or "k_self_collision" in name:
            dur[name].append(end - start)
    return [{"Name": n, "Calls": len(v), "AverageNs": round(sum(v) / len(v), 1), "MedianNs": statistics.median(v), "MinNs": min(v), "MaxNs": max(v)}
            for n, v in sorted(dur.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--cells", default=None, help="e.g. 64x64,1x4096")
    ap.add_argument("--trace-run", action="store_true", help="collisions off only, for a rocprofv3 --kernel-trace run")
    ap.add_argument("--trace-stats", default=None)
    ap.add_argument("--merge-into", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.merge_into:
        with open(a.merge_into) as f:
            doc = json.load(f)
        doc["kernel_trace_stats"] = fold_trace(a.trace_stats)
        with open(a.out or a.merge_into, "w") as f:
            json.dump(doc, f, indent=1)
        return
    cells = CELLS if a.cells is None else [tuple(int(v) for v in c.split("x")) for c in a.cells.split(",")]
    res = measure(a.calls, cells, a.trace_run)
    doc = {"what": "ms per call, device-event pair around every call, candidates alternating call by call in one process after warm-up of every shape; "
                   "a = generate_ranked_ik_solutions, b = generate_ik_solutions of the same rows, c = existing API (flow + pose_error + "
                   "joint_limits_exceeded [+ self_collision] + torch topk / gather); Panda released architecture, n_keep 4, rot_weight 0.01",
           "calls_per_candidate": a.calls, "cells": res}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
