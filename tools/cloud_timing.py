"""What a point cloud on the handle costs (profiles/cloud_timing.json): ms per call, one device-event pair around every call, the median of 30 calls
after every shape is warm - the method of tools/world_timing.py.  Panda released architecture (seeded weights), the test capsule model (5 capsules),
everything resident, point radius 0.01 m, min_clearance 0.
  clearance: ikf_cloud_clearance on 4,096 and 16,384 rows against 4,096, 65,536 and 2^20 points, with point-capsule terms per second
  ranked:    generate_ranked_ik_solutions at (m, k) = (64, 64), n_keep 4, self-collision rejection off, without a cloud and with 16,384 points,
             the two alternating call by call
The points are Gaussian clusters around end points of the Panda's moving capsules (tests/cloud_helpers.py's construction, one fixed seed).
  python tools/cloud_timing.py --out profiles/cloud_timing.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (4096, 16384)
POINTS = (4096, 65536, 1 << 20)
CELL = (64, 64)
RANKED_POINTS = 16384
N_KEEP = 4
RADIUS = 0.01


def _stats(v):
    qs = statistics.quantiles(v, n=4)
    return {"median_ms": round(statistics.median(v), 5), "iqr_ms": round(qs[2] - qs[0], 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}


def _timed(fn, calls):
    import torch

    ev = []
    for _ in range(calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        ev.append((t0, t1))
    torch.cuda.synchronize()
    return [t0.elapsed_time(t1) for t0, t1 in ev]


def measure(calls):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch

    import rank_helpers as RH
    from ikflow_amd.ikflow_solver import IKFlowSolver
    from ikflow_amd.model import hparams_for, layout_from, random_state_dict
    from ikflow_amd.robots import Panda

    dev = torch.device("cuda:0")
    hp = hparams_for("panda__full__lp191_5.25m")
    robot = Panda()
    lay = layout_from(hp, robot)
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(random_state_dict(lay, robot, 0))
    caps = RH.collision_capsules(robot)
    robot.set_collision_capsules(caps)
    eng = s.engine(dev)
    s._push_collision_model(eng)
    rng = np.random.default_rng(0)
    tips = robot.forward_kinematics(torch.tensor(robot.sample_joint_angles(16, 0.0), dtype=torch.float32, device=dev))[:, :3].cpu().numpy()

    def cloud(n):
        of = rng.integers(len(tips), size=n)
        return (tips[of] + rng.standard_normal((n, 3)) * 0.08).astype(np.float32)

    out = {"clearance": {}, "ranked": {}}
    for n_points in POINTS:
        eng.set_world_cloud(cloud(n_points), RADIUS, 0.0)
        for rows in ROWS:
            q = torch.tensor(robot.sample_joint_angles(rows, 0.0), dtype=torch.float32, device=dev)
            for _ in range(5):
                eng.cloud_clearance(q)
            v = _timed(lambda: eng.cloud_clearance(q), calls)
            cell = {"rows": rows, "points": n_points, "capsules": len(caps), **_stats(v)}
            cell["terms_per_s"] = float(f"{rows * n_points * len(caps) / (cell['median_ms'] * 1e-3):.4g}")
            out["clearance"][f"rows={rows} points={n_points}"] = cell
            print(json.dumps(cell), flush=True)
    m, k = CELL
    eng.reserve_ranked(m, k)
    g = torch.Generator(device=dev).manual_seed(0)
    y = robot.forward_kinematics(torch.tensor(robot.sample_joint_angles(m, 0.0), dtype=torch.float32, device=dev))
    lat = torch.randn(k * m, lay.dim, device=dev, generator=g)
    pts = cloud(RANKED_POINTS)
    clouds = {0: None, RANKED_POINTS: pts}
    for n_points, p in clouds.items():
        s.set_world_cloud(p, RADIUS, 0.0)
        for _ in range(10):
            s.generate_ranked_ik_solutions(y, k, N_KEEP, latent=lat, reject_self_collisions=False)
    torch.cuda.synchronize()
    ev = {n: [] for n in clouds}
    for _ in range(calls):
        for n_points, p in clouds.items():
            s.set_world_cloud(p, RADIUS, 0.0)   # (a synchronous copy, outside the event pair)
            ev[n_points] += _timed(lambda: s.generate_ranked_ik_solutions(y, k, N_KEEP, latent=lat, reject_self_collisions=False), 1)
    for n_points, v in ev.items():
        cell = {"m": m, "k": k, "points": n_points, **_stats(v)}
        out["ranked"][f"m={m} k={k} points={n_points}"] = cell
        print(json.dumps(cell), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.calls)
    doc = {"what": "ms per call, device-event pair around every call, median of the calls after warm-up of every shape; clearance = ikf_cloud_clearance "
                   "(terms_per_s = rows x points x capsules / median), ranked = generate_ranked_ik_solutions (n_keep 4, self-collision rejection off) "
                   "without a cloud and with one, alternating call by call; Panda released architecture, test capsule model (5 capsules), radius 0.01, "
                   "min_clearance 0",
           "calls_per_cell": a.calls, **res}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
