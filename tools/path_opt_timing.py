"""The path optimiser's call times (profiles/path_opt_timing.json), Panda released architecture with synthetic weights, T = 64, waypoints and
paths resident, every call between a device-event pair of its own, 50 calls per shape after a warm-up:
  optimize   ikf_path_optimize (validate = 1, smooth_weight 0.1) at n_iters = 1 and 8 for (P, T) = (1, 64), (64, 64), (512, 64), on the
             waypoints' own configurations plus N(0, 0.05) noise - evaluator, k_path_opt, evaluator, k_path_opt_commit
  kernel     the pair the handle records around k_path_opt alone between ikf_profile_begin and ikf_profile_end
  per_waypoint_iteration_us   (kernel at n_iters 8 - kernel at n_iters 1) / (iterations run - 1) / T at P = 1: one more iteration of one path -
             residual pass, recurrence and update - per waypoint; the recurrence is its sequential part
  generate_path   ikf_generate_path at T = 64, k = 32 with the state off and on (n_iters 8), alternating call by call; the lattice stage alone is
             tools/path_timing.py's figure (profiles/path_timing.json), not repeated here
Medians and interquartile ranges, milliseconds.
  python tools/path_opt_timing.py --out profiles/path_opt_timing.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, K = 64, 32
SHAPES = [(1, T), (64, T), (512, T)]
WEIGHT = 0.1


def stat(v):
    q = statistics.quantiles(v, n=4)
    return {"median_ms": statistics.median(v), "q1_ms": q[0], "q3_ms": q[2], "n": len(v)}


def measure(calls):
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
    eng.reserve_path_opt(max(p for p, _ in SHAPES), T)
    eng.reserve_path(T, K)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    out = {"optimize": {}, "kernel": {}}
    for P, t in SHAPES:
        start = 0.5 * (lo + hi) + 0.1 * (hi - lo) * torch.randn(P, 1, robot.ndof, device=dev, generator=g)
        q = torch.minimum(torch.maximum(start + torch.cumsum(0.01 * torch.randn(P, t, robot.ndof, device=dev, generator=g), 1), lo), hi)
        w = robot.forward_kinematics(q.reshape(P * t, -1)).reshape(P, t, 7).contiguous()
        noisy = (q + 0.05 * torch.randn(q.shape, device=dev, generator=g)).contiguous()
        for n_iters in (1, 8):
            run = lambda: eng.path_optimize(w, noisy, opt, n_iters, WEIGHT)
            for _ in range(5):
                run()
            key = f"P{P}_T{t}_iters{n_iters}"
            out["optimize"][key] = stat([timed(run) for _ in range(calls)])
            pairs = []
            for _ in range(calls):
                eng.profile_begin()
                run()
                n_pairs, ms = eng.profile_end()
                assert n_pairs == 1, n_pairs   # (nothing else in ikf_path_optimize records a pair: the evaluator's launches carry no mark)
                pairs.append(ms)
            out["kernel"][key] = stat(pairs)
            out["kernel"][key]["iters_kept"] = eng.path_optimize_info(P)[:, 0].tolist()[:8]
    # one more iteration of one path: n_iters = 1 runs one iteration, n_iters = 8 runs min(8, kept + 1) - the loop ends with the first step it refuses
    k1, k8 = out["kernel"][f"P1_T{T}_iters1"]["median_ms"], out["kernel"][f"P1_T{T}_iters8"]["median_ms"]
    ran = min(8, out["kernel"][f"P1_T{T}_iters8"]["iters_kept"][0] + 1)
    out["per_waypoint_iteration_us"] = {"value": (k8 - k1) / (ran - 1) / T * 1e3 if ran > 1 else None, "iterations_run_at_8": ran}
    # ikf_generate_path with the state off and on, alternating
    lat = torch.randn(K, lay.dim, device=dev, generator=g)
    w1 = w[0].contiguous()
    off, on = [], []
    for i in range(5 + calls):
        eng.set_path_optimize(0)
        t_off = timed(lambda: eng.generate_path(w1, K, lat, True, True, opt))
        eng.set_path_optimize(8, WEIGHT)
        t_on = timed(lambda: eng.generate_path(w1, K, lat, True, True, opt))
        if i >= 5:
            off.append(t_off)
            on.append(t_on)
    eng.set_path_optimize(0)
    out["generate_path"] = {"T": T, "k": K, "off": stat(off), "on_iters8": stat(on), "info_of_the_last_on_call": eng.path_optimize_info(1).tolist()}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_opt_timing.json"))
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    res = measure(a.calls)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "kernel"}, indent=1))
