"""Exact IK under the exact collision rule, what it costs (profiles/exact_world_timing.json): Panda width, seeded random weights, B = 4096 poses,
rc (1, 3, 10), 3 LM steps; every figure a device-event pair around one call, median, IQR and minimum over --calls calls after 10 warm-up calls,
inputs resident on the device.
  exact_worst_case   ikf_generate_exact with the README thresholds (1 mm / 0.01 rad): random weights, so (almost) every pose runs all three rounds
  exact_converged    the flow over B rows + ikf_refine_exact from q_true + N(0, 0.05^2) seeds: "round 0 converges"
--baseline measures these two only, through entry points every earlier commit has; with --root it imports that tree's ikflow_amd, so that a parent
checkout can be measured in alternation with this one (the rule is off in both: the off path against the parent).  Without --baseline, also:
  round_plain        ikf_refine_exact on 3 B rows (R = 3) from q_true + N(0, 0.05^2): k_exact_lm_iters + the selection
  round_rule         the same call under the rule: seven obstacles, five capsules, self rule on, thresholds at the medians of the candidates' own
                     clearances (the share of rows rejected is reported): k_exact_lm_iters_clear + the selection
  round_rule_cloud   ... plus a cloud of 16,384 points (k_cloud_clearance on the round's rows + k_exact_mask_rows)
  worst_case_rule    exact_worst_case under the rule (world and self)
  schedule           flow rows of one call on fixed latents with and without the rule: how many more rows the schedule ran because rejected poses fell
                     through to later rounds - a property of the random weights and the scene, not of the kernel
  python tools/exact_world_timing.py --out profiles/exact_world_timing.json
  python tools/exact_world_timing.py --baseline --root /path/to/parent/checkout"""
import argparse
import json
import os
import statistics
import sys

B = 4096
RC = (1, 3, 10)
STEPS = 3
POS_THR, ROT_THR = 1e-3, 0.01


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


def _capsules(robot):
    """Five capsules: the base, three moving links, a sphere on the tool."""
    act = [j.name for j in robot.joints if j.actuated]
    return [(None, (0.0, 0.0, 0.0), (0.0, 0.0, 0.2), 0.05), (act[1], (0.0, 0.0, -0.05), (0.0, 0.0, 0.1), 0.06),
            (act[3], (0.0, 0.0, 0.0), (0.08, 0.0, 0.1), 0.05), (act[-1], (0.0, 0.0, 0.0), (0.0, 0.0, 0.1), 0.04),
            (act[-1], (0.0, 0.0, 0.12), (0.0, 0.0, 0.12), 0.04)]


def _world(points):
    """Seven obstacles among tool positions of random configurations."""
    from ikflow_amd.world import World

    w = World()
    p = [tuple(float(x) for x in points[i]) for i in range(6)]
    w.add_sphere(p[0], 0.08)
    w.add_capsule(p[1], p[2], 0.04)
    w.add_half_space((0.0, 0.0, 1.0), -0.15)
    w.add_box(p[3], (0.05, 0.1, 0.15), (0.9, 0.1, 0.3, 0.2))
    w.add_box(p[4], (0.12, 0.04, 0.06), (1.0, 0.0, 0.0, 0.0), 0.02)
    w.add_sphere(p[5], 0.05)
    w.add_capsule(p[0], p[4], 0.02)
    return w


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
    q_true = lo + (hi - lo) * (0.05 + 0.9 * torch.rand(B, robot.ndof, device=dev, generator=g))
    poses = robot.forward_kinematics(q_true)
    z = torch.randn(B, lay.dim, device=dev, generator=g)
    eng.reserve_exact(B, max(RC))
    out = {}
    out["exact_worst_case"] = _timed(torch, lambda: eng.generate_exact(poses, RC, POS_THR, ROT_THR, n_lm_steps=STEPS), calls)
    seeds1 = torch.minimum(torch.maximum(q_true + 0.05 * torch.randn(B, robot.ndof, device=dev, generator=g), lo), hi).contiguous()

    def converged():
        eng.generate_approx(poses, z, True)
        return eng.refine_exact(poses, seeds1, 1, POS_THR, ROT_THR, n_lm_steps=STEPS)

    out["exact_converged"] = _timed(torch, converged, calls)
    out["exact_converged"]["valid"] = int(converged()[1].sum())
    if baseline:
        return out

    R = 3
    seeds3 = torch.minimum(torch.maximum(q_true.repeat(R, 1) + 0.05 * torch.randn(R * B, robot.ndof, device=dev, generator=g), lo), hi).contiguous()
    plain = lambda: eng.refine_exact(poses, seeds3, R, POS_THR, ROT_THR, n_lm_steps=STEPS)
    out["round_plain"] = _timed(torch, plain, calls)
    out["round_plain"]["rows"] = R * B
    # the scene, with thresholds at the medians of the candidates' own clearances
    robot.set_collision_capsules(_capsules(robot))
    eng.set_collision_model(*robot._collision_model)
    cand, ok = eng.refine_exact(poses.repeat(R, 1), seeds3, 1, POS_THR, ROT_THR, n_lm_steps=STEPS)   # every row on its own: the candidates
    cand = cand[ok]
    eng.set_world(_world(poses[:6, :3].cpu().numpy()), 0.0)
    world_thr = float(eng.world_clearance(cand)[0].median())
    self_thr = float(eng.self_collision(cand)[0].median())
    eng.set_world(_world(poses[:6, :3].cpu().numpy()), world_thr)
    eng.set_exact_collision(True, True, self_thr)
    out["round_rule"] = _timed(torch, plain, calls)
    out["round_rule"].update(rows=R * B, candidates=int(ok.sum()), rejected=eng.exact_collision_rejected()[0], world_min_clearance=world_thr,
                             self_min_clearance=self_thr, valid=int(plain()[1].sum()))
    fixed = [torch.randn(B * r, lay.dim, device=dev, generator=g) for r in RC]
    out["worst_case_rule"] = _timed(torch, lambda: eng.generate_exact(poses, RC, POS_THR, ROT_THR, n_lm_steps=STEPS), calls)
    with_rule = eng.generate_exact(poses, RC, POS_THR, ROT_THR, latents=fixed, n_lm_steps=STEPS, return_stats=True)[2]
    rejected = eng.exact_collision_rejected()[:len(RC)]
    pts = (poses[torch.randint(0, B, (16384,), device=dev, generator=g), :3] + 0.1 * torch.randn(16384, 3, device=dev, generator=g)).cpu().numpy()
    eng.set_world_cloud(pts, 0.01, 0.0)
    cloud_thr = float(eng.cloud_clearance(cand)[0].median())
    eng.set_world_cloud(pts, 0.01, cloud_thr)
    eng.reserve_exact(B, max(RC))
    out["round_rule_cloud"] = _timed(torch, plain, calls)
    out["round_rule_cloud"].update(rows=R * B, points=16384, cloud_min_clearance=cloud_thr, rejected=eng.exact_collision_rejected()[0],
                                   valid=int(plain()[1].sum()))
    eng.clear_world_cloud()
    eng.set_exact_collision(False)
    without = eng.generate_exact(poses, RC, POS_THR, ROT_THR, latents=fixed, n_lm_steps=STEPS, return_stats=True)[2]
    out["schedule"] = {"note": "a property of the random weights and the scene, not of the kernel", "stats_with_rule": with_rule.tolist(),
                       "stats_without": without.tolist(), "rejected_rows": rejected, "flow_rows_with_rule": int(with_rule[:, 1].sum()),
                       "flow_rows_without": int(without[:, 1].sum())}
    out["exact_worst_case_after"] = _timed(torch, lambda: eng.generate_exact(poses, RC, POS_THR, ROT_THR, n_lm_steps=STEPS), calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.root, a.calls, a.baseline)
    doc = {"what": "ms per call, device-event pair around the call, Panda width, seeded random weights, 4096 poses, rc (1, 3, 10), 3 LM steps",
           "calls_per_figure": a.calls, "baseline": a.baseline, "root": "this tree" if not a.baseline else "--root", "cells": res}
    print(json.dumps(doc), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
