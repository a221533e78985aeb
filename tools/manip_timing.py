"""What a manipulability floor on the handle costs (profiles/manip_timing.json): ms per call of ikf_generate_ranked (generate_ranked_ik_solutions,
n_keep 4, self-collision rejection off), one device-event pair around every call, the median of 50 calls after warm-up - the method of
tools/cloud_timing.py.  Panda released architecture (seeded weights), everything reserved, at (poses, k) = (64, 64) and (4096, 16), without a floor
and with one (part full, floor 0.03: about the median of uniform Panda draws), the two alternating call by call; the difference of the medians is
the rule's cost - one launch of k_manip_rows on poses x k rows.
  python tools/manip_timing.py --out profiles/manip_timing.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = ((64, 64), (4096, 16))
N_KEEP = 4
FLOOR = 0.03


def _stats(v):
    qs = statistics.quantiles(v, n=4)
    return {"median_ms": round(statistics.median(v), 5), "iqr_ms": round(qs[2] - qs[0], 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}


def _timed(fn):
    import torch

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    return t0, t1


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
    out = {}
    for m, k in CELLS:
        s.set_min_manipulability(FLOOR)
        eng.reserve_ranked(m, k)
        g = torch.Generator(device=dev).manual_seed(0)
        y = robot.forward_kinematics(torch.tensor(robot.sample_joint_angles(m, 0.0), dtype=torch.float32, device=dev))
        lat = torch.randn(k * m, lay.dim, device=dev, generator=g)
        call = lambda: s.generate_ranked_ik_solutions(y, k, N_KEEP, latent=lat, reject_self_collisions=False, return_row_scores=True)
        dropped = {}
        for floor in (0.0, FLOOR):
            s.set_min_manipulability(floor)
            for _ in range(10):
                res = call()
            dropped[floor] = int(torch.isinf(res.row_scores).sum())
        torch.cuda.synchronize()
        ev = {0.0: [], FLOOR: []}
        for _ in range(calls):
            for floor in ev:
                s.set_min_manipulability(floor)   # (host state only, outside the event pair)
                ev[floor].append(_timed(call))
        torch.cuda.synchronize()
        off = _stats([a.elapsed_time(b) for a, b in ev[0.0]])
        on = _stats([a.elapsed_time(b) for a, b in ev[FLOOR]])
        cell = {"poses": m, "k": k, "rows": m * k, "floor": FLOOR, "part": "full", "rule_off": off, "rule_on": on,
                "difference_ms": round(on["median_ms"] - off["median_ms"], 5), "inadmissible_rows_off": dropped[0.0], "inadmissible_rows_on": dropped[FLOOR]}
        out[f"poses={m} k={k}"] = cell
        print(json.dumps(cell), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.calls)
    doc = {"what": "ms per call of generate_ranked_ik_solutions (ikf_generate_ranked; n_keep 4, self-collision rejection off, row scores returned), "
                   "device-event pair around every call, median of the calls after warm-up; without a manipulability floor and with one (full, 0.03), "
                   "alternating call by call; Panda released architecture, seeded weights, reserved",
           "calls_per_cell": a.calls, **res}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
