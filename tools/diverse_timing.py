"""Diverse-of-K IK, what the select stage adds to a flow + ranking call (profiles/diverse_timing.json), Panda released architecture with synthetic
weights, cells (m, k) = (64, 256), (512, 64) and (4, 1024), poses and latent resident, raw C-ABI calls into preallocated outputs, one device-event
pair around every call:
  ranked   ikf_generate_ranked, n_keep 16:  flow + k_rank_candidates [+ k_rank_merge]
  diverse  ikf_generate_diverse, n_keep 16, min_separation 0 (all 15 rounds run): flow + k_rank_candidates (n_keep 1) + k_diverse_select
  select   k_diverse_select alone: the pair the handle records around that launch between ikf_profile_begin and ikf_profile_end, in an
           ikf_diverse_select call on the same rows (a call without the flow, whose launches record pairs of their own)
The two calls alternate call by call after every shape is warm (as tools/flow_inverse_timing.py does).  Reported per cell: median and
interquartile range of each, and diverse - ranked.
  python tools/diverse_timing.py --out profiles/diverse_timing.json"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = [(64, 256), (512, 64), (4, 1024)]
N_KEEP = 16


def measure(calls, cells):
    sys.path.insert(0, ROOT)
    import torch

    from ikflow_amd import _lib
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
    lib, h = eng.lib, eng._h
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device=dev).manual_seed(0)
    ropt = eng.rank_options(N_KEEP, rot_weight=0.01)
    dopt = eng.diverse_options(N_KEEP, rot_weight=0.01)
    shapes = {}
    for m, k in cells:
        eng.reserve_ranked(m, k)
        eng.reserve_diverse(m, k)
        q = torch.tensor(robot.sample_joint_angles(m), dtype=torch.float32, device=dev)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        poses = robot.forward_kinematics(q).contiguous()
        lat = torch.randn(k * m, lay.dim, device=dev, generator=g)
        shapes[(m, k)] = dict(poses=poses, lat=lat, rows=s.generate_ik_solutions(poses.repeat((k, 1)), latent=lat).contiguous(),
                              q_out=f32(m, N_KEEP, lay.ndof), score=f32(m, N_KEEP), index=i32(m, N_KEEP), sep=f32(m, N_KEEP), kept=i32(m), count=i32(m))

    def run(which, cell):
        t, (m, k) = shapes[cell], cell
        if which == "ranked":
            rc = lib.ikf_generate_ranked(h, t["poses"].data_ptr(), m, k, t["lat"].data_ptr(), 1, None, C.byref(ropt), t["q_out"].data_ptr(),
                                         t["score"].data_ptr(), t["index"].data_ptr(), t["count"].data_ptr(), None, stream)
        elif which == "select":
            rc = lib.ikf_diverse_select(h, t["poses"].data_ptr(), m, k, t["rows"].data_ptr(), None, C.byref(dopt), t["q_out"].data_ptr(),
                                        t["score"].data_ptr(), t["index"].data_ptr(), t["sep"].data_ptr(), t["kept"].data_ptr(), t["count"].data_ptr(),
                                        None, stream)
        else:
            rc = lib.ikf_generate_diverse(h, t["poses"].data_ptr(), m, k, t["lat"].data_ptr(), 1, None, C.byref(dopt), t["q_out"].data_ptr(),
                                          t["score"].data_ptr(), t["index"].data_ptr(), t["sep"].data_ptr(), t["kept"].data_ptr(), t["count"].data_ptr(),
                                          None, stream)
        assert rc == 0, _lib.last_error(lib)

    for cell in shapes:            # every shape warm before anything is timed
        for _ in range(10):
            for which in ("ranked", "diverse", "select"):
                run(which, cell)
    torch.cuda.synchronize()
    out = {}
    for cell in shapes:
        ev = {"ranked": [], "diverse": []}
        select = []
        for _ in range(calls):
            for which in ev:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run(which, cell)
                b.record()
                ev[which].append((a, b))
            eng.profile_begin()
            run("select", cell)
            n_pairs, ms = eng.profile_end()
            assert n_pairs == 1, n_pairs
            select.append(ms)
        torch.cuda.synchronize()
        ms = {n: [a.elapsed_time(b) for a, b in v] for n, v in ev.items()}
        ms["select"] = select
        m, k = cell
        res = {"m": m, "k": k, "rows": m * k, "n_keep": N_KEEP, "kept_min": int(shapes[cell]["kept"].min().item())}
        for n, v in ms.items():
            qs = statistics.quantiles(v, n=4)
            res[n] = {"median_ms": round(statistics.median(v), 5), "iqr_ms": round(qs[2] - qs[0], 5)}
        res["diverse_minus_ranked_ms"] = round(res["diverse"]["median_ms"] - res["ranked"]["median_ms"], 5)
        out[f"m={m} k={k}"] = res
        print(json.dumps(res), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--cells", default=None, help="e.g. 64x256,512x64,4x1024 (m x k)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cells = CELLS if a.cells is None else [tuple(int(v) for v in c.split("x")) for c in a.cells.split(",")]
    res = measure(a.calls, cells)
    doc = {"what": "ms per call, a device-event pair around every call, ikf_generate_ranked and ikf_generate_diverse of one build alternating call by "
                   "call in one process after warm-up of every shape, both with n_keep 16; select = the pair recorded around k_diverse_select; "
                   "Panda released architecture, synthetic weights, rot_weight 0.01, min_separation 0",
           "calls_per_candidate": a.calls, "cells": res}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
