"""What a world on the handle costs (profiles/world_timing.json): ms per call, one device-event pair around every call, the candidates alternating
call by call in one process after every shape is warm.  Panda released architecture (seeded weights), the test capsule model, latent and poses
resident, n_keep 4, self-collision rejection off, so that the call with 0 obstacles is the plain ranking.
  ranked:    generate_ranked_ik_solutions at (m, k) = (64, 64) and (1024, 32) with 0 (no world), 8 and 64 mixed obstacles
  clearance: ikf_world_clearance on 65,536 rows with 8 and 64 obstacles
The scenes are tests/world_helpers.py's 64-obstacle scene of the Panda and its first 8 obstacles; min_clearance is 0.
  python tools/world_timing.py --out profiles/world_timing.json
  python tools/world_timing.py --no-world-only --lib PATH      the 0-obstacle cells alone on another build of the library (the parent commit's), for
                                                               the alternating comparison of section 4.10: one reading = one process"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS = [(64, 64), (1024, 32)]
N_KEEP = 4
CLEARANCE_ROWS = 65536


def _stats(v):
    qs = statistics.quantiles(v, n=4)
    return {"median_ms": round(statistics.median(v), 5), "iqr_ms": round(qs[2] - qs[0], 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}


def measure(calls, no_world_only, lib):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if lib:   # another build of the library, without the world symbols
        from ikflow_amd import _lib, build

        build.lib_path = lambda flavour="": lib
        _lib.WORLD_SIGNATURES.clear()
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
    robot.set_collision_capsules(RH.collision_capsules(robot))
    eng = s.engine(dev)
    worlds = {0: None}
    if not no_world_only:
        import world_helpers as WH
        from ikflow_amd.world import World

        full = WH.scene("panda", "full64")
        for n in (8, 64):
            worlds[n] = World()
            for ob in full.obstacles[:n]:
                worlds[n]._add(*ob)
    g = torch.Generator(device=dev).manual_seed(0)
    data = {}
    for m, k in CELLS:
        eng.reserve_ranked(m, k)
        q = torch.tensor(robot.sample_joint_angles(m, 0.0), dtype=torch.float32, device=dev)
        data[(m, k)] = (robot.forward_kinematics(q), torch.randn(k * m, lay.dim, device=dev, generator=g))

    def ranked(m, k):
        y, lat = data[(m, k)]
        return s.generate_ranked_ik_solutions(y, k, N_KEEP, latent=lat, reject_self_collisions=False)

    out = {"ranked": {}, "clearance": {}}
    for n_obs, world in worlds.items():    # every shape warm before anything is timed
        if not lib:
            s.set_world(world, 0.0)
        for cell in CELLS:
            for _ in range(10):
                ranked(*cell)
    torch.cuda.synchronize()
    for m, k in CELLS:
        ev = {n: [] for n in worlds}
        for _ in range(calls):
            for n_obs, world in worlds.items():
                if not lib:
                    s.set_world(world, 0.0)   # (a synchronous 4 KB copy, outside the event pair)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                ranked(m, k)
                t1.record()
                ev[n_obs].append((t0, t1))
        torch.cuda.synchronize()
        for n_obs, v in ev.items():
            cell = {"m": m, "k": k, "obstacles": n_obs, "chunks": eng.rank_chunks(m, k), **_stats([t0.elapsed_time(t1) for t0, t1 in v])}
            out["ranked"][f"m={m} k={k} obstacles={n_obs}"] = cell
            print(json.dumps(cell), flush=True)
    if not no_world_only:
        kin = robot._collision_engine(data[CELLS[0]][0])
        q = torch.tensor(robot.sample_joint_angles(CLEARANCE_ROWS, 0.0), dtype=torch.float32, device=dev)
        for n_obs in (8, 64):
            kin.set_world(worlds[n_obs], 0.0)
            for _ in range(10):
                kin.world_clearance(q)
            ev = []
            for _ in range(calls):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                kin.world_clearance(q)
                t1.record()
                ev.append((t0, t1))
            torch.cuda.synchronize()
            cell = {"rows": CLEARANCE_ROWS, "obstacles": n_obs, "boxes": sum(ob[0] == 3 for ob in worlds[n_obs].obstacles),
                    **_stats([t0.elapsed_time(t1) for t0, t1 in ev])}
            out["clearance"][f"rows={CLEARANCE_ROWS} obstacles={n_obs}"] = cell
            print(json.dumps(cell), flush=True)
        kin.clear_world()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--no-world-only", action="store_true", help="the 0-obstacle ranked cells alone")
    ap.add_argument("--lib", default=None, help="path of another build of libikflow_amd.so (implies --no-world-only)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = measure(a.calls, a.no_world_only or bool(a.lib), a.lib)
    doc = {"what": "ms per call, device-event pair around every call, candidates alternating call by call in one process after warm-up of every shape; "
                   "ranked = generate_ranked_ik_solutions (n_keep 4, self-collision rejection off) with 0 / 8 / 64 obstacles on the handle, "
                   "clearance = ikf_world_clearance; Panda released architecture, test capsule model (5 capsules), min_clearance 0",
           "calls_per_candidate": a.calls, "library": a.lib or "this build", **res}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
