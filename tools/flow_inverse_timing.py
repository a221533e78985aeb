"""Scored sampling in one pass against the two-pass route, same box, alternating (profiles/flow_inverse_timing.json):
  A = ikf_generate_approx followed by ikf_flow_forward on its output   (what scoring the flow's own samples costs without ikf_flow_inverse)
  B = one ikf_flow_inverse with all three outputs
  C = ikf_generate_approx alone
Panda released shape, inputs resident, raw C-ABI calls into preallocated outputs, one hipEvent pair around every call; the candidates
alternate call by call after every shape has been warmed up.  Each library runs in fresh processes, `--rounds` times, alternating:
  python tools/flow_inverse_timing.py --out profiles/flow_inverse_timing.json [--parent-lib tools/bin/ab/lib_parent.so]
--parent-lib: a build of an earlier commit (no ikf_flow_inverse: A and C only) - A and C of the two builds must agree within the spread.
  rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/flow_inverse_timing.py --child - --sizes 4096 --calls 40
is the separate run for the kernel durations; --trace-stats DIR/t_results.db folds its per-kernel statistics into the JSON (with --merge-into
FILE: into an existing result file, nothing is run)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(lib, sizes, calls):
    sys.path.insert(0, ROOT)
    import ctypes as C

    import ikflow_amd.build as B
    import torch   # before any dlopen of the library: it must bind to torch's copy of the HIP runtime (ikflow_amd/_lib.py)
    from ikflow_amd import _lib
    if lib != "-":
        path, orig = os.path.abspath(lib), B.lib_path
        B.lib_path = lambda flavour="": path if flavour == "" else orig(flavour)
        B.is_stale = lambda flavour="": False
        if not hasattr(C.CDLL(path), "ikf_flow_inverse"):   # a build of an earlier commit
            _lib.SIGNATURES.pop("ikf_flow_inverse")
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
    eng.reserve(max(sizes))
    lib_, h = eng.lib, eng._h
    has_b = hasattr(lib_, "ikf_flow_inverse")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    D, ndof = lay.dim, lay.ndof
    assert D == ndof   # (A feeds generate_approx's rows straight into the forward pass)
    g = torch.Generator(device=dev).manual_seed(0)
    shapes = {}
    for n in sizes:
        poses = torch.randn(n, 7, device=dev, generator=g)
        poses[:, 3:] /= poses[:, 3:].norm(dim=1, keepdim=True)
        t = dict(poses=poses, lat=torch.randn(n, D, device=dev, generator=g), q=torch.empty(n, ndof, device=dev), z=torch.empty(n, D, device=dev),
                 ld=torch.empty(n, device=dev), x=torch.empty(n, D, device=dev), q2=torch.empty(n, ndof, device=dev), ld2=torch.empty(n, device=dev))
        shapes[n] = t

    def run(cand, n):
        t = shapes[n]
        if cand in ("A", "C"):
            rc = lib_.ikf_generate_approx(h, t["poses"].data_ptr(), 0, t["lat"].data_ptr(), n, 0, 0.0, t["q"].data_ptr(), stream)
            if cand == "A" and rc == 0:
                rc = lib_.ikf_flow_forward(h, t["q"].data_ptr(), n, t["poses"].data_ptr(), 0, 0.0, t["z"].data_ptr(), t["ld"].data_ptr(), stream)
        else:
            rc = lib_.ikf_flow_inverse(h, t["lat"].data_ptr(), n, t["poses"].data_ptr(), 0, 0.0, 0, t["x"].data_ptr(), t["q2"].data_ptr(),
                                       t["ld2"].data_ptr(), stream)
        assert rc == 0, _lib.last_error(lib_)
    cands = ["A", "B", "C"] if has_b else ["A", "C"]
    for n in sizes:            # every shape warm before anything is timed
        for _ in range(20):
            for c in cands:
                run(c, n)
    torch.cuda.synchronize()
    out = {}
    for n in sizes:
        ev = {c: [] for c in cands}
        for _ in range(calls):
            for c in cands:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run(c, n)
                b.record()
                ev[c].append((a, b))
        torch.cuda.synchronize()
        out[str(n)] = {c: [round(a.elapsed_time(b), 5) for a, b in ev[c]] for c in cands}
        if has_b:   # the two routes give the same samples and the same density terms
            t = shapes[n]
            out[str(n)]["max_abs_q_B_minus_A"] = float((t["q2"] - t["q"]).abs().max())
            out[str(n)]["max_abs_logdet_B_plus_A"] = float((t["ld2"] + t["ld"]).abs().max())
    print("RESULT " + json.dumps(out), flush=True)


def fold_trace(path):
    """Per-kernel duration statistics of the row-owner / cluster kernels from rocprofv3's result database (<out>_results.db)."""
    import collections
    import sqlite3
    dur = collections.defaultdict(list)
    for name, start, end in sqlite3.connect(path).execute("select name, start, end from kernels"):
        if "k_flow_rowowner" in name or "k_flow_cluster" in name:
            dur[name].append(end - start)
    return [{"Name": n, "Calls": len(v), "AverageNs": round(sum(v) / len(v), 1), "MedianNs": statistics.median(v), "MinNs": min(v), "MaxNs": max(v),
             "StdDev": round(statistics.pstdev(v), 1)} for n, v in sorted(dur.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--sizes", default="4096,128,512")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--trace-stats", default=None)
    ap.add_argument("--merge-into", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    if a.child is not None:
        return child(a.child, sizes, a.calls)
    if a.merge_into:
        with open(a.merge_into) as f:
            doc = json.load(f)
        doc["kernel_trace_stats"] = fold_trace(a.trace_stats)
        with open(a.out or a.merge_into, "w") as f:
            json.dump(doc, f, indent=1)
        return
    libs = [("new", "-")] + ([("parent", a.parent_lib)] if a.parent_lib else [])
    raw = {name: [] for name, _ in libs}
    for rnd in range(a.rounds):
        for name, path in libs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--sizes", a.sizes, "--calls", str(a.calls)],
                               capture_output=True, text=True, timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(r.stdout[-2000:], r.stderr[-2000:])
                raise SystemExit(f"{name} round {rnd}: child failed (rc {r.returncode})")   # nothing more is started on the GPU
            raw[name].append(json.loads(line[-1][7:]))
    summary = {}
    for name, rounds in raw.items():
        for n in sizes:
            for c in ("A", "B", "C"):
                meds = [statistics.median(r[str(n)][c]) for r in rounds if c in r[str(n)]]
                if meds:
                    summary[f"{name} n={n} {c}"] = {"median_ms_per_round": [round(m, 5) for m in meds], "median_ms": round(statistics.median(meds), 5),
                                                    "spread_ms": round(max(meds) - min(meds), 5)}
    for k, v in summary.items():
        print(f"{k:>22}: median {v['median_ms']:.4f} ms  rounds {v['median_ms_per_round']}  spread {v['spread_ms']:.4f}")
    doc = {"what": "ms per call, hipEvent pair around every call, candidates alternating call by call; A = generate_approx + flow_forward, "
                   "B = flow_inverse (x, q, log_det), C = generate_approx; Panda released shape; one fresh process per round and library",
           "calls_per_candidate": a.calls, "rounds": a.rounds, "summary": summary, "raw_ms": raw}
    if a.trace_stats:
        doc["kernel_trace_stats"] = fold_trace(a.trace_stats)
        for r in doc["kernel_trace_stats"]:
            print(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
