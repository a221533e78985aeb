"""Path IK for P paths per call (include/ikflow_amd_path_batch.h): the batch layout built from P single lattices and taken apart again, and the
swept cases of tests/test_path_batch.py with the condition the fp64 reference of tests/sweep_helpers.py puts on them.  The references are the
single path's: path_helpers.dp_f32 and sweep_helpers.verdicts."""
import numpy as np
import torch

import helpers as H
import rank_helpers as RH
import sweep_helpers as SH
import world_helpers as WH

F = np.float32


def to_batch(rows_per_path, k):
    """P tile-major blocks [k * T x c] (row r * T + t) -> [k * P * T x c] in the batch layout (row r * (P * T) + p * T + t)."""
    P = len(rows_per_path)
    T = rows_per_path[0].shape[0] // k
    g = torch.stack([torch.as_tensor(x).reshape(k, T, -1) for x in rows_per_path], 1)   # [k][P][T][c]
    return g.reshape(k * P * T, -1).contiguous()


def from_batch(rows, P, T, k, p):
    """The rows of path p of a batch layout [k * P * T (x c)] gathered into its own tile-major block [k * T (x c)]."""
    a = np.asarray(rows)
    g = a.reshape((k, P, T) + a.shape[1:])
    return np.ascontiguousarray(g[:, p].reshape((k * T,) + a.shape[1:]))


def split(out, P, T, k):
    """The outputs of a batch call {path [P * T x nd], index, cost [P], reach, node [k * P * T]} -> a list of P single-call dicts."""
    res = []
    for p in range(P):
        one = {"path": out["path"][p * T:(p + 1) * T], "index": out["index"][p * T:(p + 1) * T], "cost": out["cost"][p:p + 1],
               "reach": out["reach"][p * T:(p + 1) * T]}
        if "node" in out:
            one["node"] = from_batch(out["node"], P, T, k, p)
        res.append(one)
    return res


# ---- the swept cases ------------------------------------------------------------------------------------------------------------------------------
# Condition of a swept case, by the references alone: under the case's thresholds and step gate NO unpruned edge of any of its P lattices is in
# sweep_helpers' BAND.  Then the verdict of every edge the search can take is decided by the fp64 reference, and the BATCH form of the sweep kernel
# and its single form - which the compiler may contract differently - must agree on it.  Unpruned: the step gate allows the edge (float32, exact)
# and both of its nodes are live.  With all k * k edges of a 65-candidate lattice some sample always lies within 1e-4 of any threshold, so
#   - at k > SWEEP_LIVE only SWEEP_LIVE candidates of a waypoint are live, chosen per waypoint from the seed across the whole index range (both mask
#     words at k = 65); the rows of the others are NaN, which makes their nodes inadmissible whatever the thresholds are - exactly, with no band;
#   - the thresholds are not quantiles: each sits in the middle of the widest gap the pooled reference clearances (live nodes and the samples of the
#     unpruned edges of all P lattices) leave between their SWEEP_WINDOW quantiles - the unpruned set does not depend on the thresholds, so this is
#     one pass.  A live node is then surely admissible or surely not, and so is every sample.
# tests/test_path_batch.py asserts the condition on these references before it looks at the engine.  The seed of a case is the first of 0, 1, ...
# for which it holds with surely blocked and surely free unpruned edges in the batch (found on the CPU).
SWEEP_WHICH = "panda"
SWEEP_LIVE = 6
SWEEP_GATE = 0.6          # rad: forbids the edges to and from the candidates with the largest noise
SWEEP_WINDOW = (0.02, 0.15)
SWEEP_SEEDS = {(2, 9, 65, 4, False): 1, (2, 9, 65, 4, True): 1}   # (P, T, k, S, with q_start) -> seed; 0 where not listed
_SWEEP_CASES = {}


def _gap_threshold(values):
    """The middle of the widest gap between consecutive sorted values inside their SWEEP_WINDOW quantiles, and that gap's width."""
    v = np.sort(np.asarray(values, np.float64))
    lo, hi = (int(f * (len(v) - 1)) for f in SWEEP_WINDOW)
    gaps = np.diff(v[lo:hi + 1])
    i = int(np.argmax(gaps))
    return float(0.5 * (v[lo + i] + v[lo + i + 1])), float(gaps[i])


def sweep_case(P, T, k, S, with_start, seed=None):
    """-> dict: poses [P * T x 7], q [k * P * T x nd] (batch layout, NaN rows for the candidates that are not live), q_start [P x nd] or None, world,
    world_thr, self_thr, gate, gaps (the widths of the two gaps the thresholds sit in) and - by the fp64 reference - per lattice the numbers
    (unpruned, surely blocked, surely free, band) of its edges.  Computed once."""
    seed = SWEEP_SEEDS.get((P, T, k, S, with_start), 0) if seed is None else seed
    key = (P, T, k, S, with_start, seed)
    if key in _SWEEP_CASES:
        return _SWEEP_CASES[key]
    robot, orob = H.kin_robots(SWEEP_WHICH)
    caps = RH.collision_capsules(robot)
    rng = np.random.default_rng(7700 + seed)
    singles, lives, edges = [], [], []
    for p in range(P):
        poses, q, q_true = SH.path_inputs(orob, T, k, 1000 * seed + 37 * p + T + k)
        live = np.ones((k, T), bool)
        if k > SWEEP_LIVE:
            live[:] = False
            for t in range(T):
                live[rng.choice(k, SWEEP_LIVE, replace=False), t] = True
            live[k - 1, 0] = True                                      # (the last candidate, alone in the last mask word at k = 65)
        q = q.clone()
        q[torch.tensor(~live.reshape(-1))] = float("nan")
        start = (q_true[0] + 0.05).contiguous() if with_start else None
        a, b = SH.lattice_edges(q.numpy(), T, k, None if start is None else start.numpy())
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(a).all(1) & np.isfinite(b).all(1) & ~(np.abs(b - a) > F(SWEEP_GATE)).any(1)
        singles.append((poses, q, start))
        lives.append(live)
        edges.append((a[ok], b[ok]))
    world = WH.scene(SWEEP_WHICH, SH.LATTICE_SCENE)
    node_q = torch.cat([s[1][torch.tensor(lv.reshape(-1))] for s, lv in zip(singles, lives)])
    node_w = WH.reference(orob, caps, world, node_q)["clearance"]
    node_s = RH.clearance(orob, caps, node_q)
    smp = [SH.sample_clearances(orob, caps, world, SH.samples_f32(a, b, S)) for a, b in edges]
    world_thr, gap_w = _gap_threshold(np.concatenate([node_w] + [w.reshape(-1) for w, _ in smp]))
    self_thr, gap_s = _gap_threshold(np.concatenate([node_s] + [s.reshape(-1) for _, s in smp]))
    counts = []
    for (a, _), (w_s, s_s) in zip(edges, smp):
        v = SH.verdicts(w_s, world_thr, s_s, self_thr)
        counts.append((int(a.shape[0]), int(v["blocked"].sum()), int(v["free"].sum()), int(v["band"].sum())))
    node_band = int(((np.abs(node_w - world_thr) <= SH.BAND) | (np.abs(node_s - self_thr) <= SH.BAND)).sum())
    c = dict(poses=torch.cat([s[0] for s in singles]).contiguous(), q=to_batch([s[1] for s in singles], k),
             q_start=torch.stack([s[2] for s in singles]).contiguous() if with_start else None, world=world, world_thr=world_thr, self_thr=self_thr,
             gate=SWEEP_GATE, gaps=(gap_w, gap_s), counts=counts, node_band=node_band)
    _SWEEP_CASES[key] = c
    return c


def sweep_condition_holds(c):
    """No unpruned edge and no live node in the band, and the batch holds surely blocked and surely free unpruned edges."""
    return (all(band == 0 for _, _, _, band in c["counts"]) and c["node_band"] == 0 and sum(b for _, b, _, _ in c["counts"]) > 0
            and sum(f for _, _, f, _ in c["counts"]) > 0)
