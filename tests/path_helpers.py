"""The references of path IK (include/ikflow_amd_path.h), shared by the host build of ikflow_amd/csrc/path_math.h (tests/test_path_math_host.py)
and the GPU tests (tests/test_path.py): the lattice as sequential numpy float32 arithmetic - which the engine must reproduce bit for bit, given
the same node costs, because every step of it is rounded on its own - and brute force over all k^T paths in fp64."""
import itertools
import os
import re

import numpy as np

from helpers import same_bits  # noqa: F401  (used as PH.same_bits)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)


def backtrack_chunk():
    """IKF_PATH_BT_CHUNK of ikflow_amd/csrc/path_math.h: the waypoints of back-pointers the walk back stages at a time."""
    text = open(os.path.join(ROOT, "ikflow_amd", "csrc", "path_math.h")).read()
    return int(re.search(r"constexpr int IKF_PATH_BT_CHUNK = (\d+);", text).group(1))


def dp_f32(q, node, T, k, q_start=None, node_weight=1.0, max_step=None):
    """q [k * T x ndof] tile-major f32, node [k * T] f32 -> (path [T x ndof] f32, index [T] int32, cost f32, n_reachable [T] int32), every operation
    a float32 numpy operation in the order the header defines: d = b_j - a_j, s = s + d * d for j = 0 .. ndof - 1, sqrt, cost + edge,
    + node_weight * node.  np.argmin returns the first minimum, i.e. the lower index on ties."""
    q = np.ascontiguousarray(q, dtype=F)
    nd = q.shape[1]
    q = q.reshape(k, T, nd)
    node = np.asarray(node, dtype=F).reshape(k, T)
    nw = F(node_weight)
    step = None if max_step is None or max_step < 0 else F(max_step)
    cost = np.full((T, k), INF, F)
    back = np.zeros((T, k), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        def edges(a, b):   # a [n x nd] predecessors, b [m x nd] destinations -> e [n x m] f32, allowed [n x m]
            s = np.zeros((a.shape[0], b.shape[0]), F)
            ok = np.ones(s.shape, bool)
            for j in range(nd):
                d = b[None, :, j] - a[:, None, j]
                if step is not None:
                    ok &= ~(np.abs(d) > step)
                s = s + d * d
            return np.sqrt(s), ok

        for t in range(T):
            if t == 0:
                if q_start is None:
                    sums = np.zeros((1, k), F)
                else:
                    e, ok = edges(np.asarray(q_start, F).reshape(1, nd), q[:, 0])
                    sums = np.where(ok, F(0.0) + e, INF)
            else:
                e, ok = edges(q[:, t - 1], q[:, t])
                sums = cost[t - 1][:, None] + e
                sums = np.where(ok & (cost[t - 1] < INF)[:, None], sums, INF)
            sums = np.where(sums < INF, sums, INF).astype(F)
            j = np.argmin(sums, axis=0)
            best = sums[j, np.arange(k)]
            c = best + nw * node[:, t]
            c = np.where((node[:, t] < INF) & (best < INF) & (c < INF), c, INF).astype(F)
            cost[t], back[t] = c, j
    reach = (cost < INF).sum(1).astype(np.int32)
    if not (cost[T - 1] < INF).any():
        return np.zeros((T, nd), F), np.full(T, -1, np.int32), INF, reach
    index = np.zeros(T, np.int32)
    index[T - 1] = int(np.argmin(cost[T - 1]))
    for t in range(T - 1, 0, -1):
        index[t - 1] = back[t, index[t]]
    return q[index, np.arange(T)].copy(), index, cost[T - 1, index[T - 1]], reach


def brute_force_f64(q, node, T, k, q_start=None, node_weight=1.0, max_step=None):
    """All k^T paths in fp64 -> (index [T], total) of the cheapest admissible one, (None, inf) without one."""
    nd = q.shape[1]
    q64 = np.asarray(q, np.float64).reshape(k, T, nd)
    n64 = np.asarray(node, np.float64).reshape(k, T)
    best, best_idx = np.inf, None
    for idx in itertools.product(range(k), repeat=T):
        rows = q64[list(idx), np.arange(T)]
        if q_start is not None:
            rows = np.concatenate([np.asarray(q_start, np.float64)[None], rows])
        d = np.diff(rows, axis=0)
        if max_step is not None and d.size and np.abs(d).max() > max_step:
            continue
        total = np.sqrt((d * d).sum(1)).sum() + node_weight * n64[list(idx), np.arange(T)].sum()
        if total < best:
            best, best_idx = total, np.array(idx, np.int32)
    return best_idx, best


def random_lattice(T, k, nd, seed, spread=0.3):
    """Candidate rows around a slowly moving centre, and node costs of a few millimetres: (q [k * T x nd] tile-major f32, node [k * T] f32)."""
    rng = np.random.default_rng(seed)
    centre = np.cumsum(rng.normal(0.0, 0.05, (T, nd)), 0)
    q = centre[None] + rng.normal(0.0, spread, (k, T, nd))
    node = rng.uniform(1e-4, 2e-2, (k, T))
    return q.reshape(k * T, nd).astype(F), node.reshape(k * T).astype(F)
