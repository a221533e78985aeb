"""The references of diverse-of-K IK (include/ikflow_amd_diverse.h), shared by the host build of ikflow_amd/csrc/diverse_math.h
(tests/test_diverse_math_host.py) and the GPU tests (tests/test_diverse.py): the farthest-point selection as sequential numpy float32
arithmetic - which the engine must reproduce bit for bit, given the same row scores, because every step of it is rounded on its own - the two
guarantees of the header checked in that arithmetic, and brute force over all subsets in fp64."""
import itertools

import numpy as np

from helpers import same_bits  # noqa: F401  (used as DH.same_bits)

F = np.float32
INF = F(np.inf)


def dist2_f32(a, b, w=None):
    """a [... x nd], b [nd] f32 -> dist2 [...] f32: an explicit loop over j, every operation a float32 numpy operation in the header's order
    (np.sum is pairwise from 8 elements up and is NOT that order)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    s = np.zeros(a.shape[:-1], F)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(a.shape[-1]):
            d = a[..., j] - b[j]
            if w is not None:
                d = d * F(w[j])
            s = s + d * d
    return s.astype(F)


def select_f32(q, score, n_keep, min_separation=0.0, w=None):
    """One pose: q [k x nd] f32, score [k] f32 (+inf: inadmissible) -> dict(q_out [n_keep x nd], score [n_keep], index [n_keep] int32,
    sep [n_keep], kept, count), the definition of include/ikflow_amd_diverse.h step by step."""
    q, score = np.ascontiguousarray(q, F), np.asarray(score, F)
    k, nd = q.shape
    w = None if w is None else np.asarray(w, F)
    sep2 = F(min_separation) * F(min_separation)
    out = {"q_out": np.zeros((n_keep, nd), F), "score": np.full(n_keep, INF, F), "index": np.full(n_keep, -1, np.int32), "sep": np.full(n_keep, INF, F)}
    alive = score < INF
    out["count"], kept = int(alive.sum()), 0
    if alive.any():
        masked = np.where(alive, score, INF)
        p = int(np.argmin(masked))                        # the first minimum: the lower r on ties
        near2 = np.full(k, INF, F)
        out["q_out"][0], out["score"][0], out["index"][0], kept = q[p], score[p], p, 1
        for i in range(1, n_keep):
            alive[p] = False
            d2 = dist2_f32(q, q[p], w)
            near2 = np.where(d2 < near2, d2, near2)       # (a NaN d2 leaves near2 as it is)
            cand = np.flatnonzero(alive & ~np.isnan(near2))   # (a NaN near2 beats nothing)
            if cand.size == 0:
                break
            mx = near2[cand].max()
            if not mx >= sep2:
                break
            p = int(cand[near2[cand] == mx][0])           # the lower r on ties
            with np.errstate(invalid="ignore"):
                out["q_out"][i], out["score"][i], out["index"][i], out["sep"][i], kept = q[p], score[p], p, np.sqrt(mx), i + 1
    out["kept"] = kept
    return out


NAMES = ("q_out", "score", "index", "sep", "kept", "count")


def select_poses(q, row_score, m, k, n_keep, min_separation=0.0, w=None):
    """Tile-major q [k * m x nd], row_score [k * m] -> {q_out [m x n_keep x nd], score / index / sep [m x n_keep], kept / count [m] int32}."""
    q = np.ascontiguousarray(q, F)
    nd = q.shape[1]
    qk, sk = q.reshape(k, m, nd), np.asarray(row_score, F).reshape(k, m)
    per = [select_f32(qk[:, j], sk[:, j], n_keep, min_separation, w) for j in range(m)]
    out = {n: np.stack([p[n] for p in per]) for n in ("q_out", "score", "index", "sep")}
    out["kept"] = np.array([p["kept"] for p in per], np.int32)
    out["count"] = np.array([p["count"] for p in per], np.int32)
    return out


def check_guarantees(q, score, index, kept, n_keep, min_separation, w=None):
    """The header's two guarantees for one pose, exactly, in the f32 arithmetic of the definition: kept rows pairwise dist2 >= sep2; when
    kept < n_keep, every admissible row that was not kept has dist2 < sep2 to some kept row."""
    q, score = np.ascontiguousarray(q, F), np.asarray(score, F)
    sep2 = F(min_separation) * F(min_separation)
    rows = [int(r) for r in index[:kept]]
    assert len(set(rows)) == kept and all(score[r] < INF for r in rows)
    for a, b in itertools.combinations(rows, 2):
        assert dist2_f32(q[a], q[b], w) >= sep2 and dist2_f32(q[b], q[a], w) >= sep2, (a, b)
    if kept < n_keep and kept > 0:
        near = np.min(np.stack([dist2_f32(q, q[r], w) for r in rows]), 0)
        rest = (score < INF) & ~np.isin(np.arange(len(score)), rows)
        assert (near[rest] < sep2).all(), np.flatnonzero(rest & ~(near < sep2))[:5]
    if kept == 0:
        assert not (score < INF).any()


def min_pairwise_f64(q, rows, w=None):
    q64 = np.asarray(q, np.float64)[list(rows)]
    if w is not None:
        q64 = q64 * np.asarray(w, np.float64)
    return min(np.sqrt(((a - b) ** 2).sum()) for a, b in itertools.combinations(q64, 2))


def best_subset_f64(q, score, n, w=None):
    """The greatest smallest-pairwise-distance over all n-subsets of the admissible rows, in fp64."""
    adm = np.flatnonzero(np.asarray(score, F) < INF)
    return max(min_pairwise_f64(q, sub, w) for sub in itertools.combinations(adm, n))


def random_pose(k, nd, seed, spread=0.6, n_inf=0):
    """k rows in a few clusters (the flow's solution families) and scores of a few millimetres, n_inf of them +inf."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 1.5, (4, nd))
    q = centres[rng.integers(0, 4, k)] + rng.normal(0.0, spread, (k, nd))
    score = rng.uniform(1e-4, 2e-2, k)
    if n_inf:
        score[rng.choice(k, min(n_inf, k), replace=False)] = np.inf
    return q.astype(F), score.astype(F)
