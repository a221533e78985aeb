"""The arithmetic of diverse-of-K IK (ikflow_amd/csrc/diverse_math.h: dist2, the near2 update, the two total orders with their merges, the stop
rule, launch geometry) compiled for the HOST with g++ -ffp-contract=off and held, bit for bit, against sequential numpy float32 arithmetic
(tests/diverse_helpers.py), against the header's two guarantees and against brute force over all subsets in fp64 - the kernel's own source,
checked without a GPU.  The GPU tests check the same code where it ships (tests/test_diverse.py).  Test infrastructure: nothing in ikflow_amd/
loads it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import diverse_helpers as DH
from ikflow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("diverse_math") / "libdiverse_math_host.so"
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "diverse_math_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(str(out))
    lib.diverse_host_select.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.diverse_host_dist2.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.diverse_host_dist2.restype = C.c_float
    lib.diverse_host_lds_bytes.restype = C.c_longlong
    return lib


def _select(lib, q, score, n_keep, min_sep=0.0, w=None, n_slices=1, order=None):
    k, nd = q.shape
    q, score = np.ascontiguousarray(q, F), np.ascontiguousarray(score, F)
    wv = None if w is None else np.ascontiguousarray(w, F)
    order = np.ascontiguousarray(np.arange(n_slices) if order is None else order, np.int32)
    out = {"q_out": np.full((n_keep, nd), np.nan, F), "score": np.full(n_keep, np.nan, F), "index": np.full(n_keep, -7, np.int32),
           "sep": np.full(n_keep, np.nan, F)}
    kept, count = C.c_int(-7), C.c_int(-7)
    assert lib.diverse_host_select(nd, q.ctypes.data, score.ctypes.data, k, n_keep, min_sep, None if wv is None else wv.ctypes.data, n_slices,
                                   order.ctypes.data, out["q_out"].ctypes.data, out["score"].ctypes.data, out["index"].ctypes.data,
                                   out["sep"].ctypes.data, C.byref(kept), C.byref(count)) == 0
    out["kept"], out["count"] = kept.value, count.value
    return out


def _same(got, want):
    return all(DH.same_bits(np.asarray(got[n]), np.asarray(want[n]).astype(np.asarray(got[n]).dtype)) for n in DH.NAMES)


def _early_sep(q, score, n_keep, w=None):
    """A min_separation that stops this pose's selection early: between the separations of the second and the last pick of the free run, or -
    where the free run has only two picks - above the second pick's, so that slot 0 stays alone.  None when there is nothing to stop."""
    free = DH.select_f32(q, score, n_keep, 0.0, w)
    seps = free["sep"][1:free["kept"]]
    if len(seps) >= 2 and seps[-1] < seps[0]:
        return float(F(0.5) * (seps[0] + seps[-1]))
    return float(F(2.0) * seps[0] + F(1.0)) if len(seps) >= 1 else None


@pytest.mark.parametrize("k", [1, 2, 5, 64, 65, 257, 1024])
def test_bit_for_bit_against_sequential_numpy_float32(host_lib, k):
    """Every output identical to the numpy float32 selection: ndof 4 to 8, n_keep 1 / 2 / 16 where k allows, min_separation 0 and a value that
    stops the selection early, with and without weights (one of them 0), with a sprinkling of +inf scores."""
    stopped = 0
    for nd in range(4, 9):
        q, score = DH.random_pose(k, nd, 100 * k + nd, n_inf=k // 5)
        w = np.linspace(0.0, 2.0, nd).astype(F)           # w_0 = 0: joint 0 does not count
        for n_keep in [n for n in (1, 2, 16) if n <= k]:
            for wv in (None, w):
                for sep in (0.0, _early_sep(q, score, n_keep, wv)):
                    if sep is None:
                        continue
                    got = _select(host_lib, q, score, n_keep, sep, wv)
                    want = DH.select_f32(q, score, n_keep, sep, wv)
                    assert _same(got, want), (k, nd, n_keep, sep, wv is not None, got["index"], want["index"])
                    DH.check_guarantees(q, score, got["index"], got["kept"], n_keep, sep, wv)
                    if sep == 0.0:
                        assert got["kept"] == min(n_keep, got["count"])
                    else:
                        assert 1 <= got["kept"] < n_keep
                        stopped += 1
    assert stopped > 0 or k < 2


def test_dist2_is_the_headers_sum_in_order_and_not_fused(host_lib):
    """dist2 against the explicit float32 loop on values whose fused and pairwise sums differ; symmetric bit for bit; a zero weight removes a joint."""
    rng = np.random.default_rng(0)
    differs_from_pairwise = 0
    for nd in range(4, 9):
        for _ in range(200):
            a, b = rng.normal(0, 2.0, nd).astype(F), rng.normal(0, 2.0, nd).astype(F)
            w = rng.uniform(0, 3, nd).astype(F)
            for wv in (None, w):
                got = host_lib.diverse_host_dist2(nd, a.ctypes.data, b.ctypes.data, None if wv is None else wv.ctypes.data)
                assert F(got) == DH.dist2_f32(a, b, wv)
                assert F(got) == F(host_lib.diverse_host_dist2(nd, b.ctypes.data, a.ctypes.data, None if wv is None else wv.ctypes.data))
            d = a - b
            differs_from_pairwise += int(np.sum(d * d) != DH.dist2_f32(a, b))
    assert differs_from_pairwise > 0        # (at ndof 8 np.sum adds pairwise: the reference must not use it)
    a, b = np.array([1, 2, 3, 4], F), np.array([9, 2, 3, 5], F)
    w0 = np.array([0, 1, 1, 1], F)
    assert host_lib.diverse_host_dist2(4, a.ctypes.data, b.ctypes.data, w0.ctypes.data) == 1.0
    assert host_lib.diverse_host_dist2(4, a.ctypes.data, b.ctypes.data, None) == 65.0


@pytest.mark.parametrize("k,nd", [(5, 7), (65, 6), (257, 8), (1024, 4)])
def test_any_split_of_the_candidates_gives_the_same_picks(host_lib, k, nd):
    """1, 2, 7 and 64 slices, merged in forward, reverse and a random order: identical outputs (rows duplicated so that ties occur)."""
    q, score = DH.random_pose(k, nd, k, n_inf=k // 7)
    if k > 4:
        q[k - 1], q[k // 2] = q[1], q[1]
        score[k - 1] = score[0]
    n_keep = min(k, 16)
    ref = _select(host_lib, q, score, n_keep)
    assert _same(ref, DH.select_f32(q, score, n_keep))
    rng = np.random.default_rng(1)
    for n_slices in (2, 7, 64):
        for order in (np.arange(n_slices), np.arange(n_slices)[::-1], rng.permutation(n_slices)):
            assert _same(_select(host_lib, q, score, n_keep, n_slices=n_slices, order=order), ref), (n_slices, order)


def test_ties_go_to_the_lower_index(host_lib):
    """Exact duplicate rows: the lower r is picked first; with min_separation 0 the duplicate is kept too, with separation 0; with a positive
    min_separation never.  Equal scores in slot 0 go to the lower r."""
    nd, k = 7, 6
    q, score = DH.random_pose(k, nd, 5)
    q[:] = 0
    q[1], q[4] = 3.0, 3.0                                   # rows 1 and 4 equal and farthest from the rest (all 0)
    score[:] = 0.01
    score[2] = score[5] = 0.001                             # slot 0: rows 2 and 5 tie -> 2
    for n_slices in (1, 2, 7):
        got = _select(host_lib, q, score, k, n_slices=n_slices, order=np.arange(n_slices)[::-1])
        assert list(got["index"]) == [2, 1, 0, 3, 4, 5] and got["kept"] == k, got["index"]
        assert np.isposinf(got["sep"][0]) and got["sep"][1] == np.sqrt(F(63.0)) and (got["sep"][2:] == 0).all()
        assert _same(got, DH.select_f32(q, score, k))
        pos = _select(host_lib, q, score, k, min_sep=1e-3, n_slices=n_slices)
        assert list(pos["index"]) == [2, 1, -1, -1, -1, -1] and pos["kept"] == 2 and pos["count"] == k
        assert (pos["q_out"][2:] == 0).all() and np.isposinf(pos["score"][2:]).all() and np.isposinf(pos["sep"][2:]).all()
        assert _same(pos, DH.select_f32(q, score, k, 1e-3))
        DH.check_guarantees(q, score, pos["index"], pos["kept"], k, 1e-3)


def test_inadmissible_and_nan_rows(host_lib):
    """All rows inadmissible: nothing kept, every slot 0 / +inf / -1 / +inf.  All but one: that one, alone.  NaN rows (score +inf, as the score
    stage gives them) are never picked and change nothing for the others."""
    nd, k = 6, 9
    q, score = DH.random_pose(k, nd, 2)
    none = _select(host_lib, q, np.full(k, np.inf, F), 4)
    assert none["kept"] == 0 and none["count"] == 0 and (none["index"] == -1).all() and (none["q_out"] == 0).all()
    assert np.isposinf(none["score"]).all() and np.isposinf(none["sep"]).all()
    one = np.full(k, np.inf, F)
    one[6] = 0.5
    got = _select(host_lib, q, one, 4)
    assert got["kept"] == 1 and got["count"] == 1 and list(got["index"]) == [6, -1, -1, -1] and DH.same_bits(got["q_out"][0], q[6])
    assert _same(got, DH.select_f32(q, one, 4))
    qn, sn = q.copy(), score.copy()
    qn[3], sn[3] = np.nan, np.inf
    qn[7, 2], sn[7] = np.nan, np.inf
    got = _select(host_lib, qn, sn, k)
    assert got["kept"] == k - 2 and got["count"] == k - 2 and 3 not in got["index"] and 7 not in got["index"]
    assert np.isfinite(got["q_out"][:k - 2]).all() and np.isfinite(got["sep"][1:k - 2]).all()
    clean = _select(host_lib, np.where(np.isnan(qn), F(123.0), qn), sn, k)
    assert _same(got, clean)                               # (what an inadmissible row holds - NaN or a number - changes nothing)
    assert _same(got, DH.select_f32(qn, sn, k))


def test_greedy_is_within_the_farthest_first_bound_of_the_best_subset(host_lib):
    """k = 9 (two rows duplicated, two inadmissible), n = 2 .. 4: the greedy set's smallest pairwise distance is at least 0.5 (1 - 1e-6) of the
    best n-subset's, brute force in fp64.  0.5: the balls of half the optimal radius around the optimal set are disjoint, and fewer picks
    than balls leave one empty - from any first pick."""
    worst = 1.0
    for seed in range(40):
        nd = 4 + seed % 5
        q, score = DH.random_pose(9, nd, 700 + seed, n_inf=2)
        adm = np.flatnonzero(np.isfinite(score))
        q[adm[1]] = q[adm[0]]                               # a duplicate among the admissible rows
        w = None if seed % 2 else np.linspace(0.5, 2.0, nd).astype(F)
        for n in (2, 3, 4):
            got = _select(host_lib, q, score, n, w=w)
            assert got["kept"] == n
            greedy = DH.min_pairwise_f64(q, got["index"], w)
            best = DH.best_subset_f64(q, score, n, w)
            assert greedy >= 0.5 * (1 - 1e-6) * best, (seed, n, greedy, best)
            worst = min(worst, greedy / best)
    print(f"greedy / best smallest pairwise distance: worst {worst:.3f} (bound 0.5)")


def test_geometry_and_constants_agree_with_the_binding(host_lib):
    c = (C.c_int * 6)()
    host_lib.diverse_host_constants(c)
    max_k, max_keep, bmin, bmax, per, opt_bytes = list(c)
    assert max_k == _lib.IKF_DIVERSE_MAX_K == 1024 and max_keep == _lib.IKF_DIVERSE_MAX_KEEP == 16 and (bmin, bmax, per) == (64, 256, 4)
    assert opt_bytes == C.sizeof(_lib.ikf_diverse_options) == 32
    for k in range(1, max_k + 1):
        b = host_lib.diverse_host_block(k)
        assert 64 <= b <= 256 and b & (b - 1) == 0 and b * 4 >= k and (b == 64 or (b // 2) * 4 < k), (k, b)
    for nd in range(4, 9):
        rs = host_lib.diverse_host_row_stride(nd)
        assert rs >= nd and rs % 2 == 1
        assert host_lib.diverse_host_lds_bytes(nd, max_k) == 4 * max_k * (rs + 1) <= 40 * 1024
