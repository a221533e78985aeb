"""The arithmetic of path IK (ikflow_amd/csrc/path_math.h: edge, relaxation with the skip rule and the total order, slice merge, end of the path,
walk back in chunks, launch geometry) compiled for the HOST with g++ -ffp-contract=off and held against brute force over all paths in fp64 and,
bit for bit, against sequential numpy float32 arithmetic - the kernels' own source, checked without a GPU.  The GPU tests check the same code
where it ships (tests/test_path.py).  Test infrastructure: nothing in ikflow_amd/ loads it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import path_helpers as PH
from ikflow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("path_math") / "libpath_math_host.so"
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "path_math_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(str(out))
    lib.path_host_lattice.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.path_host_edge7.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    lib.path_host_edge7.restype = C.c_float
    for name in ("path_host_stages", "path_host_bt_chunks"):
        getattr(lib, name).argtypes = [C.c_longlong]
        getattr(lib, name).restype = C.c_longlong
    lib.path_host_bp_bytes.argtypes = [C.c_longlong, C.c_int]
    lib.path_host_bp_bytes.restype = C.c_longlong
    return lib


def _lattice(lib, q, node, T, k, q_start=None, node_weight=1.0, max_step=None, n_slices=1, order=None, chunk=0):
    nd = q.shape[1]
    q, node = np.ascontiguousarray(q, F), np.ascontiguousarray(node, F)
    qs = None if q_start is None else np.ascontiguousarray(q_start, F)
    order = np.ascontiguousarray(np.arange(n_slices) if order is None else order, np.int32)
    path, index, cost, reach = np.full((T, nd), np.nan, F), np.full(T, -7, np.int32), np.full(1, np.nan, F), np.full(T, -7, np.int32)
    assert lib.path_host_lattice(nd, q.ctypes.data, node.ctypes.data, T, k, None if qs is None else qs.ctypes.data, node_weight,
                                 -1.0 if max_step is None else max_step, n_slices, order.ctypes.data, chunk, path.ctypes.data, index.ctypes.data,
                                 cost.ctypes.data, reach.ctypes.data) == 0
    return path, index, cost[0], reach


def _same(got, want):
    return PH.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and PH.same_bits(F(got[2]), F(want[2])) and np.array_equal(got[3], want[3])


@pytest.mark.parametrize("T", [1, 2, 4])
def test_the_cheapest_of_all_paths_in_fp64(host_lib, T):
    """k = 3, every one of the 3^T paths summed in fp64: the same path (the costs of random rows are far apart against f32 rounding), the total within
    1e-5 relative; with and without q_start, with node_weight 0 / 1 / 50 (motion only, the default, pose error dominating)."""
    k, nd = 3, 7
    for seed in range(6):
        q, node = PH.random_lattice(T, k, nd, seed)
        q_start = None if seed % 2 else np.random.default_rng(seed).normal(0, 0.3, nd).astype(F)
        for nw in (0.0, 1.0, 50.0):
            path, index, cost, reach = _lattice(host_lib, q, node, T, k, q_start, nw)
            want_idx, want = PH.brute_force_f64(q, node, T, k, q_start, nw)
            assert np.array_equal(index, want_idx), (T, seed, nw)
            assert abs(float(cost) - want) <= 1e-5 * max(want, 1e-30), (T, seed, nw, float(cost), want)
            assert PH.same_bits(path, q.reshape(k, T, nd)[index, np.arange(T)]) and (reach == k).all()


CASES = [(1, 1, False), (5, 1, False), (1, 9, False), (33, 65, False), (256, 40, True), (256, 40, False)]


@pytest.mark.parametrize("k,T,with_start", CASES)
def test_bit_for_bit_against_sequential_numpy_float32(host_lib, k, T, with_start):
    """Cost, indices, path and n_reachable identical to the numpy float32 lattice - plain, with the step gate (which forbids about a third of the
    edges), and with a sprinkling of inadmissible nodes."""
    nd = 7
    q, node = PH.random_lattice(T, k, nd, 100 + k + T)
    q_start = np.random.default_rng(k).normal(0, 0.3, nd).astype(F) if with_start else None
    holes = node.copy()
    holes[np.random.default_rng(T).random(k * T) < 0.2] = np.inf
    for nodes, step in ((node, None), (node, 1.0), (holes, None)):
        if k == 1 and nodes is holes:
            nodes = node
        got = _lattice(host_lib, q, nodes, T, k, q_start, 3.0, step)
        want = PH.dp_f32(q, nodes, T, k, q_start, 3.0, step)
        assert _same(got, want), (k, T, with_start, step, float(got[2]), float(want[2]))
        if k > 1 and step is None:
            assert np.isfinite(got[2]) and (got[1] >= 0).all()


def test_ties_go_to_the_lower_index(host_lib):
    """Every candidate of a waypoint the same row and node cost: index 0 everywhere.  Candidates 2 and 4 duplicated and cheapest: 2 at the step and
    at the end."""
    T, k, nd = 6, 5, 7
    q, node = PH.random_lattice(T, 1, nd, 3)
    q, node = np.tile(q.reshape(1, T, nd), (k, 1, 1)).reshape(k * T, nd), np.tile(node.reshape(1, T), (k, 1)).reshape(k * T)
    got = _lattice(host_lib, q, node, T, k)
    assert (got[1] == 0).all() and _same(got, PH.dp_f32(q, node, T, k))
    q2, node2 = PH.random_lattice(T, k, nd, 4)
    q2, node2 = q2.reshape(k, T, nd), node2.reshape(k, T)
    q2[2] = q2[4] = np.float32(0.001) * q2[2]
    node2[2] = node2[4] = 1e-6
    for n_slices in (1, 2, 4):
        got = _lattice(host_lib, q2.reshape(k * T, nd), node2.reshape(k * T), T, k, n_slices=n_slices, order=np.arange(n_slices)[::-1])
        assert (got[1] == 2).all(), got[1]


def test_step_gate_forbids_exactly_the_cheapest_edge(host_lib):
    """Two waypoints; the cheapest path uses the edge 0 -> 0.  A max_joint_step just below that edge's largest joint move forbids it and only it (every
    other edge moves every joint by less), so the search must take another path; just above, it keeps the path."""
    T, k, nd = 2, 3, 7
    q = np.zeros((k, T, nd), F)
    q[0, 1, 0] = 0.5                                             # edge 0 -> 0: one joint moves 0.5, every other edge moves every joint by <= 0.4
    q[1, 0], q[2, 0] = 0.3, 0.4
    q[1, 1], q[2, 1] = 0.4, 0.3
    node = np.tile(np.array([[1e-3], [2.0], [2.0]], F), (1, T)).reshape(k * T)   # candidate 0 is far cheaper to be at: 0 -> 0 is the cheapest path
    qf = q.reshape(k * T, nd)
    gate = float(np.nextafter(F(0.5), F(0)))
    forbidden = []
    for i in range(k):
        for j in range(k):
            ok = C.c_int(0)
            host_lib.path_host_edge7(q[i, 0].ctypes.data, q[j, 1].ctypes.data, gate, C.byref(ok))
            forbidden += [] if ok.value else [(i, j)]
    assert forbidden == [(0, 0)]
    free = _lattice(host_lib, qf, node, T, k)
    assert list(free[1]) == [0, 0]
    above = _lattice(host_lib, qf, node, T, k, max_step=0.5)     # |d| > step is strict: a move of exactly 0.5 passes
    assert list(above[1]) == [0, 0] and _same(above, PH.dp_f32(qf, node, T, k, max_step=0.5))
    below = _lattice(host_lib, qf, node, T, k, max_step=gate)
    assert list(below[1]) != [0, 0] and np.isfinite(below[2]) and below[2] > free[2]
    assert _same(below, PH.dp_f32(qf, node, T, k, max_step=gate))
    a, b, ok = np.zeros(7, F), np.zeros(7, F), C.c_int(0)
    b[3] = 0.25
    assert host_lib.path_host_edge7(a.ctypes.data, b.ctypes.data, 0.2, C.byref(ok)) == F(0.25) and ok.value == 0
    assert host_lib.path_host_edge7(a.ctypes.data, b.ctypes.data, -1.0, C.byref(ok)) == F(0.25) and ok.value == 1


def test_blocked_waypoint_and_nan_rows(host_lib):
    """A waypoint whose nodes are all +inf: no path, n_reachable 0 from there on, outputs 0 / -1 / +inf.  A NaN row (node +inf, as the node stage scores
    it) is never chosen and changes nothing for its neighbours: the other candidates' path is that of the lattice without it.  node_weight 0 with an
    inadmissible node stays inadmissible (0 x inf never enters a sum)."""
    T, k, nd = 9, 5, 7
    q, node = PH.random_lattice(T, k, nd, 8)
    blocked = node.reshape(k, T).copy()
    blocked[:, 4] = np.inf
    got = _lattice(host_lib, q, blocked.reshape(-1), T, k)
    assert np.isposinf(got[2]) and (got[1] == -1).all() and (got[0] == 0).all()
    assert (got[3][:4] == k).all() and (got[3][4:] == 0).all() and _same(got, PH.dp_f32(q, blocked.reshape(-1), T, k))
    qn, nn = q.reshape(k, T, nd).copy(), node.reshape(k, T).copy()
    qn[1, 3], nn[1, 3] = np.nan, np.inf
    qn[3, 0, 2], nn[3, 0] = np.nan, np.inf
    for nw in (1.0, 0.0):
        got = _lattice(host_lib, qn.reshape(k * T, nd), nn.reshape(-1), T, k, node_weight=nw)
        assert np.isfinite(got[2]) and np.isfinite(got[0]).all() and got[1][3] != 1 and got[1][0] != 3
        assert got[3][3] == k - 1 and got[3][0] == k - 1 and _same(got, PH.dp_f32(qn.reshape(k * T, nd), nn.reshape(-1), T, k, node_weight=nw))
        clean = _lattice(host_lib, np.where(np.isnan(qn), F(123.0), qn).reshape(k * T, nd), nn.reshape(-1), T, k, node_weight=nw)
        assert _same(got, clean)   # (what an inadmissible row holds - NaN or a number - changes nothing)


@pytest.mark.parametrize("k,T", [(5, 9), (33, 20), (256, 6)])
def test_any_split_of_the_predecessors_gives_the_same_lattice(host_lib, k, T):
    """1, 2, 4 and 8 slices, merged in forward, reverse and a random order, and any chunk length of the walk back: identical outputs (rows duplicated
    so that ties occur)."""
    nd = 6
    q, node = PH.random_lattice(T, k, nd, k)
    q, node = q.reshape(k, T, nd), node.reshape(k, T)
    if k > 2:
        q[k - 1], node[k - 1] = q[0], node[0]
    q, node = q.reshape(k * T, nd), node.reshape(k * T)
    ref = _lattice(host_lib, q, node, T, k, max_step=1.2)
    assert _same(ref, PH.dp_f32(q, node, T, k, max_step=1.2))
    rng = np.random.default_rng(1)
    for n_slices in (2, 4, 8):
        for order in (np.arange(n_slices), np.arange(n_slices)[::-1], rng.permutation(n_slices)):
            assert _same(_lattice(host_lib, q, node, T, k, max_step=1.2, n_slices=n_slices, order=order), ref), (n_slices, order)
    for chunk in (1, 2, T - 1, T, T + 1):
        assert _same(_lattice(host_lib, q, node, T, k, max_step=1.2, chunk=chunk), ref), chunk


def test_geometry_and_constants_agree_with_the_binding(host_lib):
    c = (C.c_int * 6)()
    host_lib.path_host_constants(c)
    block, row, stage, chunk, max_k, opt_bytes = list(c)
    assert block == 256 and row == 8 and max_k == _lib.IKF_PATH_MAX_K == 256 and chunk == PH.backtrack_chunk() and stage >= 1
    assert opt_bytes == C.sizeof(_lib.ikf_path_options) == 32
    assert chunk * max_k <= 2 * stage * block * row * 4          # a chunk of back-pointers fits the row buffers it is staged in
    for k in range(1, 257):
        span = host_lib.path_host_span(k)
        assert span >= k and span & (span - 1) == 0 and (span < 2 * k or k == 1) and host_lib.path_host_slices(k) * span == block
    for T in (1, 2, 3, chunk - 1, chunk, chunk + 1, 2 * chunk + 1, 2 ** 31 - 1):
        assert host_lib.path_host_stages(T) == -(-T // stage) and host_lib.path_host_bt_chunks(T) == -(-T // chunk)
        assert host_lib.path_host_bp_bytes(T, 1) >= T + 3 and host_lib.path_host_bp_bytes(T, 1) % 4 == 0
