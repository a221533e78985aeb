"""The arithmetic of the world point cloud (ikflow_amd/csrc/cloud_math.h: the squared point-axis distance, the row clearance, its independence of
how the points are split, the launch plan) compiled for the HOST with g++ and held against the fp64 reference of tests/cloud_helpers.py - the
kernels' own source, checked without a GPU.  The GPU tests check the same code where it ships (tests/test_cloud.py).  Also here, from the fp64
reference alone: every (chain, size) the GPU tests use has few rows in the band around its threshold and enough on either side.
Test infrastructure: nothing in ikflow_amd/ loads it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cloud_helpers as CH
import helpers as H
import rank_helpers as RH
import world_helpers as WH
from ikflow_amd import _lib
from test_kin_math_host import _chain_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = CH.CLEARANCE_TOL


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("cloud_math") / "libcloud_math_host.so"
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "cloud_math_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(str(out))
    lib.kin_math_chain_bytes = lib.cloud_host_chain_bytes   # (what _chain_bytes asks the library it packs for)
    lib.cloud_host_set_capsules.argtypes = [C.c_void_p, C.c_int]
    lib.cloud_host_set_capsules.restype = None
    lib.cloud_host_dist2.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.cloud_host_dist2.restype = None
    lib.cloud_host_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.cloud_host_plan.argtypes = [C.c_longlong, C.c_longlong, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.cloud_host_plan.restype = None
    lib.cloud_host_partial_bound.argtypes = [C.c_longlong, C.c_int]
    lib.cloud_host_partial_bound.restype = C.c_longlong
    assert lib.cloud_host_point_bytes() == 16 and lib.cloud_host_max_points() == _lib.IKF_CLOUD_MAX_POINTS == 1 << 20 and lib.cloud_host_tile() == 512
    return lib


def _dist2(lib, e0, e1, p):
    seg = np.ascontiguousarray(np.concatenate([e0, e1], 1), np.float32)
    p = np.ascontiguousarray(p, np.float32)
    out = np.zeros(len(p), np.float32)
    lib.cloud_host_dist2(seg.ctypes.data, p.ctypes.data, len(p), out.ctypes.data)
    return out


def _ref_dist(e0, e1, p):
    return WH._point_segment(p.astype(np.float64), e0.astype(np.float64), e1.astype(np.float64))


def test_point_segment_dist2_on_random_and_degenerate_segments(host_lib):
    """100000 random (point, axis) terms - axes up to 1 m, points around and on them - and the named degenerate ones: sqrt(dist2) within 2e-5 of the
    fp64 distance on the same f32 inputs."""
    rng = np.random.default_rng(41)
    n = 100000
    e0 = rng.uniform(-0.8, 0.8, (n, 3)).astype(np.float32)
    d = rng.standard_normal((n, 3))
    e1 = (e0 + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.0, 1.0, (n, 1))).astype(np.float32)
    p = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    near = rng.random(n) < 0.3   # a third of the points within centimetres of the axis
    t = rng.uniform(-0.2, 1.2, (n, 1))
    p[near] = (e0 + (e1 - e0) * t + rng.standard_normal((n, 3)) * 0.01).astype(np.float32)[near]
    got = np.sqrt(_dist2(host_lib, e0, e1, p).astype(np.float64))
    ref = _ref_dist(e0, e1, p)
    worst = float(np.abs(got - ref).max())
    print(f"point_segment_dist2: worst |sqrt(kernel source) - fp64 reference| {worst:.3e} on {n} terms, {int((ref < 0.02).sum())} within 2 cm")
    assert worst <= TOL and (ref < 0.02).sum() > 1000
    a, b = np.array([[0.1, 0.2, 0.3]], np.float32), np.array([[0.5, 0.2, 0.3]], np.float32)
    cases = [
        (a, a, [[0.4, 0.6, 0.3]], 0.5),          # a zero-length axis: the distance to the point e0
        (a, a, [[0.1, 0.2, 0.3]], 0.0),          # ... and the point on it
        (a, a + np.float32(1e-7), [[0.4, 0.6, 0.3]], 0.5),   # shorter than 1e-6: treated as zero length
        (a, b, [[0.3, 0.2, 0.3]], 0.0),          # a point on the axis
        (a, b, [[0.1, 0.2, 0.3]], 0.0),          # ... at its end
        (a, b, [[0.3, 0.2, 0.7]], 0.4),          # beside the axis
        (a, b, [[-0.2, 0.2, 0.7]], 0.5),         # beyond e0: the end point counts
        (a, b, [[0.8, 0.6, 0.3]], 0.5),          # beyond e1
    ]
    for e0_, e1_, p_, want in cases:
        p_ = np.array(p_, np.float32)
        got = float(np.sqrt(_dist2(host_lib, e0_, e1_, p_)[0]))
        assert abs(got - want) <= TOL and abs(got - float(_ref_dist(e0_, e1_, p_)[0])) <= TOL, (e0_, e1_, p_, got, want)


def _set_capsules(lib, robot, caps=None):
    robot.set_collision_capsules(RH.collision_capsules(robot) if caps is None else caps)
    folded, _ = robot._collision_model
    arr = (_lib.ikf_capsule * max(len(folded), 1))()
    for c, (frame, p0, p1, r) in zip(arr, folded):
        c.frame, c.radius = int(frame), float(r)
        for i in range(3):
            c.p0[i], c.p1[i] = float(p0[i]), float(p1[i])
    lib.cloud_host_set_capsules(arr, len(folded))
    robot.set_collision_capsules(RH.collision_capsules(robot))   # (the robots are shared: the small model is back)


def _stored(points, pad=False):
    """The points as the handle stores them: (x, y, z, 0), optionally padded to a multiple of 512 with copies of the last point."""
    n = len(points)
    total = -(-n // 512) * 512 if pad and n else n
    out = np.zeros((max(total, 1), 4), np.float32)
    out[:n, :3] = points
    out[n:total, :3] = points[-1] if n else 0.0
    return out, total


def _rows(lib, chain, q, stored, n_pts, cuts=(), level=0, radius=CH.POINT_RADIUS):
    q = np.ascontiguousarray(q.numpy(), np.float32)
    out = np.zeros(q.shape[0], np.float32)
    cuts = np.ascontiguousarray(cuts, np.int64)
    assert lib.cloud_host_rows(chain, q.ctypes.data, q.shape[0], stored.ctypes.data, n_pts, radius, cuts.ctypes.data, len(cuts), level, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("which", RH.CASE_CHAINS)
def test_whole_rows_and_split_independence(host_lib, which):
    """257 rows x clouds of 1, 255, 513 and 4097 points: chain walk + cloud_clearance_row of the kernel source within 2e-5 of the fp64 reference;
    the minimum over arbitrary partitions of the points - met in dist2, after sqrtf - rc (the kernel's one register) or after the whole row - and
    the padded array give the bits of the whole cloud."""
    robot, _ = H.kin_robots(which)
    chain = _chain_bytes(robot, host_lib)
    _set_capsules(host_lib, robot)
    rng = np.random.default_rng(5)
    for n_points in CH.HOST_SIZES:
        q, ref, thr = CH.rows_and_reference(which, n_points)
        stored, _ = _stored(CH.cloud(which, n_points))
        whole = _rows(host_lib, chain, q, stored, n_points)
        err = float(np.abs(whole - ref).max())
        print(f"{which} {n_points} points: worst {err:.2e}, clearances {ref.min():.3f} .. {ref.max():.3f}, threshold {thr:.4f}")
        assert err <= TOL, (which, n_points, err)
        padded, total = _stored(CH.cloud(which, n_points), pad=True)
        assert total % 512 == 0 and H.same_bits(_rows(host_lib, chain, q, padded, total), whole)
        for trial in range(3):
            cuts = np.sort(rng.integers(0, n_points + 1, size=int(rng.integers(1, 9))))   # (empty spans among them)
            for level in (0, 1, 2):
                assert H.same_bits(_rows(host_lib, chain, q, stored, n_points, cuts, level), whole), (which, n_points, cuts, level)
        quarters = [i * 128 for i in range(1, total // 128)]   # the kernel's own split: 128 points per wave and tile
        assert H.same_bits(_rows(host_lib, chain, q, padded, total, quarters, 1), whole)
    empty = _rows(host_lib, chain, q, stored, 0)
    assert (empty == np.float32(CH.EMPTY)).all()
    _set_capsules(host_lib, robot, [])
    assert (_rows(host_lib, chain, q, stored, n_points) == np.float32(CH.EMPTY)).all()   # a model of no capsules


@pytest.mark.parametrize("which", RH.CASE_CHAINS)
def test_whole_rows_with_24_capsules(host_lib, which):
    """The 66 rows of tests/test_cloud.py's 24-capsule case through the kernel source, and the band condition it rests on.  (No spread is asked
    here: 24 capsules along the whole chain are never far from a cloud that sits where the chain passes.)"""
    robot, _ = H.kin_robots(which)
    chain = _chain_bytes(robot, host_lib)
    _set_capsules(host_lib, robot, RH.capsules(which, "caps24"))
    q, ref, thr = CH.rows_and_reference(which, 513, "caps24")
    stored, _ = _stored(CH.cloud(which, 513, "caps24"))
    err = float(np.abs(_rows(host_lib, chain, q, stored, 513) - ref).max())
    band, below, above, spread = CH.conditions(ref, thr)
    print(f"{which} caps24: worst {err:.2e}, band {band:.3f} below {below:.3f} above {above:.3f} spread {spread:.3f}")
    assert err <= TOL and band <= 0.05 and below >= 0.20 and above >= 0.20


@pytest.mark.parametrize("which", H.KIN_ALL)
def test_the_conditions_hold_on_every_scene_of_the_gpu_tests(which):
    """From the fp64 reference alone, for every (chain, size) of tests/test_cloud.py and of this module: with the threshold at the median at most
    5 % of the rows lie in the 1e-4 band, at least 20 % on either side, and the clearances spread over a decimetre or more."""
    for n_points in sorted(set(CH.SIZES) | set(CH.HOST_SIZES)):
        q, ref, thr = CH.rows_and_reference(which, n_points)
        band, below, above, spread = CH.conditions(ref, thr)
        print(f"{which} {n_points} points: threshold {thr:.4f}, band {band:.3f} below {below:.3f} above {above:.3f} spread {spread:.3f}")
        assert band <= 0.05 and below >= 0.20 and above >= 0.20 and spread >= 0.1, (which, n_points, band, below, above, spread)


@pytest.mark.parametrize("which", RH.CASE_CHAINS)
def test_the_conditions_hold_on_the_shapes_of_the_ranked_gpu_tests(which):
    for m, k in WH.RANK_SHAPES:
        if m * k >= 130:
            cl, thr = CH.rank_case(which, m, k)[5:]
            band, below, above = CH.band_shares(cl, thr)
            assert band <= 0.05 and below >= 0.20 and above >= 0.20, (which, m, k, band, below, above)


def _plan(lib, rows, n_points, n_cu):
    c, t = C.c_int(), C.c_int()
    lib.cloud_host_plan(rows, n_points, n_cu, C.byref(c), C.byref(t))
    return c.value, t.value


def test_cloud_plan_over_a_grid(host_lib):
    """chunks x tiles_per_chunk covers every tile, no chunk is empty, chunks <= 2048 and <= what two workgroups per CU ask for; more rows never
    mean more chunks, more points never fewer tiles per chunk at a fixed chunk request; the partial buffer's bound holds and is monotone."""
    sizes = [1, 511, 512, 513, 4097, 20481, 65536, 1 << 20]
    row_counts = [1, 63, 64, 65, 257, 4096, 16384, 65536, 1 << 20, (1 << 31) - 1]
    for n_cu in (1, 8, 256, 304):
        for n_points in sizes:
            tiles = -(-n_points // 512)
            prev_chunks = None
            for rows in row_counts:
                chunks, per = _plan(host_lib, rows, n_points, n_cu)
                row_tiles = -(-rows // 64)
                want = max(1, -(-2 * n_cu // row_tiles))
                assert 1 <= chunks <= 2048 and chunks <= min(tiles, want) and per >= 1
                assert chunks * per >= tiles and (chunks - 1) * per < tiles, (rows, n_points, n_cu, chunks, per)
                assert per == -(-tiles // min(tiles, want)) and chunks == -(-tiles // per)
                assert prev_chunks is None or chunks <= prev_chunks
                prev_chunks = chunks
                if chunks > 1:
                    assert chunks * rows <= host_lib.cloud_host_partial_bound(rows, n_cu)
        bounds = [host_lib.cloud_host_partial_bound(r, n_cu) for r in row_counts]
        assert bounds == sorted(bounds) and bounds[-1] <= 256 * n_cu + 64
    assert _plan(host_lib, 64, 1 << 20, 256) == (512, 4) and _plan(host_lib, 4096, 20481, 256) == (7, 6) and _plan(host_lib, 1, 20481, 256) == (41, 1)
    assert _plan(host_lib, 1 << 20, 1 << 20, 256) == (1, 2048) and _plan(host_lib, 0, 100, 256)[0] == 1 and _plan(host_lib, 100, 0, 256)[0] == 1
