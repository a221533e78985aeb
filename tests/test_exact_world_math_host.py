"""The arithmetic of exact IK under the exact collision rule (ikflow_amd/csrc/exact_world_math.h: the verdict of a candidate row, the cloud
rule's mask, the selection over admissible rows, the launch geometry) compiled for the HOST with g++ and held against a numpy statement of the
definition (include/ikflow_amd_exact_world.h; tests/exact_world_helpers.py) - the kernel's own source, checked without a GPU.  The GPU tests check
the same code where it ships (tests/test_exact_world.py).  Test infrastructure: nothing in ikflow_amd/ loads it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import exact_world_helpers as EW
import helpers as H
import world_helpers as WH
from test_kin_math_host import _chain_bytes
from test_world_math_host import _set_capsules, _structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("exact_world_math") / "libexact_world_math_host.so"
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas",
           os.path.join(ROOT, "tests", "exact_world_math_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(str(out))
    lib.kin_math_chain_bytes = lib.exact_world_host_chain_bytes       # (what _chain_bytes asks the library it packs for)
    lib.world_host_set_capsules = lib.exact_world_host_set_capsules   # (what _set_capsules calls)
    lib.exact_world_host_set_capsules.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.exact_world_host_set_capsules.restype = None
    lib.exact_world_host_set_world.argtypes = [C.c_void_p, C.c_int]
    lib.exact_world_host_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.exact_world_host_predicate.argtypes = [C.c_longlong, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_void_p,
                                               C.c_float, C.c_void_p]
    lib.exact_world_host_predicate.restype = None
    lib.exact_world_host_mask.argtypes = [C.c_longlong, C.c_void_p, C.c_void_p, C.c_float]
    lib.exact_world_host_mask.restype = C.c_longlong
    lib.exact_world_host_select.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]
    lib.exact_world_host_select.restype = None
    lib.exact_world_host_blocks.argtypes = [C.c_longlong]
    lib.exact_world_host_blocks.restype = C.c_longlong
    lib.exact_world_host_lds_bytes.restype = C.c_longlong
    return lib


def _tables(rng, rows, thr):
    """Clearance tables with values EQUAL to a threshold, just below and just above it among random ones (f32)."""
    out = []
    for t in thr:
        v = rng.uniform(t - 0.2, t + 0.2, rows).astype(np.float32)
        v[rng.integers(rows, size=rows // 8)] = np.float32(t)
        v[rng.integers(rows, size=rows // 16)] = np.nextafter(np.float32(t), np.float32(-1e9))
        v[rng.integers(rows, size=rows // 16)] = np.nextafter(np.float32(t), np.float32(1e9))
        out.append(v)
    return out


def test_predicate_mask_and_selection_against_the_definition_in_numpy(host_lib):
    """Random row_valid_iter / clearance tables, every combination of the three rules: the predicate is `any applicable clearance < its
    threshold`, strictly (a clearance equal to its threshold is admissible); the mask takes the candidate from exactly the candidate rows below
    the cloud threshold and counts them; the selection over the masked table is the earliest iteration, highest repeat among those - ties, poses
    whose candidates are all rejected and poses without a candidate included."""
    rng = np.random.default_rng(14)
    thr = (np.float32(0.013), np.float32(-0.02), np.float32(0.0))
    for n, R in ((1, 1), (7, 9), (64, 1), (65, 3), (257, 10), (33, 255)):
        rows = n * R
        world, cloud, self_ = _tables(rng, rows, thr)
        first = rng.integers(0, 4, rows).astype(np.uint8)            # 0: no candidate; few values, so ties within a pose are the rule
        first[rng.random(rows) < 0.02] = 255
        if n >= 7:
            first.reshape(R, n)[:, 0] = 0                            # a pose without a candidate
            first.reshape(R, n)[:, 1] = 2                            # a pose tied on every repeat
            world.reshape(R, n)[:, 2] = thr[0] - np.float32(0.1)     # a pose whose candidates the world rejects
            first.reshape(R, n)[:, 2] = 1
        for has_world in (0, 1):
            for has_cloud in (0, 1):
                for reject_self in (0, 1):
                    got = np.full(rows, 7, np.uint8)
                    host_lib.exact_world_host_predicate(rows, has_world, world.ctypes.data, thr[0], has_cloud, cloud.ctypes.data, thr[1], reject_self,
                                                        self_.ctypes.data, thr[2], got.ctypes.data)
                    cl = {k: v for k, v, on in (("world", world, has_world), ("cloud", cloud, has_cloud), ("self", self_, reject_self)) if on}
                    want = EW.rejected_of(cl, {"world": thr[0], "cloud": thr[1], "self": thr[2]}) if cl else np.zeros(rows, bool)
                    assert np.array_equal(got.astype(bool), want), (n, R, has_world, has_cloud, reject_self)
                    equal = np.zeros(rows, bool)
                    for k, v in cl.items():
                        equal |= v == {"world": thr[0], "cloud": thr[1], "self": thr[2]}[k]
                    only_equal = equal & ~want
                    assert not got[only_equal].any()                  # strict `<`
                    # the masked selection: world / self as the fused kernel stores them (0 for a rejected row), then the cloud's mask
                    rvi = np.where(EW.rejected_of({k: v for k, v in cl.items() if k != "cloud"}, {"world": thr[0], "self": thr[2]})
                                   if (has_world or reject_self) else np.zeros(rows, bool), 0, first).astype(np.uint8)
                    before = rvi.copy()
                    count = host_lib.exact_world_host_mask(rows, rvi.ctypes.data, cloud.ctypes.data, thr[1] if has_cloud else np.float32(-3.0e38))
                    below = (before != 0) & (cloud < thr[1]) if has_cloud else np.zeros(rows, bool)
                    assert count == int(below.sum()) and np.array_equal(rvi, np.where(below, 0, before))
                    assert np.array_equal(rvi != 0, (first != 0) & ~want)
                    winner = np.full(n, -9, np.int32)
                    host_lib.exact_world_host_select(rvi.ctypes.data, n, R, winner.ctypes.data)
                    assert np.array_equal(winner, EW.select(first.astype(np.int64), want, n, R)), (n, R, has_world, has_cloud, reject_self)
                    if n >= 7:
                        assert winner[0] == -1 and (winner[2] == -1 if has_world else True)
                        if not want.reshape(R, n)[:, 1].all():
                            assert winner[1] == np.flatnonzero(~want.reshape(R, n)[:, 1]).max()   # the tie: the highest admissible repeat


@pytest.mark.parametrize("which", ("syn4r", "syn5p", "syn6r", "panda", "fetch"))
def test_row_verdicts_are_the_predicate_on_the_functions_it_calls(host_lib, which):
    """exact_row_rejected on 257 configurations in mixed7, under the world rule, the self rule, both and neither: equal to the predicate on
    capsule_clearance and world_clearance of the same row (the walk is shared, the self rule short-cuts the world rule - neither may change a
    verdict), and to the fp64 reference outside the band."""
    robot, orob = H.kin_robots(which)
    chain = _chain_bytes(robot, host_lib)
    _set_capsules(host_lib, robot)
    q, ref, world_thr = WH.rows_and_reference(which, "mixed7")
    world = WH.scene(which, "mixed7")
    assert host_lib.exact_world_host_set_world(_structs(world.obstacles), len(world)) == 0
    qn = np.ascontiguousarray(q.numpy(), np.float32)
    n = qn.shape[0]
    self_ref = EW.RH.clearance(orob, EW.RH.capsules(which, None), q)
    self_thr = float(np.median(self_ref))
    for use_world, reject_self in ((1, 0), (0, 1), (1, 1), (0, 0)):
        rej, wcl, scl = np.full(n, 7, np.uint8), np.zeros(n, np.float32), np.zeros(n, np.float32)
        assert host_lib.exact_world_host_rows(chain, qn.ctypes.data, n, use_world, world_thr, reject_self, self_thr, rej.ctypes.data, wcl.ctypes.data,
                                              scl.ctypes.data) == 0
        want = (use_world & (wcl < np.float32(world_thr))) | (reject_self & (scl < np.float32(self_thr)))
        assert np.array_equal(rej.astype(bool), want.astype(bool)), (which, use_world, reject_self)
        by_ref = (use_world & (ref["clearance"] < world_thr)) | (reject_self & (self_ref < self_thr))
        near = (use_world & (np.abs(ref["clearance"] - world_thr) <= WH.BAND)) | (reject_self & (np.abs(self_ref - self_thr) <= WH.BAND))
        decided = ~near.astype(bool)
        assert np.array_equal(rej.astype(bool)[decided], by_ref.astype(bool)[decided]), (which, use_world, reject_self)
        if not use_world and not reject_self:
            assert not rej.any()


def test_launch_geometry(host_lib):
    assert host_lib.exact_world_host_threads() == 64
    for rows in (1, 63, 64, 65, 257, 2000, (1 << 31) - 1):
        assert host_lib.exact_world_host_blocks(rows) == -(-rows // 64)
    for n_caps in (0, 1, 5, 24):
        stride = host_lib.exact_world_host_cap_stride(n_caps)
        assert stride == (6 * n_caps) | 1 and stride % 2 == 1
        for n_obs in (0, 1, 7, 64):
            assert host_lib.exact_world_host_lds_bytes(n_obs, n_caps) == 4 * (16 * n_obs + 64 * stride)
    assert host_lib.exact_world_host_lds_bytes(64, 24) == 4096 + 37120
