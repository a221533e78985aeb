"""The arithmetic of a world track (ikflow_amd/csrc/track_math.h: the fine frame between two key frames, the verdict of one sample of a tracked edge)
compiled for the HOST with g++ as a stand-alone program (tests/track_math_host.cpp) and held against the numpy fp64 restatement and the fp64
references of tests/track_helpers.py - the API unit's and the kernel's own source, checked without a GPU.  The GPU tests check the same code where
it ships (tests/test_track.py).  Test infrastructure: nothing in ikflow_amd/ loads it."""
import ctypes as C
import os
import struct
import subprocess
import types

import numpy as np
import pytest

import helpers as H
import rank_helpers as RH
import sweep_helpers as SH
import track_helpers as TH
import world_helpers as WH
from ikflow_amd import _lib
from ikflow_amd.world import BOX, CAPSULE, HALF_SPACE, SPHERE, World
from test_kin_math_host import _chain_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = tmp_path_factory.mktemp("track_math") / "track_math_host"
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
           os.path.join(ROOT, "tests", "track_math_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return str(out)


def _records_bytes(kinds, recs):
    """[.. x n x 11] f32 records -> ikf_obstacle bytes (48 each)."""
    recs = np.asarray(recs, np.float32).reshape(-1, len(kinds), 11)
    out = np.zeros((recs.shape[0], len(kinds), 12), np.float32)
    out[:, :, 0] = np.asarray(kinds, np.int32).view(np.float32)[None, :]
    out[:, :, 1:] = recs
    return out.tobytes()


def _interp(program, tmp_path, kinds, keys, S, expect=0):
    F, n, _ = keys.shape
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("iii", F, n, S) + _records_bytes(kinds, keys))
    r = subprocess.run([program, "interp", str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == expect, (r.returncode, r.stdout, r.stderr)
    if expect:
        return tuple(int(x) for x in r.stdout.split())
    raw = np.frombuffer(dst.read_bytes(), np.float32).reshape((F - 1) * (S + 1) + 1, n, 12)
    assert np.array_equal(raw[:, :, 0].view(np.int32), np.broadcast_to(np.asarray(kinds, np.int32), raw.shape[:2]))
    return raw[:, :, 1:].copy()


def test_the_program_checks_itself(program):
    r = subprocess.run([program, "self"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)


def _turning_track():
    """Two key frames of every kind; box 1 turns by 2.2 rad about z - more than 90 degrees of the quaternion's half angle would need 3.14, so its
    second quaternion is ALSO given with the opposite sign (box 2: the same rotation, the dot product < 0); box 3 turns by 3.5 rad, where the dot
    product of the two quaternions as built is negative by itself."""
    def rot(angle):
        return (np.cos(angle / 2), 0.0, 0.0, np.sin(angle / 2))

    worlds = []
    for t in range(3):
        w = World()
        w.add_sphere((0.3 + 0.1 * t, -0.2, 0.5), 0.05 + 0.01 * t)
        w.add_capsule((0.1, 0.2 * t, 0.3), (0.4, 0.2 * t, 0.9), 0.03)
        w.add_half_space((0.2 * t, 0.3, 1.0 + t), -0.1 * t)
        w.add_box((0.5, 0.1 * t, 0.4), (0.1, 0.2 + 0.05 * t, 0.3), rot(1.1 * t), 0.01 * t)
        w.add_box((0.5, 0.1 * t, 0.4), (0.1, 0.2, 0.3), tuple(-x for x in rot(1.1 * t)) if t == 1 else rot(1.1 * t), 0.0)
        w.add_box((-0.5, 0.0, 0.4), (0.1, 0.2, 0.3), rot(3.5 * t), 0.0)
        worlds.append(w)
    return worlds


@pytest.mark.parametrize("S", [0, 1, 3, 4, 16])
def test_fine_frames_equal_the_numpy_fp64_restatement_to_one_ulp(program, tmp_path, S):
    """Every number of every fine frame within one f32 ulp of max(1, |v|) of track_helpers.interp_ref (both compute in fp64 and round once); i = 0
    is the key frame bit for bit; the cases hold every kind, a moving scene of 7 obstacles over 5 frames, and boxes whose quaternion sign flips."""
    for worlds in (_turning_track(), TH.moving_track("panda", 5, "mixed7", 0)):
        kinds, keys = TH.stored_track(worlds)
        got = _interp(program, tmp_path, kinds, keys, S)
        ref = TH.interp_ref(kinds, keys, S)
        assert got.shape == ref.shape == ((len(worlds) - 1) * (S + 1) + 1, len(kinds), 11)
        for t in range(len(worlds)):
            assert H.same_bits(got[TH.fine_index(t, 0, S)], keys[t]), f"key frame {t} is not passed through bit for bit"
        excess = TH.ulp_excess(got, ref)
        print(f"S {S}, {len(kinds)} obstacles: worst |program - numpy| = {excess:.2f} ulp")
        assert excess <= 1.0
        norms = np.sqrt((got[:, kinds == BOX, 6:10].astype(np.float64) ** 2).sum(-1))
        assert np.abs(norms - 1.0).max() < 2e-7
        hs = np.sqrt((got[:, kinds == HALF_SPACE, 0:3].astype(np.float64) ** 2).sum(-1))
        assert np.abs(hs - 1.0).max() < 2e-7


def test_the_quaternion_sign_flip_takes_the_short_way(program, tmp_path):
    """The two boxes of _turning_track that differ only in the sign of frame 1's quaternion get the same fine ROTATION (q and -q), and that
    rotation lies between the key frames'; box 3's dot product is negative as built, and its blend is not the vanishing one."""
    kinds, keys = TH.stored_track(_turning_track())
    assert (keys[0, 4, 6:10] * keys[1, 4, 6:10]).sum() < 0 < (keys[0, 3, 6:10] * keys[1, 3, 6:10]).sum()
    assert (keys[0, 5, 6:10] * keys[1, 5, 6:10]).sum() < 0
    got = _interp(program, tmp_path, kinds, keys, 3)
    for i in range(1, 4):
        qa, qb = got[i, 3, 6:10].astype(np.float64), got[i, 4, 6:10].astype(np.float64)
        assert abs(abs(qa @ qb) - 1.0) < 1e-6, (i, qa, qb)           # the same rotation
        angle = 2 * np.arctan2(abs(qa[3]), abs(qa[0]))
        assert 0.0 < angle < 1.1
        q5 = got[i, 5, 6:10].astype(np.float64)
        assert abs(np.linalg.norm(q5) - 1.0) < 2e-7


def test_a_vanishing_blended_normal_is_refused_with_frame_obstacle_and_sample(program, tmp_path):
    worlds = []
    for t in range(3):
        w = World()
        w.add_sphere((0.0, 0.0, 1.0), 0.1)
        w.add_half_space((0.0, 0.0, 1.0) if t < 2 else (0.0, 0.0, -1.0), 0.0)
        worlds.append(w)
    kinds, keys = TH.stored_track(worlds)
    assert _interp(program, tmp_path, kinds, keys, 1, expect=2) == (1, 1, 1)    # u = 1 / 2 between frames 1 and 2
    assert _interp(program, tmp_path, kinds, keys, 3, expect=2) == (1, 1, 2)    # u = 2 / 4
    _interp(program, tmp_path, kinds, keys, 2)                                  # u = 1 / 3, 2 / 3: the blend is 1 / 3 long
    _interp(program, tmp_path, kinds, keys, 0)                                  # no fine frames


def _capsule_bytes(robot, caps):
    robot.set_collision_capsules(caps)
    folded, pairs = robot._collision_model
    b = struct.pack("ii", len(folded), len(pairs))
    for frame, p0, p1, r in folded:
        b += struct.pack("i3f3ff", int(frame), *[float(x) for x in p0], *[float(x) for x in p1], float(r))
    b += np.asarray(pairs, np.int32).reshape(-1).tobytes()
    robot.set_collision_capsules(RH.collision_capsules(robot))   # (the robots are shared: the small model is back)
    return b


@pytest.mark.parametrize("case", [c for c in TH.MASK_CASES if c[:2] != (3, 65)], ids=lambda c: "-".join(map(str, c)))
def test_the_sample_test_against_fp64_and_the_condition_the_gpu_tests_rest_on(program, tmp_path, case):
    """track_sample_blocked - the kernel's per-sample test - on every sample of every edge of the small lattices of tests/test_track.py, each
    against its own fine frame: the edge verdict it implies (any sample blocked) is the fp64 reference's outside the band.  And from the
    reference alone: the case's seed satisfies sweep_helpers.shares_hold, with the start edges and without."""
    T, k, S, rule, base = case
    c = TH.mask_case(T, k, S, rule, base, TH.mask_seed(*case))
    for v in (c["v"], c["v_nostart"]):
        band, blocked, free = SH.shares(v)
        print(f"{case}: band {band:.4f} (cap 0.02), surely blocked {blocked:.3f}, surely free {free:.3f}")
        assert SH.shares_hold(v), (case, SH.shares(v))
    robot, orob = H.kin_robots(TH.MASK_CHAIN)
    size = int(subprocess.run([program, "chain_bytes"], capture_output=True, text=True).stdout)
    chain = _chain_bytes(robot, types.SimpleNamespace(kin_math_chain_bytes=lambda: size)).raw
    kinds, keys = TH.stored_track(c["worlds"])
    table = TH.interp_ref(kinds, keys, S)
    blob = chain + _capsule_bytes(robot, RH.collision_capsules(robot))
    if c["world"] is not None:
        wk, wr = TH.stored(c["world"])
        blob += struct.pack("i", len(wk)) + _records_bytes(wk, wr[None]) + struct.pack("f", c["world_thr"])
    else:
        blob += struct.pack("if", 0, 0.0)
    blob += struct.pack("ifif", int(rule == "all"), c["self_thr"] or 0.0, len(kinds), c["track_thr"])
    a, b = SH.lattice_edges(c["q"].numpy(), T, k, c["q_start"].numpy())
    n = a.shape[0]
    blob += struct.pack("ii", n, S)
    parts = []
    for e in range(n):
        t = 0 if e >= (T - 1) * k * k else e // (k * k) + 1
        frames = [table[0 if t == 0 else TH.fine_index(t - 1, i, S)] for i in range(1, S + 1)]
        parts.append(a[e].tobytes() + b[e].tobytes() + _records_bytes(kinds, np.stack(frames)))
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob + b"".join(parts))
    r = subprocess.run([program, "samples", str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    blocked = np.frombuffer(dst.read_bytes(), np.uint8).reshape(n, S).astype(bool)
    first = np.where(blocked.any(1), blocked.argmax(1), -1)
    SH.check_edges(blocked.any(1), first, c["v"], str(case))
    assert 0 < blocked.any(1).sum() < n


@pytest.mark.parametrize("case", [c for c in TH.MASK_CASES if c[:2] == (3, 65)], ids=lambda c: "-".join(map(str, c)))
def test_the_large_lattices_condition_holds_by_the_reference_alone(case):
    c = TH.mask_case(*case, TH.mask_seed(*case))
    for v in (c["v"], c["v_nostart"]):
        band, blocked, free = SH.shares(v)
        print(f"{case}: band {band:.4f} (cap 0.02), surely blocked {blocked:.3f}, surely free {free:.3f}")
        assert SH.shares_hold(v), (case, SH.shares(v))


def test_the_node_cases_have_rows_on_either_side_of_their_thresholds():
    """From the reference alone: every node case of tests/test_track.py has at most 5 % of its rows in the band (tests/test_world_math_host.py's
    cap for such rows) and a third of them surely on either side."""
    for case in TH.NODE_CASES:
        c = TH.node_case(*case)
        cl = c["ref"]["clearance"]
        band, below, above = WH.band_shares(cl[~np.isnan(cl)], c["thr"])
        print(f"{case}: band {band:.4f} (cap 0.05), below {below:.3f}, above {above:.3f}")
        assert band <= 0.05 and below > 1 / 3 and above > 1 / 3, (case, band, below, above)


def test_the_crossing_cases_are_what_they_claim_by_the_reference_alone():
    """The preconditions of "the obstacle really moves": on = "edge" - every node clear of its key frame, the middle sample of the edge
    (0, 0) -> (1, 0) deep in the sphere of fine frame (0, 1), every other middle sample clear of its fine frame, and every middle sample clear of
    every KEY frame; on = "node" - node (1, 0) in the sphere of key frame 1, every other node and every middle sample clear."""
    nodes, mids, per_key = TH.crossing_reference(TH.moving_crossing_case("edge"))
    assert nodes.min() > 1e-3 and per_key.min() > 1e-3
    assert mids[0, 0, 0] < -1e-3 and np.delete(mids.ravel(), 0).min() > 1e-3
    nodes, mids, per_key = TH.crossing_reference(TH.moving_crossing_case("node"))
    assert nodes[1, 0] < -1e-3 and np.delete(nodes.ravel(), 3).min() > 1e-3 and mids.min() > 1e-3
