"""The arithmetic of world collision (ikflow_amd/csrc/world_math.h: the four obstacle terms, the closest pair and its tie rule, the whole-row
clearance, the row score with the world rule) compiled for the HOST with g++ and held against the fp64 reference of tests/world_helpers.py - the
kernels' own source, checked without a GPU.  The GPU tests check the same code where it ships (tests/test_world.py).  Also here, from the fp64
reference alone: every (chain, scene) the GPU tests use has few rows in the band around its threshold and enough on either side.
Test infrastructure: nothing in ikflow_amd/ loads it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import rank_helpers as RH
import world_helpers as WH
from ikflow_amd import _lib
from ikflow_amd.world import BOX, CAPSULE, HALF_SPACE, SPHERE, World
from test_kin_math_host import _chain_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = WH.CLEARANCE_TOL


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("world_math") / "libworld_math_host.so"
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "world_math_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(str(out))
    lib.kin_math_chain_bytes = lib.world_host_chain_bytes   # (what _chain_bytes asks the library it packs for)
    lib.world_host_set_capsules.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.world_host_set_capsules.restype = None
    lib.world_host_set_world.argtypes = [C.c_void_p, C.c_int]
    lib.world_host_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    lib.world_host_pairs.restype = None
    lib.world_host_hit.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.world_host_hit.restype = None
    lib.world_host_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.world_host_scores.argtypes = [C.c_void_p, C.POINTER(_lib.ikf_rank_options), C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_float, C.c_void_p]
    assert lib.world_host_obstacle_words() == 16
    return lib


def _structs(obstacles):
    """ikf_obstacle array as the DEVICE holds it: normalised in fp64 (world_helpers.normalised), rounded to f32."""
    arr = (_lib.ikf_obstacle * max(len(obstacles), 1))()
    for o, ob in zip(arr, obstacles):
        kind, a, b, quat, radius = WH.normalised(ob)
        o.kind, o.radius = kind, radius
        for i in range(3):
            o.a[i], o.b[i] = a[i], b[i]
        for i in range(4):
            o.quat[i] = quat[i]
    return arr


def _f32(ob):
    """The obstacle with every number rounded to f32 - what the header's struct can hold, so the reference sees the kernel's inputs."""
    kind, a, b, quat, radius = ob
    r = lambda v: tuple(float(np.float32(x)) for x in v)
    return (kind, r(a), r(b), r(quat), float(np.float32(radius)))


def _pairs(lib, obstacles, seg, rc):
    """clearance of pair i = (obstacles[i], capsule seg[i], rc[i]) through the kernel source."""
    n = len(obstacles)
    arr = _structs(obstacles)
    seg, rc = np.ascontiguousarray(seg, np.float32), np.ascontiguousarray(rc, np.float32)
    out = np.zeros(n, np.float32)
    lib.world_host_pairs(arr, seg.ctypes.data, rc.ctypes.data, n, out.ctypes.data)
    return out


def _random_obstacle(kind, rng):
    c = rng.uniform(-0.6, 0.6, 3)
    if kind == SPHERE:
        return (SPHERE, c, (0, 0, 0), (1, 0, 0, 0), rng.uniform(0.0, 0.3))
    if kind == CAPSULE:
        return (CAPSULE, c, c + rng.uniform(-0.5, 0.5, 3), (1, 0, 0, 0), rng.uniform(0.0, 0.2))
    if kind == HALF_SPACE:
        n = rng.standard_normal(3)
        return (HALF_SPACE, n / np.linalg.norm(n), (rng.uniform(-0.5, 0.5), 0, 0), (1, 0, 0, 0), 0.0)
    q = rng.standard_normal(4)
    return (BOX, c, rng.uniform(0.02, 0.8, 3), q / np.linalg.norm(q), rng.choice([0.0, rng.uniform(0.0, 0.1)]))


@pytest.mark.parametrize("kind", [SPHERE, CAPSULE, HALF_SPACE, BOX])
def test_each_term_on_20000_random_pairs(host_lib, kind):
    """100 random obstacles of the kind x 200 random capsules each (axes up to 1 m, around and inside the obstacle): <= 2e-5 from the fp64 reference
    on the same f32 inputs."""
    rng = np.random.default_rng(100 + kind)
    worst, n_neg = 0.0, 0
    for _ in range(100):
        ob = _f32(_random_obstacle(kind, rng))
        e0 = rng.uniform(-0.8, 0.8, (200, 3)).astype(np.float32)
        d = rng.standard_normal((200, 3))
        e1 = (e0 + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.0, 1.0, (200, 1))).astype(np.float32)
        rc = rng.uniform(0.0, 0.1, 200).astype(np.float32)
        got = _pairs(host_lib, [ob] * 200, np.concatenate([e0, e1], 1), rc)
        ref = WH.pair_clearance(ob, e0.astype(np.float64), e1.astype(np.float64), rc.astype(np.float64))
        worst = max(worst, float(np.abs(got - ref).max()))
        n_neg += int((ref < 0).sum())
    print(f"kind {kind}: worst |kernel source - fp64 reference| {worst:.3e} on 20000 pairs, {n_neg} penetrating")
    assert worst <= TOL and n_neg > 500


def _one(lib, ob, e0, e1, rc=0.0):
    ob = _f32(ob)
    got = float(_pairs(lib, [ob], np.array([[*e0, *e1]], np.float32), np.array([rc], np.float32))[0])
    ref = float(WH.pair_clearance(ob, np.array([e0], np.float32).astype(np.float64), np.array([e1], np.float32).astype(np.float64), np.float64(np.float32(rc)))[0])
    assert abs(got - ref) <= TOL, (ob, e0, e1, got, ref)
    return got


def test_the_named_degenerate_cases(host_lib):
    box = (BOX, (0.1, 0.2, 0.3), (0.2, 0.1, 0.3), (1, 0, 0, 0), 0.0)
    rot = (BOX, (0.1, 0.2, 0.3), (0.2, 0.1, 0.3), (0.8, 0.2, -0.4, 0.4), 0.0)
    every = [(SPHERE, (0.3, 0.1, 0.2), (0, 0, 0), (1, 0, 0, 0), 0.1), (CAPSULE, (0.3, 0.1, 0.2), (0.1, 0.5, 0.0), (1, 0, 0, 0), 0.05),
             (HALF_SPACE, (0.0, 0.6, 0.8), (0.1, 0, 0), (1, 0, 0, 0), 0.0), box, rot]
    # a robot capsule with p0 == p1 (a sphere: the test capsule model has one), outside and inside every obstacle
    for ob in every:
        _one(host_lib, ob, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), 0.04)
        _one(host_lib, ob, (0.12, 0.22, 0.28), (0.12, 0.22, 0.28), 0.04)
    # an obstacle capsule with a == b is a sphere
    p = (0.3, 0.1, 0.2)
    as_capsule = _one(host_lib, (CAPSULE, p, p, (1, 0, 0, 0), 0.07), (0.5, 0.0, 0.1), (0.6, 0.4, 0.3), 0.02)
    as_sphere = _one(host_lib, (SPHERE, p, (0, 0, 0), (1, 0, 0, 0), 0.07), (0.5, 0.0, 0.1), (0.6, 0.4, 0.3), 0.02)
    assert abs(as_capsule - as_sphere) <= 1e-6
    _one(host_lib, (CAPSULE, p, p, (1, 0, 0, 0), 0.07), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), 0.02)   # both degenerate
    # a segment parallel to a box face: a flat minimum, equal to the height above the face
    got = _one(host_lib, box, (-0.4, 0.2, 0.75), (0.7, 0.25, 0.75))
    assert abs(got - 0.15) <= TOL
    got = _one(host_lib, box, (0.0, 0.15, 0.75), (0.2, 0.25, 0.75))   # ... wholly above the face
    assert abs(got - 0.15) <= TOL
    # a segment through the box, and one with an end point inside it: negative, the depth of the deepest axis point
    got = _one(host_lib, box, (-0.6, 0.2, 0.3), (0.8, 0.2, 0.3))
    assert abs(got + 0.1) <= TOL   # through the centre along x: the nearest faces are y = +-0.1 away
    got = _one(host_lib, box, (0.1, 0.2, 0.55), (0.1, 0.2, 1.5))
    assert abs(got + 0.05) <= TOL   # the end point is 0.05 below the top face
    assert _one(host_lib, rot, (0.1, 0.2, 0.3), (0.9, 0.9, 0.9)) < 0 and _one(host_lib, rot, (-0.5, -0.5, 0.3), (0.6, 0.8, 0.3)) < 0
    # a segment parallel to the plane of a half-space, above and below it
    hs = (HALF_SPACE, (0.0, 0.0, 1.0), (0.25, 0, 0), (1, 0, 0, 0), 0.0)
    assert abs(_one(host_lib, hs, (0.0, 0.0, 0.4), (0.7, -0.3, 0.4), 0.05) - 0.1) <= TOL
    assert abs(_one(host_lib, hs, (0.0, 0.0, 0.1), (0.7, -0.3, 0.1), 0.05) + 0.2) <= TOL
    assert abs(_one(host_lib, hs, (0.0, 0.0, 0.9), (0.7, -0.3, 0.1), 0.0) + 0.15) <= TOL   # the LOWER end point counts
    # a rounding radius grows the box by that much, on faces, edges and corners
    for e0, e1 in [((-0.4, 0.2, 0.75), (0.7, 0.25, 0.75)), ((0.6, 0.6, 0.9), (0.5, 0.5, 0.8)), ((0.1, 0.2, 0.3), (0.9, 0.9, 0.9))]:
        for b in (box, rot):
            plain = _one(host_lib, b, e0, e1, 0.01)
            rounded = _one(host_lib, b[:4] + (0.03,), e0, e1, 0.01)
            assert abs((plain - rounded) - 0.03) <= 1e-6


def test_an_unnormalised_normal_and_quaternion_describe_the_same_obstacle():
    """The host normalises in fp64 (world_helpers.normalised mirrors ikf_set_world): scaling (n, d) of a half-space or the quaternion of a box changes
    nothing in the reference - so the scenes may carry unnormalised ones."""
    e0, e1 = np.array([[0.3, -0.2, 0.5]]), np.array([[0.1, 0.4, 0.2]])
    for a, b in [((HALF_SPACE, (0.0, 0.6, 0.8), (0.1, 0, 0), (1, 0, 0, 0), 0.0), (HALF_SPACE, (0.0, 1.5, 2.0), (0.25, 0, 0), (1, 0, 0, 0), 0.0)),
                 ((BOX, (0, 0, 0), (0.1, 0.2, 0.3), (0.8, 0.2, -0.4, 0.4), 0.0), (BOX, (0, 0, 0), (0.1, 0.2, 0.3), (2.4, 0.6, -1.2, 1.2), 0.0))]:
        assert abs(WH.pair_clearance(a, e0, e1, 0.0)[0] - WH.pair_clearance(b, e0, e1, 0.0)[0]) <= 1e-12


def _hit(lib, obstacles, w, radii):
    assert lib.world_host_set_world(_structs(obstacles), len(obstacles)) == 0
    w, radii = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(radii, np.float32)
    cl, ob, cp = C.c_float(), C.c_int(), C.c_int()
    lib.world_host_hit(w.ctypes.data, radii.ctypes.data, len(radii), C.byref(cl), C.byref(ob), C.byref(cp))
    return cl.value, ob.value, cp.value


def test_ties_go_to_the_lower_obstacle_then_the_lower_capsule(host_lib):
    sph = (SPHERE, (0.3, 0.1, 0.2), (0, 0, 0), (1, 0, 0, 0), 0.1)
    far = (SPHERE, (5.0, 5.0, 5.0), (0, 0, 0), (1, 0, 0, 0), 0.1)
    box = (BOX, (0.3, 0.1, 0.2), (0.1, 0.1, 0.1), (1, 0, 0, 0), 0.0)
    cap = [0.0, 0.0, 0.0, 0.0, 0.0, 0.4]
    other = [2.0, 2.0, 2.0, 2.0, 2.0, 2.4]
    cl, ob, cp = _hit(host_lib, [far, sph, sph, far, sph], [other, cap, cap, other, cap], [0.05] * 5)
    assert (ob, cp) == (1, 1) and cl < 1.0
    for same in (box, (HALF_SPACE, (0, 0, 1), (-0.3, 0, 0), (1, 0, 0, 0), 0.0), (CAPSULE, (0.3, 0.1, 0.2), (0.3, 0.5, 0.2), (1, 0, 0, 0), 0.02)):
        assert _hit(host_lib, [far, same, same], [other, other, cap, cap], [0.05] * 4)[1:] == (1, 2)
    assert _hit(host_lib, [], [cap], [0.05]) == (pytest.approx(3.0e38), -1, -1)   # an empty world
    assert _hit(host_lib, [sph], np.zeros((0, 6)), [])[1:] == (-1, -1)          # no capsules


def _set_capsules(lib, robot, caps=None):
    """caps: a capsule list (None: the small model)."""
    robot.set_collision_capsules(RH.collision_capsules(robot) if caps is None else caps)
    folded, pairs = robot._collision_model
    arr = (_lib.ikf_capsule * max(len(folded), 1))()
    for c, (frame, p0, p1, r) in zip(arr, folded):
        c.frame, c.radius = int(frame), float(r)
        for i in range(3):
            c.p0[i], c.p1[i] = float(p0[i]), float(p1[i])
    flat = (C.c_int32 * max(2 * len(pairs), 1))(*[int(v) for ab in pairs for v in ab])
    lib.world_host_set_capsules(arr, len(folded), flat, len(pairs))
    robot.set_collision_capsules(RH.collision_capsules(robot))   # (the robots are shared: the small model is back)


def _rows(lib, chain, q):
    q = np.ascontiguousarray(q.numpy(), np.float32)
    n = q.shape[0]
    cl, ob, cp = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    assert lib.world_host_rows(chain, q.ctypes.data, n, cl.ctypes.data, ob.ctypes.data, cp.ctypes.data) == 0
    return cl, ob, cp


@pytest.mark.parametrize("which", H.KIN_ALL)
def test_whole_rows_of_every_chain_in_every_scene(host_lib, which):
    """257 rows x 6 scenes: chain walk + world clearance of the kernel source within 2e-5 of the fp64 reference, the closest pair the reference's
    unless its two best pairs are within 4e-5.  And the condition the GPU tests rest on, from the reference alone: with the scene's threshold (the
    median of these rows) at most 5 % of the rows lie in the 1e-4 band and at least 20 % on either side."""
    robot, _ = H.kin_robots(which)
    chain = _chain_bytes(robot, host_lib)
    _set_capsules(host_lib, robot)
    for name in WH.SCENES:
        world = WH.scene(which, name)
        q, ref, thr = WH.rows_and_reference(which, name)
        assert host_lib.world_host_set_world(_structs(world.obstacles), len(world)) == 0
        cl, ob, cp = _rows(host_lib, chain, q)
        err = float(np.abs(cl - ref["clearance"]).max())
        band, below, above = WH.band_shares(ref["clearance"], thr)
        print(f"{which} {name}: worst {err:.2e}, clearances {ref['clearance'].min():.3f} .. {ref['clearance'].max():.3f}, threshold {thr:.4f}, "
              f"band {band:.3f} below {below:.3f} above {above:.3f}, ambiguous pairs {int(ref['ambiguous'].sum())}")
        assert err <= TOL, (which, name, err)
        sure = ~ref["ambiguous"]
        assert np.array_equal(ob[sure], ref["obstacle"][sure]) and np.array_equal(cp[sure], ref["capsule"][sure]), (which, name)
        assert band <= 0.05 and below >= 0.20 and above >= 0.20, (which, name, band, below, above)
        assert ref["clearance"].max() - ref["clearance"].min() >= 0.1   # (spread over decimetres)


@pytest.mark.parametrize("which", H.KIN_ALL)
def test_the_condition_holds_on_the_shapes_of_the_ranked_gpu_tests(which):
    """From the fp64 reference alone: every shape of 130 rows or more of tests/test_world.py's ranked cases has at most 5 % of its rows in the band
    around its threshold and at least 20 % on either side."""
    for m, k in WH.RANK_SHAPES:
        if m * k >= 130:
            cl, thr = WH.rank_case(which, m, k)[3:]
            band, below, above = WH.band_shares(cl, thr)
            assert band <= 0.05 and below >= 0.20 and above >= 0.20, (which, m, k, band, below, above)


@pytest.mark.parametrize("which", ["panda", "fetch", "syn5p"])
def test_row_scores_with_the_world_rule(host_lib, which):
    """rank_row_score_world on the 64 x 16 candidates of the GPU's ranked test, with and without reject_collisions: rank_helpers.check_row_scores
    against the reference extended by the world term."""
    robot, orob = H.kin_robots(which)
    chain = _chain_bytes(robot, host_lib)
    _set_capsules(host_lib, robot)
    caps = RH.collision_capsules(robot)
    world = WH.scene(which, WH.RANK_SCENE)
    assert host_lib.world_host_set_world(_structs(world.obstacles), len(world)) == 0
    m, k = 64, 16
    poses, q, _, cl, thr = WH.rank_case(which, m, k)
    for collisions in (False, True):
        self_thr = RH.clearance_threshold(orob, caps, q) if collisions else 0.0
        opt = _lib.ikf_rank_options(1, 0.01, 0.0, -1.0, -1.0, 0, int(collisions), self_thr)
        out = np.zeros(k * m, np.float32)
        pn, qn = np.ascontiguousarray(poses.numpy()), np.ascontiguousarray(q.numpy())
        assert host_lib.world_host_scores(chain, C.byref(opt), pn.ctypes.data, qn.ctypes.data, m, k, thr, out.ctypes.data) == 0
        ref = WH.rank_reference(orob, caps, cl, thr, poses, q, k, 0.01, self_collisions=collisions, min_clearance=self_thr)
        RH.check_row_scores(out, ref, f"{which} collisions {collisions}")
        plain = WH.rank_reference(orob, caps, None, 0.0, poses, q, k, 0.01, self_collisions=collisions, min_clearance=self_thr)
        assert (plain["admissible"] & ~ref["admissible"]).sum() > 0.1 * k * m   # (the world rule does reject rows of its own)


# ---- the capsule models by size (rank_helpers.capsule_models) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed7", "full64"])
@pytest.mark.parametrize("which", RH.CASE_CHAINS)
def test_whole_rows_with_24_capsules(host_lib, which, name):
    """The 66 rows of tests/test_world.py's 24-capsule cases through the kernel source: within 2e-5 of the fp64 reference, the closest pair the
    reference's - and it is a capsule behind the 16th on some rows.  From the reference alone: at most 2 % of the rows in the band around the
    threshold, the share below it strictly between 10 % and 90 %."""
    robot, _ = H.kin_robots(which)
    chain = _chain_bytes(robot, host_lib)
    _set_capsules(host_lib, robot, RH.capsules(which, "caps24"))
    world = WH.scene(which, name, "caps24")
    q, ref, thr = WH.rows_and_reference(which, name, "caps24")
    assert host_lib.world_host_set_world(_structs(world.obstacles), len(world)) == 0
    cl, ob, cp = _rows(host_lib, chain, q)
    err = float(np.abs(cl - ref["clearance"]).max())
    band, below, above = WH.band_shares(ref["clearance"], thr)
    print(f"{which} {name} caps24: worst {err:.2e}, threshold {thr:.4f}, band {band:.3f} below {below:.3f} above {above:.3f}, "
          f"closest capsules {sorted(set(ref['capsule'].tolist()))}")
    assert err <= TOL, (which, name, err)
    sure = ~ref["ambiguous"]
    assert np.array_equal(ob[sure], ref["obstacle"][sure]) and np.array_equal(cp[sure], ref["capsule"][sure]), (which, name)
    assert band <= 0.02 and 0.1 < below < 0.9, (which, name, band, below)
    assert len(set(ref["capsule"].tolist())) >= 5 and ref["capsule"].max() >= 16


def test_whole_rows_without_capsules(host_lib):
    for which in RH.CASE_CHAINS:
        robot, _ = H.kin_robots(which)
        chain = _chain_bytes(robot, host_lib)
        _set_capsules(host_lib, robot, [])
        world = WH.scene(which, "mixed7")
        assert host_lib.world_host_set_world(_structs(world.obstacles), len(world)) == 0
        cl, ob, cp = _rows(host_lib, chain, WH.rows_and_reference(which, "mixed7")[0][:65])
        assert (cl == np.float32(3.0e38)).all() and (ob == -1).all() and (cp == -1).all()


@pytest.mark.parametrize("model", ["caps11", "caps12", "caps24"])
@pytest.mark.parametrize("which", RH.CASE_CHAINS)
def test_row_scores_with_the_world_rule_and_the_large_models(host_lib, which, model):
    """rank_row_score_world on the rows of tests/test_world.py's ranking around the opt-in line, with and without reject_collisions; and the
    condition from the references alone: inadmissible share strictly between 10 % and 90 %, at most 2 % of the rows inside a band."""
    robot, orob = H.kin_robots(which)
    chain = _chain_bytes(robot, host_lib)
    caps = RH.capsules(which, model)
    _set_capsules(host_lib, robot, caps)
    world = WH.scene(which, WH.RANK_SCENE, model)
    assert host_lib.world_host_set_world(_structs(world.obstacles), len(world)) == 0
    c = RH.capsule_case(which, model, "tile64")
    m, k = c["m"], c["k"]
    poses, q, _, cl, thr = WH.rank_case(which, m, k, model, RH.CASE_SEEDS.get((which, model, "tile64"), 0))
    assert (q == c["q"]).all()
    for collisions in (False, True):
        self_thr = c["min_clearance"] if collisions else 0.0
        opt = _lib.ikf_rank_options(1, 0.01, 0.0, -1.0, -1.0, 0, int(collisions), self_thr)
        out = np.zeros(k * m, np.float32)
        pn, qn = np.ascontiguousarray(poses.numpy()), np.ascontiguousarray(q.numpy())
        assert host_lib.world_host_scores(chain, C.byref(opt), pn.ctypes.data, qn.ctypes.data, m, k, thr, out.ctypes.data) == 0
        ref = WH.rank_reference(orob, caps, cl, thr, poses, q, k, 0.01, self_collisions=collisions, min_clearance=self_thr, self_clearance=c["clearance"])
        RH.check_row_scores(out, ref, f"{which} {model} collisions {collisions}")
        near, bad = RH.shares(ref)
        print(f"host world ranking {which} {model} collisions {collisions}: near-band share {near:.4f}, inadmissible share {bad:.4f}")
        assert RH.shares_hold(ref), (which, model, collisions, near, bad)
