"""The arithmetic of best-of-K ranking (ikflow_amd/csrc/rank_math.h: row score, admissibility, capsule clearance, the sorted top list, the
chunk rule) compiled for the HOST with g++ and held against the oracle and numpy - the kernels' own source, checked without a GPU.  The GPU
tests check the same code where it ships (tests/test_ranked.py).  Test infrastructure: nothing in ikflow_amd/ loads it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import rank_helpers as RH
from ikflow_amd import _lib
from test_kin_math_host import _chain_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("rank_math") / "librank_math_host.so"
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "rank_math_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(str(out))
    lib.kin_math_chain_bytes = lib.rank_host_chain_bytes   # (what _chain_bytes asks the library it packs for)
    lib.rank_host_scores.argtypes = [C.c_void_p, C.POINTER(_lib.ikf_rank_options), C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]
    lib.rank_host_set_collision.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.rank_host_set_collision.restype = None
    lib.rank_host_toplist.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.rank_host_chunks.argtypes = [C.c_longlong, C.c_int, C.c_int]
    lib.rank_host_tile_poses.argtypes = [C.c_longlong]
    return lib


def _set_collision(lib, robot, caps=None, every_pair=False):
    """caps: a capsule list (None: the small model); every_pair: all n (n - 1) / 2 pairs instead of the generated ones."""
    robot.set_collision_capsules(RH.collision_capsules(robot) if caps is None else caps)
    folded, pairs = robot._collision_model
    if every_pair:
        pairs = RH.all_pairs(len(folded))
    arr = (_lib.ikf_capsule * max(len(folded), 1))()
    for c, (frame, p0, p1, r) in zip(arr, folded):
        c.frame, c.radius = int(frame), float(r)
        for i in range(3):
            c.p0[i], c.p1[i] = float(p0[i]), float(p1[i])
    flat = (C.c_int32 * max(2 * len(pairs), 1))(*[int(v) for ab in pairs for v in ab])
    lib.rank_host_set_collision(arr, len(folded), flat, len(pairs))
    robot.set_collision_capsules(RH.collision_capsules(robot))   # (the robots are shared: the small model is back)


def _scores(lib, chain, opt, poses, q, q_ref, k, clearance=False):
    m = poses.shape[0]
    out = np.zeros(k * m, np.float32)
    cl = np.zeros(k * m, np.float32) if clearance else None
    poses, q = np.ascontiguousarray(poses.numpy()), np.ascontiguousarray(q.numpy())
    qr = None if q_ref is None else np.ascontiguousarray(q_ref.numpy())
    assert lib.rank_host_scores(chain, C.byref(opt), poses.ctypes.data, q.ctypes.data, None if qr is None else qr.ctypes.data, m, k, out.ctypes.data,
                                None if cl is None else cl.ctypes.data) == 0
    return (out, cl) if clearance else out


def _opt(n_keep=1, rot_weight=0.01, ref_weight=0.0, max_pos=None, max_rot=None, limits=False, collisions=False, min_clearance=0.0):
    return _lib.ikf_rank_options(n_keep, rot_weight, ref_weight, -1.0 if max_pos is None else max_pos, -1.0 if max_rot is None else max_rot,
                                 int(limits), int(collisions), min_clearance)


VARIANTS = {
    "plain": dict(),
    "q_ref": dict(ref_weight=0.05),
    "thresholds": dict(max_pos=0.02, max_rot=0.3),
    "limits_wild": dict(limits=True),
    "collisions": dict(collisions=True),   # min_clearance: rank_helpers.clearance_threshold of the rows
}


@pytest.mark.parametrize("rot_weight", [0.01, 1.0])
@pytest.mark.parametrize("which", ["panda", "fetch", "syn5p"])
def test_row_scores_of_the_kernel_source_on_the_host(host_lib, which, rot_weight):
    robot, orob = H.kin_robots(which)
    chain = _chain_bytes(robot, host_lib)
    _set_collision(host_lib, robot)
    caps = RH.collision_capsules(robot)
    m, k = 64, 20
    for name, v in VARIANTS.items():
        poses, q, q_ref = RH.candidates(orob, m, k, seed=3, wild=name == "limits_wild")
        use_ref = name == "q_ref"
        if name == "collisions":
            v = dict(v, min_clearance=RH.clearance_threshold(orob, caps, q))
        opt = _opt(rot_weight=rot_weight, **v)
        got = _scores(host_lib, chain, opt, poses, q, q_ref if use_ref else None, k)
        ref = RH.reference(orob, poses, q, k, rot_weight, q_ref if use_ref else None, v.get("ref_weight", 0.0), v.get("max_pos"), v.get("max_rot"),
                           v.get("limits", False), caps if v.get("collisions") else None, v.get("min_clearance", 0.0))
        worst = RH.check_row_scores(got, ref, f"{which} {name}")
        n_bad = int((~ref["admissible"]).sum())
        print(f"host row scores {which} rot_weight {rot_weight} {name}: worst {worst:.3f} of eps, {n_bad} of {k * m} rows inadmissible")
        if name != "plain" and name != "q_ref":
            assert 0 < n_bad < k * m, f"{name}: the variant rejects {n_bad} of {k * m} rows, so it does not test the rule"


@pytest.mark.parametrize("which", ["panda", "fetch", "syn5p"])
def test_the_f32_oracles_own_scores_stay_within_the_tolerance(which):
    """Where the tolerance is not taken from the code under test: on every input family of the ranking tests the f32 oracle is within eps of
    the fp64 oracle on every row."""
    orob = H.kin_robots(which)[1]
    for rot_weight in (0.01, 1.0):
        for lo_exp, hi_exp in ((-3.0, 0.0), (-0.7, 0.0)):
            poses, q, q_ref = RH.candidates(orob, 64, 50, seed=5, lo_exp=lo_exp, hi_exp=hi_exp)
            r64 = RH.reference(orob, poses, q, 50, rot_weight, q_ref, 0.05)
            r32 = RH.reference(orob, poses, q, 50, rot_weight, q_ref, 0.05, dtype=torch.float32)
            ratio = np.abs(r32["score"] - r64["score"]) / r64["eps"]
            assert ratio.max() <= 1.0, (which, rot_weight, lo_exp, float(ratio.max()))


def test_clearance_of_the_kernel_source_against_the_oracle(host_lib):
    from oracle import kinematics_oracle as ko

    for which in ("panda", "fetch", "syn5p"):
        robot, orob = H.kin_robots(which)
        chain = _chain_bytes(robot, host_lib)
        _set_collision(host_lib, robot)
        poses, q, _ = RH.candidates(orob, 64, 20, seed=4)
        _, cl = _scores(host_lib, chain, _opt(), poses, q, None, 20, clearance=True)
        ref = ko.capsule_clearance(orob, RH.collision_capsules(robot), (), q.double()).numpy()
        assert np.abs(cl - ref).max() <= 2e-5, (which, float(np.abs(cl - ref).max()))


def _toplist(lib, scores, n_keep, n_slices, rng, reverse):
    k = len(scores)
    cap = 1 if n_keep <= 1 else 4 if n_keep <= 4 else 16
    s = np.ascontiguousarray(scores, dtype=np.float32)
    order = np.ascontiguousarray(rng.permutation(n_slices), dtype=np.int32)
    out_s, out_i = np.zeros(cap, np.float32), np.zeros(cap, np.int32)
    assert lib.rank_host_toplist(cap, s.ctypes.data, k, n_slices, order.ctypes.data, int(reverse), out_s.ctypes.data, out_i.ctypes.data) == 0
    return out_s[:n_keep], out_i[:n_keep]


def _toplist_cases():
    rng = np.random.default_rng(0)
    inf = np.float32(np.inf)
    dup = rng.choice(np.array([0.1, 0.2, 0.3, 0.4], np.float32), 200)
    some_inf = rng.random(130).astype(np.float32)
    some_inf[rng.random(130) < 0.5] = inf
    few = np.full(90, inf, np.float32)
    few[[89, 3, 40]] = [0.5, 0.5, 0.25]
    return {
        "random": rng.random(1000).astype(np.float32),
        "all_equal": np.full(300, 0.25, np.float32),
        "duplicates": dup,
        "some_inf": some_inf,
        "few_finite": few,
        "all_inf": np.full(70, inf, np.float32),
        "k16": rng.random(16).astype(np.float32),
        "k1": np.array([0.7], np.float32),
        "k1_inf": np.array([inf], np.float32),
    }


@pytest.mark.parametrize("case", list(_toplist_cases()))
def test_top_list_equals_the_stable_lexsort_whatever_the_split(host_lib, case):
    """insert + merge give exactly np.lexsort((index, score))[:n_keep] of the same f32 scores, for 1, 2, 7 and 64 slices merged in a random order and
    for both insertion orders: the selection does not depend on how the candidates are split over threads, waves or workgroups."""
    scores = _toplist_cases()[case]
    k = len(scores)
    rng = np.random.default_rng(7)
    for n_keep in sorted({1, min(4, k), min(16, k), min(k, 3)}):
        want_i, want_s, want_c = RH.select(scores, 1, k, n_keep)
        for n_slices in (1, 2, 7, 64):
            for reverse in (False, True):
                got_s, got_i = _toplist(host_lib, scores, n_keep, n_slices, rng, reverse)
                got_i = np.where(np.isfinite(got_s), got_i, -1)   # (a free slot carries INT32_MAX; the kernel writes -1)
                assert np.array_equal(got_i, want_i[0]) and np.array_equal(got_s.view(np.int32), want_s[0].view(np.int32)), (case, n_keep, n_slices, reverse)
    if case == "all_equal":
        assert np.array_equal(RH.select(scores, 1, k, 16)[0][0], np.arange(16))   # ties: the lowest indices, ascending


def test_chunk_rule_is_sane_on_every_shape(host_lib):
    """rank_chunks(m, k, n_cu): 1 .. 64, never more chunks than repeats, no empty chunk, every thread of a chunked call keeps at least 4 rows' worth of
    repeats per slice, and the shapes the GPU tests rely on fall where they say (k <= 2: one chunk; one pose x 5000: chunked)."""
    for n_cu in (256, 304, 64, 8):
        for m in (1, 2, 3, 63, 64, 65, 257, 1000, 4096, 100000):
            for k in (1, 2, 4, 50, 64, 65, 1000, 5000):
                c = host_lib.rank_host_chunks(m, k, n_cu)
                per = -(-k // c)
                assert 1 <= c <= 64 and c <= k and (c - 1) * per < k, (n_cu, m, k, c)
                if c > 1:
                    slices = 128 // host_lib.rank_host_tile_poses(m)
                    assert per >= 4 * slices // 2, (n_cu, m, k, c, per)
        assert host_lib.rank_host_chunks(1, 5000, n_cu) > 1 and host_lib.rank_host_chunks(3, 1000, n_cu) > 1
        assert host_lib.rank_host_chunks(1000, 2, n_cu) == 1 and host_lib.rank_host_chunks(1, 1, n_cu) == 1
    assert [host_lib.rank_host_tile_poses(m) for m in (1, 2, 3, 33, 64, 65, 10 ** 6)] == [1, 2, 4, 64, 64, 64, 64]


# ---- the capsule models by size (rank_helpers.capsule_models) -----------------------------------------------------------------------------------
TRUNCATION_CHAINS = ("syn4r", "panda", "fetch", "syn6r")   # every chain that meets its 24-capsule model in a GPU test


def test_the_capsule_models_have_the_counts_and_occupy_every_frame():
    for which in H.KIN_ALL:
        robot = H.kin_robots(which)[0]
        models = RH.capsule_models(robot)
        assert [len(models[f"caps{n}"]) for n in RH.CAPSULE_COUNTS] == list(RH.CAPSULE_COUNTS) and models["caps5"] == RH.collision_capsules(robot)
        for n in RH.LARGE_COUNTS:
            robot.set_collision_capsules(models[f"caps{n}"])
            folded, pairs = robot._collision_model
            per_frame = np.bincount([f[0] for f in folded], minlength=robot.ndof + 1)
            assert len(per_frame) == robot.ndof + 1 and (per_frame >= 1).all() and per_frame.max() >= 2, (which, n, per_frame)
            assert len(pairs) > 9 and len(pairs) == n * (n - 1) // 2 - sum(c * (c - 1) // 2 for c in per_frame)
        robot.set_collision_capsules(models["caps5"])


@pytest.mark.parametrize("which", TRUNCATION_CHAINS)
def test_the_later_capsules_of_the_24_capsule_model_decide_rows(which):
    """From the fp64 oracle alone, on the rows of the tile64 case: the clearance under the first 16 capsules, and under the first 5, differs from
    the clearance under all 24 on at least a tenth of the rows - so a loop that stops early, or a slice stride that leaves the later capsules
    out, changes results."""
    orob = H.kin_robots(which)[1]
    c = RH.capsule_case(which, "caps24", "tile64")
    caps = RH.capsules(which, "caps24")
    full = c["clearance"]
    shares = [float((RH.clearance(orob, caps[:n], c["q"]) != full).mean()) for n in (16, 5)]
    print(f"{which}: the clearance changes on {shares[0]:.3f} of the rows without capsules 17 .. 24, on {shares[1]:.3f} without 6 .. 24; "
          f"fp64 clearances {full.min():.4f} .. {full.max():.4f}")
    assert min(shares) >= 0.1, (which, shares)


HOST_CASES = [(w, mo) for w in RH.CASE_CHAINS for mo in RH.REJECTING]


@pytest.mark.parametrize("which,model", HOST_CASES)
def test_row_scores_of_the_kernel_source_with_every_capsule_count(host_lib, which, model):
    """The capsule cases of tests/test_ranked.py through the kernel source on the CPU: clearance within 2e-5 of the oracle, row scores by
    check_row_scores.  And the condition those tests rest on, from the oracle alone: with min_clearance the median of the rows' clearances
    (seed: rank_helpers.CASE_SEEDS) the inadmissible share lies strictly between 10 % and 90 % and at most 2 % of the rows lie inside a band."""
    robot, orob = H.kin_robots(which)
    chain = _chain_bytes(robot, host_lib)
    caps = RH.capsules(which, model)
    _set_collision(host_lib, robot, caps)
    shapes = ["tile1", "tile64"] + (["chunked"] if model == "caps14" or (which, model) == ("panda", "caps24") else [])
    for shape in shapes:
        c = RH.capsule_case(which, model, shape)
        opt = _opt(collisions=True, min_clearance=c["min_clearance"])
        got, cl = _scores(host_lib, chain, opt, c["poses"], c["q"], None, c["k"], clearance=True)
        assert np.abs(cl - c["clearance"]).max() <= 2e-5, (which, model, shape, float(np.abs(cl - c["clearance"]).max()))
        ref = RH.reference(orob, c["poses"], c["q"], c["k"], 0.01, caps=caps, min_clearance=c["min_clearance"], self_clearance=c["clearance"])
        near, bad = RH.shares(ref)
        worst = RH.check_row_scores(got, ref, f"{which} {model} {shape}")
        print(f"host {which} {model} {shape}: seed {RH.CASE_SEEDS.get((which, model, shape), 0)}, near-band share {near:.4f}, inadmissible share {bad:.4f}, "
              f"worst {worst:.3f} of eps")
        assert RH.shares_hold(ref), (which, model, shape, near, bad)


@pytest.mark.parametrize("which", RH.CASE_CHAINS)
def test_models_without_pairs_and_with_every_pair_on_the_host(host_lib, which):
    """caps0 and caps1 have no pair: the clearance is 3.0e38 and reject_collisions changes no score.  caps24 with all 276 pairs listed: the
    oracle, which skips same-frame pairs, bounds the clearance from above."""
    robot, orob = H.kin_robots(which)
    chain = _chain_bytes(robot, host_lib)
    c = RH.capsule_case(which, "caps24", "tile64")
    for model in ("caps0", "caps1"):
        _set_collision(host_lib, robot, RH.capsules(which, model))
        plain = _scores(host_lib, chain, _opt(), c["poses"], c["q"], None, c["k"])
        got, cl = _scores(host_lib, chain, _opt(collisions=True, min_clearance=0.05), c["poses"], c["q"], None, c["k"], clearance=True)
        assert H.same_bits(got, plain) and (cl == np.float32(3.0e38)).all(), (which, model)
    _set_collision(host_lib, robot, RH.capsules(which, "caps24"), every_pair=True)
    _, cl = _scores(host_lib, chain, _opt(), c["poses"], c["q"], None, c["k"], clearance=True)
    assert (cl <= c["clearance"] + 2e-5).all() and (cl < c["clearance"] - 1e-4).any()   # (and same-frame pairs do decide rows)
