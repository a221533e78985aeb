"""The exact-IK round kernels (ikflow_amd/csrc/kin_kernels.hip: k_exact_lm_iters, k_exact_select_first, k_iota, k_compact_invalid, k_compact_count,
k_compact_offsets, k_compact_write; driven by run_exact, api_kin.hip) at every chain size, step count, compaction form and edge of the call.

1. / 2.  The ordered compaction is OBSERVED: the callback of exact_helpers.run_seeded_raw copies the engine's own active list to the host in every
         round, and the validity of every pose is fixed by construction (exact_helpers.pattern_inputs), so the lists, flags and counts are compared
         element for element with the pattern - no band, no tolerance.
3.       Every chain of helpers.KIN_ALL, fp64 and f32 steps, 1 / 2 / 3 / 20 / 255 steps, against the oracle under the criterion of
         test_exact_ik_seeded_is_row_exact_against_the_oracle (band <= 3 %, identical flags outside it, |dq| <= 5e-6 + 8 x twin sensitivity).
4.       The selection rule on constructed ties and late repeats: the winner is named.
5.       Row layout and independence: a pose alone, permuted, and one pose with 300 repeats - bit for bit.
6.       n = 0, refused arguments, guarded output windows, a non-default stream.

The conditions these inputs rest on (validity by construction, separable ties, small bands) are checked on the oracle alone, on every CPU run, by
tests/test_exact_rounds_inputs.py."""
import time

import numpy as np
import pytest
import torch

import exact_helpers as X
import helpers as H
from oracle import kinematics_oracle as ko

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
NAN_BITS = 0x7FC00000
_FRESH = {}


def _eng(which):
    from ikflow_amd.engine import kinematics_engine_for

    return kinematics_engine_for(H.kin_robots(which)[0], DEV)


def _growing_eng(which):
    """An engine of its own (not the shared one of kinematics_engine_for) whose exact-IK row state is never sized for the worst case up front
    (ikf_set_exact_upfront_rows 0): it starts from nothing and is re-allocated as the calls and their rounds need more."""
    if which not in _FRESH:
        from ikflow_amd.engine import Engine
        from ikflow_amd.model import FlowLayout

        robot = H.kin_robots(which)[0]
        _FRESH[which] = Engine(FlowLayout(nb_nodes=1, dim=max(robot.ndof, 2), dim_cond=8, width=256, n_hidden=1, clamp=2.5, ndof=robot.ndof), robot, DEV)
        _FRESH[which].set_exact_upfront_rows(0)
    return _FRESH[which]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


def _gather(n):
    """-> fn(idx): the engine's list (int32, host) as an index tensor on the device, after checking on the host that it stays inside the batch - an
    index the engine got wrong must fail the test, not reach a gather on the device."""
    def rows(idx):
        assert idx.dtype == np.int32
        if len(idx):
            assert idx.min() >= 0 and idx.max() < n, (int(idx.min()), int(idx.max()), n)
        return torch.from_numpy(idx.astype(np.int64)).to(DEV)
    return rows


# ---- 1. compaction against the pattern, exactly ------------------------------------------------------------------------------------------------
_B_OF = {"none": "runs16+5", "all": "none", "first": "last", "last": "first", "half": "runs16", "sparse": "half", "runs16": "runs16+5",
         "runs16+5": "blocks4096", "blocks4096": "half"}
# sizes: 1024 threads of the one-workgroup form (per = ceil(n / 1024): n < 1024 leaves threads empty, 1025 gives per = 2 and an empty tail), its
# switch to the three-launch form at kCompactSingle = 32768, the 4096-pose block of that form (36864 = 9 blocks exactly, 36865 = one pose into the
# tenth) and a size of 17 blocks with a 17-pose tail.  Every size takes at least three patterns, every pattern sizes on both sides of 32768.
_COMPACT = (
    (1, ("none", "all")), (2, ("none", "first", "last", "all")), (63, ("half", "runs16", "runs16+5")), (1023, ("half", "sparse", "last")),
    (1024, ("all", "runs16", "first")), (1025, ("none", "runs16+5", "last")), (4095, ("half", "blocks4096", "sparse")),
    (4097, ("blocks4096", "runs16+5", "last")), (32767, ("none", "half", "runs16", "last")),
    (32768, ("all", "sparse", "runs16+5", "blocks4096", "first")), (32769, ("none", "all", "first", "last", "half")),
    (36864, ("sparse", "runs16", "blocks4096")), (36865, ("runs16+5", "blocks4096", "last", "half")),
    (65536 + 17, ("none", "all", "first", "last", "half", "sparse", "runs16", "runs16+5", "blocks4096")))
_COMPACT_CASES = [("syn4r", n, k) for n, kinds in _COMPACT for k in kinds] + [("syn4r", 1, "first"), ("panda", 36865, "half")]


def _three_rounds(eng, c, dev):
    """The three-round call of exact_helpers.three_round_case on `eng` -> (sol, valid, stats, lists)."""
    n = len(c["A"])
    rows = _gather(n)

    def seed_fn(rnd, idx, repeat):
        assert repeat == 1
        return dev["seeds0" if rnd == 0 else "seeds1"][rows(idx)].contiguous()

    return X.run_seeded_raw(eng, dev["poses"], (1, 1, 1), X.POS_THR, X.ROT_THR, 1, seed_fn)


def _check_three_rounds(c, sol, valid, stats, lists, label):
    A, B = c["A"], c["B"]
    n = len(A)
    assert not (A & B).any() and B.sum() >= 0.9 * c["B_wanted"].sum(), (label, int(B.sum()), int(c["B_wanted"].sum()))   # round 2's list differs from round 1's wherever it was meant to
    expect = [np.arange(n, dtype=np.int32), np.flatnonzero(~A).astype(np.int32), np.flatnonzero(~A & ~B).astype(np.int32)]
    ran = 1 + (len(expect[1]) > 0) + (len(expect[1]) > 0 and len(expect[2]) > 0)     # a round whose list is empty is never started
    assert len(lists) == ran, (label, len(lists), ran)
    for r in range(ran):
        assert lists[r].dtype == np.int32 and np.array_equal(lists[r], expect[r]), (label, r, len(lists[r]), len(expect[r]))
    assert np.array_equal(valid.cpu().numpy(), (A | B).astype(np.uint8)), label
    unsolved = torch.from_numpy(~(A | B)).to(sol.device)
    assert not _bits(sol[unsolved]).any(), label                                      # exactly zero, bit for bit
    assert bool(sol[~unsolved].abs().sum(1).gt(0).all()), label
    active = [n, len(expect[1]), len(expect[2])]
    solved = [int(A.sum()), int(B.sum()), 0]
    want = np.zeros((3, 4), np.int64)
    for r in range(ran):
        want[r] = (active[r], active[r], active[r], solved[r])                       # poses, rows = poses x 1 repeat, rows x 1 step, solved
    assert np.array_equal(stats, want), (label, stats.tolist(), want.tolist())


@pytest.mark.parametrize("which,n,kind", _COMPACT_CASES, ids=lambda v: str(v))
def test_compaction_hands_each_round_exactly_the_unsolved_poses(which, n, kind):
    """rc = (1, 1, 1), one step, thresholds (1e-3, 0.05).  Round 0 solves pattern A, round 1 a pattern B among the rest (poses seeded 2.5 rad off in
    round 0 and at the truth in round 1), round 2 sees what remains.  The engine's own lists are arange(n), flatnonzero(~A) and
    flatnonzero(~A & ~B) as int32, element for element; valid == A | B; unsolved rows are zero; the stats rows are the constructed counts; a round
    with nothing left is not started (its callback is not called, its stats row stays 0).  The same call on an engine whose row state grows between
    calls and rounds (ikf_set_exact_upfront_rows 0) gives identical outputs."""
    c = X.three_round_case(which, X.make_pattern(kind, n, seed=n % 7), X.make_pattern(_B_OF[kind], n, seed=1 + n % 5), seed=n % 11)
    dev = {k: c[k].to(DEV) for k in ("poses", "seeds0", "seeds1")}
    label = f"{which} n={n} {kind}"
    out = _three_rounds(_eng(which), c, dev)
    _check_three_rounds(c, *out, label)
    again = _three_rounds(_growing_eng(which), c, dev)
    _check_three_rounds(c, *again, label + " (growing row state)")
    assert _same(out[0], again[0]) and _same(out[1], again[1]) and np.array_equal(out[2], again[2])
    assert all(np.array_equal(a, b) for a, b in zip(out[3], again[3]))


def test_row_state_grows_inside_a_call_without_changing_the_lists():
    """rc = (1, 2, 3) with nothing solvable: on the engine that never sizes for the worst case every round needs more rows than the one before
    (n, 2 n, 3 n), so the row state is re-allocated between the rounds of ONE call - the pose list must come through it."""
    n = 5000
    poses, q_true = X.pattern_inputs("syn4r", np.zeros(n, bool), 3)
    poses, q_true = poses.to(DEV), q_true.to(DEV)
    rows = _gather(n)
    for eng in (_growing_eng("syn4r"), _eng("syn4r")):
        sol, valid, stats, lists = X.run_seeded_raw(eng, poses, (1, 2, 3), X.POS_THR, X.ROT_THR, 1, lambda rnd, idx, repeat: q_true[rows(idx)].repeat((repeat, 1)))
        assert len(lists) == 3 and all(np.array_equal(l, np.arange(n, dtype=np.int32)) for l in lists)
        assert not valid.any() and not _bits(sol).any()
        assert np.array_equal(stats, np.array([[n, n, n, 0], [n, 2 * n, 2 * n, 0], [n, 3 * n, 3 * n, 0]]))


# ---- 2. more than 1024 compaction blocks -------------------------------------------------------------------------------------------------------
def test_compaction_over_more_than_1024_blocks():
    """n = 4,194,304 + 4096 + 5 = 1026 blocks of 4096 poses: k_compact_offsets gives two blocks to a thread (per = 2), the branch no smaller call
    reaches.  Inputs are built on the device with the engine's own FK; Bernoulli 0.5 with the first and the last block all solvable; rc = (1, 1), one
    step.  Round 1's list is flatnonzero(~pattern), int32, element for element.  Measured on the MI355X: inputs and call 0.15 s, checks 0.01 s."""
    which, n = "syn4r", 4_194_304 + 4096 + 5
    t0 = time.perf_counter()
    eng = _eng(which)
    orob = X.orob_of(which)
    pattern = np.random.default_rng(12).random(n) < 0.5
    pattern[:4096] = True
    pattern[-4096:] = True
    lo = torch.tensor([l[0] for l in orob.actuated_joints_limits], dtype=torch.float32, device=DEV)
    hi = torch.tensor([l[1] for l in orob.actuated_joints_limits], dtype=torch.float32, device=DEV)
    u = torch.rand((n, orob.ndof), device=DEV, generator=torch.Generator(device=DEV).manual_seed(13))
    q_true = (lo + 0.01) + u * ((hi - 0.01) - (lo + 0.01))
    poses = eng.forward_kinematics(q_true)
    far = torch.from_numpy(~pattern).to(DEV)
    poses[far, :3] += X.FAR_OFFSET
    rows = _gather(n)
    sol, valid, stats, lists = X.run_seeded_raw(eng, poses, (1, 1), X.POS_THR, X.ROT_THR, 1, lambda rnd, idx, repeat: q_true[rows(idx)].contiguous())
    t1 = time.perf_counter()
    expect = np.flatnonzero(~pattern).astype(np.int32)
    assert len(lists) == 2 and lists[0].dtype == np.int32 and lists[1].dtype == np.int32
    assert np.array_equal(lists[0], np.arange(n, dtype=np.int32))
    assert np.array_equal(lists[1], expect)
    assert np.array_equal(valid.cpu().numpy(), pattern.astype(np.uint8))
    assert not _bits(sol[far]).any()
    assert bool(sol[~far].abs().sum(1).gt(0).all())
    m = len(expect)
    assert np.array_equal(stats, np.array([[n, n, n, n - m], [m, m, m, 0]]))
    print(f"compaction over {-(-n // 4096)} blocks: inputs and call {t1 - t0:.2f} s, checks {time.perf_counter() - t1:.2f} s")


# ---- 3. every chain, both arithmetics, the step counts ----------------------------------------------------------------------------------------
def _parity_call(c, n_steps):
    which = c["which"]
    eng = _eng(which)
    ndof = eng.layout.ndof
    dev_tables = [t.to(DEV) for t in c["tables"]]
    rows = _gather(X.PARITY_N)

    def seed_fn(rnd, idx, repeat):
        assert repeat == X.PARITY_RC[rnd]
        return dev_tables[rnd][:, rows(idx), :].reshape(-1, ndof).contiguous()

    return X.run_seeded_raw(eng, c["poses"].to(DEV), X.PARITY_RC, X.POS_THR, X.ROT_THR, n_steps, seed_fn)


@pytest.mark.parametrize("case", X.PARITY_CASES, ids=X.parity_id)
def test_every_chain_and_step_count_against_the_oracle(case):
    """ikf_generate_exact_seeded, rc = (1, 3), n = 300, the noise levels of exact_helpers.PARITY_CASES, against the fp64 oracle with the same step
    count: flags, rows and zeros of the unsolved rows under the criterion of test_exact_ik_seeded_is_row_exact_against_the_oracle.  Every
    instance of k_exact_lm_iters<NDOF, double> (4 .. 8 joints, prismatic joints first, in the middle and last) runs here."""
    c = X.parity_case(case)
    sol, valid, stats, lists = _parity_call(c, c["n_steps"])
    X.check_pose_parity(sol, valid, c["ref_sol"], c["ref_valid"], c["twin_sol"], c["twin_valid"], c["band"], X.parity_id(case))
    assert stats[0, 0] == X.PARITY_N and int(valid.sum()) == int(stats[:, 3].sum())
    assert np.array_equal(stats[:, 1], stats[:, 0] * np.array(X.PARITY_RC)) and np.array_equal(stats[:, 2], stats[:, 1] * c["n_steps"])
    # round 1 was handed the poses round 0 left, in order: outside the band those are the oracle's
    assert np.array_equal(lists[0], np.arange(X.PARITY_N, dtype=np.int32)) and len(lists[1]) == stats[1, 0] and bool((np.diff(lists[1]) > 0).all())
    clear = ~c["band"]
    ref0 = ko.exact_round(X.orob_of(c["which"]), c["seed_cpu"](0, torch.arange(X.PARITY_N)), c["poses"], 1, X.POS_THR, X.ROT_THR,
                          n_opt_steps_max=c["n_steps"], lm_dtype=torch.float64)[1].numpy()
    left = np.zeros(X.PARITY_N, bool)
    left[lists[1]] = True
    assert np.array_equal(left[clear], ~ref0[clear])


def test_255_steps_fill_the_byte_and_zero_still_means_never():
    """ikf_refine_exact with the largest step count the API accepts, n = 64, R = 2 on syn5p (exact_helpers.long_case): far poses run all 255 steps
    and stay invalid, the others become valid anywhere between iteration 1 and 40 (iterations above 127: test_rows_valid_after_iteration_127_are_kept).
    Flags equal the oracle's outside the band."""
    c = X.long_case()
    eng = _eng(c["which"])
    sol, valid = eng.refine_exact(c["poses"].to(DEV), c["seeds"].to(DEV), c["R"], X.POS_THR, X.ROT_THR, n_lm_steps=X.LONG_STEPS)
    sol, valid = sol.cpu(), valid.cpu()
    clear = torch.from_numpy(~c["band"])
    print(f"255 steps: valid {int(valid.sum())} (oracle {int(c['valid'].sum())}) of {int(c['pattern'].sum())} solvable, band {int(c['band'].sum())}")
    assert c["band"].mean() <= X.BAND_CAP
    assert torch.equal(valid[clear], c["valid"][clear])
    assert not valid[torch.from_numpy(~c["pattern"])].any()
    assert not _bits(sol[~valid]).any() and bool(torch.isfinite(sol).all())
    pe, re = ko.calculate_pose_error(X.orob_of(c["which"]), sol[valid], c["poses"][valid])
    assert float(pe.max()) < X.POS_THR + (1e-4 * X.POS_THR + 5e-7) and float(re.max()) < X.ROT_THR + (1e-4 * X.ROT_THR + 6e-7 / X.ROT_THR)


def test_rows_valid_after_iteration_127_are_kept():
    """exact_helpers.late_byte_inputs (syn6r, 3000 rows, one repeat) at 127 and at 255 steps.  No such row can be named in advance (see there), so
    the kernel is held against itself and the oracle's FK: the first 127 iterations of the two calls are the same arithmetic, so every pose valid
    at 127 steps is valid at 255 with the same bits; the poses valid at 255 steps only became valid at an iteration of 128 .. 255 - the half of the
    byte no other test stores - and there are some (the oracle's own loop finds 11, the MI355X 14); each of their rows meets both thresholds under the oracle's
    f32 FK within the band constants.  A record that loses or refuses values above 127 leaves none; one that merely folds them (128 -> 0 only)
    would escape this test."""
    which, poses, seeds = X.late_byte_inputs()
    eng = _eng(which)
    poses_d, seeds_d = poses.to(DEV), seeds.to(DEV)
    s127, v127 = eng.refine_exact(poses_d, seeds_d, 1, X.POS_THR, X.ROT_THR, n_lm_steps=127)
    s255, v255 = eng.refine_exact(poses_d, seeds_d, 1, X.POS_THR, X.ROT_THR, n_lm_steps=255)
    assert bool(v255[v127].all()) and _same(s255[v127], s127[v127])
    late = (v255 & ~v127).cpu()
    print(f"late byte {which}: valid at 127 steps {int(v127.sum())}, at 255 steps {int(v255.sum())}, of them after iteration 127: {int(late.sum())}")
    assert int(late.sum()) >= 1
    pe, re = ko.calculate_pose_error(X.orob_of(which), s255.cpu()[late], poses[late])
    assert float(pe.max()) < X.POS_THR + (1e-4 * X.POS_THR + 5e-7) and float(re.max()) < X.ROT_THR + (1e-4 * X.ROT_THR + 6e-7 / X.ROT_THR)
    assert not _bits(s255[~v255]).any()


@pytest.mark.parametrize("which", X.STEP_CHAINS + ("syn5p",))
def test_f32_steps_on_every_chain_size(which):
    """ikf_set_lm_precision 0 (k_exact_lm_iters<NDOF, float>) on 4, 5, 6, 7 and 8 joints at 3 steps: a repeated call is bit-identical; every returned
    valid row meets both thresholds under the oracle's f32 FK, within the band constants; unsolved rows are zero; flags agree with the oracle's f32
    loop at least as often as the oracle's fp64 loop does, minus 0.005 (the rule of test_exact_ik_in_the_reference_lm_arithmetic)."""
    case = next(k for k in X.PARITY_CASES if k[0] == which and k[1] == 3)
    c = X.parity_case(case)
    ref32_valid = ko.generate_exact_ik_solutions_seeded(X.orob_of(which), c["seed_cpu"], c["poses"], X.PARITY_RC, X.POS_THR, X.ROT_THR, lm_dtype=torch.float32)[1]
    eng = _eng(which)
    assert eng.lm_precision == "f64"
    eng.set_lm_precision("f32")
    try:
        assert eng.lm_precision == "f32"
        sol, valid, stats, lists = _parity_call(c, 3)
        again = _parity_call(c, 3)
    finally:
        eng.set_lm_precision("f64")    # (engines of kinematics_engine_for are shared)
    assert _same(sol, again[0]) and _same(valid, again[1]) and np.array_equal(stats, again[2]) and all(np.array_equal(a, b) for a, b in zip(lists, again[3]))
    sol, valid = sol.cpu(), valid.cpu().bool()
    pe, re = ko.calculate_pose_error(X.orob_of(which), sol[valid], c["poses"][valid])
    agree, agree_twins = float((valid == ref32_valid).float().mean()), float((c["ref_valid"] == ref32_valid).float().mean())
    print(f"f32 steps {which}: valid {int(valid.sum())} (oracle f32 loop {int(ref32_valid.sum())}, fp64 loop {int(c['ref_valid'].sum())}); pos max {float(pe.max()):.3e} "
          f"rot max {float(re.max()):.3e}; flags agree {agree:.4f} (fp64 loop against f32 loop {agree_twins:.4f})")
    assert int(valid.sum()) > 0
    assert float(pe.max()) < X.POS_THR + (1e-4 * X.POS_THR + 5e-7) and float(re.max()) < X.ROT_THR + (1e-4 * X.ROT_THR + 6e-7 / X.ROT_THR)
    assert not _bits(sol[~valid]).any()
    assert agree >= agree_twins - 0.005


# ---- 4. the winner, named ---------------------------------------------------------------------------------------------------------------------
def _dist(sol, rows_q):
    return np.abs(sol.astype(np.float64) - rows_q).max(1)


@pytest.mark.parametrize("which", X.REDUNDANT)
def test_among_repeats_valid_in_the_same_iteration_the_highest_wins(which):
    """exact_helpers.tie_case (n = 500, R = 4, one step: all four repeats of every pose are valid at iteration 1).  valid is all true; on every
    named pose the row lies within 5e-6 + 8 x sensitivity of the oracle's row of repeat R - 1 and further than 1e-4 from the oracle's row of
    every other repeat."""
    c = X.tie_case(which)
    R = c["R"]
    sol, valid = _eng(which).refine_exact(c["poses"].to(DEV), c["seeds"].to(DEV), R, X.POS_THR, X.ROT_THR, n_lm_steps=1)
    sol, named = sol.cpu().numpy(), c["named"]
    assert bool(valid.all())
    d = [_dist(sol, c["rows"]["q"][r]) for r in range(R)]
    print(f"tie {which}: named {int(named.sum())} of {len(named)}; to the winner's row max {d[R - 1][named].max():.2e}, to the nearest other repeat's min "
          f"{min(d[r][named].min() for r in range(R - 1)):.2e}")
    assert named.mean() >= 0.9
    assert (d[R - 1][named] <= c["allowed"][named]).all()
    for r in range(R - 1):
        assert (d[r][named] > X.SEPARATION).all(), r


@pytest.mark.parametrize("swapped", [False, True], ids=["early-first", "early-last"])
@pytest.mark.parametrize("which", X.REDUNDANT)
def test_the_earliest_iteration_wins_whichever_repeat_it_is(which, swapped):
    """exact_helpers.late_case (n = 500, R = 2, 3 steps): one repeat is valid at iteration 1, the other at iteration 2 or 3.  The row is the early
    repeat's - repeat 0's although a higher repeat becomes valid later, and with the seed blocks swapped the last repeat's: neither the repeat
    order nor the pose_first hint decides the result."""
    c = X.late_case(which, swapped=swapped)
    sol, valid = _eng(which).refine_exact(c["poses"].to(DEV), c["seeds"].to(DEV), c["R"], X.POS_THR, X.ROT_THR, n_lm_steps=X.LATE_STEPS)
    sol, kept = sol.cpu().numpy(), c["kept"]
    de, dl = _dist(sol, c["rows"]["q"][c["early"]]), _dist(sol, c["rows"]["q"][c["late"]])
    print(f"late {which} early repeat {c['early']}: kept {int(kept.sum())} of {len(kept)}; to the early row max {de[kept].max():.2e}, to the late row min {dl[kept].min():.2e}")
    assert kept.mean() >= 0.5
    assert bool(valid.cpu()[torch.from_numpy(kept)].all())
    assert (de[kept] <= c["allowed"][kept]).all()
    assert (dl[kept] > X.SEPARATION).all()


# ---- 5. layout and independence -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["panda", "syn6p"])
def test_a_pose_alone_and_a_permuted_batch_are_bit_identical(which):
    """n = 257, R = 5 (row = r * n + j: 1285 rows, six workgroups; pose 256 is the last of a block of k_exact_select_first and the first of the next).
    A pose solved alone with its five seeds gives row j and flag j of the batch call; permuting the poses, and the seed columns with them,
    permutes the outputs."""
    eng = _eng(which)
    n, R = 257, 5
    poses, tab = X.layout_inputs(which, n, R)
    poses, tab = poses.to(DEV), tab.to(DEV)
    ndof = tab.shape[2]
    sol, valid = eng.refine_exact(poses, tab.reshape(R * n, ndof), R, X.POS_THR, X.ROT_THR)
    assert 0 < int(valid.sum()) < n
    for j in (0, 1, 255, 256):
        s1, v1 = eng.refine_exact(poses[j:j + 1].contiguous(), tab[:, j, :].contiguous(), R, X.POS_THR, X.ROT_THR)
        assert _same(s1, sol[j:j + 1]) and _same(v1, valid[j:j + 1]), j
    perm = torch.from_numpy(np.random.default_rng(5).permutation(n)).to(DEV)
    sp, vp = eng.refine_exact(poses[perm].contiguous(), tab[:, perm, :].reshape(R * n, ndof).contiguous(), R, X.POS_THR, X.ROT_THR)
    assert _same(sp, sol[perm]) and _same(vp, valid[perm])


@pytest.mark.parametrize("which", ["panda", "syn6p"])
def test_one_pose_with_300_repeats(which):
    """n = 1, R = 300: the repeats of one pose span two workgroups of k_exact_lm_iters and share one pose_first word.  The oracle's answer under the
    criterion, and the same bits in three calls."""
    c = X.single_pose_case(which)
    eng = _eng(which)
    poses, seeds = c["poses"].to(DEV), c["seeds"].to(DEV)
    outs = [eng.refine_exact(poses, seeds, c["R"], X.POS_THR, X.ROT_THR) for _ in range(3)]
    assert all(_same(o[0], outs[0][0]) and _same(o[1], outs[0][1]) for o in outs[1:])
    X.check_pose_parity(outs[0][0], outs[0][1], c["sol"], c["valid"], c["twin_sol"], c["twin_valid"], c["band"], f"one pose {which}")


# ---- 6. edges of the call ---------------------------------------------------------------------------------------------------------------------
def _guarded(n, ndof):
    sol = torch.full((n + 2 * GUARD, ndof), float("nan"), dtype=torch.float32, device=DEV)
    valid = torch.full((n + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    return sol, valid


def _check_guards(sol_buf, valid_buf, n, label):
    assert (_bits(sol_buf[:GUARD]) == NAN_BITS).all() and (_bits(sol_buf[GUARD + n:]) == NAN_BITS).all(), f"{label}: a row outside the {n} poses was written"
    assert (valid_buf[:GUARD] == 0xAB).all() and (valid_buf[GUARD + n:] == 0xAB).all(), f"{label}: a flag outside the {n} poses was written"


def test_zero_poses_touch_nothing_and_clear_the_stats():
    eng = _eng("syn4r")
    sol_buf, valid_buf = _guarded(0, eng.layout.ndof)
    called = []
    sol, valid, stats, lists = X.run_seeded_raw(eng, torch.zeros((0, 7), dtype=torch.float32, device=DEV), (1, 3), X.POS_THR, X.ROT_THR, 3,
                                                lambda *a: called.append(a), sol=sol_buf[GUARD:GUARD], valid=valid_buf[GUARD:GUARD], stats_fill=-7)
    assert not called and not lists
    assert not stats.any() and stats.shape == (2, 4)
    _check_guards(sol_buf, valid_buf, 0, "n = 0")


@pytest.mark.parametrize("rc,steps,message", [((1,), 0, "n_lm_steps must be in 1..255"), ((1,), 256, "n_lm_steps must be in 1..255"),
                                              ((1, 0), 3, "repeat counts must be >= 1"), ((1,) * 9, 3, "repeat_counts must hold 1..8 rounds")])
def test_refused_arguments(rc, steps, message):
    from ikflow_amd.engine import EngineError

    eng = _eng("syn4r")
    poses, q_true = X.pattern_inputs("syn4r", np.ones(8, bool), 1)
    sol_buf, valid_buf = _guarded(8, eng.layout.ndof)
    called = []
    with pytest.raises(EngineError, match=message):
        X.run_seeded_raw(eng, poses.to(DEV), rc, X.POS_THR, X.ROT_THR, steps, lambda *a: called.append(a), sol=sol_buf[GUARD:GUARD + 8], valid=valid_buf[GUARD:GUARD + 8])
    assert not called
    _check_guards(sol_buf, valid_buf, 8, message)
    assert (_bits(sol_buf) == NAN_BITS).all() and (valid_buf == 0xAB).all()           # a refused call writes nothing


def _guarded_round(which, n, stream=None):
    """One round (rc = (1,)) of a Bernoulli 0.5 pattern into NaN / 0xAB windows with guard rows on either side -> (sol window, valid window, stats)."""
    eng = _eng(which)
    pattern = X.make_pattern("half", n, 2)
    poses, q_true = X.pattern_inputs(which, pattern, 4)
    poses, q_true = poses.to(DEV), q_true.to(DEV)
    rows = _gather(n)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        sol_buf, valid_buf = _guarded(n, eng.layout.ndof)
        sol, valid, stats, lists = X.run_seeded_raw(eng, poses, (1,), X.POS_THR, X.ROT_THR, 1, lambda rnd, idx, repeat: q_true[rows(idx)].contiguous(),
                                                    sol=sol_buf[GUARD:GUARD + n], valid=valid_buf[GUARD:GUARD + n])
    torch.cuda.synchronize()
    _check_guards(sol_buf, valid_buf, n, f"{which} n={n}")
    # every element inside is written after round 0, also for poses that are never solved: zeros and 0, not the caller's bytes
    assert not torch.isnan(sol).any() and (valid <= 1).all()
    assert np.array_equal(valid.cpu().numpy(), pattern.astype(np.uint8))
    assert not _bits(sol[torch.from_numpy(~pattern).to(DEV)]).any()
    assert np.array_equal(stats, np.array([[n, n, n, int(pattern.sum())]]))
    return sol.clone(), valid.clone(), stats


@pytest.mark.parametrize("which,n", [("syn4r", 1), ("syn4r", 257), ("syn8p", 257), ("syn4r", 32769)])
def test_output_windows_are_written_whole_and_nothing_beyond(which, n):
    _guarded_round(which, n)


def test_on_a_non_default_stream():
    """One call of every kind on a stream of its own: the guarded round, a three-round compaction of either form, a parity case (rc = (1, 3),
    3 steps), a tie and a late-repeat call through refine_exact - the same bits as on the default stream - and n = 0 and a refused call, which
    touch nothing there either.  (The other cases of the parity, tie and late tables differ from these in their inputs, not in how they are
    launched; they run on the default stream only.)"""
    st = torch.cuda.Stream(device=DEV)
    ref = _guarded_round("syn5p", 257)
    got = _guarded_round("syn5p", 257, stream=st)
    assert _same(ref[0], got[0]) and _same(ref[1], got[1])
    for n in (1025, 36865):
        c = X.three_round_case("syn4r", X.make_pattern("half", n, 1), X.make_pattern("runs16+5", n), 3)
        dev = {k: c[k].to(DEV) for k in ("poses", "seeds0", "seeds1")}
        ref = _three_rounds(_eng("syn4r"), c, dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            got = _three_rounds(_eng("syn4r"), c, dev)
        torch.cuda.synchronize()
        _check_three_rounds(c, *got, f"stream n={n}")
        assert _same(ref[0], got[0]) and _same(ref[1], got[1]) and all(np.array_equal(a, b) for a, b in zip(ref[3], got[3]))
    t = X.tie_case("panda")
    eng = _eng("panda")
    poses, seeds = t["poses"].to(DEV), t["seeds"].to(DEV)
    ref = eng.refine_exact(poses, seeds, t["R"], X.POS_THR, X.ROT_THR, n_lm_steps=1)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        got = eng.refine_exact(poses, seeds, t["R"], X.POS_THR, X.ROT_THR, n_lm_steps=1)
    torch.cuda.synchronize()
    assert _same(ref[0], got[0]) and _same(ref[1], got[1])
    for t, steps in ((X.late_case("panda"), X.LATE_STEPS), (X.late_case("panda", swapped=True), X.LATE_STEPS)):
        poses, seeds = t["poses"].to(DEV), t["seeds"].to(DEV)
        ref = eng.refine_exact(poses, seeds, t["R"], X.POS_THR, X.ROT_THR, n_lm_steps=steps)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            got = eng.refine_exact(poses, seeds, t["R"], X.POS_THR, X.ROT_THR, n_lm_steps=steps)
        torch.cuda.synchronize()
        assert _same(ref[0], got[0]) and _same(ref[1], got[1])
    c = X.parity_case(next(k for k in X.PARITY_CASES if k[0] == "panda" and k[1] == 3))
    ref = _parity_call(c, 3)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        got = _parity_call(c, 3)
    torch.cuda.synchronize()
    assert _same(ref[0], got[0]) and _same(ref[1], got[1]) and np.array_equal(ref[2], got[2]) and all(np.array_equal(a, b) for a, b in zip(ref[3], got[3]))
    from ikflow_amd.engine import EngineError

    e4 = _eng("syn4r")
    p8 = X.pattern_inputs("syn4r", np.ones(8, bool), 1)[0].to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        sol_buf, valid_buf = _guarded(8, e4.layout.ndof)
        called = []
        out = X.run_seeded_raw(e4, p8[:0].contiguous(), (1, 3), X.POS_THR, X.ROT_THR, 3, lambda *a: called.append(a), sol=sol_buf[GUARD:GUARD], valid=valid_buf[GUARD:GUARD], stats_fill=-7)
        assert not called and not out[3] and not out[2].any()
        with pytest.raises(EngineError, match="n_lm_steps must be in 1..255"):
            X.run_seeded_raw(e4, p8, (1,), X.POS_THR, X.ROT_THR, 256, lambda *a: called.append(a), sol=sol_buf[GUARD:GUARD + 8], valid=valid_buf[GUARD:GUARD + 8])
    torch.cuda.synchronize()
    assert not called and (_bits(sol_buf) == NAN_BITS).all() and (valid_buf == 0xAB).all()
