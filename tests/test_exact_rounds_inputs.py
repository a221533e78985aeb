"""The conditions tests/test_exact_rounds.py leans on, checked on the oracle alone (no GPU): validity fixed by construction, ties and late repeats
whose winner can be named, parity cases with a small band and both outcomes.  Prints the shares it measures."""
import numpy as np
import pytest
import torch

import exact_helpers as X
import helpers as H
from oracle import kinematics_oracle as ko


@pytest.mark.parametrize("which", H.KIN_ALL)
def test_pattern_construction_fixes_validity(which):
    """2000 rows, Bernoulli 0.5 solvable, 2 steps, thresholds (1e-3, 0.05), LM step in fp64 and in f32: valid == pattern exactly.  A truth seed is
    valid after the FIRST step with both errors at most a tenth of their threshold (so its margin is 0.9 x the threshold, the band 1e-4 x), a far
    pose stays at least ten thresholds (in fact over 100 m) away in position: no row is in the band.  (A far pose's rotation error is free to pass
    through its threshold - the position alone keeps the pose invalid - so only its position margin is looked at.)"""
    orob = X.orob_of(which)
    pattern = X.make_pattern("half", 2000, 3)
    poses, seeds = X.pattern_inputs(which, pattern, 5)
    for dt in (torch.float64, torch.float32):
        margins = torch.full((len(pattern), 2), float("inf"), dtype=torch.float64)
        sol, valid = ko.exact_round(orob, seeds, poses, 1, X.POS_THR, X.ROT_THR, n_opt_steps_max=2, lm_dtype=dt, margins=margins)
        assert np.array_equal(valid.numpy(), pattern)
        one, _ = ko.exact_round(orob, seeds, poses, 1, X.POS_THR, X.ROT_THR, n_opt_steps_max=1, lm_dtype=dt)
        assert torch.equal(one, sol)                                               # ... after the first step already
        pe, re = ko.calculate_pose_error(orob, sol[pattern], poses[pattern])
        m = margins.numpy()
        print(f"pattern {which} {str(dt)[-7:]}: truth rows pos {float(pe.max()):.1e} rot {float(re.max()):.1e}; far rows: smallest position margin {m[~pattern, 0].min():.0f} m")
        assert float(pe.max()) <= X.POS_THR / 10 and float(re.max()) <= X.ROT_THR / 10
        assert m[~pattern, 0].min() >= 10 * X.POS_THR
        band = X.band_of(margins, X.POS_THR, X.ROT_THR)
        assert not band[pattern].any() and not (m[~pattern, 0] <= 1e-4 * X.POS_THR + 5e-7).any()
        assert torch.equal(sol[~pattern], torch.zeros_like(sol[~pattern]))


@pytest.mark.parametrize("which", ["syn4r", "panda"])
def test_three_round_schedule_on_the_oracle(which):
    """The schedule of the compaction tests through the oracle's own loop: round 0 solves A, round 1 the part of B outside A, round 2 nothing -
    and the lists the rounds are handed are flatnonzero(~A) and flatnonzero(~A & ~B)."""
    n = 1025
    want_B = X.make_pattern("runs16+5", n)
    c = X.three_round_case(which, X.make_pattern("half", n, 1), want_B, 3)
    A, B = c["A"], c["B"]
    print(f"three rounds {which}: |A| {A.sum()} |B| {B.sum()} of {(want_B & ~A).sum()} wanted")
    assert not (A & B).any() and B.sum() >= 0.9 * (want_B & ~A).sum()
    seen = []

    def seed_cpu(rnd, idx):
        seen.append(idx.numpy())
        return (c["seeds0"] if rnd == 0 else c["seeds1"])[idx]

    sol, valid, margins = X.oracle_seeded(which, seed_cpu, c["poses"], (1, 1, 1), X.POS_THR, X.ROT_THR, 1)
    assert np.array_equal(seen[0], np.arange(n)) and np.array_equal(seen[1], np.flatnonzero(~A)) and np.array_equal(seen[2], np.flatnonzero(~A & ~B))
    assert np.array_equal(valid.numpy(), A | B)


@pytest.mark.parametrize("which", X.REDUNDANT)
def test_tie_inputs_name_their_winner(which):
    """n = 500, R = 4, one step: every repeat of every pose is valid at iteration 1, the oracle's answer is repeat R - 1's row, and on at least
    90 % of the poses that row is more than 1e-4 from every other repeat's (`named`, what the GPU test uses, asks 1e-4 + the row's own allowance)."""
    c = X.tie_case(which)
    R = c["R"]
    print(f"tie {which}: separable {c['separable'].mean():.3f}, named {c['named'].mean():.3f}, band {int(c['band'].sum())}")
    assert c["rows"]["conv"].all() and (c["rows"]["steps"] == 1).all() and bool(c["valid"].all())
    assert np.array_equal(c["sol"].numpy(), c["rows"]["q"][R - 1])
    assert c["separable"].mean() >= 0.9 and c["named"].mean() >= 0.9
    assert c["band"].mean() <= X.BAND_CAP


@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("which", X.REDUNDANT)
def test_late_inputs_keep_half_of_the_poses(which, swapped):
    """n = 500, 3 steps: at least half of the poses are kept (early repeat valid at iteration 1, late repeat at 2 or 3, outside the band, rows
    apart) and on them the oracle's answer is the early repeat's row - repeat 0's, or the last repeat's when the seed blocks are swapped."""
    c = X.late_case(which, swapped=swapped)
    k = c["kept"]
    print(f"late {which}{' swapped' if swapped else ''}: kept {k.mean():.3f}; late repeat valid at iteration 1 / 2 / 3: "
          f"{[int(((c['rows']['steps'][c['late']] == s) & c['rows']['conv'][c['late']]).sum()) for s in (1, 2, 3)]}")
    assert c["early"] == (1 if swapped else 0)
    assert k.mean() >= 0.5
    assert np.array_equal(c["sol"].numpy()[k], c["rows"]["q"][c["early"]][k]) and bool(c["valid"][torch.from_numpy(k)].all())


@pytest.mark.parametrize("case", X.PARITY_CASES, ids=X.parity_id)
def test_parity_cases_have_both_outcomes_and_a_small_band(case):
    c = X.parity_case(case)
    share, nv, flips = float(c["band"].mean()), int(c["ref_valid"].sum()), X.parity_flips(case)
    print(f"parity {X.parity_id(case)}: band {share:.4f}, valid {nv}/{X.PARITY_N}, flags a one-ulp nudge flips {flips}")
    assert share <= X.BAND_CAP
    assert 0 < nv < X.PARITY_N
    assert flips == 0


def test_the_255_step_case_spans_the_byte():
    """Far poses never valid, the rest valid somewhere between iteration 1 and well past the 3 of every other test; the band is within the cap."""
    c = X.long_case()
    first, flips = X.long_case_conditions(c)
    print(f"255 steps {c['which']}: valid {int(c['valid'].sum())} of {int(c['pattern'].sum())} solvable, band {int(c['band'].sum())}, first valid iterations {sorted(set(first.ravel().tolist()))}")
    assert not c["valid"][torch.from_numpy(~c["pattern"])].any() and (first[:, ~c["pattern"]] == 0).all()
    assert first.max() > 16 and (first == 1).any() and 0 < int(c["valid"].sum())
    assert c["band"].mean() <= X.BAND_CAP and flips == 0


def test_layout_cases_on_the_oracle():
    """n = 1, R = 300 (test 5): the oracle solves the pose, outside the band, whatever the repeat."""
    for which in ("panda", "syn6p"):
        c = X.single_pose_case(which)
        print(f"one pose {which}: oracle valid {bool(c['valid'][0])}, band {bool(c['band'][0])}, valid repeats {int((c['first'] > 0).sum())} of {c['R']}")
        assert bool(c["valid"][0]) and not c["band"][0] and 0 < int((c["first"] > 0).sum()) < c["R"]
