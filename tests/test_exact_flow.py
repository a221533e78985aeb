"""ikf_generate_exact - the flow, the ordered compaction and the LM rounds in one call (run_exact, ikflow_amd/csrc/api_kin.hip) - against its own
parts, bit for bit.

Each part has a strict suite: the flow under the tiling pose source d_poses + 7 * d_idx[r % n_mod] (tests/test_flow_sample_tiled.py: every form,
bit for bit and against fp64) and the round kernels with the flow taken out (tests/test_exact_rounds.py: lists element for element, every row
against the oracle).  What joins them - which list, which modulus, how many rows, which round's latents, seeds read from the buffer the LM launch
also writes (d_q_seed == ex_q in the flow path only) - was held to 95 % / 97 % agreement with the oracle (tests/test_gpu_parity.py), because LM
amplifies the 1e-6 between the flow and ITS oracle.  Here no oracle runs and nothing is amplified: the one call must have the bits of
exact_helpers.parts - ikf_generate_approx_tiled on the predicted list, then ikf_generate_exact_seeded on those seeds.  No band, no share of rows
left out.

1. the one call equals its parts under the default plan (row-owner, cluster, seams inside a retry round);  2. the same under forced forms;
3. prefixes of the schedule;  4. the callback's contract;  5. output windows and a side stream;  6. row state that grows between rounds;
7. the default draw;  8. the Python wrappers.
What the inputs must satisfy for this to reach every round (strict sub-lists, row counts beyond the chunk sizes): tests/test_exact_flow_inputs.py."""
import functools

import numpy as np
import pytest
import torch

import exact_helpers as X
import sample_helpers as sh
from sample_helpers import DEV, force
from test_flow_sample import _eng, _no_cluster_repair

pytestmark = pytest.mark.gpu
GUARD = 64
NAN_BITS = 0x7FC00000
STEPS = X.FLOW_STEPS


@functools.lru_cache(maxsize=None)
def _case(case):
    """(model name, poses [n x 7], latents per round, schedule, pos_thr, rot_thr) of exact_helpers.FLOW_CASES on the device; never written to."""
    name, poses, lats, rc, pos_thr, rot_thr = X.flow_case_inputs(case)
    return name, poses.to(DEV).contiguous(), tuple(l.to(DEV).contiguous() for l in lats), rc, pos_thr, rot_thr


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same(one, two, label):
    """sol as int32, valid, and all four columns of the stats."""
    (sol, valid, stats), (psol, pvalid, pstats) = one[:3], two[:3]
    assert sol.shape == psol.shape and valid.shape == pvalid.shape and valid.dtype == pvalid.dtype == torch.uint8
    diff = (_bits(sol) != _bits(psol)).any(1)
    assert not bool(diff.any()), f"{label}: rows {diff.nonzero().flatten()[:8].tolist()} of {int(diff.sum())} differ from the parts"
    assert torch.equal(valid, pvalid), f"{label}: flags of poses {(valid != pvalid).nonzero().flatten()[:8].tolist()} differ from the parts"
    assert np.array_equal(stats, pstats), (label, stats.tolist(), pstats.tolist())


def _both(eng, case, rc=None):
    """The one call and the parts of a case -> ((sol, valid, stats, calls), (sol, valid, stats, lists)), compared."""
    name, P, lats, full_rc, pos_thr, rot_thr = _case(case)
    rc = full_rc if rc is None else rc
    one = X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, STEPS, lats)
    two = X.parts(eng, P, rc, pos_thr, rot_thr, STEPS, lats)
    _assert_same(one, two, case)
    lists = two[3]
    assert one[3] == [(r, len(lists[r]) * rc[r], eng.layout.dim) for r in range(len(lists))], (case, one[3], [len(l) for l in lists])
    valid, sol = one[1].bool(), one[0]
    assert int(valid.sum()) == int(one[2][:, 3].sum()) and not bool(_bits(sol[~valid]).any()), case
    return one, two


def _plans(eng, calls):
    return [eng.plan(rows) for _, rows, _ in calls]


def _strict_sub_lists(stats, label):
    """From the engine's own stats: every round ran, on a list that is non-empty and strictly shorter than the one before."""
    active = stats[:, 0].tolist()
    assert all(a > 0 for a in active) and all(b < a for a, b in zip(active, active[1:])), (label, active)


# ---- 1. one call equals its parts ------------------------------------------------------------------------------------------------------------------
_DEFAULT = ("R-1", "R-17", "R-200", "R-450-tight", "R-130-r2", "R10-17", "R10-200", "R8-17", "R8-200", "Rsig-17", "Rsig-200", "T-17", "T-200",
            "T-1800-tight")
_R_CASES = tuple(c for c in _DEFAULT if c.startswith("R-"))


@pytest.mark.parametrize("case", _DEFAULT)
def test_one_call_has_the_bits_of_its_parts(case):
    eng = _eng(X.FLOW_CASES[case][0])
    with _no_cluster_repair(eng):
        one, two = _both(eng, case)
    print(f"[exact+flow] {case}: active {one[2][:, 0].tolist()}, rows {one[2][:, 1].tolist()}, solved {one[2][:, 3].tolist()}, plans {_plans(eng, one[3])}")
    if case in X.FLOW_N200:
        assert len(one[3]) == 3
        _strict_sub_lists(one[2], case)


def test_the_default_plans_of_the_r_cases_reach_the_row_owner_form_a_cluster_form_and_a_seam_inside_a_retry_round():
    """The plans the rounds of test_one_call_has_the_bits_of_its_parts ran under, from the engine's own row counts."""
    eng = _eng("R")
    forms, seams = set(), []
    for case in _R_CASES:
        name, P, lats, rc, pos_thr, rot_thr = _case(case)
        calls = X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, STEPS, lats)[3]
        for (r, rows, _), plan in zip(calls, _plans(eng, calls)):
            chunks = sh.parse_plan(plan)
            assert sum(c[2] for c in chunks) == rows
            forms |= {sh.form_class(c[0]) for c in chunks}
            if r > 0 and len({c[0] for c in chunks}) > 1:
                seams.append((case, r, plan))
    print(f"[exact+flow] forms {sorted(forms)}, seams inside a retry round {seams}")
    assert "rowowner" in forms and "cluster" in forms and seams, (forms, seams)


# ---- 2. the same under forced forms -----------------------------------------------------------------------------------------------------------------
_FORCED = (("R-200", ("rowowner",), "rowowner"), ("R-200", ("cluster",), "cluster"), ("R-200", ("cluster-epoch",), "cluster"),
           ("R-200", ("cluster-spread",), "cluster"), ("R-200", ("perlayer",), "perlayer"), ("R-200", ("f16x3", "perlayer"), "perlayer"),
           ("R10-200", ("rowowner",), "rowowner"), ("T-200", ("unfused4",), "perlayer"), ("T-200", ("f16x3",), "perlayer"))


@pytest.mark.parametrize("case,forms,want", _FORCED, ids=lambda v: "+".join(v) if isinstance(v, tuple) else v)
def test_one_call_has_the_bits_of_its_parts_under_a_forced_form(case, forms, want):
    """The form is in force for the one call and for the parts alike; every round's rows run under one chunk of it."""
    eng = _eng(X.FLOW_CASES[case][0])
    fallbacks = eng.split_fallback_count
    with _no_cluster_repair(eng), force(eng, *forms):
        if "f16x3" in forms:
            assert eng.precision == "f16x3"
        one, two = _both(eng, case)
        plans = _plans(eng, one[3])
    print(f"[exact+flow] {case} {'+'.join(forms)}: active {one[2][:, 0].tolist()}, plans {plans}")
    assert len(plans) == 3 and all(len(p.split()) == 1 and p.startswith(want) for p in plans), plans
    _strict_sub_lists(one[2], case)
    assert eng.split_fallback_count == fallbacks, "an f16x3 call was re-run in f32: not an f16x3 result"
    assert eng.precision == "f32"


# ---- 3. prefixes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["R-200", "T-200"])
def test_a_shorter_schedule_is_a_prefix_of_the_longer_one(case):
    eng = _eng(X.FLOW_CASES[case][0])
    rc = X.FLOW_CASES[case][2]
    with _no_cluster_repair(eng):
        runs = [_both(eng, case, rc[:k])[0] for k in (1, 2, 3)]
    for short, long in zip(runs, runs[1:]):
        k = len(short[2])
        assert np.array_equal(long[2][:k], short[2]), (case, long[2].tolist(), short[2].tolist())
        assert long[3][:k] == short[3] and len(long[3]) == k + 1
        solved = short[1].bool()
        assert bool(solved.any()) and bool(long[1].bool()[solved].all()), case                 # a pose solved in round r keeps its flag ...
        assert torch.equal(_bits(long[0][solved]), _bits(short[0][solved])), case               # ... and its row
        assert int(long[1].sum()) > int(short[1].sum())


# ---- 4. the callback's contract ---------------------------------------------------------------------------------------------------------------------
def test_all_solved_in_round_0_asks_for_one_rounds_latents_and_zeroes_the_other_stats_rows():
    name, P, lats, rc, pos_thr, rot_thr = _case("T-200-all")
    eng, n = _eng(name), 200
    sol, valid, stats, calls = X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, STEPS, lats, stats_fill=-1)
    assert calls == [(0, n, eng.layout.dim)]
    assert stats.tolist() == [[n, n, 3 * n, n], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert bool((valid == 1).all())
    _assert_same((sol, valid, stats), X.parts(eng, P, rc, pos_thr, rot_thr, STEPS, lats), "T-200-all")


def test_nothing_solvable_runs_every_round_on_every_pose():
    name, P, lats, rc, pos_thr, rot_thr = _case("T-200-none")
    eng, n = _eng(name), 200
    sol, valid, stats, calls = X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, STEPS, lats, stats_fill=-1)
    assert calls == [(r, n * rc[r], eng.layout.dim) for r in range(3)]
    assert not bool(_bits(sol).any()) and not bool(valid.any())                                # + 0.0, bit for bit
    assert stats.tolist() == [[n, n * R, 3 * n * R, 0] for R in rc]
    _assert_same((sol, valid, stats), X.parts(eng, P, rc, pos_thr, rot_thr, STEPS, lats), "T-200-none")


@pytest.mark.parametrize("case", ["R-200", "T-200"])
def test_longer_and_shifted_latent_buffers_give_the_same_bits(case):
    """Every round's latents followed by 33 rows of NaN, in a buffer that starts 4 bytes past a 256-byte boundary: only the first rows of the round
    are read, and nothing assumes more than the alignment of a float."""
    name, P, lats, rc, pos_thr, rot_thr = _case(case)
    eng, D = _eng(name), _eng(name).layout.dim
    want = X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, STEPS, lats)
    moved = []
    for lt in lats:
        rows = lt.shape[0] + 33
        buf = torch.full((rows * D + 64,), float("nan"), dtype=torch.float32, device=DEV)
        off = ((4 - buf.data_ptr()) % 256) // 4
        view = buf[off: off + rows * D].view(rows, D)
        view[:lt.shape[0]] = lt
        assert view.data_ptr() % 256 == 4 and view.is_contiguous() and bool(torch.isnan(view[lt.shape[0]:]).all())
        moved.append(view)
    got = X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, STEPS, moved)
    _assert_same(got, want, case)
    assert got[3] == want[3]
    _strict_sub_lists(got[2], case)      # (so the rounds read well short of the rows they were given: the NaN rows would be seeds)


# ---- 5. output windows and a side stream ---------------------------------------------------------------------------------------------------------------
def _windows(n, ndof):
    q = torch.full(((GUARD + n + GUARD) * ndof,), NAN_BITS, dtype=torch.int32, device=DEV)
    v = torch.full((GUARD + n + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    return q, v, q[GUARD * ndof:(GUARD + n) * ndof].view(torch.float32).view(n, ndof), v[GUARD:GUARD + n]


def _check_windows(q, v, sol, valid, n, ndof, label):
    assert not bool((q[:GUARD * ndof] != NAN_BITS).any()) and not bool((q[(GUARD + n) * ndof:] != NAN_BITS).any()), f"{label}: a guard row of sol was written"
    assert not bool((v[:GUARD] != 0xAB).any()) and not bool((v[GUARD + n:] != 0xAB).any()), f"{label}: a guard entry of valid was written"
    assert not bool((_bits(sol) == NAN_BITS).any()), f"{label}: an element of sol was never written"
    assert bool((valid <= 1).all()), f"{label}: valid outside {{0, 1}}"
    assert not bool(_bits(sol[valid == 0]).any()), f"{label}: an unsolved row is not zero"


@pytest.mark.parametrize("case,side", [("R-200", False), ("R10-17", True)])
def test_the_outputs_stay_inside_their_windows(case, side):
    """64 guard rows of NaN bits (0xAB bytes) in front of and behind sol (valid); R10-17 on a stream of its own."""
    name, P, lats, rc, pos_thr, rot_thr = _case(case)
    eng, n, ndof = _eng(name), P.shape[0], _eng(name).layout.ndof
    want = X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, STEPS, lats)
    q, v, sol, valid = _windows(n, ndof)
    with _no_cluster_repair(eng):
        if side:
            stream = torch.cuda.Stream(device=DEV)
            stream.wait_stream(torch.cuda.current_stream(DEV))          # (the fills above ran on the current stream)
            with torch.cuda.stream(stream):
                got = X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, STEPS, lats, sol=sol, valid=valid)
            stream.synchronize()
        else:
            got = X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, STEPS, lats, sol=sol, valid=valid)
    torch.cuda.synchronize()
    _check_windows(q, v, sol, valid, n, ndof, case)
    _assert_same(got, want, case)
    assert got[3] == want[3] and 0 < int(valid.sum()) < n


# ---- 6. row state that grows between rounds -----------------------------------------------------------------------------------------------------------
def test_row_state_that_grows_between_the_rounds_gives_the_same_bits():
    """A fresh handle on R's weights that never sizes for the worst case (ikf_set_exact_upfront_rows 0) and has no reservation re-allocates ex_q -
    the buffer the flow writes and the LM launch reads and writes - before rounds 1 and 2; the shared handle has everything reserved."""
    name, P, lats, rc, pos_thr, rot_thr = _case("R-200")
    shared = _eng(name)
    shared.reserve_exact(P.shape[0], max(rc))
    want = X.run_flow_raw(shared, P, rc, pos_thr, rot_thr, STEPS, lats)
    fresh = sh.new_solver(sh.model(name)).engine(DEV)
    assert fresh is not shared
    fresh.set_exact_upfront_rows(0)
    got = X.run_flow_raw(fresh, P, rc, pos_thr, rot_thr, STEPS, lats)
    _assert_same(got, want, "R-200 (growing row state)")
    assert got[3] == want[3]
    rows = got[2][:, 1].tolist()
    assert rows[0] < rows[1] < rows[2], rows


# ---- 7. the default draw --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,seed", [("R-200", 1234), ("T-17", 77)])
def test_the_default_draw_is_one_randn_per_round_of_exactly_the_rounds_rows(case, seed):
    """Engine.generate_exact(latents=None) after torch.manual_seed(s) against the parts on torch.randn((rows_r, D)) drawn round by round after the
    same seed, rows_r coming from the previous prefix.  (Poses and thresholds of the case; its stored latents are not used.  Other N(0, 1) latents
    solve other poses, but that round 0 solves all of them has no chance: at these thresholds the pool's latents leave 193 of 200 and 16 of 17.)"""
    name, P, _, rc, pos_thr, rot_thr = _case(case)
    eng, D = _eng(name), _eng(name).layout.dim
    drawn = []

    def draw(r, rows):
        assert r == len(drawn)
        drawn.append(torch.randn((rows, D), device=DEV))
        return drawn[-1]

    with _no_cluster_repair(eng):
        torch.manual_seed(seed)
        psol, pvalid, pstats, lists = X.parts(eng, P, rc, pos_thr, rot_thr, STEPS, draw)
        torch.manual_seed(seed)
        sol, valid, stats = eng.generate_exact(P, rc, pos_thr, rot_thr, latents=None, n_lm_steps=STEPS, return_stats=True)
    assert valid.dtype == torch.bool
    _assert_same((sol, valid.to(torch.uint8), stats), (psol, pvalid, pstats), f"{case} default draw")
    assert len(lists) == 3 and [d.shape[0] for d in drawn] == stats[:, 1].tolist()
    # the parts on the drawn tensors handed in as latents: the same again through the raw call
    _assert_same(X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, STEPS, drawn), (psol, pvalid, pstats), f"{case} drawn latents")


# ---- 8. the wrappers ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["T-200", "R-17"])
def test_the_python_wrappers_return_the_raw_calls_bits(case):
    """The wrappers are handed every round's latents in a buffer of n * max(rc) rows (the case's rows first): a wrapper that handed out another
    round's buffer would pass its own size check and show in the bits alone."""
    name, P, exact, rc, pos_thr, rot_thr = _case(case)
    eng, n = _eng(name), P.shape[0]
    pool = sh.device_inputs(name)[0]
    lats = [pool[X.LATENT_STRIDE * i: X.LATENT_STRIDE * i + n * max(rc)] for i in range(len(rc))]
    assert all(l.shape[0] == n * max(rc) and torch.equal(l[:e.shape[0]], e) for l, e in zip(lats, exact))
    sol, valid, stats, _ = X.run_flow_raw(eng, P, rc, pos_thr, rot_thr, STEPS, exact)
    esol, evalid, estats = eng.generate_exact(P, rc, pos_thr, rot_thr, latents=list(lats), n_lm_steps=STEPS, return_stats=True)
    assert evalid.dtype == torch.bool
    _assert_same((esol, evalid.to(torch.uint8), estats), (sol, valid, stats), f"{case} Engine.generate_exact")
    ssol, svalid = sh.shared_solver(name).generate_exact_ik_solutions(P, repeat_counts=tuple(rc), pos_error_threshold=pos_thr,
                                                                      rot_error_threshold=rot_thr, latents=list(lats))
    assert svalid.dtype == torch.bool and torch.equal(_bits(ssol), _bits(sol)) and torch.equal(svalid, valid.bool()), case
