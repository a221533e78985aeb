"""The arithmetic of the path optimiser (ikflow_amd/csrc/path_opt_math.h: residual, normal blocks, the block Cholesky recurrence, the objective,
the monotone loop, the evaluator's cost fold) compiled for the HOST with g++ -O2 -ffp-contract=off and held against an independent dense fp64
solve, the fp64 LM step, and the lattice's sequential float32 arithmetic - the kernels' own source, checked without a GPU.  The GPU tests check
the same code where it ships (tests/test_path_opt.py).  Test infrastructure: nothing in ikflow_amd/ loads it."""
import numpy as np
import pytest
import torch

import helpers as H
import path_helpers as PH
import path_opt_helpers as PO
from oracle import kinematics_oracle as ko

F = np.float32
TS = (1, 2, 3, 33)
WS = (0.0, 1e-3, 0.1, 10.0)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return PO.host_lib(tmp_path_factory.mktemp("path_opt_math"))


@pytest.mark.parametrize("which", PO.CHAINS)
def test_chain_kinematics_is_the_oracles_up_to_the_f32_constants(which):
    """The reference's kinematics (PO.chain_kinematics: the engine's f32 constants walked in fp64 numpy) against oracle.kinematics_oracle.jacobian
    and pose_error_vector on the oracle's own fp64 chain.  Bound: every constant is off by at most 2^-24 relative; a chain of at most 9 transforms
    (8 joints and the tool), each rotation entry off by 6e-8 acting over a reach of at most 2 m (three entries per row) plus 6e-8 x 0.5 m of its
    own offset: 9 x (3.6e-7 + 3e-8) = 3.5e-6 in position, the same in a Jacobian column and in the rotation error."""
    robot, orob, wp, Q0, _ = PO.make_case(which, 33, 2, False)
    Jc, ec = PO.jacobian_and_error(robot, orob, wp, Q0, "chain")
    Jo, eo = PO.jacobian_and_error(robot, orob, wp, Q0, "oracle")
    print(f"{which}: max |J - J_oracle| {np.abs(Jc - Jo).max():.2e}, max |e - e_oracle| {np.abs(ec - eo).max():.2e}")
    assert np.abs(Jc - Jo).max() <= PO.KIN_EPS and np.abs(ec - eo).max() <= PO.KIN_EPS


@pytest.mark.parametrize("with_start", [False, True])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("which", PO.CHAINS)
def test_one_step_against_the_dense_fp64_solve(lib, which, T, with_start):
    """One step of the header against the dense (T ndof)^2 solve on the engine's own chain constants: every entry within ONE f32 spacing; and
    against the same solve on the oracle's jacobian and pose_error_vector: within the perturbation bound of PO.oracle_step_bound (the oracle's
    chain is fp64, the engine's f32: two slightly different systems) plus one spacing.  Two fp64 evaluations differ by about
    cond(H) 2^-53 relative, and cond(H) <= (|J|^2 + 4 w + lambda) / lambda stays below 1e7 for w <= 10 (asserted), so they round to the same or the
    adjacent f32.  Measured here: 0 spacings in every case.  Also: the step lowers F by more than half (the GPU test's accept decisions hang on
    no last bit)."""
    robot, orob, wp, Q0, qs = PO.make_case(which, T, 1, with_start)
    ch = PO.chain_bytes(robot, lib)
    worst = 0.0
    for w in WS:
        got, iters, Fv = PO.host_optimise(lib, ch, robot.ndof, wp, Q0, qs, w, 1)
        want, cond = PO.reference_step(robot, orob, wp, Q0, qs, w)
        assert cond < 1e7, (which, T, w, cond)
        f0, f1 = PO.objective_f64(robot, orob, wp, Q0, qs, w), PO.objective_f64(robot, orob, wp, want, qs, w)
        assert f1 / f0 < 0.5, (which, T, w, f1 / f0)
        assert iters == 1 and abs(Fv[0] - f0) <= 1e-12 * f0 and abs(Fv[1] - f1) <= 1e-9 * f0
        apart = PO.spacings_apart(got, want)
        assert apart <= 1.0, (which, T, with_start, w, apart)
        # ... and the ORACLE's own step (its jacobian and pose_error_vector on its fp64 chain), as close as the f32 constants provably allow
        d_or, bound = PO.oracle_step_bound(robot, orob, wp, Q0, qs, w)
        lo, hi = PO._limits(robot)
        want_or = np.clip(Q0.astype(np.float64) + d_or, lo, hi)
        off = np.abs(got.astype(np.float64) - want_or).max()
        worst = max(worst, off / bound)
        assert off <= bound + float(np.spacing(np.abs(got).max())), (which, T, with_start, w, off, bound)
    print(f"{which} T = {T}: the header's step is at most {worst:.3f} of the perturbation bound from the oracle's")


@pytest.mark.parametrize("which", PO.CHAINS)
def test_without_smoothing_a_step_is_the_fp64_lm_step_of_every_row(lib, which):
    """w = 0, one step: each row within one f32 spacing of the host build of lm_step_row<NDOF, double> (kin_math.h) - the same expressions, so in
    fact the same bits - with and without q_start, which w = 0 must ignore."""
    for T in TS:
        robot, orob, wp, Q0, qs = PO.make_case(which, T, 3, True)
        ch = PO.chain_bytes(robot, lib)
        lm = np.ascontiguousarray(Q0.copy())
        assert lib.po_host_lm(ch, np.ascontiguousarray(wp, F).ctypes.data, lm.ctypes.data, T) == 0
        for start in (None, qs):
            got, iters, _ = PO.host_optimise(lib, ch, robot.ndof, wp, Q0, start, 0.0, 1)
            assert iters == 1 and PO.spacings_apart(got, lm) <= 1.0, (which, T)


STOPS_EARLY = {("syn8r", 33, 4, False, 10.0): (1, 1),    # the second step overshoots (no adaptive damping): F 17.8 -> 1.02 -> 2.66, one step kept
               ("fetch", 3, 5, False, 10.0): (1, 3)}     # the issue's case: fetch, T = 3, seed 5 stops after 1 .. 3 steps (here: F 0.894 -> 0.241 -> 0.104 -> 0.139)


@pytest.mark.parametrize("case", [("panda", 33, 1, True, 0.1), ("fetch", 3, 5, False, 1e-3), ("syn6r", 2, 2, True, 10.0), ("syn5p", 1, 0, False, 0.0)]
                         + list(STOPS_EARLY))
def test_the_loop_keeps_only_steps_that_lower_the_objective(lib, case):
    """16 iterations.  The header's own F values of the kept steps strictly decrease, the first one it did not keep does not.  Recomputed by the
    ORACLE in fp64 (its pose_error_vector on its own chain) every kept value is below its predecessor by more than minus the tolerance the two
    chains' constants leave between the oracle's F and the header's (PO.objective_tolerance: derived from the 3.5e-6 bound on e, of both values) -
    and strictly below wherever the header's own decrease exceeds that tolerance.  The pinned cases stop early.  The returned iterate is the last
    kept one, bit for bit: n_iters = iters returns the same path."""
    which, T, seed, with_start, w = case
    robot, orob, wp, Q0, qs = PO.make_case(which, T, seed, with_start)
    ch = PO.chain_bytes(robot, lib)
    got, iters, Fv = PO.host_optimise(lib, ch, robot.ndof, wp, Q0, qs, w, 16)
    assert iters >= 1 and all(Fv[i + 1] < Fv[i] for i in range(iters))
    if iters < 16:
        assert not Fv[iters + 1] < Fv[iters] and np.isnan(Fv[iters + 2:]).all()
    if case in STOPS_EARLY:
        assert STOPS_EARLY[case][0] <= iters <= STOPS_EARLY[case][1] and iters < 16
    prev = Q0
    f_prev, tol_prev = PO.objective_f64(robot, orob, wp, Q0, qs, w, "oracle"), PO.objective_tolerance(robot, orob, wp, Q0)
    assert abs(f_prev - Fv[0]) <= tol_prev
    for i in range(1, iters + 1):
        step, kept, _ = PO.host_optimise(lib, ch, robot.ndof, wp, prev, qs, w, 1)
        assert kept == 1
        f, tol = PO.objective_f64(robot, orob, wp, step, qs, w, "oracle"), PO.objective_tolerance(robot, orob, wp, step)
        assert abs(f - Fv[i]) <= tol, (case, i, f, Fv[i], tol)                 # the oracle's F is the header's, up to the constants
        assert f < f_prev + tol + tol_prev, (case, i, f, f_prev)
        if Fv[i - 1] - Fv[i] > tol + tol_prev:
            assert f < f_prev, (case, i, f, f_prev)
        prev, f_prev, tol_prev = step, f, tol
    assert H.same_bits(prev, got)                                             # the chain of single steps ends where the loop ended
    assert H.same_bits(PO.host_optimise(lib, ch, robot.ndof, wp, Q0, qs, w, iters)[0], got)
    if iters < 16:                                                            # ... and one more step from there is refused: the input comes back
        again, kept, _ = PO.host_optimise(lib, ch, robot.ndof, wp, got, qs, w, 1)
        assert kept == 0 and H.same_bits(again, got)


def test_a_nan_row_ends_the_loop_at_once(lib):
    robot, orob, wp, Q0, qs = PO.make_case("panda", 3, 0, True)
    ch = PO.chain_bytes(robot, lib)
    bad = Q0.copy()
    bad[1, 2] = np.nan
    for w in (0.0, 0.1):
        got, iters, Fv = PO.host_optimise(lib, ch, 7, wp, bad, qs, w, 4)
        assert iters == 0 and np.isnan(Fv[0]) and H.same_bits(got, bad)


# ---- the evaluator's fold against the lattice's sequential float32 arithmetic ---------------------------------------------------------------
def _chosen(T, k, nd, seed, q_start, nw=1.0, step=None, holes=False):
    q, node = PH.random_lattice(T, k, nd, seed)
    if holes:
        node = node.copy()
        node[np.random.default_rng(seed).random(node.shape) < 0.2] = PH.INF
    path, index, cost, _ = PH.dp_f32(q, node, T, k, q_start, nw, step)
    return path, index, cost, node.reshape(k, T)


@pytest.mark.parametrize("nd", [4, 5, 6, 7, 8])
def test_the_fold_of_a_lattice_path_is_the_lattices_cost_bit_for_bit(lib, nd):
    """path_helpers.dp_f32's chosen path through path_opt_cost: the same f32 bits - with and without q_start, under the step gate, with holes in
    the lattice, with node_weight 0 / 1 / 50."""
    n = 0
    for T, k in ((1, 1), (2, 5), (9, 7), (65, 8)):
        for seed in range(3):
            qs = None if seed % 2 else np.random.default_rng(seed).normal(0, 0.3, nd).astype(F)
            for nw in (0.0, 1.0, 50.0):
                for step, holes in ((None, False), (0.9, False), (None, True), (1.2, True)):
                    path, index, cost, node = _chosen(T, k, nd, 10 * T + seed, qs, nw, step, holes)
                    if not cost < PH.INF:
                        continue
                    got, reason, where = PO.host_cost(lib, path, node[index, np.arange(T)], qs, None, nw, step)
                    assert H.same_bits(F(got), F(cost)) and (reason, where) == (0, -1), (T, k, seed, nw, step, holes)
                    n += 1
    assert n >= 100


def test_the_fold_names_the_first_offence(lib):
    T, k, nd = 9, 4, 7
    qs = np.random.default_rng(3).normal(0, 0.3, nd).astype(F)
    path, index, cost, node = _chosen(T, k, nd, 5, qs)
    node = node[index, np.arange(T)].copy()
    free = np.ones(T, np.uint64)
    assert H.same_bits(PO.host_cost(lib, path, node, qs, free)[0], F(cost))
    for t in (0, 4, 8):
        bad = node.copy()
        bad[t] = PH.INF
        assert PO.host_cost(lib, path, bad, qs) == (PH.INF, 2, t)
        bad[t] = np.nan
        assert PO.host_cost(lib, path, bad, qs) == (PH.INF, 2, t)
        swept = free.copy()
        swept[t] = 2                                      # (bit 0 clear; the other bits are not read)
        assert PO.host_cost(lib, path, node, qs, swept) == (PH.INF, 3, t)
    assert PO.host_cost(lib, path, node, None, np.zeros(T, np.uint64) + np.uint64(np.arange(T) > 0))[1:] == (0, -1)   # no q_start: no start edge to sweep
    jump = path.copy()
    jump[5:, 2] += 3.0                                    # edge 4 -> 5 moves joint 2 by 3 rad
    assert PO.host_cost(lib, jump, node, qs, None, 1.0, 1.5) == (PH.INF, 3, 5)
    assert PO.host_cost(lib, jump, node, qs, None, 1.0, None)[1:] == (0, -1)
    far = path.copy()
    far[:] += 3.0                                         # ... and the start edge under the gate
    assert PO.host_cost(lib, far, node, qs, None, 1.0, 1.5) == (PH.INF, 3, 0)
    both = node.copy()
    both[6] = PH.INF                                      # the first offence wins: the edge into 5 before the node at 6
    assert PO.host_cost(lib, jump, both, qs, None, 1.0, 1.5) == (PH.INF, 3, 5)


def test_scratch_sizes(lib):
    for nd in range(4, 9):
        assert lib.po_host_wp_doubles(nd) == nd * nd + 2 * nd + 1
        assert lib.po_host_scratch_doubles(3, 65, nd) == 3 * 65 * (nd * nd + 2 * nd + 1)
    assert lib.po_host_scratch_doubles(2 ** 20, 2 ** 11, 8) == 2 ** 31 * 81   # (no 32-bit product)
