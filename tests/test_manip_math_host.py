"""The arithmetic of the singularity rule (ikflow_amd/csrc/manip_math.h: the fp64 Jacobian, the Gram matrix of a part's rows, the Cholesky pivots,
the rule) compiled for the HOST with g++ and held against the singular-value reference of tests/manip_helpers.py - the kernel's own source,
checked without a GPU.  The GPU tests check the same code where it ships (tests/test_manip.py).  Also here, from the reference alone: every
(chain, seed, floor) the GPU gate tests use has next to no row in the band around its floor and enough on either side.
Test infrastructure: nothing in ikflow_amd/ loads it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import manip_helpers as MH
from test_kin_math_host import _chain_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("manip_math") / "libmanip_math_host.so"
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "manip_math_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(str(out))
    lib.kin_math_chain_bytes = lib.manip_host_chain_bytes   # (what _chain_bytes asks the library it packs for)
    lib.manip_host_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    assert [lib.manip_host_part(i) for i in range(3)] == [0, 1, 2]
    return lib


def _rows(lib, robot, q, part, floor=0.0):
    q = np.ascontiguousarray(q, np.float32)
    w, below = np.full(len(q), -1.0, np.float32), np.full(len(q), 7, np.uint8)
    assert lib.manip_host_rows(_chain_bytes(robot, lib), q.ctypes.data, len(q), MH.PARTS.index(part), floor, w.ctypes.data, below.ctypes.data) == 0
    return w, below


@pytest.mark.parametrize("which", MH.CHAINS)
def test_measure_against_the_singular_value_reference(host_lib, which):
    """manip_row on 2000 draws, all three parts: |kernel source - float32(w_ref)| <= MANIP_TOL_ABS against the reference over the chain's table,
    and at most one f32 ulp against the reference over the FOLDED chain the kernel reads - what is left when the inputs are the same (measured:
    0 on every chain; the table figure is 0 on the built-in robots, whose folded transforms are exact, and up to 4.77e-7 - two ulps of a w
    above 2 - on the synthetic chains, whose folded products are rounded).  With 4 and 5 joints FULL takes J^T J."""
    robot = H.kin_robots(which)[0]
    q = MH.draws(which)
    folded = MH.folded_rows(robot)
    for part in MH.PARTS:
        ref = MH.reference(which, part)
        w, below = _rows(host_lib, robot, q, part)
        assert np.isfinite(w).all() and (w > 0).all() and not below.any()   # (no floor: only a NaN row is below)
        d = np.abs(w.astype(np.float64) - ref.astype(np.float32))
        ref_f = MH.w_ref(folded, q, part).astype(np.float32)
        d_f = np.abs(w.astype(np.float64) - ref_f)
        print(f"manip {which} {part}: worst |host - f32(w_ref)| {d.max():.3e} (table), {d_f.max():.3e} (folded); w in {ref.min():.2e} .. {ref.max():.2e}")
        assert d.max() <= MH.MANIP_TOL_ABS, (which, part, d.max())
        assert (d_f <= np.spacing(ref_f)).all(), (which, part, d_f.max())
        assert np.abs(ref - np.median(ref)).max() > 100 * MH.MANIP_TOL_ABS   # (the draw spreads: a constant would not pass)


def test_the_rule_against_the_reference_on_every_gate_case(host_lib):
    """!(w >= floor) of the kernel source equals the reference's verdict on every row outside the band, for the floors of the GPU gate tests."""
    for which in MH.GATE_CASES:
        q, ref, floor, part = MH.gate_case(which)
        _, below = _rows(host_lib, H.kin_robots(which)[0], q, part, floor)
        want, decided = MH.below_ref(ref, floor)
        assert np.array_equal(below[decided], want[decided].astype(np.uint8)), which
        assert set(np.unique(below)) == {0, 1}


def test_known_answers_on_the_gantry(host_lib):
    """Three orthogonal prismatic joints and a revolute joint about z through the tool point: LINEAR exactly 1 (J J^T = I, the revolute column's
    linear part is zero), ANGULAR exactly 0 (a Gram matrix of rank 1: the first pivot is 0), FULL exactly 1 (J^T J = I) - wherever the gantry
    stands.  The reference agrees."""
    robot = MH.gantry()
    q = np.array([[0.0, 0.0, 0.0, 0.0], [0.3, -0.7, 0.25, 1.1], [-1.0, 1.0, 0.5, -2.9]], np.float32)
    for part, want in (("linear", 1.0), ("angular", 0.0), ("full", 1.0)):
        w, below = _rows(host_lib, robot, q, part, 0.5)
        assert w.dtype == np.float32 and (w == np.float32(want)).all(), (part, w)
        assert (below == (0 if want else 1)).all()
        assert np.abs(MH.w_ref(MH.table_rows(robot), q, part) - want).max() <= 1e-15


def test_a_nan_joint_gives_a_nan_measure_below_every_floor(host_lib):
    """NaN in any one joint - the first, a sliding one, the last, on which the angular rows do not depend - gives NaN for every part, and the row is
    below every floor, 0 included; its neighbours are untouched."""
    for which in ("panda", "fetch", "syn4p"):
        robot = H.kin_robots(which)[0]
        base = MH.draws(which)[:robot.ndof + 2].copy()
        q = base.copy()
        for j in range(robot.ndof):
            q[j, j] = np.nan
        for part in MH.PARTS:
            clean, _ = _rows(host_lib, robot, base, part)
            for floor in (0.0, 1e-30, 0.05, 3.0e38):
                w, below = _rows(host_lib, robot, q, part, floor)
                assert np.isnan(w[:robot.ndof]).all() and (below[:robot.ndof] == 1).all(), (which, part, floor)
                assert H.same_bits(w[robot.ndof:], clean[robot.ndof:])
                assert np.array_equal(below[robot.ndof:], (~(clean[robot.ndof:] >= np.float32(floor))).astype(np.uint8))
            assert np.isnan(MH.w_ref(MH.table_rows(robot), q, part)[:robot.ndof]).all()


def test_the_gate_cases_have_next_to_no_row_in_the_band_and_enough_on_either_side():
    """From the reference alone, for every (chain, seed, floor) of the GPU gate tests: at most 1 % of the rows within 8 x MANIP_TOL_ABS of the
    floor, at least 10 % surely below and 10 % surely above - also among the first rows, which the small shapes take."""
    assert MH.GATE_CASES["panda"][0] == 7
    for which in MH.GATE_CASES:
        q, ref, floor, part = MH.gate_case(which)
        band, below, above = MH.band_shares(ref, floor)
        print(f"gate case {which} {part}: floor {floor:.4f}, band {band:.4f}, below {below:.3f}, above {above:.3f}")
        assert band <= 0.01 and below >= 0.10 and above >= 0.10, (which, band, below, above)
        for rows in (65 * 16, 65 * 3, 5 * 16):
            b, lo, hi = MH.band_shares(ref[:rows], floor)
            assert b <= 0.01 and lo >= 0.10 and hi >= 0.10, (which, rows, b, lo, hi)
    assert abs(MH.gate_case("panda")[2] - 0.031) < 5e-4
