"""Singularity rule: the fp64 reference of a manipulability measure, the chains, draws and floors shared by the host build of
ikflow_amd/csrc/manip_math.h (tests/test_manip_math_host.py) and the GPU tests (tests/test_manip.py).

The reference shares no code with the kernel and imports nothing from oracle/: it walks Robot.chain_table() as given - every joint of the chain,
fixed ones included, the f32 table values widened to fp64; kinds 0 fixed, 1 revolute, 2 prismatic -, keeps the actuated columns of the geometric
Jacobian (rows 0-2 angular, 3-5 linear) and takes w_ref = the product of the p = min(rows, ndof) singular values of the part's rows from
numpy.linalg.svd.  The kernel factorises a Gram matrix instead.

MANIP_TOL_ABS is MEASURED, not chosen: the maximum of |host build of manip_math.h - float32(w_ref)| over every chain of CHAINS, all three parts
and the 2000 draws each of tests/test_manip_math_host.py, on the CPU (that test prints the figure per chain and part and asserts it): 4.77e-7,
on syn6p LINEAR, two f32 ulps of a w above 2; 0 on Panda, FetchArm and Fetch.  None of it is the factorisation: the kernel reads the FOLDED chain
(engine.fold_chain: the fixed transforms in front of an actuated joint multiplied in fp64, the product rounded to f32) while the reference walks
the table's f32 transforms one by one - inputs that differ by an f32 rounding per folded joint on the chains whose folded products are not
exact (the synthetic ones).  Taken over the folded chain (folded_rows) the reference gives the host build's f32 result bit for bit on every one of
the 54000 rows, which the same test asserts to one ulp.
The GPU gets 4 x MANIP_TOL_ABS (the device's fp64 sincos and its contraction choices are not the host's) plus one f32 ulp of w_ref."""
import numpy as np

import helpers as H

PARTS = ("full", "linear", "angular")
PART_ROWS = {"full": slice(0, 6), "linear": slice(3, 6), "angular": slice(0, 3)}
# Panda (7), FetchArm (7), Fetch (8, a prismatic joint) and the synthetic chains of 4, 5 and 6 joints, all-revolute and with prismatic joints
CHAINS = ("panda", "fetch_arm", "fetch", "syn4r", "syn4p", "syn5r", "syn5p", "syn6r", "syn6p")
N_DRAWS = 2000
MANIP_TOL_ABS = 4.8e-7          # measured: see the module docstring and test_measure_against_the_singular_value_reference
BAND = 8 * MANIP_TOL_ABS        # around a floor: the rule is not compared there
# The GPU gate tests: (chain) -> (seed of the draw, part); the floor is the median of the draw's reference.  Seeds: the first of 7, 8, .. under
# which, from the reference alone, at most 1 % of the rows lie in the band and at least 10 % on either side (asserted on the CPU).
GATE_ROWS = 65 * 64
GATE_CASES = {"panda": (7, "full"), "fetch": (7, "linear"), "syn4r": (7, "angular")}
_REF, _DRAW = {}, {}


def table_rows(robot):
    """The chain as the reference reads it: Robot.chain_table(), [joints x 16] float32."""
    return robot.chain_table()


def folded_rows(robot):
    """The chain as the KERNEL reads it (engine.fold_chain through f32), in the table's row format, the tool as a last fixed row: only to tell the
    error of the arithmetic from that of the folding."""
    from ikflow_amd.engine import fold_chain

    joints, tool = fold_chain(robot)
    rows = np.zeros((len(joints) + 1, 16), np.float32)
    for i, (kind, ax, pre) in enumerate(joints):
        rows[i, 0], rows[i, 1:4], rows[i, 4:] = kind, ax, np.asarray(pre).reshape(-1)
    rows[-1, 4:] = np.asarray(tool).reshape(-1)
    return rows


def jacobian(table, q):
    """fp64 geometric Jacobian of the rows of q [n x ndof] -> [n x 6 x ndof]; a NaN joint makes its row NaN throughout."""
    table = np.asarray(table, np.float64)
    q = np.asarray(q, np.float64)
    n = q.shape[0]
    R = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
    p = np.zeros((n, 3))
    axes, origins, kinds = [], [], []
    a = 0
    for row in table:
        kind, ax, F = int(row[0]), row[1:4], row[4:].reshape(3, 4)
        p = p + R @ F[:, 3]
        R = R @ F[:, :3]
        if kind == 0:
            continue
        axis_w = R @ ax
        axes.append(axis_w)
        origins.append(p.copy())
        kinds.append(kind)
        qa = q[:, a]
        a += 1
        if kind == 1:
            K = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
            # Rodrigues in the form cos I + sin [a]x + (1 - cos) a a^T: the table's f32 axis is a unit vector only to f32 rounding, and for such
            # an axis the form with [a]x^2 is another matrix (by (1 - cos)(1 - |a|^2), some 1e-7)
            c, s = np.cos(qa)[:, None, None], np.sin(qa)[:, None, None]
            M = c * np.eye(3) + s * K + (1.0 - c) * np.outer(ax, ax)
            R = R @ M
        else:
            p = p + axis_w * qa[:, None]
    assert a == q.shape[1], (a, q.shape)
    J = np.zeros((n, 6, a))
    for j, (axis_w, org, kind) in enumerate(zip(axes, origins, kinds)):
        if kind == 1:
            J[:, :3, j] = axis_w
            J[:, 3:, j] = np.cross(axis_w, p - org)
        else:
            J[:, 3:, j] = axis_w
    J[np.isnan(q).any(1)] = np.nan
    return J


def w_ref(table, q, part):
    """The product of the min(rows, ndof) singular values of the part's rows of the Jacobian, fp64 -> [n]; NaN for a row with a NaN joint."""
    J = jacobian(table, q)[:, PART_ROWS[part], :]
    out = np.full(J.shape[0], np.nan)
    ok = ~np.isnan(J).any((1, 2))
    if ok.any():
        out[ok] = np.linalg.svd(J[ok], compute_uv=False).prod(1)
    return out


def draws(which, n=N_DRAWS, seed=0):
    """n uniform draws inside the chain's limits -> [n x ndof] float32, fixed by (chain, n, seed)."""
    key = (which, n, seed)
    if key not in _DRAW:
        robot = H.kin_robots(which)[0]
        _DRAW[key] = robot.sample_joint_angles(n, 0.0, np.random.default_rng(seed))
    return _DRAW[key]


def reference(which, part, n=N_DRAWS, seed=0):
    """w_ref of draws(which, n, seed) over the chain's table, computed once."""
    key = (which, part, n, seed)
    if key not in _REF:
        _REF[key] = w_ref(table_rows(H.kin_robots(which)[0]), draws(which, n, seed), part)
    return _REF[key]


def gate_case(which):
    """-> (q [GATE_ROWS x ndof] float32, w_ref [GATE_ROWS], floor = its median, part) of a chain of GATE_CASES."""
    seed, part = GATE_CASES[which]
    ref = reference(which, part, GATE_ROWS, seed)
    return draws(which, GATE_ROWS, seed), ref, float(np.median(ref)), part


def band_shares(ref, floor):
    """(share of the rows inside the band around the floor, share surely below it, share surely at or above it) from the reference alone."""
    ref = np.asarray(ref)
    return float((np.abs(ref - floor) <= BAND).mean()), float((ref < floor - BAND).mean()), float((ref > floor + BAND).mean())


def below_ref(ref, floor):
    """-> (below [n] bool by the rule !(w >= floor) on the reference, decided [n] bool: outside the band)."""
    ref = np.asarray(ref)
    return ~(ref >= floor), ~(np.abs(ref - floor) <= BAND)


def gpu_tol(ref):
    """Per row: 4 x MANIP_TOL_ABS plus one f32 ulp of w_ref."""
    return 4 * MANIP_TOL_ABS + np.spacing(np.abs(np.asarray(ref)).astype(np.float32)).astype(np.float64)


def gantry():
    """Three orthogonal prismatic joints and one revolute joint about z through the tool point -> product Robot (4 joints): LINEAR is exactly 1,
    ANGULAR exactly 0 (its Gram matrix has rank 1)."""
    from ikflow_amd.robots import Robot

    text = "\n".join([
        '<robot name="gantry">',
        '  <joint name="x" type="prismatic"><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="1 0 0"/><limit lower="-1" upper="1"/></joint>',
        '  <joint name="y" type="prismatic"><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="0 1 0"/><limit lower="-1" upper="1"/></joint>',
        '  <joint name="z" type="prismatic"><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="0 0 1"/><limit lower="-1" upper="1"/></joint>',
        '  <joint name="yaw" type="revolute"><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="0 0 1"/><limit lower="-3" upper="3"/></joint>',
        '  <joint name="tool" type="fixed"><origin xyz="0 0 0" rpy="0 0 0"/></joint>',
        "</robot>"])
    return Robot.from_urdf(text, name="gantry")
