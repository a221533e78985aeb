"""Exact IK (ikf_generate_exact_seeded, ikf_refine_exact): the inputs and criteria that the oracle-only checks (tests/test_exact_rounds_inputs.py) and the
GPU tests (tests/test_exact_rounds.py) share.

Nothing here is a new tolerance.  The band rule (band_pos = 1e-4 thr + 5e-7, band_rot = 1e-4 thr + 6e-7 / thr), the cap of 3 % on the band's share and
|dq| <= 5e-6 + 8 x the twin's sensitivity are those of test_exact_ik_seeded_is_row_exact_against_the_oracle (tests/test_gpu_parity.py) and of
refine_helpers.check_against_oracle, from which they are imported.

The last section serves tests/test_exact_flow.py and tests/test_exact_flow_inputs.py (ikf_generate_exact, the flow in): its cases, the raw call
and the same schedule put together from ikf_generate_approx_tiled and ikf_generate_exact_seeded.  It has no criterion at all: bits."""
import ctypes as C
import functools
import os

import numpy as np
import torch

import helpers as H
import refine_helpers as RH
import sample_helpers as sh
from oracle import flow_oracle as fo
from oracle import kinematics_oracle as ko

BAND_CAP = RH.BAND_CAP
SENS_FACTOR = RH.SENS_FACTOR
band_of = RH.band_of
POS_THR, ROT_THR = 1e-3, 0.05
REDUNDANT = ("panda", "fetch_arm", "fetch", "syn7r", "syn7p", "syn8r", "syn8p")   # 7 and 8 joints: a pose has a family of solutions, so repeats end apart
SEPARATION = 1e-4
FAR_OFFSET = 100.0


def orob_of(which):
    return H.kin_robots(which)[1]


def truth(which, n, seed, eps=0.01):
    orob = orob_of(which)
    return torch.tensor(orob.sample_joint_angles(n, eps, np.random.default_rng(seed))).float()


# ---- validity by construction -----------------------------------------------------------------------------------------------------------------
def pattern_inputs(which, pattern, seed):
    """pattern [n] bool, True = "solvable" -> (poses [n x 7] f32, seeds [n x ndof] f32).  A solvable pose is FK(q_true) and its seed q_true; an
    unsolvable pose is the same pose with 100 m added to x, y and z (same seed).  With thresholds (1e-3, 0.05) a truth seed is valid after the first
    LM step (worst case over 2000 rows of each of the 13 chains, fp64 and f32 steps: pos 5.4e-7, rot 2.1e-3) and a far pose never is (smallest
    position margin 171 m): test_pattern_construction_fixes_validity checks both on the oracle, with empty bands."""
    pattern = np.asarray(pattern, bool)
    q_true = truth(which, len(pattern), seed)
    poses = ko.forward_kinematics(orob_of(which), q_true)
    poses[torch.from_numpy(~pattern), :3] += FAR_OFFSET
    return poses, q_true


def far_seeds(which, q_true, sign=1.0):
    """truth + 2.5 rad (or m) on every joint, clamped: the round-0 seed of a pose that a later round is to solve."""
    return ko.clamp_to_joint_limits(orob_of(which), q_true + sign * 2.5)


def invalid_after_one_step(which, poses, seeds):
    """Rows whose seed the oracle (fp64 step) finds invalid after one LM step at (1e-3, 0.05), outside the band."""
    orob = orob_of(which)
    if len(seeds) == 0:
        return np.zeros(0, bool)
    _, _, conv, margins = RH.oracle_refine(orob, poses, seeds, 1, POS_THR, ROT_THR)
    return ~conv.numpy() & ~band_of(margins, POS_THR, ROT_THR)


def three_round_case(which, A, B, seed):
    """The three-round schedule of the compaction tests.  A, B: bool [n]; round 0 solves A, round 1 solves B & ~A, round 2 sees what remains.
    A pose of B & ~A is solvable, but its round-0 seed is truth + 2.5 (or, where the oracle finds that seed valid or in the band after one step,
    truth - 2.5; where both are, the pose leaves B and becomes unsolvable - the returned B says what was built).
    -> dict(poses, seeds0, seeds1 [n x ndof] f32, A, B bool [n] with B disjoint from A, B_wanted: B before any pose left it)."""
    A = np.asarray(A, bool)
    B = np.asarray(B, bool) & ~A
    wanted = B
    poses, q_true = pattern_inputs(which, A | B, seed)
    seeds0 = q_true.clone()
    todo = np.flatnonzero(B)
    for sign in (1.0, -1.0):
        if len(todo) == 0:
            break
        cand = far_seeds(which, q_true[todo], sign)
        ok = invalid_after_one_step(which, poses[todo], cand)
        seeds0[todo[ok]] = cand[ok]
        todo = todo[~ok]
    if len(todo):
        B = B.copy()
        B[todo] = False
        poses[todo, :3] += FAR_OFFSET
    return dict(poses=poses, seeds0=seeds0, seeds1=q_true, A=A, B=B, B_wanted=wanted)


PATTERNS = ("none", "all", "first", "last", "half", "sparse", "runs16", "runs16+5", "blocks4096")


def make_pattern(kind, n, seed=0):
    """The solvable-pose patterns of the compaction tests, bool [n]."""
    i = np.arange(n)
    rng = np.random.default_rng(1000 + seed)
    if kind == "none":
        return np.zeros(n, bool)
    if kind == "all":
        return np.ones(n, bool)
    if kind == "first":
        return i == 0
    if kind == "last":
        return i == n - 1
    if kind == "half":
        return rng.random(n) < 0.5
    if kind == "sparse":
        return rng.random(n) < 0.01
    if kind == "runs16":
        return (i // 16) % 2 == 0
    if kind == "runs16+5":
        return ((i + 5) // 16) % 2 == 0
    if kind == "blocks4096":
        return (i // 4096) % 2 == 0
    raise KeyError(kind)


# ---- the engine's own list, observed -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hip_runtime():
    """The HIP runtime this process has mapped (torch's copy: ikflow_amd._lib loads torch first, so the engine's library is bound to it too)."""
    path = None
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                path = line.split()[-1]
                break
    if path is None:
        path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = C.CDLL(path)
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipStreamSynchronize.restype = C.c_int
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    return hip


HIP_MEMCPY_DEVICE_TO_HOST = 2


def run_seeded_raw(eng, poses, rc, pos_thr, rot_thr, n_lm_steps, seed_fn, sol=None, valid=None, stats_fill=None):
    """ikf_generate_exact_seeded through the C-ABI with a callback that LOOKS at the engine's active list: in every round the `d_idx` argument
    (n_active int32 on the device, the engine's ex_pose_idx) is copied to the host by a hipMemcpyAsync on the engine's stream followed by a stream
    synchronise - ordered after the kernels that built it, round 0's k_iota included - and `seed_fn(round, idx [n_active] int32 numpy, repeat)`
    returns that round's seeds [n_active * repeat x ndof] (device, tile-major).
    poses: device [n x 7] f32.  sol / valid: the output windows to write (device, contiguous; allocated when None).  stats_fill: value the
    stats array holds before the call.  -> (sol, valid uint8, stats [rounds x 4] int64, lists).  No exception crosses the C boundary: the first
    one raised inside the callback is re-raised after the call (the `err` list of Engine.generate_exact)."""
    from ikflow_amd import _lib

    hip = _hip_runtime()
    n, nr, ndof = int(poses.shape[0]), len(rc), eng.layout.ndof
    assert poses.dtype == torch.float32 and poses.is_contiguous() and poses.device == eng.device
    if sol is None:
        sol = torch.empty((n, ndof), dtype=torch.float32, device=eng.device)
    if valid is None:
        valid = torch.empty(n, dtype=torch.uint8, device=eng.device)
    assert sol.is_contiguous() and valid.is_contiguous() and sol.dtype == torch.float32 and valid.dtype == torch.uint8
    stream = eng._stream()
    lists, keep, err = [], [], []

    def _cb(_user, rnd, n_active, repeat, d_idx, cb_ndof):
        try:
            assert rnd == len(lists) and cb_ndof == ndof and repeat == rc[rnd], (rnd, len(lists), cb_ndof, repeat)
            host = np.full(int(n_active), -1, np.int32)
            if n_active:
                assert d_idx, "null active list"
                code = hip.hipMemcpyAsync(host.ctypes.data, d_idx, 4 * int(n_active), HIP_MEMCPY_DEVICE_TO_HOST, stream)
                assert code == 0, f"hipMemcpyAsync: {code}"
                code = hip.hipStreamSynchronize(stream)
                assert code == 0, f"hipStreamSynchronize: {code}"
            lists.append(host)
            sq = seed_fn(rnd, host, int(repeat))
            assert sq.dtype == torch.float32 and sq.is_contiguous() and sq.device == eng.device
            assert tuple(sq.shape) == (int(n_active) * int(repeat), ndof), (tuple(sq.shape), int(n_active), int(repeat), ndof)
            keep.append(sq)
            return sq.data_ptr()   # produced on the stream the engine launches on: ordered
        except BaseException as e:  # never let an exception cross the C boundary
            err.append(e)
            return 0

    cb = _lib.SEED_FN(_cb)
    c_rc = (C.c_int32 * max(nr, 1))(*[int(r) for r in rc])
    c_stats = (C.c_int64 * (4 * max(nr, 1)))()
    if stats_fill is not None:
        for i in range(4 * nr):
            c_stats[i] = stats_fill
    with torch.cuda.device(eng.device):
        code = eng.lib.ikf_generate_exact_seeded(eng._h, poses.data_ptr(), n, c_rc, nr, int(n_lm_steps), float(pos_thr), float(rot_thr), cb, None,
                                                 sol.data_ptr(), valid.data_ptr(), c_stats, stream)
        torch.cuda.current_stream(eng.device).synchronize()   # the seeds in `keep` outlive the kernels that read them
    if err:
        raise err[0]
    eng._ck(code)
    return sol, valid, np.array(list(c_stats), dtype=np.int64).reshape(max(nr, 1), 4)[:nr], lists


# ---- seeds of the parity cases (the recipe of _seed_tables, tests/test_gpu_parity.py) -----------------------------------------------------
SIGMAS = (0.01, 0.05, 0.2, 0.5, 1.0, 3.0)


def seed_tables(which, q_true, rc, seed, sigmas=SIGMAS):
    """Seeds for every (round, repeat, pose): the truth perturbed by a per-pose noise level, clamped -> [R x n x ndof] per round."""
    orob = orob_of(which)
    g = torch.Generator().manual_seed(seed)
    n, ndof = q_true.shape
    sigma = torch.tensor(sigmas)[torch.randint(0, len(sigmas), (n,), generator=g)]
    tables = []
    for R in rc:
        noise = torch.randn(R, n, ndof, generator=g) * sigma[None, :, None]
        tables.append(ko.clamp_to_joint_limits(orob, (q_true[None] + noise).reshape(R * n, ndof)).reshape(R, n, ndof))
    return tables


def oracle_seeded(which, seed_cpu, poses, rc, pos_thr, rot_thr, n_steps, lm_dtype=torch.float64, q_ulps=0):
    """ko.generate_exact_ik_solutions_seeded for a step count other than the reference's 3: the same loop over ko.exact_round, which takes
    n_opt_steps_max.  -> (solutions, valids, margins)."""
    orob = orob_of(which)
    n = poses.shape[0]
    margins = torch.full((n, 2), float("inf"), dtype=torch.float64)
    solutions = torch.zeros(n, orob.ndof, dtype=torch.float32)
    valids = torch.zeros(n, dtype=torch.bool)
    for r, R in enumerate(rc):
        idx = torch.nonzero(~valids)[:, 0]
        if idx.numel() == 0:
            break
        sub = torch.full((idx.numel(), 2), float("inf"), dtype=torch.float64)
        new_sol, new_valid = ko.exact_round(orob, seed_cpu(r, idx), poses[idx], R, pos_thr, rot_thr, n_opt_steps_max=n_steps, lm_dtype=lm_dtype,
                                            margins=sub, q_ulps=q_ulps)
        margins[idx] = torch.minimum(margins[idx], sub)
        solutions[idx] = new_sol
        valids[idx] = new_valid
    return solutions, valids, margins


# (chain, n_lm_steps, seed, noise levels): rc = (1, 3), n = 300, thresholds (1e-3, 0.05).  Every chain at the reference's 3 steps; 1, 2 and 20
# steps on one chain of 7, 4, 6 and 8 joints.  test_parity_cases_have_both_outcomes_and_a_small_band holds every row of this table, on the oracle
# alone, to a band share <= 3 %, both outcomes present and no flag outside the band that moving every iterate by one f32 ulp changes.
# Twenty steps from 1 rad and more of noise wander: on panda and syn6r the oracle's OWN flag changes under such a nudge on 5 % to 10 % of those
# poses (0 to 1 % from 0.5 rad, none from 0.2 rad; measured over 600 poses per level), which no comparison of flags can be asked to survive.  These
# two chains take the levels up to 0.5 rad at 20 steps, which still leaves poses that need most of the 20 steps and poses that never arrive.
PARITY_N, PARITY_RC = 300, (1, 3)
STEP_CHAINS = ("panda", "syn4p", "syn6r", "syn8p")
CALM_SIGMAS = (0.01, 0.05, 0.2, 0.5)
PARITY_CASES = tuple((w, 3, 200 + i, SIGMAS) for i, w in enumerate(H.KIN_ALL)) + (
    ("panda", 1, 300, SIGMAS), ("panda", 2, 301, SIGMAS), ("panda", 20, 440, CALM_SIGMAS),
    ("syn4p", 1, 310, SIGMAS), ("syn4p", 2, 311, SIGMAS), ("syn4p", 20, 312, SIGMAS),
    ("syn6r", 1, 320, SIGMAS), ("syn6r", 2, 321, SIGMAS), ("syn6r", 20, 445, CALM_SIGMAS),
    ("syn8p", 1, 330, SIGMAS), ("syn8p", 2, 331, SIGMAS), ("syn8p", 20, 332, SIGMAS))


def parity_id(case):
    return f"{case[0]}-{case[1]}steps"


@functools.lru_cache(maxsize=None)
def parity_case(case):
    """Inputs of one row of PARITY_CASES and, computed once and shared, the fp64 oracle on them with its margins and its one-ulp twin."""
    which, n_steps, seed, sigmas = case
    q_true = truth(which, PARITY_N, seed)
    poses = ko.forward_kinematics(orob_of(which), q_true)
    tables = seed_tables(which, q_true, PARITY_RC, seed + 1, sigmas)
    seed_cpu = lambda rnd, idx: tables[rnd][:, idx, :].reshape(-1, q_true.shape[1]).contiguous()
    if n_steps == 3:   # the reference's loop as the oracle states it (oracle_seeded is that loop over ko.exact_round with another step count)
        ref_sol, ref_valid, margins = ko.generate_exact_ik_solutions_seeded(orob_of(which), seed_cpu, poses, PARITY_RC, POS_THR, ROT_THR,
                                                                            lm_dtype=torch.float64, return_margins=True)
    else:
        ref_sol, ref_valid, margins = oracle_seeded(which, seed_cpu, poses, PARITY_RC, POS_THR, ROT_THR, n_steps)
    twin_sol, twin_valid, _ = oracle_seeded(which, seed_cpu, poses, PARITY_RC, POS_THR, ROT_THR, n_steps, q_ulps=1)
    return dict(which=which, n_steps=n_steps, poses=poses, tables=tables, seed_cpu=seed_cpu, ref_sol=ref_sol, ref_valid=ref_valid, margins=margins,
                twin_sol=twin_sol, twin_valid=twin_valid, band=band_of(margins, POS_THR, ROT_THR))


def parity_flips(case):
    """Flags outside the band that moving every iterate of the oracle's loop by f32 ulps changes: the case table admits none.  One ulp up (the twin
    every case has anyway) at up to 3 steps; at 20 steps, where the question arises, also one ulp down."""
    c = parity_case(case)
    flipped = (c["twin_valid"] != c["ref_valid"]).numpy()
    for u in ((-1,) if c["n_steps"] > 3 else ()):
        flipped |= (oracle_seeded(c["which"], c["seed_cpu"], c["poses"], PARITY_RC, POS_THR, ROT_THR, c["n_steps"], q_ulps=u)[1] != c["ref_valid"]).numpy()
    return int((flipped & ~c["band"]).sum())


def check_pose_parity(sol, valid, ref_sol, ref_valid, twin_sol, twin_valid, band, label):
    """The criterion of test_exact_ik_seeded_is_row_exact_against_the_oracle, pose by pose: band share <= 3 %, identical flags outside the band,
    |dq| <= 5e-6 + 8 x the pose's twin sensitivity on the poses valid on both sides (a pose whose twin is not valid has none), unsolved rows zero."""
    sol, valid = torch.as_tensor(sol).cpu(), torch.as_tensor(valid).cpu().bool()
    band = torch.as_tensor(band)
    clear = ~band
    share = float(band.float().mean())
    assert share <= BAND_CAP, (label, share)
    assert torch.equal(valid[clear], ref_valid[clear]), (label, torch.nonzero(valid[clear] != ref_valid[clear])[:, 0].tolist()[:8])
    both = clear & valid & ref_valid
    d = (sol[both] - ref_sol[both]).abs().max(1).values.double()
    sens = (twin_sol - ref_sol).abs().max(1).values[both].double()
    sens[~twin_valid[both]] = float("inf")
    allowed = 5e-6 + SENS_FACTOR * sens
    print(f"exact {label}: valid {int(valid.sum())}/{len(valid)} (oracle {int(ref_valid.sum())}), band {int(band.sum())} ({share:.4f}), |dq| max "
          f"{float(d.max()) if len(d) else 0.0:.2e}, beyond 5e-6: {int((d > 5e-6).sum())}, max d / allowed {float((d / allowed).max()) if len(d) else 0.0:.2f}")
    assert bool((d <= allowed).all()), (label, float(d.max()), float((d / allowed).max()))
    assert torch.equal(sol[~valid], torch.zeros_like(sol[~valid])), label
    return share


# ---- the winner, named ------------------------------------------------------------------------------------------------------------------------
def _rows(which, poses, seeds, R, n_steps):
    """Every (repeat, pose) row alone through the oracle's loop and its one-ulp twin: rows are independent, so repeat r's row of a round is the
    row of a one-repeat round on its seed.  -> dict(q [R x n x ndof], steps, conv [R x n], band [R x n], sens [R x n])."""
    orob = orob_of(which)
    n = poses.shape[0]
    tiled = poses.repeat((R, 1))
    q, steps, conv, margins = RH.oracle_refine(orob, tiled, seeds, n_steps, POS_THR, ROT_THR)
    tq, tsteps, tconv, _ = RH.oracle_refine(orob, tiled, seeds, n_steps, POS_THR, ROT_THR, q_ulps=1)
    sens = (tq - q).abs().max(1).values.double().numpy()
    sens[(tsteps != steps).numpy() | (tconv != conv).numpy()] = np.inf
    sh = lambda a: np.asarray(a).reshape(R, n, *np.asarray(a).shape[1:])
    return dict(q=sh(q.numpy()), steps=sh(steps.numpy()), conv=sh(conv.numpy()), band=sh(band_of(margins, POS_THR, ROT_THR)), sens=sh(sens))


def _apart(rows, winner):
    """Per pose: the distance (max over joints) from the winner's oracle row to the nearest other repeat's oracle row."""
    R = rows["q"].shape[0]
    return np.min([np.abs(rows["q"][winner] - rows["q"][r]).max(1) for r in range(R) if r != winner], axis=0)


def tie_inputs(which, n, R, seed):
    """(poses [n x 7], seeds [R * n x ndof] tile-major): every repeat is seeded at q_true + 3e-3 * randn, clamped, so all R repeats of a pose
    are valid after the first step (1e-3, 0.05) and the rule names the winner: repeat R - 1.  On the seven REDUNDANT chains the repeats end more
    than 1e-4 apart on 93.2 % to 100 % of the poses (n = 500, R = 4, seed 5; 93.0 % to 100 % are
    `named` by tie_case); chains with at most 6 joints converge to one point and tell nothing."""
    q_true = truth(which, n, seed, eps=0.05)
    poses = ko.forward_kinematics(orob_of(which), q_true)
    g = torch.Generator().manual_seed(seed + 1)
    seeds = q_true[None] + 3e-3 * torch.randn((R,) + tuple(q_true.shape), generator=g)
    return poses, ko.clamp_to_joint_limits(orob_of(which), seeds.reshape(R * n, -1).float())


@functools.lru_cache(maxsize=None)
def tie_case(which, n=500, R=4, seed=5):
    """tie_inputs and the oracle on them, one step.  `allowed` [n]: 5e-6 + 8 x the winner row's twin sensitivity.  `named` [n]: poses outside the
    band (no repeat's decision hangs on rounding) whose winner row is further than 1e-4 + allowed from every other repeat's row - so any row within
    `allowed` of the winner's is, by the triangle inequality, further than 1e-4 from the others'."""
    poses, seeds = tie_inputs(which, n, R, seed)
    rows = _rows(which, poses, seeds, R, 1)
    sol, valid = ko.exact_round(orob_of(which), seeds, poses, R, POS_THR, ROT_THR, n_opt_steps_max=1, lm_dtype=torch.float64)
    allowed = 5e-6 + SENS_FACTOR * rows["sens"][R - 1]
    apart = _apart(rows, R - 1)
    band = rows["band"].any(0)
    return dict(which=which, poses=poses, seeds=seeds, R=R, rows=rows, sol=sol, valid=valid, allowed=allowed, band=band, apart=apart,
                separable=apart > SEPARATION, named=~band & (apart > SEPARATION + allowed))


LATE_STEPS = 3


def late_inputs(which, n, seed, swapped=False):
    """(poses [n x 7], seeds [2 * n x ndof] tile-major, R = 2): repeat 0 is seeded as in tie_inputs (valid after the first step), the last repeat 0.3 rad
    from the truth (a random direction of joint space, length 0.3, clamped): it becomes valid at iteration 2 or 3 on most poses, at iteration 1
    on almost none (0.3 on EVERY joint is too far for three steps: 33 % to 54 % of the poses get there at all).  swapped: the two seed blocks change places.
    late_case keeps the poses where, outside the band, the early repeat is valid at iteration 1 and the late one at iteration 2 or 3, and whose
    two rows are apart as in tie_case.  Kept of n = 500 (seed 7), measured on the oracle, the same with and without the swap: panda 452, fetch_arm
    466, fetch 489, syn7r 489, syn7p 475, syn8r 486, syn8p 462 (90.4 % to 97.8 %; the condition is at least half)."""
    q_true = truth(which, n, seed, eps=0.05)
    orob = orob_of(which)
    poses = ko.forward_kinematics(orob, q_true)
    g = torch.Generator().manual_seed(seed + 1)
    early = ko.clamp_to_joint_limits(orob, (q_true + 3e-3 * torch.randn(q_true.shape, generator=g)).float())
    d = torch.randn(q_true.shape, generator=g)
    late = ko.clamp_to_joint_limits(orob, (q_true + 0.3 * d / d.norm(dim=1, keepdim=True)).float())
    return poses, torch.cat([late, early] if swapped else [early, late]), 2


@functools.lru_cache(maxsize=None)
def late_case(which, n=500, seed=7, swapped=False):
    poses, seeds, R = late_inputs(which, n, seed, swapped)
    rows = _rows(which, poses, seeds, R, LATE_STEPS)
    e, l = (1, 0) if swapped else (0, 1)
    sol, valid = ko.exact_round(orob_of(which), seeds, poses, R, POS_THR, ROT_THR, n_opt_steps_max=LATE_STEPS, lm_dtype=torch.float64)
    allowed = 5e-6 + SENS_FACTOR * rows["sens"][e]
    apart = _apart(rows, e)
    kept = ~rows["band"].any(0) & rows["conv"][e] & (rows["steps"][e] == 1) & rows["conv"][l] & (rows["steps"][l] >= 2) & (apart > SEPARATION + allowed)
    return dict(which=which, poses=poses, seeds=seeds, R=R, rows=rows, sol=sol, valid=valid, allowed=allowed, kept=kept, early=e, late=l)


# ---- the ends of the step range ---------------------------------------------------------------------------------------------------------------
LONG_STEPS = 255


@functools.lru_cache(maxsize=None)
def long_case(which="syn5p", n=64, R=2, seed=41):
    """One ikf_refine_exact round of 255 steps: every third pose is a far pose (its rows run the whole loop: 0 must still mean "never"), the others
    are seeded as in seed_tables, so some become valid in the first steps and some only after tens of them (the byte must hold what a 3-step
    round never writes).  -> the inputs and the fp64 oracle's answer with its band."""
    pattern = np.arange(n) % 3 != 2
    poses, q_true = pattern_inputs(which, pattern, seed)
    seeds = seed_tables(which, q_true, (R,), seed + 1)[0].reshape(R * n, -1).contiguous()
    margins = torch.full((n, 2), float("inf"), dtype=torch.float64)
    sol, valid = ko.exact_round(orob_of(which), seeds, poses, R, POS_THR, ROT_THR, n_opt_steps_max=LONG_STEPS, lm_dtype=torch.float64, margins=margins)
    band = band_of(margins, POS_THR, ROT_THR) & pattern   # (a far pose is 100 m off whatever its rotation error does: it has no band)
    return dict(which=which, poses=poses, seeds=seeds, R=R, pattern=pattern, sol=sol, valid=valid, band=band)


def long_case_conditions(c):
    """What the oracle alone says about long_case: per row its first valid iteration (0 = never), and the number of flags outside the band that
    moving every iterate by one f32 ulp, up or down, changes (a pose is valid when one of its rows is) - one pass of nudged_rows for all three."""
    R, n = c["R"], len(c["pattern"])
    first = nudged_rows(c["which"], c["poses"].repeat((R, 1)), c["seeds"], LONG_STEPS, (0, 1, -1)).reshape(3, R, n)
    assert np.array_equal((first[0] > 0).any(0), c["valid"].numpy())
    flipped = ((first[1] > 0).any(0) != c["valid"].numpy()) | ((first[2] > 0).any(0) != c["valid"].numpy())
    return first[0], int((flipped & ~c["band"]).sum())


# ---- layout and independence ------------------------------------------------------------------------------------------------------------------
def layout_inputs(which, n=257, R=5, seed=51):
    """(poses [n x 7], seeds [R x n x ndof]) with the noise levels of seed_tables."""
    q_true = truth(which, n, seed)
    return ko.forward_kinematics(orob_of(which), q_true), seed_tables(which, q_true, (R,), seed + 1)[0]


@functools.lru_cache(maxsize=None)
def single_pose_case(which, R=300, seed=53, sigma=0.5):
    """One pose, R = 300 repeats seeded sigma = 0.5 from the truth (some repeats get there in three steps, most do not): the rows of one pose span
    two workgroups of k_exact_lm_iters and share one pose_first word.  -> inputs, the fp64 oracle's answer, its twin's, the pose's band flag and
    per repeat the oracle's first valid iteration."""
    q_true = truth(which, 1, seed)
    poses = ko.forward_kinematics(orob_of(which), q_true)
    seeds = seed_tables(which, q_true, (R,), seed + 1, sigmas=(sigma,))[0].reshape(R, -1).contiguous()
    margins = torch.full((1, 2), float("inf"), dtype=torch.float64)
    sol, valid = ko.exact_round(orob_of(which), seeds, poses, R, POS_THR, ROT_THR, lm_dtype=torch.float64, margins=margins)
    twin_sol, twin_valid = ko.exact_round(orob_of(which), seeds, poses, R, POS_THR, ROT_THR, lm_dtype=torch.float64, q_ulps=1)
    rows = RH.oracle_refine(orob_of(which), poses.repeat((R, 1)), seeds, 3, POS_THR, ROT_THR)
    return dict(which=which, poses=poses, seeds=seeds, R=R, sol=sol, valid=valid, twin_sol=twin_sol, twin_valid=twin_valid,
                band=band_of(margins, POS_THR, ROT_THR), first=np.where(rows[2].numpy(), rows[1].numpy(), 0))


def nudged_rows(which, poses, seeds, n_steps, ulps=(0, 1, -1)):
    """The oracle's loop of one row (ko.lm_step in fp64, q rounded to f32, clamp, ko.calculate_pose_error, stop at the first valid iteration) on
    every row of `seeds` [m x ndof] against `poses` [m x 7], once per entry of `ulps` in ONE pass: copy u has every iterate that leaves a step
    moved by u f32 ulps (refine_helpers.oracle_refine, which takes one u per pass).  -> first valid iteration [len(ulps) x m] (0 = never)."""
    orob = orob_of(which)
    m, k = seeds.shape[0], len(ulps)
    q = seeds.float().repeat((k, 1))
    tgt = poses.repeat((k, 1))
    u = torch.tensor(ulps, dtype=torch.int64).repeat_interleave(m)
    first = torch.zeros(k * m, dtype=torch.int64)
    active = torch.arange(k * m)
    for it in range(n_steps):
        if active.numel() == 0:
            break
        qa = ko.lm_step(orob, tgt[active].double(), q[active].double()).float()
        ua = u[active][:, None]
        for step in range(1, int(u.abs().max()) + 1):
            toward = torch.where(ua > 0, float("inf"), -float("inf")).expand_as(qa)
            qa = torch.where(ua.abs() >= step, torch.nextafter(qa, toward), qa)
        qa = ko.clamp_to_joint_limits(orob, qa)
        q[active] = qa
        pe, re = ko.calculate_pose_error(orob, qa, tgt[active])
        done = (pe < POS_THR) & (re < ROT_THR)
        first[active[done]] = it + 1
        active = active[~done]
    return first.reshape(k, m).numpy()


# ---- the upper half of the byte ---------------------------------------------------------------------------------------------------------------
LATE_BYTE = ("syn6r", 3000, 77)


def late_byte_inputs():
    """(which, poses [3000 x 7], seeds [3000 x ndof]): syn6r, one repeat, seeds 1 rad and 3 rad of noise from the truth.  A row that becomes valid
    after iteration 127 got there by wandering: the oracle finds 11 such rows here (nudged_rows, 255 steps), and NONE of them keeps its iteration,
    or stays late, when every iterate is moved by one ulp (the same on syn5p: 4 rows of 3000, and none on syn4r).  A steady approach cannot be that
    late either: a direction of singular value s contracts by r = s^2 / (s^2 + 1e-4) per step, crossing at step k needs a start e0 = thr e^(r k),
    and a crossing that clears the band needs r thr >> 6e-7 - for k = 150 and a start within the linear range (0.3 rad x s) no r satisfies both.
    So no row can be NAMED that the oracle and the kernel must both find valid at an iteration of 128 .. 255; what can be asked is what the test
    of this case asks of the kernel against itself."""
    which, n, seed = LATE_BYTE
    q_true = truth(which, n, seed)
    return which, ko.forward_kinematics(orob_of(which), q_true), seed_tables(which, q_true, (1,), seed + 1, sigmas=(1.0, 3.0))[0][0].contiguous()


# ---- the flow in (tests/test_exact_flow.py, tests/test_exact_flow_inputs.py) --------------------------------------------------------------------
# ikf_generate_exact against its two parts, ikf_generate_approx_tiled followed by ikf_generate_exact_seeded.  Models, pools and weights are those of
# sample_helpers; loose thresholds on random weights give all three rounds a strict sub-list (tests/test_exact_flow_inputs.py holds the counts).
FLOW_RC = (1, 3, 10)
FLOW_THR = (0.2, 1.0)
FLOW_STEPS = 3
LATENT_STRIDE = 37        # round i's latents start at row 37 i of the pool: no two rounds of a case share a row position
# name -> (model, n, schedule, (pos_thr, rot_thr))
FLOW_CASES = {f"{m}-{n}": (m, n, FLOW_RC, FLOW_THR) for m, n in (("R", 200), ("R10", 200), ("R8", 200), ("Rsig", 200), ("T", 200), ("R", 17),
                                                                 ("R10", 17), ("R8", 17), ("Rsig", 17), ("T", 17), ("R", 1))}
FLOW_CASES.update({
    "R-450-tight": ("R", 450, FLOW_RC, (0.05, 0.3)),        # round 2 beyond one 4096-row row-owner chunk
    "R-130-r2": ("R", 130, (2, 4, 40), FLOW_THR),           # R > 1 in round 0, and the same
    "T-1800-tight": ("T", 1800, FLOW_RC, (0.02, 0.1)),      # round 2 beyond the 16384-row per-layer chunk
    "T-200-all": ("T", 200, FLOW_RC, (10.0, 4.0)),          # everything solved in round 0
    "T-200-none": ("T", 200, FLOW_RC, (1e-9, 1e-9)),        # nothing ever solved
})
FLOW_N200 = ("R-200", "R10-200", "R8-200", "Rsig-200", "T-200")


def flow_latents(name, n, rc):
    """Per round i the latents [n * rc[i] x D] on the CPU: rows 37 i .. of the model's pool (sample_helpers.inputs), or, where the pool is shorter
    than that, helpers.latents(n * rc[i], D, 100 + i)."""
    pool = sh.inputs(name)[0]
    out = []
    for i, R in enumerate(rc):
        a, rows = LATENT_STRIDE * i, n * R
        out.append(pool[a:a + rows] if a + rows <= pool.shape[0] else H.latents(rows, pool.shape[1], 100 + i))
    return out


def flow_case_inputs(case):
    """(model name, poses [n x 7], latents per round, schedule, pos_thr, rot_thr) of one entry of FLOW_CASES, on the CPU."""
    name, n, rc, (pos_thr, rot_thr) = FLOW_CASES[case]
    return name, sh.inputs(name)[1][:n], flow_latents(name, n, rc), rc, pos_thr, rot_thr


def oracle_flow_fn(name):
    robot, hp, lay, sd = sh.model(name)
    return lambda latent, poses_tiled: fo.generate_ik_solutions_torch(sd, lay, robot, poses_tiled, latent[: poses_tiled.shape[0]], clamp=True)


@functools.lru_cache(maxsize=None)
def oracle_schedule(case):
    """The oracle's schedule on one entry of FLOW_CASES, round by round (the loop of ko.generate_exact_ik_solutions over ko.exact_round, fp64 LM,
    which does not report its rounds) -> dict(active, rows, solved: one int per round run, sol, valid)."""
    name, poses, lats, rc, pos_thr, rot_thr = flow_case_inputs(case)
    robot = sh.model(name)[0]
    flow_fn = oracle_flow_fn(name)
    sol = torch.zeros(poses.shape[0], robot.ndof)
    valid = torch.zeros(poses.shape[0], dtype=torch.bool)
    active, rows, solved = [], [], []
    for r, R in enumerate(rc):
        idx = torch.nonzero(~valid)[:, 0]
        if idx.numel() == 0:
            break
        new_sol, new_valid = ko.exact_round(robot, flow_fn(lats[r][: idx.numel() * R], poses[idx].repeat((R, 1))), poses[idx], R, pos_thr, rot_thr,
                                            lm_dtype=torch.float64)
        sol[idx], valid[idx] = new_sol, new_valid
        active.append(int(idx.numel()))
        rows.append(int(idx.numel()) * R)
        solved.append(int(new_valid.sum()))
    return dict(active=active, rows=rows, solved=solved, sol=sol, valid=valid)


def run_flow_raw(eng, poses, rc, pos_thr, rot_thr, n_lm_steps, latents, sol=None, valid=None, stats_fill=None):
    """The twin of run_seeded_raw for ikf_generate_exact: the _lib.LATENT_FN callback records (round, rows, dim) of every call and returns
    latents[round].data_ptr() - device tensors made before the call, so the callback allocates nothing and enqueues nothing.
    -> (sol, valid uint8, stats [rounds x 4] int64, calls)."""
    from ikflow_amd import _lib

    n, nr, ndof = int(poses.shape[0]), len(rc), eng.layout.ndof
    assert poses.dtype == torch.float32 and poses.is_contiguous() and poses.device == eng.device
    for lt in latents:
        assert lt.dtype == torch.float32 and lt.is_contiguous() and lt.device == eng.device and lt.ndim == 2
    if sol is None:
        sol = torch.empty((n, ndof), dtype=torch.float32, device=eng.device)
    if valid is None:
        valid = torch.empty(n, dtype=torch.uint8, device=eng.device)
    assert sol.is_contiguous() and valid.is_contiguous() and sol.dtype == torch.float32 and valid.dtype == torch.uint8
    stream = eng._stream()
    calls, err = [], []

    def _cb(_user, rnd, rows, dim):
        try:
            calls.append((int(rnd), int(rows), int(dim)))
            lt = latents[rnd]
            assert lt.shape[1] == dim and lt.shape[0] >= rows, (rnd, tuple(lt.shape), int(rows), int(dim))   # never hand out fewer rows than asked for
            return lt.data_ptr()
        except BaseException as e:  # never let an exception cross the C boundary
            err.append(e)
            return 0

    cb = _lib.LATENT_FN(_cb)
    c_rc = (C.c_int32 * max(nr, 1))(*[int(r) for r in rc])
    c_stats = (C.c_int64 * (4 * max(nr, 1)))()
    if stats_fill is not None:
        for i in range(4 * nr):
            c_stats[i] = stats_fill
    with torch.cuda.device(eng.device):
        code = eng.lib.ikf_generate_exact(eng._h, poses.data_ptr(), n, c_rc, nr, int(n_lm_steps), float(pos_thr), float(rot_thr), cb, None,
                                          sol.data_ptr(), valid.data_ptr(), c_stats, stream)
        torch.cuda.current_stream(eng.device).synchronize()   # the latents outlive the kernels that read them
    if err:
        raise err[0]
    eng._ck(code)
    return sol, valid, np.array(list(c_stats), dtype=np.int64).reshape(max(nr, 1), 4)[:nr], calls


def parts(eng, P, rc, pos_thr, rot_thr, n_lm_steps, latents):
    """The schedule of ikf_generate_exact put together from the two entries that have strict suites of their own, with no re-entrant call on the
    handle.  Round r's list is predicted on the host (arange(n), then the ascending poses with valid == 0 after the prefix rc[:r]); its seeds
    are ikf_generate_approx_tiled (sample_helpers.guarded_tiled: clamp on, softflow 0) under the source (P, list_r, len(list_r)) on the first
    len(list_r) * rc[r] rows of latents[r]; the prefix rc[:r + 1] is then run by run_seeded_raw on the seeds of rounds 0 .. r, and every list
    the engine showed its callback must be the predicted one.  `latents`: per round a device tensor, or a callable (round, rows) -> tensor.
    -> (sol, valid, stats [len(rc) x 4], lists) of the last prefix (stats rows of rounds never started are zero, as the one call leaves them)."""
    n = int(P.shape[0])
    lst = np.arange(n, dtype=np.int32)
    predicted, seeds, out = [], [], None
    for r in range(len(rc)):
        if r > 0:
            lst = np.flatnonzero(out[1].cpu().numpy() == 0).astype(np.int32)
            if len(lst) == 0:
                break
        predicted.append(lst)
        rows = len(lst) * int(rc[r])
        Z = latents(r, rows) if callable(latents) else latents[r][:rows]
        assert Z.shape[0] == rows and Z.is_contiguous(), (r, tuple(Z.shape), rows)
        seeds.append(sh.guarded_tiled(eng, P, torch.from_numpy(lst).to(P.device), len(lst), Z, clamp=1))
        out = run_seeded_raw(eng, P, rc[:r + 1], pos_thr, rot_thr, n_lm_steps, lambda rnd, idx, repeat: seeds[rnd])
        assert len(out[3]) == len(predicted), (r, len(out[3]), len(predicted))
        for j, (seen, want) in enumerate(zip(out[3], predicted)):
            assert seen.dtype == np.int32 and np.array_equal(seen, want), (r, j, len(seen), len(want))
    sol, valid, stats, lists = out
    full = np.zeros((len(rc), 4), np.int64)
    full[:len(stats)] = stats
    return sol, valid, full, lists
