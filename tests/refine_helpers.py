"""Refined candidates (include/ikflow_amd_refine.h): the loop of one row as a loop of the ORACLE - ko.lm_step in fp64 (or f32) and
ko.calculate_pose_error - and the criterion the host build (tests/test_refine_math_host.py) and the GPU tests (tests/test_refine.py) share.  The
criterion is that of test_exact_ik_seeded_is_row_exact_against_the_oracle (tests/test_gpu_parity.py), row by row instead of pose by pose."""
import functools

import numpy as np
import torch

import helpers as H
from oracle import kinematics_oracle as ko

CHAINS = ("panda", "fetch", "syn4p", "syn6r", "syn8p")
TOLERANCES = ((1e-3, 0.1), (1e-4, 5e-3))
N_STEPS = 4
BAND_CAP = 0.03          # share of rows whose stop decision hangs on rounding; on the oracle alone 0 .. 2.2 % for CHAINS x TOLERANCES at 600 rows
SENS_FACTOR = 8.0
SEED = 71             # helpers.lm_inputs(orob, 600, 0.05, 71): on panda at (1e-3, 0.1) the oracle loop stops after 1 / 2 / 3 / 4 steps on 159 / 420 / 19 / 2 rows


def oracle_refine(orob, poses, q, n_steps, pos_tol, rot_tol, lm_dtype=torch.float64, q_ulps=0):
    """poses [rows x 7] (one per row), q [rows x ndof] f32 -> (q [rows x ndof] f32, steps [rows] int64, converged [rows] bool, margins [rows x 2]:
    the smallest |pos_err - pos_tol| and |rot_err - rot_tol| over the iterations the row evaluated).  lm_dtype float64: the step in double, q
    rounded to f32 after it (what the kernel does by default); q_ulps: every iterate that leaves a step moved by that many f32 ulps (the twin)."""
    q = q.clone().to(torch.float32)
    rows = q.shape[0]
    steps = torch.zeros(rows, dtype=torch.int64)
    conv = torch.zeros(rows, dtype=torch.bool)
    margins = torch.full((rows, 2), float("inf"), dtype=torch.float64)
    active = torch.arange(rows)
    for it in range(n_steps):
        if active.numel() == 0:
            break
        qa = ko.lm_step(orob, poses[active].to(lm_dtype), q[active].to(lm_dtype)).to(torch.float32)
        for _u in range(abs(int(q_ulps))):
            qa = torch.nextafter(qa, torch.full_like(qa, float("inf") if q_ulps > 0 else -float("inf")))
        qa = ko.clamp_to_joint_limits(orob, qa)
        q[active] = qa
        steps[active] = it + 1
        pe, re = ko.calculate_pose_error(orob, qa, poses[active])
        margins[active, 0] = torch.minimum(margins[active, 0], (pe - pos_tol).abs().double())
        margins[active, 1] = torch.minimum(margins[active, 1], (re - rot_tol).abs().double())
        done = (pe < pos_tol) & (re < rot_tol)
        conv[active[done]] = True
        active = active[~done]
    return q, steps, conv, margins


def refine_inputs(which, n_poses, k, seed=SEED, noise=0.05):
    """(poses [n_poses x 7] f32, seeds [k * n_poses x ndof] f32 tile-major): truth + `noise` rad (or m) of Gaussian noise, clamped - the recipe of
    helpers.lm_inputs, k seeds per pose."""
    orob = H.kin_robots(which)[1]
    q_true = torch.tensor(orob.sample_joint_angles(n_poses, 0.01, np.random.default_rng(seed)))
    poses = ko.forward_kinematics(orob, q_true)
    g = torch.Generator().manual_seed(seed + 1)
    seeds = q_true[None] + noise * torch.randn((k,) + tuple(q_true.shape), generator=g)
    return poses, ko.clamp_to_joint_limits(orob, seeds.reshape(k * n_poses, orob.ndof).float())


@functools.lru_cache(maxsize=None)
def oracle_case(which, n_poses, k, pos_tol, rot_tol, n_steps=N_STEPS, seed=SEED):
    """The inputs of refine_inputs and, computed once and shared, the fp64 oracle loop on them, its one-ulp twin and the f32 oracle loop."""
    orob = H.kin_robots(which)[1]
    poses, seeds = refine_inputs(which, n_poses, k, seed)
    tiled = poses.repeat((k, 1))
    ref = oracle_refine(orob, tiled, seeds, n_steps, pos_tol, rot_tol)
    twin = oracle_refine(orob, tiled, seeds, n_steps, pos_tol, rot_tol, q_ulps=1)
    ref32 = oracle_refine(orob, tiled, seeds, n_steps, pos_tol, rot_tol, lm_dtype=torch.float32)
    return dict(which=which, orob=orob, poses=poses, seeds=seeds, tiled=tiled, ref=ref, twin=twin, ref32=ref32, pos_tol=pos_tol, rot_tol=rot_tol)


def band_of(margins, pos_tol, rot_tol):
    """Rows for which some evaluated iteration had an error within rounding of its tolerance (the band of tests/test_gpu_parity.py)."""
    return ((margins[:, 0] <= 1e-4 * pos_tol + 5e-7) | (margins[:, 1] <= 1e-4 * rot_tol + 6e-7 / rot_tol)).numpy()


def check_against_oracle(case, q, steps, converged, label=""):
    """fp64 mode.  Outside the band: steps and converged identical to the oracle's, |dq| <= 5e-6 + SENS_FACTOR x the row's own sensitivity (the
    twin's distance from the oracle; a row whose twin stops elsewhere has none).  Every output inside the limits, exactly.  -> rows in the band."""
    orob = case["orob"]
    ref_q, ref_steps, ref_conv, margins = case["ref"]
    twin_q, twin_steps, twin_conv, _ = case["twin"]
    q = np.asarray(q)
    lo = np.array([l[0] for l in orob.actuated_joints_limits], np.float32)
    hi = np.array([l[1] for l in orob.actuated_joints_limits], np.float32)
    assert q.dtype == np.float32 and q.shape == tuple(ref_q.shape) and np.isfinite(q).all()
    assert (q >= lo).all() and (q <= hi).all()
    band = band_of(margins, case["pos_tol"], case["rot_tol"])
    clear = ~band
    if steps is not None:
        assert np.array_equal(np.asarray(steps, np.int64)[clear], ref_steps.numpy()[clear]), label
        assert (np.asarray(steps) >= 1).all()
    if converged is not None:
        assert np.array_equal(np.asarray(converged, bool)[clear], ref_conv.numpy()[clear]), label
    d = np.abs(q.astype(np.float64) - ref_q.numpy()).max(1)
    sens = (twin_q - ref_q).abs().max(1).values.double().numpy()
    sens[(twin_steps != ref_steps).numpy() | (twin_conv != ref_conv).numpy()] = np.inf
    allowed = 5e-6 + SENS_FACTOR * sens
    print(f"refine {label or case['which']} tol ({case['pos_tol']:g}, {case['rot_tol']:g}): rows {len(d)}, band {int(band.sum())}, steps "
          f"{np.bincount(ref_steps.numpy(), minlength=N_STEPS + 1)[1:].tolist()}, converged {int(ref_conv.sum())}, |dq| max outside the band "
          f"{d[clear].max(initial=0.0):.2e}, beyond 5e-6: {int((d[clear] > 5e-6).sum())}, max d / allowed {(d[clear] / allowed[clear]).max(initial=0.0):.2f}")
    assert (d[clear] <= allowed[clear]).all(), (label, float(d[clear].max()), float((d[clear] / allowed[clear]).max()))
    return int(band.sum())


def f32_distances(case, q):
    """f32 mode, one case: (kernel distance, f32 oracle loop's distance) from the fp64 oracle loop's FINAL rows, in units of
    cond(J^T J + 1e-4 I) x 2^-24 x max(|dq|, 1e-3) (cond at the seed, dq = final - seed), over the rows outside the band of both oracle loops whose
    f32 oracle loop took the steps of the fp64 one and whose seed is not near a branch point of the error vector; and the share of rows kept.
    Every output finite and inside the limits, exactly."""
    orob = case["orob"]
    ref_q, ref_steps, _, m64 = case["ref"]
    o32_q, o32_steps, _, m32 = case["ref32"]
    q = np.asarray(q)
    lo = np.array([l[0] for l in orob.actuated_joints_limits], np.float32)
    hi = np.array([l[1] for l in orob.actuated_joints_limits], np.float32)
    assert q.dtype == np.float32 and q.shape == tuple(ref_q.shape) and np.isfinite(q).all() and (q >= lo).all() and (q <= hi).all()
    keep = ~band_of(m64, case["pos_tol"], case["rot_tol"]) & ~band_of(m32, case["pos_tol"], case["rot_tol"]) & (o32_steps == ref_steps).numpy()
    keep &= ~H.lm_near_branch(orob, case["tiled"], case["seeds"])
    seeds = case["seeds"]
    J = ko.jacobian(orob, seeds.double())
    cond = torch.linalg.cond(J.transpose(1, 2) @ J + 1e-4 * torch.eye(orob.ndof, dtype=torch.float64)).numpy()
    unit = cond * 2.0 ** -24 * np.maximum(np.abs(ref_q.double().numpy() - seeds.double().numpy()).max(1), 1e-3)
    d = np.abs(q.astype(np.float64) - ref_q.double().numpy()).max(1) / unit
    o = np.abs(o32_q.double().numpy() - ref_q.double().numpy()).max(1) / unit
    return d[keep], o[keep], keep


def check_f32_against_oracle(parts, label):
    """f32 mode, the statistical form of helpers.check_lm on the final rows, pooled over `parts` (f32_distances of one or more cases): the
    kernel's median and p99 <= LM_MARGIN x the f32 oracle loop's, its maximum <= LM_MAX_MARGIN x; at least 90 % of the rows compared."""
    d, o, keep = (np.concatenate([p[i] for p in parts]) for i in range(3))
    k3, r3 = H._q3(d), H._q3(o)
    print(f"refine f32 {label}: {int(keep.sum())} of {len(keep)} rows, kernel (median, p99, max) {tuple(round(x, 3) for x in k3)} oracle f32 loop "
          f"{tuple(round(x, 3) for x in r3)} [units of cond eps |dq|]")
    assert keep.mean() >= 0.9, float(keep.mean())
    assert k3[0] <= H.LM_MARGIN * r3[0] and k3[1] <= H.LM_MARGIN * r3[1] and k3[2] <= H.LM_MAX_MARGIN * r3[2], (label, k3, r3)
