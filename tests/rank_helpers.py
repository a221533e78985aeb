"""Inputs, the fp64 reference and the tolerance of a best-of-K row score, shared by the host build of ikflow_amd/csrc/rank_math.h
(tests/test_rank_math_host.py) and the GPU tests (tests/test_ranked.py).

Tolerance of a row score, from the project's existing figures only (position error 2e-6; rotation error 2e-5 above helpers.ROT_FLOOR and, below
it, the f32 noise that include/ikflow_amd.h documents as 9.3e-4, rounded up to 1e-3; 1e-6 relative on the joint distance):
    eps = 2e-6 + rot_weight * (2e-5 if the fp64 angle > ROT_FLOOR else 1e-3) + 1e-6 * ref_weight * max(1, joint distance)
Admissibility is compared exactly except on rows inside a band around a decision: eps around the position threshold, the rotation figure of eps
(2e-5 / 1e-3, radians) around the rotation threshold, 1e-4 around min_clearance (as test_capsule_geometry_against_the_oracle), one ulp around a limit."""
import numpy as np
import torch

import helpers as H
from oracle import kinematics_oracle as ko

INF = float("inf")


def collision_capsules(robot):
    """The small capsule model of tests/test_kinematics.py (_collision_capsules), rebuilt: base, three moving links, a sphere."""
    act = [j.name for j in robot.joints if j.actuated]
    rng = np.random.default_rng(5)
    caps = [(None, (0.0, 0.0, 0.0), (0.0, 0.0, 0.2), 0.05)]
    for nm in (act[1], act[2], act[-1]):
        caps.append((nm, tuple(rng.uniform(-0.08, 0.08, 3)), tuple(rng.uniform(-0.15, 0.15, 3)), float(rng.uniform(0.03, 0.08))))
    caps.append((act[-1], (0.01, 0.02, 0.03), (0.01, 0.02, 0.03), 0.04))
    return caps


def limits(orob):
    lo = torch.tensor([l[0] for l in orob.actuated_joints_limits], dtype=torch.float32)
    hi = torch.tensor([l[1] for l in orob.actuated_joints_limits], dtype=torch.float32)
    return lo, hi


def candidates(orob, m, k, seed=0, lo_exp=-3.0, hi_exp=0.0, wild=False):
    """m reachable poses and k candidates each, tile-major [k * m x ndof]: the truth plus noise of scale logspace(lo_exp, hi_exp, k) per repeat,
    clamped to the limits - or, `wild`, left unclamped and stretched so that many rows leave the limits.  Also a reference configuration per pose."""
    g = torch.Generator().manual_seed(1000 + seed)
    q_true, poses = H.reachable_poses(orob, m, 40 + seed)
    scale = torch.logspace(lo_exp, hi_exp, k)
    noise = torch.randn(k, m, orob.ndof, generator=g) * scale[:, None, None]
    q = q_true[None] + noise
    if wild:
        lo, hi = limits(orob)
        q = q + 0.3 * (hi - lo) * torch.randn(k, m, orob.ndof, generator=g) * (torch.rand(k, m, 1, generator=g) < 0.3)
    else:
        q = ko.clamp_to_joint_limits(orob, q.reshape(k * m, -1)).reshape(k, m, -1)
    q_ref = ko.clamp_to_joint_limits(orob, q_true + 0.2 * torch.randn(m, orob.ndof, generator=g))
    return poses.float().contiguous(), q.reshape(k * m, orob.ndof).float().contiguous(), q_ref.float().contiguous()


def clearance_threshold(orob, caps, q):
    """min_clearance for the tests with capsules: the median of the fp64 oracle's clearances of these rows, so that on every chain about half of
    the rows are rejected (with a fixed value every row of a short chain collides with this capsule model, and nothing would be compared)."""
    return float(np.median(ko.capsule_clearance(orob, caps, (), q.double()).numpy()))


def reference(orob, poses, q, k, rot_weight, q_ref=None, ref_weight=0.0, max_pos=None, max_rot=None, reject_limits=False, caps=None,
              min_clearance=0.0, dtype=torch.float64):
    """-> dict of numpy arrays over the k * m rows: score (fp64 arithmetic on the f32 inputs, or `dtype`), eps, admissible, near (inside a band)."""
    m = poses.shape[0]
    tgt = poses.repeat((k, 1))
    pe, re = ko.calculate_pose_error(orob, q.to(dtype), tgt.to(dtype))
    _, re64 = (pe, re) if dtype == torch.float64 else ko.calculate_pose_error(orob, q.double(), tgt.double())
    pe, re, re64 = pe.double().numpy(), re.double().numpy(), re64.numpy()
    rot_fig = np.where(re64 > H.ROT_FLOOR, 2e-5, 1e-3)
    score = pe + rot_weight * re
    eps = 2e-6 + rot_weight * rot_fig
    if q_ref is not None:
        dist = torch.norm(q.to(dtype) - q_ref.repeat((k, 1)).to(dtype), dim=1).double().numpy()
        score = score + ref_weight * dist
        eps = eps + 1e-6 * ref_weight * np.maximum(1.0, dist)
    adm = np.isfinite(score)
    near = np.zeros_like(adm)
    if max_pos is not None:
        adm &= pe < max_pos
        near |= np.abs(pe - max_pos) <= eps
    if max_rot is not None:
        adm &= re < max_rot
        near |= np.abs(re - max_rot) <= rot_fig
    if reject_limits:
        adm &= ~ko.calculate_joint_limits_exceeded(q, orob.actuated_joints_limits).numpy()
        lo, hi = limits(orob)
        qn = q.numpy()
        ulp = np.spacing(np.maximum(np.abs(lo.numpy()), np.abs(hi.numpy())))
        near |= ((np.abs(qn - lo.numpy()) <= ulp) | (np.abs(qn - hi.numpy()) <= ulp)).any(1)
    if caps is not None:
        cl = ko.capsule_clearance(orob, caps, (), q.double()).numpy()
        adm &= ~(cl < min_clearance)
        near |= np.abs(cl - min_clearance) <= 1e-4
    return {"score": score, "eps": eps, "admissible": adm, "near": near}


def check_row_scores(got, ref, what=""):
    """`got` [k * m] f32 row scores (+inf = inadmissible) against reference(...): admissibility exact outside the bands, every admissible row
    within its eps.  Returns the worst |difference| / eps (printed by the callers)."""
    got = np.asarray(got, dtype=np.float64)
    sure = ~ref["near"]
    bad = sure & (np.isfinite(got) != ref["admissible"])
    assert not bad.any(), f"{what}: admissibility differs on {int(bad.sum())} rows outside every band, first {np.flatnonzero(bad)[:5]}"
    both = np.isfinite(got) & ref["admissible"]
    assert both.any(), f"{what}: no admissible row to compare"
    ratio = np.abs(got[both] - ref["score"][both]) / ref["eps"][both]
    assert ratio.max() <= 1.0, f"{what}: a row score is {ratio.max():.2f} x its tolerance from the fp64 reference"
    return float(ratio.max())


def select(row_scores, m, k, n_keep):
    """numpy selection of a pose's best n_keep: stable lexsort (score, then repeat index) of its finite scores -> (index [m x n_keep] int32,
    score [m x n_keep] f32, count [m] int32); unfilled slots -1 / +inf."""
    s = np.asarray(row_scores, dtype=np.float32).reshape(k, m)
    idx = np.full((m, n_keep), -1, np.int32)
    sc = np.full((m, n_keep), np.inf, np.float32)
    cnt = np.isfinite(s).sum(0).astype(np.int32)
    rep = np.arange(k)
    for j in range(m):
        order = np.lexsort((rep, s[:, j]))
        order = order[np.isfinite(s[order, j])][:n_keep]
        idx[j, :len(order)] = order
        sc[j, :len(order)] = s[order, j]
    return idx, sc, cnt
