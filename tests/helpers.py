"""Shared builders for the tests: seeded models, poses, latents.

Weights, layouts, joint limits, sampled configurations and target poses all come from the ORACLE's own tables and
generators (oracle/flow_oracle.py, oracle/robot_tables.py); the product only contributes the objects its API needs
(ikflow_amd Robot + IkflowModelParameters).  tests/test_oracle_independence.py checks the two sets of tables agree."""
import math

import numpy as np
import torch

from ikflow_amd.model import TINY_MODEL_PARAMS, IkflowModelParameters, hparams_for
from ikflow_amd.robots import get_robot
from oracle import flow_oracle as fo
from oracle import kinematics_oracle as ko
from oracle.robot_tables import OracleRobot
from oracle.robot_tables import robot as oracle_robot_by_name


def same_bits(a, b):
    """Same shape, dtype and bytes: equality that tells -0.0 from 0.0 and one NaN from another."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def O(robot) -> OracleRobot:
    """The oracle's own description of `robot` (looked up by name only)."""
    return robot if isinstance(robot, OracleRobot) else oracle_robot_by_name(robot if isinstance(robot, str) else robot.name)


def released_model(model_name, seed=0, gain=1.0):
    """(product Robot, product hparams, oracle layout, oracle-generated state_dict) of a released architecture."""
    lay = fo.layout_for(model_name)
    robot_name = fo.RELEASED[model_name][0]
    return get_robot(robot_name), hparams_for(model_name), lay, fo.make_state_dict(lay, robot_name, seed=seed, output_gain=gain)


def panda_model(seed=0, gain=1.0):
    return released_model("panda__full__lp191_5.25m", seed, gain)


def fetch_arm_model(seed=0, gain=1.0):
    return released_model("fetch_arm__large__mh186_9.25m", seed, gain)


def tiny_model(seed=0, gain=1.0):
    lay = fo.layout_for("tiny")
    return get_robot("panda"), TINY_MODEL_PARAMS, lay, fo.make_state_dict(lay, "panda", seed=seed, output_gain=gain)


def custom_model(nb_nodes=2, dim=9, n_hidden=2, width=256, robot_name="panda", softflow=True, sigmoid=False, seed=0, gain=1.0):
    """Any (coeff_fn_config, coeff_fn_internal_size, ...) the reference's IkflowModelParameters can express."""
    hp = IkflowModelParameters()
    hp.nb_nodes, hp.dim_latent_space, hp.coeff_fn_config, hp.coeff_fn_internal_size = nb_nodes, dim, n_hidden, width
    hp.softflow_enabled, hp.sigmoid_on_output = softflow, sigmoid
    lay = fo.OracleLayout(nb_nodes, dim, 8 if softflow else 7, width, n_hidden, float(hp.rnvp_clamp), O(robot_name).ndof, sigmoid)
    return get_robot(robot_name), hp, lay, fo.make_state_dict(lay, robot_name, seed=seed, output_gain=gain)


def _dense_fixed_transform(model, seed):
    """The builders' state_dicts carry the reference's FixedLinearTransform: diagonal M, b = 0 on plain graphs - neither the bias, the
    index order of x.mm(M) / (x - b).mm(M_inv) nor the sign of log|det M_inv| shows there.  This one is dense and non-symmetric with b != 0
    and |det| far from 1 (M_inv the fp64 inverse of the f32 M, both rounded to f32)."""
    robot, hp, lay, sd = model
    rng = np.random.default_rng(seed)
    D = lay.dim
    M = np.asarray(sd["module_list.0.M"], dtype=np.float64) @ (np.eye(D) + 0.3 * rng.standard_normal((D, D)) / np.sqrt(D))
    sd = dict(sd)
    sd["module_list.0.M"] = M.astype(np.float32)
    sd["module_list.0.M_inv"] = np.linalg.inv(M.astype(np.float32).astype(np.float64)).astype(np.float32)
    sd["module_list.0.b"] = (0.2 * rng.standard_normal((1, D))).astype(np.float32)
    return robot, hp, lay, sd


def shuffled_permutations(model, seed):
    """The builders always produce PermuteRandom's np.random.seed(i) tables: an index slip that is right for those tables only stays hidden.
    Here every block gets another seeded permutation (perm and perm_inv consistent: perm_inv[perm[k]] = k) that differs from its seed-i
    table, no two blocks share one, and no position is a fixed point of every block."""
    robot, hp, lay, sd = model
    rng = np.random.default_rng(seed)
    D = lay.dim
    stock = [fo.permute_random_tables(D, i)[0] for i in range(lay.nb_nodes)]
    while True:
        perms = [rng.permutation(D).astype(np.int64) for _ in range(lay.nb_nodes)]
        differs = all(not np.array_equal(p, s) for p, s in zip(perms, stock))
        distinct = len({p.tobytes() for p in perms}) == len(perms)
        fixed_everywhere = np.all([p == np.arange(D) for p in perms], axis=0).any()
        if differs and distinct and not fixed_everywhere:
            break
    sd = dict(sd)
    for i, perm in enumerate(perms):
        perm_inv = np.empty_like(perm)
        perm_inv[perm] = np.arange(D)
        sd[f"module_list.{lay.perm_module(i)}.perm"] = perm
        sd[f"module_list.{lay.perm_module(i)}.perm_inv"] = perm_inv
    return robot, hp, lay, sd


def plain_bias(model, seed):
    """A non-zero module_list.0.b on a plain (non-sigmoid) graph, whose builder leaves it at zero; M and M_inv stay as they are."""
    robot, hp, lay, sd = model
    assert not lay.sigmoid_on_output
    sd = dict(sd)
    sd["module_list.0.b"] = (0.2 * np.random.default_rng(seed).standard_normal((1, lay.dim))).astype(np.float32)
    return robot, hp, lay, sd


def reachable_poses(robot, n, seed=0, eps=0.004363323129985824):
    """poses = FK(q), q ~ U(lo+eps, hi-eps) (scripts/build_dataset.py:186 convention)."""
    q = torch.tensor(O(robot).sample_joint_angles(n, eps, np.random.default_rng(seed)))
    return q, ko.forward_kinematics(robot, q)


def latents(n, dim, seed=1):
    return torch.randn(n, dim, generator=torch.Generator().manual_seed(seed))


# ---- kinematics: synthetic chains and the inputs / criteria the host build and the GPU tests share ------------------------------------------
def synthetic_chain(ndof, prismatic=(), seed=0):
    """URDF text (a bare <joint> list, as oracle/robot_tables.py keeps its robots) of a serial chain of `ndof` actuated joints: random origins
    (|xyz| up to 0.3 m per component, rpy over the full range), random unit axes, a fixed joint before every second actuated joint and a fixed tool
    joint.  `prismatic`: the actuated indices that slide.  Every joint has limits of its own, so a clamp against the wrong joint's limits shows."""
    rng = np.random.default_rng(1000 * ndof + 17 * seed + sum(3 ** p for p in prismatic))
    f = lambda v: " ".join(repr(float(x)) for x in v)
    origin = lambda: f'<origin xyz="{f(rng.uniform(-0.3, 0.3, 3))}" rpy="{f(rng.uniform(-np.pi, np.pi, 3))}"/>'
    out = [f'<robot name="syn{ndof}">']
    for i in range(ndof):
        if i % 2 == 1:
            out.append(f'  <joint name="fixed{i}" type="fixed">{origin()}</joint>')
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        if i in prismatic:
            typ, lo, hi = "prismatic", rng.uniform(-0.25, -0.05), rng.uniform(0.1, 0.45)
        else:
            typ, lo, hi = "revolute", rng.uniform(-3.0, -1.6), rng.uniform(1.6, 3.0)
        out.append(f'  <joint name="joint{i}" type="{typ}">{origin()}<axis xyz="{f(ax)}"/><limit lower="{lo!r}" upper="{hi!r}"/></joint>')
    out.append(f'  <joint name="tool" type="fixed">{origin()}</joint>')
    out.append("</robot>")
    return "\n".join(out)


# ndof 4 .. 8, each all-revolute and with prismatic joints that between them sit first, in the middle and last; the built-in robots stay in
KIN_CHAINS = {"syn4r": (4, ()), "syn4p": (4, (3,)), "syn5r": (5, ()), "syn5p": (5, (2,)), "syn6r": (6, ()), "syn6p": (6, (0, 5)),
              "syn7r": (7, ()), "syn7p": (7, (3,)), "syn8r": (8, ()), "syn8p": (8, (0, 4, 7))}
KIN_BUILTIN = ("panda", "fetch_arm", "fetch")
KIN_ALL = KIN_BUILTIN + tuple(KIN_CHAINS)
_KIN_CACHE = {}


def kin_robots(which):
    """(product Robot, OracleRobot) of a built-in robot or a synthetic chain: the same URDF text through the product's reader and through the
    oracle's own, so the two share no code."""
    if which not in _KIN_CACHE:
        if which in KIN_BUILTIN:
            _KIN_CACHE[which] = (get_robot(which), oracle_robot_by_name(which))
        else:
            from ikflow_amd.robots import Robot
            from oracle.robot_tables import parse_chain

            text = synthetic_chain(*KIN_CHAINS[which])
            _KIN_CACHE[which] = (Robot.from_urdf(text, name=which), OracleRobot(which, parse_chain(text)))
    return _KIN_CACHE[which]


def quat_branches(orob, q):
    """Which of the four mat_to_quat candidates (largest of |w|, |x|, |y|, |z|) each row takes, from the oracle's fp64 rotation matrix."""
    R = ko._chain_transforms(orob, q.double())[0][:, :3, :3]
    t = torch.stack([R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2], R[:, 0, 0] - R[:, 1, 1] - R[:, 2, 2],
                     -R[:, 0, 0] + R[:, 1, 1] - R[:, 2, 2], -R[:, 0, 0] - R[:, 1, 1] + R[:, 2, 2]], 1)
    return t.argmax(1).numpy()


def limit_edge_rows(orob):
    """Rows exactly on a limit and one float32 ulp either side of it, joint by joint (tests/golden/make_ref_vectors.py does this for Panda);
    returns (cfg [m x ndof] float32, exceeded [m] bool as the strict inequalities define it)."""
    lo = np.array([l[0] for l in orob.actuated_joints_limits], np.float32)
    hi = np.array([l[1] for l in orob.actuated_joints_limits], np.float32)
    mid = ((lo.astype(np.float64) + hi) / 2).astype(np.float32)
    rows, exp = [lo.copy(), hi.copy()], [False, False]
    for j in range(orob.ndof):
        for base, toward, ex in ((hi, np.inf, True), (hi, -np.inf, False), (lo, -np.inf, True), (lo, np.inf, False)):
            r = mid.copy()
            r[j] = np.nextafter(base[j], np.float32(toward))
            rows.append(r)
            exp.append(ex)
            r = mid.copy()
            r[j] = base[j]
            rows.append(r)
            exp.append(False)
    return np.stack(rows), np.array(exp)


def _quat_mul(a, b):
    return ko.quaternion_product(a, b)


def lm_inputs(orob, n, noise, seed):
    """(target poses [m x 7] f32, seeds [m x ndof] f32, n_random): `n` rows of truth + `noise` rad (or m) of Gaussian noise, clamped, then the
    hand-made rows, 8 of each: rotation error of exactly pi about x, y, z; pitch error of +pi/2 and -pi/2; every joint on its lower (upper)
    limit; target equal to FK(seed)."""
    q_true = torch.tensor(orob.sample_joint_angles(n, 0.01, np.random.default_rng(seed)))
    poses = ko.forward_kinematics(orob, q_true)
    seeds = ko.clamp_to_joint_limits(orob, q_true + noise * torch.randn(q_true.shape, generator=torch.Generator().manual_seed(seed + 1)))
    k = 8
    s0 = seeds[:k]
    cur = ko.forward_kinematics(orob, s0.double())
    extra_p, extra_q = [], []
    h = math.sqrt(0.5)
    for e in ([0.0, 1, 0, 0], [0.0, 0, 1, 0], [0.0, 0, 0, 1], [h, 0, h, 0], [h, 0, -h, 0]):   # target = e * current: error quaternion exactly e
        tq = _quat_mul(torch.tensor([e], dtype=torch.float64).expand(k, 4), cur[:, 3:])
        extra_p.append(torch.cat([cur[:, :3], tq], 1).float())
        extra_q.append(s0)
    lo = torch.tensor([l[0] for l in orob.actuated_joints_limits], dtype=torch.float32)
    hi = torch.tensor([l[1] for l in orob.actuated_joints_limits], dtype=torch.float32)
    for edge in (lo, hi):
        extra_p.append(poses[k:2 * k])
        extra_q.append(edge.repeat(k, 1))
    extra_p.append(ko.forward_kinematics(orob, s0))
    extra_q.append(s0)
    return torch.cat([poses] + extra_p), torch.cat([seeds] + extra_q), n


def lm_near_branch(orob, poses, seeds, margin=0.01):
    """Rows whose fp64 oracle error vector is within `margin` of a branch point: roll or yaw at +-pi (atan2), pitch at +-pi/2 (asin)."""
    e = ko.pose_error_vector(orob, poses.double(), seeds.double())[:, :3].abs().numpy()
    return (e[:, 0] > math.pi - margin) | (e[:, 2] > math.pi - margin) | (e[:, 1] > math.pi / 2 - margin)


def _q3(e):
    return float(np.median(e)), float(np.quantile(e, 0.99)), float(e.max())


def check_fk(fk_fn, which, n=20000, seed=4):
    """FK of a backend (`fk_fn(q f32 numpy) -> [n x 7]`) against the oracle in fp64 on every row: position and quaternion (up to sign) at the
    project's 2e-6, under 1 % of the rows with the other sign, all four mat_to_quat branches in the sample."""
    _, orob = kin_robots(which)
    q = torch.tensor(orob.sample_joint_angles(n, 0.0, np.random.default_rng(seed)))
    ref = ko.forward_kinematics(orob, q.double()).numpy()
    got = np.asarray(fk_fn(q.numpy()), np.float64)
    dp = np.abs(got[:, :3] - ref[:, :3]).max()
    same, flip = np.abs(got[:, 3:] - ref[:, 3:]).max(1), np.abs(got[:, 3:] + ref[:, 3:]).max(1)
    dq = np.minimum(same, flip).max()
    share = float((same > 2e-6).mean())
    br = np.bincount(quat_branches(orob, q), minlength=4) / n
    print(f"fk {which}: |dp| {dp:.2e} |dquat| {dq:.2e} other sign {share:.4f} branches {np.round(br, 3).tolist()}")
    assert (br > 0).all(), br
    assert dp <= 2e-6 and dq <= 2e-6, (dp, dq)
    assert share < 0.01, share


def check_position_error(pe_fn, which, n=20000, seed=8):
    """Position error of `pe_fn(q, target) -> (pos [n], rot [n])` at the project's 2e-6 for unrelated configurations and targets."""
    _, orob = kin_robots(which)
    _, poses = reachable_poses(orob, n, seed)
    q2 = torch.tensor(orob.sample_joint_angles(n, 0.0, np.random.default_rng(seed + 1)))
    pe, _ = pe_fn(q2.numpy(), poses.numpy())
    ref, _ = ko.calculate_pose_error(orob, q2.double(), poses.double())
    d = float(np.abs(np.asarray(pe, np.float64) - ref.numpy()).max())
    print(f"pose error {which}: |dpos| {d:.2e}")
    assert d <= 2e-6, d


# margins of the statistical criteria (kernel quantile <= margin x the f32 oracle's quantile on the same rows).  fp64 mode needs none, on the host
# build and on the MI355X (measured there: at most 0.39 x at the median, 0.15 x at p99, 0.073 x at the maximum).  f32 mode and the rotation error
# below the floor take the 1.5 x that test_lm_step_in_the_reference_arithmetic_carries_the_reference_noise allows for its median and p99; the
# measured ratios are in the docstrings of tests/test_kinematics.py and in CHANGELOG.md.
LM_MARGIN = 1.5
LM64_MARGIN = 1.0


def check_lm(lm_fn, which, noise, n=20000, seed=21):
    """One LM step of a backend (`lm_fn(targets, seeds, mode) -> [m x ndof]`, mode "f64" / "f32") on truth + `noise` and the hand-made rows.
    Every output finite and inside the limits, exactly.  Rows near a branch point of the error vector (at most 1 %) are left out of the
    comparison with the oracle.  fp64 mode: no further from the fp64 oracle than the oracle's f32 step, at the median, p99 and maximum
    (no margin: LM64_MARGIN); the project's absolute 5e-6 where it is known to hold (built-in robots, 0.15 rad).  f32 mode: in units of
    cond(J^T J + 1e-4 I) x 2^-24 x max(|dq|, 1e-3), median and p99 <= LM_MARGIN x the f32 oracle's, maximum <= LM_MAX_MARGIN x.  Returns the measured ratios."""
    _, orob = kin_robots(which)
    poses, seeds, _ = lm_inputs(orob, n, noise, seed)
    lo = np.array([l[0] for l in orob.actuated_joints_limits], np.float32)
    hi = np.array([l[1] for l in orob.actuated_joints_limits], np.float32)
    near = lm_near_branch(orob, poses, seeds)
    share = float(near.mean())
    on_limit = 0.0
    ref64 = ko.lm_step(orob, poses.double(), seeds.double()).numpy()
    ref32 = ko.lm_step(orob, poses, seeds).numpy().astype(np.float64)
    J = ko.jacobian(orob, seeds.double())
    cond = torch.linalg.cond(J.transpose(1, 2) @ J + 1e-4 * torch.eye(orob.ndof, dtype=torch.float64)).numpy()
    unit = cond * 2.0 ** -24 * np.maximum(np.abs(ref64 - seeds.numpy()).max(1), 1e-3)
    keep = ~near
    ratios = {}
    for mode in ("f64", "f32"):
        got = np.asarray(lm_fn(poses.numpy(), seeds.numpy(), mode))
        assert got.dtype == np.float32 and np.isfinite(got).all()
        assert (got >= lo).all() and (got <= hi).all()                      # inside the limits, exactly, the left-out rows included
        on_limit = float(((got == lo) | (got == hi)).any(1).mean())
        d = np.abs(got.astype(np.float64) - ref64).max(1)[keep]
        o = np.abs(ref32 - ref64).max(1)[keep]
        if mode == "f32":
            d, o = d / unit[keep], o / unit[keep]
        k, r = _q3(d), _q3(o)
        ratios[mode] = tuple(a / b for a, b in zip(k, r))
        print(f"lm {which} noise {noise} {mode}: kernel (median, p99, max) {k} oracle f32 {r} ratio {tuple(round(x, 3) for x in ratios[mode])}"
              f"{' [units of cond eps |dq|]' if mode == 'f32' else ''}; left out {share:.4f}, on a limit {on_limit:.3f}")
        m = LM64_MARGIN if mode == "f64" else LM_MARGIN
        assert k[0] <= m * r[0] and k[1] <= m * r[1] and k[2] <= (m if mode == "f64" else LM_MAX_MARGIN) * r[2], (mode, k, r)
        if mode == "f64" and which in KIN_BUILTIN and noise <= 0.15:
            assert k[2] <= 5e-6, k
    assert share <= 0.01, share
    return ratios


# Rotation error: above this fp64 angle the f32 oracle itself stays within 1e-5 of fp64 on these inputs (one ulp of the quaternion dot product
# is worth 2.4e-7 / theta: below it the error of ANY f32 evaluation grows as 1 / theta).  Found on the CPU over every chain of KIN_ALL and the
# five seed distances: see test_rotation_error_floor_is_where_the_f32_oracle_meets_1e_5 in tests/test_kin_math_host.py.
ROT_FLOOR = 0.15
POSE_NOISES = (1e-4, 1e-3, 1e-2, 5e-2, 0.3)
ACOS_CLAMP_ANGLE = float(2.0 * np.arccos(np.float32(1.0 - 1e-7), dtype=np.float32))   # 9.766e-4 = 2 acosf(1 - 1e-7 rounded to f32)


def pose_error_cases(orob, n, seed=31):
    """{case: (q, targets)}: targets FK(q) in f32 (identical), the same with the quaternion negated (antipodal), scaled by 0.5 and by 2, and
    targets FK(truth) for q = truth + each of POSE_NOISES."""
    q = torch.tensor(orob.sample_joint_angles(n, 0.0, np.random.default_rng(seed)))
    fk = ko.forward_kinematics(orob, q)
    scaled = lambda s: torch.cat([fk[:, :3], s * fk[:, 3:]], 1)
    cases = {"identical": (q, fk), "antipodal": (q, scaled(-1.0)), "half": (q, scaled(0.5)), "double": (q, scaled(2.0))}
    for i, noise in enumerate(POSE_NOISES):
        seeds = ko.clamp_to_joint_limits(orob, q + noise * torch.randn(q.shape, generator=torch.Generator().manual_seed(seed + 2 + i)))
        cases[f"noise{noise:g}"] = (seeds, fk)
    return cases


def rot_reference(orob, q, tgt, acos_epsilon=None):
    """(fp64 oracle, f32 oracle) rotation error of FK(q) against the target quaternions."""
    r64 = ko.geodesic_distance_between_quaternions(tgt[:, 3:].double(), ko.forward_kinematics(orob, q.double())[:, 3:], acos_epsilon)
    r32 = ko.geodesic_distance_between_quaternions(tgt[:, 3:], ko.forward_kinematics(orob, q)[:, 3:], acos_epsilon)
    return r64.numpy(), r32.numpy().astype(np.float64)


def check_rot_error(case, got, r64, r32, clamp_angle=ACOS_CLAMP_ANGLE):
    """Rotation error of a backend on one case of pose_error_cases.  Identical / antipodal / doubled targets (the acos clamp decides): between
    the clamp angle - 1e-6 and the f32 oracle's maximum on the same rows - never near 2 pi.  Everything else: the project's 2e-5 against fp64 on
    the rows whose fp64 angle is above ROT_FLOOR.  Returns (kernel, f32 oracle) distances from fp64 of the rows below the floor, for
    check_rot_below_floor to pool over the cases of a chain."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all()
    if case in ("identical", "antipodal", "double"):
        print(f"rot {case}: kernel [{got.min():.4e}, {got.max():.4e}] oracle f32 [{r32.min():.4e}, {r32.max():.4e}] clamp {clamp_angle:.4e}")
        assert got.min() >= clamp_angle - 1e-6 and got.max() <= r32.max(), (got.min(), got.max(), r32.max())
        return np.zeros(0), np.zeros(0)
    high = r64 > ROT_FLOOR
    if high.any():
        d = float(np.abs(got - r64)[high].max())
        print(f"rot {case}: {int(high.sum())} rows above the floor, |d| {d:.2e}")
        assert d <= 2e-5, d
    return np.abs(got - r64)[~high], np.abs(r32 - r64)[~high]


# The maximum of a sample is a noisy statistic: in units of cond eps |dq| the f32 oracle's OWN maximum over the even and over the odd rows of one
# LM sample differs by up to 3.8 x on the chains of KIN_ALL - measured on the oracle alone (test_spread_of_the_f32_oracles_own_maximum in
# tests/test_kin_math_host.py).  A bound on the kernel's maximum tighter than that would refuse an exact copy of the oracle that rounds
# differently, so the f32-mode maxima are compared with the oracle's own spread, rounded up, as the margin.  (The same spread of the rotation
# error below the floor is 1.23 x: LM_MARGIN covers it.)
LM_MAX_MARGIN = 4.0


def check_rot_below_floor(which, parts):
    """The rows below ROT_FLOOR of every seed distance of one chain, pooled: the kernel's distance from fp64 against the f32 oracle's distance from
    fp64 on the same rows - median, p99 and maximum x LM_MARGIN.  Returns the ratios."""
    dk, do = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert len(dk) >= 1000, len(dk)
    k, r = _q3(dk), _q3(do)
    ratio = tuple(a / b for a, b in zip(k, r))
    print(f"rot {which}: {len(dk)} rows below the floor, kernel (median, p99, max) {k} oracle f32 {r} ratio {tuple(round(x, 3) for x in ratio)}")
    assert all(a <= LM_MARGIN * b for a, b in zip(k, r)), (k, r)
    return ratio
