"""What tests/test_flow_sample.py (GPU) and tests/test_flow_sample_inputs.py (CPU) share: the models, transforms, inputs and fp64 references
of the sampling-pass tests, the guarded raw call and the switch that forces one launch form.

Every reference a GPU test compares with comes from `reference(...)`, which only serves the keys listed in REFERENCE_SETS - and the CPU file
holds every one of those to "the f32 torch oracle alone is within FLOW_TOL / 2 of the fp64 twin on every row".  A GPU test therefore cannot
use an input on which the tolerance would be spent by the reference itself."""
import contextlib
import ctypes as C
import functools

import numpy as np
import torch

from helpers import O, _dense_fixed_transform, custom_model, latents, plain_bias, reachable_poses, shuffled_permutations, tiny_model
from ikflow_amd import _lib
from ikflow_amd.ikflow_solver import IKFlowSolver
from oracle import flow_oracle as fo

DEV = "cuda:0"
FLOW_TOL = 1e-5          # relative to max(1, |x|): the tolerance of every unclamped comparison in the suite
SENTINEL = 0x7FC0DEAD    # a quiet NaN with a payload: see test_sentinel_is_a_nan_no_float32_arithmetic_yields
GUARD = 64               # rows of sentinel in front of and behind the n rows a call may write (a 16-row tile past the end stays inside)
SOFT = 0.37              # the non-zero softflow entry
BROADCAST_ROW = 5        # the pose a broadcast call uses for every row
GAIN = 1.5

# ---- models ------------------------------------------------------------------------------------------------------------------------------
# "A": the weights every test uses (gain 1.5); "B": the other weights of the reload test (gain 2.0)
WEIGHTS = {"A": (31, GAIN), "B": (32, 2.0)}
# T1 (one hidden layer: a subnet is two Linears, nothing averages the first one's rounding): at seed 31 / gain 1.5 the f32 torch oracle is
# itself up to 1.2e-5 from fp64 on the rows used here (seeds 33 .. 35: 1.9e-5, 8.3e-6, 5.4e-6), which leaves a kernel no room inside FLOW_TOL.
# At gain 1.0 and seed 35 it is 2.7e-6 (tests/test_flow_sample_inputs.py keeps it below FLOW_TOL / 2).
WEIGHTS_OF = {"T1": {"A": (35, 1.0)}}
_RELEASED_WIDTH = dict(nb_nodes=2, n_hidden=3, width=1024)   # the released width and depth (row-owner and cluster forms), 2 blocks instead of 12
MODELS = {
    "R": lambda seed, gain: custom_model(dim=7, seed=seed, gain=gain, **_RELEASED_WIDTH),
    "R10": lambda seed, gain: custom_model(dim=10, robot_name="fetch_arm", seed=seed, gain=gain, **_RELEASED_WIDTH),   # ndof 7 < D: the slice matters
    "R8": lambda seed, gain: custom_model(dim=8, robot_name="fetch", seed=seed, gain=gain, **_RELEASED_WIDTH),         # 8 joints
    "Rpad": lambda seed, gain: custom_model(nb_nodes=2, dim=7, n_hidden=3, width=1000, seed=seed, gain=gain),          # padded to 1024
    "Rsig": lambda seed, gain: custom_model(dim=7, softflow=False, sigmoid=True, seed=seed, gain=gain, **_RELEASED_WIDTH),
    "T": lambda seed, gain: tiny_model(seed=seed, gain=gain),                                                          # width 256, two hidden layers
    "T300": lambda seed, gain: custom_model(nb_nodes=2, dim=10, n_hidden=3, width=300, robot_name="fetch_arm", seed=seed, gain=gain),   # padded to 512
    "T1": lambda seed, gain: custom_model(n_hidden=1, width=256, seed=seed, gain=gain),                                # the unfused pipeline, automatically
}


def _without(model, key):
    robot, hp, lay, sd = model
    return robot, hp, lay, {k: v for k, v in sd.items() if k != key}


TRANSFORMS = {
    "plain": lambda m: m,
    "dense": lambda m: _dense_fixed_transform(m, 23),                                  # dense non-symmetric M_inv, b != 0, M present
    "dense-noM": lambda m: _without(_dense_fixed_transform(m, 23), "module_list.0.M"),   # ... M absent
    "bias": lambda m: plain_bias(m, 24),                                               # b != 0 alone
    "no-b": lambda m: _without(m, "module_list.0.b"),                                   # the key deleted
    "perm": lambda m: shuffled_permutations(m, 25),
    "all": lambda m: shuffled_permutations(_dense_fixed_transform(m, 23), 25),
}
EXIT_TRANSFORMS = ("dense", "dense-noM", "bias", "no-b", "perm", "all")


@functools.lru_cache(maxsize=None)
def model(name, transform="plain", weights="A"):
    """(product Robot, product hparams, oracle layout, state_dict)"""
    seed, gain = {**WEIGHTS, **WEIGHTS_OF.get(name, {})}[weights]
    return TRANSFORMS[transform](MODELS[name](seed, gain))


# ---- inputs: one pool of rows per model; every test uses leading rows of it ------------------------------------------------------------------
POOL = {"R": 2 * 4096 + 2049, "R10": 4096 + 200, "R8": 4096 + 17, "Rpad": 4096 + 17, "Rsig": 4096 + 17, "T": 16385, "T300": 4096 + 200, "T1": 4096 + 200}
INPUT_SEED = 41


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(latent [POOL x D] ~ N(0, 1), reachable target poses [POOL x 7]) on the CPU."""
    robot, hp, lay, sd = model(name)
    _, poses = reachable_poses(robot, POOL[name], INPUT_SEED)
    return latents(POOL[name], lay.dim, INPUT_SEED + 1), poses


@functools.lru_cache(maxsize=None)
def device_inputs(name):
    z, poses = inputs(name)
    return z.to(DEV), poses.to(DEV)


def conditional(name, n, soft=0.0, broadcast=False):
    """The oracle's conditional of the first n rows: [pose] or [pose, softflow scale]; broadcast: pose BROADCAST_ROW on every row."""
    lay = model(name)[2]
    poses = inputs(name)[1].numpy().astype(np.float64)
    c = np.repeat(poses[BROADCAST_ROW:BROADCAST_ROW + 1], n, 0) if broadcast else poses[:n]
    if lay.dim_cond == 8:
        c = np.concatenate([c, np.full((n, 1), soft)], 1)
    else:
        assert soft == 0.0
    return c


# ---- references --------------------------------------------------------------------------------------------------------------------------
def _reference_sets():
    """{(model, transform, weights, soft, broadcast): rows}: every input a GPU test compares with the oracle, with the largest n it uses."""
    sets = {}
    # guarded stores, position independence, input forms: per-row and broadcast pose, softflow 0 and SOFT (8-entry conditional only)
    guarded = {"R": 4096 + 17, "R10": 4096 + 17, "R8": 4096 + 17, "Rpad": 4096 + 17, "Rsig": 4096 + 17, "T": 16385, "T300": 2049, "T1": 700}
    for name, n in guarded.items():
        for soft in ((0.0, SOFT) if model(name)[2].dim_cond == 8 else (0.0,)):
            for broadcast in (False, True):
                sets[(name, "plain", "A", soft, broadcast)] = n
    # plan seams (and the reload test's first weights): R, default settings, up to 2 x 4096 + 2049 rows
    for broadcast in (False, True):
        sets[("R", "plain", "A", 0.0, broadcast)] = POOL["R"]
    # exit transform and permutations
    for name in ("R", "R10", "T", "T1"):
        for tr in EXIT_TRANSFORMS:
            sets[(name, tr, "A", 0.0, False)] = 4096 + 200
    # reload: the other weights
    for name in ("R", "T"):
        sets[(name, "all", "B", 0.0, False)] = 4096 + 200
    sets[("T", "plain", "A", 0.0, False)] = max(sets[("T", "plain", "A", 0.0, False)], 4096 + 200)
    return sets


REFERENCE_SETS = _reference_sets()


@functools.lru_cache(maxsize=None)
def reference(name, transform="plain", weights="A", soft=0.0, broadcast=False):
    """fp64 oracle, unclamped, [rows x ndof] with rows = REFERENCE_SETS[key]: computed once, sliced by the tests, never changed."""
    n = REFERENCE_SETS[(name, transform, weights, soft, broadcast)]
    robot, hp, lay, sd = model(name, transform, weights)
    z = inputs(name)[0][:n].numpy().astype(np.float64)
    ref = fo.run_inference_f64(sd, lay, robot, z, conditional(name, n, soft, broadcast), False)
    ref.setflags(write=False)
    return ref


def reference_f32(name, transform="plain", weights="A", soft=0.0, broadcast=False):
    """The same rows through the f32 torch oracle (the reference implementation's own arithmetic)."""
    n = REFERENCE_SETS[(name, transform, weights, soft, broadcast)]
    robot, hp, lay, sd = model(name, transform, weights)
    cond = torch.from_numpy(conditional(name, n, soft, broadcast).astype(np.float32))
    return fo.run_inference_torch(sd, lay, robot, inputs(name)[0][:n], cond, False).numpy()


def rel_err(got, ref):
    """max |got - ref| / max(1, |ref|); NaN if anything is not finite."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


def limits(name, device=None):
    """(lo, hi) of the joints, f32 tensors."""
    lim = O(model(name)[0]).actuated_joints_limits
    lo, hi = torch.tensor([l[0] for l in lim], dtype=torch.float32), torch.tensor([l[1] for l in lim], dtype=torch.float32)
    return (lo, hi) if device is None else (lo.to(device), hi.to(device))


# ---- handles -------------------------------------------------------------------------------------------------------------------------------
def new_solver(mdl, precision="f32"):
    robot, hp, lay, sd = mdl
    s = IKFlowSolver(hp, robot)
    s.load_state_dict_tensors(sd)
    if precision != "f32":
        s.set_precision(precision)
    return s


@functools.lru_cache(maxsize=None)
def shared_solver(name, transform="plain", weights="A"):
    """One handle per model for the tests that leave it as they found it (every switch goes through `force`)."""
    return new_solver(model(name, transform, weights))


# ---- the guarded raw call ----------------------------------------------------------------------------------------------------------------
def guarded_approx(eng, P, Z, clamp, soft=0.0, broadcast=False, stream=None, shift=0):
    """ikf_generate_approx through the raw C-ABI into an int32 buffer of (GUARD + n + GUARD) x ndof words filled with SENTINEL (with `shift`
    further words in front: shift = 1 makes the output pointer 4-byte aligned only); the pointer passed is that of row GUARD.  Both guard
    bands must come back bit-unchanged, and no element of rows 0 .. n - 1 may still hold the sentinel - a NaN payload no kernel produces, so
    a hit is an element nobody wrote.  Returns the n rows as float32."""
    n, ndof = Z.shape[0], eng.layout.ndof
    front = shift + GUARD * ndof
    buf = torch.full((front + (n + GUARD) * ndof,), SENTINEL, dtype=torch.int32, device=Z.device)
    rows = buf[front: front + n * ndof]
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(Z.device))   # (the fill above ran on the current stream)
    s = C.c_void_p((torch.cuda.current_stream(Z.device) if stream is None else stream).cuda_stream)
    code = eng.lib.ikf_generate_approx(eng._h, P.data_ptr(), 1 if broadcast else 0, Z.data_ptr(), n, 1 if clamp else 0, float(soft),
                                       rows.data_ptr(), s)
    assert code == _lib.IKF_OK, _lib.last_error(eng.lib)
    torch.cuda.synchronize()
    before, unwritten, after = torch.stack([(buf[:front] != SENTINEL).sum(), (rows == SENTINEL).sum(),
                                            (buf[front + n * ndof:] != SENTINEL).sum()]).tolist()
    assert before == 0, f"n={n}: {before} words in front of row 0 were written"
    assert after == 0, f"n={n}: {after} words behind row n - 1 were written"
    assert unwritten == 0, f"n={n}: {unwritten} elements of rows 0 .. n - 1 were never written"
    return rows.view(torch.float32).view(n, ndof)


# ---- forcing a launch form ---------------------------------------------------------------------------------------------------------------
FORMS = {"perlayer": (180, 185), "rowowner": (182,), "cluster": (187,), "cluster-epoch": (187, 192), "cluster-tagged": (187, 193),
         "cluster-spread": (187, 189), "entry-off": (110,), "entry-forced": (112,), "rows16-off": (150,),
         "cluster-off": (185,), "rowowner-off": (180, 187)}   # (the last two: the plan-seam test's other planner settings; without the row-owner
#                                                               launch the planner keeps the cluster form only where it is asked for: 187)
FORMS.update({f"tile{c}": (101 + c,) for c in (0, 1, 2, 3, 4, 6)})
FORMS.update({f"unfused{v}": (v,) for v in range(9)})
# (the give-up hooks 188 and 191 are not here on purpose: the repair path has its own tests in tests/test_gpu_parity.py)


@contextlib.contextmanager
def force(eng, *forms):
    """Sets the ikf_set_gemm_variant codes (or the precision) of the named forms, in the order given, and puts the handle's defaults back on
    the way out, also when the body fails: 181, 186, 111, -1, precision f32 - and the switches a named form may have moved beside them:
    tagged hand-over (193), 16-row tiles (151), XCD-local placement (190, where the handle had it)."""
    was_local = eng.cluster_local
    try:
        for form in forms:
            if form == "f16x3":
                eng.set_precision("f16x3")
            else:
                for code in FORMS[form]:
                    eng.set_gemm_variant(code)
        yield eng
    finally:
        for code in (181, 186, 111, -1, 193, 151):
            eng.set_gemm_variant(code)
        if was_local and not eng.cluster_local:
            eng.set_gemm_variant(190)
        eng.set_precision("f32")


def parse_plan(text):
    """"rowowner:4096 cluster16:200" -> [("rowowner", 0, 4096), ("cluster16", 4096, 200)]: (form, first row, rows)."""
    out, r0 = [], 0
    for part in text.split():
        form, rows = part.split(":")
        out.append((form, r0, int(rows)))
        r0 += int(rows)
    return out


def form_class(form):
    return "cluster" if form.startswith("cluster") else form
