"""What tests/test_flow_sample.py, tests/test_flow_sample_tiled.py (GPU) and tests/test_flow_sample_inputs.py,
tests/test_flow_sample_tiled_inputs.py (CPU) share: the models, transforms, inputs and fp64 references of the sampling-pass tests, the guarded
raw calls, the pose sources of the tiled tests and the switch that forces one launch form.

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
def _guarded_rows(eng, Z, stream, shift, call):
    """The frame of guarded_approx and guarded_tiled: `call(n, rows pointer, stream pointer)` is the raw C-ABI call and returns its status."""
    n, ndof = Z.shape[0], eng.layout.ndof
    front = shift + GUARD * ndof
    buf = torch.full((front + (n + GUARD) * ndof,), SENTINEL, dtype=torch.int32, device=Z.device)
    rows = buf[front: front + n * ndof]
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(Z.device))   # (the fill above ran on the current stream)
    s = C.c_void_p((torch.cuda.current_stream(Z.device) if stream is None else stream).cuda_stream)
    code = call(n, rows.data_ptr(), s)
    assert code == _lib.IKF_OK, _lib.last_error(eng.lib)
    torch.cuda.synchronize()
    before, unwritten, after = torch.stack([(buf[:front] != SENTINEL).sum(), (rows == SENTINEL).sum(),
                                            (buf[front + n * ndof:] != SENTINEL).sum()]).tolist()
    assert before == 0, f"n={n}: {before} words in front of row 0 were written"
    assert after == 0, f"n={n}: {after} words behind row n - 1 were written"
    assert unwritten == 0, f"n={n}: {unwritten} elements of rows 0 .. n - 1 were never written"
    return rows.view(torch.float32).view(n, ndof)


def guarded_approx(eng, P, Z, clamp, soft=0.0, broadcast=False, stream=None, shift=0):
    """ikf_generate_approx through the raw C-ABI into an int32 buffer of (GUARD + n + GUARD) x ndof words filled with SENTINEL (with `shift`
    further words in front: shift = 1 makes the output pointer 4-byte aligned only); the pointer passed is that of row GUARD.  Both guard
    bands must come back bit-unchanged, and no element of rows 0 .. n - 1 may still hold the sentinel - a NaN payload no kernel produces, so
    a hit is an element nobody wrote.  Returns the n rows as float32."""
    return _guarded_rows(eng, Z, stream, shift, lambda n, rows, s: eng.lib.ikf_generate_approx(
        eng._h, P.data_ptr(), 1 if broadcast else 0, Z.data_ptr(), n, 1 if clamp else 0, float(soft), rows, s))


def guarded_tiled(eng, P, idx, n_mod, Z, clamp, soft=0.0, stream=None):
    """The twin of guarded_approx for ikf_generate_approx_tiled (include/ikflow_amd_debug.h): the pose of row r is P[idx[r % n_mod]], or
    P[r % n_mod] without a list (idx: device int32 [n_mod], or None).  Same sentinel, same guard bands, same three assertions."""
    assert idx is None or (idx.dtype == torch.int32 and idx.is_contiguous() and idx.device == Z.device)
    return _guarded_rows(eng, Z, stream, 0, lambda n, rows, s: eng.lib.ikf_generate_approx_tiled(
        eng._h, P.data_ptr(), None if idx is None else idx.data_ptr(), int(n_mod), Z.data_ptr(), n, 1 if clamp else 0, float(soft), rows, s))


# ---- the tiling pose source (tests/test_flow_sample_tiled.py) ----------------------------------------------------------------------------------
# The pose table is always the model's whole pool (device_inputs: POOL rows, at least n); a list points anywhere into it.
LIST_SEED = 43
LIST_KINDS = ("scatter", "compacted")


@functools.lru_cache(maxsize=None)
def pose_list(kind, n_mod, pool):
    """The index list of a pose source, a function of (kind, n_mod, pool) only, int32 [n_mod], read-only; None for kind None.
    "scatter": n_mod draws with replacement from range(pool), entry 0 forced to pool - 1 and (n_mod >= 2) the last entry to 0: not monotone,
    both ends of the table, and with n_mod == 1 a single entry that is not 0.  "compacted": an ascending subset without repeats, the shape
    launch_compact_invalid produces."""
    if kind is None:
        return None
    rng = np.random.default_rng([LIST_SEED, LIST_KINDS.index(kind), n_mod, pool])
    if kind == "scatter":
        idx = rng.integers(0, pool, size=n_mod)
        idx[0] = pool - 1
        if n_mod >= 2:
            idx[-1] = 0
    else:
        idx = np.sort(rng.choice(pool, size=n_mod, replace=False))
    idx = idx.astype(np.int32)
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def device_pose_list(kind, n_mod, pool):
    idx = pose_list(kind, n_mod, pool)
    return None if idx is None else torch.from_numpy(idx.copy()).to(DEV)


def source_rows(n_mod, kind, pool, n):
    """int64 [n]: the row of the pose table that row r of a call reads under the source (n_mod, kind)."""
    pm = np.arange(n, dtype=np.int64) % n_mod
    idx = pose_list(kind, n_mod, pool)
    return pm if idx is None else idx.astype(np.int64)[pm]


def gathered(P, idx, n_mod, n):
    """The n pose rows P[idx[r % n_mod]] (P[r % n_mod] without a list), by integer indexing only: what the batch form is given."""
    pm = torch.arange(n, device=P.device) % n_mod
    return (P[pm] if idx is None else P[idx.long()[pm]]).contiguous()


def SOURCES(n):
    """[(n_mod, list kind)]: the pose sources a call of n rows is run under - n_mod in {1, 2, 3, 15, 16, 17, 61, n - 1, n} within [1, n], each
    without a list, scattered and compacted, and one list longer than the call (n + 5 entries, only the first n read)."""
    mods = sorted({m for m in (1, 2, 3, 15, 16, 17, 61, n - 1, n) if 1 <= m <= n})
    return [(m, kind) for m in mods for kind in (None,) + LIST_KINDS] + [(n + 5, "scatter")]


# (a) of tests/test_flow_sample_tiled.py: (forms, models, sizes, plan must contain) - R runs the per-layer forms with "perlayer" in front
TILED_ROWOWNER_N = (1, 17, 4097)
TILED_CLUSTER_N = (17, 129, 257, 513, 1025, 2048)      # every member count G = 32, 16, 8, 4, 2 (two sizes at G = 2)
TILED_PERLAYER_N = (1, 17, 33, 129, 513, 2049)         # the 16-row head, the 32-row head and k_subnet_entry
ROWOWNER_LAUNCH_ROWS = 1 << 24                          # rows of one row-owner launch (kMaxLaunchRows, api_flow.hip)
PER_LAYER_CHUNK = 16384                                 # rows of the per-layer kernels' scratch up to width 1024 (chunk_cap, api_handle.hip)
TILED_CHUNK_N = (16385,)                               # T: the last chunk of the per-layer chunk loop starts at a non-zero row0
TILED_TILE_N = (33, 300)
TILED_UNFUSED_N = (100, 700)
TILED_F16X3_N = (257, 2049)
TILED_TILE_FORMS = ("tile0", "tile1", "tile2", "tile3", "tile4", "tile6", "entry-off", "entry-forced", "rows16-off")
# (b): the seam sizes and their sources
TILED_SEAM_N = (600, 2304, 4096 + 200, 2 * 4096 + 2049)


def seam_sources(n):
    mods = [m for m in (1, 7, 1000, 4097, n - 1) if m < 4097 or n >= 4097]
    out = [(m, kind) for m in mods for kind in (None, "scatter")]
    return out + ([(4096, None)] if n == 4096 + 200 else [])   # row 4096 + j wraps to pose j


# (c): per model the sizes whose rows are compared with fp64 (the largest n of every row of (a)'s table), under three sources each
TILED_REF_N = {"R": (4097, 2048, 2049, 300), "R10": (4097,), "T": (2049, 16385, 300, 700), "T300": (2049,), "T1": (700,)}


def ref_sources(n):
    return [(17, "scatter"), (n - 1, None), (1, "scatter")]


def _tiled_sets():
    """{(model, n_mod, list kind): rows}: every tiled input a GPU test compares with the oracle (plain transform, weights A, softflow 0).  A list
    is a function of (n_mod, POOL), so the rows of a smaller n under the same source are the leading rows of the largest."""
    sets = {}
    for name, sizes in TILED_REF_N.items():
        for n in sizes:
            for key in ref_sources(n):
                sets[(name,) + key] = max(sets.get((name,) + key, 0), n)
    return sets


TILED_SETS = _tiled_sets()
# (d): (poses m, candidates k) of the ikf_generate_ranked comparison - a call of k * m rows under (n_mod = m, no list); (e): the edge tests' call
TILED_RANKED = ((1, 16), (5, 3), (65, 16), (257, 16))
TILED_EDGE = (333, 61, "scatter")


def tiled_cases():
    """{(model, n, n_mod, list kind)}: every call the GPU tests of tests/test_flow_sample_tiled.py make."""
    table = [(("R", "R10"), TILED_ROWOWNER_N), (("R",), TILED_CLUSTER_N), (("R", "T", "T300"), TILED_PERLAYER_N), (("T",), TILED_CHUNK_N),
             (("T", "R"), TILED_TILE_N), (("T", "T1"), TILED_UNFUSED_N), (("T", "R"), TILED_F16X3_N)]
    cases = {(name, n) + src for names, sizes in table for name in names for n in sizes for src in SOURCES(n)}
    cases |= {("R", n) + src for n in TILED_SEAM_N for src in seam_sources(n)}
    cases |= {(name, n) + src for name, sizes in TILED_REF_N.items() for n in sizes for src in ref_sources(n)}
    cases |= {("R", k * m, m, None) for m, k in TILED_RANKED}
    cases |= {(name,) + TILED_EDGE for name in ("R", "T")}
    return cases


def tiled_conditional(name, n_mod, kind, n, soft=0.0):
    lay = model(name)[2]
    c = inputs(name)[1].numpy().astype(np.float64)[source_rows(n_mod, kind, POOL[name], n)]
    return np.concatenate([c, np.full((n, 1), soft)], 1) if lay.dim_cond == 8 else c


@functools.lru_cache(maxsize=None)
def reference_tiled(name, n_mod, kind):
    """fp64 oracle on the gathered conditional, unclamped, [TILED_SETS[key] x ndof]: computed once, sliced by the tests, never changed."""
    n = TILED_SETS[(name, n_mod, kind)]
    robot, hp, lay, sd = model(name)
    ref = fo.run_inference_f64(sd, lay, robot, inputs(name)[0][:n].numpy().astype(np.float64), tiled_conditional(name, n_mod, kind, n), False)
    ref.setflags(write=False)
    return ref


def reference_tiled_f32(name, n_mod, kind):
    n = TILED_SETS[(name, n_mod, kind)]
    robot, hp, lay, sd = model(name)
    cond = torch.from_numpy(tiled_conditional(name, n_mod, kind, n).astype(np.float32))
    return fo.run_inference_torch(sd, lay, robot, inputs(name)[0][:n], cond, False).numpy()


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
