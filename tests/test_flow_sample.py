"""The sampling pass: ikf_generate_approx through the raw C-ABI, every launch form it can be cut into.

The call the benchmark headline times and every higher feature sits on.  A batch is cut by plan_rows into chunks, each run by one of six forms
(fused per-layer kernels in several tile configurations with their 32- and 16-row small-batch heads, the unfused four-kernel pipeline, the
row-owner launch, the cluster form with 32 .. 2 members in its epoch / tagged and spread / XCD-local variants, the f16x3 contractions, mixed
plans).  tests/test_gpu_parity.py compares their values with the oracle; what it cannot see is closed here:
  1. stray stores: every call writes into a buffer with 64 rows of a NaN sentinel on either side (sample_helpers.guarded_approx), on both sides
     of every tile edge of every form;
  2. plan seams: every multi-chunk plan against its chunks run alone under their own form, bit for bit, and every row written;
  3. the exit transform (x - b).mm(M_inv), [:, :ndof], clamp - four separate copies - with a dense non-symmetric M_inv, b != 0, a deleted b and
     permutation tables other than the seeded ones;
  4. a row's result does not depend on its place in the batch or on the batch size, within a form;
  5. reload on a live handle refreshes every weight image;
  6. pointers that are 4-byte aligned only, a non-default stream.
Values: sample_helpers.reference (fp64, oracle.flow_oracle.run_inference_f64) on every row, FLOW_TOL = 1e-5 relative to max(1, |x|).  The inputs'
own conditions are checked without a GPU in tests/test_flow_sample_inputs.py.  Every call here uses the batch or the single-pose source; the
tiling pose source of exact and ranked IK (n_mod below the rows, an index list) has the sibling tests/test_flow_sample_tiled.py.  No test here uses the give-up hooks (188 / 191), and every
test that runs a cluster form requires ikf_cluster_repairs unchanged: a repaired call must not pass for a cluster result."""
import contextlib

import numpy as np
import pytest
import torch

import sample_helpers as sh
from sample_helpers import DEV, FLOW_TOL, force, guarded_approx

pytestmark = pytest.mark.gpu
RT_TOL = 3e-5   # forward(inverse(z)) = z on the device: the round-trip bound of tests/test_flow_forward.py and tests/test_flow_inverse.py

ROWOWNER_N = (1, 15, 16, 17, 31, 33, 4095, 4096, 4097, 4096 + 17)
CLUSTER_N = (1, 16, 17, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048)   # both ends of every G range
PERLAYER_N = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)
CHUNK_N = (16383, 16384, 16385)   # T only: the per-layer chunk loop
TILE_N = (1, 33, 100, 129, 300, 700)
UNFUSED_N = (1, 100, 129, 700)
F16X3_N = (1, 255, 256, 257, 511, 512, 513, 1024, 1025, 2048, 2049, 2100)   # 32x32 and 32x64 small-batch kernels, configurations 3, 2, 1, the DMA form


def _eng(name, transform="plain", weights="A"):
    return sh.shared_solver(name, transform, weights).engine(DEV)


@contextlib.contextmanager
def _no_cluster_repair(eng):
    before = eng.cluster_repairs
    yield
    torch.cuda.synchronize()
    assert eng.cluster_repairs == before, "a cluster launch gave up and was repaired by the row-owner launch: not a cluster result"


def _cluster_variants(eng):
    """Every variant the device accepts: spread placement always, the XCD-local default only where the handle has it."""
    variants = [("cluster-spread",), ("cluster-epoch", "cluster-spread")]
    if eng.cluster_local:
        variants += [("cluster-tagged",), ("cluster-epoch",)]
    return variants


def _clamped(q, name):
    lo, hi = sh.limits(name, q.device)
    return torch.minimum(torch.maximum(q, lo), hi)


def _guarded_sweep(name, forms, sizes, tag, want_plan=None):
    """Every n of `sizes` under `forms`: clamp off and on, per-row pose and broadcast pose, softflow 0 and SOFT (8-entry conditional), each call
    guarded; unclamped against fp64 on every row, clamped = min(max(unclamped, lo), hi) bit for bit.  Returns the largest relative error."""
    eng = _eng(name)
    Z, P = sh.device_inputs(name)
    worst = 0.0
    with force(eng, *forms):
        for soft in ((0.0, sh.SOFT) if eng.layout.dim_cond == 8 else (0.0,)):
            for broadcast in (False, True):
                ref = sh.reference(name, "plain", "A", soft, broadcast)
                for n in sizes:
                    if want_plan is not None:
                        assert want_plan in eng.plan(n), (n, eng.plan(n))
                    Pn = P[sh.BROADCAST_ROW] if broadcast else P[:n]
                    q = guarded_approx(eng, Pn, Z[:n], False, soft, broadcast)
                    qc = guarded_approx(eng, Pn, Z[:n], True, soft, broadcast)
                    err = sh.rel_err(q, ref[:n])
                    assert err <= FLOW_TOL, f"{tag} n={n} soft={soft} broadcast={broadcast}: {err:.2e} from fp64"
                    assert torch.equal(qc, _clamped(q, name)), f"{tag} n={n} soft={soft} broadcast={broadcast}: clamped rows"
                    worst = max(worst, err)
    print(f"[sample] {tag}: n = {sizes[0]} .. {sizes[-1]}, largest relative error against fp64 {worst:.2e}")
    return worst


# ---- 1. guarded stores, every form, both sides of every tile edge -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["R", "R10", "R8", "Rpad", "Rsig"])
def test_rowowner_writes_n_rows_and_nothing_else(name):
    """k_flow_rowowner, a workgroup per 16 rows: both sides of the tile, of a round of workgroups, and a ragged tile behind a full round."""
    _guarded_sweep(name, ("rowowner",), ROWOWNER_N, f"rowowner {name}", want_plan="rowowner")


@pytest.mark.parametrize("name", ["R", "R10", "Rsig"])
def test_cluster_writes_n_rows_and_nothing_else(name):
    """k_flow_cluster<G>, G = 32 .. 2, and the conditional repair launch queued behind it over the same rows: both ends of every G range,
    tagged and epoch-word hand-over, spread and (where the device groups workgroups by XCD) XCD-local placement."""
    eng = _eng(name)
    with _no_cluster_repair(eng):
        for variant in _cluster_variants(eng):
            _guarded_sweep(name, variant, CLUSTER_N, f"{'+'.join(variant)} {name}", want_plan="cluster")


@pytest.mark.parametrize("name", ["R", "T", "T300"])
def test_per_layer_kernels_write_n_rows_and_nothing_else(name):
    """The fused per-layer kernels by batch size (forced on the released width, the default elsewhere): 16- and 32-row heads, 32 / 64 / 128-row
    tiles, the finalize kernel's 32-row blocks; on T also the 16384-row chunk loop."""
    sizes = PERLAYER_N + (CHUNK_N if name == "T" else ())
    _guarded_sweep(name, ("perlayer",) if name == "R" else (), sizes, f"perlayer {name}", want_plan="perlayer")


@pytest.mark.parametrize("form", ["tile0", "tile1", "tile2", "tile3", "tile4", "tile6", "entry-off", "entry-forced", "rows16-off"])
@pytest.mark.parametrize("name", ["T", "R"])
def test_forced_tiles_and_heads_write_n_rows_and_nothing_else(name, form):
    _guarded_sweep(name, ("perlayer", form) if name == "R" else (form,), TILE_N, f"{form} {name}", want_plan="perlayer")


@pytest.mark.parametrize("name,form", [("T", f"unfused{v}") for v in range(9)] + [("T1", None)] + [("T1", f"unfused{v}") for v in range(9)])
def test_unfused_pipeline_writes_n_rows_and_nothing_else(name, form):
    """flow_kernels.hip: every contraction variant, and the one-hidden-layer model that takes this pipeline by itself."""
    _guarded_sweep(name, () if form is None else (form,), UNFUSED_N, f"{form or 'unfused by default'} {name}", want_plan="perlayer")


@pytest.mark.parametrize("name", ["T", "R"])
def test_f16x3_contractions_write_n_rows_and_nothing_else(name):
    eng = _eng(name)
    assert eng.split_fallback_count == 0
    _guarded_sweep(name, ("f16x3", "perlayer") if name == "R" else ("f16x3",), F16X3_N, f"f16x3 {name}", want_plan="perlayer")
    assert eng.split_fallback_count == 0, "an f32 re-run is not an f16x3 result"


# ---- 2. plan seams ---------------------------------------------------------------------------------------------------------------------------
SEAM_N = (600, 1536, 2304, 2560, 3072, 513, 1025, 2049, 4097, 4096 + 200, 4096 + 513, 2 * 4096 + 2049)


def _pairs(chunks):
    forms = [sh.form_class(c[0]) for c in chunks]
    return set(zip(forms, forms[1:]))


@pytest.mark.parametrize("setting", ["default", "cluster-off", "rowowner-off"])
def test_every_chunk_of_a_plan_is_its_form_run_alone_on_those_rows(setting):
    """R: the planner's own chunks (eng.plan: nothing here knows a CU count), default settings, cluster form off (185) and row-owner launch off
    (180 + 187: whole cluster2 launches peeled off in plan_rows).  One guarded call over the whole batch - every row written, none beside them, right
    against fp64 - then each chunk's rows alone under the form that ran them: bit for bit the rows of the whole call, so every form took its
    latent, pose and output offsets from the chunk's first row.  Per-row pose and broadcast pose."""
    name = "R"
    eng = _eng(name)
    Z, P = sh.device_inputs(name)
    base = () if setting == "default" else (setting,)
    with force(eng, *base):
        plans = {n: sh.parse_plan(eng.plan(n)) for n in SEAM_N}
        # every pair of neighbouring forms the planner can produce under this setting (any n up to three rounds of the largest plan's first chunk)
        possible = set()
        for n in range(1, 3 * 4096 + 1):
            possible |= _pairs(sh.parse_plan(eng.plan(n)))
    seen = set().union(*[_pairs(c) for c in plans.values()])
    print(f"[sample] seams {setting}: " + "; ".join(f"{n}: {' '.join(f'{f}:{r}' for f, _, r in plans[n])}" for n in SEAM_N))
    assert possible and possible <= seen, f"{setting}: the sizes reach the seams {sorted(seen)} of {sorted(possible)}"
    for n in SEAM_N:
        if setting == "default":   # (the other settings leave the sizes below a round, or below a forced cluster launch, in one chunk)
            assert len(plans[n]) >= 2, (setting, n, plans[n])
        assert sum(r for _, _, r in plans[n]) == n
    assert sum(len(c) >= 2 for c in plans.values()) >= 4, plans
    worst = 0.0
    with _no_cluster_repair(eng):
        for broadcast in (False, True):
            ref = sh.reference(name, "plain", "A", 0.0, broadcast)
            for n in SEAM_N:
                Pn = P[sh.BROADCAST_ROW] if broadcast else P[:n]
                with force(eng, *base):
                    assert sh.parse_plan(eng.plan(n)) == plans[n]
                    whole = guarded_approx(eng, Pn, Z[:n], False, 0.0, broadcast).clone()
                err = sh.rel_err(whole, ref[:n])
                assert err <= FLOW_TOL, f"{setting} n={n} broadcast={broadcast}: {err:.2e} from fp64"
                worst = max(worst, err)
                for form, r0, rows in plans[n]:
                    with force(eng, sh.form_class(form)):
                        assert eng.plan(rows) == f"{form}:{rows}", (form, rows, eng.plan(rows))
                        alone = guarded_approx(eng, Pn if broadcast else P[r0:r0 + rows], Z[r0:r0 + rows], False, 0.0, broadcast)
                    assert torch.equal(alone, whole[r0:r0 + rows]), f"{setting} n={n} broadcast={broadcast}: chunk {form}:{rows} at row {r0}"
    print(f"[sample] seams {setting}: largest relative error against fp64 {worst:.2e}")


# ---- 3. exit transform and permutations, every form -----------------------------------------------------------------------------------------
def _exit_forms(name, eng):
    """(forms, n, plan must contain) per model: every copy of the exit - k_flow_finalize (fused per-layer, f16x3), k_last_layer_coupling (unfused),
    the row-owner exit, the cluster exit at one n per member count - and the default plan at 4096 + 200."""
    out = []
    if name in ("R", "R10"):
        out += [(("rowowner",), 700, "rowowner")]
        out += [(("cluster",), n, f"cluster{g}:") for n, g in ((100, 32), (200, 16), (400, 8), (900, 4), (2000, 2))]
        out += [(("perlayer",), 700, "perlayer"), (("perlayer", "unfused4"), 700, "perlayer"), (("f16x3", "perlayer"), 700, "perlayer")]
    elif name == "T":
        out += [((), 700, "perlayer"), (("unfused4",), 700, "perlayer"), (("f16x3",), 700, "perlayer")]
    else:
        out += [((), 700, "perlayer"), (("unfused4",), 700, "perlayer")]
    return out + [((), 4096 + 200, "")]


@pytest.mark.parametrize("transform", sh.EXIT_TRANSFORMS)
@pytest.mark.parametrize("name", ["R", "R10", "T", "T1"])
def test_exit_transform_and_permutations_under_every_form(name, transform):
    """dense: a dense non-symmetric M_inv with b != 0 (M given / absent); bias: b != 0 alone; no-b: the key deleted; perm: permutation tables
    other than PermuteRandom's seeded ones; all: together.  Unclamped against fp64 on every row; clamped: the clamp applies after the transform,
    to the sliced columns - min(max(unclamped, lo), hi) bit for bit.  Where ndof = D (R) the rows also go back through ikf_flow_forward, whose
    row-owner table folds the next block's forward permutation into each subnet entry: forward(sample(z)) = z."""
    robot, hp, lay, sd = sh.model(name, transform)
    if transform in ("dense", "dense-noM", "all"):
        assert abs(np.linalg.slogdet(np.asarray(sd["module_list.0.M_inv"], dtype=np.float64))[1]) > 1.0   # far from diagonal
    eng = _eng(name, transform)
    Z, P = sh.device_inputs(name)
    ref = sh.reference(name, transform, "A", 0.0, False)
    lo, hi = (t.double().numpy() for t in sh.limits(name))
    worst, cluster_counts = 0.0, set()
    with _no_cluster_repair(eng):
        for forms, n, want in _exit_forms(name, eng):
            with force(eng, *forms):
                plan = eng.plan(n)
                if want.startswith("cluster"):
                    assert "cluster" in plan   # (the member count follows the CU count: one n per G on a 256-CU chip)
                    cluster_counts.add(plan.split(":")[0])
                else:
                    assert want in plan, (forms, n, plan)
                q = guarded_approx(eng, P[:n], Z[:n], False)
                qc = guarded_approx(eng, P[:n], Z[:n], True)
                if lay.ndof == lay.dim and forms == ("rowowner",):
                    back = eng.flow_forward(q, P[:n])[0]
            tag = f"{name} {transform} {'+'.join(forms) or 'default'} n={n} ({plan})"
            err, err_c = sh.rel_err(q, ref[:n]), sh.rel_err(qc, np.clip(ref[:n], lo, hi))
            assert err <= FLOW_TOL and err_c <= FLOW_TOL, f"{tag}: {err:.2e} unclamped, {err_c:.2e} clamped from fp64"
            assert torch.equal(qc, _clamped(q, name)), f"{tag}: the clamp is not min(max(q, lo), hi) of the transformed, sliced columns"
            assert not torch.equal(qc, q), f"{tag}: no element was clamped - the clamped call shows nothing"
            if lay.ndof == lay.dim and forms == ("rowowner",):
                rt = float((back - Z[:n]).abs().max())
                assert rt <= RT_TOL, f"{tag}: forward(sample(z)) differs from z by {rt:.2e}"
            worst = max(worst, err)
    if name in ("R", "R10"):
        assert len(cluster_counts) == 5, cluster_counts
    print(f"[sample] exit {name} {transform}: largest relative error against fp64 {worst:.2e}")


# ---- 4. position and batch-size independence within a form ---------------------------------------------------------------------------------
def _with_copies_of_row_0(name, n_long):
    """The first n_long rows of the pool with row 0 copied to a row of the next 16-row tile, of another wave's rows, of the far half and to the last."""
    Z, P = (t[:n_long].clone() for t in sh.device_inputs(name))
    copies = sorted({r for r in (17, 70, n_long // 2 + 3, n_long - 1) if 0 < r < n_long})
    for r in copies:
        Z[r], P[r] = Z[0], P[0]
    return Z, P, copies


def _independence(eng, name, sizes, tag):
    """The longest n of `sizes`: row 0's copies give row 0's bits; every shorter n gives the bits of the leading rows."""
    n_long = max(sizes)
    Z, P, copies = _with_copies_of_row_0(name, n_long)
    long = guarded_approx(eng, P, Z, False).clone()
    for r in copies:
        assert torch.equal(long[r], long[0]), f"{tag}: row 0 copied to row {r} of {n_long} gives other bits"
    for n in sizes:
        if n != n_long:
            assert torch.equal(guarded_approx(eng, P[:n], Z[:n], False), long[:n]), f"{tag}: n={n} against the leading rows of n={n_long}"


@pytest.mark.parametrize("name,forms,sizes", [
    ("R", ("rowowner",), ROWOWNER_N), ("R", ("perlayer", "tile0"), PERLAYER_N), ("T", ("tile0",), PERLAYER_N + CHUNK_N),
    ("R", ("perlayer", "tile6"), PERLAYER_N), ("T", ("unfused4",), UNFUSED_N + (2049,)), ("R", ("perlayer", "unfused4"), UNFUSED_N + (2049,))],
    ids=lambda v: v if isinstance(v, str) else "+".join(v) if isinstance(v[0], str) else f"upto{max(v)}")
def test_a_row_does_not_depend_on_its_place_or_on_the_batch_size(name, forms, sizes):
    eng = _eng(name)
    with force(eng, *forms):
        _independence(eng, name, sizes, f"{name} {'+'.join(forms)}")


def _by_plan_key(sizes, key):
    groups = {}
    for n in sizes:
        groups.setdefault(key(n), []).append(n)
    return groups


def test_a_row_does_not_depend_on_its_place_or_on_the_batch_size_within_a_cluster_member_count():
    """The member count G changes with n, and with it the summation order: bit equality holds within a G range (across ranges the oracle is
    the standard, test 1)."""
    name = "R"
    eng = _eng(name)
    with _no_cluster_repair(eng):
        for variant in _cluster_variants(eng):
            with force(eng, *variant):
                groups = _by_plan_key(CLUSTER_N, lambda n: eng.plan(n).split(":")[0])
                assert len(groups) == 5 and all(g.startswith("cluster") for g in groups), groups
                for g, sizes in groups.items():
                    _independence(eng, name, sizes, f"{'+'.join(variant)} {g}")


@pytest.mark.parametrize("name", ["R", "T"])
def test_a_row_does_not_depend_on_its_place_or_on_the_batch_size_within_an_f16x3_kernel(name):
    """f16x3 picks its contraction kernel by n (up to 128 rows the 16-row f32 kernels step in, on 16x16 tiles up to 64 rows and 16x32 above;
    32x32 tiles up to 256, 32x64 up to 512, configurations 3 / 2 / 1 up to 1024 / 2048, the DMA form above), and the kernels sum the last
    Linear's partial sums in slots of their own width: bit equality holds within a kernel's range."""
    eng = _eng(name)
    edges = (64, 128, 256, 512, 1024, 2048)
    with force(eng, *(("f16x3", "perlayer") if name == "R" else ("f16x3",))):
        for kernel, sizes in _by_plan_key(F16X3_N + (17, 64, 65, 100, 128, 129), lambda n: sum(n > e for e in edges)).items():
            _independence(eng, name, sizes, f"{name} f16x3 range {kernel}")
    assert eng.split_fallback_count == 0


# ---- 5. reload on one handle, every image ---------------------------------------------------------------------------------------------------
RELOAD_N = (5, 200, 512, 700, 4096 + 200)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("name", ["R", "T"])
def test_reload_refreshes_every_weight_image_of_the_sampling_pass(name, precision):
    """load A, call; load B (other weights at gain 2.0, shuffled permutations, a dense M_inv with bias) on the same handle, call: bit-identical
    to a fresh handle loaded with B and right against fp64; load A again: bit-identical to the first run.  Default plan at five sizes, on R
    also every forced form: the row-major image, the fragment-major small-batch image (built lazily), the row-owner stream the cluster form
    shares, and - the handle in f16x3 mode throughout - the split-32 images."""
    A, B = sh.model(name, "plain", "A"), sh.model(name, "all", "B")
    Z, P = sh.device_inputs(name)
    runs = [((), n) for n in RELOAD_N]
    if name == "R" and precision == "f32":
        runs += [(forms, n) for forms in (("rowowner",), ("perlayer",), ("perlayer", "unfused4")) for n in RELOAD_N]
        runs += [(("cluster",), n) for n in RELOAD_N if n <= 2048]

    def sweep(eng):
        out = []
        for forms, n in runs:
            with (force(eng, *forms) if forms else contextlib.nullcontext()):
                out.append(guarded_approx(eng, P[:n], Z[:n], False).clone())
        assert eng.precision == precision
        return out

    s = sh.new_solver(A, precision)
    eng = s.engine(DEV)
    with _no_cluster_repair(eng):
        first = sweep(eng)
        s.load_state_dict_tensors(B[3])
        second = sweep(eng)
        fresh = sweep(sh.new_solver(B, precision).engine(DEV))
        s.load_state_dict_tensors(A[3])
        third = sweep(eng)
    ref_a, ref_b = sh.reference(name, "plain", "A", 0.0, False), sh.reference(name, "all", "B", 0.0, False)
    worst = 0.0
    for (forms, n), a, b, f, a2 in zip(runs, first, second, fresh, third):
        tag = f"{name} {precision} {'+'.join(forms) or 'default'} n={n}"
        assert torch.equal(b, f), f"{tag}: after loading B the handle differs from a fresh handle loaded with B"
        assert torch.equal(a2, a), f"{tag}: after loading A again the handle differs from its first run"
        err_a, err_b = sh.rel_err(a, ref_a[:n]), sh.rel_err(b, ref_b[:n])
        assert err_a <= FLOW_TOL and err_b <= FLOW_TOL, f"{tag}: {err_a:.2e} (A), {err_b:.2e} (B) from fp64"
        worst = max(worst, err_a, err_b)
    assert eng.split_fallback_count == 0
    print(f"[sample] reload {name} {precision}: {len(runs)} calls per load, largest relative error against fp64 {worst:.2e}")


# ---- 6. input forms ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forms", [("rowowner",), ("cluster",), ("perlayer",), ("f16x3", "perlayer")], ids="+".join)
def test_pointers_aligned_to_4_bytes_only_and_a_non_default_stream(forms):
    """latent and poses as views that start one row (28 bytes) into a larger allocation, an output pointer one word into its allocation, a
    non-default stream - one at a time and together: the bits of the aligned call on the current stream."""
    name = "R"
    eng = _eng(name)
    n = 333
    Z, P = (t[:n] for t in sh.device_inputs(name))
    Zbig, Pbig = torch.empty((n + 1, Z.shape[1]), device=DEV), torch.empty((n + 1, 7), device=DEV)
    Zbig[1:], Pbig[1:] = Z, P
    Zv, Pv = Zbig[1:], Pbig[1:]
    assert Zv.is_contiguous() and Pv.is_contiguous() and Zv.data_ptr() % 8 == 4 and Pv.data_ptr() % 8 == 4 and Z.data_ptr() % 16 == 0
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with _no_cluster_repair(eng), force(eng, *forms):
        for clamp, broadcast in ((False, False), (True, False), (False, True)):
            pose = lambda t: t[sh.BROADCAST_ROW] if broadcast else t
            want = guarded_approx(eng, pose(P), Z, clamp, 0.0, broadcast).clone()
            got = {"latent and poses one row in": guarded_approx(eng, pose(Pv), Zv, clamp, 0.0, broadcast),
                   "output one word in": guarded_approx(eng, pose(P), Z, clamp, 0.0, broadcast, shift=1),
                   "side stream": guarded_approx(eng, pose(P), Z, clamp, 0.0, broadcast, stream=side),
                   "all three": guarded_approx(eng, pose(Pv), Zv, clamp, 0.0, broadcast, stream=side, shift=1)}
            for what, q in got.items():
                assert torch.equal(q, want), f"{'+'.join(forms)} clamp={clamp} broadcast={broadcast}: {what}"
            if not clamp:
                err = sh.rel_err(want, sh.reference(name, "plain", "A", 0.0, broadcast)[:n])
                assert err <= FLOW_TOL, err
