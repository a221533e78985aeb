"""The sampling pass under the TILING pose source: the pose of global row r is P[idx[r % n_mod]] (or P[r % n_mod]) with n_mod smaller than the
call - what exact IK (run_exact) and the candidate stage of ranked, path, diverse and refined IK (flow_candidates) hand to every flow kernel.

The index arithmetic exists in six hand-written copies (k_flow_rowowner, k_flow_cluster<G>, k_subnet_entry, the 32-row and the 16-row head of
the small-batch entry kernels, k_first_layer of the unfused pipeline), each taking row0 from another argument block.  tests/test_flow_sample.py
runs every form under the batch and the single-pose source only; here the debug entry ikf_generate_approx_tiled (include/ikflow_amd_debug.h)
runs the same path - flow_call, run_flow_guarded - under any source, and the flow rows themselves are observed:
  (a) every form, every source of sample_helpers.SOURCES(n), bit for bit against the batch form on the gathered poses (same kernel, same rows
      in the same places, same values: only the address the conditional is read from differs, so no tolerance is involved);
  (b) every call that is cut into pieces - the multi-chunk plans on R, the per-layer chunk loop on T, the row-owner launch split at 2^24 rows:
      one tiled call over the whole batch against the batch-form call on the gathered poses AND against every piece's rows run alone (the two
      entries share every kernel, so a copy that took its local row for the global one would be wrong in both alike);
  (c) against fp64 (sample_helpers.reference_tiled), so that the two entries cannot be wrong together;
  (d) ikf_generate_ranked's candidate rows are the entry's rows, bit for bit;
  (e) statuses and edges.
Every call is guarded (sample_helpers.guarded_tiled: 64 rows of a NaN sentinel either side); a test that runs a cluster form requires
ikf_cluster_repairs unchanged, an f16x3 test split_fallback_count unchanged.  The inputs' own conditions: tests/test_flow_sample_tiled_inputs.py."""
import ctypes as C

import pytest
import torch

import sample_helpers as sh
from ikflow_amd import _lib
from sample_helpers import DEV, FLOW_TOL, force, gathered, guarded_approx, guarded_tiled
from test_flow_sample import _cluster_variants, _eng, _no_cluster_repair

pytestmark = pytest.mark.gpu


def _source(name, n_mod, kind):
    return sh.device_pose_list(kind, n_mod, sh.POOL[name])


def _tiled_sweep(name, forms, sizes, tag, want_plan, sources=sh.SOURCES):
    """Every n of `sizes` under `forms`, every source of `sources(n)`, softflow 0 and SOFT (8-entry conditional), clamp alternating: the tiled
    call equals the batch-form call on the gathered poses, bit for bit.  Returns the number of (n, source) pairs compared."""
    eng = _eng(name)
    Z, P = sh.device_inputs(name)
    assert P.shape[0] == sh.POOL[name] >= max(sizes)
    compared = 0
    with force(eng, *forms):
        for n in sizes:
            assert want_plan in eng.plan(n), (n, eng.plan(n))
            for i, (n_mod, kind) in enumerate(sources(n)):
                idx = _source(name, n_mod, kind)
                Pg = gathered(P, idx, n_mod, n)
                for j, soft in enumerate((0.0, sh.SOFT) if eng.layout.dim_cond == 8 else (0.0,)):
                    clamp = (i + j) % 2 == 1
                    got = guarded_tiled(eng, P, idx, n_mod, Z[:n], clamp, soft)
                    want = guarded_approx(eng, Pg, Z[:n], clamp, soft)
                    assert torch.equal(got, want), (f"{tag} n={n} n_mod={n_mod} list={kind} soft={soft} clamp={clamp}: rows "
                                                    f"{(got != want).any(1).nonzero().flatten()[:8].tolist()} differ from the batch form on the gathered poses")
                compared += 1
    print(f"[tiled] {tag}: n = {', '.join(map(str, sizes))}: {compared} (n, source) pairs, bit-identical to the batch form")
    return compared


def _pieces(eng, n):
    """(form, first row, rows) of every launch sequence a call of n rows is cut into under the handle's current settings: the planner's chunks,
    a per-layer chunk further cut into pieces of the scratch's 16384 rows (the chunk loop)."""
    out = []
    for form, r0, rows in sh.parse_plan(eng.plan(n)):
        step = sh.PER_LAYER_CHUNK if form == "perlayer" else rows
        out += [(form, a, min(step, r0 + rows - a)) for a in range(r0, r0 + rows, step)]
    return out


def _tiled_sweep_by_pieces(name, base, sizes, tag, sources, alone_forms):
    """_tiled_sweep for calls that are cut into pieces.  The batch form on the gathered poses shares every kernel with the tiled call, so a copy
    that took its local row for the global one would be wrong in both alike: every piece's rows are therefore also run ALONE (first row 0, where
    local and global row are one) by the batch form under `alone_forms(form)` on that piece's gathered poses, and must be the whole call's rows
    bit for bit.  Returns the number of (n, source) pairs compared."""
    eng = _eng(name)
    Z, P = sh.device_inputs(name)
    compared = 0
    for n in sizes:
        with force(eng, *base):
            pieces = _pieces(eng, n)
        for i, (n_mod, kind) in enumerate(sources(n)):
            idx = _source(name, n_mod, kind)
            Pg = gathered(P, idx, n_mod, n)
            for j, soft in enumerate((0.0, sh.SOFT) if eng.layout.dim_cond == 8 else (0.0,)):
                clamp = (i + j) % 2 == 1
                what = f"{tag} n={n} n_mod={n_mod} list={kind} soft={soft} clamp={clamp}"
                with force(eng, *base):
                    got = guarded_tiled(eng, P, idx, n_mod, Z[:n], clamp, soft).clone()
                    want = guarded_approx(eng, Pg, Z[:n], clamp, soft)
                    assert torch.equal(got, want), f"{what}: rows {(got != want).any(1).nonzero().flatten()[:8].tolist()} differ from the batch form on the gathered poses"
                for form, r0, rows in pieces:
                    with force(eng, *alone_forms(form)):
                        assert eng.plan(rows) == f"{form}:{rows}", (form, rows, eng.plan(rows))
                        alone = guarded_approx(eng, Pg[r0:r0 + rows], Z[r0:r0 + rows], clamp, soft)
                    assert torch.equal(alone, got[r0:r0 + rows]), f"{what}: piece {form}:{rows} at row {r0} differs from those rows run alone"
            compared += 1
    print(f"[tiled] {tag}: n = {', '.join(map(str, sizes))}: {compared} (n, source) pairs, bit-identical to the batch form and to every piece run alone")
    return compared


# ---- (a) every form, every source, bit for bit against the batch form ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["R", "R10"])
def test_rowowner_reads_the_pose_of_every_source(name):
    _tiled_sweep(name, ("rowowner",), sh.TILED_ROWOWNER_N, f"rowowner {name}", "rowowner")


@pytest.mark.parametrize("n", sh.TILED_CLUSTER_N)
def test_cluster_reads_the_pose_of_every_source(n):
    """k_flow_cluster<G>: every member count (G = 32, 16, 8, 4 and two sizes at 2), every variant the device accepts."""
    eng = _eng("R")
    counts = set()
    with _no_cluster_repair(eng):
        for variant in _cluster_variants(eng):
            with force(eng, *variant):
                counts.add(eng.plan(n).split(":")[0])
            _tiled_sweep("R", variant, (n,), f"{'+'.join(variant)} R", "cluster")
    assert len(counts) == 1 and counts.pop().startswith("cluster"), counts


def test_the_cluster_sizes_reach_every_member_count():
    eng = _eng("R")
    with force(eng, "cluster-spread"):
        assert len({eng.plan(n).split(":")[0] for n in sh.TILED_CLUSTER_N}) == 5


@pytest.mark.parametrize("name", ["R", "T", "T300"])
def test_per_layer_kernels_read_the_pose_of_every_source(name):
    """The 16-row head, the 32-row head and k_subnet_entry (forced on the released width, the default elsewhere)."""
    _tiled_sweep(name, ("perlayer",) if name == "R" else (), sh.TILED_PERLAYER_N, f"perlayer {name}", "perlayer")


@pytest.mark.parametrize("form", [None, "unfused4"])
def test_per_layer_chunk_loop_reads_the_pose_of_every_source(form):
    """T at 16385 rows: the last piece of the chunk loop starts at row 16384 - the fused kernels' 16-row head, and k_first_layer of the unfused
    pipeline, with a non-zero row0."""
    base = () if form is None else (form,)
    eng = _eng("T")
    with force(eng, *base):
        assert [(r0, rows) for _, r0, rows in _pieces(eng, sh.TILED_CHUNK_N[0])] == [(0, 16384), (16384, 1)]
    _tiled_sweep_by_pieces("T", base, sh.TILED_CHUNK_N, f"perlayer chunks T {form or 'default'}", sh.SOURCES, lambda f: base)


@pytest.mark.parametrize("form", sh.TILED_TILE_FORMS)
@pytest.mark.parametrize("name", ["T", "R"])
def test_forced_tiles_and_heads_read_the_pose_of_every_source(name, form):
    _tiled_sweep(name, ("perlayer", form) if name == "R" else (form,), sh.TILED_TILE_N, f"{form} {name}", "perlayer")


@pytest.mark.parametrize("name,form", [("T", "unfused0"), ("T", "unfused4"), ("T1", None)])
def test_unfused_pipeline_reads_the_pose_of_every_source(name, form):
    """k_first_layer of flow_kernels.hip, and the one-hidden-layer model that takes this pipeline by itself."""
    _tiled_sweep(name, () if form is None else (form,), sh.TILED_UNFUSED_N, f"{form or 'unfused by default'} {name}", "perlayer")


@pytest.mark.parametrize("name", ["T", "R"])
def test_f16x3_contractions_read_the_pose_of_every_source(name):
    eng = _eng(name)
    before = eng.split_fallback_count
    _tiled_sweep(name, ("f16x3", "perlayer") if name == "R" else ("f16x3",), sh.TILED_F16X3_N, f"f16x3 {name}", "perlayer")
    assert eng.split_fallback_count == before, "an f32 re-run is not an f16x3 result"


# ---- (b) plan seams ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["default", "cluster-off", "rowowner-off"])
def test_a_tiled_call_over_a_multi_chunk_plan_is_the_batch_form_on_the_gathered_poses(setting):
    """R, the planner's own chunks: one tiled call over the whole batch is the batch-form call on the gathered poses, and every chunk's rows are
    those rows run alone under the chunk's form.  None of the n_mod but 4096 divides a chunk's first row, and 4096 wraps row 4096 + j to pose j,
    so a chunk that took its local row for the global one cannot pass."""
    name = "R"
    eng = _eng(name)
    base = () if setting == "default" else (setting,)
    with force(eng, *base):
        plans = {n: sh.parse_plan(eng.plan(n)) for n in sh.TILED_SEAM_N}
    print(f"[tiled] seams {setting}: " + "; ".join(f"{n}: {' '.join(f'{f}:{r}' for f, _, r in plans[n])}" for n in sh.TILED_SEAM_N))
    for n in sh.TILED_SEAM_N:
        assert sum(r for _, _, r in plans[n]) == n
        if setting == "default":
            assert len(plans[n]) >= 2, (n, plans[n])
        for _, r0, _ in plans[n][1:]:   # (n_mod = n - 1 divides the first row of a last chunk of one row: that row wraps to pose 0 either way)
            assert all(r0 % n_mod != 0 or n_mod == 4096 or r0 == n_mod == n - 1 for n_mod, _ in sh.seam_sources(n) if n_mod > 1), (n, r0)
    with _no_cluster_repair(eng):
        compared = _tiled_sweep_by_pieces(name, base, sh.TILED_SEAM_N, f"seams {setting}", sh.seam_sources, lambda form: (sh.form_class(form),))
    assert compared == sum(len(sh.seam_sources(n)) for n in sh.TILED_SEAM_N)


def test_rowowner_launch_split_at_two_to_the_24_rows_reads_the_pose_of_the_global_row():
    """The planner puts the row-owner chunk first, so k_flow_rowowner meets a non-zero first row only where run_flow_rowowner cuts a call into
    launches of 2^24 rows.  2^24 + 17 rows under (n_mod 61, scattered) - 61 does not divide 2^24: the last 16 rows of the first launch and the
    17 rows of the second are those rows run alone by the batch form on their gathered poses, bit for bit."""
    name = "R"
    eng = _eng(name)
    Z, P = sh.device_inputs(name)
    split, n = sh.ROWOWNER_LAUNCH_ROWS, sh.ROWOWNER_LAUNCH_ROWS + 17
    Zbig = Z[torch.arange(n, device=DEV) % Z.shape[0]]
    with force(eng, "rowowner"):
        assert eng.plan(n) == f"rowowner:{n}"
        for n_mod, kind in ((61, "scatter"),):
            assert split % n_mod != 0
            idx = _source(name, n_mod, kind)
            got = guarded_tiled(eng, P, idx, n_mod, Zbig, False).clone()
            for r0, rows in ((split - 16, 16), (split, 17)):
                pm = torch.arange(r0, r0 + rows, device=DEV) % n_mod
                Pg = (P[pm] if idx is None else P[idx.long()[pm]]).contiguous()
                alone = guarded_approx(eng, Pg, Zbig[r0:r0 + rows], False)
                assert torch.equal(alone, got[r0:r0 + rows]), f"n_mod={n_mod} list={kind}: rows {r0} .. {r0 + rows - 1} differ from those rows run alone"
            del got


# ---- (c) against fp64 --------------------------------------------------------------------------------------------------------------------------------
def _fp64_forms(eng):
    """(tag, model, forms, n, plan must contain): the largest n of every row of (a)'s table."""
    out = [(f"rowowner {name}", name, ("rowowner",), 4097, "rowowner") for name in ("R", "R10")]
    out += [("+".join(v) + " R", "R", v, 2048, "cluster") for v in _cluster_variants(eng)]
    out += [(f"perlayer {name}", name, ("perlayer",) if name == "R" else (), 2049, "perlayer") for name in ("R", "T", "T300")]
    out += [("perlayer chunks T", "T", (), 16385, "perlayer"), ("unfused4 chunks T", "T", ("unfused4",), 16385, "perlayer")]
    out += [(f"{form} {name}", name, ("perlayer", form) if name == "R" else (form,), 300, "perlayer") for form in sh.TILED_TILE_FORMS for name in ("T", "R")]
    out += [("unfused0 T", "T", ("unfused0",), 700, "perlayer"), ("unfused4 T", "T", ("unfused4",), 700, "perlayer"), ("unfused by default T1", "T1", (), 700, "perlayer")]
    out += [(f"f16x3 {name}", name, ("f16x3", "perlayer") if name == "R" else ("f16x3",), 2049, "perlayer") for name in ("T", "R")]
    return out


def test_tiled_rows_against_fp64_under_every_form():
    """Unclamped rows under (n_mod 17, scattered), (n_mod n - 1, no list) and (n_mod 1, scattered) against run_inference_f64 on the gathered
    conditional, FLOW_TOL relative to max(1, |x|) on every row."""
    R = _eng("R")
    fallbacks = {name: _eng(name).split_fallback_count for name in ("R", "T")}
    with _no_cluster_repair(R):
        for tag, name, forms, n, want_plan in _fp64_forms(R):
            assert n in sh.TILED_REF_N[name]
            eng = _eng(name)
            Z, P = sh.device_inputs(name)
            worst = 0.0
            with force(eng, *forms):
                assert want_plan in eng.plan(n), (tag, n, eng.plan(n))
                for n_mod, kind in sh.ref_sources(n):
                    q = guarded_tiled(eng, P, _source(name, n_mod, kind), n_mod, Z[:n], False)
                    err = sh.rel_err(q, sh.reference_tiled(name, n_mod, kind)[:n])
                    assert err <= FLOW_TOL, f"{tag} n={n} n_mod={n_mod} list={kind}: {err:.2e} from fp64"
                    worst = max(worst, err)
            print(f"[tiled] {tag}: n = {n}, largest relative error against fp64 {worst:.2e}")
    for name, before in fallbacks.items():
        assert _eng(name).split_fallback_count == before, "an f32 re-run is not an f16x3 result"


# ---- (d) the public route: ikf_generate_ranked's candidate rows are the entry's rows -----------------------------------------------------------------
def _ranked_rows(eng, P, m, k, Z, clamp):
    """ikf_generate_ranked, n_keep = k, every rejection off, no refinement: the kept rows put back in tile-major order through index_out (row
    r * m + j is candidate r of pose j, include/ikflow_amd_rank.h)."""
    ndof = eng.layout.ndof
    opt = _lib.ikf_rank_options(k, 0.01, 0.0, -1.0, -1.0, 0, 0, 0.0)
    q_out = torch.full((m, k, ndof), float("nan"), device=DEV)
    index = torch.full((m, k), -7, dtype=torch.int32, device=DEV)
    count = torch.full((m,), -7, dtype=torch.int32, device=DEV)
    Pm = P[:m].contiguous()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = eng.lib.ikf_generate_ranked(eng._h, Pm.data_ptr(), m, k, Z.data_ptr(), 1 if clamp else 0, None, C.byref(opt), q_out.data_ptr(), None,
                                       index.data_ptr(), count.data_ptr(), None, s)
    assert code == _lib.IKF_OK, _lib.last_error(eng.lib)
    torch.cuda.synchronize()
    assert bool((count == k).all()), "with every rejection off each pose keeps all k candidates"
    assert torch.equal(index.sort(1).values, torch.arange(k, dtype=torch.int32, device=DEV).expand(m, k)), "index_out is not a permutation of 0 .. k - 1"
    rows = torch.full((k * m, ndof), float("nan"), device=DEV)
    rows[index.long() * m + torch.arange(m, device=DEV)[:, None]] = q_out
    return rows


@pytest.mark.parametrize("forms,shapes", [((), sh.TILED_RANKED), (("rowowner",), ((65, 16),)), (("cluster-spread",), ((65, 16),)),
                                          (("perlayer",), ((65, 16),)), (("f16x3", "perlayer"), ((65, 16),))],
                         ids=["default", "rowowner", "cluster-spread", "perlayer", "f16x3+perlayer"])
def test_generate_ranked_ranks_the_rows_of_the_tiled_entry(forms, shapes):
    name = "R"
    eng = _eng(name)
    Z, P = sh.device_inputs(name)
    assert eng.lib.ikf_get_candidate_refine(eng._h, None, None) == 0, "a refinement is set on the shared handle"
    before = eng.split_fallback_count
    with _no_cluster_repair(eng), force(eng, *forms):
        for i, (m, k) in enumerate(shapes):
            clamp = i % 2 == 0
            got = _ranked_rows(eng, P, m, k, Z[:k * m], clamp)
            want = guarded_tiled(eng, P[:m].contiguous(), None, m, Z[:k * m], clamp)
            assert torch.equal(got, want), f"{'+'.join(forms) or 'default'} (m, k) = ({m}, {k}), plan {eng.plan(k * m)}: ikf_generate_ranked ranked other rows"
    assert eng.split_fallback_count == before


# ---- (e) statuses and edges ------------------------------------------------------------------------------------------------------------------------------
def test_statuses_of_the_tiled_entry():
    name = "T"
    eng = _eng(name)
    lib, h = eng.lib, eng._h
    Z, P = sh.device_inputs(name)
    n, ndof = 40, eng.layout.ndof
    idx = _source(name, 7, "scatter")
    out = torch.full((n, ndof), float("nan"), device=DEV)
    call = lambda h_, p, i, n_mod, z, rows, o: lib.ikf_generate_approx_tiled(h_, p, i, n_mod, z, rows, 0, 0.0, o, None)
    # n == 0 touches nothing, whatever the pointers
    assert call(h, P.data_ptr(), idx.data_ptr(), 7, Z.data_ptr(), 0, out.data_ptr()) == _lib.IKF_OK
    assert call(h, None, None, 7, None, 0, None) == _lib.IKF_OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    for n_mod in (0, -1):
        assert call(h, P.data_ptr(), idx.data_ptr(), n_mod, Z.data_ptr(), n, out.data_ptr()) == _lib.IKF_ERR_BAD_ARGUMENT
        assert "n_mod" in _lib.last_error(lib) and "ikf_generate_approx_tiled" in _lib.last_error(lib)
        assert call(h, P.data_ptr(), None, n_mod, Z.data_ptr(), 0, out.data_ptr()) == _lib.IKF_ERR_BAD_ARGUMENT
    assert call(h, P.data_ptr(), None, 7, Z.data_ptr(), -1, out.data_ptr()) == _lib.IKF_ERR_BAD_ARGUMENT
    assert call(h, None, idx.data_ptr(), 7, Z.data_ptr(), n, out.data_ptr()) == _lib.IKF_ERR_NULL_POINTER
    assert call(h, P.data_ptr(), idx.data_ptr(), 7, None, n, out.data_ptr()) == _lib.IKF_ERR_NULL_POINTER
    assert call(h, P.data_ptr(), idx.data_ptr(), 7, Z.data_ptr(), n, None) == _lib.IKF_ERR_NULL_POINTER
    assert call(None, P.data_ptr(), idx.data_ptr(), 7, Z.data_ptr(), n, out.data_ptr()) == _lib.IKF_ERR_NULL_POINTER
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote rows"
    # before the weights are loaded
    from ikflow_amd.engine import Engine

    fresh = Engine(eng.layout, eng.robot, DEV)
    assert call(fresh._h, P.data_ptr(), idx.data_ptr(), 7, Z.data_ptr(), n, out.data_ptr()) == _lib.IKF_ERR_NOT_LOADED
    # the batch form's own edge still holds: n == 0 without broadcast is fine
    assert lib.ikf_generate_approx(h, P.data_ptr(), 0, Z.data_ptr(), 0, 0, 0.0, out.data_ptr(), None) == _lib.IKF_OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("name,forms", [("R", ("rowowner",)), ("R", ("cluster",)), ("R", ("perlayer",)), ("T", ())],
                         ids=["R-rowowner", "R-cluster", "R-perlayer", "T-default"])
def test_a_side_stream_and_a_repeated_call_give_the_same_bits(name, forms):
    eng = _eng(name)
    Z, P = sh.device_inputs(name)
    n, n_mod, kind = sh.TILED_EDGE
    idx = _source(name, n_mod, kind)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with _no_cluster_repair(eng), force(eng, *forms):
        first = guarded_tiled(eng, P, idx, n_mod, Z[:n], True, sh.SOFT if eng.layout.dim_cond == 8 else 0.0).clone()
        again = guarded_tiled(eng, P, idx, n_mod, Z[:n], True, sh.SOFT if eng.layout.dim_cond == 8 else 0.0)
        on_side = guarded_tiled(eng, P, idx, n_mod, Z[:n], True, sh.SOFT if eng.layout.dim_cond == 8 else 0.0, stream=side)
    assert torch.equal(again, first), "the same call twice"
    assert torch.equal(on_side, first), "a side stream"
