"""CPU-only conditions of tests/test_flow_sample_tiled.py: what its pose sources, lists and references must satisfy for its assertions to mean
what they say.  Nothing here needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sample_helpers as sh
from ikflow_amd import _lib
from oracle import flow_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_KEYS = sorted(sh.TILED_SETS, key=str)
_CASES = sorted(sh.tiled_cases(), key=str)
TILE = 16   # rows of the smallest row tile of any form: a wrong index must show in every such tile it can touch


@pytest.mark.parametrize("key", _KEYS, ids=lambda k: "-".join(str(v) for v in k))
def test_the_f32_oracle_alone_is_within_half_the_tolerance_of_the_fp64_twin_on_every_tiled_row(key):
    """The rule of tests/test_flow_sample_inputs.py for every key of TILED_SETS: an input that misses it gets another seed, never a wider
    tolerance."""
    ref64 = sh.reference_tiled(*key)
    assert ref64.shape == (sh.TILED_SETS[key], sh.model(key[0])[2].ndof) and np.isfinite(ref64).all()
    err = sh.rel_err(sh.reference_tiled_f32(*key), ref64)
    print(f"{key}: {ref64.shape[0]} rows, f32 oracle against fp64 {err:.2e}, max |x| {np.abs(ref64).max():.1f}")
    assert err <= sh.FLOW_TOL / 2, (key, err)


def test_every_reference_the_gpu_tests_ask_for_is_registered_and_every_call_fits_the_pool():
    for name, sizes in sh.TILED_REF_N.items():
        for n in sizes:
            for src in sh.ref_sources(n):
                assert sh.TILED_SETS[(name,) + src] >= n
    for name, n, n_mod, kind in _CASES:
        pool = sh.POOL[name]
        assert 1 <= n <= pool and n_mod >= 1
        rows = sh.source_rows(n_mod, kind, pool, n)
        assert rows.shape == (n,) and rows.min() >= 0 and rows.max() < pool, (name, n, n_mod, kind)
        if kind is None:   # (without a list the source reads the first min(n, n_mod) rows of the table)
            assert min(n, n_mod) <= pool
        else:
            assert kind in sh.LIST_KINDS and n_mod <= pool + 5
    assert len(_CASES) > 500


# ---- the lists are what they claim ---------------------------------------------------------------------------------------------------------------
def _listed():
    return sorted({(kind, n_mod, sh.POOL[name]) for name, n, n_mod, kind in _CASES if kind is not None})


def test_the_lists_are_what_they_claim():
    seen = {"scatter": 0, "compacted": 0}
    for kind, n_mod, pool in _listed():
        idx = sh.pose_list(kind, n_mod, pool)
        assert idx.dtype == np.int32 and idx.shape == (n_mod,) and not idx.flags.writeable
        assert idx.min() >= 0 and idx.max() < pool, (kind, n_mod, pool)
        assert np.array_equal(idx, sh.pose_list.__wrapped__(kind, n_mod, pool)), "a list is a function of (kind, n_mod, pool) only"
        d = np.diff(idx.astype(np.int64))
        if kind == "scatter":
            assert idx[0] == pool - 1 and (n_mod == 1 or idx[-1] == 0)
            if n_mod >= 2:
                assert not (d > 0).all(), "ascending"
            if n_mod >= 4:
                assert (d > 0).any() and (d < 0).any(), (n_mod, pool, "monotone")
        else:
            assert (d > 0).all(), "not strictly ascending"
            if n_mod < pool:   # (a subset that leaves something out is not the identity)
                assert idx[-1] != n_mod - 1
        if n_mod == 1:
            assert idx[0] != 0, (kind, pool, "with one entry the list must be visible")
        seen[kind] += 1
    assert min(seen.values()) > 20, seen


def test_sources_of_a_call():
    assert sh.SOURCES(1) == [(1, None), (1, "scatter"), (1, "compacted"), (6, "scatter")]
    s = sh.SOURCES(300)
    assert sorted({m for m, _ in s}) == [1, 2, 3, 15, 16, 17, 61, 299, 300, 305] and len(s) == 9 * 3 + 1 and s[-1] == (305, "scatter")
    assert {m for m, _ in sh.SOURCES(17)} == {1, 2, 3, 15, 16, 17, 22}
    assert sh.seam_sources(600) == [(1, None), (1, "scatter"), (7, None), (7, "scatter"), (1000, None), (1000, "scatter"), (599, None), (599, "scatter")]
    assert (4097, "scatter") in sh.seam_sources(4096 + 200) and sh.seam_sources(4096 + 200)[-1] == (4096, None)
    assert (4097, None) in sh.seam_sources(2 * 4096 + 2049) and (4096, None) not in sh.seam_sources(2 * 4096 + 2049)


def test_gathered_is_the_source_rows_of_the_table():
    import torch

    P = torch.arange(40 * 7, dtype=torch.float32).reshape(40, 7)
    for n_mod, kind, n in ((7, None, 30), (7, "scatter", 30), (7, "compacted", 30), (1, "scatter", 5), (35, "scatter", 30), (30, None, 30)):
        idx = sh.pose_list(kind, n_mod, 40)
        got = sh.gathered(P, None if idx is None else torch.from_numpy(idx.copy()), n_mod, n)
        want = P.numpy()[sh.source_rows(n_mod, kind, 40, n)]
        assert got.is_contiguous() and np.array_equal(got.numpy(), want)
        assert all(np.array_equal(want[r], P[(idx[r % n_mod] if idx is not None else r % n_mod)].numpy()) for r in range(n))


# ---- the wrong index is visible ------------------------------------------------------------------------------------------------------------------------
def _wrong_rows(n_mod, kind, pool, n):
    """{what: int64 [n]}: the table rows a wrong copy of the index arithmetic would read.
    list ignored:    P[r % n_mod] (a source with a list only);
    modulus ignored: the batch form's arithmetic, P[min(r, pool - 1)], with a list the last entry for every row past it;
    late wrap:       row n_mod does not wrap yet - it reads the table row (with a list: the entry) behind the last one it may read."""
    r = np.arange(n, dtype=np.int64)
    idx = sh.pose_list(kind, n_mod, pool)
    right = sh.source_rows(n_mod, kind, pool, n)
    out = {}
    if idx is not None:
        out["list ignored"] = r % n_mod
    out["modulus ignored"] = np.minimum(r, pool - 1) if idx is None else idx.astype(np.int64)[np.minimum(r, n_mod - 1)]
    late = right.copy()
    if n > n_mod:
        late[n_mod] = min(n_mod, pool - 1) if idx is None else int(idx[n_mod - 1])
    out["late wrap"] = late
    return right, out


def _equal_by_definition(what, n_mod, kind, pool, n):
    if what == "list ignored":   # an ascending subset of the whole pool is the identity
        return kind == "compacted" and n_mod >= pool
    return n <= n_mod or (kind is not None and n_mod == 1)   # no row wraps; one entry, read by every row either way


def _required_tiles(what, n_mod, kind, n, wrong, right):
    """The 16-row tiles in which the wrong copy must show: those with a row whose wrong table row is another one than the right one.  These are
    every tile with a listed row (a scattered list ignored), every tile with a wrapped row (modulus ignored, no list) and the tile of row n_mod
    (late wrap).  An ascending list equals the identity up to its first gap, and with a list the rows that wrap onto its last entry read that
    entry either way: there the tiles are those the definition leaves."""
    tiles = np.arange(n) // TILE
    need = np.unique(tiles[wrong != right])
    if what == "list ignored" and kind == "scatter":
        assert np.array_equal(need, np.unique(tiles))
    elif what == "modulus ignored" and kind is None:
        assert np.array_equal(need, np.unique(tiles[n_mod:]))
    elif what == "late wrap":
        assert np.array_equal(need, [n_mod // TILE])
    return need


def test_a_wrong_index_is_visible_in_every_tile_it_can_touch():
    """For every (n, source) a GPU test uses, the conditional a wrong copy would gather differs from the right one - unless the two are the same
    rows by definition - in at least one row of every 16-row tile that contains a listed or wrapped row."""
    checked = {}
    for name, n, n_mod, kind in _CASES:
        pool = sh.POOL[name]
        poses = sh.inputs(name)[1].numpy()
        right, wrongs = _wrong_rows(n_mod, kind, pool, n)
        for what, wrong in wrongs.items():
            differs = (poses[wrong] != poses[right]).any(1)
            if _equal_by_definition(what, n_mod, kind, pool, n):
                assert np.array_equal(wrong, right), (what, name, n, n_mod, kind)
                continue
            assert differs.any(), (what, name, n, n_mod, kind)
            need = _required_tiles(what, n_mod, kind, n, wrong, right)
            assert len(need) > 0
            seen = np.unique((np.arange(n) // TILE)[differs])
            missing = np.setdiff1d(need, seen)
            assert len(missing) == 0, f"{what} {name} n={n} n_mod={n_mod} list={kind}: the 16-row tiles {missing[:8]} would pass"
            checked[what] = checked.get(what, 0) + 1
    print(f"{len(_CASES)} (model, n, source) cases; wrong copies visible: {checked}")
    assert set(checked) == {"list ignored", "modulus ignored", "late wrap"} and min(checked.values()) > 100


@pytest.mark.parametrize("name", sorted(sh.TILED_REF_N))
def test_a_wrong_index_moves_the_fp64_outputs_by_far_more_than_the_tolerance(name):
    """The map from a row's pose to its output does not depend on n: for every source the GPU tests run on this model (n_mod as a number, or as
    n - 1 / n / n + 5), at the largest n it is used with, and for every wrong copy, the fp64 outputs of (up to) 256 rows that would read another
    pose move by more than 100 x FLOW_TOL."""
    robot, hp, lay, sd = sh.model(name)
    pool = sh.POOL[name]
    largest = {}
    for _, n, n_mod, kind in [c for c in _CASES if c[0] == name]:
        key = (("n +", n_mod - n) if n_mod >= n - 1 else ("", n_mod), kind)
        if key not in largest or n > largest[key][0]:
            largest[key] = (n, n_mod, kind)
    z_all, poses = sh.inputs(name)[0].numpy().astype(np.float64), sh.inputs(name)[1].numpy().astype(np.float64)
    cond = lambda rows: np.concatenate([poses[rows], np.zeros((len(rows), 1))], 1) if lay.dim_cond == 8 else poses[rows]
    least, runs = np.inf, 0
    for n, n_mod, kind in largest.values():
        right, wrongs = _wrong_rows(n_mod, kind, pool, n)
        for what, wrong in wrongs.items():
            if _equal_by_definition(what, n_mod, kind, pool, n):
                continue
            sample = np.flatnonzero(wrong != right)[:256]
            assert len(sample) > 0
            a = fo.run_inference_f64(sd, lay, robot, z_all[sample], cond(right[sample]), False)
            b = fo.run_inference_f64(sd, lay, robot, z_all[sample], cond(wrong[sample]), False)
            moved = float((np.abs(b - a) / np.maximum(1.0, np.abs(a))).max())
            assert moved > 100 * sh.FLOW_TOL, (what, name, n, n_mod, kind, moved)
            least, runs = min(least, moved), runs + 1
    print(f"{name}: {runs} wrong gathers, the outputs move by at least {least:.2e}")
    assert runs >= 20


# ---- the new entry's signature ----------------------------------------------------------------------------------------------------------------------
_CTYPE = {"ikf_model*": C.c_void_p, "const float*": C.c_void_p, "const int32_t*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p,
          "int64_t": C.c_int64, "int": C.c_int, "float": C.c_float}


def test_generate_approx_tiled_is_exported_and_its_ctypes_signature_matches_the_header():
    header = open(os.path.join(ROOT, "include", "ikflow_amd_debug.h")).read()
    m = re.search(r"ikf_status\s+ikf_generate_approx_tiled\s*\(([^;]*)\)\s*;", header)
    assert m, "ikf_generate_approx_tiled is not declared in include/ikflow_amd_debug.h"
    assert "ikf_generate_approx_tiled" not in open(os.path.join(ROOT, "include", "ikflow_amd.h")).read()   # a test entry, not the boundary
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == ["m", "d_poses", "d_idx", "n_mod", "d_latent", "n", "clamp_to_limits", "softflow_scale", "d_q_out", "stream"]
    types = [re.match(r"(.*?)\s*\b\w+$", p).group(1).replace(" *", "*").strip() for p in params]
    restype, argtypes = _lib.SIGNATURES["ikf_generate_approx_tiled"]
    assert restype is C.c_int
    assert argtypes == [_CTYPE[t] for t in types], (types, argtypes)
    for flavour in ("", "probes"):
        assert hasattr(_lib.load(flavour), "ikf_generate_approx_tiled")
    assert _lib.load().ikf_abi_version() == _lib.IKF_ABI_VERSION == 3   # additive change
