"""CPU-only conditions of tests/test_flow_sample.py: what its inputs and helpers must satisfy for its assertions to mean what they say.
Nothing here needs a GPU."""
import numpy as np
import pytest

import sample_helpers as sh
from oracle import flow_oracle as fo

_KEYS = sorted(sh.REFERENCE_SETS)


@pytest.mark.parametrize("key", _KEYS, ids=lambda k: "-".join(str(v) for v in k))
def test_the_f32_oracle_alone_is_within_half_the_tolerance_of_the_fp64_twin_on_every_row(key):
    """Every (model, transform, weights, softflow, pose form) a GPU test compares with the oracle: the reference implementation's own f32
    arithmetic (torch on the CPU) differs from the fp64 twin by at most FLOW_TOL / 2 relative to max(1, |x|), on every row the GPU tests
    use.  A kernel is left as much room as the reference takes.  An input that misses this gets another seed or a lower gain, never a wider
    tolerance."""
    ref64 = sh.reference(*key)
    assert ref64.shape == (sh.REFERENCE_SETS[key], sh.model(*key[:3])[2].ndof) and np.isfinite(ref64).all()
    err = sh.rel_err(sh.reference_f32(*key), ref64)
    print(f"{key}: {ref64.shape[0]} rows, f32 oracle against fp64 {err:.2e}, max |x| {np.abs(ref64).max():.1f}")
    assert err <= sh.FLOW_TOL / 2, (key, err)


@pytest.mark.parametrize("name", ["R", "R10", "T", "T1"])
def test_shuffled_permutations_differ_from_the_seeded_tables_and_are_valid_pairs(name):
    for weights in ("A", "B"):
        robot, hp, lay, sd = sh.model(name, "perm", weights)
        plain = sh.model(name, "plain", weights)[3]
        D = lay.dim
        perms = []
        for i in range(lay.nb_nodes):
            perm, perm_inv = sd[f"module_list.{lay.perm_module(i)}.perm"], sd[f"module_list.{lay.perm_module(i)}.perm_inv"]
            assert perm.dtype == np.int64 and perm_inv.dtype == np.int64
            assert sorted(perm.tolist()) == list(range(D)) and sorted(perm_inv.tolist()) == list(range(D))
            assert (perm_inv[perm] == np.arange(D)).all() and (perm[perm_inv] == np.arange(D)).all()
            stock, stock_inv = fo.permute_random_tables(D, i)
            assert (plain[f"module_list.{lay.perm_module(i)}.perm_inv"] == stock_inv).all()   # (what the builders produce)
            assert not (perm == stock).all() and not (perm_inv == stock_inv).all()
            perms.append(perm)
        assert len({p.tobytes() for p in perms}) == lay.nb_nodes, "two blocks share a table"
        assert not np.all([p == np.arange(D) for p in perms], axis=0).any(), "a position is a fixed point of every block"
        # ... and the tables matter: the outputs move by far more than the tolerance
        n = 64
        z, c = sh.inputs(name)[0][:n].numpy().astype(np.float64), sh.conditional(name, n)
        moved = sh.rel_err(fo.run_inference_f64(sd, lay, robot, z, c, False), fo.run_inference_f64(plain, lay, robot, z, c, False))
        assert moved > 100 * sh.FLOW_TOL, moved


@pytest.mark.parametrize("name", ["R", "R10", "T", "T1"])
@pytest.mark.parametrize("transform,weights", [("dense", "A"), ("dense-noM", "A"), ("all", "A"), ("all", "B")])
def test_a_transposed_read_of_the_dense_m_inv_cannot_pass(name, transform, weights):
    """The dense M_inv is far from diagonal (|log|det|| > 1) and far from symmetric: the oracle run on M_inv.T moves the outputs of these
    very inputs by more than 100 x FLOW_TOL, and so does dropping b."""
    robot, hp, lay, sd = sh.model(name, transform, weights)
    Minv = np.asarray(sd["module_list.0.M_inv"], dtype=np.float64)
    assert abs(np.linalg.slogdet(Minv)[1]) > 1.0
    assert ("module_list.0.M" in sd) == (transform != "dense-noM")
    n = 256
    z, c = sh.inputs(name)[0][:n].numpy().astype(np.float64), sh.conditional(name, n)
    ref = fo.run_inference_f64(sd, lay, robot, z, c, False)
    transposed = dict(sd)
    transposed["module_list.0.M_inv"] = np.ascontiguousarray(np.asarray(sd["module_list.0.M_inv"]).T)
    no_bias = {k: v for k, v in sd.items() if k != "module_list.0.b"}
    for what, other in (("M_inv transposed", transposed), ("b dropped", no_bias)):
        moved = np.abs(fo.run_inference_f64(other, lay, robot, z, c, False) - ref) / np.maximum(1.0, np.abs(ref))
        print(f"{name} {transform} {weights}: {what}: outputs move by {moved.max():.2e} (median row {np.median(moved.max(1)):.2e})")
        assert moved.max() > 100 * sh.FLOW_TOL, (what, moved.max())
        assert np.median(moved.max(1)) > 100 * sh.FLOW_TOL, (what, np.median(moved.max(1)))


@pytest.mark.parametrize("name", ["R", "R10", "T", "T1"])
def test_plain_bias_and_the_deleted_key_are_what_they_say(name):
    plain, bias, no_b = (sh.model(name, t)[3] for t in ("plain", "bias", "no-b"))
    assert not np.asarray(plain["module_list.0.b"]).any(), "the builders' b of a plain graph is zero"
    b = np.asarray(bias["module_list.0.b"])
    assert b.shape == (1, sh.model(name)[2].dim) and b.dtype == np.float32 and (np.abs(b) > 1e-3).all()
    assert all(np.array_equal(bias[k], plain[k]) for k in plain if k != "module_list.0.b")
    assert "module_list.0.b" not in no_b and set(no_b) == set(plain) - {"module_list.0.b"}


def test_sentinel_is_a_nan_no_float32_arithmetic_yields():
    """By construction: exponent all ones and a non-zero mantissa (a NaN), quiet bit set (never altered by a move), and a payload below
    the quiet bit - while every NaN that float32 arithmetic makes out of finite inputs is the default one, payload zero."""
    s = sh.SENTINEL
    assert (s >> 23) & 0xFF == 0xFF and s & 0x7FFFFF != 0, "not a NaN"
    assert s & 0x400000, "a signalling NaN may be quietened on its way through a register"
    assert s & 0x3FFFFF != 0, "the default NaN: arithmetic produces it"
    assert np.isnan(np.array([s], dtype=np.uint32).view(np.float32)[0])
    assert np.array([s], dtype=np.int32).view(np.uint32)[0] == s, "fits the int32 buffer unchanged"
    with np.errstate(all="ignore"):
        big, zero, one = np.float32(3e38), np.float32(0.0), np.float32(1.0)
        inf = big * big
        made = [inf - inf, zero * inf, zero / zero, inf / inf, np.sqrt(np.float32(-1.0)), np.log(np.float32(-1.0)),
                np.arcsin(np.float32(2.0)), np.float32(np.float64("nan")), (inf - inf) + one, np.exp(inf - inf), np.arctan(zero / zero)]
    for v in made:
        bits = int(np.array([v], dtype=np.float32).view(np.uint32)[0])
        assert np.isnan(v) and bits & 0x7FFFFFFF == 0x7FC00000, hex(bits)
        assert bits != s


def test_force_names_every_form_of_the_issue_and_no_give_up_hook():
    want = {"perlayer": (180, 185), "rowowner": (182,), "cluster": (187,), "cluster-epoch": (187, 192), "cluster-tagged": (187, 193),
            "cluster-spread": (187, 189), "entry-off": (110,), "entry-forced": (112,), "rows16-off": (150,)}
    want.update({f"tile{c}": (101 + c,) for c in (0, 1, 2, 3, 4, 6)})
    want.update({f"unfused{v}": (v,) for v in range(9)})
    for form, codes in want.items():
        assert sh.FORMS[form] == codes, form
    assert not {188, 191} & {c for codes in sh.FORMS.values() for c in codes}


def test_parse_plan():
    assert sh.parse_plan("rowowner:4096 cluster16:200") == [("rowowner", 0, 4096), ("cluster16", 4096, 200)]
    assert sh.parse_plan("cluster2:2048 cluster2:2048 perlayer:1") == [("cluster2", 0, 2048), ("cluster2", 2048, 2048), ("perlayer", 4096, 1)]
    assert sh.form_class("cluster32") == "cluster" and sh.form_class("perlayer") == "perlayer"
