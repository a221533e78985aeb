"""CPU-only conditions of tests/test_exact_flow.py: what the oracle alone (ko.generate_exact_ik_solutions with the fp64 LM step, on the torch flow
oracle) says about the inputs of exact_helpers.FLOW_CASES, so that the bit-for-bit comparisons of the GPU file reach what they are meant to reach -
a strict sub-list in every retry round, a modulus that is no multiple of 16, a retry round beyond one 4096-row row-owner chunk and beyond the
16384-row per-layer chunk, more than one repeat in round 0.  These are conditions on the inputs, not tolerances.  Nothing here needs a GPU.

The oracle's own counts (active poses per round; rows per round where the case is about rows), recorded when the cases were chosen:
    R-200 200, 193, 168     R10-200 200, 171, 114     R8-200 200, 157, 87     Rsig-200 200, 183, 127     T-200 200, 191, 160
    R-17 17, 17, 15         R10-17 17, 14, 10         R8-17 17, 14, 7         R-1 1, 1, 1
    R-450-tight rows 450, 1338, 4350     R-130-r2 rows 260, 504, 4400     T-1800-tight rows 1800, 5394, 17810"""
import ctypes as C
import os
import re

import pytest
import torch

import exact_helpers as X
import sample_helpers as sh
from ikflow_amd import _lib
from oracle import kinematics_oracle as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_OWNER_CHUNK = 4096


def _show(case):
    s = X.oracle_schedule(case)
    print(f"{case}: active {s['active']}, rows {s['rows']}, solved {s['solved']}, valid at the end {int(s['valid'].sum())}")
    return s


@pytest.mark.parametrize("case", sorted(X.FLOW_CASES))
def test_the_round_by_round_schedule_is_the_oracles_own(case):
    """exact_helpers.oracle_schedule restates the loop of ko.generate_exact_ik_solutions to see its rounds: both give the same rows and flags."""
    name, poses, lats, rc, pos_thr, rot_thr = X.flow_case_inputs(case)
    s = _show(case)
    sol, valid = ko.generate_exact_ik_solutions(sh.model(name)[0], X.oracle_flow_fn(name), poses, lats, rc, pos_thr, rot_thr, lm_dtype=torch.float64)
    assert torch.equal(valid, s["valid"]) and torch.equal(sol.view(torch.int32), s["sol"].view(torch.int32))
    assert s["active"][0] == poses.shape[0] and all(a - b == c for a, b, c in zip(s["active"], s["active"][1:], s["solved"]))
    assert int(valid.sum()) == sum(s["solved"])
    assert poses.shape[0] <= sh.POOL[name] and all(l.shape == (poses.shape[0] * R, sh.model(name)[2].dim) for l, R in zip(lats, rc))


@pytest.mark.parametrize("case", X.FLOW_N200)
def test_every_retry_round_of_the_200_pose_cases_sees_a_strict_sub_list(case):
    """Rounds 0 and 1 each solve at least 3 poses and leave at least 50: the lists of rounds 1 and 2 are strict, non-empty sub-lists whose lengths
    (the pose modulus of the round's flow call) differ from n and from each other.  At least 87 poses are left after round 1 in every model."""
    s = _show(case)
    assert len(s["active"]) == 3
    for r in (0, 1):
        assert s["solved"][r] >= 3 and s["active"][r] - s["solved"][r] >= 50, (case, r, s["active"], s["solved"])
    assert s["active"][2] >= 87
    assert any(a % 16 for a in s["active"][1:]), s["active"]      # a modulus that is no multiple of the 16-row tile


@pytest.mark.parametrize("case", ["R-450-tight", "R-130-r2"])
def test_round_2_of_the_long_cases_is_just_beyond_one_row_owner_chunk(case):
    s = _show(case)
    assert len(s["rows"]) == 3 and ROW_OWNER_CHUNK + 1 <= s["rows"][2] <= 4500, s["rows"]
    assert s["active"][2] < s["active"][1] <= s["active"][0]          # still a sub-list
    assert s["rows"][0] == X.FLOW_CASES[case][1] * X.FLOW_CASES[case][2][0]
    if case == "R-130-r2":
        assert X.FLOW_CASES[case][2][0] > 1 and s["rows"][0] == 260


def test_round_2_of_the_1800_pose_case_is_beyond_the_per_layer_chunk():
    s = _show("T-1800-tight")
    assert len(s["rows"]) == 3 and s["rows"][2] > sh.PER_LAYER_CHUNK + 500, s["rows"]
    assert s["active"][2] < s["active"][1] < 1800


def test_the_two_extremes_solve_everything_at_once_and_nothing_ever():
    every = _show("T-200-all")
    assert every["active"] == [200] and every["solved"] == [200] and bool(every["valid"].all())
    none = _show("T-200-none")
    assert none["active"] == [200, 200, 200] and none["solved"] == [0, 0, 0] and not bool(none["valid"].any())
    assert not none["sol"].view(torch.int32).any()


@pytest.mark.parametrize("case", sorted(X.FLOW_CASES))
def test_the_latents_of_the_rounds_of_a_case_are_pairwise_different(case):
    """A round that read another round's latents must show: over the rows two rounds have in common no row of one equals that row of the other."""
    lats = X.flow_case_inputs(case)[2]
    for i in range(len(lats)):
        for j in range(i + 1, len(lats)):
            m = min(lats[i].shape[0], lats[j].shape[0])
            assert m >= 1 and not bool((lats[i][:m] == lats[j][:m]).all(1).any()), (case, i, j)


_CTYPE = {"ikf_model*": C.c_void_p, "const float*": C.c_void_p, "const int32_t*": C.POINTER(C.c_int32), "float*": C.c_void_p, "uint8_t*": C.c_void_p,
          "int64_t*": C.POINTER(C.c_int64), "void*": C.c_void_p, "int64_t": C.c_int64, "int": C.c_int, "float": C.c_float,
          "ikf_latent_fn": _lib.LATENT_FN}


def _params(text):
    params = [re.sub(r"\s+", " ", p).strip() for p in text.split(",")]
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    types = [re.match(r"(.*?)\s*\b\w+$", p).group(1).replace(" *", "*").strip() for p in params]
    return names, types


def test_the_latent_callback_and_generate_exact_match_the_header():
    header = open(os.path.join(ROOT, "include", "ikflow_amd.h")).read()
    m = re.search(r"typedef\s+const\s+float\s*\*\s*\(\s*\*\s*ikf_latent_fn\s*\)\s*\(([^;]*)\)\s*;", header)
    assert m, "ikf_latent_fn is not declared in include/ikflow_amd.h"
    names, types = _params(m.group(1))
    assert names == ["user", "round", "rows", "dim"] and types == ["void*", "int", "int64_t", "int"]
    assert _lib.LATENT_FN._restype_ is C.c_void_p and list(_lib.LATENT_FN._argtypes_) == [C.c_void_p, C.c_int, C.c_int64, C.c_int]
    m = re.search(r"ikf_status\s+ikf_generate_exact\s*\(([^;]*)\)\s*;", header)
    assert m, "ikf_generate_exact is not declared in include/ikflow_amd.h"
    names, types = _params(m.group(1))
    assert names == ["m", "d_target_poses", "n", "repeat_counts", "n_rounds", "n_lm_steps", "pos_error_threshold", "rot_error_threshold", "latent_fn",
                     "latent_user", "d_q_out", "d_valid_out", "h_stats", "stream"]
    restype, argtypes = _lib.SIGNATURES["ikf_generate_exact"]
    assert restype is C.c_int
    assert argtypes == [_CTYPE[t] for t in types], (types, argtypes)
