"""The conditions the GPU tests of the exact collision rule (tests/test_exact_world.py) lean on, by the oracle and the fp64 references alone
(tests/exact_world_helpers.py): no GPU, no engine.

  - every case of "equals its parts" has candidates, at most 5 % of its poses in the 1e-4 band of a threshold, and both outcomes: at least 20 % of
    its candidate rows surely rejected and at least 20 % surely admissible;
  - the sibling cases hold at least 5 poses whose iteration-1 candidate is rejected while a later candidate of another repeat is selected;
  - the retry-round cases: round 0's candidates of the blocked poses at least 1 cm deep, round 1's and the free poses' at least 1 cm clear, every
    candidate valid outside the band of the pose thresholds;
  - the binding table matches the header."""
import os
import re

import numpy as np
import pytest

import exact_world_helpers as EW
from ikflow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", [c.name for c in EW.CASES])
def test_cases_have_both_outcomes_and_a_small_band(name):
    c = EW.CASE_BY_NAME[name]
    cand, rejected, admissible, band = EW.shares(name)
    _, first, cl, thr = EW.oracle_rows(name)
    print(f"{name}: rows {c.n * c.R}, candidates {cand}, first iterations {np.bincount(first, minlength=c.steps + 1).tolist()}, rules {sorted(cl)}, "
          f"thresholds {({k: round(v, 4) for k, v in thr.items()})}, surely rejected {rejected:.3f}, surely admissible {admissible:.3f}, "
          f"poses in the band {band:.4f}")
    assert cand >= 0.3 * c.n * c.R, (name, cand)
    assert band <= EW.BAND_SHARE_CAP, (name, band)
    assert rejected >= EW.MIN_SHARE and admissible >= EW.MIN_SHARE, (name, rejected, admissible)
    winner = EW.select(first, EW.rejected_of(cl, thr), c.n, c.R)
    assert (winner >= 0).any()
    if c.R > 1:   # the rule changes a selection somewhere: a pose whose plain winner is rejected
        plain = EW.select(first, np.zeros(len(first), bool), c.n, c.R)
        assert (plain != winner).any(), name


def test_cases_cover_the_shapes():
    cs = EW.CASES
    assert {len(EW.capsules_of(c)) for c in cs} >= {1, 5, 24}
    assert {EW.X.orob_of(c.which).ndof for c in cs} == {4, 5, 6, 7, 8}
    assert {c.lm for c in cs} == {"f64", "f32"} and {c.steps for c in cs} == {1, 3, 20}
    assert {(c.n, c.R) for c in cs} >= {(7, 9), (13, 5), (64, 1), (65, 1), (257, 1), (200, 10)}
    assert {c.world for c in cs} >= {"one", "mixed7", "full64"} and {c.cloud for c in cs} >= {1, 512, 513, 4096}
    rules = {(c.world is not None, c.cloud > 0, c.reject_self) for c in cs}
    assert rules >= {(True, False, False), (False, True, False), (False, False, True), (True, True, True)}


@pytest.mark.parametrize("with_cloud", (False, True))
@pytest.mark.parametrize("name", sorted(EW.SIBLING_CASES))
def test_sibling_cases_hold_enough_poses(name, with_cloud):
    s = EW.sibling_case(name, with_cloud)
    count = int(s["siblings"].sum())
    print(f"sibling {name} cloud {with_cloud}: {count} poses of {s['n']} (thresholds {s['thr']})")
    assert count >= EW.SIBLING_MIN, (name, with_cloud, count)


@pytest.mark.parametrize("name", sorted(EW.SIBLING_CASES))
def test_cloud_only_sibling_cases_hold_enough_poses(name):
    s = EW.sibling_cloud_case(name)
    count = int(s["siblings"].sum())
    print(f"sibling {name}, the sphere as a cloud of one point: {count} poses of {s['n']}")
    assert count >= EW.SIBLING_MIN, (name, count)


@pytest.mark.parametrize("n,kind", [(64, "all"), (1, "all"), (255, "half"), (257, "runs16"), (4099, "half")])
def test_retry_round_cases_have_their_depths_and_margins(n, kind):
    c = EW.blocked_case(n, kind)
    deep, clear1, clear_free, valid = EW.blocked_margins(c)
    print(f"blocked_case({n}, {kind}): blocked {int(c['blocked'].sum())}, round-0 clearance of the blocked <= {deep}, round-1 >= {clear1}, free >= {clear_free}")
    assert valid
    if c["blocked"].any():
        assert deep <= -EW.MARGIN and clear1 >= EW.MARGIN, (deep, clear1)
    if (~c["blocked"]).any():
        assert clear_free >= EW.MARGIN, clear_free


def test_exact_world_signatures_match_the_header():
    text = open(os.path.join(ROOT, "include", "ikflow_amd_exact_world.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", code))
    assert declared == {"ikf_set_exact_collision", "ikf_get_exact_collision", "ikf_exact_collision_rejected"} == set(_lib.EXACT_WORLD_SIGNATURES)
    assert re.findall(r"#define (IKF_[A-Z_]+) ", code) == []
    for name, (restype, argtypes) in _lib.EXACT_WORLD_SIGNATURES.items():
        decl = re.search(r"ikf_status\s+" + name + r"\s*\(([^)]*)\)", code)
        assert decl, name
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(argtypes), name
        assert restype is _lib.C.c_int
