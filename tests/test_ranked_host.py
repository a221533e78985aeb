"""Best-of-K ranking, what can be checked without a GPU: the argument asserts of IKFlowSolver.generate_ranked_ik_solutions, and the binding table of
include/ikflow_amd_rank.h against both flavours of the library."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import tiny_model
from ikflow_amd import _lib
from ikflow_amd.ikflow_solver import IKFlowSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranked_solver_argument_asserts_fire_before_any_device_work():
    robot, hp, lay, sd = tiny_model()
    s = IKFlowSolver(hp, robot)
    y = torch.zeros(4, 7)
    with pytest.raises(AssertionError, match="Model weights have not been loaded"):
        s.generate_ranked_ik_solutions(y, 5)
    s.load_state_dict_tensors(sd)
    bad = [
        (dict(y=[0.0] * 7, k=5), "y must be a torch.Tensor"),
        (dict(y=torch.zeros(4, 6), k=5), "y must be of shape"),
        (dict(y=y, k=0), "k must be a positive int"),
        (dict(y=y, k=5.0), "k must be a positive int"),
        (dict(y=y, k=5, n_keep=0), "n_keep must be in"),
        (dict(y=y, k=5, n_keep=6), "n_keep must be in"),
        (dict(y=y, k=50, n_keep=17), "n_keep must be in"),
        (dict(y=y, k=5, latent_scale=1), None),
        (dict(y=y, k=5, latent=np.zeros((20, 9))), "latent must either be"),
        (dict(y=y, k=5, latent=torch.zeros(19, 9)), r"latent must be \[20 x 9\]"),
        (dict(y=y, k=5, q_ref=torch.zeros(3, 7)), r"q_ref must be \[4 x 7\]"),
        (dict(y=y, k=5, reject_self_collisions=True), "needs a collision model"),
        (dict(y=y, k=5, pos_error_threshold=-1.0), "pos_error_threshold"),
        (dict(y=y, k=2 ** 30), "at most 2"),
    ]
    for kw, msg in bad:
        with pytest.raises(AssertionError, match=msg):
            s.generate_ranked_ik_solutions(**kw)
    assert not robot.has_collision_model   # (so reject_self_collisions=None means "off" here)
    if not torch.cuda.is_available():      # a call that passes every assert gets as far as the engine, which has no CPU path
        from ikflow_amd.engine import EngineError

        with pytest.raises(EngineError, match="no CPU path"):
            s.generate_ranked_ik_solutions(y, 5)


def test_rank_header_is_bound_and_exported_by_both_flavours():
    """Every ikf_ name that include/ikflow_amd_rank.h declares is in _lib.RANK_SIGNATURES (and only those), none of them is in the boundary
    header's table, and both flavours of the library export them; the options struct of the binding has the header's fields in its order."""
    text = open(os.path.join(ROOT, "include", "ikflow_amd_rank.h")).read()
    declared = set(re.findall(r"\b(ikf_[a-z_0-9]+)\s*\(", text))
    assert declared == {"ikf_rank_candidates", "ikf_generate_ranked", "ikf_reserve_ranked"}
    assert declared == set(_lib.RANK_SIGNATURES) and not (declared & set(_lib.SIGNATURES))
    assert "ikf_rank_chunks" in _lib.SIGNATURES
    body = re.search(r"typedef struct ikf_rank_options \{(.*?)\} ikf_rank_options;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in _lib.ikf_rank_options._fields_]
    assert int(re.search(r"#define IKF_RANK_MAX_KEEP (\d+)", text).group(1)) == _lib.IKF_RANK_MAX_KEEP
    for flavour in ("", "probes"):
        lib = _lib.load(flavour)
        for name in declared | {"ikf_rank_chunks"}:
            assert hasattr(lib, name), f"{name} is not exported by the {flavour or 'product'} library"
        assert lib.ikf_rank_chunks(None, 10, 10) == 0   # (no handle, no device)
