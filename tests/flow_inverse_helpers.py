"""What tests/test_flow_inverse.py and tests/test_flow_inverse_shapes.py share: the fp64 references of the inverse pass with its
log-determinant, the comparison against them, the row sample and the raw C-ABI call with sentinel rows behind every output."""
import ctypes as C

import numpy as np
import torch

from flow_logdet import forward_with_logdet
from ikflow_amd import _lib
from oracle import flow_oracle as fo

DEV = "cuda:0"
FLOW_TOL = 1e-5     # relative to max(1, |x|)
LD_TOL = 1e-4       # absolute, log|det| of O(10)
SENTINEL = 0x7FC0DEAD   # a NaN whose payload no kernel writes


def _cond(lay, poses, soft=0.0):
    """The oracle's conditional: [pose] or [pose, softflow scale]."""
    c = np.asarray(poses, dtype=np.float64)
    if lay.dim_cond == 8:
        c = np.concatenate([c, np.full((c.shape[0], 1), soft)], 1)
    return c


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _refs(sd, lay, z, cond):
    """fp64 (x [n x D] = output_rev, log|det dx/dz| [n] = minus the forward log-det at x)."""
    x_ref = fo.flow_inverse_f64(sd, lay, np.asarray(_np(z), dtype=np.float64), cond)
    return x_ref, -forward_with_logdet(sd, lay, x_ref, cond)[1]


def _rel(a, ref):
    return float((np.abs(_np(a) - ref) / np.maximum(1.0, np.abs(ref))).max())


def _check(tag, sd, lay, z, cond, x, ld, rows=None, refs=None):
    """x (FLOW_TOL relative to max(1, |x|)) and log|det dx/dz| (LD_TOL absolute) against the fp64 references on `rows` (None: every row)."""
    z, x, ld = _np(z), _np(x), _np(ld)
    idx = np.arange(x.shape[0]) if rows is None else np.asarray(rows)
    x_ref, ld_ref = refs if refs is not None else _refs(sd, lay, z[idx], cond[idx])
    assert np.isfinite(x[idx]).all() and np.isfinite(ld[idx]).all(), tag
    xerr, lerr = _rel(x[idx], x_ref), float(np.abs(ld[idx] - ld_ref).max())
    line = (f"{tag}: {'every row' if rows is None else f'{len(idx)} sampled rows'} of {x.shape[0]}: max |dx| rel {xerr:.2e}, "
            f"max |dlog_det| {lerr:.2e} (|log_det| up to {np.abs(ld_ref).max():.1f})")
    print(line)
    assert xerr <= FLOW_TOL and lerr <= LD_TOL, line
    return xerr, lerr


def _edge_rows(n, edges=(), k=256, seed=0):
    """Row sample: first, last, both rows at every edge, k seeded random rows (sorted, unique)."""
    s = {0, n - 1}
    for e in edges:
        s.update(r for r in (e - 1, e) if 0 <= r < n)
    s.update(np.random.default_rng(seed).integers(0, n, size=min(k, n)).tolist())
    return np.array(sorted(s))


def _guarded_inverse(eng, Z, P, clamp=False, soft=0.0, broadcast=False, want=(True, True, True)):
    """ikf_flow_inverse through the raw C-ABI into x / q / log_det buffers with 64 extra rows of a NaN sentinel behind each: the rows
    past n - 1 - and a buffer whose pointer was not passed - must come back bit-unchanged.  Returns (x, q, log_det), None where not wanted."""
    n, D = Z.shape
    ndof = eng.layout.ndof
    bufs = [torch.full((n + 64, D), SENTINEL, dtype=torch.int32, device=DEV), torch.full((n + 64, ndof), SENTINEL, dtype=torch.int32, device=DEV),
            torch.full((n + 64,), SENTINEL, dtype=torch.int32, device=DEV)]
    ptrs = [b.data_ptr() if w else None for b, w in zip(bufs, want)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    code = eng.lib.ikf_flow_inverse(eng._h, Z.data_ptr(), n, P.data_ptr(), 1 if broadcast else 0, soft, 1 if clamp else 0, ptrs[0], ptrs[1],
                                    ptrs[2], stream)
    assert code == _lib.IKF_OK, _lib.last_error()
    torch.cuda.synchronize()
    out = []
    for b, w in zip(bufs, want):
        assert bool((b[n if w else 0:] == SENTINEL).all()), f"n={n}: store past row n - 1, or into an output that was not asked for"
        out.append(b[:n].view(torch.float32) if w else None)
    return out
