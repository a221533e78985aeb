"""fp64 forward pass WITH its log-determinant, for tests/test_flow_forward.py - written here, independently of the engine.

forward_with_logdet: FixedLinearTransform forward (x.mm(M) + b, log|det M|), on sigmoid graphs the flipped sigmoid's forward (logit, term
-sum log(v (1 - v))), then per block PermuteRandom forward and the GLOW coupling forward (each half adds sum clamp 0.636 atan(s)).
fd_logdet: slogdet of a central-difference Jacobian of any row-wise map - the check on the formula above that does not recall it."""
import numpy as np

from oracle import flow_oracle as fo


def _subnet(sd, lay, block, which, u, dt=np.float64):
    base = f"module_list.{lay.glow_module(block)}.subnet{which}."
    slope = dt(np.float32(fo.LEAKY_SLOPE))
    h = u
    for layer in range(lay.n_hidden + 1):
        h = h @ np.asarray(sd[f"{base}{2 * layer}.weight"], dtype=dt).T + np.asarray(sd[f"{base}{2 * layer}.bias"], dtype=dt)
        if layer != lay.n_hidden:
            h = np.where(h > 0, h, slope * h)
    return h


def forward_with_logdet(sd, lay, x, cond, dt=np.float64):
    """[n x D] rows, [n x dim_cond] conditional -> (z [n x D], log|det dz/dx| [n]), float64.  dt=np.float32: the same arithmetic in float32
    (log|det M| still fp64, rounded once) - the rounding noise of an f32 evaluation, for the cases where that noise itself exceeds the
    tolerances (trained-like gains)."""
    L1, L2 = lay.dim // 2, lay.dim - lay.dim // 2
    clamp = dt(np.float32(lay.clamp))
    gain = dt(np.float32(fo.GLOW_ATAN_GAIN))
    # (a state_dict without M: its inverse from M_inv, as the oracle's forward does)
    M = (np.asarray(sd["module_list.0.M"], dtype=np.float64) if "module_list.0.M" in sd
         else np.linalg.inv(np.asarray(sd["module_list.0.M_inv"], dtype=np.float64)))
    b = np.asarray(sd["module_list.0.b"], dtype=dt).reshape(-1)
    c = np.asarray(cond, dtype=dt)
    v = np.asarray(x, dtype=dt) @ M.astype(dt) + b
    ld = np.full(v.shape[0], np.linalg.slogdet(M)[1], dtype=dt)
    if lay.sigmoid_on_output:
        ld = ld - np.sum(np.log(v * (dt(1) - v)), 1)
        v = np.log(v / (dt(1) - v))
    for i in range(lay.nb_nodes):
        perm = np.argsort(np.asarray(sd[f"module_list.{lay.perm_module(i)}.perm_inv"], dtype=np.int64))
        v = v[:, perm]
        x1, x2 = v[:, :L1], v[:, L1:]
        r2 = _subnet(sd, lay, i, 2, np.concatenate([x2, c], 1), dt)
        s2 = clamp * gain * np.arctan(r2[:, :L1])
        y1 = np.exp(s2) * x1 + r2[:, L1:]
        r1 = _subnet(sd, lay, i, 1, np.concatenate([y1, c], 1), dt)
        s1 = clamp * gain * np.arctan(r1[:, :L2])
        y2 = np.exp(s1) * x2 + r1[:, L2:]
        ld = ld + s2.sum(1) + s1.sum(1)
        v = np.concatenate([y1, y2], 1)
    return v, ld


def fd_logdet(fn, x, h=1e-7):
    """log|det J| per row of the row-wise map fn: [n x D] -> [n x D], J by central differences in float64."""
    x = np.asarray(x, dtype=np.float64)
    n, D = x.shape
    J = np.empty((n, D, D))
    for k in range(D):
        e = np.zeros(D)
        e[k] = h
        J[:, :, k] = (fn(x + e) - fn(x - e)) / (2.0 * h)
    return np.linalg.slogdet(J)[1]
