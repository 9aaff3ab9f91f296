"""float64 restatement of the decoder form of row f-9 (tests only): a trunk of Linear + exact GELU layers and heads off its last
activation, forward and backward, written from the formulas:

    z_l = a_{l-1} W_l^T + b_l,  a_l = gelu(z_l) = z_l Phi(z_l),  Phi(z) = (1 + erf(z / sqrt 2)) / 2,  a_0 = x
    y_k = act_k(a_L Wh_k^T + bh_k),  act in {None, 'gelu', 'sigmoid'}
    gelu'(z) = Phi(z) + z exp(-z^2 / 2) / sqrt(2 pi),  sigmoid'(z) = s (1 - s)
    gz = dL/dy * act'(z);  dW = gz^T a_in;  db = sum over points of gz;  dL/da_in = gz W

Weights are torch's Linear layout [out, in].  Every array is float64; the inputs are whatever float32 values the test feeds, cast up.
"""
import numpy as np
import torch


def _erf(a):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).numpy()


def _phi_cdf(z):
    return 0.5 * (1.0 + _erf(z / np.sqrt(2.0)))


def _act(kind, z):
    """(value, derivative)"""
    if kind in (None, "none"):
        return z, np.ones_like(z)
    if kind == "gelu":
        cdf = _phi_cdf(z)
        return z * cdf, cdf + z * np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)
    if kind == "sigmoid":
        s = 1.0 / (1.0 + np.exp(-z))
        return s, s * (1.0 - s)
    raise ValueError(kind)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def forward(x, trunk, heads):
    """x [n, in]; trunk [(W, b), ...]; heads [(W, b, act), ...] -> (outputs, cache)"""
    a = _f64(x)
    acts, derivs = [a], []
    for W, b in trunk:
        a, d = _act("gelu", a @ _f64(W).T + _f64(b))
        acts.append(a)
        derivs.append(d)
    outs, head_derivs = [], []
    for W, b, kind in heads:
        y, d = _act(kind, a @ _f64(W).T + _f64(b))
        outs.append(y)
        head_derivs.append(d)
    return outs, (acts, derivs, head_derivs)


def backward(x, trunk, heads, g_outs):
    """g_outs: one [n, out] per head or None (that head is unused).
    -> dict(dx, trunk=[(dW, db), ...], heads=[(dW, db), ...], factors): `factors` are the (gz, a_in) pairs whose products over the
    points the parameter gradients are, in the order trunk layers then heads (for the sequential-float32 yardstick)."""
    _, (acts, derivs, head_derivs) = forward(x, trunk, heads)
    a_last = acts[-1]
    g_a = np.zeros_like(a_last)
    head_grads, head_factors = [], []
    for (W, b, _), d, g in zip(heads, head_derivs, g_outs):
        gz = np.zeros_like(d) if g is None else _f64(g) * d
        head_grads.append((gz.T @ a_last, gz.sum(0)))
        head_factors.append((gz, a_last))
        g_a = g_a + gz @ _f64(W)
    trunk_grads, trunk_factors = [None] * len(trunk), [None] * len(trunk)
    for l in range(len(trunk) - 1, -1, -1):
        gz = g_a * derivs[l]
        trunk_grads[l] = (gz.T @ acts[l], gz.sum(0))
        trunk_factors[l] = (gz, acts[l])
        g_a = gz @ _f64(trunk[l][0])
    return {"dx": g_a, "trunk": trunk_grads, "heads": head_grads, "factors": trunk_factors + head_factors}


def sequential_f32_error(gz, a, exact_w, exact_b, max_cols=None, chunk=256):
    """Error of dW = sum_p gz[p]^T a[p] and db = sum_p gz[p] when the factors are rounded to float32 and the per-point outer products
    are accumulated in float32 IN POINT ORDER (cumsum is sequential by definition; chunked only to bound memory, the running sum
    carried into each chunk's first row).  max_cols: only the first max_cols input columns (a lower bound of the full maximum)."""
    gz32, a32 = gz.astype(np.float32), a.astype(np.float32)
    cols = a32.shape[1] if max_cols is None else min(max_cols, a32.shape[1])
    acc_w = np.zeros((gz32.shape[1], cols), np.float32)
    acc_b = np.zeros(gz32.shape[1], np.float32)
    for s in range(0, gz32.shape[0], chunk):
        prod = gz32[s:s + chunk, :, None] * a32[s:s + chunk, None, :cols]
        prod[0] += acc_w
        acc_w = np.cumsum(prod, axis=0, dtype=np.float32)[-1]
        col = gz32[s:s + chunk].copy()
        col[0] += acc_b
        acc_b = np.cumsum(col, axis=0, dtype=np.float32)[-1]
    return float(np.abs(acc_w - exact_w[:, :cols]).max()), float(np.abs(acc_b - exact_b).max())
