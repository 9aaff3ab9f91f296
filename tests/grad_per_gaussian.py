"""A gradient held Gaussian by Gaussian against the fp64 oracle (imported by tests/test_gpu_grad_per_gaussian.py; numpy only).

A relative L2 norm over a whole gradient tensor is a statement about its few strongest rows: within one tensor the per-Gaussian norms
of visible Gaussians span four to seven decades, and a 1 % error on every row below 3 % of the largest stays under 1e-3 of the tensor.
The measure here weighs every visible Gaussian's row by its OWN norm, with a floor so that rows of (nearly) no gradient are not asked
for digits they do not have:

    n_i = ||r_i||2,  d_i = ||g_i - r_i||2,  s_i = d_i / (n_i + PHI * max_{j visible} n_j)          g under test, r the fp64 oracle's

and the bar is never chosen: it is F x the distance of the fp32 restatement of the same algorithm (the C oracle built with REAL=float)
from the fp64 one, on the same frame and tensor, for the largest and for the median s_i (hold()).
"""
import numpy as np

PHI = 1e-3               # the floor: with 1e-3 the fp32 oracle's worst s_i over the module's frames is 6.4e-4, with 1e-5 it is 8.8e-3
MAX_SLACK, MEDIAN_SLACK = 1e-6, 1e-7
MAX_SET_ASIDE = 3        # Gaussians behind a pixel on the other side of a threshold (tests/test_gpu_fuzz.py's allowance)
FLIP_COLOUR_FACTOR = 16  # a pixel is flipped where its colour is further from the fp64 oracle's than 16 x the fp32 oracle's worst pixel
SH_BANDS = ((0, 1), (1, 4), (4, 9), (9, 16))   # coefficients of degree 0, 1, 2, 3


def rows(name, g):
    """the tensor as [P, k] float64; of means2D the two screen columns (the third is identically zero and asserted so elsewhere)"""
    g = np.asarray(g, np.float64)
    g = g.reshape(g.shape[0], -1)
    return g[:, :2] if name == "means2D" else g


def split(name, g, D=None):
    """[(label, [P, k] float64)]: the tensor itself and, for SH coefficients [P, M, 3], each degree band up to degree D as a tensor of
    its own (a wrong constant in one band must not be averaged into the DC term)"""
    out = [(name, rows(name, g))]
    if name == "shs":
        g = np.asarray(g, np.float64)
        for lo, hi in SH_BANDS:
            if lo < (D + 1) ** 2 and hi <= g.shape[1]:
                out.append((f"shs[{lo}:{hi}]", g[:, lo:hi].reshape(g.shape[0], -1)))
    return out


def scores(g, r, vis):
    """s_i of every visible Gaussian (in index order), or None where the reference has no gradient at all (not an input of the frame)"""
    n = np.linalg.norm(r, axis=1)
    top = float(n[vis].max()) if vis.any() else 0.0
    if not top > 0.0:
        return None
    return np.linalg.norm(g - r, axis=1)[vis] / (n[vis] + PHI * top)


def hold(s, s_ref, F, may_leave_out=None):
    """The bar on scores `s` given the fp32 oracle's `s_ref`:  max s <= F max s_ref + 1e-6  and  median s <= F median s_ref + 1e-7.
    `may_leave_out` (bool per visible Gaussian): at most MAX_SET_ASIDE of those beyond the bar are left out of the MAX; the median is
    always over all.  Returns dict(err, err_ref, med, med_ref, ratio, med_ratio, left_out, ok)."""
    err_ref, med_ref = float(s_ref.max()), float(np.median(s_ref))
    bar = F * err_ref + MAX_SLACK
    keep = np.ones(s.shape, bool)
    if may_leave_out is not None:
        cand = np.flatnonzero((s > bar) & may_leave_out)
        keep[cand[np.argsort(-s[cand])][:MAX_SET_ASIDE]] = False
    err, med = float(s[keep].max()), float(np.median(s))
    return dict(err=err, err_ref=err_ref, med=med, med_ref=med_ref, ratio=err / err_ref if err_ref > 0 else float("inf") if err > 0 else 0.0,
                med_ratio=med / med_ref if med_ref > 0 else float("inf") if med > 0 else 0.0, left_out=int((~keep).sum()),
                worst=int(np.argmax(np.where(keep, s, -1.0))), ok=bool(err <= bar and med <= F * med_ref + MEDIAN_SLACK))


def flipped_pixels(n_contrib, images, ref64, ref32):
    """[H, W] bool: the flipped pixels.  n_contrib = (the tested run's, the fp64 oracle's): flipped where they differ.  images / ref64 /
    ref32: lists of arrays [..., H, W] in the same order (colour, or a map): flipped where the tested image lies further from the fp64
    oracle's than FLIP_COLOUR_FACTOR x the fp32 oracle's largest difference on this frame."""
    got, want = n_contrib
    out = np.asarray(got).astype(np.int64) != np.asarray(want).astype(np.int64)
    for a, b, c in zip(images, ref64, ref32):
        tol = FLIP_COLOUR_FACTOR * float(np.abs(np.asarray(c, np.float64) - b).max())
        d = np.abs(np.asarray(a, np.float64) - b) > tol
        out |= d.reshape((-1,) + d.shape[-2:]).any(axis=0)
    return out


def behind_flipped(flipped, ranges, values, P):
    """[P] bool: the Gaussians in the sorted list of a 16 x 16 tile that holds a flipped pixel (ranges / values: the oracle's lists)"""
    H, W = flipped.shape
    gx = (W + 15) // 16
    ys, xs = np.nonzero(flipped)
    out = np.zeros(P, bool)
    for t in np.unique((ys // 16) * gx + xs // 16):
        out[np.asarray(values[int(ranges[t, 0]):int(ranges[t, 1])], np.int64)] = True
    return out


# ---- the two errors a tensor-wide 1e-3 lets through (applied to the fp32 oracle's gradients by the CPU tests)
def mutate_weak_rows(m):
    """(a) every row whose norm is below 3 % of the tensor's largest, times 1.01"""
    m = m.copy()
    n = np.linalg.norm(m, axis=1)
    m[n < 0.03 * n.max()] *= 1.01
    return m


def mutate_drop_median(m, vis):
    """(b) the row of the visible Gaussian of median non-zero norm, set to zero"""
    m = m.copy()
    n = np.linalg.norm(m, axis=1)
    idx = np.flatnonzero(vis & (n > 0))
    m[idx[np.argsort(n[idx], kind="stable")][len(idx) // 2]] = 0.0
    return m
