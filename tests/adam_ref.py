"""Float64 numpy restatement of the Adam step of row f-11 (csrc/optim.hip, hugs_amd/optim.py), per tensor with its own step count:

    m' = m + (g - m) * (1 - b1)
    v' = v * b2 + (1 - b2) * g * g
    p' = p - step_size * (m' / (sqrt(v') / bc2_sqrt + eps)),   step_size = lr / (1 - b1^t),  bc2_sqrt = sqrt(1 - b2^t)

with t the tensor's step count after the increment: the single-tensor, non-capturable form of torch.optim.Adam without weight decay,
amsgrad or maximize.  tests/test_optim.py pins it to torch.optim.Adam(foreach=False) in float64 and shows that two wrong variants
(`variant="swapped_betas"`, `"no_bias_correction"`) break that agreement."""
import math

import numpy as np


def adam_update(p, g, m, v, t, lr, betas, eps, variant=None):
    """One step on float64 arrays; t is the step count AFTER the increment.  Returns the new (p, m, v)."""
    b1, b2 = betas
    if variant == "swapped_betas":
        b1, b2 = b2, b1
    g = np.asarray(g, np.float64)
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    if variant == "no_bias_correction":
        step_size, bc2_sqrt = lr, 1.0
    else:
        step_size, bc2_sqrt = lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)
    p = p - step_size * (m / (np.sqrt(v) / bc2_sqrt + eps))
    return p, m, v


class RefTensor:
    """A parameter with torch's per-parameter state: p, exp_avg, exp_avg_sq in float64 and its own step count (state appears at the
    first step with a gradient)."""

    def __init__(self, p, lr, betas=(0.9, 0.999), eps=1e-8, variant=None):
        self.p = np.array(p, np.float64)
        self.m, self.v, self.t = np.zeros_like(self.p), np.zeros_like(self.p), 0
        self.lr, self.betas, self.eps, self.variant = lr, betas, eps, variant

    def step(self, g):
        if g is None:   # no gradient: no step increment, nothing touched
            return
        self.t += 1
        self.p, self.m, self.v = adam_update(self.p, g, self.m, self.v, self.t, self.lr, self.betas, self.eps, self.variant)

    # the reference's optimizer surgery (scene.py:310-379) on the same state: rows along dimension 0
    def replace(self, p):
        self.p = np.array(p, np.float64)
        self.m, self.v = np.zeros_like(self.p), np.zeros_like(self.p)   # (the step count is carried over)

    def prune(self, mask):
        self.p, self.m, self.v = self.p[mask], self.m[mask], self.v[mask]

    def cat(self, rows):
        rows = np.array(rows, np.float64)
        self.p = np.concatenate((self.p, rows), 0)
        self.m, self.v = np.concatenate((self.m, np.zeros_like(rows)), 0), np.concatenate((self.v, np.zeros_like(rows)), 0)


def gradient(rng, shape, zeros_every=0):
    """float32 gradients whose every element is exactly 0 or has 1e-6 <= |g| <= 1e2 (g * g neither underflows nor overflows in fp32)"""
    n = int(np.prod(shape))
    g = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-5.9, 1.9, n)).astype(np.float32)
    if zeros_every:
        g[::zeros_every] = 0.0
    a = np.abs(g[g != 0])
    assert a.size == 0 or (a.min() >= 1e-6 and a.max() <= 1e2)
    return g.reshape(shape)
