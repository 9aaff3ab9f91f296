#!/usr/bin/env python3
"""Measurement for row f-8 on one MI355X: TriPlane.forward + backward for the 110 210 human Gaussians of a HUGS step
(hugs_trimlp.py:206,408), F = 32, three 256 x 256 planes -- (a) the reference's torch statements on NCHW parameters against
(b) the fused kernels on channels-last parameters.  Both include what a training step pays: the allocation and zeroing of the
planes' gradients and dL/dx.  One hipEvent pair per step (a third event splits forward from backward), the two variants
interleaved step by step, medians.  Points: a person-sized body shell in the canonical box (hugs_amd.synthetic's person:
semi-axes 0.28 x 0.85 x 0.18), and uniform in the box as the second figure.  Prints one JSON line.
    python tools/bench_triplane.py [--steps 100] [--warmup 10]"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-hugs_amd"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

ATOMIC_RATE = 1.3e12   # bytes of float atomic adds per second, chip-wide (measured shape: two 128-byte segments per wave-instruction)


def torch_statements(plane_xy, plane_xz, plane_yz, x, center=0.0, scale=2.0):
    """triplane.py:27-39 without the assertion (a host synchronisation the fused module does not have either by default)"""
    from torch.nn.functional import grid_sample
    x = (x - center) / scale + 0.5
    x = x * 2 - 1
    coords = x.reshape(1, -1, 1, 3)
    feats = [grid_sample(p, coords[..., ax], align_corners=True)[0, :, :, 0].transpose(0, 1)
             for p, ax in ((plane_xy, [0, 1]), (plane_xz, [0, 2]), (plane_yz, [1, 2]))]
    return torch.cat(feats, dim=1)


def person_points(n, rng):
    th, ph = rng.uniform(0, 2 * math.pi, n), np.arccos(rng.uniform(-1, 1, n))
    return np.stack([0.28 * np.sin(ph) * np.cos(th), 0.85 * np.cos(ph) + 0.05, 0.18 * np.sin(ph) * np.sin(th) + 0.004 * rng.standard_normal(n)], 1).astype(np.float32)


def measure(x_np, steps, warmup, dev, features=32, res=256):
    from hugs_amd.triplane import triplane_sample
    gen = torch.Generator(device="cpu").manual_seed(0)
    nchw = [torch.randn(1, features, res, res, generator=gen).to(dev).requires_grad_(True) for _ in range(3)]
    cl = [p.detach().clone().contiguous(memory_format=torch.channels_last).requires_grad_(True) for p in nchw]
    x = torch.from_numpy(x_np).to(dev).requires_grad_(True)
    g = torch.randn(x.shape[0], 3 * features, generator=gen).to(dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def step(fn, planes):
        for t in (*planes, x):
            t.grad = None
        e = (ev(), ev(), ev())
        e[0].record()
        feat = fn(*planes, x)
        e[1].record()
        feat.backward(g)
        e[2].record()
        return e

    variants = {"torch_statements": (torch_statements, nchw), "fused": (triplane_sample, cl)}
    for _ in range(warmup):
        for fn, planes in variants.values():
            step(fn, planes)
    torch.cuda.synchronize()
    events = {k: [] for k in variants}
    for _ in range(steps):                                   # interleaved: both variants see the same moments of the machine
        for k, (fn, planes) in variants.items():
            events[k].append(step(fn, planes))
    torch.cuda.synchronize()
    out = {}
    for k, evs in events.items():
        out[f"{k}_ms"] = round(statistics.median(e[0].elapsed_time(e[2]) for e in evs), 4)
        out[f"{k}_forward_ms"] = round(statistics.median(e[0].elapsed_time(e[1]) for e in evs), 4)
        out[f"{k}_backward_ms"] = round(statistics.median(e[1].elapsed_time(e[2]) for e in evs), 4)
    out["torch_over_fused"] = round(out["torch_statements_ms"] / out["fused_ms"], 2)
    # every in-box point adds 4 corners x 32 channels x 4 bytes to each of the 3 planes
    out["atomic_bytes"] = int(x.shape[0]) * 3 * 4 * features * 4
    out["atomic_floor_ms"] = round(out["atomic_bytes"] / ATOMIC_RATE * 1e3, 4)
    out["fused_backward_fraction_of_atomic_rate"] = round(out["atomic_floor_ms"] / out["fused_backward_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--points", type=int, default=110_210)
    a = ap.parse_args()
    if a.steps < 50:
        ap.error("--steps: at least 50 (medians)")
    from build_id import csrc_sha16
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    out = {"workload": f"TriPlane fwd+bwd, {a.points} points, F=32, 3 x 256x256 fp32; (a) torch statements on NCHW, (b) fused on channels-last; "
                       f"medians of {a.steps} interleaved steps (hipEvents), gradient allocation + zeroing included",
           "points": "person shell"}
    out.update(measure(person_points(a.points, rng), a.steps, a.warmup, dev))
    out["uniform_in_box"] = measure(rng.uniform(-1.0, 1.0, (a.points, 3)).astype(np.float32), a.steps, a.warmup, dev)
    out["atomic_rate_assumed_TBps"] = ATOMIC_RATE / 1e12
    out["csrc_sha16"] = csrc_sha16()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
