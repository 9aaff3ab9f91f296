#!/usr/bin/env python3
"""Measurement for the alpha / depth maps on one MI355X, forward + backward per step:
  (a) colour only;
  (b) colour + maps through return_alpha_depth=True, all three in the loss;
  (c) what a user did before the flag: the colour render plus a second render of colours (z, 1, 0) on black, the z statement
      (means3D @ V[:3, 2] + V[3, 2]) counted.
Workloads: bench.py's own scene (200 000 Gaussians, 1920x1080, SH degree 3) and the 110 210-Gaussian human at 512x512 of
tools/bench_c3.py.  Warm-up per variant, then the three variants alternate in one process: `--repeats` rounds (at least 5) of
`--steps` steps (at least 200) each, wall clock around a drained GPU.  Reported: the median over the rounds per variant, the spread
(max - min) of the rounds, and (b - a) / (c - a).  Prints one JSON line.
    python tools/bench_maps.py [--steps 200] [--repeats 5]
    python tools/bench_maps.py --trace-steps 100     # variant (b) on the 200 000-Gaussian frame only: the run to put under
                                                     # rocprofv3 --kernel-trace --stats for the three kernels' times"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-hugs_amd"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer   # noqa: E402
from hugs_amd import synthetic as syn                                                       # noqa: E402


def scene_workload(dev):
    """bench.py's scene"""
    P, H, W, D = 200_000, 1080, 1920, 3
    cam = syn.pinhole_camera(H, W)
    g = syn.scene_gaussians(P, cam, seed=0, sigma_px=4.0)
    return "200 000 Gaussians, 1920x1080, SH degree 3 (bench.py's scene)", g, cam, H, W, D, syn.pixel_grad(H, W)


def human_workload(dev):
    """tools/bench_c3.py's human"""
    P, S = 110_210, 512
    rng = np.random.default_rng(5)
    q = rng.standard_normal((P, 4))
    g = {"means3D": (rng.standard_normal((P, 3)) * np.array([0.22, 0.55, 0.14])).astype(np.float32),
         "scales": (0.035 / math.sqrt(P / 6890.0) * np.exp(0.3 * rng.standard_normal((P, 3)))).astype(np.float32),
         "rotations": (q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.8, 1.2, (P, 1))).astype(np.float32),
         "shs": (0.3 * rng.standard_normal((P, 16, 3))).astype(np.float32), "opacities": rng.uniform(0.05, 1.0, (P, 1)).astype(np.float32)}
    cam = syn.rotating_camera(3, 10, dist=5.0, fov=0.4, img_size=S)
    return "110 210 human Gaussians, 512x512, SH degree 0, rotating rig (tools/bench_c3.py)", g, cam, S, S, 0, \
        (rng.standard_normal((3, S, S)) * 1e-3).astype(np.float32)


def variants_of(workload, dev):
    _, g, cam, H, W, D, dL = workload
    d = lambda a, grad=False: torch.from_numpy(np.ascontiguousarray(a)).float().to(dev).requires_grad_(grad)
    t = {k: d(g[k], True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    P = t["means3D"].shape[0]
    means2D = torch.zeros(P, 3, device=dev, requires_grad=True)
    V = d(np.asarray(cam["world_view_transform"], np.float32).reshape(4, 4))
    common = dict(image_height=H, image_width=W, tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), scale_modifier=1.0,
                  viewmatrix=V, projmatrix=d(cam["full_proj_transform"]), sh_degree=D, campos=d(cam["camera_center"]), prefiltered=False,
                  debug=False)
    white = GaussianRasterizationSettings(bg=torch.ones(3, device=dev), **common)
    black = GaussianRasterizationSettings(bg=torch.zeros(3, device=dev), **common)
    rng = np.random.default_rng(9)
    scale = float(np.abs(dL).mean())
    gA, gD = (d((rng.standard_normal((1, H, W)) * scale).astype(np.float32)) for _ in range(2))
    g3 = torch.cat([gD, gA, torch.zeros_like(gA)], 0)
    dLd = d(dL)
    leaves = list(t.values()) + [means2D]
    geom = dict(means3D=t["means3D"], means2D=means2D, opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])

    def done():
        for x in leaves:
            x.grad = None

    def colour_only():
        color, _ = GaussianRasterizer(white)(shs=t["shs"], **geom)
        color.backward(dLd)
        done()

    def with_maps():
        color, _, alpha, depth = GaussianRasterizer(white)(shs=t["shs"], return_alpha_depth=True, **geom)
        torch.autograd.backward([color, alpha, depth], [dLd, gA, gD])
        done()

    def second_render():
        color, _ = GaussianRasterizer(white)(shs=t["shs"], **geom)
        z = t["means3D"] @ V[:3, 2] + V[3, 2]
        img, _ = GaussianRasterizer(black)(colors_precomp=torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], 1), **geom)
        torch.autograd.backward([color, img], [dLd, g3])
        done()

    return {"a_colour_only": colour_only, "b_colour_and_maps": with_maps, "c_colour_and_second_render": second_render}


def timed(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def measure(workload, dev, steps, repeats, warmup):
    variants = variants_of(workload, dev)
    for step in variants.values():
        for _ in range(warmup):
            step()
    rounds = {k: [] for k in variants}
    for _ in range(repeats):   # the variants alternate: each round sees the same moments of the machine
        for k, step in variants.items():
            rounds[k].append(timed(step, steps))
    out = {"workload": workload[0]}
    for k, ms in rounds.items():
        out[k + "_ms"] = round(statistics.median(ms), 4)
        out[k + "_spread_ms"] = round(max(ms) - min(ms), 4)
        out[k + "_rounds_ms"] = [round(x, 4) for x in ms]
    a, b, c = (out[k + "_ms"] for k in variants)
    out["maps_cost_ms"] = round(b - a, 4)
    out["second_render_cost_ms"] = round(c - a, 4)
    out["maps_over_second_render"] = round((b - a) / (c - a), 3) if c > a else None
    out["largest_spread_ms"] = max(out[k + "_spread_ms"] for k in variants)
    out["b_below_c_by_more_than_the_spread"] = bool(c - b > out["largest_spread_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--trace-steps", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.trace_steps:
        step = variants_of(scene_workload(dev), dev)["b_colour_and_maps"]
        for _ in range(a.trace_steps):
            step()
        torch.cuda.synchronize()
        return
    if a.steps < 200 or a.repeats < 5:
        ap.error("at least 5 repeats of at least 200 steps")
    from build_id import csrc_sha16
    out = {"protocol": f"fwd+bwd per step; warm-up {a.warmup} steps per variant; {a.repeats} rounds of {a.steps} steps per variant, the variants "
                       "alternating in one process; wall clock around a drained GPU; median over the rounds, spread = max - min of the rounds",
           "scene_200k_1080p": measure(scene_workload(dev), dev, a.steps, a.repeats, a.warmup),
           "human_110k_512": measure(human_workload(dev), dev, a.steps, a.repeats, a.warmup),
           "csrc_sha16": csrc_sha16()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
