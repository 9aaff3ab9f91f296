#!/usr/bin/env python3
"""Measurement for row f-10 on one MI355X: the SMPL body model's forward + backward at V = 6 890, J = 24, NB = 10 -- (a) the fused
call (hugs_amd.smpl.smpl_forward: three launches forward, seven backward) against (b) the torch-statement form (tests/smpl_ref.py's
float32 restatement of the same formulas, torch ops on the GPU), on equal buffers and inputs, gradients to betas, pose and the
translation, cotangents on A and on the vertices.  With and without disable_posedirs.

The work is launch-bound, so the figure is wall-clock: `--iters` iterations between two synchronisations, divided by their number,
after `--warmup` iterations; `--repeats` repeats, their median and spread (max - min).  Launch counts come from a torch.profiler
trace of one iteration of each form, taken after the timing (no counters are collected).  Prints one JSON line; --out also writes it.
    python tools/bench_smpl.py [--iters 200] [--warmup 20] [--repeats 3] [--out profiles/<tag>_smpl.json]"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ml-hugs_amd", "profiles", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--vertices", type=int, default=6890)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import smpl_ref as sr
    from build_id import csrc_sha16
    from hugs_amd.smpl import smpl_forward
    dev = torch.device("cuda:0")
    V, J, NB = a.vertices, 24, 10
    model = sr.torch_model(sr.synthetic_model(1, V, J, NB, "smpl"), dev)
    model["parents_list"] = model["parents"].tolist()
    ns = SimpleNamespace(**model)
    betas, pose, transl = (torch.from_numpy(x).to(dev).requires_grad_() for x in sr.synthetic_inputs(1, J, NB))
    cot = {k: torch.from_numpy(v).to(dev) for k, v in sr.cotangents(1, V, J).items() if k in ("A", "verts")}

    def fused(disable):
        o = smpl_forward(ns, betas, pose[:, 3:], pose[:, :3], transl, disable_posedirs=disable)
        return o.A, o.vertices

    def statements(disable):
        o = sr.smpl_torch(dict(model, parents=model["parents_list"]), betas, pose, transl, disable)   # (the tree as a host list: no per-joint sync)
        return o["A"], o["verts"]

    def step(fn, disable):
        for t in (betas, pose, transl):
            t.grad = None
        A, verts = fn(disable)
        torch.autograd.backward([A, verts], [cot["A"], cot["verts"]])

    def timed(fn, disable):
        for _ in range(a.warmup):
            step(fn, disable)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            step(fn, disable)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.iters * 1e3

    def launches(fn, disable):
        from torch.profiler import ProfilerActivity, profile
        step(fn, disable)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step(fn, disable)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
        return len(names), len([n for n in names if "smpl_" in n or "lbs_skin" in n])

    out = {"workload": f"SMPL forward + backward, V={V} J={J} NB={NB} fp32, gradients to betas / pose / transl, cotangents on A and verts; "
                       f"(a) fused kernels, (b) torch statements on the GPU; wall-clock ms per iteration over {a.iters} iterations after "
                       f"{a.warmup} warm-up, median of {a.repeats} repeats, spread = max - min"}
    for disable in (False, True):
        tag = "posedirs_disabled" if disable else "posedirs"
        reps = {"fused": [], "torch_statements": []}
        for _ in range(a.repeats):                               # interleaved: both forms see the same moments of the machine
            for k, fn in (("fused", fused), ("torch_statements", statements)):
                reps[k].append(timed(fn, disable))
        for k, v in reps.items():
            out[f"{tag}_{k}_ms"] = round(statistics.median(v), 4)
            out[f"{tag}_{k}_spread_ms"] = round(max(v) - min(v), 4)
            out[f"{tag}_{k}_repeats_ms"] = [round(x, 4) for x in v]
        out[f"{tag}_torch_over_fused"] = round(out[f"{tag}_torch_statements_ms"] / out[f"{tag}_fused_ms"], 2)
        out[f"{tag}_fused_is_faster_by_more_than_the_spread"] = bool(
            out[f"{tag}_torch_statements_ms"] - out[f"{tag}_fused_ms"] > max(out[f"{tag}_fused_spread_ms"], out[f"{tag}_torch_statements_spread_ms"]))
    for disable in (False, True):
        tag = "posedirs_disabled" if disable else "posedirs"
        for k, fn in (("fused", fused), ("torch_statements", statements)):
            total, own = launches(fn, disable)
            out[f"{tag}_{k}_device_launches"] = total
            if k == "fused":
                out[f"{tag}_fused_own_kernel_launches"] = own
    out["launch_counts_from"] = "torch.profiler, one iteration, device-side events (kernels and memory operations)"
    out["csrc_sha16"] = csrc_sha16()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
