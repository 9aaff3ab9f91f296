#!/usr/bin/env python3
"""Measurement for row f-11 on one MI355X: the optimizer step of a joint human + scene training step at C4's sizes.

Tensor sets -- scene: 200 000 Gaussians, the six tensors at SH degree 3, six groups with the reference's learning rates (scene.py:201-213);
human: 110 210 x 3 `xyz`, the three (1, 32, 256, 256) channels-last planes, the three decoders of hugs_amd/decoders.py at 96 features as the
reference constructs them, four small pose tensors, nine groups (hugs_trimlp.py:673-701).  Gradients are preallocated tensors (in their
parameter's layout) attached every iteration; each optimizer's step is followed by zero_grad(set_to_none=True), as the trainer has it
(gs_trainer.py:344-351).  Variants, on parameter sets of their own, alternating in one process:
  (a) torch.optim.Adam(params, lr=0.0, eps=1e-15), the reference's construction (torch picks its foreach path on the GPU)
  (b) the same with fused=True, if this torch build accepts it
  (c) hugs_amd.optim.Adam, one step() per optimizer
  (d) hugs_amd.optim.fused_step(human, scene)
Wall-clock ms per iteration over `--iters` iterations between two synchronisations after `--warmup`, `--rounds` rounds, their median and
spread (max - min); the host's share (time until the loop returns, before the synchronisation); device launches per iteration from a
torch.profiler trace of one iteration; the layout-copy counter per iteration.  The launch counts of (c) and (d) are asserted.
The kernel's own time comes from a rocprofv3 run of its own (no counters in it, the program after `--`):
    rocprofv3 --kernel-trace --stats -d DIR -o adam -- python3 tools/bench_adam.py --trace-steps 100
    python3 profiles/summarize_rocprof.py DIR/adam_results.db > profiles/<tag>_adam_kernel_stats.txt
    python3 tools/bench_adam.py --kernel-stats profiles/<tag>_adam_kernel_stats.txt --out profiles/<tag>_adam.json
--trace-steps runs variant (d) only: every call of the kernel is then one whole step, 28 bytes per parameter."""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ml-hugs_amd", "profiles", "tools"):
    sys.path.insert(0, os.path.join(ROOT, p))

KERNEL = "adam_multi_tensor_kernel"
# hugs_scene.yaml:100-110 / hugs_human_scene.yaml:49-71 (position x the spatial scale)
SCENE_LR = {"xyz": 1.6e-4 * 5.0, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20.0, "opacity": 5e-2, "scaling": 5e-3, "rotation": 1e-3}
HUMAN_LR = {"xyz": 1.6e-4 * 2.0, "v_embed": 1e-3, "geometry_dec": 1e-3, "appearance_dec": 1e-3, "deform_dec": 1e-4, "global_orient": 1e-4,
            "body_pose": 1e-4, "betas": 1e-4, "transl": 1e-4}


def tensor_sets(dev, seed):
    """-> (scene groups, human groups) of fresh parameters"""
    import warnings
    from hugs_amd import decoders as D
    gen = torch.Generator(device="cpu").manual_seed(seed)
    new = lambda *s: torch.nn.Parameter(torch.randn(*s, generator=gen).to(dev))
    P, Ph, frames = 200_000, 110_210, 100
    scene = {"xyz": [new(P, 3)], "f_dc": [new(P, 1, 3)], "f_rest": [new(P, 15, 3)], "opacity": [new(P, 1)], "scaling": [new(P, 3)], "rotation": [new(P, 4)]}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(seed)
        dec = {"geometry_dec": D.GeometryDecoder(96).to(dev), "appearance_dec": D.AppearanceDecoder(96).to(dev), "deform_dec": D.DeformationDecoder(96).to(dev)}
    planes = [torch.nn.Parameter(torch.randn(1, 32, 256, 256, generator=gen).to(dev).contiguous(memory_format=torch.channels_last)) for _ in range(3)]
    human = {"xyz": [new(Ph, 3)], "v_embed": planes, **{k: list(m.parameters()) for k, m in dec.items()},
             "global_orient": [new(frames, 3)], "body_pose": [new(frames, 69)], "betas": [new(10)], "transl": [new(frames, 3)]}
    groups = lambda d, lr: [{"params": ps, "lr": lr[k], "name": k} for k, ps in d.items()]
    return groups(scene, SCENE_LR), groups(human, HUMAN_LR)


def copy_rate(dev, nbytes=1 << 30, reps=10):
    """GB/s (read + write) of the library's float4-per-thread device-to-device copy on this GPU, now: the practical HBM ceiling"""
    import diff_gaussian_rasterization as dgr
    lib = dgr._load()
    a = torch.empty(nbytes // 4, dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    copy = lambda: lib.hgs_copy_bandwidth(b.data_ptr(), a.data_ptr(), nbytes, stream)
    for _ in range(3):
        copy()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        copy()
    e1.record()
    e1.synchronize()
    return 2.0 * nbytes * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9


class Variant:
    def __init__(self, name, dev, make, fused_pair=False):
        self.name = name
        scene, human = tensor_sets(dev, seed=1)
        self.opts = [make(human), make(scene)]   # the trainer steps the human's optimizer first
        self.params = [[p for g in o.param_groups for p in g["params"]] for o in self.opts]
        self.fused_pair = fused_pair

    def attach(self, grads):
        for ps, gs in zip(self.params, grads):
            for p, g in zip(ps, gs):
                p.grad = g

    def iteration(self, grads):
        self.attach(grads)
        if self.fused_pair:
            from hugs_amd.optim import fused_step
            fused_step(*self.opts)
            for o in self.opts:
                o.zero_grad(set_to_none=True)
        else:
            for o in self.opts:
                o.step()
                o.zero_grad(set_to_none=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-steps", type=int, default=0, help="run variant (d) this many times and exit (for a rocprofv3 kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="summarize_rocprof.py's text of such a trace: the kernel's own time goes into the line")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from build_id import csrc_sha16
    from hugs_amd import optim as O
    dev = torch.device("cuda:0")
    ours = lambda groups: O.Adam(groups, lr=0.0, eps=1e-15)
    d = Variant("d_fused_step", dev, ours, fused_pair=True)
    # gradients in their parameter's layout (what the fused rows' backward hands over), shared by the variants: no variant writes them
    gen = torch.Generator(device="cpu").manual_seed(2)
    grads = [[torch.empty_like(p).copy_(torch.randn(p.shape, generator=gen) * 1e-2) for p in ps] for ps in d.params]
    n_params = sum(p.numel() for ps in d.params for p in ps)
    n_tensors = [len(ps) for ps in d.params]

    if a.trace_steps:
        for _ in range(a.trace_steps):
            d.iteration(grads)
        torch.cuda.synchronize()
        print(json.dumps({"traced": "d_fused_step", "steps": a.trace_steps, "parameters": n_params, "tensors": n_tensors}))
        return

    variants = [Variant("a_torch", dev, lambda g: torch.optim.Adam(g, lr=0.0, eps=1e-15))]
    fused_note = None
    try:
        b = Variant("b_torch_fused", dev, lambda g: torch.optim.Adam(g, lr=0.0, eps=1e-15, fused=True))
        b.iteration(grads)
        torch.cuda.synchronize()
        variants.append(b)
    except Exception as e:   # recorded, not hidden: this build's fused path does not take these tensors
        fused_note = f"unavailable: {type(e).__name__}: {str(e)[:200]}"
    variants += [Variant("c_hip_per_optimizer", dev, ours), d]

    def timed(v):
        for _ in range(a.warmup):
            v.iteration(grads)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            v.iteration(grads)
        host = time.perf_counter() - t0
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.iters * 1e3, host / a.iters * 1e3

    def launches(v):
        from torch.profiler import ProfilerActivity, profile
        v.iteration(grads)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            v.iteration(grads)
            torch.cuda.synchronize()
        events = list(prof.events())
        # a record_function range around kernels (Optimizer.step's own) is mirrored on the device side as an annotation of the same name: not a launch
        host_names = {e.name for e in events if not str(e.device_type).endswith("CUDA")}
        names = [e.name for e in events if str(e.device_type).endswith("CUDA") and e.name not in host_names and not e.name.startswith("Optimizer.step#")]
        return len(names), len([n for n in names if KERNEL in n])

    out = {"workload": f"Adam step of the human optimizer ({n_tensors[0]} tensors, 9 groups) and the scene optimizer ({n_tensors[1]} tensors, 6 groups), "
                       f"{n_params} fp32 parameters, eps 1e-15, gradients re-attached and zero_grad(set_to_none=True) every iteration; wall-clock ms per "
                       f"iteration over {a.iters} iterations after {a.warmup}, median of {a.rounds} rounds, spread = max - min",
           "parameters": n_params, "tensors": n_tensors, "b_torch_fused": fused_note or "available"}
    reps = {v.name: [] for v in variants}
    host = {v.name: [] for v in variants}
    for _ in range(a.rounds):                                   # alternating: every variant sees the same moments of the machine
        for v in variants:
            ms, h = timed(v)
            reps[v.name].append(ms), host[v.name].append(h)
    for v in variants:
        r = reps[v.name]
        out[f"{v.name}_ms"] = round(statistics.median(r), 4)
        out[f"{v.name}_spread_ms"] = round(max(r) - min(r), 4)
        out[f"{v.name}_rounds_ms"] = [round(x, 4) for x in r]
        out[f"{v.name}_host_ms"] = round(statistics.median(host[v.name]), 4)
    for v in variants:
        O.layout_copies(reset=True)
        total, own = launches(v)
        out[f"{v.name}_device_launches"] = total
        out[f"{v.name}_own_kernel_launches"] = own
        out[f"{v.name}_layout_copies_per_iteration"] = O.layout_copies(reset=True) / 2
    out["launch_counts_from"] = "torch.profiler, one iteration, device-side events (kernels and memory operations; the device-side mirrors of record_function ranges are not counted)"
    spread = max(out["a_torch_spread_ms"], out["c_hip_per_optimizer_spread_ms"])
    out["a_over_c"] = round(out["a_torch_ms"] / out["c_hip_per_optimizer_ms"], 2)
    out["c_is_faster_than_a_by_more_than_the_spread"] = bool(out["a_torch_ms"] - out["c_hip_per_optimizer_ms"] > spread)
    rate = copy_rate(dev)
    out["algorithmic_bytes_per_step"] = 28 * n_params
    out["copy_rate_measured_GBps"] = round(rate, 1)
    out["ideal_step_us_at_the_copy_rate"] = round(28 * n_params / rate * 1e-3, 1)
    if a.kernel_stats:
        for line in open(a.kernel_stats):
            m = re.match(r"\s*(\d+)\s+([\d.]+)\s+([\d.]+)\s+[\d.]+\s+.*" + KERNEL, line)
            if m:
                us = float(m.group(3))
                out.update({"kernel_us_traced": us, "kernel_calls_traced": int(m.group(1)), "kernel_stats_file": os.path.basename(a.kernel_stats),
                            "kernel_GBps": round(28 * n_params / us * 1e-3, 1), "kernel_frac_of_copy_rate": round(28 * n_params / us * 1e-3 / rate, 3)})
    out["csrc_sha16"] = csrc_sha16()
    try:
        import bench_common
        out["box"] = bench_common.box()
    except Exception:
        pass
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    # one launch per optimizer, one for both: from the profiler's count (after the line is out, so that a failure here keeps the figures)
    assert out["c_hip_per_optimizer_own_kernel_launches"] == 2 == out["c_hip_per_optimizer_device_launches"], "(c) must be one launch per optimizer"
    assert out["d_fused_step_own_kernel_launches"] == 1 == out["d_fused_step_device_launches"], "(d) must be one launch"


if __name__ == "__main__":
    main()
