#!/usr/bin/env python3
"""Measurement for row f-9 on one MI355X: the three human decoders of a HUGS step (hugs_trimlp.py:409-410,430) on the 110 210 x 96
triplane features, forward + backward -- (a) the reference's torch statements (Linear, GELU, sigmoid; weight norm on
skinning_linear) against (b) the fused kernels of hugs_amd.decoders, on equal parameters.  Both include what a training step pays:
the allocation and zeroing of every gradient.  One hipEvent pair per step (a third event splits forward from backward), the two
variants interleaved step by step, medians.  Peak memory: torch.cuda.max_memory_allocated over one step of each variant, above what
was allocated before it.  Prints one JSON line.
    python tools/bench_decoders.py [--steps 100] [--warmup 10]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-hugs_amd"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

F32_MATRIX_PEAK_TFLOPS = 157.3     # v_mfma_f32_32x32x2_f32: 64 FLOP / clk / SIMD x 1024 SIMDs x 2.4 GHz
MACS_PER_POINT = {"appearance": 96 * 64 + 64 * 64 + 64 * 49, "geometry": 96 * 128 + 128 * 128 + 128 * 12,
                  "deformation": 96 * 128 + 2 * 128 * 128 + 128 * 24}   # (96 -> 128, then net.2 and skinning_linear at 128 x 128, then the 24 columns)


def torch_statements(mods, x):
    """decoders.py:38-43, 72-84, 102-111 on the fused modules' own submodule trees (the same parameters, the reference's statements)"""
    a, g, d = mods
    h = a.net(x)
    out = [a.shs(h), a.opacity(h)]
    out += [g.xyz(x), g.rotations(x), F.gelu(g.scales(x))]
    h = d.net(x)
    out.append(F.gelu(d.skinning(F.gelu(d.skinning_linear(h)))))
    return out


def fused(mods, x):
    return [v for m in mods for v in m(x).values() if v is not None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--points", type=int, default=110_210)
    a = ap.parse_args()
    if a.steps < 50:
        ap.error("--steps: at least 50 (medians)")
    from build_id import csrc_sha16
    from hugs_amd.decoders import AppearanceDecoder, DeformationDecoder, GeometryDecoder
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mods = [AppearanceDecoder(96).to(dev), GeometryDecoder(96).to(dev), DeformationDecoder(96, disable_posedirs=True).to(dev)]
    params = [p for m in mods for p in m.parameters()]
    x = torch.randn(a.points, 96, device=dev).requires_grad_(True)
    gs = [torch.randn(a.points, w, device=dev) for w in (48, 1, 3, 6, 3, 24)]
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def step(fn):
        for t in (*params, x):
            t.grad = None
        e = (ev(), ev(), ev())
        e[0].record()
        outs = fn(mods, x)
        e[1].record()
        torch.autograd.backward(outs, gs)
        e[2].record()
        return e

    variants = {"torch_statements": torch_statements, "fused": fused}
    for _ in range(a.warmup):
        for fn in variants.values():
            step(fn)
    torch.cuda.synchronize()
    events = {k: [] for k in variants}
    for _ in range(a.steps):                                     # interleaved: both variants see the same moments of the machine
        for k, fn in variants.items():
            events[k].append(step(fn))
    torch.cuda.synchronize()
    macs = sum(MACS_PER_POINT.values()) * a.points
    out = {"workload": f"the three human decoders fwd+bwd, {a.points} points x 96 features fp32; (a) torch statements, (b) fused kernels; "
                       f"medians of {a.steps} interleaved steps (hipEvents), gradient allocation + zeroing included",
           "forward_gflop": round(2 * macs / 1e9, 2), "forward_backward_gflop": round(6 * macs / 1e9, 2),
           "fused_executed_gflop": round(8 * macs / 1e9, 2)}     # the fused backward recomputes the forward
    for k, evs in events.items():
        out[f"{k}_ms"] = round(statistics.median(e[0].elapsed_time(e[2]) for e in evs), 4)
        out[f"{k}_forward_ms"] = round(statistics.median(e[0].elapsed_time(e[1]) for e in evs), 4)
        out[f"{k}_backward_ms"] = round(statistics.median(e[1].elapsed_time(e[2]) for e in evs), 4)
        out[f"{k}_tflops"] = round(6 * macs / (out[f"{k}_ms"] * 1e-3) / 1e12, 2)     # algorithmic FLOP (no recomputation counted) per second
    out["fused_executed_tflops"] = round(8 * macs / (out["fused_ms"] * 1e-3) / 1e12, 2)
    out["fused_executed_fraction_of_f32_matrix_peak"] = round(out["fused_executed_tflops"] / F32_MATRIX_PEAK_TFLOPS, 3)
    out["f32_matrix_peak_tflops"] = F32_MATRIX_PEAK_TFLOPS
    out["torch_over_fused"] = round(out["torch_statements_ms"] / out["fused_ms"], 2)
    for k, fn in variants.items():                               # peak memory of one step above what lives across steps
        for t in (*params, x):
            t.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        step(fn)
        torch.cuda.synchronize()
        out[f"{k}_peak_memory_MB"] = round((torch.cuda.max_memory_allocated(dev) - base) / 1e6, 1)
    out["csrc_sha16"] = csrc_sha16()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
