#!/usr/bin/env python3
"""Measurement for row f-12 on one MI355X: one densification round (clone, split, prune, optimizer surgery, statistics).

Workloads -- scene: 200 000 Gaussians at SH degree 3, the six parameter groups of scene.py:201-208 with Adam state present; human:
110 210 Gaussians, the `xyz` group with Adam state, scaling_multiplier and the three tmp tensors of hugs_trimlp.py:861-863.  About 10 %
of the rows are cloned, 5 % split and 5 % pruned (drawn once per workload, the same rows for both variants).  Variants:
  (a) the reference's torch statements: tests/densify_ref.py in fp32 on the GPU, drawing its noise with torch.normal as the reference does
  (b) hugs_amd.densify.densify_and_prune_scene / densify_and_prune_human
Per round the inputs are freshly cloned (untimed); the round runs between two synchronisations: wall-clock ms per round INCLUDING its
host synchronisations (the round is synchronisation-bound: device time alone would flatter the torch statements), median of `--rounds`
after `--warmup`, spread = max - min.  From a torch.profiler trace of one round: device time (sum of the device-side events) and
launches (kernels and memory operations).  Host synchronisations: what torch.cuda.set_sync_debug_mode("warn") reports during one round.
Peak memory: the allocator's high-water mark above what was allocated when the round began.  The scatter's bytes (every source row read
once, every result row written once) are set against the library's measured copy rate, as bench_adam.py does for the Adam step."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("ml-hugs_amd", "profiles", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

SCATTER = "densify_scatter_kernel"


def workload(flavour, n, seed):
    """a fixture in tests/densify_ref.py's format: ~10 % cloned, ~5 % split, ~5 % pruned by opacity, the rest stays"""
    import densify_ref as ref
    rng = np.random.default_rng(seed)
    u = lambda lo, hi: rng.uniform(lo, hi, n)
    kind = rng.choice(4, n, p=(0.80, 0.10, 0.05, 0.05))          # stays, clone, split, pruned
    g = np.where((kind == 1) | (kind == 2), u(1.3, 8.0), u(0.05, 0.8)) * ref.MAX_GRAD
    top = np.where(kind == 1, u(0.2, 0.9), u(1.2, 6.0)) * ref.SMALL_T
    mid = top * np.where(kind == 2, u(0.1, 0.45), u(0.55, 0.95))
    scales = np.stack((top, mid, mid * u(0.3, 1.0)), 1)
    o = np.where(kind == 3, u(1e-4, 0.9 * ref.MIN_OPACITY), u(0.02, 0.99))
    denom = rng.integers(1, 31, n).astype(np.float64)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    quat = rng.normal(size=(n, 4))
    fx = {"flavour": flavour, "n": n, "xyz": f32(rng.normal(size=(n, 3)) * 2), "accum": f32((g * denom)[:, None]), "denom": f32(denom[:, None]),
          "radii": f32(rng.integers(0, 19, n)),
          "args": dict(max_grad=ref.MAX_GRAD, min_opacity=ref.MIN_OPACITY, extent=ref.EXTENT, max_screen_size=ref.SCREEN, max_n_gs=None,
                       percent_dense=ref.PERCENT_DENSE)}
    if flavour == ref.SCENE:
        fx.update(f_dc=f32(rng.normal(size=(n, 1, 3))), f_rest=f32(rng.normal(size=(n, 15, 3)) * 0.1), opacity=f32(np.log(o / (1 - o))[:, None]),
                  scaling=f32(np.log(scales)), rotation=f32(quat))
    else:
        q = quat / np.linalg.norm(quat, axis=1, keepdims=True)
        fx.update(scaling_multiplier=f32(u(0.5, 2.0)[:, None]), opacity=f32(o[:, None]), scales_canon=f32(scales),
                  rotmat_canon=f32(ref.build_rotation(torch.from_numpy(q)).numpy()))
    return fx, {"stays": int((kind == 0).sum()), "cloned": int((kind == 1).sum()), "split": int((kind == 2).sum()), "pruned": int((kind == 3).sum())}


class Variant:
    def __init__(self, name, fx, dev):
        import densify_ref as ref
        self.name, self.fx, self.dev, self.ref = name, fx, dev, ref
        self.master = ref.instantiate(fx, torch.float32, dev)      # never run on: every round clones it
        self.gen = torch.Generator(device=dev).manual_seed(1)

    def fresh(self):
        ref, m = self.ref, self.master
        c = lambda t: t.detach().clone()
        groups = []
        for group in m["optimizer"].param_groups:
            groups.append({"params": [torch.nn.Parameter(c(p)) for p in group["params"]], "lr": group["lr"], "name": group["name"]})
        opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        for old, new in zip(m["optimizer"].param_groups, opt.param_groups):
            for p, q in zip(old["params"], new["params"]):
                st = m["optimizer"].state[p]
                opt.state[q] = {"step": st["step"].clone(), "exp_avg": c(st["exp_avg"]), "exp_avg_sq": c(st["exp_avg_sq"])}
        inst = {"optimizer": opt, "params": {g["name"]: g["params"][0] for g in opt.param_groups}, "stats": tuple(c(t) for t in m["stats"])}
        if self.fx["flavour"] == ref.HUMAN:
            inst.update(scaling_multiplier=c(m["scaling_multiplier"]), human_gs_out={k: c(v) for k, v in m["human_gs_out"].items()})
        return inst

    def round(self, inst):
        from hugs_amd import densify as D
        ref, a = self.ref, self.fx["args"]
        if self.name == "a_torch":
            if self.fx["flavour"] == ref.SCENE:
                return ref.scene_round(inst["optimizer"], inst["stats"], None, self.gen, **a)[0]["xyz"].shape[0]
            return ref.human_round(inst["optimizer"], inst["scaling_multiplier"], inst["human_gs_out"], inst["stats"], None, self.gen, **a)[0]["xyz"].shape[0]
        if self.fx["flavour"] == ref.SCENE:
            return D.densify_and_prune_scene(inst["params"], inst["optimizer"], inst["stats"], generator=self.gen, **a)[0]["xyz"].shape[0]
        return D.densify_and_prune_human(inst["params"]["xyz"], inst["scaling_multiplier"], inst["human_gs_out"], inst["optimizer"], inst["stats"],
                                         generator=self.gen, **a)[0]["xyz"].shape[0]

    def timed(self):
        """-> (wall ms of one round between two synchronisations, rows afterwards, peak bytes above the start)"""
        inst = self.fresh()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(self.dev)
        base = torch.cuda.memory_allocated(self.dev)
        t0 = time.perf_counter()
        rows = self.round(inst)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, rows, torch.cuda.max_memory_allocated(self.dev) - base

    def traced(self):
        """-> (device us, launches, scatter kernel us or None) of one round, from torch.profiler"""
        from torch.profiler import ProfilerActivity, profile
        inst = self.fresh()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            self.round(inst)
            torch.cuda.synchronize()
        events = list(prof.events())
        host_names = {e.name for e in events if not str(e.device_type).endswith("CUDA")}
        dev = [e for e in events if str(e.device_type).endswith("CUDA") and e.name not in host_names]
        dur = lambda e: getattr(e, "device_time_total", 0) or getattr(e, "cuda_time_total", 0) or (e.time_range.end - e.time_range.start)
        own = [dur(e) for e in dev if SCATTER in e.name]
        return sum(dur(e) for e in dev), len(dev), (sum(own) if own else None)

    def syncs(self):
        inst = self.fresh()
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                self.round(inst)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        return len([w for w in seen if "synchroniz" in str(w.message).lower()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import densify_ref as ref
    from bench_adam import copy_rate
    from build_id import csrc_sha16
    dev = torch.device("cuda:0")
    out = {"workload": "one densification round with Adam state present, inputs freshly cloned per round (untimed); wall-clock ms between two "
                       f"synchronisations, median of {a.rounds} rounds after {a.warmup}, spread = max - min; a = the reference's torch statements "
                       "(tests/densify_ref.py, fp32, on the GPU), b = hugs_amd.densify"}
    rate = copy_rate(dev)
    out["copy_rate_measured_GBps"] = round(rate, 1)
    for tag, flavour, n in (("scene", ref.SCENE, 200_000), ("human", ref.HUMAN, 110_210)):
        fx, mix = workload(flavour, n, seed=3)
        out[f"{tag}_rows"], out[f"{tag}_mix"] = n, mix
        variants = [Variant("a_torch", fx, dev), Variant("b_hip", fx, dev)]
        reps = {v.name: [] for v in variants}
        for k in range(a.warmup + a.rounds):                       # alternating: both variants see the same moments of the machine
            for v in variants:
                ms, rows, peak = v.timed()
                if k >= a.warmup:
                    reps[v.name].append(ms)
                out[f"{tag}_{v.name}_rows_after"], out[f"{tag}_{v.name}_peak_MB"] = rows, round(peak / 2 ** 20, 1)
        for v in variants:
            r = reps[v.name]
            out[f"{tag}_{v.name}_ms"], out[f"{tag}_{v.name}_spread_ms"] = round(statistics.median(r), 4), round(max(r) - min(r), 4)
            out[f"{tag}_{v.name}_rounds_ms"] = [round(x, 4) for x in r]
            device_us, launches, scatter_us = v.traced()
            out[f"{tag}_{v.name}_device_us"], out[f"{tag}_{v.name}_device_launches"] = round(device_us, 1), launches
            out[f"{tag}_{v.name}_host_syncs"] = v.syncs()
            if scatter_us is not None:
                rows_after = out[f"{tag}_{v.name}_rows_after"]
                # per densified tensor: the parameter and two moments read once, written once; the statistics are written only
                widths = (3 + 3 + 45 + 1 + 3 + 4) * 3 if flavour == ref.SCENE else 3 * 3 + 1 + 1 + 3 + 9
                moved = 4 * (widths * (n + rows_after) + 3 * rows_after)
                out[f"{tag}_scatter_bytes"], out[f"{tag}_scatter_us"] = moved, round(scatter_us, 1)
                out[f"{tag}_scatter_ideal_us_at_the_copy_rate"] = round(moved / rate * 1e-3, 1)
                out[f"{tag}_scatter_frac_of_copy_rate"] = round(moved / scatter_us * 1e-3 / rate, 3)
        assert out[f"{tag}_a_torch_rows_after"] == out[f"{tag}_b_hip_rows_after"], "the two variants disagree on the row count"
        out[f"{tag}_a_over_b"] = round(out[f"{tag}_a_torch_ms"] / out[f"{tag}_b_hip_ms"], 2)
        spread = max(out[f"{tag}_a_torch_spread_ms"], out[f"{tag}_b_hip_spread_ms"])
        out[f"{tag}_b_is_faster_than_a_by_more_than_the_spread"] = bool(out[f"{tag}_a_torch_ms"] - out[f"{tag}_b_hip_ms"] > spread)
        del variants
        torch.cuda.empty_cache()
    out["launch_counts_from"] = "torch.profiler, one round, device-side events (kernels and memory operations)"
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
    # the row's own promise, checked after the line is out so that a failure here keeps the figures
    assert out["scene_b_hip_host_syncs"] == 1 == out["human_b_hip_host_syncs"], "a round must synchronise with the host exactly once"


if __name__ == "__main__":
    main()
