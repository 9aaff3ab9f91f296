#!/usr/bin/env python3
"""Measurement for row f-5 with HumanSceneLoss's masks on one MI355X: forward + backward of 0.8 * Ll1 + 0.2 * loss_ssim in the `human`
and `scene` modes (hugs/losses/loss.py:70-107) at 3 x 1080 x 1920 and 3 x 512 x 512, three forms alternating in one process:

    (a) the reference's statements entirely in torch (composites, conv2d SSIM, mask.sum() scalings);
    (b) the mask statements in torch in front of the fused `l1_loss` / `ssim` -- the best form without this row's masked kernels;
    (c) `masked_l1_ssim`: the composites inside the fused pass;
    and the unmasked fused `l1_ssim` on the same images, which shows what the mask costs.

HIP events around `--iters` iterations after `--warmup`, `--rounds` rounds, their median and spread (max - min); device launches per
call from a torch.profiler trace of one call; peak memory of one call above what is allocated before it; the largest difference of
(c) from (a) in the two terms and the gradient at the timed size.  Prints one JSON line (and writes it to --out).  (c) must be faster
than (b): (b) does all of (c)'s work plus the composites.

    python tools/bench_masked_loss.py [--out profiles/<tag>_masked_loss.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ml-hugs_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)


def forms(pred, gt, mask, bg, mode):
    """-> {name: callable() -> (Ll1, loss_ssim)} on the same tensors"""
    from hugs_amd import losses
    from test_losses import _torch_statements
    H, W = pred.shape[-2:]

    def composites():                                    # loss.py:66-80, word for word
        m = mask.unsqueeze(0)
        if mode == "human":
            return pred, gt * m + bg[:, None, None] * (1. - m), m, m
        m = 1. - mask.unsqueeze(0)
        return pred * m, gt * m, m, 1 - m                # (the mask the l1 divides by: inverted again, :91)

    def a_torch():
        x, y, m, m_l1 = composites()
        s, _ = _torch_statements(x, y)
        l1 = torch.abs(x - y).sum() / m_l1.sum()         # utils.py:57
        area = m if mode == "human" else 1 - m           # loss.py:101,103
        return l1, (1.0 - s) * (area.sum() / (H * W))

    def b_torch_masks_fused_loss():
        x, y, m, m_l1 = composites()
        l1 = losses.l1_loss(x, y, mask=m_l1)
        area = m if mode == "human" else 1 - m
        return l1, (1.0 - losses.ssim(x, y)) * (area.sum() / (H * W))

    def c_masked_l1_ssim():
        return losses.masked_l1_ssim(pred, gt, mask, mode, bg)

    def unmasked_l1_ssim():
        l1, s = losses.l1_ssim(pred, gt)
        return l1, 1.0 - s

    return {"a_torch": a_torch, "b_torch_masks_fused_loss": b_torch_masks_fused_loss, "c_masked_l1_ssim": c_masked_l1_ssim,
            "unmasked_l1_ssim": unmasked_l1_ssim}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="1080x1920,512x512")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-profiler", action="store_true", help="no torch.profiler launch count (for a run under rocprofv3, which owns the tracer)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is nothing to fall back to"
    dev = torch.device("cuda:0")
    from build_id import csrc_sha16
    out = {"workload": "forward + backward of 0.8 * Ll1 + 0.2 * loss_ssim of HumanSceneLoss's human / scene mode, fp32, C = 3; ms per call from "
                       f"HIP events around {a.iters} calls after {a.warmup}, median of {a.rounds} alternating rounds, spread = max - min",
           "launch_counts_from": "torch.profiler, one call, device-side events (kernels and memory operations)", "results": {}}
    ok = True
    for shape in a.shapes.split(","):
        H, W = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cpu").manual_seed(0)
        gt = torch.nn.functional.avg_pool2d(torch.rand(1, 3, H, W, generator=g), 9, 1, 4)[0].contiguous().to(dev)     # image-like: smooth
        pred = (gt + 0.03 * torch.randn(gt.shape, generator=g).to(dev)).clamp(0, 1).requires_grad_(True)
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        mask = ((((yy - H / 2) / (0.4 * H)) ** 2 + ((xx - W / 2) / (0.15 * W)) ** 2) < 1).float().to(dev)            # a standing figure: ~19 % of the frame
        bg = torch.tensor([1.0, 1.0, 1.0], device=dev)
        for mode in ("human", "scene"):
            fs = forms(pred, gt, mask, bg, mode)

            def call(f):
                pred.grad = None
                l1, ls = f()
                (0.8 * l1 + 0.2 * ls).backward()
                return l1, ls

            def timed(f):
                for _ in range(a.warmup):
                    call(f)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.iters):
                    call(f)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / a.iters

            def launches(f):
                from torch.profiler import ProfilerActivity, profile
                call(f)
                torch.cuda.synchronize()
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    call(f)
                    torch.cuda.synchronize()
                events = list(prof.events())
                host_names = {e.name for e in events if not str(e.device_type).endswith("CUDA")}
                return len([e for e in events if str(e.device_type).endswith("CUDA") and e.name not in host_names])

            def peak(f):
                call(f)
                pred.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                r = call(f)
                torch.cuda.synchronize()
                del r
                return (torch.cuda.max_memory_allocated() - before) / 1e6

            res = {"mask_fraction": round(mask.mean().item(), 4)}
            reps = {name: [] for name in fs}
            for _ in range(a.rounds):                    # alternating: every form sees the same moments of the machine
                for name, f in fs.items():
                    reps[name].append(timed(f))
            for name, f in fs.items():
                r = reps[name]
                res[name] = {"ms": round(statistics.median(r), 4), "spread_ms": round(max(r) - min(r), 4), "rounds_ms": [round(x, 4) for x in r],
                             "device_launches": None if a.no_profiler else launches(f), "peak_MB": round(peak(f), 1)}
            # faster and different is not faster: (c) against the reference's statements on these inputs
            la, sa = call(fs["a_torch"])
            ga = pred.grad.clone()
            lc, sc = call(fs["c_masked_l1_ssim"])
            res["c_against_a"] = {"l1_rel": abs(lc.item() - la.item()) / abs(la.item()), "ssim_term_abs": abs(sc.item() - sa.item()),
                                  "grad_max_over_largest": ((pred.grad - ga).abs().max() / ga.abs().max()).item()}
            b, c, u = res["b_torch_masks_fused_loss"], res["c_masked_l1_ssim"], res["unmasked_l1_ssim"]
            res["a_over_c"] = round(res["a_torch"]["ms"] / c["ms"], 2)
            res["b_over_c"] = round(b["ms"] / c["ms"], 2)
            res["c_over_unmasked"] = round(c["ms"] / u["ms"], 3)
            res["c_is_faster_than_b_by_more_than_the_spread"] = bool(b["ms"] - c["ms"] > max(b["spread_ms"], c["spread_ms"]))
            ok = ok and res["c_is_faster_than_b_by_more_than_the_spread"]
            out["results"][f"3x{H}x{W}_{mode}"] = res
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
    assert ok, "(c) is not faster than (b): a defect to find, not a result to report"   # (after the line is out: the figures are kept)


if __name__ == "__main__":
    main()
