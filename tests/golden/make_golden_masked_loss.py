#!/usr/bin/env python3
"""Generates tests/golden/reference_masked_loss.npz: inputs, every loss_dict value and the autograd gradients of the reference's own
HumanSceneLoss.forward (/root/reference/hugs/losses/loss.py:16-162) over its own l1_loss and ssim (hugs/losses/utils.py:54-108).
The class and the five functions are compiled from the reference's source files in THIS container (read-only; the modules
themselves import lpips, cv2 and pytorch3d, which are absent, so the definitions are taken one by one) and run on CPU in fp32.
LPIPS and PatchSampler are stubs (an nn.Module whose forward is ((a - b) ** 2).mean((1, 2, 3)); a sampler that cuts one fixed
corner): the golden runs have l_lpips_w = 0, where the reference still evaluates them for `lpips_patch_human` and multiplies by 0.
Only these vectors travel.

    python tests/golden/make_golden_masked_loss.py

Cases (C = 3; each in `human`, `scene` and `human_scene` + human-separation modes; the tile of the kernels is 64 x 16):
    c1  37 x 53    ragged, scalar load path               mask: a rectangle across the tile seams + one pixel of 0.5
    c2  40 x 132   float4 path, 3 x 3 tiles, last partial mask: the same kind
    c3   5 x 7     smaller than the window                mask: the same kind
    c4  37 x 53    (c1's images)                          mask: soft, every value strictly inside (0, 1)
    c5  40 x 132   (c2's images)                          mask: all ones
"""
import ast
import os
from math import exp

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Variable

REF = os.environ.get("HUGS_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_masked_loss.npz")
MODES = ("human", "scene", "human_scene")
WEIGHTS = dict(l_ssim_w=0.2, l_l1_w=0.8, l_lpips_w=0.0, l_lbs_w=1000.0, l_humansep_w=1.0)   # (every kind of term active; LPIPS weighs 0)


class LPIPS(nn.Module):
    def __init__(self, **kw):
        super().__init__()

    def to(self, *a, **kw):
        return self

    def forward(self, a, b):
        return ((a - b) ** 2).mean((1, 2, 3))


class PatchSampler:
    def __init__(self, num_patch=4, patch_size=32, **kw):
        self.p = patch_size

    def sample(self, mask, *images):
        p = self.p
        return [mask[None, :, :p, :p]] + [img[None, :, :p, :p] for img in images]


def reference_class():
    ns = {"torch": torch, "F": F, "nn": nn, "Variable": Variable, "exp": exp, "LPIPS": LPIPS, "PatchSampler": PatchSampler}
    path = os.path.join(REF, "hugs", "losses", "utils.py")
    tree = ast.parse(open(path).read())
    for name in ("l1_loss", "gaussian", "create_window", "ssim", "_ssim"):
        node = next(f for f in tree.body if isinstance(f, ast.FunctionDef) and f.name == name)
        exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    path = os.path.join(REF, "hugs", "losses", "loss.py")
    node = next(c for c in ast.parse(open(path).read()).body if isinstance(c, ast.ClassDef) and c.name == "HumanSceneLoss")
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns["HumanSceneLoss"]


def smooth(c, h, w, phase=0.0):
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    return np.stack([0.5 + 0.4 * np.sin(6.0 * xx + k + phase) * np.cos(4.0 * yy - k) for k in range(c)]).astype(np.float32)


def rect_mask(h, w, rows, cols, half):
    m = np.zeros((h, w), np.float32)
    m[rows[0]:rows[1], cols[0]:cols[1]] = 1.0
    m[half] = 0.5
    return m


def main():
    cls = reference_class()
    r = np.random.default_rng(11)
    images = {}
    for h, w in ((37, 53), (40, 132), (5, 7)):
        gt = np.round(smooth(3, h, w) * 255.0).astype(np.float32) / np.float32(255.0)          # (an 8-bit photograph)
        pred = np.clip(gt + 0.05 * r.standard_normal(gt.shape), 0, 1.2).astype(np.float32)     # (a render: may exceed 1)
        human = np.clip(smooth(3, h, w, 0.3) + 0.05 * r.standard_normal(gt.shape), 0, 1.2).astype(np.float32)
        images[(h, w)] = (pred, gt, human)
    cases = {"c1": ((37, 53), rect_mask(37, 53, (10, 30), (8, 45), (31, 50))),
             "c2": ((40, 132), rect_mask(40, 132, (10, 35), (40, 100), (3, 70))),
             "c3": ((5, 7), rect_mask(5, 7, (1, 4), (2, 6), (0, 0))),
             "c4": ((37, 53), (0.05 + 0.9 * r.random((37, 53))).astype(np.float32)),
             "c5": ((40, 132), np.ones((40, 132), np.float32))}
    bg = np.array([1.0, 0.25, 0.0], np.float32)
    lbs, lbs_gt = r.random((20, 24)).astype(np.float32), r.random((20, 24)).astype(np.float32)
    out = {"bg": bg, "lbs": lbs, "lbs_gt": lbs_gt}
    for (h, w), (pred, gt, human) in images.items():
        out.update({f"pred_{h}x{w}": pred, f"gt_{h}x{w}": gt, f"human_{h}x{w}": human})
    for name, ((h, w), mask) in cases.items():
        out[f"{name}_mask"] = mask
        out[f"{name}_shape"] = np.array([h, w])
        pred, gt, human = images[(h, w)]
        for mode in MODES:
            module = cls(**WEIGHTS)
            tp = torch.from_numpy(pred.copy()).requires_grad_(True)
            th = torch.from_numpy(human.copy()).requires_grad_(True)
            tl = torch.from_numpy(lbs.copy()).requires_grad_(True)
            torch.manual_seed(0)
            loss, loss_dict, extras = module({"rgb": torch.from_numpy(gt), "mask": torch.from_numpy(mask)},
                                             {"render": tp, "human_img": th}, {"lbs_weights": tl, "gt_lbs_weights": torch.from_numpy(lbs_gt)},
                                             mode, bg_color=torch.from_numpy(bg))
            loss.backward()
            key = f"{name}_{mode}"
            out[f"{key}_keys"] = np.array(sorted(loss_dict))
            out[f"{key}_loss"] = np.float32(loss.item())
            for k, v in loss_dict.items():
                out[f"{key}_{k}"] = np.float32(v.item())
            out[f"{key}_grad"] = tp.grad.numpy().copy()
            if mode == "human_scene":
                out[f"{key}_grad_human"] = th.grad.numpy().copy()
            if mode != "scene":
                out[f"{key}_grad_lbs"] = tl.grad.numpy().copy()
            assert torch.equal(extras["pred_img"], tp)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
