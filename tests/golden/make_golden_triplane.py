#!/usr/bin/env python3
"""Generates tests/golden/reference_triplane.npz: planes, points, the features TriPlane.forward returns for them, a random
dL/dfeat and autograd's gradients for the planes and the points -- the class `TriPlane` (and its EPS) is compiled from
/root/reference/hugs/models/modules/triplane.py (read-only; the module itself imports loguru, which is not needed to run the
class) in THIS container and run on CPU.  Only these vectors travel.      python tests/golden/make_golden_triplane.py

F = 32 and UNEQUAL resolutions (resX, resY, resZ) = (6, 10, 14): an implementation that transposes a plane's axes fails on them.
The points: uniform in the box; exactly on its faces; outside it by less than EPS (in the unit cube's measure, so the reference's
assertion still holds); on texel centres (both in-plane coordinates integral) and on cell edges (one integral).  A texel
coordinate k / (W - 1) with W - 1 = 5, 9, 13 is no binary fraction, so such a point is the float32 NEAREST to the centre / edge,
moved by single ulps until the float32 and the float64 evaluation of `ix` fall into the same cell: dL/dx jumps from one cell to
the next, and a point whose cell depends on the evaluation's precision has no reference value for it."""
import ast
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

REF = "/root/reference/hugs/models/modules/triplane.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_triplane.npz")
RES = (6, 10, 14)


def reference_class():
    tree = ast.parse(open(REF).read())
    keep = [n for n in tree.body if (isinstance(n, ast.ClassDef) and n.name == "TriPlane") or
            (isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "EPS" for t in n.targets))]
    ns = {"torch": torch, "np": np, "nn": nn, "F": F}
    exec(compile(ast.Module(body=keep, type_ignores=[]), REF, "exec"), ns)
    return ns["TriPlane"], ns["EPS"]


def cell_index(x32, size, dtype):
    """floor(ix) of one coordinate as the reference's statements evaluate it (center 0, scale 2) in `dtype`"""
    t = dtype
    u = (x32.astype(t) - t(0.0)) / t(2.0) + t(0.5)
    g = u * t(2.0) - t(1.0)
    return np.floor(((g + t(1.0)) / t(2.0)) * t(size - 1))


def on_texel(k, size):
    """the float32 nearest to texel k's coordinate whose cell is the same in float32 and float64"""
    x = np.float32(2.0 * k / (size - 1) - 1.0)
    for _ in range(8):
        if cell_index(x, size, np.float32) == cell_index(x, size, np.float64):
            return x
        x = np.nextafter(x, np.float32(2.0))
    raise AssertionError((k, size))


def main():
    TriPlane, EPS = reference_class()
    r = np.random.default_rng(8)
    torch.manual_seed(8)
    m = TriPlane(32, *RES)
    pts = [r.uniform(-1.0, 1.0, (180, 3))]
    faces = r.uniform(-1.0, 1.0, (36, 3))
    for i in range(36):
        faces[i, i % 3] = 1.0 if (i // 3) % 2 else -1.0
        if i >= 24:
            faces[i, (i + 1) % 3] = -1.0 if i % 2 else 1.0       # edges and corners of the box
        if i >= 32:
            faces[i] = r.choice([-1.0, 1.0], 3)
    pts.append(faces)
    outside = r.uniform(-1.0, 1.0, (24, 3))
    for i in range(24):
        outside[i, i % 3] = (1.0 + 1.5 * EPS * r.uniform(0.1, 1.0)) * (1.0 if (i // 3) % 2 else -1.0)   # |u - 0.5| < 0.5 + EPS
    pts.append(outside)
    # size of the plane axis each coordinate runs along on its two planes: x -> resY (xy), resZ (xz); y -> resX (xy), resZ (yz); z -> resX (xz), resY (yz)
    sizes = ((RES[1], RES[2]), (RES[0], RES[2]), (RES[0], RES[1]))
    centres = r.uniform(-1.0, 1.0, (60, 3))
    for i in range(60):
        axes = (0, 1, 2) if i < 20 else ((i % 3,) if i < 40 else (i % 3, (i + 1) % 3))
        for a in axes:
            size = sizes[a][i % 2]
            centres[i, a] = on_texel(int(r.integers(0, size)), size)
    pts.append(centres)
    x = np.concatenate(pts).astype(np.float32)
    for a in range(3):
        for size in sizes[a]:
            same = cell_index(x[:, a], size, np.float32) == cell_index(x[:, a], size, np.float64)
            assert same.all(), (a, size, x[~same, a])
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    feat = m(xt)
    g = r.standard_normal(tuple(feat.shape)).astype(np.float32)
    feat.backward(torch.from_numpy(g))
    arrays = {"x": x, "feat": feat.detach().numpy(), "g_feat": g, "grad_x": xt.grad.numpy(), "center": np.float32(m.center),
              "scale": np.float32(m.scale), "n_output_dims": np.int32(m.n_output_dims), "eps": np.float32(EPS)}
    for name, p in m.named_parameters():
        arrays[name] = p.detach().numpy()
        arrays[f"grad_{name}"] = p.grad.numpy()
    arrays["parameter_names"] = np.frombuffer(",".join(n for n, _ in m.named_parameters()).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {len(arrays)} arrays, {x.shape[0]} points, {os.path.getsize(OUT) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
