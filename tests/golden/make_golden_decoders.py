#!/usr/bin/env python3
"""Generates tests/golden/reference_decoders.npz and reference_decoders_grads.npz (autograd's gradients): for each of AppearanceDecoder, GeometryDecoder and DeformationDecoder
(disable_posedirs=True), 200 random feature rows, the module's state_dict after every parameter was moved by 0.05 randn (so that no
zero or default initialisation hides a layer), the outputs, random upstream gradients, autograd's dL/dx and every parameter
gradient (a state_dict key that aliases an earlier one stores that key's name, not the tensor
again), and the state_dict key list and the named_parameters list as byte strings.  The three classes, `act_fn_dict` and
`SineActivation` are compiled from /root/reference/hugs/models/modules/{decoders,activation}.py (read-only; the module imports
loguru, which the classes do not need) in THIS container and run on CPU.  Only these vectors travel.
    python tests/golden/make_golden_decoders.py
"""
import ast
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

REF_DIR = "/root/reference/hugs/models/modules"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_decoders.npz")
OUT_GRADS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_decoders_grads.npz")
N, FEATURES = 200, 96
CLASSES = ("AppearanceDecoder", "DeformationDecoder", "GeometryDecoder")


def reference_classes():
    ns = {"torch": torch, "np": np, "nn": nn, "F": F, "math": math}
    path = os.path.join(REF_DIR, "activation.py")
    keep = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.ClassDef) and n.name == "SineActivation"]
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    path = os.path.join(REF_DIR, "decoders.py")
    keep = [n for n in ast.parse(open(path).read()).body if (isinstance(n, ast.ClassDef) and n.name in CLASSES) or
            (isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "act_fn_dict" for t in n.targets))]
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return {name: ns[name] for name in CLASSES}


def main():
    classes = reference_classes()
    torch.manual_seed(9)
    x = torch.randn(N, FEATURES)
    arrays = {"x": x.numpy().copy()}
    made = {"appearance": classes["AppearanceDecoder"](FEATURES), "geometry": classes["GeometryDecoder"](FEATURES),
            "deformation": classes["DeformationDecoder"](FEATURES, disable_posedirs=True)}
    for tag, m in made.items():
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.05 * torch.randn_like(p))
        keys = list(m.state_dict().keys())
        names = [n for n, _ in m.named_parameters()]
        first = {}   # GeometryDecoder's heads hold `net` again: an alias key stores the NAME of the key that has the tensor
        for k, v in m.state_dict().items():
            if v.data_ptr() in first:
                arrays[f"{tag}.alias.{k}"] = np.frombuffer(first[v.data_ptr()].encode(), dtype=np.uint8)
            else:
                first[v.data_ptr()] = k
                arrays[f"{tag}.state.{k}"] = v.detach().numpy().copy()
        xt = x.clone().requires_grad_(True)
        out = m(xt)
        outs = {k: v for k, v in out.items() if v is not None}
        gs = {k: torch.randn_like(v) for k, v in outs.items()}
        torch.autograd.backward([outs[k] for k in outs], [gs[k] for k in outs])
        for k in outs:
            arrays[f"{tag}.out.{k}"] = outs[k].detach().numpy().copy()
            arrays[f"{tag}.g_out.{k}"] = gs[k].numpy().copy()
        arrays[f"{tag}.grad_x"] = xt.grad.numpy().copy()
        for n, p in m.named_parameters():
            arrays[f"{tag}.grad.{n}"] = p.grad.numpy().copy()
        arrays[f"{tag}.state_dict_keys"] = np.frombuffer(",".join(keys).encode(), dtype=np.uint8)
        arrays[f"{tag}.parameter_names"] = np.frombuffer(",".join(names).encode(), dtype=np.uint8)
        arrays[f"{tag}.output_keys"] = np.frombuffer(",".join(out.keys()).encode(), dtype=np.uint8)
    # two files: random float32 does not compress, and together the vectors pass the repository's 1 MiB limit for one file
    is_grad = lambda k: ".grad." in k or k.endswith(".grad_x")
    for path, part in ((OUT, {k: v for k, v in arrays.items() if not is_grad(k)}), (OUT_GRADS, {k: v for k, v in arrays.items() if is_grad(k)})):
        np.savez_compressed(path, **part)
        print(f"wrote {path}: {len(part)} arrays, {N} rows, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
