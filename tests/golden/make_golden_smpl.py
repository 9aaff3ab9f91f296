"""Golden vectors for row f-10: the reference's own lbs() (/root/reference/hugs/models/modules/lbs.py:76-187), compiled from its
source file and executed on CPU in float32, forward and autograd backward.

    python tests/golden/make_golden_smpl.py        ->  tests/golden/reference_smpl.npz

smplx (a pip dependency) is absent: the four functions lbs.py imports from smplx.lbs are supplied by tests/smpl_ref.py's torch
forms of the published formulas.  So the vectors pin the statements of lbs() itself -- the order of operations, the pose-feature
layout, which tensor feeds which -- and not those four functions or the translation lines of SMPL.forward.

Inputs are not stored: tests regenerate them from smpl_ref.synthetic_model(7, V=48, J=24, NB=10, 'smpl'), synthetic_inputs(7, ...)
and cotangents(7, ...).  Stored: the eight outputs and the gradients w.r.t. betas and pose, for both values of disable_posedirs.
Nothing is written to /root/reference, and this script never runs on a GPU machine."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import smpl_ref as sr  # noqa: E402

REF = "/root/reference/hugs/models/modules/lbs.py"
OUT = os.path.join(HERE, "reference_smpl.npz")
SEED, V, J, NB = 7, 48, 24, 10


def _reference_lbs():
    stub = types.ModuleType("smplx.lbs")
    for name in ("batch_rodrigues", "blend_shapes", "vertices2joints", "batch_rigid_transform"):
        setattr(stub, name, getattr(sr, name))
    pkg = types.ModuleType("smplx")
    pkg.lbs = stub
    sys.modules["smplx"], sys.modules["smplx.lbs"] = pkg, stub
    mod = types.ModuleType("reference_lbs")
    exec(compile(open(REF).read(), REF, "exec"), mod.__dict__)
    return mod.lbs


def main():
    lbs = _reference_lbs()
    model = sr.synthetic_model(SEED, V, J, NB, "smpl")
    tm = sr.torch_model(model)
    betas, pose, _ = sr.synthetic_inputs(SEED, J, NB)
    cot = sr.cotangents(SEED, V, J)
    out = {}
    for disable in (False, True):
        b, p = torch.from_numpy(betas).requires_grad_(), torch.from_numpy(pose).requires_grad_()
        res = lbs(b, p, tm["v_template"], tm["shapedirs"], tm["posedirs"], tm["J_regressor"], tm["parents"], tm["lbs_weights"],
                  pose2rot=True, disable_posedirs=disable)
        loss = sum((r * torch.from_numpy(cot[k])).sum() for k, r in zip(sr.OUTPUTS, res))
        loss.backward()
        tag = "nopd" if disable else "pd"
        for k, r in zip(sr.OUTPUTS, res):
            out[f"{tag}_{k}"] = r.detach().numpy().astype(np.float32)
        out[f"{tag}_grad_betas"], out[f"{tag}_grad_pose"] = b.grad.numpy(), p.grad.numpy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
