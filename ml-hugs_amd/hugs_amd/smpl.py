"""The SMPL body model's forward from the pose parameters to vertices and joint transforms, fused.

Drop-ins, with the reference's names, argument order and return values, for

    lbs(betas, pose, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, pose2rot=True,
        disable_posedirs=False, vert_offsets=None)              /root/reference/hugs/models/modules/lbs.py:76-187
        -> (verts, J_transformed, A, T, v_posed, v_shaped, shape_offsets, pose_offsets)

and `smpl_forward(model, betas, body_pose, global_orient, transl, disable_posedirs)`, the statements of SMPL.forward
(/root/reference/hugs/models/modules/smpl_layer.py:411-519, called every human step at hugs/models/hugs_trimlp.py:458) around that
call: the cat of the two pose halves (:471) and the translation of vertices, joints, A and T (:498-504), which runs inside the kernels.

Shape blend, joint regression, Rodrigues, the pose-corrective product, the kinematic chain, the skinning and all of their backward
run in hand-written HIP (csrc/smpl.hip; three launches forward, three to seven backward) behind the C ABI.  Gradients reach betas,
pose and transl; the model buffers are constants, as the reference's register_buffers are.  No CPU fallback.
"""
import ctypes as C
from types import SimpleNamespace

import torch

from diff_gaussian_rasterization import _aligned, _launch, _load, _require_gpu
from diff_gaussian_rasterization import _row_f32c as _f32c, _row_ptr as _ptr


def _host_parents(parents):
    """The kinematic tree as a host int32 array.  A tensor is read from the device once: the array travels with the tensor object,
    tagged with its data pointer and version counter, so later calls do not synchronise and an in-place change is seen."""
    if not isinstance(parents, torch.Tensor):
        vals = [int(v) for v in parents]
        return (C.c_int32 * len(vals))(*vals)
    tag = (parents.data_ptr(), parents._version)
    hit = getattr(parents, "_hgs_host_parents", None)
    if hit is None or hit[0] != tag:
        vals = [int(v) for v in parents.detach().reshape(-1).tolist()]
        hit = (tag, (C.c_int32 * len(vals))(*vals))
        parents._hgs_host_parents = hit
    return hit[1]


class _Smpl(torch.autograd.Function):
    """The whole batch in one node; the kernels take one element per call."""

    @staticmethod
    def forward(ctx, betas, pose, transl, v_template, shapedirs, posedirs, J_regressor, lbs_weights, parents, disable_posedirs):
        lib = _load()
        B, NB = betas.shape
        V, J = v_template.shape[0], J_regressor.shape[0]
        dev = betas.device
        betas, pose = _f32c(betas), _f32c(pose)
        transl = None if transl is None else _f32c(transl)
        new = lambda *s: torch.empty(B, *s, dtype=torch.float32, device=dev)
        verts, Jtr, A, T = new(V, 3), new(J, 3), new(J, 4, 4), new(V, 4, 4)
        v_posed, v_shaped, shape_offsets, pose_offsets = new(V, 3), new(V, 3), new(V, 3), new(V, 3)
        ws = torch.empty(B, max(lib.hgs_smpl_workspace(V, J, NB), 16), dtype=torch.uint8, device=dev)
        pd = None if disable_posedirs else posedirs
        with torch.cuda.device(dev):
            for b in range(B):
                _launch(dev, "smpl lbs", lib.hgs_smpl_forward, V, J, NB, parents, betas[b].data_ptr(), pose[b].data_ptr(),
                        None if transl is None else transl[b].data_ptr(), v_template.data_ptr(), shapedirs.data_ptr(),
                        _ptr(pd), J_regressor.data_ptr(), lbs_weights.data_ptr(), int(disable_posedirs),
                        verts[b].data_ptr(), Jtr[b].data_ptr(), A[b].data_ptr(), T[b].data_ptr(), v_posed[b].data_ptr(),
                        v_shaped[b].data_ptr(), shape_offsets[b].data_ptr(), pose_offsets[b].data_ptr(), ws[b].data_ptr())
        ctx.save_for_backward(pose, shapedirs, J_regressor, lbs_weights, v_posed, T, ws, *(() if pd is None else (pd,)))
        ctx.parents, ctx.disable, ctx.has_transl, ctx.sizes = parents, bool(disable_posedirs), transl is not None, (B, V, J, NB)
        ctx.set_materialize_grads(False)
        return verts, Jtr, A, T, v_posed, v_shaped, shape_offsets, pose_offsets

    @staticmethod
    def backward(ctx, *grads):
        lib = _load()
        pose, shapedirs, J_regressor, lbs_weights, v_posed, T, ws = ctx.saved_tensors[:7]
        pd = None if ctx.disable else ctx.saved_tensors[7]
        B, V, J, NB = ctx.sizes
        dev = pose.device
        grads = [None if g is None else _f32c(g) for g in grads]
        d_betas = torch.empty(B, NB, dtype=torch.float32, device=dev)
        d_pose = torch.empty(B, 3 * J, dtype=torch.float32, device=dev)
        d_transl = torch.empty(B, 3, dtype=torch.float32, device=dev) if ctx.has_transl else None
        g_verts, g_Jtr, g_A, g_T, g_vp, g_vs, g_so, g_po = grads
        g_T = _aligned(g_T)   # read as float4s, an element a whole number of them (the other seven gradients: scalar loads)
        with torch.cuda.device(dev):
            for b in range(B):
                at = lambda g: None if g is None else g[b].data_ptr()
                _launch(dev, "smpl lbs backward", lib.hgs_smpl_backward, V, J, NB, ctx.parents, pose[b].data_ptr(), shapedirs.data_ptr(),
                        _ptr(pd), J_regressor.data_ptr(), lbs_weights.data_ptr(), int(ctx.disable), v_posed[b].data_ptr(), T[b].data_ptr(),
                        at(g_verts), at(g_Jtr), at(g_A), at(g_T), at(g_vp), at(g_vs), at(g_so), at(g_po), d_betas[b].data_ptr(),
                        d_pose[b].data_ptr(), None if d_transl is None else d_transl[b].data_ptr(), ws[b].data_ptr())
        return d_betas, d_pose, d_transl, None, None, None, None, None, None, None


def _fused(betas, pose, transl, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, disable_posedirs):
    buffers = [("v_template", v_template), ("shapedirs", shapedirs), ("J_regressor", J_regressor), ("lbs_weights", lbs_weights)]
    if not disable_posedirs:
        buffers.append(("posedirs", posedirs))
    for name, t in buffers:
        if t.requires_grad:
            raise NotImplementedError(f"smpl lbs: `{name}` requires grad; the model buffers are constants here (the reference registers them as buffers)")
    for name, t in [("betas", betas), ("pose", pose)] + buffers:
        _require_gpu(t, name)
    if v_template.dim() == 3 and v_template.shape[0] == 1:
        v_template = v_template[0]
    V, J = v_template.shape[0], J_regressor.shape[0]
    B = max(betas.shape[0], pose.shape[0])
    if betas.shape[0] != B:
        betas = betas.expand(B, -1)
    if pose.shape[0] != B:
        pose = pose.expand(B, -1)
    pose = pose.reshape(B, -1)
    NB = betas.shape[1]
    if (v_template.shape != (V, 3) or shapedirs.shape != (V, 3, NB) or J_regressor.shape != (J, V) or lbs_weights.shape != (V, J)
            or pose.shape[1] != 3 * J or (not disable_posedirs and posedirs.shape != (9 * (J - 1), 3 * V))
            or (transl is not None and transl.shape != (B, 3))):
        raise ValueError("smpl lbs: expected betas [B,NB], pose [B,3J], v_template [V,3], shapedirs [V,3,NB], posedirs [9(J-1),3V], "
                         "J_regressor [J,V], lbs_weights [V,J], transl [B,3]")
    hp = _host_parents(parents)
    if len(hp) != J:
        raise ValueError("smpl lbs: parents must have one entry per joint")
    with torch.no_grad():
        v_template, shapedirs, J_regressor, lbs_weights = _f32c(v_template), _f32c(shapedirs), _f32c(J_regressor), _f32c(lbs_weights)
        posedirs = None if disable_posedirs else _f32c(posedirs)
    return _Smpl.apply(betas, pose, transl, v_template, shapedirs, posedirs, J_regressor, lbs_weights, hp, bool(disable_posedirs))


def lbs(betas, pose, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, pose2rot=True, disable_posedirs=False,
        vert_offsets=None):
    """lbs.py:76-187, same arguments and return tuple (verts, J_transformed, A, T, v_posed, v_shaped, shape_offsets, pose_offsets),
    each with the leading batch dimension.  pose2rot=False, vert_offsets and buffers that require grad are not implemented: no call
    site of the reference uses them."""
    if not pose2rot:
        raise NotImplementedError("smpl lbs: pose2rot=False (rotation matrices as input) is not implemented")
    if vert_offsets is not None:
        raise NotImplementedError("smpl lbs: vert_offsets is not implemented")
    return _fused(betas, pose, None, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, disable_posedirs)


def smpl_forward(model, betas=None, body_pose=None, global_orient=None, transl=None, disable_posedirs=False):
    """SMPL.forward (smpl_layer.py:411-519) on `model`, any object with the reference's buffers v_template, shapedirs, posedirs,
    J_regressor, parents, lbs_weights (and, for arguments left None, its betas / body_pose / global_orient / transl).  Returns a
    namespace with SMPLOutput's field names.  One difference: `joints` holds the J model joints (J_transformed + transl); the
    reference appends joints picked from vertices by a third-party selector that the training path never reads."""
    global_orient = global_orient if global_orient is not None else model.global_orient
    body_pose = body_pose if body_pose is not None else model.body_pose
    betas = betas if betas is not None else model.betas
    if transl is None and hasattr(model, "transl"):
        transl = model.transl
    full_pose = torch.cat([global_orient, body_pose], dim=1)
    B = max(betas.shape[0], global_orient.shape[0], body_pose.shape[0])
    if betas.shape[0] != B:
        betas = betas.expand(B, -1)
    if transl is not None and transl.shape[0] != B:
        transl = transl.expand(B, -1)
    if transl is not None:
        _require_gpu(transl, "transl")
    vertices, joints, A, T, v_posed, v_shaped, shape_offsets, pose_offsets = _fused(
        betas, full_pose, transl, model.v_template, model.shapedirs, getattr(model, "posedirs", None), model.J_regressor, model.parents,
        model.lbs_weights, disable_posedirs)
    return SimpleNamespace(vertices=vertices, global_orient=global_orient, body_pose=body_pose, joints=joints, betas=betas,
                           full_pose=full_pose, A=A, T=T, shape_offsets=shape_offsets, pose_offsets=pose_offsets, v_posed=v_posed,
                           v_shaped=v_shaped)
