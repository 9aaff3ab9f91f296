"""Fused SceneGS.forward (row f-6): the statements that turn the scene model's raw parameters into the rasterizer's inputs on
every training step, /root/reference/hugs/models/scene.py:147-160 --

    def forward(self):                                   # in hugs/models/scene.py
        return hugs_amd.scene_forward.scene_forward(self._xyz, self._scaling, self._rotation, self._opacity,
                                                    self._features_dc, self._features_rest, self.active_sh_degree)

exp / normalize / sigmoid / cat in one HIP kernel, their backward in one more (the reference: 5 + ~17 torch kernels).  Same
dict, same keys, same values (fp32: expf and the division by the norm are correctly rounded here as there).  No CPU fallback.
"""
import torch

from diff_gaussian_rasterization import _aligned, _call, _load, _ptr, _require_gpu


class _SceneActivations(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling, rotation, opacity, features_dc, features_rest):
        lib = _load()
        P, M = scaling.shape[0], 1 + features_rest.shape[1]
        dev = scaling.device
        scales, rotq = torch.empty_like(scaling), torch.empty_like(rotation)
        opac = torch.empty_like(opacity)
        shs = torch.empty(P, M, 3, dtype=torch.float32, device=dev)
        _call(dev, "scene_forward", lib.hgs_scene_forward, P, M, scaling.data_ptr(), rotation.data_ptr(), opacity.data_ptr(),
              features_dc.data_ptr(), features_rest.data_ptr() if M > 1 else None, scales.data_ptr(), rotq.data_ptr(), opac.data_ptr(),
              shs.data_ptr())
        ctx.save_for_backward(rotation, scales, opac)
        ctx.M = M
        ctx.set_materialize_grads(False)
        return scales, rotq, opac, shs

    @staticmethod
    def backward(ctx, g_scales, g_rotq, g_opac, g_shs):
        rotation, scales, opac = ctx.saved_tensors
        lib = _load()
        P, M, dev = scales.shape[0], ctx.M, scales.device
        c = _aligned
        g_scales, g_rotq, g_opac, g_shs = c(g_scales), c(g_rotq), c(g_opac), c(g_shs)
        new = lambda g, shape: torch.empty(shape, dtype=torch.float32, device=dev) if g is not None else None
        d_scaling, d_rot, d_op = new(g_scales, (P, 3)), new(g_rotq, (P, 4)), new(g_opac, (P, 1))
        d_dc, d_rest = new(g_shs, (P, 1, 3)), new(g_shs, (P, M - 1, 3))
        # (_ptr is the rasterizer's form: an empty tensor -- d_rest at M == 1 -- goes as NULL)
        _call(dev, "scene_backward", lib.hgs_scene_backward, P, M, rotation.data_ptr(), scales.data_ptr(), opac.data_ptr(), _ptr(g_scales),
              _ptr(g_rotq), _ptr(g_opac), _ptr(g_shs), _ptr(d_scaling), _ptr(d_rot), _ptr(d_op), _ptr(d_dc), _ptr(d_rest))
        return d_scaling, d_rot, d_op, d_dc, d_rest


def scene_activations(scaling, rotation, opacity, features_dc, features_rest):
    """-> (exp(scaling), normalize(rotation), sigmoid(opacity), cat(features_dc, features_rest, dim=1)), one kernel."""
    named = (("_scaling", scaling, 3), ("_rotation", rotation, 4), ("_opacity", opacity, 1))
    P = scaling.shape[0]
    for name, t, w in named:
        _require_gpu(t, name)
        if t.dtype != torch.float32 or t.shape != (P, w):
            raise RuntimeError(f"{name} must be a float32 tensor of shape [{P}, {w}]")
    for name, t in (("_features_dc", features_dc), ("_features_rest", features_rest)):
        _require_gpu(t, name)
        if t.dtype != torch.float32 or t.ndim != 3 or t.shape[0] != P or t.shape[2] != 3:
            raise RuntimeError(f"{name} must be a float32 tensor of shape [{P}, k, 3]")
    if features_dc.shape[1] != 1:
        raise RuntimeError("_features_dc must have one coefficient per Gaussian")
    return _SceneActivations.apply(_aligned(scaling), _aligned(rotation), _aligned(opacity), _aligned(features_dc), _aligned(features_rest))


def scene_forward(xyz, scaling, rotation, opacity, features_dc, features_rest, active_sh_degree):
    """The dict SceneGS.forward returns (scene.py:153-160)."""
    scales, rotq, opac, shs = scene_activations(scaling, rotation, opacity, features_dc, features_rest)
    return {"xyz": xyz, "scales": scales, "rotq": rotq, "shs": shs, "opacity": opac, "active_sh_degree": active_sh_degree}
