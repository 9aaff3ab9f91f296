"""Fused human decoders (row f-9): the three networks that consume the triplane features,
/root/reference/hugs/models/hugs_trimlp.py:409-410,430 `appearance_dec(tri_feats)`, `geometry_dec(tri_feats)`, `deformation_dec(tri_feats)`
(/root/reference/hugs/models/modules/decoders.py:24-111), each as one HIP kernel forward and one backward (csrc/mlp.hip).

    from hugs_amd.decoders import AppearanceDecoder, DeformationDecoder, GeometryDecoder   # instead of `from .modules.decoders import ...`

Same constructors, submodule tree, state_dict keys (the aliases of GeometryDecoder's shared `net` included), parameter order, shapes
and initialisation as the reference's modules: its checkpoints load and save back unchanged.  Only the heads are written; no hidden
activation reaches memory or is kept for the backward, which recomputes them per tile of points.  fp32 throughout.
The parameter gradients are summed with float atomics (one flush per workgroup): their last bits depend on arrival order.  The
forward and dL/dx are bit-reproducible.  No host synchronisation.  No CPU fallback.

Implemented: act='gelu' (what hugs_trimlp.py:103-106 constructs) and disable_posedirs=True (every release config); any other form
constructs and raises NotImplementedError in forward.
"""
import ctypes as C

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from diff_gaussian_rasterization import _aligned, _call, _load, _require_gpu
from diff_gaussian_rasterization import _row_ptr as _ptr
from diff_gaussian_rasterization._abi import MLP_MAX_HEADS as MAX_HEADS, MLP_MAX_TRUNK as MAX_TRUNK, _Desc, _Grads

ACT_NONE, ACT_GELU, ACT_SIGMOID = 0, 1, 2
_ACT_CODES = {None: ACT_NONE, "none": ACT_NONE, "gelu": ACT_GELU, "sigmoid": ACT_SIGMOID}


def tile_points():
    """points per tile of the two kernels (tests choose their sizes around it)"""
    return int(_load().hgs_mlp_tile())


def _describe(x, params, n_trunk, acts):
    """params = (W_0, b_0, ..., W_{L-1}, b_{L-1}, Wh_0, bh_0, ...)"""
    d = _Desc()
    d.in_width, d.n_trunk, d.n_heads = x.shape[1], n_trunk, len(acts)
    for l in range(n_trunk):
        d.trunk_width[l] = params[2 * l].shape[0]
        d.trunk_weight[l], d.trunk_bias[l] = params[2 * l].data_ptr(), params[2 * l + 1].data_ptr()
    for k, a in enumerate(acts):
        w, b = params[2 * (n_trunk + k)], params[2 * (n_trunk + k) + 1]
        d.head_width[k], d.head_act[k] = w.shape[0], a
        d.head_weight[k], d.head_bias[k] = w.data_ptr(), b.data_ptr()
    return d


class _DecoderMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n_trunk, acts, *params):
        lib = _load()
        n, dev = x.shape[0], x.device
        outs = tuple(torch.empty(n, params[2 * (n_trunk + k)].shape[0], dtype=torch.float32, device=dev) for k in range(len(acts)))
        desc = _describe(x, params, n_trunk, acts)
        _call(dev, "decoder_mlp", lib.hgs_mlp_forward, n, C.byref(desc), x.data_ptr(), (C.c_void_p * MAX_HEADS)(*[o.data_ptr() for o in outs]))
        ctx.set_materialize_grads(False)    # a head the loss does not use arrives as None and is skipped
        ctx.save_for_backward(x, *params)   # the inputs only: the hidden activations are recomputed
        ctx.n_trunk, ctx.acts = n_trunk, acts
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *g_outs):
        x, *params = ctx.saved_tensors
        lib = _load()
        n_trunk, acts = ctx.n_trunk, ctx.acts
        n, dev = x.shape[0], x.device
        g_outs = [None if g is None else _aligned(g) for g in g_outs]
        d_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        # (the parameters of a head the loss does not use get None, as autograd gives a Linear outside the graph)
        used = lambda j: j < 2 * n_trunk or g_outs[(j - 2 * n_trunk) // 2] is not None
        d_params = [torch.zeros_like(p) if ctx.needs_input_grad[3 + j] and used(j) else None for j, p in enumerate(params)]
        grads = _Grads()
        for l in range(n_trunk):
            grads.trunk_weight[l], grads.trunk_bias[l] = _ptr(d_params[2 * l]), _ptr(d_params[2 * l + 1])
        for k in range(len(acts)):
            grads.head_weight[k], grads.head_bias[k] = _ptr(d_params[2 * (n_trunk + k)]), _ptr(d_params[2 * (n_trunk + k) + 1])
        desc = _describe(x, params, n_trunk, acts)
        _call(dev, "decoder_mlp backward", lib.hgs_mlp_backward, n, C.byref(desc), x.data_ptr(), (C.c_void_p * MAX_HEADS)(*[_ptr(g) for g in g_outs]),
              _ptr(d_x), C.byref(grads))
        return (d_x, None, None, *d_params)


def decoder_mlp(x, trunk, heads):
    """x [..., in]; trunk: [(weight [out, in], bias [out]), ...] -- 1 to 3 Linear layers, each followed by exact GELU; heads:
    [(weight, bias, act), ...] off the last trunk activation, act in {None, 'gelu', 'sigmoid'}.  Returns one [..., out] tensor per head."""
    if not 1 <= len(trunk) <= MAX_TRUNK or not 1 <= len(heads) <= MAX_HEADS:
        raise RuntimeError(f"decoder_mlp: 1 to {MAX_TRUNK} trunk layers and 1 to {MAX_HEADS} heads")
    acts = []
    for _, _, a in heads:
        if a not in _ACT_CODES:
            raise RuntimeError(f"decoder_mlp: unknown head activation {a!r} (None, 'gelu' or 'sigmoid')")
        acts.append(_ACT_CODES[a])
    params = [t for w, b in trunk for t in (w, b)] + [t for w, b, _ in heads for t in (w, b)]
    for name, t in [("x", x)] + [(f"parameter {j}", p) for j, p in enumerate(params)]:
        _require_gpu(t, name)
        if t.dtype != torch.float32:
            raise RuntimeError(f"decoder_mlp: {name} must be float32")
    if x.ndim < 1:
        raise RuntimeError("decoder_mlp: x must have shape [..., in]")
    width = x.shape[-1]
    for k, (w, b) in enumerate([(w, b) for w, b in trunk] + [(w, b) for w, b, _ in heads]):
        if w.ndim != 2 or w.shape[1] != width or tuple(b.shape) != (w.shape[0],):
            raise RuntimeError(f"decoder_mlp: expected weight [out, {width}] and bias [out], got {tuple(w.shape)} and {tuple(b.shape)}")
        if k < len(trunk):
            width = w.shape[0]
    outs = _DecoderMLP.apply(_aligned(x.reshape(-1, x.shape[-1])), len(trunk), tuple(acts), *[p.contiguous() for p in params])
    return tuple(o.reshape(*x.shape[:-1], o.shape[-1]) for o in outs)


class SineActivation(nn.Module):
    def __init__(self, omega_0=30):
        super().__init__()
        self.omega_0 = omega_0

    def forward(self, x):
        return torch.sin(self.omega_0 * x)


def _act_module(act):
    return {"softplus": nn.Softplus, "relu": nn.ReLU, "sine": SineActivation, "gelu": nn.GELU, "tanh": nn.Tanh}[act]()


def _net(n_features, hidden_dim, act):
    a = _act_module(act)   # (the reference shares one activation module between the two places too)
    return nn.Sequential(nn.Linear(n_features, hidden_dim), a, nn.Linear(hidden_dim, hidden_dim), a)


def _only_gelu(name, act):
    if act != "gelu":
        raise NotImplementedError(f"{name} (MI355X): only act='gelu' is fused (what the reference's model constructs), got {act!r}")


def _wb(linear):
    return linear.weight, linear.bias


class AppearanceDecoder(nn.Module):
    def __init__(self, n_features, hidden_dim=64, act='gelu'):
        super().__init__()
        self.hidden_dim = hidden_dim
        self.act = act
        self.net = _net(n_features, hidden_dim, act)
        self.opacity = nn.Sequential(nn.Linear(hidden_dim, 1), nn.Sigmoid())
        self.shs = nn.Linear(hidden_dim, 16 * 3)

    def forward(self, x):
        _only_gelu("AppearanceDecoder", self.act)
        shs, opacity = decoder_mlp(x, [_wb(self.net[0]), _wb(self.net[2])], [(*_wb(self.shs), None), (*_wb(self.opacity[0]), "sigmoid")])
        return {'shs': shs, 'opacity': opacity}


class DeformationDecoder(nn.Module):
    def __init__(self, n_features, hidden_dim=128, weight_norm=True, act='gelu', disable_posedirs=False):
        super().__init__()
        self.hidden_dim = hidden_dim
        self.act = act
        self.sine = SineActivation(omega_0=30)
        self.disable_posedirs = disable_posedirs
        self.net = _net(n_features, hidden_dim, act)
        self.skinning_linear = nn.Linear(hidden_dim, hidden_dim)
        self.skinning = nn.Linear(hidden_dim, 24)
        if weight_norm:
            self.skinning_linear = nn.utils.weight_norm(self.skinning_linear)
        if not disable_posedirs:
            self.blendshapes = nn.Linear(hidden_dim, 3 * 207)
            nn.init.constant_(self.blendshapes.bias, 0.0)
            nn.init.constant_(self.blendshapes.weight, 0.0)

    def forward(self, x):
        _only_gelu("DeformationDecoder", self.act)
        if not self.disable_posedirs:
            raise NotImplementedError("DeformationDecoder (MI355X): only disable_posedirs=True is fused (every release config sets it)")
        sl = self.skinning_linear
        # the effective weight of the weight-normed layer, by torch's own op: autograd carries its gradient to weight_g and weight_v
        w_sl = torch._weight_norm(sl.weight_v, sl.weight_g, 0) if hasattr(sl, "weight_g") else sl.weight
        lbs_weights, = decoder_mlp(x, [_wb(self.net[0]), _wb(self.net[2]), (w_sl, sl.bias)], [(*_wb(self.skinning), "gelu")])
        return {'lbs_weights': lbs_weights, 'posedirs': None}


class GeometryDecoder(nn.Module):
    def __init__(self, n_features, use_surface=False, hidden_dim=128, act='gelu'):
        super().__init__()
        self.hidden_dim = hidden_dim
        self.act = act
        self.net = _net(n_features, hidden_dim, act)
        self.xyz = nn.Sequential(self.net, nn.Linear(hidden_dim, 3))
        self.rotations = nn.Sequential(self.net, nn.Linear(hidden_dim, 6))
        self.scales = nn.Sequential(self.net, nn.Linear(hidden_dim, 2 if use_surface else 3))

    def forward(self, x):
        _only_gelu("GeometryDecoder", self.act)
        xyz, rotations, scales = decoder_mlp(x, [_wb(self.net[0]), _wb(self.net[2])],
                                             [(*_wb(self.xyz[1]), None), (*_wb(self.rotations[1]), None), (*_wb(self.scales[1]), "gelu")])
        return {'xyz': xyz, 'rotations': rotations, 'scales': scales}
