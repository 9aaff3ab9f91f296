"""Fused TriPlane.forward (row f-8): the statement that opens every human step of the reference,
/root/reference/hugs/models/hugs_trimlp.py:206,408 `self.triplane(self.get_xyz)` -- three F.grid_sample calls and a cat
(/root/reference/hugs/models/modules/triplane.py:26-40) -- as one HIP kernel forward and one backward (csrc/triplane.hip).

    from hugs_amd.triplane import TriPlane                  # instead of `from .modules.triplane import TriPlane`

Same constructor, attributes, parameter names and logical shapes as the reference's module; the three parameters are held in
torch.channels_last (a texel's 32 channels are then one 128-byte segment: the backward's float atomics take the fast shape).
`load_state_dict` of NCHW tensors, Adam's state and its update keep those strides, and `state_dict()` saves reference shapes.
The plane gradients are summed with float atomics: their last bits depend on arrival order.  The forward and dL/dx are
bit-reproducible.  No host synchronisation (the reference's range assertion is `check_range=True`).  No CPU fallback.
"""
import ctypes as C

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from diff_gaussian_rasterization import _aligned, _call, _load, _require_gpu
from diff_gaussian_rasterization import _row_ptr as _ptr

EPS = 1e-3
_FEATURES = 32


def _geometry(planes):
    """(res, strides) as the C ABI takes them: res = (resX, resY, resZ), strides[p] = (channel, row, column) in elements"""
    res = (C.c_int32 * 3)(planes[0].shape[2], planes[0].shape[3], planes[1].shape[3])
    strides = (C.c_int64 * 9)(*[s for p in planes for s in p.stride()[1:]])
    return res, strides


class _TriplaneSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plane_xy, plane_xz, plane_yz, x, center, scale):
        lib = _load()
        planes = (plane_xy, plane_xz, plane_yz)
        n, F, dev = x.shape[0], plane_xy.shape[1], x.device
        feat = torch.empty(n, 3 * F, dtype=torch.float32, device=dev)
        res, strides = _geometry(planes)
        _call(dev, "triplane_sample", lib.hgs_triplane_forward, n, F, res, strides, center, scale, x.data_ptr(), plane_xy.data_ptr(),
              plane_xz.data_ptr(), plane_yz.data_ptr(), feat.data_ptr())
        ctx.save_for_backward(plane_xy, plane_xz, plane_yz, x)
        ctx.center, ctx.scale = center, scale
        return feat

    @staticmethod
    @once_differentiable
    def backward(ctx, g_feat):
        *planes, x = ctx.saved_tensors
        lib = _load()
        n, F, dev = x.shape[0], planes[0].shape[1], x.device
        g_feat = _aligned(g_feat)
        # zeroed with the PARAMETER's strides: the kernel adds into them through the same strides it reads the planes with
        d_planes = [torch.zeros_like(p, memory_format=torch.preserve_format) if ctx.needs_input_grad[i] else None for i, p in enumerate(planes)]
        d_x = torch.empty_like(x) if ctx.needs_input_grad[3] else None
        res, strides = _geometry(planes)
        _call(dev, "triplane_sample backward", lib.hgs_triplane_backward, n, F, res, strides, ctx.center, ctx.scale, x.data_ptr(),
              (C.c_void_p * 3)(*[p.data_ptr() for p in planes]), g_feat.data_ptr(), _ptr(d_x), (C.c_void_p * 3)(*[_ptr(d) for d in d_planes]))
        return d_planes[0], d_planes[1], d_planes[2], d_x, None, None


def _dense(p):
    """a plane whose strides the kernel can address as they stand: NCHW-contiguous or channels-last; anything else is copied"""
    return p if p.is_contiguous() or p.is_contiguous(memory_format=torch.channels_last) else p.contiguous()


def triplane_sample(plane_xy, plane_xz, plane_yz, x, center=0.0, scale=2.0):
    """plane_xy [1,F,resX,resY], plane_xz [1,F,resX,resZ], plane_yz [1,F,resY,resZ] (NCHW or channels-last strides), x [..., 3]
    -> [..., 3F]: cat of the three bilinear samples at ((x - center) / scale + 0.5) * 2 - 1, as TriPlane.forward forms them."""
    planes = (plane_xy, plane_xz, plane_yz)
    if any(p.ndim != 4 or p.shape[0] != 1 for p in planes):
        raise RuntimeError("triplane_sample: every plane must have shape [1, F, H, W]")
    if plane_xy.shape[1] != _FEATURES:
        raise NotImplementedError(f"triplane_sample (MI355X): only {_FEATURES} features per plane (all the reference uses), got {plane_xy.shape[1]}")
    for name, t in (("plane_xy", plane_xy), ("plane_xz", plane_xz), ("plane_yz", plane_yz), ("x", x)):
        _require_gpu(t, name)
        if t.dtype != torch.float32:
            raise RuntimeError(f"triplane_sample: {name} must be float32")
    F, (rx, ry), rz = plane_xy.shape[1], plane_xy.shape[2:], plane_xz.shape[3]
    if tuple(plane_xz.shape) != (1, F, rx, rz) or tuple(plane_yz.shape) != (1, F, ry, rz):
        raise RuntimeError(f"triplane_sample: expected plane_xz [1, {F}, {rx}, resZ] and plane_yz [1, {F}, {ry}, resZ], "
                           f"got {tuple(plane_xz.shape)} and {tuple(plane_yz.shape)}")
    if x.ndim < 1 or x.shape[-1] != 3:
        raise RuntimeError("triplane_sample: x must have shape [..., 3]")
    feat = _TriplaneSample.apply(_dense(plane_xy), _dense(plane_xz), _dense(plane_yz), x.reshape(-1, 3).contiguous(), float(center), float(scale))
    return feat.reshape(*x.shape[:-1], 3 * F)


class TriPlane(nn.Module):
    def __init__(self, features=32, resX=256, resY=256, resZ=256):
        super().__init__()
        cl = lambda *shape: nn.Parameter(torch.randn(*shape).contiguous(memory_format=torch.channels_last))
        self.plane_xy = cl(1, features, resX, resY)
        self.plane_xz = cl(1, features, resX, resZ)
        self.plane_yz = cl(1, features, resY, resZ)
        self.dim = features
        self.n_input_dims = 3
        self.n_output_dims = 3 * features
        self.center = 0.0
        self.scale = 2.0

    def forward(self, x, check_range=False):
        if check_range:   # the reference's assertion (triplane.py:29): synchronises with the host
            u = (x - self.center) / self.scale + 0.5
            assert u.max() <= 1 + EPS and u.min() >= -EPS, f"x must be in [0, 1], got {u.min()} and {u.max()}"
        return triplane_sample(self.plane_xy, self.plane_xz, self.plane_yz, x, self.center, self.scale)
