"""The optimizer step of the two models as one fused launch each, or one for both.

`Adam` takes the place of `torch.optim.Adam` where the reference builds its optimizers,

    self.optimizer = torch.optim.Adam(params, lr=0.0, eps=1e-15)        /root/reference/hugs/models/scene.py:213
                                                                         /root/reference/hugs/models/hugs_trimlp.py:701

one parameter group per tensor (6 for the scene; 9 groups, 37 tensors for the human: 36 weights and biases, one of them split into `g` and `v` by weight_norm), stepped at
/root/reference/hugs/trainer/gs_trainer.py:344-351.  torch walks such an optimizer group by group, about a dozen elementwise launches
and as many passes over memory per group; here every tensor of the optimizer -- `fused_step(a, b)`: of several optimizers -- is one
record of a table that travels in the argument of ONE kernel (csrc/optim.hip), which reads p, g, m, v once and writes p, m, v once.

State, defaults and parameter groups are torch's own (`step` a CPU float32 scalar tensor, `exp_avg`, `exp_avg_sq`), so `state_dict()` /
`load_state_dict()` interchange with `torch.optim.Adam` both ways and the reference's optimizer surgery (`replace_tensor_to_optimizer`,
`_prune_optimizer`, `cat_tensors_to_optimizer`: scene.py:310-379, hugs_trimlp.py:718-790) works unchanged: nothing is cached between
steps, `group["lr"]` is read every step.  fp32 parameters on the GPU only: no CPU fallback.  weight_decay, amsgrad, maximize,
capturable and differentiable are not implemented (the reference uses none of them); `foreach` and `fused` are accepted and ignored.
"""
import ctypes as C
import math
import struct

import torch

from diff_gaussian_rasterization import _call, _load, _require_gpu
from diff_gaussian_rasterization._abi import _AdamTensor

# the table is packed with `struct` (one call per record) and handed over as an array of the mirror, _AdamTensor:
# param, grad, exp_avg, exp_avg_sq, numel, 1 - b1, b2, 1 - b2, eps, step_size, bc2_sqrt
_RECORD = struct.Struct("@PPPPq6f")
assert _RECORD.size == C.sizeof(_AdamTensor) == 64
_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable")
_layout_copies = 0


def adam_limits():
    """(tensors per launch, elements per workgroup) of the kernel: launch-shape facts, results do not depend on them."""
    k, chunk = C.c_int32(0), C.c_int32(0)
    _load().hgs_adam_limits(C.byref(k), C.byref(chunk))
    return k.value, chunk.value


def layout_copies(reset=False):
    """How many gradients or moments had to be brought to their parameter's memory layout with a copy so far (debug counter)."""
    global _layout_copies
    n = _layout_copies
    if reset:
        _layout_copies = 0
    return n


def _dense(t):
    """non-overlapping and dense: the tensor's elements are exactly the numel() floats behind data_ptr(), in some order"""
    if t.is_contiguous():
        return True
    expect = 1
    for stride, size in sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz != 1):
        if stride != expect:
            return False
        expect *= size
    return True


def _as_laid_out(x, p):
    """x in p's memory layout (same sizes and strides): x itself, or one copy"""
    global _layout_copies
    if x.stride() == p.stride() or x.numel() == 0:
        return x
    if all(sx == sp for sx, sp, n in zip(x.stride(), p.stride(), p.shape) if n != 1):   # (the stride of a dimension of one element says nothing)
        return x
    _layout_copies += 1
    return torch.empty_like(p, requires_grad=False).copy_(x)


def _check_group(group):
    if group["weight_decay"] != 0:
        raise NotImplementedError("hugs_amd.optim.Adam: weight_decay is not implemented (the reference's optimizers use none)")
    for key in _UNSUPPORTED:
        if group.get(key):
            raise NotImplementedError(f"hugs_amd.optim.Adam: {key}=True is not implemented (the reference's optimizers do not use it)")


class Adam(torch.optim.Optimizer):
    """torch.optim.Adam's signature, state and state_dict; `step()` is one launch of the multi-tensor kernel per adam_limits()[0] tensors with a gradient."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, **more):
        _check_group(dict(weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, capturable=capturable, differentiable=differentiable))
        # torch's own constructor validates lr / betas / eps and says which keys a group of the installed version carries
        template = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **more)
        super().__init__(params, dict(template.defaults))
        for group in self.param_groups:
            _check_group(group)

    def __setstate__(self, state):
        super().__setstate__(state)
        template = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).defaults
        for group in self.param_groups:
            for key, value in template.items():
                group.setdefault(key, value)
            for p in group["params"]:
                st = self.state.get(p)
                if st and "step" in st:
                    step = st["step"]
                    # a checkpoint of a fused=True / capturable=True optimizer keeps `step` on the device: to the host ONCE, here
                    if torch.is_tensor(step):
                        if step.device.type != "cpu":
                            st["step"] = step.detach().to("cpu", torch.float32)
                    else:
                        st["step"] = torch.tensor(float(step), dtype=torch.float32)

    def _records(self, out):
        """Appends (param, grad, exp_avg, exp_avg_sq, group, state) of every parameter with a gradient; creates missing state; raises on
        anything the kernel does not take.  Nothing is stepped yet."""
        for group in self.param_groups:
            _check_group(group)
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                _require_gpu(p, "param")
                if p.dtype != torch.float32 or g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape:
                    raise RuntimeError("hugs_amd.optim.Adam: parameters and gradients must be float32 on the same GPU and of one shape; there is no CPU fallback")
                if not _dense(p):
                    raise RuntimeError("hugs_amd.optim.Adam: a parameter must be non-overlapping and dense (an expanded or strided view cannot be updated in place as flat storage)")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if torch.is_tensor(st["step"]) and st["step"].device.type != "cpu":   # (put there by hand after load_state_dict; moved once)
                    st["step"] = st["step"].detach().to("cpu", torch.float32)
                for key in ("exp_avg", "exp_avg_sq"):
                    m = st[key]
                    if m.dtype != torch.float32 or m.device != p.device or m.shape != p.shape:
                        raise RuntimeError(f"hugs_amd.optim.Adam: state `{key}` must be float32 on the parameter's GPU and of its shape")
                    st[key] = _as_laid_out(m, p)
                out.append((p, _as_laid_out(g, p), st["exp_avg"], st["exp_avg_sq"], group, st))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        _fused_step((self,))
        return loss


def _fused_step(optimizers):
    with torch.no_grad():
        recs = []
        for opt in optimizers:
            if not isinstance(opt, Adam):
                raise TypeError("fused_step: every optimizer must be a hugs_amd.optim.Adam")
            opt._records(recs)
        if not recs:
            return
        by_device = {}
        for r in recs:
            by_device.setdefault(r[0].device, []).append(r)
        lib = _load()
        for dev, rs in by_device.items():
            buf = bytearray(_RECORD.size * len(rs))
            for i, (p, g, m, v, group, st) in enumerate(rs):
                t = float(st["step"]) + 1.0   # (a CPU tensor or a number; _records() has seen to a tensor on the device)
                b1, b2 = (float(b) for b in group["betas"])
                lr = float(group["lr"])
                _RECORD.pack_into(buf, i * _RECORD.size, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), 1.0 - b1, b2, 1.0 - b2,
                                  float(group["eps"]), lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t))
            # (validated before any launch: when this raises, no tensor and no step count has moved)
            _call(dev, "adam step", lib.hgs_adam_step, (_AdamTensor * len(rs)).from_buffer(buf), len(rs))
            for r in rs:
                st = r[5]
                if torch.is_tensor(st["step"]):
                    st["step"] += 1
                else:
                    st["step"] = st["step"] + 1
            # the kernel rewrote memory behind autograd's back: whoever keys a cache on `_version` (hugs_amd.losses' shared pass, the SMPL
            # wrapper's host copy of `parents`) must see it
            torch.autograd.graph.increment_version([x for r in rs for x in r[:1] + r[2:4]])


def fused_step(*optimizers):
    """`a.step(); b.step()` of several hugs_amd.optim.Adam optimizers as ONE table: the trainer's two back-to-back optimizer steps (43
    tensors) are one launch.  Bit for bit what the separate steps give.  Optimizer step hooks are not run."""
    _fused_step(optimizers)
