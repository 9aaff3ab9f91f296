"""Fused densification statistics.

Drop-in for the two statements that open `GaussianTrainer.scene_densification` / `human_densification`
(/root/reference/hugs/trainer/gs_trainer.py:406-411, 429-435) together with `add_densification_stats`
(/root/reference/hugs/models/scene.py:460-462, hugs/models/hugs_trimlp.py:880-882):

    model.max_radii2D[vis] = torch.max(model.max_radii2D[vis], radii[vis])
    model.xyz_gradient_accum[vis] += torch.norm(viewspace_points.grad[:vis.shape[0]][vis, :2], dim=-1, keepdim=True)
    model.denom[vis] += 1

One HIP kernel instead of four boolean-indexed torch ops; same in-place semantics, including the reference's
habit of pairing the FIRST n rows of the gradient with the model's n Gaussians.  No CPU fallback.

The densification round itself (row f-12): `densify_and_prune_scene` and `densify_and_prune_human` do what
`SceneGS.densify_and_prune` (/root/reference/hugs/models/scene.py:325-458) and `HUGS_TRIMLP.densify_and_prune`
(hugs/models/hugs_trimlp.py:733-878) do -- clone, split, prune, the optimizer surgery, the statistics -- as a stream compaction
(csrc/densify.hip): a plan pass (classify + scan), ONE host readback of five counts, one `torch.randn` for the split noise, and one
multi-tensor scatter that reads every source row once and writes every result at its final size.  The rules, row by row, are in
include/hgs_rasterizer.h.
"""
import ctypes as C
import struct

import torch

from diff_gaussian_rasterization import _call, _load, _require_gpu

SCENE, HUMAN = 0, 1                                                        # HGS_DENSIFY_SCENE, HGS_DENSIFY_HUMAN
COPY, MOMENT, ZERO, XYZ_SPLIT, LOG_SCALE_SPLIT, DIV_SPLIT = range(6)       # HGS_DENSIFY_* modes
_RECORD = struct.Struct("@PPii")                                           # hgs_densify_tensor: src, dst, width, mode
SCENE_GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")   # the reference's group names, scene.py:201-208
_SCENE_MODES = {"xyz": XYZ_SPLIT, "scaling": LOG_SCALE_SPLIT}


def update_densification_stats(max_radii2D, xyz_gradient_accum, denom, viewspace_point_tensor, visibility_filter, radii):
    """In-place update of the three per-Gaussian statistics tensors (fp32; [n], [n,1], [n,1])."""
    lib = _load()
    grad = viewspace_point_tensor.grad if viewspace_point_tensor.grad is not None else None
    if grad is None:
        raise RuntimeError("viewspace_point_tensor has no .grad (call backward first)")
    n = int(visibility_filter.shape[0])
    for t, name in ((max_radii2D, "max_radii2D"), (xyz_gradient_accum, "xyz_gradient_accum"), (denom, "denom"), (grad, "grad")):
        _require_gpu(t, name)
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous float32 tensor")
    if grad.shape[0] < n or max_radii2D.numel() != n or xyz_gradient_accum.numel() != n or denom.numel() != n:
        raise RuntimeError("size mismatch between the statistics tensors, the filter and the gradient")
    vis = visibility_filter.contiguous().view(torch.uint8) if visibility_filter.dtype == torch.bool else \
        (visibility_filter != 0).contiguous().view(torch.uint8)
    rad = radii.to(torch.int32).contiguous()
    _call(grad.device, "densification_stats", lib.hgs_densification_stats, n, grad.data_ptr(), rad.data_ptr(), vis.data_ptr(),
          max_radii2D.data_ptr(), xyz_gradient_accum.data_ptr(), denom.data_ptr())


# ---------------------------------------------------------------------------------------------------------------------------------
# row f-12: the round

def densify_limits():
    """(rows per workgroup of the passes, tensors per scatter launch): launch-shape facts, results do not depend on them."""
    rows, tensors = C.c_int32(0), C.c_int32(0)
    _load().hgs_densify_limits(C.byref(rows), C.byref(tensors))
    return rows.value, tensors.value


def _read_totals(totals):
    """THE host synchronisation of a round: [originals kept, clones, split copy 1, split copy 2, split-selected rows]."""
    return totals.tolist()


def _rows(t, name, n, tail=None):
    """t as the kernels take it: on the GPU, fp32, contiguous, n rows (and the given trailing shape)"""
    _require_gpu(t, name)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous float32 tensor")
    if t.dim() == 0 or t.shape[0] != n or (tail is not None and tuple(t.shape[1:]) != tuple(tail)):
        raise RuntimeError(f"{name}: expected shape ({n}, {', '.join(map(str, tail)) if tail is not None else '...'}), got {tuple(t.shape)}")
    return t.detach()


def _width(t):
    w = 1
    for s in t.shape[1:]:
        w *= s
    return w


def _groups(optimizer, names, params):
    """{name: group} of the optimizer's groups named in `names`; each holds exactly the one parameter `params[name]`"""
    found = {}
    for group in optimizer.param_groups:
        name = group.get("name")
        if name in names:
            if name in found:
                raise RuntimeError(f"the optimizer has two groups named `{name}`")
            if len(group["params"]) != 1:
                raise RuntimeError(f"group `{name}` must hold exactly one parameter")
            if name in params and group["params"][0] is not params[name]:
                raise RuntimeError(f"group `{name}` does not hold the parameter that was passed for it")
            found[name] = group
    missing = [name for name in names if name not in found]
    if missing:
        raise RuntimeError(f"the optimizer has no group named {missing}")
    return found


def _round(flavour, n, dev, densify, stats, scales, opacity, rotation, thresholds, sources, generator):
    """Plan, readback, noise, scatter.  `sources`: [(tensor or None, mode, trailing shape)], the statistics last; returns the results
    in that order.  Everything has been validated: nothing here raises after the first launch but the library itself."""
    lib = _load()
    max_grad, min_opacity, small_max, use_screen, max_screen_size, big_max = thresholds
    new = lambda rows, tail: torch.empty((rows,) + tuple(tail), dtype=torch.float32, device=dev)
    if n == 0:
        torch.randn((0, 3), generator=generator, device=dev, dtype=torch.float32)
        return [new(0, tail) for _, _, tail in sources]
    rows_per_block, _ = densify_limits()
    blocks = (n + rows_per_block - 1) // rows_per_block
    kind = torch.empty(n, dtype=torch.uint8, device=dev)
    partials = torch.empty(4 * blocks, dtype=torch.int32, device=dev)
    totals = torch.empty(5, dtype=torch.int32, device=dev)
    accum, denom, radii = stats
    _call(dev, "densify plan", lib.hgs_densify_plan, flavour, n, int(densify), accum.data_ptr(), denom.data_ptr(), radii.data_ptr(),
          scales.data_ptr(), opacity.data_ptr(), max_grad, min_opacity, small_max, int(use_screen), max_screen_size, big_max,
          kind.data_ptr(), partials.data_ptr(), totals.data_ptr())
    kept, clones, split1, split2, selected = _read_totals(totals)
    total = kept + clones + split1 + split2
    if total >= 2 ** 31:
        raise RuntimeError(f"the round would leave {total} rows: beyond 2^31 - 1")
    # normal(0, 1) then scaled by std inside the kernel: what torch.normal(mean=zeros, std=stds) draws (hugs_trimlp.py:827, scene.py:412)
    noise = torch.randn((2 * selected, 3), generator=generator, device=dev, dtype=torch.float32)
    out = [new(total, tail) for _, _, tail in sources]
    if total == 0:
        return out
    buf = bytearray(_RECORD.size * len(sources))
    for i, ((src, mode, tail), dst) in enumerate(zip(sources, out)):
        _RECORD.pack_into(buf, i * _RECORD.size, 0 if src is None else src.data_ptr(), dst.data_ptr(), _width(dst), mode)
    _call(dev, "densify scatter", lib.hgs_densify_scatter, flavour, n, kind.data_ptr(), partials.data_ptr(), totals.data_ptr(), bytes(buf),
          len(sources), scales.data_ptr(), rotation.data_ptr(), noise.data_ptr() if selected else scales.data_ptr())
    return out


def _sources_of(names, params, optimizer, modes):
    """The scatter's sources of the densified groups: parameter, then its two moments where the optimizer holds state for it"""
    sources, layout = [], []
    for name in names:
        p = params[name]
        state = optimizer.state.get(p, None)
        has_state = state is not None and "exp_avg" in state
        sources.append((p.detach(), modes.get(name, COPY), p.shape[1:]))
        if has_state:
            for key in ("exp_avg", "exp_avg_sq"):
                m = state[key]
                _require_gpu(m, f"{name}.{key}")
                if m.dtype != torch.float32 or m.shape != p.shape:
                    raise RuntimeError(f"state `{key}` of group `{name}` must be float32 and of its parameter's shape")
                sources.append((m.detach().contiguous(), MOMENT, p.shape[1:]))
        layout.append((name, has_state))
    return sources, layout


def _surgery(groups, layout, optimizer, results):
    """What _prune_optimizer / cat_tensors_to_optimizer leave behind (scene.py:325-379): a new nn.Parameter per group, the SAME state
    dict re-keyed to it with its moments replaced; `step` and every other key untouched.  Consumes `results` front to back."""
    new_params = {}
    for name, has_state in layout:
        group = groups[name]
        old = group["params"][0]
        param = torch.nn.Parameter(results.pop(0).requires_grad_(True))
        if has_state:
            state = optimizer.state[old]
            state["exp_avg"], state["exp_avg_sq"] = results.pop(0), results.pop(0)
            del optimizer.state[old]
            optimizer.state[param] = state
        group["params"][0] = param
        new_params[name] = param
    return new_params


def _stats_sources(stats, n, densify):
    accum, denom, radii = stats
    accum, denom, radii = _rows(accum, "xyz_gradient_accum", n, (1,)), _rows(denom, "denom", n, (1,)), _rows(radii, "max_radii2D", n, ())
    # the densify branch has reset them (densification_postfix): zeros of the final size; beyond max_n_gs they are gathered
    mode = ZERO if densify else COPY
    return (accum, denom, radii), [(None if densify else t, mode, t.shape[1:]) for t in (accum, denom, radii)]


def _thresholds(max_grad, min_opacity, extent, max_screen_size, percent_dense):
    return (float(max_grad), float(min_opacity), float(percent_dense * extent), bool(max_screen_size),
            float(max_screen_size) if max_screen_size else 0.0, float(0.1 * extent))


@torch.no_grad()
def densify_and_prune_scene(params, optimizer, stats, max_grad, min_opacity, extent, max_screen_size, max_n_gs=None, percent_dense=0.01,
                            generator=None):
    """`SceneGS.densify_and_prune` (scene.py:441-458) on `params` = {xyz, f_dc, f_rest, opacity, scaling, rotation: nn.Parameter}, the
    optimizer that holds them one per group under those names, and stats = (xyz_gradient_accum [n,1], denom [n,1], max_radii2D [n]).
    Returns (new params by name, (xyz_gradient_accum, denom, max_radii2D)); the optimizer's groups and state are moved to the new
    parameters as the reference's surgery moves them.  One host synchronisation; results are allocated once at their final size."""
    if set(params) != set(SCENE_GROUPS):
        raise RuntimeError(f"params must hold exactly {SCENE_GROUPS}")
    n = int(params["xyz"].shape[0])
    dev = params["xyz"].device
    for name, tail in (("xyz", (3,)), ("f_dc", None), ("f_rest", None), ("opacity", (1,)), ("scaling", (3,)), ("rotation", (4,))):
        _rows(params[name], name, n, tail)
    groups = _groups(optimizer, SCENE_GROUPS, params)
    densify = n <= (max_n_gs if max_n_gs else n + 1)
    stats, stat_sources = _stats_sources(stats, n, densify)
    sources, layout = _sources_of(SCENE_GROUPS, params, optimizer, _SCENE_MODES)
    results = _round(SCENE, n, dev, densify, stats, params["scaling"].detach(), params["opacity"].detach(), params["rotation"].detach(),
                     _thresholds(max_grad, min_opacity, extent, max_screen_size, percent_dense), sources + stat_sources, generator)
    new_stats = tuple(results[-3:])
    return _surgery(groups, layout, optimizer, results[:-3]), new_stats


@torch.no_grad()
def densify_and_prune_human(xyz, scaling_multiplier, human_gs_out, optimizer, stats, max_grad, min_opacity, extent, max_screen_size,
                            max_n_gs=None, percent_dense=0.01, generator=None, densify_group_names=("xyz",)):
    """`HUGS_TRIMLP.densify_and_prune` (hugs_trimlp.py:857-878): `xyz` the parameter of the optimizer's group "xyz", the plain tensor
    `scaling_multiplier` [n,1], and from `human_gs_out` the keys 'opacity' [n,1], 'scales_canon' [n,3], 'rotmat_canon' [n,3,3].  Only the
    groups named in `densify_group_names` are looked at (the complement of the model's `non_densify_params_keys`); a group other than
    "xyz" in it has its rows copied.  Returns (new params by name, (xyz_gradient_accum, denom, max_radii2D), scaling_multiplier,
    opacity_tmp, scales_tmp, rotmat_tmp).  One host synchronisation."""
    names = tuple(densify_group_names)
    if "xyz" not in names:
        raise RuntimeError("densify_group_names must contain 'xyz'")
    n = int(xyz.shape[0])
    dev = xyz.device
    _rows(xyz, "xyz", n, (3,))
    groups = _groups(optimizer, names, {"xyz": xyz})
    params = {name: groups[name]["params"][0] for name in names}
    for name in names:
        _rows(params[name], name, n)
    mult = _rows(scaling_multiplier, "scaling_multiplier", n, (1,))
    opacity = _rows(human_gs_out["opacity"], "human_gs_out['opacity']", n, (1,))
    scales = _rows(human_gs_out["scales_canon"], "human_gs_out['scales_canon']", n, (3,))
    rotmat = _rows(human_gs_out["rotmat_canon"], "human_gs_out['rotmat_canon']", n, (3, 3))
    densify = n <= (max_n_gs if max_n_gs else n + 1)
    stats, stat_sources = _stats_sources(stats, n, densify)
    sources, layout = _sources_of(names, params, optimizer, {"xyz": XYZ_SPLIT})
    # scales_tmp of a split copy is the source row's, unchanged: the reference's own habit (hugs_trimlp.py:832)
    extra = [(mult, DIV_SPLIT, (1,)), (opacity, COPY, (1,)), (scales, COPY, (3,)), (rotmat, COPY, (3, 3))]
    results = _round(HUMAN, n, dev, densify, stats, scales, opacity, rotmat,
                     _thresholds(max_grad, min_opacity, extent, max_screen_size, percent_dense), sources + extra + stat_sources, generator)
    new_stats = tuple(results[-3:])
    new_mult, opacity_tmp, scales_tmp, rotmat_tmp = results[-7:-3]
    return _surgery(groups, layout, optimizer, results[:-7]), new_stats, new_mult, opacity_tmp, scales_tmp, rotmat_tmp
