"""Fused photometric loss (row f-5): drop-ins for `l1_loss` and `ssim` of /root/reference/hugs/losses/utils.py:54-58,77-108,
the two terms every training step computes on the rendered image (hugs/losses/loss.py:88-107) and again on the human-only
render (:128-137).

    from hugs_amd.losses import l1_loss, ssim            # instead of `from .utils import l1_loss, ssim` (loss.py:13)

Same signatures, same values (fp32; the 11x11 window is applied as 11 + 11 taps, so sums differ from conv2d's in the last
bits), same gradient with respect to the first argument -- the render; the target never requires a gradient at the
reference's call sites and asking for one raises.  `l1_ssim(pred, gt)` returns both terms from ONE pass over the images
(`ssim` and `l1_loss` called one after the other on the same pair share that pass too: the second call finds the first
one's result).  No CPU fallback: the HIP library does the work or the call raises.

The reference's trainer reaches the two functions through `HumanSceneLoss.forward` (hugs/losses/loss.py:46-162), which wraps them
in mask arithmetic on full images.  `masked_l1_ssim(pred, gt, mask, mode, bg)` is that arithmetic inside the fused pass (the
composites are formed while the tiles are loaded, none is written to memory), and `HumanSceneLoss` the module itself:

    from hugs_amd.losses import HumanSceneLoss           # instead of `from hugs.losses.loss import HumanSceneLoss`
"""
import os
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from diff_gaussian_rasterization import _call, _load, _require_gpu
from diff_gaussian_rasterization import _row_ptr as _ptr


class _SsimL1(torch.autograd.Function):
    """(pred [C,H,W], gt [C,H,W]) -> ONE tensor [ssim mean, l1 mean, l1 sum]: hgs_ssim_l1_forward / hgs_ssim_l1_backward.
    (One output: the terms the callers hand out are views of it, and a view keeps its base alive -- which is what lets the
    shared-pass entry below hold a WEAK reference and still be found while any of the terms is in use.)"""

    @staticmethod
    def forward(ctx, pred, gt):
        lib = _load()
        Cn, H, W = pred.shape
        need_grad = pred.requires_grad
        out = torch.empty(3, dtype=torch.float32, device=pred.device)
        maps = torch.empty(3, Cn, H, W, dtype=torch.float32, device=pred.device) if need_grad else None
        ws = torch.empty(lib.hgs_ssim_l1_workspace(Cn, H, W), dtype=torch.uint8, device=pred.device)
        _call(pred.device, "ssim_l1_forward", lib.hgs_ssim_l1_forward, Cn, H, W, pred.data_ptr(), gt.data_ptr(), _ptr(maps), ws.data_ptr(),
              out.data_ptr())
        ctx.save_for_backward(pred, gt, maps)
        return out

    @staticmethod
    def backward(ctx, g):
        hit = _LAST.get("entry")                  # (THIS graph is spent: a later call on the same pair computes afresh;
        if hit is not None and hit[4] == id(ctx):  #  an entry that belongs to another graph stays)
            _LAST.pop("entry", None)
        pred, gt, maps = ctx.saved_tensors
        lib = _load()
        Cn, H, W = pred.shape
        # d(l1 mean) = d(l1 sum) / (C H W): one device scalar for the kernel, no host round trip
        g = g.to(torch.float32)
        g_s = g[0:1].contiguous()
        g_l1 = (g[1:2] / float(Cn * H * W) + g[2:3]).contiguous()
        grad = torch.empty_like(pred)
        _call(pred.device, "ssim_l1_backward", lib.hgs_ssim_l1_backward, Cn, H, W, pred.data_ptr(), gt.data_ptr(), _ptr(maps), g_s.data_ptr(),
              g_l1.data_ptr(), grad.data_ptr())
        return grad, None


def _prep(pred, gt):
    if pred.shape != gt.shape or pred.ndim not in (3, 4):
        raise ValueError("expected two images of the same shape, [C,H,W] or [B,C,H,W]")
    if gt.requires_grad:
        raise NotImplementedError("the fused loss differentiates with respect to its first argument only (the render)")
    _require_gpu(pred, "network_output")
    _require_gpu(gt, "gt")
    if pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise RuntimeError("the fused loss takes float32 images")
    return pred.contiguous(), gt.contiguous()


# ssim(a, b) followed by l1_loss(a, b) on the same tensors (loss.py:88-99) is one pass: the pair's result is found again
# while both tensors are alive and unchanged (same objects, same version counters, same storage), while the CALLER still
# holds the first call's result -- the entry keeps only weak references to the three outputs, so a result nobody uses takes
# its autograd node and the 3 x C x H x W partials (75 MB at 1080p) with it at once, not at the next call -- and until that
# graph's backward has run (a backward of ANOTHER graph leaves the entry alone).  `l1_ssim` is the explicit form of the same.
# HGS_LOSS_SHARE_PASS=0 turns the sharing off (every call computes afresh) -- for callers whose custom kernels rewrite a
# tensor's memory behind autograd's back, which no version counter records.
_LAST = {}
_SHARE = os.environ.get("HGS_LOSS_SHARE_PASS", "1") != "0"


def _terms(pred, gt):
    """[ssim mean, l1 mean, l1 sum] (one tensor) of one [C,H,W] pair, computed once per (pred, gt) pair and version."""
    key = (id(pred), id(gt), pred._version, gt._version, pred.data_ptr(), gt.data_ptr(), pred.requires_grad and torch.is_grad_enabled())
    hit = _LAST.get("entry")
    if _SHARE and hit is not None and hit[0] == key and hit[1]() is pred and hit[2]() is gt:
        out = hit[3]()
        if out is not None:
            return out
    out = _SsimL1.apply(pred, gt)
    if not _SHARE:
        return out
    try:
        _LAST["entry"] = (key, weakref.ref(pred), weakref.ref(gt), weakref.ref(out), id(out.grad_fn))
    except TypeError:
        _LAST.pop("entry", None)
    return out


def l1_ssim(network_output, gt):
    """-> (l1_loss(network_output, gt), ssim(network_output, gt)) from one pass over the two images."""
    pred, tgt = _prep(network_output, gt)
    if pred.ndim == 4:
        terms = [_terms(pred[i], tgt[i]) for i in range(pred.shape[0])]
        return torch.stack([t[1] for t in terms]).mean(), torch.stack([t[0] for t in terms]).mean()
    s, l1_mean, _ = _terms(pred, tgt)
    return l1_mean, s


def l1_loss(network_output, gt, mask=None):
    """utils.py:54-58: mean |a - b|, or sum |a - b| / mask.sum() with a mask."""
    pred, tgt = _prep(network_output, gt)
    if pred.ndim == 4:
        terms = [_terms(pred[i], tgt[i]) for i in range(pred.shape[0])]
        total = torch.stack([t[2] for t in terms]).sum()
        return total / mask.sum() if mask is not None else total / float(pred.numel())
    _, l1_mean, l1_sum = _terms(pred, tgt)
    return l1_sum / mask.sum() if mask is not None else l1_mean


def ssim(img1, img2, window_size=11, size_average=True, mask=None):
    """utils.py:77-108 (the `mask` argument is accepted and ignored, as there)."""
    if window_size != 11:
        raise NotImplementedError("ssim (MI355X): window_size 11 (all the reference uses)")
    pred, tgt = _prep(img1, img2)
    if pred.ndim == 3:
        return _terms(pred, tgt)[0]              # (size_average=False on a [C,H,W] image fails in the reference: mean(1) x3)
    per_image = torch.stack([_terms(pred[i], tgt[i])[0] for i in range(pred.shape[0])])
    return per_image.mean() if size_average else per_image


# ---------------------------------------------------------------------------------------------
# HumanSceneLoss's masks (hugs/losses/loss.py:46-162)
_MASKED_MODES = {"human": 1, "scene": 2}                 # HGS_MASKED_HUMAN, HGS_MASKED_SCENE


class _MaskedSsimL1(torch.autograd.Function):
    """(pred [C,H,W], gt [C,H,W], mask [H,W], bg [C] or None, mode) -> ONE tensor [l1, ssim_term, sum(mask), ssim mean]:
    hgs_masked_loss_forward / hgs_masked_loss_backward.  Saved for the backward: the four inputs, the three partial maps and
    the reduced scalars -- no composited image.  Differentiable with respect to pred only."""

    @staticmethod
    def forward(ctx, pred, gt, mask, bg, mode, need_grad):
        lib = _load()
        Cn, H, W = pred.shape
        out = torch.empty(4, dtype=torch.float32, device=pred.device)
        maps = torch.empty(3, Cn, H, W, dtype=torch.float32, device=pred.device) if need_grad else None
        ws = torch.empty(lib.hgs_masked_loss_workspace(Cn, H, W), dtype=torch.uint8, device=pred.device)
        _call(pred.device, "masked_loss_forward", lib.hgs_masked_loss_forward, mode, Cn, H, W, pred.data_ptr(), gt.data_ptr(), mask.data_ptr(),
              _ptr(bg), _ptr(maps), ws.data_ptr(), out.data_ptr())
        ctx.mode = mode
        ctx.save_for_backward(pred, gt, mask, bg, maps, out)
        return out

    @staticmethod
    def backward(ctx, g):
        pred, gt, mask, bg, maps, out = ctx.saved_tensors
        lib = _load()
        Cn, H, W = pred.shape
        g = g.to(torch.float32).contiguous()             # [dL/dl1, dL/dssim_term, .., ..]: two device scalars, read by the kernel
        grad = torch.empty_like(pred)
        _call(pred.device, "masked_loss_backward", lib.hgs_masked_loss_backward, ctx.mode, Cn, H, W, pred.data_ptr(), gt.data_ptr(),
              mask.data_ptr(), _ptr(bg), _ptr(maps), out.data_ptr(), g.data_ptr(), g.data_ptr() + 4, grad.data_ptr())
        return grad, None, None, None, None, None


def masked_l1_ssim(pred, gt, mask, mode, bg=None):
    """-> (Ll1, loss_ssim), the two pre-weight terms of HumanSceneLoss.forward in its `human` or `scene` mode, from one pass:

        human:  x = pred,             y = gt * mask + bg[:, None, None] * (1 - mask)          (loss.py:71,89,99-101; :130-136)
        scene:  x = pred * (1 - mask), y = gt * (1 - mask)                                    (loss.py:78-80,91,99,103)
        Ll1 = |x - y|.sum() / mask.sum(),   loss_ssim = (1 - ssim(x, y)) * mask.sum() / (H * W)

    BOTH modes use the sum of `mask` as it is handed in -- the human mask: the reference's scene mode inverts it and inverts it
    again wherever it sums it.  pred, gt: [C,H,W]; mask: [H,W] or [1,H,W]; bg: [C], required in the human mode; all float32 on
    the GPU, any strides and offsets.  Differentiable with respect to pred only.  mask.sum() == 0 divides by zero on the device,
    as the reference does; nothing is raised.  (Not part of the `ssim` / `l1_loss` shared-pass cache.)"""
    if mode not in _MASKED_MODES:
        raise ValueError(f"masked_l1_ssim: mode must be 'human' or 'scene', not {mode!r}")
    if pred.shape != gt.shape or pred.ndim != 3:
        raise ValueError("expected two images of the same shape, [C,H,W]")
    if mask.shape not in (pred.shape[1:], (1,) + tuple(pred.shape[1:])):
        raise ValueError(f"expected a mask of shape [H,W] or [1,H,W] = {tuple(pred.shape[1:])}, got {tuple(mask.shape)}")
    if mode == "human" and bg is None:
        raise ValueError("masked_l1_ssim: the human mode needs bg, one colour per channel [C]")
    if mode == "scene":
        bg = None                                        # (the scene composites have no background term)
    if bg is not None and tuple(bg.shape) != (pred.shape[0],):
        raise ValueError(f"expected bg of shape [C] = [{pred.shape[0]}], got {tuple(bg.shape)}")
    if gt.requires_grad or mask.requires_grad or (bg is not None and bg.requires_grad):
        raise NotImplementedError("the fused loss differentiates with respect to its first argument only (the render)")
    for t, name in ((pred, "network_output"), (gt, "gt"), (mask, "mask"), (bg, "bg")):
        if t is not None:
            _require_gpu(t, name)
            if t.dtype != torch.float32:
                raise RuntimeError("the fused loss takes float32 images")
    out = _MaskedSsimL1.apply(pred.contiguous(), gt.contiguous(), mask.reshape(mask.shape[-2:]).contiguous(),
                              bg.contiguous() if bg is not None else None, _MASKED_MODES[mode],
                              pred.requires_grad and torch.is_grad_enabled())   # (forward-only, also under no_grad: no maps are kept)
    return out[0], out[1]


class _Extras(dict):
    """extras_dict: `gt_img` is built when somebody reads it (the trainer does at logging steps only, gs_trainer.py:309-310), so a
    training step materialises no composite."""

    def __init__(self, make_gt, **items):
        super().__init__(**items)
        self._make_gt = make_gt

    def __missing__(self, key):
        if key != "gt_img":
            raise KeyError(key)
        self[key] = value = self._make_gt()
        return value


class HumanSceneLoss(nn.Module):
    """hugs/losses/loss.py:16-162 with the masks inside the fused pass: same constructor arguments, same forward signature, same
    keys and values in loss_dict and extras_dict.  `human` and `scene` modes and the human-separation terms of `human_scene` go
    through masked_l1_ssim, the plain `human_scene` terms through l1_ssim; the lbs term is F.mse_loss.  The LPIPS terms are torch
    statements around two objects the caller supplies (keyword-only: nothing here imports lpips or cv2): `lpips`, a callable
    (pred_patches, gt_patches) -> [N] as lpips.LPIPS is, and `patch_sampler`, an object with sample(mask, *images) as
    hugs.utils.sampler.PatchSampler is (num_patches / patch_size are its business and are kept here only for the signature).
    With l_lpips_w == 0 nothing is sampled, `lpips_patch_human` is still present (a zero: the reference runs LPIPS there and
    multiplies by 0), and forward performs no host synchronisation."""

    def __init__(self, l_ssim_w=0.2, l_l1_w=0.8, l_lpips_w=0.0, l_lbs_w=0.0, l_humansep_w=0.0, num_patches=4, patch_size=32,
                 use_patches=True, bg_color='white', *, lpips=None, patch_sampler=None):
        super().__init__()
        self.l_ssim_w, self.l_l1_w, self.l_lpips_w, self.l_lbs_w, self.l_humansep_w = l_ssim_w, l_l1_w, l_lpips_w, l_lbs_w, l_humansep_w
        self.num_patches, self.patch_size, self.use_patches, self.bg_color = num_patches, patch_size, use_patches, bg_color
        if l_lpips_w > 0.0 and lpips is None:
            raise ValueError("HumanSceneLoss: l_lpips_w > 0 needs `lpips`, a callable (pred, gt) -> per-patch distances")
        if l_lpips_w > 0.0 and patch_sampler is None:
            raise ValueError("HumanSceneLoss: l_lpips_w > 0 needs `patch_sampler`, an object with sample(mask, *images)")
        self.lpips, self.patch_sampler = lpips, patch_sampler

    def _lpips_of_patches(self, mask, pred_img, gt_img):
        _, pred_patches, gt_patches = self.patch_sampler.sample(mask, pred_img, gt_img)
        return self.lpips(pred_patches.clip(max=1), gt_patches).mean()

    def forward(self, data, render_pkg, human_gs_out, render_mode, human_gs_init_values=None, bg_color=None, human_bg_color=None):
        if render_mode not in ("human", "scene", "human_scene"):
            raise NotImplementedError
        if bg_color is not None:
            self.bg_color = bg_color
        if human_bg_color is None:
            human_bg_color = self.bg_color
        gt, mask2d, pred = data['rgb'], data['mask'], render_pkg['render']
        mask = mask2d.unsqueeze(0)
        loss_dict = {}
        if render_mode == "human":
            make_gt = lambda: gt * mask + human_bg_color[:, None, None] * (1. - mask)
        elif render_mode == "scene":
            make_gt = lambda: gt * (1. - mask)
        else:
            make_gt = lambda: gt
        extras_dict = _Extras(make_gt, pred_img=pred)

        if self.l_l1_w > 0.0 or self.l_ssim_w > 0.0:
            if render_mode == "human_scene":
                Ll1, s = l1_ssim(pred, gt)
                loss_ssim = 1.0 - s
            else:
                Ll1, loss_ssim = masked_l1_ssim(pred, gt, mask2d, render_mode, human_bg_color if render_mode == "human" else None)
            if self.l_l1_w > 0.0:
                loss_dict['l1'] = self.l_l1_w * Ll1
            if self.l_ssim_w > 0.0:
                loss_dict['ssim'] = self.l_ssim_w * loss_ssim

        if self.l_lpips_w > 0.0 and render_mode != "scene":
            if self.use_patches:
                if render_mode == "human":
                    noise = torch.rand_like(pred)
                    inv = 1. - mask
                    loss_lpips = self._lpips_of_patches(mask, pred * mask + noise * inv, extras_dict['gt_img'] * mask + noise * inv)
                else:
                    loss_lpips = self._lpips_of_patches(mask, pred, gt)
                loss_dict['lpips_patch'] = self.l_lpips_w * loss_lpips
            else:
                bbox = data['bbox'].to(int)
                crop = lambda img: img[:, bbox[0]:bbox[2], bbox[1]:bbox[3]]
                loss_dict['lpips'] = self.l_lpips_w * self.lpips(crop(pred).clip(max=1), crop(extras_dict['gt_img'])).mean()

        if self.l_humansep_w > 0.0 and render_mode == "human_scene":
            human_img = render_pkg['human_img']
            Ll1_human, loss_ssim_human = masked_l1_ssim(human_img, gt, mask2d, "human", human_bg_color)
            loss_dict['l1_human'] = self.l_l1_w * Ll1_human * self.l_humansep_w
            loss_dict['ssim_human'] = self.l_ssim_w * loss_ssim_human * self.l_humansep_w
            if self.l_lpips_w > 0.0:
                noise = torch.rand_like(human_img)
                inv = 1. - mask
                gt_human = gt * mask + human_bg_color[:, None, None] * inv
                loss_lpips_human = self._lpips_of_patches(mask, human_img * mask + noise * inv, gt_human * mask + noise * inv)
                loss_dict['lpips_patch_human'] = self.l_lpips_w * loss_lpips_human * self.l_humansep_w
            else:
                loss_dict['lpips_patch_human'] = torch.zeros((), dtype=human_img.dtype, device=human_img.device)

        if self.l_lbs_w > 0.0 and human_gs_out['lbs_weights'] is not None and render_mode != "scene":
            if 'gt_lbs_weights' in human_gs_out.keys():
                target = human_gs_out['gt_lbs_weights'].detach()
            else:
                target = human_gs_init_values['lbs_weights']
            loss_dict['lbs'] = self.l_lbs_w * F.mse_loss(human_gs_out['lbs_weights'], target).mean()

        loss = 0.0
        for v in loss_dict.values():
            loss += v
        return loss, loss_dict, extras_dict
