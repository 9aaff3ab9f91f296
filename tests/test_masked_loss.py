"""Row f-5 with HumanSceneLoss's masks (/root/reference/hugs/losses/loss.py:46-162): `masked_l1_ssim` and `HumanSceneLoss` of
hugs_amd.losses over hgs_masked_loss_forward / hgs_masked_loss_backward.
CPU: a float64 restatement of the reference's two masked terms, composed from oracle.loss_oracle's ssim and grad (unchanged), against
values and autograd gradients of the reference's own module (tests/golden/make_golden_masked_loss.py compiles it from /root/reference
and runs it on CPU in fp32); the three entry points at the C boundary.
GPU: the fused kernels, through the function and the module, against the restatement and the golden vectors, on every case and mode.
Tolerances are tests/test_losses.py's: values 2e-5 * max(1, |value|), gradients 1e-4 of the largest entry (the reference's fp32 result
and the restatement differ by at most 1.5e-7 relative in value and 1.4e-7 of the largest gradient entry: two orders of margin)."""
import functools
import os

import numpy as np
import pytest
import torch

import layouts
from oracle import loss_oracle as lo

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_masked_loss.npz"))
CASES = ["c1", "c2", "c3", "c4", "c5"]   # 37x53 ragged | 40x132 float4, 3x3 tiles | 5x7 below the window | 37x53 soft mask | 40x132 mask of ones
MODES = ["human", "scene", "human_scene"]
VALUE_TOL, GRAD_TOL = 2e-5, 1e-4
W_L1, W_SSIM, W_LBS, W_SEP = 0.8, 0.2, 1000.0, 1.0   # make_golden_masked_loss.py's WEIGHTS


def inputs(case):
    h, w = (int(v) for v in G[f"{case}_shape"])
    return G[f"pred_{h}x{w}"], G[f"gt_{h}x{w}"], G[f"human_{h}x{w}"], G[f"{case}_mask"], G["bg"]


def restate(pred, gt, mask, mode, bg, w_l1=W_L1, w_ssim=W_SSIM):
    """-> (Ll1, loss_ssim, d(w_l1 Ll1 + w_ssim loss_ssim)/dpred) in float64: the reference's two pre-weight terms of one mode."""
    p, g, m = (np.asarray(a, np.float64) for a in (pred, gt, mask))
    if mode == "human":
        x, y, s = p, g * m + np.asarray(bg, np.float64)[:, None, None] * (1.0 - m), 1.0
    else:
        x, y, s = p * (1.0 - m), g * (1.0 - m), 1.0 - m
    H, W = m.shape
    area = m.sum()                                       # BOTH modes: the sum of the human mask (loss.py:78,91,103 invert it twice)
    with np.errstate(divide="ignore", invalid="ignore"):
        l1 = np.abs(x - y).sum() / area
        ssim_term = (1.0 - lo.ssim(x, y)) * area / (H * W)
        grad = s * lo.grad(x, y, g_ssim_mean=-w_ssim * area / (H * W), g_l1_sum=w_l1 / area)
    return float(l1), float(ssim_term), grad


@functools.lru_cache(maxsize=None)
def expected(case, mode):
    """what HumanSceneLoss.forward(...)[1] and the gradients hold for one case and mode with the golden weights, in float64
    (computed once, shared by every test; callers do not write into it)"""
    pred, gt, human, mask, bg = inputs(case)
    lbs = W_LBS * float(np.mean((G["lbs"].astype(np.float64) - G["lbs_gt"]) ** 2))
    if mode in ("human", "scene"):
        l1, st, grad = restate(pred, gt, mask, mode, bg)
        vals = {"l1": W_L1 * l1, "ssim": W_SSIM * st}
        if mode == "human":
            vals["lbs"] = lbs
        return vals, grad, None
    l1h, sth, grad_h = restate(human, gt, mask, "human", bg, W_L1 * W_SEP, W_SSIM * W_SEP)
    vals = {"l1": W_L1 * lo.l1_loss(pred, gt), "ssim": W_SSIM * (1.0 - lo.ssim(pred, gt)), "l1_human": W_L1 * l1h * W_SEP,
            "ssim_human": W_SSIM * sth * W_SEP, "lpips_patch_human": 0.0, "lbs": lbs}
    return vals, lo.grad(pred, gt, g_ssim_mean=-W_SSIM, g_l1_sum=W_L1 / pred.size), grad_h


def close(got, want):
    return abs(got - want) <= VALUE_TOL * max(1.0, abs(want))


def grad_close(got, want):
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want).max() <= GRAD_TOL * max(np.abs(want).max(), 1e-8)


# ---------------------------------------------------------------- CPU
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_reference_module(case, mode):
    vals, grad, grad_h = expected(case, mode)
    key = f"{case}_{mode}"
    assert sorted(vals) == list(G[f"{key}_keys"])
    for k, v in vals.items():
        assert close(v, float(G[f"{key}_{k}"])), (k, v, float(G[f"{key}_{k}"]))
    assert close(sum(vals.values()), float(G[f"{key}_loss"]))
    assert grad_close(grad, G[f"{key}_grad"])
    if grad_h is not None:
        assert grad_close(grad_h, G[f"{key}_grad_human"])


def test_the_cases_are_what_they_are_for():
    for case in ("c1", "c2", "c3"):
        m = inputs(case)[3]
        assert (m == 0.5).sum() == 1 and set(np.unique(m)) == {0.0, 0.5, 1.0}
    ys, xs = np.nonzero(inputs("c2")[3] == 1.0)
    assert ys.min() < 16 <= 32 <= ys.max() and xs.min() < 64 <= xs.max()          # the rectangle crosses tile seams both ways
    ys = np.nonzero(inputs("c1")[3] == 1.0)[0]
    assert ys.min() < 16 <= ys.max()
    m4 = inputs("c4")[3]
    assert m4.min() > 0.0 and m4.max() < 1.0 and (inputs("c5")[3] == 1.0).all()
    assert inputs("c1")[0].shape[2] % 4 and inputs("c2")[0].shape[2] % 4 == 0     # scalar path | float4 path


def _lib():
    import diff_gaussian_rasterization as dgr
    return dgr, dgr._load()   # with the prototypes the wrapper calls through (diff_gaussian_rasterization/_abi.py)


def test_the_entry_points_are_exported_and_size_their_workspace():
    dgr, lib = _lib()
    for name in ("hgs_masked_loss_workspace", "hgs_masked_loss_forward", "hgs_masked_loss_backward"):
        assert hasattr(lib, name), name
    assert lib.hgs_masked_loss_workspace(3, 40, 132) == 16 * 3 * 3 * 3           # one float4 per 64 x 16 tile and channel
    assert lib.hgs_masked_loss_workspace(3, 1080, 1920) == 16 * 3 * 68 * 30
    assert lib.hgs_masked_loss_workspace(0, 40, 132) == 0 and lib.hgs_masked_loss_workspace(3, 40, -1) == 0


def test_the_entry_points_reject_bad_arguments_through_the_c_abi():
    """The entry points' own checks (they return before any launch; the pointers are small fake addresses)."""
    _, lib = _lib()
    err = lambda: lib.hgs_last_error()
    P = 256
    fwd = lambda mode=1, C_=3, H=8, W=8, pred=P, gt=P, mask=P, bg=P, maps=P, ws=P, out=P: \
        lib.hgs_masked_loss_forward(mode, C_, H, W, pred, gt, mask, bg, maps, ws, out, None)
    bwd = lambda mode=1, C_=3, H=8, W=8, pred=P, gt=P, mask=P, bg=P, maps=P, terms=P, g_l1=P, g_ssim=P, grad=P: \
        lib.hgs_masked_loss_backward(mode, C_, H, W, pred, gt, mask, bg, maps, terms, g_l1, g_ssim, grad, None)
    for what, call in (("forward", fwd), ("backward", bwd)):
        tag = f"masked_loss_{what}".encode()
        for mode in (0, 3, -1):
            assert call(mode=mode) == -1 and tag in err() and b"unknown mode" in err(), (what, mode)
        for bad in (dict(C_=0), dict(H=0), dict(W=-4), dict(C_=65536)):
            assert call(**bad) == -1 and tag in err() and b"need 1 <= C <= 65535" in err(), (what, bad)
        for name in ("pred", "gt", "mask"):
            assert call(**{name: None}) == -1 and tag in err() and b"null pointer" in err(), (what, name)
        assert call(mode=1, bg=None) == -1 and tag in err() and b"human mode needs bg" in err(), what
    for name in ("ws", "out"):
        assert fwd(**{name: None}) == -1 and b"null pointer" in err(), name
    assert fwd(ws=P + 8) == -1 and b"16-byte aligned" in err()
    for name in ("terms", "grad"):
        assert bwd(**{name: None}) == -1 and b"null pointer" in err(), name
    assert bwd(maps=None) == -1 and b"needs forward's maps" in err()


def test_the_lazy_extras_build_gt_img_on_first_access_only():
    from hugs_amd.losses import _Extras
    calls = []
    e = _Extras(lambda: calls.append(1) or "composite", pred_img="render")
    assert e["pred_img"] == "render" and "gt_img" not in e and not calls
    assert e["gt_img"] == "composite" and e["gt_img"] == "composite" and calls == [1] and "gt_img" in e
    with pytest.raises(KeyError):
        e["other"]


def test_the_constructor_names_the_missing_lpips_argument():
    from hugs_amd.losses import HumanSceneLoss
    with pytest.raises(ValueError, match="`lpips`"):
        HumanSceneLoss(l_lpips_w=0.1, patch_sampler=object())
    with pytest.raises(ValueError, match="`patch_sampler`"):
        HumanSceneLoss(l_lpips_w=0.1, lpips=lambda a, b: a)
    HumanSceneLoss()                                     # (l_lpips_w == 0: neither is needed)


# ---------------------------------------------------------------- GPU
def _dev(a, device, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(device).requires_grad_(grad)


def _module(**kw):
    from hugs_amd.losses import HumanSceneLoss
    return HumanSceneLoss(**dict(dict(l_ssim_w=W_SSIM, l_l1_w=W_L1, l_lpips_w=0.0, l_lbs_w=W_LBS, l_humansep_w=W_SEP), **kw))


def _module_args(case, device):
    pred, gt, human, mask, bg = inputs(case)
    t = dict(pred=_dev(pred, device, True), human=_dev(human, device, True), lbs=_dev(G["lbs"], device, True), gt=_dev(gt, device),
             mask=_dev(mask, device), bg=_dev(bg, device), lbs_gt=_dev(G["lbs_gt"], device))
    args = ({"rgb": t["gt"], "mask": t["mask"]}, {"render": t["pred"], "human_img": t["human"]},
            {"lbs_weights": t["lbs"], "gt_lbs_weights": t["lbs_gt"]})
    return t, args


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES)
def test_hip_module_matches_the_restatement_and_the_reference_vectors(case, mode, device):
    t, args = _module_args(case, device)
    loss, loss_dict, extras = _module()(*args, mode, bg_color=t["bg"])
    loss.backward()
    vals, grad, grad_h = expected(case, mode)
    key = f"{case}_{mode}"
    assert sorted(loss_dict) == sorted(vals) == list(G[f"{key}_keys"])
    for k, v in loss_dict.items():
        print(f"{key} {k}: hip {v.item():.9g} restated {vals[k]:.9g} reference {float(G[f'{key}_{k}']):.9g}")
        assert close(v.item(), vals[k]) and close(v.item(), float(G[f"{key}_{k}"])), k
    assert close(loss.item(), float(G[f"{key}_loss"]))
    got = t["pred"].grad.cpu().numpy()
    print(f"{key} grad: max |hip - reference| {np.abs(got - G[f'{key}_grad']).max():.3e} of {np.abs(G[f'{key}_grad']).max():.3e}")
    assert grad_close(got, grad) and grad_close(got, G[f"{key}_grad"])
    if mode == "human_scene":
        got_h = t["human"].grad.cpu().numpy()
        assert grad_close(got_h, grad_h) and grad_close(got_h, G[f"{key}_grad_human"])
    else:
        assert t["human"].grad is None
    if mode != "scene":
        assert grad_close(t["lbs"].grad.cpu().numpy(), G[f"{key}_grad_lbs"])
    # extras: the render itself; gt_img only once somebody reads it
    assert extras["pred_img"] is t["pred"] and "gt_img" not in extras
    pred, gt, human, mask, bg = inputs(case)
    want_gt = {"human": gt * mask + bg[:, None, None] * (1.0 - mask), "scene": gt * (1.0 - mask), "human_scene": gt}[mode]
    assert np.abs(extras["gt_img"].cpu().numpy() - want_gt).max() <= 1e-6 and "gt_img" in extras


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["human", "scene"])
@pytest.mark.parametrize("case", CASES)
def test_hip_function_matches_the_restatement_and_the_reference_vectors(case, mode, device):
    from hugs_amd.losses import masked_l1_ssim
    pred, gt, human, mask, bg = inputs(case)
    tp = _dev(pred, device, True)
    l1, st = masked_l1_ssim(tp, _dev(gt, device), _dev(mask, device)[None], mode, _dev(bg, device))    # ([1,H,W] here, [H,W] in the module)
    assert l1._base is st._base and l1._base is not None                           # views of one device tensor
    saved = l1._base.grad_fn.saved_tensors
    assert sum(s is not None and s.numel() == pred.size for s in saved) == 2      # pred and gt: no composited image is kept
    assert sum(s is not None and s.numel() == 3 * pred.size for s in saved) == 1  # the three partial maps
    (W_L1 * l1 + W_SSIM * st).backward()
    want_l1, want_st, want_grad = restate(pred, gt, mask, mode, bg)
    key = f"{case}_{mode}"
    assert close(l1.item(), want_l1) and close(st.item(), want_st)
    assert close(W_L1 * l1.item(), float(G[f"{key}_l1"])) and close(W_SSIM * st.item(), float(G[f"{key}_ssim"]))
    assert grad_close(tp.grad.cpu().numpy(), want_grad) and grad_close(tp.grad.cpu().numpy(), G[f"{key}_grad"])


@pytest.mark.gpu
def test_hip_mask_of_ones_is_the_unmasked_loss(device):
    from hugs_amd import losses
    pred, gt, human, mask, bg = inputs("c5")
    tp, tg, tm = _dev(pred, device), _dev(gt, device), _dev(mask, device)
    l1, st = losses.masked_l1_ssim(tp, tg, tm, "human", _dev(bg, device))
    want_l1, want_st = losses.l1_loss(tp, tg, mask=tm).item(), 1.0 - losses.ssim(tp, tg).item()
    assert close(l1.item(), want_l1) and close(st.item(), want_st)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["all", "mask"])
@pytest.mark.parametrize("layout", ["odd_offset", "strided"])
@pytest.mark.parametrize("mode", ["human", "scene"])
def test_hip_views_equal_the_aligned_contiguous_call(mode, layout, which, device):
    """c2 (W % 4 == 0): the canonical call moves float4s; an odd storage offset breaks the 16-byte alignment of whichever planes carry
    it and sends those through the scalar loads (`mask`: the mask alone, so one loader of the pair goes each way); a strided slice of a
    wider tensor is gathered by the wrapper.  Same values, same gradients."""
    from hugs_amd.losses import masked_l1_ssim
    pred, gt, human, mask, bg = inputs("c2")
    tb = _dev(bg, device)

    def run(build_images, build_mask):
        leaf = _dev(pred, device, True)
        vp, vg, vm = build_images(layouts.fresh(leaf)), build_images(layouts.fresh(_dev(gt, device))), build_mask(layouts.fresh(_dev(mask, device)))
        l1, st = masked_l1_ssim(vp, vg, vm, mode, tb)
        (W_L1 * l1 + W_SSIM * st).backward()
        return (vp, vg, vm), l1.item(), st.item(), leaf.grad.cpu().numpy()

    same = lambda t: t
    build = lambda t: layouts.build(layout, t)
    (vp, vg, vm), l1, st, grad = run(build if which == "all" else same, build)
    assert layouts.has_layout(layout, vm) and (which == "mask" or (layouts.has_layout(layout, vp) and layouts.has_layout(layout, vg)))
    base, l1_0, st_0, grad_0 = run(same, same)
    assert all(layouts.has_layout("fresh", v) for v in base)
    assert close(l1, l1_0) and close(st, st_0) and grad_close(grad, grad_0)
    want_l1, want_st, want_grad = restate(pred, gt, mask, mode, bg)
    assert close(l1, want_l1) and close(st, want_st) and grad_close(grad, want_grad)


@pytest.mark.gpu
def test_hip_module_steps_without_a_host_synchronisation(device):
    module = _module()
    prepared = [(mode, _module_args("c2", device)) for mode in MODES]

    def step(mode, t, args):
        loss, _, _ = module(*args, mode, bg_color=t["bg"])
        loss.backward()
        return loss

    for mode, (t, args) in prepared:                     # warm-up: code objects, the allocator's blocks
        step(mode, t, args)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")              # from here on a host synchronisation raises
    try:
        losses_ = [step(mode, t, args) for mode, (t, args) in prepared]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for (mode, _), loss in zip(prepared, losses_):
        assert close(loss.item(), float(G[f"c2_{mode}_loss"])), mode


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["human", "scene"])
def test_hip_forward_only_keeps_no_maps_and_two_calls_are_bit_identical(mode, device):
    from hugs_amd.losses import masked_l1_ssim
    pred, gt, human, mask, bg = inputs("c2")
    tp, tg, tm, tb = _dev(pred, device, True), _dev(gt, device), _dev(mask, device), _dev(bg, device)
    a = masked_l1_ssim(tp, tg, tm, mode, tb)
    b = masked_l1_ssim(tp, tg, tm, mode, tb)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                     # the reduction order is fixed
    (a[0] + a[1]).backward()
    g1 = tp.grad.clone()
    tp.grad = None
    (b[0] + b[1]).backward()
    assert torch.equal(tp.grad, g1)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        c = masked_l1_ssim(tp, tg, tm, mode, tb)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < 3 * pred.size * 4          # (the three partial maps alone are that much)
    assert not c[0].requires_grad and not c[1].requires_grad
    assert torch.equal(c[0], a[0]) and torch.equal(c[1], a[1])


class _StubSampler:
    """hugs.utils.sampler.PatchSampler's interface with fixed corners: two p x p patches that straddle the edge of c2's mask rectangle
    (rows 10-34, columns 40-99), so that the composites differ inside them"""

    def __init__(self, p=16, corners=((4, 36), (24, 90))):
        self.p, self.corners = p, corners

    def sample(self, mask, *images):
        p = self.p
        return [torch.stack([t[..., y:y + p, x:x + p] for y, x in self.corners]) for t in (mask,) + images]


def _stub_lpips(a, b):
    return ((a - b) ** 2).mean((1, 2, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["human", "human_scene"])
def test_hip_module_lpips_branch_is_the_statements_written_out(mode, device):
    w = 0.1
    sampler = _StubSampler()
    module = _module(l_lpips_w=w, lpips=_stub_lpips, patch_sampler=sampler)
    t, args = _module_args("c2", device)
    torch.manual_seed(7)
    loss, loss_dict, _ = module(*args, mode, bg_color=t["bg"])
    loss.backward()
    assert t["pred"].grad is not None and torch.isfinite(t["pred"].grad).all()
    torch.manual_seed(7)
    pred, human, gt, mask, bg = t["pred"].detach(), t["human"].detach(), t["gt"], t["mask"][None], t["bg"]
    patches = lambda a, b: _stub_lpips(sampler.sample(mask, a, b)[1].clip(max=1), sampler.sample(mask, a, b)[2]).mean()
    if mode == "human":
        gt_c = gt * mask + bg[:, None, None] * (1. - mask)
        noise = torch.rand_like(pred)
        want = {"lpips_patch": w * patches(pred * mask + noise * (1. - mask), gt_c * mask + noise * (1. - mask))}
    else:
        gt_c = gt * mask + bg[:, None, None] * (1. - mask)
        want = {"lpips_patch": w * patches(pred, gt)}
        noise = torch.rand_like(human)
        want["lpips_patch_human"] = w * patches(human * mask + noise * (1. - mask), gt_c * mask + noise * (1. - mask)) * W_SEP
    for k, v in want.items():
        assert v.item() > 0 and abs(loss_dict[k].item() - v.item()) <= 1e-5, (k, loss_dict[k].item(), v.item())
    rest, _, _ = expected("c2", mode)
    for k, v in rest.items():
        if k not in want:
            assert close(loss_dict[k].item(), v), k


@pytest.mark.gpu
def test_hip_empty_mask_divides_by_zero_on_the_device_and_raises_nothing(device):
    """sum(m) == 0: Ll1 = sum |x - y| / 0 is inf, as in the reference (loss_ssim = (1 - ssim) * 0 stays 0, as there); the total is not
    finite and neither call raises."""
    from hugs_amd.losses import masked_l1_ssim
    pred, gt, human, mask, bg = inputs("c1")
    for mode in ("human", "scene"):
        tp = _dev(pred, device, True)
        l1, st = masked_l1_ssim(tp, _dev(gt, device), torch.zeros(mask.shape, device=device), mode, _dev(bg, device))
        (l1 + st).backward()
        torch.cuda.synchronize()
        assert not np.isfinite(l1.item()) and st.item() == 0.0, mode
    t, args = _module_args("c1", device)
    args[0]["mask"] = torch.zeros_like(t["mask"])
    loss, _, _ = _module()(*args, "human", bg_color=t["bg"])
    loss.backward()
    assert not np.isfinite(loss.item())


@pytest.mark.gpu
def test_hip_masked_loss_refusals(device):
    from hugs_amd.losses import HumanSceneLoss, masked_l1_ssim
    a, m, bg = torch.rand(3, 8, 12, device=device), torch.rand(8, 12, device=device), torch.rand(3, device=device)
    for bad in ((a.double(), a, m, "human", bg), (a, a.double(), m, "human", bg), (a, a, m.double(), "scene", None), (a, a, m, "human", bg.double())):
        with pytest.raises(RuntimeError, match="float32"):
            masked_l1_ssim(*bad)
    with pytest.raises(ValueError, match="mode"):
        masked_l1_ssim(a, a, m, "human_scene", bg)
    for wrong in (m[:4], m.t(), m[None, None], a):
        with pytest.raises(ValueError, match="mask"):
            masked_l1_ssim(a, a, wrong, "scene")
    with pytest.raises(ValueError, match="bg"):
        masked_l1_ssim(a, a, m, "human")
    with pytest.raises(ValueError, match="bg"):
        masked_l1_ssim(a, a, m, "human", bg[:2])
    for bad in ((a, a.clone().requires_grad_(True), m, "human", bg), (a, a, m.clone().requires_grad_(True), "scene", None),
                (a, a, m, "human", bg.clone().requires_grad_(True))):
        with pytest.raises(NotImplementedError):
            masked_l1_ssim(*bad)
    with pytest.raises(RuntimeError, match="GPU"):
        masked_l1_ssim(a, a, m.cpu(), "scene")
    with pytest.raises(ValueError, match="`lpips`"):
        HumanSceneLoss(l_lpips_w=0.5, patch_sampler=_StubSampler())
    with pytest.raises(ValueError, match="`patch_sampler`"):
        HumanSceneLoss(l_lpips_w=0.5, lpips=_stub_lpips)
