"""Row f-11 inside a training loop: the scene fit of tests/test_psnr_parity.py in miniature (gs_trainer.py:218-391: the reference's loss,
Adam with one group per tensor and the reference's learning rates, densification statistics every step, ONE opacity reset and ONE
clone / split / prune round on the way -- both go through the optimizer surgery of tests/test_hugs_loop.py's GaussianSet), run from the
same seed once per optimizer class: `torch.optim.Adam` twice, `hugs_amd.optim.Adam` once.  Only `_make_opt` differs.

The runs differ among themselves whatever the optimizer (the rasterizer's float atomics land in another order, Adam amplifies it), so
the bars are the project's own: both fits improve, the final PSNRs agree within 0.1 dB (tests/test_psnr_parity.py's criterion; HIP runs
of one fit spread by 0.007-0.011 dB there), and the Gaussian counts after the densification round differ by no more than the two
torch.optim.Adam runs differ from each other."""
import numpy as np
import pytest
import torch

import test_hugs_loop as loop
from hugs_amd import metrics, synthetic as syn

pytestmark = pytest.mark.gpu

H = W = 128
P_MODEL, P_TARGET, DEGREE = 3000, 12_000, 3
STEPS, RESET_AT, DENSIFY_AT = 120, 40, 80
LR = {"xyz": 1.6e-4 * 5.0, "features_dc": 2.5e-3, "features_rest": 2.5e-3 / 20.0, "opacity": 5e-2, "scaling": 5e-3, "rotation": 1e-3}   # hugs_scene.yaml:104-110


class HipAdamGaussianSet(loop.GaussianSet):
    """tests/test_hugs_loop.py's model with the one line of scene.py:213 changed"""

    def _make_opt(self, moments):
        from hugs_amd.optim import Adam
        self.opt = Adam([{"params": [self.p[k]], "lr": loop.LR[k], "name": k} for k in loop.LR], lr=0.0, eps=1e-15)
        for k, (m, v, step) in moments.items():
            self.opt.state[self.p[k]] = {"step": step, "exp_avg": m, "exp_avg_sq": v}


def _render(act, data, bg):
    from hugs_amd.renderer.gs_renderer import render
    return render(means3D=act["xyz"], feats=act["shs"], opacity=act["opacity"], scales=act["scales"], rotations=act["rotq"], data=data,
                  bg_color=bg, active_sh_degree=DEGREE)


def _fit(cls, init, target, data, device):
    """-> (PSNR before, PSNR after, Gaussians after the densification round, the optimizer's class)"""
    from hugs_amd.densify import update_densification_stats
    from hugs_amd.losses import l1_loss, ssim
    gs = cls({k: torch.from_numpy(v.copy()).to(device) for k, v in init.items()}, DEGREE)
    gs.noise_gen = torch.Generator(device="cpu").manual_seed(4)    # the same split noise in every fit
    bg = torch.ones(3, device=device)
    psnr = lambda: float(metrics.psnr(_render(gs.activated(), data, bg)["render"][None], target[None]).mean())
    with torch.no_grad():
        before = psnr()
    n_densified = None
    for step in range(STEPS):
        gs.opt.zero_grad(set_to_none=True)
        pkg = _render(gs.activated(), data, bg)
        (0.8 * l1_loss(pkg["render"], target) + 0.2 * (1.0 - ssim(pkg["render"], target))).backward()
        with torch.no_grad():
            update_densification_stats(gs.max_radii2D, gs.grad_accum, gs.denom, pkg["viewspace_points"], pkg["visibility_filter"], pkg["radii"])
        gs.opt.step()
        if step + 1 == DENSIFY_AT:
            gs.densify_and_prune(0.0002, 0.005, extent=5.0, max_screen_size=None)
            n_densified = int(gs.p["xyz"].shape[0])
        if step + 1 == RESET_AT:     # scene.py reset_opacity: opacities capped at 0.01, Adam's moments of the group restart
            with torch.no_grad():
                capped = torch.minimum(gs.p["opacity"], torch.full_like(gs.p["opacity"], float(np.log(0.01 / 0.99))))
            gs._rebuild(lambda k, t, is_moment: (torch.zeros_like(t) if is_moment else capped) if k == "opacity" else t)
    assert all(torch.isfinite(v).all() for v in gs.p.values())
    with torch.no_grad():
        after = psnr()
    return before, after, n_densified, type(gs.opt)


@pytest.fixture(scope="module")
def fits(device):
    cam = syn.pinhole_camera(H, W)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    t = lambda a: torch.from_numpy(f32(a)).to(device)
    tgt = syn.scene_gaussians(P_TARGET, cam, seed=77, sigma_px=1.2, ref_P=P_TARGET)
    g = syn.scene_gaussians(P_MODEL, cam, seed=78, sigma_px=3.0, ref_P=P_MODEL)
    r = np.random.default_rng(9)
    op = np.clip(g["opacities"], 0.02, 0.98)
    init = {"xyz": f32(g["means3D"]), "features_dc": f32(0.3 * r.standard_normal((P_MODEL, 1, 3))), "features_rest": np.zeros((P_MODEL, 15, 3), np.float32),
            "opacity": f32(np.log(op / (1 - op))).reshape(-1, 1), "scaling": f32(np.log(g["scales"])), "rotation": f32(g["rotations"])}
    data = {k: (t(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
    with torch.no_grad():
        target = _render({"xyz": t(tgt["means3D"]), "shs": t(tgt["shs"]), "opacity": t(tgt["opacities"]), "scales": t(tgt["scales"]),
                          "rotq": t(tgt["rotations"])}, data, torch.ones(3, device=device))["render"].clone()
    loop_lr, loop.LR = loop.LR, LR    # (GaussianSet rebuilds its optimiser from the module's table after every growth)
    try:
        out = {"torch": _fit(loop.GaussianSet, init, target, data, device), "torch again": _fit(loop.GaussianSet, init, target, data, device),
               "hip": _fit(HipAdamGaussianSet, init, target, data, device)}
    finally:
        loop.LR = loop_lr
    print("adam-loop (PSNR before, after, Gaussians after densification):", {k: v[:3] for k, v in out.items()})
    return out


def test_each_fit_ran_its_own_optimizer_through_the_surgery(fits):
    from hugs_amd.optim import Adam
    assert fits["torch"][3] is torch.optim.Adam and fits["torch again"][3] is torch.optim.Adam and fits["hip"][3] is Adam
    assert all(v[2] is not None and v[2] != P_MODEL for v in fits.values()), "the densification round did nothing"


def test_both_optimizers_improve_the_fit_and_end_within_a_tenth_of_a_db(fits):
    for name, (before, after, _, _) in fits.items():
        assert after > before, (name, before, after)
    assert abs(fits["hip"][1] - fits["torch"][1]) <= 0.1, fits


def test_the_densified_sets_differ_no_more_than_two_torch_runs_do(fits):
    assert abs(fits["hip"][2] - fits["torch"][2]) <= abs(fits["torch"][2] - fits["torch again"][2]), fits
