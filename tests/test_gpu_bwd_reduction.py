"""The backward's per-(tile, entry) cross-lane reduction (blend.hip, backward_entry / backward_read / backward_finish): nine
per-lane partial sums go through a wave-private LDS transpose (v0..v7) and a DPP chain (v8), and nine lanes -- the eight lane
groups' leaders and lane 63 -- add the totals into the Gaussian's [12] accumulator record.  Frames built to stress that lane
and slot mapping, through each backward form, against the oracle at the suite's bar."""
import numpy as np
import pytest

from oracle import hgs_oracle as ho
from scenes import make_scene, oracle_inputs
from test_gpu_parity import GRAD_REL_TOL, _stacked_scene, reload_switches, rel_l2, run_gpu, to_dev

pytestmark = pytest.mark.gpu

# the three forms a frame without deep tiles can take: one wave per tile, one wave per quad (both without checkpoints), and the
# library's own choice with checkpoints (the depth-segmented walk for a sparse frame)
FORMS = ["per_tile", "per_quad", "default"]

FRAMES = {
    # one tiny splat: the entry is taken by one lane of one quad
    "one_lane": lambda: make_scene(P=1, H=32, W=32, seed=20, D=3, with_culled=False, sigma_px=0.35),
    # a few big opaque-ish splats: entries taken by all 256 pixels of a tile
    "whole_tile": lambda: make_scene(P=3, H=48, W=48, seed=21, D=3, with_culled=False, sigma_px=60.0),
    # tiles cut by the right and bottom edges, lists of every length (odd ones end on a half-used pair)
    "ragged_edges": lambda: make_scene(P=401, H=75, W=101, seed=22, D=2),
    # one Gaussian in hundreds of tiles
    "one_in_many_tiles": lambda: make_scene(P=1, H=320, W=320, seed=23, D=3, with_culled=False, sigma_px=150.0),
    # a few Gaussians of every size: some lists of length 1, 2, 3, ...
    "short_lists": lambda: make_scene(P=7, H=64, W=80, seed=24, D=1, with_culled=False, sigma_px=9.0),
    # a stack: lists hundreds of entries deep, many segments per quad on the checkpointed path
    "deep_stack": lambda: _stacked_scene(1200, 64, 64, seed=25, spread_px=8.0),
}


def _set_form(form, monkeypatch):
    import diff_gaussian_rasterization as dgr
    ckpt = form == "default"
    monkeypatch.setattr(dgr, "_USE_CKPT", ckpt)
    if dgr._cpp is not None:
        dgr._cpp.use_checkpoints(ckpt)
    if form == "default":
        monkeypatch.delenv("HGS_BWD_WAVES_PER_TILE", raising=False)
    else:
        # (blend.hip, launch_blend_backward: 1 = blend_backward_kernel<4>, one wave per tile; 4 = blend_backward_kernel<1>, one wave per quad)
        monkeypatch.setenv("HGS_BWD_WAVES_PER_TILE", "1" if form == "per_tile" else "4")
    reload_switches(monkeypatch)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("frame", list(FRAMES))
def test_reduction_lane_and_slot_mapping_against_the_oracle(frame, form, device, monkeypatch):
    import diff_gaussian_rasterization as dgr
    sc = FRAMES[frame]()
    if "dL_dpix" not in sc:
        sc["dL_dpix"] = np.random.default_rng(7).standard_normal((3, sc["H"], sc["W"])).astype(np.float32)
    inp = oracle_inputs(sc)
    ref = ho.forward(inp)
    assert ref["N"] > 0
    refg = ho.backward(inp, ref, sc["dL_dpix"])
    _set_form(form, monkeypatch)
    try:
        t, color, _ = run_gpu(sc, device)
        color.backward(to_dev(sc["dL_dpix"], device))
    finally:
        if dgr._cpp is not None:
            dgr._cpp.use_checkpoints(True)
    keys = ["means3D", "means2D", "opacities", "shs", "scales", "rotations"]
    for k in keys:
        g = t[k].grad.cpu().numpy()
        assert np.isfinite(g).all(), f"{frame}/{form}: non-finite {k}"
        r = refg[k]
        err = rel_l2(g.reshape(r.shape), r)
        assert err <= GRAD_REL_TOL, f"{frame}/{form}: grad {k} rel L2 {err:.3e}"
    # every one of the nine slots a reduction writes is exercised: the colour (v6..v8) and geometry (v0..v5) sums of a
    # Gaussian that reaches a pixel are not all zero, and a lost or misrouted slot shows in these two
    vis = ref["radii"] > 0
    assert np.abs(refg["opacities"][vis]).sum() > 0 and np.abs(refg["shs"][vis]).sum() > 0
