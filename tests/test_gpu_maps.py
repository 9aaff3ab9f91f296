"""GPU: the rasterizer's alpha and depth maps (return_alpha_depth=True; csrc/maps.hip behind hgs_maps_forward / _backward / _finish)
against the C oracle's render of colours (z, 1, 0) on black (tests/maps_ref.py, itself held to fp64 by tests/test_maps_abi.py), and
against the library's own render of the same colours.

Bars: check_image of test_gpu_parity on alpha and on depth / z_max (the depth map is a colour render whose colours
are at most z_max, the largest depth of a visible Gaussian); gradients at most 1e-3 relative L2 per input tensor; radii and the colour
image bit-equal to the same call without the flag; two GPU forms of one arithmetic: 1e-6 on 99.98 % of pixels, gradients order_tol.
"""
import functools

import numpy as np
import pytest
import torch

from maps_ref import colour_reference, map_upstreams, maps_reference, summed
from scenes import CASES, make_scene
from test_gpu_parity import (COLOR_INLIER_FRAC, GRAD_REL_TOL, _force_ctypes_binding, check_image, gpu_settings, gpu_tensors, order_tol,
                             rel_l2, reload_switches, to_dev)

pytestmark = pytest.mark.gpu

# GPU tensor -> key of the oracle's gradient dict
GRAD_KEYS = (("means3D", "means3D"), ("means2D", "means2D"), ("opacities", "opacities"), ("shs", "shs"), ("colors_precomp", "colors"),
             ("scales", "scales"), ("rotations", "rotations"), ("cov3D_precomp", "cov3D"))

DEEP = {
    # lists of 2 381 .. 2 658 entries, last contributors up to position 2 527
    "deep_thin": (dict(P=3000, H=64, W=64, seed=21, D=0, sigma_px=12.0), 0.02),
    # every pixel reaches the transmittance stop, between positions 445 and 1 206 of lists of 2 425 .. 2 697 entries
    "deep_stop": (dict(P=3000, H=40, W=56, seed=24, D=0, sigma_px=12.0), 0.05),
}


@functools.lru_cache(maxsize=None)
def scene_of(name):
    if name in CASES:
        return make_scene(**CASES[name])
    kw, opacity = DEEP[name]
    sc = make_scene(**kw)
    sc["opacities"] = (opacity * np.random.default_rng(1).uniform(0.5, 1.5, sc["opacities"].shape)).astype(np.float32)
    return sc


@functools.lru_cache(maxsize=None)
def reference(name):
    """(scene, gA, gD, the oracle's maps with their gradients, the oracle's colour forward, its gradients): computed once, never changed"""
    sc = scene_of(name)
    gA, gD = map_upstreams(sc["H"], sc["W"])
    f, g = colour_reference(sc, sc["dL_dpix"])
    return sc, gA, gD, maps_reference(sc, gA, gD), f, g


def rasterize(sc, device, grad=True, **extra):
    from diff_gaussian_rasterization import GaussianRasterizer
    t = gpu_tensors(sc, device, grad)
    if not grad:
        t["means2D"] = t["means2D"].detach()
    out = GaussianRasterizer(gpu_settings(sc, device))(
        means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], shs=t["shs"], colors_precomp=t["colors_precomp"],
        scales=t["scales"], rotations=t["rotations"], cov3D_precomp=t["cov3D_precomp"], **extra)
    return t, out


def grads_of(t):
    return {k: v.grad.detach().cpu().numpy() for k, v in t.items() if v is not None and v.grad is not None}


def check_maps(alpha, depth, ref, what):
    H, W = ref["alpha"].shape
    assert alpha.shape == (1, H, W) and depth.shape == (1, H, W) and alpha.dtype == torch.float32 and depth.dtype == torch.float32
    a, d = alpha.detach().cpu().numpy()[0], depth.detach().cpu().numpy()[0]
    assert np.isfinite(a).all() and np.isfinite(d).all()
    print(f"{what}: alpha max |d| {np.abs(a - ref['alpha']).max():.2e}, depth / z_max max |d| {np.abs(d - ref['depth']).max() / ref['z_max']:.2e}")
    check_image(a, ref["alpha"], f"{what} alpha")
    check_image(d / ref["z_max"], ref["depth"] / ref["z_max"], f"{what} depth / z_max")


def check_grads(got, want, sc, what, tol=GRAD_REL_TOL, keys=GRAD_KEYS):
    for k, rk in keys:
        if sc.get(k) is None and k != "means2D":
            continue
        assert k in got, f"{what}: no gradient for {k}"
        g, r = got[k], want[rk]
        assert np.isfinite(g).all(), f"{what}: non-finite gradient in {k}"
        err = rel_l2(g.reshape(r.shape), r)
        print(f"{what}: grad {k} rel L2 {err:.2e}")
        assert err <= tol, f"{what}: grad {k} rel L2 err {err:.3e}"


def run_against_the_oracle(name, mode, device):
    sc, gA, gD, ref, cf, cg = reference(name)
    clamp = mode == "clamp"
    _, (color0, radii0) = rasterize(sc, device, clamp_output=clamp)
    t, (color, radii, alpha, depth) = rasterize(sc, device, clamp_output=clamp, return_alpha_depth=True)
    assert torch.equal(radii, radii0) and torch.equal(color, color0), "the flag changed the colour render"
    assert np.array_equal(radii.cpu().numpy(), ref["fwd"]["radii"])
    check_maps(alpha, depth, ref, f"{name} {mode}")
    tA, tD, dL = to_dev(gA, device), to_dev(gD, device), to_dev(sc["dL_dpix"], device)
    loss = (alpha[0] * tA).sum() + (depth[0] * tD).sum()
    if mode != "maps_only":
        loss = loss + (color * dL).sum()
    loss.backward()
    torch.cuda.synchronize()
    if mode == "maps_only":
        want = dict({k: np.zeros_like(v) for k, v in cg.items()}, **ref["grads"])   # (the colour inputs receive zeros)
    elif clamp:
        # torch.clamp's backward passes dL/dcolour where the unclamped value lies inside [0, 1]: the oracle's colour backward is given
        # the mask of the library's own unclamped image (bit-equal to what the clamped call blended: test_gpu_parity)
        _, (raw, _) = rasterize(sc, device)
        assert torch.equal(color, raw.clamp(0.0, 1.0))
        passes = ((raw >= 0.0) & (raw <= 1.0)).cpu().numpy()
        want = summed(ref["grads"], colour_reference(sc, sc["dL_dpix"] * passes)[1])
    else:
        want = summed(ref["grads"], cg)
    check_grads(grads_of(t), want, sc, f"{name} {mode}")
    assert float(t["means2D"].grad[:, 2].abs().max()) == 0.0


@pytest.mark.parametrize("mode", ["all", "maps_only", "clamp"])
@pytest.mark.parametrize("name", list(CASES))
def test_maps_and_gradients_against_the_oracle(name, mode, device):
    """Loss (color * dL).sum() + (alpha * gA).sum() + (depth * gD).sum(): the maps, and every gradient against the sum of the oracle's
    two backward passes; again with only the maps in the loss; again with clamp_output=True."""
    run_against_the_oracle(name, mode, device)


@pytest.mark.parametrize("name", list(DEEP))
def test_deep_lists_against_the_oracle(name, device):
    sc, _, _, ref, _, _ = reference(name)
    f = ref["fwd"]
    length = f["ranges"][:, 1].astype(np.int64) - f["ranges"][:, 0]
    nc = f["n_contrib"].astype(np.int64)
    gx = (sc["W"] + 15) // 16
    tile = (np.arange(sc["H"])[:, None] // 16) * gx + np.arange(sc["W"])[None, :] // 16
    if name == "deep_thin":
        assert (length.min(), length.max()) == (2381, 2658) and nc.max() == 2527 and nc.min() > 1600
    else:
        assert (length.min(), length.max()) == (2425, 2697) and (nc.min(), nc.max()) == (445, 1206)
        assert (nc < length[tile]).all() and f["final_T"].max() < 1.1e-4, "every pixel reaches the transmittance stop"
    run_against_the_oracle(name, "all", device)


_default_path = {}

FORCED = [("HGS_FRAME_KIND", "d"), ("HGS_FRAME_KIND", "s"), ("HGS_FUSED_SORT_BLEND", "0"), ("HGS_DEEP_FORWARD", "0"), ("HGS_BWD_SEGMENTED", "0")]


def _maps_run(name, device):
    sc, gA, gD, _, _, _ = reference(name)
    t, (color, radii, alpha, depth) = rasterize(sc, device, return_alpha_depth=True)
    ((color * to_dev(sc["dL_dpix"], device)).sum() + (alpha[0] * to_dev(gA, device)).sum() + (depth[0] * to_dev(gD, device)).sum()).backward()
    torch.cuda.synchronize()
    return color.detach(), alpha.detach(), depth.detach(), grads_of(t)


@pytest.mark.parametrize("switch", FORCED, ids=lambda s: f"{s[0]}={s[1]}")
@pytest.mark.parametrize("name", ["deep_thin", "basic_d3"])
def test_maps_do_not_depend_on_the_path_the_frame_took(name, switch, device, monkeypatch):
    """The map passes read the lists and walk them one way whatever kernels produced the frame: bit-equal maps under every forced
    path; the gradients move by the order of the colour backward's atomics only."""
    if name not in _default_path:
        _default_path[name] = _maps_run(name, device)
    _, alpha0, depth0, g0 = _default_path[name]
    monkeypatch.setenv(*switch)
    reload_switches(monkeypatch)
    _, alpha, depth, g = _maps_run(name, device)
    assert torch.equal(alpha, alpha0), f"alpha differs on {int((alpha != alpha0).sum())} pixels, max {float((alpha - alpha0).abs().max()):.2e}"
    assert torch.equal(depth, depth0), f"depth differs on {int((depth != depth0).sum())} pixels, max {float((depth - depth0).abs().max()):.2e}"
    for k in g0:
        err = rel_l2(g[k], g0[k])
        print(f"{name} {switch}: grad {k} against the default path {err:.2e}")
        assert err <= order_tol(k), (k, err)


def test_second_segment_against_the_oracle_on_the_concatenation(device):
    """300 + 500 Gaussians at 80 x 112 as two segments: every gradient lands in its own model's tensor, seg2's dL/dmeans3D -- which
    the finish pass writes through another pointer -- included."""
    from diff_gaussian_rasterization import GaussianRasterizer
    sc = make_scene(P=800, H=80, W=112, seed=31, D=2)
    cut = 300
    gA, gD = map_upstreams(sc["H"], sc["W"])
    ref = maps_reference(sc, gA, gD)
    want = summed(ref["grads"], colour_reference(sc, sc["dL_dpix"])[1])
    keys = ("means3D", "opacities", "shs", "scales", "rotations")
    a = {k: to_dev(sc[k][:cut], device, True) for k in keys}
    b = {k: to_dev(sc[k][cut:], device, True) for k in keys}
    means2D = torch.zeros(800, 3, device=device, requires_grad=True)
    color, radii, alpha, depth = GaussianRasterizer(gpu_settings(sc, device))(
        means3D=a["means3D"], means2D=means2D, opacities=a["opacities"], shs=a["shs"], scales=a["scales"], rotations=a["rotations"],
        second=b, return_alpha_depth=True)
    assert np.array_equal(radii.cpu().numpy(), ref["fwd"]["radii"]) and (ref["fwd"]["radii"][cut:] > 0).sum() > 100
    check_maps(alpha, depth, ref, "two segments")
    ((color * to_dev(sc["dL_dpix"], device)).sum() + (alpha[0] * to_dev(gA, device)).sum() + (depth[0] * to_dev(gD, device)).sum()).backward()
    torch.cuda.synchronize()
    assert rel_l2(means2D.grad.cpu().numpy(), want["means2D"]) <= GRAD_REL_TOL
    for k in keys:
        r = want[k]
        for part, sl in ((a, slice(0, cut)), (b, slice(cut, None))):
            g = part[k].grad.cpu().numpy()
            err = rel_l2(g.reshape(r[sl].shape), r[sl])
            print(f"two segments: grad {k} rows {sl} rel L2 {err:.2e}")
            assert np.linalg.norm(r[sl]) > 0 and err <= GRAD_REL_TOL, (k, sl, err)


def _own_render_of_z_1_0(sc, device, gA, gD):
    """What a user did before the flag: a second render with colours (z, 1, 0) on black, the z statement in torch."""
    from diff_gaussian_rasterization import GaussianRasterizer
    t = gpu_tensors(sc, device)
    V = to_dev(np.asarray(sc["cam"]["world_view_transform"], np.float32).reshape(4, 4), device)
    z = t["means3D"] @ V[:3, 2] + V[3, 2]
    cols = torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], 1)
    sc0 = dict(sc, bg=np.zeros(3, np.float32))
    img, _ = GaussianRasterizer(gpu_settings(sc0, device))(
        means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], colors_precomp=cols, scales=t["scales"],
        rotations=t["rotations"], cov3D_precomp=t["cov3D_precomp"])
    ((img[1] * to_dev(gA, device)).sum() + (img[0] * to_dev(gD, device)).sum()).backward()
    torch.cuda.synchronize()
    return img.detach(), grads_of(t)


@pytest.mark.parametrize("name,walk", [("basic_d3", "as it comes"), ("rotcam_d2", "as it comes"), ("deep_stop", "one wave"),
                                       ("deep_stop", "as it comes")])
def test_maps_equal_the_librarys_own_render_of_z_1_0(name, walk, device, monkeypatch):
    """Two GPU forms of one arithmetic: at most 1e-6 on at least 99.98 % of pixels, on the z_max scale;
    gradients within order_tol.  One arithmetic means one summation order: the map passes add a pixel's contributors front to back,
    as the colour walk of one wave per quad does.  The deep scene's lists are long, and by default the library blends long tiles
    split by depth -- partial sums per 32-entry segment, added afterwards.  So the deep scene is compared twice: with
    HGS_DEEP_FORWARD=0 (the colour render walks front to back too) under the bar above, and as it comes under the bound fp32 gives two
    orders of one sum: n terms, each partial sum at most 1 (alpha) or z_max (depth) and rounded to 2^-24 relative: n 2^-24 on the
    z_max scale, n = 1 206 the deepest last contributor -- 7.2e-5, every pixel."""
    sc, gA, gD, ref, _, _ = reference(name)
    if walk == "one wave":
        monkeypatch.setenv("HGS_DEEP_FORWARD", "0")
        reload_switches(monkeypatch)
    img, g_own = _own_render_of_z_1_0(sc, device, gA, gD)
    t, (_, _, alpha, depth) = rasterize(sc, device, return_alpha_depth=True)
    ((alpha[0] * to_dev(gA, device)).sum() + (depth[0] * to_dev(gD, device)).sum()).backward()
    torch.cuda.synchronize()
    two_orders = name == "deep_stop" and walk == "as it comes"
    for what, mine, own in (("alpha", alpha[0].detach(), img[1]), ("depth / z_max", depth[0].detach() / ref["z_max"], img[0] / ref["z_max"])):
        d = (mine - own).abs()
        frac = float((d <= 1e-6).float().mean())
        print(f"{name}, {walk}: {what} against the library's own render: max {float(d.max()):.2e}, {frac:.6f} within 1e-6")
        if two_orders:
            assert float(d.max()) <= int(ref["fwd"]["n_contrib"].max()) * 2.0 ** -24, (what, float(d.max()))
        else:
            assert frac >= COLOR_INLIER_FRAC, (what, frac)
    g = grads_of(t)
    for k in ("means3D", "means2D", "opacities", "scales", "rotations"):
        err = rel_l2(g[k], g_own[k])
        print(f"{name}, {walk}: grad {k} against the library's own render {err:.2e}")
        assert err <= order_tol(k), (k, err)


def test_both_bindings_give_the_same_maps(device, monkeypatch):
    import diff_gaussian_rasterization as dgr
    sc = scene_of("basic_d3")
    outs = []
    for binding in ("cpp", "ctypes"):
        if binding == "ctypes":
            _force_ctypes_binding(monkeypatch)
        elif dgr._load_cpp() is None:
            pytest.skip("the C++ binding is not built / not selected")
        _, out = rasterize(sc, device, return_alpha_depth=True)
        assert out[2].grad_fn is not None and type(out[2].grad_fn).__name__.startswith("_RasterizeGaussiansMaps")
        _, plain = rasterize(sc, device)
        assert torch.equal(plain[0], out[0]) and torch.equal(plain[1], out[1])
        outs.append(out)
    for x, y in zip(*outs):
        assert torch.equal(x, y)


GEOMETRY_GRAD_KEYS = tuple((k, rk) for k, rk in GRAD_KEYS if k not in ("shs", "colors_precomp"))


@functools.lru_cache(maxsize=None)
def normalised_depth_reference(name):
    """The oracle's gradients of (depth / alpha.clamp_min(1e-6)).sum(): the chain rule in fp64 on the oracle's own maps -- gD = 1 /
    max(alpha, 1e-6), gA = -depth / alpha^2 where alpha exceeds 1e-6 (the clamp passes no gradient below), else 0 -- and the oracle's
    backward under these upstreams.  (A pixel with a contributor has alpha >= 1/255: the upstreams stay below 255 and 255^2 z_max.)"""
    sc, _, _, ref, _, _ = reference(name)
    a, d = ref["alpha"].astype(np.float64), ref["depth"].astype(np.float64)
    live = a > 1e-6
    gD = 1.0 / np.maximum(a, 1e-6)
    gA = np.where(live, -d / np.where(live, a, 1.0) ** 2, 0.0)
    return maps_reference(sc, gA, gD)["grads"]


@pytest.mark.parametrize("name", ["basic_d3", "deep_stop"])
def test_the_callers_normalisation_against_the_oracle(name, device):
    """(depth / alpha.clamp_min(1e-6)).sum(), the expected depth a caller forms from the two maps: upstream gradients that depend on
    the maps themselves, every geometry gradient against the oracle's."""
    sc = scene_of(name)
    t, (_, _, alpha, depth) = rasterize(sc, device, return_alpha_depth=True)
    (depth / alpha.clamp_min(1e-6)).sum().backward()
    torch.cuda.synchronize()
    check_grads(grads_of(t), normalised_depth_reference(name), sc, f"{name}, depth / alpha", keys=GEOMETRY_GRAD_KEYS)
    for k in ("shs", "colors_precomp"):
        if t[k] is not None:
            assert float(t[k].grad.abs().max()) == 0.0, k


def test_visibility_filter_together_with_the_maps(device):
    """with_visibility=True and return_alpha_depth=True in one call: (colour, radii, filter, alpha, depth) -- backward finds the maps'
    gradients behind radii's AND the filter's None."""
    sc, gA, gD, ref, _, _ = reference("basic_d3")
    tA, tD, dL = to_dev(gA, device), to_dev(gD, device), to_dev(sc["dL_dpix"], device)
    grads = []
    for extra in (dict(), dict(with_visibility=True)):
        t, out = rasterize(sc, device, return_alpha_depth=True, **extra)
        assert len(out) == 4 + len(extra)
        color, radii, alpha, depth = out[0], out[1], out[-2], out[-1]
        ((color * dL).sum() + (alpha[0] * tA).sum() + (depth[0] * tD).sum()).backward()
        torch.cuda.synchronize()
        grads.append((out, grads_of(t)))
    (plain, g0), (five, g1) = grads
    color, radii, visible, alpha, depth = five
    assert visible.dtype == torch.bool and visible.shape == radii.shape and torch.equal(visible, radii > 0) and bool(visible.any())
    assert not visible.requires_grad and not radii.requires_grad and alpha.requires_grad and depth.requires_grad
    assert alpha.shape == (1, sc["H"], sc["W"]) and depth.shape == alpha.shape and color.shape == (3, sc["H"], sc["W"])
    for a, b in zip((color, radii, alpha, depth), plain):
        assert torch.equal(a, b)
    check_maps(alpha, depth, ref, "with the visibility filter")
    assert set(g0) == set(g1)
    for k in g0:
        err = rel_l2(g1[k], g0[k])
        print(f"with the visibility filter: grad {k} against the call without it {err:.2e}")
        assert err <= order_tol(k), (k, err)


def test_maps_without_a_graph_come_from_the_streams_arena(device):
    """Under torch.no_grad() and with inputs that ask for no gradient the frame's scratch is the stream's arena, which the next frame
    on the stream overwrites: the maps are bit-equal to the grad-enabled call's, and -- cloned before it -- still are after another
    frame has used the arena.  (Inputs that require a gradient keep the frame on scratch of its own under no_grad as well:
    ctx.needs_input_grad does not look at the grad mode; that call is held to the same.)"""
    import diff_gaussian_rasterization as dgr
    first, second = scene_of("basic_d3"), scene_of("rotcam_d2")
    assert (first["H"], first["W"], first["means3D"].shape[0]) != (second["H"], second["W"], second["means3D"].shape[0])
    want = {}
    for name, sc in (("first", first), ("second", second)):
        _, (color, radii, alpha, depth) = rasterize(sc, device, return_alpha_depth=True)
        assert alpha.grad_fn is not None
        want[name] = (color.detach().clone(), alpha.detach().clone(), depth.detach().clone())
    for grad in (False, True):
        with torch.no_grad():
            dgr._arenas.clear()
            _, (color, radii, alpha, depth) = rasterize(first, device, grad=grad, return_alpha_depth=True)
            assert alpha.grad_fn is None and not alpha.requires_grad
            assert len(dgr._arenas) == (0 if grad else 1), "the frame's scratch is not where this test says it is"
            kept = (color.clone(), alpha.clone(), depth.clone())
            _, (color2, _, alpha2, depth2) = rasterize(second, device, grad=grad, return_alpha_depth=True)
            torch.cuda.synchronize()
            assert len(dgr._arenas) == (0 if grad else 1)
        for what, got, ref in (("first", kept, want["first"]), ("second", (color2, alpha2, depth2), want["second"])):
            for k, a, b in zip(("colour", "alpha", "depth"), got, ref):
                assert torch.equal(a, b), f"{what}, inputs require grad: {grad}: {k} differs from the grad-enabled call's on {int((a != b).sum())} pixels"
    check_maps(kept[1], kept[2], reference("basic_d3")[3], "no_grad")


def test_render_returns_the_two_maps(device):
    from hugs_amd.renderer import gs_renderer
    from test_gpu_configs import cam_data
    sc, gA, gD, ref, _, _ = reference("basic_d3")
    t = gpu_tensors(sc, device)
    kw = dict(means3D=t["means3D"], feats=t["shs"], opacity=t["opacities"], scales=t["scales"], rotations=t["rotations"],
              data=cam_data(sc["cam"], device), bg_color=to_dev(sc["bg"], device), active_sh_degree=sc["D"])
    plain = gs_renderer.render(**kw)
    assert "alpha" not in plain and "depth" not in plain
    pkg = gs_renderer.render(**kw, return_alpha_depth=True)
    assert set(pkg) == set(plain) | {"alpha", "depth"}
    assert torch.equal(pkg["render"], plain["render"]) and torch.equal(pkg["radii"], plain["radii"])
    assert torch.equal(pkg["visibility_filter"], pkg["radii"] > 0)
    check_maps(pkg["alpha"], pkg["depth"], ref, "render()")
    (pkg["depth"] / pkg["alpha"].clamp_min(1e-6)).sum().backward()   # the caller's normalisation
    torch.cuda.synchronize()
    assert float(pkg["viewspace_points"].grad.abs().max()) > 0.0
    got = dict(grads_of(t), means2D=pkg["viewspace_points"].grad.detach().cpu().numpy())
    check_grads(got, normalised_depth_reference("basic_d3"), sc, "render(), depth / alpha", keys=GEOMETRY_GRAD_KEYS)


def test_render_human_scene_returns_the_main_renders_maps(device):
    from hugs_amd.renderer import gs_renderer
    from test_gpu_configs import cam_data
    sc = scene_of("basic_d3")
    cut = 120
    m = lambda sl: {"xyz": to_dev(sc["means3D"][sl], device, True), "shs": to_dev(sc["shs"][sl], device, True),
                    "opacity": to_dev(sc["opacities"][sl], device, True), "scales": to_dev(sc["scales"][sl], device, True),
                    "rotq": to_dev(sc["rotations"][sl], device, True), "active_sh_degree": sc["D"]}
    human, scene = m(slice(0, cut)), m(slice(cut, None))
    pkg = gs_renderer.render_human_scene(cam_data(sc["cam"], device), human, scene, to_dev(sc["bg"], device), render_human_separate=True,
                                         return_alpha_depth=True)
    ref = reference("basic_d3")[3]
    check_maps(pkg["alpha"], pkg["depth"], ref, "render_human_scene()")
    assert "human_img" in pkg and not [k for k in pkg if k.startswith("human_") and ("alpha" in k or "depth" in k)]
    (pkg["alpha"].sum() + pkg["depth"].sum() + pkg["render"].sum() + pkg["human_img"].sum()).backward()
    assert float(scene["xyz"].grad.abs().max()) > 0.0 and float(human["xyz"].grad.abs().max()) > 0.0


def test_no_gaussians_give_zero_maps(device):
    sc = make_scene(P=0, H=32, W=48, seed=0, with_culled=False)
    t, (color, radii, alpha, depth) = rasterize(sc, device, return_alpha_depth=True)
    assert alpha.shape == (1, 32, 48) and depth.shape == (1, 32, 48) and radii.shape == (0,)
    assert float(alpha.abs().max()) == 0.0 and float(depth.abs().max()) == 0.0 and float(color.abs().max()) == 0.0
    (alpha.sum() + depth.sum()).backward()
    assert t["means3D"].grad.shape == (0, 3)


def test_pixels_without_a_contributor_are_zero(device):
    """All Gaussians behind the camera: empty lists, both maps zero, zero gradients."""
    sc = make_scene(P=50, H=40, W=56, seed=3, with_culled=False)
    sc["means3D"][:, 2] = -1.0
    t, (color, radii, alpha, depth) = rasterize(sc, device, return_alpha_depth=True)
    assert int(radii.abs().sum()) == 0 and float(alpha.abs().max()) == 0.0 and float(depth.abs().max()) == 0.0
    (alpha.sum() + depth.sum()).backward()
    assert float(t["means3D"].grad.abs().max()) == 0.0


def test_only_one_map_in_the_loss(device):
    """Either upstream gradient may be missing (a NULL pointer at the C boundary)."""
    sc, gA, gD, ref, _, _ = reference("basic_d3")
    zero = np.zeros_like(gA)
    for what, wA, wD in (("alpha only", gA, zero), ("depth only", zero, gD)):
        t, (_, _, alpha, depth) = rasterize(sc, device, return_alpha_depth=True)
        ((alpha[0] * to_dev(gA, device)).sum() if what == "alpha only" else (depth[0] * to_dev(gD, device)).sum()).backward()
        torch.cuda.synchronize()
        want = maps_reference(sc, wA, wD)["grads"]
        got = grads_of(t)
        for k in ("means3D", "means2D", "opacities", "scales", "rotations"):
            err = rel_l2(got[k], want[k].reshape(got[k].shape))
            assert err <= GRAD_REL_TOL, (what, k, err)


def test_second_backward_through_a_retained_graph_repeats_the_first(device):
    sc, gA, gD, _, _, _ = reference("basic_d3")
    t, (color, radii, alpha, depth) = rasterize(sc, device, return_alpha_depth=True)
    loss = (color * to_dev(sc["dL_dpix"], device)).sum() + (alpha[0] * to_dev(gA, device)).sum() + (depth[0] * to_dev(gD, device)).sum()
    loss.backward(retain_graph=True)
    first = {k: v.grad.clone() for k, v in t.items() if v is not None and v.grad is not None}
    held = {k: v.grad for k, v in t.items() if v is not None and v.grad is not None}   # aliases of the first slab
    for v in t.values():
        if v is not None:
            v.grad = None
    loss.backward()
    torch.cuda.synchronize()
    for k, v in first.items():
        assert torch.equal(held[k], v), f"{k}: the first backward's gradient was overwritten"
        err = rel_l2(t[k].grad.cpu().numpy(), v.cpu().numpy())
        assert err <= order_tol(k), (k, err)
