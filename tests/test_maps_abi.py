"""The alpha / depth map passes at the C boundary, without a GPU: the header's symbols are exported, the three entry points reject bad
arguments on the host before any launch, and the reference the GPU tests use (tests/maps_ref.py) is itself held to fp64."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from maps_ref import GEOMETRY_KEYS, map_upstreams, maps_reference
from scenes import CASES, make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import diff_gaussian_rasterization as dgr
    return dgr, dgr._load()   # with the prototypes the binding calls through (diff_gaussian_rasterization/_abi.py)


def test_every_function_the_header_declares_is_exported():
    _, lib = _lib()
    text = open(os.path.join(ROOT, "include", "hgs_rasterizer.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(hgs_\w+)\s*\(", text, flags=re.M)
    assert len(names) >= 50 and {"hgs_maps_forward", "hgs_maps_backward", "hgs_maps_finish", "hgs_rasterize_forward"} <= set(names)
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"declared in the header, not exported by the library: {missing}"


def _frame_args(dgr, lib, P=4, H=32, W=48, N=10):
    """A backward argument block that passes every host check -- its pointers are small fake addresses: nothing may be launched."""
    bw = dgr._BackwardArgs()
    f, s = bw.fwd, bw.state
    f.s.image_height, f.s.image_width, f.s.tanfovx, f.s.tanfovy, f.s.scale_modifier = H, W, 0.5, 0.5, 1.0
    f.s.bg = f.s.viewmatrix = f.s.projmatrix = f.s.campos = 256
    f.P, f.means3D, f.colors_precomp, f.opacities, f.cov3D_precomp = P, 256, 256, 256, 256
    s.geom, s.image, s.binning = 256, 256, 256
    s.geom_bytes, s.image_bytes, s.binning_bytes = lib.hgs_geom_bytes(P, H, W), lib.hgs_image_bytes(H, W), lib.hgs_binning_bytes(N, H, W)
    s.num_rendered = s.binning_capacity = N
    bw.grad_accum, bw.dL_dmeans3D = 256, 256
    return bw


def _calls(lib, bw):
    return (("forward", lambda: lib.hgs_maps_forward(C.byref(bw.fwd), C.byref(bw.state), 256, 256, None)),
            ("backward", lambda: lib.hgs_maps_backward(C.byref(bw), 256, 256, None)),
            ("finish", lambda: lib.hgs_maps_finish(C.byref(bw), None)))


def test_map_passes_reject_bad_arguments_through_the_c_abi():
    """The entry points' own checks (they return before any launch)."""
    dgr, lib = _lib()
    err = lambda: lib.hgs_last_error()
    # null pointers
    bw = _frame_args(dgr, lib)
    assert lib.hgs_maps_forward(None, C.byref(bw.state), 256, 256, None) == -1 and b"null argument" in err()
    assert lib.hgs_maps_forward(C.byref(bw.fwd), None, 256, 256, None) == -1 and b"null argument" in err()
    assert lib.hgs_maps_backward(None, 256, 256, None) == -1 and b"null argument" in err()
    assert lib.hgs_maps_finish(None, None) == -1 and b"null argument" in err()
    # a state that no forward filled in
    bw = _frame_args(dgr, lib)
    bw.state.image = None
    for what, call in _calls(lib, bw):
        assert call() == -1 and b"forward state is missing" in err(), what
    # a deferred frame nobody polled
    bw = _frame_args(dgr, lib)
    bw.state.num_rendered = -1
    for what, call in _calls(lib, bw):
        assert call() == -1 and b"hgs_forward_poll has not resolved" in err(), what
    # the arguments name another image size than the frame's, either way round
    for H, W in ((64, 48), (32, 96), (16, 16)):
        bw = _frame_args(dgr, lib)
        bw.fwd.s.image_height, bw.fwd.s.image_width = H, W
        for what, call in _calls(lib, bw):
            assert call() == -1 and b"wrong size" in err() and f"{H} x {W}".encode() in err(), (what, H, W)
    # ... or more Gaussians, or a larger binning buffer, than the state holds
    bw = _frame_args(dgr, lib)
    bw.fwd.P = 100_000
    for what, call in _calls(lib, bw):
        assert call() == -1 and b"wrong size" in err(), what
    bw = _frame_args(dgr, lib)
    bw.state.binning_capacity = 1 << 20
    for what, call in _calls(lib, bw):
        assert call() == -1 and b"wrong size" in err(), what
    # the forward's own argument checks come first
    bw = _frame_args(dgr, lib)
    bw.fwd.s.image_height = 0
    for what, call in _calls(lib, bw):
        assert call() == -1 and b"image size must be positive" in err(), what
    # the gradient buffers
    bw = _frame_args(dgr, lib)
    bw.grad_accum = None
    assert lib.hgs_maps_backward(C.byref(bw), 256, 256, None) == -1 and b"grad_accum" in err()
    assert lib.hgs_maps_finish(C.byref(bw), None) == -1 and b"grad_accum" in err()
    bw = _frame_args(dgr, lib)
    bw.dL_dmeans3D = None
    assert lib.hgs_maps_finish(C.byref(bw), None) == -1 and b"dL_dmeans3D" in err()
    # nothing to do: no Gaussians (whatever the state holds), no map asked for, no upstream gradient
    bw = _frame_args(dgr, lib)
    bw.fwd.P = 0
    bw.state.image = None
    for what, call in _calls(lib, bw):
        assert call() == 0, what
    bw = _frame_args(dgr, lib)
    assert lib.hgs_maps_forward(C.byref(bw.fwd), C.byref(bw.state), None, None, None) == 0
    assert lib.hgs_maps_backward(C.byref(bw), None, None, None) == 0


def test_the_binding_declares_the_flag_everywhere():
    import inspect
    import diff_gaussian_rasterization as dgr
    from hugs_amd.renderer import gs_renderer
    for fn in (dgr.rasterize_gaussians, dgr.GaussianRasterizer.forward, gs_renderer.render, gs_renderer.render_human_scene):
        assert inspect.signature(fn).parameters["return_alpha_depth"].default is False, fn


@pytest.mark.parametrize("name", ["basic_d3", "deg1_ragged"])
def test_the_maps_reference_holds_against_fp64(name):
    """tests/maps_ref.py in fp32 (what the GPU tests compare with) against the same construction in fp64.  The GPU's bars are 1e-4 per
    pixel (on the z_max scale) and 1e-3 relative L2 per gradient tensor; the reference may use up a tenth of either.  Its alpha channel
    is 1 - final_T up to the rounding of a sum of at most a few hundred fp32 terms below 1: 1e-6."""
    sc = make_scene(**CASES[name])
    gA, gD = map_upstreams(sc["H"], sc["W"])
    r32, r64 = maps_reference(sc, gA, gD), maps_reference(sc, gA, gD, dtype=np.float64)
    assert r32["alpha"].dtype == np.float32 and r64["alpha"].dtype == np.float64
    assert (r32["fwd"]["radii"] > 0).sum() > 100 and r32["alpha"].max() > 0.9 and r32["depth"].max() > 1.0
    assert np.abs(r32["alpha"] - (1.0 - r32["fwd"]["final_T"])).max() <= 1e-6
    assert np.array_equal(r32["fwd"]["n_contrib"], r64["fwd"]["n_contrib"])
    zm = r64["z_max"]
    assert abs(r32["z_max"] - zm) <= 1e-6 * zm
    # (a contributor whose alpha lies within rounding of 1/255 may be taken in one precision and not in the other: the threshold's own
    #  semantics, which the project's image bar allows on two pixels, each within 2/255; every other pixel is held to a tenth of 1e-4)
    for what, d in (("alpha", np.abs(r32["alpha"] - r64["alpha"])), ("depth / z_max", np.abs(r32["depth"] - r64["depth"]) / zm)):
        print(f"{name}: {what} fp32 against fp64: max {d.max():.2e}, {int((d > 1e-5).sum())} pixels beyond 1e-5")
        assert (d > 1e-5).sum() <= 2 and d.max() <= 2.0 / 255.0, what
    for k in GEOMETRY_KEYS:
        a, b = r32["grads"][k].astype(np.float64), r64["grads"][k]
        rel = np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)
        print(f"{name}: grad {k} fp32 against fp64 {rel:.2e}")
        if k == "cov3D":
            continue   # (scales + rotations scenes: not an input)
        assert np.linalg.norm(b) > 0 and rel <= 1e-4, (k, rel)


def test_the_depth_term_of_means3D_is_the_derivative_of_the_depth_map():
    """The one term tests/maps_ref.py adds by hand, checked against a central difference of the fp64 depth map along a random
    direction of means3D (one large splat: no threshold in reach of the step)."""
    sc = make_scene(**CASES["single"])
    H, W = sc["H"], sc["W"]
    gA, gD = map_upstreams(H, W)
    ref = maps_reference(sc, gA, gD, dtype=np.float64)
    assert ref["alpha"].max() > 0.1
    d = np.random.default_rng(5).standard_normal(sc["means3D"].shape)
    loss = lambda r: float((r["alpha"] * gA).sum() + (r["depth"] * gD).sum())
    h = 1e-6
    lp, lm = (loss(maps_reference(dict(sc, means3D=sc["means3D"].astype(np.float64) + s * h * d), dtype=np.float64)) for s in (1, -1))
    fd, an = (lp - lm) / (2 * h), float((ref["grads"]["means3D"] * d).sum())
    assert abs(fd - an) <= 1e-5 * max(abs(an), 1e-3), (fd, an)
