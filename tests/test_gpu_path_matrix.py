"""Every rasterizer path the frame rule or a switch can select, against the oracle and against the default path.

The scan kernel decides a frame's kind, its long-list threshold, whether long tiles are blended split by depth and which tiles
leave checkpoints (binning.hip, frame_is_sparse and tile_scan_body); the host picks the binning order, emit-scan folding, fused or
stand-alone sort + forward, the backward form and the per-Gaussian backward's SH staging.  tools/shape_scan.py times the default
against every forced alternative (its VARIANTS, imported here so that a variant added there is covered at once); this module
checks what those alternatives COMPUTE, on frames that between them drive every variant off the default's path:

  * every (frame, variant) cell: three frames forward + backward through the drop-in API (image bit for bit, gradients within
    1e-4 of each other), the lists and the path from _debug_forward_state, and against the oracle: radii, N, sorted list and
    tile ranges exact, colour and final_T within check_image, n_contrib at test_gpu_parity.py's bar, every leaf gradient within
    GRAD_REL_TOL; against the default variant on the same frame at the bar of the variant's class (CLASS below);
  * a reachability guard per variant: it must change the path -- the scan's decisions or the host's launch forms
    (hgs_debug_stat "last_forward_forms" / "last_backward_forms") -- on at least one frame of the matrix;
  * SH stored as [P, M, 3] with M != 16 (K1 and K8 then take per-thread rows), through both bindings, with K8's cooperative
    loads asked for, and as the second segment of a joint call, against the oracle.

Not here: the sparse frame that leaves no checkpoints (>= 7 168 non-empty tiles, binning.hip NO_CKPT_MIN_TILES) --
tests/test_gpu_shapes.py covers it (trained_2097152_at_1080p), and its oracle run is too heavy for a matrix of this size."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from oracle import hgs_oracle as ho
from scenes import make_scene, oracle_inputs
from test_gpu_parity import (ALT_BACKWARD_TOL, COLOR_INLIER_FRAC, COLOR_TOL, GRAD_REL_TOL, _force_ctypes_binding, _stacked_scene,
                             check_image, gpu_settings, order_tol, rel_l2, reload_switches, run_gpu, to_dev)

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import shape_scan  # noqa: E402

# the library switches the scan does not force: name -> (environment, leave checkpoints?)
EXTRA_VARIANTS = {
    "k8_coop_per_thread": ({"HGS_K8_COOP": "0"}, True),
    "k8_coop_load_and_store": ({"HGS_K8_COOP": "3"}, True),
    "k1_stage_sh": ({"HGS_K1_STAGE_SH": "1"}, True),
    "no_bwd_segmented": ({"HGS_BWD_SEGMENTED": "0"}, True),
}
VARIANTS = dict(shape_scan.VARIANTS, **EXTRA_VARIANTS)
SWITCH_NAMES = sorted({k for env, _ in VARIANTS.values() for k in env})

# What a variant may change against the default on the same frame, and so the bar it is held to:
#   "order":   the same arithmetic in another launch or binning order -- image bit-equal, gradients within order_tol(k)
#   "backward": another backward form or other checkpoints -- image bit-equal, gradients within ALT_BACKWARD_TOL
#   "split":   how long tiles' forward is split by depth (frame kind, long thresholds, deep forward, deep_min) -- images within
#              1e-6 on >= 99.98 % of pixels and n_contrib equal there (test_depth_parallel_forward_equals_the_one_wave_forward),
#              gradients within ALT_BACKWARD_TOL
CLASS = {
    "default": None,
    # hgs_api.hip, bin_mode: both LDS binning paths emit the same (tile, depth) keys; the tile sort orders them
    "bin_by_cell": "order",
    "bin_in_order": "order",
    # binning.hip, frame_is_sparse(force_kind): the kind sets the long-list threshold and the deep workers (n_total[4], [8])
    "kind_sparse": "split",
    "kind_dense": "split",
    "kind_sparse_no_ckpt": "split",
    "kind_dense_no_ckpt": "split",
    # binning.hip, tile_scan_body: long_min_sparse / long_min_dense pick which tiles the deep workers blend split by depth
    "long_sparse_256": "split",
    "long_sparse_1024": "split",
    "long_sparse_2048": "split",
    "long_dense_768": "split",
    "long_dense_2048": "split",
    # hgs_api.hip want_ckpt: no checkpoints, the backward walks every tile from the front (blend.hip, launch_blend_backward)
    "no_ckpt": "backward",
    # blend.hip, launch_blend_backward: HGS_BWD_WAVES_PER_TILE=1 -> blend_backward_kernel<4> (a wave per tile), 4 -> <1> (a wave per quad)
    "bwd_wave_per_tile": "backward",
    "bwd_wave_per_quad": "backward",
    # blend.hip: the mixed kernel runs blend_backward_slot and blend_backward_wave<4> -- the two launches run the same two walks
    "bwd_two_launches": "order",
    # blend.hip, blend_forward_kernel: the same blend_fwd.h walks and deep workers as the fused kernel of binning.hip
    "unfused_sort_blend": "order",
    # binning.hip, emit_scan_kernel: the stand-alone scan's ranges and counters, computed inside emit
    "no_emit_scan": "order",
    # blend_fwd.h: HGS_DEEP_FORWARD=0 blends long tiles one wave per quad, not split by depth
    "no_deep_forward": "split",
    "long_sparse_256_no_deep": "split",
    "long_sparse_512": "split",
    "long_sparse_512_no_deep": "split",
    "long_sparse_1024_no_deep": "split",
    "long_sparse_2048_no_deep": "split",
    # binning.hip, n_total[8] = max(threshold, deep_min): long tiles up to deep_min entries are blended one wave per quad
    "deep_min_1536": "split",
    "deep_min_2048": "split",
    "deep_min_3072": "split",
    "long_dense_512": "split",
    "long_dense_768_no_deep": "split",
    "long_dense_1024": "split",
    # hgs_api.hip big_per_group: where the big splats sit in the binning order
    "big_spread": "order",
    # preprocess.hip, preprocess_backward_kernel coop_mode: the same rows, from LDS or per thread
    "k8_coop_per_thread": "order",
    "k8_coop_load_and_store": "order",
    # preprocess.hip, preprocess_kernel<MODE, true>: the same SH rows through LDS, the same summation order
    "k1_stage_sh": "order",
    # hgs_api.hip want_ckpt (the library's own switch): no checkpoints
    "no_bwd_segmented": "backward",
}
GRAD_KEYS = [("means3D", "means3D"), ("means2D", "means2D"), ("opacities", "opacities"), ("shs", "shs"), ("colors_precomp", "colors"),
             ("scales", "scales"), ("rotations", "rotations"), ("cov3D_precomp", "cov3D")]


def _add(sc, g):
    for k in ("means3D", "scales", "rotations", "opacities", "shs"):
        sc[k] = np.concatenate([sc[k], np.asarray(g[k], np.float32).reshape((-1,) + sc[k].shape[1:])], 0)
    return sc


def _from_frame(kind, H, W, P, D, seed):
    import test_gpu_shapes
    cam, g = test_gpu_shapes._frame(kind, H, W, P)
    rng = np.random.default_rng(seed)
    return dict(means3D=g["means3D"], opacities=g["opacities"], shs=g["shs"], scales=g["scales"], rotations=g["rotations"], colors_precomp=None,
                cov3D_precomp=None, cam=cam, H=H, W=W, D=D, M=16, bg=np.array([0.3, 0.5, 0.7], np.float32), scale_modifier=1.0,
                tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5), dL_dpix=rng.standard_normal((3, H, W)).astype(np.float32))


def _sparse_deep_stack():
    # 36 tiles, 32 lists beyond 256 entries, 16 beyond 768 and 4 beyond 3 072 (the longest ~5 700): a sparse frame with deep lists,
    # long from long_min_sparse on, blended by the deep workers -- and the deep_min_* variants move lists of 256 .. 3 072 entries
    # to one wave per quad
    return _add(_stacked_scene(14000, 160, 160, seed=81, spread_px=36.0), _stacked_scene(10000, 160, 160, seed=82, spread_px=10.0))


def _dense_with_stack():
    # every one of 68 x 68 tiles non-empty with a stack in the middle (4 lists beyond 3 072 entries, 8 of CKPT_DEEP_MIN and more):
    # dense with deep tiles -- the mixed backward -- and 48 faint splats of ~1 000 tiles each (big splats: binning groups of their own)
    from hugs_amd import synthetic as syn
    sc = _stacked_scene(9000, 1088, 1088, seed=31, spread_px=14.0)
    _add(sc, syn.scene_gaussians(24_000, sc["cam"], seed=32, sigma_px=2.0))   # (33 048 Gaussians in all: binned by cell, hgs_common.h bin_mode_for)
    big = syn.scene_gaussians(48, sc["cam"], seed=33, sigma_px=90.0, ref_P=48)
    big["opacities"] = (0.05 * np.asarray(big["opacities"])).astype(np.float32)
    return _add(sc, big)


FRAMES = {
    "sparse_deep_stack": _sparse_deep_stack,
    "dense_with_stack": _dense_with_stack,
    # 1 024 lists of 1 600 .. 2 150 entries, all flat: sparse, long from 1 024 on, NOT split by depth (binning.hip many_flat_long)
    "many_flat_long": lambda: _from_frame("uniform", 512, 512, 200_000, 0, seed=85),
    # a person filling 512 x 512 (1 020 tiles, longest / E = 1.7): sparse, long lists one wave per quad (binning.hip even_and_full)
    "even_and_full": lambda: _from_frame("human_d3", 512, 512, 110_210, 0, seed=86),
    # small ragged frames, lists of 300 .. 700 entries: SH of degree 2 with cov3D_precomp, and colors_precomp
    "ragged_sh_cov3D": lambda: make_scene(P=900, H=75, W=101, seed=83, D=2, cov3D_precomp=True, sigma_px=9.0),
    "ragged_colors_precomp": lambda: make_scene(P=700, H=70, W=93, seed=84, colors_precomp=True, sigma_px=12.0),
}

# module-scope caches: the scene and its oracle run per frame, the default variant's outputs per frame, the path per (frame, variant)
_SCENE, _ORACLE, _DEFAULT, _PATH = {}, {}, {}, {}


def _scene(frame):
    if frame not in _SCENE:
        _SCENE[frame] = FRAMES[frame]()
    return _SCENE[frame]


def _oracle(frame):
    if frame not in _ORACLE:
        sc = _scene(frame)
        inp = oracle_inputs(sc)
        ho.set_threads(ho.usable_cpus())
        ref = ho.forward(inp)
        _ORACLE[frame] = (ref, ho.backward(inp, ref, sc["dL_dpix"]))
    return _ORACLE[frame]


def _set_variant(name, monkeypatch):
    """the variant's switches set, every other switch name unset, the library told; checkpoints as the variant wants them
    (the caller restores dgr._USE_CKPT and the C++ binding's flag)"""
    import diff_gaussian_rasterization as dgr
    env, ckpt = VARIANTS[name]
    for k in SWITCH_NAMES:
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)
    reload_switches(monkeypatch)
    dgr._USE_CKPT = ckpt
    if dgr._cpp is not None:
        dgr._cpp.use_checkpoints(ckpt)


def _forms():
    import diff_gaussian_rasterization as dgr
    lib = dgr._load()
    return int(lib.hgs_debug_stat(b"last_forward_forms")), int(lib.hgs_debug_stat(b"last_backward_forms"))


def _run(frame, variant, device, monkeypatch, frames=3):
    """`frames` frames forward + backward (repeat bars), then the forward state of one more; returns the outputs and the path"""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _debug_forward_state
    sc = _scene(frame)
    use_ckpt = dgr._USE_CKPT
    try:
        _set_variant(variant, monkeypatch)
        dL = to_dev(sc["dL_dpix"], device)
        first = grads = None
        for k in range(frames):   # (later frames run on what the first taught the shape's record: hints, checkpoint slots, binning mode)
            t, color, radii = run_gpu(sc, device)
            color.backward(dL)
            torch.cuda.synchronize()
            got = {name: t[name].grad.cpu().numpy() for name, _ in GRAD_KEYS if t[name] is not None}
            if first is None:
                first = (color.detach().clone(), radii.clone())
            else:   # the same frame again: image bit for bit, gradients up to the order of the float atomics
                assert torch.equal(color, first[0]) and torch.equal(radii, first[1]), f"{frame}/{variant}: frame {k} differs from the first"
                for name in got:
                    assert rel_l2(got[name], grads[name]) <= 1e-4, f"{frame}/{variant}: frame {k}, grad {name}"
            grads = got
        bwd_forms = _forms()[1]
        tg = {k: to_dev(sc[k], device) for k in ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")}
        color, radii, st = _debug_forward_state(tg["means3D"], tg["opacities"], gpu_settings(sc, device), shs=tg["shs"],
                                                colors_precomp=tg["colors_precomp"], scales=tg["scales"], rotations=tg["rotations"],
                                                cov3D_precomp=tg["cov3D_precomp"])
        torch.cuda.synchronize()
        fwd_forms = _forms()[0]
    finally:
        dgr._USE_CKPT = use_ckpt
        if dgr._cpp is not None:
            dgr._cpp.use_checkpoints(use_ckpt)
    assert torch.equal(color, first[0]), f"{frame}/{variant}: the forward-state frame differs from the first"
    nt = st["n_total"].cpu().numpy()
    path = dict(sparse_frame=st["sparse_frame"], has_long_tiles=st["has_long_tiles"], ckpt_kind=int(nt[3]), long_from=int(nt[4]),
                deep_from=int(nt[8]), has_checkpoints=st["has_checkpoints"], ckpt_slots_used=st["ckpt_slots_used"],
                forward_forms=fwd_forms, backward_forms=bwd_forms)
    _PATH[(frame, variant)] = path
    out = dict(color=first[0].cpu().numpy(), radii=first[1].cpu().numpy(), grads=grads, N=st["N"],
               values=st["values"].cpu().numpy().view(np.uint32), ranges=st["ranges"].cpu().numpy().view(np.uint32),
               final_T=st["final_T"].cpu().numpy(), n_contrib=st["n_contrib"].cpu().numpy().view(np.uint32))
    return out, path


def _default(frame, device, monkeypatch):
    if frame not in _DEFAULT:
        _DEFAULT[frame] = _run(frame, "default", device, monkeypatch)[0]
    return _DEFAULT[frame]


def _path(frame, variant, device, monkeypatch):
    if (frame, variant) not in _PATH:
        _run(frame, variant, device, monkeypatch, frames=2)
    return _PATH[(frame, variant)]


def grad_distance(g, r, flipped):
    """relative L2 of a gradient tensor against the oracle's; where it lies beyond the bar and a pixel took the other branch of a
    threshold (test_gpu_fuzz.py), without the three Gaussians furthest off"""
    err = rel_l2(g, r)
    if err > GRAD_REL_TOL and flipped:
        worst = np.argsort(-np.abs(g - r).reshape(g.shape[0], -1).max(axis=1))[:3]
        keep = np.ones(g.shape[0], bool)
        keep[worst] = False
        err = rel_l2(g[keep], r[keep])
    return err


def _check_against_oracle(out, ref, refg, what):
    assert np.array_equal(out["radii"], ref["radii"]), f"{what}: radii"
    assert out["N"] == ref["N"], f"{what}: N {out['N']} != {ref['N']}"
    assert np.array_equal(out["values"], ref["values"]), f"{what}: sorted list"
    assert np.array_equal(out["ranges"], ref["ranges"]), f"{what}: tile ranges"
    check_image(out["color"], ref["color"], f"{what} colour")
    check_image(out["final_T"], ref["final_T"], f"{what} final_T")
    mism = int((out["n_contrib"] != ref["n_contrib"]).sum())
    assert mism <= max(2, (1 - COLOR_INLIER_FRAC) * out["n_contrib"].size), f"{what}: n_contrib differs on {mism} pixels"
    flipped = int((np.abs(out["color"].astype(np.float64) - ref["color"]) > COLOR_TOL).any(axis=0).sum())
    for name, rk in GRAD_KEYS:
        if name not in out["grads"]:
            continue
        g, r = out["grads"][name], refg[rk]
        assert np.isfinite(g).all(), f"{what}: non-finite gradient in {name}"
        err = grad_distance(g.reshape(r.shape), r, flipped)
        assert err <= GRAD_REL_TOL, f"{what}: grad {name} rel L2 {err:.3e} against the oracle"


def _check_against_default(out, base, cls, what):
    if cls in ("order", "backward"):
        assert np.array_equal(out["color"], base["color"]), f"{what}: image not bit-equal to the default's"
        assert np.array_equal(out["n_contrib"], base["n_contrib"]), f"{what}: n_contrib not equal to the default's"
    else:
        d = np.abs(out["color"].astype(np.float64) - base["color"]).max(axis=0)
        assert float((d <= 1e-6).mean()) >= 0.9998 and d.max() <= COLOR_TOL, \
            f"{what}: image against the default's: max {d.max():.3e}, {(d > 1e-6).sum()} pixels beyond 1e-6"
        assert float((out["n_contrib"] == base["n_contrib"]).mean()) >= 0.9998, f"{what}: n_contrib against the default's"
    for name in base["grads"]:
        bar = order_tol(name) if cls == "order" else ALT_BACKWARD_TOL
        err = rel_l2(out["grads"][name], base["grads"][name])
        assert err <= bar, f"{what}: grad {name} rel L2 {err:.3e} against the default's (bar {bar:g}, class {cls})"


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("frame", list(FRAMES))
def test_path_matrix_cell(frame, variant, device, monkeypatch):
    assert variant in CLASS, f"variant {variant} has no class in CLASS: say what it may change against the default"
    ref, refg = _oracle(frame)
    what = f"{frame}/{variant}"
    out, _ = _run(frame, variant, device, monkeypatch)
    _check_against_oracle(out, ref, refg, what)
    if variant == "default":
        _DEFAULT.setdefault(frame, out)
        return
    _check_against_default(out, _default(frame, device, monkeypatch), CLASS[variant], what)


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "default"])
def test_every_variant_leaves_the_default_path_on_some_frame(variant, device, monkeypatch):
    """the scan's decisions (sparse_frame, has_long_tiles, n_total[3], [4], [8], checkpoints) or the host's launch forms
    (hgs_api.hip, last_forward_forms / last_backward_forms) differ from the default's on at least one frame of the matrix"""
    for frame in FRAMES:
        a, b = _path(frame, "default", device, monkeypatch), _path(frame, variant, device, monkeypatch)
        if a != b:
            print(f"{variant} took effect on {frame}: {', '.join(f'{k} {a[k]} -> {b[k]}' for k in a if a[k] != b[k])}")
            return
    pytest.fail(f"{variant}: the path is the default's on every frame -- the matrix lacks a frame for this variant")


# ---- SH stored as [P, M, 3] with M != 16: K1 skips its staged rows, K8 its cooperative ones (preprocess.hip), both index rows at 3 M
M_CASES = [(0, 1), (1, 4), (2, 9), (1, 9)]


# the per-Gaussian backward asked to load its SH rows cooperatively and the preprocess kernel to stage them: with M != 16 both
# must fall back to per-thread rows, with the default's results
STAGED_ROWS = {"HGS_K8_COOP": "3", "HGS_K1_STAGE_SH": "1"}


@pytest.mark.parametrize("binding", ["cpp", "ctypes"])
@pytest.mark.parametrize("D,M", M_CASES)
def test_sh_rows_of_another_width_against_the_oracle(D, M, binding, device, monkeypatch):
    from diff_gaussian_rasterization import _debug_forward_state
    if binding == "ctypes":
        _force_ctypes_binding(monkeypatch)
    sc = make_scene(P=500, H=70, W=101, seed=90 + 10 * D + M, D=D, M=M)
    assert sc["shs"].shape[1] == M
    inp = oracle_inputs(sc)
    ref = ho.forward(inp)
    refg = ho.backward(inp, ref, sc["dL_dpix"])
    K = (D + 1) ** 2
    vis = ref["radii"] > 0
    out = {}
    for mode in ("default", "staged_rows"):
        for k in STAGED_ROWS:
            if mode == "default":
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, STAGED_ROWS[k])
        reload_switches(monkeypatch)
        what = f"D={D} M={M} {binding} {mode}"
        t, color, radii = run_gpu(sc, device)
        color.backward(to_dev(sc["dL_dpix"], device))
        torch.cuda.synchronize()
        assert np.array_equal(radii.cpu().numpy(), ref["radii"]), what
        check_image(color.detach().cpu().numpy(), ref["color"], what)
        tg = {k: to_dev(sc[k], device) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        _, _, st = _debug_forward_state(tg["means3D"], tg["opacities"], gpu_settings(sc, device), shs=tg["shs"], scales=tg["scales"],
                                        rotations=tg["rotations"])
        torch.cuda.synchronize()
        assert st["N"] == ref["N"] and np.array_equal(st["values"].cpu().numpy().view(np.uint32), ref["values"]), what
        sp = st["splats"].cpu().numpy()
        assert np.array_equal(sp[vis, 6:9].view(np.uint32), np.ascontiguousarray(ref["rgb"][vis]).view(np.uint32)), f"{what}: colours not bit-exact"
        g_sh = t["shs"].grad.cpu().numpy()
        assert g_sh.shape == (500, M, 3)
        assert not g_sh[:, K:].any(), f"{what}: coefficients above the active degree got a gradient"
        grads = {}
        for name, rk in GRAD_KEYS:
            if t[name] is None:
                continue
            r = refg[rk]
            grads[name] = t[name].grad.cpu().numpy()
            err = rel_l2(grads[name].reshape(r.shape), r)
            assert err <= GRAD_REL_TOL, f"{what}: grad {name} rel L2 {err:.3e}"
        out[mode] = (color.detach().cpu().numpy(), sp, grads)
    (c0, s0, g0), (c1, s1, g1) = out["default"], out["staged_rows"]
    assert np.array_equal(c0, c1) and np.array_equal(s0, s1), f"D={D} M={M} {binding}: staged rows asked for changed the forward"
    for name in g0:
        assert rel_l2(g1[name], g0[name]) <= order_tol(name), f"D={D} M={M} {binding}: staged rows asked for changed grad {name}"


@pytest.mark.parametrize("binding", ["cpp", "ctypes"])
@pytest.mark.parametrize("D,M1,M2", [(2, 16, 9), (1, 9, 4), (1, 4, 16)])
def test_second_segment_of_another_sh_width_against_the_oracle(D, M1, M2, binding, device, monkeypatch):
    """The joint call with each set's SH at its own width, against the oracle of the concatenated set (the second's SH zero-padded
    to the first's width): image, radii, and each set's gradients -- the first K columns of the second's SH."""
    from diff_gaussian_rasterization import GaussianRasterizer
    if binding == "ctypes":
        _force_ctypes_binding(monkeypatch)
    sc = make_scene(P=600, H=75, W=96, seed=70 + M1 + M2, D=D, M=max(M1, M2))
    P, cut = 600, 247
    sh = sc["shs"].copy()
    sh[:cut, M1:] = 0.0
    sh[cut:, M2:] = 0.0
    sc["shs"] = sh
    inp = oracle_inputs(sc)
    ref = ho.forward(inp)
    refg = ho.backward(inp, ref, sc["dL_dpix"])
    keys = ("means3D", "opacities", "scales", "rotations")
    a = {k: to_dev(sc[k][:cut], device, True) for k in keys}
    b = {k: to_dev(sc[k][cut:], device, True) for k in keys}
    a["shs"] = to_dev(np.ascontiguousarray(sh[:cut, :M1]), device, True)
    b["shs"] = to_dev(np.ascontiguousarray(sh[cut:, :M2]), device, True)
    means2D = torch.zeros(P, 3, device=device, requires_grad=True)
    color, radii = GaussianRasterizer(gpu_settings(sc, device))(means3D=a["means3D"], means2D=means2D, opacities=a["opacities"],
                                                                shs=a["shs"], scales=a["scales"], rotations=a["rotations"], second=b)
    color.backward(to_dev(sc["dL_dpix"], device))
    torch.cuda.synchronize()
    what = f"D={D} M={M1}/{M2} {binding}"
    assert np.array_equal(radii.cpu().numpy(), ref["radii"]), what
    check_image(color.detach().cpu().numpy(), ref["color"], what)
    assert rel_l2(means2D.grad.cpu().numpy(), refg["means2D"]) <= GRAD_REL_TOL, what
    K = (D + 1) ** 2
    for k in keys + ("shs",):
        r = refg[k]
        ga, gb = a[k].grad.cpu().numpy(), b[k].grad.cpu().numpy()
        if k == "shs":
            assert ga.shape == (cut, M1, 3) and gb.shape == (P - cut, M2, 3)
            assert not ga[:, K:].any() and not gb[:, K:].any(), f"{what}: coefficients above the active degree got a gradient"
            ga, gb, r = ga[:, :K], gb[:, :K], r[:, :K]
        full = np.concatenate([ga.reshape((cut,) + r.shape[1:]), gb.reshape((P - cut,) + r.shape[1:])], 0)
        assert rel_l2(full, r) <= GRAD_REL_TOL, f"{what}: grad {k}"
        assert rel_l2(gb.reshape(r[cut:].shape), r[cut:]) <= GRAD_REL_TOL, f"{what}: grad {k} of the second set"
