"""Every gradient of the rasterizer, Gaussian by Gaussian, against the fp64 oracle -- on every backward form.

The other GPU modules hold a gradient tensor to a relative L2 norm of 1e-3 (test_gpu_parity.GRAD_REL_TOL) over the whole tensor.  That
figure is a statement about the few strongest Gaussians: a 1 % error on every row below 3 % of the largest, or the loss of one median
Gaussian's row altogether, passes it (the CPU tests below show both).  What hides there is what the backward kernels do last and
least: entries deep in a list where T is small, the first entries restored from a checkpoint, Gaussians cut by the right and bottom
image edges, the tail of a depth-split tile, rows of the second set of a joint call.  Here every visible Gaussian's row is weighed by
its own norm (tests/grad_per_gaussian.py: s_i = |g_i - r_i| / (|r_i| + 1e-3 max_j |r_j|), r the fp64 oracle's), and the bar is

    max_i s_i(GPU) <= F max_i s_i(fp32 oracle) + 1e-6,     median_i s_i(GPU) <= F median_i s_i(fp32 oracle) + 1e-7

F = 4 being the project's margin for "the same arithmetic in another order of summation" (tests/test_triplane.py, _hold).  A pixel
within rounding of a threshold (alpha 1/255, T 1e-4, the 0.99 clamp) takes the other branch on the GPU: n_contrib differs from the fp64
oracle's there, or the colour by more than 16 x the fp32 oracle's worst pixel; of the Gaussians in the list of a tile with such a
pixel at most 3 per (frame, form, tensor) are left out of the max, never of the median.  The fp32 oracle itself needs none of it.

Frames: FRAMES below -- ten small ones (both oracle runs of one take well under a second) and one dense frame of 640 x 640 for the
mixed backward (_dense_with_deep_tile; two seconds).  Forms: the backward and per-Gaussian-backward
variants of test_gpu_path_matrix.VARIANTS (FORM_VARIANTS), two frames in a row each (the second runs on the record the first left);
on ragged and deep_stack_3k also the ctypes binding, the frame split into two sets through `second=` under both bindings, the C++
binding's render_pair (joint + first-set-only render in one node: the add_* instantiation of the per-Gaussian backward; cotangents
zeroed where the fp64 image is within 1e-4 of the output clamp, so that no pixel's clamp mask hangs on rounding), and a call with
return_alpha_depth=True under cotangents on colour, alpha and depth (references: tests/maps_ref.py in both precisions).  A guard
holds the frames to the backward forms the path matrix reaches with these variants on its own, far larger, frames.

Measured on an MI355X (run with -s: every (frame, form, pass, tensor, walk) prints err, err_ref, their ratio, the same of the medians,
F and what was left out), 109 cells x 2 passes, worst ratio per tensor of max s_i to the fp32 oracle's (of the medians, after the 1e-7):

  tensor           Gaussians walked from the end of the lists       Gaussians a walk from the forward's checkpoints reaches
                   (one wave per tile / per quad, no checkpoints)   (segmented, mixed, two launches: the default on every frame here)
  means3D          3.0 (1.0)   F = 4                                17.7 (16.8)   F = 16, 1 cell beyond it
  means2D          3.5 (1.0)   F = 4                                76.3 (10.7)   F = 16, 10 cells beyond it
  opacities        1.5 (1.0)   F = 4                                30.0 (22.8)   F = 16, 1 cell beyond it
  scales           1.8 (1.0)   F = 4                                12.2 (10.7)   F = 16
  rotations        1.5 (1.0)   F = 4                                18.3 (8.9)    F = 16, 5 cells beyond it
  shs, every band  3.1 (1.0)   F = 4                                1.9 (1.0)     F = 4
  colors_precomp   1.4 (0)     F = 4                                1.4 (0)       F = 4
  cov3D_precomp    0.8 (0)     F = 4                                3.4 (0)       F = 4

No pixel of any cell was flipped (n_contrib equal to the fp64 oracle's everywhere, colours and maps within 16 x the fp32 oracle's worst
pixel), so no Gaussian was set aside anywhere: the allowance is unused (a CPU test exercises it).  The maps cells, the two-set cells and
render_pair read like the default cells of their frames; both passes of a cell agree to 1 % of the figures.

Which Gaussians a pass walked from checkpoints is read from last_backward_forms and the oracle's lists (_from_checkpoints): all of a
sparse frame whose backward is the segmented one; on the dense frame's mixed kernel and two launches only those in the list of
CKPT_DEEP_MIN = 512 entries and more -- every other Gaussian of that frame is held to F = 4 there too.  Each group is compared with the
fp32 oracle's max and median over the SAME Gaussians.

The finding, and the arithmetic difference behind the right-hand column: a walk that starts at a checkpoint takes S, everything
composited behind its segment dotted with dL/dpixel, as g . (C_end - C_checkpoint) -- a difference of two fp32 colour prefixes of the
forward's running sum (blend.hip, blend_backward_wave<1, true>), each rounded at every entry the forward added: an ABSOLUTE error of a
few 6e-8 |C| |g|.  The walk from the end of the list builds S from the back, smallest terms first: a RELATIVE error.  S enters
dL/dalpha = T (c . g) - S / (1 - alpha), so an entry at transmittance T carries a relative error of ~1e-7 / T from a checkpoint: nothing
of a tensor's norm (the tensor-wide 1e-3 bars of the other modules hold throughout), up to 77 x the fp32 oracle's distance on the
weakest rows.  The colour gradients (shs, colors_precomp) do not read S and hold at F = 4.  So the five tensors that read S are held to
F = 16 from checkpoints (worst ratios 12 .. 76: 1.5 x any of them asks for 32 and more, capped at 16), on EVERY (frame, form, tensor)
cell -- and 18 cells measure beyond it, on two frames of large splats over nearly opaque pixels: big_splats (means2D 2.5 x its bar,
rotations 1.13 x, in all five checkpointed variants) and ragged_colors_precomp (means2D 1.95 x in all five, 4.6 x under no_deep_forward,
where also means3D 1.08 x and opacities 1.87 x).  Those 18, and no other, carry xfail(strict=True) with the figure (BEYOND_16): a
regression on any other cell fails, and so does a repair of one of these until its mark is removed.  It cannot be repaired in the
backward -- the prefix is already rounded when the forward stores it; a forward that kept a second colour accumulator per pixel,
restarted at every checkpoint, would hand the backward relative sums (three more FMAs per pixel and entry in the forward's loop, in
both walkers, and a backward that adds up the deeper segments' sums): a kernel change of its own, not part of this module.
On big_splats the MEDIAN of means3D, opacities and scales from checkpoints sits at its bar (0.8 .. 1.2 of it from run to run: med_ref
is 7e-9 .. 1e-8 there, the bar mostly the rule's 1e-7, and the float atomics' order moves the median by as much): on those 15 cells the
max is asserted and a median beyond the bar is reported as an expected failure that is not strict (MEDIAN_AT_THE_BAR).
What F = 16 lets through is stated by the CPU tests: mutation (a) passes it on opacities of deep_stack_3k and dense_with_deep_tile.
"""
import numpy as np
import pytest
import torch

import grad_per_gaussian as gpg
import test_gpu_path_matrix as pm
from maps_ref import map_upstreams, maps_reference, summed
from oracle import hgs_oracle as ho
from scenes import make_scene, oracle_inputs
from test_gpu_parity import GRAD_REL_TOL, _force_ctypes_binding, _stacked_scene, gpu_settings, gpu_tensors, rel_l2, run_gpu, to_dev
from test_gpu_path_matrix import GRAD_KEYS, VARIANTS, _forms, _set_variant

gpu = pytest.mark.gpu   # (the tests of section 1 run on the CPU)

# The margin per tensor: 4 unless the measured worst ratio (the docstring's table) asks for more, never above 16 -- one table for the
# Gaussians whose entries are walked from the end of the lists, one for those a walk from the forward's checkpoints reaches
F = {"means3D": 4, "means2D": 4, "opacities": 4, "shs": 4, "colors_precomp": 4, "scales": 4, "rotations": 4, "cov3D_precomp": 4}
F_CHECKPOINTED = dict(F, means3D=16, means2D=16, opacities=16, scales=16, rotations=16)
BWD_TILE, BWD_SEGMENTED, BWD_MIXED = 1 << 0, 1 << 2, 1 << 3   # hgs_common.h: bits of last_backward_forms
CKPT_DEEP_MIN = 512                                           # hgs_common.h: the lists of a DENSE frame that are walked from checkpoints
# a frame ill-conditioned enough for the fp32 oracle to lie this far from the fp64 one says nothing through F x err_ref (largest here: 6.4e-4)
ERR_REF_MAX = 2e-3
FORM_VARIANTS = ["default", "no_ckpt", "bwd_wave_per_tile", "bwd_wave_per_quad", "bwd_two_launches", "no_bwd_segmented", "no_deep_forward",
                 "k8_coop_per_thread", "k8_coop_load_and_store"]
EXTRA_FORMS = ["ctypes", "second", "second_ctypes", "render_pair", "maps"]   # on EXTRA_FRAMES, all under the default variant
EXTRA_FRAMES = ["ragged", "deep_stack_3k"]
PER_GAUSSIAN = ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")


def _dense_with_deep_tile(seed=40, side=640, n_real=1000, n_faint=8000, n_stack=2150):
    """The one DENSE frame of the module (binning.hip, frame_is_sparse: >= 1 536 non-empty tiles, E = sum len^2 / N within 2.5 x the mean
    list) with a list beyond 2 048 entries (hgs_api.hip: only then does a dense frame take the checkpoint buffer, from the shape's second
    frame on): the mixed backward -- one wave per tile beside the checkpointed walk of the deep tile -- and its two-launch twin.
    40 x 40 tiles take 409 600 pixels, and at pixel coordinates of some hundreds the fp32 oracle takes the other side of alpha = 1/255
    from the fp64 one on about 1.5e-5 of the pixels a splat's 1/255 contour passes (measured: 8 pixels of a frame with ordinary lists of
    50).  So the lists are filled with 8 000 FAINT splats -- opacity below 1/255: in every list they cover, skipped at every pixel, in
    either precision -- among 1 000 small ordinary ones (sigma 1.6 px), and 2 150 of sigma 1 px at 0.02 of their opacity sit in the middle
    of tile (20, 20), reaching no other: a list of 2 209 walked to its end.  Seeds 40 .. 51 were tried for a frame on which the two
    oracles agree (radii, n_contrib, colours to 3e-5, gradients within ERR_REF_MAX): 40, 45, 46, 49, 50 and 51 do, 40 by the most."""
    import math
    from hugs_amd import synthetic as syn
    sc = make_scene(P=n_real, H=side, W=side, seed=seed, D=1, sigma_px=1.6, with_culled=False)
    rng = np.random.default_rng(seed + 500)
    faint = syn.scene_gaussians(n_faint, sc["cam"], seed=seed + 1, sigma_px=4.0, ref_P=n_faint)
    faint["opacities"] = rng.uniform(0.0005, 0.0035, (n_faint, 1)).astype(np.float32)
    stack = syn.scene_gaussians(n_stack, sc["cam"], seed=seed + 2, sigma_px=1.0, ref_P=n_stack)
    z = stack["means3D"][:, 2].astype(np.float64)
    f = side / (2.0 * math.tan(sc["cam"]["fovx"] / 2))
    for axis in (0, 1):   # (the image centre is the corner of four tiles: 8 pixels further lies the middle of one)
        stack["means3D"][:, axis] = (8.0 + rng.uniform(-2.0, 2.0, n_stack)) / f * z
    stack["opacities"] = (0.02 * stack["opacities"]).astype(np.float32)
    return pm._add(pm._add(sc, faint), stack)


FRAMES = {
    "ragged": lambda: make_scene(P=401, H=75, W=101, seed=22, D=2),
    "deg3": lambda: make_scene(P=600, H=96, W=128, seed=3, D=3),
    "tiny_splats": lambda: make_scene(P=800, H=64, W=64, seed=6, D=3, sigma_px=1.2),
    "big_splats": lambda: make_scene(P=60, H=64, W=80, seed=5, D=3, sigma_px=40.0),
    "opaque_wide": lambda: make_scene(P=500, H=90, W=130, seed=31, D=3, opaque=True, wide=True),
    "deep_stack": lambda: _stacked_scene(1200, 64, 64, seed=25, spread_px=8.0),
    "deep_stack_3k": lambda: _stacked_scene(3000, 64, 64, seed=26, spread_px=12.0),
    "deep_stack_6k": lambda: _stacked_scene(6000, 96, 96, seed=27, spread_px=10.0),
    "ragged_sh_cov3D": lambda: make_scene(P=900, H=75, W=101, seed=83, D=2, cov3D_precomp=True, sigma_px=9.0),
    "ragged_colors_precomp": lambda: make_scene(P=700, H=70, W=93, seed=84, colors_precomp=True, sigma_px=12.0),
    "dense_with_deep_tile": _dense_with_deep_tile,
}
LONGEST_LIST = {"ragged": 221, "deg3": 212, "tiny_splats": 140, "big_splats": 54, "opaque_wide": 238, "deep_stack": 603, "deep_stack_3k": 1236,
                "deep_stack_6k": 2693, "ragged_sh_cov3D": 665, "ragged_colors_precomp": 598, "dense_with_deep_tile": 2209}

# frames on which ONE Gaussian of median norm is more than 1e-3 of every gradient tensor (test_the_bar_catches_...: mutation (b))
ONE_ROW_WEIGHS_1E_3 = {"tiny_splats", "deep_stack", "deep_stack_3k", "deep_stack_6k", "dense_with_deep_tile"}

_SCENE, _REF = {}, {}


def _scene(frame):
    if frame not in _SCENE:
        _SCENE[frame] = FRAMES[frame]()
    return _SCENE[frame]


def _named(sc, refg):
    """an oracle gradient dict under the API's tensor names, the inputs of this frame only"""
    return {name: refg[rk] for name, rk in GRAD_KEYS if sc.get(name) is not None or name == "means2D"}


def _both(fn):
    """fn(dtype) under the fp64 and the fp32 oracle, every usable CPU each"""
    out = []
    for dt in (np.float64, np.float32):
        ho.set_threads(ho.usable_cpus(), dt)
        out.append(fn(dt))
    return out


def _colour(sc, dL, dtype):
    inp = oracle_inputs(sc, dtype)
    fwd = ho.forward(inp)
    return fwd, ho.backward(inp, fwd, dL)


def _subset(sc, sl):
    return dict(sc, **{k: sc[k][sl] for k in PER_GAUSSIAN if sc.get(k) is not None})


def _inside_clamp(img64):
    """1 where the fp64 image is clear of the output clamp by 1e-4 (ten times what a GPU pixel that is not flipped may differ by)"""
    return ((img64 > 1e-4) & (img64 < 1.0 - 1e-4)).astype(np.float32)


def _reference(frame, kind="colour"):
    """dict(fwd64, fwd32, g64, g32 (API names), vis, images64 / images32 (what a flipped pixel is judged on)) of a frame, once:
    kind "colour": the frame under its own dL_dpix;  "maps": colour + alpha + depth cotangents (tests/maps_ref.py);
    "render_pair": the joint render and the first set's own render on the complementary background, both clamped to [0, 1]"""
    if (frame, kind) in _REF:
        return _REF[(frame, kind)]
    sc = _scene(frame)
    if kind == "colour":
        (f64, g64), (f32, g32) = _both(lambda dt: _colour(sc, sc["dL_dpix"], dt))
        ref = dict(fwd64=f64, fwd32=f32, g64=_named(sc, g64), g32=_named(sc, g32), raw64=g64, raw32=g32, images64=[f64["color"]], images32=[f32["color"]])
    elif kind == "maps":
        base = _reference(frame)
        gA, gD = map_upstreams(sc["H"], sc["W"])
        m64, m32 = _both(lambda dt: maps_reference(sc, gA, gD, dtype=dt))
        ref = dict(fwd64=base["fwd64"], fwd32=base["fwd32"], g64=_named(sc, summed(m64["grads"], base["raw64"])), g32=_named(sc, summed(m32["grads"], base["raw32"])),
                   images64=[base["fwd64"]["color"], m64["alpha"], m64["depth"]], images32=[base["fwd32"]["color"], m32["alpha"], m32["depth"]],
                   upstreams=(gA, gD))
    else:
        base = _reference(frame)
        cut = _cut(sc)
        first = dict(_subset(sc, slice(0, cut)), bg=(1.0 - sc["bg"]).astype(np.float32))
        h64 = ho.forward(oracle_inputs(first, np.float64))["color"]
        dL_joint = sc["dL_dpix"] * _inside_clamp(base["fwd64"]["color"])
        dL_first = np.random.default_rng(7).standard_normal(h64.shape).astype(np.float32) * _inside_clamp(h64)
        grads, firsts = [], []
        for (_, gj), (fh, gh) in zip(_both(lambda dt: _colour(sc, dL_joint, dt)), _both(lambda dt: _colour(first, dL_first, dt))):
            g = {k: v.copy() for k, v in _named(sc, gj).items()}
            for k, v in _named(first, gh).items():
                if k != "means2D":   # (the first set's own render has a viewspace tensor of its own, which nothing reads)
                    g[k][:cut] += v
            grads.append(g)
            firsts.append(fh)
        clip = lambda a: np.clip(a, 0.0, 1.0)
        ref = dict(fwd64=base["fwd64"], fwd32=base["fwd32"], g64=grads[0], g32=grads[1], first64=firsts[0], first32=firsts[1],
                   images64=[clip(base["fwd64"]["color"]), clip(firsts[0]["color"])], images32=[clip(base["fwd32"]["color"]), clip(firsts[1]["color"])],
                   upstreams=(dL_joint, dL_first), first=first)
    ref["vis"] = ref["fwd64"]["radii"] > 0
    _REF[(frame, kind)] = ref
    return ref


def _cut(sc):
    return (2 * sc["means3D"].shape[0]) // 5 + 1


def _tensors(sc, grads):
    """[(tensor name, label, [P, k])] of a gradient dict under the API's names: every tensor, and the SH degree bands"""
    return [(name, label, m) for name in grads for label, m in gpg.split(name, grads[name], sc["D"])]


def _ref_scores(frame, kind="colour"):
    ref = _reference(frame, kind)
    if "s32" not in ref:
        sc = _scene(frame)
        want = {label: m for _, label, m in _tensors(sc, ref["g64"])}
        ref["s32"] = {label: gpg.scores(m, want[label], ref["vis"]) for _, label, m in _tensors(sc, ref["g32"])}
    return ref["s32"]


# ------------------------------------------------------------------------------------------------ 1. what the bar means (no GPU)
@pytest.mark.parametrize("frame", list(FRAMES))
def test_the_fp32_oracle_needs_no_allowance_and_lies_close_to_fp64(frame):
    """radii and n_contrib of the two precisions are equal everywhere, so no pixel is flipped and nothing would be set aside; and the
    fp32 oracle's worst s_i stays under ERR_REF_MAX on every tensor -- F x err_ref is a bar of a few 1e-3 at most"""
    ref, sc = _reference(frame), _scene(frame)
    f64, f32 = ref["fwd64"], ref["fwd32"]
    lens = f64["ranges"][:, 1].astype(np.int64) - f64["ranges"][:, 0]
    print(f"{frame}: P {sc['means3D'].shape[0]}, visible {int(ref['vis'].sum())}, N {f64['N']}, longest list {int(lens.max())}, "
          f"non-empty tiles {int((lens > 0).sum())} of {len(lens)}, colours fp32 against fp64 {np.abs(f32['color'] - f64['color']).max():.2e}")
    assert int(lens.max()) == LONGEST_LIST[frame]
    assert np.array_equal(f32["radii"], f64["radii"]) and np.array_equal(f32["values"], f64["values"]) and np.array_equal(f32["ranges"], f64["ranges"])
    assert np.array_equal(f32["n_contrib"], f64["n_contrib"]), f"{frame}: n_contrib differs on {(f32['n_contrib'] != f64['n_contrib']).sum()} pixels"
    flipped = gpg.flipped_pixels((f32["n_contrib"], f64["n_contrib"]), ref["images32"], ref["images64"], ref["images32"])
    assert not flipped.any() and not gpg.behind_flipped(flipped, f64["ranges"], f64["values"], len(ref["vis"])).any()
    for label, s in _ref_scores(frame).items():
        assert s is not None, f"{frame}: the fp64 oracle has no gradient for {label}"
        print(f"{frame} {label}: err_ref {s.max():.2e}, med_ref {np.median(s):.2e}")
        assert s.max() <= ERR_REF_MAX, f"{frame} {label}: the fp32 oracle's worst Gaussian is {s.max():.2e} from the fp64 oracle's"


@pytest.mark.parametrize("kind", ["maps", "render_pair"])
@pytest.mark.parametrize("frame", EXTRA_FRAMES)
def test_the_references_of_the_maps_and_of_the_pair_lie_close_to_fp64(frame, kind):
    """the same of the two summed references: colour + alpha + depth (tests/maps_ref.py), and the joint render + the first set's own"""
    ref = _reference(frame, kind)
    if kind == "render_pair":
        assert np.array_equal(ref["first32"]["n_contrib"], ref["first64"]["n_contrib"]) and np.array_equal(ref["first32"]["radii"], ref["first64"]["radii"])
        print(f"{frame}: cotangents zeroed at the clamp on {float((ref['upstreams'][0] == 0).mean()):.4f} of the joint image, "
              f"{float((ref['upstreams'][1] == 0).mean()):.4f} of the first set's")
    for label, s in _ref_scores(frame, kind).items():
        print(f"{frame} {kind} {label}: err_ref {s.max():.2e}, med_ref {np.median(s):.2e}")
        assert s.max() <= ERR_REF_MAX, f"{frame} {kind} {label}: the fp32 reference's worst Gaussian is {s.max():.2e} from the fp64 one's"


def test_the_allowance_leaves_out_three_at_the_most_and_only_behind_a_flipped_pixel():
    """hold() and behind_flipped() on made-up scores: of the Gaussians beyond the bar only those in the list of a tile with a flipped
    pixel are left out of the max, the three furthest off at the most, and the median is over all of them whatever is left out"""
    s_ref = np.full(40, 1e-5)
    s = s_ref.copy()
    s[[3, 7, 11, 19]] = [0.5, 0.4, 0.3, 0.2]
    allowed = np.zeros(40, bool)
    assert not gpg.hold(s, s_ref, 4)["ok"] and not gpg.hold(s, s_ref, 4, allowed)["ok"]
    allowed[[3, 7, 11, 19]] = True
    h = gpg.hold(s, s_ref, 4, allowed)                       # four beyond the bar, three may go: the fourth decides
    assert (h["left_out"], h["err"], h["ok"]) == (3, 0.2, False)
    s[19] = 1e-5
    h = gpg.hold(s, s_ref, 4, allowed)
    assert (h["left_out"], h["ok"]) == (3, True) and h["err"] == 1e-5
    allowed[7] = False                                       # one of them not behind a flipped pixel: it stays in the max
    assert gpg.hold(s, s_ref, 4, allowed)["err"] == 0.4
    s = np.where(np.arange(40) < 21, 1e-3, 1e-5)             # the median is beyond its bar: nothing left out repairs that
    assert not gpg.hold(s, s_ref, 4, np.ones(40, bool))["ok"]
    flipped = np.zeros((20, 40), bool)
    flipped[17, 33] = True                                   # tile (1, 2) of a 3 x 2 grid: tile 5
    ranges = np.array([[0, 2], [2, 2], [2, 3], [3, 3], [3, 4], [4, 6]], np.uint32)
    values = np.array([0, 1, 2, 3, 4, 1], np.uint32)
    assert gpg.behind_flipped(flipped, ranges, values, 6).tolist() == [False, True, False, False, True, False]


def test_the_dense_frame_is_dense_by_the_scan_rule():
    """dense_with_deep_tile by the numbers binning.hip's frame_is_sparse reads: >= 1 536 non-empty tiles (DENSE_MIN_TILES), E = sum len^2 / N
    within 0.45 (tiles - 800) and within 2.5 x the mean list, and one list beyond 2 048 entries (it alone of CKPT_DEEP_MIN = 512 and more) for the
    segmented half (the GPU guard below holds the library to it: the mixed backward must be reached)"""
    f64 = _reference("dense_with_deep_tile")["fwd64"]
    lens = (f64["ranges"][:, 1].astype(np.int64) - f64["ranges"][:, 0])
    tiles, total, E = int((lens > 0).sum()), int(lens.sum()), float((lens ** 2).sum()) / float(lens.sum())
    print(f"dense_with_deep_tile: {tiles} non-empty tiles, N {total}, E {E:.1f}, mean {total / tiles:.1f}, {int((lens >= 512).sum())} deep tiles, longest {lens.max()}")
    assert tiles >= 1536 and E <= 0.45 * (tiles - 800) and E <= 2.5 * total / tiles * 0.9 and (lens > 2048).sum() == 1 and (lens >= 512).sum() == 1


# (frame, tensor) on which mutation (a) stays within the bar at F_CHECKPOINTED = 16: 16 x the fp32 oracle's worst opacity row (6.4e-4 and 9.5e-4:
# sums that cancel in deep lists) is more than the 9.7e-3 the mutation reads, and the median does not see it.  At F = 4 it is caught there too.
WEAK_ROWS_PASS_AT_16 = {("deep_stack_3k", "opacities"), ("dense_with_deep_tile", "opacities")}


@pytest.mark.parametrize("mutation", ["weak_rows_1_percent", "median_row_dropped"])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_the_bar_catches_what_the_tensor_wide_norm_lets_through(frame, mutation):
    """The fp32 oracle's gradients with (a) every row below 3 % of the tensor's largest times 1.01, (b) the row of the visible Gaussian
    of median norm zeroed, against BOTH bars the GPU tests apply -- F (walks from the end of the lists) and F_CHECKPOINTED (walks from
    checkpoints: 16 for means3D, means2D, opacities, scales, rotations).  At F each fails the bar on EVERY tensor of EVERY frame ((a) reads
    max s = 9.7e-3 to 9.8e-3 against bars of at most 3.9e-3, (b) 0.033 to 0.99).  At F_CHECKPOINTED (b) fails it everywhere, and (a)
    everywhere but on WEAK_ROWS_PASS_AT_16: opacities of deep_stack_3k and of dense_with_deep_tile, where a 1 % error of the weak rows
    passes a walk from checkpoints (asserted as such, so that this sentence stays true).
    Each also passes the tensor-wide rel_l2 <= GRAD_REL_TOL on at least one tensor of the frame: (a) on every frame; (b) on every frame
    but ONE_ROW_WEIGHS_1E_3 -- tiny_splats, deep_stack, deep_stack_3k, deep_stack_6k, dense_with_deep_tile -- where the tensor-wide norm
    does notice it: there a single median Gaussian carries more than 1e-3 of every tensor (the figure reads 6.1e-3 .. 1.6e-2 on
    tiny_splats, 8.3e-3 .. 1.6e-2 on deep_stack, 4.5e-3 .. 9.6e-3 on deep_stack_3k, 1.3e-3 .. 3.0e-3 on deep_stack_6k), which is
    arithmetic on the reference, not a property of any code; on the other six it reads 2.0e-5 .. 2.4e-3 and passes on one tensor at least."""
    ref, sc, s32 = _reference(frame), _scene(frame), _ref_scores(frame)
    want = {label: m for _, label, m in _tensors(sc, ref["g64"])}
    passes_old, missed, missed_at_16 = [], [], set()
    for name, label, m in _tensors(sc, ref["g32"]):
        bad = gpg.mutate_weak_rows(m) if mutation == "weak_rows_1_percent" else gpg.mutate_drop_median(m, ref["vis"])
        s = gpg.scores(bad, want[label], ref["vis"])
        h, h16 = gpg.hold(s, s32[label], F[name]), gpg.hold(s, s32[label], F_CHECKPOINTED[name])
        old = rel_l2(bad, want[label])
        print(f"{frame} {mutation} {label}: max s {h['err']:.2e} (bars {F[name] * h['err_ref'] + gpg.MAX_SLACK:.2e}, from checkpoints "
              f"{F_CHECKPOINTED[name] * h['err_ref'] + gpg.MAX_SLACK:.2e}), median s {h['med']:.2e} (bars {F[name] * h['med_ref'] + gpg.MEDIAN_SLACK:.2e}, "
              f"{F_CHECKPOINTED[name] * h['med_ref'] + gpg.MEDIAN_SLACK:.2e}), tensor-wide rel L2 {old:.2e}")
        if h["ok"]:
            missed.append(label)
        if h16["ok"]:
            missed_at_16.add((frame, label))
        if label == name and old <= GRAD_REL_TOL:
            passes_old.append(label)
    assert not missed, f"{frame} {mutation}: within the per-Gaussian bar on {missed}"
    expected = {k for k in WEAK_ROWS_PASS_AT_16 if k[0] == frame} if mutation == "weak_rows_1_percent" else set()
    assert missed_at_16 == expected, f"{frame} {mutation}: within the bar of the walks from checkpoints on {sorted(missed_at_16)}, expected {sorted(expected)}"
    if mutation == "weak_rows_1_percent" or frame not in ONE_ROW_WEIGHS_1E_3:
        assert passes_old, f"{frame} {mutation}: the tensor-wide bar catches it on every tensor -- this frame shows nothing the old bar misses"


# ------------------------------------------------------------------------------------------------ 2. the GPU, cell by cell
_CELL = {}


def _grads_of(t):
    return {name: t[name].grad.cpu().numpy() for name, _ in GRAD_KEYS if t[name] is not None}


def _state(sc, device):
    """colour and n_contrib of a forward of `sc` through the ctypes function that exposes its scratch"""
    from diff_gaussian_rasterization import _debug_forward_state
    tg = {k: to_dev(sc[k], device) for k in PER_GAUSSIAN}
    color, _, st = _debug_forward_state(tg["means3D"], tg["opacities"], gpu_settings(sc, device), shs=tg["shs"], colors_precomp=tg["colors_precomp"],
                                        scales=tg["scales"], rotations=tg["rotations"], cov3D_precomp=tg["cov3D_precomp"])
    torch.cuda.synchronize()
    return color.cpu().numpy(), st["n_contrib"].cpu().numpy().view(np.uint32)


def _two_sets(sc, device):
    cut = _cut(sc)
    a, b = ({k: to_dev(sc[k][sl], device, True) for k in PER_GAUSSIAN if sc.get(k) is not None} for sl in (slice(0, cut), slice(cut, None)))
    return a, b


def _joined(sc, a, b, means2D):
    cut, P = _cut(sc), sc["means3D"].shape[0]
    for k in a:
        assert a[k].grad is not None and b[k].grad is not None, f"no gradient for {k} of one of the two sets"
        assert a[k].grad.shape == a[k].shape and b[k].grad.shape == b[k].shape and a[k].shape[0] == cut and b[k].shape[0] == P - cut
    g = {k: torch.cat([a[k].grad, b[k].grad], 0).cpu().numpy() for k in a}
    g["means2D"] = means2D.grad.cpu().numpy()
    return g


def _frame_once(sc, form, ref, device):
    """one forward + backward in the given form: (gradients under the API's names, images, radii, last_backward_forms)"""
    from diff_gaussian_rasterization import GaussianRasterizer
    import diff_gaussian_rasterization as dgr
    P = sc["means3D"].shape[0]
    if form in ("second", "second_ctypes"):
        a, b = _two_sets(sc, device)
        means2D = torch.zeros(P, 3, device=device, requires_grad=True)
        color, radii = GaussianRasterizer(gpu_settings(sc, device))(means3D=a["means3D"], means2D=means2D, opacities=a["opacities"], shs=a["shs"],
                                                                    scales=a["scales"], rotations=a["rotations"], second=b)
        color.backward(to_dev(sc["dL_dpix"], device))
        torch.cuda.synchronize()
        return _joined(sc, a, b, means2D), [color.detach().cpu().numpy()], radii.cpu().numpy(), _forms()[1]
    if form == "render_pair":
        cpp = dgr._load_cpp()
        assert cpp is not None, "lib/_hgs_torch.so is missing: __graft_entry__.build() makes it"
        a, b = _two_sets(sc, device)
        cam, (dL_joint, dL_first) = sc["cam"], ref["upstreams"]
        five = lambda s: [s["means3D"], s["shs"], s["opacities"], s["scales"], s["rotations"]]
        image, radii, _, viewspace, first_image, first_radii, _ = cpp.render_pair(
            five(a), five(b), to_dev(sc["bg"], device), to_dev(ref["first"]["bg"], device), to_dev(cam["world_view_transform"], device),
            to_dev(cam["full_proj_transform"], device), to_dev(cam["camera_center"], device), sc["H"], sc["W"], float(cam["fovx"]), float(cam["fovy"]),
            float(sc["scale_modifier"]), sc["D"])
        assert np.array_equal(first_radii.cpu().numpy(), ref["first64"]["radii"]), "radii of the first set's own render"
        ((image * to_dev(dL_joint, device)).sum() + (first_image * to_dev(dL_first, device)).sum()).backward()
        torch.cuda.synchronize()
        return _joined(sc, a, b, viewspace), [image.detach().cpu().numpy(), first_image.detach().cpu().numpy()], radii.cpu().numpy(), _forms()[1]
    if form == "maps":
        t = gpu_tensors(sc, device)
        color, radii, alpha, depth = GaussianRasterizer(gpu_settings(sc, device))(
            means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], shs=t["shs"], colors_precomp=t["colors_precomp"], scales=t["scales"],
            rotations=t["rotations"], cov3D_precomp=t["cov3D_precomp"], return_alpha_depth=True)
        gA, gD = ref["upstreams"]
        ((color * to_dev(sc["dL_dpix"], device)).sum() + (alpha[0] * to_dev(gA, device)).sum() + (depth[0] * to_dev(gD, device)).sum()).backward()
        torch.cuda.synchronize()
        return _grads_of(t), [color.detach().cpu().numpy(), alpha.detach().cpu().numpy()[0], depth.detach().cpu().numpy()[0]], radii.cpu().numpy(), _forms()[1]
    t, color, radii = run_gpu(sc, device)
    color.backward(to_dev(sc["dL_dpix"], device))
    torch.cuda.synchronize()
    return _grads_of(t), [color.detach().cpu().numpy()], radii.cpu().numpy(), _forms()[1]


def _run(frame, form, device, monkeypatch):
    """the frame twice in a row in the given form (the second on the record the first left: hints, checkpoint slots), switches set
    and restored as test_gpu_path_matrix._run does; then the forward state of the same Gaussians for n_contrib"""
    if (frame, form) in _CELL:
        return _CELL[(frame, form)]
    import diff_gaussian_rasterization as dgr
    sc = _scene(frame)
    variant = form if form in VARIANTS else "default"
    ref = _reference(frame, form if form in ("maps", "render_pair") else "colour")
    use_ckpt = dgr._USE_CKPT
    with monkeypatch.context() as m:   # (what this cell forces -- the binding, the switches -- ends with the cell, whichever test runs it)
        if form in ("ctypes", "second_ctypes"):
            _force_ctypes_binding(m)
        try:
            _set_variant(variant, m)
            passes = [_frame_once(sc, form, ref, device) for _ in range(2)]
            bwd_forms = passes[-1][3]
            states = [_state(sc, device)]
            if form == "render_pair":
                states.append(_state(ref["first"], device))
        finally:
            dgr._USE_CKPT = use_ckpt
            if dgr._cpp is not None:
                dgr._cpp.use_checkpoints(use_ckpt)
    out = _CELL[(frame, form)] = dict(passes=passes, backward_forms=bwd_forms, states=states)
    return out


def _flipped_behind(sc, ref, images, states):
    """([P] bool: the Gaussians that may be set aside, number of flipped pixels)"""
    f64, P = ref["fwd64"], sc["means3D"].shape[0]
    flipped = gpg.flipped_pixels((states[0][1], f64["n_contrib"]), images, ref["images64"], ref["images32"])
    behind = gpg.behind_flipped(flipped, f64["ranges"], f64["values"], P)
    count = int(flipped.sum())
    if len(states) > 1:   # the first set's own render: its lists are the first set's (the same indices: it comes first)
        h64 = ref["first64"]
        fl = gpg.flipped_pixels((states[1][1], h64["n_contrib"]), [], [], [])
        behind |= np.pad(gpg.behind_flipped(fl, h64["ranges"], h64["values"], len(h64["radii"])), (0, P - len(h64["radii"])))
        count += int(fl.sum())
    return behind, count


def _from_checkpoints(ref, forms):
    """[P] bool: the Gaussians with an entry that the pass walked from a checkpoint.  A sparse frame's segmented backward walks every
    list so; the mixed kernel and the two launches of a dense frame only the lists of CKPT_DEEP_MIN entries and more."""
    f64 = ref["fwd64"]
    out = np.zeros(len(ref["vis"]), bool)
    if forms & (BWD_MIXED | BWD_TILE) and forms & (BWD_MIXED | BWD_SEGMENTED):
        for lo, hi in f64["ranges"].astype(np.int64):
            if hi - lo >= CKPT_DEEP_MIN:
                out[f64["values"][lo:hi].astype(np.int64)] = True
    elif forms & BWD_SEGMENTED:
        out[:] = True
    return out


def _hold_frame(what, frame, kind, got, radii, images, states, forms):
    """one pass against the bar: (what is wrong whatever the bar, {tensor name: [(holds at the max?, holds at the median?, message)]})"""
    sc, ref, s32 = _scene(frame), _reference(frame, kind), _ref_scores(frame, kind)
    vis, problems, verdicts = ref["vis"], [], {}
    if not np.array_equal(radii, ref["fwd64"]["radii"]):
        problems.append(f"{what}: radii differ from the oracle's")
    behind, n_flipped = _flipped_behind(sc, ref, images, states)
    ckpt = _from_checkpoints(ref, forms)[vis]
    want = {label: m for _, label, m in _tensors(sc, ref["g64"])}
    if set(got) != set(ref["g64"]):
        return [f"{what}: gradients for {sorted(got)}, inputs {sorted(ref['g64'])}"], {}
    for name, g in got.items():
        g = np.asarray(g).reshape(g.shape[0], -1)
        if not np.isfinite(g).all():
            problems.append(f"{what} {name}: non-finite gradient")
        if g[~vis].any():
            problems.append(f"{what} {name}: {int(g[~vis].any(axis=1).sum())} Gaussians with radii == 0 have a gradient")
        if name == "means2D" and g[:, 2].any():
            problems.append(f"{what}: dL/dmeans2D[:, 2] is not identically zero")
        if name == "shs" and got[name][:, (sc["D"] + 1) ** 2:].any():
            problems.append(f"{what}: SH coefficients above the active degree got a gradient")
    for name, label, m in _tensors(sc, got):
        s = gpg.scores(m, want[label], vis)
        for walk, grp, f in (("from the end", ~ckpt, F[name]), ("from checkpoints", ckpt, F_CHECKPOINTED[name])):
            if not grp.any():
                continue
            h = gpg.hold(s[grp], s32[label][grp], f, behind[vis][grp])   # (err_ref, med_ref: the fp32 oracle's over the same Gaussians)
            worst = int(np.flatnonzero(vis)[np.flatnonzero(grp)[h["worst"]]])
            ok_max, ok_med = h["err"] <= f * h["err_ref"] + gpg.MAX_SLACK, h["med"] <= f * h["med_ref"] + gpg.MEDIAN_SLACK
            print(f"{what} | {walk} {forms:#05x} | {label} | err {h['err']:.2e} err_ref {h['err_ref']:.2e} ratio {h['ratio']:.2f} | med {h['med']:.2e} "
                  f"med_ref {h['med_ref']:.2e} ratio {h['med_ratio']:.2f} | F {f} | {int(grp.sum())} Gaussians | left out {h['left_out']} "
                  f"({n_flipped} flipped pixels, {int(behind[vis].sum())} Gaussians behind them) | worst Gaussian {worst}")
            verdicts.setdefault(name, []).append((ok_max, ok_med, f"{what} {label}, {walk}: max s {h['err']:.3e} against {f} x {h['err_ref']:.3e}, median s "
                                                                  f"{h['med']:.3e} against {f} x {h['med_ref']:.3e} (Gaussian {worst}, {h['left_out']} left out)"))
    return problems, verdicts


def _hold_cell(frame, form, device, monkeypatch):
    out = _run(frame, form, device, monkeypatch)
    if "held" not in out:
        kind = form if form in ("maps", "render_pair") else "colour"
        out["held"] = [_hold_frame(f"{frame}/{form}[{k}]", frame, kind, got, radii, images, out["states"], forms)
                       for k, (got, images, radii, forms) in enumerate(out["passes"])]
    return out["held"]


def _inputs(frame):
    """the tensors of a frame that get a gradient, known without building the scene"""
    return ["means3D", "means2D", "opacities", "colors_precomp" if frame == "ragged_colors_precomp" else "shs"] + \
        (["cov3D_precomp"] if frame == "ragged_sh_cov3D" else ["scales", "rotations"])


CELLS = [(f, v) for f in FRAMES for v in FORM_VARIANTS] + [(f, e) for f in EXTRA_FRAMES for e in EXTRA_FORMS]
# The variants of FORM_VARIANTS whose backward starts from the forward's checkpoints (the docstring's finding)
CHECKPOINTED_VARIANTS = ("default", "bwd_two_launches", "no_deep_forward", "k8_coop_per_thread", "k8_coop_load_and_store")
# (frame, form, tensor) whose worst Gaussian, walked from checkpoints, was MEASURED beyond F = 16: max s over its bar.  Each is an expected
# failure of its own, strict; every other (frame, form, tensor) is asserted.
BEYOND_16 = {("big_splats", v, "means2D"): 2.5 for v in CHECKPOINTED_VARIANTS}
BEYOND_16.update({("big_splats", v, "rotations"): 1.13 for v in CHECKPOINTED_VARIANTS})
BEYOND_16.update({("ragged_colors_precomp", v, "means2D"): 1.95 for v in CHECKPOINTED_VARIANTS})
BEYOND_16.update({("ragged_colors_precomp", "no_deep_forward", "means2D"): 4.6, ("ragged_colors_precomp", "no_deep_forward", "means3D"): 1.08,
                  ("ragged_colors_precomp", "no_deep_forward", "opacities"): 1.87})
# ... and whose MEDIAN s reads 0.8 to 1.2 of its bar from run to run (big_splats: 54 Gaussians of ~1 000 pixels each, med_ref 7e-9 .. 1e-8, so the
# bar is the 1e-7 of the rule plus 1.1e-7 .. 1.7e-7, and the float atomics' order moves the median by as much): the max is asserted, a median beyond
# the bar is reported as an expected failure, not strict
MEDIAN_AT_THE_BAR = {("big_splats", v, t) for v in CHECKPOINTED_VARIANTS for t in ("means3D", "opacities", "scales")}
XFAIL_REASON = ("a walk from a checkpoint starts from S = g . (C_end - C_checkpoint), a difference of two fp32 colour prefixes: an absolute error "
                "where the walk from the end of the list carries a relative one (the module's docstring); measured max s = {} x its bar at F = 16")


def _cell_params():
    for frame, form in CELLS:
        for name in _inputs(frame):
            beyond = BEYOND_16.get((frame, form, name))
            yield pytest.param(frame, form, name, marks=[pytest.mark.xfail(strict=True, reason=XFAIL_REASON.format(beyond))] if beyond else [])


@gpu
@pytest.mark.parametrize("frame,form,name", list(_cell_params()))
def test_every_gaussians_gradient_in_every_form(frame, form, name, device, monkeypatch):
    """Both passes of the cell (run once, shared by the cell's tensors): radii, exact zeros where there must be (Gaussians with radii == 0,
    dL/dmeans2D[:, 2], SH above the active degree), and the tensor -- with every SH band -- within F x the fp32 oracle's own distance: F for
    the Gaussians walked from the end of the lists, F_CHECKPOINTED for those a walk from the forward's checkpoints reaches."""
    assert name in _reference(frame, form if form in ("maps", "render_pair") else "colour")["g64"]
    bad, median_only = [], []
    for problems, verdicts in _hold_cell(frame, form, device, monkeypatch):
        bad += problems
        for ok_max, ok_med, msg in verdicts.get(name, [(False, False, f"{frame}/{form}: no gradient for {name}")]):
            if not ok_max or (not ok_med and (frame, form, name) not in MEDIAN_AT_THE_BAR):
                bad.append(msg)
            elif not ok_med:
                median_only.append(msg)
    assert not bad, "\n".join(bad)
    if median_only:
        pytest.xfail("the median at its bar (MEDIAN_AT_THE_BAR): " + "; ".join(median_only))


@gpu
@pytest.mark.parametrize("variant", FORM_VARIANTS)
def test_the_frames_reach_the_backward_forms_the_path_matrix_reaches(variant, device, monkeypatch):
    """hgs_debug_stat("last_backward_forms") over this module's frames takes at least the values it takes over the path matrix's own
    frames under the same variant (one wave per tile / per quad, segmented, mixed, two launches; the per-Gaussian backward's row
    staging) -- a variant whose form no frame here reaches would be held to nothing."""
    want = {pm._path(frame, variant, device, monkeypatch)["backward_forms"] for frame in pm.FRAMES}
    got = {_run(frame, variant, device, monkeypatch)["backward_forms"] for frame in FRAMES}
    print(f"{variant}: backward forms of the path matrix {sorted(map(hex, want))}, of this module's frames {sorted(map(hex, got))}")
    assert want <= got, f"{variant}: no frame of this module reaches the backward form(s) {sorted(map(hex, want - got))}"
    if variant in CHECKPOINTED_VARIANTS:
        assert all(f & (BWD_SEGMENTED | BWD_MIXED) for f in got), f"{variant}: a frame whose backward left the checkpoints: {sorted(map(hex, got))}"
    else:
        assert not any(f & (BWD_SEGMENTED | BWD_MIXED) for f in got), f"{variant}: a frame whose backward took checkpoints: {sorted(map(hex, got))}"
