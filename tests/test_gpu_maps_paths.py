"""The alpha and depth maps (return_alpha_depth=True; csrc/maps.hip) on every rasterizer path and on the record another frame left.

The three map kernels compute nothing about the frame themselves: they read what a colour forward leaves in scratch -- the per-quad
compacted lists act / act_count, the splat records, final_T, n_contrib and the gate word n_total[1] -- and every one of those is
written by another kernel depending on the path the frame took: tile_sort_small<1|2|4|8>, the mid kernel or plan + parts + fallback
(binning.hip), the fused or the stand-alone sort + blend, the depth-parallel workers or one wave per quad (blend_fwd.h), a frame
enqueued once or again after a capacity, checkpoint or long-tile miss (hgs_api.hip).  tests/test_gpu_maps.py holds the maps to the
oracle on lists of at most 2 700 entries and on each frame's own record; here

  1. (no GPU) the six frames of tests/test_gpu_path_matrix.py between them put a list into every list kernel's bracket and walk it deep,
     and the fp32 reference the GPU is compared with lies within half of every bar of the fp64 one, under the upstreams the tests use;
  2. every (frame, variant) cell of the path matrix with the flag: maps and gradients against the oracle and against the default path;
  3. the stacked_512 sequence of tests/test_gpu_frame_sequences.py with the flag on every frame, hinted against cold, and through the
     C++ binding with the flag on every other frame.

References: the C oracle's render of colours (z, 1, 0) on black (tests/maps_ref.py), fp32, one per distinct frame at module scope.
Bars: test_gpu_parity's check_image on alpha and on depth / z_max, GRAD_REL_TOL per gradient tensor; against another GPU path the
maps are bit-equal wherever n_contrib is (the map passes walk one list front to back whatever produced it) and the gradients within
the variant's class bar (test_gpu_path_matrix.CLASS).  Every measured distance is printed (run with -s).

Measured on an MI355X, the worst over all variants; maps as max |d| of alpha, of depth / z_max, gradients as relative L2 (fp32 against
fp64 oracle from section 1 in brackets):
  frame                   maps against the oracle            gradients against the oracle   against the default path
  sparse_deep_stack       4.8e-7, 1.6e-7 (4.3e-6, 2.5e-6)    4.3e-7 (9.1e-6)                maps bit-equal, gradients 2.2e-7
  dense_with_stack        9.8e-5, 5.7e-5 (1.6e-3, 1.3e-3)    3.8e-6 (2.3e-4)                maps bit-equal, gradients 1.9e-6
  many_flat_long          6.6e-7, 3.4e-5 (1.1e-4, 1.7e-4)    1.0e-4 (3.4e-4)                maps bit-equal, gradients 8.6e-7
  even_and_full           7.8e-7, 1.0e-5 (3.5e-3, 2.7e-3)    5.5e-6 (2.1e-4)                maps bit-equal, gradients 2.5e-7
  ragged_sh_cov3D         4.8e-7, 4.8e-8 (5.7e-7, 1.0e-7)    7.3e-7 (6.3e-7)                maps bit-equal, gradients 6.2e-7
  ragged_colors_precomp   3.6e-7, 3.0e-8 (5.4e-7, 5.3e-8)    1.5e-6 (7.0e-7)                maps bit-equal, gradients 6.7e-7
n_contrib equals the default's on every pixel of every cell, the "split" class included; no pixel of a map beyond 1e-4 of the oracle's,
so the rule for a pixel on the other side of a threshold is never used.  stacked_512 with the flag: maps within 1.8e-4 / 3.4e-4 of the
oracle's (fp32 against fp64: 3.9e-3 / 3.5e-3), hinted against cold bit-equal, gradients 6.9e-6 apart at most; capacity re-runs at 0, 6, 9,
11, 14, 15, 17, the checkpoint re-run at 13, the repair at 5.  Taking turns with plain calls: the same frames, all three kinds.
(Before diff_gaussian_rasterization._remember carried the checkpoint-slot count from either binding's table to the other's, the turns
gave the repair at 5 AND 13 and the checkpoint re-run at 18: a flagged call reset the C++ node's count to 0, and a plain call left
the Python table's count two frames old.  test_calls_with_and_without_the_flag_take_turns_on_one_shape is the test that shows it.)

A per-quad list is shorter than its tile's: the longest of these frames holds fewer than 4 096 entries (the oracle counts at most 2 685
contributors in one quad of sparse_deep_stack), so entries_up_to with its count capped at 4 096 passes every test here and in
tests/test_gpu_maps.py -- nothing it walks is that long.  Mutations of maps.hip tried on a scratch build, with tests/test_gpu_maps.py
as it stood before this module run beside the default cells of section 2 and the hinted-against-cold test of section 3:
  * maps_forward_kernel returns early when n_total[3] is non-zero: five of the six default cells and the sequence test fail -- and so
    do 60 tests of tests/test_gpu_maps.py: n_total[3] is 1 on every sparse frame, and every small frame is sparse;
  * maps_forward_kernel returns early when n_total[6] is non-zero (the frame has a list beyond 4 096 entries):
    test_maps_in_every_cell_of_the_path_matrix[sparse_deep_stack-default] fails (alpha off by 0.9999: uninitialised memory) and
    test_maps_of_every_frame_of_the_sequence_equal_the_oracle_and_the_cold_twin fails already on the largest frame rendered first;
    tests/test_gpu_maps.py stays green;
  * entries_up_to caps its count at 2 660 (above the 2 658 entries of the longest list of tests/test_gpu_maps.py):
    test_maps_in_every_cell_of_the_path_matrix[sparse_deep_stack-default] fails (12 pixels of alpha beyond 1e-4);
    tests/test_gpu_maps.py stays green.
"""
import numpy as np
import pytest
import torch

from maps_ref import GEOMETRY_KEYS, map_upstreams, maps_reference, smooth_map_upstreams, summed
from test_gpu_frame_sequences import (GRAD_KEYS as SEQ_GRAD_KEYS, _Scene, _against_oracle, _bindings, _oracle_frame, _run_pass, _sequence,
                                      _show, predicted_capacity_reruns, sequence_stats)
from test_gpu_parity import (ALT_BACKWARD_TOL, COLOR_INLIER_FRAC, COLOR_TOL, GRAD_REL_TOL, check_image, gpu_settings, gpu_tensors,
                             order_tol, rel_l2, to_dev)
from test_gpu_maps import grads_of
from test_gpu_path_matrix import CLASS, FRAMES, GRAD_KEYS, VARIANTS, _forms, _oracle, _scene, _set_variant, grad_distance

gpu = pytest.mark.gpu   # (the tests of section 1 run on the CPU)

# ------------------------------------------------------------------------------------------------ references, once per distinct frame
_REF = {}


def _reference(kind, key, sc, upstreams, dtype):
    hit = _REF.get((kind, key, dtype))
    if hit is None:
        from oracle import hgs_oracle as ho
        ho.set_threads(ho.usable_cpus(), dtype)
        gA, gD = upstreams(sc["H"], sc["W"])
        hit = _REF[(kind, key, dtype)] = (gA, gD, maps_reference(sc, gA, gD, dtype=dtype))
    return hit


def frame_reference(frame, dtype=np.float32):
    """(gA, gD, maps_reference) of a frame of the path matrix under the noise upstreams"""
    return _reference("matrix", frame, _scene(frame), map_upstreams, dtype)


def sequence_reference(fr, dtype=np.float32):
    """(gA, gD, maps_reference) of a frame of a sequence (by its tag) under the smooth upstreams"""
    return _reference("sequence", fr["tag"], fr, smooth_map_upstreams, dtype)


def _stacked_frames():
    prime, seq = _sequence("stacked_512")
    return [prime] + list(seq)


# ------------------------------------------------------------------------------------------------ 1. the frames and the references
BRACKETS = ((1, 256), (257, 512), (513, 1024), (1025, 2048), (2049, 4096), (4097, 1 << 28))


def _lists(frame):
    f = frame_reference(frame)[2]["fwd"]
    return f["ranges"][:, 1].astype(np.int64) - f["ranges"][:, 0], f["n_contrib"].astype(np.int64)


def test_the_matrix_frames_reach_every_list_kernel_and_walk_the_lists_deep():
    """(no GPU needed) What the oracle says of the (z, 1, 0) render of the six frames: a list in each bracket between the producers'
    limits (tile_sort_small<1|2|4|8> up to 256 / 512 / 1 024 / 2 048 entries, the mid kernel up to 4 096, plan + parts beyond), and
    last contributors as deep as the lists are long -- a map pass that stopped early, or read a list one producer lays out otherwise,
    has pixels to show it."""
    seen = [0] * len(BRACKETS)
    for frame in FRAMES:
        lens, _ = _lists(frame)
        for b, (lo, hi) in enumerate(BRACKETS):
            seen[b] += int(((lens >= lo) & (lens <= hi)).sum())
    print("lists per bracket:", dict(zip(BRACKETS, seen)))
    assert all(seen), f"no list in bracket {BRACKETS[seen.index(0)]}"
    lens, nc = _lists("sparse_deep_stack")
    assert (int(lens.max()), int((lens > 4096).sum()), int(nc.max())) == (5727, 4, 5727)
    lens, nc = _lists("dense_with_stack")
    assert (len(lens), int((lens > 0).sum()), int(lens.max()), int(nc.max())) == (4624, 4624, 4079, 4079)
    lens, nc = _lists("many_flat_long")
    assert (int(lens.max()), int(nc.max())) == (2134, 617)
    lens, nc = _lists("even_and_full")
    assert (int(lens.max()), int(nc.max())) == (2318, 600)


def _reference_against_fp64(what, r32, r64):
    """the bars of the GPU tests, on the fp32 reference against the fp64 one: check_image, and half of GRAD_REL_TOL"""
    zm = r64["z_max"]
    worst = {}
    for name, a, b in (("alpha", r32["alpha"], r64["alpha"]), ("depth / z_max", r32["depth"] / zm, r64["depth"] / zm)):
        d = np.abs(a.astype(np.float64) - b)
        worst[name] = float(d.max())
        print(f"{what}: fp32 against fp64 oracle, {name}: max {d.max():.2e}, {float((d <= COLOR_TOL).mean()):.6f} within {COLOR_TOL}")
        check_image(a, b, f"{what} {name}, fp32 against fp64 oracle")
    for k in GEOMETRY_KEYS:
        b = r64["grads"][k]
        if not np.linalg.norm(b) > 0:
            continue   # (cov3D where the frame has scales + rotations, and the other way round: not an input)
        err = rel_l2(r32["grads"][k], b)
        worst[k] = err
        print(f"{what}: fp32 against fp64 oracle, grad {k} {err:.2e}")
        assert err <= GRAD_REL_TOL / 2, f"{what}: grad {k} of the fp32 oracle is {err:.3e} from the fp64 oracle's"
    return worst


@pytest.mark.parametrize("frame", list(FRAMES))
def test_the_matrix_references_hold_against_fp64(frame):
    """(no GPU needed) Noise upstreams (maps_ref.map_upstreams).  Observed over the six frames: at least 0.999976 of the pixels within
    1e-4, largest difference 3.5e-3 (a contributor within rounding of 1/255 taken in one precision only), gradients at most 3.4e-4."""
    _reference_against_fp64(frame, frame_reference(frame)[2], frame_reference(frame, np.float64)[2])


def test_the_sequence_references_hold_against_fp64():
    """(no GPU needed) stacked_512 under the smooth upstreams, every distinct frame.  This test licenses the choice: under the noise
    upstreams frame 7's gradients differ by 8.8e-4 between the two precisions (threshold pixels under a gradient whose sum nearly
    cancels), under the smooth ones by 4.2e-6; the worst frame under the smooth ones is 5 with 7.4e-5."""
    done = set()
    for i, fr in enumerate(_stacked_frames()):
        if fr["tag"] not in done:
            done.add(fr["tag"])
            _reference_against_fp64(f"stacked_512[{i - 1}]", sequence_reference(fr)[2], sequence_reference(fr, np.float64)[2])
    gA, gD = smooth_map_upstreams(512, 512)
    for g in (gA, gD):
        assert g.dtype == np.float32 and g.shape == (512, 512) and 0.1 <= g.min() < 0.15 and 0.95 < g.max() <= 1.0
    assert np.abs(gA - gD).max() > 0.5, "gA and gD must differ in phase"


# ------------------------------------------------------------------------------------------------ 2. every cell of the path matrix
_CELL = {}   # (frame, variant) -> what the cell's calls gave; the default's is what the others are compared with


def _own_state(fn, sc):
    """n_contrib (clamp flags masked off), the scan's decisions and the frame record, from the scratch and the state the function
    itself keeps for its backward -- not from a second render"""
    import diff_gaussian_rasterization as dgr
    lib = dgr._load()
    P, H, W = sc["means3D"].shape[0], sc["H"], sc["W"]
    buf, (_go, _gl, io, il, _bo, _bl) = fn.scratch
    image = buf[io:io + il]
    sub = lambda name, nbytes: image[lib.hgs_scratch_offset(name, P, fn.binning_capacity, H, W):][:nbytes].view(torch.int32)
    nt = sub(b"n_total", 64).cpu().numpy()
    st = fn.bw.state
    return (sub(b"n_contrib", 4 * H * W).view(H, W) & 0x0FFFFFFF).cpu().numpy(), \
        dict(sparse_frame=bool(st.sparse_frame), has_long_tiles=bool(st.has_long_tiles), ckpt_slots_used=int(st.ckpt_slots_used),
             ckpt_kind=int(nt[3]), long_from=int(nt[4]), deep_from=int(nt[8]))


def _run_cell(frame, variant, device, monkeypatch):
    """Under the variant: the frame without the flag, with it (what the shape's record then holds is this variant's own), with it again
    + backward of (alpha * gA).sum() + (depth * gD).sum(); on the default variant once more with the colour in the loss."""
    if (frame, variant) in _CELL:
        return _CELL[(frame, variant)]
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import GaussianRasterizer
    sc = _scene(frame)
    gA, gD, _ = frame_reference(frame)
    tA, tD = to_dev(gA, device), to_dev(gD, device)
    use_ckpt = dgr._USE_CKPT
    try:
        _set_variant(variant, monkeypatch)
        t = gpu_tensors(sc, device)
        rast = GaussianRasterizer(gpu_settings(sc, device))
        call = lambda **kw: rast(means3D=t["means3D"], means2D=t["means2D"], opacities=t["opacities"], shs=t["shs"],
                                 colors_precomp=t["colors_precomp"], scales=t["scales"], rotations=t["rotations"],
                                 cov3D_precomp=t["cov3D_precomp"], **kw)
        color0, radii0 = call()
        first = call(return_alpha_depth=True)
        color, radii, alpha, depth = call(return_alpha_depth=True)
        fwd_forms = _forms()[0]
        assert type(alpha.grad_fn).__name__.startswith("_RasterizeGaussiansMaps")
        for a, b in zip(first, (color, radii, alpha, depth)):
            assert torch.equal(a, b), f"{frame}/{variant}: the second call with the flag differs from the first"
        assert torch.equal(color, color0) and torch.equal(radii, radii0), f"{frame}/{variant}: the flag changed colour or radii"
        n_contrib, path = _own_state(alpha.grad_fn, sc)
        ((alpha[0] * tA).sum() + (depth[0] * tD).sum()).backward()
        torch.cuda.synchronize()
        path.update(forward_forms=fwd_forms, backward_forms=_forms()[1])
        out = dict(alpha=alpha.detach().cpu().numpy()[0], depth=depth.detach().cpu().numpy()[0], radii=radii.cpu().numpy(),
                   n_contrib=n_contrib, grads=grads_of(t), means2D_z=float(t["means2D"].grad[:, 2].abs().max()), path=path)
        if variant == "default":
            for v in t.values():
                if v is not None:
                    v.grad = None
            color, _, alpha, depth = call(return_alpha_depth=True)
            ((color * to_dev(sc["dL_dpix"], device)).sum() + (alpha[0] * tA).sum() + (depth[0] * tD).sum()).backward()
            torch.cuda.synchronize()
            out["color"], out["grads_summed"] = color.detach().cpu().numpy(), grads_of(t)
    finally:
        dgr._USE_CKPT = use_ckpt
        if dgr._cpp is not None:
            dgr._cpp.use_checkpoints(use_ckpt)
    _CELL[(frame, variant)] = out
    return out


def _grads_against_the_oracle(got, want, sc, flipped, what, colour_inputs=True):
    """every gradient within GRAD_REL_TOL by test_gpu_path_matrix.grad_distance (_check_against_oracle's rule for a pixel that took the
    other side of a threshold, here a pixel of a MAP beyond COLOR_TOL)"""
    worst = 0.0
    for name, rk in GRAD_KEYS:
        if sc.get(name) is None and name != "means2D" or not colour_inputs and name in ("shs", "colors_precomp"):
            continue
        assert name in got, f"{what}: no gradient for {name}"
        g, r = got[name], want[rk]
        assert np.isfinite(g).all(), f"{what}: non-finite gradient in {name}"
        g = g.reshape(r.shape)
        if flipped:
            print(f"{what}: grad {name} rel L2 {rel_l2(g, r):.2e} with every Gaussian ({flipped} pixels beyond {COLOR_TOL})")
        err = grad_distance(g, r, flipped)
        print(f"{what}: grad {name} rel L2 {err:.2e} against the oracle")
        worst = max(worst, err)
        assert err <= GRAD_REL_TOL, f"{what}: grad {name} rel L2 {err:.3e} against the oracle"
    return worst


def _maps_against_the_oracle(alpha, depth, ref, what):
    """check_image on alpha and on depth / z_max; returns (largest distances, pixels beyond COLOR_TOL on either map)"""
    assert alpha.shape == ref["alpha"].shape and depth.shape == ref["depth"].shape
    assert np.isfinite(alpha).all() and np.isfinite(depth).all(), f"{what}: non-finite map"
    zm = ref["z_max"]
    dA, dD = np.abs(alpha.astype(np.float64) - ref["alpha"]), np.abs(depth.astype(np.float64) - ref["depth"]) / zm
    flipped = int(((dA > COLOR_TOL) | (dD > COLOR_TOL)).sum())
    print(f"{what}: alpha max |d| {dA.max():.2e}, depth / z_max max |d| {dD.max():.2e} against the oracle, {flipped} pixels beyond {COLOR_TOL}")
    check_image(alpha, ref["alpha"], f"{what} alpha")
    check_image(depth / zm, ref["depth"] / zm, f"{what} depth / z_max")
    return (float(dA.max()), float(dD.max())), flipped


@gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("frame", list(FRAMES))
def test_maps_in_every_cell_of_the_path_matrix(frame, variant, device, monkeypatch):
    """One call with return_alpha_depth=True under the variant, one backward of (alpha * gA).sum() + (depth * gD).sum():
    colour and radii bit-equal to the call without the flag; maps and geometry gradients against the oracle; the colour inputs'
    gradients and dL/dmeans2D[:, 2] exactly zero; against the default variant's maps bit-equal on every pixel whose n_contrib -- read
    from the function's own scratch -- equals the default's (all of them for the classes "order" and "backward", COLOR_INLIER_FRAC of
    them for "split"), gradients within the class's bar.  On the default variant also colour . dL + alpha . gA + depth . gD against
    the sum of the oracle's two backward passes."""
    assert variant in CLASS, f"variant {variant} has no class in CLASS: say what it may change against the default"
    sc = _scene(frame)
    _, _, ref = frame_reference(frame)
    what = f"{frame}/{variant}"
    out = _run_cell(frame, variant, device, monkeypatch)
    assert np.array_equal(out["radii"], ref["fwd"]["radii"]), f"{what}: radii"
    _, flipped = _maps_against_the_oracle(out["alpha"], out["depth"], ref, what)
    mism = int((out["n_contrib"] != ref["fwd"]["n_contrib"]).sum())
    assert mism <= max(2, (1 - COLOR_INLIER_FRAC) * out["n_contrib"].size), f"{what}: n_contrib differs from the oracle's on {mism} pixels"
    _grads_against_the_oracle(out["grads"], ref["grads"], sc, flipped, what, colour_inputs=False)
    for k in ("shs", "colors_precomp"):
        if sc.get(k) is not None:
            assert k in out["grads"] and not out["grads"][k].any(), f"{what}: the maps gave {k} a gradient"
    assert out["means2D_z"] == 0.0, f"{what}: dL/dmeans2D[:, 2] is not zero"
    if variant == "default":
        cref, cgrads = _oracle(frame)
        check_image(out["color"], cref["color"], f"{what} colour")
        c_flipped = int((np.abs(out["color"].astype(np.float64) - cref["color"]) > COLOR_TOL).any(axis=0).sum())
        _grads_against_the_oracle(out["grads_summed"], summed(ref["grads"], cgrads), sc, flipped + c_flipped, f"{what}, colour + maps")
        return
    base, cls = _run_cell(frame, "default", device, monkeypatch), CLASS[variant]
    same = out["n_contrib"] == base["n_contrib"]
    print(f"{what}: n_contrib equals the default's on {float(same.mean()):.6f} of the pixels (class {cls})")
    if cls in ("order", "backward"):
        assert same.all(), f"{what}: n_contrib differs from the default's on {int((~same).sum())} pixels"
    else:
        assert float(same.mean()) >= COLOR_INLIER_FRAC, f"{what}: n_contrib equals the default's on {float(same.mean()):.6f} of the pixels only"
    for k in ("alpha", "depth"):
        d = np.abs(out[k].astype(np.float64) - base[k])
        print(f"{what}: {k} against the default's: max |d| {d.max():.2e}, {int((d[same] != 0).sum())} pixels of equal n_contrib differ")
        assert np.array_equal(out[k][same], base[k][same]), \
            f"{what}: {k} differs from the default's on {int((d[same] != 0).sum())} pixels of equal n_contrib, max {d[same].max():.3e}"
    for name in base["grads"]:
        bar = ALT_BACKWARD_TOL if cls == "split" else order_tol(name)
        err = rel_l2(out["grads"][name], base["grads"][name])
        print(f"{what}: grad {name} rel L2 {err:.2e} against the default's (bar {bar:g})")
        assert err <= bar, f"{what}: grad {name} rel L2 {err:.3e} against the default's (bar {bar:g}, class {cls})"


@gpu
@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "default"])
def test_the_flag_does_not_pin_the_frame_to_one_path(variant, device, monkeypatch):
    """What the call WITH the flag recorded -- the scan's decisions and the frame record in the function's own state, the host's launch
    forms -- differs from the default's on at least one frame, as test_every_variant_leaves_the_default_path_on_some_frame asks of
    the call without it."""
    for frame in FRAMES:
        a, b = _run_cell(frame, "default", device, monkeypatch)["path"], _run_cell(frame, variant, device, monkeypatch)["path"]
        if a != b:
            print(f"{variant} took effect on {frame}: {', '.join(f'{k} {a[k]} -> {b[k]}' for k in a if a[k] != b[k])}")
            return
    pytest.fail(f"{variant}: with the flag the path is the default's on every frame")


# ------------------------------------------------------------------------------------------------ 3. on the record another frame left
class _MapsScene(_Scene):
    """_Scene whose frames carry the flag where `flagged(position in the sequence; the priming frame is -1)` says so, under the
    smooth upstreams; the bookkeeping is _Scene.render's"""

    def __init__(self, base, device, flagged=lambda i: True):
        super().__init__(base, device)
        self.flagged, self.calls = flagged, 0
        self.upstreams = tuple(to_dev(g, device) for g in smooth_map_upstreams(base["H"], base["W"]))

    def render(self, fr, lib, cpp, backward=True):
        i = self.calls - 1
        self.calls += 1
        return super().render(fr, lib, cpp, backward, maps=self.upstreams if self.flagged(i) else None)

    def run(self, frames, lib, cpp, dgr, hinted, monkeypatch):
        self.calls = 0
        return _run_pass(self, frames, lib, cpp, dgr, hinted, monkeypatch)

    def prefill(self, lib, cpp):
        """the largest frame of the sequence with the flag, its outputs let go: blocks the caching allocator MAY hand the next
        frames' maps (nothing here checks that it does; the assertion is the comparison with the oracle on every frame)"""
        st = sequence_stats("stacked_512")
        big = _sequence("stacked_512")[1][max(range(len(st)), key=lambda i: st[i]["N"])]
        rec = super().render(big, lib, cpp, maps=self.upstreams)[0]
        assert float(rec["alpha"].min()) > 0.5 and float(rec["depth"].min()) > 0.0   # (every pixel covered: nothing of it looks like an empty map)
        del rec
        torch.cuda.synchronize()


_SUMMED = {}


def _summed_oracle(fr):
    """the colour oracle's record of the frame with the maps' gradients added (tests/maps_ref.summed, on the sequence tests' keys)"""
    if fr["tag"] not in _SUMMED:
        hit, mg = _oracle_frame(fr), sequence_reference(fr)[2]["grads"]
        _SUMMED[fr["tag"]] = dict(hit, grads={k: hit["grads"][k] + mg[k].reshape(hit["grads"][k].shape) if k in mg else hit["grads"][k]
                                              for k in SEQ_GRAD_KEYS})
    return _SUMMED[fr["tag"]]


def _frame_against_oracle(problems, what, fr, res):
    """radii, N, image and gradients by test_gpu_frame_sequences._against_oracle (the summed gradients where the frame had the flag),
    the maps by check_image"""
    rec, img, radii, grads = res
    flagged = "alpha" in rec
    _against_oracle(problems, what, _summed_oracle(fr) if flagged else _oracle_frame(fr), img, radii, grads, rec["N"])
    if flagged:
        try:
            _maps_against_the_oracle(rec["alpha"].cpu().numpy()[0], rec["depth"].cpu().numpy()[0], sequence_reference(fr)[2], what)
        except AssertionError as e:
            problems.append(str(e))


@gpu
def test_maps_of_every_frame_of_the_sequence_equal_the_oracle_and_the_cold_twin(device, monkeypatch):
    """stacked_512 (the priming frame and its 19 frames, one shape) with return_alpha_depth=True on every frame, loss colour + alpha +
    depth under the smooth upstreams, on the records the frame before left; then the same frames without any guess.  Maps, colour and
    radii bit-equal between the two; gradients within order_tol (ALT_BACKWARD_TOL where another backward form ran); every frame against
    the oracle.  The misses happen under the flag where they do without it: capacity re-runs on the frames the oracle's N predicts, the
    checkpoint re-run at frame 13, the long-tile repair at frame 5 -- so the gate n_total[1] and the lists a re-run or a repair leaves
    are what the map passes read on those frames.
    The maps are allocated with torch.empty, and a map pass that returns at the gate leaves them as they come.  So the largest frame is
    rendered first and let go: blocks the allocator hands out afterwards may hold ITS maps (no guarantee: the allocator decides), and
    no pixel of a later frame may keep them -- which the comparison with the oracle on every frame already says; the order only makes
    it less likely that stale memory is right by luck."""
    dgr, lib, cpp = _bindings("cpp", monkeypatch)
    frames = _stacked_frames()
    scene = _MapsScene(frames[1], device)
    scene.prefill(lib, cpp)
    hot = scene.run(frames, lib, cpp, dgr, True, monkeypatch)
    scene.prefill(lib, cpp)
    cold = scene.run(frames, lib, cpp, dgr, False, monkeypatch)
    problems, seen = [], dict(over=[], ckpt=[], repair=[])
    for i, fr in enumerate(frames):
        (h, h_img, h_radii, h_g), (c, c_img, c_radii, c_g) = hot[i], cold[i]
        same_bwd = h["bwd_forms"] == c["bwd_forms"]
        errs = {k: rel_l2(h_g[k].cpu().numpy(), c_g[k].cpu().numpy()) for k in SEQ_GRAD_KEYS}
        _show("stacked_512", i - 1, h, f"| cold: fwd {c['fwd_forms']:#05x} bwd {c['bwd_forms']:#06x} worst grad diff {max(errs.values()):.2e} "
                                     f"({max(errs, key=errs.get)})")
        _frame_against_oracle(problems, f"stacked_512[{i - 1}]", fr, hot[i])
        for k, a, b in (("alpha", h["alpha"], c["alpha"]), ("depth", h["depth"], c["depth"]), ("image", h_img, c_img), ("radii", h_radii, c_radii)):
            if not torch.equal(a, b):
                problems.append(f"stacked_512[{i - 1}]: {k} not bit-equal to the cold render's: {int((a != b).sum())} elements, "
                                f"max |d| {float((a - b).abs().max()):.3e}")
        for k in SEQ_GRAD_KEYS:
            tol = order_tol(k) if same_bwd else ALT_BACKWARD_TOL
            if not errs[k] <= tol:
                problems.append(f"stacked_512[{i - 1}]: grad {k} differs from the cold render's by {errs[k]:.3e} > {tol} (same backward form: {same_bwd})")
        if c["binning_reruns"] or c["ckpt_reruns"] or c["long_repair"] or c["capacity"] != c["N"]:
            problems.append(f"stacked_512[{i - 1}]: the cold render ran on a guess")
        if i:
            seen["over"] += [i - 1] * h["binning_reruns"]
            seen["ckpt"] += [i - 1] * h["ckpt_reruns"]
            seen["repair"] += [i - 1] if h["long_repair"] else []
    print(f"stacked_512 with the flag: observed {seen}, predicted capacity re-runs {predicted_capacity_reruns('stacked_512')}")
    assert not problems, "\n".join(problems)
    assert seen["over"] == predicted_capacity_reruns("stacked_512"), "capacity re-runs: not on the frames the oracle's N predicts"
    assert seen["ckpt"] == [13] and seen["repair"] == [5], "the sequence must meet both repairs under the flag"


@gpu
def test_calls_with_and_without_the_flag_take_turns_on_one_shape(device, monkeypatch):
    """stacked_512 through the C++ binding, the frames at even positions with the flag -- they go through the ctypes function and teach
    the C++ node's table through _remember(..., to_cpp=True) --, those at odd positions (and the priming frame) without -- the C++ node
    runs them and teaches the Python tables: every frame against the oracle, and capacity re-runs, the checkpoint re-run and the
    long-tile repair on the frames they fall on with one kind of call only (frames 13 and 5), which holds the two tables to one
    another across the two kinds of call -- the checkpoint-slot count included, which neither used to hand to the other."""
    dgr, lib, cpp = _bindings("cpp", monkeypatch)
    frames = _stacked_frames()
    scene = _MapsScene(frames[1], device, flagged=lambda i: i >= 0 and i % 2 == 0)
    scene.prefill(lib, cpp)
    res = scene.run(frames, lib, cpp, dgr, True, monkeypatch)
    problems, seen = [], dict(over=[], ckpt=[], repair=[])
    for i, fr in enumerate(frames):
        rec = res[i][0]
        assert ("alpha" in rec) == (i >= 1 and (i - 1) % 2 == 0)
        _show("stacked_512", i - 1, rec, "| with the flag" if "alpha" in rec else "")
        _frame_against_oracle(problems, f"stacked_512[{i - 1}], taking turns", fr, res[i])
        if i:
            seen["over"] += [i - 1] * rec["binning_reruns"]
            seen["ckpt"] += [i - 1] * rec["ckpt_reruns"]
            seen["repair"] += [i - 1] if rec["long_repair"] else []
    print(f"stacked_512 taking turns: observed {seen}, predicted capacity re-runs {predicted_capacity_reruns('stacked_512')}")
    assert not problems, "\n".join(problems)
    assert seen["over"] == predicted_capacity_reruns("stacked_512"), "capacity re-runs: not on the frames the oracle's N predicts"
    assert seen["ckpt"] == [13] and seen["repair"] == [5], "a checkpoint re-run or a long-tile repair on another frame than with one kind of call"
