"""Sequences of DIFFERENT frames on one shape, every frame against the oracle (missing #1 / weak #6).

Every frame is launched from what three records remember of the previous frame of its (device, P, H, W): the Python binding's
tables, the C++ node's g_hints and the library's FrameHistory.  hgs_common.h: "launch-size hints only -- results never depend on
them".  The other GPU modules render each frame from its OWN history; here frame B runs on the record frame A really left, for
frames that differ in N, in non-empty tiles, in long / huge lists and in the frame's kind at once -- the access pattern of a trainer
that draws another capture frame every step.

  stacked_512   35 000 Gaussians at 512 x 512: a core stacked into a few tiles in front of a background; yaw pans the core out of
                view, shifts along the view axis and scale_modifier 0.3 .. 2.4 swing N by two orders of magnitude
  c2_cameras    the benchmark's 200 000-Gaussian scene at 1920 x 1080 from eight seeded cameras (yaw +-20 deg, pitch +-8 deg,
                +-1.5 units): non-empty tiles on both sides of NO_CKPT_MIN_TILES, frames of both kinds

The unmarked tests check on the CPU (C oracle, binning only) that the sequences contain the transitions they are there for.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import hgs_oracle as ho
from scenes import oracle_inputs
from test_gpu_parity import (ALT_BACKWARD_TOL, GRAD_REL_TOL, _force_ctypes_binding, _stacked_scene, check_image, gpu_settings,
                             gpu_tensors, order_tol, rel_l2, to_dev)

gpu = pytest.mark.gpu   # (the tests that only check the constructions run on the CPU)

GRAD_KEYS = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")
SORT_CAP_SMALL, SORT_CAP_MID, LONG_EVERY_RULE = 2048, 4096, 1024   # binning.hip; beyond 1 024 entries a list is long under every rule but the deep-sparse one
NO_CKPT_MIN_TILES = 7168
FWD_LONG_REPAIR, FWD_DEEP_WORKERS = 1 << 5, 1 << 8                 # hgs_common.h
CORE = 5000                                                        # Gaussians of the stacked core (the first rows of stacked_512)

# (yaw in degrees, camera shift along the view axis, scale_modifier) -- one shape throughout
STACKED_DESIGN = [(0, 0, 1.0), (0, 0, 1.0), (-50, 0, 2.2), (3, 0.5, 0.5), (50, 0, 0.5), (0, 5.0, 0.2), (0, 0, 0.6), (50, 0, 1.6), (0, 0, 0.4),
                  (-4, 0, 1.0), (2, 3.0, 0.45), (0, -1.0, 1.9), (50, 0, 0.5), (0, 4.0, 0.3), (0, 0, 1.0), (1, 2.5, 2.2), (55, 1.0, 0.4),
                  (0, -1.0, 2.4), (0, 0, 1.0)]
STACKED_PRIME = (55, 1.0, 0.4)    # rendered once before frame 0: what the three records hold when the sequence begins
C2_SEED, C2_CAMERAS = 0, 8
WORKER_CAP_FRAME = 7               # stacked_512: 4 long lists before it, 317 on it (what the scan counts: lists beyond 256 entries of a deep sparse frame)


def _w2c(yaw_deg, pitch_deg=0.0, shift=(0.0, 0.0, 0.0)):
    y, p = math.radians(yaw_deg), math.radians(pitch_deg)
    ry = np.array([[math.cos(y), 0, math.sin(y)], [0, 1, 0], [-math.sin(y), 0, math.cos(y)]])
    rx = np.array([[1, 0, 0], [0, math.cos(p), -math.sin(p)], [0, math.sin(p), math.cos(p)]])
    m = np.eye(4)
    m[:3, :3] = rx @ ry
    m[:3, 3] = shift
    return m


def _frame(base, w2c, mod, tag=None):
    """the base scene seen from another camera with another scale_modifier (the Gaussians are shared)"""
    from hugs_amd import synthetic as syn
    f = dict(base)
    f["cam"] = syn.camera_from_w2c(w2c, base["cam"]["fovx"], base["cam"]["fovy"], base["H"], base["W"])
    f["scale_modifier"] = float(mod)
    f["tag"] = tag
    return f


@functools.lru_cache(maxsize=None)
def _stacked_base():
    from hugs_amd import synthetic as syn
    sc = _stacked_scene(CORE, 512, 512, seed=31, spread_px=8.0)
    bgd = syn.scene_gaussians(30000, sc["cam"], seed=32, sigma_px=3.0)
    for k in ("means3D", "scales", "rotations", "opacities", "shs"):
        sc[k] = np.concatenate([sc[k], np.asarray(bgd[k], np.float32).reshape((-1,) + sc[k].shape[1:])], 0)
    return sc


@functools.lru_cache(maxsize=None)
def _core_base():
    """the core alone at 256 x 256: the human-only frame that takes turns with the joint one"""
    full = _stacked_base()
    sc = _stacked_scene(1, 256, 256, seed=33, spread_px=8.0)     # (camera, settings and dL/dpixel of the other shape)
    for k in ("means3D", "scales", "rotations", "opacities", "shs"):
        sc[k] = np.ascontiguousarray(full[k][:CORE])
    return sc


@functools.lru_cache(maxsize=None)
def _c2_base():
    from hugs_amd import synthetic as syn
    H, W = 1080, 1920
    cam = syn.pinhole_camera(H, W)
    g = syn.scene_gaussians(200_000, cam, seed=0, sigma_px=4.0)
    sc = dict(means3D=g["means3D"], scales=g["scales"], rotations=g["rotations"], opacities=g["opacities"], shs=g["shs"],
              colors_precomp=None, cov3D_precomp=None, cam=cam, H=H, W=W, D=3, M=16, bg=np.ones(3, np.float32), scale_modifier=1.0,
              tanfovx=math.tan(cam["fovx"] * 0.5), tanfovy=math.tan(cam["fovy"] * 0.5))
    sc["dL_dpix"] = syn.pixel_grad(H, W) * np.float32(3 * H * W)
    return sc


def _design_frames(base, design, name):
    return [_frame(base, _w2c(yaw, 0.0, (0.0, 0.0, dz)), mod, f"{name}:{yaw}:{dz}:{mod}") for yaw, dz, mod in design]


@functools.lru_cache(maxsize=None)
def _sequence(name):
    """(priming frame, [frames])"""
    if name == "stacked_512":
        return _design_frames(_stacked_base(), [STACKED_PRIME], name)[0], _design_frames(_stacked_base(), STACKED_DESIGN, name)
    if name == "core_256":
        return _design_frames(_core_base(), [STACKED_PRIME], name)[0], _design_frames(_core_base(), STACKED_DESIGN, name)
    assert name == "c2_cameras"
    base, rng, cams = _c2_base(), np.random.default_rng(C2_SEED), []
    for i in range(C2_CAMERAS):
        yaw, pitch, shift = rng.uniform(-20, 20), rng.uniform(-8, 8), rng.uniform(-1.5, 1.5, 3)
        cams.append(_frame(base, _w2c(yaw, pitch, shift), 1.0, f"{name}:{C2_SEED}:{i}"))
    frames = [{**cams[i], "scale_modifier": mod, "tag": f"{cams[i]['tag']}:{mod}"} for i, mod in C2_DESIGN]
    return _frame(base, np.eye(4), 1.0, f"{name}:identity"), frames


# (camera, scale_modifier): camera 0 as the benchmark renders it at the start, in the middle and at the end; larger splats make the
# lists deep enough for the frame rule (binning.hip, frame_is_sparse) to call a 1080p frame sparse
C2_DESIGN = [(0, 1.0), (4, 3.2), (2, 3.2), (1, 1.0), (0, 1.0), (3, 3.2), (5, 2.6), (7, 1.0), (6, 2.6), (0, 1.0)]


def _stats(fr):
    ref = ho.forward(oracle_inputs(fr), stop_after="binning")
    lens = ref["ranges"][:, 1].astype(np.int64) - ref["ranges"][:, 0]
    return dict(N=int(ref["N"]), nonempty=int((lens > 0).sum()), longest=int(lens.max()), n1024=int((lens > LONG_EVERY_RULE).sum()),
                n2048=int((lens > SORT_CAP_SMALL).sum()), n4096=int((lens > SORT_CAP_MID).sum()))


@functools.lru_cache(maxsize=None)
def sequence_stats(name):
    ho.set_threads(ho.usable_cpus())
    return [_stats(fr) for fr in _sequence(name)[1]]


def _overflows(n_prev, n):
    import diff_gaussian_rasterization as dgr
    return n > dgr._round_capacity(n_prev)


def transitions(name):
    """frames i >= 1 of the sequence whose step from frame i - 1 is of each kind the contract is tested on"""
    st = sequence_stats(name)
    idx = range(1, len(st))
    over = [i for i in idx if _overflows(st[i - 1]["N"], st[i]["N"])]
    fits = [i for i in idx if i not in over]
    return dict(
        overflow=over, fits=fits,
        long_appears=[i for i in idx if st[i]["n2048"] and not st[i - 1]["n2048"]],
        long_appears_fitting=[i for i in fits if st[i]["n2048"] and not st[i - 1]["n2048"]],
        long_disappears=[i for i in idx if not st[i]["n2048"] and st[i - 1]["n2048"]],
        huge_appears_fitting=[i for i in fits if st[i]["n4096"] and not st[i - 1]["n4096"]],
        worker_cap_fitting=[i for i in fits if st[i]["n1024"] > 5 * st[i - 1]["n1024"] + 64],
        across_no_ckpt=[i for i in idx if (st[i]["nonempty"] >= NO_CKPT_MIN_TILES) != (st[i - 1]["nonempty"] >= NO_CKPT_MIN_TILES)])


def _repeats(name):
    """{tag: [positions]} of the frames that occur more than once"""
    at = {}
    for i, fr in enumerate(_sequence(name)[1]):
        at.setdefault(fr["tag"], []).append(i)
    return {k: v for k, v in at.items() if len(v) > 1}


def predicted_capacity_reruns(name, order=None):
    """frames (positions in the rendered order, the priming frame in front of them) that overflow the capacity their predecessor leaves"""
    prime, _ = _sequence(name)
    st = sequence_stats(name)
    ns = [_stats(prime)["N"]] + [st[i]["N"] for i in (order if order is not None else range(len(st)))]
    return [i - 1 for i in range(1, len(ns)) if _overflows(ns[i - 1], ns[i])]


# ------------------------------------------------------------------------------------------------ 1. the sequences are what they say
def test_the_stacked_sequence_is_what_it_says():
    """(no GPU needed) What the C oracle says of the 19 frames, by position -- a frame taken out or moved fails this test:
      N overflows round_capacity(N of the frame before) at 6, 9, 11, 14, 15, 17 (and at frame 0, after the priming frame); the other
      twelve frames run to the end on a stale record;
      lists beyond 2 048 entries appear at 5, 8, 13 (the capacity fits: no re-run hides the wrong guess) and 17, disappear at 4, 7, 12, 16;
      a list beyond 4 096 entries appears at 5, 10 and 13 on a frame that fits: 10 follows a frame WITH long lists, so nothing but the
      library's stale n_huge == 0 decides whether the plan kernel is launched;
      lists beyond 1 024 entries grow from 4 to 280 at frame 2 and from 4 to 201 at frame 7 (more than 5 n + 64 = 84: the worker cap)
      on frames that fit;
      non-empty tiles 292 .. 1 024; the frame (0, 0, 1.0) stands at 0, 1, 14 and 18 behind four different predecessors."""
    st, tr = sequence_stats("stacked_512"), transitions("stacked_512")
    assert len(st) == len(STACKED_DESIGN) == 19
    assert tr["overflow"] == [6, 9, 11, 14, 15, 17] and len(tr["overflow"]) >= 4
    assert tr["fits"] == [1, 2, 3, 4, 5, 7, 8, 10, 12, 13, 16, 18] and len(tr["fits"]) >= 4
    assert predicted_capacity_reruns("stacked_512") == [0] + tr["overflow"]
    assert tr["long_appears"] == [5, 8, 13, 17] and tr["long_appears_fitting"] == [5, 8, 13] and tr["long_disappears"] == [4, 7, 12, 16]
    assert tr["huge_appears_fitting"] == [5, 10, 13] and st[9]["n2048"] > 0 and st[9]["n4096"] == 0 and st[10]["N"] < st[9]["N"]
    assert tr["worker_cap_fitting"] == [2, WORKER_CAP_FRAME]
    assert (st[1]["n1024"], st[2]["n1024"]) == (4, 280) and (st[WORKER_CAP_FRAME - 1]["n1024"], st[WORKER_CAP_FRAME]["n1024"]) == (4, 201)
    tiles = [s["nonempty"] for s in st]
    assert min(tiles) == 292 and max(tiles) == 1024 and max(tiles) >= 3 * min(tiles)
    assert min(s["N"] for s in st) == 35_911 and max(s["N"] for s in st) == 3_499_600 and max(s["longest"] for s in st) == 7_563
    assert list(_repeats("stacked_512").values()) == [[0, 1, 14, 18], [4, 12]]
    # the deferred frames of test_deferred_frames_...: only the smallest frame is on record when the first frame beyond 2 000 000 entries arrives
    import diff_gaussian_rasterization as dgr
    order = _deferred_order()
    assert st[order[0]]["N"] == 35_911 and dgr._deferred_capacity(35_911, 512, 512) == 262_144 and st[order[1]]["N"] > 2_000_000


def test_the_camera_sequence_is_what_it_says():
    """(no GPU needed) The benchmark's scene from eight seeded cameras, camera 0 as the benchmark renders it at positions 0, 4 and 9,
    five of the others with scale_modifier 2.6 / 3.2: N 1 205 099 .. 7 408 292, non-empty tiles 5 741 .. 8 160; the capacity overflows
    at 1, 4, 5 and 8, five frames fit; consecutive frames stand on either side of NO_CKPT_MIN_TILES at 1 and 4."""
    st, tr = sequence_stats("c2_cameras"), transitions("c2_cameras")
    assert len(st) == 10 and list(_repeats("c2_cameras").values()) == [[0, 4, 9]]
    assert sorted({cam for cam, _ in C2_DESIGN}) == list(range(C2_CAMERAS))
    assert tr["overflow"] == [1, 4, 5, 8] and tr["fits"] == [2, 3, 6, 7, 9]
    assert predicted_capacity_reruns("c2_cameras") == tr["overflow"]          # (the priming frame is the benchmark's own: it leaves room for frame 0)
    assert tr["across_no_ckpt"] == [1, 4]
    assert (min(s["N"] for s in st), max(s["N"] for s in st)) == (1_205_099, 7_408_292)
    assert (min(s["nonempty"] for s in st), max(s["nonempty"] for s in st)) == (5_741, 8_160)


def test_the_core_sequence_moves_in_and_out_of_view():
    """(no GPU needed) the human-only frames that take turns with stacked_512: four tiles deep when in view, nothing at all at yaw +-50 / 55"""
    st = sequence_stats("core_256")
    assert [i for i, s in enumerate(st) if s["N"] == 0] == [2, 4, 7, 12, 16]
    assert max(s["longest"] for s in st) == 5000 and sum(1 for s in st if s["n4096"]) >= 4


def _deferred_order():
    """stacked_512 with the smallest frame first and the largest right behind it"""
    small, big = STACKED_DESIGN.index((55, 1.0, 0.4)), STACKED_DESIGN.index((0, -1.0, 2.4))
    return [small, big] + [i for i in range(len(STACKED_DESIGN)) if i not in (small, big)]


# ------------------------------------------------------------------------------------------------ GPU side
_ORACLE = {}
_ORACLE_SECONDS = [0.0]   # what the module spends in the C oracle (printed: run with -s)


def _oracle_frame(fr, with_lists=False):
    """forward + backward of the C oracle for one frame, kept per distinct frame (both bindings, every order ask for the same ones)"""
    hit = _ORACLE.get(fr["tag"])
    if hit is None or (with_lists and "values" not in hit):
        import time
        t0 = time.perf_counter()
        ho.set_threads(ho.usable_cpus())
        inp = oracle_inputs(fr)
        ref = ho.forward(inp)
        g = ho.backward(inp, ref, fr["dL_dpix"])
        _ORACLE_SECONDS[0] += time.perf_counter() - t0
        print(f"  (oracle, {fr['tag']}: {time.perf_counter() - t0:.2f} s, {_ORACLE_SECONDS[0]:.1f} s so far)")
        hit = dict(N=int(ref["N"]), radii=ref["radii"], color=ref["color"], grads={k: g[k] for k in GRAD_KEYS})
        if with_lists:
            hit["values"], hit["ranges"] = ref["values"], ref["ranges"]
        _ORACLE[fr["tag"]] = hit
    return hit


def _bindings(binding, monkeypatch):
    """(dgr, lib, cpp or None): the calls of this test go through the named binding, hints on"""
    import diff_gaussian_rasterization as dgr
    lib = dgr._load()
    monkeypatch.setattr(dgr, "_CPP_WANTED", True)          # (also when the suite runs with HGS_BINDING=ctypes)
    cpp = dgr._load_cpp()
    assert cpp is not None, "lib/_hgs_torch.so is missing: __graft_entry__.build() makes it"
    cpp.clear_hints()
    cpp.use_hints(True)
    monkeypatch.setattr(dgr, "_USE_HINT", True)
    if binding == "ctypes":
        _force_ctypes_binding(monkeypatch)
        cpp = None
    return dgr, lib, cpp


def _forget(dgr, device, *shapes):
    """empty the bindings' records of these (P, H, W)"""
    real = dgr._load_cpp() if dgr._CPP_WANTED else None
    if real is not None:
        real.clear_hints()
    for P, H, W in shapes:
        key = (torch.device(device).index or 0, P, H, W)
        for table in (dgr._last_num_rendered, dgr._max_num_rendered, dgr._last_sparse, dgr._last_ckpt_used):
            table.pop(key, None)


def _shape(fr):
    return fr["means3D"].shape[0], fr["H"], fr["W"]


class _Scene:
    """the Gaussians of a base scene on the device, once; every frame makes fresh leaves of them"""

    def __init__(self, base, device, second_from=None):
        self.device, self.cut = device, second_from
        self.t = {k: to_dev(base[k], device) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
        self.dL = to_dev(base["dL_dpix"], device)

    def render(self, fr, lib, cpp, backward=True, maps=None):
        """one frame through GaussianRasterizer [+ backward]: (record of what ran, image, radii, {gradients})
        maps=(gA, gD), device tensors [H, W]: the call has return_alpha_depth=True -- it then goes through the ctypes function whatever
        the binding --, the loss gains (alpha * gA).sum() + (depth * gD).sum(), and the record the two maps (tests/test_gpu_maps_paths.py)"""
        from diff_gaussian_rasterization import GaussianRasterizer
        stat = lambda k: lib.hgs_debug_stat(k.encode())
        before = stat("binning_reruns"), stat("ckpt_reruns")
        P = self.t["means3D"].shape[0]
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in self.t.items()}
        means2D = torch.zeros(P, 3, device=self.device, requires_grad=True)
        rast = GaussianRasterizer(gpu_settings(fr, self.device))
        flag = dict(return_alpha_depth=True) if maps is not None else {}
        if self.cut is None:
            color, radii, *ad = rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"], shs=leaves["shs"],
                                     scales=leaves["scales"], rotations=leaves["rotations"], **flag)
        else:   # the rows from `cut` on first, the rows before it as the second set (hgs_segment): the caller's frame has them in that order
            a = {k: v.detach()[self.cut:].clone().requires_grad_(True) for k, v in self.t.items()}
            b = {k: v.detach()[:self.cut].clone().requires_grad_(True) for k, v in self.t.items()}
            color, radii, *ad = rast(means3D=a["means3D"], means2D=means2D, opacities=a["opacities"], shs=a["shs"], scales=a["scales"],
                                     rotations=a["rotations"], second=b, **flag)
        assert len(ad) == (2 if maps is not None else 0)
        rec = dict(fwd_forms=int(stat("last_forward_forms")))
        if maps is not None:
            rec["alpha"], rec["depth"] = ad[0].detach(), ad[1].detach()
        if cpp is not None and maps is None:
            assert color.grad_fn is None or color.grad_fn.name() == "HgsRasterizeBackward"
            rec["N"], rec["capacity"], rec["has_long"], rec["sparse"] = cpp.last_frame_info()
            rec["ckpt_bytes"], rec["ckpt_used"] = cpp.last_ckpt_info()
        else:
            assert "_RasterizeGaussians" in color.grad_fn.name()
            s = color.grad_fn.bw.state
            rec.update(N=int(s.num_rendered), capacity=int(s.binning_capacity), has_long=bool(s.has_long_tiles), sparse=bool(s.sparse_frame),
                       ckpt_bytes=int(s.ckpt_bytes), ckpt_used=int(s.ckpt_slots_used))
        grads = {}
        if backward:
            if maps is None:
                color.backward(self.dL)
            else:
                ((color * self.dL).sum() + (ad[0][0] * maps[0]).sum() + (ad[1][0] * maps[1]).sum()).backward()
            torch.cuda.synchronize()
            rec["bwd_forms"] = int(stat("last_backward_forms"))
            if self.cut is None:
                grads = {k: leaves[k].grad for k in leaves}
            else:
                grads = {k: torch.cat([a[k].grad, b[k].grad], 0) for k in a}
            grads["means2D"] = means2D.grad
        torch.cuda.synchronize()
        rec["binning_reruns"], rec["ckpt_reruns"] = stat("binning_reruns") - before[0], stat("ckpt_reruns") - before[1]
        rec["long_repair"] = bool(rec["fwd_forms"] & FWD_LONG_REPAIR)
        return rec, color.detach(), radii, grads


def _against_oracle(problems, what, ref, image, radii, grads, N):
    """the bars of test_backward_gradients: radii and N exactly, image by check_image, every leaf gradient within GRAD_REL_TOL"""
    if N != ref["N"]:
        problems.append(f"{what}: N {N} != {ref['N']}")
    if not np.array_equal(radii.cpu().numpy(), ref["radii"]):
        problems.append(f"{what}: radii differ from the oracle's")
    try:
        check_image(image.cpu().numpy(), ref["color"], what)
    except AssertionError as e:
        problems.append(str(e))
    for k in GRAD_KEYS:
        if k in grads:
            g, r = grads[k].cpu().numpy(), ref["grads"][k]
            err = rel_l2(g.reshape(r.shape), r) if np.isfinite(g).all() else float("inf")
            if not err <= GRAD_REL_TOL:
                problems.append(f"{what}: grad {k} rel L2 err {err:.3e} against the oracle")


def _run_pass(scene, frames, lib, cpp, dgr, hinted, monkeypatch):
    """prime + frames in order from empty records; hinted=False: no capacity / long-tile / checkpoint-slot guess from either binding"""
    _forget(dgr, scene.device, _shape(frames[0]))
    real = dgr._load_cpp() if dgr._CPP_WANTED else None
    out = []
    try:
        if real is not None:
            real.use_hints(hinted)
        monkeypatch.setattr(dgr, "_USE_HINT", hinted)
        for fr in frames:
            out.append(scene.render(fr, lib, cpp))
    finally:
        if real is not None:
            real.use_hints(True)
        monkeypatch.setattr(dgr, "_USE_HINT", True)
    return out


def _show(name, i, rec, extra=""):
    print(f"  {name}[{i:2d}] N {rec['N']:8d} cap {rec['capacity']:8d} sparse {int(rec['sparse'])} long {int(rec['has_long'])} ckpt_used {rec['ckpt_used']:6d} "
          f"ckpt_bytes {rec['ckpt_bytes']:10d} fwd {rec['fwd_forms']:#05x} bwd {rec.get('bwd_forms', 0):#06x} reruns {rec['binning_reruns']}/{rec['ckpt_reruns']} "
          f"repair {int(rec['long_repair'])} {extra}")


@gpu
@pytest.mark.parametrize("name", ["stacked_512", "c2_cameras"])
@pytest.mark.parametrize("binding", ["cpp", "ctypes"])
def test_every_frame_of_a_sequence_equals_the_oracle_and_its_cold_twin(binding, name, device, monkeypatch):
    """Every frame of the sequence, forward + backward, on the records its predecessor left (hints on, one stream): radii and N equal
    to the oracle's, image and gradients within the bars of test_backward_gradients.  Then the same frames without any guess from the
    binding: image and radii of the two renders bit-equal, gradients within order_tol where the same backward form ran
    and ALT_BACKWARD_TOL where another did.  The misses are proved: capacity re-runs on exactly the frames the oracle's N predicts, the
    long-tile repair and the checkpoint re-run on exactly the frames the cold pass's reports predict.
    stacked_512 (always sparse: a frame under 1 536 tiles is, whatever its lists): the repair runs at frame 5 (long lists behind a frame
    without), the checkpoint re-run at frame 13; seven frames run on a stale has_long_tiles.  c2_cameras: frames of both kinds, each
    behind the other; a dense frame that keeps the checkpoint buffer its sparse predecessor earned it takes another backward form than
    its cold twin, which knows the frame is dense before it is enqueued.
    Observed on an MI355X, the same through both bindings -- stacked_512: 7 capacity re-runs (frames 0, 6, 9, 11, 14, 15, 17), 1 checkpoint
    re-run (13), 1 long-tile repair (5), no frame with another backward form; c2_cameras: 4 capacity re-runs (1, 4, 5, 8), no checkpoint
    re-run, no repair, 6 frames behind a frame of the other kind, frame 3 with blend_backward_mixed_kernel where its cold twin runs one
    wave per tile (gradients 6e-7 apart)."""
    import diff_gaussian_rasterization as dgr_mod
    dgr, lib, cpp = _bindings(binding, monkeypatch)
    prime, seq = _sequence(name)
    frames = [prime] + list(seq)
    scene = _Scene(seq[0], device)
    hot = _run_pass(scene, frames, lib, cpp, dgr, True, monkeypatch)
    cold = _run_pass(scene, frames, lib, cpp, dgr, False, monkeypatch)
    problems = []
    expect_over = [i + 1 for i in predicted_capacity_reruns(name)]          # (positions in `frames`)
    seen = dict(over=[], ckpt=[], repair=[], stale_sparse=[], stale_long=[], other_backward=[])
    want = dict(ckpt=[], repair=[])
    for i, fr in enumerate(frames):
        (h, h_img, h_radii, h_g), (c, c_img, c_radii, c_g) = hot[i], cold[i]
        same_bwd = h["bwd_forms"] == c["bwd_forms"]
        errs = {k: rel_l2(h_g[k].cpu().numpy(), c_g[k].cpu().numpy()) for k in GRAD_KEYS}
        _show(name, i - 1, h, f"| cold: cap {c['capacity']} fwd {c['fwd_forms']:#05x} bwd {c['bwd_forms']:#06x} ckpt_used {c['ckpt_used']} worst grad diff "
                              f"{max(errs.values()):.2e} ({max(errs, key=errs.get)})")
        _against_oracle(problems, f"{name}[{i - 1}] {binding}", _oracle_frame(fr), h_img, h_radii, h_g, h["N"])
        if not (torch.equal(h_img, c_img) and torch.equal(h_radii, c_radii)):
            problems.append(f"{name}[{i - 1}]: image / radii not bit-equal to the cold render (max |d| {float((h_img - c_img).abs().max()):.3e})")
        for k in GRAD_KEYS:
            tol = order_tol(k) if same_bwd else ALT_BACKWARD_TOL
            if not errs[k] <= tol:
                problems.append(f"{name}[{i - 1}]: grad {k} differs from the cold render's by {errs[k]:.3e} > {tol} (same backward form: {same_bwd})")
        if c["binning_reruns"] or c["ckpt_reruns"] or c["long_repair"] or c["capacity"] != c["N"]:
            problems.append(f"{name}[{i - 1}]: the cold render ran on a guess")
        if i == 0:
            continue
        p = cold[i - 1][0]
        over = i in expect_over
        ckpt = (not over) and c["ckpt_used"] > 0 and p["ckpt_used"] > 0 and c["ckpt_used"] > dgr_mod._round_ckpt_slots(p["ckpt_used"])
        repair = (not over) and (not ckpt) and c["has_long"] and not p["has_long"]
        want["ckpt"] += [i - 1] if ckpt else []
        want["repair"] += [i - 1] if repair else []
        seen["over"] += [i - 1] * h["binning_reruns"]
        seen["ckpt"] += [i - 1] * h["ckpt_reruns"]
        seen["repair"] += [i - 1] if h["long_repair"] else []
        seen["stale_sparse"] += [i - 1] if c["sparse"] != p["sparse"] else []
        seen["stale_long"] += [i - 1] if c["has_long"] != p["has_long"] else []
        seen["other_backward"] += [i - 1] if not same_bwd else []
        if not over and not ckpt and h["capacity"] != dgr_mod._round_capacity(p["N"]):
            problems.append(f"{name}[{i - 1}]: capacity {h['capacity']} is not round_capacity of the frame before")
        for k in ("N", "has_long", "sparse", "ckpt_used"):
            if h[k] != c[k]:
                problems.append(f"{name}[{i - 1}]: {k} {h[k]} hinted, {c[k]} cold")
    print(f"{name} {binding}: observed {seen}\n  predicted capacity re-runs {[i - 1 for i in expect_over]}, checkpoint re-runs {want['ckpt']}, repairs {want['repair']}")
    print(f"  sparse_frame values: {sorted({int(r[0]['sparse']) for r in hot})}")
    assert not problems, "\n".join(problems)
    assert seen["over"] == [i - 1 for i in expect_over], "capacity re-runs: not on the frames the oracle's N predicts"
    assert seen["ckpt"] == want["ckpt"] and seen["repair"] == want["repair"], (seen, want)
    if name == "stacked_512":
        assert seen["stale_long"], "no frame ran on a stale has_long_tiles"
        assert seen["ckpt"] == [13] and seen["repair"] == [5], "the sequence must meet both repairs"
    else:
        assert {bool(r[0]["sparse"]) for r in hot} == {False, True} and seen["stale_sparse"]
        assert seen["other_backward"], "no frame took another backward form than its cold twin"


@gpu
@pytest.mark.parametrize("name", ["stacked_512", "c2_cameras"])
def test_lists_of_every_frame_of_a_sequence_equal_the_oracle(name, device, monkeypatch):
    """The sequence once more through _debug_forward_state (a frame like any other: it feeds the records and runs on them): N, tile
    ranges and the sorted list equal to the oracle's position by position -- also on the frame whose list beyond 4 096 entries meets a
    record that says there is none (stacked_512, frame 10: no plan kernel), and with fewer depth-parallel workers than the frame has
    long lists (frame 7: the cap from the 4 long lists of frame 6 is below the long-list count the scan reports in n_total[2])."""
    from diff_gaussian_rasterization import _debug_forward_state
    dgr, lib, _ = _bindings("ctypes", monkeypatch)
    prime, seq = _sequence(name)
    _forget(dgr, device, _shape(prime))
    t = gpu_tensors(seq[0], device, grad=False)
    problems, n_long = [], []
    for i, fr in enumerate([prime] + list(seq)):
        ref = _oracle_frame(fr, with_lists=True)
        color, radii, st = _debug_forward_state(t["means3D"], t["opacities"], gpu_settings(fr, device), shs=t["shs"], scales=t["scales"],
                                                rotations=t["rotations"])
        torch.cuda.synchronize()
        forms = int(lib.hgs_debug_stat(b"last_forward_forms"))
        nt = st["n_total"].cpu().numpy()
        n_long.append((int(nt[2]), int(nt[8]), forms))
        print(f"  {name}[{i - 1:2d}] N {st['N']:8d} cap {st['binning_capacity']:8d} long lists {int(nt[2]):5d} threshold {int(nt[4]):5d} deep from {int(nt[8]):5d} "
              f"huge {int(nt[6]):3d} ckpt kind {int(nt[3])} fwd {forms:#05x}")
        if st["N"] != ref["N"]:
            problems.append(f"{name}[{i - 1}]: N {st['N']} != {ref['N']}")
            continue
        for k, view in (("ranges", np.uint32), ("values", np.uint32)):
            if not np.array_equal(st[k].cpu().numpy().view(view), ref[k]):
                problems.append(f"{name}[{i - 1}]: {k} differ from the oracle's")
        if not np.array_equal(radii.cpu().numpy(), ref["radii"]):
            problems.append(f"{name}[{i - 1}]: radii differ from the oracle's")
        try:
            check_image(color.cpu().numpy(), ref["color"], f"{name}[{i - 1}]")
        except AssertionError as e:
            problems.append(str(e))
    assert not problems, "\n".join(problems)
    if name == "stacked_512":
        i = WORKER_CAP_FRAME
        (before, deep_before, _), (now, _, forms) = n_long[i], n_long[i + 1]      # (n_long[0] is the priming frame's)
        tiles = 1024
        cap = min((min(4 * tiles, 2048) + 7) & ~7, (5 * before + 64 + 7) & ~7)      # binning.hip, launch_tile_sort
        assert deep_before and forms & FWD_DEEP_WORKERS and cap < now, f"the worker cap ({cap}, from {before} long lists) was not below the frame's {now} long lists"


def _by_tag(frames, results):
    out = {}
    for fr, res in zip(frames, results):
        out.setdefault(fr["tag"], []).append(res)
    return out


@gpu
def test_the_order_of_the_frames_does_not_matter(device, monkeypatch):
    """stacked_512 forward + backward as designed, reversed and in one seeded shuffle, each from empty records and the priming frame:
    image and radii of a frame are bit-equal whatever came before it -- the frame that stands at four places also with itself --,
    gradients within ALT_BACKWARD_TOL."""
    dgr, lib, cpp = _bindings("cpp", monkeypatch)
    prime, seq = _sequence("stacked_512")
    scene = _Scene(seq[0], device)
    n = len(seq)
    orders = [list(range(n)), list(range(n))[::-1], [int(i) for i in np.random.default_rng(5).permutation(n)]]
    first, problems = {}, []
    for o, order in enumerate(orders):
        frames = [prime] + [seq[i] for i in order]
        res = _run_pass(scene, frames, lib, cpp, dgr, True, monkeypatch)
        reruns = [i for i, r in enumerate(res[1:]) for _ in range(r[0]["binning_reruns"])]
        assert reruns == predicted_capacity_reruns("stacked_512", order), f"order {o}"
        for tag, runs in _by_tag(frames, res).items():
            for rec, img, radii, g in runs:
                ref = first.setdefault(tag, (img, radii, g))
                if not (torch.equal(img, ref[0]) and torch.equal(radii, ref[1])):
                    problems.append(f"order {o}, frame {tag}: image / radii depend on what came before (max |d| {float((img - ref[0]).abs().max()):.3e})")
                for k in GRAD_KEYS:
                    err = rel_l2(g[k].cpu().numpy(), ref[2][k].cpu().numpy())
                    if not err <= ALT_BACKWARD_TOL:
                        problems.append(f"order {o}, frame {tag}: grad {k} differs by {err:.3e}")
    assert len(first) == len({fr["tag"] for fr in seq})
    assert not problems, "\n".join(problems)


@gpu
@pytest.mark.parametrize("num_streams", [1, 3])
def test_deferred_frames_that_meet_a_record_of_small_frames_are_run_again(num_streams, device, monkeypatch):
    """render_batch over stacked_512 with the smallest frame first: the shape's record then says 35 911 entries, every later frame of
    the batch is deferred with the 262 144 entries that gives a 512 x 512 frame, and the frames beyond that -- the second has 3 499 600
    -- overflow for real (no monkeypatch): resolve() runs them again.  Second pass: the record knows the largest, everything fits.
    Every image and radii bit-equal to the frame rendered on its own (the serial renders of the test above, clamped as render does)."""
    from hugs_amd.renderer import render_batch
    dgr, lib, cpp = _bindings("cpp", monkeypatch)
    prime, seq = _sequence("stacked_512")
    scene = _Scene(seq[0], device)
    order = _deferred_order()
    frames = [seq[i] for i in order]
    with torch.no_grad():
        serial = [scene.render(fr, lib, cpp, backward=False) for fr in frames]
    for fr, (rec, img, radii, _g) in zip(frames, serial):
        ref = _oracle_frame(fr)
        assert rec["N"] == ref["N"] and np.array_equal(radii.cpu().numpy(), ref["radii"])
        check_image(img.cpu().numpy(), ref["color"], fr["tag"])
    items = []
    for fr in frames:
        data = {k: (to_dev(v, device) if isinstance(v, np.ndarray) else v) for k, v in fr["cam"].items()}
        items.append(dict(means3D=scene.t["means3D"], feats=scene.t["shs"], opacity=scene.t["opacities"], scales=scene.t["scales"],
                          rotations=scene.t["rotations"], data=data, scaling_modifier=fr["scale_modifier"], bg_color=to_dev(fr["bg"], device),
                          active_sh_degree=fr["D"]))
    _forget(dgr, device, _shape(prime))
    rerun = []
    orig = dgr.DeferredFrame.resolve

    def resolve(self):
        deferred = self.num_rendered is None
        n = orig(self)
        rerun.append(deferred and int(self.args.defer_n) == 0)    # (the second run of a frame is a waiting one)
        return n

    monkeypatch.setattr(dgr.DeferredFrame, "resolve", resolve)
    n_of = [sequence_stats("stacked_512")[i]["N"] for i in order]
    for rep in range(2):
        rerun.clear()
        batch = render_batch(items, num_streams=num_streams)
        torch.cuda.synchronize()
        assert len(batch) == len(serial)
        for fr, a, (rec, img, radii, _g) in zip(frames, batch, serial):
            assert torch.equal(a["render"], torch.clamp(img, 0.0, 1.0)) and torch.equal(a["radii"], radii), f"pass {rep}, {fr['tag']}"
        # pass 0: the first frame has no record and waits; the others were given 262 144 entries
        expect = [False] + [n > 262_144 for n in n_of[1:]] if rep == 0 else [False] * len(frames)
        assert rerun == expect and (rep == 1 or sum(expect) >= 8), f"pass {rep}: re-run {rerun}"


@gpu
@pytest.mark.parametrize("form", ["one_set", "second_set"])
def test_two_shapes_taking_turns_do_not_share_their_records(form, device, monkeypatch):
    """The reference's step renders the joint frame and the human-only frame in turn on one stream.  stacked_512 frame by frame in turn
    with the core alone at 256 x 256 (in view, out of view: N = 0), forward + backward, both on the records their own shape left:
    every frame against the oracle at the bars of the sequence test; capacity re-runs exactly where each shape's own N predicts.
    second_set: the joint frame hands the core over as `second=` behind the background (hgs_segment; the key is P + P2)."""
    dgr, lib, cpp = _bindings("cpp", monkeypatch)
    prime_a, seq_a = _sequence("stacked_512")
    prime_b, seq_b = _sequence("core_256")
    if form == "second_set":    # the same Gaussians, background first: what the call concatenates
        def reordered(fr):
            f = dict(fr)
            for k in ("means3D", "scales", "rotations", "opacities", "shs"):
                f[k] = np.concatenate([fr[k][CORE:], fr[k][:CORE]], 0)
            f["tag"] = fr["tag"] + ":background_first"
            return f
        base = reordered(seq_a[0])
        share = lambda fr: {**fr, **{k: base[k] for k in ("means3D", "scales", "rotations", "opacities", "shs")}, "tag": fr["tag"] + ":background_first"}
        prime_a, seq_a = share(prime_a), [share(fr) for fr in seq_a]
        # (on the device the rows stay as they were: _Scene.render hands the rows from CORE on over first, the core as `second`)
        scene_a = _Scene(_sequence("stacked_512")[1][0], device, second_from=CORE)
    else:
        scene_a = _Scene(seq_a[0], device)
    scene_b = _Scene(seq_b[0], device)
    _forget(dgr, device, _shape(prime_a), _shape(prime_b))
    problems, reruns = [], {"a": [], "b": []}
    turns = [("a", -1, prime_a), ("b", -1, prime_b)] + [x for i in range(len(seq_a)) for x in (("a", i, seq_a[i]), ("b", i, seq_b[i]))]
    for which, i, fr in turns:
        scene = scene_a if which == "a" else scene_b
        rec, img, radii, g = scene.render(fr, lib, cpp)
        _against_oracle(problems, f"{fr['tag']} (turn {i})", _oracle_frame(fr), img, radii, g, rec["N"])
        reruns[which] += [i] * rec["binning_reruns"]
    assert not problems, "\n".join(problems)
    assert reruns["a"] == predicted_capacity_reruns("stacked_512") and reruns["b"] == predicted_capacity_reruns("core_256")
