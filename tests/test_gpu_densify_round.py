"""GPU: one densification round of either model (row f-12: hugs_amd.densify.densify_and_prune_scene / _human, csrc/densify.hip) against
tests/densify_ref.py's restatement of the reference's round on the same inputs and the same noise.

Sizes: with R = rows per workgroup of the passes, n in 0, 1, R-1, R, R+1, 2R+17 (three workgroups with unequal totals: the scan of the
per-workgroup counts).  On fixtures whose predicates are decidable (tests/test_densify_round.py shows the restatement takes the same
branches in fp32 and fp64 on every one of them):

* row count and row order are exact;
* every copied value is bit-equal to the fp32 restatement's: the parameters outside the split copies' xyz / scaling /
  scaling_multiplier, all gathered moments and the zeros of the new rows' moments, the statistics, the human's tmp tensors;
* the transformed values -- split xyz, the scene's split _scaling, the human's split scaling_multiplier -- are a third fp32 evaluation
  (torch divides by a scalar through its reciprocal; its exp / log are not the device's) and are held to

      |ours - ref64| <= F * max(|ref32 - ref64|, FLOOR_ULP ulp(ref64))        per element,

  ref32 / ref64 the restatement in fp32 / fp64 on the CPU.  Measured on an MI355X over every fixture of densify_ref.cases(), both
  optimizers and the generator path (the figures the tests print; test_the_worst_ratios_of_this_session collects them) -- the largest
  ratio per transformed tensor, and F = twice that, rounded up to a power of two:

      scene  split xyz                  23.09   (generator path 4.69)     F = 64
      scene  split _scaling              2.64                             F = 8
      human  split xyz                   1.00   (generator path 1.33)     F = 4
      human  split scaling_multiplier    0.156                            F = 0.5

  The scene's xyz ratio is large where xyz and the offset R (noise * std) cancel: the floor is ulps of the RESULT, both fp32 evaluations
  err by ulps of the TERMS.  The human's R and std are inputs, not exp / normalise / build_rotation: its evaluation is torch's but for
  the product's order.
"""
import numpy as np
import pytest
import torch

import densify_ref as ref

pytestmark = pytest.mark.gpu

F = {("scene", "xyz"): 64.0, ("scene", "scaling"): 8.0, ("human", "xyz"): 4.0, ("human", "scaling_multiplier"): 0.5}
FLOOR_ULP = 4
_worst = {}


def _limits():
    from hugs_amd.densify import densify_limits
    return densify_limits()


def _bits(a, b):
    """bit-equal fp32 tensors (shape included)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _ratio(ours, r32, r64):
    """max over the elements of |ours - ref64| / max(|ref32 - ref64|, FLOOR_ULP ulp(ref64)); 0 for no elements"""
    if ours.numel() == 0:
        return 0.0
    o, a, b = ours.detach().cpu().double().numpy(), r32.detach().cpu().double().numpy(), r64.detach().cpu().double().numpy()
    assert np.isfinite(o).all() and o.shape == b.shape
    floor = FLOOR_ULP * np.spacing(np.abs(b).astype(np.float32)).astype(np.float64)
    return float((np.abs(o - b) / np.maximum(np.abs(a - b), floor)).max())


def _ours(fx, device, make_optimizer=None, with_state=True, generator=None):
    from hugs_amd import densify as D
    inst = ref.instantiate(fx, torch.float32, device, make_optimizer, with_state)
    opt = inst["optimizer"]
    steps = {id(st): st["step"].clone() for st in opt.state.values()}
    if fx["flavour"] == ref.SCENE:
        params, stats = D.densify_and_prune_scene(inst["params"], opt, inst["stats"], generator=generator, **fx["args"])
        plain = {}
    else:
        params, stats, mult, o_tmp, s_tmp, r_tmp = D.densify_and_prune_human(inst["params"]["xyz"], inst["scaling_multiplier"], inst["human_gs_out"], opt,
                                                                             inst["stats"], generator=generator, **fx["args"])
        plain = {"scaling_multiplier": mult, "opacity_tmp": o_tmp, "scales_tmp": s_tmp, "rotmat_tmp": r_tmp}
    return {"params": params, "stats": stats, "plain": plain, "optimizer": opt, "inst": inst, "steps": steps}


def _compare(fx, device, seed=3, make_optimizer=None, with_state=True):
    """One round of ours against the restatement in fp32 and fp64 -> the three ratios (xyz, scaling, scaling_multiplier)"""
    gen = torch.Generator(device=device).manual_seed(seed)
    ours = _ours(fx, device, make_optimizer, with_state, gen)
    twin = torch.Generator(device=device).manual_seed(seed)
    drawn = {}

    def noise(count):      # the same draw, once, for both restatements
        if "n" not in drawn:
            drawn["n"] = torch.randn((2 * count, 3), generator=twin, device=device, dtype=torch.float32).cpu()
        return drawn["n"]

    r32 = ref.run_ref(fx, torch.float32, noise, with_state=with_state)
    r64 = ref.run_ref(fx, torch.float64, noise, with_state=with_state)
    if r32["masks"].get("split") is not None and "n" in drawn:
        assert torch.equal(gen.get_state(), twin.get_state())
    tag = (fx["flavour"], fx["n"], fx["pattern"], fx["args"]["max_screen_size"], fx["args"]["max_n_gs"])
    n_new = r32["params"]["xyz"].shape[0]
    split_rows = 0
    if "split" in r32["masks"]:
        # rows behind [originals | clones] that survived the last prune: the split copies
        before = int((~r32["masks"]["split"]).sum())
        split_rows = int((~r32["masks"]["prune"][before:]).sum())
    head = n_new - split_rows
    transformed = {"xyz": "xyz", "scaling": "scaling"} if fx["flavour"] == ref.SCENE else {"xyz": "xyz"}
    ratios = {}
    opt = ours["optimizer"]
    for name, p in ours["params"].items():
        q = r32["params"][name]
        assert p.shape == q.shape, (tag, name, p.shape, q.shape)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf
        group = next(g for g in opt.param_groups if g["name"] == name)
        assert group["params"][0] is p and len(group["params"]) == 1
        if name in transformed:
            assert _bits(p[:head], q[:head]), (tag, name, "rows that are copied")
            ratios[name] = _ratio(p[head:], q[head:], r64["params"][name][head:])
        else:
            assert _bits(p, q), (tag, name)
        if with_state:
            assert set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq"}
            for k, key in enumerate(("exp_avg", "exp_avg_sq")):
                assert _bits(opt.state[p][key], r32["moments"][name][k]), (tag, name, key)
            assert id(opt.state[p]) in ours["steps"] and torch.equal(opt.state[p]["step"], ours["steps"][id(opt.state[p])])
            assert opt.state[p]["step"].device.type == "cpu"
        else:
            assert p not in opt.state
    assert len(opt.state) == (sum(len(g["params"]) for g in opt.param_groups) if with_state else 0)    # no stale keys
    for a, b in zip(ours["stats"], r32["stats"]):
        assert _bits(a, b), (tag, "statistics")
    for k, v in ours["plain"].items():
        q = r32["plain"][k]
        if k == "scaling_multiplier":
            assert _bits(v[:head], q[:head]), (tag, k)
            ratios[k] = _ratio(v[head:], q[head:], r64["plain"][k][head:])
        else:
            assert _bits(v, q), (tag, k)
    if fx["flavour"] == ref.HUMAN:      # the groups that are not densified: same objects, same state
        for name, ps in ours["inst"]["bystanders"].items():
            group = next(g for g in opt.param_groups if g["name"] == name)
            assert all(a is b for a, b in zip(group["params"], ps))
            if with_state:
                assert all(_bits(opt.state[p]["exp_avg"], torch.from_numpy(ref.moments(p.shape, "exp_avg"))) for p in ps)
    for k, v in ratios.items():
        _worst[(fx["flavour"], k)] = max(_worst.get((fx["flavour"], k), 0.0), v)
    return ratios, n_new, split_rows


@pytest.mark.parametrize("flavour", (ref.SCENE, ref.HUMAN))
@pytest.mark.parametrize("which", range(6))
def test_a_round_equals_the_restatement(device, flavour, which):
    """Every selection pattern, with and without max_screen_size, the branch beyond max_n_gs, the scene without higher SH bands."""
    rows, _ = _limits()
    n = ref.sizes(rows)[which]
    worst = {}
    for case in ref.cases(rows):
        if case["flavour"] != flavour or case["n"] != n:
            continue
        fx = ref.make_fixture(**case)
        ratios, n_new, split_rows = _compare(fx, device)
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if case["pattern"] == "pruned":
            assert n_new == 0
        if case["pattern"] == "split" and n and not case["screen"]:
            assert split_rows == 2 * n == n_new
        if case["pattern"] == "clone" and n:
            assert n_new == 2 * n and split_rows == 0
        if case["pattern"] == "none":
            assert n_new == n
    print(f"densify round {flavour} n={n}: worst |ours - ref64| / max(|ref32 - ref64|, {FLOOR_ULP} ulp) = {worst}")
    assert all(v <= F[flavour, k] for k, v in worst.items()), worst


def test_beyond_max_n_gs_only_the_prune_runs_on_the_real_radii(device):
    rows, _ = _limits()
    for flavour in (ref.SCENE, ref.HUMAN):
        fx = ref.make_fixture(flavour, rows + 1, "mix", screen=True, skip_branch=True)
        ours = _ours(fx, device)
        accum, denom, radii = (t.cpu() for t in ours["stats"])
        o = torch.from_numpy(fx["opacity"][:, 0])
        if flavour == ref.SCENE:
            o, top = torch.sigmoid(o), torch.exp(torch.from_numpy(fx["scaling"])).max(1).values
        else:
            top = torch.from_numpy(fx["scales_canon"]).max(1).values
        by_radius = torch.from_numpy(fx["radii"]) > ref.SCREEN
        keep = ~((o < ref.MIN_OPACITY) | by_radius | (top > ref.BIG_T))
        assert by_radius.any() and (by_radius & ~((o < ref.MIN_OPACITY) | (top > ref.BIG_T))).any()      # max_radii2D alone prunes some
        assert ours["params"]["xyz"].shape[0] == int(keep.sum()) < fx["n"]
        # gathered, not zeroed
        assert _bits(radii, torch.from_numpy(fx["radii"])[keep]) and _bits(accum, torch.from_numpy(fx["accum"])[keep])
        assert _bits(denom, torch.from_numpy(fx["denom"])[keep]) and (radii <= ref.SCREEN).all() and radii.max() > 0


@pytest.mark.parametrize("flavour", (ref.SCENE, ref.HUMAN))
@pytest.mark.parametrize("optimizer", ("torch", "hip"))
@pytest.mark.parametrize("with_state", (True, False))
def test_the_optimizer_surgery_on_both_optimizers_with_and_without_state(device, flavour, optimizer, with_state):
    from hugs_amd.optim import Adam
    rows, _ = _limits()
    make = (lambda g: Adam(g, lr=0.0, eps=1e-15)) if optimizer == "hip" else (lambda g: torch.optim.Adam(g, lr=0.0, eps=1e-15))
    for degree in ((0, 3) if flavour == ref.SCENE else (3,)):
        fx = ref.make_fixture(flavour, rows + 1, "mix", sh_degree=degree)
        ratios, n_new, split_rows = _compare(fx, device, make_optimizer=make, with_state=with_state)
        assert n_new > 0 and split_rows > 0 and all(v <= F[flavour, k] for k, v in ratios.items()), ratios


def test_more_tensors_than_one_scatter_launch_takes(device):
    """A human optimizer with eleven more densified groups: 12 x 3 + 4 + 3 = 43 records, beyond one launch's table -- the scatter is chunked."""
    from hugs_amd import densify as D
    rows, per_launch = _limits()
    extras = [f"extra{i}" for i in range(11)]
    assert (1 + len(extras)) * 3 + 7 > per_launch
    fx = ref.make_fixture(ref.HUMAN, rows + 1, "mix")

    def build(dev):
        inst = ref.instantiate(fx, torch.float32, dev)
        for i, name in enumerate(extras):
            shape = (fx["n"], i % 4 + 1)
            p = torch.nn.Parameter(torch.from_numpy(ref.moments(shape, "exp_avg") * (i + 2)).to(dev))
            inst["optimizer"].add_param_group({"params": [p], "lr": 1e-3, "name": name})
            inst["optimizer"].state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.from_numpy(ref.moments(shape, "exp_avg") + i).to(dev),
                                          "exp_avg_sq": torch.from_numpy(ref.moments(shape, "exp_avg_sq") + i).to(dev)}
        return inst

    ours, theirs = build(device), build("cpu")
    gen, twin = torch.Generator(device=device).manual_seed(9), torch.Generator(device=device).manual_seed(9)
    params, stats, mult, o_tmp, s_tmp, r_tmp = D.densify_and_prune_human(ours["params"]["xyz"], ours["scaling_multiplier"], ours["human_gs_out"], ours["optimizer"],
                                                                         ours["stats"], generator=gen, densify_group_names=["xyz"] + extras, **fx["args"])
    noise = lambda count: torch.randn((2 * count, 3), generator=twin, device=device, dtype=torch.float32).cpu()
    r_params, r_stats, r_plain, masks = ref.human_round(theirs["optimizer"], theirs["scaling_multiplier"], theirs["human_gs_out"], theirs["stats"], noise, **fx["args"])
    assert set(params) == set(r_params) == {"xyz", *extras} and masks["split"].any() and masks["clone"].any()
    for name in extras:
        p, q = params[name], r_params[name]
        assert _bits(p, q), name
        for key in ("exp_avg", "exp_avg_sq"):
            assert _bits(ours["optimizer"].state[p][key], theirs["optimizer"].state[q][key]), (name, key)
        assert float(ours["optimizer"].state[p]["step"]) == 3.0
    assert params["xyz"].shape == r_params["xyz"].shape and _bits(s_tmp, r_plain["scales_tmp"]) and _bits(r_tmp, r_plain["rotmat_tmp"])
    assert all(_bits(a, b) for a, b in zip(stats, r_stats))


@pytest.mark.parametrize("flavour", (ref.SCENE, ref.HUMAN))
def test_the_generator_is_consumed_as_the_references_normal_consumes_it(device, flavour):
    """Same seed, same device: a round with generator= leaves the generator where the restatement's torch.normal(mean, std) round leaves
    it, and the split positions agree."""
    rows, _ = _limits()
    fx = ref.make_fixture(flavour, 2 * rows + 17, "mix")
    g1, g2 = torch.Generator(device=device).manual_seed(21), torch.Generator(device=device).manual_seed(21)
    ours = _ours(fx, device, generator=g1)
    theirs = ref.run_ref(fx, torch.float32, noise=None, generator=g2, device=device)
    assert theirs["masks"]["split"].any()
    assert torch.equal(g1.get_state(), g2.get_state())
    p, q = ours["params"]["xyz"].detach().cpu(), theirs["params"]["xyz"].detach().cpu()
    assert p.shape == q.shape
    # the restatement on the device IS an fp32 evaluation; its fp64 twin on the noise it drew bounds both
    twin = torch.Generator(device=device).manual_seed(21)
    r64 = ref.run_ref(fx, torch.float64, noise=lambda count: torch.randn((2 * count, 3), generator=twin, device=device, dtype=torch.float32).cpu())
    ratio = _ratio(p, q, r64["params"]["xyz"])
    print(f"densify round {flavour}: generator path, worst ratio {ratio}")
    assert ratio <= F[flavour, "xyz"]


def test_a_round_then_an_adam_step_then_a_render(device):
    import math
    from hugs_amd import synthetic as syn
    from hugs_amd.densify import densify_and_prune_scene
    from hugs_amd.optim import Adam
    from hugs_amd.renderer.gs_renderer import render
    from hugs_amd.scene_forward import scene_forward
    P, H, W = 3000, 96, 128
    cam = syn.pinhole_camera(H, W)
    g = syn.scene_gaussians(P, cam, seed=5, sigma_px=3.0, ref_P=P)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    t = lambda a: torch.from_numpy(f32(a)).to(device)
    op = np.clip(g["opacities"], 0.001, 0.98).reshape(-1, 1)
    r = np.random.default_rng(1)
    params = {"xyz": t(g["means3D"]), "f_dc": t(0.3 * r.standard_normal((P, 1, 3))), "f_rest": t(0.05 * r.standard_normal((P, 15, 3))),
              "opacity": t(np.log(op / (1 - op))), "scaling": t(np.log(g["scales"])), "rotation": t(g["rotations"])}
    params = {k: torch.nn.Parameter(v) for k, v in params.items()}
    opt = Adam([{"params": [p], "lr": 1e-3, "name": k} for k, p in params.items()], lr=0.0, eps=1e-15)
    for p in params.values():
        p.grad = torch.randn_like(p) * 1e-3
    opt.step()
    grads = t(np.abs(r.standard_normal((P, 1))) * 3e-4)
    extent = float(np.linalg.norm(g["means3D"].max(0) - g["means3D"].min(0)))
    stats = (grads * 4, torch.full((P, 1), 4.0, device=device), torch.zeros(P, device=device))
    new, stats = densify_and_prune_scene(params, opt, stats, 2e-4, 0.005, extent, None, generator=torch.Generator(device=device).manual_seed(2))
    n = new["xyz"].shape[0]
    assert n > P and all(v.shape[0] == n for v in new.values()) and all(s.shape[0] == n and not s.any() for s in stats)
    for p in new.values():
        p.grad = torch.randn_like(p) * 1e-3
    opt.step()
    assert all(float(opt.state[p]["step"]) == 2.0 for p in new.values())
    data = {k: (t(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
    act = scene_forward(new["xyz"], new["scaling"], new["rotation"], new["opacity"], new["f_dc"], new["f_rest"], 3)
    pkg = render(means3D=act["xyz"], feats=act["shs"], opacity=act["opacity"], scales=act["scales"], rotations=act["rotq"], data=data,
                 bg_color=torch.ones(3, device=device), active_sh_degree=3)
    pkg["render"].sum().backward()
    assert torch.isfinite(pkg["render"]).all() and all(torch.isfinite(p).all() and torch.isfinite(p.grad).all() for p in new.values())
    assert math.isfinite(float(pkg["render"].detach().mean()))


@pytest.mark.parametrize("flavour", (ref.SCENE, ref.HUMAN))
def test_a_round_synchronises_with_the_host_exactly_once(device, flavour, monkeypatch):
    from hugs_amd import densify as D
    rows, _ = _limits()
    fx = ref.make_fixture(flavour, 2 * rows + 17, "mix")
    _ours(fx, device, generator=torch.Generator(device=device).manual_seed(1))      # warm-up: code objects, the allocator's blocks
    inst = ref.instantiate(fx, torch.float32, device)
    gen = torch.Generator(device=device).manual_seed(1)
    readbacks = []
    inner = D._read_totals

    def counted(totals):      # the one readback, let through; anything else that waits for the device raises
        torch.cuda.set_sync_debug_mode("default")
        try:
            readbacks.append(inner(totals))
        finally:
            torch.cuda.set_sync_debug_mode("error")
        return readbacks[-1]

    monkeypatch.setattr(D, "_read_totals", counted)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if flavour == ref.SCENE:
            out = D.densify_and_prune_scene(inst["params"], inst["optimizer"], inst["stats"], generator=gen, **fx["args"])
        else:
            out = D.densify_and_prune_human(inst["params"]["xyz"], inst["scaling_multiplier"], inst["human_gs_out"], inst["optimizer"], inst["stats"],
                                            generator=gen, **fx["args"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert len(readbacks) == 1 and len(readbacks[0]) == 5
    kept, clones, split1, split2, selected = readbacks[0]
    assert out[0]["xyz"].shape[0] == kept + clones + split1 + split2 and split1 == split2 <= selected and min(kept, clones, split1) > 0


def test_the_worst_ratios_of_this_session():
    """Not a check of its own: prints what the comparisons above measured, per model and transformed tensor (the figures F is set from)."""
    print("densify round, worst ratios over this session:", {f"{a}.{b}": round(v, 4) for (a, b), v in sorted(_worst.items())})
    assert all(v <= F[key] for key, v in _worst.items())
