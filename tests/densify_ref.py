"""Torch restatement of one densification round of either model (row f-12: csrc/densify.hip, hugs_amd/densify.py), in the order and
with the optimizer surgery of the reference:

    SceneGS.densify_and_prune        hugs/models/scene.py:441-458       (clone 426-439, split 401-424, postfix 381-399,
                                                                          cat 359-379, prune 325-357)
    HUGS_TRIMLP.densify_and_prune    hugs/models/hugs_trimlp.py:857-878 (clone 840-855, split 810-838, postfix 794-808,
                                                                          cat 769-792, prune 733-767)

It runs in the dtype of the tensors it is given (fp32 or fp64) on their device, on a real torch.optim.Adam (or any optimizer with
torch's state layout), and takes the split's noise explicitly: `noise` is a [>= 2 |S|, 3] tensor or a callable S -> [2 S, 3]; its row
c |S| + k belongs to copy c of the k-th split-selected row, which is how `torch.normal(mean, std)` on the [2 |S|, 3] `stds` pairs them
(scene.py:410-412).  With `noise=None` the reference's own draw is made: torch.normal(mean=zeros, std=stds, generator=generator).

make_fixture() builds inputs whose predicates are decidable: every compared quantity lies at a relative distance of at least 1e-3 from
its threshold (values that fall nearer are pushed to 4e-3, always the same way), so fp32 and fp64 evaluations -- and another fp32
evaluation with other exp / log / sigmoid roundings -- take the same branches.  check_fixture() asserts that on the fp32 inputs."""
import numpy as np
import torch

SCENE_GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
NON_DENSIFY = ("global_orient", "body_pose", "betas", "transl", "v_embed", "geometry_dec", "appearance_dec", "deform_dec")   # hugs_trimlp.py:693-696
SCENE, HUMAN = "scene", "human"


class _Rows:
    """The row-indexed state of a model: the optimizer's densified groups, plain row tensors, the three statistics."""

    def __init__(self, optimizer, names, plain, stats):
        self.opt, self.names, self.plain = optimizer, tuple(names), dict(plain)
        self.accum, self.denom, self.radii = stats

    def param(self, name):
        return next(g for g in self.opt.param_groups if g.get("name") == name)["params"][0]

    @property
    def n(self):
        return self.param("xyz").shape[0]

    def _replace(self, group, tensor, moments):
        old = group["params"][0]
        state = self.opt.state.get(old, None)
        new = torch.nn.Parameter(tensor.requires_grad_(True))
        if state is not None:
            state["exp_avg"], state["exp_avg_sq"] = moments(state["exp_avg"]), moments(state["exp_avg_sq"])
            del self.opt.state[old]
            self.opt.state[new] = state
        group["params"][0] = new

    def cat(self, rows, plain_rows):
        """cat_tensors_to_optimizer + densification_postfix: append, zero moments for the new rows, reset the statistics"""
        for group in self.opt.param_groups:
            if group.get("name") not in self.names:
                continue
            assert len(group["params"]) == 1
            ext = rows[group["name"]]
            self._replace(group, torch.cat((group["params"][0].detach(), ext), 0), lambda m: torch.cat((m, torch.zeros_like(ext)), 0))
        for k, ext in plain_rows.items():
            self.plain[k] = torch.cat((self.plain[k], ext), 0)
        x = self.param("xyz")
        self.accum, self.denom = x.new_zeros((self.n, 1)), x.new_zeros((self.n, 1))
        self.radii = x.new_zeros((self.n,))

    def prune(self, drop):
        """prune_points: keep ~drop everywhere"""
        keep = ~drop
        for group in self.opt.param_groups:
            if group.get("name") not in self.names:
                continue
            self._replace(group, group["params"][0].detach()[keep], lambda m: m[keep])
        self.plain = {k: v[keep] for k, v in self.plain.items()}
        self.accum, self.denom, self.radii = self.accum[keep], self.denom[keep], self.radii[keep]


def build_rotation(q):
    """utils/general.py:177-198: the quaternion (w, x, y, z) is normalised first"""
    q = q / torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])[:, None]
    w, x, y, z = q.unbind(1)
    return torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), 1).reshape(-1, 3, 3)


def _samples(stds, noise, generator):
    count = stds.shape[0] // 2
    if noise is None:
        return torch.normal(mean=torch.zeros_like(stds), std=stds, generator=generator), count
    if callable(noise):
        noise = noise(count)
    return noise[:2 * count].to(stds) * stds, count


@torch.no_grad()
def _round(flavour, m, noise, generator, max_grad, min_opacity, extent, max_screen_size, max_n_gs, percent_dense):
    """The body shared by the two models: they differ in where scales, opacity and the rotation come from and in what a split copy gets."""
    scene = flavour == SCENE
    scales_of = (lambda: torch.exp(m.param("scaling").detach())) if scene else (lambda: m.plain["scales_tmp"])
    opacity_of = (lambda: torch.sigmoid(m.param("opacity").detach())) if scene else (lambda: m.plain["opacity_tmp"])
    masks = {}
    grads = m.accum / m.denom
    grads[grads.isnan()] = 0.0
    n0 = m.n
    max_n_gs = max_n_gs if max_n_gs else n0 + 1
    if n0 <= max_n_gs:
        # clone: |g| >= max_grad and small
        clone = (torch.norm(grads, dim=-1) >= max_grad) & (scales_of().max(dim=1).values <= percent_dense * extent)
        masks["clone"] = clone
        m.cat({name: m.param(name).detach()[clone] for name in m.names}, {k: v[clone] for k, v in m.plain.items()})
        # split: over originals + clones, the clones' gradient padded with zeros
        padded = grads.new_zeros((m.n,))
        padded[:n0] = grads.squeeze(-1)
        scales = scales_of()
        split = (padded >= max_grad) & (scales.max(dim=1).values > percent_dense * extent)
        if not scene:
            med = scales.median(dim=1, keepdim=True).values
            split = split & (((scales - med) / med) >= 1.0).any(dim=-1)
        masks["split"] = split
        stds = scales[split].repeat(2, 1)
        samples, count = _samples(stds if scene else torch.relu(stds), noise, generator)
        rots = (build_rotation(m.param("rotation").detach()[split]) if scene else m.plain["rotmat_tmp"][split]).repeat(2, 1, 1)
        new = {name: m.param(name).detach()[split].repeat(2, *([1] * (m.param(name).dim() - 1))) for name in m.names}
        new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + m.param("xyz").detach()[split].repeat(2, 1)
        plain = {k: v[split].repeat(2, *([1] * (v.dim() - 1))) for k, v in m.plain.items()}
        if scene:
            new["scaling"] = torch.log(scales[split].repeat(2, 1) / (0.8 * 2))
        else:
            plain["scaling_multiplier"] = m.plain["scaling_multiplier"][split].repeat(2, 1) / (0.8 * 2)   # (scales_tmp stays as it is)
        m.cat(new, plain)
        m.prune(torch.cat((split, torch.zeros(2 * count, dtype=torch.bool, device=split.device))))
    drop = (opacity_of() < min_opacity).squeeze(-1)
    if max_screen_size:
        drop = drop | (m.radii > max_screen_size) | (scales_of().max(dim=1).values > 0.1 * extent)
    masks["prune"] = drop
    m.prune(drop)
    return masks


def scene_round(optimizer, stats, noise=None, generator=None, *, max_grad, min_opacity, extent, max_screen_size, max_n_gs=None,
                percent_dense=0.01):
    """-> (params by name, (xyz_gradient_accum, denom, max_radii2D), masks).  Every group of the optimizer is a scene group."""
    m = _Rows(optimizer, SCENE_GROUPS, {}, stats)
    masks = _round(SCENE, m, noise, generator, max_grad, min_opacity, extent, max_screen_size, max_n_gs, percent_dense)
    return {name: m.param(name) for name in SCENE_GROUPS}, (m.accum, m.denom, m.radii), masks


def human_round(optimizer, scaling_multiplier, human_gs_out, stats, noise=None, generator=None, *, max_grad, min_opacity, extent,
                max_screen_size, max_n_gs=None, percent_dense=0.01):
    """-> (params by name, statistics, plain row tensors, masks); the densified groups are those not named in NON_DENSIFY."""
    names = [g["name"] for g in optimizer.param_groups if g["name"] not in NON_DENSIFY]
    plain = {"scaling_multiplier": scaling_multiplier, "opacity_tmp": human_gs_out["opacity"], "scales_tmp": human_gs_out["scales_canon"],
             "rotmat_tmp": human_gs_out["rotmat_canon"]}
    m = _Rows(optimizer, names, plain, stats)
    masks = _round(HUMAN, m, noise, generator, max_grad, min_opacity, extent, max_screen_size, max_n_gs, percent_dense)
    return {name: m.param(name) for name in names}, (m.accum, m.denom, m.radii), m.plain, masks


# ---------------------------------------------------------------------------------------------------------------------------------
# fixtures

PATTERNS = ("none", "clone", "split", "pruned", "mix", "nan", "inf")
EXTENT, PERCENT_DENSE, MAX_GRAD, MIN_OPACITY, SCREEN = 4.0, 0.01, 2e-4, 0.005, 20
SMALL_T, BIG_T = PERCENT_DENSE * EXTENT, 0.1 * EXTENT
CLEAR, PUSH = 1e-3, 4e-3
# row kinds
COLD, CLONE, SPLIT, LOW, CLONE_LOW, SPLIT_LOW, BIG, ROUND, SPLIT_MID, SPLIT_HUGE, NAN, INF = range(12)
_MIX = (COLD, CLONE, SPLIT, LOW, SPLIT_MID, CLONE_LOW, BIG, SPLIT_LOW, ROUND, SPLIT_HUGE)


def _push(q, threshold):
    """values within PUSH (relative) of the threshold go to exactly that distance, on the side they are on"""
    q = np.array(q, np.float64)
    near = np.abs(q / threshold - 1.0) < PUSH
    q[near] = np.where(q[near] >= threshold, threshold * (1.0 + PUSH), threshold * (1.0 - PUSH))
    return q


def _kinds(n, pattern):
    i = np.arange(n)
    if pattern in ("none", "clone", "split"):
        return np.full(n, {"none": COLD, "clone": CLONE, "split": SPLIT}[pattern])
    if pattern == "pruned":
        return np.array((LOW, CLONE_LOW, SPLIT_LOW))[i % 3]
    kinds = np.array(_MIX)[(i * 7 + i // 10) % 10]     # every ten consecutive rows hold every kind
    if pattern in ("nan", "inf"):
        kinds[i % 5 == 2] = NAN if pattern == "nan" else INF
    return kinds


def make_fixture(flavour, n, pattern, seed=0, sh_degree=3, screen=True, skip_branch=False):
    """-> dict of float32 numpy arrays and the round's arguments.  Deterministic in its arguments."""
    rng = np.random.default_rng(1000 * seed + 17 * n + PATTERNS.index(pattern))
    kinds = _kinds(n, pattern)
    is_ = lambda *ks: np.isin(kinds, ks)
    u = lambda lo, hi: rng.uniform(lo, hi, n)
    edge = (np.arange(n) % 37 == 11) & (pattern == "mix")     # rows that start out ON a threshold, to give _push work
    hot = is_(CLONE, SPLIT, CLONE_LOW, SPLIT_LOW, ROUND, SPLIT_MID, SPLIT_HUGE)
    g = np.where(hot, u(1.3, 8.0), u(0.05, 0.8)) * MAX_GRAD
    g[edge] = MAX_GRAD * (1.0 + 2e-5 * np.where(hot[edge], 1.0, -1.0))
    g = _push(g, MAX_GRAD)
    small = is_(CLONE, CLONE_LOW, NAN) | (is_(INF) & (np.arange(n) % 2 == 0))
    top = np.where(small, u(0.2, 0.9), u(1.2, 6.0)) * SMALL_T
    top = np.where(is_(BIG), u(1.2, 3.0) * BIG_T, top)
    top = np.where(is_(SPLIT_MID), u(1.05, 1.5) * BIG_T, top)
    top = np.where(is_(SPLIT_HUGE), u(1.8, 4.0) * BIG_T, top)
    top[edge] = SMALL_T * (1.0 + 3e-5 * np.where(small[edge], -1.0, 1.0))
    for t in (SMALL_T, BIG_T, 1.6 * BIG_T):      # 1.6 * BIG_T: where a split copy's scale / 1.6 crosses the world-size bound
        top = _push(top, t)
    elongated = ~is_(ROUND, COLD, BIG)
    mid = top * np.where(elongated, u(0.1, 0.45), u(0.55, 0.95))
    mid[edge] = top[edge] * 0.5 * (1.0 + 1e-5)
    mid = top / _push(top / mid, 2.0)            # the human's test (max - med) / med >= 1 is max / med >= 2
    low = np.minimum(mid * u(0.3, 1.0), 0.4 * top)
    axes = np.argsort(rng.random((n, 3)), axis=1)
    scales = np.empty((n, 3))
    np.put_along_axis(scales, axes, np.stack((top, mid, low), 1), axis=1)
    opaque = ~is_(LOW, CLONE_LOW, SPLIT_LOW)
    o = np.where(opaque, u(0.02, 0.99), u(1e-4, 0.9 * MIN_OPACITY))
    o[edge] = MIN_OPACITY * (1.0 + 2e-5)
    o = _push(o, MIN_OPACITY)
    denom = rng.integers(1, 31, n).astype(np.float64)
    accum = g * denom
    denom[is_(NAN, INF)] = 0.0
    accum[is_(NAN)] = 0.0
    radii = rng.choice(np.array([0, 3, 11, 19, 21, 33, 40], np.float64), n)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    quat = rng.normal(size=(n, 4)) * u(0.5, 2.0)[:, None]
    fx = {"flavour": flavour, "n": n, "pattern": pattern, "kinds": kinds,
          "xyz": f32(rng.normal(size=(n, 3)) * EXTENT / 2), "accum": f32(accum[:, None]), "denom": f32(denom[:, None]), "radii": f32(radii),
          "args": dict(max_grad=MAX_GRAD, min_opacity=MIN_OPACITY, extent=EXTENT, max_screen_size=SCREEN if screen else None,
                       max_n_gs=(n - 1 if skip_branch else None), percent_dense=PERCENT_DENSE)}
    if flavour == SCENE:
        rest = (sh_degree + 1) ** 2 - 1
        fx.update(f_dc=f32(rng.normal(size=(n, 1, 3))), f_rest=f32(rng.normal(size=(n, rest, 3)) * 0.1), opacity=f32(np.log(o / (1.0 - o))[:, None]),
                  scaling=f32(np.log(scales)), rotation=f32(quat))
    else:
        q = quat / np.linalg.norm(quat, axis=1, keepdims=True)
        R = build_rotation(torch.from_numpy(q)).numpy()
        fx.update(scaling_multiplier=f32(u(0.5, 2.0)[:, None]), opacity=f32(o[:, None]), scales_canon=f32(scales), rotmat_canon=f32(R))
    check_fixture(fx)
    return fx


def check_fixture(fx):
    """Every compared quantity, recomputed in float64 from the float32 inputs, is at least CLEAR (relative) from its threshold."""
    d = lambda k: fx[k].astype(np.float64)
    clear = lambda q, t: bool((np.abs(q / t - 1.0) >= CLEAR).all())
    with np.errstate(divide="ignore", invalid="ignore"):
        g = d("accum")[:, 0] / d("denom")[:, 0]
    g = g[np.isfinite(g)]
    assert clear(g, fx["args"]["max_grad"]), "g against max_grad"
    if fx["flavour"] == SCENE:
        scales, o = np.exp(d("scaling")), 1.0 / (1.0 + np.exp(-d("opacity")[:, 0]))
    else:
        scales, o = d("scales_canon"), d("opacity")[:, 0]
    top = scales.max(1) if len(scales) else np.zeros(0)
    assert clear(top, SMALL_T) and clear(top, BIG_T) and clear(top, 1.6 * BIG_T), "max(scales) against its three bounds"
    assert clear(o, fx["args"]["min_opacity"]), "opacity against min_opacity"
    assert clear(d("radii") + 1e-30, float(SCREEN)), "max_radii2D against max_screen_size"
    if fx["flavour"] == HUMAN and len(scales):
        med = np.median(scales, 1)
        assert clear((top - med) / med, 1.0), "the elongation ratio against 1"


def sizes(rows_per_workgroup):
    R = rows_per_workgroup
    return (0, 1, R - 1, R, R + 1, 2 * R + 17)     # 2 R + 17: three workgroups with unequal totals


def cases(rows_per_workgroup):
    """Every fixture the GPU tests compare on, as make_fixture's keyword arguments: all sizes x patterns x both screen settings for
    both models, the branch beyond max_n_gs, and the scene without higher SH bands."""
    out = []
    for flavour in (SCENE, HUMAN):
        for n in sizes(rows_per_workgroup):
            for pattern in PATTERNS:
                for screen in (False, True):
                    out.append(dict(flavour=flavour, n=n, pattern=pattern, screen=screen))
            if n >= 2:
                for screen in (False, True):
                    out.append(dict(flavour=flavour, n=n, pattern="mix", screen=screen, skip_branch=True))
    for n in sizes(rows_per_workgroup):
        out.append(dict(flavour=SCENE, n=n, pattern="mix", screen=True, sh_degree=0))
    return out


def moments(shape, which):
    """Adam moments filled with distinct nonzero values (exp_avg signed, exp_avg_sq positive)"""
    count = int(np.prod(shape))
    i = np.arange(1, count + 1, dtype=np.float64)
    v = i * 1e-3 * np.where(i % 2 == 0, -1.0, 1.0) if which == "exp_avg" else i * 1e-6 + 0.5
    return v.reshape(shape).astype(np.float32)


def instantiate(fx, dtype, device, make_optimizer=None, with_state=True, step=7.0):
    """The fixture as tensors of `dtype` on `device` with an optimizer over them (default: torch.optim.Adam as the reference builds it).
    -> dict(optimizer=, params=, stats=, and for the human scaling_multiplier=, human_gs_out=, bystanders=)"""
    make_optimizer = make_optimizer or (lambda groups: torch.optim.Adam(groups, lr=0.0, eps=1e-15))
    t = lambda k: torch.from_numpy(fx[k]).to(device=device, dtype=dtype)
    names = SCENE_GROUPS if fx["flavour"] == SCENE else ("xyz",)
    params = {k: torch.nn.Parameter(t(k)) for k in names}
    groups = [{"params": [p], "lr": 1e-3, "name": k} for k, p in params.items()]
    out = {"params": params, "stats": (t("accum"), t("denom"), t("radii"))}
    if fx["flavour"] == HUMAN:
        gen = torch.Generator().manual_seed(5)
        by = {"v_embed": [torch.nn.Parameter(torch.randn(4, 8, generator=gen).to(device=device, dtype=dtype))],
              "geometry_dec": [torch.nn.Parameter(torch.randn(s, generator=gen).to(device=device, dtype=dtype)) for s in ((8, 4), (8,))]}
        groups += [{"params": ps, "lr": 1e-3, "name": k} for k, ps in by.items()]
        out.update(scaling_multiplier=t("scaling_multiplier"), bystanders=by,
                   human_gs_out={"opacity": t("opacity"), "scales_canon": t("scales_canon"), "rotmat_canon": t("rotmat_canon")})
    opt = make_optimizer(groups)
    if with_state:
        for group in opt.param_groups:
            for p in group["params"]:
                opt.state[p] = {"step": torch.tensor(step, dtype=torch.float32),
                                "exp_avg": torch.from_numpy(moments(p.shape, "exp_avg")).to(device=device, dtype=dtype),
                                "exp_avg_sq": torch.from_numpy(moments(p.shape, "exp_avg_sq")).to(device=device, dtype=dtype)}
    out["optimizer"] = opt
    return out


def run_ref(fx, dtype, noise=None, generator=None, device="cpu", with_state=True):
    """The restatement on the fixture -> dict(params=, moments=, stats=, plain=, masks=, optimizer=, inst=)"""
    inst = instantiate(fx, dtype, device, with_state=with_state)
    if fx["flavour"] == SCENE:
        params, stats, masks = scene_round(inst["optimizer"], inst["stats"], noise, generator, **fx["args"])
        plain = {}
    else:
        params, stats, plain, masks = human_round(inst["optimizer"], inst["scaling_multiplier"], inst["human_gs_out"], inst["stats"], noise,
                                                  generator, **fx["args"])
    opt = inst["optimizer"]
    mom = {k: (opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for k, p in params.items() if p in opt.state}
    return {"params": params, "moments": mom, "stats": stats, "plain": plain, "masks": masks, "optimizer": opt, "inst": inst}
