"""Row f-11: the multi-tensor Adam step (csrc/optim.hip, hugs_amd/optim.py).

CPU part: the float64 restatement (tests/adam_ref.py) pins itself to torch.optim.Adam(foreach=False) in float64 and two wrong variants
break that bound; the optimizer's construction; the C ABI's argument validation (it runs before any launch, so without a GPU).

GPU part, per tensor and per quantity (p, exp_avg, exp_avg_sq), row f-10's bar:

    max|hip - fp64| <= 4 * yardstick + 1e-6 * max|fp64|,    yardstick = max|torch.optim.Adam(foreach=False) in float32 on the CPU - fp64|

on gradients whose elements are exactly 0 or have 1e-6 <= |g| <= 1e2, eps = 1e-15 (the reference's).  Every figure is printed before it
is asserted (`adam-ratio <case> <tensor> <quantity> <max err / yardstick> <floor used>`), DESIGN.md 7f quotes them."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_ref as ar

GUARD = 8          # guard elements either side of every view (a multiple of 4: the view's 16-byte phase is its offset alone)
EPS = 1e-15
SIZES = lambda chunk: [1, 3, 4, 5, 63, 64, 65, 255, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 3]
# storage offsets (elements past a 16-byte-aligned address) of (p, g, m, v): all aligned -> the vector path; any other -> the element path
OFFSETS = [(0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 2, 3), (2, 0, 0, 0), (0, 0, 0, 3), (0, 3, 0, 0)]


# ------------------------------------------------------------------------------------------------------------ CPU part
def _torch_run(specs, dtype, cls=torch.optim.Adam, **kw):
    """specs: [{p0, lr, betas, eps, grads: [array or None per step]}] -> [(p, m, v, step)] after all steps, one group per tensor"""
    ps = [torch.nn.Parameter(torch.from_numpy(np.asarray(s["p0"])).to(dtype).clone()) for s in specs]
    opt = cls([{"params": [p], "lr": s["lr"], "betas": s["betas"], "eps": s["eps"]} for p, s in zip(ps, specs)], lr=0.0, **kw)
    for k in range(len(specs[0]["grads"])):
        for p, s in zip(ps, specs):
            g = s["grads"][k]
            p.grad = None if g is None else torch.from_numpy(np.asarray(g)).to(dtype).clone()
        opt.step()
    out = []
    for p in ps:
        st = opt.state.get(p) or {}
        z = np.zeros(p.shape)
        out.append((p.detach().double().numpy(), st["exp_avg"].double().numpy() if st else z, st["exp_avg_sq"].double().numpy() if st else z,
                    float(st["step"]) if st else 0.0))
    return out


def _ref_run(specs, variant=None):
    out = []
    for s in specs:
        r = ar.RefTensor(s["p0"], s["lr"], s["betas"], s["eps"], variant)
        for g in s["grads"]:
            r.step(g)
        out.append((r.p, r.m, r.v, float(r.t)))
    return out


def _pin_specs():
    rng = np.random.default_rng(7)
    groups = [(1e-2, (0.9, 0.999), 1e-15), (0.0, (0.8, 0.99), 1e-8), (3e-3, (0.95, 0.9), 1e-12)]
    specs = []
    for i, (lr, betas, eps) in enumerate(groups):
        n = 200 + i
        grads = [ar.gradient(rng, (n,), zeros_every=7 if k == 2 else 0).astype(np.float64) for k in range(5)]
        if i == 2:
            grads[1] = grads[2] = None   # no gradient on steps 2 and 3
        specs.append({"p0": rng.standard_normal(n) * 3, "lr": lr, "betas": betas, "eps": eps, "grads": grads})
    return specs


def _rel_to_max(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_the_restatement_agrees_with_torch_in_float64_and_its_mutations_do_not():
    specs = _pin_specs()
    want = _torch_run(specs, torch.float64, foreach=False)
    worst = {None: 0.0, "swapped_betas": 0.0, "no_bias_correction": 0.0}
    for variant in worst:
        got = _ref_run(specs, variant)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a[3] == b[3], "step counts"
            for q in range(3):
                if specs[i]["lr"] == 0.0 and q == 0:
                    assert np.array_equal(a[0], specs[i]["p0"])   # lr = 0: p does not move in either
                worst[variant] = max(worst[variant], _rel_to_max(a[q], b[q]))
    print("adam restatement vs torch float64:", worst)
    assert want[2][3] == 3.0 and want[0][3] == 5.0
    assert worst[None] <= 1e-14
    assert worst["swapped_betas"] > 1e-14 * 1e6 and worst["no_bias_correction"] > 1e-14 * 1e6


def test_construction_takes_the_references_forms_and_refuses_the_rest():
    from hugs_amd.optim import Adam
    names = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
    mk = lambda: [{"params": [torch.nn.Parameter(torch.zeros(5, 3))], "lr": 1e-3 * (i + 1), "name": n} for i, n in enumerate(names)]
    ours, theirs = Adam(mk(), lr=0.0, eps=1e-15), torch.optim.Adam(mk(), lr=0.0, eps=1e-15)                      # scene.py:213
    assert [set(g) for g in ours.param_groups] == [set(g) for g in theirs.param_groups]
    assert ours.defaults == theirs.defaults
    for a, b in zip(ours.param_groups, theirs.param_groups):
        assert {k: v for k, v in a.items() if k != "params"} == {k: v for k, v in b.items() if k != "params"}
    # hugs_trimlp.py:690-701: groups of several tensors, a plain list of groups
    net = torch.nn.Sequential(torch.nn.Linear(4, 8), torch.nn.Linear(8, 2))
    h = Adam([{"params": [torch.nn.Parameter(torch.zeros(7, 3))], "lr": 1e-4, "name": "xyz"},
              {"params": net.parameters(), "lr": 1e-3, "name": "geometry_dec"}], lr=0.0, eps=1e-15)
    assert len(h.param_groups) == 2 and len(h.param_groups[1]["params"]) == 4
    Adam([torch.nn.Parameter(torch.zeros(2))], foreach=True), Adam([torch.nn.Parameter(torch.zeros(2))], fused=True)   # accepted, ignored
    for kw in ({"weight_decay": 0.1}, {"amsgrad": True}, {"maximize": True}, {"capturable": True}, {"differentiable": True}):
        with pytest.raises(NotImplementedError):
            Adam([torch.nn.Parameter(torch.zeros(2))], **kw)
    with pytest.raises(NotImplementedError):
        Adam([{"params": [torch.nn.Parameter(torch.zeros(2))], "weight_decay": 0.5}])
    with pytest.raises(ValueError):
        Adam([torch.nn.Parameter(torch.zeros(2))], betas=(0.9, 1.5))   # torch's own validation
    # state dicts go both ways on the CPU too (no step is taken here)
    theirs.load_state_dict(ours.state_dict()), ours.load_state_dict(theirs.state_dict())
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Adam([p]).step()


def _lib():
    import diff_gaussian_rasterization as dgr
    from hugs_amd import optim as O
    return dgr._load(), O._RECORD   # with the prototypes the wrapper calls through (diff_gaussian_rasterization/_abi.py)


def _table(buf):
    """packed records as the array of hgs_adam_tensor mirrors the bound prototype takes"""
    from diff_gaussian_rasterization._abi import _AdamTensor
    return (_AdamTensor * (len(buf) // C.sizeof(_AdamTensor))).from_buffer(buf) if buf else None


def _call(lib, n, blob):
    return lib.hgs_adam_step(_table(bytearray(blob)), n, None)


GOOD = (16, 32, 48, 64, 5, 0.1, 0.999, 0.001, 1e-15, 0.01, 0.03)
BAD = {"null pointer": [(0,) + GOOD[1:], GOOD[:1] + (0,) + GOOD[2:], GOOD[:2] + (0,) + GOOD[3:], GOOD[:3] + (0,) + GOOD[4:]],
       "not 4-byte aligned": [(18,) + GOOD[1:], GOOD[:1] + (33,) + GOOD[2:], GOOD[:2] + (50,) + GOOD[3:], GOOD[:3] + (67,) + GOOD[4:]],
       "numel < 0": [GOOD[:4] + (-1,) + GOOD[5:]],
       "non-finite": [GOOD[:5 + i] + (bad,) + GOOD[6 + i:] for i in range(6) for bad in (float("nan"), float("inf"))],
       "bc2_sqrt <= 0": [GOOD[:10] + (0.0,), GOOD[:10] + (-0.5,)]}


def test_the_c_abi_validates_before_any_launch():
    """No GPU is needed: every rejected form returns HGS_ERR_INVALID_ARGUMENT (-1; a launch attempted here would be HGS_ERR_HIP, -3)
    with its message, also when the bad record follows good ones."""
    lib, R = _lib()
    k, chunk = C.c_int32(0), C.c_int32(0)
    lib.hgs_adam_limits(C.byref(k), C.byref(chunk))
    assert k.value >= 48 and chunk.value >= 256 and R.size == 64 and k.value * R.size + 4 * (k.value + 1) <= 4096
    assert _call(lib, 0, b"") == 0 and lib.hgs_adam_step(None, 0, None) == 0           # n == 0: a no-op
    assert _call(lib, -1, R.pack(*GOOD)) == -1 and b"n < 0" in lib.hgs_last_error()
    assert lib.hgs_adam_step(None, 1, None) == -1 and b"null" in lib.hgs_last_error()
    for what, recs in BAD.items():
        for rec in recs:
            assert _call(lib, 1, R.pack(*rec)) == -1 and what.encode() in lib.hgs_last_error(), (what, rec, lib.hgs_last_error())
            assert _call(lib, 3, R.pack(*GOOD) * 2 + R.pack(*rec)) == -1 and what.encode() in lib.hgs_last_error(), (what, rec)
    # numel == 0 with null pointers is legal (an empty tensor's data pointer is null) and launches nothing
    assert _call(lib, 1, R.pack(0, 0, 0, 0, 0, *GOOD[5:])) == 0


# ------------------------------------------------------------------------------------------------------------ GPU part
def _spec(rng, n, offs=(0, 0, 0, 0), lr=1e-2, betas=(0.9, 0.999), eps=EPS, steps=3, no_grad_on=(), shape=None):
    shape = (n,) if shape is None else shape
    grads = [None if k + 1 in no_grad_on else ar.gradient(rng, shape, zeros_every=7 if k == 1 else 0) for k in range(steps)]
    return {"p0": (rng.standard_normal(shape) * 3).astype(np.float32), "lr": lr, "betas": betas, "eps": eps, "grads": grads, "offs": offs}


class _Views:
    """One tensor's four device views (p, g, m, v), each `off` elements past a 16-byte-aligned address inside a buffer with GUARD
    elements of noise on both sides; remembers the buffers' bits."""

    def __init__(self, device, rng, s):
        n = int(np.prod(s["p0"].shape))
        self.n, self.bufs, self.views = n, [], []
        for which, off in zip("pgmv", s["offs"]):
            host = rng.standard_normal(GUARD + off + n + GUARD).astype(np.float32)
            if which == "p":
                host[GUARD + off: GUARD + off + n] = s["p0"].reshape(-1)
            elif which in "mv":
                host[GUARD + off: GUARD + off + n] = 0.0
            buf = torch.from_numpy(host).to(device)
            assert buf.data_ptr() % 16 == 0
            self.bufs.append(buf)
            self.views.append(buf[GUARD + off: GUARD + off + n].view(s["p0"].shape))
        self.before = [b.clone() for b in self.bufs]
        self.offs = s["offs"]

    def guards_untouched(self):
        for which, off, buf, before in zip("pgmv", self.offs, self.bufs, self.before):
            lo, hi = GUARD + off, GUARD + off + self.n
            a, b = buf.view(torch.int32), before.view(torch.int32)
            if which == "g":
                assert torch.equal(a, b), "a gradient was written"
            else:
                assert torch.equal(a[:lo], b[:lo]) and torch.equal(a[hi:], b[hi:]), f"guard elements of {which} changed"


def _hip_run(device, rng, specs, stepper=None, seed_state=True):
    """The specs through hugs_amd.optim.Adam on views with guards -> ([(p, m, v, step)], optimizer, views)"""
    from hugs_amd.optim import Adam
    views = [_Views(device, rng, s) for s in specs]
    ps = [v.views[0].detach().requires_grad_(True) for v in views]
    opt = Adam([{"params": [p], "lr": s["lr"], "betas": s["betas"], "eps": s["eps"]} for p, s in zip(ps, specs)], lr=0.0)
    if seed_state:   # the moments as views at their own offsets (torch's state, put there the way the reference's surgery does)
        for p, v in zip(ps, views):
            opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": v.views[2], "exp_avg_sq": v.views[3]}
    for k in range(len(specs[0]["grads"])):
        for p, s, v in zip(ps, specs, views):
            if s["grads"][k] is None:
                p.grad = None
            else:
                v.views[1].copy_(torch.from_numpy(s["grads"][k]))
                v.before[1] = v.bufs[1].clone()
                p.grad = v.views[1]
        (stepper or (lambda o: o.step()))(opt)
    torch.cuda.synchronize()
    out = []
    for p, v in zip(ps, views):
        st = opt.state.get(p) or None
        v.guards_untouched()
        z = np.zeros(p.shape)
        out.append((p.detach().cpu().double().numpy(), st["exp_avg"].cpu().double().numpy() if st else z,
                    st["exp_avg_sq"].cpu().double().numpy() if st else z, float(st["step"]) if st else 0.0))
    return out, opt, views


def _assert_bar(label, got, specs, ref=None, yard=None):
    """the bar of the module docstring, every figure printed first; returns the figures"""
    ref = _ref_run(specs) if ref is None else ref
    yard = _torch_run(specs, torch.float32, foreach=False) if yard is None else yard
    bad = []
    for i, (h, r, y) in enumerate(zip(got, ref, yard)):
        assert h[3] == r[3] == y[3], (label, i, "step counts", h[3], r[3], y[3])
        for q, name in enumerate(("p", "exp_avg", "exp_avg_sq")):
            err, ys, scale = float(np.abs(h[q] - r[q]).max(initial=0.0)), float(np.abs(y[q] - r[q]).max(initial=0.0)), float(np.abs(r[q]).max(initial=0.0))
            floor = err > 4 * ys
            print(f"adam-ratio {label} t{i}[{h[q].size}] {name} {err / ys if ys else (0.0 if err == 0 else float('inf')):.3f} {'floor' if floor else '-'}")
            if not err <= 4 * ys + 1e-6 * scale:
                bad.append((label, i, name, err, ys, scale))
    assert not bad, bad


@pytest.fixture(scope="module")
def limits():
    from hugs_amd.optim import adam_limits
    return adam_limits()


@pytest.mark.gpu
@pytest.mark.parametrize("offs", OFFSETS, ids=lambda o: "p%dg%dm%dv%d" % o)
def test_every_size_at_every_alignment(device, limits, offs):
    """13 sizes around the vector width, the wave, the workgroup and the chunk, as views at the given element offsets: the vector and
    the element path, chunk boundaries, tails; guard elements stay bit for bit."""
    rng = np.random.default_rng(100 + sum(o << (2 * i) for i, o in enumerate(offs)))
    specs = [_spec(rng, n, offs) for n in SIZES(limits[1])]
    got, _, _ = _hip_run(device, rng, specs)
    _assert_bar("sizes-%d%d%d%d" % offs, got, specs)


@pytest.mark.gpu
@pytest.mark.parametrize("count", ["1", "2", "K-1", "K", "K+1", "2K+1"])
def test_tensor_counts_around_the_table_size(device, limits, count):
    K, chunk = limits
    n_t = {"1": 1, "2": 2, "K-1": K - 1, "K": K, "K+1": K + 1, "2K+1": 2 * K + 1}[count]
    rng = np.random.default_rng(200 + n_t)
    sizes = SIZES(chunk)
    # sizes and alignments mixed inside one table: both paths in one launch, and the tensors behind the K-th in a second one
    specs = [_spec(rng, sizes[(5 * i + 3) % len(sizes)], OFFSETS[i % len(OFFSETS)], lr=1e-2 * (1 + i % 3), steps=2) for i in range(n_t)]
    got, _, _ = _hip_run(device, rng, specs)
    _assert_bar(f"count-{count}", got, specs)


@pytest.mark.gpu
def test_a_parameter_without_gradient_and_an_empty_one(device, limits):
    rng = np.random.default_rng(3)
    specs = [_spec(rng, 257, (0, 0, 0, 0)), _spec(rng, limits[1] + 1, (1, 0, 2, 0), no_grad_on=(1, 2, 3)), _spec(rng, 65, (0, 1, 0, 0)),
             _spec(rng, 0)]
    got, opt, views = _hip_run(device, rng, specs)
    _assert_bar("skipped", got, specs)
    # the one without a gradient: every bit of p, m and v as it was (the guards' check covers the rest of its buffers), step still 0
    for buf, before in zip(views[1].bufs, views[1].before):
        assert torch.equal(buf.view(torch.int32), before.view(torch.int32))
    assert got[1][3] == 0.0 and got[0][3] == got[2][3] == got[3][3] == 3.0
    # ... and without seeded state it gets none at all
    got2, opt2, _ = _hip_run(device, np.random.default_rng(3), specs, seed_state=False)
    assert not opt2.state.get(opt2.param_groups[1]["params"][0])
    for a, b in ((0, 0), (2, 2)):
        assert all(np.array_equal(got[a][q], got2[b][q]) for q in range(3))


@pytest.mark.gpu
def test_every_tensor_has_its_own_scalars_and_step_count(device, limits):
    rng = np.random.default_rng(4)
    steps = 5
    specs = [_spec(rng, 1000, (0, 0, 0, 0), lr=1e-2, betas=(0.9, 0.999), eps=EPS, steps=steps),
             _spec(rng, 1001, (0, 0, 0, 0), lr=3e-3, betas=(0.8, 0.99), eps=1e-8, steps=steps),
             _spec(rng, limits[1] + 5, (1, 1, 1, 1), lr=5e-2, betas=(0.95, 0.9), eps=1e-12, steps=steps, no_grad_on=(1, 2)),   # joins at step 3
             _spec(rng, 515, (0, 0, 0, 0), lr=0.0, steps=steps)]
    got, _, _ = _hip_run(device, rng, specs)
    _assert_bar("scalars", got, specs)
    assert [g[3] for g in got] == [5.0, 5.0, 3.0, 5.0]
    assert np.array_equal(got[3][0].astype(np.float32).view(np.int32), specs[3]["p0"].view(np.int32)), "lr = 0 must leave p's bits alone"
    assert np.abs(got[3][1]).max() > 0 and np.abs(got[3][2]).max() > 0


@pytest.mark.gpu
def test_channels_last_parameters_walk_their_own_storage(device):
    """The triplane's planes: the moments take the parameter's strides, a gradient may arrive contiguous -> one copy, counted."""
    from hugs_amd import optim as O
    rng = np.random.default_rng(5)
    s = _spec(rng, 0, steps=2, shape=(1, 8, 5, 7))
    t = lambda a: torch.from_numpy(a).to(device)

    def run(param_cl, grad_cl):
        p = t(s["p0"])
        p = (p.contiguous(memory_format=torch.channels_last) if param_cl else p).detach().requires_grad_(True)
        opt = O.Adam([{"params": [p], "lr": 1e-2}], lr=0.0, eps=EPS)
        O.layout_copies(reset=True)
        copies = []
        for g in s["grads"]:
            g = t(g)
            p.grad = g.contiguous(memory_format=torch.channels_last) if grad_cl else g
            opt.step()
            copies.append(O.layout_copies(reset=True))
        st = opt.state[p]
        assert st["exp_avg"].stride() == p.stride() == st["exp_avg_sq"].stride()
        return (p.detach().cpu(), st["exp_avg"].cpu(), st["exp_avg_sq"].cpu()), copies

    flat, c0 = run(False, False)
    cl_contig_grad, c1 = run(True, False)
    cl_cl_grad, c2 = run(True, True)
    assert c0 == [0, 0] and c1 == [1, 1] and c2 == [0, 0], (c0, c1, c2)
    for a, b, c in zip(flat, cl_contig_grad, cl_cl_grad):
        assert torch.equal(a, b) and torch.equal(a, c)
    got = [tuple(x.double().numpy() for x in flat) + (2.0,)]
    _assert_bar("channels-last", got, [s])
    # moments that lost the parameter's layout (a checkpoint of contiguous tensors) are brought back once and stored
    p = t(s["p0"]).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    opt = O.Adam([p], lr=1e-2)
    opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.zeros(1, 8, 5, 7, device=device), "exp_avg_sq": torch.zeros(1, 8, 5, 7, device=device)}
    p.grad = t(s["grads"][0]).contiguous(memory_format=torch.channels_last)
    opt.step(), opt.step()
    assert O.layout_copies(reset=True) == 2 and opt.state[p]["exp_avg"].stride() == p.stride()
    # an expanded parameter has fewer elements of storage than of tensor
    e = torch.zeros(3, 1, device=device).expand(3, 4).detach().requires_grad_(True)
    e.grad = torch.ones(3, 4, device=device)
    with pytest.raises(RuntimeError, match="non-overlapping and dense"):
        O.Adam([e]).step()
    # sparse gradients, other dtypes
    q = torch.zeros(4, 2, device=device, requires_grad=True)
    q.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 2)).to(device)
    with pytest.raises(RuntimeError, match="sparse"):
        O.Adam([q]).step()
    h = torch.zeros(4, device=device, dtype=torch.float64, requires_grad=True)
    h.grad = torch.ones(4, device=device, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="float32"):
        O.Adam([h]).step()


@pytest.mark.gpu
def test_the_step_is_in_place_and_autograd_sees_it(device):
    from hugs_amd.optim import Adam
    p = torch.randn(1000, 3, device=device, requires_grad=True)
    opt = Adam([p], lr=1e-2)
    p.grad = torch.randn(1000, 3, device=device)
    opt.step()
    st = opt.state[p]
    ts = (p, st["exp_avg"], st["exp_avg_sq"])
    ptrs, versions = [t.data_ptr() for t in ts], [t._version for t in ts]
    opt.step()
    assert [t.data_ptr() for t in ts] == ptrs and opt.state[p]["exp_avg"] is ts[1] and opt.state[p]["exp_avg_sq"] is ts[2]
    assert all(t._version > v for t, v in zip(ts, versions))
    assert st["step"].device.type == "cpu" and float(st["step"]) == 2.0


@pytest.mark.gpu
def test_two_runs_give_the_same_bits_at_36_tensors(device, limits):
    sizes = SIZES(limits[1])
    runs = []
    for _ in range(2):
        rng = np.random.default_rng(6)
        specs = [_spec(rng, sizes[i % len(sizes)], OFFSETS[i % len(OFFSETS)], steps=2) for i in range(36)]
        runs.append(_hip_run(device, rng, specs)[0])
    for a, b in zip(*runs):
        assert all(np.array_equal(a[q], b[q]) for q in range(3))


def _gpu_torch_then(device, specs, first, second, device_step=False):
    """three steps with one optimizer class, state_dict() into the other, three more"""
    from hugs_amd.optim import Adam
    cls = {"torch": torch.optim.Adam, "hip": Adam}
    ps = [torch.from_numpy(s["p0"].copy()).to(device).requires_grad_(True) for s in specs]
    groups = lambda: [{"params": [p], "lr": s["lr"], "betas": s["betas"], "eps": s["eps"]} for p, s in zip(ps, specs)]

    grads = [[torch.from_numpy(g).to(device) for g in s["grads"]] for s in specs]   # (uploaded up front: a pageable copy waits for the device)

    def steps(opt, ks):
        for k in ks:
            for p, g in zip(ps, grads):
                p.grad = g[k]
            opt.step()

    a = cls[first](groups(), lr=0.0)
    steps(a, range(3))
    sd = a.state_dict()
    if device_step:
        for st in sd["state"].values():
            st["step"] = st["step"].to(device)
    b = cls[second](groups(), lr=0.0)
    b.load_state_dict(sd)
    if second == "hip":
        assert all(b.state[p]["step"].device.type == "cpu" and float(b.state[p]["step"]) == 3.0 for p in ps)
    if device_step:
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")   # from here on a host synchronisation raises
    try:
        steps(b, range(3, 6))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return [(p.detach().cpu().double().numpy(), b.state[p]["exp_avg"].cpu().double().numpy(), b.state[p]["exp_avg_sq"].cpu().double().numpy(),
             float(b.state[p]["step"])) for p in ps]


@pytest.fixture(scope="module")
def interchange_case():
    rng = np.random.default_rng(8)
    specs = [_spec(rng, 3000, lr=1e-2, steps=6), _spec(rng, 777, lr=2e-3, betas=(0.8, 0.99), steps=6)]
    return specs, _ref_run(specs), _torch_run(specs, torch.float32, foreach=False)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["torch-then-hip", "hip-then-torch", "device-step"])
def test_state_dicts_interchange_with_torch(device, interchange_case, order):
    specs, ref, yard = interchange_case
    first, second = ("hip", "torch") if order == "hip-then-torch" else ("torch", "hip")
    got = _gpu_torch_then(device, specs, first, second, device_step=order == "device-step")
    _assert_bar(f"interchange-{order}", got, specs, ref, yard)


class _Model:
    """scene.py:310-379 restated: one group per tensor, `replace_tensor_to_optimizer`, `_prune_optimizer`, `cat_tensors_to_optimizer`."""

    def __init__(self, params, opt_cls, lrs, **kw):
        self.p = {k: torch.nn.Parameter(v.clone().requires_grad_(True)) for k, v in params.items()}
        self.optimizer = opt_cls([{"params": [self.p[k]], "lr": lrs[k], "name": k} for k in params], lr=0.0, eps=EPS, **kw)

    def replace_tensor_to_optimizer(self, tensor, name):
        for group in self.optimizer.param_groups:
            if group["name"] == name:
                stored_state = self.optimizer.state.get(group["params"][0], None)
                stored_state["exp_avg"] = torch.zeros_like(tensor)
                stored_state["exp_avg_sq"] = torch.zeros_like(tensor)
                del self.optimizer.state[group["params"][0]]
                group["params"][0] = torch.nn.Parameter(tensor.requires_grad_(True))
                self.optimizer.state[group["params"][0]] = stored_state
                self.p[name] = group["params"][0]

    def _prune_optimizer(self, mask):
        for group in self.optimizer.param_groups:
            stored_state = self.optimizer.state.get(group["params"][0], None)
            if stored_state is not None:
                stored_state["exp_avg"] = stored_state["exp_avg"][mask]
                stored_state["exp_avg_sq"] = stored_state["exp_avg_sq"][mask]
                del self.optimizer.state[group["params"][0]]
                group["params"][0] = torch.nn.Parameter(group["params"][0][mask].requires_grad_(True))
                self.optimizer.state[group["params"][0]] = stored_state
            else:
                group["params"][0] = torch.nn.Parameter(group["params"][0][mask].requires_grad_(True))
            self.p[group["name"]] = group["params"][0]

    def cat_tensors_to_optimizer(self, tensors_dict):
        for group in self.optimizer.param_groups:
            assert len(group["params"]) == 1
            extension_tensor = tensors_dict[group["name"]]
            stored_state = self.optimizer.state.get(group["params"][0], None)
            if stored_state is not None:
                stored_state["exp_avg"] = torch.cat((stored_state["exp_avg"], torch.zeros_like(extension_tensor)), dim=0)
                stored_state["exp_avg_sq"] = torch.cat((stored_state["exp_avg_sq"], torch.zeros_like(extension_tensor)), dim=0)
                del self.optimizer.state[group["params"][0]]
                group["params"][0] = torch.nn.Parameter(torch.cat((group["params"][0], extension_tensor), dim=0).requires_grad_(True))
                self.optimizer.state[group["params"][0]] = stored_state
            else:
                group["params"][0] = torch.nn.Parameter(torch.cat((group["params"][0], extension_tensor), dim=0).requires_grad_(True))
            self.p[group["name"]] = group["params"][0]


@pytest.mark.gpu
def test_the_references_optimizer_surgery_works_unchanged(device):
    """300 rows, steps, prune 100, steps, append 50, steps, reset one group, steps -- through hugs_amd.optim.Adam on the GPU, through
    torch.optim.Adam in float32 on the CPU (the yardstick) and through the float64 restatement."""
    from hugs_amd.optim import Adam
    rng = np.random.default_rng(9)
    shapes = {"xyz": (3,), "opacity": (1,), "f_rest": (15, 3)}
    lrs = {"xyz": 1.6e-4 * 50, "opacity": 5e-2, "f_rest": 2.5e-3 / 20}
    p0 = {k: (rng.standard_normal((300,) + s) * 3).astype(np.float32) for k, s in shapes.items()}
    keep = np.ones(300, bool)
    keep[rng.permutation(300)[:100]] = False
    extra = {k: (rng.standard_normal((50,) + s) * 3).astype(np.float32) for k, s in shapes.items()}
    reset = np.minimum(rng.standard_normal((250, 1)).astype(np.float32), -2.0)
    grads = [{k: ar.gradient(rng, (rows,) + s, zeros_every=7 if i % 2 else 0) for k, s in shapes.items()}
             for i, rows in enumerate([300, 300, 200, 200, 250, 250, 250, 250])]
    grads[0]["f_rest"] = None   # f_rest has no state yet when the rows are pruned ... (the surgery's `else` branches)
    grads[1]["f_rest"] = None

    def through(dev, cls, **kw):
        t = lambda a: torch.from_numpy(a.copy()).to(dev)   # (a copy: on the CPU .to() would share the array with the model)
        m = _Model({k: t(v) for k, v in p0.items()}, cls, lrs, **kw)

        def steps(ks):
            for k in ks:
                for name, p in m.p.items():
                    p.grad = None if grads[k][name] is None else t(grads[k][name])
                m.optimizer.step()
                m.optimizer.zero_grad(set_to_none=True)
        steps((0, 1))
        m._prune_optimizer(t(keep))
        steps((2, 3))
        m.cat_tensors_to_optimizer({k: t(v) for k, v in extra.items()})
        steps((4, 5))
        m.replace_tensor_to_optimizer(t(reset), "opacity")
        steps((6, 7))
        if dev.type == "cuda":
            torch.cuda.synchronize()
        out = []
        for name in shapes:
            st = m.optimizer.state[m.p[name]]
            out.append((m.p[name].detach().cpu().double().numpy(), st["exp_avg"].cpu().double().numpy(), st["exp_avg_sq"].cpu().double().numpy(), float(st["step"])))
        return out

    refs = {k: ar.RefTensor(p0[k], lrs[k], (0.9, 0.999), EPS) for k in shapes}
    step_ref = lambda ks: [refs[n].step(grads[k][n]) for k in ks for n in shapes]
    step_ref((0, 1))
    [r.prune(keep) for r in refs.values()]
    step_ref((2, 3))
    [refs[k].cat(extra[k]) for k in shapes]
    step_ref((4, 5))
    refs["opacity"].replace(reset)
    step_ref((6, 7))
    ref = [(refs[k].p, refs[k].m, refs[k].v, float(refs[k].t)) for k in shapes]
    assert [r[3] for r in ref] == [8.0, 8.0, 6.0] and ref[0][0].shape == (250, 3)
    yard = through(torch.device("cpu"), torch.optim.Adam, foreach=False)
    got = through(device, Adam)
    _assert_bar("surgery", got, [None] * 3, ref, yard)


@pytest.mark.gpu
def test_fused_step_of_two_optimizers_is_their_two_steps(device, limits):
    from hugs_amd.optim import Adam, fused_step
    sizes = SIZES(limits[1])

    def run(fused):
        rng = np.random.default_rng(10)
        ps = [torch.from_numpy((rng.standard_normal(sizes[i % len(sizes)]) * 3).astype(np.float32)).to(device).requires_grad_(True) for i in range(42)]
        a = Adam([{"params": [p], "lr": 1e-3 * (i + 1)} for i, p in enumerate(ps[:6])], lr=0.0, eps=EPS)
        b = Adam([{"params": ps[6 + 4 * i: 10 + 4 * i], "lr": 2e-3 * (i + 1)} for i in range(9)], lr=0.0, eps=EPS)
        for k in range(3):
            for i, p in enumerate(ps):
                p.grad = None if (k == 1 and i == 20) else torch.from_numpy(ar.gradient(rng, p.shape)).to(device)
            if fused:
                fused_step(a, b)
            else:
                a.step(), b.step()
        torch.cuda.synchronize()
        st = lambda p: (a if p in a.state else b).state[p]
        return [(p.detach().cpu(), st(p)["exp_avg"].cpu(), st(p)["exp_avg_sq"].cpu(), float(st(p)["step"])) for p in ps]

    for x, y in zip(run(False), run(True)):
        assert x[3] == y[3] and all(torch.equal(x[q].view(torch.int32), y[q].view(torch.int32)) for q in range(3))
    with pytest.raises(TypeError):
        fused_step(torch.optim.Adam([torch.zeros(1, device=device, requires_grad=True)]))


@pytest.mark.gpu
def test_a_rejected_table_launches_nothing(device, limits):
    """2K + 1 records, the LAST one bad: a negative code, the message, and not a bit of the good tensors changed."""
    lib, R = _lib()
    K = limits[0]
    n = 2 * K + 1
    bufs = [torch.rand(4, 300, device=device) for _ in range(n)]
    before = [b.clone() for b in bufs]
    good = lambda b: R.pack(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), 300, *GOOD[5:])
    head = b"".join(good(b) for b in bufs[:-1])
    last = bufs[-1]
    ptrs = [last[i].data_ptr() for i in range(4)]
    stream = torch.cuda.current_stream(device).cuda_stream
    for what, recs in BAD.items():
        for rec in recs:
            rec = tuple(p if r in GOOD[:4] else (p + r % 16 if r else 0) for p, r in zip(ptrs, rec[:4])) + rec[4:]
            buf = bytearray(head + R.pack(*rec))
            rc = lib.hgs_adam_step(_table(buf), n, stream)
            assert rc < 0 and what.encode() in lib.hgs_last_error(), (what, rec)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(bufs, before))
    buf = bytearray(head + good(last))   # ... and the same table with a good last record runs
    assert lib.hgs_adam_step(_table(buf), n, stream) == 0
    torch.cuda.synchronize()
    assert all(not torch.equal(a[0], b[0]) for a, b in zip(bufs, before)) and all(torch.equal(a[1], b[1]) for a, b in zip(bufs, before))


@pytest.mark.gpu
def test_one_launch_per_optimizer_and_one_for_both(device):
    """6 + 37 tensors, the reference's two optimizers: the profiler sees one kernel per step() and one per fused_step(), nothing else."""
    from torch.profiler import ProfilerActivity, profile
    from hugs_amd.optim import Adam, fused_step
    ps = [torch.randn(100 + i, device=device, requires_grad=True) for i in range(43)]
    gs = [torch.randn_like(p) for p in ps]
    a = Adam([{"params": [p], "lr": 1e-3} for p in ps[:6]], lr=0.0, eps=EPS)
    b = Adam([{"params": ps[6 + 4 * i: 10 + 4 * i], "lr": 1e-3} for i in range(8)] + [{"params": ps[38:], "lr": 1e-3}], lr=0.0, eps=EPS)

    def launches(fn):
        for _ in range(2):   # (the first call creates the state: fills)
            for p, g in zip(ps, gs):
                p.grad = g
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
        events = list(prof.events())
        # (a record_function range around kernels -- Optimizer.step's own -- is mirrored on the device side under the same name: not a launch)
        host = {e.name for e in events if not str(e.device_type).endswith("CUDA")}
        names = [e.name for e in events if str(e.device_type).endswith("CUDA") and e.name not in host and not e.name.startswith("Optimizer.step#")]
        return len(names), len([n for n in names if "adam_multi_tensor_kernel" in n])

    assert launches(a.step) == (1, 1) and launches(b.step) == (1, 1)
    assert launches(lambda: (b.step(), a.step())) == (2, 2)
    assert launches(lambda: fused_step(b, a)) == (1, 1)
