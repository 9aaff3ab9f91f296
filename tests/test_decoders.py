"""Row f-9 -- the three human decoders fused (/root/reference/hugs/models/modules/decoders.py:24-111, called at
/root/reference/hugs/models/hugs_trimlp.py:409-410,430).

CPU: the float64 restatement (tests/decoders_ref.py) against the outputs and autograd gradients of the reference's own classes
(tests/golden/make_golden_decoders.py compiles them from /root/reference and runs them on CPU); the library's exports and host-side
validation; the modules' state_dict keys, parameter names, shapes and round trip; the forms that are not implemented.

GPU: the HIP kernels through `decoder_mlp` and the three modules.  Tolerance, per tensor (each head output, dL/dx, each parameter
gradient): the float64 restatement of the same float32 inputs is the truth, the yardstick comes from the reference's arithmetic alone,
    err_ref = max |torch_fp32_cpu - fp64|        (golden vectors: max |golden - fp64|)
and for a parameter gradient -- a sum over the n points -- the larger of err_ref and
    err_seq = the error of that same sum accumulated in float32 in point order (the float64 factors rounded to float32),
because a k-ordered fmaf chain is a legal float32 evaluation and can sit above a blocked CPU GEMM's error.  The requirement is
    max |hip - fp64| <= 4 yardstick + 1e-6 max |fp64|
(the factor and the floor are tests/test_triplane.py's rule).  Every figure is printed before it is asserted (pytest -s shows them).
At 110 210 points err_seq is taken over the first 8 input columns of each weight only (a lower bound of the full figure: stricter).

CPU bound of the restatement against the golden vectors, from the number formats (u = 2^-24), first order, propagated per point in
the 2-norm (`_rounding_bounds`): a dot product of K terms and a bias is off by at most (K + 2) u (|W| |a| + |b|), whatever its
summation order; an activation or its derivative adds 8 u of its value (erf and exp are good to a few ulps) and passes an error of
its argument on with |gelu'|, |gelu''|, |sigmoid'| <= 1.13; a layer passes an error of its input on with its spectral norm.  The
backward's errors follow the same way from gz = g act'(z) and dL/da = gz W; a parameter gradient collects, over the n points,
|d gz| |a| + |gz| |d a| and (n + 2) u sum |gz| |a| for the sum itself; weight norm's g and v take the effective weight's bound times
(|g| / |v| + 2) and the row length.  The bounds come out at 4e-4 .. 2e-3 on the outputs (values 0.2 .. 0.7; measured 5e-8 .. 4e-7),
1e-2 .. 4e-2 on dL/dx and 0.05 .. 7 on the parameter gradients (values 0.5 .. 26; measured 7e-8 .. 1e-5): a worst case over 200 points
ignores all cancellation.  A dropped row, a wrong activation or a transposed weight moves the outputs by 1e-2 and more, which the test
also asserts for a wrong head activation; the sharp check of the gradients is the GPU rule above.
No wall-clock assertion here: timing lives in tools/bench_decoders.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import decoders_ref as dr

_HERE = os.path.dirname(os.path.abspath(__file__))
G = dict(np.load(os.path.join(_HERE, "golden", "reference_decoders.npz")))
G.update(np.load(os.path.join(_HERE, "golden", "reference_decoders_grads.npz")))
TAGS = ("appearance", "geometry", "deformation")
TILE = 32          # the kernels' point tile (asserted against the library below)
FEATURES = 96
U = 2.0 ** -24


def _names(tag, what):
    return bytes(G[f"{tag}.{what}"]).decode().split(",")


def _state(tag):
    """the reference's state_dict as numpy arrays, alias keys resolved"""
    out = {}
    for k in _names(tag, "state_dict_keys"):
        out[k] = G[f"{tag}.state.{k}"] if f"{tag}.state.{k}" in G else G[f"{tag}.state.{bytes(G[f'{tag}.alias.{k}']).decode()}"]
    return out


def _weight_norm64(v, g):
    v, g = np.asarray(v, np.float64), np.asarray(g, np.float64)
    return g * v / np.sqrt((v * v).sum(1, keepdims=True))


def _network(tag, s, f64_weight_norm=False):
    """(trunk, heads, output keys) of a decoder from its state_dict arrays `s`"""
    trunk = [(s["net.0.weight"], s["net.0.bias"]), (s["net.2.weight"], s["net.2.bias"])]
    if tag == "appearance":
        return trunk, [(s["shs.weight"], s["shs.bias"], None), (s["opacity.0.weight"], s["opacity.0.bias"], "sigmoid")], ["shs", "opacity"]
    if tag == "geometry":
        return trunk, [(s["xyz.1.weight"], s["xyz.1.bias"], None), (s["rotations.1.weight"], s["rotations.1.bias"], None),
                       (s["scales.1.weight"], s["scales.1.bias"], "gelu")], ["xyz", "rotations", "scales"]
    v, g = s["skinning_linear.weight_v"], s["skinning_linear.weight_g"]
    w = _weight_norm64(v, g) if f64_weight_norm else torch._weight_norm(torch.from_numpy(v), torch.from_numpy(g), 0).numpy()
    return trunk + [(w, s["skinning_linear.bias"])], [(s["skinning.weight"], s["skinning.bias"], "gelu")], ["lbs_weights"]


def _param_grads64(tag, s, back):
    """the restatement's gradients keyed like named_parameters (weight norm's g and v from the effective weight's gradient)"""
    t, h = back["trunk"], back["heads"]
    out = {"net.0.weight": t[0][0], "net.0.bias": t[0][1], "net.2.weight": t[1][0], "net.2.bias": t[1][1]}
    if tag == "appearance":
        out.update({"opacity.0.weight": h[1][0], "opacity.0.bias": h[1][1], "shs.weight": h[0][0], "shs.bias": h[0][1]})
    elif tag == "geometry":
        for k, name in enumerate(("xyz", "rotations", "scales")):
            out[f"{name}.1.weight"], out[f"{name}.1.bias"] = h[k]
    else:
        v, g = np.asarray(s["skinning_linear.weight_v"], np.float64), np.asarray(s["skinning_linear.weight_g"], np.float64)
        norm = np.sqrt((v * v).sum(1, keepdims=True))
        dot = (t[2][0] * v).sum(1, keepdims=True)
        out.update({"skinning_linear.bias": t[2][1], "skinning_linear.weight_g": dot / norm,
                    "skinning_linear.weight_v": g / norm * (t[2][0] - dot / (norm * norm) * v),
                    "skinning.weight": h[0][0], "skinning.bias": h[0][1]})
    return out


def _rounding_bounds(x, trunk, heads, g_outs):
    """the bounds of the docstring: (outputs, dx, trunk [(dW, db)], heads [(dW, db)]), one number per tensor"""
    f = lambda a: np.abs(np.asarray(a, np.float64))
    n2 = lambda a: np.sqrt((a * a).sum(1))                      # per point
    spec = lambda W: float(np.linalg.norm(np.asarray(W, np.float64), 2))
    _, (acts, derivs, head_derivs) = dr.forward(x, trunk, heads)
    n = x.shape[0]
    e_a, e_d = [np.zeros(n)], []                                # 2-norm error of a_l and of gelu'(z_l), per point
    for l, (W, b) in enumerate(trunk):
        e_z = spec(W) * e_a[-1] + (W.shape[1] + 2) * U * n2(f(acts[l]) @ f(W).T + f(b))
        e_a.append(1.13 * e_z + 8 * U * n2(acts[l + 1]))
        e_d.append(1.13 * e_z + 8 * U * n2(derivs[l]))
    outs64, _ = dr.forward(x, trunk, heads)
    out_bounds, e_ga, head_bounds = [], np.zeros(n), []
    back = dr.backward(x, trunk, heads, g_outs)
    nt = len(trunk)
    for k, ((W, b, _), d, g) in enumerate(zip(heads, head_derivs, g_outs)):
        e_z = spec(W) * e_a[-1] + (W.shape[1] + 2) * U * n2(f(acts[-1]) @ f(W).T + f(b))
        out_bounds.append(float((1.13 * e_z + 8 * U * n2(outs64[k])).max()))
        gz, a = back["factors"][nt + k]
        e_gz = f(g).max(1) * (1.13 * e_z + 8 * U * n2(d)) + U * n2(gz)
        head_bounds.append((float((e_gz * f(a).max(1) + f(gz).max(1) * e_a[-1]).sum() + (n + 2) * U * (f(gz).T @ f(a)).max()),
                            float(e_gz.sum() + (n + 2) * U * f(gz).sum(0).max())))
        e_ga = e_ga + spec(W) * e_gz + (W.shape[0] + 2) * U * n2(f(gz) @ f(W))
    trunk_bounds = [None] * nt
    g_a = sum(back["factors"][nt + k][0] @ np.asarray(W, np.float64) for k, (W, _, _) in enumerate(heads))
    for l in range(nt - 1, -1, -1):
        gz, a = back["factors"][l]
        W = trunk[l][0]
        e_gz = 1.13 * e_ga + f(g_a).max(1) * e_d[l] + U * n2(gz)
        trunk_bounds[l] = (float((e_gz * f(a).max(1) + f(gz).max(1) * e_a[l]).sum() + (n + 2) * U * (f(gz).T @ f(a)).max()),
                           float(e_gz.sum() + (n + 2) * U * f(gz).sum(0).max()))
        e_ga = spec(W) * e_gz + (W.shape[0] + 2) * U * n2(f(gz) @ f(W))
        g_a = gz @ np.asarray(W, np.float64)
    return out_bounds, float(e_ga.max()), trunk_bounds, head_bounds


@pytest.mark.parametrize("tag", TAGS)
def test_fp64_restatement_reproduces_the_reference_outputs_and_gradients(tag):
    s = _state(tag)
    x = G["x"]
    trunk, heads, keys = _network(tag, s, f64_weight_norm=True)
    assert _names(tag, "output_keys")[:len(keys)] == keys
    g_outs = [G[f"{tag}.g_out.{k}"] for k in keys]
    outs, _ = dr.forward(x, trunk, heads)
    back = dr.backward(x, trunk, heads, g_outs)
    b_outs, b_dx, t, h = _rounding_bounds(x, trunk, heads, g_outs)

    def hold(name, got, want, bound):
        err, bound = np.abs(got - want).max(), bound + 1e-6 * np.abs(want).max()
        print(f"  {tag} {name}: |fp64 - golden| {err:.3e}  bound {bound:.3e}  max|golden| {np.abs(want).max():.4g}")
        assert got.shape == want.shape and err <= bound, (name, err, bound)

    for k, y, bound in zip(keys, outs, b_outs):
        hold(f"out {k}", y, G[f"{tag}.out.{k}"], bound)
    hold("dL/dx", back["dx"], G[f"{tag}.grad_x"], b_dx)
    grads = _param_grads64(tag, s, back)
    mags = {"net.0.weight": t[0][0], "net.0.bias": t[0][1], "net.2.weight": t[1][0], "net.2.bias": t[1][1]}
    if tag == "deformation":
        v, g = np.abs(s["skinning_linear.weight_v"]).astype(np.float64), np.abs(s["skinning_linear.weight_g"]).astype(np.float64)
        norm = np.sqrt((v * v).sum(1, keepdims=True))
        fct = float((g / norm).max() + 2.0) * v.shape[1]         # (dg is a row's dot product with v / |v|: at most its 128 entries' errors)
        mags.update({"skinning_linear.bias": t[2][1], "skinning_linear.weight_g": fct * t[2][0], "skinning_linear.weight_v": fct * t[2][0],
                     "skinning.weight": h[0][0], "skinning.bias": h[0][1]})
    else:
        for k, name in enumerate(("shs", "opacity.0") if tag == "appearance" else ("xyz.1", "rotations.1", "scales.1")):
            mags[f"{name}.weight"], mags[f"{name}.bias"] = h[k]
    assert list(grads) == _names(tag, "parameter_names")
    for n in grads:
        hold(f"dL/d{n}", grads[n].reshape(G[f"{tag}.grad.{n}"].shape), G[f"{tag}.grad.{n}"], mags[n])
    # a wrong activation on a head is far outside: the same check with gelu where the head has none / sigmoid
    wrong = [(W, b, "gelu" if kind != "gelu" else None) for W, b, kind in heads]
    assert np.abs(dr.forward(x, trunk, wrong)[0][0] - G[f"{tag}.out.{keys[0]}"]).max() > 1e-2


def _lib():
    import diff_gaussian_rasterization as dgr
    from hugs_amd import decoders
    return dgr._load(), decoders   # with the prototypes the wrapper calls through (diff_gaussian_rasterization/_abi.py)


def test_library_exports_the_entry_points_and_the_header_documents_the_row():
    lib, decoders = _lib()
    assert hasattr(lib, "hgs_mlp_forward") and hasattr(lib, "hgs_mlp_backward")
    assert decoders.tile_points() == TILE
    header = open(os.path.join(os.path.dirname(_HERE), "include", "hgs_rasterizer.h")).read()
    assert "Row f-9" in header and "hgs_mlp_forward(" in header and "hgs_mlp_backward(" in header
    assert "/root/reference/hugs/models/modules/decoders.py:24-111" in header and "hugs_trimlp.py:409-410,430" in header


def _fake_desc(decoders, in_width=96, widths=(128, 128), head_widths=(3, 6, 3), acts=(0, 0, 1), ptr=64):
    d = decoders._Desc()
    d.in_width, d.n_trunk, d.n_heads = in_width, len(widths), len(head_widths)
    for l, w in enumerate(widths[:3]):
        d.trunk_width[l], d.trunk_weight[l], d.trunk_bias[l] = w, ptr, ptr
    for k, w in enumerate(head_widths[:3]):
        d.head_width[k], d.head_act[k], d.head_weight[k], d.head_bias[k] = w, acts[k], ptr, ptr
    return d


def test_entry_points_validate_on_the_host_before_any_launch():
    """Every call here returns from the argument checks (there is no GPU in a CPU run): fake non-null pointers are never dereferenced."""
    lib, decoders = _lib()
    three = lambda *v: (C.c_void_p * 3)(*v)
    grads = decoders._Grads()
    grads.trunk_weight[0] = 64

    def fwd(n=4, d=None, x=64, outs=three(64, 64, 64)):
        return lib.hgs_mlp_forward(n, C.byref(d or _fake_desc(decoders)), x, outs, None)

    def bwd(n=4, d=None, x=64, g=three(64, 64, 64), dx=64, gr=grads):
        return lib.hgs_mlp_backward(n, C.byref(d or _fake_desc(decoders)), x, g, dx, None if gr is None else C.byref(gr), None)

    for call, what in ((fwd, b"mlp_forward"), (bwd, b"mlp_backward")):
        assert call(n=0) == 0                                                         # nothing to do, nothing touched
        assert call(n=-1) == -1 and what in lib.hgs_last_error() and b"n >= 0" in lib.hgs_last_error()
        for bad in (48, 0, 160):
            assert call(d=_fake_desc(decoders, in_width=bad)) == -1 and b"input width must be a multiple of 32 up to 128" in lib.hgs_last_error()
        assert call(d=_fake_desc(decoders, widths=(96, 96))) == -1 and b"trunk widths must be 64 or 128" in lib.hgs_last_error()
        assert call(d=_fake_desc(decoders, widths=(64, 128))) == -1 and b"same width" in lib.hgs_last_error()
        assert call(d=_fake_desc(decoders, widths=())) == -1 and b"1 to 3 trunk layers" in lib.hgs_last_error()
        d4 = _fake_desc(decoders)
        d4.n_trunk = 4
        assert call(d=d4) == -1 and b"1 to 3 trunk layers" in lib.hgs_last_error()
        assert call(d=_fake_desc(decoders, head_widths=())) == -1 and b"1 to 3 heads" in lib.hgs_last_error()
        d4 = _fake_desc(decoders)
        d4.n_heads = 4
        assert call(d=d4) == -1 and b"1 to 3 heads" in lib.hgs_last_error()
        assert call(d=_fake_desc(decoders, head_widths=(48, 16, 1))) == -1 and b"at most 64 head columns" in lib.hgs_last_error()
        assert call(d=_fake_desc(decoders, head_widths=(3, 0, 3))) == -1 and b"at least one column" in lib.hgs_last_error()
        assert call(d=_fake_desc(decoders, acts=(0, 3, 1))) == -1 and b"unknown activation code" in lib.hgs_last_error()
        d0 = _fake_desc(decoders)
        d0.trunk_bias[1] = None
        assert call(d=d0) == -1 and b"null trunk weight or bias" in lib.hgs_last_error()
        d0 = _fake_desc(decoders)
        d0.head_weight[2] = None
        assert call(d=d0) == -1 and b"null head weight or bias" in lib.hgs_last_error()
        assert call(x=None) == -1 and b"null pointer" in lib.hgs_last_error()
        assert call(x=68) == -1 and b"x must be 16-byte aligned" in lib.hgs_last_error()
    assert lib.hgs_mlp_forward(4, None, 64, three(64, 64, 64), None) == -1 and b"null network description" in lib.hgs_last_error()
    assert fwd(outs=None) == -1 and b"null pointer" in lib.hgs_last_error()
    assert fwd(outs=three(64, None, 64)) == -1 and b"null head output" in lib.hgs_last_error()
    assert fwd(outs=three(64, 72, 64)) == -1 and b"head output must be 16-byte aligned" in lib.hgs_last_error()
    assert bwd(g=None) == -1 and b"null pointer" in lib.hgs_last_error()
    assert bwd(g=three(64, 72, 64)) == -1 and b"head gradient must be 16-byte aligned" in lib.hgs_last_error()
    assert bwd(dx=72) == -1 and b"dL_dx must be 16-byte aligned" in lib.hgs_last_error()
    assert bwd(dx=None, gr=None) == 0 and bwd(dx=None, gr=decoders._Grads()) == 0     # nothing asked for: no launch
    assert bwd(g=three(None, None, None), dx=None) == 0                               # no head is used and no dL/dx: nothing to write


def _modules(use_surface=False):
    from hugs_amd.decoders import AppearanceDecoder, DeformationDecoder, GeometryDecoder
    return {"appearance": AppearanceDecoder(FEATURES), "geometry": GeometryDecoder(FEATURES, use_surface=use_surface),
            "deformation": DeformationDecoder(FEATURES, disable_posedirs=True)}


@pytest.mark.parametrize("tag", TAGS)
def test_modules_have_the_reference_state_dict_and_round_trip(tag):
    m = _modules()[tag]
    s = _state(tag)
    assert list(m.state_dict().keys()) == _names(tag, "state_dict_keys")
    assert [n for n, _ in m.named_parameters()] == _names(tag, "parameter_names")
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == s[k].shape and v.dtype == torch.float32, k
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in s.items()})
    saved = m.state_dict()
    assert list(saved) == list(s)
    for k in s:
        assert np.array_equal(saved[k].numpy(), s[k]), k


def test_module_constructors_and_initialisation_follow_the_reference():
    from hugs_amd.decoders import AppearanceDecoder, DeformationDecoder, GeometryDecoder
    assert tuple(GeometryDecoder(FEATURES, use_surface=True).scales[1].weight.shape) == (2, 128)
    assert tuple(AppearanceDecoder(64, hidden_dim=32).shs.weight.shape) == (48, 32)
    d = DeformationDecoder(FEATURES)                                   # disable_posedirs=False constructs, with zero blendshapes
    assert tuple(d.blendshapes.weight.shape) == (621, 128) and not d.blendshapes.weight.any() and not d.blendshapes.bias.any()
    assert not hasattr(DeformationDecoder(FEATURES, weight_norm=False).skinning_linear, "weight_g")
    g = GeometryDecoder(FEATURES)
    assert g.xyz[0] is g.net and g.rotations[0] is g.net and g.scales[0] is g.net
    # the same seed gives the reference's initial values: the parameters are created in its order by the same torch initialisers
    torch.manual_seed(3)
    a = AppearanceDecoder(FEATURES)
    torch.manual_seed(3)
    want = [torch.nn.Linear(FEATURES, 64), torch.nn.Linear(64, 64), torch.nn.Linear(64, 1), torch.nn.Linear(64, 48)]
    for got, ref in zip((a.net[0], a.net[2], a.opacity[0], a.shs), want):
        assert torch.equal(got.weight, ref.weight) and torch.equal(got.bias, ref.bias)


def test_unsupported_forms_raise_and_cpu_tensors_have_no_fallback():
    from hugs_amd.decoders import AppearanceDecoder, DeformationDecoder, GeometryDecoder, decoder_mlp
    x = torch.zeros(5, FEATURES)
    for act in ("softplus", "relu", "sine", "tanh"):
        for make in (lambda: AppearanceDecoder(FEATURES, act=act), lambda: GeometryDecoder(FEATURES, act=act),
                     lambda: DeformationDecoder(FEATURES, act=act, disable_posedirs=True)):
            with pytest.raises(NotImplementedError, match="only act='gelu'"):
                make()(x)
    with pytest.raises(NotImplementedError, match="disable_posedirs=True"):
        DeformationDecoder(FEATURES)(x)
    for m in _modules().values():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(x)
    w = lambda o, i: (torch.zeros(o, i), torch.zeros(o))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decoder_mlp(x, [w(64, FEATURES)], [(*w(3, 64), None)])


# ------------------------------------------------------------------------------------------------------------------ GPU

def torch_statements(x, trunk, heads):
    """the reference's statements: Linear + GELU trunk, one Linear and its activation per head"""
    import torch.nn.functional as F
    for W, b in trunk:
        x = F.gelu(F.linear(x, W, b))
    act = {None: lambda t: t, "gelu": F.gelu, "sigmoid": torch.sigmoid}
    return [act[kind](F.linear(x, W, b)) for W, b, kind in heads]


def _flat(trunk, heads):
    return [t for W, b in trunk for t in (W, b)] + [t for W, b, _ in heads for t in (W, b)]


def _torch_fp32_cpu(x, trunk, heads, g_outs):
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).requires_grad_(True)
    xt = tt(x)
    tr_, hd_ = [(tt(W), tt(b)) for W, b in trunk], [(tt(W), tt(b), k) for W, b, k in heads]
    outs = torch_statements(xt, tr_, hd_)
    used = [(o, torch.from_numpy(g)) for o, g in zip(outs, g_outs) if g is not None]
    torch.autograd.backward([o for o, _ in used], [g for _, g in used])
    zero = lambda p: np.zeros(tuple(p.shape), np.float32) if p.grad is None else p.grad.numpy()
    return [o.detach().numpy() for o in outs], zero(xt), [zero(p) for p in _flat(tr_, hd_)]


def _run_hip(x, trunk, heads, g_outs, device, x_grad=True, frozen=()):
    """-> outs, dx (None when x_grad is off), parameter gradients in _flat order (None for the indices in `frozen`)"""
    from hugs_amd.decoders import decoder_mlp
    tt = lambda a, grad=True: torch.from_numpy(np.ascontiguousarray(a)).to(device).requires_grad_(grad)
    xt = tt(x, x_grad)
    flat = [tt(p, j not in frozen) for j, p in enumerate(_flat(trunk, heads))]
    L = len(trunk)
    outs = decoder_mlp(xt, [(flat[2 * l], flat[2 * l + 1]) for l in range(L)],
                       [(flat[2 * (L + k)], flat[2 * (L + k) + 1], heads[k][2]) for k in range(len(heads))])
    used = [(o, torch.from_numpy(g).to(device)) for o, g in zip(outs, g_outs) if g is not None]
    torch.autograd.backward([o for o, _ in used], [g for _, g in used])
    cpu = lambda t: None if t is None else t.cpu().numpy()
    return [o.detach().cpu().numpy() for o in outs], cpu(xt.grad), [cpu(p.grad) for p in flat]


def _hold(name, hip, yardstick, f64):
    hip, f64 = np.asarray(hip, np.float64), np.asarray(f64, np.float64)
    assert hip.shape == f64.shape, (name, hip.shape, f64.shape)
    err, top = np.abs(hip - f64).max(), np.abs(f64).max()
    bound = 4 * yardstick + 1e-6 * top
    print(f"  {name}: |hip - fp64| {err:.3e}  yardstick {yardstick:.3e}  ratio {err / max(yardstick, 1e-300):.2f}  bound {bound:.3e}  max|fp64| {top:.4g}")
    assert err <= bound, (name, err, yardstick, bound)


def _err(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _check_all(label, x, trunk, heads, g_outs, ref32, got, seq_cols=None, skip=()):
    """ref32 = (outs, dx, flat parameter gradients) of the reference's float32 arithmetic; got likewise from the kernels.
    skip: flat parameter indices the kernels were not asked for."""
    print(label)
    outs64, _ = dr.forward(x, trunk, heads)
    back = dr.backward(x, trunk, heads, g_outs)
    for k in range(len(heads)):
        _hold(f"head {k}", got[0][k], _err(ref32[0][k], outs64[k]), outs64[k])
    if got[1] is not None:
        _hold("dL/dx", got[1], _err(ref32[1], back["dx"]), back["dx"])
    pairs = back["trunk"] + back["heads"]
    for j, ((dW, db), (gz, a)) in enumerate(zip(pairs, back["factors"])):
        seq_w, seq_b = dr.sequential_f32_error(gz, a, dW, db, max_cols=seq_cols)
        kind = f"trunk {j}" if j < len(trunk) else f"head {j - len(trunk)}"
        for at, want, seq, what in ((2 * j, dW, seq_w, "weight"), (2 * j + 1, db, seq_b, "bias")):
            if at in skip:
                assert got[2][at] is None, (kind, what)
                continue
            _hold(f"dL/d({kind} {what})", got[2][at], max(_err(ref32[2][at], want), seq), want)


SHAPES = {  # trunk widths, (head width, activation)
    "appearance": ((64, 64), ((48, None), (1, "sigmoid"))),
    "geometry": ((128, 128), ((3, None), (6, None), (3, "gelu"))),
    "deformation": ((128, 128, 128), ((24, "gelu"),)),
    # not a decoder of the reference: the other supported widths
    "one_layer": ((128,), ((64, "sigmoid"),)),
    "narrow3": ((64, 64, 64), ((31, "gelu"), (2, None), (31, "sigmoid"))),
}


def _random_case(tag, n, seed, in_width=FEATURES):
    r = np.random.default_rng(seed)
    widths, head_shapes = SHAPES[tag]
    lin = lambda o, i: ((r.uniform(-1, 1, (o, i)) / np.sqrt(i) + 0.05 * r.standard_normal((o, i))).astype(np.float32),
                        (r.uniform(-1, 1, o) / np.sqrt(i) + 0.05 * r.standard_normal(o)).astype(np.float32))
    trunk, width = [], in_width
    for wd in widths:
        trunk.append(lin(wd, width))
        width = wd
    heads = [(*lin(o, width), kind) for o, kind in head_shapes]
    x = r.standard_normal((n, in_width)).astype(np.float32)
    g_outs = [r.standard_normal((n, o)).astype(np.float32) for o, _ in head_shapes]
    return x, trunk, heads, g_outs


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_hip_matches_the_reference_vectors(tag, device):
    s = _state(tag)
    trunk, heads, keys = _network(tag, s)
    x, g_outs = G["x"], [G[f"{tag}.g_out.{k}"] for k in keys]
    # the golden gradients are keyed by parameter; decoder_mlp sees plain weights, so the yardstick for the weight-normed layer's
    # effective weight comes from torch's float32 statements on that same effective weight
    ref32 = _torch_fp32_cpu(x, trunk, heads, g_outs)
    golden_outs = [G[f"{tag}.out.{k}"] for k in keys]
    got = _run_hip(x, trunk, heads, g_outs, device)
    if tag != "deformation":   # plain parameters: the golden vectors themselves are the float32 reference
        names = _names(tag, "parameter_names")
        order = names[:4] + [n for k in (("shs", "opacity.0") if tag == "appearance" else ("xyz.1", "rotations.1", "scales.1")) for n in (f"{k}.weight", f"{k}.bias")]
        ref32 = (golden_outs, G[f"{tag}.grad_x"], [G[f"{tag}.grad.{n}"] for n in order])
    else:
        ref32 = (golden_outs, G[f"{tag}.grad_x"], ref32[2])
    _check_all(f"golden vectors, {tag}", x, trunk, heads, g_outs, ref32, got)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1, 4099])
@pytest.mark.parametrize("tag", TAGS)
def test_hip_against_fp64_within_four_times_the_reference_arithmetics_error(tag, n, device):
    x, trunk, heads, g_outs = _random_case(tag, n, seed=2000 + n)
    ref32 = _torch_fp32_cpu(x, trunk, heads, g_outs)
    _check_all(f"{tag}, n = {n}", x, trunk, heads, g_outs, ref32, _run_hip(x, trunk, heads, g_outs, device))


@pytest.mark.gpu
def test_hip_against_fp64_at_the_workloads_size(device):
    n = 110_210
    x, trunk, heads, g_outs = _random_case("deformation", n, seed=2000 + n)
    ref32 = _torch_fp32_cpu(x, trunk, heads, g_outs)
    _check_all(f"deformation, n = {n}", x, trunk, heads, g_outs, ref32, _run_hip(x, trunk, heads, g_outs, device), seq_cols=8)


@pytest.mark.gpu
def test_other_supported_widths(device):
    """input widths 32 and 128, one trunk layer, a 64-wide trunk of three layers, 64 head columns: the paths the decoders do not take"""
    for tag, in_width in (("one_layer", 32), ("narrow3", 128), ("geometry", 64)):
        x, trunk, heads, g_outs = _random_case(tag, 333, seed=77, in_width=in_width)
        ref32 = _torch_fp32_cpu(x, trunk, heads, g_outs)
        _check_all(f"{tag}, in = {in_width}", x, trunk, heads, g_outs, ref32, _run_hip(x, trunk, heads, g_outs, device))


@pytest.mark.gpu
def test_partial_gradients(device):
    x, trunk, heads, g_outs = _random_case("geometry", 777, seed=5)
    full32 = _torch_fp32_cpu(x, trunk, heads, g_outs)
    # x without grad, the second trunk layer frozen
    got = _run_hip(x, trunk, heads, g_outs, device, x_grad=False, frozen=(2, 3))
    assert got[1] is None and got[2][2] is None and got[2][3] is None
    _check_all("x without grad, trunk layer 1 frozen", x, trunk, heads, g_outs, full32, got, skip=(2, 3))
    # one head's output unused in the loss: it contributes nothing, and its own parameters get no gradient
    g_part = [g_outs[0], None, g_outs[2]]
    got = _run_hip(x, trunk, heads, g_part, device)
    assert got[2][6] is None and got[2][7] is None
    _check_all("head 1 unused", x, trunk, heads, g_part, _torch_fp32_cpu(x, trunk, heads, g_part), got, skip=(6, 7))


@pytest.mark.gpu
def test_forward_and_dx_are_bitwise_reproducible(device):
    x, trunk, heads, g_outs = _random_case("deformation", 20_000, seed=7)
    a, b = _run_hip(x, trunk, heads, g_outs, device), _run_hip(x, trunk, heads, g_outs, device)
    assert all(np.array_equal(p, q) for p, q in zip(a[0], b[0])) and np.array_equal(a[1], b[1])


@pytest.mark.gpu
def test_leading_dimensions(device):
    from hugs_amd.decoders import decoder_mlp
    x, trunk, heads, _ = _random_case("geometry", 77, seed=6)
    dev = lambda a: torch.from_numpy(a).to(device)
    tr_, hd_ = [(dev(W), dev(b)) for W, b in trunk], [(dev(W), dev(b), k) for W, b, k in heads]
    flat = decoder_mlp(dev(x), tr_, hd_)
    shaped = decoder_mlp(dev(x.reshape(7, 11, FEATURES)), tr_, hd_)
    for f, s_, (W, _, _) in zip(flat, shaped, heads):
        assert s_.shape == (7, 11, W.shape[0]) and torch.equal(s_.reshape(77, -1), f)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_modules_end_to_end_on_the_reference_checkpoint(tag, device):
    s = _state(tag)
    m = _modules()[tag]
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in s.items()})
    m = m.to(device)
    xt = torch.from_numpy(G["x"].copy()).to(device).requires_grad_(True)
    out = m(xt)
    assert list(out.keys()) == _names(tag, "output_keys")
    trunk, heads, keys = _network(tag, s, f64_weight_norm=True)
    if tag == "deformation":
        assert out["posedirs"] is None
    g_outs = [G[f"{tag}.g_out.{k}"] for k in keys]
    torch.autograd.backward([out[k] for k in keys], [torch.from_numpy(g).to(device) for g in g_outs])
    outs64, _ = dr.forward(G["x"], trunk, heads)
    back = dr.backward(G["x"], trunk, heads, g_outs)
    print(f"module {tag}, end to end")
    for k, y in zip(keys, outs64):
        _hold(f"out {k}", out[k].detach().cpu().numpy(), _err(G[f"{tag}.out.{k}"], y), y)
    _hold("dL/dx", xt.grad.cpu().numpy(), _err(G[f"{tag}.grad_x"], back["dx"]), back["dx"])
    grads64 = _param_grads64(tag, s, back)
    params = dict(m.named_parameters())
    for n, want in grads64.items():
        ref = G[f"{tag}.grad.{n}"]
        _hold(f"dL/d{n}", params[n].grad.cpu().numpy(), _err(ref, want.reshape(ref.shape)), want.reshape(ref.shape))


@pytest.mark.gpu
def test_geometry_decoder_on_a_surface_has_two_scales(device):
    m = _modules(use_surface=True)["geometry"].to(device)
    out = m(torch.randn(50, FEATURES, device=device))
    assert out["scales"].shape == (50, 2) and out["xyz"].shape == (50, 3) and out["rotations"].shape == (50, 6)
    want = torch_statements(torch.zeros(1, FEATURES), [(m.net[0].weight.cpu(), m.net[0].bias.cpu()), (m.net[2].weight.cpu(), m.net[2].bias.cpu())],
                            [(m.scales[1].weight.cpu(), m.scales[1].bias.cpu(), "gelu")])[0]
    got = m(torch.zeros(1, FEATURES, device=device))["scales"].cpu()
    assert torch.allclose(got, want.detach(), atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_adam_moves_every_parameter(tag, device):
    torch.manual_seed(11)
    m = _modules()[tag].to(device)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    x = torch.randn(3000, FEATURES, device=device)
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        sum(v.square().mean() for v in m(x).values() if v is not None).backward()
        opt.step()
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and torch.isfinite(p).all() and not torch.equal(p.detach(), before[n]), n
    if tag == "deformation":
        assert m.skinning_linear.weight_g.grad.abs().max() > 0 and m.skinning_linear.weight_v.grad.abs().max() > 0


@pytest.mark.gpu
def test_no_activation_is_kept_for_the_backward(device):
    from hugs_amd.decoders import decoder_mlp
    x, trunk, heads, _ = _random_case("deformation", 4099, seed=8)
    dev = lambda a: torch.from_numpy(a).to(device).requires_grad_(True)
    xt = dev(x)
    tr_, hd_ = [(dev(W), dev(b)) for W, b in trunk], [(dev(W), dev(b), k) for W, b, k in heads]
    torch.cuda.synchronize(device)
    before = torch.cuda.memory_allocated(device)
    outs = decoder_mlp(xt, tr_, hd_)
    after = torch.cuda.memory_allocated(device)
    out_bytes = sum(o.numel() * 4 for o in outs)
    print(f"  allocated by the forward: {after - before} B, outputs {out_bytes} B")
    assert outs[0].requires_grad and after - before <= out_bytes + 64 * 1024
