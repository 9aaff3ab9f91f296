"""Row f-8 -- TriPlane.forward fused (/root/reference/hugs/models/modules/triplane.py:26-40).

CPU: the float64 restatement (tests/triplane_ref.py) against the outputs and autograd gradients of the reference's own class
(tests/golden/make_golden_triplane.py compiles it from /root/reference and runs it on CPU: unequal resolutions 6 x 10 x 14, so the
axis convention is part of what is checked); the library's exports and its host-side validation; the module's parameters and layout.

GPU: the HIP kernels through `triplane_sample` / `TriPlane`.  Tolerance, per tensor (features, each plane's gradient, dL/dx): the
float64 restatement of the same float32 inputs is the truth, the yardstick is the reference's own float32 error
    err_ref = max |torch_fp32_cpu - fp64|        (golden vectors: max |golden - fp64|)
and the requirement is
    max |hip - fp64| <= 4 err_ref + 1e-6 max |fp64|.
What dominates err_ref is the rounding of the texel coordinate ix (an ulp of 255 is 1.5e-5); the factor 4 leaves room for another legal
rounding sequence, the floor covers inputs whose err_ref is 0; a wrong corner, weight or axis is off by 1e-2 and more.  Every figure is
printed before it is asserted (pytest -s shows them).

CPU bound of the restatement against the golden vectors, from the number formats: ix is the result of six float32 operations on values
of at most res - 1, so |d ix| <= D = 6 * 2^-24 * (res_max - 1).  A feature moves by at most the difference of two corners per axis:
4 D max|plane| (+ 1e-6 max|feat| for the four-term sum).  A texel of a plane's gradient collects weight errors of at most 2 D |g| from
each of the m points in the four cells around it: 2 D max|g| m_max.  dL/dx: the 32-channel sum of go * v * (d weight), whose weights'
derivatives move by D, times (res - 1) / 2 * 2 / scale, on two planes per coordinate: 2 * 32 * 4 max|g| max|plane| D (res_max - 1) / scale.
No wall-clock assertion here: timing lives in tools/bench_triplane.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import triplane_ref as tr

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_triplane.npz"))
PLANES = ("plane_xy", "plane_xz", "plane_yz")
CENTER, SCALE = float(G["center"]), float(G["scale"])


def _golden_planes():
    return [G[k] for k in PLANES]


def test_fp64_restatement_reproduces_the_reference_features_and_gradients():
    planes, x, g = _golden_planes(), G["x"], G["g_feat"]
    assert [p.shape for p in planes] == [(1, 32, 6, 10), (1, 32, 6, 14), (1, 32, 10, 14)]      # [1,F,resX,resY], [1,F,resX,resZ], [1,F,resY,resZ]
    res_max = 14
    D = 6 * 2.0 ** -24 * (res_max - 1)
    vmax, gmax = max(np.abs(p).max() for p in planes), np.abs(g).max()
    feat = tr.forward(planes, x, CENTER, SCALE)
    assert feat.shape == G["feat"].shape == (x.shape[0], 96)
    err = np.abs(feat - G["feat"]).max()
    print(f"features: {err:.3e} (bound {4 * D * vmax + 1e-6 * np.abs(feat).max():.3e})")
    assert err <= 4 * D * vmax + 1e-6 * np.abs(feat).max()
    d_planes, d_x = tr.backward(planes, x, g, CENTER, SCALE)
    u = ((x.astype(np.float64) - CENTER) / SCALE + 0.5)
    for p, name in enumerate(PLANES):
        aw, ah = tr.AXES[p]
        H, W = planes[p].shape[2:]
        cells = np.floor(u[:, ah] * (H - 1)) * 64 + np.floor(u[:, aw] * (W - 1))
        m_max = 4 * np.unique(cells, return_counts=True)[1].max()
        err = np.abs(d_planes[p] - G[f"grad_{name}"]).max()
        print(f"dL/d{name}: {err:.3e} (bound {2 * D * gmax * m_max:.3e})")
        assert d_planes[p].shape == planes[p].shape and err <= 2 * D * gmax * m_max
    err = np.abs(d_x - G["grad_x"]).max()
    bound = 2 * 32 * 4 * gmax * vmax * D * (res_max - 1) / SCALE
    print(f"dL/dx: {err:.3e} (bound {bound:.3e}, largest entry {np.abs(d_x).max():.1f})")
    assert err <= bound
    # the axis convention is part of the agreement: x and y exchanged on plane_xy (a transposed implementation) is off by far more than any bound here
    assert np.abs(tr.forward(planes, x[:, [1, 0, 2]], CENTER, SCALE)[:, :32] - G["feat"][:, :32]).max() > 1e-2


def _lib():
    import diff_gaussian_rasterization as dgr
    return dgr._load()   # with the prototypes the wrapper calls through (diff_gaussian_rasterization/_abi.py)


def test_library_exports_both_entry_points():
    lib = _lib()
    assert hasattr(lib, "hgs_triplane_forward") and hasattr(lib, "hgs_triplane_backward")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hgs_rasterizer.h")).read()
    assert "Row f-8" in header and "hgs_triplane_forward(" in header and "hgs_triplane_backward(" in header
    assert "/root/reference/hugs/models/modules/triplane.py:26-40" in header


def test_entry_points_validate_on_the_host_before_any_launch():
    """Every call here returns from the argument checks (there is no GPU in a CPU run): fake non-null pointers are never dereferenced."""
    lib = _lib()
    res = (C.c_int32 * 3)(6, 10, 14)
    cl = (C.c_int64 * 9)(1, 320, 32, 1, 448, 32, 1, 448, 32)
    three = lambda *v: (C.c_void_p * 3)(*v)
    fwd = lambda n=4, F=32, res=res, st=cl, x=64, p=(64, 64, 64), feat=64: lib.hgs_triplane_forward(n, F, res, st, 0.0, 2.0, x, *p, feat, None)
    bwd = lambda n=4, F=32, res=res, st=cl, x=64, planes=three(64, 64, 64), g=64, dx=64, dp=three(64, 64, 64): \
        lib.hgs_triplane_backward(n, F, res, st, 0.0, 2.0, x, planes, g, dx, dp, None)
    for call, what in ((fwd, b"triplane_forward"), (bwd, b"triplane_backward")):
        assert call(n=0) == 0                                                         # nothing to do, nothing touched
        assert call(n=-1) == -1 and what in lib.hgs_last_error()
        assert call(F=16) == -1 and b"only F = 32" in lib.hgs_last_error() and what in lib.hgs_last_error()
        assert call(res=(C.c_int32 * 3)(6, 1, 14)) == -1 and b"resolution must be at least 2" in lib.hgs_last_error()
        assert call(res=None) == -1 and b"null pointer" in lib.hgs_last_error()
        assert call(st=None) == -1 and b"null pointer" in lib.hgs_last_error()
        assert call(st=(C.c_int64 * 9)(1, 320, 32, 1, -448, 32, 1, 448, 32)) == -1 and b"negative stride" in lib.hgs_last_error()
        assert call(x=None) == -1 and b"null pointer" in lib.hgs_last_error()
    assert fwd(p=(64, None, 64)) == -1 and b"null pointer" in lib.hgs_last_error()
    assert fwd(feat=None) == -1 and b"null pointer" in lib.hgs_last_error()
    assert fwd(feat=68) == -1 and b"feat must be 16-byte aligned" in lib.hgs_last_error()
    assert bwd(g=None) == -1 and b"null pointer" in lib.hgs_last_error()
    assert bwd(g=72) == -1 and b"dL_dfeat must be 16-byte aligned" in lib.hgs_last_error()
    assert bwd(planes=three(64, None, 64)) == -1 and b"dL_dx needs the three planes" in lib.hgs_last_error()
    assert bwd(planes=None) == -1 and b"dL_dx needs the three planes" in lib.hgs_last_error()
    assert bwd(dx=None, dp=None) == 0 and bwd(dx=None, dp=three(None, None, None)) == 0      # neither half asked for: no launch


def test_module_has_the_reference_parameters_in_channels_last():
    from hugs_amd.triplane import TriPlane, triplane_sample
    m = TriPlane(32, 6, 10, 14)
    names = bytes(G["parameter_names"]).decode().split(",")
    assert [n for n, _ in m.named_parameters()] == names == list(PLANES)
    cl = lambda p: p.stride() == (p.shape[1] * p.shape[2] * p.shape[3], 1, p.shape[3] * p.shape[1], p.shape[1])
    for n, p in m.named_parameters():
        assert tuple(p.shape) == G[n].shape and p.dtype == torch.float32 and cl(p), n
    assert (m.dim, m.n_input_dims, m.n_output_dims, m.center, m.scale) == (32, 3, 96, CENTER, SCALE) and int(G["n_output_dims"]) == 96
    ref_state = {n: torch.from_numpy(G[n].copy()) for n in PLANES}                    # NCHW tensors: a reference checkpoint
    assert all(t.is_contiguous() for t in ref_state.values())
    m.load_state_dict(ref_state)
    for n, p in m.named_parameters():
        assert cl(p) and torch.equal(p.detach(), ref_state[n]), n
    saved = m.state_dict()
    assert list(saved) == list(PLANES) and all(tuple(saved[n].shape) == G[n].shape for n in PLANES)
    d = TriPlane()
    assert tuple(d.plane_xy.shape) == (1, 32, 256, 256) and d.n_output_dims == 96 and cl(d.plane_yz)
    with pytest.raises(NotImplementedError, match="32 features"):
        TriPlane(16, 6, 10, 14)(torch.zeros(5, 3))
    with pytest.raises(NotImplementedError):
        triplane_sample(torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 4, 4), torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(5, 3))


# ------------------------------------------------------------------------------------------------------------------ GPU

def torch_statements(plane_xy, plane_xz, plane_yz, x, center=0.0, scale=2.0):
    """the reference's statements (triplane.py:27-39) without its assertion"""
    from torch.nn.functional import grid_sample
    x = (x - center) / scale + 0.5
    x = x * 2 - 1
    shape = x.shape
    coords = x.reshape(1, -1, 1, 3)
    feats = [grid_sample(p, coords[..., ax], align_corners=True)[0, :, :, 0].transpose(0, 1)
             for p, ax in ((plane_xy, [0, 1]), (plane_xz, [0, 2]), (plane_yz, [1, 2]))]
    return torch.cat(feats, dim=1).reshape(*shape[:-1], 3 * plane_xy.shape[1])


def _torch_fp32_cpu(planes, x, g):
    t = [torch.from_numpy(np.ascontiguousarray(p)).requires_grad_(True) for p in planes]
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    feat = torch_statements(*t, xt, CENTER, SCALE)
    feat.backward(torch.from_numpy(g))
    return feat.detach().numpy(), [p.grad.numpy() for p in t], xt.grad.numpy()


def _hold(name, hip, ref32, f64):
    hip, ref32, f64 = (np.asarray(a, np.float64) for a in (hip, ref32, f64))
    assert hip.shape == f64.shape, (name, hip.shape, f64.shape)
    err_ref, err, top = np.abs(ref32 - f64).max(), np.abs(hip - f64).max(), np.abs(f64).max()
    bound = 4 * err_ref + 1e-6 * top
    print(f"  {name}: |hip - fp64| {err:.3e}  err_ref {err_ref:.3e}  ratio {err / max(err_ref, 1e-300):.2f}  bound {bound:.3e}  max|fp64| {top:.4g}")
    assert err <= bound, (name, err, err_ref, bound)


def _run_hip(planes, x, g, device, channels_last=True, center=CENTER, scale=SCALE):
    from hugs_amd.triplane import triplane_sample
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    t = [torch.from_numpy(np.ascontiguousarray(p)).to(device).contiguous(memory_format=fmt).requires_grad_(True) for p in planes]
    xt = torch.from_numpy(x.copy()).to(device).requires_grad_(True)
    feat = triplane_sample(*t, xt, center, scale)
    feat.backward(torch.from_numpy(g).to(device))
    for p in t:
        assert p.grad.stride() == p.stride()
    return feat.detach().cpu().numpy(), [p.grad.cpu().numpy() for p in t], xt.grad.cpu().numpy()


def _cell_is_the_same_in_both_precisions(planes, x):
    """per point: floor(ix) of every coordinate on both of its planes comes out the same in float32 (as the reference and the kernel
    evaluate it) and in float64.  dL/dx jumps from one cell to the next, so at a point within an ulp of a cell edge the float32
    evaluations and the float64 one differentiate different cells, and err_ref there is the size of the jump, not of a rounding."""
    def cells(t):
        u = (x.astype(t) - t(CENTER)) / t(SCALE) + t(0.5)
        gq = (u * t(2.0) - t(1.0) + t(1.0)) / t(2.0)
        return np.stack([np.floor(gq[:, a] * t(planes[p].shape[3 - k] - 1)) for p in range(3) for k, a in enumerate(tr.AXES[p])])
    return np.all(cells(np.float32) == cells(np.float64), axis=0)


def _check_all(planes, x, g, ref32, got):
    f64_feat = tr.forward(planes, x, CENTER, SCALE)
    f64_planes, f64_x = tr.backward(planes, x, g, CENTER, SCALE)
    _hold("features", got[0], ref32[0], f64_feat)
    for p, name in enumerate(PLANES):
        _hold(f"dL/d{name}", got[1][p], ref32[1][p], f64_planes[p])
    _hold("dL/dx", got[2], ref32[2], f64_x)
    same = _cell_is_the_same_in_both_precisions(planes, x)
    if not same.all():   # the rule again without those points, where it would otherwise say little about all the others
        print(f"  {int((~same).sum())} of {x.shape[0]} points lie within an ulp of a cell edge")
        _hold("dL/dx of the other points", got[2][same], ref32[2][same], f64_x[same])


@pytest.mark.gpu
@pytest.mark.parametrize("channels_last", [True, False], ids=["channels_last", "nchw"])
def test_hip_matches_the_reference_vectors(channels_last, device):
    planes, x, g = _golden_planes(), G["x"], G["g_feat"]
    got = _run_hip(planes, x, g, device, channels_last)
    print(f"golden vectors, {'channels-last' if channels_last else 'NCHW'} planes")
    _check_all(planes, x, g, (G["feat"], [G[f"grad_{k}"] for k in PLANES], G["grad_x"]), got)


def _random_case(n, res, seed):
    r = np.random.default_rng(seed)
    rx, ry, rz = res
    planes = [r.standard_normal((1, 32, a, b)).astype(np.float32) for a, b in ((rx, ry), (rx, rz), (ry, rz))]
    x = r.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    g = r.standard_normal((n, 96)).astype(np.float32)
    return planes, x, g


@pytest.mark.gpu
@pytest.mark.parametrize("n,res", [(1, (256, 256, 256)), (63, (256, 256, 256)), (4097, (256, 256, 256)), (110_210, (256, 256, 256)),
                                   (5000, (40, 72, 130))])
def test_hip_against_fp64_within_four_times_torchs_own_error(n, res, device):
    planes, x, g = _random_case(n, res, seed=1000 + n)
    ref32 = _torch_fp32_cpu(planes, x, g)
    print(f"n = {n}, res = {res}")
    _check_all(planes, x, g, ref32, _run_hip(planes, x, g, device))


@pytest.mark.gpu
def test_partial_gradients(device):
    from hugs_amd.triplane import triplane_sample
    planes, x, g = _random_case(777, (32, 48, 64), seed=5)
    gt = torch.from_numpy(g).to(device)
    cl = lambda grad: [torch.from_numpy(p).to(device).contiguous(memory_format=torch.channels_last).requires_grad_(grad) for p in planes]
    full = _run_hip(planes, x, g, device)
    frozen, xt = cl(False), torch.from_numpy(x.copy()).to(device).requires_grad_(True)             # frozen planes: dL/dx only
    triplane_sample(*frozen, xt).backward(gt)
    assert all(p.grad is None for p in frozen) and np.array_equal(xt.grad.cpu().numpy(), full[2])   # (dL/dx has no atomics: bitwise)
    live, xc = cl(True), torch.from_numpy(x.copy()).to(device)                                      # x without grad: planes only
    live[1].requires_grad_(False)
    triplane_sample(*live, xc).backward(gt)
    assert xc.grad is None and live[1].grad is None
    f64_planes, _ = tr.backward(planes, x, g, CENTER, SCALE)
    ref32 = _torch_fp32_cpu(planes, x, g)
    for p in (0, 2):
        _hold(f"dL/d{PLANES[p]} alone", live[p].grad.cpu().numpy(), ref32[1][p], f64_planes[p])


@pytest.mark.gpu
def test_leading_dimensions_and_center_scale(device):
    from hugs_amd.triplane import triplane_sample
    planes, x, g = _random_case(77, (16, 20, 24), seed=6)
    t = [torch.from_numpy(p).to(device).contiguous(memory_format=torch.channels_last) for p in planes]
    flat = triplane_sample(*t, torch.from_numpy(x).to(device))
    shaped = triplane_sample(*t, torch.from_numpy(x.reshape(7, 11, 3)).to(device))
    assert shaped.shape == (7, 11, 96) and torch.equal(shaped.reshape(77, 96), flat)
    moved = triplane_sample(*t, torch.from_numpy(x * 1.5 + 0.25).to(device), center=0.25, scale=3.0)
    want = tr.forward(planes, x * np.float32(1.5) + np.float32(0.25), 0.25, 3.0)
    assert np.abs(moved.cpu().numpy() - want).max() <= 1e-4 * np.abs(want).max()                    # (a wrong center / scale is off by O(1))


@pytest.mark.gpu
def test_forward_is_bitwise_reproducible(device):
    from hugs_amd.triplane import triplane_sample
    planes, x, _ = _random_case(20_000, (256, 256, 256), seed=7)
    t = [torch.from_numpy(p).to(device).contiguous(memory_format=torch.channels_last) for p in planes]
    xt = torch.from_numpy(x).to(device)
    assert torch.equal(triplane_sample(*t, xt), triplane_sample(*t, xt))


@pytest.mark.gpu
def test_adam_keeps_channels_last_and_moves_the_planes(device):
    from hugs_amd.triplane import TriPlane
    m = TriPlane(32, 24, 32, 40).to(device)
    strides = [p.stride() for p in m.parameters()]
    assert all(s[1] == 1 for s in strides)
    before = [p.detach().clone() for p in m.parameters()]
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    x = torch.rand(3000, 3, device=device) * 2 - 1
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        m(x).square().mean().backward()
        opt.step()
    for p, s, b in zip(m.parameters(), strides, before):
        assert p.stride() == s and p.grad.stride() == s and not torch.equal(p.detach(), b) and torch.isfinite(p).all()
        assert all(v.stride() == s for v in opt.state[p].values() if torch.is_tensor(v) and v.ndim == 4)


@pytest.mark.gpu
def test_module_equals_the_torch_statements_end_to_end(device):
    from hugs_amd.triplane import TriPlane
    m = TriPlane(32, 6, 10, 14)
    m.load_state_dict({n: torch.from_numpy(G[n].copy()) for n in PLANES})
    m = m.to(device)
    assert all(p.stride()[1] == 1 for p in m.parameters())
    x, g = G["x"], G["g_feat"]
    xt = torch.from_numpy(x.copy()).to(device).requires_grad_(True)
    feat = m(xt, check_range=True)                                                     # the golden points satisfy the reference's assertion
    feat.backward(torch.from_numpy(g).to(device))
    planes = _golden_planes()
    got = (feat.detach().cpu().numpy(), [getattr(m, n).grad.cpu().numpy() for n in PLANES], xt.grad.cpu().numpy())
    print("module, end to end")
    _check_all(planes, x, g, _torch_fp32_cpu(planes, x, g), got)
    with pytest.raises(AssertionError, match=r"x must be in \[0, 1\], got"):
        m(torch.full((4, 3), 1.5, device=device), check_range=True)
    out = m(torch.full((4, 3), 1.5, device=device))                                    # the default does not look: outside every plane -> zeros
    assert torch.equal(out, torch.zeros_like(out))
