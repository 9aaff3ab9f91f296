"""tests/layouts.py on CPU: every builder keeps the values bit for bit and has the layout it states; the three layouts the GPU matrix
(tests/test_gpu_row_layouts.py) sends into the rows' backwards are what ordinary torch statements downstream of a row produce; and
the library refuses, on the host and before any launch, the misaligned pointers the Python wrappers realign (`_aligned` in
diff_gaussian_rasterization): that refusal is what makes a forgotten realignment an exception instead of a misaligned float4 access."""
import ctypes as C

import pytest
import torch

import layouts as L

SHAPES = [(257, 3), (33, 4, 4), (5, 16, 3), (1, 7, 2), (12,), (3, 20, 68)]


def _values(shape, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.bool:
        return torch.rand(shape, generator=g) > 0.5
    if dtype == torch.int32:
        return torch.randint(-50, 50, shape, generator=g, dtype=torch.int32)
    return torch.randn(shape, generator=g, dtype=dtype)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.bool], ids=["f32", "i32", "bool"])
def test_builders_keep_the_values_and_have_the_stated_layout(shape, dtype):
    t = _values(shape, dtype)
    f = L.fresh(t)
    assert torch.equal(f, t) and f.is_contiguous() and f.data_ptr() % 16 == 0 and f.data_ptr() != t.data_ptr()
    o = L.odd_offset(t)
    assert torch.equal(o, t) and o.shape == t.shape and o.is_contiguous() and o.storage_offset() == 1
    assert o.data_ptr() % 16 == t.element_size()                     # 4 for float32 and int32: not a float4 boundary
    assert o.contiguous().data_ptr() == o.data_ptr()                 # what makes the layout a trap: .contiguous() returns it unchanged
    s = L.strided(t)
    assert torch.equal(s, t) and s.shape == t.shape and not s.is_contiguous() and 0 not in s.stride() and L.has_layout("strided", s)
    assert max(a // b for a, b in zip(s.stride(), t.contiguous().stride())) == 2   # every second row of a buffer twice as long
    if t.ndim >= 2 and min(t.shape[-2:]) > 1:
        tr = L.strided(t, "transposed")
        assert torch.equal(tr, t) and not tr.is_contiguous() and tr.stride()[-2] == 1 and tr.stride()[-1] == t.shape[-2]
    else:
        with pytest.raises(ValueError):
            L.strided(t, "transposed")
    for name in ("fresh", "odd_offset", "strided"):
        assert L.has_layout(name, L.build(name, t)), name
        assert not L.has_layout(name, {"fresh": o, "odd_offset": f, "strided": f}[name]), name   # ... and tells the others apart


def test_expanded_and_float64_builders():
    row = _values((1, 4, 4))
    t = row.repeat(33, 1, 1)
    e = L.expanded(t)
    assert torch.equal(e, t) and e.shape == t.shape and e.stride() == (0, 4, 1) and L.has_layout("expanded", e)
    c = torch.full((33, 4, 4), 0.37)
    e = L.expanded(c)
    assert torch.equal(e, c) and e.stride() == (0, 0, 0)
    assert not L.has_layout("expanded", c) and not L.has_layout("fresh", e)
    with pytest.raises(ValueError):
        L.expanded(_values((33, 4, 4)))
    d = L.float64(row)
    assert d.dtype == torch.float64 and torch.equal(d.float(), row) and L.has_layout("float64", d) and not L.has_layout("float64", row)
    assert L.build("fresh", None) is None


@pytest.mark.parametrize("name", ["fresh", "odd_offset", "strided", "strided_transposed", "float64"])
def test_a_leaf_sent_through_a_builder_still_gets_its_gradient_in_its_own_shape(name):
    leaf = _values((9, 4, 4)).requires_grad_()
    w = _values((9, 4, 4), seed=1)
    (L.build(name, leaf) * w.to(torch.float64 if name == "float64" else torch.float32)).sum().backward()
    assert leaf.grad.shape == leaf.shape and leaf.grad.dtype == torch.float32 and torch.equal(leaf.grad, w)


def test_the_three_layouts_reach_a_backward_from_ordinary_statements():
    """a pass-through Function in the place of a row: what its backward receives from three statements a model writes after it"""
    x = _values((33, 4, 4)).requires_grad_()
    w = _values((33, 4, 4), seed=2)
    seen = []
    y = L.probe(x, seen)
    (torch.cat([torch.zeros(1), y.reshape(-1)]) * torch.cat([torch.zeros(1), w.reshape(-1)])).sum().backward()
    got = seen.pop()
    assert got["contiguous"] and got["offset"] == 1 and got["mod16"] == 4 and got["strides"] == (16, 4, 1), got
    L.probe(x, seen).sum().backward()
    got = seen.pop()
    assert got["strides"] == (0, 0, 0) and not got["contiguous"], got
    # (.mean() divides the expanded scalar by the count, which materialises it: the stride-0 layout comes from .sum())
    (L.probe(x, seen).transpose(1, 2) * w).sum().backward()
    got = seen.pop()
    assert got["strides"] == (16, 1, 4) and not got["contiguous"], got
    # inputs get the same layouts from narrow, split, slicing and permute
    packed = _values((1 + 33 * 16,))
    assert L.describe(packed.narrow(0, 1, 33 * 16).view(33, 4, 4))["mod16"] == 4
    assert L.describe(packed.split([1, 33 * 16])[1])["offset"] == 1
    assert not _values((4, 4, 33)).permute(2, 0, 1).is_contiguous() and not _values((66, 3))[::2].is_contiguous()


@pytest.mark.parametrize("name", ["odd_offset", "strided", "strided_transposed", "expanded"])
def test_inject_hands_the_named_layout_to_the_backward_in_front_of_it(name):
    x = _values((33, 4, 4)).requires_grad_()
    g = _values((1, 4, 4), seed=3).repeat(33, 1, 1) if name == "expanded" else _values((33, 4, 4), seed=3)
    seen, handed = [], []
    y = L.inject(L.probe(x, seen), name, handed)
    assert torch.equal(y, x)
    y.backward(g)
    assert len(seen) == 1 and seen == handed                          # the very tensor: autograd neither copied nor re-laid it
    assert torch.equal(x.grad, g)
    d = seen[0]
    if name == "odd_offset":
        assert d["contiguous"] and d["mod16"] == 4 and d["offset"] == 1
    elif name == "expanded":
        assert d["strides"] == (0, 4, 1)
    else:
        assert not d["contiguous"] and 0 not in d["strides"]
    if name == "expanded":                                             # a gradient that is not constant cannot be expanded: said, not faked
        with pytest.raises(ValueError):
            L.inject(x, name).backward(_values((33, 4, 4), seed=4))


def test_the_shared_aligned_copies_only_what_is_misaligned_or_strided():
    """`_aligned` of diff_gaussian_rasterization, the one definition every wrapper uses (on CPU tensors: it only looks at layout)"""
    from diff_gaussian_rasterization import _aligned
    import hugs_amd.decoders, hugs_amd.knn, hugs_amd.lbs, hugs_amd.rotations, hugs_amd.scene_forward, hugs_amd.smpl, hugs_amd.triplane
    for mod in (hugs_amd.decoders, hugs_amd.knn, hugs_amd.lbs, hugs_amd.rotations, hugs_amd.scene_forward, hugs_amd.smpl, hugs_amd.triplane):
        assert mod._aligned is _aligned, mod.__name__
    t = L.fresh(_values((33, 4, 4)))
    assert _aligned(None) is None and _aligned(t) is t                 # the usual case costs nothing
    for name in ("odd_offset", "strided", "strided_transposed"):
        a = _aligned(L.build(name, t))
        assert torch.equal(a, t) and a.is_contiguous() and a.data_ptr() % 16 == 0, name
    a = _aligned(L.expanded(torch.full((33, 4, 4), 2.5)))
    assert a.is_contiguous() and a.data_ptr() % 16 == 0 and torch.equal(a, torch.full((33, 4, 4), 2.5))


# ------------------------------------------------------------------------------------------------ the library's host-side refusals

def _lib():
    import diff_gaussian_rasterization as dgr
    return dgr._load()   # with the prototypes the wrappers call through (diff_gaussian_rasterization/_abi.py)


INVALID = -1   # HGS_ERR_INVALID_ARGUMENT (include/hgs_rasterizer.h)
F = 256        # a fake, 16-byte aligned device pointer: every call below returns from the argument checks and never dereferences it


def test_lbs_skin_refuses_misaligned_float4_pointers_before_any_launch():
    lib = _lib()

    def fwd(**kw):
        a = dict(A=F, weights=F, v=F, rotmat=None, T=F, verts=F, rot=None)
        a.update(kw)
        return lib.hgs_lbs_skin_forward(4, 24, *a.values(), None)

    def bwd(**kw):
        a = dict(A=F, weights=F, v=F, rotmat=None, T=F, g_verts=F, g_T=F, g_rot=None, dA=F, dW=F, dv=F, dR=None, ws=F)
        a.update(kw)
        return lib.hgs_lbs_skin_backward(4, 24, *a.values(), None)

    for off in (4, 8, 12):
        assert fwd(T=F + off) == INVALID and lib.hgs_last_error() == b"lbs_skin: T must be 16-byte aligned"
        for name in ("T", "g_T", "ws"):
            assert bwd(**{name: F + off}) == INVALID, (name, off)
            assert lib.hgs_last_error() == b"lbs_skin backward: T, dL_dT and workspace must be 16-byte aligned", (name, off)
    assert bwd(g_T=F + 4, g_verts=None) == INVALID and b"16-byte aligned" in lib.hgs_last_error()   # dL/dT alone, as a loss on T sends it
    assert fwd(T=None) == INVALID and bwd(ws=None) == INVALID and b"null pointer" in lib.hgs_last_error()


def test_smpl_refuses_misaligned_float4_pointers_before_any_launch():
    import smpl_ref as sr
    lib = _lib()
    parents = (C.c_int32 * 24)(*sr.SMPL_PARENTS)

    def fwd(**kw):
        a = dict(betas=F, pose=F, transl=None, v_template=F, shapedirs=F, posedirs=F, J_regressor=F, lbs_weights=F)
        o = dict(verts=F, Jtr=F, A=F, T=F, v_posed=F, v_shaped=F, so=F, po=F, ws=F)
        o.update(kw)
        return lib.hgs_smpl_forward(4, 24, 10, parents, *a.values(), 0, *o.values(), None)

    def bwd(**kw):
        a = dict(pose=F, shapedirs=F, posedirs=F, J_regressor=F, lbs_weights=F)
        o = dict(v_posed=F, T=F, g_verts=None, g_Jtr=None, g_A=F, g_T=F, g_vp=None, g_vs=None, g_so=None, g_po=None, d_betas=F, d_pose=F,
                 d_transl=None, ws=F)
        o.update(kw)
        return lib.hgs_smpl_backward(4, 24, 10, parents, *a.values(), 0, *o.values(), None)

    for off in (4, 8, 12):
        for name in ("T", "ws"):
            assert fwd(**{name: F + off}) == INVALID, (name, off)
            assert lib.hgs_last_error() == b"smpl_forward: T and workspace must be 16-byte aligned", (name, off)
        for name in ("T", "g_T", "ws"):
            assert bwd(**{name: F + off}) == INVALID, (name, off)
            assert lib.hgs_last_error() == b"smpl_backward: T, dL_dT and workspace must be 16-byte aligned", (name, off)


def test_lbsmap_top_k_refuses_misaligned_transforms_before_any_launch():
    lib = _lib()

    def call(**kw):
        a = dict(points=F, m=8, templ=F, lbs_weights=F, J=24, K=6, vt=F, info=None, C=0, dist=F, out_T=F, out_info=None, idx=F, wgt=F, ws=None)
        a.update(kw)
        return lib.hgs_smpl_lbsmap_top_k(4, *a.values(), None)

    for off in (4, 8, 12):
        for name in ("vt", "out_T"):
            assert call(**{name: F + off}) == INVALID, (name, off)
            assert lib.hgs_last_error() == b"smpl_lbsmap_top_k: verts_transform and out_transform must be 16-byte aligned", (name, off)
    assert call(ws=F + 4) == INVALID and lib.hgs_last_error() == b"smpl_lbsmap_top_k: the workspace must be 16-byte aligned"
    assert call(templ=F + 2) == INVALID and b"float-aligned" in lib.hgs_last_error()
    assert call(vt=None) == INVALID and b"null pointer" in lib.hgs_last_error()
