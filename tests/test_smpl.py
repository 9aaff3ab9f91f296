"""Row f-10 -- the SMPL body model's forward fused (SMPL.forward, /root/reference/hugs/models/modules/smpl_layer.py:411-519, and
lbs(), /root/reference/hugs/models/modules/lbs.py:76-187).

CPU: the float64 restatement (tests/smpl_ref.py) against the outputs and autograd gradients of the reference's own lbs()
(tests/golden/make_golden_smpl.py compiles it from /root/reference and runs it in float32 on CPU, smplx's four functions supplied by
the restatement's torch forms); three deliberately wrong variants against the same vectors; the hand-written backward against central
differences; the zero pose; the library's exports and its host-side validation; the wrapper's refusals.

The CPU bound, first order in U = 2^-24, from the number formats (|.| entry-wise, g_n = (n + 2) U for a length-n dot product in
any summation order):
  shape_offsets   g_NB max(|S| |beta|)                                  v_shaped   that + U max|v_shaped|
  Jrest           e(v_shaped) (rows of J_regressor sum to 1) + g_V max(|Jreg| |v_shaped|)
  R               e_R = 32 U: a, n, sin a, cos a each within 4 U, three terms of size <= 1 per entry
  pose_offsets    e_R max_e sum_p |posedirs[p,e]| + g_P max(|pf| |posedirs|)    v_posed   e(v_shaped) + e(pose_offsets) + U max|v_posed|
  chain           in the 2-norm: E_R(j) = E_R(parent) + 3 e_R + 12 U (a product of rotations, so depth enters linearly);
                  e_t(j) = e_t(parent) + E_R(parent) |d_j| + sqrt 3 (2 e(Jrest) + U |d_j|) + 5 U (|G_p| |d_j| + |t_p|)
  J_transformed   e_t;      A's translation   e_t + E_R |J_j| + sqrt 3 e(Jrest) + 5 U (|t_j| + |G_j| |J_j|);   A's rotation E_R
  T               max_j e(A_j) (weights sum to 1) + g_J max(|W| |A|)
  verts           sum_c e(T[r,c]) |v_posed_c| + sum_c |T[r,c]| e(v_posed) + e(T[r,3]) + 6 U max(|T| [|v_posed|, 1])
Gradients: a running bound, kappa U * (the sum of |terms| behind the entry), the sum of |terms| from smpl_ref.backward(absolute=True)
and kappa = NB + V + P + J + 16 (depth + 1) + 64 the roundings along the longest path (the dot products, the chain both ways, Rodrigues).

GPU: the HIP kernels through hugs_amd.smpl.  Tolerance, per tensor (the eight outputs, dL/dbetas, dL/dpose, dL/dtransl): the float64
restatement of the same float32 inputs is the truth, the yardstick is the float32 torch restatement's own error on CPU,
    err_ref = max |torch_fp32_cpu - fp64|,      requirement    max |hip - fp64| <= 4 err_ref + 1e-6 max |fp64|
(the project's rule, tests/test_triplane.py).  All three figures are printed per tensor before the assertion (pytest -s).
No wall-clock assertion here: timing lives in tools/bench_smpl.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import smpl_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "reference_smpl.npz"))
U = 2.0 ** -24
SEED, GV, GJ, GNB = 7, 48, 24, 10
GRADS = ("grad_betas", "grad_pose", "grad_transl")


# ------------------------------------------------------------------------------------------------------------------- CPU

def _forward_bounds(model, out, cache, betas, disable):
    """the bounds of the docstring, one number per output tensor"""
    a = lambda x: np.abs(np.asarray(x, np.float64))
    S, Jreg, W, pd = a(model["shapedirs"]), a(model["J_regressor"]), a(model["lbs_weights"]), a(model["posedirs"])
    V, J, NB = S.shape[0], Jreg.shape[0], S.shape[2]
    P = 9 * (J - 1)
    g = lambda n: (n + 2) * U
    e_so = g(NB) * (S @ a(betas).reshape(-1)).max()
    e_vs = e_so + U * a(out["v_shaped"]).max()
    e_J = e_vs + g(V) * (Jreg @ a(out["v_shaped"])).max()
    e_R = 32 * U
    pf = a(cache["R"][1:] - np.eye(3)).reshape(-1)
    e_po = 0.0 if disable else e_R * pd.sum(0).max() + g(P) * (pf @ pd).max()
    e_vp = e_vs + e_po + U * a(out["v_posed"]).max()
    Gm, Jr, parents = cache["G"], cache["Jr"], cache["parents"]
    n2 = np.linalg.norm
    E_R, e_t = np.zeros(J), np.zeros(J)
    E_R[0], e_t[0] = 3 * e_R, np.sqrt(3) * e_J
    for j in range(1, J):
        p = parents[j]
        d = Jr[j] - Jr[p]
        E_R[j] = E_R[p] + 3 * e_R + 12 * U
        e_t[j] = e_t[p] + E_R[p] * n2(d) + np.sqrt(3) * (2 * e_J + U * n2(d)) + 5 * U * ((a(Gm[p, :3, :3]) @ a(d)).max() + a(Gm[p, :3, 3]).max())
    e_At = e_t + E_R * n2(Jr, axis=1) + np.sqrt(3) * e_J + 5 * U * (a(Gm[:, :3, 3]).max(1) + np.einsum("jrc,jc->jr", a(Gm[:, :3, :3]), a(Jr)).max(1))
    e_A_rot, e_A_tr = E_R.max(), e_At.max()
    Aabs = a(out["A"]).reshape(J, 16)
    e_T_sum = g(J) * (W @ Aabs).max()
    e_T_rot, e_T_tr = e_A_rot + e_T_sum, e_A_tr + e_T_sum
    T, vp = a(out["T"]), a(out["v_posed"])
    e_verts = (e_T_rot * vp.sum(1).max() + T[:, :3, :3].sum(2).max() * e_vp + e_T_tr
               + 6 * U * (np.einsum("vrc,vc->vr", T[:, :3, :3], vp) + T[:, :3, 3]).max())
    return {"shape_offsets": e_so, "v_shaped": e_vs, "pose_offsets": e_po, "v_posed": e_vp, "J_transformed": e_t.max(),
            "A": max(e_A_rot, e_A_tr), "T": max(e_T_rot, e_T_tr), "verts": e_verts}


@functools.lru_cache(maxsize=None)
def _golden_case(disable):
    model = sr.synthetic_model(SEED, GV, GJ, GNB, "smpl")
    betas, pose, _ = sr.synthetic_inputs(SEED, GJ, GNB)
    cot = {k: v[0] for k, v in sr.cotangents(SEED, GV, GJ).items()}
    out, cache = sr.forward(model, betas[0], pose[0], None, disable)
    return model, betas[0], pose[0], cot, out, cache


@pytest.mark.parametrize("disable", [False, True], ids=["posedirs", "posedirs_disabled"])
def test_fp64_restatement_reproduces_the_reference_outputs_and_gradients(disable):
    model, betas, pose, cot, out, cache = _golden_case(disable)
    tag = "nopd" if disable else "pd"
    bounds = _forward_bounds(model, out, cache, betas, disable)
    for k in sr.OUTPUTS:
        gold = G[f"{tag}_{k}"][0]
        assert gold.shape == out[k].shape, k
        err = np.abs(out[k] - gold).max()
        print(f"{tag} {k}: |fp64 - golden| {err:.3e}  bound {bounds[k]:.3e}  max |fp64| {np.abs(out[k]).max():.3e}")
        assert err <= bounds[k], k
    # gradients: the reference's v_posed IS v_shaped when posedirs are disabled, so both cotangents reach it -- as they do here
    d_betas, d_pose, _ = sr.backward(cache, cot)
    s_betas, s_pose, _ = sr.backward(cache, cot, absolute=True)
    kappa = GNB + GV + 9 * (GJ - 1) + GJ + 16 * (sr.depths(cache["parents"]).max() + 1) + 64
    for name, mine, sums in (("grad_betas", d_betas, s_betas), ("grad_pose", d_pose, s_pose)):
        err, bound = np.abs(mine - G[f"{tag}_{name}"][0]).max(), kappa * U * sums.max()
        print(f"{tag} {name}: |fp64 - golden| {err:.3e}  bound {bound:.3e}  max |fp64| {np.abs(mine).max():.3e}")
        assert err <= bound, name


@pytest.mark.parametrize("variant,tensors", [("transposed_pose_feature", ("pose_offsets", "v_posed", "verts")),
                                             ("parent_shifted", ("J_transformed", "A", "T", "verts")),
                                             ("rest_joint_kept", ("A", "T", "verts"))])
def test_a_wrong_variant_breaks_the_rounding_bound_a_hundredfold(variant, tensors):
    model, betas, pose, cot, out, cache = _golden_case(False)
    bounds = _forward_bounds(model, out, cache, betas, False)
    wrong, _ = sr.forward(model, betas, pose, None, False, variant=variant)
    for k in tensors:
        ratio = np.abs(wrong[k] - G[f"pd_{k}"][0]).max() / bounds[k]
        print(f"{variant} {k}: error / bound = {ratio:.3e}")
        assert ratio >= 100, (variant, k)


@pytest.mark.parametrize("tree,zero_pose", [("smpl", False), ("chain", False), ("star", False), ("smpl", True)])
def test_hand_written_backward_agrees_with_central_differences(tree, zero_pose):
    """float64; the loss is sum_k <cotangent_k, output_k>.  Step h = 1e-5: rounding 2.2e-16 |L| / h with |L| <~ 1e3 is 2e-8, truncation
    h^2 / 6 |L'''| with third derivatives of the size of the gradient is 2e-11 of it: the tolerance is 1e-6 max(1, max |gradient|)."""
    V, J, NB = 20, 24, 4
    model = sr.synthetic_model(11, V, J, NB, tree)
    betas, pose, transl = (x[0].astype(np.float64) for x in sr.synthetic_inputs(11, J, NB, zero_pose=zero_pose))
    cot = {k: v[0].astype(np.float64) for k, v in sr.cotangents(11, V, J).items()}
    loss = lambda b, p, t: sum((cot[k] * o).sum() for k, o in sr.forward(model, b, p, t)[0].items())
    _, cache = sr.forward(model, betas, pose, transl)
    grads = sr.backward(cache, cot)
    assert all(np.isfinite(g).all() for g in grads)
    h = 1e-5
    for i, (name, x, g) in enumerate(zip(GRADS, (betas, pose, transl), grads)):
        num = np.zeros_like(x)
        for e in range(x.size):
            args = [betas.copy(), pose.copy(), transl.copy()]
            args[i][e] += h
            up = loss(*args)
            args[i][e] -= 2 * h
            num[e] = (up - loss(*args)) / (2 * h)
        err, tol = np.abs(num - g).max(), 1e-6 * max(1.0, np.abs(g).max())
        print(f"{tree} zero_pose={zero_pose} {name}: |central difference - backward| {err:.3e}  tolerance {tol:.3e}")
        assert err <= tol, name


def test_zero_pose_gives_identity_rotations_and_transforms():
    V, J, NB = 20, 24, 4
    model = sr.synthetic_model(12, V, J, NB, "smpl")
    out, cache = sr.forward(model, np.zeros(NB), np.zeros(3 * J))
    assert np.array_equal(cache["R"], np.broadcast_to(np.eye(3), (J, 3, 3)))          # n = 0 / a: K = 0 exactly
    Jtemplate = model["J_regressor"].astype(np.float64) @ model["v_template"].astype(np.float64)
    assert np.abs(out["J_transformed"] - Jtemplate).max() <= 1e-15
    assert np.abs(out["A"] - np.eye(4)).max() <= 1e-15
    # T = sum_j w_j I: the float32 weights of a vertex sum to 1 within (J + 2) U
    assert np.abs(out["verts"] - model["v_template"].astype(np.float64)).max() <= (J + 2) * U * np.abs(model["v_template"]).max()
    # the float32 torch form too: exact identity rotations, finite gradients
    tm = sr.torch_model(model)
    pose = torch.zeros(1, 3 * J, requires_grad=True)
    res = sr.smpl_torch(tm, torch.zeros(1, NB), pose)
    assert torch.equal(sr.batch_rodrigues(pose.detach().view(-1, 3)), torch.eye(3).expand(J, 3, 3))
    res["A"].sum().backward()
    assert torch.isfinite(pose.grad).all()


def _lib():
    import diff_gaussian_rasterization as dgr
    return dgr._load()   # with the prototypes the wrapper calls through (diff_gaussian_rasterization/_abi.py)


def test_library_exports_the_three_entry_points():
    lib = _lib()
    assert all(hasattr(lib, s) for s in ("hgs_smpl_workspace", "hgs_smpl_forward", "hgs_smpl_backward"))
    header = open(os.path.join(ROOT, "include", "hgs_rasterizer.h")).read()
    assert "Row f-10" in header and all(s + "(" in header for s in ("hgs_smpl_workspace", "hgs_smpl_forward", "hgs_smpl_backward"))
    assert "/root/reference/hugs/models/modules/lbs.py:76-187" in header and "smpl_layer.py:411-519" in header


def test_workspace_is_monotone_in_V_and_zero_for_no_vertices():
    lib = _lib()
    assert lib.hgs_smpl_workspace(0, 24, 10) == 0
    sizes = [lib.hgs_smpl_workspace(V, 24, 10) for V in (1, 63, 64, 65, 256, 257, 6890, 100_000)]
    print("workspace bytes:", sizes)
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]


def test_entry_points_validate_on_the_host_before_any_launch():
    """Every call here returns from the argument checks (there is no GPU in a CPU run): fake non-null pointers are never dereferenced."""
    lib = _lib()
    smpl = (C.c_int32 * 24)(*sr.SMPL_PARENTS)
    F = 256   # a fake, 16-byte aligned device pointer

    def fwd(V=4, J=24, NB=10, parents=smpl, disable=0, **kw):
        a = dict(betas=F, pose=F, transl=None, v_template=F, shapedirs=F, posedirs=F, J_regressor=F, lbs_weights=F)
        o = dict(verts=F, Jtr=F, A=F, T=F, v_posed=F, v_shaped=F, so=F, po=F, ws=F)
        for k, v in kw.items():
            (a if k in a else o)[k] = v
        return lib.hgs_smpl_forward(V, J, NB, parents, *a.values(), disable, *o.values(), None)

    def bwd(V=4, J=24, NB=10, parents=smpl, disable=0, **kw):
        a = dict(pose=F, shapedirs=F, posedirs=F, J_regressor=F, lbs_weights=F)
        o = dict(v_posed=F, T=F, g_verts=None, g_Jtr=None, g_A=F, g_T=None, g_vp=None, g_vs=None, g_so=None, g_po=None, d_betas=F,
                 d_pose=F, d_transl=None, ws=F)
        for k, v in kw.items():
            (a if k in a else o)[k] = v
        return lib.hgs_smpl_backward(V, J, NB, parents, *a.values(), disable, *o.values(), None)

    for call, what in ((fwd, b"smpl_forward"), (bwd, b"smpl_backward")):
        for bad in (dict(V=-1), dict(J=1), dict(J=33, parents=(C.c_int32 * 33)(-1, *range(32))), dict(NB=0), dict(NB=17)):
            assert call(**bad) == -1 and what in lib.hgs_last_error() and b"need V >= 0" in lib.hgs_last_error(), bad
        assert call(parents=None) == -1 and b"null pointer" in lib.hgs_last_error()
        for tree in ((0,) + sr.SMPL_PARENTS[1:], (-1, 1) + sr.SMPL_PARENTS[2:], sr.SMPL_PARENTS[:23] + (23,), sr.SMPL_PARENTS[:5] + (-1,) + sr.SMPL_PARENTS[6:]):
            assert call(parents=(C.c_int32 * 24)(*tree)) == -1 and b"bad parents array" in lib.hgs_last_error() and what in lib.hgs_last_error(), tree
        for name in ("pose", "shapedirs", "J_regressor", "lbs_weights", "v_posed", "T", "ws"):
            assert call(**{name: None}) == -1 and b"null pointer" in lib.hgs_last_error(), name
        assert call(posedirs=None) == -1 and b"disable_posedirs" in lib.hgs_last_error()
        assert call(T=F + 4) == -1 and b"16-byte aligned" in lib.hgs_last_error()
    assert fwd(V=0) == 0 and fwd(V=0, betas=None, ws=None) == 0                       # nothing to do, nothing touched
    assert fwd(V=0, J=40) == -1                                                        # ... but the sizes are still checked
    for name in ("betas", "v_template", "verts", "Jtr", "A", "so", "po", "v_shaped"):
        assert fwd(**{name: None}) == -1 and b"null pointer" in lib.hgs_last_error(), name
    for name in ("d_betas", "d_pose"):
        assert bwd(**{name: None}) == -1 and b"null pointer" in lib.hgs_last_error(), name
    assert bwd(g_T=F + 4) == -1 and b"16-byte aligned" in lib.hgs_last_error()


def test_the_wrapper_refuses_what_it_does_not_implement_and_cpu_tensors():
    from hugs_amd.smpl import lbs, smpl_forward
    m = sr.torch_model(sr.synthetic_model(3, 8, 24, 10, "smpl"))
    betas, pose, transl = (torch.from_numpy(x) for x in sr.synthetic_inputs(3, 24, 10))
    args = lambda **kw: (betas, pose, kw.get("v_template", m["v_template"]), m["shapedirs"], kw.get("posedirs", m["posedirs"]), m["J_regressor"],
                         m["parents"], m["lbs_weights"])
    with pytest.raises(NotImplementedError, match="pose2rot"):
        lbs(*args(), pose2rot=False)
    with pytest.raises(NotImplementedError, match="vert_offsets"):
        lbs(*args(), vert_offsets=torch.zeros(1, 8, 3))
    with pytest.raises(NotImplementedError, match="requires grad"):
        lbs(*args(v_template=m["v_template"].clone().requires_grad_()))
    with pytest.raises(NotImplementedError, match="requires grad"):
        lbs(*args(posedirs=m["posedirs"].clone().requires_grad_()))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lbs(*args())
    from types import SimpleNamespace
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        smpl_forward(SimpleNamespace(**m), betas, pose[:, 3:], pose[:, :3], transl)


# ------------------------------------------------------------------------------------------------------------------- GPU

@functools.lru_cache(maxsize=None)
def _reference(V, J, NB, tree, disable, with_transl, zero_pose, B, which):
    """float64 truth and the float32 torch yardstick for one case, computed once: (model, inputs, cotangents, truth [b] dicts, err_ref dict).
    `which`: the outputs that carry a cotangent."""
    seed = 100 + V % 97 + J + NB
    model = sr.synthetic_model(seed, V, J, NB, tree)
    betas, pose, transl = sr.synthetic_inputs(seed, J, NB, B=B, zero_pose=zero_pose)
    cot = {k: v for k, v in sr.cotangents(seed, V, J, B=B).items() if k in which}
    truth = []
    for b in range(B):
        out, cache = sr.forward(model, betas[b], pose[b], transl[b] if with_transl else None, disable)
        gb, gp, gt = sr.backward(cache, {k: v[b] for k, v in cot.items()})
        truth.append(dict(out, grad_betas=gb, grad_pose=gp, grad_transl=gt))
    tm = sr.torch_model(model)
    tb, tp, tt = (torch.from_numpy(x).requires_grad_() for x in (betas, pose, transl))
    res = sr.smpl_torch(tm, tb, tp, tt if with_transl else None, disable)
    sum((res[k] * torch.from_numpy(v)).sum() for k, v in cot.items()).backward()
    ref32 = {k: v.detach().numpy() for k, v in res.items()}
    ref32.update(grad_betas=tb.grad.numpy(), grad_pose=tp.grad.numpy())
    if with_transl:
        ref32["grad_transl"] = tt.grad.numpy()
    err_ref = {k: max(np.abs(ref32[k][b] - truth[b][k]).max() for b in range(B)) for k in ref32}
    return model, (betas, pose, transl), cot, truth, err_ref


def _run_hip(device, model, inputs, cot, disable, with_transl):
    from hugs_amd.smpl import smpl_forward
    from types import SimpleNamespace
    m = SimpleNamespace(**sr.torch_model(model, device))
    betas, pose, transl = (torch.from_numpy(x).to(device).requires_grad_() for x in inputs)
    out = smpl_forward(m, betas, pose[:, 3:], pose[:, :3], transl if with_transl else None, disable_posedirs=disable)
    res = dict(verts=out.vertices, J_transformed=out.joints, A=out.A, T=out.T, v_posed=out.v_posed, v_shaped=out.v_shaped,
               shape_offsets=out.shape_offsets, pose_offsets=out.pose_offsets)
    torch.autograd.backward([res[k] for k in cot], [torch.from_numpy(v).to(device) for v in cot.values()])
    torch.cuda.synchronize()
    got = {k: v.detach().cpu().numpy() for k, v in res.items()}
    got.update(grad_betas=betas.grad.cpu().numpy(), grad_pose=pose.grad.cpu().numpy())
    if with_transl:
        got["grad_transl"] = transl.grad.cpu().numpy()
    return got


def _check(label, got, truth, err_ref):
    bad = []
    for k in err_ref:
        B = len(truth)
        err = max(np.abs(got[k][b].astype(np.float64) - truth[b][k].reshape(got[k][b].shape)).max() for b in range(B))
        scale = max(np.abs(truth[b][k]).max() for b in range(B))
        tol = 4 * err_ref[k] + 1e-6 * scale
        print(f"{label} {k}: |hip - fp64| {err:.3e}  |torch_fp32 - fp64| {err_ref[k]:.3e}  max |fp64| {scale:.3e}  ratio {err / max(err_ref[k], 1e-300):.2f}"
              f"{'' if err <= 4 * err_ref[k] else '  (held by the floor)' if err <= tol else '  FAILS'}")
        assert np.isfinite(got[k]).all(), k
        if not err <= tol:
            bad.append(k)
    assert not bad, (label, bad)


ALL = sr.OUTPUTS
CASES = [  # V, J, NB, tree, disable_posedirs, transl, zero pose
    (1, 24, 10, "smpl", False, True, False), (63, 24, 10, "smpl", False, True, False), (64, 24, 10, "smpl", False, True, False),
    (65, 24, 10, "smpl", False, True, False), (257, 24, 10, "smpl", False, True, False), (6890, 24, 10, "smpl", False, True, False),
    (65, 24, 10, "smpl", True, True, False), (6890, 24, 10, "smpl", True, False, False), (257, 24, 10, "smpl", False, False, False),
    (257, 2, 10, "star", False, True, False), (257, 32, 10, "chain", False, True, False), (257, 24, 1, "smpl", False, True, False),
    (257, 24, 16, "smpl", False, True, False), (257, 24, 10, "chain", False, True, False), (257, 24, 10, "star", False, True, False),
    (257, 24, 10, "smpl", False, True, True), (257, 24, 10, "smpl", True, True, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("V,J,NB,tree,disable,with_transl,zero_pose", CASES)
def test_gpu_outputs_and_gradients_with_all_eight_cotangents(device, V, J, NB, tree, disable, with_transl, zero_pose):
    model, inputs, cot, truth, err_ref = _reference(V, J, NB, tree, disable, with_transl, zero_pose, 1, ALL)
    got = _run_hip(device, model, inputs, cot, disable, with_transl)
    _check(f"V={V} J={J} NB={NB} {tree} disable={disable} transl={with_transl} zero_pose={zero_pose}", got, truth, err_ref)
    if zero_pose:
        A0 = got["A"][0].copy()
        if with_transl:
            A0[:, :3, 3] -= inputs[2][0]
        assert np.abs(A0[:, :3, :3] - np.eye(3)).max() == 0.0                       # R = I exactly


@pytest.mark.gpu
@pytest.mark.parametrize("disable", [False, True], ids=["posedirs", "posedirs_disabled"])
def test_gpu_backward_with_only_the_cotangent_of_A(device, disable):
    """the HUGS training case: smpl_output.A is all the step reads"""
    model, inputs, cot, truth, err_ref = _reference(6890, 24, 10, "smpl", disable, True, False, 1, ("A",))
    _check(f"only A, disable={disable}", _run_hip(device, model, inputs, cot, disable, True), truth, err_ref)


@pytest.mark.gpu
def test_gpu_batch_of_three_through_the_wrapper(device):
    model, inputs, cot, truth, err_ref = _reference(257, 24, 10, "smpl", False, True, False, 3, ALL)
    got = _run_hip(device, model, inputs, cot, False, True)
    assert got["verts"].shape == (3, 257, 3) and got["A"].shape == (3, 24, 4, 4) and got["grad_pose"].shape == (3, 72)
    _check("batch of 3", got, truth, err_ref)


@pytest.mark.gpu
def test_gpu_lbs_has_the_reference_return_tuple(device):
    from hugs_amd.smpl import lbs
    model, inputs, cot, truth, err_ref = _reference(257, 24, 10, "smpl", False, False, False, 1, ALL)
    m = sr.torch_model(model, device)
    betas, pose = (torch.from_numpy(x).to(device) for x in inputs[:2])
    res = lbs(betas, pose, m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["parents"], m["lbs_weights"])
    assert len(res) == 8
    got = {k: v.cpu().numpy() for k, v in zip(sr.OUTPUTS, res)}
    _check("lbs()", got, truth, {k: err_ref[k] for k in sr.OUTPUTS})


@pytest.mark.gpu
def test_gpu_two_identical_calls_are_bit_identical(device):
    model, inputs, cot, _, _ = _reference(6890, 24, 10, "smpl", False, True, False, 1, ALL)
    a = _run_hip(device, model, inputs, cot, False, True)
    b = _run_hip(device, model, inputs, cot, False, True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
def test_gpu_A_feeds_lbs_extra_and_backpropagates_to_body_pose(device):
    """smpl_forward(...).A -> hugs_amd.lbs.lbs_extra on n = 1 000 points -> a loss on the deformed points; dL/dbody_pose, dL/dbetas
    and dL/dtransl against the float64 chain under the same rule."""
    from hugs_amd.lbs import lbs_extra
    from hugs_amd.smpl import smpl_forward
    from types import SimpleNamespace
    V, J, NB, n = 257, 24, 10, 1000
    model, inputs, _, _, _ = _reference(V, J, NB, "smpl", True, True, False, 1, ALL)
    rs = np.random.RandomState(5)
    pts = rs.normal(0, 0.3, (1, n, 3)).astype(np.float32)
    logits = rs.normal(0, 2.0, (n, J))
    Wn = (np.exp(logits) / np.exp(logits).sum(1, keepdims=True)).astype(np.float32)
    g_pts = rs.normal(0, 1.0, (1, n, 3)).astype(np.float32)
    betas, pose, transl = inputs
    # float64: deformed = sum_j Wn A_j [pts, 1]  =>  dL/dA_j = sum_i Wn[i,j] g_i [pts_i, 1]^T
    out, cache = sr.forward(model, betas[0], pose[0], transl[0], True)
    ph = np.concatenate([pts[0].astype(np.float64), np.ones((n, 1))], 1)
    dT = np.zeros((n, 4, 4))
    dT[:, :3, :] = g_pts[0].astype(np.float64)[:, :, None] * ph[:, None, :]
    gA = (Wn.astype(np.float64).T @ dT.reshape(n, 16)).reshape(J, 4, 4)
    truth = dict(zip(GRADS, sr.backward(cache, {"A": gA})))
    # float32 torch on CPU: the yardstick
    tm = sr.torch_model(model)
    tb, tp, tt = (torch.from_numpy(x).requires_grad_() for x in inputs)
    A32 = sr.smpl_torch(tm, tb, tp, tt, True)["A"]
    T32 = torch.matmul(torch.from_numpy(Wn), A32.view(1, J, 16)).view(1, n, 4, 4)
    d32 = torch.matmul(T32[:, :, :3, :3], torch.from_numpy(pts)[..., None])[..., 0] + T32[:, :, :3, 3]
    (d32 * torch.from_numpy(g_pts)).sum().backward()
    err_ref = {k: np.abs(t.grad.numpy()[0] - truth[k]).max() for k, t in zip(GRADS, (tb, tp, tt))}
    # the fused rows
    m = SimpleNamespace(**sr.torch_model(model, device))
    hb, hp, ht = (torch.from_numpy(x).to(device).requires_grad_() for x in inputs)
    body_pose = hp[:, 3:].detach().clone().requires_grad_()
    A = smpl_forward(m, hb, body_pose, hp[:, :3], ht, disable_posedirs=True).A
    verts = lbs_extra(A, torch.from_numpy(pts).to(device), None, torch.from_numpy(Wn).to(device), None, disable_posedirs=True)[0]
    (verts * torch.from_numpy(g_pts).to(device)).sum().backward()
    torch.cuda.synchronize()
    assert body_pose.grad is not None and torch.isfinite(body_pose.grad).all()
    got = dict(grad_betas=hb.grad.cpu().numpy(), grad_pose=np.concatenate([hp.grad.cpu().numpy()[:, :3], body_pose.grad.cpu().numpy()], 1),
               grad_transl=ht.grad.cpu().numpy())
    _check("smpl_forward -> lbs_extra", got, [truth], err_ref)
