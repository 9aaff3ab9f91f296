"""Row f-10 -- the SMPL body model's forward, restated from the published formulas (not from the reference's text).

Two forms of the same statements:
  * float64 numpy, one batch element: `forward` and a hand-written `backward` (the truth the kernels are measured against);
  * torch, any dtype and device, batched: the four third-party functions the reference imports (`batch_rodrigues`, `blend_shapes`,
    `vertices2joints`, `batch_rigid_transform`), `lbs_torch` and `smpl_torch` (with the translation).  In float32 this form is the
    yardstick of tests/test_smpl.py and the torch-statement side of tools/bench_smpl.py; tests/golden/make_golden_smpl.py hands the
    four functions to the reference's own lbs().

Formulas (J joints, V vertices, NB shape coefficients, P = 9 (J - 1)):
  shape_offsets[v,k] = sum_l shapedirs[v,k,l] beta_l;  v_shaped = v_template + shape_offsets;  Jrest = J_regressor v_shaped
  a = |r + 1e-8|, n = r / a, K = hat(n), R = I + sin a K + (1 - cos a) K^2                   (epsilon inside the norm only)
  pose_feature = (R[1:] - I) flattened row-major per joint;  pose_offsets = pose_feature posedirs;  v_posed = v_shaped + pose_offsets
  G_0 = [R_0 | Jrest_0],  G_j = G_parent(j) [R_j | Jrest_j - Jrest_parent(j)];  J_transformed = G[:, :3, 3]
  A_j = G_j with translation t_j - G_j[:3,:3] Jrest_j;  T_v = sum_j W[v,j] A_j;  verts_v = T_v [v_posed_v, 1]
  transl, if given, is added to verts, J_transformed, A[:, :3, 3] and T[:, :3, 3].
"""
import numpy as np

SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)
OUTPUTS = ("verts", "J_transformed", "A", "T", "v_posed", "v_shaped", "shape_offsets", "pose_offsets")


def tree_parents(tree, J):
    if tree == "smpl":
        assert J == 24
        return np.array(SMPL_PARENTS, np.int64)
    if tree == "chain":
        return np.arange(-1, J - 1, dtype=np.int64)
    if tree == "star":
        return np.array([-1] + [0] * (J - 1), np.int64)
    raise ValueError(tree)


def depths(parents):
    d = np.zeros(len(parents), np.int64)
    for j in range(1, len(parents)):
        d[j] = d[parents[j]] + 1
    return d


def synthetic_model(seed, V, J, NB, tree):
    """A body-model-shaped set of buffers (float32) from numpy.random.RandomState(seed): a smooth template of about a metre,
    shapedirs / posedirs that move a vertex by centimetres, a sparse-ish non-negative J_regressor with unit row sums, softmax
    skinning weights."""
    rs = np.random.RandomState(seed)
    u = (np.arange(V) + 0.5) / V
    amp, ph = rs.uniform(0.1, 0.4, (4, 3)), rs.uniform(0, 2 * np.pi, (4, 3))
    v_template = sum(amp[m] * np.sin(2 * np.pi * (m + 1) * u[:, None] + ph[m]) for m in range(4))
    shapedirs = rs.normal(0, 0.01, (V, 3, NB))
    posedirs = rs.normal(0, 0.005, (9 * (J - 1), 3 * V))
    keep = rs.uniform(size=(J, V)) < min(1.0, 8.0 / V)
    keep[np.arange(J), rs.randint(0, V, J)] = True
    Jr = rs.uniform(0.1, 1.0, (J, V)) * keep
    Jr /= Jr.sum(1, keepdims=True)
    logits = rs.normal(0, 2.0, (V, J))
    W = np.exp(logits - logits.max(1, keepdims=True))
    W /= W.sum(1, keepdims=True)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(v_template=f(v_template), shapedirs=f(shapedirs), posedirs=f(posedirs), J_regressor=f(Jr), lbs_weights=f(W),
                parents=tree_parents(tree, J))


def synthetic_inputs(seed, J, NB, B=1, zero_pose=False):
    rs = np.random.RandomState(seed + 1000)
    betas = rs.normal(0, 1.0, (B, NB)).astype(np.float32)
    pose = rs.normal(0, 0.3, (B, 3 * J)).astype(np.float32)
    transl = rs.normal(0, 0.5, (B, 3)).astype(np.float32)
    if zero_pose:
        pose[:] = 0
    return betas, pose, transl


def cotangents(seed, V, J, B=1):
    """fixed random cotangents of the eight outputs, float32, in OUTPUTS' order"""
    rs = np.random.RandomState(seed + 2000)
    shapes = {"verts": (V, 3), "J_transformed": (J, 3), "A": (J, 4, 4), "T": (V, 4, 4), "v_posed": (V, 3), "v_shaped": (V, 3),
              "shape_offsets": (V, 3), "pose_offsets": (V, 3)}
    return {k: rs.normal(0, 1.0, (B,) + shapes[k]).astype(np.float32) for k in OUTPUTS}


# ------------------------------------------------------------------------------------------------------------ float64 numpy

def _hat(n):
    K = np.zeros(n.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -n[..., 2], n[..., 1]
    K[..., 1, 0], K[..., 1, 2] = n[..., 2], -n[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -n[..., 1], n[..., 0]
    return K


def rodrigues(r, eps=1e-8):
    """r [J,3] -> R [J,3,3]"""
    r = np.asarray(r, np.float64)
    a = np.sqrt(((r + eps) ** 2).sum(-1))
    K = _hat(r / a[:, None])
    return np.eye(3) + np.sin(a)[:, None, None] * K + (1 - np.cos(a))[:, None, None] * (K @ K)


def rodrigues_backward(r, dR, eps=1e-8):
    r = np.asarray(r, np.float64)
    rp = r + eps
    a = np.sqrt((rp ** 2).sum(-1))
    K = _hat(r / a[:, None])
    s, c = np.sin(a)[:, None, None], np.cos(a)[:, None, None]
    Kt = K.transpose(0, 2, 1)
    dK = s * dR + (1 - c) * (dR @ Kt + Kt @ dR)
    dn = np.stack([dK[:, 2, 1] - dK[:, 1, 2], dK[:, 0, 2] - dK[:, 2, 0], dK[:, 1, 0] - dK[:, 0, 1]], -1)
    da = c[:, 0, 0] * (dR * K).sum((1, 2)) + s[:, 0, 0] * (dR * (K @ K)).sum((1, 2)) - (dn * r).sum(-1) / a ** 2
    return dn / a[:, None] + da[:, None] * rp / a[:, None]


def forward(model, betas, pose, transl=None, disable_posedirs=False, variant=None):
    """One batch element in float64.  `variant` builds one of three deliberately wrong forms (the CPU test shows each breaks the
    rounding bound): 'transposed_pose_feature' (R^T - I), 'parent_shifted' (the chain walks to parent - 1), 'rest_joint_kept' (A
    without the removal of the rest joint).  Returns (outputs dict, cache for backward)."""
    f = lambda a: np.asarray(a, np.float64)
    vt, S, Jreg, W = f(model["v_template"]), f(model["shapedirs"]), f(model["J_regressor"]), f(model["lbs_weights"])
    parents = np.asarray(model["parents"]).astype(np.int64).copy()
    if variant == "parent_shifted":
        parents[1:] = np.maximum(parents[1:] - 1, 0)
    betas, pose = f(betas).reshape(-1), f(pose).reshape(-1, 3)
    V, J = vt.shape[0], Jreg.shape[0]
    so = S @ betas
    vs = vt + so
    Jr = Jreg @ vs
    R = rodrigues(pose)
    pf = (R[1:].transpose(0, 2, 1) if variant == "transposed_pose_feature" else R[1:]) - np.eye(3)
    po = np.zeros_like(vs) if disable_posedirs else (pf.reshape(-1) @ f(model["posedirs"])).reshape(V, 3)
    vp = vs + po
    G = np.zeros((J, 4, 4))
    G[:, 3, 3] = 1
    G[0, :3, :3], G[0, :3, 3] = R[0], Jr[0]
    for j in range(1, J):
        L = np.eye(4)
        L[:3, :3], L[:3, 3] = R[j], Jr[j] - Jr[parents[j]]
        G[j] = G[parents[j]] @ L
    Jtr = G[:, :3, 3].copy()
    A = G.copy()
    if variant != "rest_joint_kept":
        A[:, :3, 3] -= np.einsum("jrc,jc->jr", G[:, :3, :3], Jr)
    T = (W @ A.reshape(J, 16)).reshape(V, 4, 4)
    verts = np.einsum("vrc,vc->vr", T[:, :3, :3], vp) + T[:, :3, 3]
    cache = dict(model=model, pose=pose, R=R, Jr=Jr, G=G, vp=vp, T0=T.copy(), parents=parents, disable=disable_posedirs)
    if transl is not None:
        tr = f(transl).reshape(3)
        verts, Jtr, A, T = verts + tr, Jtr + tr, A.copy(), T.copy()
        A[:, :3, 3] += tr
        T[:, :3, 3] += tr
    return dict(verts=verts, J_transformed=Jtr, A=A, T=T, v_posed=vp, v_shaped=vs, shape_offsets=so, pose_offsets=po), cache


def backward(cache, grads, absolute=False):
    """Hand-written reverse pass: `grads` maps output names to cotangents (missing / None = zero) -> (d_betas [NB], d_pose [3J],
    d_transl [3]).  With absolute=True every factor and cotangent enters by its absolute value and every difference becomes a sum:
    the result bounds the sum of |terms| behind each gradient entry, the quantity a running rounding-error bound multiplies."""
    ab = (lambda a: np.abs(a)) if absolute else (lambda a: a)
    sg = 1.0 if absolute else -1.0
    f = lambda a: ab(np.asarray(a, np.float64))
    m = cache["model"]
    S, Jreg, W = f(m["shapedirs"]), f(m["J_regressor"]), f(m["lbs_weights"])
    R, Jr, G, vp, T0, parents = ab(cache["R"]), ab(cache["Jr"]), ab(cache["G"]), ab(cache["vp"]), ab(cache["T0"]), cache["parents"]
    V, J = vp.shape[0], R.shape[0]
    z = {"verts": (V, 3), "J_transformed": (J, 3), "A": (J, 4, 4), "T": (V, 4, 4), "v_posed": (V, 3), "v_shaped": (V, 3),
         "shape_offsets": (V, 3), "pose_offsets": (V, 3)}
    g = {k: (np.zeros(s) if grads.get(k) is None else f(grads[k]).reshape(s)) for k, s in z.items()}
    d_transl = g["verts"].sum(0) + g["J_transformed"].sum(0) + g["A"][:, :3, 3].sum(0) + g["T"][:, :3, 3].sum(0)
    dT = g["T"].copy()
    dT[:, :3, :3] += g["verts"][:, :, None] * vp[:, None, :]
    dT[:, :3, 3] += g["verts"]
    dvp = np.einsum("vrc,vr->vc", T0[:, :3, :3], g["verts"]) + g["v_posed"]
    dA = (W.T @ dT.reshape(V, 16)).reshape(J, 4, 4) + g["A"]
    Rg, dAt = G[:, :3, :3], dA[:, :3, 3]
    dRg = dA[:, :3, :3] + sg * dAt[:, :, None] * Jr[:, None, :]
    dt = dAt + g["J_transformed"]
    dJ = sg * np.einsum("jrc,jr->jc", Rg, dAt)
    dR = np.zeros((J, 3, 3))
    for j in range(J - 1, 0, -1):
        p = parents[j]
        d = (Jr[j] + Jr[p]) if absolute else (Jr[j] - Jr[p])
        dR[j] = Rg[p].T @ dRg[j]
        dRg[p] += dRg[j] @ R[j].T + np.outer(dt[j], d)
        u = Rg[p].T @ dt[j]
        dJ[j] += u
        dJ[p] += sg * u
        dt[p] += dt[j]
    dR[0] = dRg[0]
    dJ[0] += dt[0]
    if not cache["disable"]:
        dR[1:] += (f(m["posedirs"]) @ (dvp + g["pose_offsets"]).reshape(-1)).reshape(J - 1, 3, 3)
    if absolute:   # |dr| <= sum |dR| |dR/dr|, the Jacobian by central differences of the formula itself
        r, h = cache["pose"], 1e-6
        d_pose = np.zeros((J, 3))
        for k in range(3):
            e = np.zeros(3)
            e[k] = h
            d_pose[:, k] = (dR * np.abs(rodrigues(r + e) - rodrigues(r - e)) / (2 * h)).sum((1, 2))
    else:
        d_pose = rodrigues_backward(cache["pose"], dR)
    dvs = dvp + g["v_shaped"] + Jreg.T @ dJ
    d_betas = np.einsum("vkl,vk->l", S, dvs + g["shape_offsets"])
    return d_betas, d_pose.reshape(-1), d_transl


# -------------------------------------------------------------------------------------------------------------------- torch

def batch_rodrigues(rot_vecs, epsilon=1e-8):
    """axis-angle [N,3] -> [N,3,3]"""
    import torch
    angle = torch.norm(rot_vecs + epsilon, dim=1, keepdim=True)
    n = rot_vecs / angle
    cos, sin = torch.cos(angle)[:, None], torch.sin(angle)[:, None]
    nx, ny, nz = n[:, 0:1], n[:, 1:2], n[:, 2:3]
    zero = torch.zeros_like(nx)
    K = torch.cat([zero, -nz, ny, nz, zero, -nx, -ny, nx, zero], dim=1).view(-1, 3, 3)
    eye = torch.eye(3, dtype=rot_vecs.dtype, device=rot_vecs.device)[None]
    return eye + sin * K + (1 - cos) * torch.bmm(K, K)


def blend_shapes(betas, shape_disps):
    """betas [B,NB], shape_disps [V,3,NB] -> [B,V,3]"""
    import torch
    return torch.einsum("bl,mkl->bmk", betas, shape_disps)


def vertices2joints(J_regressor, vertices):
    """[J,V], [B,V,3] -> [B,J,3]"""
    import torch
    return torch.einsum("bik,ji->bjk", vertices, J_regressor)


def batch_rigid_transform(rot_mats, joints, parents, dtype=None):
    """rot_mats [B,J,3,3], joints [B,J,3], parents [J] -> (posed joints [B,J,3], relative transforms A [B,J,4,4])"""
    import torch
    B, J = joints.shape[:2]
    rel = joints.clone()
    rel[:, 1:] = rel[:, 1:] - joints[:, parents[1:]]
    bottom = torch.zeros(B, J, 1, 4, dtype=joints.dtype, device=joints.device)
    bottom[..., 3] = 1
    local = torch.cat([torch.cat([rot_mats, rel[..., None]], dim=3), bottom], dim=2)
    chain, plist = [local[:, 0]], [int(p) for p in (parents.tolist() if hasattr(parents, "tolist") else parents)]
    for j in range(1, J):
        chain.append(torch.matmul(chain[plist[j]], local[:, j]))
    G = torch.stack(chain, dim=1)
    posed = G[:, :, :3, 3]
    moved = torch.matmul(G[:, :, :3, :3], joints[..., None])                      # G's rotation applied to the rest joint
    A = torch.cat([G[..., :3], torch.cat([G[:, :, :3, 3:] - moved, G[:, :, 3:, 3:]], dim=2)], dim=3)
    return posed, A


def lbs_torch(betas, pose, v_template, shapedirs, posedirs, J_regressor, parents, lbs_weights, disable_posedirs=False):
    """the statements of the module docstring with torch ops, batched; the same return tuple as the fused lbs()"""
    import torch
    B = max(betas.shape[0], pose.shape[0])
    shape_offsets = blend_shapes(betas, shapedirs)
    v_shaped = v_template + shape_offsets
    J = vertices2joints(J_regressor, v_shaped)
    R = batch_rodrigues(pose.reshape(-1, 3)).view(B, -1, 3, 3)
    eye = torch.eye(3, dtype=betas.dtype, device=betas.device)
    if disable_posedirs:
        pose_offsets = torch.zeros_like(v_shaped)
        v_posed = v_shaped
    else:
        pose_offsets = torch.matmul((R[:, 1:] - eye).reshape(B, -1), posedirs).view(B, -1, 3)
        v_posed = v_shaped + pose_offsets
    J_transformed, A = batch_rigid_transform(R, J, parents)
    T = torch.matmul(lbs_weights[None].expand(B, -1, -1), A.view(B, -1, 16)).view(B, -1, 4, 4)
    verts = torch.matmul(T[:, :, :3, :3], v_posed[..., None])[..., 0] + T[:, :, :3, 3]
    return verts, J_transformed, A, T, v_posed, v_shaped, shape_offsets, pose_offsets


def smpl_torch(model, betas, pose, transl=None, disable_posedirs=False):
    """lbs_torch on a dict of torch buffers, then the translation; returns a dict keyed by OUTPUTS"""
    import torch
    out = list(lbs_torch(betas, pose, model["v_template"], model["shapedirs"], model["posedirs"], model["J_regressor"], model["parents"],
                         model["lbs_weights"], disable_posedirs))
    if transl is not None:
        t = transl[:, None]
        out[0] = out[0] + t
        out[1] = out[1] + t
        shift = torch.zeros(transl.shape[0], 1, 4, 4, dtype=transl.dtype, device=transl.device)
        shift[:, 0, :3, 3] = transl
        out[2] = out[2] + shift
        out[3] = out[3] + shift
    return dict(zip(OUTPUTS, out))


def torch_model(model, device="cpu", dtype=None):
    import torch
    dtype = dtype or torch.float32
    d = {k: torch.from_numpy(np.asarray(model[k])).to(device=device, dtype=dtype) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights")}
    d["parents"] = torch.from_numpy(np.asarray(model["parents"]).astype(np.int64)).to(device)
    return d
