"""float64 numpy restatement of row f-8 (TriPlane.forward and its backward), written from the semantics, for tests/test_triplane.py:

    g = ((x - center) / scale + 0.5) * 2 - 1
    per plane, grid_sample(align_corners=True, bilinear, zeros padding): ix = ((g_w + 1) / 2) (W - 1), iy likewise with H;
    (x0, y0) = floor; weights nw = (x0 + 1 - ix)(y0 + 1 - iy), ne = (ix - x0)(y0 + 1 - iy), sw = (x0 + 1 - ix)(iy - y0),
    se = (ix - x0)(iy - y0); a corner outside the plane contributes nothing forward and receives nothing backward.
    feat[n, p F + c], planes p = xy, xz, yz.

Which coordinate runs along which axis: a plane is [1, F, H, W] and grid[..., 0] indexes W, the LAST axis -- plane_xy [1,F,resX,resY]:
x along W = resY, y along H = resX; plane_xz [1,F,resX,resZ]: x along W = resZ, z along H = resX; plane_yz [1,F,resY,resZ]: y along
W = resZ, z along H = resY.  Inputs are taken as they are (float32 values) and everything is evaluated in float64."""
import numpy as np

AXES = ((0, 1), (0, 2), (1, 2))   # per plane: (coordinate along W, coordinate along H)


def _cells(planes, x, center, scale):
    g = ((np.asarray(x, np.float64).reshape(-1, 3) - float(center)) / float(scale) + 0.5) * 2.0 - 1.0
    for p, (aw, ah) in enumerate(AXES):
        v = np.asarray(planes[p], np.float64)[0]                    # [F, H, W]
        H, W = v.shape[1:]
        ix, iy = ((g[:, aw] + 1.0) / 2.0) * (W - 1), ((g[:, ah] + 1.0) / 2.0) * (H - 1)
        x0, y0 = np.floor(ix), np.floor(iy)
        tx0, tx1, ty0, ty1 = ix - x0, x0 + 1.0 - ix, iy - y0, y0 + 1.0 - iy
        # corner: (dx, dy, weight, d weight / d ix, d weight / d iy)
        corners = ((0, 0, tx1 * ty1, -ty1, -tx1), (1, 0, tx0 * ty1, ty1, -tx0), (0, 1, tx1 * ty0, -ty0, tx1), (1, 1, tx0 * ty0, ty0, tx0))
        out = []
        for dx, dy, w, wx, wy in corners:
            cx, cy = x0 + dx, y0 + dy
            ok = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)          # (NaN compares false: no corner)
            out.append((ok, np.where(ok, cx, 0).astype(np.int64), np.where(ok, cy, 0).astype(np.int64), w, wx, wy))
        yield p, v, H, W, out


def forward(planes, x, center=0.0, scale=2.0):
    """planes: three [1,F,H,W] arrays, x [..., 3] -> feat [..., 3F] (float64)"""
    x = np.asarray(x)
    F = planes[0].shape[1]
    feat = np.zeros((x.reshape(-1, 3).shape[0], 3 * F))
    for p, v, H, W, corners in _cells(planes, x, center, scale):
        for ok, cx, cy, w, _, _ in corners:
            feat[:, p * F:(p + 1) * F] += np.where(ok[:, None], v[:, cy, cx].T * w[:, None], 0.0)
    return feat.reshape(*x.shape[:-1], 3 * F)


def backward(planes, x, g_feat, center=0.0, scale=2.0):
    """-> ([dL/dplane_xy, dL/dplane_xz, dL/dplane_yz] each [1,F,H,W], dL/dx with x's shape), float64"""
    x = np.asarray(x)
    F = planes[0].shape[1]
    go = np.asarray(g_feat, np.float64).reshape(-1, 3 * F)
    d_planes, d_g = [], np.zeros((go.shape[0], 3))
    for p, v, H, W, corners in _cells(planes, x, center, scale):
        gp = go[:, p * F:(p + 1) * F]                               # [n, F]
        acc = np.zeros((H, W, F))
        gix, giy = np.zeros(go.shape[0]), np.zeros(go.shape[0])
        for ok, cx, cy, w, wx, wy in corners:
            np.add.at(acc, (cy[ok], cx[ok]), gp[ok] * w[ok, None])
            s = np.where(ok, (v[:, cy, cx].T * gp).sum(1), 0.0)     # sum over channels of value * dL/dfeat
            gix += np.where(ok, s * wx, 0.0)
            giy += np.where(ok, s * wy, 0.0)
        d_planes.append(np.ascontiguousarray(acc.transpose(2, 0, 1))[None])
        aw, ah = AXES[p]
        d_g[:, aw] += gix * (W - 1) / 2.0
        d_g[:, ah] += giy * (H - 1) / 2.0
    return d_planes, (d_g * 2.0 / float(scale)).reshape(x.shape)
