"""Reference for the rasterizer's alpha and depth maps, from the C oracle as it stands (no oracle change).

The maps are a colour render whose colours are (z, 1, 0) on a black background: channel 0 is sum_i w_i z_i (the depth map), channel 1
sum_i w_i (the alpha map), over the same lists and contributors as the colour render of the same geometry.  z is the view-space depth
the oracle's preprocess stage computes.  The oracle's backward with dL = (gD, gA, 0) then gives every geometry gradient of the maps but
one term: z itself depends on means3D, z = x V[2] + y V[6] + z V[10] + V[14] (row-vector view matrix), so dL/dmeans3D gains
dL/dcolour[:, 0] * (V[2], V[6], V[10]).
"""
import numpy as np

from oracle import hgs_oracle as ho
from scenes import oracle_inputs

GEOMETRY_KEYS = ("means3D", "means2D", "opacities", "scales", "rotations", "cov3D")


def map_upstreams(H, W, seed=77):
    """(gA, gD): seeded upstream gradients of the alpha and the depth map, [H, W] float32 each"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((H, W)).astype(np.float32), rng.standard_normal((H, W)).astype(np.float32)


def smooth_map_upstreams(H, W):
    """(gA, gD): two low-frequency sinusoids in pixel coordinates, values in 0.1 .. 1.0, of different phase, [H, W] float32 each.
    Under the noise of map_upstreams a gradient's sum can nearly cancel, and the few pixels that take the other side of a threshold
    in another precision then weigh in at 1e-3 of it (tests/test_gpu_maps_paths.py measures both); under these it does not."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    wave = lambda fx, fy, phase: 0.55 + 0.45 * np.sin(2.0 * np.pi * (fx * x / W + fy * y / H) + phase)
    return wave(1.5, 1.0, 0.3).astype(np.float32), wave(1.0, 2.0, 1.9).astype(np.float32)


def maps_reference(sc, gA=None, gD=None, dtype=np.float32):
    """The oracle's maps of scene `sc` (tests/scenes.make_scene) and, given upstream gradients, their gradients.
    Returns dict(alpha [H,W], depth [H,W], z [P], z_max, fwd (the oracle's forward of the (z, 1, 0) render), grads or None)."""
    inp = oracle_inputs(sc, dtype)
    z = ho.forward(inp, stop_after="preprocess")["depths"].astype(dtype)
    cols = np.stack([z, np.ones_like(z), np.zeros_like(z)], 1)
    sc2 = dict(sc, shs=None, colors_precomp=cols, bg=np.zeros(3, np.float32))
    inp2 = oracle_inputs(sc2, dtype)
    f2 = ho.forward(inp2)
    vis = f2["radii"] > 0
    out = dict(alpha=f2["color"][1], depth=f2["color"][0], z=z, z_max=float(z[vis].max()) if vis.any() else 1.0, fwd=f2, grads=None)
    if gA is not None:
        g = ho.backward(inp2, f2, np.stack([gD, gA, np.zeros_like(gA)]))
        V = np.asarray(sc["cam"]["world_view_transform"], np.float64).reshape(4, 4)
        g["means3D"] = g["means3D"] + g["colors"][:, 0:1] * V[:3, 2].astype(dtype)
        out["grads"] = {k: g[k] for k in GEOMETRY_KEYS}
    return out


def colour_reference(sc, dL, dtype=np.float32):
    """The oracle's colour render of `sc` and its gradients for the upstream image gradient dL [3,H,W]."""
    inp = oracle_inputs(sc, dtype)
    f = ho.forward(inp)
    return f, ho.backward(inp, f, dL)


def summed(maps_grads, colour_grads):
    """Gradients of a loss on colour, alpha and depth together: the geometry gradients add, the colour inputs' are the colour render's."""
    g = dict(colour_grads)
    for k in GEOMETRY_KEYS:
        g[k] = colour_grads[k] + maps_grads[k]
    return g
