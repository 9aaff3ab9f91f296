"""bench.py --dump-outputs DIR: what the timed path computed in its last step, as DIR/<name>.npy, so that two builds can be compared
output for output on the same seeded inputs; and the split between a plain run (the headline figure) and --full (everything else).
CPU: the dump's layout, limit and sample.  GPU: a small workload through both forms, its dump against the oracle."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _frame(P, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"color": r(3, H, W), "radii": torch.randint(0, 40, (P,), generator=g, dtype=torch.int32), "grad_means3D": r(P, 3),
            "grad_shs": r(P, 16, 3)}


def test_dump_writes_every_output_whole_under_the_limit(tmp_path):
    frame = _frame(500, 12, 20, 0)
    shapes = bench.dump_outputs(str(tmp_path), [frame])
    assert shapes == {k: list(v.shape) for k, v in frame.items()}
    for k, v in frame.items():
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, v.float().numpy()), k
    # several frames per step: one file per frame and output
    shapes = bench.dump_outputs(str(tmp_path / "two"), [frame, _frame(500, 12, 20, 1)])
    assert sorted(shapes) == sorted(f"{k}_frame{i}" for k in frame for i in (0, 1))


def test_dump_above_the_limit_keeps_one_fixed_sample_of_rows_and_pixels(tmp_path):
    P, H, W = 3000, 40, 60
    frame = _frame(P, H, W, 2)
    total = sum(v.numel() * 4 for v in frame.values())
    limit = total // 3
    a_dir, b_dir = tmp_path / "a", tmp_path / "b"
    shapes = bench.dump_outputs(str(a_dir), [frame], limit=limit)
    bench.dump_outputs(str(b_dir), [frame], limit=limit)
    assert sum(os.path.getsize(a_dir / f) for f in os.listdir(a_dir)) <= limit
    rows = shapes["grad_means3D"][0]
    assert 0 < rows < P and shapes["radii"] == [rows] and shapes["grad_shs"] == [rows, 16, 3]
    assert shapes["color"][0] == 3 and 0 < shapes["color"][1] < H * W
    for k in frame:   # the same arguments keep the same items
        assert np.array_equal(np.load(a_dir / f"{k}.npy"), np.load(b_dir / f"{k}.npy")), k
    # every per-Gaussian array keeps the same Gaussians, and they are rows of the output as it was
    m = frame["grad_means3D"].numpy()
    kept = np.load(a_dir / "grad_means3D.npy")
    idx = np.array([int(np.flatnonzero((m == row).all(axis=1))[0]) for row in kept])
    assert np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(a_dir / "radii.npy"), frame["radii"].numpy()[idx].astype(np.float32))
    assert np.array_equal(np.load(a_dir / "grad_shs.npy"), frame["grad_shs"].numpy()[idx])
    px = frame["color"].numpy().reshape(3, -1)
    col = np.load(a_dir / "color.npy")
    assert all((px == col[:, j:j + 1]).all(axis=0).any() for j in range(0, col.shape[1], 97))


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr and r.stdout.strip() == ""


def _bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


SMALL = ["--gaussians", "4000", "--height", "128", "--width", "192"]


@pytest.mark.gpu
def test_plain_run_dumps_what_the_oracle_computes(device, tmp_path):
    """A plain run: the headline fields and nothing of --full; its dump is the last step's image, radii and gradients on bench.py's
    seeded inputs, which the oracle recomputes."""
    from hugs_amd import synthetic as syn
    from oracle import hgs_oracle as ho
    from test_gpu_parity import GRAD_REL_TOL, check_image, rel_l2
    out = _bench(SMALL + ["--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path)])
    assert out["steps"] == 7 and out["full"] is False and out["ranks_seen"] == 1
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in out, k
    assert out["value"] > 0 and abs(out["ms_per_step"] * out["value"] / 1e3 - 1.0) < 0.01
    for k in ("cpu_baseline", "stages_ms", "box", "two_frames_in_flight", "ranks_host"):
        assert k not in out, k

    P, H, W = 4000, 128, 192
    cam = syn.pinhole_camera(H, W)
    g = syn.scene_gaussians(P, cam, seed=0, sigma_px=4.0)
    inp = ho.Inputs(g["means3D"], g["opacities"], cam["world_view_transform"], cam["full_proj_transform"], cam["camera_center"],
                    math.tan(cam["fovx"] * 0.5), math.tan(cam["fovy"] * 0.5), H, W, np.ones(3, np.float32), shs=g["shs"],
                    scales=g["scales"], rotations=g["rotations"], sh_degree=3)
    ref = ho.forward(inp)
    refg = ho.backward(inp, ref, syn.pixel_grad(H, W))
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == sorted(["color", "radii"] + ["grad_" + k for k in ("means3D", "opacities", "shs", "scales", "rotations", "means2D")])
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["radii"], ref["radii"].astype(np.float32))
    check_image(got["color"], ref["color"], "dumped colour")
    for k in ("means3D", "opacities", "shs", "scales", "rotations", "means2D"):
        assert rel_l2(got["grad_" + k].reshape(refg[k].shape), refg[k]) <= GRAD_REL_TOL, k


@pytest.mark.gpu
def test_full_run_keeps_everything_else(device):
    out = _bench(SMALL + ["--steps", "5", "--warmup", "2", "--full", "--cpu-seconds", "1"])
    assert out["full"] is True and out["steps"] == 5
    for k in ("cpu_baseline", "stages_ms", "box", "two_frames_in_flight", "ranks_host", "memory", "whole_frame", "stage_rooflines"):
        assert k in out, k
    assert out["roofline"]["peak_measured"] > 0 and out["stages_ms"] and out["cpu_baseline"]["value"] > 0
