"""CPU: what row f-12 (the densification round, csrc/densify.hip) can be held to without a GPU.

* The fixtures the GPU test compares on are decidable: tests/densify_ref.py's restatement selects, splits and prunes the same rows in
  float32 and in float64 on every one of them.  That is what lets tests/test_gpu_densify_round.py demand exact row lists.
* The restatement's explicit noise is the reference's own draw: normal(0, 1) scaled by std (on the CPU generator; the GPU test repeats
  it on the device's).
* The entry points reject bad sizes, pointers, counts and modes on the host, through hgs_last_error(), before any launch.
* hgs_densify_tensor, the one record the header declares for this row, is laid out as hugs_amd/densify.py packs it.
"""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import densify_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import diff_gaussian_rasterization as dgr
    return dgr._load()


def _limits():
    from hugs_amd.densify import densify_limits
    return densify_limits()


def test_the_limits_query_returns_positive_values():
    rows, tensors = _limits()
    assert rows > 0 and tensors > 0
    # a scene round is 6 parameters x 3 + 3 statistics = 21 records: one launch
    assert tensors >= 21


def test_the_fixtures_select_the_same_rows_in_fp32_and_fp64():
    rows, _ = _limits()
    seen = set()
    for case in ref.cases(rows):
        fx = ref.make_fixture(**case)
        noise = torch.randn(2 * fx["n"], 3, generator=torch.Generator().manual_seed(1))
        a, b = ref.run_ref(fx, torch.float32, noise), ref.run_ref(fx, torch.float64, noise.double())
        assert set(a["masks"]) == set(b["masks"])
        for k in a["masks"]:
            assert torch.equal(a["masks"][k], b["masks"][k]), (case, k)
        assert a["params"]["xyz"].shape == b["params"]["xyz"].shape
        if case["pattern"] == "pruned":
            assert a["params"]["xyz"].shape[0] == 0, case
        if case["pattern"] == "mix" and fx["n"] >= rows - 1 and not case.get("skip_branch"):
            m = a["masks"]
            seen |= {("clone", bool(m["clone"].any())), ("split", bool(m["split"].any())), ("prune", bool(m["prune"].any())),
                     ("stay", bool((~m["prune"]).any()))}
    assert seen == {("clone", True), ("split", True), ("prune", True), ("stay", True)}


@pytest.mark.parametrize("flavour", (ref.SCENE, ref.HUMAN))
def test_the_mix_holds_every_kind_in_every_workgroup(flavour):
    rows, _ = _limits()
    fx = ref.make_fixture(flavour, 2 * rows + 17, "mix")
    for start in range(0, fx["n"], rows):
        assert set(fx["kinds"][start:start + rows].tolist()) == set(ref._MIX), start


def test_fixture_nudging_is_what_keeps_the_rows_decidable():
    """Rows start out within 3e-5 of a threshold; check_fixture() would refuse them as generated."""
    fx = ref.make_fixture(ref.SCENE, 200, "mix")
    bad = dict(fx)
    bad["accum"] = fx["accum"].copy()
    bad["accum"][0, 0] = np.float32(ref.MAX_GRAD * (1 + 2e-5)) * fx["denom"][0, 0]
    with pytest.raises(AssertionError, match="max_grad"):
        ref.check_fixture(bad)


def test_explicit_noise_is_the_references_draw_on_the_cpu_generator():
    """torch.normal(mean=zeros, std=stds) consumes a generator as randn of the same shape does and scales by std."""
    fx = ref.make_fixture(ref.HUMAN, 300, "mix")
    g1, g2 = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    a = ref.run_ref(fx, torch.float32, noise=None, generator=g1)
    b = ref.run_ref(fx, torch.float32, noise=lambda count: torch.randn((2 * count, 3), generator=g2))
    assert torch.equal(a["params"]["xyz"], b["params"]["xyz"]) and a["masks"]["split"].any()
    assert torch.equal(g1.get_state(), g2.get_state())


def test_validation_errors_come_back_through_last_error():
    lib = _lib()
    rows, tensors = _limits()
    err = lambda: lib.hgs_last_error()
    A = 4096                                   # a non-null, 16-byte aligned address that is never dereferenced: every call returns before a launch
    plan = lambda flavour, n, ptr, totals=A: lib.hgs_densify_plan(flavour, n, 1, ptr, ptr, ptr, ptr, ptr, 1e-4, 5e-3, 0.04, 1, 20.0, 0.4, ptr, ptr, totals, None)
    assert plan(0, -1, A) == -1 and b"densify_plan: n < 0" in err()
    assert plan(0, 5, None) == -1 and b"null pointer" in err()
    assert plan(7, 5, A) == -1 and b"unknown flavour" in err()
    assert plan(1, 0, None, None) == -1 and b"null `totals`" in err()
    assert lib.hgs_densify_plan(0, 5, 1, A, A, A, A, A, 1e-4, 5e-3, 0.04, 1, 20.0, 0.4, A, A + 4, A, None) == -1 and b"16-byte aligned" in err()

    from hugs_amd import densify as D
    rec = lambda src, dst, width, mode: D._RECORD.pack(src, dst, width, mode)
    scatter = lambda n, recs, count=None, kind=A, aux=A, flavour=0: lib.hgs_densify_scatter(
        flavour, n, kind, A, A, b"".join(recs) if recs else None, len(recs) if count is None else count, aux, aux, aux, None)
    assert scatter(-1, [rec(A, A, 3, D.COPY)]) == -1 and b"n < 0" in err()
    assert scatter(5, [rec(A, A, 3, D.COPY)], kind=None) == -1 and b"null pointer (kind, partials or totals)" in err()
    assert scatter(5, [rec(A, A, 3, D.COPY)], count=16 * tensors + 1) == -1 and b"more tensors" in err()
    assert scatter(5, [rec(A, A, 3, D.COPY)], count=-1) == -1 and b"count < 0" in err()
    assert scatter(5, [], count=2) == -1 and b"null `tensors`" in err()
    assert scatter(5, [rec(A, A, 3, D.COPY), rec(A, A, 3, 6)]) == -1 and b"unknown mode" in err()
    assert scatter(5, [rec(A, A, 3, -1)]) == -1 and b"unknown mode" in err()
    assert scatter(5, [rec(0, A, 3, D.COPY)]) == -1 and b"null pointer (src or dst)" in err()
    assert scatter(5, [rec(A, 0, 3, D.ZERO)]) == -1 and b"null pointer (src or dst)" in err()
    assert scatter(5, [rec(A, A, 4, D.XYZ_SPLIT)]) == -1 and b"width 3" in err()
    assert scatter(5, [rec(A, A, 3, D.XYZ_SPLIT)], aux=None) == -1 and b"scales, rotation and noise" in err()
    assert scatter(5, [rec(A, A, 1025, D.COPY)]) == -1 and b"width" in err()
    assert scatter(5, [rec(A, A + 2, 3, D.COPY)]) == -1 and b"4-byte aligned" in err()
    assert scatter(5, [rec(A, A, 3, D.COPY)], flavour=2) == -1 and b"unknown flavour" in err()
    # nothing to do is not an error, and launches nothing: no rows, or only records of width 0 (f_rest at SH degree 0) -- even with null data
    assert scatter(0, [rec(0, 0, 3, D.COPY)], kind=None) == 0
    assert scatter(5, [rec(0, 0, 0, D.COPY)]) == 0


def test_the_python_wrappers_validate_before_anything_runs():
    from hugs_amd import densify as D
    fx = ref.make_fixture(ref.SCENE, 8, "mix")
    inst = ref.instantiate(fx, torch.float32, "cpu")
    args = dict(fx["args"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.densify_and_prune_scene(inst["params"], inst["optimizer"], inst["stats"], **args)
    with pytest.raises(RuntimeError, match="params must hold exactly"):
        D.densify_and_prune_scene({"xyz": inst["params"]["xyz"]}, inst["optimizer"], inst["stats"], **args)
    fxh = ref.make_fixture(ref.HUMAN, 8, "mix")
    insth = ref.instantiate(fxh, torch.float32, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.densify_and_prune_human(insth["params"]["xyz"], insth["scaling_multiplier"], insth["human_gs_out"], insth["optimizer"], insth["stats"], **fxh["args"])
    with pytest.raises(RuntimeError, match="must contain 'xyz'"):
        D.densify_and_prune_human(insth["params"]["xyz"], insth["scaling_multiplier"], insth["human_gs_out"], insth["optimizer"], insth["stats"],
                                  densify_group_names=("v_embed",), **fxh["args"])


def test_the_record_is_laid_out_as_the_wrapper_packs_it():
    """hgs_densify_tensor against the C compiler, the way test_abi.py holds the mirrored structs: size, and offset and size per field."""
    from hugs_amd import densify as D

    class Record(C.Structure):
        _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("width", C.c_int32), ("mode", C.c_int32)]

    lines, want = ['printf("%zu\\n", sizeof(hgs_densify_tensor));'], [C.sizeof(Record)]
    for field, _ in Record._fields_:
        lines.append(f'printf("%zu %zu\\n", offsetof(hgs_densify_tensor, {field}), sizeof(((hgs_densify_tensor *)0)->{field}));')
        want += [getattr(Record, field).offset, getattr(Record, field).size]
    names = ("HGS_DENSIFY_SCENE", "HGS_DENSIFY_HUMAN", "HGS_DENSIFY_COPY", "HGS_DENSIFY_MOMENT", "HGS_DENSIFY_ZERO", "HGS_DENSIFY_XYZ_SPLIT",
             "HGS_DENSIFY_LOG_SCALE_SPLIT", "HGS_DENSIFY_DIV_SPLIT")
    lines += [f'printf("%d\\n", (int){name});' for name in names]
    want += [D.SCENE, D.HUMAN, D.COPY, D.MOMENT, D.ZERO, D.XYZ_SPLIT, D.LOG_SCALE_SPLIT, D.DIV_SPLIT]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "hgs_rasterizer.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "t")]).decode().split()))
    assert got == want
    assert D._RECORD.size == C.sizeof(Record) == 24
    packed = D._RECORD.pack(0x1122334455667788, 0x0102030405060708, 45, D.MOMENT)
    r = Record.from_buffer_copy(packed)
    assert (r.src, r.dst, r.width, r.mode) == (0x1122334455667788, 0x0102030405060708, 45, D.MOMENT)
    assert struct.calcsize("@PPii") == 24
