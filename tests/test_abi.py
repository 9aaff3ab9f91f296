"""CPU: the C-ABI library loads, exports every function include/hgs_rasterizer.h declares, its ctypes mirror -- one table of
prototypes and eight structs -- agrees with the header line by line and with the C compiler's layout field by field, and host-side
validation errors come back through hgs_last_error().
No compute call is made (there is no GPU here)."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hgs_rasterizer.h")


def _declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(hgs_[a-z_0-9]+)\s*\(", src)) - {"hgs_alloc_fn"})


def test_library_exports_every_declared_symbol():
    import diff_gaussian_rasterization as dgr
    lib = dgr._load()
    names = _declared_functions()
    assert {"hgs_rasterize_forward", "hgs_rasterize_backward", "hgs_mark_visible", "hgs_last_error"} <= set(names)
    for n in names:
        assert hasattr(lib, n), f"{n} is declared in the header but not exported"
    header_version = int(re.search(r"#define HGS_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    assert lib.hgs_abi_version() == header_version == dgr._ABI_VERSION


def _declarations():
    """{name: (return type, [parameter, ...])} of every function the header declares, as text: comments stripped, `type name(params);`."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"^\s*((?:const\s+)?\w+\s*\*?)\s*\b(hgs_\w+)\s*\(([^()]*)\)\s*;", src, flags=re.M):
        assert name not in out, f"{name} is declared twice"
        params = " ".join(params.split())
        out[name] = (" ".join(ret.split()), [] if params == "void" else [p.strip() for p in params.split(",")])
    return out


_SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "size_t": C.c_size_t, "float": C.c_float}


def _check_parameter(decl, got, abi):
    """The rule of diff_gaussian_rasterization/_abi.py for one parameter: `decl` is the header's text, `got` the table's ctypes type."""
    words = [w for w in re.sub(r"[\*\[\]]", " ", decl).split() if w != "const"]
    base = words[0]
    if "*" not in decl and "[" not in decl:
        return got is (abi._ALLOC_FN if base == "hgs_alloc_fn" else _SCALARS[base])
    if base in abi.STRUCTS:
        return got is C.POINTER(abi.STRUCTS[base])
    return got in (C.c_void_p, C.c_char_p) or (isinstance(got, type) and issubclass(got, C._Pointer))


def test_the_prototype_table_matches_the_header():
    """Every line of PROTOTYPES against the declaration it mirrors: the same functions, return type, parameter count, and per position
    the table's rule (scalars exact, pointers to mirrored structs typed, any other pointer or array some pointer type).  Needs no library."""
    from diff_gaussian_rasterization import _abi
    decls = _declarations()
    assert len(decls) == len(_declared_functions()), sorted(set(_declared_functions()) - set(decls))   # a declaration the parser cannot read
    assert set(decls) == set(_abi.PROTOTYPES), set(decls) ^ set(_abi.PROTOTYPES)
    returns = dict(_SCALARS, **{"void": None, "const char *": C.c_char_p})
    for name, (ret, params) in decls.items():
        restype, argtypes = _abi.PROTOTYPES[name]
        assert restype is returns[ret], f"{name}: returns {ret}, the table says {restype}"
        assert len(argtypes) == len(params), f"{name}: {len(params)} parameters, the table has {len(argtypes)}"
        for k, (decl, got) in enumerate(zip(params, argtypes)):
            assert _check_parameter(decl, got, _abi), f"{name}: parameter {k} is `{decl}`, the table says {got}"


def test_ctypes_structs_match_the_c_layout():
    """Every field of every mirrored struct: size of the struct, offset and size of the field, as the C compiler lays the header out."""
    from diff_gaussian_rasterization import _abi
    lines, want = [], []
    for cname, mirror in _abi.STRUCTS.items():
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(C.sizeof(mirror))
        for field, _ in mirror._fields_:
            lines.append(f'printf("%zu %zu\\n", offsetof({cname}, {field}), sizeof((({cname} *)0)->{field}));')
            want += [getattr(mirror, field).offset, getattr(mirror, field).size]
    assert len(_abi.STRUCTS) == 8
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "hgs_rasterizer.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = subprocess.check_output([os.path.join(d, "t")]).decode().split()
    got = list(map(int, out))
    names = [f"sizeof({c})" if f is None else f"{c}.{f} {what}" for c, m in _abi.STRUCTS.items()
             for f, what in [(None, None)] + [(f, w) for f, _ in m._fields_ for w in ("offset", "size")]]
    assert got == want, [(n, g, w) for n, g, w in zip(names, got, want) if g != w]
    # hgs_alloc_fn: void *(*)(void *ctx, int buffer_id, size_t bytes)
    assert _abi._ALLOC_FN._restype_ is C.c_void_p and _abi._ALLOC_FN._argtypes_ == (C.c_void_p, C.c_int, C.c_size_t)


def test_prototypes_are_declared_in_the_table_only():
    """No drift back: under ml-hugs_amd/, tests/ and tools/ nothing but the table module assigns a prototype of a function the header
    declares (symbols of A/B and trace builds that the header does not declare are bound where they are used)."""
    declared = set(_declared_functions())
    assign = re.compile(r"(\w+)\s*\.\s*(?:argtypes|restype)\s*=[^=]")
    found = []
    for top in ("ml-hugs_amd", "tests", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                path = os.path.join(dirpath, f)
                if not f.endswith(".py") or path.endswith(os.path.join("diff_gaussian_rasterization", "_abi.py")):
                    continue
                for k, line in enumerate(open(path).read().splitlines(), 1):
                    for name in assign.findall(line):
                        if name in declared or not name.startswith("hgs_"):   # (a variable may stand for any function)
                            found.append(f"{os.path.relpath(path, ROOT)}:{k}: {name}")
    assert not found, found


def test_scratch_size_queries_and_offsets():
    import diff_gaussian_rasterization as dgr
    lib = dgr._load()
    assert lib.hgs_geom_bytes(1000, 1080, 1920) >= 1000 * (64 + 4) + 4 * 8160
    assert lib.hgs_image_bytes(1080, 1920) >= 1080 * 1920 * 8 + 8160 * 8
    n = 123456
    assert lib.hgs_binning_bytes(n, 1080, 1920) >= n * 24
    off = {k: lib.hgs_scratch_offset(k.encode(), 1000, n, 64, 64) for k in
           ("splats", "tiles_touched", "list", "final_T", "n_contrib", "ranges")}
    assert off["splats"] == 0 and off["final_T"] == 0
    assert off["list"] >= 8 * n
    assert lib.hgs_scratch_offset(b"nope", 1, 1, 16, 16) == C.c_size_t(-1).value
    assert [lib.hgs_stage_name(i).decode() for i in range(7)] == list(dgr.STAGES)


def test_argument_validation_reports_through_last_error():
    import diff_gaussian_rasterization as dgr
    lib = dgr._load()
    a, st = dgr._ForwardArgs(), dgr._ForwardState()
    a.P = 5
    a.s.image_height, a.s.image_width = 0, 16
    cb = dgr._ALLOC_FN(lambda ctx, which, n: None)
    assert lib.hgs_rasterize_forward(C.byref(a), cb, None, C.byref(st), None) == -1
    assert b"image size" in lib.hgs_last_error()
    a.s.image_height = 16
    assert lib.hgs_rasterize_forward(C.byref(a), cb, None, C.byref(st), None) == -1
    assert b"means3D must have dimensions (num_points, 3)" in lib.hgs_last_error()
    assert lib.hgs_mark_visible(3, None, None, None, None) == -1


def test_product_path_has_no_cpu_fallback_and_never_touches_the_oracle():
    """CPU tensors must raise; and nothing under ml-hugs_amd/ may import or link the oracle."""
    import torch
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    s = GaussianRasterizationSettings(16, 16, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                                      False, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GaussianRasterizer(s)(means3D=torch.zeros(2, 3), means2D=torch.zeros(2, 3), opacities=torch.ones(2, 1),
                              shs=torch.zeros(2, 16, 3), scales=torch.ones(2, 3), rotations=torch.ones(2, 4))
    pkg = os.path.join(ROOT, "ml-hugs_amd")
    for dirpath, _, files in os.walk(pkg):
        if os.sep + "build" in dirpath or os.sep + "lib" in dirpath:
            continue
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", "Makefile")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.lower().replace("the oracle", "").replace("cpu oracle", "") or \
                    not re.search(r"^\s*(from|import)\s+oracle|hgs_oracle|#include.*oracle", txt, re.M), os.path.join(dirpath, f)


def test_widening_rows_have_no_cpu_fallback_either():
    """l1_loss / ssim, SceneGS.forward and the rotation conversions (rows f-5..f-7): CPU tensors raise, nothing is computed."""
    import torch
    from hugs_amd import losses, rotations, scene_forward
    a = torch.rand(3, 12, 12)
    for call in (lambda: losses.ssim(a, a.clone()), lambda: losses.l1_loss(a, a.clone()), lambda: losses.l1_ssim(a, a.clone()),
                 lambda: rotations.matrix_to_quaternion(torch.eye(3)[None]), lambda: rotations.rotation_6d_to_matrix(torch.rand(4, 6)),
                 lambda: scene_forward.scene_activations(torch.zeros(2, 3), torch.ones(2, 4), torch.zeros(2, 1), torch.zeros(2, 1, 3),
                                                         torch.zeros(2, 15, 3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_widening_rows_reject_bad_arguments_through_the_c_abi():
    """The entry points' own checks (they return before any launch): sizes, null pointers, alignment."""
    import diff_gaussian_rasterization as dgr
    lib = dgr._load()
    assert lib.hgs_ssim_l1_workspace(3, 1080, 1920) == 8 * 3 * 30 * 68 and lib.hgs_ssim_l1_workspace(0, 4, 4) == 0
    assert lib.hgs_ssim_l1_forward(3, 0, 8, None, None, None, None, None, None) == -1 and b"ssim_l1_forward" in lib.hgs_last_error()
    assert lib.hgs_ssim_l1_forward(3, 8, 8, None, None, None, None, None, None) == -1 and b"null pointer" in lib.hgs_last_error()
    assert lib.hgs_ssim_l1_backward(3, 8, 8, 16, 16, None, 16, None, 16, None) == -1 and b"needs forward's maps" in lib.hgs_last_error()
    assert lib.hgs_scene_forward(4, 0, *([None] * 10)) == -1 and lib.hgs_scene_forward(0, 16, *([None] * 10)) == 0
    assert lib.hgs_scene_forward(4, 16, 16, 20, 16, 16, 16, 16, 16, 16, 16, None) == -1 and b"16-byte aligned" in lib.hgs_last_error()
    assert lib.hgs_matrix_to_quaternion(-1, None, None, None) == -1 and lib.hgs_matrix_to_quaternion(0, None, None, None) == 0
    assert lib.hgs_matrix_to_quaternion(5, 16, 20, None) == -1
    assert lib.hgs_knn_workspace(110_210, 6890) > 0 and lib.hgs_knn_workspace(1000, 6890) == 0 and lib.hgs_knn_workspace(10_000, 100) == 0


def test_the_path_selection_tables_are_generated_from_the_sources():
    """include/hgs_rasterizer.h and INTEGRATION.md carry ONE table of the library's thresholds, generated from the constants in
    csrc/hgs_common.h and csrc/binning.hip (tools/gen_thresholds.py): a constant changed without regenerating fails here."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "gen_thresholds.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
