"""Every HGS_* switch the rasterizer's code reads from the environment is either a variant of the path matrix
(tests/test_gpu_path_matrix.py: tools/shape_scan.py's VARIANTS plus the matrix's EXTRA_VARIANTS) or exempt below, with the reason
and the test that covers it.  A switch added without parity coverage fails here, on a CPU run.  Sources are read as text (ast
for the variant tables): nothing here imports GPU code."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ml-hugs_amd")

# name -> (why it is no rasterizer path of the matrix, the test that covers it)
EXEMPT = {
    "HGS_WAIT_SLEEP": ("host timing of the wait for N, not what the kernels compute",
                       "tests/test_gpu_configs.py::test_the_wait_for_n_survives_sleeps_that_overshoot"),
    "HGS_WAIT_TEST_OVERSLEEP_US": ("injects an overslept wait for N (host timing only)",
                                   "tests/test_gpu_configs.py::test_the_wait_for_n_survives_sleeps_that_overshoot"),
    "HGS_UPSTREAM_SCALE_GRAD": ("changes the answer by design (dL/dscale without the scale modifier); the oracle takes the same switch",
                                "tests/test_gpu_parity.py::test_scale_gradient_convention_switch"),
    "HGS_BINDING": ("which binding calls the library (C++ autograd node or ctypes), the same launches",
                    "tests/test_gpu_parity.py::test_cpp_binding_equals_ctypes_binding"),
    "HGS_BINNING_HINT": ("whether a frame is enqueued on a guess of N; a wrong guess is repaired",
                         "tests/test_gpu_parity.py::test_binning_capacity_guess_never_changes_results"),
    "HGS_RASTERIZER_LIB": ("the path of the library that is loaded (A/B builds), not a path inside it",
                           "tests/test_abi.py::test_library_exports_every_declared_symbol"),
    "HGS_JOINT_CONCAT": ("renderer form: the joint render concatenates as the reference does instead of the second segment",
                         "tests/test_gpu_configs.py::test_c4_joint_human_scene_1080p"),
    "HGS_VIEWSPACE_NONLEAF": ("renderer form: the viewspace tensor as a non-leaf clone",
                              "tests/test_gpu_parity.py::test_fused_visibility_and_viewspace_sink"),
    "HGS_FUSED_VISIBILITY": ("renderer form: the visibility mask from the forward's radii instead of a separate pass",
                             "tests/test_gpu_parity.py::test_fused_visibility_and_viewspace_sink"),
    "HGS_FRAME_CALL": ("renderer form: the frame call against the statement-by-statement adapter",
                       "tests/test_gpu_frame_call.py"),
    "HGS_CONCURRENT_RENDERS": ("renderer form: the two renders of a frame on two streams, the same rasterizer calls",
                               "tests/test_gpu_frame_call.py"),
    "HGS_KNN_GRID": ("k-nearest-neighbour search (grid or whole-cloud scan), not the rasterizer",
                     "tests/test_knn.py::test_hip_dist_cuda2_grid_search_is_bit_exact"),
    "HGS_LOSS_SHARE_PASS": ("the losses' shared pass over the images, not the rasterizer",
                            "tests/test_losses.py::test_shared_pass_is_found_again_only_while_the_caller_holds_the_result"),
    "HGS_SHARDING_FORCE_COLLECTIVES": ("multi-GPU sharding of the training step, not the rasterizer",
                                       "tests/test_gpu_configs.py::test_rccl_branch_of_the_bench_runs_as_a_process_group_of_one"),
}

# a quoted HGS_* name in the library's sources is an environment read: getenv(...) directly or through read_switches_from_env's
# num / on / off helpers (hgs_api.hip)
_C_NAME = re.compile(r'"(HGS_[A-Z0-9_]+)"')
_PY_READ = re.compile(r'(?:environ\.get|getenv|environ\.setdefault)\(\s*["\'](HGS_[A-Z0-9_]+)["\']|environ\[\s*["\'](HGS_[A-Z0-9_]+)["\']\s*\]')


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def read_switch_names():
    """{name: [files that read it]} over the library's HIP sources, the drop-in binding and hugs_amd/"""
    found = {}
    for path in sorted(glob.glob(os.path.join(PKG, "csrc", "*.hip"))):
        for name in _C_NAME.findall(_read(path)):
            found.setdefault(name, []).append(os.path.relpath(path, ROOT))
    py = [os.path.join(PKG, "diff_gaussian_rasterization", "__init__.py")]
    py += sorted(glob.glob(os.path.join(PKG, "hugs_amd", "**", "*.py"), recursive=True))
    for path in py:
        for m in _PY_READ.finditer(_read(path)):
            found.setdefault(m.group(1) or m.group(2), []).append(os.path.relpath(path, ROOT))
    return found


def _dict_literal(path, name):
    for node in ast.walk(ast.parse(_read(path))):
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets):
            return ast.literal_eval(node.value)
    raise AssertionError(f"{name} not found in {path}")


def matrix_switch_names():
    names = set()
    for path, table in ((os.path.join(ROOT, "tools", "shape_scan.py"), "VARIANTS"),
                        (os.path.join(ROOT, "tests", "test_gpu_path_matrix.py"), "EXTRA_VARIANTS")):
        for env, _ckpt in _dict_literal(path, table).values():
            names.update(env)
    return names


def test_the_reader_finds_the_known_switches():
    found = read_switch_names()
    # (one of each way of reading: getenv, the helpers of read_switches_from_env, os.environ.get in the binding and in hugs_amd/)
    for name in ("HGS_BIN_MODE", "HGS_BWD_TWO_LAUNCHES", "HGS_K8_COOP", "HGS_BINDING", "HGS_FRAME_CALL", "HGS_KNN_GRID"):
        assert name in found, name
    assert {"HGS_K8_COOP", "HGS_K1_STAGE_SH", "HGS_BWD_SEGMENTED", "HGS_FRAME_KIND", "HGS_DEEP_MIN"} <= matrix_switch_names()


def test_every_switch_is_in_the_path_matrix_or_exempt():
    found = read_switch_names()
    covered = matrix_switch_names()
    missing = {n: f for n, f in found.items() if n not in covered and n not in EXEMPT}
    assert not missing, ("switches read from the environment that the path matrix (tests/test_gpu_path_matrix.py) does not set and "
                         f"that are not exempt in tests/test_switch_coverage.py: {missing}")


def test_exemptions_are_live_and_name_their_test():
    found = read_switch_names()
    for name, (reason, test) in EXEMPT.items():
        assert name in found, f"{name} is exempt but no longer read"
        assert name not in matrix_switch_names(), f"{name} is exempt and in the matrix"
        assert reason and os.path.exists(os.path.join(ROOT, test.split("::")[0])), (name, test)
        if "::" in test:
            assert re.search(rf"def {re.escape(test.split('::')[1])}\(", _read(os.path.join(ROOT, test.split("::")[0]))), (name, test)
