"""Resource budgets of the backward blend kernels (blend.hip), read from the kernel metadata of a device-only compile with the
Makefile's own flags -- no GPU needed.  The per-(tile, entry) reduction goes through a wave-private LDS region; these are the
limits inside which it keeps eight waves per SIMD (profiles/r4_occupancy_*.txt)."""
import os
import re
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ml-hugs_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# kernel name fragment -> (max VGPRs, max SGPRs); every backward kernel: no spills, no scratch, at most 20 KB of static LDS
BUDGETS = {
    "blend_backward_kernelILi4E": (64, 79),
    "blend_backward_kernelILi1E": (64, 79),
    "blend_backward_segmented_kernel": (64, 79),
    "blend_backward_mixed_kernel": (64, 98),
}
LDS_MAX = 20 * 1024


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^HIPFLAGS\s*:=\s*(.*)$", text, re.M)
    return [f.replace("$(ARCH)", "gfx950") for f in shlex.split(m.group(1)) if f != "-fPIC"]


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("bwd_res") / "blend.s")
    subprocess.check_call([HIPCC if os.path.exists(HIPCC) else "hipcc", *_makefile_flags(), "--cuda-device-only", "-S",
                           os.path.join(CSRC, "blend.hip"), "-o", out], cwd=CSRC)
    meta = open(out).read().split("amdhsa.kernels:", 1)[1]
    found = {}
    for block in re.split(r"\n\s*- \.", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        fields = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
        found[name.group(1)] = fields
    return found


@pytest.mark.parametrize("frag", list(BUDGETS))
def test_backward_kernel_resource_budget(frag, kernels):
    names = [n for n in kernels if frag in n]
    assert len(names) == 1, f"{frag}: {names}"
    k = kernels[names[0]]
    vmax, smax = BUDGETS[frag]
    assert k["vgpr_count"] <= vmax, f"{frag}: {k['vgpr_count']} VGPRs"
    assert k["sgpr_count"] <= smax, f"{frag}: {k['sgpr_count']} SGPRs"
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, f"{frag}: spills"
    assert k["private_segment_fixed_size"] == 0, f"{frag}: scratch"
    assert 0 < k["group_segment_fixed_size"] <= LDS_MAX, f"{frag}: {k['group_segment_fixed_size']} B of LDS"
