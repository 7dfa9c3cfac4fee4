"""The lean likelihood-only kernels (gpv_sets_kernel<P, D, COV | 16, true>, built into sets_p{21,26,31}_lean.o) share the
SIMD with a second wavefront like the kernels they stand in for: each must fit 256 VGPRs without AGPRs, scratch or spilled
VGPRs, and the DPP reads of their sweeps, whose neighbourhood changed (no EXEC-masked move behind the reciprocal any more),
must keep their two wait states."""
import os
import re
import subprocess
import tempfile

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"


def _resources(obj):
    """{mangled kernel name: (VGPRs, AGPRs, scratch bytes, spilled VGPRs)} of the gfx950 code object inside obj"""
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "x.fat"), os.path.join(td, "x.co")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
    out = {}
    for m in re.finditer(r"\.agpr_count:\s+(\d+)[\s\S]*?\.name:\s+(\S+)[\s\S]*?\.private_segment_fixed_size:\s+(\d+)"
                         r"[\s\S]*?\.vgpr_count:\s+(\d+)\s+\.vgpr_spill_count:\s+(\d+)", notes):
        out[m.group(2)] = (int(m.group(4)), int(m.group(1)), int(m.group(3)), int(m.group(5)))
    return out


@pytest.mark.parametrize("P", [21, 26, 31])
def test_lean_kernels_fit_their_registers_and_keep_the_dpp_wait_states(P):
    if not all(os.path.exists(f"{LLVM}/{t}") for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")):
        pytest.skip("no ROCm llvm tools on this machine")
    from gpvecchia_amd import build as B
    obj = os.path.join(B.CSRC, "build", f"sets_p{P}_lean.o")
    if not os.path.exists(obj):
        pytest.skip("no object files in this tree (library built elsewhere)")
    res = _resources(obj)
    # Itanium mangling: gpv_sets_kernel<P, D, COV | 16, true>, COV = 0, 1, 2
    lean = {k: v for k, v in res.items() if re.search(r"gpv_sets_kernelILi%dELi[123]ELi1[678]ELb1EEEv" % P, k)}
    assert len(lean) == 9                                     # 3 dimensions x Matern 0.5 / 1.5 / 2.5
    assert len([k for k in res if "gpv_sets_kernel" in k]) == 9      # and nothing else: no general nu, esqe, run-time dimension
    for k, (vgpr, agpr, scratch, vspill) in lean.items():
        assert vgpr <= 256 and agpr == 0, (k, vgpr, agpr)
        assert scratch == 0 and vspill == 0, (k, scratch, vspill)
    ndpp, bad = B.dpp_hazards(obj)
    assert ndpp and bad == 0
