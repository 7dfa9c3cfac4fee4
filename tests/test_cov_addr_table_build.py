"""The likelihood-only set kernels keep the covariance rounds' staging addresses in registers across the task loop
(k_cov_addr_table in gpv_sets_kernel.hpp).  That only pays while the registers exist: every kernel of the built
sets_p{21,26,31}_lik.o units that carries the table must fit 256 VGPRs (two wavefronts per SIMD) without scratch, and the
DPP reads of their sweeps must keep their two wait states."""
import os
import re
import subprocess
import tempfile

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
COV_MATERN_GEN = 5         # general nu: the table up to m + 1 = 21 only; its out-of-line exact pass is a call with a stack frame


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
def test_lik_kernels_with_the_table_fit_their_registers(P):
    from gpvecchia_amd import build as B
    obj = os.path.join(B.CSRC, "build", f"sets_p{P}_lik.o")
    if not os.path.exists(obj):
        pytest.skip("no object files in this tree (library built elsewhere)")
    res = _resources(obj)
    # Itanium mangling: gpv_sets_kernel<P, D, COV, true>
    fixed = {k: (int(mm.group(2)), v) for k, v in res.items()
             if (mm := re.search(r"gpv_sets_kernelILi%dELi(\d)ELi(\d)ELb1E" % P, k)) and mm.group(1) != "0"}
    assert len(fixed) == 15                                   # 3 fixed dimensions x 5 covariance families
    for k, (cov, (vgpr, agpr, scratch, vspill)) in fixed.items():
        assert vgpr <= 256 and agpr == 0, (k, vgpr, agpr)
        if cov != COV_MATERN_GEN:                             # closed forms: the table everywhere
            assert scratch == 0 and vspill == 0, (k, scratch, vspill)
        elif P <= 21:                                         # general nu with the table: no register spilled for it
            assert vspill == 0, (k, vspill)
    ndpp, bad = B.dpp_hazards(obj)
    assert ndpp and bad == 0
