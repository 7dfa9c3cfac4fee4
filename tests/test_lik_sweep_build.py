"""The likelihood-only set kernels (lower-triangle sweep) are built in translation units of their own and issue fewer DPP
instructions than the Gauss-Jordan kernels of the same row length."""
import os
import re
import subprocess
import tempfile

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"


def _newbcast_per_kernel(obj):
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "x.fat"), os.path.join(td, "x.co")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
    out = {}
    for blk in re.split(r"\n(?=[0-9a-f]+ <)", dis):
        head = blk.split("\n", 1)[0]
        if "gpv_sets_kernel" in head:
            out[head.split("<")[1].split(">")[0]] = blk.count("row_newbcast")
    return out


def test_lik_kernels_built_apart_and_shorter():
    from gpvecchia_amd import build as B
    lik, gj = (os.path.join(B.CSRC, "build", f) for f in ("sets_p31_lik.o", "sets_p31.o"))
    if not (os.path.exists(lik) and os.path.exists(gj)):
        pytest.skip("no object files in this tree (library built elsewhere)")
    k_lik, k_gj = _newbcast_per_kernel(lik), _newbcast_per_kernel(gj)
    # Matern 1.5, two dimensions: the flagship instantiation.  Itanium mangling: <31, 2, 1, true> / <31, 2, 1, false>
    name = "_ZN3gpv15gpv_sets_kernelILi31ELi2ELi1ELb{}EEEvNS_7SetArgsE"
    assert set(k_lik) and all(k.endswith("Lb1EEEvNS_7SetArgsE") for k in k_lik)       # only likelihood-only kernels there
    assert not any(k.endswith("Lb1EEEvNS_7SetArgsE") for k in k_gj)                   # and none in the main unit
    assert len(k_lik) == 20                                       # 5 covariance families x 4 dimension variants
    # P = 31 sweep: 585 FMAs (slot 0: 120, slot 1 with the data row: 465) against Gauss-Jordan's 825 + 14
    assert k_gj[name.format(0)] - k_lik[name.format(1)] == 254
    assert all(k_lik[k] < k_gj[k.replace("Lb1E", "Lb0E")] for k in k_lik)
    assert all(not B.lik_p(p) or os.path.exists(os.path.join(B.CSRC, "build", f"sets_p{p}_lik.o")) for p in B.plist())
