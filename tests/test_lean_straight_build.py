"""The lean likelihood-only kernels (sets_p{21,26,31}_lean.o) keep per-wavefront tables of staging addresses in registers
through the task loop.  The tables must not cost what they save: every instantiation still fits 256 VGPRs without AGPRs or
scratch, spills no SGPR (a spilled SGPR travels through v_writelane / v_readlane, VALU issue slots of a kernel bound by
them), has no v_readlane / v_writelane at all -- so none inside the task loop --, keeps the two wait states in front of
every DPP read, and issues exactly the sweep's DPP instructions it issued before."""
import os
import re
import subprocess
import tempfile

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
# row_newbcast per kernel: the lower-triangle sweep's DPP FMAs, one broadcast per pivot, v and -mu_k (P = 31: 585 + 30 + 2)
NEWBCAST = {21: 352, 26: 472, 31: 617}


def _code_object(obj):
    """(disassembly, notes) of the gfx950 code object inside obj"""
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "x.fat"), os.path.join(td, "x.co")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
    return dis, notes


@pytest.mark.parametrize("P", [21, 26, 31])
def test_lean_kernels_keep_their_tables_in_registers(P):
    if not all(os.path.exists(f"{LLVM}/{t}") for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")):
        pytest.skip("no ROCm llvm tools on this machine")
    from gpvecchia_amd import build as B
    obj = os.path.join(B.CSRC, "build", f"sets_p{P}_lean.o")
    if not os.path.exists(obj):
        pytest.skip("no object files in this tree (library built elsewhere)")
    dis, notes = _code_object(obj)
    res = {}
    for m in re.finditer(r"\.agpr_count:\s+(\d+)[\s\S]*?\.name:\s+(\S+)[\s\S]*?\.private_segment_fixed_size:\s+(\d+)"
                         r"[\s\S]*?\.sgpr_spill_count:\s+(\d+)[\s\S]*?\.vgpr_count:\s+(\d+)\s+\.vgpr_spill_count:\s+(\d+)", notes):
        res[m.group(2)] = dict(agpr=int(m.group(1)), scratch=int(m.group(3)), sspill=int(m.group(4)), vgpr=int(m.group(5)),
                               vspill=int(m.group(6)))
    # Itanium mangling: gpv_sets_kernel<P, D, COV | 16, true>, COV = 0, 1, 2
    lean = {k: v for k, v in res.items() if re.search(r"gpv_sets_kernelILi%dELi[123]ELi1[678]ELb1EEEv" % P, k)}
    assert len(lean) == 9                                     # 3 dimensions x Matern 0.5 / 1.5 / 2.5
    for k, r in lean.items():
        assert r["vgpr"] <= 256 and r["agpr"] == 0, (k, r)
        assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, (k, r)
    seen = 0
    for blk in re.split(r"\n(?=[0-9a-f]+ <)", dis):
        head = blk.split("\n", 1)[0]
        if "gpv_sets_kernel" not in head:
            continue
        seen += 1
        ops = [l.split("//")[0].split() for l in blk.split("\n")[1:]]
        ops = [t[0] for t in ops if t and not t[0].endswith(":")]
        assert not [o for o in ops if o.startswith(("v_readlane", "v_writelane"))], head
        assert blk.count("row_newbcast") == NEWBCAST[P], (head, blk.count("row_newbcast"))
        # the verdict: one v_or3_b32 per two pivots in each sweep of the kernel, and a v_or_b32 for an odd pivot out
        assert ops.count("v_or3_b32") >= (P - 1) // 2, (head, ops.count("v_or3_b32"))
    assert seen == 9
    ndpp, bad = B.dpp_hazards(obj)
    assert ndpp and bad == 0
