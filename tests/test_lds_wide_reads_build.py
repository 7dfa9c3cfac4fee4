"""The 2-D closed-form set kernels read a partner's (x, y) as ONE 16-byte LDS load from the bank-checked layout of
SetsLdsDims ("LDS layout of the 2-D set kernels").  On the built objects sets_p{21,26,31}_lean.o and sets_p31.o:

  * every 2-D closed-form kernel has at least 2 * (P / 2) ds_read_b128 (one per row slot and round);
  * the 2-D lean kernels have no ds_read2_b64 with adjacent offsets (offset0:2k offset1:2k+1, what hipcc makes of two doubles
    read through a pointer it knows to be 8-byte aligned only) beyond the few the parent commit's 1-D kernels also have --
    the read-back of a row slot's own coordinates: none left on the coordinate base in the rounds;
  * VGPRs no higher than the parent commit's for the same kernel (recorded below), no AGPR, no scratch, no spill;
  * build.dpp_hazards reports 0;
  * the workgroup's LDS (.group_segment_fixed_size) is what tools/lds_bank_model.py computes from the layout formulas, for one,
    two and three dimensions (one and three: the parent commit's sizes)."""
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
_spec = importlib.util.spec_from_file_location("lds_bank_model", os.path.join(ROOT, "tools", "lds_bank_model.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

# The parent commit's figures for gpv_sets_kernel<P, 2, COV, LIK> (COV 0 / 1 / 2 = Matern 0.5 / 1.5 / 2.5, 3 = esqe, + 16 = lean).
# Lean kernels <P, 2, 16..18, true>: vgpr_count; no SGPR spill then or now.
PARENT_VGPR_LEAN = {21: 178, 26: 200, 31: 218}
# sets_p31.o's Gauss-Jordan kernels <31, 2, COV, false>: (vgpr_count, sgpr_spill_count).  They spilled SGPRs before this change
# (no register room); the bound here is "no more than they did".
PARENT_GJ31 = {0: (231, 24), 1: (231, 26), 2: (231, 28), 3: (209, 53)}


def _code_object(obj):
    with tempfile.TemporaryDirectory() as td:
        fat, co = os.path.join(td, "x.fat"), os.path.join(td, "x.co")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
    return dis, notes


def _kernels(obj):
    """{mangled name: figures} of the set kernels in obj, and {mangled name: disassembly}"""
    dis, notes = _code_object(obj)
    res = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        def g(key):
            return re.search(r"\.%s:\s+(\S+)" % key, blk).group(1)
        if "gpv_sets_kernel" in g("name"):
            res[g("name")] = dict(agpr=int(blk.split()[0]), lds=int(g("group_segment_fixed_size")),
                                  scratch=int(g("private_segment_fixed_size")), sspill=int(g("sgpr_spill_count")),
                                  vgpr=int(g("vgpr_count")), vspill=int(g("vgpr_spill_count")))
    text = {}
    for blk in re.split(r"\n(?=[0-9a-f]+ <)", dis):
        m = re.search(r"<(\S+)>", blk.split("\n", 1)[0])
        if m and m.group(1) in res:
            text[m.group(1)] = blk
    assert set(text) == set(res)
    return res, text


def _name(k):
    """(P, D, COVX, LIK) of a mangled gpv_sets_kernel<P, D, COVX, LIK>"""
    m = re.search(r"gpv_sets_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])EEEv", k)
    return int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4) == "1"


def _adjacent_read2(blk):
    """ds_read2_b64 with offset1 == offset0 + 1: two adjacent doubles"""
    n = 0
    for line in blk.split("\n"):
        if "ds_read2_b64" in line:
            o0 = re.search(r"offset0:(\d+)", line)
            o1 = re.search(r"offset1:(\d+)", line)
            n += (int(o1.group(1)) if o1 else 0) == (int(o0.group(1)) if o0 else 0) + 1
    return n


def _obj(name):
    if not all(os.path.exists(f"{LLVM}/{t}") for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")):
        pytest.skip("no ROCm llvm tools on this machine")
    from gpvecchia_amd import build as B
    obj = os.path.join(B.CSRC, "build", name)
    if not os.path.exists(obj):
        pytest.skip("no object files in this tree (library built elsewhere)")
    return B, obj


@pytest.mark.parametrize("P", [21, 26, 31])
def test_lean_kernels_read_coordinates_16_bytes_wide(P):
    B, obj = _obj(f"sets_p{P}_lean.o")
    res, text = _kernels(obj)
    assert len(res) == 9                                      # 3 dimensions x Matern 0.5 / 1.5 / 2.5
    rows_read2 = {}
    for k, r in res.items():
        p, d, covx, lik = _name(k)
        assert p == P and lik and covx in (16, 17, 18)
        assert r["agpr"] == 0 and r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, (k, r)
        assert r["lds"] == M.Layout(P, d, True).workgroup, (k, r["lds"])
        nb128 = len(re.findall(r"\bds_read_b128\b", text[k]))
        if d == 2:
            assert r["vgpr"] <= PARENT_VGPR_LEAN[P], (k, r)
            assert nb128 >= 2 * (P // 2), (k, nb128)
        else:
            assert nb128 == 0, (k, nb128)                     # one and three dimensions: as they were
        rows_read2[(d, covx)] = _adjacent_read2(text[k])
    for covx in (16, 17, 18):
        # adjacent-offset pairs left in a 2-D kernel: the row reads (two columns of a row) and one read-back of a slot's own
        # coordinates -- what the 1-D kernel, which reads one coordinate at a time, has for its rows, plus at most that one
        # per task path (straight and padded rounds); the 2 * (P / 2) partner fetches per path are gone
        assert rows_read2[(2, covx)] <= rows_read2[(1, covx)] + 2, (covx, rows_read2)
    ndpp, bad = B.dpp_hazards(obj)
    assert ndpp and bad == 0


def test_gauss_jordan_kernels_of_p31_read_coordinates_16_bytes_wide():
    B, obj = _obj("sets_p31.o")
    res, text = _kernels(obj)
    seen = 0
    for k, r in res.items():
        p, d, cov, lik = _name(k)
        if d != 2 or cov not in PARENT_GJ31:
            continue                                          # general nu keeps its layout (every spare byte of LDS holds its table)
        seen += 1
        vg, ss = PARENT_GJ31[cov]
        assert not lik and r["vgpr"] <= vg and r["sspill"] <= ss, (k, r)
        assert r["agpr"] == 0 and r["scratch"] == 0 and r["vspill"] == 0, (k, r)
        assert r["lds"] == M.Layout(31, 2, True).workgroup == 81920, (k, r["lds"])
        assert len(re.findall(r"\bds_read_b128\b", text[k])) >= 2 * (31 // 2), k
    assert seen == 4
    ndpp, bad = B.dpp_hazards(obj)
    assert ndpp and bad == 0
