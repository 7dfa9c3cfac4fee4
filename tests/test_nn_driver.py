"""The host half of gpv_find_ordered_nn under AddressSanitizer + UBSan, on the CPU, as a stand-alone program
(tests/sanitize/nn_driver.cpp).

The recipe is that of tests/test_whiten_driver.py, cut down to what the entry needs: csrc/gpv_nn.hip compiled --offload-host-only
with the sanitizers and the product's own -ffp-contract=off, linked against tests/sanitize/mock_hip_runtime.cpp instead of the HIP
runtime, and driven through the public C ABI.  gpv_find_ordered_nn calls nothing else of the library, so no other unit is
needed.  Kernels do not run, so the program checks statuses, bounds, lifetimes and leaks, never indices.  Nothing is preloaded
and nothing is loaded into python: the driver is a program of its own with the sanitizer linked in.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpvecchia_amd", "csrc")
SAN = os.path.join(ROOT, "tests", "sanitize")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LLVM = "/opt/rocm/lib/llvm/bin"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
CFLAGS = ["--offload-host-only", "-O1", "-g", "-std=c++17", "-fPIC", "-fno-omit-frame-pointer", "-Wno-unused-variable"] + SANITIZE
BAD = re.compile(r"runtime error|ERROR: AddressSanitizer|ERROR: LeakSanitizer")


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, **kw)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stdout}\n{r.stderr}"
    return r.stdout


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not (os.path.exists(HIPCC) and os.path.exists(f"{LLVM}/clang++") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("no hipcc on this machine")
    B = str(tmp_path_factory.mktemp("nn_driver"))
    units = [(f"{CSRC}/gpv_nn.hip", f"{B}/gpv_nn.o", ["-ffp-contract=off"]),
             (f"{SAN}/mock_hip_runtime.cpp", f"{B}/mock.o", []),
             (f"{SAN}/nn_driver.cpp", f"{B}/nn_driver.main.o", [])]
    for src, obj, extra in units:
        _run([HIPCC] + CFLAGS + extra + ["-c", src, "-o", obj])
    # the object names its (absent) device image: one dummy symbol
    syms = sorted(set(re.findall(r"\bUND\s+(__hip_fatbin_\w+)", _run([f"{LLVM}/llvm-readelf", "-s", "-W", f"{B}/gpv_nn.o"]))))
    with open(f"{B}/fatbin_stubs.c", "w") as fh:
        fh.writelines(f"const char {s}[8] = {{0}};\n" for s in syms)
    _run([f"{LLVM}/clang", "-c", f"{B}/fatbin_stubs.c", "-o", f"{B}/fatbin_stubs.o"])
    _run([f"{LLVM}/clang++"] + SANITIZE + ["-g"] + [o for _, o, _ in units] + [f"{B}/fatbin_stubs.o", "-o", f"{B}/nn_driver",
                                                                              "-lpthread", "-ldl", "-lm"])
    return B


def test_nn_driver_is_clean(program):
    """The driver ends with status 0 (no failed expectation) and neither sanitizer nor LeakSanitizer has anything to say."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(program, "nn_driver")], capture_output=True, text=True, cwd=program, env=env, timeout=600)
    log = r.stdout + r.stderr
    print(log[-4000:])
    assert r.returncode == 0 and not BAD.search(log), log[-4000:]
    assert "0 failed expectation(s)" in log
    assert re.search(r"nn_driver: 0 failed expectation\(s\); [1-9]\d* kernel launches", log)
