"""The host side of gpv_plan_krige / gpv_find_query_nn under AddressSanitizer + UBSan, on the CPU, as a stand-alone program
(tests/sanitize/krige_driver.cpp).

The recipe is that of tests/test_blockcv_driver.py, copied so that this file stands on its own, plus gpv_krige.hip: every .hip
unit is compiled --offload-host-only with the sanitizers (a short row-length list; gpv_nn.hip with the product's own
-ffp-contract=off), linked against tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime, and driven through the public
C ABI.  Kernels do not run, so the program checks statuses, refusals before the device is touched, the chunk arithmetic by its
launches, bounds, lifetimes and leaks, never numbers.  Nothing is preloaded and nothing is loaded into python: the driver is a
program of its own with the sanitizer linked in.
"""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpvecchia_amd", "csrc")
SAN = os.path.join(ROOT, "tests", "sanitize")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LLVM = "/opt/rocm/lib/llvm/bin"
PLIST = (4, 21)                                        # 21: the row length with likelihood-only and lean units (m = 20)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
CFLAGS = ["--offload-host-only", "-O1", "-g", "-std=c++17", "-fPIC", "-fno-omit-frame-pointer", "-DGPV_DEVELOPER",
          "-Wno-unused-variable"] + SANITIZE
DRIVERS = {"krige_driver": []}
BAD = re.compile(r"runtime error|ERROR: AddressSanitizer|ERROR: LeakSanitizer")


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, **kw)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stdout}\n{r.stderr}"
    return r.stdout


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    if not (os.path.exists(HIPCC) and os.path.exists(f"{LLVM}/clang++") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("no hipcc on this machine")
    from gpvecchia_amd.build import lean_p, lik_p
    B = str(tmp_path_factory.mktemp("krige_driver"))
    plx = "-DGPV_P_LIST(X)=" + " ".join(f"X({P})" for P in PLIST)
    units = []                                         # (source, object, extra flags)
    for f in ("gpv_api", "gpv_aux_kernels", "gpv_posterior", "gpv_lincomb", "gpv_laplace", "gpv_sets_generic"):
        units.append((f"{CSRC}/{f}.hip", f"{B}/{f}.o", [plx]))
    units.append((f"{CSRC}/gpv_nn.hip", f"{B}/gpv_nn.o", ["-ffp-contract=off"]))
    for pb in (16, 32, 64):
        units.append((f"{CSRC}/gpv_grad.hip", f"{B}/grad_pb{pb}.o", [f"-DGPV_GRAD_PB={pb}"]))
    units.append((f"{CSRC}/gpv_grad.hip", f"{B}/grad.o", []))
    units.append((f"{CSRC}/gpv_whiten.hip", f"{B}/whiten.o", []))
    units.append((f"{CSRC}/gpv_unwhiten.hip", f"{B}/unwhiten.o", []))
    units.append((f"{CSRC}/gpv_loo.hip", f"{B}/loo.o", []))
    units.append((f"{CSRC}/gpv_blockcv.hip", f"{B}/blockcv.o", []))
    units.append((f"{CSRC}/gpv_krige.hip", f"{B}/krige.o", []))
    for P in PLIST:
        units.append((f"{CSRC}/gpv_sets_inst.hip", f"{B}/sets_p{P}.o", [plx, f"-DGPV_INST_P={P}"]))
        if lik_p(P):
            units.append((f"{CSRC}/gpv_sets_inst.hip", f"{B}/sets_p{P}_lik.o", [plx, f"-DGPV_INST_P={P}", "-DGPV_INST_LIK"]))
        if lean_p(P):
            units.append((f"{CSRC}/gpv_sets_inst.hip", f"{B}/sets_p{P}_lean.o", [plx, f"-DGPV_INST_P={P}", "-DGPV_INST_LEAN"]))
    units.append((f"{CSRC}/gpv_order.cpp", f"{B}/order.o", ["-x", "c++"]))
    units.append((f"{SAN}/mock_hip_runtime.cpp", f"{B}/mock.o", []))
    lib_objs = [o for _, o, _ in units]
    for d in DRIVERS:
        units.append((f"{SAN}/{d}.cpp", f"{B}/{d}.main.o", []))
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(lambda u: _run([HIPCC] + CFLAGS + u[2] + ["-c", u[0], "-o", u[1]]), units))
    # the objects name their (absent) device images: one dummy symbol each
    syms = sorted(set(re.findall(r"\bUND\s+(__hip_fatbin_\w+)", _run([f"{LLVM}/llvm-readelf", "-s", "-W"] + lib_objs))))
    with open(f"{B}/fatbin_stubs.c", "w") as fh:
        fh.writelines(f"const char {s}[8] = {{0}};\n" for s in syms)
    _run([f"{LLVM}/clang", "-c", f"{B}/fatbin_stubs.c", "-o", f"{B}/fatbin_stubs.o"])
    for d in DRIVERS:
        _run([f"{LLVM}/clang++"] + SANITIZE + ["-g"] + lib_objs + [f"{B}/fatbin_stubs.o", f"{B}/{d}.main.o", "-o", f"{B}/{d}",
                                                                   "-lpthread", "-ldl", "-lm"])
    return B


@pytest.mark.parametrize("driver", list(DRIVERS))
def test_krige_driver_is_clean(programs, driver):
    """The driver ends with status 0 (no failed expectation) and neither sanitizer nor LeakSanitizer has anything to say."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(programs, driver)] + DRIVERS[driver], capture_output=True, text=True, cwd=programs, env=env,
                       timeout=600)
    log = r.stdout + r.stderr
    print(log[-4000:])
    assert r.returncode == 0 and not BAD.search(log), log[-4000:]
    assert re.search(r"krige_driver: 0 failed expectation\(s\); [1-9]\d* kernel launches", log)
