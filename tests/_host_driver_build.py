"""Build recipe of the stand-alone sanitizer drivers under tests/sanitize/, as a function, for test files that add a driver: every
.hip unit of the library is compiled --offload-host-only with the sanitizers (a short row-length list), linked against
tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime, and each driver becomes a program of its own with the sanitizer
linked in.  Kernels do not run; nothing is preloaded and nothing is loaded into python.  (The recipe of tests/test_host_drivers.py
and tools/sanitize_host.sh; the older driver tests carry their own copies.)"""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpvecchia_amd", "csrc")
SAN = os.path.join(ROOT, "tests", "sanitize")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LLVM = "/opt/rocm/lib/llvm/bin"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
BAD = re.compile(r"runtime error|ERROR: AddressSanitizer|ERROR: LeakSanitizer")


def have_toolchain():
    return os.path.exists(HIPCC) and os.path.exists(f"{LLVM}/clang++") and os.path.exists(f"{LLVM}/llvm-readelf")


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, **kw)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stdout}\n{r.stderr}"
    return r.stdout


def build_programs(B, drivers, plist=(4, 21), sanitize=SANITIZE):
    """compiles the library's host side and the drivers (names of tests/sanitize/<name>.cpp) into the folder B; returns B"""
    from gpvecchia_amd.build import lean_p, lik_p
    cflags = ["--offload-host-only", "-O1", "-g", "-std=c++17", "-fPIC", "-fno-omit-frame-pointer", "-DGPV_DEVELOPER",
              "-Wno-unused-variable"] + list(sanitize)
    plx = "-DGPV_P_LIST(X)=" + " ".join(f"X({P})" for P in plist)
    units = []                                         # (source, object, extra flags)
    for f in ("gpv_api", "gpv_aux_kernels", "gpv_posterior", "gpv_lincomb", "gpv_laplace", "gpv_sets_generic", "gpv_nn"):
        units.append((f"{CSRC}/{f}.hip", f"{B}/{f}.o", [plx]))
    for pb in (16, 32, 64):
        units.append((f"{CSRC}/gpv_grad.hip", f"{B}/grad_pb{pb}.o", [f"-DGPV_GRAD_PB={pb}"]))
    units.append((f"{CSRC}/gpv_grad.hip", f"{B}/grad.o", []))
    for P in plist:
        units.append((f"{CSRC}/gpv_sets_inst.hip", f"{B}/sets_p{P}.o", [plx, f"-DGPV_INST_P={P}"]))
        if lik_p(P):
            units.append((f"{CSRC}/gpv_sets_inst.hip", f"{B}/sets_p{P}_lik.o", [plx, f"-DGPV_INST_P={P}", "-DGPV_INST_LIK"]))
        if lean_p(P):
            units.append((f"{CSRC}/gpv_sets_inst.hip", f"{B}/sets_p{P}_lean.o", [plx, f"-DGPV_INST_P={P}", "-DGPV_INST_LEAN"]))
    units.append((f"{CSRC}/gpv_order.cpp", f"{B}/order.o", ["-x", "c++"]))
    units.append((f"{SAN}/mock_hip_runtime.cpp", f"{B}/mock.o", []))
    lib_objs = [o for _, o, _ in units]
    for d in drivers:
        units.append((f"{SAN}/{d}.cpp", f"{B}/{d}.main.o", []))
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(lambda u: _run([HIPCC] + cflags + u[2] + ["-c", u[0], "-o", u[1]]), units))
    # the objects name their (absent) device images: one dummy symbol each
    syms = sorted(set(re.findall(r"\bUND\s+(__hip_fatbin_\w+)", _run([f"{LLVM}/llvm-readelf", "-s", "-W"] + lib_objs))))
    with open(f"{B}/fatbin_stubs.c", "w") as fh:
        fh.writelines(f"const char {s}[8] = {{0}};\n" for s in syms)
    _run([f"{LLVM}/clang", "-c", f"{B}/fatbin_stubs.c", "-o", f"{B}/fatbin_stubs.o"])
    for d in drivers:
        _run([f"{LLVM}/clang++"] + list(sanitize) + ["-g"] + lib_objs + [f"{B}/fatbin_stubs.o", f"{B}/{d}.main.o", "-o", f"{B}/{d}",
                                                                       "-lpthread", "-ldl", "-lm"])
    return B


def run_driver(B, driver, args=()):
    """runs a built driver; returns (return code, log)"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(B, driver)] + list(args), capture_output=True, text=True, cwd=B, env=env, timeout=600)
    return r.returncode, r.stdout + r.stderr
