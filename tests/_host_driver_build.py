"""The one build recipe of the stand-alone sanitizer drivers under tests/sanitize/: every unit of gpvecchia_amd.build.units() is
compiled --offload-host-only with the sanitizers in place of --offload-arch (a short row-length list), linked against
tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime, and each driver becomes a program of its own with the sanitizer
linked in.  Kernels do not run; nothing is preloaded and nothing is loaded into python.  The library's objects are compiled once
per process and (row-length list, sanitizer).  The driver tests and tools/sanitize_host.sh (through the command line below) use it:

    python tests/_host_driver_build.py --sanitize asan|tsan --plist 4,11,21 --out DIR driver[=args] ...
"""
import atexit
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpvecchia_amd", "csrc")
SAN = os.path.join(ROOT, "tests", "sanitize")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LLVM = "/opt/rocm/lib/llvm/bin"
PLIST = (4, 11, 21)                # 4, 11: the rows and bands of the drivers; 21: the row length with likelihood-only and lean units
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
SANITIZE_THREAD = ["-fsanitize=thread"]
BAD = re.compile(r"runtime error|ERROR: AddressSanitizer|ERROR: LeakSanitizer|WARNING: ThreadSanitizer")
_built = {}                        # (plist, sanitize) -> (folder, the library's objects, the drivers linked against them)


def have_toolchain():
    return os.path.exists(HIPCC) and os.path.exists(f"{LLVM}/clang++") and os.path.exists(f"{LLVM}/llvm-readelf")


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, **kw)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stdout}\n{r.stderr}"
    return r.stdout


def _cflags(sanitize):
    return ["--offload-host-only", "-O1", "-g", "-std=c++17", "-fPIC", "-fno-omit-frame-pointer", "-DGPV_DEVELOPER",
            "-Wno-unused-variable"] + list(sanitize)


def _library(plist, sanitize, out):
    """the library's host side and the mock runtime as objects in a folder (`out`, or a temporary one that lives as long as
    the process); compiled on the first call with these arguments"""
    key = (tuple(plist), tuple(sanitize))
    if key not in _built:
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        from gpvecchia_amd.build import units
        if out:
            os.makedirs(out, exist_ok=True)
        else:
            out = tempfile.mkdtemp(prefix="gpv_host_drivers_")
            atexit.register(shutil.rmtree, out, ignore_errors=True)
        plx = "-DGPV_P_LIST(X)=" + " ".join(f"X({P})" for P in sorted(plist))
        work = [(f"{CSRC}/{src}", f"{out}/{obj}", flags) for src, obj, flags, _ in units(plist, [plx])]
        work.append((f"{SAN}/mock_hip_runtime.cpp", f"{out}/mock.o", []))
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(lambda w: _run([HIPCC] + _cflags(sanitize) + w[2] + ["-c", w[0], "-o", w[1]]), work))
        objs = [o for _, o, _ in work]
        # the objects name their (absent) device images: one dummy symbol each
        syms = sorted(set(re.findall(r"\bUND\s+(__hip_fatbin_\w+)", _run([f"{LLVM}/llvm-readelf", "-s", "-W"] + objs))))
        with open(f"{out}/fatbin_stubs.c", "w") as fh:
            fh.writelines(f"const char {s}[8] = {{0}};\n" for s in syms)
        _run([f"{LLVM}/clang", "-c", f"{out}/fatbin_stubs.c", "-o", f"{out}/fatbin_stubs.o"])
        _built[key] = (out, objs + [f"{out}/fatbin_stubs.o"], set())
    return _built[key]


def build_programs(drivers, plist=PLIST, sanitize=SANITIZE, out=None):
    """links the drivers (names of tests/sanitize/<name>.cpp), each a program of its own, against the library's host side;
    returns the folder they are in"""
    B, objs, linked = _library(plist, sanitize, out)
    todo = [d for d in drivers if d not in linked]       # by this process, never by what lies in the folder: `out` may be an old one

    def link(d):
        _run([HIPCC] + _cflags(sanitize) + ["-c", f"{SAN}/{d}.cpp", "-o", f"{B}/{d}.main.o"])
        _run([f"{LLVM}/clang++"] + list(sanitize) + ["-g"] + objs + [f"{B}/{d}.main.o", "-o", f"{B}/{d}", "-lpthread", "-ldl", "-lm"])
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(link, todo))
    linked.update(todo)
    return B


def programs_or_skip(drivers, plist=PLIST):
    """body of the test files' module fixture"""
    if not have_toolchain():
        import pytest
        pytest.skip("no hipcc on this machine")
    return build_programs(drivers, plist)


def run_driver(B, driver, args=(), timeout=600):
    """runs a built driver; returns (return code, log)"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1")
    r = subprocess.run([os.path.join(B, driver)] + list(args), capture_output=True, text=True, cwd=B, env=env, timeout=timeout)
    return r.returncode, r.stdout + r.stderr


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="build the host-only sanitizer programs and run them")
    ap.add_argument("--sanitize", choices=["asan", "tsan"], default="asan")
    ap.add_argument("--plist", default=",".join(map(str, PLIST)), help="row lengths whose launch wrappers are compiled")
    ap.add_argument("--out", required=True, help="folder of the objects, the programs and their logs")
    ap.add_argument("--timeout", type=int, default=1500, help="seconds per driver")
    ap.add_argument("drivers", nargs="+", metavar="driver[=args]")
    a = ap.parse_args()
    sanitize = SANITIZE if a.sanitize == "asan" else SANITIZE_THREAD
    todo = {d: arg.split() for d, _, arg in (s.partition("=") for s in a.drivers)}
    B = build_programs(todo, [int(p) for p in re.split(r"[ ,]+", a.plist.strip())], sanitize, a.out)
    failed = []
    for d, args in todo.items():
        print(f"== {a.sanitize}: running {d} {' '.join(args)}", flush=True)
        try:
            rc, log = run_driver(B, d, args, a.timeout)
        except subprocess.TimeoutExpired as e:
            rc, log = 124, f"{e.stdout or ''}{e.stderr or ''}\n{d}: no end after {a.timeout} s"
        with open(f"{B}/run_{d}.log", "w") as fh:
            fh.write(log)
        print(log[-2000:])
        if rc != 0 or BAD.search(log):
            print(f"== {a.sanitize}: {d} FAILED (rc {rc})")
            failed.append(d)
    print(f"== {a.sanitize}: " + ("FAILED: " + " ".join(failed) if failed else "clean"))
    sys.exit(1 if failed else 0)
