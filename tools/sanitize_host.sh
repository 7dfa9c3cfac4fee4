#!/bin/bash
# Sanitizers over the HOST side of the product and over the oracle, on the CPU (no GPU needed; sanitizers are not available on
# the GPU pool).  Exits 0 when every build is clean.
#
#   1. libgpvecchia_hip's host code (gpv_api.hip, the launch wrappers of every kernel TU, gpv_order.cpp): every unit of the
#      library's build list compiled --offload-host-only with -fsanitize=address,undefined, linked against
#      tests/sanitize/mock_hip_runtime.cpp (host-memory stand-in for the HIP runtime: kernels do not run) and driven through the
#      public C ABI by tests/sanitize/host_driver.cpp and the other programs there, each a program of its own;
#   2. the same under -fsanitize=thread (hash threads, staged copies, plan cache mutex, replica threads);
#   3. oracle/*.c with -fsanitize=address,undefined, driven by the non-GPU test suite's oracle tests.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${SAN_OUT:-/tmp/gpv_sanitize}
PLIST="${SAN_PLIST:-4 11 21 31 61}"          # row lengths whose launch wrappers are compiled (host side only: seconds each)
mkdir -p "$OUT"

# the drivers every sanitizer runs; the build and the per-driver run, timeout and log check are tests/_host_driver_build.py,
# which takes the library's units from gpvecchia_amd/build.py units()
DRIVERS="solve_t_driver draws_summary_driver loglik_grad_driver loglik_grad_nu_driver whiten_driver loglik_rep_driver
  scaledim_driver selinv_driver sgv_grad_driver nn_driver loo_driver blockcv_driver krige_driver krige_groups_driver
  csim_driver csim_summary_driver"
python "$ROOT/tests/_host_driver_build.py" --sanitize asan --plist "$PLIST" --out "$OUT/asan" host_driver $DRIVERS \
  unwhiten_driver loglik_fisher_driver alloc_failure_driver
python "$ROOT/tests/_host_driver_build.py" --sanitize tsan --plist "$PLIST" --out "$OUT/tsan" host_driver=--quick $DRIVERS

echo "== oracle: -fsanitize=address,undefined under the oracle's own tests"
OB=$OUT/oracle; mkdir -p $OB
cp $ROOT/oracle/u_nzentries_oracle.c $ROOT/oracle/sparse_chol_oracle.c $OB/
gcc -O1 -g -fopenmp -fPIC -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -shared -o $OB/liboracle.so $OB/u_nzentries_oracle.c $OB/sparse_chol_oracle.c -lm
( cd $ROOT && GPV_ORACLE_LIB=$OB/liboracle.so LD_PRELOAD=$(gcc -print-file-name=libasan.so) ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 \
    UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 timeout 1500 python -m pytest tests/test_oracle.py tests/test_golden.py -x -q -m "not gpu" \
    -p no:cacheprovider ) 2>&1 | tee $OB/run.log | tail -5
if [ ${PIPESTATUS[0]} -ne 0 ] || grep -q "runtime error\|ERROR: AddressSanitizer" $OB/run.log; then echo "== oracle: FAILED"; exit 1; fi
echo "== oracle: clean"
echo "sanitize_host.sh: all clean"
