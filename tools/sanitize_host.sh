#!/bin/bash
# Sanitizers over the HOST side of the product and over the oracle, on the CPU (no GPU needed; sanitizers are not available on
# the GPU pool).  Exits 0 when every build is clean.
#
#   1. libgpvecchia_hip's host code (gpv_api.hip, the launch wrappers of every kernel TU, gpv_order.cpp): every .hip file compiled
#      --offload-host-only with -fsanitize=address,undefined, linked against tests/sanitize/mock_hip_runtime.cpp (host-memory
#      stand-in for the HIP runtime: kernels do not run) and driven through the public C ABI by tests/sanitize/host_driver.cpp;
#   2. the same under -fsanitize=thread (hash threads, staged copies, plan cache mutex, replica threads);
#   3. oracle/*.c with -fsanitize=address,undefined, driven by the non-GPU test suite's oracle tests.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${SAN_OUT:-/tmp/gpv_sanitize}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
CLANGXX=/opt/rocm/lib/llvm/bin/clang++
CSRC=$ROOT/gpvecchia_amd/csrc
PLIST="${SAN_PLIST:-4 11 21 31 61}"          # row lengths whose launch wrappers are compiled (host side only: seconds each)
mkdir -p "$OUT"

build_and_run() {   # $1 = tag, $2 = sanitizer flags, $3 = driver args
  local tag=$1 san=$2 args=$3 B=$OUT/$1
  mkdir -p "$B"
  local CF="--offload-host-only -O1 -g -std=c++17 -fPIC -fno-omit-frame-pointer $san -DGPV_DEVELOPER -Wno-unused-variable"
  local plx=""; for P in $PLIST; do plx="$plx X($P)"; done
  local pids=()
  for f in gpv_api gpv_aux_kernels gpv_posterior gpv_lincomb gpv_laplace gpv_sets_generic gpv_nn; do
    $HIPCC $CF "-DGPV_P_LIST(X)=$plx" -c $CSRC/$f.hip -o $B/$f.o & pids+=($!)
  done
  for pb in 16 32 64; do                         # value + gradient kernel: one unit per row-length bucket, then its dispatcher
    $HIPCC $CF -DGPV_GRAD_PB=$pb -c $CSRC/gpv_grad.hip -o $B/grad_pb$pb.o & pids+=($!)
  done
  $HIPCC $CF -c $CSRC/gpv_grad.hip -o $B/grad.o & pids+=($!)
  $HIPCC $CF -c $CSRC/gpv_whiten.hip -o $B/whiten.o & pids+=($!)    # whitening and Gram passes: launchers only on the host
  $HIPCC $CF -c $CSRC/gpv_selinv.hip -o $B/selinv.o & pids+=($!)    # selected inverse: launchers only on the host
  $HIPCC $CF -c $CSRC/gpv_loo.hip -o $B/loo.o & pids+=($!)          # transposed whitening: launchers and the index builder
  $HIPCC $CF -c $CSRC/gpv_blockcv.hip -o $B/blockcv.o & pids+=($!)  # leave-block-out: launchers and the block index builder
  $HIPCC $CF -c $CSRC/gpv_krige.hip -o $B/krige.o & pids+=($!)      # local kriging: the launcher of the predict pass
  for pb in 16 32 64; do                         # gradient pass of the SGV likelihood: the same buckets, then its dispatcher
    $HIPCC $CF -DGPV_SGV_PB=$pb -c $CSRC/gpv_grad_sgv.hip -o $B/grad_sgv_pb$pb.o & pids+=($!)
  done
  $HIPCC $CF -c $CSRC/gpv_grad_sgv.hip -o $B/grad_sgv.o & pids+=($!)
  for P in $PLIST; do
    $HIPCC $CF "-DGPV_P_LIST(X)=$plx" -DGPV_INST_P=$P -c $CSRC/gpv_sets_inst.hip -o $B/sets_p$P.o & pids+=($!)
    if [ $P -gt 16 ] && [ $P -lt 32 ]; then      # likelihood-only kernels: a unit of their own (gpvecchia_amd/build.py lik_p)
      $HIPCC $CF "-DGPV_P_LIST(X)=$plx" -DGPV_INST_P=$P -DGPV_INST_LIK -c $CSRC/gpv_sets_inst.hip -o $B/sets_p${P}_lik.o & pids+=($!)
    fi
    if [ $P -eq 21 ] || [ $P -eq 26 ] || [ $P -eq 31 ]; then   # lean likelihood-only kernels (gpvecchia_amd/build.py lean_p)
      $HIPCC $CF "-DGPV_P_LIST(X)=$plx" -DGPV_INST_P=$P -DGPV_INST_LEAN -c $CSRC/gpv_sets_inst.hip -o $B/sets_p${P}_lean.o & pids+=($!)
    fi
  done
  $HIPCC $CF -x c++ -c $CSRC/gpv_order.cpp -o $B/order.o & pids+=($!)
  $HIPCC $CF -c $ROOT/tests/sanitize/mock_hip_runtime.cpp -o $B/mock.o & pids+=($!)
  $HIPCC $CF -c $ROOT/tests/sanitize/host_driver.cpp -o $B/driver.o & pids+=($!)
  for p in "${pids[@]}"; do wait $p; done
  # the objects name their (absent) device images: one dummy symbol each
  nm -u $B/*.o | awk '/__hip_fatbin_/ {print $2}' | sort -u | awk '{print "const char " $1 "[8] = {0};"}' > $B/fatbin_stubs.c
  gcc -c $B/fatbin_stubs.c -o $B/fatbin_stubs.o
  $CLANGXX $san -g $B/*.o -o $B/host_driver -lpthread -ldl -lm
  echo "== $tag: running host_driver $args"
  ( cd $B && ASAN_OPTIONS=detect_leaks=1:abort_on_error=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
      TSAN_OPTIONS=halt_on_error=1:second_deadlock_stack=1 timeout 1500 ./host_driver $args ) 2>&1 | tee $B/run.log
  local rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ] || grep -q "runtime error\|ERROR: AddressSanitizer\|WARNING: ThreadSanitizer\|ERROR: LeakSanitizer" $B/run.log; then
    echo "== $tag: FAILED (rc $rc)"; return 1
  fi
  # the same objects under the driver of gpv_plan_solve_t (a program of its own: tests/sanitize/solve_t_driver.cpp)
  mkdir -p $B/solve_t
  $HIPCC $CF -c $ROOT/tests/sanitize/solve_t_driver.cpp -o $B/solve_t/driver.o
  $CLANGXX $san -g $(ls $B/*.o | grep -v "/driver\.o$") $B/solve_t/driver.o -o $B/solve_t_driver -lpthread -ldl -lm
  ( cd $B && ASAN_OPTIONS=detect_leaks=1:abort_on_error=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
      TSAN_OPTIONS=halt_on_error=1 timeout 600 ./solve_t_driver ) 2>&1 | tee $B/run_solve_t.log
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ] || grep -q "runtime error\|ERROR: AddressSanitizer\|WARNING: ThreadSanitizer\|ERROR: LeakSanitizer" $B/run_solve_t.log; then
    echo "== $tag: solve_t_driver FAILED (rc $rc)"; return 1
  fi
  # ... and under the driver of the draws summaries (tests/sanitize/draws_summary_driver.cpp)
  mkdir -p $B/draws_summary
  $HIPCC $CF -c $ROOT/tests/sanitize/draws_summary_driver.cpp -o $B/draws_summary/driver.o
  $CLANGXX $san -g $(ls $B/*.o | grep -v "/driver\.o$") $B/draws_summary/driver.o -o $B/draws_summary_driver -lpthread -ldl -lm
  ( cd $B && ASAN_OPTIONS=detect_leaks=1:abort_on_error=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
      TSAN_OPTIONS=halt_on_error=1 timeout 600 ./draws_summary_driver ) 2>&1 | tee $B/run_draws_summary.log
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ] || grep -q "runtime error\|ERROR: AddressSanitizer\|WARNING: ThreadSanitizer\|ERROR: LeakSanitizer" $B/run_draws_summary.log; then
    echo "== $tag: draws_summary_driver FAILED (rc $rc)"; return 1
  fi
  # ... and under the driver of the value-and-gradient entry (tests/sanitize/loglik_grad_driver.cpp)
  mkdir -p $B/loglik_grad
  $HIPCC $CF -c $ROOT/tests/sanitize/loglik_grad_driver.cpp -o $B/loglik_grad/driver.o
  $CLANGXX $san -g $(ls $B/*.o | grep -v "/driver\.o$") $B/loglik_grad/driver.o -o $B/loglik_grad_driver -lpthread -ldl -lm
  ( cd $B && ASAN_OPTIONS=detect_leaks=1:abort_on_error=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
      TSAN_OPTIONS=halt_on_error=1 timeout 600 ./loglik_grad_driver ) 2>&1 | tee $B/run_loglik_grad.log
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ] || grep -q "runtime error\|ERROR: AddressSanitizer\|WARNING: ThreadSanitizer\|ERROR: LeakSanitizer" $B/run_loglik_grad.log; then
    echo "== $tag: loglik_grad_driver FAILED (rc $rc)"; return 1
  fi
  # ... and under the driver of the entries that differentiate the smoothness (tests/sanitize/loglik_grad_nu_driver.cpp)
  mkdir -p $B/loglik_grad_nu
  $HIPCC $CF -c $ROOT/tests/sanitize/loglik_grad_nu_driver.cpp -o $B/loglik_grad_nu/driver.o
  $CLANGXX $san -g $(ls $B/*.o | grep -v "/driver\.o$") $B/loglik_grad_nu/driver.o -o $B/loglik_grad_nu_driver -lpthread -ldl -lm
  ( cd $B && ASAN_OPTIONS=detect_leaks=1:abort_on_error=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
      TSAN_OPTIONS=halt_on_error=1 timeout 600 ./loglik_grad_nu_driver ) 2>&1 | tee $B/run_loglik_grad_nu.log
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ] || grep -q "runtime error\|ERROR: AddressSanitizer\|WARNING: ThreadSanitizer\|ERROR: LeakSanitizer" $B/run_loglik_grad_nu.log; then
    echo "== $tag: loglik_grad_nu_driver FAILED (rc $rc)"; return 1
  fi
  # ... and under the driver of the whitening entry (tests/sanitize/whiten_driver.cpp)
  mkdir -p $B/whiten
  $HIPCC $CF -c $ROOT/tests/sanitize/whiten_driver.cpp -o $B/whiten/driver.o
  $CLANGXX $san -g $(ls $B/*.o | grep -v "/driver\.o$") $B/whiten/driver.o -o $B/whiten_driver -lpthread -ldl -lm
  ( cd $B && ASAN_OPTIONS=detect_leaks=1:abort_on_error=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
      TSAN_OPTIONS=halt_on_error=1 timeout 600 ./whiten_driver ) 2>&1 | tee $B/run_whiten.log
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ] || grep -q "runtime error\|ERROR: AddressSanitizer\|WARNING: ThreadSanitizer\|ERROR: LeakSanitizer" $B/run_whiten.log; then
    echo "== $tag: whiten_driver FAILED (rc $rc)"; return 1
  fi
  # ... and under the driver of the replicate entries (tests/sanitize/loglik_rep_driver.cpp)
  mkdir -p $B/loglik_rep
  $HIPCC $CF -c $ROOT/tests/sanitize/loglik_rep_driver.cpp -o $B/loglik_rep/driver.o
  $CLANGXX $san -g $(ls $B/*.o | grep -v "/driver\.o$") $B/loglik_rep/driver.o -o $B/loglik_rep_driver -lpthread -ldl -lm
  ( cd $B && ASAN_OPTIONS=detect_leaks=1:abort_on_error=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
      TSAN_OPTIONS=halt_on_error=1 timeout 600 ./loglik_rep_driver ) 2>&1 | tee $B/run_loglik_rep.log
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ] || grep -q "runtime error\|ERROR: AddressSanitizer\|WARNING: ThreadSanitizer\|ERROR: LeakSanitizer" $B/run_loglik_rep.log; then
    echo "== $tag: loglik_rep_driver FAILED (rc $rc)"; return 1
  fi
  # ... and under the driver of the family with one range per coordinate (tests/sanitize/scaledim_driver.cpp)
  mkdir -p $B/scaledim
  $HIPCC $CF -c $ROOT/tests/sanitize/scaledim_driver.cpp -o $B/scaledim/driver.o
  $CLANGXX $san -g $(ls $B/*.o | grep -v "/driver\.o$") $B/scaledim/driver.o -o $B/scaledim_driver -lpthread -ldl -lm
  ( cd $B && ASAN_OPTIONS=detect_leaks=1:abort_on_error=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
      TSAN_OPTIONS=halt_on_error=1 timeout 600 ./scaledim_driver ) 2>&1 | tee $B/run_scaledim.log
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ] || grep -q "runtime error\|ERROR: AddressSanitizer\|WARNING: ThreadSanitizer\|ERROR: LeakSanitizer" $B/run_scaledim.log; then
    echo "== $tag: scaledim_driver FAILED (rc $rc)"; return 1
  fi
  # ... and under the driver of the selected inverse (tests/sanitize/selinv_driver.cpp)
  mkdir -p $B/selinv
  $HIPCC $CF -c $ROOT/tests/sanitize/selinv_driver.cpp -o $B/selinv/driver.o
  $CLANGXX $san -g $(ls $B/*.o | grep -v "/driver\.o$") $B/selinv/driver.o -o $B/selinv_driver -lpthread -ldl -lm
  ( cd $B && ASAN_OPTIONS=detect_leaks=1:abort_on_error=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
      TSAN_OPTIONS=halt_on_error=1 timeout 600 ./selinv_driver ) 2>&1 | tee $B/run_selinv.log
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ] || grep -q "runtime error\|ERROR: AddressSanitizer\|WARNING: ThreadSanitizer\|ERROR: LeakSanitizer" $B/run_selinv.log; then
    echo "== $tag: selinv_driver FAILED (rc $rc)"; return 1
  fi
  # ... and under the driver of the gradient of the SGV likelihood (tests/sanitize/sgv_grad_driver.cpp)
  mkdir -p $B/sgv_grad
  $HIPCC $CF -c $ROOT/tests/sanitize/sgv_grad_driver.cpp -o $B/sgv_grad/driver.o
  $CLANGXX $san -g $(ls $B/*.o | grep -v "/driver\.o$") $B/sgv_grad/driver.o -o $B/sgv_grad_driver -lpthread -ldl -lm
  ( cd $B && ASAN_OPTIONS=detect_leaks=1:abort_on_error=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
      TSAN_OPTIONS=halt_on_error=1 timeout 600 ./sgv_grad_driver ) 2>&1 | tee $B/run_sgv_grad.log
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ] || grep -q "runtime error\|ERROR: AddressSanitizer\|WARNING: ThreadSanitizer\|ERROR: LeakSanitizer" $B/run_sgv_grad.log; then
    echo "== $tag: sgv_grad_driver FAILED (rc $rc)"; return 1
  fi
  # ... and under the driver of the ordered nearest-neighbour search (tests/sanitize/nn_driver.cpp)
  mkdir -p $B/nn
  $HIPCC $CF -c $ROOT/tests/sanitize/nn_driver.cpp -o $B/nn/driver.o
  $CLANGXX $san -g $(ls $B/*.o | grep -v "/driver\.o$") $B/nn/driver.o -o $B/nn_driver -lpthread -ldl -lm
  ( cd $B && ASAN_OPTIONS=detect_leaks=1:abort_on_error=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
      TSAN_OPTIONS=halt_on_error=1 timeout 600 ./nn_driver ) 2>&1 | tee $B/run_nn.log
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ] || grep -q "runtime error\|ERROR: AddressSanitizer\|WARNING: ThreadSanitizer\|ERROR: LeakSanitizer" $B/run_nn.log; then
    echo "== $tag: nn_driver FAILED (rc $rc)"; return 1
  fi
  # ... and under the driver of the transposed whitening and leave-one-out entries (tests/sanitize/loo_driver.cpp)
  mkdir -p $B/loo
  $HIPCC $CF -c $ROOT/tests/sanitize/loo_driver.cpp -o $B/loo/driver.o
  $CLANGXX $san -g $(ls $B/*.o | grep -v "/driver\.o$") $B/loo/driver.o -o $B/loo_driver -lpthread -ldl -lm
  ( cd $B && ASAN_OPTIONS=detect_leaks=1:abort_on_error=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
      TSAN_OPTIONS=halt_on_error=1 timeout 600 ./loo_driver ) 2>&1 | tee $B/run_loo.log
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ] || grep -q "runtime error\|ERROR: AddressSanitizer\|WARNING: ThreadSanitizer\|ERROR: LeakSanitizer" $B/run_loo.log; then
    echo "== $tag: loo_driver FAILED (rc $rc)"; return 1
  fi
  # ... and under the driver of the leave-block-out entries (tests/sanitize/blockcv_driver.cpp)
  mkdir -p $B/blockcv
  $HIPCC $CF -c $ROOT/tests/sanitize/blockcv_driver.cpp -o $B/blockcv/driver.o
  $CLANGXX $san -g $(ls $B/*.o | grep -v "/driver\.o$") $B/blockcv/driver.o -o $B/blockcv_driver -lpthread -ldl -lm
  ( cd $B && ASAN_OPTIONS=detect_leaks=1:abort_on_error=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
      TSAN_OPTIONS=halt_on_error=1 timeout 600 ./blockcv_driver ) 2>&1 | tee $B/run_blockcv.log
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ] || grep -q "runtime error\|ERROR: AddressSanitizer\|WARNING: ThreadSanitizer\|ERROR: LeakSanitizer" $B/run_blockcv.log; then
    echo "== $tag: blockcv_driver FAILED (rc $rc)"; return 1
  fi
  # ... and under the driver of the local kriging entries (tests/sanitize/krige_driver.cpp)
  mkdir -p $B/krige
  $HIPCC $CF -c $ROOT/tests/sanitize/krige_driver.cpp -o $B/krige/driver.o
  $CLANGXX $san -g $(ls $B/*.o | grep -v "/driver\.o$") $B/krige/driver.o -o $B/krige_driver -lpthread -ldl -lm
  ( cd $B && ASAN_OPTIONS=detect_leaks=1:abort_on_error=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 \
      TSAN_OPTIONS=halt_on_error=1 timeout 600 ./krige_driver ) 2>&1 | tee $B/run_krige.log
  rc=${PIPESTATUS[0]}
  if [ $rc -ne 0 ] || grep -q "runtime error\|ERROR: AddressSanitizer\|WARNING: ThreadSanitizer\|ERROR: LeakSanitizer" $B/run_krige.log; then
    echo "== $tag: krige_driver FAILED (rc $rc)"; return 1
  fi
  echo "== $tag: clean"
}

build_and_run asan "-fsanitize=address,undefined -fno-sanitize-recover=undefined" ""
build_and_run tsan "-fsanitize=thread" "--quick"

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
