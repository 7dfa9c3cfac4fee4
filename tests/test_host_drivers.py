"""The host side of libgpvecchia_hip under AddressSanitizer + UBSan, on the CPU, as stand-alone programs.

Every unit of gpvecchia_amd.build.units() is compiled --offload-host-only with the sanitizers (a short row-length list: seconds,
not minutes), linked against tests/sanitize/mock_hip_runtime.cpp instead of the HIP runtime, and driven through the public C ABI
by the programs under tests/sanitize/.  Kernels do not run, so the programs check statuses, bounds, lifetimes and leaks, never
numbers.  Nothing is preloaded and nothing is loaded into python: each driver is a program of its own with the sanitizer linked
in.  The recipe is tests/_host_driver_build.py, which the other driver tests and tools/sanitize_host.sh use as well.
"""
import pytest

import _host_driver_build as H

DRIVERS = {"host_driver": ["--quick"], "solve_t_driver": [], "draws_summary_driver": [], "loglik_grad_driver": [],
           "alloc_failure_driver": []}


@pytest.fixture(scope="module")
def programs():
    return H.programs_or_skip(DRIVERS)


@pytest.mark.parametrize("driver", list(DRIVERS))
def test_host_driver_is_clean(programs, driver):
    """The driver ends with status 0 (no failed expectation) and neither sanitizer nor LeakSanitizer has anything to say.
    alloc_failure_driver: every allocation of one pass through the ABI fails once; the failed call reports GPV_ERR_HIP with
    the allocating call's name, succeeds when repeated, the pass ends with the undisturbed outputs and nothing stays allocated."""
    rc, log = H.run_driver(programs, driver, DRIVERS[driver])
    print(log[-4000:])
    assert rc == 0 and not H.BAD.search(log), log[-4000:]
    assert "0 failed expectation(s)" in log
    if driver in ("host_driver", "alloc_failure_driver"):
        assert "0 device allocation(s) still alive" in log or "0 allocation(s) still alive" in log
