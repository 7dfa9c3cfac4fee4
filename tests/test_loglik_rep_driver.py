"""The host side of gpv_plan_set_replicates / gpv_plan_loglik_rep / gpv_plan_loglik_rep_nu under AddressSanitizer + UBSan, on the
CPU, as a stand-alone program (tests/sanitize/loglik_rep_driver.cpp).

Kernels do not run, so the program checks statuses, bounds, lifetimes and leaks, never numbers. Built by
tests/_host_driver_build.py: a program of its own with the sanitizer linked in; nothing is preloaded and nothing is loaded into
python.
"""
import pytest

import _host_driver_build as H

DRIVERS = {"loglik_rep_driver": []}


@pytest.fixture(scope="module")
def programs():
    return H.programs_or_skip(DRIVERS)


@pytest.mark.parametrize("driver", list(DRIVERS))
def test_rep_driver_is_clean(programs, driver):
    """The driver ends with status 0 (no failed expectation) and neither sanitizer nor LeakSanitizer has anything to say."""
    rc, log = H.run_driver(programs, driver, DRIVERS[driver])
    print(log[-4000:])
    assert rc == 0 and not H.BAD.search(log), log[-4000:]
    assert "0 failed expectation(s)" in log
