"""The host side of gpv_plan_cond_sim_summary under AddressSanitizer + UBSan, on the CPU, as a stand-alone program
(tests/sanitize/csim_summary_driver.cpp).

Kernels do not run, so the program checks statuses, refusals before the device is touched, the launch counts against the schedule
(the factor pass by its chunks, one sweep for the means and one per batch of 16 draws that the requested range touches, the
folds of a batch by the chunks and joins of the regions), the size of every output (heap blocks of exactly the stated length),
that an evaluation stays what it was, that gpv_plan_cond_sim launches what it did before, lifetimes and leaks, never numbers.
Built by tests/_host_driver_build.py: a program of its own with the sanitizer linked in; nothing is preloaded and nothing is
loaded into python.
"""
import re

import pytest

import _host_driver_build as H

DRIVERS = {"csim_summary_driver": []}


@pytest.fixture(scope="module")
def programs():
    return H.programs_or_skip(DRIVERS)


@pytest.mark.parametrize("driver", list(DRIVERS))
def test_csim_summary_driver_is_clean(programs, driver):
    """The driver ends with status 0 (no failed expectation) and neither sanitizer nor LeakSanitizer has anything to say."""
    rc, log = H.run_driver(programs, driver, DRIVERS[driver])
    print(log[-4000:])
    assert rc == 0 and not H.BAD.search(log), log[-4000:]
    assert re.search(r"csim_summary_driver: 0 failed expectation\(s\); [1-9]\d* kernel launches", log)
