"""The host side of gpv_plan_cond_sim and gpv_csim_levels_host under AddressSanitizer + UBSan, on the CPU, as a stand-alone
program (tests/sanitize/csim_driver.cpp).

Kernels do not run, so the program checks statuses, refusals before the device is touched, the launch counts against the level
schedule (the factor pass by its chunks, a sweep by its wide levels and narrow runs, the packing, the batches of draws), the size
of every output (heap blocks of exactly the stated length), that an evaluation stays what it was, lifetimes and leaks, never
numbers.  Built by tests/_host_driver_build.py: a program of its own with the sanitizer linked in; nothing is preloaded and
nothing is loaded into python.
"""
import re

import pytest

import _host_driver_build as H

DRIVERS = {"csim_driver": []}


@pytest.fixture(scope="module")
def programs():
    return H.programs_or_skip(DRIVERS)


@pytest.mark.parametrize("driver", list(DRIVERS))
def test_csim_driver_is_clean(programs, driver):
    """The driver ends with status 0 (no failed expectation) and neither sanitizer nor LeakSanitizer has anything to say."""
    rc, log = H.run_driver(programs, driver, DRIVERS[driver])
    print(log[-4000:])
    assert rc == 0 and not H.BAD.search(log), log[-4000:]
    assert re.search(r"csim_driver: 0 failed expectation\(s\); [1-9]\d* kernel launches", log)
