"""The host half of gpv_find_ordered_nn under AddressSanitizer + UBSan, on the CPU, as a stand-alone program
(tests/sanitize/nn_driver.cpp).

Kernels do not run, so the program checks statuses, bounds, lifetimes and leaks, never indices.  Built by
tests/_host_driver_build.py (gpv_nn.hip with the product's own -ffp-contract=off, as every recipe has it from
gpvecchia_amd.build.units()): a program of its own with the sanitizer linked in; nothing is preloaded and nothing is loaded into
python.
"""
import re

import pytest

import _host_driver_build as H

DRIVERS = {"nn_driver": []}


@pytest.fixture(scope="module")
def program():
    return H.programs_or_skip(DRIVERS)


def test_nn_driver_is_clean(program):
    """The driver ends with status 0 (no failed expectation) and neither sanitizer nor LeakSanitizer has anything to say."""
    rc, log = H.run_driver(program, "nn_driver", DRIVERS["nn_driver"])
    print(log[-4000:])
    assert rc == 0 and not H.BAD.search(log), log[-4000:]
    assert "0 failed expectation(s)" in log
    assert re.search(r"nn_driver: 0 failed expectation\(s\); [1-9]\d* kernel launches", log)
