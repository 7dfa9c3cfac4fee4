"""The host side of covType "matern_scaledim" (one range per coordinate) under AddressSanitizer + UBSan, on the CPU, as a
stand-alone program (tests/sanitize/scaledim_driver.cpp, built by tests/_host_driver_build.py): with the mock runtime a plan
exists without a device, so the refusals of the family at the C ABI (wrong count, a range <= 0, more than three coordinates into
the gradient-type entries, a smoothness no entry takes), the one launch more per evaluation and the shapes of the outputs in 1, 2,
3 and 5 dimensions are checked here.  The covparms of the one- and three-dimensional cases sit in heap blocks of exactly
ncovparms doubles: an entry that reads covparms[ncovparms] is a sanitizer report.  Kernels do not run, so the program checks
statuses, bounds, lifetimes and leaks, never numbers."""
import pytest

import _host_driver_build as H

DRIVERS = {"scaledim_driver": []}


@pytest.fixture(scope="module")
def programs():
    return H.programs_or_skip(DRIVERS)


def test_scaledim_driver_is_clean(programs):
    """The driver ends with status 0 (no failed expectation) and neither sanitizer nor LeakSanitizer has anything to say."""
    rc, log = H.run_driver(programs, "scaledim_driver", DRIVERS["scaledim_driver"])
    print(log[-4000:])
    assert rc == 0 and not H.BAD.search(log), log[-4000:]
    assert "0 failed expectation(s)" in log
