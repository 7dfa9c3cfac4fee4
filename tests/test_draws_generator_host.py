"""The counter-based generator of the posterior draws on the HOST (gpv_draws_normals_host, csrc/gpv_philox.hpp) against a
restatement in Python integers and NumPy: Philox4x32-10 known answers (the vectors of the Random123 distribution), the
52-bit uniforms and FP64 Box-Muller, and the contract that a normal depends on (seed, location, draw) only.  No device."""
import math

import numpy as np
import pytest

M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(ctr, key):
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return c


def normal_ref(seed, k, j):
    """The normal of (ordered location k, draw j): counter (k, q = j // 2), key seed; draw 2q the cosine, 2q + 1 the sine."""
    q = j // 2
    w = philox4x32_10([k & MASK, k >> 32, q & MASK, q >> 32], [seed & MASK, seed >> 32])
    a, b = (w[0] << 20) | (w[1] >> 12), (w[2] << 20) | (w[3] >> 12)
    u1, u2 = (a + 0.5) * 2.0 ** -52, (b + 0.5) * 2.0 ** -52
    assert 0.0 < u1 < 1.0 and 0.0 < u2 < 1.0
    r = math.sqrt(-2.0 * math.log(u1))
    return r * (math.sin(2.0 * math.pi * u2) if j & 1 else math.cos(2.0 * math.pi * u2))


def _host(seed, k0, nk, col0, ncols):
    from gpvecchia_amd import lincomb as LC
    return LC.draws_normals_host(seed, k0, nk, col0, ncols)


def test_philox_known_answers():
    assert philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_symbols_and_argument_checks():
    from gpvecchia_amd import _lib as L
    import gpvecchia_amd as G
    lib = L.lib()
    for name in ("gpv_draws_normals_host", "gpv_plan_draws_normals", "gpv_plan_draws_summary"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert callable(G.vecchia_posterior_summary) and hasattr(G.Plan, "draws_summary") and hasattr(G.Plan, "draws_normals")
    e = np.zeros(8)
    assert lib.gpv_draws_normals_host(1, 0, 4, 0, 2, None, 4) == 2                 # GPV_ERR_BAD_ARG
    assert lib.gpv_draws_normals_host(1, -1, 4, 0, 2, L.dptr(e), 4) == 2
    assert lib.gpv_draws_normals_host(1, 0, 4, -1, 2, L.dptr(e), 4) == 2
    assert lib.gpv_draws_normals_host(1, 0, 4, 0, 2, L.dptr(e), 3) == 2            # lde < nk
    assert lib.gpv_draws_normals_host(1, 0, 0, 0, 2, L.dptr(e), 4) == 0 and np.all(e == 0.0)
    assert lib.gpv_draws_normals_host(1, 0, 4, 0, 2, L.dptr(e), 4) == 0 and np.all(e != 0.0)
    m = np.zeros(4)
    assert lib.gpv_plan_draws_normals(None, 1, 0, 0, 1, L.dptr(m), 4) == 2         # no plan: before any device is touched
    assert lib.gpv_plan_draws_summary(None, 4, 1, 0, None, 0, 0, None, None, L.dptr(m), L.dptr(m), None, None, None) == 2


@pytest.mark.parametrize("seed", [0, 1, 2 ** 63 + 5])
def test_normals_against_the_restatement(seed):
    """|diff| <= 1e-13: Box-Muller values stay below 8.5, a few ulp of log, sqrt and sincos there are below 1e-14."""
    ks = [0, 1, 63, 64, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]
    draws = [0, 1, 2, 31, 32, 33]
    worst = 0.0
    for k in ks:
        got = _host(seed, k, 1, 0, 34)                                             # (34, 1): the draws 0 .. 33
        for j in draws:
            ref = normal_ref(seed, k, j)
            assert abs(ref) < 8.5
            worst = max(worst, abs(got[j, 0] - ref))
            assert np.array_equal(_host(seed, k, 1, j, 1), got[j:j + 1])           # the same bits when asked for alone
    print(f"seed {seed}: max |host - restatement| = {worst:.3e}")
    assert worst <= 1e-13


def test_a_normal_does_not_depend_on_the_request():
    seed = 77
    blk = _host(seed, 0, 200, 0, 70)
    assert blk.shape == (70, 200) and np.all(np.isfinite(blk))
    for j in (0, 1, 31, 32, 33, 69):
        assert np.array_equal(_host(seed, 0, 200, j, 1)[0], blk[j])
    assert np.array_equal(_host(seed, 64, 1, 0, 70)[:, 0], blk[:, 64])
    assert np.array_equal(_host(seed, 64, 1, 5, 3)[:, 0], blk[5:8, 64])
    # and the values look like standard normals: 14 000 of them
    assert abs(blk.mean()) < 5.0 / np.sqrt(blk.size) and abs(blk.var() - 1.0) < 5.0 * np.sqrt(2.0 / blk.size)
    assert not np.array_equal(_host(seed + 1, 0, 200, 0, 70), blk)
