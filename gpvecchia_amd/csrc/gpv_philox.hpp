// gpv_philox.hpp — the counter-based generator of the posterior draws, the same function on the host and on the device.
//
// Philox4x32 with 10 rounds (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11).  The normal
// of (ordered location k, draw j) is a function of (seed, k, j) alone: key = (seed low, seed high), counter = (k low, k high,
// q low, q high) with q = j / 2 the draw PAIR; the four output words give two uniforms of 52 random bits in (0, 1) and
// Box-Muller in FP64 turns them into the draws 2q (cosine) and 2q + 1 (sine).  Nothing depends on Nlocs, on the batch, on the
// position in the batch or on how many draws are asked for.  Plain C++: the 32 x 32 -> 64 bit products compile to
// v_mul_hi_u32 / v_mul_lo_u32 on the device.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GPV_PHILOX_HD __host__ __device__
#else
#define GPV_PHILOX_HD
#endif

namespace gpv {

// c[0..4) <- Philox4x32-10(counter c, key (k0, k1))
GPV_PHILOX_HD inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1;
        c[3] = (uint32_t)p0;
        c[0] = n0;
        c[2] = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// the standard normals of the draws 2q (z0) and 2q + 1 (z1) at ordered location k
GPV_PHILOX_HD inline void draws_normal_pair(uint64_t seed, uint64_t k, uint64_t q, double &z0, double &z1)
{
    uint32_t w[4] = {(uint32_t)k, (uint32_t)(k >> 32), (uint32_t)q, (uint32_t)(q >> 32)};
    philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t a = ((uint64_t)w[0] << 20) | (uint64_t)(w[1] >> 12);
    const uint64_t b = ((uint64_t)w[2] << 20) | (uint64_t)(w[3] >> 12);
    const double two52 = 2.220446049250313e-16;              // 2^-52; (a + 0.5) 2^-52 is exact and in (0, 1)
    const double u1 = ((double)a + 0.5) * two52, u2 = ((double)b + 0.5) * two52;
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
#if defined(__HIP_DEVICE_COMPILE__)
    sincospi(2.0 * u2, &s, &c);
#else
    sincos(6.283185307179586476925286766559 * u2, &s, &c);
#endif
    z0 = r * c;
    z1 = r * s;
}

}  // namespace gpv
