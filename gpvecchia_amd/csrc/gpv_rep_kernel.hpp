// gpv_rep_kernel.hpp — value, gradient and expected Fisher information of the cond.yz='z' Vecchia log-likelihood SUMMED OVER R
// REPLICATES of the data over the same locations (gpv_plan_loglik_rep), gfx950, FP64.  Included by gpv_grad.hip inside its
// per-bucket half: the kernel is gpv_rep_kernel of that file (gpv_grad_set_pass.inc, kSetsRep), the Fisher mode with the
// replicate loop described here in place of the one column's row terms; every other phase is shared.
//
// Nothing of the factorisation depends on the data.  Per set, in the notation of gpv_grad.hip (u = S'^-1 e_last,
// t_p = D_p u with t_NPAR = u for the nugget, a_p = u't_p, y_p = S'^-1 t_p), the data enter a replicate's row terms only through
//     q_r = u'z_r       and       b_{p,r} = w_r't_p = z_r'S'^-1 t_p = z_r'y_p          (S' is symmetric),
// so the sweep carries the one right-hand side e_last, the replay gives y_p as it does for the information, and replicate r then
// costs NPAR + 2 dot products of length PB with the data-free vectors {u, y_0 .. y_NPAR}.  Summed over the replicates:
//     sum_r l_{k,r}             = R (1/2 log u_last - 1/2 log 2 pi) - 1/2 Q2 / u_last                    Q2   = sum_r q_r^2
//     sum_r dl_{k,r}/dtheta_p   = -1/2 R a_p / u_last + QB_p / u_last - 1/2 Q2 a_p / u_last^2            QB_p = sum_r q_r b_{p,r}
//     information               = R F_k                                            (it does not depend on the data)
//
// Replicate loop: lane i reads kRepChunk values of its neighbour at a time from Z[pos][RP] (contiguous, RP a multiple of
// kRepChunk, zeros behind column R) and forms the kRepChunk products with one of the NPAR + 2 vectors.  They are summed over the
// lanes by a reduce-scatter: the steps at lane distance 32, 16, 8 each HALVE the number of values a lane holds (a lane keeps the
// replicates of its half and hands over the others), 4 + 2 + 1 shuffles, and the steps at distance 4, 2, 1 finish the one value
// left, so a dot product costs 10 / 8 shuffles instead of 6.  Lane l then holds replicate (l >> 3) of the chunk, for every
// vector alike, squares and multiplies there, and accumulates over the chunks; one lane of each group of 8 enters the final sums.
// The order of every addition is fixed by the lane numbers: bitwise reproducible.
//
// Builtins only, no inline assembly.
#pragma once

// sum over the 64 lanes of each of the kRepChunk values x[c]; lane l returns the sum of x[l >> 3]
__device__ __forceinline__ double rep_reduce_scatter(const double (&x)[kRepChunk], const int lane)
{
    static_assert(kRepChunk == 8, "three halving steps");
    const bool h32 = lane & 32, h16 = lane & 16, h8 = lane & 8;
    double s4[4], s2[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) s4[i] = (h32 ? x[4 + i] : x[i]) + __shfl_xor(h32 ? x[i] : x[4 + i], 32, 64);
#pragma unroll
    for (int i = 0; i < 2; ++i) s2[i] = (h16 ? s4[2 + i] : s4[i]) + __shfl_xor(h16 ? s4[i] : s4[2 + i], 16, 64);
    double s = (h8 ? s2[1] : s2[0]) + __shfl_xor(h8 ? s2[0] : s2[1], 8, 64);
#pragma unroll
    for (int off = 4; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}
