// occ_conv.hip -- the kernel of the per-site convergence diagnostics and its launcher (occ_conv.hpp).  A
// translation unit of its own, linked into libocc_gibbs.so: it shares occ_state.hpp with the engine's unit and none of its
// kernels.
#include "occ_conv.hpp"

namespace occ {

// Does the sequence of parity e count for this chain?  Uniform over the chain, written as hist_counts_now (occ_hist.hip) writes
// it: the kernels of sequence e read ChainScalars::ctl[e]; its z update, the kernel in front of this one, left ctl[e ^ 1]:
// it + 1 if it completed iteration `it`, and `it` itself if the chain idled -- past it_stop, err set, or a solve carried to the
// next replay.  err (which the z update itself may have raised) is asked again.  The window is the one of the site sums: every
// iteration past the call's burn-in, whatever `keep` -- so occ_step, whose window has burn-in 0, counts.
__device__ __forceinline__ bool conv_counts_now(const ConvArgs &a, const ChainScalars &sc, int chain, int e)
{
    const uint32_t t = sc.ctl[e].it, after = sc.ctl[e ^ 1].it;
    const uint32_t rel = t - sc.it_base;
    return a.on[chain] != 0u && a.sums != nullptr && after == t + 1u && sc.err == 0 && rel >= sc.burnin;
}

// One quantity's five slots of one column: at[k Cn] is slot k.  first: the site's count was 0; closes: this value ends a batch.
__device__ __forceinline__ void conv_update(double *at, size_t Cn, double v, bool first, bool closes)
{
    const double ref = first ? v : at[CONV_REF * Cn];
    const double d = v - ref;
    double run = at[CONV_RUN * Cn] + d;
    if (first) at[CONV_REF * Cn] = ref;
    at[CONV_S1 * Cn] += d;
    at[CONV_S2 * Cn] += d * d;
    if (closes) {
        at[CONV_BSQ * Cn] += run * run;
        run = 0.0;
    }
    at[CONV_RUN * Cn] = run;
}

__global__ void __launch_bounds__(256) k_conv_sites(const ConvArgs a, const ChainScalars *__restrict__ scs, int e)
{
    const int chain = blockIdx.y;
    const ChainScalars &sc = scs[chain];
    if (!conv_counts_now(a, sc, chain, e)) return;
    if (blockIdx.x == 0u && threadIdx.x == 0u) a.count[chain] += 1.0;
    const int n = a.n, i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    const size_t col = (size_t)chain * n + i;
    const double eta = a.eta[col];
    const double psi = expit(xdot(a.Xt, n, i, sc.beta, a.p) + eta);
    double *at = a.sums + col;
    const double m = at[CONV_CNT * a.Cn];  // (a whole number below 2^53: the host admits nothing else)
    const bool first = m == 0.0;
    const bool closes = ((unsigned long long)m + 1ull) % (unsigned long long)a.L == 0ull;
    conv_update(at + CONV_PSI * a.Cn, a.Cn, psi, first, closes);
    conv_update(at + CONV_ETA * a.Cn, a.Cn, eta, first, closes);
    at[CONV_CNT * a.Cn] = m + 1.0;
}

void conv_launch(const ConvArgs &a, const ChainScalars *scs, int C, int e, hipStream_t st)
{
    const dim3 grid((unsigned)((a.n + 255) / 256), (unsigned)C);
    hipLaunchKernelGGL(k_conv_sites, grid, dim3(256), 0, st, a, scs, e);
}

}  // namespace occ
