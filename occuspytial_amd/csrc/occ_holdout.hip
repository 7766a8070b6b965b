// occ_holdout.hip -- the kernel of the held-out predictive scoring and its launcher (occ_holdout.hpp).  A
// translation unit of its own, linked into libocc_gibbs.so: it shares occ_state.hpp with the engine's unit and none of its
// kernels.
#include "occ_holdout.hpp"

namespace occ {

// Does the sequence of parity e count for this chain?  Uniform over the chain, written as conv_counts_now (occ_conv.hip) and
// hist_counts_now (occ_hist.hip) write it: the kernels of sequence e read ChainScalars::ctl[e]; its z update, the kernel in
// front of this one, left ctl[e ^ 1]: it + 1 if it completed iteration `it`, and `it` itself if the chain idled -- past
// it_stop, err set, or a solve carried to the next replay.  err (which the z update itself may have raised) is asked again.
// The window is the one of the site sums: every iteration past the call's burn-in, whatever `keep` -- so occ_step, whose
// window has burn-in 0, counts.
__device__ __forceinline__ bool holdout_counts_now(const HoldoutArgs &a, const ChainScalars &sc, int chain, int e)
{
    const uint32_t t = sc.ctl[e].it, after = sc.ctl[e ^ 1].it;
    const uint32_t rel = t - sc.it_base;
    return a.on[chain] != 0u && a.sums != nullptr && after == t + 1u && sc.err == 0 && rel >= sc.burnin;
}

// log expit(t) = min(t, 0) - log1p(exp(-|t|)) from e = exp(-|t|); expit(t) and 1 - expit(t) come from the same e by
// expit_e and expit_c (occ_state.hpp).  As the streaming WAIC's z update has them.
__device__ __forceinline__ double hold_lsig(double t, double e) { return fmin(t, 0.0) - log1p(e); }

__global__ void __launch_bounds__(256) k_holdout_sites(const HoldoutArgs a, const ChainScalars *__restrict__ scs, int e)
{
    const int chain = blockIdx.y;
    const ChainScalars &sc = scs[chain];
    if (!holdout_counts_now(a, sc, chain, e)) return;
    if (blockIdx.x == 0u && threadIdx.x == 0u) a.count[chain] += 1.0;
    const int n = a.n, h = (int)(blockIdx.x * 256u + threadIdx.x);
    if (h >= a.H) return;
    const int i = a.site[h], r0 = a.ptr[h], r1 = a.ptr[h + 1];
    const bool seen = a.seen[h] != 0;
    const double a0 = xdot(a.Xt, n, i, sc.beta, a.p) + a.eta[(size_t)chain * n + i], e0 = exp(-fabs(a0));
    const double psi = expit_e(a0, e0);
    double prod = 1.0, ll = seen ? hold_lsig(a0, e0) : 0.0;
    for (int r = r0; r < r1; ++r) {  // ONE loop for both kinds of entry: the same load, dot product and exponential
        double t = 0.0;
        for (int k = 0; k < a.q; ++k) t = fma(a.Wt[(size_t)k * a.R + r], -sc.alpha[k], t);
        const double et = exp(-fabs(t));
        const double ex = expit_e(t, et);
        prod = (r == r0) ? ex : prod * ex;
        if (seen) ll += hold_lsig(a.y[r] ? -t : t, et);  // rows in row order
    }
    double lik;
    if (seen) {
        lik = exp(ll);
    } else {
        lik = z_den(a0, e0, psi, psi * prod);
        ll = log(lik);
    }
    const double pd = psi * (1.0 - prod);
    double *at = a.sums + (size_t)chain * a.H + h;
    at[HOLD_CNT * a.CH] += 1.0;
    at[HOLD_LIK * a.CH] += lik;
    at[HOLD_LOG * a.CH] += ll;
    at[HOLD_LOG2 * a.CH] = fma(ll, ll, at[HOLD_LOG2 * a.CH]);
    at[HOLD_PD * a.CH] += pd;
}

void holdout_launch(const HoldoutArgs &a, const ChainScalars *scs, int C, int e, hipStream_t st)
{
    const dim3 grid((unsigned)((a.H + 255) / 256), (unsigned)C);
    hipLaunchKernelGGL(k_holdout_sites, grid, dim3(256), 0, st, a, scs, e);
}

}  // namespace occ
