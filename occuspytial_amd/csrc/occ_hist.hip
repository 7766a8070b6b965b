// occ_hist.hip -- the kernel of the per-site intervals and its launcher (occ_hist.hpp).  A translation
// unit of its own, linked into libocc_gibbs.so: it shares occ_state.hpp with the engine's unit and none of its kernels.
#include "occ_hist.hpp"

namespace occ {

// Does the sequence of parity e count for this chain?  Uniform over the chain, written as sp_row (occ_spatial.hip) writes it:
// the kernels of sequence e read ChainScalars::ctl[e]; its z update, the kernel in front of this one, left ctl[e ^ 1]: it + 1
// if it completed iteration `it`, and `it` itself if the chain idled -- past it_stop, err set, or a solve carried to the next
// replay.  err (which the z update itself may have raised) is asked again.  The window is the one of the site sums: every
// iteration past the call's burn-in, whatever `keep` -- so occ_step, whose window has burn-in 0, counts.
__device__ __forceinline__ bool hist_counts_now(const HistArgs &a, const ChainScalars &sc, int chain, int e)
{
    const uint32_t t = sc.ctl[e].it, after = sc.ctl[e ^ 1].it;
    const uint32_t rel = t - sc.it_base;
    return a.on[chain] != 0u && a.cnt != nullptr && after == t + 1u && sc.err == 0 && rel >= sc.burnin;
}

__global__ void __launch_bounds__(256) k_hist_psi(const HistArgs a, const ChainScalars *__restrict__ scs, int e)
{
    const int chain = blockIdx.y;
    const ChainScalars &sc = scs[chain];
    if (!hist_counts_now(a, sc, chain, e)) return;
    if (blockIdx.x == 0u && threadIdx.x == 0u) a.count[chain] += 1u;
    const int n = a.n, i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    const double psi = expit(xdot(a.Xt, n, i, sc.beta, a.p) + a.eta[(size_t)chain * n + i]);
    const int b = max(0, min(a.B - 1, (int)(psi * (double)a.B)));  // (0 <= psi <= 1; the lower clamp keeps a NaN's column in bounds)
    uint32_t *at = a.cnt + ((size_t)chain * (size_t)a.B + (size_t)b) * (size_t)n + (size_t)i;
    *at = *at + 1u;
}

void hist_launch(const HistArgs &a, const ChainScalars *scs, int C, int e, hipStream_t st)
{
    const dim3 grid((unsigned)((a.n + 255) / 256), (unsigned)C);
    hipLaunchKernelGGL(k_hist_psi, grid, dim3(256), 0, st, a, scs, e);
}

}  // namespace occ
