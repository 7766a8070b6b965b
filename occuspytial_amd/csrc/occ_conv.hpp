// occ_conv.hpp -- per-site convergence diagnostics (state names conv_stats, conv_count, conv_sums; logit models): running
// batch-means sums of the occupancy probability psi_i and of the spatial effect eta_i per site and chain.  R-hat needs each
// chain's mean and variance, ESS and the Monte-Carlo standard error need the variance of batch means: a handful of running
// sums per site, so the draws are not needed.  DESIGN.md section 21 is the specification.
//
// One kernel (occ_conv.hip, a translation unit of its own inside libocc_gibbs.so: the units of occ_gibbs.hip, occ_spatial.hip
// and occ_hist.hip keep the kernel symbols they had), launched directly behind the z update on its stream while a chain of
// the handle has the switch on.  Stream order is the synchronisation: nothing writes eta or beta between the z update and
// the first kernel of the next sequence, and two launches on the stream follow one another.
//
//   k_conv_sites   per site i of a chain c whose switch is on, for v = psi_i = expit(x_i beta + eta_i) (the operations of
//                  k_hist_psi and of k_sp_resid) and for v = eta_i, with m = cnt the site's own count:
//                      if (m == 0) ref = v;   d = v - ref;   s1 += d;  s2 += d d;  run += d;
//                      if ((m + 1) % L == 0) { bsq += run run;  run = 0; }
//                  and then cnt = m + 1; the first thread of the chain's first workgroup adds 1 to count[c].
// Eleven float64 slots per chain and site -- cnt, then ref, s1, s2, run, bsq of psi, then the same five of eta -- slot-major,
// [slot][c n + i], so every access of a wave is coalesced.  A column belongs to one thread and a site keeps its own count:
// nothing depends on a word that another thread of the same launch writes, there are no atomics, additions run in iteration
// order, and the sums do not depend on path, placement, block size or how calls are split.  The shift by the first counted
// value keeps s2 - s1^2 / N from cancelling.  Zeroing the eleven slots is the whole reset.
#pragma once
#include "occ_state.hpp"

namespace occ {

constexpr int CONV_SLOTS = 11;
constexpr int CONV_CNT = 0, CONV_PSI = 1, CONV_ETA = 6;            // cnt; the first slot of psi's five; of eta's five
constexpr int CONV_REF = 0, CONV_S1 = 1, CONV_S2 = 2, CONV_RUN = 3, CONV_BSQ = 4;  // within a quantity's five
constexpr int CONV_BATCH_MAX = 1 << 30;

// By-value argument block of the kernel: a change of L or of an address drops the captured graphs on the host.
struct ConvArgs {
    int n, p, L;
    size_t Cn;           // C n: the stride between slots
    const double *Xt;    // Ctx::Xt
    const double *eta;   // Ctx::eta  [C][n] (reduced rank: K theta as stored)
    double *sums;        // [11][C n] the slots, slot-major
    double *count;       // [C] accumulated iterations
    const uint32_t *on;  // [C] the chains' switches (a word of the handle, not a bit of ChainScalars::site_on)
};

// The kernel behind the z update of sequence parity e on `st`, a (ceil(n / 256), C) grid of 256 threads (occ_conv.hip).
// A launch the runtime rejects shows in hipGetLastError(), which the caller asks.
void conv_launch(const ConvArgs &a, const ChainScalars *scs, int C, int e, hipStream_t st);

}  // namespace occ
