// occ_hist.hpp -- per-site intervals (state names hist_stats, hist_count, hist_counts; logit models): a histogram of the
// occupancy probability psi_i per site and chain, B equal bins on (0, 1), one count per accumulated iteration.  psi lives in
// (0, 1), so the histogram answers every quantile of psi_i to within 1 / B with an exact bracket, and the chains' histograms
// merge by addition.  DESIGN.md section 20 is the specification.
//
// One kernel (occ_hist.hip, a translation unit of its own inside libocc_gibbs.so: the units of occ_gibbs.hip and of
// occ_spatial.hip keep the kernel symbols they had), launched directly behind the z update on its stream while a chain of
// the handle has the switch on.  Stream order is the synchronisation: nothing writes eta or beta between the z update and
// the first kernel of the next sequence, and two launches on the stream follow one another.
//
//   k_hist_psi   per site i of a chain whose switch is on:  psi_i = expit(x_i beta + eta_i) (the operations of the z update's
//                site_psi and of k_sp_resid),  b = min(B - 1, (int)(psi_i B)),  cnt[(c B + b) n + i] += 1: a plain 32-bit
//                read-modify-write -- the (chain, site) column belongs to one thread; the first thread of the chain's first
//                workgroup adds 1 to count[c].
// Integer counts: no path, placement or block size can change a bit.  The layout is bin-major, [chain][bin][site]: psi is
// spatially smooth, so the 64 sites of a wave fall into few bins k and touch k to 2k cache lines; site-major would touch 64.
// The host keeps every count below 2^32 (it refuses a call that could take one past 2^32 - 1).
#pragma once
#include "occ_state.hpp"

namespace occ {

constexpr int HIST_BINS_MIN = 4, HIST_BINS_MAX = 1024;

// By-value argument block of the kernel: a change of B or of an address drops the captured graphs on the host.
struct HistArgs {
    int n, p, B;
    const double *Xt;    // Ctx::Xt
    const double *eta;   // Ctx::eta  [C][n] (reduced rank: K theta as stored)
    uint32_t *cnt;       // [C][B][n] the histograms, bin-major
    uint32_t *count;     // [C] accumulated iterations
    const uint32_t *on;  // [C] the chains' switches (a word of the handle, not a bit of ChainScalars::site_on)
};

// The kernel behind the z update of sequence parity e on `st`, a (ceil(n / 256), C) grid of 256 threads (occ_hist.hip).
// A launch the runtime rejects shows in hipGetLastError(), which the caller asks.
void hist_launch(const HistArgs &a, const ChainScalars *scs, int C, int e, hipStream_t st);

}  // namespace occ
