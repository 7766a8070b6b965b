// occ_holdout.hpp -- held-out predictive scoring (state names holdout_data, holdout_stats, holdout_count, holdout_sums; logit
// models): running sums of the predictive density of WITHHELD detection histories at sites the handle's problem does not
// survey.  The log predictive density of a held-out site needs the mean over the kept draws of the site's marginal
// likelihood of its withheld visits: a handful of running sums per held-out entry, so the draws are not needed.  DESIGN.md
// section 22 is the specification.
//
// One kernel (occ_holdout.hip, a translation unit of its own inside libocc_gibbs.so: the units of occ_gibbs.hip,
// occ_spatial.hip, occ_hist.hip and occ_conv.hip keep the kernel symbols they had), launched directly behind the z update on
// its stream while a chain of the handle has the switch on.  Stream order is the synchronisation: nothing writes eta, beta
// or alpha between the z update and the first kernel of the next sequence (the side stream's draw of the next alpha waits
// for that kernel's start, or for an event recorded behind this launch), and two launches on the stream follow one another.
//
//   k_holdout_sites   per held-out entry h (site i = site[h], withheld rows r = ptr[h] .. ptr[h + 1] - 1) of a chain c whose
//                     switch is on, with a = x_i beta + eta_i (xdot and the stored eta: the operations of k_conv_sites),
//                     psi = expit(a), t_r = -w_r alpha and lsig(t) = min(t, 0) - log1p(exp(-|t|)):
//                         P = prod_r expit(t_r)  (rows in row order),   pd = psi (1 - P)
//                         no detection:  D = (1 - psi) + psi P,   L = D,   l = log D
//                         a detection:   l = lsig(a) + sum_r lsig(y_r ? -t_r : t_r)  (rows in row order),   L = exp(l)
//                         cnt += 1;  sum L += L;  sum l += l;  sum l^2 = fma(l, l, sum l^2);  sum pd += pd
//                     -- the formulas of the streaming WAIC (z_update_site_ll) over the withheld rows; the first thread of
//                     the chain's first workgroup adds 1 to count[c].
// Five float64 slots per chain and entry, slot-major [slot][c H + h], so every access of a wave to them is coalesced.  The
// withheld rows lie as the problem's own visit rows lie for the z update: the covariates as q columns over the flat row
// index, Wt[a R + r], the detections as one byte per row, entries in the order given, so the lanes of a wave walk
// neighbouring row ranges and every line a wave fetches is used whole by it.  A column belongs to one thread: nothing depends
// on a word that another thread of the same launch writes, there are no atomics, additions run in iteration order, and the
// sums do not depend on path, placement, block size or how calls are split.  Zeroing the five slots is the whole reset.
#pragma once
#include "occ_state.hpp"

namespace occ {

constexpr int HOLD_SLOTS = 5;
constexpr int HOLD_CNT = 0, HOLD_LIK = 1, HOLD_LOG = 2, HOLD_LOG2 = 3, HOLD_PD = 4;

// By-value argument block of the kernel: a change of an address or of a size drops the captured graphs on the host.
struct HoldoutArgs {
    int n, p, q, H, R;
    size_t CH;            // C H: the stride between slots
    const double *Xt;     // Ctx::Xt
    const double *eta;    // Ctx::eta  [C][n] (reduced rank: K theta as stored)
    const int *site;      // [H] the entry's site, not surveyed in the handle's problem
    const int *ptr;       // [H + 1] the entry's rows
    const uint8_t *seen;  // [H] the entry's withheld history has a detection
    const uint8_t *y;     // [R] the withheld detections
    const double *Wt;     // [q][R] the withheld rows' covariates, column-major over the flat row index
    double *sums;         // [5][C H] the slots, slot-major
    double *count;        // [C] accumulated iterations
    const uint32_t *on;   // [C] the chains' switches (a word of the handle, not a bit of ChainScalars::site_on)
};

// The kernel behind the z update of sequence parity e on `st`, a (ceil(H / 256), C) grid of 256 threads (occ_holdout.hip).
// A launch the runtime rejects shows in hipGetLastError(), which the caller asks.
void holdout_launch(const HoldoutArgs &a, const ChainScalars *scs, int C, int e, hipStream_t st);

}  // namespace occ
